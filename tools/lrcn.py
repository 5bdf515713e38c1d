#!/usr/bin/env python3
"""Driver with the flag surface of `lrcn.jl`'s main (lrcn.jl:29-188): tokenise -> init/load -> one of
{train, generate, extfeatures}, running the hot path on an MI355X through liblrcn_hip (no CPU path).

    python tools/lrcn.py --coco --train --datafiles captions_train2014.json captions_val2014.json \
        --features train_feats.npz val_feats.npz --savefile m.npz
    python tools/lrcn.py --coco --loadfile m.npz --generate 30 --beam_width 5 --datafiles ... --features ...
    python tools/lrcn.py --cnn --model imagenet-vgg-verydeep-16.mat --loadfile m.npz --generate 30 photo.jpg
    python tools/lrcn.py --flickr --loadfile m.npz --retrieval --capnumber 1000 --datafiles results_20130124.token --features ...
    python tools/lrcn.py --cnn --model vgg.mat --extfeatures --imagedir train2014 --prefix COCO_train2014_ --datafiles ...
    python tools/lrcn.py --coco --train --gpus 8 --batchsize 256 --datafiles ... --features ...           # data-parallel: 8 x 32 rows
    python tools/lrcn.py --coco --train --gpus 8 --cnn --model vgg.mat --imagedir train2014 --prefix COCO_train2014_ --datafiles ...   # from images

Training runs on dp.DataParallelTrainer (train.py = train! / train1 / average_loss, lrcn.jl:223-246, 330-397, 407-486): every bucketed
batch is split by rows over the ranks (same T everywhere, the global batch as normaliser, gradients summed over RCCL, identical Adam).
`--varlen` batches captions of mixed lengths (padded, masked loss) instead of the reference's equal-length batches: nothing is dropped.
`--ss_start E` turns scheduled sampling on from epoch E (counted from 0): an input word is, with a probability that grows by `--ss_step`
every `--ss_every` epochs up to `--ss_max`, drawn on the device from the model's own logits of the step before (include/lrcn_sched.h).
`--generate N --nbest --loadfile m0.npz --ensemble m1.npz ...` decodes several checkpoints of one vocabulary as one model
(include/lrcn_ensemble.h).
`--generate N --nbest --force_words "dog|dogs,frisbee"` (or `--force_file F`, sets per image) returns only captions that hold a word of
every set (include/lrcn_forced.h) and writes them to `forced`.
`--label_smoothing E` scores every training step against (1 - E) onehot + E / V inside the loss kernels (include/lrcn_smooth.h); it combines
with `--varlen`, `--ss_start`, `--scst` and `--gclip`, and the per-epoch loss line stays the plain NLL of average_loss.
`--gpus N` starts the ranks itself from a parent that never touches the GPU; the torchrun form works too.  `--cnn --train --imagedir`
trains end to end from images: the VGG forward of the next batch runs beside the LSTM step of the current one.

Differences from the reference, all documented in SURVEY.md 5.6 / A.8: `--lr` (default 0.001 = what the reference's
Adam() actually uses) and `--gclip` (default 0 = off) are honoured instead of being parsed and ignored; `--bestfile` is
accepted; data locations are flags (`--features`, `--imagedir`, `--out`) instead of hard-coded paths; files are `.npz`
(formats.py) because JLD/HDF5 cannot be read here; `--dropout` exists (default 0.4 = the hard-coded pdrop of train!).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_parser():
    p = argparse.ArgumentParser(description="LRCN (MI355X): Long-term Recurrent Convolutional Networks for Visual "
                                            "Recognition and Description -- lrcn.jl's CLI on liblrcn_hip")
    p.add_argument("image", nargs="?", default=None, help="Image file (with --cnn --generate).")
    p.add_argument("--model", default="imagenet-vgg-verydeep-16.mat", help="Location of the MatConvNet VGG-16 file")
    p.add_argument("--datafiles", nargs="+", default=[], help="first file: training captions, second: dev, others: test")
    p.add_argument("--loadfile", help="Initialize model from file")
    p.add_argument("--savefile", help="Save final model to file")
    p.add_argument("--bestfile", help="accepted for compatibility (lrcn.jl:63 reads it)")
    p.add_argument("--generate", type=int, default=0, help="If non-zero generate captions of at most this many words.")
    p.add_argument("--hidden", nargs="+", type=int, default=[1000, 1000], help="Sizes of the two LSTM layers.")
    p.add_argument("--embed", type=int, default=1000, help="Size of the embedding vector.")
    p.add_argument("--epochs", type=int, default=10)
    p.add_argument("--capnumber", type=int, default=1000, help="Number of captions to generate.")
    p.add_argument("--batchsize", type=int, default=25, help="Number of sentences to train on in parallel.")
    p.add_argument("--lr", type=float, default=0.001, help="Adam learning rate (the reference always ran 0.001).")
    p.add_argument("--gclip", type=float, default=0.0, help="Gradient-norm clip (0 = off, as in the reference).")
    p.add_argument("--seed", type=int, default=-1)
    p.add_argument("--atype", default="bf16", choices=["bf16", "f32", "fp8", "KnetArray{Float32}", "Array{Float32}"],
                   help="arithmetic type of the LSTM/VGG kernels (the reference's array-type strings select f32; fp8 = e4m3 "
                        "conv2_2..conv5_3 for --generate / --extfeatures, calibrated on the first batch of crops, bf16 elsewhere)")
    p.add_argument("--train", action="store_true")
    p.add_argument("--cnn", action="store_true", help="load the VGG-16 weights")
    p.add_argument("--extfeatures", action="store_true", help="extract fc7 features for the first caption file's images")
    p.add_argument("--flickr", action="store_true")
    p.add_argument("--coco", action="store_true")
    p.add_argument("--beam_width", type=int, default=3)
    p.add_argument("--sample", type=int, default=0, help="--generate: draw this many captions per image instead of beam search (0 = beam search)")
    p.add_argument("--temperature", type=float, default=1.0, help="--sample: softmax temperature (0 = greedy)")
    p.add_argument("--topk", type=int, default=0, help="--sample: draw among the k most probable words only (0 = all; any k up to the vocabulary)")
    p.add_argument("--topp", type=float, default=1.0, help="--sample: nucleus sampling -- draw among the most probable words that together hold "
                                                            "this share of the mass (after the --topk cut; 1.0 = off)")
    p.add_argument("--nbest", action="store_true",
                   help="--generate: n-best beam search in log space (include/lrcn_nbest.h) at --beam_width; writes <out>/nbest with "
                        "--beam_width lines per image (id, score, logp, caption), candidates / ids keep each image's best")
    p.add_argument("--length_norm", type=float, default=0.0,
                   help="--nbest: rank by logp / len^ALPHA, len = predicted tokens (0 = raw log-likelihood, 1 = per token)")
    p.add_argument("--diverse_groups", type=int, default=0,
                   help="--nbest: diverse beam search (include/lrcn_diverse.h) -- --beam_width beams in this many groups (a divisor of it); writes "
                        "<out>/diverse with --beam_width lines per image (id, group, score, logp, caption), candidates / ids keep the "
                        "best-scoring entry over all groups (0 = off)")
    p.add_argument("--diverse_strength", type=float, default=0.5,
                   help="--diverse_groups: what a word loses per beam of an earlier group that took it at the same step")
    p.add_argument("--ban_words", default="",
                   help="--nbest: constrained beam search (include/lrcn_constrain.h) -- comma-separated vocabulary words that no caption may "
                        "hold (their probability is not given to the others: logp stays the model's)")
    p.add_argument("--min_len", type=int, default=0, help="--nbest: a caption does not end before it has this many words (at most --generate)")
    p.add_argument("--no_repeat_ngram", type=int, default=0, help="--nbest: no caption holds the same N words in a row twice (0 = off; 1 = no word twice)")
    p.add_argument("--force_words", default="",
                   help="--nbest: forced-word beam search (include/lrcn_forced.h) -- every caption holds a word of each comma-separated set, a "
                        "set being alternatives joined by '|' (\"dog|dogs,frisbee\"); at most 3 sets of 4 words, 2^sets * --beam_width <= 32; "
                        "writes <out>/forced in place of nbest; composes with --ban_words / --min_len / --no_repeat_ngram")
    p.add_argument("--force_file", default="", help="--force_words per image: lines \"IMAGE_ID set,set,...\"; an image without a line has no set")
    p.add_argument("--ensemble", nargs="+", default=[], metavar="CHECKPOINT",
                   help="--nbest: ensemble beam search (include/lrcn_ensemble.h) -- further checkpoints of the same vocabulary that decode "
                        "together with --loadfile, one context each, sized from the checkpoint; the files --nbest / --diverse_groups write")
    p.add_argument("--ensemble_weights", default="", help="--ensemble: comma-separated positive weights, --loadfile's first (default: uniform)")
    p.add_argument("--ensemble_mode", choices=["prob", "logprob"], default="prob",
                   help="--ensemble: mix the members' word distributions by their arithmetic (prob) or geometric (logprob) mean")
    p.add_argument("--retrieval", action="store_true",
                   help="image-caption retrieval (paper section 5.1 / Table 2): score --capnumber images of the --generate split, drawn as --generate "
                        "draws them (a permutation seeded by --seed), against all their captions; R@1/5/10 and Medr both ways, "
                        "<out>/retrieval.json and <out>/scores.npy")
    p.add_argument("--retrieval_norm", default="mean", choices=["mean", "sum"],
                   help="--retrieval: rank by log-likelihood per predicted token (mean) or in total (sum)")
    p.add_argument("--dropout", type=float, default=0.4, help="pdrop of train! (lrcn.jl:227)")
    p.add_argument("--features", nargs="+", default=[], help=".npz feature dictionaries: train [val] (formats.save_features)")
    p.add_argument("--imagedir", default=".", help="directory of the images for --extfeatures")
    p.add_argument("--prefix", default="", help="file-name prefix before the zero-padded id (COCO_train2014_)")
    p.add_argument("--out", default="eval", help="directory for candidates / ids files of --generate")
    p.add_argument("--workers", type=int, default=max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))),
                   help="threads that decode images for --cnn --train / --extfeatures")
    p.add_argument("--gpus", type=int, default=1, help="--train: ranks of the data-parallel job (one per GPU); batches are split by rows")
    p.add_argument("--dp_backend", default="torch", choices=["torch", "abi"], help="collectives through torch.distributed's RCCL group or the library's own")
    p.add_argument("--shard_adam", action="store_true", help="N > 1: reduce-scatter -> Adam on 1/N of the parameters -> all-gather (dp.py)")
    p.add_argument("--varlen", action="store_true",
                   help="--train: padded batches of mixed caption lengths (include/lrcn_varlen.h) for the training and the evaluation splits: the "
                        "length-sorted captions cut into windows of --batchsize, none dropped, no forced batch 10 (needs --features)")
    p.add_argument("--ss_start", type=int, default=-1,
                   help="--train: scheduled sampling (include/lrcn_sched.h) from this epoch on, counted from 0 (-1 = off): an input word is, "
                        "with probability eps, drawn from the model's own logits of the step before (needs --features, --dp_backend torch)")
    p.add_argument("--ss_every", type=int, default=5, help="--ss_start: eps grows every this many epochs")
    p.add_argument("--ss_step", type=float, default=0.05, help="--ss_start: eps starts at this value and grows by it")
    p.add_argument("--ss_max", type=float, default=0.25, help="--ss_start: the largest eps")
    p.add_argument("--ss_temperature", type=float, default=1.0, help="--ss_start: temperature of the draw (0 = the argmax)")
    p.add_argument("--label_smoothing", type=float, default=0.0,
                   help="--train: label smoothing eps in [0, 1] of every training step's loss (include/lrcn_smooth.h; 0 = off); the per-epoch "
                        "(:epoch, n, :loss, ...) line stays the plain NLL")
    p.add_argument("--scst", action="store_true",
                   help="--train: self-critical training on the model's own samples with a CIDEr-D reward (lrcn_amd/scst.py); needs --loadfile")
    p.add_argument("--scst_samples", type=int, default=5, help="--scst: samples per image; a step takes batchsize // scst_samples images")
    p.add_argument("--scst_baseline", default="greedy", choices=["greedy", "mean"],
                   help="--scst: the reward a sample is compared with -- the greedy caption's, or the mean of the image's other samples")
    p.add_argument("--scst_nword", type=int, default=20, help="--scst: sampled captions have at most this many words")
    p.add_argument("--scst_reward", default=None, choices=["host", "device"],
                   help="--scst: where CIDEr-D runs -- host (lrcn_amd/cider.py, the default) or device (include/lrcn_cider.h, one kernel call per batch)")
    p.add_argument("--no_normalize", action="store_true", help="--cnn --train: do not divide fc7 features by their sum (lrcn.jl:595-597 does)")
    return p


def tokenize_all(o, cap):
    """Tokenizer.tokenize (tokenizer.jl:6-31): vocab over all files, caption lists per split."""
    lists, counted = [], []
    for path in o.datafiles:
        kind = path.split(".")[-1]
        with open(path) as f:
            if kind == "token":
                lines = f.readlines()
                counted.append(cap.tokenize_flickr(lines))  # vocab counts every caption incl. val/test (:13-15)
                lists.extend(cap.split_flickr(lines))
            elif kind == "json":
                d = cap.tokenize_coco(f.read())
                lists.append(d)
                counted.append(d)
            else:
                print("invalid caption file:", path)
    return cap.build_vocab(counted), lists


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    parser = build_parser()
    o = parser.parse_args(argv)
    ban_words = [w for w in o.ban_words.split(",") if w]
    constrained = bool(ban_words) or o.min_len != 0 or o.no_repeat_ngram != 0
    if constrained and not (o.nbest and o.generate > 0 and o.sample <= 0):
        parser.error("--ban_words / --min_len / --no_repeat_ngram constrain the n-best beam: give --generate N --nbest (without --sample)")
    if o.min_len < 0 or o.no_repeat_ngram < 0 or o.min_len > max(o.generate, 0):
        parser.error("--min_len must be in [0, --generate] and --no_repeat_ngram >= 0")
    forcing = bool(o.force_words or o.force_file)
    if forcing and not (o.nbest and o.generate > 0 and o.sample <= 0):
        parser.error("--force_words / --force_file force words into the n-best beam: give --generate N --nbest (without --sample)")
    if forcing and (o.diverse_groups > 0 or o.ensemble):
        parser.error("--force_words / --force_file do not combine with --diverse_groups or --ensemble")
    if o.force_words and o.force_file:
        parser.error("give --force_words (the same sets for every image) or --force_file (sets per image), not both")
    if o.force_file and o.cnn:
        parser.error("--force_file names the images of a feature table: with --cnn --image give --force_words")

    def parse_sets(text, where):   # "dog|dogs,frisbee" -> [["dog", "dogs"], ["frisbee"]]
        sets = [[w for w in part.split("|") if w] for part in text.split(",")]
        sets = [alt for alt in sets if alt]
        if len(sets) > 3 or any(len(alt) > 4 for alt in sets):
            parser.error("%s: at most 3 sets of at most 4 alternatives" % where)
        if (o.beam_width << len(sets)) > 32:
            parser.error("%s: 2^sets * --beam_width = %d rows per image, at most 32" % (where, o.beam_width << len(sets)))
        if o.generate < len(sets):
            parser.error("%s: %d sets do not fit into --generate %d words" % (where, len(sets), o.generate))
        return sets
    force_sets = parse_sets(o.force_words, "--force_words") if o.force_words else []
    force_by_image = {}
    if o.force_file:
        with open(o.force_file) as fh:
            for ln in fh:
                if ln.strip():
                    key, _, rest = ln.strip().partition(" ") if "\t" not in ln else ln.strip().partition("\t")
                    try:
                        force_by_image[int(key)] = parse_sets(rest.strip(), "--force_file, image %s" % key)
                    except ValueError:
                        parser.error("--force_file: %r is no image id" % key)
    ens_weights = None
    if o.ensemble and not (o.nbest and o.generate > 0 and o.sample <= 0 and o.loadfile):
        parser.error("--ensemble decodes several checkpoints with the n-best beam: give --loadfile m0 --generate N --nbest (without --sample)")
    if o.ensemble_weights:
        if not o.ensemble:
            parser.error("--ensemble_weights weighs the members of --ensemble")
        try:
            ens_weights = [float(w) for w in o.ensemble_weights.split(",")]
        except ValueError:
            parser.error("--ensemble_weights: comma-separated numbers")
        if len(ens_weights) != 1 + len(o.ensemble):
            parser.error("--ensemble_weights: %d weights for %d members (--loadfile and --ensemble)" % (len(ens_weights), 1 + len(o.ensemble)))
        if not all(0.0 < w < float("inf") for w in ens_weights):
            parser.error("--ensemble_weights must be positive and finite")
    if o.varlen and not o.train:
        raise SystemExit("--varlen chooses the batches of the TRAINING job (--train)")
    if o.ss_start >= 0 and (not o.train or o.scst):
        raise SystemExit("--ss_start is a mode of the cross-entropy TRAINING job (--train without --scst)")
    if o.scst_reward is not None and not o.scst:
        raise SystemExit("--scst_reward is an option of self-critical TRAINING (--train --scst)")
    if o.scst and not o.train:
        raise SystemExit("--scst is a mode of the TRAINING job (--train)")
    if not 0.0 <= o.label_smoothing <= 1.0:
        raise SystemExit("--label_smoothing must be in [0, 1]")
    if o.label_smoothing > 0 and not o.train:
        raise SystemExit("--label_smoothing is an option of the TRAINING job (--train)")
    if o.scst and not o.loadfile:
        raise SystemExit("--scst starts from a trained model: give --loadfile (train with cross-entropy first)")
    world_env = os.environ.get("WORLD_SIZE")
    if o.gpus > 1 and world_env is None:   # before any torch / HIP import: this parent only starts the ranks and passes their output on
        if not o.train:
            raise SystemExit("--gpus N is the data-parallel TRAINING job (--train)")
        from lrcn_amd import launch
        rc, _ = launch.run_ranks(__file__, argv, o.gpus, {"LRCN_DP_BACKEND": o.dp_backend}, float(os.environ.get("LRCN_CLI_WATCHDOG_S", "86400")),
                                 capture=False)
        return rc
    world, rank, local_rank = int(world_env or "1"), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    if world != o.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (o.gpus, world))
    say = print if rank == 0 else (lambda *a, **k: None)
    say("opts=", sorted(vars(o).items()))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import numpy as np
    import torch
    import torch.distributed as dist
    import lrcn_amd
    from lrcn_amd import captions as cap
    from lrcn_amd import dp
    from lrcn_amd import formats as fmt
    from lrcn_amd import lrcn as L
    from lrcn_amd import train as trn

    # LRCN_CLI_FAKE_MULTI=1 (validation on a ONE-GPU box): every rank uses device 0 over gloo -- the N-rank control flow on the real kernels
    fake_multi = world > 1 and os.environ.get("LRCN_CLI_FAKE_MULTI", "0")[:1] == "1"
    torch.cuda.set_device(0 if fake_multi else local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if fake_multi:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))

    if o.seed > 0:
        np.random.seed(o.seed)
    rng = np.random.default_rng(o.seed if o.seed > 0 else None)
    dt = lrcn_amd.LRCN_F32 if o.atype in ("f32", "KnetArray{Float32}", "Array{Float32}") else lrcn_amd.LRCN_BF16
    vdt = lrcn_amd.LRCN_FP8 if o.atype == "fp8" else dt
    if vdt == lrcn_amd.LRCN_FP8 and o.train and o.cnn:
        raise SystemExit("--atype fp8 is the caption-generation / feature-extraction precision; train with bf16 or f32")
    vocab, lists = None, []
    if o.datafiles:
        say("Tokenization starts")
        vocab, lists = tokenize_all(o, cap)
        say("Tokenization finished")
    adam_state = None
    host_model = None
    if o.loadfile:
        say("Loading model from", o.loadfile)
        host_model, vocab, adam_state, _ = fmt.load_checkpoint(o.loadfile)
    if vocab is None:
        raise SystemExit("need --datafiles or --loadfile (no vocabulary)")
    V = len(vocab)
    say("%d unique words" % V)
    ban_ids = []
    for w in ban_words:   # 0-based ABI ids; the end of a caption is --min_len's business
        if w in ("<eos>", cap.EOS_WORD) or w not in vocab:
            parser.error("--ban_words: %r %s" % (w, "ends a caption: use --min_len" if w in ("<eos>", cap.EOS_WORD) else "is not in the vocabulary"))
        if vocab[w] - 1 not in ban_ids:
            ban_ids.append(vocab[w] - 1)
    def force_ids(sets, where):   # words -> 0-based ABI ids, as --ban_words
        out, seen = [], set()
        for alt in sets:
            ids = []
            for w in alt:
                if w in ("<eos>", cap.EOS_WORD) or w not in vocab:
                    parser.error("%s: %r %s" % (where, w, "ends a caption" if w in ("<eos>", cap.EOS_WORD) else "is not in the vocabulary"))
                if vocab[w] - 1 in ban_ids:
                    parser.error("%s: %r is in --ban_words" % (where, w))
                if vocab[w] - 1 in seen:
                    parser.error("%s: %r occurs twice" % (where, w))
                seen.add(vocab[w] - 1)
                ids.append(vocab[w] - 1)
            out.append(ids)
        return out
    force_sets = force_ids(force_sets, "--force_words")
    force_by_image = {i: force_ids(sets, "--force_file, image %d" % i) for i, sets in force_by_image.items()}
    force_banks = max([len(force_sets)] + [len(sets) for sets in force_by_image.values()]) if forcing else 0
    if len(o.hidden) != 2 or o.hidden[1] % 2:
        raise SystemExit("--hidden takes two sizes, the second even (LRCN-2f, lrcn.jl:496-504)")
    H1, H2 = o.hidden
    gen_chunk = 256  # images decoded together by the batched beam search (1280 hypothesis rows at beam 5: the decode GEMMs fill the chip)
    if o.scst and not 1 <= o.scst_nword < L._lib.MAX_T:
        raise SystemExit("--scst_nword must be in [1, %d]" % (L._lib.MAX_T - 1))
    ctx = L.Context(o.embed, H1, H2, V, max_B=max(o.batchsize, (o.sample or o.beam_width) * (gen_chunk if o.generate > 0 or o.retrieval else 1), 10), lstm_dtype=dt, vgg_dtype=vdt,
                    max_images=max(o.batchsize, 256 if o.train else 1) if o.cnn else 0)   # training: room for the crops of several batches per forward
    param = L.initweights(ctx, seed=o.seed if o.seed > 0 else 42) if host_model is None else L.model_from_arrays(host_model)
    ens_ctxs, ens_params = [ctx], [param]
    for path in o.ensemble:   # one context per checkpoint, sized from its arrays: Wembed (V, E), b1 (1, 4 H1), Wout (H2, V); no W2: one layer
        say("Loading ensemble member from", path)
        m_model, m_vocab, _, _ = fmt.load_checkpoint(path)
        if m_vocab != vocab:   # the word lists, not only their length: column v must be the same word in every member
            parser.error("--ensemble: the vocabulary of %s is not that of %s" % (path, o.loadfile))
        ens_ctxs.append(L.Context(m_model[6].shape[1], m_model[1].shape[1] // 4, m_model[7].shape[0], V, max_B=max(o.beam_width * gen_chunk, 10),
                                  lstm_dtype=dt, n_layers=2 if m_model[2].size else 1))
        ens_params.append(L.model_from_arrays(m_model))
    say("LSTM is initialized")
    mean = L.VGG_MEAN
    if o.cnn:
        say("Reading", o.model)
        if o.model.startswith("synthetic"):  # "synthetic[:seed]": He-normal weights (no pretrained file offline) -- tests / benchmarks
            L.vgg_load(ctx, *L.synthetic_vgg_weights(seed=int(o.model.split(":")[1]) if ":" in o.model else 1, bias_std=0.05))
        else:
            cw, cb, fc6, fc7, m = fmt.load_vgg_mat(o.model)
            if m is not None:
                mean = tuple(float(v) for v in m)
            L.vgg_load(ctx, [L.to_jl(w) for w in cw], [torch.as_tensor(b).cuda() for b in cb],
                       (L.to_jl(fc6[0]), torch.as_tensor(fc6[1]).cuda()), (L.to_jl(fc7[0]), torch.as_tensor(fc7[1]).cuda()))
            if fmt.load_vgg_mat.average_image is not None:  # the reference subtracts the full array (lrcn.jl:113, 770)
                L.set_average_image(ctx, fmt.load_vgg_mat.average_image)
                mean = None
        say("Cnn is initialized")

    decode_pool = []

    def load_crops(paths):
        """read_image_data (lrcn.jl:750-765) for a batch: decode on the host -- in parallel over the CPUs this process may use (PIL's
        decoders release the GIL); the reference decodes image by image -- then resize / crop / grey->RGB on the GPU."""
        from PIL import Image

        def decode(pth):
            im = Image.open(pth)
            return np.asarray(im if im.mode in ("L", "RGB", "RGBA") else im.convert("RGB"))

        if len(paths) < 4 or o.workers <= 1:
            ims = [decode(p_) for p_ in paths]
        else:
            if not decode_pool:
                from concurrent.futures import ThreadPoolExecutor
                decode_pool.append(ThreadPoolExecutor(max_workers=o.workers))
            ims = list(decode_pool[0].map(decode, paths))
        return L.resize_crop_u8(ctx, ims)
    feats = [fmt.load_features(p) for p in o.features]
    idx2word = cap.index_to_word(vocab)

    def feature_rows(table, ids):
        return L.to_jl(np.stack([table[i].reshape(-1) for i in ids]).astype(np.float32))

    def ensemble_lists(f, groups):   # --nbest --ensemble: every member's context behind one search, constraints and groups included
        return L.beam_ensemble_batch(ens_ctxs, ens_params, f, o.beam_width, o.generate, o.length_norm, ens_weights, o.ensemble_mode, ban_ids,
                                     o.min_len, o.no_repeat_ngram, groups=groups, strength=o.diverse_strength)

    def forced_lists(f, image_ids=None):   # --nbest --force_words / --force_file: per image its sets, under the same constraints
        sets = [force_by_image.get(i, []) for i in image_ids] if o.force_file else [force_sets] * f.shape[0]
        return L.beam_forced_batch(ctx, param, f, o.beam_width, o.generate, o.length_norm, sets, ban_ids, o.min_len, o.no_repeat_ngram), sets

    def nbest_lists(f):     # --nbest, under --ban_words / --min_len / --no_repeat_ngram the constrained beam
        if o.ensemble:
            return ensemble_lists(f, 0)
        if constrained:
            return L.beam_constrained_batch(ctx, param, f, o.beam_width, o.generate, o.length_norm, ban_ids, o.min_len, o.no_repeat_ngram)
        return L.beam_nbest_batch(ctx, param, f, o.beam_width, o.generate, o.length_norm)

    def diverse_lists(f):   # --nbest --diverse_groups, likewise
        if o.ensemble:
            return ensemble_lists(f, o.diverse_groups)
        if constrained:
            return L.beam_constrained_batch(ctx, param, f, o.beam_width, o.generate, o.length_norm, ban_ids, o.min_len, o.no_repeat_ngram,
                                            groups=o.diverse_groups, strength=o.diverse_strength)
        return L.beam_diverse_batch(ctx, param, f, o.beam_width, o.diverse_groups, o.diverse_strength, o.generate, o.length_norm)

    # ---------------------------------------------------------------- generate (lrcn.jl:127-160)
    if o.generate > 0:
        sample_seed = o.seed if o.seed > 0 else 0
        if o.cnn:
            crop = load_crops([o.image])
            if vdt == lrcn_amd.LRCN_FP8:
                L.vgg_calibrate(ctx, crop, mean=mean)
            f = L.convnet_u8(ctx, crop, mean=mean, normalize=True)  # input = input / sum(input)  (lrcn.jl:595-597)
            if o.sample > 0:  # the S draws, highest log-likelihood first
                for line in L.sample_captions(ctx, param, f, idx2word, o.sample, o.generate, o.temperature, o.topk, sample_seed, top_p=o.topp)[0]:
                    print(line)
                return 0
            if o.nbest and o.diverse_groups > 0:   # the groups in order, each best score first: group<TAB>score<TAB>logp<TAB>caption
                for g, grp in enumerate(diverse_lists(f)[0]):
                    for toks, lp, sc in grp:
                        print("%d\t%.6f\t%.6f\t%s" % (g, sc, lp, cap.caption_text(toks, idx2word)))
                return 0
            if o.nbest:   # the n-best list, best score first: score<TAB>logp<TAB>caption
                for toks, lp, sc in (forced_lists(f)[0] if forcing else nbest_lists(f))[0]:
                    print("%.6f\t%.6f\t%s" % (sc, lp, cap.caption_text(toks, idx2word)))
                return 0
            toks, _ = L.beam_search(ctx, param, f, o.beam_width, o.generate)
            print(cap.caption_text(toks, idx2word))
            return 0
        split = lists[2] if o.flickr and len(lists) > 2 else lists[min(1, len(lists) - 1)]
        table = feats[min(1, len(feats) - 1)] if o.coco else feats[0]
        ids = []
        for k in rng.permutation(len(split)):
            i = split[k][0][0]
            if i not in ids:
                ids.append(i)
            if len(ids) == o.capnumber:
                break
        os.makedirs(o.out, exist_ok=True)
        suffix = "_flickr" if o.flickr else ".txt"
        import gc  # tools/beam_bench.py: keep full cyclic-GC passes (tens of ms with torch's objects) out of the decode loop
        gc.collect()
        gc.freeze()
        smp = open(os.path.join(o.out, "samples" + suffix), "w") if o.sample > 0 else None
        dvf = open(os.path.join(o.out, "diverse" + suffix), "w") if o.nbest and o.diverse_groups > 0 and o.sample <= 0 else None
        nbf = open(os.path.join(o.out, ("forced" if forcing else "nbest") + suffix), "w") if o.nbest and o.sample <= 0 and dvf is None else None
        chunk_n = gen_chunk >> force_banks   # a forced image owns 2^sets * beam_width rows of the decode
        met = with_sets = 0
        with open(os.path.join(o.out, "candidates" + suffix), "w") as out, open(os.path.join(o.out, "candidate_ids" + suffix), "w") as ido:
            for s0 in range(0, len(ids), chunk_n):  # the reference decodes image by image; here gen_chunk images x beam_width rows per step
                chunk = ids[s0:s0 + chunk_n]
                if o.sample > 0:
                    # candidates / ids keep one line per image (the best log-likelihood of the S draws); `samples` holds all of them:
                    # "id<TAB>log-likelihood<TAB>caption", the image's draws in sample order.  The draws of an image depend on its index in the
                    # call, so every chunk takes its own seed
                    drawn = L.sample_batch(ctx, param, feature_rows(table, chunk), o.sample, o.generate, o.temperature, o.topk, sample_seed + s0, top_p=o.topp)
                    for i, rows in zip(chunk, drawn):
                        best = max(range(len(rows)), key=lambda s: (rows[s][1], -s))
                        ido.write("%d\n" % i)
                        out.write(cap.caption_text(rows[best][0], idx2word) + "\n")
                        for toks, lp in rows:
                            smp.write("%d\t%.6f\t%s\n" % (i, lp, cap.caption_text(toks, idx2word)))
                    continue
                if dvf is not None:
                    # candidates / ids keep the best-scoring entry over all groups (the earlier group wins a tie); `diverse` holds the groups
                    # in order, each best first: "id<TAB>group<TAB>score<TAB>logp<TAB>caption"
                    res = diverse_lists(feature_rows(table, chunk))
                    for i, groups in zip(chunk, res):
                        best = max((grp[0] for grp in groups if grp), key=lambda e: e[2])
                        ido.write("%d\n" % i)
                        out.write(cap.caption_text(best[0], idx2word) + "\n")
                        for g, grp in enumerate(groups):
                            for toks, lp, sc in grp:
                                dvf.write("%d\t%d\t%.6f\t%.6f\t%s\n" % (i, g, sc, lp, cap.caption_text(toks, idx2word)))
                    continue
                if nbf is not None and forcing:
                    # as `nbest` below; an image whose sets could not be met within --generate words has no entry and an empty caption
                    res, sets = forced_lists(feature_rows(table, chunk), chunk)
                    for i, entries, st in zip(chunk, res, sets):
                        ido.write("%d\n" % i)
                        out.write(cap.caption_text(entries[0][0] if entries else [lrcn_amd.BOS], idx2word) + "\n")
                        for toks, lp, sc in entries:
                            nbf.write("%d\t%.6f\t%.6f\t%s\n" % (i, sc, lp, cap.caption_text(toks, idx2word)))
                        with_sets += bool(st)
                        met += bool(st) and bool(entries)
                    continue
                if nbf is not None:
                    # candidates / ids keep each image's best entry; `nbest` holds the list: "id<TAB>score<TAB>logp<TAB>caption", best first
                    for i, entries in zip(chunk, nbest_lists(feature_rows(table, chunk))):
                        ido.write("%d\n" % i)
                        out.write(cap.caption_text(entries[0][0], idx2word) + "\n")
                        for toks, lp, sc in entries:
                            nbf.write("%d\t%.6f\t%.6f\t%s\n" % (i, sc, lp, cap.caption_text(toks, idx2word)))
                    continue
                for i, (toks, _) in zip(chunk, L.beam_search_batch(ctx, param, feature_rows(table, chunk), o.beam_width, o.generate)):
                    ido.write("%d\n" % i)
                    out.write(cap.caption_text(toks, idx2word) + "\n")
        if smp is not None:
            smp.close()
        if nbf is not None:
            nbf.close()
        if forcing:
            say("forced words: %d of %d images with sets met them" % (met, with_sets))
        if dvf is not None:
            dvf.close()
        return 0

    # ---------------------------------------------------------------- retrieval (paper section 5.1 / Table 2; not in lrcn.jl)
    if o.retrieval:
        import json
        from lrcn_amd import retrieval
        split = lists[2] if o.flickr and len(lists) > 2 else lists[min(1, len(lists) - 1)]   # the split and table of --generate
        table = feats[min(1, len(feats) - 1)] if o.coco else feats[0]
        ids = []
        for k in rng.permutation(len(split)):
            i = split[k][0][0]
            if i not in ids:
                ids.append(i)
            if len(ids) == o.capnumber:
                break
        pos = {i: n for n, i in enumerate(ids)}
        caps, img_of = [], []
        for (i, words), n in split:   # every caption of those images that the model can score (1 .. 28 words, lrcn.jl:353)
            if i in pos and 1 <= n <= 28:
                caps.append([vocab.get(w, cap.UNK) - 1 for w in words])
                img_of.append(pos[i])
        s = L.score_matrix(ctx, param, feature_rows(table, ids), caps)
        lens = [len(c) for c in caps]
        res = retrieval.metrics(s, img_of, norm=o.retrieval_norm, lens=lens)
        print(retrieval.format_line("Caption to Image", res["caption_to_image"]))
        print(retrieval.format_line("Image to Caption", res["image_to_caption"]))
        os.makedirs(o.out, exist_ok=True)
        np.save(os.path.join(o.out, "scores.npy"), s)
        with open(os.path.join(o.out, "retrieval.json"), "w") as fh:
            json.dump(dict(res, norm=o.retrieval_norm, image_ids=[int(i) for i in ids], captions=len(caps), img_of_caption=img_of, lens=lens), fh)
        return 0

    # ---------------------------------------------------------------- extract features (lrcn.jl:162-172, 190-221)
    if o.extfeatures:
        ids = sorted({c[0][0] for c in lists[0]})
        table, B = {}, max(o.batchsize, 1)
        for s in range(0, len(ids), B):  # the reference extracts image by image (lrcn.jl:190-221); here B images per VGG forward
            chunk = ids[s:s + B]
            crops = load_crops([os.path.join(o.imagedir, "%s%012d.jpg" % (o.prefix, i) if o.prefix else "%d.jpg" % i) for i in chunk])
            if vdt == lrcn_amd.LRCN_FP8 and s == 0:  # activation scales of the e4m3 layers from the first batch
                L.vgg_calibrate(ctx, crops, mean=mean)
            f = L.from_jl(L.convnet_u8(ctx, crops, mean=mean))
            for i, row in zip(chunk, f):
                table[i] = row.copy()
        fmt.save_features(o.savefile or "feats.npz", table)
        print("image features extracted")
        return 0

    # ---------------------------------------------------------------- train! (lrcn.jl:223-246) on dp.DataParallelTrainer
    if lists and o.train and o.scst:
        from lrcn_amd import scst
        from lrcn_amd.cider import CiderD
        if o.dp_backend == "abi" and world > 1:
            raise SystemExit("--scst needs --dp_backend torch")
        if not feats:
            raise SystemExit("--scst trains on precomputed features (--features)")
        S = o.scst_samples
        per_step = o.batchsize // max(S, 1) // world     # images per rank and step
        if S < 1 or per_step < 1 or (o.scst_baseline == "mean" and S < 2):
            raise SystemExit("--scst: batchsize // scst_samples images per step (at least one per rank); the mean baseline needs 2 samples")
        tables = [feats[0], feats[min(1, len(feats) - 1)]]
        refs = scst.references_by_image(lists[0], vocab)
        on_device = o.scst_reward == "device"
        if on_device:
            from lrcn_amd.cider_device import DeviceCiderD
            word_ids = {w: i - 1 for w, i in vocab.items()}      # the C ABI's ids: what the sampler and the beam search write
            reward = DeviceCiderD(refs, word_ids, word_ids[cap.UNK_WORD])
        else:
            reward = scst.cider_reward(CiderD(refs), idx2word)
        ids = [i for i in refs if i in tables[0]]
        mine = ids[rank::world][:len(ids) // world]       # the same count on every rank
        dev = None
        if len(lists) > 1:
            dev_refs = scst.references_by_image(lists[1], vocab)
            dev = (DeviceCiderD(dev_refs, word_ids, word_ids[cap.UNK_WORD]) if on_device else CiderD(dev_refs), [i for i in dev_refs if i in tables[1]])
        say("scst: %d images with references, %d per step on %d rank%s, %d samples each, baseline %s"
            % (len(ids), per_step * world, world, "" if world == 1 else "s", S, o.scst_baseline))
        optim = L.initparams(param)
        optim.lr = o.lr
        seed = o.seed if o.seed > 0 else 0
        trainer = dp.DataParallelTrainer(ctx, param, optim, per_step * S * world, world, rank, pdrop=o.dropout, seed=seed, backend="torch",
                                         ops=dp.HipOps(ctx, mean=mean), shard_adam=bool(o.shard_adam) and world > 1, gclip=o.gclip)
        if adam_state is not None:
            trainer.restore(adam=(adam_state["m"], adam_state["v"], adam_state["step"]))
        import time
        for epoch in range(1, o.epochs + 1):
            t0 = time.time()
            rs, rg, steps, seen = scst.train_epoch(trainer, mine, lambda part: feature_rows(tables[0], part), reward, per_step, S, o.scst_nword,
                                                   seed + rank, epoch, temperature=o.temperature, top_k=o.topk, top_p=o.topp,
                                                   baseline=o.scst_baseline, label_smoothing=o.label_smoothing)
            ctx.sync()
            dt_s = time.time() - t0
            if o.savefile:
                trainer.gather_optim_state()
                if rank == 0:
                    fmt.save_checkpoint(o.savefile, [L.from_jl(p) for p in param], vocab,
                                        adam={"m": [L.from_jl(t) for t in optim.m], "v": [L.from_jl(t) for t in optim.v], "step": optim.t})
            line = "(:epoch, %d, :scst_reward, %.4f, :greedy_reward, %s" % (epoch, rs, "%.4f" % rg if rg is not None else "nothing")
            if dev is not None and rank == 0:
                line += ", :dev_cider, %.4f" % scst.beam_cider(ctx, param, dev[0], dev[1], lambda part: feature_rows(tables[1], part), idx2word,
                                                                o.beam_width, o.scst_nword)
            say(line + ")  [%d steps, %.0f images/s on %d rank%s]" % (steps, seen * world / max(dt_s, 1e-9), world, "" if world == 1 else "s"))
        trainer.close()
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return 0
    if lists and o.train:
        say("Batching starts")
        if o.varlen:
            if o.cnn and not o.features:
                raise SystemExit("--varlen trains on precomputed features (--features)")
            if o.dp_backend == "abi" and world > 1:
                raise SystemExit("--varlen needs --dp_backend torch")
            vb = [cap.minibatch_varlen(c, vocab, o.batchsize) for c in lists[:2]]
            splits = [list(v) for v in vb]
            cut = 0
            if world > 1 and splits[0] and len(splits[0][-1][0]) % world:   # the short last window must divide by the ranks
                ids_, toks_, lens_ = splits[0].pop()
                keep = len(ids_) - len(ids_) % world
                cut = len(ids_) - keep
                if keep:
                    splits[0].append((ids_[:keep], np.ascontiguousarray(toks_[:, :keep]), lens_[:keep]))
            for name, c, v, lost in zip(("train", "dev"), lists, vb, (cut, 0)):
                say("%s: %d captions, %d dropped, %d longer than 28 words skipped, %d batches of up to %d, %.1f%% of the rows are padding"
                    % (name, len(c), lost, v.skipped, len(v), o.batchsize, 100.0 * v.padded_share))
            B_global = o.batchsize
        else:
            seqs = [cap.minibatch(c, vocab, o.batchsize) for c in lists]
            for name, c, sq in zip(("train", "dev"), lists, seqs[:2]):   # cap.batches skips the batches of captions longer than 28 words
                say("%s: %d captions, %d dropped, %d longer than 28 words skipped, batches of %d"
                    % (name, len(c), len(c) - len(sq[2]), sum(1 for n in sq[2] if n > 28), sq[3]))
            B_global = seqs[0][3]   # splits with <= 30000 captions are forced to batch 10 (lrcn.jl:260-270)
        say("Batching finished")
        if B_global % world:
            raise SystemExit("the batch of %d captions does not split over %d ranks" % (B_global, world))
        optim = L.initparams(param)
        optim.lr = o.lr
        from_images = bool(o.cnn) and not o.features
        seed = o.seed if o.seed > 0 else 0
        # small per-GPU batches: the VGG forward of several upcoming batches as one forward (dp.DataParallelTrainer.step)
        lookahead = trn.batches_per_forward(B_global // world) if from_images else 1
        trainer = dp.DataParallelTrainer(ctx, param, optim, B_global, world, rank, pdrop=o.dropout, seed=seed, backend=o.dp_backend, ops=dp.HipOps(ctx, mean=mean),
                                         vgg_chunk=lookahead, rows=B_global // world,
                                         shard_adam=bool(o.shard_adam) and world > 1, normalize_features=from_images and not o.no_normalize,
                                         gclip=o.gclip)
        if adam_state is not None:   # resume: moments and step count (the reference never saved them)
            trainer.restore(adam=(adam_state["m"], adam_state["v"], adam_state["step"]))
        if not o.varlen:
            splits = [list(cap.batches(sq[0], sq[1], sq[2], sq[3])) for sq in seqs[:2]]

        def image_path(i):
            return os.path.join(o.imagedir, "%s%012d.jpg" % (o.prefix, i) if o.prefix else "%d.jpg" % i)

        def crops_of(ids):
            return load_crops([image_path(i) for i in ids])

        if from_images:   # end to end: ids -> crops -> VGG on the device; average_loss runs the same forward batch by batch
            def eval_f(ids):
                return L.convnet_u8(ctx, crops_of(ids), mean=mean, normalize=not o.no_normalize)
            kw = dict(crops_of=crops_of, eval_feats_of=[eval_f] * len(splits))
        else:
            if not feats:
                raise SystemExit("--train needs --features (precomputed fc7 features) or --cnn --imagedir (train from images)")
            tables = [feats[0], feats[min(1, len(feats) - 1)]]
            kw = dict(feats_of=lambda ids: feature_rows(tables[0], ids), eval_feats_of=[(lambda ids, t=t: feature_rows(t, ids)) for t in tables[:len(splits)]])

        def save(epoch):
            if o.savefile and rank == 0:
                fmt.save_checkpoint(o.savefile, [L.from_jl(p) for p in param], vocab,
                                    adam={"m": [L.from_jl(t) for t in optim.m], "v": [L.from_jl(t) for t in optim.v], "step": optim.t})

        if o.ss_start >= 0:
            if from_images:
                raise SystemExit("--ss_start trains on precomputed features (--features)")
            if o.dp_backend == "abi" and world > 1:
                raise SystemExit("--ss_start needs --dp_backend torch")
            from lrcn_amd import sched as ss
            kw["sched_of"] = ss.sched_of(o.ss_start, o.ss_every, o.ss_step, o.ss_max, temperature=o.ss_temperature, seed=seed)
        if o.label_smoothing > 0:
            if o.dp_backend == "abi" and world > 1:
                raise SystemExit("--label_smoothing needs --dp_backend torch")
            kw["label_smoothing"] = o.label_smoothing
        trn.train(trainer, splits, o.epochs, seed, save=save, log=say, sync=ctx.sync, lookahead=lookahead, **kw)
        trainer.close()
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return 0
    if o.savefile and not o.train:
        fmt.save_checkpoint(o.savefile, [L.from_jl(p) for p in param], vocab)
    return 0


if __name__ == "__main__":
    sys.exit(main())
