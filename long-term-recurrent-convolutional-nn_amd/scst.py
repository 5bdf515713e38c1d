"""Self-critical sequence training (Rennie et al. 2017, "Self-critical Sequence Training for Image Captioning") on the pieces the library
already has: the sampler draws captions on the device, a host metric (cider.CiderD) rewards them, and one weighted training step
(include/lrcn_weighted.h) with row weight = reward - baseline is the REINFORCE update

    loss = -(1 / norm_tokens) * sum_r (r(sample_r) - b_r) * log p(sample_r | image_r).

The reward runs on the host by default: it is a few hundred n-gram look-ups per caption on word strings, needs the whole sampled sentence,
and the sampler hands its tokens to the host anyway.  A reward object with a score_batch method (cider_device.DeviceCiderD, the same
metric over token ids as one HIP kernel call per batch) is scored in one call per batch instead; the sampler's tokens still pass through
the host.

The sampler's output (include/lrcn_sample.h, lrcn.sample_batch) and the training batch.  A sampled row is seq[0] = bos, then one token
per step current = 1 .. nword + 1; it stops after the step that emits eos, or after step nword + 1 whatever that step emitted, and its
length out_len counts bos and the eos.  The padded batch of include/lrcn_varlen.h wants lens[r] = the number of WORDS, after bos and
before eos:
    the row ends in eos         lens = out_len - 2   (eos at the first step: 0 words; the loss terms are exactly the sample's own)
    nword + 1 steps, no eos     lens = out_len - 1 = nword + 1, all of them words
The second case is the one deliberate deviation from the sampled sequence's own log-probability: such a row is trained with the ordinary
eos term after its last word (a padded batch has lens + 1 terms per row, the last one eos), although the sampler never drew that eos.
"""
import numpy as np
import torch
import torch.distributed as dist

from . import lrcn as L


def advantages(r_sample, r_greedy=None, baseline="greedy"):
    """r_sample [N][S] rewards of the samples, r_greedy [N] of the greedy captions -> [N][S] float64 advantages.
    "greedy": r_sample[i][s] - r_greedy[i] (self-critical).  "mean": r_sample[i][s] minus the mean of image i's OTHER samples (needs
    S >= 2 and no greedy decode)."""
    r = np.asarray(r_sample, dtype=np.float64)
    if r.ndim != 2:
        raise L.LrcnError("r_sample must be [N][S]")
    if baseline == "greedy":
        if r_greedy is None:
            raise L.LrcnError("the greedy baseline needs r_greedy")
        g = np.asarray(r_greedy, dtype=np.float64).reshape(-1)
        if g.shape[0] != r.shape[0]:
            raise L.LrcnError("r_greedy has %d entries for %d images" % (g.shape[0], r.shape[0]))
        return r - g[:, None]
    if baseline == "mean":
        S = r.shape[1]
        if S < 2:
            raise L.LrcnError("the mean baseline needs at least 2 samples per image")
        return r - (r.sum(axis=1, keepdims=True) - r) / (S - 1)
    raise L.LrcnError("unknown baseline %r (greedy or mean)" % (baseline,))


def pack_samples(samples, nword):
    """lrcn.sample_batch's result (per image S entries (token ids incl. bos, log-likelihood)) -> (tokens [N][S][nword + 2] int32, eos in
    the unused tail; out_len [N][S] int32), the arrays lrcn_sample_batch itself fills."""
    N, S = len(samples), len(samples[0])
    tok = np.full((N, S, nword + 2), L.EOS, np.int32)
    n = np.zeros((N, S), np.int32)
    for i, row in enumerate(samples):
        for s, (ids, _) in enumerate(row):
            tok[i, s, :len(ids)] = ids
            n[i, s] = len(ids)
    return tok, n


def sample_words(tokens, out_len):
    """The word ids of one sampled row (tokens [nword + 2], its out_len): after bos, before a closing eos -- see the module docstring."""
    n = int(out_len)
    ids = [int(t) for t in tokens[1:n]]
    return ids[:-1] if ids and ids[-1] == L.EOS else ids


def build_batch(tokens, lens, adv):
    """The sampler's output -> the weighted padded training batch.  tokens [N][S][nword + 2] and lens [N][S] as lrcn_sample_batch writes
    out_tokens / out_len (bos first; lens counts bos and a closing eos); adv [N][S].
    -> (tokens [T][R] int32, lens [R] int32, row_weights [R] float32, norm_tokens) with R = N S, row r = i S + s, T = the longest sample's
    word count (at least 1), and lens[r] the number of words after bos and before eos: out_len - 2 for a row that ends in eos, out_len - 1
    (= nword + 1) for one that ran nword + 1 steps without -- that row is trained with the ordinary eos term after its last word, the one
    deliberate deviation from the sampled sequence's own log-probability.  Padding positions hold eos.
    norm_tokens = sum(lens + 1) over all R rows, zero-weight rows included: a step's scale is that of a cross-entropy step over the same
    captions."""
    tokens = np.asarray(tokens, dtype=np.int32)
    out_len = np.asarray(lens, dtype=np.int32)
    adv = np.asarray(adv, dtype=np.float64)
    if tokens.ndim != 3 or out_len.shape != tokens.shape[:2] or adv.shape != out_len.shape:
        raise L.LrcnError("build_batch wants tokens [N][S][nword + 2], lens [N][S] and adv [N][S]")
    N, S, Lmax = tokens.shape
    if (out_len < 2).any() or (out_len > Lmax).any():
        raise L.LrcnError("a sampled row has bos and at least one step: lens in [2, %d]" % Lmax)
    if (tokens[:, :, 0] != L.BOS).any():
        raise L.LrcnError("a sampled row starts with bos")
    R = N * S
    words = [sample_words(tokens[i, s], out_len[i, s]) for i in range(N) for s in range(S)]
    wl = np.asarray([len(w) for w in words], np.int32)
    T = max(1, int(wl.max()))
    tok = np.full((T, R), L.EOS, np.int32)
    for r, w in enumerate(words):
        tok[:len(w), r] = w
    return tok, wl, adv.reshape(R).astype(np.float32), int(wl.astype(np.int64).sum()) + R


def cider_reward(cider, index_to_word):
    """reward(image_id, word ids) for scst_step from a cider.CiderD and the vocabulary's id -> word table."""
    return lambda image_id, ids: cider.score(image_id, [index_to_word[t] for t in ids])


def references_by_image(caps, vocab=None):
    """captions.tokenize_* output [((image_id, words), length)] -> {image_id: [words, ...]} for cider.CiderD.  With a vocabulary, words
    outside it become the unk word: what the model can say at best for them."""
    from . import captions as cap
    refs = {}
    for (i, words), _n in caps:
        refs.setdefault(i, []).append([w if vocab is None or w in vocab else cap.UNK_WORD for w in words])
    return refs


def beam_cider(ctx, param, cider, image_ids, feats_of, index_to_word, beam_width, nword, chunk=None):
    """Mean CIDEr-D of the beam-search captions of `image_ids` (each image once) against `cider`'s references."""
    ids = list(dict.fromkeys(image_ids))
    chunk = chunk or max(1, ctx.max_B // max(1, beam_width))
    hyps = {}
    batch = hasattr(cider, "score_batch")     # cider_device.DeviceCiderD: scores ids, every caption in one call
    for k in range(0, len(ids), chunk):
        part = ids[k:k + chunk]
        for i, (seq, _) in zip(part, L.beam_search_batch(ctx, param, feats_of(part), beam_width, nword)):
            words = sample_words(seq, len(seq))
            hyps[i] = words if batch else [index_to_word[t] for t in words]
    if batch:
        return float(np.mean(cider.score_batch(ids, [hyps[i] for i in ids]))) if ids else 0.0
    return cider.corpus(hyps)[0]


def train_epoch(trainer, image_ids, feats_of, reward, images_per_step, S, nword, seed, epoch, **kw):
    """One pass over `image_ids` (this rank's, each once) in a seeded order, images_per_step images per scst_step; a short last window
    is dropped (every rank must take the same number of steps).  kw: scst_step's temperature / top_k / top_p / baseline / label_smoothing.
    -> (mean sample reward, mean greedy reward or None, steps taken, images seen)."""
    ids = list(image_ids)
    order = np.random.default_rng([int(seed) & 0x7FFFFFFF, int(epoch)]).permutation(len(ids))
    rs, rg, steps, seen = [], [], 0, 0
    for k in range(0, len(ids) - images_per_step + 1, images_per_step):
        part = [ids[j] for j in order[k:k + images_per_step]]
        out = scst_step(trainer, feats_of(part), part, reward, S, nword, seed=(int(seed) * 1000003 + int(epoch)) * 65536 + k, **kw)
        rs.append(out["reward_sample"])
        if out["reward_greedy"] is not None:
            rg.append(out["reward_greedy"])
        steps += int(out["stepped"])
        seen += len(part)
    return (float(np.mean(rs)) if rs else 0.0), (float(np.mean(rg)) if rg else None), steps, seen


def scst_step(trainer, feats, image_ids, reward, S, nword, temperature=1.0, top_k=0, top_p=1.0, seed=0, baseline="greedy", label_smoothing=0.0):
    """One self-critical step of dp.DataParallelTrainer `trainer` on N images.  feats: N x 4096 (column-major device tensor, as every call
    takes them); image_ids [N]; reward(image_id, word ids without bos / eos) -> float, on the host -- or an object with
    score_batch(image ids [R], R lists of word ids) -> R floats (cider_device.DeviceCiderD): the N S samples are then scored in one call and
    the N greedy captions in a second one, with no Python loop over the captions' rewards.
      1. lrcn.sample_batch draws S samples per image (temperature / top_k / top_p / seed as there);
      2. baseline "greedy": lrcn.beam_search_batch with K = 1 (= temperature 0, include/lrcn_sample.h) gives each image's baseline caption;
         "mean": the mean reward of the image's other samples, no second decode;
      3. the rewards, advantages() and build_batch();
      4. one trainer.step on the N S rows -- image i's feature row S times -- with lens, row_weights and norm_tokens set.
    label_smoothing: passed to that step (include/lrcn_smooth.h).
    When every advantage is exactly 0 no step is taken and Adam's step count does not move.  N S must fit the context's max_B.  Under data
    parallelism each rank calls this on its own images (the same N and S everywhere); norm_tokens and the all-zero test are summed over the
    ranks before the step.
    -> {"reward_sample", "reward_greedy" (None for "mean"), "zero_share", "loss" (None when no step was taken), "stepped"}: this rank's
    means, the global loss."""
    ctx = trainer.ctx
    N = int(feats.shape[0])
    if len(image_ids) != N:
        raise L.LrcnError("%d image ids for %d feature rows" % (len(image_ids), N))
    if S < 1 or N * S > ctx.max_B:
        raise L.LrcnError("N * S = %d * %d rows do not fit the context's max_B = %d" % (N, S, ctx.max_B))
    if baseline not in ("greedy", "mean") or (baseline == "mean" and S < 2):
        raise L.LrcnError("baseline is greedy, or mean with at least 2 samples per image")
    samples = L.sample_batch(ctx, trainer.param, feats, S, nword, temperature=temperature, top_k=top_k, seed=seed, top_p=top_p)
    tok, out_len = pack_samples(samples, nword)
    batch = hasattr(reward, "score_batch")
    if batch:
        r_sample = np.asarray(reward.score_batch([image_ids[i] for i in range(N) for _ in range(S)],
                                                 [sample_words(tok[i, s], out_len[i, s]) for i in range(N) for s in range(S)]), np.float64).reshape(N, S)
    else:
        r_sample = np.asarray([[reward(image_ids[i], sample_words(tok[i, s], out_len[i, s])) for s in range(S)] for i in range(N)], np.float64)
    r_greedy = None
    if baseline == "greedy":
        greedy = L.beam_search_batch(ctx, trainer.param, feats, 1, nword)
        if batch:
            r_greedy = np.asarray(reward.score_batch(list(image_ids), [sample_words(ids, len(ids)) for ids, _ in greedy]), np.float64)
        else:
            r_greedy = np.asarray([reward(image_ids[i], sample_words(ids, len(ids))) for i, (ids, _) in enumerate(greedy)], np.float64)
    adv = advantages(r_sample, r_greedy, baseline)
    tokens, lens, weights, norm_tokens = build_batch(tok, out_len, adv)
    nonzero = int(np.count_nonzero(weights))
    if trainer.world > 1:
        t = torch.tensor([norm_tokens, nonzero], dtype=torch.int64, device=trainer.param[0].device if dist.get_backend(trainer.group) == "nccl" else "cpu")
        dist.all_reduce(t, group=trainer.group)
        norm_tokens, nonzero_all = int(t[0].item()), int(t[1].item())
    else:
        nonzero_all = nonzero
    out = {"reward_sample": float(r_sample.mean()), "reward_greedy": None if r_greedy is None else float(r_greedy.mean()),
           "zero_share": 1.0 - nonzero / float(N * S), "loss": None, "stepped": False}
    if nonzero_all == 0:
        return out
    rows = feats.repeat_interleave(S, dim=0)      # row r = i S + s reads image i
    kw = {"label_smoothing": label_smoothing} if label_smoothing else {}   # (a trainer stand-in without the keyword keeps working)
    trainer.step(None, tokens, feats=L.to_jl(rows), lens=lens, norm_tokens=norm_tokens, row_weights=weights, **kw)
    out["loss"], out["stepped"] = trainer.loss_value(), True
    return out
