#!/usr/bin/env python
"""Activity recognition with LRCN (paper section 4) on pre-extracted video frames.

    # per-frame VGG features (pre-ReLU fc7, 4096 wide) of every video listed, one [n_frames x 4096] array per video
    python tools/lrcn_activity.py --extfeatures --cnn --model imagenet-vgg-verydeep-16.mat --list trainlist.txt --features train.npz
    # train the LSTM + softmax head on 16-frame clips with stride 8
    python tools/lrcn_activity.py --train --features train.npz --hidden 256 --clip 16 --stride 8 --batchsize 32 --epochs 10 \
        --lr 1e-3 --atype bf16 --savefile act.npz
    # the same with the paper's dropout: 0.9 on the frame feature, 0.5 on the LSTM output (seeded by --seed; the reported loss is the masked one)
    python tools/lrcn_activity.py --train --features train.npz --drop_in 0.9 --drop_out 0.5 --savefile act.npz
    # clip accuracy (mean of a clip's per-step distributions) and video accuracy (mean of its clips' distributions)
    python tools/lrcn_activity.py --eval --loadfile act.npz --features test.npz

A list file holds one `frames_dir label` per line (UCF101-style split files over frames extracted to JPEG, label a 0-based class id);
a video's frames are the directory's .jpg / .jpeg / .png files sorted by name.  `--model synthetic:N` loads seeded He-normal VGG weights
(tests and benchmarks, no pretrained file).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def say(*a):
    print(*a, flush=True)


def parse(argv):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--list", help="one `frames_dir label` per line")
    p.add_argument("--features", help="per-video features (.npz): written by --extfeatures, read by --train / --eval")
    p.add_argument("--extfeatures", action="store_true", help="decode the frames and run the VGG on them")
    p.add_argument("--cnn", action="store_true", help="load the VGG (needed by --extfeatures)")
    p.add_argument("--model", default="imagenet-vgg-verydeep-16.mat", help="MatConvNet VGG-16 file, or synthetic:N")
    p.add_argument("--vggtype", default="bf16", choices=("f32", "bf16"), help="arithmetic of the VGG forward")
    p.add_argument("--chunk", type=int, default=64, help="frames per VGG forward")
    p.add_argument("--train", action="store_true")
    p.add_argument("--eval", action="store_true")
    p.add_argument("--hidden", type=int, default=256)
    p.add_argument("--clip", type=int, default=16, help="frames per clip (T)")
    p.add_argument("--stride", type=int, default=8, help="frames between clip starts")
    p.add_argument("--batchsize", type=int, default=32, help="clips per step")
    p.add_argument("--epochs", type=int, default=1)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--gclip", type=float, default=0.0, help="Clip the global gradient norm to this on the device (0 = off).")
    p.add_argument("--drop_in", type=float, default=0.0, metavar="P",
                   help="--train: dropout on the frame feature that enters the LSTM (the paper: 0.9; 0 = off)")
    p.add_argument("--drop_out", type=float, default=0.0, metavar="P",
                   help="--train: dropout on the LSTM output before the classifier (the paper: 0.5; 0 = off)")
    p.add_argument("--atype", default="bf16", choices=("f32", "bf16"), help="arithmetic of the LSTM and the head")
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--savefile")
    p.add_argument("--loadfile")
    return p.parse_args(argv)


def read_list(path):
    out = []
    base = os.path.dirname(os.path.abspath(path))
    with open(path) as fh:
        for line in fh:
            parts = line.split()
            if not parts:
                continue
            d = parts[0] if os.path.isabs(parts[0]) else os.path.join(base, parts[0])
            out.append((d, int(parts[1]) if len(parts) > 1 else -1))
    return out


def frame_files(d):
    return [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.lower().endswith((".jpg", ".jpeg", ".png"))]


def load_features(path):
    z = np.load(path)
    n = int(z["n_videos"])
    return [z["video_%d" % i] for i in range(n)], z["labels"].astype(np.int32), [str(s) for s in z["names"]]


def extract(o):
    import torch
    from PIL import Image

    from lrcn_amd import lrcn as L
    from lrcn_amd import formats as fmt

    if not o.cnn:
        raise SystemExit("--extfeatures needs --cnn")
    vdt = L.LRCN_BF16 if o.vggtype == "bf16" else L.LRCN_F32
    ctx = L.Context(8, 8, 8, 8, max_B=1, max_T=1, vgg_dtype=vdt, max_images=o.chunk)   # the VGG only: a minimal caption shape
    mean = L.VGG_MEAN
    if o.model.startswith("synthetic"):
        L.vgg_load(ctx, *L.synthetic_vgg_weights(seed=int(o.model.split(":")[1]) if ":" in o.model else 1, bias_std=0.05))
    else:
        cw, cb, fc6, fc7, m = fmt.load_vgg_mat(o.model)
        if m is not None:
            mean = tuple(float(v) for v in m)
        L.vgg_load(ctx, [L.to_jl(w) for w in cw], [torch.as_tensor(b).cuda() for b in cb],
                   (L.to_jl(fc6[0]), torch.as_tensor(fc6[1]).cuda()), (L.to_jl(fc7[0]), torch.as_tensor(fc7[1]).cuda()))
        if fmt.load_vgg_mat.average_image is not None:
            L.set_average_image(ctx, fmt.load_vgg_mat.average_image)
            mean = None
    videos = read_list(o.list)
    out = {"n_videos": np.array(len(videos)), "labels": np.array([lab for _, lab in videos], np.int32),
           "names": np.array([os.path.basename(d.rstrip("/")) for d, _ in videos])}
    for i, (d, _) in enumerate(videos):
        files = frame_files(d)
        if not files:
            raise SystemExit("%s holds no frames" % d)
        feats = np.zeros((len(files), L.CNNOUT), np.float32)
        for s in range(0, len(files), o.chunk):
            ims = []
            for f in files[s:s + o.chunk]:
                im = Image.open(f)
                ims.append(np.asarray(im if im.mode in ("L", "RGB", "RGBA") else im.convert("RGB")))
            crops = L.resize_crop_u8(ctx, ims)
            feats[s:s + len(ims)] = L.from_jl(L.convnet_u8(ctx, crops, mean=mean))
        out["video_%d" % i] = feats
        say("video %d / %d: %d frames" % (i + 1, len(videos), len(files)))
    ctx.sync()
    np.savez(o.features, **out)
    say("features written to", o.features)
    return 0


def train(o):
    from lrcn_amd import activity as A

    vf, labels, _ = load_features(o.features)
    C = int(labels.max()) + 1
    dt = A.LRCN_BF16 if o.atype == "bf16" else A.LRCN_F32
    if o.loadfile:
        m = A.ActivityModel.load(o.loadfile, max_B=o.batchsize, max_T=o.clip, dtype=dt)
        if m.C < C:
            raise SystemExit("the model has %d classes, the features' labels go up to %d" % (m.C, C - 1))
    else:
        m = A.ActivityModel(vf[0].shape[1], o.hidden, C, max_B=o.batchsize, max_T=o.clip, dtype=dt, seed=o.seed)
    specs = [(v, s, n) for v, f in enumerate(vf) for (s, n) in A.clips(f.shape[0], o.clip, o.stride)]
    rng = np.random.default_rng(o.seed)
    say("%d videos, %d clips, %d classes" % (len(vf), len(specs), C))
    for ep in range(1, o.epochs + 1):
        order = rng.permutation(len(specs))
        tot, n = 0.0, 0
        for i in range(0, len(order), o.batchsize):
            sp = [specs[k] for k in order[i:i + o.batchsize]]
            x, lens = A.gather_clips(vf, sp, o.clip)
            lab = labels[[v for v, _, _ in sp]]
            tot += m.train_step(x, lab, lens, o.clip, lr=o.lr, gclip=o.gclip, pdrop_in=o.drop_in, pdrop_out=o.drop_out) * float(lens.sum())
            n += int(lens.sum())
        say("epoch %d loss %.6f" % (ep, tot / max(n, 1)))
    m.sync()
    if o.savefile:
        m.save(o.savefile)
        say("model written to", o.savefile)
    return 0


def evaluate(o):
    from lrcn_amd import activity as A

    if not o.loadfile:
        raise SystemExit("--eval needs --loadfile")
    vf, labels, _ = load_features(o.features)
    m = A.ActivityModel.load(o.loadfile, max_B=o.batchsize, max_T=o.clip)
    vp, per_clip = m.predict_videos(vf, T=o.clip, stride=o.stride, batch=o.batchsize)
    clip_acc = float(np.mean([np.argmax(p) == labels[v] for v, p in per_clip]))
    video_acc = float(np.mean(np.argmax(vp, 0) == labels))
    say("clip accuracy %.4f (%d clips) video accuracy %.4f (%d videos)" % (clip_acc, len(per_clip), video_acc, len(vf)))
    return 0


def main(argv=None):
    o = parse(sys.argv[1:] if argv is None else argv)
    if o.extfeatures:
        if not o.list or not o.features:
            raise SystemExit("--extfeatures needs --list and --features")
        return extract(o)
    if o.train:
        if not o.features:
            raise SystemExit("--train needs --features")
        return train(o)
    if o.eval:
        if not o.features:
            raise SystemExit("--eval needs --features")
        return evaluate(o)
    raise SystemExit("nothing to do: --extfeatures, --train or --eval")


if __name__ == "__main__":
    sys.exit(main())
