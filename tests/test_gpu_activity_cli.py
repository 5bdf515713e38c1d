"""GPU: tools/lrcn_activity.py end to end on a few tiny JPEG-frame "videos": --extfeatures (synthetic VGG) -> --train -> --eval; the loss
falls, the checkpoint round-trips to identical predictions and the features are lrcn_vgg_forward_u8 on the same crops."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_extract_train_eval(tmp_path, capsys):
    from PIL import Image

    from lrcn_amd import activity as A
    from lrcn_amd import lrcn as L

    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    cli = importlib.import_module("lrcn_activity")
    rng = np.random.default_rng(0)
    lines = []
    for v in range(6):
        d = tmp_path / ("v%d" % v)
        d.mkdir()
        label = v % 2
        for f in range(int(rng.integers(5, 9))):
            im = np.full((40, 48, 3), 40, np.uint8)
            im[..., label] = 200 if f % 2 == 0 else 120          # class = which colour channel carries the signal
            im += rng.integers(0, 30, im.shape).astype(np.uint8)
            Image.fromarray(im).save(str(d / ("%04d.jpg" % f)))
        lines.append("v%d %d" % (v, label))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(lines) + "\n")
    feats = str(tmp_path / "feats.npz")
    assert cli.main(["--extfeatures", "--cnn", "--model", "synthetic:1", "--list", str(lst), "--features", feats, "--chunk", "16"]) == 0
    z = np.load(feats)
    assert int(z["n_videos"]) == 6 and z["video_0"].shape[1] == 4096

    # the features are lrcn_vgg_forward_u8 on the same crops
    ctx = L.Context(8, 8, 8, 8, max_B=1, max_T=1, vgg_dtype=L.LRCN_BF16, max_images=16)
    L.vgg_load(ctx, *L.synthetic_vgg_weights(seed=1, bias_std=0.05))
    files = cli.frame_files(str(tmp_path / "v0"))
    crops = L.resize_crop_u8(ctx, [np.asarray(Image.open(f)) for f in files])
    ref = L.from_jl(L.convnet_u8(ctx, crops))
    np.testing.assert_array_equal(z["video_0"], ref)
    capsys.readouterr()

    # the synthetic VGG's untrained fc7 values are far outside a pretrained network's range and saturate the LSTM's gates: train on
    # standardised copies of the same features (a feature file is just per-video arrays, so this is what a user would do as well)
    allf = np.concatenate([z["video_%d" % i] for i in range(6)])
    mu, sd = allf.mean(0), allf.std(0) + 1e-6
    std = {k: z[k] for k in z.files}
    for i in range(6):
        std["video_%d" % i] = ((z["video_%d" % i] - mu) / sd).astype(np.float32)
    feats = str(tmp_path / "feats_std.npz")
    np.savez(feats, **std)
    z = np.load(feats)

    ck = str(tmp_path / "act.npz")
    assert cli.main(["--train", "--features", feats, "--hidden", "32", "--clip", "4", "--stride", "2", "--batchsize", "8", "--epochs", "10",
                     "--lr", "0.01", "--atype", "bf16", "--savefile", ck, "--seed", "2"]) == 0
    out = capsys.readouterr().out
    losses = [float(x) for x in re.findall(r"epoch \d+ loss ([0-9.]+)", out)]
    assert len(losses) == 10 and losses[-1] < 0.8 * losses[0], out
    assert cli.main(["--eval", "--loadfile", ck, "--features", feats, "--clip", "4", "--stride", "2", "--batchsize", "8"]) == 0
    out = capsys.readouterr().out
    assert re.search(r"clip accuracy [0-9.]+ \(\d+ clips\) video accuracy [0-9.]+ \(6 videos\)", out), out

    # the checkpoint round-trips to identical predictions
    vf = [z["video_%d" % i] for i in range(6)]
    m1 = A.ActivityModel.load(ck, max_B=8, max_T=4)
    p1, _ = m1.predict_videos(vf, T=4, stride=2)
    ck2 = str(tmp_path / "act2.npz")
    m1.save(ck2)
    p2, _ = A.ActivityModel.load(ck2, max_B=8, max_T=4).predict_videos(vf, T=4, stride=2)
    np.testing.assert_array_equal(p1, p2)
    z1, z2 = np.load(ck), np.load(ck2)
    for k in z1.files:
        np.testing.assert_array_equal(z1[k], z2[k])
