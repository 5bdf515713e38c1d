"""The fixture of test_gpu_image_front.py::test_full_vgg_fp8_with_average_image_vs_oracle, shared with its CPU side
(tests/test_avg_image_case.py): synthetic VGG-16 weights made on the HOST (so that both sides hold the same numbers), the two images of
test_full_vgg_with_average_image_vs_oracle, an average image that is far from symmetric, and the oracle's features for it (`ref`) and for
its transpose (`wrong`, what a forward that reads the average image in the other orientation computes).

The fp8 path's stated bound is loose -- cosine >= 0.99 and relative L2 <= 0.15 per image -- so the average image has to be decisive at THAT
bound: the ramp's amplitude is raised until ||wrong - ref|| / ||ref|| > 0.30 per image (0.8 per row, the bf16 test's, gives 0.177; 2 gives
0.26; 4 gives 0.41).  Features within 0.15 of `ref` then cannot be within 0.15 of `wrong`."""
import functools

import numpy as np

from lrcn_amd import lrcn as L
from oracle import oracle as orc

RAMP = 4.0          # per row of the average image: 40 .. 932 over the 224 rows
SEPARATION = 0.30   # ||wrong - ref|| / ||ref|| per image, at least


@functools.lru_cache(maxsize=None)
def weights():
    """(conv_w, conv_b, (fc6, b6), (fc7, b7)) on the host, in the layout L.vgg_load takes (move the tensors to the device as they are)."""
    return L.synthetic_vgg_weights(seed=2, device="cpu", bias_std=0.05)


def _host(w):
    return ([L.from_jl(t) for t in w[0]], [t.numpy() for t in w[1]], (L.from_jl(w[2][0]), w[2][1].numpy()), (L.from_jl(w[3][0]), w[3][1].numpy()))


@functools.lru_cache(maxsize=None)
def inputs():
    """(uint8 images [2][224][224][3], average image [224][224][3] float32)"""
    rng = np.random.default_rng(81)
    img = rng.integers(0, 256, size=(2, 224, 224, 3), dtype=np.uint8)
    avg = (40.0 + RAMP * np.arange(224, dtype=np.float32)[:, None, None] + rng.random((224, 224, 3)).astype(np.float32) * 20).astype(np.float32)
    return img, avg


@functools.lru_cache(maxsize=None)
def features(transposed=False):
    """The fp32 oracle's fc7 features [2][4096] under the average image, or under its transpose."""
    img, avg = inputs()
    h = _host(weights())
    return orc.vgg_forward(h[0], h[1], h[2], h[3], orc.preprocess_u8_avg(img, np.transpose(avg, (1, 0, 2)) if transposed else avg))


def rel_l2(a, ref):
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))
