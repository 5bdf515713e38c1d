"""CPU: image-caption retrieval metrics (lrcn_amd.retrieval; paper section 5.1 / Table 2) on hand-built score matrices with known answers."""
import numpy as np
import pytest

from lrcn_amd import retrieval as R


def test_caption_to_image_known_ranks_and_ties():
    # 3 images x 4 captions; caption m belongs to image gt[m]
    s = np.array([[5.0, 1.0, 2.0, 0.0],
                  [5.0, 3.0, 2.0, 1.0],
                  [1.0, 2.0, 2.0, 9.0]])
    gt = [1, 1, 2, 0]
    # caption 0: images 0 and 1 tie at 5 -> image 0 first (lower index), image 1 rank 2
    # caption 1: image 1 (3) first -> rank 1;  caption 2: all tie at 2 -> image 2 rank 3;  caption 3: image 0 (0) last -> rank 3
    m = R.metrics(s, gt, norm="sum")["caption_to_image"]
    assert m == {"R@1": 25.0, "R@5": 100.0, "R@10": 100.0, "Medr": 2.5}


def test_image_to_caption_best_of_ground_truth_captions():
    # image 0 has five captions (0..4) and only the 3rd (index 2) is ranked first; the others rank below foreign captions
    N, M = 2, 10
    s = np.zeros((N, M))
    s[0] = [0.1, 0.2, 9.0, 0.3, 0.4, 5.0, 6.0, 7.0, 8.0, 0.5]
    s[1] = [10.0, 11.0, 12.0, 13.0, 14.0, 6.0, 7.0, 0.0, 0.0, 0.0]
    gt = [0, 0, 0, 0, 0, 1, 1, 1, 1, 1]
    # image 0: caption 2 at rank 1.  image 1: captions 4, 3, 2, 1, 0 first, then its own caption 6 at rank 6
    i2c = R.metrics(s, gt, norm="sum")["image_to_caption"]
    assert i2c == {"R@1": 50.0, "R@5": 50.0, "R@10": 100.0, "Medr": 3.5}
    # image 1's best own caption (5) ties with a foreign one (0) at the top: the lower index, the foreign caption, goes first -> rank 2
    s[1] = [5.0, 0.0, 0.0, 0.0, 0.0, 5.0, 0.0, 0.0, 0.0, 0.0]
    i2c = R.metrics(s, gt, norm="sum")["image_to_caption"]
    assert i2c == {"R@1": 50.0, "R@5": 100.0, "R@10": 100.0, "Medr": 1.5}


def test_ties_go_to_the_lower_index_in_both_directions():
    s = np.ones((3, 3))
    gt = [2, 1, 0]
    m = R.metrics(s, gt, norm="sum")
    # caption m ranks images 0, 1, 2: its image gt[m] has rank gt[m] + 1
    assert m["caption_to_image"]["Medr"] == 2.0 and m["caption_to_image"]["R@1"] == pytest.approx(100.0 / 3)
    # image n ranks captions 0, 1, 2: its caption 2 - n has rank 3 - n
    assert m["image_to_caption"]["Medr"] == 2.0 and m["image_to_caption"]["R@1"] == pytest.approx(100.0 / 3)


def test_recall_at_k_boundaries():
    N = 12
    s = np.zeros((N, N))
    for m in range(N):   # caption m's own image (m) ranked exactly m + 1 by the caption
        order = [i for i in range(N) if i != m]
        order.insert(m, m)
        for rank, n in enumerate(order):
            s[n, m] = -rank
    c2i = R.metrics(s, list(range(N)), norm="sum")["caption_to_image"]
    assert c2i["R@1"] == pytest.approx(100.0 / 12) and c2i["R@5"] == pytest.approx(500.0 / 12)
    assert c2i["R@10"] == pytest.approx(1000.0 / 12) and c2i["Medr"] == 6.5


def test_caption_to_image_does_not_depend_on_the_normalisation():
    rng = np.random.default_rng(0)
    N, M = 15, 60
    s = rng.standard_normal((N, M)) * 5 - 20
    gt = rng.integers(0, N, size=M)
    lens = rng.integers(1, 29, size=M)
    a = R.metrics(s, gt, norm="sum", lens=lens)
    b = R.metrics(s, gt, norm="mean", lens=lens)
    assert a["caption_to_image"] == b["caption_to_image"]
    # image to caption does depend on it here: divide by (L + 1) by hand and compare with "sum"
    c = R.metrics(s / (lens + 1.0)[None, :], gt, norm="sum")
    assert b["image_to_caption"] == c["image_to_caption"]


def test_bad_arguments():
    s = np.zeros((2, 3))
    with pytest.raises(ValueError):
        R.metrics(s, [0, 1], norm="sum")
    with pytest.raises(ValueError):
        R.metrics(s, [0, 1, 2], norm="sum")
    with pytest.raises(ValueError):
        R.metrics(s, [0, 1, 1], norm="mean")
    with pytest.raises(ValueError):
        R.metrics(s, [0, 1, 1], norm="max", lens=[1, 1, 1])


def test_format_line():
    m = {"R@1": 40.0, "R@5": 71.25, "R@10": 80.0, "Medr": 2.0}
    assert R.format_line("Caption to Image", m) == "Caption to Image: R@1 40.0 R@5 71.2 R@10 80.0 Medr 2.0"
