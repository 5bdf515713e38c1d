"""CPU: tests/avg_image_case.py's average image is decisive at the fp8 path's bound -- the oracle's features under the transposed average
image lie more than 0.30 (relative L2, per image) from those under the right one, twice the 0.15 the GPU test allows."""
import numpy as np

import avg_image_case as ac


def test_the_transposed_average_image_is_more_than_twice_the_fp8_bound_away():
    img, avg = ac.inputs()
    assert img.shape == (2, 224, 224, 3) and img.dtype == np.uint8 and avg.shape == (224, 224, 3) and avg.dtype == np.float32
    assert np.abs(avg - np.transpose(avg, (1, 0, 2))).max() > 800.0      # far from symmetric
    ref, wrong = ac.features(), ac.features(True)
    assert ref.shape == wrong.shape == (2, 4096) and np.isfinite(ref).all() and np.isfinite(wrong).all()
    for n in range(2):
        sep = ac.rel_l2(wrong[n], ref[n])
        cos = float((wrong[n] * ref[n]).sum() / (np.linalg.norm(wrong[n]) * np.linalg.norm(ref[n])))
        print("image %d: ||wrong - ref|| / ||ref|| = %.4f, cosine %.5f" % (n, sep, cos))
        assert sep > ac.SEPARATION, (n, sep)
    assert ac.SEPARATION >= 2 * 0.15
