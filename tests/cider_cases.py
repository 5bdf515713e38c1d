"""The corpora of the device CIDEr-D tests (tests/test_gpu_cider.py, tests/test_cider_table_host.py): not a test module.

The reference is lrcn_amd.cider.CiderD over the same ids written as word strings (str(id))."""
import functools

import numpy as np

from lrcn_amd.cider import CiderD

BOS, EOS = 1, 0


@functools.lru_cache(maxsize=None)
def seeded(V, seed=5):
    """37 images with 1 to 6 references each of 1 to 30 words, ids in [3, V); 300 hypotheses in three kinds by turns: a reference of the
    image with each word redrawn with probability 0.3, a reference of another image, 0 to 30 random words.
    -> (refs {image: [id lists]}, [(image, id list)] hypotheses)."""
    rng = np.random.default_rng(seed)
    n_images = 37
    refs = {i: [[int(t) for t in rng.integers(3, V, size=int(rng.integers(1, 31)))] for _ in range(int(rng.integers(1, 7)))] for i in range(n_images)}
    hyps = []
    for k in range(300):
        i = int(rng.integers(0, n_images))
        if k % 3 == 0:
            base = refs[i][int(rng.integers(0, len(refs[i])))]
            redraw = rng.random(len(base)) < 0.3
            fresh = rng.integers(3, V, size=len(base))
            h = [int(f) if r else b for b, r, f in zip(base, redraw, fresh)]
        elif k % 3 == 1:
            j = (i + 1 + int(rng.integers(0, n_images - 1))) % n_images
            h = list(refs[j][int(rng.integers(0, len(refs[j])))])
        else:
            h = [int(t) for t in rng.integers(3, V, size=int(rng.integers(0, 31)))]
        hyps.append((i, h))
    return refs, hyps


def as_words(ids):
    return [str(t) for t in ids]


def host_metric(refs):
    """cider.CiderD over the ids written as words."""
    return CiderD({i: [as_words(r) for r in rs] for i, rs in refs.items()})


@functools.lru_cache(maxsize=None)
def seeded_host_scores(V, seed=5):
    refs, hyps = seeded(V, seed)
    c = host_metric(refs)
    return np.asarray([c.score(i, as_words(h)) for i, h in hyps], np.float64)


def pack(id_lists, ld=None, eos=True, junk=None):
    """Word-id lists -> (tokens [R][ld] int32, out_len [R]) in the sampler's form: bos, the words, a closing eos when `eos`.  The tail behind
    out_len holds eos, or `junk` (an int) when given."""
    R = len(id_lists)
    n = np.asarray([len(w) for w in id_lists], np.int32)
    ld = ld or int(n.max()) + 2
    tok = np.full((R, ld), EOS if junk is None else junk, np.int32)
    tok[:, 0] = BOS
    out_len = n + (2 if eos else 1)
    for r, w in enumerate(id_lists):
        tok[r, 1:1 + len(w)] = w
        if eos:
            tok[r, 1 + len(w)] = EOS
    return tok, out_len.astype(np.int32)


def identity_vocab(V):
    """word str(id) -> id, for DeviceCiderD over references written as words."""
    return {str(t): t for t in range(V)}
