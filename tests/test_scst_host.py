"""CPU: the host pieces of lrcn_amd/scst.py -- advantages() and build_batch() -- on hand-written sampler outputs.  No GPU."""
import numpy as np
import pytest

from lrcn_amd import scst
from lrcn_amd.lrcn import BOS, EOS, LrcnError


def test_advantages_greedy_and_mean():
    r = [[1.0, 3.0, 2.0], [0.5, 0.5, 0.5]]
    a = scst.advantages(r, [2.0, 0.5], baseline="greedy")
    assert a.shape == (2, 3) and np.array_equal(a, [[-1.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
    # "mean": each sample against the mean of the image's OTHER samples: 1 - (3 + 2) / 2, 3 - (1 + 2) / 2, 2 - (1 + 3) / 2
    m = scst.advantages(r, baseline="mean")
    assert np.array_equal(m, [[-1.5, 1.5, 0.0], [0.0, 0.0, 0.0]])
    assert np.array_equal(scst.advantages(r, [9.0, 9.0], baseline="mean"), m)    # r_greedy is not used
    with pytest.raises(LrcnError):
        scst.advantages([[1.0], [2.0]], baseline="mean")                         # S = 1: there are no other samples
    with pytest.raises(LrcnError):
        scst.advantages(r, baseline="greedy")                                    # needs r_greedy
    with pytest.raises(LrcnError):
        scst.advantages(r, [1.0], baseline="greedy")
    with pytest.raises(LrcnError):
        scst.advantages(r, [1.0, 2.0], baseline="median")


def sampler_output():
    """N = 2 images, S = 3 samples, nword = 3: rows of nword + 2 = 5 ids as lrcn_sample_batch writes them (bos first; out_len counts bos and
    the closing eos; the tail past out_len is not part of the row -- here a value that must not show up anywhere)."""
    J = 99   # junk past the row's end
    tok = np.asarray([[[BOS, EOS, J, J, J],        # eos at the first step: 0 words
                       [BOS, 7, 8, 9, 5],          # nword + 1 = 4 steps without eos: 4 words, trained with the eos term after them
                       [BOS, 4, EOS, J, J]],       # 1 word
                      [[BOS, 6, 5, EOS, J],        # 2 words
                       [BOS, 3, 4, 5, EOS],        # eos AT step nword + 1: 3 words, the row's own eos
                       [BOS, 8, EOS, J, J]]], np.int32)
    out_len = np.asarray([[2, 5, 3], [4, 5, 3]], np.int32)
    return tok, out_len


def test_build_batch_lengths_row_order_padding_and_norm_tokens():
    tok, out_len = sampler_output()
    adv = np.asarray([[0.5, -1.25, 0.0], [2.0, 0.0, -0.75]])
    tokens, lens, w, nt = scst.build_batch(tok, out_len, adv)
    assert tokens.dtype == np.int32 and lens.dtype == np.int32 and w.dtype == np.float32
    assert lens.tolist() == [0, 4, 1, 2, 3, 1]                     # row r = i S + s
    assert tokens.shape == (4, 6)                                  # T = the longest sample
    assert w.tolist() == [0.5, -1.25, 0.0, 2.0, 0.0, -0.75]
    assert nt == sum(n + 1 for n in lens.tolist()) == 17           # zero-weight rows included
    want = {0: [], 1: [7, 8, 9, 5], 2: [4], 3: [6, 5], 4: [3, 4, 5], 5: [8]}
    for r, ids in want.items():
        assert tokens[:lens[r], r].tolist() == ids, r
    assert ((tokens >= 0) & (tokens < 10)).all()                   # padding holds a valid id, never the junk past a row's end
    for i in range(2):
        for s in range(3):
            assert scst.sample_words(tok[i, s], out_len[i, s]) == want[i * 3 + s]


def test_build_batch_when_every_sample_is_empty_and_bad_input():
    tok = np.asarray([[[BOS, EOS, 0, 0], [BOS, EOS, 0, 0]]], np.int32)
    tokens, lens, w, nt = scst.build_batch(tok, [[2, 2]], [[1.0, -1.0]])
    assert tokens.shape == (1, 2) and lens.tolist() == [0, 0] and nt == 2      # T >= 1: the library's tokens array is never empty here
    with pytest.raises(LrcnError):
        scst.build_batch(tok, [[2, 2]], [[1.0]])                   # adv of another shape
    with pytest.raises(LrcnError):
        scst.build_batch(tok, [[1, 2]], [[1.0, 1.0]])              # a row has bos and at least one step
    bad = tok.copy()
    bad[0, 1, 0] = 5
    with pytest.raises(LrcnError):
        scst.build_batch(bad, [[2, 2]], [[1.0, 1.0]])              # no bos


def test_pack_samples_is_the_samplers_layout():
    res = [[([BOS, 4, EOS], -1.0), ([BOS, 7, 8, 9, 5], -2.0)]]
    tok, n = scst.pack_samples(res, nword=3)
    assert tok.shape == (1, 2, 5) and n.tolist() == [[3, 5]]
    assert tok[0, 0].tolist() == [BOS, 4, EOS, EOS, EOS] and tok[0, 1].tolist() == [BOS, 7, 8, 9, 5]
