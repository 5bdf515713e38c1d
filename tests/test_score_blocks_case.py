"""CPU: the plan score_impl makes of tests/score_blocks_case.py is the one tests/test_gpu_score.py's ride-along tests describe, and the
fixture can SEE a caption block that is fed another block's words: with the oracle alone, block 1's scores under block 0's input words
lie bounds away from the right ones."""
import numpy as np

import score_blocks_case as sc


def test_the_plan_of_blocks_pieces_and_active_rows():
    c = sc.case()
    assert sc.M == 300 and len(c.caps) == sc.M and c.feats.shape == (sc.N, 4096) and len(c.pi) == len(c.pc) == sc.P
    assert set(c.pc.tolist()) == set(range(sc.M)) and set(c.pi.tolist()) == set(range(sc.N))
    lens = np.array([len(c.caps[k]) for k in c.order])
    assert (np.diff(lens) <= 0).all() and (lens[:40] == 6).all() and lens[40] == 5
    # caption step t holds the Ma(t) captions of at least t words (steps 0 .. len): block 0 = ranks 0 .. 255, block 1 = ranks 256 .. 299
    Ma = [int((lens + 1 > t).sum()) for t in range(7)]
    assert Ma == [300, 300, 292, 229, 166, 103, 40]
    assert [min(256, a) for a in Ma] == [256, 256, 256, 229, 166, 103, 40]       # block 0: 216 rows ride along at its last step
    assert [max(0, a - 256) for a in Ma] == [44, 44, 36, 0, 0, 0, 0]             # block 1: 8 captions of one word, 36 of two
    # pair rows in caption-rank order, in pieces of 256, 256 and 8; the last piece holds one-word captions only
    rank = {k: j for j, k in enumerate(c.order)}
    rows = sorted(len(c.caps[k]) for k in c.pc.tolist())[::-1]
    assert rows[0] == 6 and rows[255] < 6 and rows[256] >= 2 and set(rows[512:]) == {1}
    assert sorted(rank[k] for k in c.pc.tolist())[-8] >= 292
    assert sc.N - sc.MAX_B == 4


def test_block_1_under_block_0s_words_is_bounds_away():
    """What `d_in + off[t]` without `+ j0` computes for caption block 1: the caption of rank 256 + j is fed word t - 1 of the caption of rank
    j.  Against the right score, in units of the bf16 bound: median 3.5, and three quarters of the 44 captions beyond one bound."""
    c, m = sc.case(), sc.model()
    ratio, emu = [], []
    for j in range(256, sc.M):
        k, other = c.order[j], c.order[j - 256]
        words = c.caps[k]
        feat = c.feats[j % sc.N]
        right = sc.score(m, feat, words, words)
        wrong = sc.score(m, feat, c.caps[other][:len(words)], words)
        ratio.append(abs(wrong - right) / sc.bound(right))
        emu.append(abs(sc.score(m, feat, words, words, bf16=True) - right) / sc.bound(right))
    ratio = np.array(ratio)
    print("block 1 fed block 0's words: |score - right| / bound min %.3g median %.3g max %.3g; beyond one bound: %d of %d; "
          "the emulation's own distance to f32 / bound: max %.3g" % (ratio.min(), np.median(ratio), ratio.max(), int((ratio > 1).sum()), len(ratio), max(emu)))
    assert np.median(ratio) >= 2.0 and (ratio > 1.0).mean() >= 0.75
    assert max(emu) <= 0.25   # while bf16 rounding itself stays a quarter of the bound away at most
