"""CPU: the case table of tests/embed_grad_ref.py is what it says it is.  Every `int` case's float64 reference is integer-valued and below
2^24 (so float32 holds it, and every partial sum of it, exactly, and the GPU test may demand equality), and every token pattern has the segment
lengths it claims.  The issue's list of edges is asserted against the table, so a case cannot quietly leave it."""
import numpy as np
import pytest

import embed_grad_ref as er

ids = [c.id for c in er.CASES]


def test_ids_are_unique_and_the_named_edges_are_in_the_table():
    assert len(set(ids)) == len(ids)
    assert {1, 63, 64, 65, 4097, 8191, 8192} <= {c.n for c in er.CASES}
    assert {7, 8, 9, 511, 512, 513, 1025} <= {c.arg for c in er.CASES if c.pattern == "segment"}
    assert {64, 70, 72, 100, 1000} <= {c.E for c in er.CASES}
    assert {301, 320, 2540, 10640} <= {c.V for c in er.CASES}
    assert any(c.pattern == "one" and c.n == 8192 and c.kind == k for c in er.CASES for k in ("int",))
    assert any(c.pattern == "distinct" and c.n == c.V for c in er.CASES)
    real = [(c.pattern, c.arg, c.n, c.E, c.V) for c in er.CASES if c.kind == "real"]
    assert ("zipf", None, 3072, 1000, 10640) in real and any(r[:2] == ("segment", 513) for r in real) and any(r[0] == "one" and r[2] == 8192 for r in real)
    assert max(c.n * c.E for c in er.CASES) == 8192 * 1000


@pytest.mark.parametrize("c", er.CASES, ids=ids)
def test_token_pattern_has_the_segment_lengths_it_claims(c):
    tok = er.tokens(c)
    assert tok.dtype == np.int32 and tok.shape == (c.n,) and tok.min() >= 0 and tok.max() < c.V
    cnt = np.bincount(tok, minlength=c.V)
    exact, low, high = er.claims(c)
    for t, k in exact.items():
        assert cnt[t] == k, (t, cnt[t], k)
    rest = np.delete(cnt, list(exact))
    assert rest.max(initial=0) <= high and (rest.max(initial=0) >= low), (rest.max(initial=0), low, high)
    if c.pattern == "uniform":
        assert cnt[c.V - 1] >= 1 and (c.n == 1 or cnt[0] >= 1)
    if c.pattern == "segment":
        pos = np.flatnonzero(tok == er.SEG_TOKEN)
        assert (np.diff(pos) > 1).any(), "the segment's rows must be scattered through the row order, not one run"
        assert pos.max() - pos.min() >= c.n // 2
    if c.pattern == "distinct" and c.n == c.V:
        assert cnt.min() == 1


@pytest.mark.parametrize("c", er.CASES, ids=ids)
def test_int_references_are_exact_in_float32(c):
    x, ref = er.rows(c), er.reference(c)
    assert x.dtype == np.float32 and x.shape == (c.n, c.E) and ref.shape == (c.V, c.E)
    assert er.abi_image(ref).shape == (c.V * c.E,) and er.abi_image(ref)[1] == ref[1, 0]   # memory [E][V]: the token index runs fastest
    if c.kind == "real":
        b = er.bound(er.tokens(c), x, c.V)
        owned = np.bincount(er.tokens(c), minlength=c.V) > 0
        assert (b[owned] > 0).all() and (b[~owned] == 0).all() and (ref[~owned] == 0).all()
        return
    assert np.abs(x).max() <= 8 and np.array_equal(x, np.rint(x))
    assert np.array_equal(ref, np.rint(ref)) and np.abs(ref).max() < 2 ** 24
    # every partial sum of every subset: bounded by the sum of magnitudes
    assert er.scatter_sum(er.tokens(c), np.abs(x), c.V).max() < 2 ** 24
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
