"""CPU: the variable-length caption path's host side (no GPU) -- captions.minibatch_varlen on the length histogram of the COCO reference
captions, the binding against include/lrcn_varlen.h, train.shard_block on padded batches, and the test oracle tests/varlen_ref.py itself
(on an equal-length batch it must reproduce the equal-length oracle)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import lrcn_amd
from lrcn_amd import _lib
from lrcn_amd import captions as cap
from lrcn_amd import train as trn
from oracle import oracle as orc

import varlen_ref as vr

HERE = os.path.dirname(os.path.abspath(__file__))


def reference_caps(times=1):
    """Captions of distinct words with the lengths of tests/golden/coco_ref_caption_lengths.json, sorted by length as the tokenizer
    returns them: ((id, words), length)."""
    hist = json.load(open(os.path.join(HERE, "golden", "coco_ref_caption_lengths.json")))["histogram"]
    lens = sorted(int(k) for k, v in hist.items() for _ in range(v * times))
    rng = np.random.default_rng(7)
    return [((i, ["w%d" % w for w in rng.integers(0, 50, size=n)]), n) for i, n in enumerate(lens)]


def test_binding_covers_exactly_the_varlen_header():
    lrcn_amd.build()
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.VARLEN_HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(lrcn_[a-z0-9_]+)\s*\(", txt)))
    assert names == ["lrcn_loss_grad_var", "lrcn_loss_var", "lrcn_train_step_var"]
    assert sorted(_lib.VARLEN_SIGNATURES) == names
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(L, n), "missing export: " + n
    assert not set(names) & set(_lib.SIGNATURES)   # lrcn.h's set is unchanged
    assert L.lrcn_abi_version() == _lib.LRCN_ABI_VERSION == 5


@pytest.mark.parametrize("B,share", [(256, 0.040), (64, 0.010)])
def test_minibatch_varlen_invariants_on_the_reference_lengths(B, share):
    caps = reference_caps()
    assert len(caps) == 5000 and caps[0][1] == 8 and caps[-1][1] == 45
    vocab = cap.build_vocab([caps], threshold=1)
    v = cap.minibatch_varlen(caps, vocab, B)
    kept = [c for c in caps if c[1] <= 28]
    assert len(kept) == 4996 and v.skipped == 4
    # every caption of <= 28 words exactly once, in the sorted list's order: batch k is the k-th window of `kept`
    assert [i for ids, _, _ in v for i in ids] == [c[0][0] for c in kept]
    assert all(len(ids) == B for ids, _, _ in v[:-1]) and 1 <= len(v[-1][0]) <= B and len(v) == -(-len(kept) // B)
    rows = padded = 0
    k = 0
    for ids, toks, lens in v:
        assert toks.dtype == np.int32 and lens.dtype == np.int32
        assert toks.shape == (int(lens.max()), len(ids)) and lens.shape == (len(ids),)
        for b in range(len(ids)):
            (i, words), n = kept[k]
            k += 1
            assert ids[b] == i and lens[b] == n
            np.testing.assert_array_equal(toks[:n, b], [vocab[w] - 1 for w in words])   # 0-based ABI ids
            assert (toks[n:, b] == 0).all()
        rows += (toks.shape[0] + 1) * len(ids)
        padded += int((toks.shape[0] - lens).sum())
    assert abs(padded / rows - share) < 5e-4, padded / rows   # the share the issue's table states, recomputed from the batches
    assert v.rows == rows and v.padded_rows == padded and abs(v.padded_share - padded / rows) < 1e-15


def test_minibatch_varlen_drops_nothing_where_the_reference_batcher_does():
    caps = reference_caps()
    vocab = cap.build_vocab([caps], threshold=1)
    gone = len(cap.reference_delete_ranges([c[1] for c in caps], 256))
    assert gone > 0.15 * len(caps)
    v = cap.minibatch_varlen(caps, vocab, 256)
    assert sum(len(ids) for ids, _, _ in v) + v.skipped == len(caps)
    # unknown words map to unk, a short split is one short batch, an empty one no batch
    one = cap.minibatch_varlen([((5, ["zzz", "w1"]), 2)], vocab, 8)
    assert len(one) == 1 and one[0][1].tolist() == [[cap.UNK - 1], [vocab["w1"] - 1]] and one[0][2].tolist() == [2]
    assert len(cap.minibatch_varlen([], vocab, 8)) == 0 and cap.minibatch_varlen([], vocab, 8).padded_share == 0.0
    with pytest.raises(ValueError):
        cap.minibatch_varlen(caps, vocab, 0)


def test_shard_block_slices_lens_and_passes_the_global_token_count():
    ids, toks, lens = list(range(8)), np.arange(24).reshape(3, 8), np.asarray([3, 3, 2, 2, 1, 1, 0, 0], np.int32)
    parts = [trn.shard_block((ids, toks, lens), 4, r) for r in range(4)]
    assert sum((p[0] for p in parts), []) == ids
    np.testing.assert_array_equal(np.concatenate([p[1] for p in parts], axis=1), toks)
    np.testing.assert_array_equal(np.concatenate([p[2] for p in parts]), lens)
    assert all(p[3] == int(lens.sum()) + 8 for p in parts) and trn.block_tokens(lens) == 20
    assert len(trn.shard_block((ids, toks), 4, 1)) == 2   # the equal-length block is what it was


def _tiny(seed, B, T, E=12, H=16, V=29, n_layers=2):
    rng = np.random.default_rng(seed)
    m = orc.init_weights(E, H, H, V, seed=seed + 1, n_layers=n_layers)
    feats = (rng.standard_normal((B, 4096)) * 0.05).astype(np.float32)
    tokens = rng.integers(3, V, size=(T, B)).astype(np.int32)
    return rng, m, feats, tokens


@pytest.mark.parametrize("n_layers", [2, 1])
@pytest.mark.parametrize("masks", [False, True])
def test_varlen_ref_reproduces_the_equal_length_oracle(n_layers, masks):
    B, T, E, H = 6, 4, 12, 16
    rng, m, feats, tokens = _tiny(3, B, T, n_layers=n_layers)
    kw = {}
    if masks:
        kw["mask1"] = ((rng.random((T + 1, B, E if n_layers == 2 else E + H // 2)) > 0.4) / 0.6).astype(np.float32)
        if n_layers == 2:
            kw["mask2"] = ((rng.random((T + 1, B, H)) > 0.4) / 0.6).astype(np.float32)
    for norm_B in (B, 4 * B):
        ref, ref_g = orc.loss(m, feats, tokens, norm_B=norm_B, want_grad=True, **kw)
        got, got_g = vr.loss(m, feats, tokens, [T] * B, norm_tokens=norm_B * (T + 1), want_grad=True, **kw)
        # float64 sums of float32 per-row results against one float32 batch result: a few float32 ulps
        assert abs(got - ref) <= 2e-6 * abs(ref)
        for n in orc.PARAM_NAMES:
            if ref_g.p[n].size:
                np.testing.assert_allclose(got_g.p[n], ref_g.p[n], rtol=2e-4, atol=2e-6 * np.abs(ref_g.p[n]).max(), err_msg=n)
    # integer row norms (the bf16 checks' form) give the same combination
    nb = vr.integer_row_norms([T] * B)
    assert nb == [B] * B
    a = vr.loss(m, feats, tokens, [T] * B, row_norms=nb, **kw)
    assert abs(a - orc.loss(m, feats, tokens, **kw)) <= 2e-6 * abs(a)


def test_varlen_ref_ignores_padding_and_counts_eos_of_an_empty_caption():
    B, T = 5, 4
    rng, m, feats, tokens = _tiny(9, B, T)
    lens = np.asarray([4, 2, 0, 3, 1], np.int32)
    a = vr.loss(m, feats, vr.pad_with(tokens, lens, 0), lens)
    b = vr.loss(m, feats, vr.pad_with(tokens, lens, rng.integers(0, 29, size=tokens.shape)), lens)
    assert a == b
    assert vr.norm_tokens_of(lens) == 15 and vr.integer_row_norms(lens) is None and vr.integer_row_norms([1, 1, 0, 0]) == [3, 3, 6, 6]
    # one empty caption: the single term -log p(eos | bos)
    one = vr.loss(m, feats[:1], np.zeros((0, 1), np.int32), [0])
    assert abs(one - orc.loss(m, feats[:1], np.zeros((0, 1), np.int32))) == 0.0
    l2 = vr.lens_with_integer_shares(17, rng)
    assert vr.integer_row_norms(l2) is not None and len(l2) == 17


def test_cli_rejects_varlen_without_train():
    """--varlen chooses the batches of --train; alone it is refused before anything is loaded."""
    import importlib
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    cli = importlib.import_module("lrcn")
    with pytest.raises(SystemExit, match="--varlen"):
        cli.main(["--coco", "--varlen", "--generate", "20"])
