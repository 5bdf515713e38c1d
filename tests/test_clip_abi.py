"""CPU: liblrcn_hip.so exports every symbol include/lrcn_clip.h declares, the binding covers exactly that set, and include/lrcn.h's own
set is what it was (no compute calls)."""
import ctypes
import os
import re

import lrcn_amd
from lrcn_amd import _lib


def _declared(header):
    txt = open(header).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(lrcn_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_symbol_of_lrcn_clip_h():
    lrcn_amd.build()
    assert os.path.exists(_lib.LIB_PATH)
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared(_lib.CLIP_HEADER)
    assert len(names) == 10 and "lrcn_train_step_clip" in names and "lrcn_clip_stats" in names
    for n in names:
        assert hasattr(L, n), "missing export: " + n
    assert sorted(_lib.CLIP_SIGNATURES) == names


def test_lrcn_h_keeps_its_own_set():
    base = _declared(_lib.HEADER)
    assert sorted(_lib.SIGNATURES) == base
    assert not set(base) & set(_lib.CLIP_SIGNATURES)
    assert "LRCN_ABI_VERSION" not in open(_lib.CLIP_HEADER).read().replace("LRCN_ABI_VERSION is unchanged", "")


def test_stats_struct_matches_the_header():
    assert ctypes.sizeof(_lib.ClipStats) == 40
    assert [f[0] for f in _lib.ClipStats._fields_] == ["last_norm", "last_scale", "last_skipped", "steps", "clipped", "skipped"]


def test_bad_arguments_are_rejected_before_any_gpu_work():
    L = _lib.lib()
    st = _lib.ClipStats()
    assert L.lrcn_grad_sumsq(None, None, 0, 0, None) != 0
    assert L.lrcn_clip_set(None, 9, 5.0, None) != 0
    assert L.lrcn_clip_stats(None, ctypes.byref(st)) != 0
