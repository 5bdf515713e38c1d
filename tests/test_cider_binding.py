"""CPU: include/lrcn_cider.h beside the ABI -- declared by its own header, bound by its own table, exported by the library, absent from
lrcn.h and SIGNATURES (no compute calls)."""
import ctypes
import re

import lrcn_amd
from lrcn_amd import _lib

NAMES = ["lrcn_cider_create", "lrcn_cider_destroy", "lrcn_cider_last_error", "lrcn_cider_score", "lrcn_cider_score_dev", "lrcn_cider_set_stream",
         "lrcn_cider_stats"]


def test_cider_binding_declares_exactly_its_header():
    lrcn_amd.build()
    raw = open(_lib.CIDER_HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert sorted(set(re.findall(r"\b(lrcn_[a-z0-9_]+)\s*\(", txt))) == sorted(_lib.CIDER_SIGNATURES) == NAMES
    header = open(_lib.HEADER).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert name not in _lib.SIGNATURES and name not in header, name
        assert hasattr(so, name), name
    assert "#define LRCN_ABI_VERSION" not in raw and '#include "lrcn.h"' in raw
    assert "cider" not in header


def test_cider_stats_structure_has_the_headers_fields():
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.CIDER_HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct \{(.*?)\} lrcn_cider_stats_t;", txt, flags=re.S).group(1)
    fields = [re.sub(r"\[\d+\]", "", f.strip()) for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    assert fields == [f[0] for f in _lib.CiderStats._fields_], fields
    assert ctypes.sizeof(_lib.CiderStats) == 8 * 15


def test_bound_by_lib_and_create_rejects_bad_arguments_without_a_gpu():
    L = _lib.lib()     # binds CIDER_SIGNATURES too
    h = ctypes.c_void_p()
    img = (ctypes.c_int32 * 1)(0)
    off = (ctypes.c_int64 * 2)(0, 2)
    tok = (ctypes.c_int32 * 2)(3, 9)
    # a word id outside [0, V): refused by the host-side table builder, before any device is looked for
    assert L.lrcn_cider_create(0, 1, 1, img, off, tok, 9, ctypes.byref(h)) == -1 and not h.value
    assert b"outside [0,9)" in L.lrcn_cider_last_error(None)
    img[0] = 1
    assert L.lrcn_cider_create(0, 1, 1, img, off, tok, 10, ctypes.byref(h)) == -1
    assert b"ref_image[0]" in L.lrcn_cider_last_error(None)
