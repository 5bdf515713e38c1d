"""CPU: the LRCN_* environment variables of csrc/ -- the code, DESIGN.md's table and the list of removed names agree."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "long-term-recurrent-convolutional-nn_amd", "csrc")
READERS = "knob.h"  # the one file that may call getenv

# removed as unreachable from any test, benchmark, binding or tool (DESIGN_HISTORY.md, Appendix A2)
REMOVED = {"LRCN_FREE_8P_MIN", "LRCN_BG_MINN", "LRCN_BG_SPLITK", "LRCN_8P_CFG", "LRCN_8P_TALL", "LRCN_FASTDIV", "LRCN_BG_ROUTE",
           "LRCN_BG_MINB", "LRCN_BG_CAP", "LRCN_FREE_CUS_HINT", "LRCN_ADAM_GROUP_WGS", "LRCN_XCNN_FORK", "LRCN_EMBED_SCATTER",
           "LRCN_LSTM_FUSED_MAXB", "LRCN_GEMM_TRACE", "LRCN_BENCH_ZERO"}


def read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def csrc_files():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(files) > 20, files
    return files


def names(text):
    return set(re.findall(r"\bLRCN_[A-Z0-9_]+\b", text))


def test_getenv_only_in_the_readers_header():
    callers = [os.path.basename(p) for p in csrc_files() if "getenv" in read(p)]
    assert callers == [READERS]


def test_knobs_read_in_csrc_are_the_ones_design_md_lists():
    in_code = set()
    for p in csrc_files():
        in_code |= set(re.findall(r"\bknob_(?:set|char|off|int)\(\s*\"(LRCN_[A-Z0-9_]+)\"", read(p)))
    rows = re.findall(r"^\| `(LRCN_[A-Z0-9_]+)` \|", read(os.path.join(ROOT, "DESIGN.md")), flags=re.M)
    assert len(rows) == len(set(rows)), "a variable has two rows"
    assert in_code == set(rows), (sorted(in_code - set(rows)), sorted(set(rows) - in_code))
    assert len(in_code) == 24
    # every reader call names its variable literally (nothing computed, nothing the scan above could miss)
    for p in csrc_files():
        if os.path.basename(p) == READERS:
            continue
        for call in re.findall(r"\bknob_(?:set|char|off|int)\(([^,)]*)", read(p)):
            assert re.fullmatch(r"\s*\"LRCN_[A-Z0-9_]+\"\s*", call), (p, call)


def test_removed_knobs_are_gone():
    for p in csrc_files() + [os.path.join(ROOT, "README.md"), os.path.join(ROOT, "DESIGN.md")]:
        assert not (names(read(p)) & REMOVED), (p, sorted(names(read(p)) & REMOVED))
