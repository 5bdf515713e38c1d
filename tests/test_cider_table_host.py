"""CPU: the host side of the device CIDEr-D (csrc/cider_table.h) against lrcn_amd.cider.CiderD on the seeded V = 13 corpus.  The header is
compiled into a stand-alone program (tests/cider_table_main.cpp) under AddressSanitizer and UBSan; nothing is loaded into Python."""
import os
import shutil
import struct
import subprocess

import pytest

import cider_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "long-term-recurrent-convolutional-nn_amd", "csrc")


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_tables_match_the_host_metric(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "cider_table_main")
    argv = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
            os.path.join(HERE, "cider_table_main.cpp"), "-o", exe]
    r = subprocess.run(argv, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("the compiler has no sanitizer runtime: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-3000:]

    V = 13
    refs, _ = cc.seeded(V)
    refs = dict(refs)
    refs[37] = [[], [5], [5, 6]]      # references that are empty or shorter than n
    refs[38] = []                     # an image without references (it still counts in N)
    flat = [(i, r) for i, rs in refs.items() for r in rs]
    corpus = str(tmp_path / "corpus.txt")
    with open(corpus, "w") as fh:
        fh.write("%d %d %d\n" % (len(refs), len(flat), V))
        for i, r in flat:
            fh.write(" ".join(str(x) for x in [i, len(r)] + list(r)) + "\n")
    r = subprocess.run([exe, corpus], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]

    host = cc.host_metric(refs)
    counts, keys, norms = {}, [dict() for _ in range(4)], {}
    for line in r.stdout.split("\n"):
        f = line.split()
        if not f:
            continue
        if f[0] == "N":
            counts[int(f[1])] = (int(f[2]), int(f[3]))
        elif f[0] == "K":
            g = tuple(f[3:])
            assert len(g) == int(f[1]) and g not in keys[len(g) - 1], line
            keys[len(g) - 1][g] = int(f[2], 16)
        elif f[0] == "R":
            norms[(int(f[1]), int(f[2]))] = (struct.unpack("<d", struct.pack("<Q", int(f[3], 16)))[0], int(f[4]), int(f[5]))
    for n in range(1, 5):
        want = host._idf[n - 1]
        distinct, slots = counts[n]
        assert distinct == len(want) == len(keys[n - 1]) and slots >= 2 * distinct and slots & (slots - 1) == 0, (n, distinct, len(want), slots)
        assert set(keys[n - 1]) == set(want)
        for g, b in keys[n - 1].items():
            assert b == bits(want[g]), (g, b, bits(want[g]))      # the host's bits: log N - log max(1, df)
    k = 0
    checked = 0
    for i, rs in refs.items():
        for j, words in enumerate(rs):
            vecs, hn, length = host._refs[i][j]
            for n in range(1, 5):
                got, entries, got_len = norms[(k, n)]
                assert got_len == length == len(words) and entries == len(vecs[n - 1])
                assert abs(got - hn[n - 1]) <= 1e-15 * abs(hn[n - 1]), (k, n, got, hn[n - 1])
                checked += 1
            k += 1
    assert checked == 4 * len(flat) and any(v[0] == 0.0 for v in norms.values()) and any(v[0] > 0.0 for v in norms.values())
