"""Exact host reference and the case table of the embedding-gradient tests (tests only; numpy, no GPU, nothing of the code under test).

dWembed[tok[m]][e] += rows[m][e]: the dual of the embedding gather.  The reference is a float64 np.add.at into [V][E]; the ABI's gradient is
V x E column-major, i.e. the memory image [E][V] that abi_image() returns.

Values (`kind`):
  int   integers in [-8, 8].  At most 8192 rows reach one token, so every partial sum of every subset is an integer of magnitude at most
        8192 * 8 = 65536 < 2^24, which float32 holds exactly: whatever the order -- atomics, eight waves, 512-row chunks -- a chain that adds
        every row once returns exactly the integer result, and exact zeros at every token that owns no row.
  real  standard normal.  n - 1 float32 additions in any order plus one rounding stay within n 2^-24 sum|x_i| per element (bound()).

Token patterns (`pattern`, with `arg`), every one checked against what it claims by tests/test_embed_grad_ref.py (claims()):
  uniform   n random ids; from two rows on, ids V - 1 and 0 are present (first and last row).  One row: id V - 1.
  one       one token owns every row.
  segment   token SEG_TOKEN owns exactly `arg` rows, scattered through the row order (a random subset of the positions, not a run); the other
            rows draw from the other tokens.
  distinct  no token twice (n <= V); n = V is every token once, in a random order.
  zipf      ids 3 + Zipf(1) over V - 3 words, as a caption batch has them: the busiest token owns about a tenth of the rows.

The edges the kernels of csrc/train_kernels.hip name, and the cases that walk them:
  rank_token_rows_kernel: 64 rows per block (n = 1, 63, 64, 65, 4097, 8191), the 8192-key maximum, four waves a quarter of the keys each;
  embed_segsum_kernel: the 512-row LDS chunk (segments of 511, 512, 513, 1025; 8192 = 16 chunks), eight waves (7, 8, 9), 256-column slices
  (E = 1000: three whole slices and 232 columns; E = 64 .. 100: part of one); embed_stage_to_grad_kernel: 64 x 64 tiles (E = 72, 100, 70, 1000;
  V = 301, 2540, 10640 are no multiple of 64), V % 4 != 0 (301, and 2540 % 4 == 0 / 320 % 64 == 0 for the vector stores), E % 4 != 0 (70).
"""
import functools

import numpy as np

SEG_TOKEN = 5
MAX_ROWS = 8192


class Case:
    def __init__(self, E, V, n, pattern, arg=None, kind="int"):
        self.E, self.V, self.n, self.pattern, self.arg, self.kind = E, V, n, pattern, arg, kind
        assert 1 <= n <= MAX_ROWS and kind in ("int", "real")

    @property
    def id(self):
        return "E%d-V%d-n%d-%s%s-%s" % (self.E, self.V, self.n, self.pattern, "" if self.arg is None else str(self.arg), self.kind)


def _table():
    c = []
    add = lambda *a, **k: c.append(Case(*a, **k))   # noqa: E731
    # row counts around the 64 rows of a rank block and up to the 8192 keys of the counting sort
    for n in (1, 63, 64, 65):
        add(64, 301, n, "uniform")
    add(72, 320, 4097, "uniform")
    add(100, 2540, 8191, "uniform")
    add(72, 301, 8192, "uniform")
    # one token owns every row: 16 chunks of 512
    add(100, 301, 8192, "one")
    add(64, 2540, 8192, "one", kind="real")
    # one segment at the wave and chunk edges, among other tokens
    add(64, 301, 260, "segment", 7)
    add(70, 301, 260, "segment", 8)
    add(100, 320, 260, "segment", 9)
    add(72, 2540, 900, "segment", 511)
    add(100, 2540, 900, "segment", 512)
    add(1000, 301, 900, "segment", 513)
    add(100, 301, 900, "segment", 513, kind="real")
    add(72, 10640, 1500, "segment", 1025)
    # no token twice
    add(64, 301, 301, "distinct")
    add(70, 320, 300, "distinct")
    # caption-like ids at the benchmark's width and row count
    add(1000, 10640, 3072, "zipf")
    add(1000, 10640, 3072, "zipf", kind="real")
    add(72, 2540, 4097, "zipf")
    # the largest upload: 8192 rows of 1000 floats
    add(1000, 320, 8192, "zipf")
    return c


CASES = _table()


def _seed(c):
    return [c.E, c.V, c.n, sorted(("uniform", "one", "segment", "distinct", "zipf")).index(c.pattern), c.arg or 0, int(c.kind == "real")]


@functools.lru_cache(maxsize=None)
def tokens(c):
    """int32 [n] token ids of the case (read-only)."""
    rng = np.random.default_rng(_seed(c) + [1])
    n, V = c.n, c.V
    if c.pattern == "uniform":
        t = rng.integers(0, V, size=n)
        t[0] = V - 1
        if n > 1:
            t[-1] = 0
    elif c.pattern == "one":
        t = np.full(n, SEG_TOKEN)
    elif c.pattern == "segment":
        others = np.delete(np.arange(V), SEG_TOKEN)
        t = rng.choice(others, size=n)
        t[rng.choice(n, size=c.arg, replace=False)] = SEG_TOKEN
    elif c.pattern == "distinct":
        t = rng.permutation(V)[:n]
    else:
        pz = 1.0 / np.arange(1, V - 3 + 1)
        t = rng.choice(V - 3, size=n, p=pz / pz.sum()) + 3
    t = t.astype(np.int32)
    t.setflags(write=False)
    return t


def claims(c):
    """What the pattern promises about the segment lengths, as (exact, low, high): `exact` {token: rows}; every token NOT in `exact` owns
    between 0 and `high` rows, and the busiest of them at least `low`."""
    n, V = c.n, c.V
    if c.pattern == "one":
        return {SEG_TOKEN: n}, 0, 0
    if c.pattern == "segment":
        return {SEG_TOKEN: c.arg}, 0, n - c.arg
    if c.pattern == "distinct":
        return {}, 1, 1
    if c.pattern == "zipf":
        return {0: 0, 1: 0, 2: 0}, n // 20, n // 5   # 1 / H(10637) = 0.101, 1 / H(2537) = 0.119, 1 / H(317) = 0.158 of the rows
    return {}, 1, n   # uniform: presence of V - 1 and 0 is checked apart


@functools.lru_cache(maxsize=None)
def rows(c):
    """float32 [n][E] addends of the case (read-only)."""
    rng = np.random.default_rng(_seed(c) + [2])
    if c.kind == "int":
        x = rng.integers(-8, 9, size=(c.n, c.E)).astype(np.float32)
    else:
        x = rng.standard_normal((c.n, c.E)).astype(np.float32)
    x.setflags(write=False)
    return x


def scatter_sum(tok, x, V):
    """float64 [V][E]: sum of the rows of x per token id."""
    out = np.zeros((V, x.shape[1]), np.float64)
    np.add.at(out, np.asarray(tok, np.int64), np.asarray(x, np.float64))
    return out


def bound(tok, x, V, extra=0):
    """float64 [V][E]: (n_seg + extra) 2^-24 sum|x_i| over each token's addends; 0 where a token owns no row.  Derived, not measured:
    n - 1 float32 additions in any order err by at most gamma(n - 1) sum|x_i|, gamma(k) = k u / (1 - k u), u = 2^-24 (Higham, Accuracy and
    Stability of Numerical Algorithms, section 4.2), and gamma(n - 1) <= n u while n (n - 1) <= 2^24, i.e. up to 4096 addends.  For the 8192-row
    segments gamma(8191) = 8195 u: the worst case lies 4e-4 of the bound above it, the bound is kept as n u all the same.  `extra`: further
    roundings per addend sum (a mask multiply the compiler may or may not fuse into the add)."""
    cnt = np.bincount(np.asarray(tok, np.int64), minlength=V).astype(np.float64)
    cnt = np.where(cnt > 0, cnt + extra, 0.0)
    return cnt[:, None] * 2.0 ** -24 * scatter_sum(tok, np.abs(np.asarray(x, np.float64)), V)


@functools.lru_cache(maxsize=None)
def reference(c):
    r = scatter_sum(tokens(c), rows(c), c.V)
    r.setflags(write=False)
    return r


def abi_image(g):
    """[V][E] logical -> the flat memory image of the ABI's V x E column-major gradient ([E][V])."""
    return np.ascontiguousarray(np.asarray(g).T).reshape(-1)
