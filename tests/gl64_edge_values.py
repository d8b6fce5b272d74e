"""Edge words of the 64-bit field for the tests (test infrastructure; the 252-bit field's counterpart is tests/edge_values.py).

p = 2^64 - 2^32 + 1.  csrc/gl64.h keeps values as LAZY words - any 64-bit word congruent to the value - and only a residue below
EPS = 2^32 - 1 has a second word (r + p < 2^64): one uniform draw in 2^32.  So the events the lazy discipline exists for - the borrow
in gl_reduce128_lazy, a product or a sum landing in [p, 2^64) - never happen on uniform data.  This module supplies
  * EDGE / edge_column: the words at both ends of the field and at its 32-bit seams, mixed into draws from the whole of [0, p);
  * small_targets / force3: residues below EPS and the solver that FORCES an Fq3 output of a kernel onto them (where a missing
    canonicalisation stores p + r with certainty, not with probability 2^-32);
  * a model of gl64.h's word arithmetic in Python integers, written from the header's comments, that says which branch a call took."""
import numpy as np

P = 2**64 - 2**32 + 1
EPS = 2**32 - 1                                             # 2^64 mod p; residues below it have a second 64-bit word
INV7 = pow(7, -1, P)
ROOT32 = pow(7, (P - 1) >> 32, P)                           # the 2^32-th root of unity 1753635133440165772


def _edge_list():
    vals = [0, 1, 2, 3,
            P - 1, P - 2, P - 3,
            2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1,          # EPS - 1, EPS, EPS + 1 ...: the last residues with two words, the first without
            P - 2**32 - 1, P - 2**32, P - 2**32 + 1,         # 2^64 - 2^33 + {0, 1, 2}: where a wrapped sum + EPS comes closest to 2^64
            2**63, 2**63 - 1,
            (P - 1) // 2, (P + 1) // 2,
            2**48, P - 2**48,                                # 2^48 * 2^48 = 2^96 = -1
            7, INV7,
            ROOT32, P - ROOT32,
            2**32 * (2**32 - 1) % P, 2**64 - 2**33,          # hi_lo * EPS at its largest; the largest wrapped word before + EPS
            0xFFFFFFFE00000002, 0x00000000FFFFFFFF << 16]
    out = []
    for v in vals:
        assert 0 <= v < P
        if v not in out:
            out.append(v)
    return out


EDGE = _edge_list()
_EDGE_WORDS = np.array(EDGE, dtype=np.uint64)


def edge_column(n, seed=0):
    """(n,) uint64 of residues < p: uniform draws from the whole of [0, p) with EDGE entries at about half of the positions, chosen at
    random; the EDGE list first, in order, rotated by the seed; and for n >= 8 len(EDGE) a run of p - 1 and the alternations
    0 / p - 1 and 1 / p - 2 - so that an edge word meets every butterfly partner, fold row and column"""
    rng = np.random.default_rng(0x6164ED6E0000 + seed)
    out = rng.integers(0, P, size=n, dtype=np.uint64)
    scattered = rng.random(n) < 0.5
    out[scattered] = _EDGE_WORDS[rng.integers(0, len(EDGE), size=int(scattered.sum()))]
    ne = len(EDGE)
    head = min(n, ne)
    out[:head] = _EDGE_WORDS[(np.arange(head) + seed) % ne]
    if n >= 8 * ne:
        q = n // 4
        out[q:q + ne] = P - 1
        alt = np.arange(2 * q, 2 * q + 2 * ne)
        out[alt[0::2]], out[alt[1::2]] = 0, P - 1
        alt = np.arange(3 * q, 3 * q + 2 * ne)
        out[alt[0::2]], out[alt[1::2]] = 1, P - 2
    assert (out < np.uint64(P)).all()
    return out


def small_targets(shape, seed=0):
    """uint64 residues in [0, EPS): uniform there, with 0, 1 and EPS - 1 = 2^32 - 2 at about a quarter of the positions.  Each has
    the second word r + p < 2^64, which is what a kernel stores when the last canonicalisation is missing"""
    rng = np.random.default_rng(0x5A11 + seed)
    out = rng.integers(0, EPS, size=shape, dtype=np.uint64)
    pick = rng.random(out.shape) < 0.25
    out[pick] = np.array([0, 1, EPS - 1], dtype=np.uint64)[rng.integers(0, 3, size=int(pick.sum()))]
    assert (out < np.uint64(EPS)).all()
    return out


def assert_canonical(arr, what):
    """every word of a uint64 array is < p; names the first (flattened) offender"""
    a = np.asarray(arr)
    assert a.dtype == np.uint64, (what, a.dtype)
    bad = np.nonzero(a.reshape(-1) >= np.uint64(P))[0]
    if bad.size:
        v = int(a.reshape(-1)[bad[0]])
        raise AssertionError("%s: non-canonical words stored: %d, first at %d: %#x = p + %d" % (what, bad.size, bad[0], v, v - P))


# ---- forcing Fq3 outputs ---------------------------------------------------------------------------------------------------------
def solve3(m, rhs):
    """x with m x = rhs (mod p): a 3 x 3 matrix of Python integers, Gaussian elimination with the first non-zero pivot; None if singular"""
    a = [[int(v) % P for v in m[r]] + [int(rhs[r]) % P] for r in range(3)]
    for c in range(3):
        piv = next((r for r in range(c, 3) if a[r][c]), None)
        if piv is None:
            return None
        a[c], a[piv] = a[piv], a[c]
        inv = pow(a[c][c], -1, P)
        a[c] = [v * inv % P for v in a[c]]
        for r in range(3):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [(v - f * u) % P for v, u in zip(a[r], a[c])]
    return [a[r][3] for r in range(3)]


def force3(ref, inputs, cells, targets):
    """inputs: list of uint64 arrays; ref(inputs) -> (m, 3) uint64, output j (an element of Fq3) Fp-AFFINE in the three input cells
    cells[j] = ((array, index), (array, index), (array, index)) and independent of the other outputs' cells.  Four runs of ref - all
    those cells 0, then each one of the three at 1 - give every output's 3 x 3 matrix and offset; returns a copy of the inputs with the
    cells solved so that ref(result) == targets.  Every output must be solvable (a singular matrix has probability ~2^-64: loud)."""
    flat = [c for trio in cells for c in trio]
    assert all(len(trio) == 3 for trio in cells) and len(set(flat)) == len(flat), "three cells of its own per output"
    trial = [np.array(a, dtype=np.uint64, copy=True) for a in inputs]

    def run(which):
        for trio in cells:
            for i, (arr, idx) in enumerate(trio):
                trial[arr][idx] = 1 if i == which else 0
        return [[int(v) for v in row] for row in np.asarray(ref(trial)).reshape(-1, 3)]
    y0 = run(-1)
    ys = [run(i) for i in range(3)]
    tgt = np.asarray(targets, dtype=np.uint64).reshape(-1, 3)
    assert len(y0) == len(cells) == len(tgt)
    out = [np.array(a, dtype=np.uint64, copy=True) for a in inputs]
    for j, trio in enumerate(cells):
        m = [[(ys[i][j][t] - y0[j][t]) % P for i in range(3)] for t in range(3)]
        x = solve3(m, [(int(tgt[j][t]) - y0[j][t]) % P for t in range(3)])
        assert x is not None, "output %d does not depend on its three cells (singular system)" % j
        for (arr, idx), v in zip(trio, x):
            out[arr][idx] = v
    got = np.asarray(ref(out)).reshape(-1, 3)
    assert np.array_equal(got, tgt), "the reference does not reach the targets: the outputs are not affine in their own cells alone"
    return out


# ---- gl64.h's word arithmetic in Python integers -----------------------------------------------------------------------------------
# Written from the header's comments, word for word: every intermediate is masked to 64 bits where the C is a uint64_t.  Each function
# returns (result, branches), branches being the set of the names of the conditional corrections the call took.
M64 = (1 << 64) - 1


def gl_canon(r):
    return (r - P, {"canon"}) if r >= P else (r, set())


def gl_add(a, b):
    """canonical + canonical -> canonical"""
    s, br = (a + b) & M64, set()
    if s < a:
        s, br = s + EPS, {"add_wrap"}                        # + 2^64 = + EPS; cannot wrap again: a, b < p
        assert s <= M64
    if s >= P:
        br.add("sum_above_p")                                # the word a lazy addition would leave
    return gl_canon(s)[0], br


def gl_sub_lazy(a, b):
    """lazy - canonical -> lazy"""
    s, br = (a - b) & M64, set()
    if a < b:
        assert s > EPS                                       # wrapped word >= 2^64 - (p - 1) = 2^32
        s, br = s - EPS, {"sub_borrow"}
    return s, br


def gl_mul_wide(a, b):
    """any two words -> (lo, hi) by four 32 x 32 + 64 multiply-adds, none of which overflows"""
    a0, a1, b0, b1 = a & EPS, a >> 32, b & EPS, b >> 32
    p00 = a0 * b0
    p01 = a0 * b1 + (p00 >> 32)
    p10 = a1 * b0 + (p01 & EPS)
    hi = a1 * b1 + (p01 >> 32) + (p10 >> 32)
    lo = ((p10 << 32) & M64) | (p00 & EPS)
    assert max(p00, p01, p10, hi) <= M64 and (hi << 64 | lo) == a * b
    return lo, hi


def gl_reduce128_lazy(lo, hi):
    """lo + 2^64 hi = lo + EPS hi_lo - hi_hi, as a lazy word"""
    hi_hi, hi_lo, br = hi >> 32, hi & EPS, set()
    t = (lo - hi_hi) & M64
    if lo < hi_hi:
        assert t >= 2**64 - 2**32                            # so no second borrow
        t, br = t - EPS, {"reduce_borrow"}
    m = hi_lo * EPS
    r = (t + m) & M64
    if r < t:
        assert r <= 2**64 - 2**33                            # so + EPS stays below 2^64
        r += EPS
        br.add("reduce_wrap")
    if r >= P:
        br.add("product_above_p")
    return r, br


def gl_mul(a, b):
    """lazy x lazy -> canonical"""
    r, br = gl_reduce128_lazy(*gl_mul_wide(a, b))
    return gl_canon(r)[0], br


def glw_reduce(l0, l1, h0, h1):
    """the wide accumulator l0 + 2^32 l1 + 2^64 h0 + 2^96 h1 = l0 + 2^32 l1 + (2^32 - 1) h0 - h1 -> canonical"""
    def add128(lo, hi, alo, ahi):
        lo2 = (lo + alo) & M64
        return lo2, (hi + ahi + (lo2 < alo)) & M64
    lo, hi = add128(l0, 0, (l1 << 32) & M64, l1 >> 32)
    lo, hi = add128(lo, hi, (h0 << 32) & M64, h0 >> 32)
    hi = (hi - (lo < h0)) & M64
    lo = (lo - h0) & M64
    r, br = gl_reduce128_lazy(lo, hi)
    r = gl_canon(r)[0]
    b = gl_canon(h1)[0]
    return (r - b if r >= b else (r + (P - b)) & M64), br
