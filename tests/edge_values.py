"""Edge values of the 252-bit field for the tests (test infrastructure).

`examples.random_column` masks the top limb to 59 bits, so every element it draws is below 2^251 - and p = 2^251 + 17 2^192 + 1,
so the stored values in [2^251, p) (p - 1 and p - 2 among them: the ones whose top 28-bit limb holds a quotient bit, fl252.h)
never reach a kernel from it.  This module draws from the whole of [0, p) and mixes in the values where the lazy bounds of
fl252.h / fp252.h have their edge cases.  Everything here is a STORED value: the kernels take and return Montgomery images, any
integer < p being one."""
import numpy as np

P = 2**251 + 17 * 2**192 + 1
MASK64 = (1 << 64) - 1
R256 = pow(2, 256, P)                     # the memory format's Montgomery factor
R280 = pow(2, 280, P)                     # the Pedersen kernels' domain (ec252.h: x * 2^280)


def _edge_list():
    rng = np.random.default_rng(0x251)
    top = [2**251 + int.from_bytes(rng.bytes(24), "little") % (P - 2**251) for _ in range(4)]     # [2^251, p)
    vals = [0, 1, 2,
            P - 1, P - 2, P - 3,
            2**251 - 1, 2**251, 2**251 + 1, 2**251 + 2**192,
            *top,
            (P - 1) // 2, (P + 1) // 2,
            2**192 - 1, 2**224 - 1,                                   # a 32-bit word boundary on a 28-bit limb boundary
            R256, P - R256, 2 * R256 % P, (P - 2 * R256) % P,           # Montgomery images of 1, -1, 2, -2 (0 is above)
            R280, P - R280]                                             # R280 images of 1, -1
    out = []
    for v in vals:
        assert 0 <= v < P
        if v not in out:
            out.append(v)
    return out


EDGE = _edge_list()


def to_limbs(values):
    """python ints -> (len, 4) uint64 little-endian limbs (no conversion: stored values stay stored values)"""
    return np.array([[(int(v) >> (64 * k)) & MASK64 for k in range(4)] for v in values], dtype=np.uint64).reshape(-1, 4)


def from_limbs(arr):
    """(..., 4) uint64 -> list of python ints (flattened over the leading axes)"""
    a = np.ascontiguousarray(arr, dtype="<u8").reshape(-1, 4)
    return [int(a[i, 0]) | int(a[i, 1]) << 64 | int(a[i, 2]) << 128 | int(a[i, 3]) << 192 for i in range(a.shape[0])]


EDGE_LIMBS = to_limbs(EDGE)
_P_LIMBS = to_limbs([P])[0]


def below_p(arr):
    """(..., 4) uint64 -> bool (...,): the element is < p (limb-wise compare, most significant first)"""
    a = np.asarray(arr, dtype=np.uint64)
    lt = np.zeros(a.shape[:-1], dtype=bool)
    eq = np.ones(a.shape[:-1], dtype=bool)
    for k in (3, 2, 1, 0):
        lt |= eq & (a[..., k] < _P_LIMBS[k])
        eq &= a[..., k] == _P_LIMBS[k]
    return lt


def uniform_column(n, rng):
    """(n, 4) uint64 uniform on [0, p): 252-bit draws, the ones >= p drawn again (rejection, not masking)"""
    out = np.empty((n, 4), dtype=np.uint64)
    todo = np.arange(n)
    while todo.size:
        v = rng.integers(0, 1 << 64, size=(todo.size, 4), dtype=np.uint64, endpoint=False)
        v[:, 3] &= np.uint64((1 << 60) - 1)
        ok = below_p(v)
        out[todo[ok]] = v[ok]
        todo = todo[~ok]
    return out


def edge_column(n, seed=0):
    """(n, 4) uint64 of stored values < p: uniform draws from the whole of [0, p) with edge values mixed in - the EDGE list in order
    (rotated by the seed), a run of p - 1, the alternations 0 / p - 1 and 1 / p - 2, and edge values at about half of the other
    positions, chosen at random, so that an edge value meets every partner position of a butterfly, a fold row and a column"""
    rng = np.random.default_rng(0xED6E0000 + seed)
    out = uniform_column(n, rng)
    scattered = rng.random(n) < 0.5
    out[scattered] = EDGE_LIMBS[rng.integers(0, len(EDGE), size=int(scattered.sum()))]
    ne = len(EDGE)
    head = min(n, ne)
    out[:head] = EDGE_LIMBS[(np.arange(head) + seed) % ne]
    if n >= 8 * ne:
        q = n // 4
        pm1, zero, one, pm2 = (to_limbs([v])[0] for v in (P - 1, 0, 1, P - 2))
        run = slice(q, q + ne)
        out[run] = pm1
        alt = np.arange(2 * q, 2 * q + 2 * ne)
        out[alt[0::2]], out[alt[1::2]] = zero, pm1
        alt = np.arange(3 * q, 3 * q + 2 * ne)
        out[alt[0::2]], out[alt[1::2]] = one, pm2
    assert below_p(out).all()
    return out


def assert_canonical(arr, what):
    """every element of (..., 4) uint64 is < p; names the first (flattened) index that is not"""
    ok = below_p(arr).reshape(-1)
    if not ok.all():
        i = int(np.argmin(ok))
        v = from_limbs(np.asarray(arr).reshape(-1, 4)[i])[0]
        raise AssertionError("%s: element %d is not below p: %#x (p + %d)" % (what, i, v, v - P))


def solve_cell(ref, inputs, cell_index, targets):
    """inputs: list of (n, 4) stored columns; ref(inputs) -> (m, 4) stored outputs, output j AFFINE in the input cell
    cell_index[j] = (column, row) (over the field of stored values: Montgomery images are p-linear in what they stand for) and
    independent of the other outputs' cells.  Runs ref with all those cells 0, then 1, and returns a copy of the inputs in which
    each cell holds the value that makes output j equal targets[j] (python ints, mod p).  Outputs whose slope is 0 keep the cell."""
    cells = [tuple(c) for c in cell_index]
    assert len(set(cells)) == len(cells), "one cell per output"
    trial = [np.array(c, dtype=np.uint64, copy=True) for c in inputs]

    def run(v):
        for c, r in cells:
            trial[c][r] = to_limbs([v])[0]
        return from_limbs(ref(trial))
    y0, y1 = run(0), run(1)
    tgt = from_limbs(targets)
    out = [np.array(c, dtype=np.uint64, copy=True) for c in inputs]
    solved = 0
    for j, (c, r) in enumerate(cells):
        slope = (y1[j] - y0[j]) % P
        if slope:
            out[c][r] = to_limbs([(tgt[j] - y0[j]) * pow(slope, -1, P) % P])[0]
            solved += 1
    assert solved >= len(cells) * 3 // 4, "most outputs must depend on their cell"
    return out
