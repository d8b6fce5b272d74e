"""The C oracle at the top of the field: its transforms, FRI folds and polynomial evaluation on edge columns (tests/edge_values.py:
values in [2^251, p), p - 1, the Montgomery images of +-1 ...) against the big-integer restatements of tests/pyref.py.  The oracle
judges the kernels on these columns in tests/test_gpu_edge_values.py, so it has to be right there first.  CPU only."""
import numpy as np
import pytest

from tests import pyref
from tests.edge_values import EDGE, P, assert_canonical, edge_column, from_limbs, solve_cell, to_limbs, uniform_column


def _plain(oracle, col):
    return [int(v) for v in oracle.from_mont(col)]


def _stored(oracle, vals):
    return oracle.to_mont(list(vals))


def test_edge_list_and_columns():
    """the edge list holds what it promises, and edge_column draws from the whole of [0, p)"""
    for v in (0, 1, 2, P - 1, P - 2, P - 3, 2**251 - 1, 2**251, 2**251 + 1, 2**251 + 2**192, (P - 1) // 2, (P + 1) // 2,
              2**192 - 1, 2**224 - 1, pow(2, 256, P), P - pow(2, 256, P), pow(2, 280, P), P - pow(2, 280, P)):
        assert v in EDGE, hex(v)
    assert sum(2**251 <= v < P for v in EDGE) >= 8
    col = edge_column(1 << 12, 3)
    assert_canonical(col, "edge_column")
    vals = from_limbs(col)
    assert sum(v >= 2**251 for v in vals) > 300 and P - 1 in vals and 0 in vals
    top = from_limbs(uniform_column(1 << 12, np.random.default_rng(1)))
    assert max(top) < P and sum(v >= 2**250 for v in top) > 1500           # not masked: half of [0, p) is above 2^250
    with pytest.raises(AssertionError, match="element 5"):
        bad = col.copy()
        bad[5] = to_limbs([P])[0]
        assert_canonical(bad, "x")


def test_solve_cell_forces_outputs():
    """an affine reference: the solved cells give the targets"""
    a, b = 12345, P - 7

    def ref(cols):
        return to_limbs([(a * x + b * y) % P for x, y in zip(from_limbs(cols[0]), from_limbs(cols[1]))])
    x, y = edge_column(64, 1), edge_column(64, 2)
    t = edge_column(64, 3)
    x2, y2 = solve_cell(ref, [x, y], [(0, i) for i in range(64)], t)
    assert np.array_equal(ref([x2, y2]), t) and np.array_equal(y2, y)


@pytest.mark.parametrize("log_n", [1, 2, 3, 5, 8, 10])
@pytest.mark.parametrize("coset", [False, True])
def test_oracle_ntt_on_edge_columns(oracle, log_n, coset):
    n = 1 << log_n
    off = 3 if coset else 1
    off_m = oracle.to_mont([off])[0] if coset else None
    for seed in range(2):
        col = edge_column(n, seed + log_n)
        got = oracle.ntt(col, offset=off_m)
        assert_canonical(got, "oracle ntt")
        assert _plain(oracle, got) == pyref.ntt(_plain(oracle, col), off), (log_n, seed)
        back = oracle.ntt(col, inverse=True, offset=off_m)
        assert_canonical(back, "oracle intt")
        assert _plain(oracle, back) == pyref.intt(_plain(oracle, col), off), (log_n, seed)
        # a forced edge output: the forward transform of the reference inverse of an edge column
        x = _stored(oracle, pyref.intt(_plain(oracle, col), off))
        assert np.array_equal(oracle.ntt(x, offset=off_m), col)


@pytest.mark.parametrize("fold", [2, 4, 8, 16])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_oracle_fri_fold_on_edge_columns(oracle, fold, flags):
    log_len = 6
    ev = edge_column(1 << log_len, fold + 7 * flags)
    for alpha in (0, 1, P - 1, 2**251, 0xABCDEF ** 5 % P):
        am, off = oracle.to_mont([alpha])[0], 3
        got = oracle.fri_fold(ev, fold, am, oracle.to_mont([off])[0], flags)
        assert_canonical(got, "oracle fold")
        want = pyref.fri_fold(_plain(oracle, ev), fold, alpha, off, bool(flags & 1), bool(flags & 2))
        assert _plain(oracle, got) == want, (fold, flags, alpha)


@pytest.mark.parametrize("log_n", [0, 1, 4, 10])
def test_oracle_poly_eval_on_edge_columns(oracle, log_n):
    co = edge_column(1 << log_n, 40 + log_n)
    cp = _plain(oracle, co)
    for x in [0, 1, P - 1, 2**251, P - 2] + EDGE[-6:]:
        got = oracle.poly_eval(co, oracle.to_mont([x])[0])
        assert_canonical(got, "oracle poly_eval")
        assert int(oracle.from_mont(got)) == pyref.horner(cp, x), (log_n, hex(x))


def test_oracle_lde_on_edge_columns(oracle):
    """or_lde: the coefficients are pyref's inverse over the trace domain, the evaluations its forward transform on the coset"""
    log_n, lb = 6, 2
    col = edge_column(1 << log_n, 9)
    ev, co = oracle.lde(col, lb, oracle.to_mont([3])[0])
    c = pyref.intt(_plain(oracle, col))
    assert _plain(oracle, co) == c
    assert _plain(oracle, ev) == pyref.ntt(c + [0] * ((1 << (log_n + lb)) - len(c)), 3)
