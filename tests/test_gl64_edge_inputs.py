"""CPU: the inputs of tests/test_gpu_gl64_edge_values.py do reach the rare branches of csrc/gl64.h, and the oracle those tests compare
with is right where they look.

The census runs tests/gl64_edge_values.py's Python-integer model of the header's word arithmetic over adjacent pairs of edge columns:
the borrow of gl_reduce128_lazy, a product landing in [p, 2^64) and a sum landing in [p, 2^64) each occur in at least 1 % of the
pairs (the half-mixed column measures 2 - 3 %; the bound leaves room for another seed's draw), and never on uniform pairs.  The pinning holds
oracle/goldilocks.c's gl_* / gl3_* functions to Python integers written from the definitions, on edge columns and on outputs forced
onto residues below 2^32 - 1, at n <= 2^5 - tests/test_goldilocks.py pins them on uniform data only."""
import numpy as np
import pytest

from oracle.gl_cpu_context import add3, inv3, mul3, scale3, sub3
from tests import gl64_edge_values as ge
from tests.gl64_edge_values import EDGE, EPS, P, edge_column, force3, small_targets

OFFSET = 7
RARE = ("reduce_borrow", "product_above_p", "sum_above_p")


def _census(pairs):
    seen = dict.fromkeys(RARE, 0)
    for a, b in pairs:
        prod, br = ge.gl_mul(a, b)
        s, bs = ge.gl_add(a, b)
        assert prod == a * b % P and s == (a + b) % P, (a, b)
        d, _ = ge.gl_sub_lazy(a, b)
        assert d % P == (a - b) % P
        for name in RARE:
            seen[name] += name in br or name in bs
    return seen


def test_edge_columns_reach_the_rare_branches():
    for seed in range(3):
        col = [int(v) for v in edge_column(4096, seed)]
        seen = _census(zip(col, col[1:]))
        for name in RARE:
            assert seen[name] >= 0.01 * (len(col) - 1), (seed, seen)
    rng = np.random.default_rng(3)
    col = [int(v) for v in rng.integers(0, P, size=4096, dtype=np.uint64)]
    assert _census(zip(col, col[1:])) == dict.fromkeys(RARE, 0)


def test_the_model_is_the_arithmetic_on_every_pair_of_edge_words():
    """every pair of EDGE words and of their second words (r + p where r < 2^32 - 1): the model's products, sums and wide sums are
    Python's, and its assertions (the bounds the header's comments claim) hold"""
    lazy = EDGE + [v + P for v in EDGE if v < EPS] + [2**64 - 1]
    for a in lazy:
        for b in lazy:
            r, _ = ge.gl_reduce128_lazy(*ge.gl_mul_wide(a, b))
            assert r < 2**64 and r % P == a * b % P
            if b < P:
                s, _ = ge.gl_sub_lazy(a, b)
                assert s < 2**64 and s % P == (a - b) % P
            if a < P and b < P:
                assert ge.gl_add(a, b)[0] == (a + b) % P
    # a wide accumulator of all the products of one word with the list: four digit sums, one reduction
    for a in lazy:
        l0 = l1 = h0 = h1 = 0
        for b in lazy:
            lo, hi = ge.gl_mul_wide(a, b)
            l0, l1, h0, h1 = l0 + (lo & EPS), l1 + (lo >> 32), h0 + (hi & EPS), h1 + (hi >> 32)
        assert ge.glw_reduce(l0, l1, h0, h1)[0] == a * sum(lazy) % P


def test_edge_helpers():
    assert all(0 <= v < P for v in EDGE) and len(set(EDGE)) == len(EDGE) >= 23
    c = edge_column(1024, 2)
    assert [int(v) for v in c[:len(EDGE)]] == [EDGE[(i + 2) % len(EDGE)] for i in range(len(EDGE))]
    assert (c[256:256 + len(EDGE)] == P - 1).all() and [int(v) for v in c[512:516]] == [0, P - 1, 0, P - 1] and [int(v) for v in c[768:772]] == [1, P - 2, 1, P - 2]
    assert 0.4 < np.isin(c, np.array(EDGE, dtype=np.uint64)).mean() < 0.75
    t = small_targets((64, 3), 1)
    assert (t < EPS).all() and (t == 0).any() and (t == EPS - 1).any()
    ge.assert_canonical(c, "an edge column")
    with pytest.raises(AssertionError, match="non-canonical words stored: 2, first at 3"):
        ge.assert_canonical(np.array([0, 1, P - 1, P, 5, 2**64 - 1], dtype=np.uint64), "x")
    assert ge.solve3([[1, 2, 3], [0, 1, 4], [5, 6, 0]], [14, 14, 17]) == [1, 2, 3] and ge.solve3([[1, 2, 3], [2, 4, 6], [0, 0, 1]], [1, 2, 3]) is None


# ---- the oracle at the edges -----------------------------------------------------------------------------------------------------
def _root(log_n):
    return pow(7, (P - 1) >> log_n, P)


def ntt_definition(a, off):
    n = len(a)
    w = _root(n.bit_length() - 1)
    return [sum(int(a[i]) * pow(off * pow(w, k, P), i, P) for i in range(n)) % P for k in range(n)]


def _ints(a):
    return [[int(v) for v in row] for row in a] if np.asarray(a).ndim == 2 else [int(v) for v in a]


@pytest.mark.parametrize("log_n", [1, 2, 5])
def test_oracle_transforms_at_the_edges(oracle, log_n):
    n = 1 << log_n
    for off in (1, OFFSET):
        x, y = edge_column(n, log_n), small_targets(n, log_n + off)
        if n >= 16:
            y[4:8], y[8:12] = 0, EPS - 1
        assert _ints(oracle.gl_ntt(x, offset=off)) == ntt_definition(x, off)
        for v in (x, y):                                    # the inverse is the vector the definition maps back (forced outputs: y)
            back = oracle.gl_ntt(v, inverse=True, offset=off)
            assert (back < np.uint64(P)).all() and ntt_definition(back, off) == _ints(v)
    for lb in (0, 1, 2):                                    # blowup 1, 2 and 4
        ev, co = oracle.gl_lde(x, lb, OFFSET)
        assert ntt_definition(co, 1) == _ints(x)
        W = _root(log_n + lb)
        assert _ints(ev) == [sum(int(co[i]) * pow(OFFSET * pow(W, k, P), i, P) for i in range(n)) % P for k in range(n << lb)]


def fold_definition(evals, fold, alpha, off, unnormalised):
    """row j: the polynomial of degree < fold through (x_j w_fold^m, evals[j + m rows]), evaluated at alpha - times fold when unnormalised"""
    L = len(evals)
    rows = L // fold
    wL = _root(L.bit_length() - 1)
    wf = pow(wL, rows, P)
    alpha = tuple(int(v) for v in alpha)
    out = []
    for j in range(rows):
        x = off * pow(wL, j, P) % P
        pts = [x * pow(wf, m, P) % P for m in range(fold)]
        vals = [tuple(int(v) for v in evals[j + m * rows]) for m in range(fold)]
        # coefficient t of the interpolant: (1 / fold) sum_m v_m (x w^m)^-t, checked by evaluating it back at the points
        coef = [scale3(tuple(sum(vals[m][c] * pow(pts[m], -t, P) for m in range(fold)) % P for c in range(3)), pow(fold, -1, P)) for t in range(fold)]
        for m in range(fold):
            assert tuple(sum(coef[t][c] * pow(pts[m], t, P) for t in range(fold)) % P for c in range(3)) == tuple(v % P for v in vals[m])
        acc = (0, 0, 0)
        for t in reversed(range(fold)):
            acc = add3(mul3(acc, alpha), coef[t])
        out.append(list(scale3(acc, fold) if unnormalised else acc))
    return out


@pytest.mark.parametrize("fold", [2, 4, 8, 16])
@pytest.mark.parametrize("unnormalised", [False, True])
def test_oracle_fri_fold_at_the_edges(oracle, fold, unnormalised):
    from tests.test_gpu_gl64_edge_values import fold_alphas, fold_cells
    L = 32
    rows = L // fold
    evals = np.stack([edge_column(L, fold + c) for c in range(3)], axis=1)
    targets = small_targets((rows, 3), fold)
    for alpha in fold_alphas(fold):
        ref = lambda arrs: oracle.gl3_fri_fold(arrs[0], fold, alpha, OFFSET, unnormalised)
        assert _ints(ref([evals])) == fold_definition(evals, fold, alpha, OFFSET, unnormalised)
        forced = force3(ref, [evals], fold_cells(rows), targets)[0]
        assert fold_definition(forced, fold, alpha, OFFSET, unnormalised) == _ints(targets)


def test_oracle_inverse_at_the_edges(oracle):
    assert _ints(oracle.gl3_inv(np.zeros(3, dtype=np.uint64))) == [0, 0, 0]
    cases = [(v, 0, 0) for v in EDGE[1:]] + [(0, v, 0) for v in EDGE[1:8]] + [(0, 0, v) for v in EDGE[1:8]]
    cases += [(EDGE[i], EDGE[(i + 5) % len(EDGE)], EDGE[(2 * i + 1) % len(EDGE)]) for i in range(len(EDGE))]
    for a in cases:
        if not any(a):
            continue
        got = tuple(int(v) for v in oracle.gl3_inv(np.array(a, dtype=np.uint64)))
        assert all(v < P for v in got) and mul3(a, got) == (1, 0, 0) and got == inv3(a), a


def ood_definition(coeffs, mc, mo, z):
    n = len(coeffs[0])
    w = _root(n.bit_length() - 1)
    out = []
    for c, o in zip(mc, mo):
        pt = scale3(tuple(int(v) for v in z), pow(w, o % n, P))
        acc, pw = (0, 0, 0), (1, 0, 0)
        for k in range(n):
            acc, pw = add3(acc, scale3(pw, int(coeffs[c][k]))), mul3(pw, pt)
        out.append(list(acc))
    return out


def deep_definition(trace, comp, log_n, lb, mc, mo, ood_t, ct, ood_c, cc, z, zc):
    """out[i] = sum_j ct_j (T_cj[i] - ood_t_j) / (x_i - z w_n^oj) + sum_k cc_k (H_k[i] - ood_c_k) / (x_i - zc), x_i = OFFSET w_N^i"""
    n, N = 1 << log_n, (1 << log_n) << lb
    wn, wN = _root(log_n), _root(log_n + lb)
    t3 = lambda v: tuple(int(u) for u in v)
    out = []
    for i in range(N):
        x, acc = OFFSET * pow(wN, i, P) % P, (0, 0, 0)
        for j, (c, o) in enumerate(zip(mc, mo)):
            den = sub3((x, 0, 0), scale3(t3(z), pow(wn, o % n, P)))
            acc = add3(acc, mul3(mul3(t3(ct[j]), sub3((int(trace[c][i]), 0, 0), t3(ood_t[j]))), inv3(den)))
        for k in range(len(comp)):
            acc = add3(acc, mul3(mul3(t3(cc[k]), sub3((int(comp[k][i]), 0, 0), t3(ood_c[k]))), inv3(sub3((x, 0, 0), t3(zc)))))
        out.append(list(acc))
    return out


@pytest.mark.parametrize("log_n", [3, 5])
def test_oracle_ood_and_deep_at_the_edges(oracle, log_n):
    from tests.test_gpu_gl64_edge_values import deep_case, edge3, ood_points
    n, lb = 1 << log_n, 1
    N = n << lb
    coeffs = [edge_column(n, 60 + c + log_n) for c in range(3)]
    mc, mo = [0, 0, 1, 1, 2, 2, 2], [0, 1, 1, n - 1, 5 % n, 2, n + 3]
    for z in ood_points(log_n):
        assert _ints(oracle.gl3_ood_eval(coeffs, mc, mo, z)) == ood_definition(coeffs, mc, mo, z)
    z = ood_points(log_n)[0]
    fc, fo = [0, 1, 2], [1, n - 1, 2]
    targets = small_targets((3, 3), log_n)
    forced = force3(lambda cs: oracle.gl3_ood_eval(cs, fc, fo, z), coeffs, [tuple((c, (c + 3 * t) % n) for t in range(3)) for c in range(3)], targets)
    assert ood_definition(forced, fc, fo, z) == _ints(targets)
    # DEEP: honest values on columns whose sub-coset rows are edge words, then outputs forced through three same-row cells
    for ncomp in (0, 2):
        lde, co, comp_lde, comp_co, mc, mo, ct, cc = deep_case(oracle, log_n, lb, ncomp, 100 * log_n + ncomp)
        z, zc = edge3(1), edge3(2)
        ood_t = oracle.gl3_ood_eval(co, mc, mo, z)
        ood_c = oracle.gl3_ood_eval(comp_co, list(range(ncomp)), [0] * ncomp, zc) if ncomp else np.zeros((0, 3), dtype=np.uint64)
        ref = lambda cols: oracle.gl3_deep_compose(cols, comp_lde, log_n, lb, OFFSET, mc, mo, ood_t, ct, ood_c, cc, z, zc)
        assert _ints(ref(lde)) == deep_definition(lde, comp_lde, log_n, lb, mc, mo, ood_t, ct, ood_c, cc, z, zc)
        targets = small_targets((N, 3), log_n + ncomp)
        raw = [edge_column(N, 20 + c) for c in range(3)]
        forced = force3(ref, raw, [tuple((c, i) for c in range(3)) for i in range(N)], targets)
        assert deep_definition(forced, comp_lde, log_n, lb, mc, mo, ood_t, ct, ood_c, cc, z, zc) == _ints(targets)


def test_oracle_program_at_the_edges(oracle):
    from tests.test_goldilocks import _py_program
    from tests.test_gpu_gl64_edge_values import edge_program, forcing_program
    log_n, lb = 4, 1
    N = 2 << log_n
    code, consts, n_slots = edge_program(1, 30, 3)
    lde = [edge_column(N, 200 + c) for c in range(3)]
    lde[0][1::3] = 0
    tables, desc = np.concatenate([edge_column(4, 210), edge_column(8, 220)]), [0, 2, 4, 3]
    got = oracle.gl3_eval_program(code, consts, n_slots, tables, desc, lde, log_n, lb, OFFSET)
    want = _py_program(code, consts, n_slots, tables, desc, lde, log_n + lb, lb, OFFSET, range(N))
    assert _ints(got) == [want[i] for i in range(N)] and got.any()
    prog = forcing_program()
    code, consts = np.array(prog.code, dtype=np.uint32), np.array(prog.consts, dtype=np.uint64).reshape(-1, 3)
    lde = [edge_column(N, 230 + c) for c in range(5)]
    targets = small_targets((N, 3), 240)
    forced = force3(lambda cols: oracle.gl3_eval_program(code, consts, prog.n_slots, None, [], cols, log_n, lb, OFFSET), lde,
                    [tuple((c, i) for c in range(3)) for i in range(N)], targets)
    want = _py_program(code, consts, prog.n_slots, [], [], forced, log_n + lb, lb, OFFSET, range(N))
    assert [want[i] for i in range(N)] == _ints(targets)
