"""The 64-bit field's kernels on edge words and on forced outputs (the 252-bit counterpart is tests/test_gpu_edge_values.py).

csrc/gl64.h keeps values as lazy words, and only a residue below 2^32 - 1 has a second word: a lazy word passed where a canonical one
is promised, stored to HBM, hashed or compared shows on one uniform draw in 2^32 - never in tests/test_goldilocks.py, whose inputs
are uniform.  Here the inputs are tests/gl64_edge_values.py's columns (the words at both ends of the field and at its 32-bit seams
among draws from the whole of [0, p)) and, wherever a kernel's output can be steered, the outputs are FORCED onto residues below
2^32 - 1: by the oracle's inverse where the map is linear in a whole column, by solving a 3 x 3 system over Fp per output where an
Fq3 output is affine in three input cells (force3).  A kernel that leaves out the last canonicalisation then stores p + r.

Every test checks that each downloaded word is canonical (< p), then compares bit for bit with the oracle, which
tests/test_gl64_edge_inputs.py holds to Python integers on the same kinds of input.  The sizes are the smallest at which each path
of the kernels exists; the file also runs on the host build of the device code (tests/test_device_code_on_host.py)."""
import copy
import os
import re

import numpy as np
import pytest

from tests.gl64_edge_values import EDGE, EPS, P, assert_canonical, edge_column, force3, small_targets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSET = 7


@pytest.fixture(scope="module")
def ctx():
    from sandstorm_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def be():
    from sandstorm_amd import backend
    return backend


def _check(got, want, what):
    assert_canonical(got, what)
    want = np.asarray(want, dtype=np.uint64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).reshape(-1))[0]
        raise AssertionError("%s: %d of %d words differ, first at %d: %#x != %#x" % (what, len(bad), got.size, bad[0], int(got.reshape(-1)[bad[0]]),
                                                                                   int(want.reshape(-1)[bad[0]])))


def _brev(log_n):
    return np.array([int(format(i, "0%db" % log_n)[::-1], 2) if log_n else 0 for i in range(1 << log_n)], dtype=np.int64)


def edge3(seed):
    """an element of Fq3 whose coordinates are EDGE words (non-zero upper coordinates)"""
    ne = len(EDGE)
    return np.array([EDGE[(5 * seed + 4) % ne], EDGE[(7 * seed + 5) % ne] or 1, EDGE[(11 * seed + 6) % ne] or P - 1], dtype=np.uint64)


def forced_column(n, seed):
    """the wanted output column of a transform: residues below 2^32 - 1, with a run of 0 and a run of 2^32 - 2"""
    y = small_targets(n, seed)
    if n >= 16:
        y[n // 4:n // 4 + n // 8] = 0
        y[n // 2:n // 2 + n // 8] = EPS - 1
    return y


# ----------------------------------------------------------------------------- transforms
@pytest.mark.parametrize("log_n", [1, 2, 5, 13, 14])        # one register group ... one full 2^13 tile, two passes
def test_ntt_on_edge_words_and_forced_outputs(ctx, be, oracle, log_n):
    n = 1 << log_n
    x = edge_column(n, log_n)
    for off in (1, OFFSET):
        y = forced_column(n, 10 * log_n + off)
        x_y = oracle.gl_ntt(y, inverse=True, offset=off)    # forward(x_y) = y
        y_x = oracle.gl_ntt(y, offset=off)                  # inverse(y_x) = y
        srcs, wants = (x, x_y), (oracle.gl_ntt(x, offset=off), y)
        d = [ctx.column(s) for s in srcs]
        ctx.ntt_gl64(d, log_n, be.FORWARD, off)
        for k, (dc, w) in enumerate(zip(d, wants)):
            _check(dc.download(np.uint64, (n,)), w, "forward 2^%d offset %d column %d" % (log_n, off, k))
        srcs, wants = (x, y_x, y), (oracle.gl_ntt(x, inverse=True, offset=off), y, x_y)
        d = [ctx.column(s) for s in srcs]
        ctx.ntt_gl64(d, log_n, be.INVERSE, off)
        for k, (dc, w) in enumerate(zip(d, wants)):
            _check(dc.download(np.uint64, (n,)), w, "inverse 2^%d offset %d column %d" % (log_n, off, k))
    # the bit-reversed orders, once each: inverse to bit-reversed output, forward from bit-reversed input, forward to bit-reversed output
    br = _brev(log_n)
    d = [ctx.column(y_x), ctx.column(x)]
    ctx.ntt_gl64(d, log_n, be.INVERSE, OFFSET, be.NATURAL, be.BITREV)
    _check(d[0].download(np.uint64, (n,)), y[br], "inverse, bit-reversed out, forced")
    _check(d[1].download(np.uint64, (n,)), oracle.gl_ntt(x, inverse=True, offset=OFFSET)[br], "inverse, bit-reversed out")
    d = [ctx.column(np.ascontiguousarray(x_y[br])), ctx.column(np.ascontiguousarray(x[br]))]
    ctx.ntt_gl64(d, log_n, be.FORWARD, OFFSET, be.BITREV, be.NATURAL)
    _check(d[0].download(np.uint64, (n,)), y, "forward, bit-reversed in, forced")
    _check(d[1].download(np.uint64, (n,)), oracle.gl_ntt(x, offset=OFFSET), "forward, bit-reversed in")
    d = [ctx.column(x_y)]
    ctx.ntt_gl64(d, log_n, be.FORWARD, OFFSET, be.NATURAL, be.BITREV)
    _check(d[0].download(np.uint64, (n,)), y[br], "forward, bit-reversed out, forced")


@pytest.mark.parametrize("log_n,lb", [(3, 1), (12, 1), (12, 2), (13, 1)])
def test_lde_on_edge_words(ctx, oracle, log_n, lb):
    """both outputs of ss_lde_gl64 (evaluations, bit-reversed coefficients) of edge columns, and of a column whose coefficients are forced"""
    n, N = 1 << log_n, (1 << log_n) << lb
    small = forced_column(n, 50 + log_n + lb)
    cols = [edge_column(n, 20 + log_n), edge_column(n, 30 + log_n + lb), oracle.gl_ntt(small, offset=1)]
    ev, co = [ctx.alloc(8 * N) for _ in cols], [ctx.alloc(8 * n) for _ in cols]
    ctx.lde_gl64([ctx.column(c) for c in cols], log_n, lb, OFFSET, ev, co)
    br = _brev(log_n)
    for k, c in enumerate(cols):
        want_ev, want_co = oracle.gl_lde(c, lb, OFFSET)
        _check(ev[k].download(np.uint64, (N,)), want_ev, "lde evaluations, column %d" % k)
        _check(co[k].download(np.uint64, (n,)), want_co[br], "lde coefficients, column %d" % k)
    assert np.array_equal(oracle.gl_lde(cols[2], lb, OFFSET)[1], small)


# ----------------------------------------------------------------------------- FRI fold
def fold_alphas(seed):
    return [np.array([1, 0, 0], dtype=np.uint64), np.array([0, 0, P - 1], dtype=np.uint64), edge3(seed)]


def fold_cells(rows):
    """output row j of a fold through the three coordinates of evals[j]"""
    return [tuple((0, (j, c)) for c in range(3)) for j in range(rows)]


@pytest.mark.parametrize("fold", [2, 4, 8, 16])
@pytest.mark.parametrize("unnormalised", [False, True])
@pytest.mark.parametrize("row_bits", [4, 9])               # 2^9 rows: more than one 256-lane block
def test_fri_fold_on_edge_words_and_forced_outputs(ctx, be, oracle, fold, unnormalised, row_bits):
    log_len = row_bits + fold.bit_length() - 1
    L, rows = 1 << log_len, 1 << row_bits
    flags = be.FRI_UNNORMALISED if unnormalised else 0
    evals = np.stack([edge_column(L, 3 * fold + c + 40 * row_bits + unnormalised) for c in range(3)], axis=1)
    targets = small_targets((rows, 3), fold + row_bits + unnormalised)
    out = ctx.alloc(24 * rows)
    for k, alpha in enumerate(fold_alphas(fold + row_bits)):
        ref = lambda arrs: oracle.gl3_fri_fold(arrs[0], fold, alpha, OFFSET, unnormalised)
        forced = force3(ref, [evals], fold_cells(rows), targets)[0]
        for src, want, name in ((evals, ref([evals]), "edge"), (forced, targets, "forced")):
            ctx.fri_fold_gl64x3(ctx.column(src), log_len, fold, alpha, OFFSET, out, flags)
            _check(out.download(np.uint64, (rows, 3)), want, "fold %d, flags %d, alpha %d, %s" % (fold, flags, k, name))


# ----------------------------------------------------------------------------- out-of-domain evaluation
def ood_points(seed):
    """z with edge coordinates; z with zero upper coordinates; z = (p - 1, p - 1, p - 1)"""
    return [edge3(seed), np.array([EDGE[(seed + 9) % len(EDGE)] or 5, 0, 0], dtype=np.uint64), np.array([P - 1] * 3, dtype=np.uint64)]


@pytest.mark.parametrize("log_n", [3, 7, 12])              # the power kernel's 64-entry table: below, at (2 groups) and above 2^6 groups
def test_ood_eval_on_edge_words_and_forced_outputs(ctx, oracle, log_n):
    n = 1 << log_n
    coeffs = [edge_column(n, 60 + c + log_n) for c in range(3)]
    br = _brev(log_n)
    up = lambda cs: [ctx.column(np.ascontiguousarray(c[br])) for c in cs]
    at_z = ([0, 1, 2], [0, 0, 0])                          # columns read at z only: the dot-product path
    shifted = ([0, 0, 1, 1, 2, 2, 2], [0, 1, 1, n - 1, 5 % n, 2, n + 3])     # several offsets per column (one wrapped): three transforms
    d = up(coeffs)
    for k, z in enumerate(ood_points(log_n)):
        for (mc, mo), path in ((at_z, "dot"), (shifted, "transform")):
            _check(ctx.ood_eval_gl64x3(d, log_n, mc, mo, z), oracle.gl3_ood_eval(coeffs, mc, mo, z), "ood 2^%d, z %d, %s path" % (log_n, k, path))
            if k:
                continue                                   # (a base-field z makes the three cells' system singular: forced with z 0 only)
            # one mask cell per column forced onto small residues through three coefficient cells of that column
            fc, fo = ([0, 1, 2], [0, 0, 0]) if path == "dot" else ([0, 1, 2], [1, n - 1, 2])
            cells = [tuple((c, (7 * c + 3 * t + 1) % n if n > 8 else (c + 3 * t) % n) for t in range(3)) for c in range(3)]
            targets = small_targets((3, 3), log_n + len(path))
            forced = force3(lambda cs: oracle.gl3_ood_eval(cs, fc, fo, z), coeffs, cells, targets)
            got = ctx.ood_eval_gl64x3(up(forced), log_n, mc, mo, z)
            _check(got, oracle.gl3_ood_eval(forced, mc, mo, z), "ood 2^%d, forced, %s path" % (log_n, path))
            rows = [j for j, (c, o) in enumerate(zip(mc, mo)) if (c, o) in set(zip(fc, fo))]
            assert len(rows) == 3 and np.array_equal(got[rows], targets)


@pytest.mark.parametrize("log_n", [3, 7, 12])
def test_ood_dot_product_whose_partial_sums_have_two_words(ctx, oracle, log_n):
    """gl3_dot_kernel adds its lanes' values in a tree, and a sum is an operand of the next level: at z = 1 a lane's value is its
    coefficient, so the two pairs that meet first are made to sum to p + 2^32 - 2 as integers (the residue 2^32 - 2, whose second
    word a lazy addition would leave) and meet each other one level later - two such words overflow a lazy addition"""
    n = 1 << log_n
    m = min(n, 256) // 2                                   # the first level at which two non-zero lanes meet: lanes t and t + m
    col = np.zeros(n, dtype=np.uint64)
    col[[0, m // 2]], col[[m, m // 2 + m]] = P - 1, EPS
    cols = [col, edge_column(n, 70 + log_n)]
    cols[1][[0, m // 2, m, m // 2 + m]] = col[[0, m // 2, m, m // 2 + m]]
    br = _brev(log_n)                                      # the device's arrays are bit-reversed: lane q holds coefficient bitrev(q)
    nat = [np.ascontiguousarray(c[br]) for c in cols]
    for z in ([P - 1, 0, 0], [1, 0, 0]):
        got = ctx.ood_eval_gl64x3([ctx.column(c) for c in cols], log_n, [0, 1], [0, 0], z)
        _check(got, oracle.gl3_ood_eval(nat, [0, 1], [0, 0], z), "dot product at z = %d" % z[0])
    assert [int(v) for v in got[0]] == [2 * (P - 1 + EPS) % P, 0, 0]


# ----------------------------------------------------------------------------- DEEP
def _on_coset(values, lb, oracle):
    """(coefficients, evaluations over OFFSET <w_N>) of the polynomial of degree < n whose values on the sub-coset OFFSET <w_n> - the
    only rows of an LDE column that the DEEP kernel reads - are `values`"""
    n = len(values)
    co = oracle.gl_ntt(values, inverse=True, offset=OFFSET)
    return co, oracle.gl_ntt(np.concatenate([co, np.zeros((n << lb) - n, dtype=np.uint64)]), offset=OFFSET)


def deep_case(oracle, log_n, lb, ncomp, seed):
    n = 1 << log_n
    ncols = 3
    coeffs, lde = zip(*[_on_coset(edge_column(n, seed + c), lb, oracle) for c in range(ncols)])
    comp_coeffs, comp_lde = zip(*[_on_coset(edge_column(n, seed + 10 + k), lb, oracle) for k in range(ncomp)]) if ncomp else ((), ())
    offsets = [0, 1, n - 1, n + 2]                         # n + 2 wraps to 2
    mask = [(c, o) for c in range(ncols) for o in offsets if (c + o) % 4 != 1]
    mc, mo = [c for c, _ in mask], [o for _, o in mask]
    ct = np.stack([edge3(seed + j) for j in range(len(mask))])
    cc = np.stack([edge3(seed + 50 + k) for k in range(ncomp)]) if ncomp else np.zeros((0, 3), dtype=np.uint64)
    return list(lde), list(coeffs), list(comp_lde), list(comp_coeffs), mc, mo, ct, cc


@pytest.mark.parametrize("log_n,lb", [(3, 1), (9, 1), (9, 2)])
@pytest.mark.parametrize("ncomp", [0, 2])
def test_deep_compose_on_edge_words_and_forced_outputs(ctx, oracle, log_n, lb, ncomp):
    n, N, step = 1 << log_n, (1 << log_n) << lb, 1 << lb
    seed = 100 * log_n + 10 * lb + ncomp
    lde, coeffs, comp_lde, comp_coeffs, mc, mo, ct, cc = deep_case(oracle, log_n, lb, ncomp, seed)
    assert np.array_equal(lde[0][::step], edge_column(n, seed))          # what the kernel reads of a column are edge words
    out = ctx.alloc(24 * N)
    zero3 = np.zeros((0, 3), dtype=np.uint64)

    def run(trace, comp, ood_t, ood_c, z, zc):
        ctx.deep_compose_gl64x3([ctx.column(c) for c in trace], [ctx.column(c) for c in comp], log_n, lb, OFFSET, mc, mo, ood_t, ct, ood_c, cc, z, zc, out)
        return out.download(np.uint64, (N, 3))
    # (a) honest out-of-domain values: the whole domain
    z, zc = edge3(seed + 1), edge3(seed + 2)
    ood_t = oracle.gl3_ood_eval(coeffs, mc, mo, z)
    ood_c = oracle.gl3_ood_eval(comp_coeffs, list(range(ncomp)), [0] * ncomp, zc) if ncomp else zero3
    want = oracle.gl3_deep_compose(lde, comp_lde, log_n, lb, OFFSET, mc, mo, ood_t, ct, ood_c, cc, z, zc)
    _check(run(lde, comp_lde, ood_t, ood_c, z, zc), want, "deep, honest")
    # (b) the sub-coset rows forced onto small residues through the same-row cells of the three trace columns (the values are then no
    # polynomial's: the sub-coset rows are the definition's, the rest their extension)
    raw = [edge_column(N, seed + 20 + c) for c in range(3)]
    raw_comp = [edge_column(N, seed + 30 + k) for k in range(ncomp)]
    bad_t = np.stack([edge3(seed + 60 + j) for j in range(len(mc))])
    bad_c = np.stack([edge3(seed + 80 + k) for k in range(ncomp)]) if ncomp else zero3
    ref = lambda cols: oracle.gl3_deep_compose(cols, raw_comp, log_n, lb, OFFSET, mc, mo, bad_t, ct, bad_c, cc, z, zc)[::step]
    targets = small_targets((n, 3), seed)
    forced = force3(ref, raw, [tuple((c, i * step) for c in range(3)) for i in range(n)], targets)
    _check(run(raw, raw_comp, bad_t, bad_c, z, zc)[::step], ref(raw), "deep, edge columns")
    _check(run(forced, raw_comp, bad_t, bad_c, z, zc)[::step], targets, "deep, forced")
    # (c) z on the evaluation domain: the inverse table's entry for x = z is 0 (gl3_inverse_table_kernel; the oracle's gl3_inv maps
    # 0 to 0), and the other seven entries of that lane's chunk are the inverses they are without it
    wn = oracle.gl_root_of_unity(log_n)
    for m in (3 if n == 8 else 11, n - 1):                  # inside a chunk of 8 (m = 3 mod 8); the table's last index
        zd = np.array([OFFSET * pow(wn, m, P) % P, 0, 0], dtype=np.uint64)
        zcd = np.array([OFFSET * pow(wn, (m + 4) % n, P) % P, 0, 0], dtype=np.uint64)
        want = oracle.gl3_deep_compose(raw, raw_comp, log_n, lb, OFFSET, mc, mo, bad_t, ct, bad_c, cc, zd, zcd)[::step]
        _check(run(raw, raw_comp, bad_t, bad_c, zd, zcd)[::step], want, "deep, z = x_%d" % m)


# ----------------------------------------------------------------------------- the constraint program
def edge_program(seed, size, ncols):
    """tests/test_goldilocks.py's random program with constants whose coordinates are EDGE words: full ones and (c, 0, 0) alternate"""
    from tests.test_goldilocks import _gl_program
    code, consts, n_slots = _gl_program(seed, size, ncols)
    ne = len(EDGE)
    for k in range(len(consts) - 1):                        # (the last one, (3, 1, 4), belongs to the INV tail)
        consts[k] = [EDGE[(k + seed) % ne], 0, 0] if k % 2 else [EDGE[(3 * k + seed) % ne], EDGE[(5 * k + 1) % ne], EDGE[(7 * k + 2) % ne]]
    return code, consts, n_slots


def forcing_program():
    """OUT = K0 c0 + K1 c1 + K2 c2 + c3 c4 + K3 c3[+1] c0[+2]: Fp-affine in the row's own cells of columns 0, 1, 2 - the other
    cells come from other rows or columns"""
    from sandstorm_amd import air_program as ap
    T = ap.Trace
    k = [ap.Const3(*(int(v) for v in edge3(s))) for s in (1, 2, 3, 4)]
    root = k[0] * T(0) + k[1] * T(1) + k[2] * T(2) + T(3) * T(4) + k[3] * T(3, 1) * T(4, 2)
    return ap.lower(root, P, ext=True)


def _quotient(ctx, code, consts, n_slots, tables, desc, cols, log_n, lb, interpret):
    N = (1 << log_n) << lb
    out = ctx.alloc(24 * N)
    ctx.zero(out)
    if interpret:
        os.environ["SS_QUOTIENT_INTERPRET"] = "1"
    try:
        ctx.eval_quotient_gl64x3(code, consts, n_slots, ctx.column(tables) if tables is not None else None, desc, [ctx.column(c) for c in cols], log_n, lb, OFFSET, out)
    finally:
        os.environ.pop("SS_QUOTIENT_INTERPRET", None)
    return out.download(np.uint64, (N, 3))


@pytest.mark.parametrize("seed,size,log_n", [(1, 30, 3), (2, 120, 8), (3, 400, 12)])
def test_eval_quotient_on_edge_words(ctx, oracle, seed, size, log_n):
    lb, ncols = 1, 3
    N = 2 << log_n
    code, consts, n_slots = edge_program(seed, size, ncols)
    lde = [edge_column(N, 200 + seed + c) for c in range(ncols)]
    # gl3_mul_typed / gl3_inv_typed branch per lane on zero upper coordinates: a column with 0 in some lanes only makes every product
    # with it a base-field value (0) in those lanes and a full one in the others
    lde[0][1::3] = 0
    assert (lde[0] != 0).any()
    tables, desc = np.concatenate([edge_column(4, 210 + seed), edge_column(8, 220 + seed)]), [0, 2, 4, 3]
    want = oracle.gl3_eval_program(code, consts, n_slots, tables, desc, lde, log_n, lb, OFFSET)
    for interpret in (False, True):
        _check(_quotient(ctx, code, consts, n_slots, tables, desc, lde, log_n, lb, interpret), want, "program %d, interpret %d" % (seed, interpret))


@pytest.mark.parametrize("log_n", [3, 9])
def test_eval_quotient_forced_outputs(ctx, oracle, log_n):
    lb = 1
    N = 2 << log_n
    prog = forcing_program()
    code, consts = np.array(prog.code, dtype=np.uint32), np.array(prog.consts, dtype=np.uint64).reshape(-1, 3)
    lde = [edge_column(N, 230 + log_n + c) for c in range(5)]
    ref = lambda cols: oracle.gl3_eval_program(code, consts, prog.n_slots, None, [], cols, log_n, lb, OFFSET)
    targets = small_targets((N, 3), 240 + log_n)
    forced = force3(ref, lde, [tuple((c, i) for c in range(3)) for i in range(N)], targets)
    for interpret in (False, True):
        _check(_quotient(ctx, code, consts, prog.n_slots, None, [], lde, log_n, lb, interpret), ref(lde), "forcing program, edge cells")
        _check(_quotient(ctx, code, consts, prog.n_slots, None, [], forced, log_n, lb, interpret), targets, "forcing program, forced")


def test_compiled_composition_kernel_on_edge_words(ctx, oracle):
    """tests/test_goldilocks_stark.py test_compiled_composition_kernel_is_the_interpreter (whose cells stay below 2^62) with all eight
    LDE columns from the whole of [0, p): compiled = interpreter = oracle, and the program is the one the compiled kernel serves"""
    from sandstorm_amd import air_program as ap
    from sandstorm_amd.layouts import plain as pl
    log_n, lb = 10, 1
    n, N = 1 << log_n, 2 << log_n
    prog = pl.example_program(10)
    states, memory = pl.run(prog, 64)
    stmt = copy.deepcopy(pl.public_input_of(prog, states, memory))
    stmt.n_steps = n // 16
    ch, alpha = [(11, 22, 33), (5, 6, 7), (9, 8, 7)], (123456789, 987654321, 55555)
    tables = pl.Tables(n, lb)
    root = pl.composition(n, pl.Hints.from_public_input(stmt, ch, n), ch, alpha, tables)
    program = ap.lower(root, pl.P, ext=True, symbols=tables.symbols)
    code, consts = np.array(program.code, dtype=np.uint32), np.array(program.consts, dtype=np.uint64)
    tvals, tdesc = tables.device_tables()
    lde = [edge_column(N, 250 + c) for c in range(8)]
    want = oracle.gl3_eval_program(code, consts, program.n_slots, tvals, tdesc, lde, log_n, lb, pl.GENERATOR)
    assert pl.GENERATOR == OFFSET
    compiled = _quotient(ctx, code, consts, program.n_slots, tvals, tdesc, lde, log_n, lb, False)
    interpreted = _quotient(ctx, code, consts, program.n_slots, tvals, tdesc, lde, log_n, lb, True)
    _check(interpreted, want, "interpreter")
    _check(compiled, want, "compiled kernel")
    # the library must in fact have taken the compiled kernel for this program: the generated hash is this program's
    inc = open(os.path.join(ROOT, "sandstorm_amd", "csrc", "quotient_gen_plain_gl.inc")).read()
    h = 0xcbf29ce484222325
    for w in program.code:
        for k in range(4):
            h = ((h ^ ((int(w) >> (8 * k)) & 0xff)) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    assert h == int(re.search(r"GL3_PLAIN_CODE_HASH = (0x[0-9a-f]+)ull", inc).group(1), 16), "regenerate csrc/quotient_gen_plain_gl.inc"


# ----------------------------------------------------------------------------- the constraint check
U2 = (0, 0, 1)


def check_program():
    """three constraints on every row:  0: c0 + c1   1: c2 c3 - 1   2: c4 + X^2 c5 (a numerator with an upper coordinate of its own)"""
    from sandstorm_amd import air_program as ap
    T = ap.Trace
    return ap.lower_checks([T(0) + T(1), T(2) * T(3) - 1, T(4) + ap.Const3(*U2) * T(5)], P, ext=True)


def check_columns(n, seed):
    """every numerator is exactly 0, reached through wrap-around: c0 + c1 = p (p - 1 + 1 among them), c2 c3 = 1 (mod p) ((p - 1)(p - 1) among them)"""
    c0 = edge_column(n, 300 + seed)
    c1 = (np.uint64(P) - c0) % np.uint64(P)
    c2 = np.where(edge_column(n, 310 + seed) == 0, np.uint64(P - 1), edge_column(n, 310 + seed))
    c3 = np.array([pow(int(v), -1, P) for v in c2], dtype=np.uint64)
    c0[5], c1[5], c2[6], c3[6] = P - 1, 1, P - 1, P - 1
    return [c0, c1, c2, c3, np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)]


def check_report(cols, n):
    """(first row, count) per constraint in Python integers"""
    bad = [[], [], []]
    for r in range(n):
        c = [int(col[r]) for col in cols]
        nums = [((c[0] + c[1]) % P, 0, 0), ((c[2] * c[3] - 1) % P, 0, 0), (c[4] % P, 0, c[5] % P)]
        for k, v in enumerate(nums):
            if any(v):
                bad[k].append(r)
    return [b[0] if b else 2**64 - 1 for b in bad], [len(b) for b in bad]


@pytest.mark.parametrize("n", [64, 512])
def test_check_constraints_on_edge_words(ctx, n):
    prog = check_program()
    code, consts = np.array(prog.code, dtype=np.uint32), np.array(prog.consts, dtype=np.uint64).reshape(-1, 3)
    domains = [([], [(n, 0)])] * 3

    def device(cols):
        first, count = ctx.check_constraints_gl64x3(code, consts, prog.n_slots, None, [], [ctx.column(c) for c in cols], n.bit_length() - 1, domains)
        return [int(v) for v in first], [int(v) for v in count]
    cols = check_columns(n, n)
    assert (cols[0] == P - 1).any() and (cols[2] == P - 1).any()
    assert check_report(cols, n) == ([2**64 - 1] * 3, [0] * 3)
    assert device(cols) == ([2**64 - 1] * 3, [0] * 3)        # zeros reached through wrap-around are not reported
    # numerators equal to p - 1 (rows 9 and n - 1 of constraint 0, row 17 of constraint 1) and to 2^32 - 2 in coordinate 2 only (constraint 2)
    cols[1][9] = (P - 1 - int(cols[0][9])) % P
    cols[1][n - 1] = (P - 1 - int(cols[0][n - 1])) % P
    cols[3][17] = (P - int(cols[3][17])) % P                # c2 c3 = -1: the numerator is p - 2; and 0 * anything - 1 = p - 1:
    cols[2][33] = 0
    cols[5][n - 2] = EPS - 1
    cols[5][3] = P - 1
    want = check_report(cols, n)
    assert want == ([9, 17, 3], [2, 2, 2])
    assert device(cols) == want


# ----------------------------------------------------------------------------- running products
def _running(ctx, na, nv, da, dv, stride, count, z, alpha, out_stride, out_offset):
    """the device's column(s) and last value beside oracle/gl_cpu_context.py's"""
    from oracle.gl_cpu_context import GlCpuContext
    rows = count * out_stride + out_offset
    outs = [ctx.alloc(8 * rows) for _ in range(3)]
    for o in outs:
        ctx.zero(o)
    dev = lambda a: ctx.column(a) if a is not None else None
    last = ctx.running_product_gl64x3(dev(na), dev(nv), dev(da), dev(dv), stride, count, z, alpha, outs, out_stride, out_offset)
    got = np.stack([o.download(np.uint64, (rows,)) for o in outs])
    want = [np.zeros(rows, dtype=np.uint64) for _ in range(3)]
    want_last = GlCpuContext().running_product_gl64x3(na, nv, da, dv, stride, count, z, alpha, want, out_stride, out_offset)
    assert_canonical(np.array(last, dtype=np.uint64), "the last value")
    assert last == tuple(int(v) for v in want_last), (count, last, want_last)
    return got, np.stack(want)


@pytest.mark.parametrize("count", [1, 8, 9, 129, 1025])    # the level boundaries of the groups of 8
@pytest.mark.parametrize("two_columns", [False, True])
def test_running_product_on_edge_words_and_forced_outputs(ctx, count, two_columns):
    from oracle.gl_cpu_context import add3, f3, scale3, sub3
    stride, out_stride, out_offset = (2, 2, 1) if two_columns else (1, 1, 0)
    size, seed = count * stride, 400 + count + two_columns
    # (a) edge operands; z and alpha with edge coordinates (no term z - (alpha v + a) vanishes: z has upper coordinates alpha v cannot all match)
    z, alpha = [int(v) for v in edge3(seed)], ([int(v) for v in edge3(seed + 1)] if two_columns else None)
    na, da = edge_column(size, seed), edge_column(size, seed + 1)
    nv, dv = (edge_column(size, seed + 2), edge_column(size, seed + 3)) if two_columns else (None, None)
    for a, v in ((na, nv), (da, dv)):
        for i in range(0, size, stride):
            assert any(sub3(z, add3(scale3(alpha, int(v[i])) if two_columns else (0, 0, 0), f3(int(a[i])))))
    got, want = _running(ctx, na, nv, da, dv, stride, count, z, alpha, out_stride, out_offset)
    _check(got, want, "running product of %d, edge operands" % count)
    # (b) z and alpha in the base field, every output forced onto a small non-zero residue by solving na[k] in turn:
    # t_k = t_(k-1) (z - al nv_k - na_k) / (z - al dv_k - da_k); coordinates 1 and 2 are then exactly 0
    z0, al0 = EDGE[(seed + 3) % len(EDGE)] or 11, EDGE[(seed + 8) % len(EDGE)] or 13
    targets = [int(v) or 2 for v in small_targets(count, seed)]
    na, prev = na.copy(), 1
    for k in range(count):
        i = k * stride
        den = (z0 - (al0 * int(dv[i]) if two_columns else 0) - int(da[i])) % P
        if den == 0:
            da[i] = (int(da[i]) + 1) % P
            den = P - 1
        na[i] = (z0 - (al0 * int(nv[i]) if two_columns else 0) - targets[k] * pow(prev, -1, P) * den) % P
        prev = targets[k]
    got, want = _running(ctx, na, nv, da, dv, stride, count, [z0, 0, 0], [al0, 0, 0] if two_columns else None, out_stride, out_offset)
    _check(got, want, "running product of %d, forced" % count)
    assert [int(v) for v in got[0][out_offset::out_stride]] == targets and not got[1:].any()
    # (d) two columns: every term's first coordinate al0 v + a is a small non-zero residue r reached as the integer p + r (the word a
    # lazy addition would leave, and no legal second operand of the subtraction from z that follows), with z0 = 0 < r
    if two_columns:
        z, al = [0] + [int(v) for v in edge3(seed + 4)[1:]], [int(v) for v in edge3(seed + 5)]
        for a, v, s in ((na, nv, seed + 6), (da, dv, seed + 7)):
            r = [int(t) or 3 for t in small_targets(count, s)]
            for k in range(count):
                a[k * stride] = (r[k] - al[0] * int(v[k * stride])) % P
        got, want = _running(ctx, na, nv, da, dv, stride, count, z, al, out_stride, out_offset)
        _check(got, want, "running product of %d, terms with two words" % count)
    # (c) a numerator term that vanishes: z = (na[k0], 0, 0) (single column) - the column is 0 from there on
    if not two_columns:
        k0 = count // 2
        z1 = int(na[k0])
        da = np.where(da == np.uint64(z1), np.uint64((z1 + 1) % P), da)
        got, want = _running(ctx, na, None, da, None, 1, count, [z1, 0, 0], None, 1, 0)
        _check(got, want, "running product of %d, a vanishing term" % count)
        assert not got[:, k0:].any()


# ----------------------------------------------------------------------------- row hashing
@pytest.mark.parametrize("nseg,seg_len", [(1, 1), (8, 3), (16, 1)])
def test_hash_rows_of_edge_words(ctx, be, nseg, seg_len):
    """what is hashed is the canonical word's little-endian bytes: rows of EDGE words against hashlib (and the library's host Keccak)"""
    import hashlib
    from sandstorm_amd.coin import keccak256
    nrows = 64
    segs = [edge_column(nrows * seg_len, 500 + s + nseg) for s in range(nseg)]
    for s in range(nseg):                                   # a row of p - 1 in every position, a row of zeros
        segs[s][seg_len:2 * seg_len], segs[s][2 * seg_len:3 * seg_len] = P - 1, 0
    d_segs = [ctx.column(s) for s in segs]
    row_bytes = lambda i: b"".join(int(s[i * seg_len + e]).to_bytes(8, "little") for s in segs for e in range(seg_len))
    for kind, h in ((be.HASH_KECCAK, keccak256), (be.HASH_SHA256, lambda d: hashlib.sha256(d).digest()), (be.HASH_BLAKE2S, lambda d: hashlib.blake2s(d).digest())):
        out = ctx.alloc(32 * nrows)
        ctx.hash_rows_gl64(d_segs, seg_len, nrows, out, kind)
        got = out.download(np.uint8, (nrows, 32))
        assert [bytes(r) for r in got] == [h(row_bytes(i)) for i in range(nrows)], (kind, nseg, seg_len)
