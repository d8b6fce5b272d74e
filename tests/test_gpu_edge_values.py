"""The 252-bit kernels at the top of the field.  Every other parity test draws its felts from `examples.random_column`, which keeps
them below 2^251; here the inputs are tests/edge_values.py's columns - values in [2^251, p), p - 1, p - 2, (p +- 1) / 2, the
Montgomery and R280 images of +-1 and +-2, word / limb boundaries, uniform draws from the whole of [0, p) - and, where a kernel's
output is easy to steer, outputs FORCED onto those values (the reference's inverse of an edge column, or an input cell solved for per
row).  This is where the lazy bounds of fl252.h / fp252.h have their edge cases: the quotient read off the top limb, the
subtraction constants' preconditions, the final reduction at x = p.  Every output is checked to be canonical (< p) first, then
compared bit for bit with the oracle (which tests/test_oracle_edge_values.py holds to big-integer restatements on the same columns).

Sizes above 2^14 carry `large` in their names: the CPU run of this file (tests/test_device_code_on_host.py) leaves them out."""
import random

import numpy as np
import pytest

from tests.edge_values import EDGE, P, R256, assert_canonical, edge_column, from_limbs, solve_cell, to_limbs

pytestmark = pytest.mark.gpu


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


def _felt(v):
    return to_limbs([v])[0]


G3 = _felt(3 * R256 % P)                                   # the domain offset 3, stored
# FRI fold challenges: 0, Mont(1), Mont(-1), p - 1, 2^251
ALPHAS = [0, R256, P - R256, P - 1, 2**251]


def _down(buf, n):
    return buf.download(np.uint64, (n, 4))


def _check(got, want, what):
    assert_canonical(got, what)
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=-1).reshape(-1))[0]
        raise AssertionError("%s: %d of %d differ, first at %d: %#x != %#x" % (what, len(bad), got.reshape(-1, 4).shape[0], bad[0],
                             from_limbs(got.reshape(-1, 4)[bad[0]])[0], from_limbs(want.reshape(-1, 4)[bad[0]])[0]))


def _brev(log_n):
    return np.array([int(format(i, "0%db" % log_n)[::-1], 2) if log_n else 0 for i in range(1 << log_n)], dtype=np.int64)


# ----------------------------------------------------------------------------- NTT
def _ntt_edges(ctx, be, oracle, log_n, coset):
    n = 1 << log_n
    off = G3 if coset else None
    x = edge_column(n, log_n)
    y = edge_column(n, 100 + log_n)                        # the forced outputs: forward(x_y) = y with x_y the reference inverse of y
    x_y = oracle.ntt(y, inverse=True, offset=off)
    br = _brev(log_n)
    # edge inputs, both directions, natural order
    for direction, src, want in ((be.FORWARD, x, oracle.ntt(x, offset=off)), (be.INVERSE, x, oracle.ntt(x, inverse=True, offset=off)),
                                 (be.FORWARD, x_y, y), (be.INVERSE, y, x_y)):
        d = ctx.column(src)
        ctx.ntt([d], log_n, direction, off)
        _check(_down(d, n), want, "ntt 2^%d dir %d coset %d" % (log_n, direction, coset))
    # bit-reversed orders: forward from bit-reversed input, forward to bit-reversed output, inverse to bit-reversed coefficients
    d = ctx.column(np.ascontiguousarray(x_y[br]))
    ctx.ntt([d], log_n, be.FORWARD, off, be.BITREV, be.NATURAL)
    _check(_down(d, n), y, "ntt bitrev in")
    d = ctx.column(x_y)
    ctx.ntt([d], log_n, be.FORWARD, off, be.NATURAL, be.BITREV)
    _check(_down(d, n), np.ascontiguousarray(y[br]), "ntt bitrev out")
    d = ctx.column(y)
    ctx.ntt([d], log_n, be.INVERSE, off, be.NATURAL, be.BITREV)
    _check(_down(d, n), np.ascontiguousarray(x_y[br]), "intt bitrev out")


@pytest.mark.parametrize("log_n", [1, 2, 5, 11, 12, 14])   # one pass up to 2^11 (SS_NTT_LOG_TILE), two up to 2^18
@pytest.mark.parametrize("coset", [False, True])
def test_ntt_on_edge_values(ctx, be, oracle, log_n, coset):
    _ntt_edges(ctx, be, oracle, log_n, coset)


@pytest.mark.parametrize("log_n", [19, 20])                # three passes
def test_ntt_on_edge_values_large(ctx, be, oracle, log_n):
    _ntt_edges(ctx, be, oracle, log_n, True)


# ----------------------------------------------------------------------------- LDE / evaluate
@pytest.mark.parametrize("log_n,log_blowup", [(3, 1), (10, 2), (12, 1), (5, 9)])
def test_lde_and_evaluate_on_edge_values(ctx, be, oracle, log_n, log_blowup):
    """Matrix.lde of edge trace-domain values; ctx.evaluate (the few-coefficients path when the blow-up is large) of edge
    coefficient columns, and of the coefficients of trace-domain values forced to edges"""
    n, N = 1 << log_n, 1 << (log_n + log_blowup)
    cols = [edge_column(n, 7 * c + log_n) for c in range(2)]
    m = be.Matrix.from_host(ctx, cols)
    ev, co = m.lde(log_blowup, G3)
    ev_h, co_h = ev.to_host(), co.to_host()
    for c in range(2):
        want_ev, want_co = oracle.lde(cols[c], log_blowup, G3)
        _check(ev_h[c], want_ev, "lde evaluations")
        _check(co_h[c], oracle.bitrev_permute(want_co), "lde coefficients")
    br = _brev(log_n)
    coeffs = [edge_column(n, 50 + log_n), oracle.ntt(edge_column(n, 60 + log_n), inverse=True)]
    outs = [ctx.alloc(32 * N) for _ in coeffs]
    ctx.evaluate([ctx.column(np.ascontiguousarray(c[br])) for c in coeffs], log_n, log_blowup, G3, outs)
    for c, out in zip(coeffs, outs):
        _check(_down(out, N), oracle.ntt(np.concatenate([c, np.zeros((N - n, 4), dtype=np.uint64)]), offset=G3), "evaluate")
    # the second column's values on the trace domain (offset 1) are the forced edges
    one = [ctx.alloc(32 * N)]
    ctx.evaluate([ctx.column(np.ascontiguousarray(coeffs[1][br]))], log_n, log_blowup, _felt(R256), one)
    _check(_down(one[0], N)[::1 << log_blowup], edge_column(n, 60 + log_n), "evaluate onto the trace domain")


# ----------------------------------------------------------------------------- FRI fold
@pytest.mark.parametrize("fold", [2, 4, 8, 16])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("row_bits", [4, 9])               # below / above the power tables' bar (2^8 rows)
def test_fri_fold_on_edge_values(ctx, be, oracle, fold, flags, row_bits):
    log_fold = fold.bit_length() - 1
    log_len = row_bits + log_fold
    n, rows = 1 << log_len, 1 << row_bits
    ev = edge_column(n, 3 * fold + flags + row_bits)
    targets = edge_column(rows, 200 + fold + flags)
    d_out = ctx.alloc(32 * rows)
    for alpha in ALPHAS:
        am = _felt(alpha)
        ref = lambda cols: oracle.fri_fold(cols[0], fold, am, G3, flags)
        forced = solve_cell(ref, [ev], [(0, fold * j if flags & 1 else j) for j in range(rows)], targets)[0]
        assert np.array_equal(ref([forced]), targets)
        for src, want in ((ev, ref([ev])), (forced, targets)):
            ctx.fri_fold(ctx.column(src), log_len, fold, am, G3, d_out, flags)
            _check(_down(d_out, rows), want, "fold %d flags %d alpha %#x" % (fold, flags, alpha))
            if not flags & 1:                              # a row range (bit-reversed layers are folded whole)
                r0, cnt = rows // 4, rows // 2
                local = np.concatenate([src[k * rows + r0:k * rows + r0 + cnt] for k in range(fold)])
                part = ctx.alloc(32 * cnt)
                ctx.fri_fold_rows(ctx.column(local), log_len, fold, am, G3, r0, cnt, part, flags)
                _check(_down(part, cnt), want[r0:r0 + cnt], "fold rows")


# ----------------------------------------------------------------------------- OOD / poly eval
POINTS = [0, 1, P - 1, 2**251, P - 2, R256, P - R256, 2**224 - 1, 0x1F2E3D4C5B6A7988 ** 3 % P]


@pytest.mark.parametrize("log_n", [1, 3, 7, 12])
def test_poly_eval_on_edge_values(ctx, be, oracle, log_n):
    n = 1 << log_n
    cols = [edge_column(n, 300 + c + log_n) for c in range(2)]
    br = _brev(log_n)
    d = [ctx.column(np.ascontiguousarray(c[br])) for c in cols]
    for x in POINTS:
        got = ctx.poly_eval(d, log_n, _felt(x))
        _check(got, np.stack([oracle.poly_eval(c, _felt(x)) for c in cols]), "poly_eval at %#x" % x)


@pytest.mark.parametrize("log_n", [4, 11])
def test_ood_eval_on_edge_values(ctx, be, oracle, log_n):
    n = 1 << log_n
    cols = [edge_column(n, 400 + c + log_n) for c in range(3)]
    br = _brev(log_n)
    d = [ctx.column(np.ascontiguousarray(c[br])) for c in cols]
    mask = [(0, 0), (0, 1), (1, 0), (2, 3), (2, n - 1), (1, 7 % n), (0, 5 % n)]
    w = pow(3, (P - 1) >> log_n, P)
    for z in POINTS:
        got = ctx.ood_eval(d, log_n, [c for c, _ in mask], [o for _, o in mask], _felt(z))
        zp = z * pow(R256, -1, P) % P                       # the point the stored value stands for
        want = np.stack([oracle.poly_eval(cols[c], _felt(zp * pow(w, o, P) % P * R256 % P)) for c, o in mask])
        _check(got, want, "ood_eval at %#x" % z)


# ----------------------------------------------------------------------------- DEEP
def _outside(z_stored, log_n, log_blowup, offs):
    """z w_n^o (o in offs) and z^2 are off the evaluation coset 3 <w_N>"""
    N = 1 << (log_n + log_blowup)
    z = z_stored * pow(R256, -1, P) % P
    w = pow(3, (P - 1) >> log_n, P)
    pts = [z * pow(w, o, P) % P for o in offs] + [z * z % P]
    return all(pow(x * pow(3, -1, P) % P, N, P) != 1 for x in pts)


@pytest.mark.parametrize("log_n", [3, 9])
@pytest.mark.parametrize("prepared", [False, True])
def test_deep_compose_on_edge_values(ctx, be, oracle, log_n, prepared):
    """The DEEP polynomial has degree < n, so ss_deep_compose composes it on the sub-coset (every blow-up-th LDE row, one input row
    per point) and re-expands it (include/sandstorm_hip.h).  With edge inputs - which no real LDE and out-of-domain values make
    consistent - the sub-coset rows are the oracle's composition point by point and the rest its extension; with a composition cell
    solved for per sub-coset row, the sub-coset rows are the forced edge targets."""
    lb = 1
    n, N = 1 << log_n, 1 << (log_n + lb)
    ev = [edge_column(N, 500 + c + log_n) for c in range(3)]
    comp = [edge_column(N, 510 + k + log_n) for k in range(2)]
    mask = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 5 % n), (0, n - 1), (2, 1)]
    mc, mo = [c for c, _ in mask], [o for _, o in mask]
    ood_t = edge_column(len(mask), 520 + log_n)
    ood_c = edge_column(2, 530)
    ct = edge_column(len(mask), 540 + log_n)
    cc = to_limbs([P - 1, 2**251])
    targets = edge_column(n, 550 + log_n)
    zero_pad = np.zeros((N - n, 4), dtype=np.uint64)
    d_ev = [ctx.column(c) for c in ev]
    out = ctx.alloc(32 * N)
    tried = 0
    for z in [0, 2**251, P - 2, R256 * 5 % P, 0x13579BDF02468ACE ** 3 % P] + EDGE[10:14]:
        if not _outside(z, log_n, lb, mo):
            continue
        tried += 1
        zm = _felt(z)
        ref = lambda cm: oracle.deep_compose(ev, cm, log_n, lb, G3, mc, mo, ood_t, ct, ood_c, cc, zm)[::1 << lb]
        forced = solve_cell(ref, comp, [(0, i << lb) for i in range(n)], targets)
        for cm, want in ((comp, ref(comp)), (forced, targets)):
            if prepared:
                ctx.deep_prepare(len(cm), log_n, G3, zm)
            ctx.deep_compose(d_ev, [ctx.column(c) for c in cm], log_n, lb, G3, mc, mo, ood_t, ct, ood_c, cc, zm, out)
            got = _down(out, N)
            _check(got[::1 << lb], want, "deep_compose z %#x" % z)
            ext = oracle.ntt(np.concatenate([oracle.ntt(want, inverse=True, offset=G3), zero_pad]), offset=G3)
            _check(got, ext, "deep_compose z %#x, extended" % z)
    assert tried >= 6


# ----------------------------------------------------------------------------- constraint evaluation
@pytest.mark.parametrize("seed,size,log_n", [(1, 30, 3), (2, 120, 8), (3, 400, 10)])
def test_eval_quotient_on_edge_values(ctx, be, oracle, seed, size, log_n):
    from sandstorm_amd import air_program as ap
    from tests.test_air_program import random_dag
    lb, ncols = 1, 3
    N = 1 << (log_n + lb)
    cols = [edge_column(N, 600 + seed + c) for c in range(ncols)]
    tabs = [edge_column(4, 610 + seed), edge_column(8, 620 + seed)]
    tables, desc = np.concatenate(tabs), [0, 2, 4, 3]
    prog = ap.lower(random_dag(random.Random(seed), ncols, 2, 5, size), P)
    m = be.Matrix.from_host(ctx, cols)
    out = ctx.alloc(32 * N)
    ctx.eval_quotient(prog, ctx.column(tables), desc, m.cols, log_n, lb, G3, out)
    want = oracle.eval_program(prog.code, oracle.to_mont(prog.consts), tables, desc, prog.n_slots, cols, log_n, lb, G3)
    _check(_down(out, N), want, "eval_quotient")


@pytest.mark.parametrize("layout", ["starknet", "recursive"])
def test_compiled_kernel_on_edge_values_large(oracle, layout, monkeypatch):
    """the generated starknet / recursive constraint kernels against the interpreter (as test_compiled_kernel_is_the_interpreter,
    at the size the kernels were generated for) with edge LDE columns and tables"""
    from sandstorm_amd import backend as be, hostlib
    from tests.test_gpu_real_quotient import _Prog
    from tests.test_layout_recursive import load_run
    from tests.test_layout_starknet import CHALLENGES, starknet_example
    log_n = 18
    if layout == "starknet":
        from sandstorm_amd.layouts import starknet as lay
        _, _, pi = starknet_example(11)
        cpp = hostlib.StarknetHostAir(None, pi, log_n)
    else:
        from sandstorm_amd.layouts import recursive as lay
        _, _, pi = load_run()
        cpp = hostlib.RecursiveHostAir(None, pi, log_n)
    n, N = 1 << log_n, 2 << log_n
    code, consts, n_slots, specs = cpp.dump(n, [oracle.to_mont([c])[0] for c in CHALLENGES], oracle.to_mont([pow(3, 99, P)])[0])
    cpp.close()
    tables = lay.Tables(n)
    tabs, desc, off = [], [], 0
    for k, spec in enumerate(specs):
        t = edge_column(tables.length(spec), 700 + k)
        desc += [off, len(t).bit_length() - 1]
        off += len(t)
        tabs.append(t)
    tab = np.concatenate(tabs)
    lde = [edge_column(N, 710 + c) for c in range(10)]
    ctx = be.Context(0)
    m = be.Matrix.from_host(ctx, lde)
    d_tab = ctx.column(tab)
    prog = _Prog(code, [int(v) for v in oracle.from_mont(consts)], n_slots)
    out = ctx.alloc(32 * N)
    ctx.eval_quotient(prog, d_tab, desc, m.cols, log_n, 1, G3, out)
    compiled = _down(out, N)
    monkeypatch.setenv("SS_QUOTIENT_INTERPRET", "1")
    ctx.zero(out)
    ctx.eval_quotient(prog, d_tab, desc, m.cols, log_n, 1, G3, out)
    interpreted = _down(out, N)
    assert_canonical(interpreted, "interpreter")
    _check(compiled, interpreted, "compiled %s kernel" % layout)
    assert compiled.any()
    ctx.close()


# ----------------------------------------------------------------------------- extension scans
def _nonzero_denominators(a, stride, a_off, v_off, count, z, alpha):
    """edge columns meet edge challenges: move the cells whose denominator term z - (a + alpha v) is 0 (that case has its own test)"""
    rinv = pow(R256, -1, P)                                # stored -> plain
    zi, ai = from_limbs(z)[0] * rinv % P, (from_limbs(alpha)[0] * rinv % P if alpha is not None else 0)
    vals = [v * rinv % P for v in from_limbs(a)]
    for i in range(count):
        ia = stride * i + a_off
        v = vals[stride * i + v_off] if v_off >= 0 else 0
        if (zi - (vals[ia] + ai * v)) % P == 0:
            a[ia] = _felt((from_limbs(a[ia])[0] + 1) % P)
    return a


@pytest.mark.parametrize("count", [65, 4097])
@pytest.mark.parametrize("challenge", [0, 1, 2])
def test_extension_scans_on_edge_values(ctx, oracle, count, challenge):
    """ss_permutation_product (address / value pairs and single cells), ss_diluted_aggregate (dense and strided) with edge columns
    and edge challenges"""
    z, alpha = [(to_limbs([P - 1])[0], to_limbs([2**251])[0]), (to_limbs([R256])[0], to_limbs([P - R256])[0]),
                (to_limbs([EDGE[11]])[0], to_limbs([P - 2])[0])][challenge]
    a = _nonzero_denominators(edge_column(2 * count, 800 + challenge), 2, 0, 1, count, z, alpha)
    b = _nonzero_denominators(edge_column(2 * count, 810 + challenge), 2, 0, 1, count, z, alpha)
    r = _nonzero_denominators(_nonzero_denominators(edge_column(4 * count, 820 + challenge), 4, 0, -1, count, z, None), 4, 2, -1, count, z, None)
    for num, den, os_, oo, al, src in (((a, 2, 0, 1), (b, 2, 0, 1), 2, 0, alpha, (a, b)), ((r, 4, 0, -1), (r, 4, 2, -1), 4, 1, None, (r, r))):
        want = np.zeros((count * os_, 4), dtype=np.uint64)
        last_want = oracle.permutation_product(num, den, count, z, al if al is not None else np.zeros(4, dtype=np.uint64), want, os_, oo)
        dout = ctx.alloc(32 * count * os_)
        ctx.zero(dout)
        da, db = ctx.column(src[0]), ctx.column(src[1])
        last = ctx.permutation_product((da,) + num[1:], (db,) + den[1:], count, z, al, dout, os_, oo)
        _check(_down(dout, count * os_), want, "permutation_product")
        _check(last, last_want, "permutation_product last")
    for stride, off, os_, oo in ((1, 0, 1, 0), (8, 5, 8, 3)):
        x = edge_column(stride * count, 830 + stride + challenge)
        want = np.zeros((count * os_, 4), dtype=np.uint64)
        oracle.diluted_aggregate(x, stride, off, count, z, alpha, want, os_, oo)
        dout = ctx.alloc(32 * count * os_)
        ctx.zero(dout)
        ctx.diluted_aggregate(ctx.column(x), stride, off, count, z, alpha, dout, os_, oo)
        _check(_down(dout, count * os_), want, "diluted_aggregate")


@pytest.mark.parametrize("dense", [True, False])
def test_block_scans_on_edge_values(ctx, oracle, dense):
    """ss_diluted_aggregate_block + ss_affine_apply and ss_permutation_product + ss_scale_strided over 4 row blocks of edge values, the
    blocks before a block folded in on the host: the single scan's cells"""
    world, count = 4, 256
    stride, off, os_, oo = (1, 0, 1, 0) if dense else (8, 5, 8, 3)
    total = count * world
    x = edge_column(stride * total, 900 + dense)
    z, alpha = to_limbs([P - 1])[0], to_limbs([2**251 + 2**192])[0]
    want = np.zeros((total * os_, 4), dtype=np.uint64)
    oracle.diluted_aggregate(x, stride, off, total, z, alpha, want, os_, oo)
    zc, ac = (int(v) for v in oracle.from_mont(np.stack([z, alpha])))
    xs = [int(v) for v in oracle.from_mont(x[off::stride])]
    value, got = None, np.zeros_like(want)
    for r in range(world):
        dx = ctx.column(x[r * count * stride:(r + 1) * count * stride])
        maps = ctx.alloc(64 * count)
        M, Cc = ctx.diluted_aggregate_block(dx, stride, off, count, r == 0, z, alpha, maps)
        assert_canonical(np.stack([M, Cc]), "block map")
        m, c = (int(oracle.from_mont(t[None])[0]) for t in (M, Cc))
        start = 0
        if r:
            u = (xs[r * count] - xs[r * count - 1]) % P
            start = (value * (1 + zc * u) + ac * u * u) % P
        dout = ctx.alloc(32 * count * os_)
        ctx.zero(dout)
        ctx.affine_apply(maps, count, oracle.to_mont([start])[0], dout, os_, oo)
        got[r * count * os_:(r + 1) * count * os_] = _down(dout, count * os_)
        value = (m * start + c) % P
    _check(got, want, "diluted_aggregate blocks")
    a = _nonzero_denominators(_nonzero_denominators(edge_column(4 * total, 910 + dense), 4, 0, -1, total, z, None), 4, 2, -1, total, z, None)
    want = np.zeros((total * 4, 4), dtype=np.uint64)
    oracle.permutation_product((a, 4, 0, -1), (a, 4, 2, -1), total, z, np.zeros(4, dtype=np.uint64), want, 4, 1)
    got, before = np.zeros_like(want), P - 1                # the factor the first block is scaled by: -1 ...
    for r in range(world):
        da = ctx.column(a[4 * r * count:4 * (r + 1) * count])
        dout = ctx.alloc(32 * count * 4)
        ctx.zero(dout)
        last = ctx.permutation_product((da, 4, 0, -1), (da, 4, 2, -1), count, z, None, dout, 4, 1)
        ctx.scale_strided(dout, 4, 1, count, oracle.to_mont([before])[0])
        got[4 * r * count:4 * (r + 1) * count] = _down(dout, count * 4)
        before = before * int(oracle.from_mont(last[None])[0]) % P
    sel = np.arange(1, total * 4, 4)
    neg = oracle.to_mont([(P - int(v)) % P for v in oracle.from_mont(want[sel])])   # ... so every cell is the negated scan
    _check(got[sel], neg, "permutation_product blocks")


# ----------------------------------------------------------------------------- row hashing / felt leaves
def _be_row(row):
    return b"".join(v.to_bytes(32, "big") for v in from_limbs(row))


@pytest.mark.parametrize("kind", [0, 2])
@pytest.mark.parametrize("ncols", [1, 2, 9])
def test_hash_rows_on_edge_values(ctx, be, oracle, kind, ncols):
    """Keccak / Blake2s of a row: the hash of its stored values' 32-byte big-endian images, computed here"""
    import hashlib
    n = 300
    cols = [edge_column(n, 950 + c + ncols) for c in range(ncols)]
    got = be.Matrix.from_host(ctx, cols).hash_rows(kind).download(np.uint8, (n, 32))
    assert oracle.keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    h = oracle.keccak256 if kind == be.HASH_KECCAK else (lambda b: hashlib.blake2s(b).digest())
    for i in range(n):
        assert bytes(got[i]) == h(_be_row(np.stack([c[i] for c in cols]))), (kind, ncols, i)


@pytest.mark.parametrize("tree", [0, 1])
def test_felt_leaves_on_edge_values(ctx, be, oracle, tree):
    """a tree over felt leaves: the leaves' parents are Keccak of two felts' images (masked to 20 bytes for tree 1), computed here"""
    n = 64
    leaves = edge_column(n, 990 + tree)
    nodes, tags = ctx.alloc(64 * n), ctx.alloc(2 * n)
    ctx.merkle_build(tree, 0, 1, ctx.column(leaves), n, nodes, tags)
    got = nodes.download(np.uint8, (2 * n, 32))
    for k in range(n // 2, n):
        d = oracle.keccak256(_be_row(leaves[2 * (k - n // 2):2 * (k - n // 2) + 2]))
        if tree == 1:
            d = d[:20] + bytes(12)
        assert bytes(got[k]) == d, (tree, k)
    want_nodes, _ = oracle.merkle_build(tree, 0, 1, leaves)
    assert np.array_equal(got[1:], want_nodes[1:])
