"""Real ECDSA builtin instances traced ON the device from their inputs (csrc/trace.hip trace_ecdsa_kernel behind ss_trace_ecdsa;
host/device_trace.hpp DeviceTrace::ecdsa, behind hostlib.trace_ecdsa_on_device) against the C++ host generator
(host/trace_starknet.cpp) and the Python mirror (layouts/starknet.py EcdsaInstanceTrace), bit for bit: the cells are field elements,
every comparison is exact.  The template path runs three scalar multiplications per distinct signature on the host and uploads 172 KB
for it; with the switch on 168 bytes per instance go up (the key's x, a root y the host has taken, the message, r, w) and a table of 252
constant points - which hostlib.trace_last_stats() makes observable, since the cells are the same whichever way they are made.  The
switch is off by default: other modules pin the template path.

Runs on the MI355X (`-m gpu`) and, in the CPU suite, on the host build of the device code (tests/test_ecdsa_trace_on_host.py)."""
import ctypes as C
import gzip
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_gpu_builtin_trace as bt          # noqa: E402  (its helpers: the statements, zeroed device columns, packed records, column comparison)
from test_gpu_ec_op_trace import Prefilled, SENTINEL, ADDR_SENTINEL       # noqa: E402  (columns that hold a sentinel everywhere)

pytestmark = pytest.mark.gpu
EMULATED = os.environ.get("SS_TEST_HIPEMU") == "1"
P = 2**251 + 17 * 2**192 + 1
ERR_ECDSA_INSTANCE, ERR_ECDSA_INVALID, ERR_ECDSA_DIVISOR, ERR_ECDSA_MEETS = 1 << 20, 1 << 21, 1 << 22, 1 << 23
BLOCK_ROWS, STEPS, STRIDE, GEN_STRIDE = 32768, 256, 64, 128
STEP_FIELDS = ("off_dbl_x", "off_dbl_y", "off_dbl_slope", "off_sum_x", "off_sum_y", "off_slope", "off_x_diff_inv", "off_suffix")
GEN_FIELDS = ("off_gen_x", "off_gen_y", "off_gen_slope", "off_gen_x_diff_inv", "off_gen_suffix")
SINGLE_FIELDS = ("off_r_point_slope", "off_r_point_x_diff_inv", "off_r_inv", "off_w_inv", "off_message_inv", "off_pubkey_x_squared", "off_b_slope", "off_b_x_diff_inv")
ECDSA_FIELDS = ("col", "row_stride", "gen_stride") + STEP_FIELDS + GEN_FIELDS + SINGLE_FIELDS + ("col_pool", "off_pair")


@pytest.fixture(scope="module")
def ctx():
    from sandstorm_amd import backend as be
    c = be.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def ecdsa_on_device():
    """the switch on for this module, and what it was afterwards (other modules of the same process pin the template path)"""
    from sandstorm_amd import hostlib
    before = hostlib.trace_ecdsa_on_device(True)
    try:
        yield
    finally:
        hostlib.trace_ecdsa_on_device(before)


def ecdsa_placement(col=0, col_pool=1):
    """where the starknet layout's ECDSA section writes (the `place` lambda of host/trace_starknet.cpp) as the fields of
    ss_trace_ecdsa_layout, for a column table that holds the auxiliary column at `col` and the memory pool at `col_pool`"""
    from sandstorm_amd.layouts import starknet as sk
    E, N = sk.Ecdsa, sk.Npc
    return dict(col=col, row_stride=STRIDE, gen_stride=GEN_STRIDE, off_dbl_x=E.PUBKEY_DOUBLING_X, off_dbl_y=E.PUBKEY_DOUBLING_Y, off_dbl_slope=E.PUBKEY_DOUBLING_SLOPE,
                off_sum_x=E.PUBKEY_PARTIAL_SUM_X, off_sum_y=E.PUBKEY_PARTIAL_SUM_Y, off_slope=E.PUBKEY_PARTIAL_SUM_SLOPE, off_x_diff_inv=E.PUBKEY_PARTIAL_SUM_X_DIFF_INV,
                off_suffix=E.R_SUFFIX, off_gen_x=E.GENERATOR_PARTIAL_SUM_X, off_gen_y=E.GENERATOR_PARTIAL_SUM_Y, off_gen_slope=E.GENERATOR_PARTIAL_SUM_SLOPE,
                off_gen_x_diff_inv=E.GENERATOR_PARTIAL_SUM_X_DIFF_INV, off_gen_suffix=E.MESSAGE_SUFFIX, off_r_point_slope=E.R_POINT_SLOPE,
                off_r_point_x_diff_inv=E.R_POINT_X_DIFF_INV, off_r_inv=E.R_INV, off_w_inv=E.W_INV, off_message_inv=E.MESSAGE_INV, off_pubkey_x_squared=E.PUBKEY_X_SQUARED,
                off_b_slope=E.B_SLOPE, off_b_x_diff_inv=E.B_X_DIFF_INV, col_pool=col_pool, off_pair=[N.ECDSA_PUBKEY_ADDR, N.ECDSA_MESSAGE_ADDR])


def ecdsa_writes(f):
    """the host section's writes of one instance in its order, as (column, row offset, what): the two halves' eight cells per step, the
    generator's five, the eight cells an instance has one of, the two pairs.  A later write of a cell wins"""
    out = []
    for half in range(2):
        for j in range(STEPS):
            out += [(f["col"], f[k] + STRIDE * (STEPS * half + j), (k, half, j)) for k in STEP_FIELDS]
    for j in range(STEPS):
        out += [(f["col"], f[k] + GEN_STRIDE * j, (k, j)) for k in GEN_FIELDS]
    out += [(f["col"], f[k], (k,)) for k in SINGLE_FIELDS]
    out += [(f["col_pool"], off + j, ("pair", k, j)) for k, off in enumerate(f["off_pair"]) for j in range(2)]
    return out


def ecdsa_cells(f):
    """-> {(column, row offset): what the LAST write of the cell is}"""
    return {(col, off): what for col, off, what in ecdsa_writes(f)}


def curve_points_array():
    """ss_trace_ecdsa's d_points: 2^i G for i <= 250, then the shift point, as Montgomery felts (x, y)"""
    from sandstorm_amd import backend as be
    from sandstorm_amd.layouts import starknet as sk
    pts = sk.ecdsa_generator_points()[:251] + [sk.SHIFT_POINT]
    assert len(pts) == 252 and pts[250] == sk.ecdsa_generator_points()[255]
    return np.ascontiguousarray(np.stack([be.felt(v) for p in pts for v in p]).astype(np.uint64))


def key_roots(x):
    """-> (the larger, the smaller) root of x^3 + x + beta"""
    from sandstorm_amd.layouts import starknet as sk
    y = sk._sqrt((pow(x, 3, P) + x + sk.CURVE_BETA) % P)
    assert y is not None
    return max(y, P - y), min(y, P - y)


def device_records(rows, which):
    """(index, x, message, r, w) rows -> the entry point's records (index, x, y, message, r, w); which[k]: 0 the larger root, 1 the smaller"""
    return bt.records([(i, x, key_roots(x)[which[k % len(which)]], m, r, w) for k, (i, x, m, r, w) in enumerate(rows)])


def call_ecdsa(ctx, z, f, points, recs, n_given, n_blocks, begin, ncols=2):
    return ctx.lib.ss_trace_ecdsa(ctx.handle, z.ptrs(), ncols, z.n, bt.flat(f, ECDSA_FIELDS), points.ptr, recs.ptr, n_given, n_blocks, BLOCK_ROWS, begin, z.pool_addr.ptr,
                                  z.status.ptr)


_ENTRY = {}


def entry_point_instances():
    """the two signatures of test_layout_starknet.real_instances() (blocks 1 and 4; the second has a one-bit message), the dummy signature
    (block 0) and two seeded ones (blocks 2, 3) chosen among the first of examples.seeded_ecdsa_instances so that the five hold a key
    whose LARGER root verifies and one whose SMALLER root does -> (rows, [which root each key's accepted y is: 0 larger, 1 smaller])"""
    if not _ENTRY:
        from sandstorm_amd import examples
        from sandstorm_amd.layouts import starknet as sk
        from test_layout_starknet import real_instances
        rows = list(real_instances()["ecdsa"])
        assert sorted(r[0] for r in rows) == [1, 4] and rows[1][2] == 1 << 7
        rows.append((0,) + tuple(sk.ecdsa_dummy_instance()))
        accepted = lambda row: 0 if sk.EcdsaInstanceTrace(*row[1:]).pubkey[1] == key_roots(row[1])[0] else 1
        seeded = examples.seeded_ecdsa_instances(8)
        roots = [accepted(r) for r in seeded]
        first = seeded[0]
        other = next(r for r, a in zip(seeded, roots) if a != roots[0])
        rows += [(2,) + first[1:], (3,) + other[1:]]
        _ENTRY["rows"], _ENTRY["accepted"] = rows, [accepted(r) for r in rows]
    return _ENTRY["rows"], _ENTRY["accepted"]


# ---- 1. the entry point alone
def test_ecdsa_entry_point_alone_writes_the_generators_cells_and_nothing_else(ctx):
    """ss_trace_ecdsa through ctypes into two columns (auxiliary, pool) of 6 blocks that hold a sentinel: every cell the host generator's
    ECDSA section places holds the host generator's value and the Python mirror's - the four step-255 cells that the section's single
    cells land on hold the single cells' values; every other cell still holds the sentinel; d_pool_addr holds the two addresses and the
    sentinel elsewhere.  The records carry the larger root for some keys and the smaller for others, and both roots are accepted ones.
    Four of the section's cells - the chord's slope and the x-difference's inverse at step 255 of either half - are the two flag cells of
    the two EC-op blocks that share the rows: the generator's EC-op section, which runs later, rewrites them, so the generator's columns
    hold the EC-op dummy's flags there and those four cells are compared with the Python mirror alone (as every cell is, further down)"""
    from sandstorm_amd import backend as be, hostlib
    from sandstorm_amd.layouts import starknet as sk
    trace_bin, memory_bin, pi = bt.statement("starknet")
    n_blocks = 6
    n = n_blocks * BLOCK_ROWS
    f = ecdsa_placement()
    instances, accepted = entry_point_instances()
    assert 0 in accepted and 1 in accepted, "both the larger and the smaller root are accepted ones"
    want_all = hostlib.starknet_base_trace(trace_bin, memory_bin, pi, {"ecdsa": instances})
    want = [want_all[sk.COL_AUXILIARY][:n], want_all[sk.COL_NPC][:n]]
    begin = pi.memory_segments["ecdsa"][0]
    z = Prefilled(ctx, 2, n)
    given_root = [0, 1, 1, 0, 1]                                       # the y of the record: the accepted root or the other one, larger or smaller
    assert any(g == a for g, a in zip(given_root, accepted)) and any(g != a for g, a in zip(given_root, accepted))
    recs = ctx.alloc(168 * len(instances)).upload(device_records(instances, given_root))
    points = ctx.alloc(252 * 64).upload(curve_points_array())
    st = call_ecdsa(ctx, z, f, points, recs, len(instances), n_blocks, begin)
    assert st == 0, ctx.lib.ss_last_error()
    assert z.read_status()[0] == 0
    got = z.columns()
    pool_addr = z.pool_addr.download(np.uint32, (n // 2,))
    z.free()
    recs.free()
    points.free()
    cells = ecdsa_cells(f)
    assert len(ecdsa_writes(f)) == 2 * 256 * 8 + 256 * 5 + 8 + 4
    assert len(cells) == 5380 + 4, "four of the eight single cells are step-255 cells of the chains"
    for single, step in (("off_r_inv", ("off_dbl_slope", 0, 255)), ("off_w_inv", ("off_dbl_slope", 1, 255)), ("off_b_slope", ("off_gen_slope", 255)),
                         ("off_b_x_diff_inv", ("off_gen_x_diff_inv", 255))):
        assert cells[(0, f[single])] == (single,) and (0, f[single], step) in ecdsa_writes(f)
    rewritten = {(0, sk.EC_OP_BUILTIN_RATIO * 16 * k + off) for k in range(2) for off in (sk.EcOp.M_BIT251_AND_BIT196, sk.EcOp.M_BIT251_AND_BIT196_AND_BIT192)}
    assert rewritten == {(0, f[k] + STRIDE * (STEPS * half + 255)) for k in ("off_slope", "off_x_diff_inv") for half in range(2)} and rewritten < set(cells)
    masks = [np.zeros(n, dtype=bool) for _ in range(2)]
    want_addr = np.full(n // 2, ADDR_SENTINEL, dtype=np.uint32)
    for row in instances:
        for col, off in cells:
            masks[col][row[0] * BLOCK_ROWS + off] = True
        for col, off in rewritten:                                     # the device's value there is the section's; the generator's the later section's
            assert not want[col][row[0] * BLOCK_ROWS + off].any(), "the EC-op dummy's flags are zero"
            want[col][row[0] * BLOCK_ROWS + off] = got[col][row[0] * BLOCK_ROWS + off]
        for k, off in enumerate(f["off_pair"]):
            want_addr[(row[0] * BLOCK_ROWS + off) // 2] = begin + 2 * row[0] + k
    for c in range(2):
        assert np.array_equal(got[c][masks[c]], want[c][masks[c]]), "column %d: the instances' cells" % c
        assert (got[c][~masks[c]] == np.uint64(SENTINEL)).all(), "column %d: a cell outside the instances' was written" % c
    assert np.array_equal(pool_addr, want_addr)
    # the Python mirror, converted with backend.felt, in the section's write order (a later value of a cell replaces an earlier one)
    for (index, x, message, r, w), root in zip(instances, accepted):
        t = sk.EcdsaInstanceTrace(x, message, r, w)
        assert t.pubkey == (x, key_roots(x)[root])
        base = index * BLOCK_ROWS
        value = {}
        for half, (mad, dbl) in enumerate(((t.rq_steps, t.pubkey_doubling), (t.wb_steps, t.b_doubling))):
            for j in range(STEPS):
                (point, dslope), (partial, _, suffix, slope, inv) = dbl[j], mad[j]
                for k, v in zip(STEP_FIELDS, (point[0], point[1], dslope, partial[0], partial[1], slope, inv, suffix)):
                    value[(0, f[k] + STRIDE * (STEPS * half + j))] = (v, "instance %d half %d step %d %s" % (index, half, j, k))
        for j, (partial, _, suffix, slope, inv) in enumerate(t.zg_steps):
            for k, v in zip(GEN_FIELDS, (partial[0], partial[1], slope, inv, suffix)):
                value[(0, f[k] + GEN_STRIDE * j)] = (v, "instance %d generator step %d %s" % (index, j, k))
        for k, v in zip(SINGLE_FIELDS, (t.r_point_slope, t.r_point_x_diff_inv, t.r_inv, t.w_inv, t.message_inv, x * x % P, t.b_slope, t.b_x_diff_inv)):
            value[(0, f[k])] = (v, "instance %d %s" % (index, k))
        for k, v in enumerate((x, message)):
            value[(1, f["off_pair"][k])] = (begin + 2 * index + k, "instance %d pool address %d" % (index, k))
            value[(1, f["off_pair"][k] + 1)] = (v, "instance %d pool value %d" % (index, k))
        assert set(value) == set(cells)
        for (col, off), (v, what) in value.items():
            assert np.array_equal(got[col][base + off], be.felt(v % P)), what


# ---- 2. what the entry point refuses, what it skips, what it finds
def test_entry_point_refuses_what_it_cannot_serve_skips_what_it_must_not_write_and_reports_what_it_finds(ctx):
    """NULL / zero / oversize arguments, a column beyond ncols, a cell that leaves its block, an odd pool offset, strides of zero and too
    large, NULL points: an error, a message, nothing launched (n_given = 0 does not excuse a NULL pointer).  An instance of the DEVICE
    array whose index is beyond the blocks, or whose input has bit 252 set, is skipped with SS_TRACE_ERR_ECDSA_INSTANCE while its
    neighbour is written.  A wrong r, a zero w and a message with bit 251 are SS_TRACE_ERR_ECDSA_INVALID; a record with y = 0 is
    SS_TRACE_ERR_ECDSA_DIVISOR (the first doubling of the key divides by 2 y; include/sandstorm_hip.h says so).  Through the generators
    each refusal is the host generator's, and the context works afterwards.  (Input errors are reported through status bits: nothing here
    faults the device.)"""
    from sandstorm_amd import hostlib
    from sandstorm_amd._lib import SandstormHipError
    from sandstorm_amd.layouts import starknet as sk
    from test_layout_starknet import real_instances
    lib, h = ctx.lib, ctx.handle
    f = ecdsa_placement()
    n = 4 * BLOCK_ROWS
    z = bt.Zeroed(ctx, 2, n)
    (_, x, message, r, w), other = real_instances()["ecdsa"]
    rec_of = lambda index, values, which=0: bt.records([(index, values[0], key_roots(x)[which]) + tuple(values[1:])])
    good = rec_of(1, (x, message, r, w))
    recs = ctx.alloc(168 * 3).upload(np.concatenate([good, good, good]))
    points = ctx.alloc(252 * 64).upload(curve_points_array())
    L = bt.flat(f, ECDSA_FIELDS)
    call = lambda **kw: lib.ss_trace_ecdsa(*[kw.get(k, v) for k, v in (("ctx", h), ("cols", z.ptrs()), ("ncols", 2), ("col_rows", n), ("layout", L), ("points", points.ptr),
                                                                      ("inst", recs.ptr), ("n_given", 1), ("n_blocks", 4), ("block_rows", BLOCK_ROWS),
                                                                      ("begin", 100), ("pool_addr", z.pool_addr.ptr), ("status", z.status.ptr))])
    relaid = lambda name, value, at=None: dict(layout=bt.flat(bt.changed(f, name, value, at), ECDSA_FIELDS))
    refused = {"NULL context": dict(ctx=None), "NULL columns": dict(cols=None), "NULL columns, nothing given": dict(cols=None, n_given=0),
               "NULL layout, nothing given": dict(layout=None, n_given=0), "NULL instances": dict(inst=None), "NULL pool addresses": dict(pool_addr=None),
               "NULL pool addresses, nothing given": dict(pool_addr=None, n_given=0), "NULL status": dict(status=None),
               "NULL status, nothing given": dict(status=None, n_given=0), "NULL points": dict(points=None), "NULL points, nothing given": dict(points=None, n_given=0),
               "no columns": dict(ncols=0), "too many columns": dict(ncols=17),
               "the pool's column beyond ncols": dict(ncols=1), "the cells' column beyond ncols": relaid("col", 2), "no blocks": dict(n_blocks=0),
               "blocks beyond the columns": dict(n_blocks=5), "columns shorter than the blocks": dict(col_rows=n - 1),
               "huge blocks": dict(n_blocks=1 << 62, block_rows=1 << 62), "empty blocks": dict(block_rows=0), "more instances than blocks": dict(n_given=5),
               "no stride": relaid("row_stride", 0), "a stride that leaves the block": relaid("row_stride", 65),
               "no generator stride": relaid("gen_stride", 0), "a generator stride that leaves the block": relaid("gen_stride", 129),
               "a pair leaves the block": relaid("off_pair", BLOCK_ROWS, 1), "an odd pool offset": relaid("off_pair", f["off_pair"][0] + 1, 0),
               "a NULL column in the table": dict(cols=(C.c_void_p * 2)(z.cols[0].ptr, None))}
    for name in STEP_FIELDS:
        refused["%s leaves the block" % name] = relaid(name, BLOCK_ROWS - 511 * STRIDE)
    for name in GEN_FIELDS:
        refused["%s leaves the block" % name] = relaid(name, BLOCK_ROWS - 255 * GEN_STRIDE)
    for name in SINGLE_FIELDS:
        refused["%s leaves the block" % name] = relaid(name, BLOCK_ROWS)
    for what, kw in refused.items():
        assert call(**kw) != 0, what
        assert lib.ss_last_error(), what
    ctx.sync()
    assert all(not c.any() for c in z.columns()), "a refused call wrote"
    assert call(n_given=0) == 0                                      # nothing given, everything else in order: served, nothing launched
    # skipped: an index beyond the blocks, an input with bit 252 set
    values = (x, message, r, w)
    recs.upload(np.concatenate([rec_of(4, values), good, rec_of(2, (x, message, r | 1 << 252, w))]))
    assert call(n_given=3) == 0
    assert z.read_status()[0] == ERR_ECDSA_INSTANCE
    got = z.columns()
    for c in range(2):
        assert not got[c][:BLOCK_ROWS].any() and not got[c][2 * BLOCK_ROWS:].any(), "column %d: a skipped instance was written" % c
        assert got[c][BLOCK_ROWS:2 * BLOCK_ROWS].any()
    for k in range(5):                                               # bit 252 in each of the five inputs: x, y, message, r, w
        five = [x, key_roots(x)[0], message, r, w]
        five[k] |= 1 << 252
        recs.upload(np.concatenate([bt.records([(3,) + tuple(five)]), good, good]))
        assert ctx.lib.ss_dev_zero(h, z.status.ptr, 64) == 0
        assert call(n_given=1) == 0
        assert z.read_status()[0] == ERR_ECDSA_INSTANCE, "input %d" % k
    assert not z.columns()[0][3 * BLOCK_ROWS:].any()
    # found on the device - block 0's cells outside the instance's own stay untouched
    cells = np.zeros(BLOCK_ROWS, dtype=bool)
    for col, off in ecdsa_cells(f):
        if col == 0:
            cells[off] = True
    found = {"a wrong r": (bt.records([(0, x, key_roots(x)[1], message, r ^ 2, w)]), ERR_ECDSA_INVALID),
             "a zero w": (rec_of(0, (x, message, r, 0)), ERR_ECDSA_INVALID),
             "a message with bit 251": (rec_of(0, (x, message | 1 << 251, r, w)), ERR_ECDSA_INVALID),
             "y = 0": (bt.records([(0, x, 0, message, r, w)]), ERR_ECDSA_DIVISOR)}
    for name, (rec, bit) in found.items():
        recs.upload(np.concatenate([rec, good, good]))
        assert ctx.lib.ss_dev_zero(h, z.status.ptr, 64) == 0
        assert call(n_given=1) == 0, name
        assert z.read_status()[0] == bit, name
        assert not z.columns()[0][:BLOCK_ROWS][~cells].any(), name
        assert not z.columns()[1][:BLOCK_ROWS].any(), name
    z.free()
    recs.free()
    points.free()
    # through the generators: the host generator's message from both, one bad instance per call, nothing counted as traced on the host
    trace_bin, memory_bin, pi = bt.statement("starknet")
    slots = 1 << 17 >> 11
    off_curve = next(v for v in range(2, 100) if sk._sqrt((pow(v, 3, P) + v + sk.CURVE_BETA) % P) is None)
    cases = [([(slots,) + values], "beyond the trace"), ([(3,) + values, (3,) + tuple(other[1:])], "given twice"),
             ([(2,) + values, (5, off_curve, message, r, w)], "the public key is not on the curve"),
             ([(2,) + values, (5, x, message, r ^ 2, w)], "signature is invalid")]
    for rows, message_of in cases:
        with pytest.raises(SandstormHipError, match=message_of):
            hostlib.starknet_base_trace(trace_bin, memory_bin, pi, {"ecdsa": rows})
        with pytest.raises(SandstormHipError, match=message_of):
            bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, {"ecdsa": rows})
        assert hostlib.trace_last_stats()["ecdsa_on_host"] == 0
    # an input >= p keeps the template path (the key's x + p names the same key); the context works after the refusals
    priv = {"ecdsa": [(3,) + values, (6, x + P, message, r, w), (8,) + tuple(other[1:])]}
    got, stats = bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, priv)
    bt.assert_same_columns(got, hostlib.starknet_base_trace(trace_bin, memory_bin, pi, priv))
    assert stats["ecdsa_on_device"] == 2 and stats["ecdsa_on_host"] == 1


# ---- 3. a whole generation with every slot a real instance
_SATURATED = {}


def saturated_input(log_steps):
    """every ECDSA slot a distinct seeded signature, together with the saturated Pedersen, bitwise and Poseidon slots -> (rows, counts)"""
    if log_steps not in _SATURATED:
        from sandstorm_amd import examples
        priv, counts = bt.saturated_input("starknet", log_steps)
        priv["ecdsa"] = examples.seeded_ecdsa_instances(examples.ecdsa_slots(log_steps))
        counts["ecdsa"] = len(priv["ecdsa"])
        _SATURATED[log_steps] = (priv, counts)
    return _SATURATED[log_steps]


def assert_all_on_device(stats, counts):
    for name in ("bitwise", "poseidon", "pedersen", "ecdsa"):
        assert stats[name + "_on_host"] == 0, (name, stats)
        assert stats[name + "_on_device"] == counts.get(name, 0), (name, stats)


def test_saturated_generation_uploads_inputs_not_templates(ctx):
    """the padded starknet statement at 2^17 steps with all 64 ECDSA slots seeded - and the 4096 Pedersen, 2048 bitwise and 4096
    Poseidon slots too -, handed over packed: the host generator accepts every signature and its columns are the device's cell for
    cell; no ECDSA instance traced on the host, 64 on the device; no template more than the bare statement's; the uploads grow by 168
    bytes an instance and the table of 252 points over the run without ECDSA instances (64 KB of slack for the allocation granules, as
    in the neighbouring tests)"""
    from sandstorm_amd import hostlib
    trace_bin, memory_bin, pi = bt.statement("starknet")
    priv, counts = saturated_input(17)
    assert counts["ecdsa"] == 64
    _, bare = bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, None)
    packed = {name: hostlib.pack_instances(name, rows) for name, rows in priv.items()}
    _, without = bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, {name: rows for name, rows in packed.items() if name != "ecdsa"})
    got, stats = bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, packed)
    print("uploads %d B bare, %d B without ECDSA instances, %d B saturated, stats %s" % (bare["bytes_uploaded"], without["bytes_uploaded"], stats["bytes_uploaded"], stats))
    bt.assert_same_columns(got, hostlib.starknet_base_trace(trace_bin, memory_bin, pi, priv))
    assert_all_on_device(bare, {})
    assert_all_on_device(stats, counts)
    assert stats["ecdsa_on_host"] == 0 and stats["ecdsa_on_device"] == 64
    assert stats["templates_uploaded"] == bare["templates_uploaded"]
    assert stats["bytes_uploaded"] <= without["bytes_uploaded"] + 168 * 64 + 252 * 64 + (64 << 10)


# ---- 4. the switch
def test_the_switch_is_off_by_default_and_the_bootloader_run_follows_it(ctx):
    """with the switch off the saturated private input goes the template path: no ECDSA instance on the device, a template per distinct
    signature where the bare statement has the dummy signature's.  With it on, example/bootloader of the reference (starknet layout, 2^17 steps) with the two
    real signatures and the run's own Pedersen instances: cell for cell the host generator's, two ECDSA instances on the device, no
    template more than the run with its Pedersen instances alone"""
    from sandstorm_amd import hostlib
    from test_layout_starknet import real_instances, bootloader_run
    trace_bin, memory_bin, pi = bt.statement("starknet")
    priv, _ = saturated_input(17)
    _, bare = bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, None)
    assert hostlib.trace_ecdsa_on_device(False) is True              # the module's fixture had it on
    try:
        _, off = bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, {"ecdsa": priv["ecdsa"]})
    finally:
        assert hostlib.trace_ecdsa_on_device(True) is False
    assert off["ecdsa_on_device"] == 0 and off["ecdsa_on_host"] == 64
    # (the 64 distinct signatures take the place of the dummy signature's template, which no block holds any more)
    assert off["templates_uploaded"] == bare["templates_uploaded"] - 1 + 64
    g = os.path.join(ROOT, "tests", "golden")
    with gzip.open(os.path.join(g, "bootloader", "trace.bin.gz")) as fh:
        trace_bin = fh.read()
    with gzip.open(os.path.join(g, "bootloader", "memory.bin.gz")) as fh:
        memory_bin = fh.read()
    _, _, pi, own_priv = bootloader_run()
    both = {"ecdsa": real_instances()["ecdsa"], "pedersen": own_priv["pedersen"]}
    got, stats = bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, both)
    bt.assert_same_columns(got, hostlib.starknet_base_trace(trace_bin, memory_bin, pi, both))
    assert stats["ecdsa_on_device"] == 2 and stats["ecdsa_on_host"] == 0
    _, own = bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, {"pedersen": own_priv["pedersen"]})
    assert stats["templates_uploaded"] == own["templates_uploaded"]


# ---- 5. hardware only
@pytest.mark.skipif(EMULATED, reason="a whole starknet proof: hardware only")
def test_saturated_statement_is_proven_from_the_files(ctx):
    """the starknet 2^17-step statement with every ECDSA, bitwise, Poseidon and Pedersen slot filled, through hostlib.prove_files_device
    with the switch on: the C++ verifier and the Python verifier accept the proof at the same query positions, a flipped byte is refused,
    and the bytes are those hostlib.prove writes from the HOST generator's columns"""
    from sandstorm_amd import backend as be, hostlib, verifier
    from sandstorm_amd._lib import SandstormHipError
    from sandstorm_amd.layouts import starknet as sk
    trace_bin, memory_bin, pi = bt.statement("starknet")
    priv, counts = saturated_input(17)
    log_n = 21
    n = 1 << log_n
    dev = [ctx.alloc(32 * n) for _ in range(9)]
    air, seed, build_extension, keep = bt.starknet_prover(ctx, pi, log_n, dev)
    raw, times = hostlib.prove_files_device(ctx, "starknet", trace_bin, memory_bin, pi, priv, dev, air, be.TREE_KECCAK_M20, 0, be.COIN_SOLIDITY, seed, build_extension)
    assert_all_on_device(hostlib.trace_last_stats(), counts)
    assert 0 < times["trace_gen_s"] <= times["total_s"]
    positions = hostlib.verify(air, be.TREE_KECCAK_M20, be.COIN_SOLIDITY, seed, raw)
    assert verifier.verify(raw, sk.verifier_air(pi), be.TREE_KECCAK_M20, be.COIN_SOLIDITY, seed) == positions
    flipped = bytearray(raw)
    flipped[len(raw) // 2] ^= 1
    with pytest.raises(SandstormHipError):
        hostlib.verify(air, be.TREE_KECCAK_M20, be.COIN_SOLIDITY, seed, bytes(flipped))
    want = hostlib.starknet_base_trace(trace_bin, memory_bin, pi, priv)
    for c in range(9):
        dev[c].upload(want[c])
    from_host = hostlib.prove(ctx, air, be.TREE_KECCAK_M20, 0, be.COIN_SOLIDITY, seed, dev, log_n, build_extension, wire=True)
    assert raw == from_host
    for m in keep:
        m.close()
    air.close()
    for d in dev:
        d.free()
