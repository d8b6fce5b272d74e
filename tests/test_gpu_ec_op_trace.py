"""Real EC-op builtin instances traced ON the device from their inputs (csrc/trace.hip trace_ec_op_kernel behind ss_trace_ec_op;
host/device_trace.hpp DeviceTrace::ec_op) against the C++ host generator (host/trace_starknet.cpp) and the Python mirror
(layouts/starknet.py EcOpInstanceTrace), bit for bit: the cells are field elements.  The device path used to run the doubling chain and
the multiply-add chain on the host and upload a 66 KB template per distinct instance; here 168 bytes per instance go up - which
hostlib.trace_last_stats() makes observable, since the cells are the same whichever way they are made.  ECDSA instances keep their
templates.

Runs on the MI355X (`-m gpu`) and, in the CPU suite, on the host build of the device code (tests/test_ec_op_trace_on_host.py)."""
import ctypes as C
import gzip
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_gpu_builtin_trace as bt          # noqa: E402  (its helpers: the statements, zeroed device columns, packed records, column comparison)

pytestmark = pytest.mark.gpu
EMULATED = os.environ.get("SS_TEST_HIPEMU") == "1"
P = 2**251 + 17 * 2**192 + 1
ERR_EC_OP_INSTANCE, ERR_EC_OP_DIVISOR, ERR_EC_OP_MEETS = 131072, 262144, 524288
BLOCK_ROWS, STEPS, STRIDE = 16384, 256, 64
SENTINEL = 0xa5a5a5a5a5a5a5a5                 # in all four limbs: no field element, and nothing the kernels make
ADDR_SENTINEL = 0xdeadbeef
EC_OP_FIELDS = ("col", "row_stride", "off_dbl_x", "off_dbl_y", "off_dbl_slope", "off_sum_x", "off_sum_y", "off_suffix", "off_slope", "off_x_diff_inv",
                "off_flag2", "off_flag3", "col_pool", "off_pair")


@pytest.fixture(scope="module")
def ctx():
    from sandstorm_amd import backend as be
    c = be.Context(0)
    yield c
    c.close()


def ec_op_placement(col=0, col_pool=1):
    """where the starknet layout's EC-op section writes (the `place` lambda of host/trace_starknet.cpp) as the fields of
    ss_trace_ec_op_layout, for a column table that holds the auxiliary column at `col` and the memory pool at `col_pool`"""
    from sandstorm_amd.layouts import starknet as sk
    E, N = sk.EcOp, sk.Npc
    return dict(col=col, row_stride=STRIDE, off_dbl_x=E.Q_DOUBLING_X, off_dbl_y=E.Q_DOUBLING_Y, off_dbl_slope=E.Q_DOUBLING_SLOPE, off_sum_x=E.R_PARTIAL_SUM_X,
                off_sum_y=E.R_PARTIAL_SUM_Y, off_suffix=E.M_SUFFIX, off_slope=E.R_PARTIAL_SUM_SLOPE, off_x_diff_inv=E.R_PARTIAL_SUM_X_DIFF_INV,
                off_flag2=E.M_BIT251_AND_BIT196, off_flag3=E.M_BIT251_AND_BIT196_AND_BIT192, col_pool=col_pool,
                off_pair=[N.EC_OP_P_X_ADDR, N.EC_OP_P_Y_ADDR, N.EC_OP_Q_X_ADDR, N.EC_OP_Q_Y_ADDR, N.EC_OP_M_ADDR, N.EC_OP_R_X_ADDR, N.EC_OP_R_Y_ADDR])


def ec_op_cells(f):
    """the (column, row offset) cells of one instance: six per step, the chord's slope and the x-difference's inverse for steps 0 .. 254
    only, the two flags, the seven pairs"""
    every = ("off_dbl_x", "off_dbl_y", "off_dbl_slope", "off_sum_x", "off_sum_y", "off_suffix")
    cells = {(f["col"], f[k] + STRIDE * j) for k in every for j in range(STEPS)}
    cells |= {(f["col"], f[k] + STRIDE * j) for k in ("off_slope", "off_x_diff_inv") for j in range(STEPS - 1)}
    cells |= {(f["col"], f["off_flag2"]), (f["col"], f["off_flag3"])}
    cells |= {(f["col_pool"], off + j) for off in f["off_pair"] for j in range(2)}
    return cells


class Prefilled(bt.Zeroed):
    """device columns and pool addresses that hold a sentinel everywhere, and a zeroed status block"""

    def __init__(self, ctx, ncols, n):
        super().__init__(ctx, ncols, n)
        fill = np.full((n, 4), SENTINEL, dtype=np.uint64)
        for c in self.cols:
            c.upload(fill)
        self.pool_addr.upload(np.full(n // 2, ADDR_SENTINEL, dtype=np.uint32))


def call_ec_op(ctx, z, f, recs, n_given, n_blocks, begin, ncols=2):
    return ctx.lib.ss_trace_ec_op(ctx.handle, z.ptrs(), ncols, z.n, bt.flat(f, EC_OP_FIELDS), recs.ptr, n_given, n_blocks, BLOCK_ROWS, begin, z.pool_addr.ptr,
                                  z.status.ptr)


def entry_point_instances():
    """the six EC-op instances of test_layout_starknet.real_instances() - scalars 1, 3, 2^250 - 1, the bit-251/196/192 pattern, random -
    and, in the two blocks they leave free below 12, m = 0 (no addition at all) and m = 2^251 alone"""
    from sandstorm_amd.layouts import starknet as sk
    from test_layout_starknet import real_instances
    rows = list(real_instances()["ec_op"])
    assert sorted(r[0] for r in rows) == [0, 2, 3, 6, 7, 9]
    p11, q13 = sk._ec_mul(11, sk.GENERATOR), sk._ec_mul(13, sk.GENERATOR)
    return rows + [(10, p11[0], p11[1], q13[0], q13[1], 0), (11, q13[0], q13[1], p11[0], p11[1], 1 << 251)]


# ---- 1. the entry point alone
def test_ec_op_entry_point_alone_writes_the_generators_cells_and_nothing_else(ctx):
    """ss_trace_ec_op through ctypes into two columns (auxiliary, pool) of 12 blocks that hold a sentinel: every cell the host
    generator's EC-op section places holds the host generator's value and the Python mirror's; every other cell - step 255's slope and
    x-difference cells among them - still holds the sentinel; d_pool_addr holds the seven addresses and the sentinel elsewhere"""
    from sandstorm_amd import backend as be, hostlib
    from sandstorm_amd.layouts import starknet as sk
    trace_bin, memory_bin, pi = bt.statement("starknet")
    n_blocks = 12
    n = n_blocks * BLOCK_ROWS
    f = ec_op_placement()
    instances = entry_point_instances()
    want_all = hostlib.starknet_base_trace(trace_bin, memory_bin, pi, {"ec_op": instances})
    want = [want_all[sk.COL_AUXILIARY][:n], want_all[sk.COL_NPC][:n]]
    begin = pi.memory_segments["ec_op"][0]
    z = Prefilled(ctx, 2, n)
    recs = ctx.alloc(168 * len(instances)).upload(bt.records(instances))
    st = call_ec_op(ctx, z, f, recs, len(instances), n_blocks, begin)
    assert st == 0, ctx.lib.ss_last_error()
    assert z.read_status()[0] == 0
    got = z.columns()
    pool_addr = z.pool_addr.download(np.uint32, (n // 2,))
    z.free()
    recs.free()
    cells = ec_op_cells(f)
    assert len(cells) == 6 * 256 + 2 * 255 + 2 + 14
    for k in ("off_slope", "off_x_diff_inv"):
        assert (f["col"], f[k] + STRIDE * 255) not in cells
    masks = [np.zeros(n, dtype=bool) for _ in range(2)]
    want_addr = np.full(n // 2, ADDR_SENTINEL, dtype=np.uint32)
    for row in instances:
        for col, off in cells:
            masks[col][row[0] * BLOCK_ROWS + off] = True
        for k, off in enumerate(f["off_pair"]):
            want_addr[(row[0] * BLOCK_ROWS + off) // 2] = begin + 7 * row[0] + k
    for c in range(2):
        assert np.array_equal(got[c][masks[c]], want[c][masks[c]]), "column %d: the instances' cells" % c
        assert (got[c][~masks[c]] == np.uint64(SENTINEL)).all(), "column %d: a cell outside the instances' was written" % c
    assert np.array_equal(pool_addr, want_addr)
    # the Python mirror, converted with backend.felt
    same = lambda col, row, value, what: np.array_equal(got[col][row], be.felt(value % P)) or pytest.fail(what)
    for index, px, py, qx, qy, m in instances:
        t = sk.EcOpInstanceTrace((px, py), (qx, qy), m)
        base = index * BLOCK_ROWS
        for j in range(STEPS):
            r = base + STRIDE * j
            (dx, dy), dslope = t.q_doubling[j]
            (sx, sy), _, suffix, slope, x_diff_inv = t.r_steps[j]
            what = "instance %d step %d: " % (index, j)
            same(0, r + f["off_dbl_x"], dx, what + "doubling x"); same(0, r + f["off_dbl_y"], dy, what + "doubling y")
            same(0, r + f["off_dbl_slope"], dslope, what + "tangent's slope")
            same(0, r + f["off_sum_x"], sx, what + "partial sum x"); same(0, r + f["off_sum_y"], sy, what + "partial sum y")
            same(0, r + f["off_suffix"], suffix, what + "suffix")
            if j != STEPS - 1:
                same(0, r + f["off_slope"], slope, what + "chord's slope"); same(0, r + f["off_x_diff_inv"], x_diff_inv, what + "x-difference's inverse")
        same(0, base + f["off_flag2"], t.bit251_and_bit196, "instance %d flag 251 & 196" % index)
        same(0, base + f["off_flag3"], t.bit251_and_bit196_and_bit192, "instance %d flag 251 & 196 & 192" % index)
        for k, v in enumerate((px, py, qx, qy, m, t.r[0], t.r[1])):
            same(1, base + f["off_pair"][k] + 1, v, "instance %d pool value %d" % (index, k))
            same(1, base + f["off_pair"][k], begin + 7 * index + k, "instance %d pool address %d" % (index, k))


# ---- 2. what the entry point refuses, what it skips, what it finds
def bad_instances():
    """-> {name: ((p, q, m), the host generator's message)}: Q with y = 0 (a doubling divides by zero); P = 2 Q with m = 2 (the partial sum
    meets 2 Q at step 1, having passed step 0 on a clear bit) and with m = 4 (the same meeting, at a step whose own bit is clear too: no
    addition ever looks at that difference); P = Q with m = 1 (meets at step 0)"""
    from sandstorm_amd.layouts import starknet as sk
    p5, q7 = sk._ec_mul(5, sk.GENERATOR), sk._ec_mul(7, sk.GENERATOR)
    return {"divisor": ((p5, (q7[0], 0), 5), "a curve step divides by zero", ERR_EC_OP_DIVISOR),
            "meets at step 1": ((sk._ec_mul(14, sk.GENERATOR), q7, 2), "a partial sum meets the fixed point", ERR_EC_OP_MEETS),
            "meets at step 1, bit clear": ((sk._ec_mul(14, sk.GENERATOR), q7, 4), "a partial sum meets the fixed point", ERR_EC_OP_MEETS),
            "meets at step 0": ((q7, q7, 1), "a partial sum meets the fixed point", ERR_EC_OP_MEETS)}


def test_entry_point_refuses_what_it_cannot_serve_skips_what_it_must_not_write_and_reports_what_it_finds(ctx):
    """NULL / zero / oversize arguments, a column beyond ncols, a cell that leaves its block, an odd pool offset: an error, a message,
    nothing launched (n_given = 0 does not excuse a NULL pointer).  An instance of the DEVICE array whose index is beyond the blocks, or
    whose input has bit 252 set, is skipped with SS_TRACE_ERR_EC_OP_INSTANCE while its neighbour is written.  A doubling whose y is
    zero and a partial sum that meets its step's point set their status bits; through device_base_trace each is the host generator's
    refusal, and the context works afterwards.  (Input errors reported through status bits: nothing here faults the device.)"""
    from sandstorm_amd import hostlib
    from sandstorm_amd._lib import SandstormHipError
    from sandstorm_amd.layouts import starknet as sk
    lib, h = ctx.lib, ctx.handle
    f = ec_op_placement()
    n = 4 * BLOCK_ROWS
    z = bt.Zeroed(ctx, 2, n)
    p5, q7 = sk._ec_mul(5, sk.GENERATOR), sk._ec_mul(7, sk.GENERATOR)
    good = bt.records([(1,) + p5 + q7 + (5,)])
    recs = ctx.alloc(168 * 3).upload(np.concatenate([good, good, good]))
    L = bt.flat(f, EC_OP_FIELDS)
    call = lambda **kw: lib.ss_trace_ec_op(*[kw.get(k, v) for k, v in (("ctx", h), ("cols", z.ptrs()), ("ncols", 2), ("col_rows", n), ("layout", L),
                                                                      ("inst", recs.ptr), ("n_given", 1), ("n_blocks", 4), ("block_rows", BLOCK_ROWS),
                                                                      ("begin", 100), ("pool_addr", z.pool_addr.ptr), ("status", z.status.ptr))])
    relaid = lambda name, value, at=None: dict(layout=bt.flat(bt.changed(f, name, value, at), EC_OP_FIELDS))
    refused = {"NULL context": dict(ctx=None), "NULL columns": dict(cols=None), "NULL columns, nothing given": dict(cols=None, n_given=0),
               "NULL layout, nothing given": dict(layout=None, n_given=0), "NULL instances": dict(inst=None), "NULL pool addresses": dict(pool_addr=None),
               "NULL pool addresses, nothing given": dict(pool_addr=None, n_given=0), "NULL status": dict(status=None),
               "NULL status, nothing given": dict(status=None, n_given=0), "no columns": dict(ncols=0), "too many columns": dict(ncols=17),
               "the pool's column beyond ncols": dict(ncols=1), "the cells' column beyond ncols": relaid("col", 2), "no blocks": dict(n_blocks=0),
               "blocks beyond the columns": dict(n_blocks=5), "columns shorter than the blocks": dict(col_rows=n - 1),
               "huge blocks": dict(n_blocks=1 << 62, block_rows=1 << 62), "empty blocks": dict(block_rows=0), "more instances than blocks": dict(n_given=5),
               "no stride": relaid("row_stride", 0), "a stride that leaves the block": relaid("row_stride", 65),
               "a pair leaves the block": relaid("off_pair", BLOCK_ROWS, 6), "an odd pool offset": relaid("off_pair", f["off_pair"][3] + 1, 3),
               "a flag leaves the block": relaid("off_flag3", BLOCK_ROWS),
               "a NULL column in the table": dict(cols=(C.c_void_p * 2)(z.cols[0].ptr, None))}
    for name in EC_OP_FIELDS[2:10]:
        refused["%s leaves the block" % name] = relaid(name, BLOCK_ROWS - 255 * STRIDE)
    for what, kw in refused.items():
        assert call(**kw) != 0, what
        assert lib.ss_last_error(), what
    ctx.sync()
    assert all(not c.any() for c in z.columns()), "a refused call wrote"
    assert call(n_given=0) == 0                                      # nothing given, everything else in order: served, nothing launched
    # skipped: an index beyond the blocks, an input with bit 252 set
    recs.upload(np.concatenate([bt.records([(4,) + p5 + q7 + (5,)]), good, bt.records([(2,) + p5 + (q7[0], q7[1] | 1 << 252, 5)])]))
    assert call(n_given=3) == 0
    assert z.read_status()[0] == ERR_EC_OP_INSTANCE
    got = z.columns()
    for c in range(2):
        assert not got[c][:BLOCK_ROWS].any() and not got[c][2 * BLOCK_ROWS:].any(), "column %d: a skipped instance was written" % c
        assert got[c][BLOCK_ROWS:2 * BLOCK_ROWS].any()
    for k in range(5):                                               # bit 252 in each of the five inputs
        values = list(p5 + q7 + (5,))
        values[k] |= 1 << 252
        recs.upload(np.concatenate([bt.records([(3,) + tuple(values)]), good, good]))
        assert ctx.lib.ss_dev_zero(h, z.status.ptr, 64) == 0
        assert call(n_given=1) == 0
        assert z.read_status()[0] == ERR_EC_OP_INSTANCE, "input %d" % k
    assert not z.columns()[0][3 * BLOCK_ROWS:].any()
    # found on the device: the divisor, the meetings - block 0's cells outside the instance's own stay untouched
    cells = np.zeros(n, dtype=bool)
    for col, off in ec_op_cells(f):
        if col == 0:
            cells[off] = True
    for name, ((p, q, m), _, bit) in bad_instances().items():
        recs.upload(np.concatenate([bt.records([(0,) + p + q + (m,)]), good, good]))
        assert ctx.lib.ss_dev_zero(h, z.status.ptr, 64) == 0
        assert call(n_given=1) == 0, name
        assert z.read_status()[0] == bit, name
        assert not z.columns()[0][:BLOCK_ROWS][~cells[:BLOCK_ROWS]].any(), name
    z.free()
    recs.free()
    # through the generators: the host generator's message from both, one bad instance per call, nothing counted as traced on the device
    trace_bin, memory_bin, pi = bt.statement("starknet")
    slots = 1 << 17 >> 10
    cases = [([(slots,) + p5 + q7 + (5,)], "beyond the trace"), ([(3,) + p5 + q7 + (5,), (3,) + q7 + p5 + (6,)], "given twice")]
    cases += [([(2,) + p5 + q7 + (9,), (5,) + p + q + (m,)], message) for (p, q, m), message, _ in bad_instances().values()]
    for rows, message in cases:
        with pytest.raises(SandstormHipError, match=message):
            hostlib.starknet_base_trace(trace_bin, memory_bin, pi, {"ec_op": rows})
        with pytest.raises(SandstormHipError, match=message):
            bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, {"ec_op": rows})
        assert hostlib.trace_last_stats()["ec_op_on_host"] == 0
    # an input >= p keeps the template path; the context works after the refusals
    priv = {"ec_op": [(3,) + p5 + q7 + (5,), (4,) + p5 + q7 + (P + 5,), (8, p5[0] + P) + p5[1:] + q7 + (6,)]}
    got, stats = bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, priv)
    bt.assert_same_columns(got, hostlib.starknet_base_trace(trace_bin, memory_bin, pi, priv))
    assert stats["ec_op_on_device"] == 1 and stats["ec_op_on_host"] == 2


# ---- 3. a whole generation with every slot a real instance
def saturated_input(log_steps):
    """every EC-op slot a distinct seeded instance, together with the saturated Pedersen, bitwise and Poseidon slots -> (rows, counts)"""
    from sandstorm_amd import examples
    priv, counts = bt.saturated_input("starknet", log_steps)
    priv["ec_op"] = examples.seeded_ec_op_instances(examples.ec_op_slots(log_steps))
    counts["ec_op"] = len(priv["ec_op"])
    return priv, counts


def assert_all_on_device(stats, counts):
    for name in ("bitwise", "poseidon", "pedersen", "ec_op"):
        assert stats[name + "_on_host"] == 0, (name, stats)
        assert stats[name + "_on_device"] == counts.get(name, 0), (name, stats)


def test_saturated_generation_uploads_inputs_not_templates(ctx):
    """the padded starknet statement at 2^17 steps with all 128 EC-op slots seeded - and the 4096 Pedersen, 2048 bitwise and 4096
    Poseidon slots too -, handed over packed: the host generator accepts every instance and its columns are the device's cell for cell;
    no EC-op instance traced on the host, 128 on the device; no template more than the bare statement's; the uploads grow by 168 bytes
    an instance over the run without EC-op instances (64 KB of slack for the allocation granules, as in the neighbouring tests)"""
    from sandstorm_amd import hostlib
    trace_bin, memory_bin, pi = bt.statement("starknet")
    priv, counts = saturated_input(17)
    assert counts["ec_op"] == 128
    _, bare = bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, None)
    packed = {name: hostlib.pack_instances(name, rows) for name, rows in priv.items()}
    _, without = bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, {name: rows for name, rows in packed.items() if name != "ec_op"})
    got, stats = bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, packed)
    print("uploads %d B bare, %d B without EC-op instances, %d B saturated, stats %s" % (bare["bytes_uploaded"], without["bytes_uploaded"], stats["bytes_uploaded"], stats))
    bt.assert_same_columns(got, hostlib.starknet_base_trace(trace_bin, memory_bin, pi, priv))
    assert_all_on_device(bare, {})
    assert_all_on_device(stats, counts)
    assert stats["ec_op_on_host"] == 0 and stats["ec_op_on_device"] == 128
    assert stats["templates_uploaded"] == bare["templates_uploaded"]
    assert stats["bytes_uploaded"] <= without["bytes_uploaded"] + 168 * 128 + (64 << 10)


# ---- 4. the reference's bootloader run
def test_bootloader_run_traces_its_ec_op_instances_on_the_device_and_keeps_the_ecdsa_templates(ctx):
    """example/bootloader of the reference (starknet layout, 2^17 steps) with real instances of every builtin on top: cell for cell; the
    six EC-op instances go to the device; the two ECDSA instances keep their templates, so the run uploads more templates than the run
    with its own Pedersen instances alone"""
    from sandstorm_amd import hostlib
    from test_layout_starknet import real_instances, bootloader_run
    g = os.path.join(ROOT, "tests", "golden")
    with gzip.open(os.path.join(g, "bootloader", "trace.bin.gz")) as f:
        trace_bin = f.read()
    with gzip.open(os.path.join(g, "bootloader", "memory.bin.gz")) as f:
        memory_bin = f.read()
    _, _, pi, priv = bootloader_run()
    real = real_instances()
    both = dict(real, pedersen=priv["pedersen"])
    got, stats = bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, both)
    bt.assert_same_columns(got, hostlib.starknet_base_trace(trace_bin, memory_bin, pi, both))
    assert stats["ec_op_on_host"] == 0 and stats["ec_op_on_device"] == len(real["ec_op"]) == 6
    _, own = bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, {"pedersen": priv["pedersen"]})
    assert stats["templates_uploaded"] > own["templates_uploaded"]
    # without the ECDSA instances nothing is left that needs a template of its own
    rest = {name: rows for name, rows in both.items() if name != "ecdsa"}
    got, two = bt.device_columns(ctx, "starknet", trace_bin, memory_bin, pi, rest)
    bt.assert_same_columns(got, hostlib.starknet_base_trace(trace_bin, memory_bin, pi, rest))
    assert two["templates_uploaded"] == own["templates_uploaded"] and two["ec_op_on_device"] == 6


# ---- 5, 6. hardware only
@pytest.mark.skipif(EMULATED, reason="a whole starknet proof: hardware only")
def test_saturated_statement_is_proven_from_the_files(ctx):
    """the starknet 2^17-step statement with every EC-op, bitwise, Poseidon and Pedersen slot filled, through hostlib.prove_files_device:
    the C++ verifier and the Python verifier accept the proof at the same query positions, a flipped byte is refused, and the bytes are
    those hostlib.prove writes from the HOST generator's columns"""
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


@pytest.mark.skipif(EMULATED, reason="the bench's size: hardware only")
def test_saturated_columns_at_2p20_steps(ctx):
    """2^20 steps with all 1024 EC-op slots filled (and the 16384 bitwise, 32768 Poseidon and 32768 Pedersen slots): every cell of every
    column against the host generator, column by column"""
    from sandstorm_amd import hostlib
    trace_bin, memory_bin, pi = bt.padded_statement("starknet", 20)
    priv, counts = saturated_input(20)
    assert counts["ec_op"] == 1024
    n = 16 << 20
    packed = {name: hostlib.pack_instances(name, rows) for name, rows in priv.items()}
    cols = hostlib.device_base_trace(ctx, "starknet", trace_bin, memory_bin, pi, packed)
    assert_all_on_device(hostlib.trace_last_stats(), counts)
    want = hostlib.starknet_base_trace(trace_bin, memory_bin, pi, packed)
    for c, col in enumerate(cols):
        got = col.download(np.uint64, (n, 4))
        assert np.array_equal(got, want[c]), "column %d" % c
        col.free()
        want[c] = None
