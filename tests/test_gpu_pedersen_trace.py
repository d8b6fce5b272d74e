"""Real Pedersen builtin instances traced ON the device from their two inputs (csrc/trace.hip trace_pedersen_*, behind
ss_trace_pedersen; host/device_trace.hpp DeviceTrace::pedersen) against the C++ host generator (host/trace_{recursive,starknet}.cpp),
bit for bit: the cells are field elements.  The host generator walks an instance's 512 curve steps on a host thread; the device path
used to do the same and upload the result as a 66 KB template per distinct instance.  Here only 72 bytes per instance go up - which
hostlib.trace_last_stats() makes observable, since the cells are the same whichever way they are made.

Runs on the MI355X (`-m gpu`) and, in the CPU suite, on the host build of the device code (tests/test_pedersen_trace_on_host.py)."""
import ctypes as C
import gzip
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
EMULATED = os.environ.get("SS_TEST_HIPEMU") == "1"
EX = os.path.join(ROOT, "tests", "golden", "example")
P = 2**251 + 17 * 2**192 + 1


@pytest.fixture(scope="module")
def ctx():
    from sandstorm_amd import backend as be
    c = be.Context(0)
    yield c
    c.close()


def example_files():
    from sandstorm_amd import public_input
    with open(os.path.join(EX, "trace.bin"), "rb") as f:
        trace_bin = f.read()
    with open(os.path.join(EX, "memory.bin"), "rb") as f:
        memory_bin = f.read()
    pi = public_input.AirPublicInput.from_json(os.path.join(ROOT, "tests", "golden", "air_public_input_array_sum.json"))
    return trace_bin, memory_bin, pi


def padded_statement(layout, log_steps):
    from sandstorm_amd import binary, examples
    states, memory, pi = (examples.starknet_example if layout == "starknet" else examples.recursive_example)(log_steps)
    return binary.write_register_states(states), binary.write_memory(memory), pi


def statement(layout):
    """the smallest statement of each layout the suite has: (files, public input, Pedersen slots)"""
    from sandstorm_amd import examples
    if layout == "recursive":
        return example_files() + (examples.pedersen_slots("recursive", 14),)
    return padded_statement("starknet", 17) + (examples.pedersen_slots("starknet", 17),)


def assert_same_columns(got, want):
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        if not np.array_equal(g, w):
            rows = np.nonzero((g != w).any(axis=1))[0]
            raise AssertionError("column %d differs in %d rows, first %s" % (c, len(rows), rows[:8]))


def device_columns(ctx, layout, trace_bin, memory_bin, pi, priv):
    """-> (the device generator's columns on the host, its stats)"""
    from sandstorm_amd import hostlib
    n = 16 * (len(trace_bin) // 24)
    cols = hostlib.device_base_trace(ctx, layout, trace_bin, memory_bin, pi, priv)
    stats = hostlib.trace_last_stats()
    out = [c.download(np.uint64, (n, 4)) for c in cols]
    for c in cols:
        c.free()
    return out, stats


# ---- 1. the entry point alone
def placement(layout):
    """where the Pedersen section of a layout writes (the `place` lambdas of host/trace_{starknet,recursive}.cpp) as the fields of
    ss_trace_pedersen_layout, with the rows of a block and the number of columns"""
    if layout == "starknet":
        from sandstorm_amd.layouts import starknet as sk
        fields = dict(col_x=sk.COL_PEDERSEN_X, off_x=0, col_y=sk.COL_PEDERSEN_Y, off_y=0, col_suffix=sk.COL_PEDERSEN_SUFFIX, off_suffix=0,
                      col_slope=sk.COL_PEDERSEN_SLOPE, off_slope=0, row_stride=1, col_flag2=sk.COL_PEDERSEN_SLOPE, off_flag2=255,
                      col_flag3=sk.COL_AUXILIARY, off_flag3=71, col_pool=sk.COL_NPC, off_input0=sk.Npc.PEDERSEN_INPUT0_ADDR,
                      off_input1=sk.Npc.PEDERSEN_INPUT1_ADDR, off_output=sk.Npc.PEDERSEN_OUTPUT_ADDR)
        return fields, sk.PEDERSEN_BUILTIN_RATIO * 16, 9
    from sandstorm_amd.layouts import recursive as rec
    fields = dict(col_x=rec.COL_RANGE_CHECK, off_x=1, col_y=rec.COL_RANGE_CHECK, off_y=3, col_suffix=rec.COL_AUXILIARY, off_suffix=0,
                  col_slope=rec.COL_AUXILIARY, off_slope=2, row_stride=4, col_flag2=rec.COL_AUXILIARY, off_flag2=1022,
                  col_flag3=rec.COL_AUXILIARY, off_flag3=7, col_pool=rec.COL_NPC, off_input0=rec.Npc.PEDERSEN_INPUT0_ADDR,
                  off_input1=rec.Npc.PEDERSEN_INPUT1_ADDR, off_output=rec.Npc.PEDERSEN_OUTPUT_ADDR)
    return fields, rec.PEDERSEN_BUILTIN_RATIO * 16, 7


FIELDS = ("col_x", "off_x", "col_y", "off_y", "col_suffix", "off_suffix", "col_slope", "off_slope", "row_stride", "col_flag2", "off_flag2", "col_flag3",
          "off_flag3", "col_pool", "off_input0", "off_input1", "off_output")


def layout_struct(fields):
    return (C.c_uint32 * len(FIELDS))(*[int(fields[k]) for k in FIELDS])


def instance_cells(f):
    """(column, row offset in the block) of every cell the section writes for one instance"""
    cells = set()
    for j in range(512):
        for name in ("x", "y", "suffix", "slope"):
            cells.add((f["col_" + name], f["off_" + name] + f["row_stride"] * j))
    for half in range(2):
        cells.add((f["col_flag2"], f["off_flag2"] + 256 * f["row_stride"] * half))
        cells.add((f["col_flag3"], f["off_flag3"] + 256 * f["row_stride"] * half))
    for off in (f["off_input0"], f["off_input1"], f["off_output"]):
        cells.add((f["col_pool"], off))
        cells.add((f["col_pool"], off + 1))
    return cells


def instance_records(instances):
    rec = np.zeros((len(instances), 9), dtype=np.uint64)
    for k, (index, a, b) in enumerate(instances):
        rec[k, 0] = index
        for j in range(4):
            rec[k, 1 + j] = (a >> (64 * j)) & (2**64 - 1)
            rec[k, 5 + j] = (b >> (64 * j)) & (2**64 - 1)
    return rec


def the_cases():
    """random 250-bit pairs, the values tests/test_layout_recursive.py::test_pedersen_builtin_with_real_instances uses, the dummy instance
    given explicitly, single bits at 0, at the boundary between the two constant-point chains (247 | 248) and at the top"""
    rng = random.Random(1717)
    pairs = [(rng.getrandbits(250), rng.getrandbits(250)) for _ in range(3)]
    pairs += [(P - 1, 2**251 + 2**196), (0, 5), (2**251, 1), (1, 0), (0, 0)]
    pairs += [(1 << 0, 1 << 247), (1 << 247, 1 << 248), (1 << 248, 1 << 251), (1 << 251, 1 << 0)]
    return pairs


class Zeroed:
    """zeroed device columns, the pool's integer addresses and the status block for a call of the entry point alone"""

    def __init__(self, ctx, ncols, n):
        self.ctx, self.n = ctx, n
        self.cols = [ctx.alloc(32 * n) for _ in range(ncols)]
        self.pool_addr = ctx.alloc(4 * (n // 2))
        self.status = ctx.alloc(64)
        for b in self.cols + [self.pool_addr, self.status]:
            assert ctx.lib.ss_dev_zero(ctx.handle, b.ptr, b.nbytes) == 0

    def ptrs(self):
        from sandstorm_amd import backend as be
        return be._ptr_array(self.cols)

    def read_status(self):
        st = (C.c_uint32 * 16)()
        assert self.ctx.lib.ss_trace_status(self.ctx.handle, self.status.ptr, st) == 0
        return list(st)

    def free(self):
        for b in self.cols + [self.pool_addr, self.status]:
            b.free()


@pytest.mark.parametrize("layout", ["recursive", "starknet"])
def test_entry_point_alone_writes_the_generators_cells_and_nothing_else(ctx, layout):
    """ss_trace_pedersen through ctypes into zeroed columns: the given blocks' Pedersen cells are the host generator's for the same
    private input, every other cell is still zero, d_pool_addr holds the three addresses, every output cell is pedersen_hash_host(a, b)"""
    from sandstorm_amd import backend as be, hostlib
    trace_bin, memory_bin, pi, slots = statement(layout)
    n = 16 * (len(trace_bin) // 24)
    f, block_rows, ncols = placement(layout)
    assert slots * block_rows == n
    pairs = the_cases()
    rng = random.Random(5)
    indices = rng.sample(range(slots - 1), len(pairs) - 1) + [slots - 1]          # scattered over the blocks, not in order, the last block among them
    instances = [(i, a, b) for i, (a, b) in zip(indices, pairs)]
    gen = hostlib.starknet_base_trace if layout == "starknet" else hostlib.recursive_base_trace
    want = gen(trace_bin, memory_bin, pi, {"pedersen": instances})
    begin = pi.memory_segments["pedersen"][0]

    z = Zeroed(ctx, ncols, n)
    recs = ctx.alloc(72 * len(instances)).upload(instance_records(instances))
    st = ctx.lib.ss_trace_pedersen(ctx.handle, z.ptrs(), ncols, n, layout_struct(f), recs.ptr, len(instances), slots, block_rows, begin, z.pool_addr.ptr, z.status.ptr)
    assert st == 0, ctx.lib.ss_last_error()
    assert z.read_status()[0] == 0
    got = [c.download(np.uint64, (n, 4)) for c in z.cols]
    pool_addr = z.pool_addr.download(np.uint32, (n // 2,))
    z.free()
    recs.free()

    cells = instance_cells(f)
    assert len(cells) == 2048 + 2 + 6            # 4 x 512 steps (the first flag cells are step 255's slope cells), the second flag cells, three pairs
    mask = [np.zeros(n, dtype=bool) for _ in range(ncols)]
    for index, _, _ in instances:
        for col, off in cells:
            mask[col][index * block_rows + off] = True
    for c in range(ncols):
        assert np.array_equal(got[c][mask[c]], want[c][mask[c]]), "column %d: the instances' cells" % c
        assert not got[c][~mask[c]].any(), "column %d: a cell outside the instances' was written" % c
    want_addr = np.zeros(n // 2, dtype=np.uint32)
    for index, a, b in instances:
        for k, off in enumerate((f["off_input0"], f["off_input1"], f["off_output"])):
            want_addr[(index * block_rows + off) // 2] = begin + 3 * index + k
        out = got[f["col_pool"]][index * block_rows + f["off_output"] + 1]
        assert np.array_equal(out, be.pedersen_hash_host(be.felt(a), be.felt(b))), "instance %d: the output cell is not the hash" % index
    assert np.array_equal(pool_addr, want_addr)


def test_entry_point_refuses_what_it_cannot_serve_and_skips_what_it_must_not_write(ctx):
    """NULL / zero / oversize arguments: an error, a message, nothing written (n_given = 0 does not excuse a NULL column table or layout);
    an instance of the DEVICE array whose index is beyond the blocks, or whose input has a bit from 252 up, is skipped with its error bit"""
    f, block_rows, ncols = placement("starknet")
    n = 4 * block_rows
    z = Zeroed(ctx, ncols, n)
    lib, h = ctx.lib, ctx.handle
    L = layout_struct(f)
    good = instance_records([(1, 3, 4)])
    recs = ctx.alloc(72 * 3).upload(np.concatenate([good, good, good]))
    call = lambda **kw: lib.ss_trace_pedersen(*[kw.get(k, v) for k, v in (("ctx", h), ("cols", z.ptrs()), ("ncols", ncols), ("col_rows", n), ("layout", L),
                                                                         ("inst", recs.ptr), ("n_given", 1), ("n_blocks", 4), ("block_rows", block_rows),
                                                                         ("begin", 100), ("pool_addr", z.pool_addr.ptr), ("status", z.status.ptr))])
    refused = {"NULL context": dict(ctx=None), "NULL columns": dict(cols=None), "NULL columns, nothing given": dict(cols=None, n_given=0),
               "NULL layout, nothing given": dict(layout=None, n_given=0), "NULL instances": dict(inst=None), "NULL pool addresses": dict(pool_addr=None),
               "NULL status": dict(status=None), "no columns": dict(ncols=0), "too many columns": dict(ncols=17), "a column beyond ncols": dict(ncols=5),
               "no blocks": dict(n_blocks=0), "blocks beyond the columns": dict(n_blocks=5), "huge blocks": dict(n_blocks=1 << 62, block_rows=1 << 62),
               "empty blocks": dict(block_rows=0), "more instances than blocks": dict(n_given=5)}
    for off_field in ("off_x", "off_suffix", "off_flag2", "off_flag3", "off_output"):
        refused["%s leaves the block" % off_field] = dict(layout=layout_struct(dict(f, **{off_field: block_rows})))
    refused["a stride that leaves the block"] = dict(layout=layout_struct(dict(f, row_stride=2)))
    refused["no stride"] = dict(layout=layout_struct(dict(f, row_stride=0)))
    nulled = (C.c_void_p * ncols)(*[c.ptr for c in z.cols[:-1]] + [None])
    refused["a NULL column in the table"] = dict(cols=nulled)
    for what, kw in refused.items():
        assert call(**kw) != 0, what
        assert lib.ss_last_error(), what
    ctx.sync()
    assert all(not c.download(np.uint64, (n, 4)).any() for c in z.cols), "a refused call wrote"
    # the device array is the caller's: an index >= n_blocks and an input that is no field element are skipped, the good one is traced
    bad = np.concatenate([instance_records([(4, 1, 2)]), good, instance_records([(2, 1 << 252, 2)])])
    recs.upload(bad)
    assert call(n_given=3) == 0
    st = z.read_status()
    assert st[0] == 16384                                                       # SS_TRACE_ERR_PEDERSEN_INSTANCE
    got = [c.download(np.uint64, (n, 4)) for c in z.cols]
    for c in range(ncols):
        assert not got[c][:block_rows].any() and not got[c][2 * block_rows:].any(), "column %d: a skipped instance was written" % c
    assert got[f["col_x"]][block_rows:2 * block_rows].any()
    z.free()
    recs.free()


# ---- 2. whole generations with every Pedersen slot a real instance
@pytest.mark.parametrize("layout", ["recursive", "starknet"])
def test_saturated_generation_uploads_inputs_not_templates(ctx, layout):
    """the recursive example run (2^14 steps, 128 slots) and the padded starknet statement at 2^17 steps (4096 slots), every Pedersen slot
    a distinct seeded instance: the host generator's columns cell for cell; no instance traced on the host, all on the device; the
    uploads grow by the instances' 72 bytes each (64 KB of slack for the allocation and table granules), not by 66 KB templates"""
    from sandstorm_amd import examples, hostlib
    trace_bin, memory_bin, pi, slots = statement(layout)
    priv = {"pedersen": examples.seeded_pedersen_instances(slots)}
    gen = hostlib.starknet_base_trace if layout == "starknet" else hostlib.recursive_base_trace
    _, bare = device_columns(ctx, layout, trace_bin, memory_bin, pi, None)
    # (the device call takes the instances packed once - hostlib.pack_instances -, the host generator the row list: the same statement)
    got, stats = device_columns(ctx, layout, trace_bin, memory_bin, pi, {"pedersen": hostlib.pack_instances("pedersen", priv["pedersen"])})
    print("%s: %d instances, uploads %d B bare, %d B saturated, stats %s" % (layout, slots, bare["bytes_uploaded"], stats["bytes_uploaded"], stats))
    assert_same_columns(got, gen(trace_bin, memory_bin, pi, priv))
    assert bare["pedersen_on_host"] == 0 and bare["pedersen_on_device"] == 0
    assert stats["pedersen_on_host"] == 0 and stats["pedersen_on_device"] == slots
    assert stats["templates_uploaded"] == bare["templates_uploaded"]
    assert stats["bytes_uploaded"] <= bare["bytes_uploaded"] + 72 * slots + (64 << 10)


# ---- 3. the reference's bootloader run
def test_bootloader_run_traces_its_pedersen_instances_on_the_device(ctx):
    """example/bootloader of the reference (starknet layout, 2^17 steps, two real Pedersen instances) with real instances of the other
    builtins on top: cell for cell; the run's own two Pedersen instances go to the device, the other builtins' still through a template
    per distinct instance"""
    from sandstorm_amd import hostlib
    from test_layout_starknet import real_instances, bootloader_run
    g = os.path.join(ROOT, "tests", "golden")
    with gzip.open(os.path.join(g, "bootloader", "trace.bin.gz")) as f:
        trace_bin = f.read()
    with gzip.open(os.path.join(g, "bootloader", "memory.bin.gz")) as f:
        memory_bin = f.read()
    _, _, pi, priv = bootloader_run()
    assert len(priv["pedersen"]) == 2
    both = dict(real_instances(), pedersen=priv["pedersen"])
    got, stats = device_columns(ctx, "starknet", trace_bin, memory_bin, pi, both)
    assert_same_columns(got, hostlib.starknet_base_trace(trace_bin, memory_bin, pi, both))
    assert stats["pedersen_on_host"] == 0 and stats["pedersen_on_device"] == 2
    # (the run reads its hashes: without its own Pedersen instances it is no valid statement)
    _, own = device_columns(ctx, "starknet", trace_bin, memory_bin, pi, {"pedersen": priv["pedersen"]})
    assert own["pedersen_on_device"] == 2
    assert stats["templates_uploaded"] > own["templates_uploaded"]              # ECDSA, bitwise, EC op, Poseidon: a template per distinct instance
    assert stats["bytes_uploaded"] > own["bytes_uploaded"] + (64 << 10)


# ---- 4. refusals
def test_refusals_are_the_generators(ctx):
    """an index beyond the slots, an index given twice, an input that is not a field element: the host generator's messages from both
    generators, before anything is traced; the context works afterwards"""
    from sandstorm_amd import hostlib
    from sandstorm_amd._lib import SandstormHipError
    trace_bin, memory_bin, pi, slots = statement("recursive")
    for priv, message in (({"pedersen": [(slots, 1, 2)]}, "beyond the trace"), ({"pedersen": [(3, 1, 2), (3, 4, 5)]}, "given twice"),
                          ({"pedersen": [(3, P, 2)]}, "do not end at the hash"), ({"pedersen": [(3, 1, (1 << 256) - 1)]}, "do not end at the hash")):
        with pytest.raises(SandstormHipError, match=message):
            hostlib.recursive_base_trace(trace_bin, memory_bin, pi, priv)
        with pytest.raises(SandstormHipError, match=message):
            device_columns(ctx, "recursive", trace_bin, memory_bin, pi, priv)
        assert hostlib.trace_last_stats()["pedersen_on_device"] == 0
    priv = {"pedersen": [(3, P - 1, 2)]}
    got, stats = device_columns(ctx, "recursive", trace_bin, memory_bin, pi, priv)
    assert_same_columns(got, hostlib.recursive_base_trace(trace_bin, memory_bin, pi, priv))
    assert stats["pedersen_on_device"] == 1


# ---- 5, 6: hardware only
def starknet_prover(ctx, pi, log_n, dev):
    from sandstorm_amd import backend as be, hostlib, public_input
    from sandstorm_amd.layouts import starknet as sk
    air = hostlib.StarknetHostAir(ctx, pi, log_n, 1)
    seed = public_input.public_coin_seed(pi, be.COIN_SOLIDITY)
    keep = []

    def build_extension(challenges):
        keep.append(hostlib.build_extension_columns(ctx, "starknet", [dev[c] for c in (sk.COL_NPC, sk.COL_MEMORY, sk.COL_RANGE_CHECK)], 1 << log_n, challenges))
        return keep[-1].cols
    return air, seed, build_extension, keep


@pytest.mark.skipif(EMULATED, reason="a whole starknet proof: hardware only")
def test_saturated_statement_is_proven_from_the_files(ctx):
    """the saturated starknet 2^17-step statement through hostlib.prove_files_device: the proof is accepted, a flipped byte is not, and
    the bytes are those hostlib.prove writes from the HOST generator's columns of the same statement"""
    from sandstorm_amd import backend as be, examples, hostlib
    from sandstorm_amd._lib import SandstormHipError
    trace_bin, memory_bin, pi, slots = statement("starknet")
    priv = {"pedersen": examples.seeded_pedersen_instances(slots)}
    log_n = 21
    n = 1 << log_n
    dev = [ctx.alloc(32 * n) for _ in range(9)]
    air, seed, build_extension, keep = starknet_prover(ctx, pi, log_n, dev)
    raw, times = hostlib.prove_files_device(ctx, "starknet", trace_bin, memory_bin, pi, priv, dev, air, be.TREE_KECCAK_M20, 0, be.COIN_SOLIDITY, seed, build_extension)
    stats = hostlib.trace_last_stats()
    assert stats["pedersen_on_host"] == 0 and stats["pedersen_on_device"] == slots
    assert 0 < times["trace_gen_s"] <= times["total_s"]
    hostlib.verify(air, be.TREE_KECCAK_M20, be.COIN_SOLIDITY, seed, raw)
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
    """starknet, 2^20 steps, 32768 distinct Pedersen instances: every cell of the 9 columns against the host generator, column by column"""
    from sandstorm_amd import examples, hostlib
    trace_bin, memory_bin, pi = padded_statement("starknet", 20)
    slots = examples.pedersen_slots("starknet", 20)
    assert slots == 32768
    priv = {"pedersen": examples.seeded_pedersen_instances(slots)}
    n = 16 << 20
    cols = hostlib.device_base_trace(ctx, "starknet", trace_bin, memory_bin, pi, priv)
    stats = hostlib.trace_last_stats()
    assert stats["pedersen_on_host"] == 0 and stats["pedersen_on_device"] == slots
    want = hostlib.starknet_base_trace(trace_bin, memory_bin, pi, priv)
    for c, col in enumerate(cols):
        got = col.download(np.uint64, (n, 4))
        assert np.array_equal(got, want[c]), "column %d" % c
        col.free()
        want[c] = None
