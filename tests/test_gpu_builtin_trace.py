"""Real bitwise and Poseidon builtin instances traced ON the device from their inputs (csrc/trace.hip trace_bitwise_kernel /
trace_poseidon_kernel behind ss_trace_bitwise / ss_trace_poseidon; host/device_trace.hpp DeviceTrace::bitwise / ::poseidon) against the
C++ host generator (host/trace_{recursive,starknet}.cpp), bit for bit: the cells are field elements.  The device path used to build a
host trace and upload a template per distinct instance; here 72 / 104 bytes per instance go up - which hostlib.trace_last_stats()
makes observable, since the cells are the same whichever way they are made.

Runs on the MI355X (`-m gpu`) and, in the CPU suite, on the host build of the device code (tests/test_builtin_trace_on_host.py)."""
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
M251 = 2**251 - 1
ERR_BITWISE_INSTANCE, ERR_POSEIDON_INSTANCE = 32768, 65536
CELLS, PAIRS = 1, 2


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
    """the smallest statement of each layout the suite has: the recursive example run (2^14 steps), the padded starknet one (2^17)"""
    return example_files() if layout == "recursive" else padded_statement("starknet", 17)


def log_steps_of(layout):
    return 14 if layout == "recursive" else 17


def host_generator(layout):
    from sandstorm_amd import hostlib
    return hostlib.starknet_base_trace if layout == "starknet" else hostlib.recursive_base_trace


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


class Zeroed:
    """zeroed device columns, the pool's integer addresses and the status block for a call of an entry point alone"""

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

    def columns(self):
        return [c.download(np.uint64, (self.n, 4)) for c in self.cols]

    def free(self):
        for b in self.cols + [self.pool_addr, self.status]:
            b.free()


def records(instances):
    """[(index, v0, v1, ...)] -> the entry points' uint64 records (hostlib.pack_instances makes the same rows)"""
    width = 1 + 4 * (len(instances[0]) - 1)
    rec = np.zeros((len(instances), width), dtype=np.uint64)
    for k, row in enumerate(instances):
        rec[k, 0] = row[0]
        for v, value in enumerate(row[1:]):
            for j in range(4):
                rec[k, 1 + 4 * v + j] = (value >> (64 * j)) & (2**64 - 1)
    return rec


def check_cells(got, want, pool_addr, want_addr, masks):
    for c in range(len(got)):
        assert np.array_equal(got[c][masks[c]], want[c][masks[c]]), "column %d: the instances' cells" % c
        assert not got[c][~masks[c]].any(), "column %d: a cell outside the instances' was written" % c
    assert np.array_equal(pool_addr, want_addr)


# ---- 1. the entry points alone
BITWISE_FIELDS = ("col_diluted", "off_part", "stride_p", "stride_c", "stride_s", "off_shifted", "col_pool", "off_pair")


def bitwise_placement(layout):
    """where the bitwise section of a layout writes (the `place` lambdas of host/trace_{starknet,recursive}.cpp) as the fields of
    ss_trace_bitwise_layout, with the rows of a block and the number of columns"""
    if layout == "starknet":
        from sandstorm_amd.layouts import starknet as sk
        f = dict(col_diluted=sk.COL_RANGE_CHECK, off_part=1, stride_p=256, stride_c=64, stride_s=16, off_shifted=[9, 521, 265, 777], col_pool=sk.COL_NPC,
                 off_pair=[sk.Npc.BITWISE_POOL_ADDR + 256 * k for k in range(4)] + [sk.Npc.BITWISE_X_OR_Y_ADDR])
        return f, sk.BITWISE_RATIO * 16, 9
    from sandstorm_amd.layouts import recursive as rec
    f = dict(col_diluted=rec.COL_DILUTED_UNORDERED, off_part=0, stride_p=32, stride_c=8, stride_s=2, off_shifted=[1, 65, 33, 97], col_pool=rec.COL_NPC,
             off_pair=[rec.Npc.BITWISE_POOL_ADDR + 32 * k for k in range(4)] + [rec.Npc.BITWISE_X_OR_Y_ADDR])
    return f, rec.BITWISE_RATIO * 16, 7


def flat(fields, names):
    out = []
    for k in names:
        out += list(fields[k]) if isinstance(fields[k], (list, tuple)) else [fields[k]]
    return (C.c_uint32 * len(out))(*[int(v) for v in out])


def bitwise_cells(f, what):
    cells = set()
    if what & CELLS:
        cells |= {(f["col_diluted"], f["off_part"] + f["stride_p"] * p + f["stride_c"] * c + f["stride_s"] * sg) for p in range(4) for c in range(4) for sg in range(4)}
        cells |= {(f["col_diluted"], off) for off in f["off_shifted"]}
    if what & PAIRS:
        cells |= {(f["col_pool"], off + j) for off in f["off_pair"] for j in range(2)}
    return cells


def bitwise_cases():
    """seeded 251-bit pairs, the dummy instance given explicitly, x = y, 2^251 - 1 with its complement in 251 bits (zero), a seeded value
    with its complement in 251 bits, single bits at the words' edges and at the top"""
    from sandstorm_amd import examples
    pairs = [(x, y) for _, x, y in examples.seeded_bitwise_instances(3)]
    rng = random.Random(99)
    v = rng.getrandbits(251)
    pairs += [(0, 0), (v, v), (M251, 0), (M251, M251), (v, v ^ M251)]
    bits = (0, 63, 64, 191, 192, 250)
    pairs += [(1 << b, 1 << bits[(k + 1) % len(bits)]) for k, b in enumerate(bits)]
    return pairs


@pytest.mark.parametrize("layout", ["recursive", "starknet"])
def test_bitwise_entry_point_alone_writes_the_generators_cells_and_nothing_else(ctx, layout):
    """ss_trace_bitwise through ctypes into zeroed columns, with the cells-only, the pairs-only and the full mask: the given blocks' cells
    that the mask names are the host generator's for the same private input, every other cell is still zero, d_pool_addr holds the five
    addresses exactly when the pairs are asked for"""
    from sandstorm_amd import examples
    trace_bin, memory_bin, pi = statement(layout)
    n = 16 * (len(trace_bin) // 24)
    f, block_rows, ncols = bitwise_placement(layout)
    slots = examples.bitwise_slots(layout, log_steps_of(layout))
    assert slots * block_rows == n
    pairs = bitwise_cases()
    rng = random.Random(5)
    indices = rng.sample(range(slots - 1), len(pairs) - 1) + [slots - 1]          # scattered over the blocks, not in order, the last block among them
    instances = [(i, x, y) for i, (x, y) in zip(indices, pairs)]
    want = host_generator(layout)(trace_bin, memory_bin, pi, {"bitwise": instances})
    begin = pi.memory_segments["bitwise"][0]
    recs = ctx.alloc(72 * len(instances)).upload(records(instances))
    for what in (CELLS, PAIRS, CELLS | PAIRS):
        z = Zeroed(ctx, ncols, n)
        st = ctx.lib.ss_trace_bitwise(ctx.handle, z.ptrs(), ncols, n, flat(f, BITWISE_FIELDS), recs.ptr, len(instances), slots, block_rows, begin, what,
                                      z.pool_addr.ptr, z.status.ptr)
        assert st == 0, ctx.lib.ss_last_error()
        assert z.read_status()[0] == 0
        got = z.columns()
        pool_addr = z.pool_addr.download(np.uint32, (n // 2,))
        z.free()
        cells = bitwise_cells(f, what)
        assert len(cells) == (68 if what & CELLS else 0) + (10 if what & PAIRS else 0)
        masks = [np.zeros(n, dtype=bool) for _ in range(ncols)]
        want_addr = np.zeros(n // 2, dtype=np.uint32)
        for index, x, y in instances:
            for col, off in cells:
                masks[col][index * block_rows + off] = True
            if what & PAIRS:
                for k, off in enumerate(f["off_pair"]):
                    want_addr[(index * block_rows + off) // 2] = begin + 5 * index + k
        check_cells(got, want, pool_addr, want_addr, masks)
    recs.free()


POSEIDON_FIELDS = ("col_full", "full_stride", "off_full", "off_full_sq", "col_partial", "partial_stride", "off_partial", "off_partial_sq", "n_partial", "col_tail",
                   "tail_stride", "off_tail", "off_tail_sq", "tail_first", "col_pool", "off_pair")


def poseidon_placement():
    """where the starknet layout's Poseidon section writes, as the fields of ss_trace_poseidon_layout"""
    from sandstorm_amd.layouts import starknet as sk
    f = dict(col_full=sk.COL_AUXILIARY, full_stride=64, off_full=[53, 13, 45], off_full_sq=[29, 61, 3], col_partial=sk.COL_RANGE_CHECK, partial_stride=8,
             off_partial=3, off_partial_sq=7, n_partial=64, col_tail=sk.COL_AUXILIARY, tail_stride=16, off_tail=6, off_tail_sq=14, tail_first=61,
             col_pool=sk.COL_NPC, off_pair=[38, 102, 166, 230, 294, 358])
    return f, sk.POSEIDON_RATIO * 16, 9


def poseidon_cells(f):
    cells = {(f["col_full"], f["full_stride"] * r + off) for r in range(8) for off in f["off_full"] + f["off_full_sq"]}
    cells |= {(f["col_partial"], f["partial_stride"] * k + off) for k in range(f["n_partial"]) for off in (f["off_partial"], f["off_partial_sq"])}
    cells |= {(f["col_tail"], f["tail_stride"] * (k - f["tail_first"]) + off) for k in range(f["tail_first"], 83) for off in (f["off_tail"], f["off_tail_sq"])}
    cells |= {(f["col_pool"], off + j) for off in f["off_pair"] for j in range(2)}
    return cells


def round_keys_array():
    """the 91 x 3 round keys as Montgomery felts, from the Python layout's own derivation (what host/air_starknet.cpp derives too)"""
    from sandstorm_amd import backend as be
    from sandstorm_amd.layouts import starknet as sk
    rk = sk.poseidon_round_keys()
    assert len(rk) == 91
    return np.stack([be.felt(int(v)) for row in rk for v in row]).astype(np.uint64)


def poseidon_cases():
    from sandstorm_amd import examples
    from test_layout_starknet import real_instances
    triples = [(0, 0, 0), (P - 1, P - 1, P - 1), (1, 0, 0)]
    triples += [tuple(row[1:]) for row in examples.seeded_poseidon_instances(3)]
    triples += [tuple(row[1:]) for row in real_instances()["poseidon"]]
    return triples


def test_poseidon_entry_point_alone_writes_the_generators_cells_and_nothing_else(ctx):
    """ss_trace_poseidon through ctypes into zeroed columns: the given blocks' cells are the host generator's, every other cell is still
    zero, d_pool_addr holds the six addresses; and the cells are the independent Python mirror's (layouts/starknet.py poseidon_states,
    squares by pow) converted with backend.felt"""
    from sandstorm_amd import backend as be, examples
    from sandstorm_amd.layouts import starknet as sk
    trace_bin, memory_bin, pi = statement("starknet")
    n = 16 * (len(trace_bin) // 24)
    f, block_rows, ncols = poseidon_placement()
    slots = examples.poseidon_slots(17)
    assert slots * block_rows == n
    triples = poseidon_cases()
    rng = random.Random(6)
    indices = rng.sample(range(slots - 1), len(triples) - 1) + [slots - 1]
    instances = [(i,) + t for i, t in zip(indices, triples)]
    want = host_generator("starknet")(trace_bin, memory_bin, pi, {"poseidon": instances})
    begin = pi.memory_segments["poseidon"][0]
    z = Zeroed(ctx, ncols, n)
    recs = ctx.alloc(104 * len(instances)).upload(records(instances))
    keys = ctx.alloc(91 * 3 * 32).upload(round_keys_array())
    st = ctx.lib.ss_trace_poseidon(ctx.handle, z.ptrs(), ncols, n, flat(f, POSEIDON_FIELDS), keys.ptr, recs.ptr, len(instances), slots, block_rows, begin,
                                   z.pool_addr.ptr, z.status.ptr)
    assert st == 0, ctx.lib.ss_last_error()
    assert z.read_status()[0] == 0
    got = z.columns()
    pool_addr = z.pool_addr.download(np.uint32, (n // 2,))
    z.free()
    recs.free()
    keys.free()
    cells = poseidon_cells(f)
    assert len(cells) == 48 + 128 + 44 + 12
    masks = [np.zeros(n, dtype=bool) for _ in range(ncols)]
    want_addr = np.zeros(n // 2, dtype=np.uint32)
    for row in instances:
        for col, off in cells:
            masks[col][row[0] * block_rows + off] = True
        for k, off in enumerate(f["off_pair"]):
            want_addr[(row[0] * block_rows + off) // 2] = begin + 6 * row[0] + k
    check_cells(got, want, pool_addr, want_addr, masks)
    same = lambda col, row, value, what: np.array_equal(got[col][row], be.felt(value % P)) or pytest.fail(what)
    for row in instances:
        base = row[0] * block_rows
        full, partial, out = sk.poseidon_states(row[1:])
        for r in range(8):
            for j in range(3):
                same(f["col_full"], base + 64 * r + f["off_full"][j], full[r][j], "instance %d full round %d state %d" % (row[0], r, j))
                same(f["col_full"], base + 64 * r + f["off_full_sq"][j], pow(full[r][j], 2, P), "instance %d full round %d square %d" % (row[0], r, j))
        for k in range(83):
            if k < 64:
                same(f["col_partial"], base + 8 * k + 3, partial[k], "instance %d partial round %d" % (row[0], k))
                same(f["col_partial"], base + 8 * k + 7, pow(partial[k], 2, P), "instance %d partial round %d square" % (row[0], k))
            if k >= 61:
                same(f["col_tail"], base + 16 * (k - 61) + 6, partial[k], "instance %d partial round %d (tail)" % (row[0], k))
                same(f["col_tail"], base + 16 * (k - 61) + 14, pow(partial[k], 2, P), "instance %d partial round %d square (tail)" % (row[0], k))
        for k in range(3):
            same(f["col_pool"], base + f["off_pair"][k] + 1, row[1 + k], "instance %d input %d" % (row[0], k))
            same(f["col_pool"], base + f["off_pair"][3 + k] + 1, out[k], "instance %d output %d" % (row[0], k))


# ---- 2. what the entry points refuse, and what they skip
def refusals_common(ncols, block_rows):
    return {"NULL context": dict(ctx=None), "NULL columns": dict(cols=None), "NULL columns, nothing given": dict(cols=None, n_given=0),
            "NULL layout, nothing given": dict(layout=None, n_given=0), "NULL instances": dict(inst=None), "NULL pool addresses": dict(pool_addr=None),
            "NULL pool addresses, nothing given": dict(pool_addr=None, n_given=0), "NULL status": dict(status=None), "no columns": dict(ncols=0),
            "too many columns": dict(ncols=17), "a column beyond ncols": dict(ncols=5), "no blocks": dict(n_blocks=0), "blocks beyond the columns": dict(n_blocks=5),
            "columns shorter than the blocks": dict(col_rows=4 * block_rows - 1), "huge blocks": dict(n_blocks=1 << 62, block_rows=1 << 62),
            "empty blocks": dict(block_rows=0), "more instances than blocks": dict(n_given=5)}


def changed(fields, name, value, at=None):
    out = dict(fields)
    if at is None:
        out[name] = value
    else:
        out[name] = list(fields[name])
        out[name][at] = value
    return out


def test_entry_points_refuse_what_they_cannot_serve_and_skip_what_they_must_not_write(ctx):
    """NULL / zero / oversize arguments, a column beyond ncols, a cell that leaves its block, an odd pool offset: an error, a message,
    nothing written (n_given = 0 does not excuse a NULL pointer); an instance of the DEVICE array whose index is beyond the blocks, or
    whose input has bit 252 set, is skipped with the builtin's error bit while its neighbours are written"""
    lib, h = ctx.lib, ctx.handle
    # -- bitwise (the starknet placement; the pool column is column 5, so ncols = 5 leaves it out)
    f, block_rows, ncols = bitwise_placement("starknet")
    n = 4 * block_rows
    z = Zeroed(ctx, ncols, n)
    good = records([(1, 3, 5)])
    recs = ctx.alloc(72 * 3).upload(np.concatenate([good, good, good]))
    L = flat(f, BITWISE_FIELDS)
    call = lambda **kw: lib.ss_trace_bitwise(*[kw.get(k, v) for k, v in (("ctx", h), ("cols", z.ptrs()), ("ncols", ncols), ("col_rows", n), ("layout", L),
                                                                        ("inst", recs.ptr), ("n_given", 1), ("n_blocks", 4), ("block_rows", block_rows),
                                                                        ("begin", 100), ("what", CELLS | PAIRS), ("pool_addr", z.pool_addr.ptr),
                                                                        ("status", z.status.ptr))])
    refused = refusals_common(ncols, block_rows)
    refused.update({"no mask": dict(what=0), "an unknown mask bit": dict(what=4)})
    refused["the parts leave the block"] = dict(layout=flat(changed(f, "off_part", block_rows - 3 * (256 + 64 + 16)), BITWISE_FIELDS))
    refused["a stride that leaves the block"] = dict(layout=flat(changed(f, "stride_p", 512), BITWISE_FIELDS))
    refused["a shifted cell leaves the block"] = dict(layout=flat(changed(f, "off_shifted", block_rows, 2), BITWISE_FIELDS))
    refused["a pair leaves the block"] = dict(layout=flat(changed(f, "off_pair", block_rows, 4), BITWISE_FIELDS))
    refused["an odd pool offset"] = dict(layout=flat(changed(f, "off_pair", 199, 0), BITWISE_FIELDS))
    refused["a NULL column in the table"] = dict(cols=(C.c_void_p * ncols)(*[c.ptr for c in z.cols[:-1]] + [None]))
    for what, kw in refused.items():
        assert call(**kw) != 0, "bitwise: " + what
        assert lib.ss_last_error(), "bitwise: " + what
    ctx.sync()
    assert all(not c.any() for c in z.columns()), "a refused bitwise call wrote"
    recs.upload(np.concatenate([records([(4, 1, 2)]), good, records([(2, 1 << 252, 2)])]))
    assert call(n_given=3) == 0
    assert z.read_status()[0] == ERR_BITWISE_INSTANCE
    got = z.columns()
    for c in range(ncols):
        assert not got[c][:block_rows].any() and not got[c][2 * block_rows:].any(), "column %d: a skipped bitwise instance was written" % c
    assert got[f["col_diluted"]][block_rows:2 * block_rows].any() and got[f["col_pool"]][block_rows:2 * block_rows].any()
    z.free()
    recs.free()
    # -- Poseidon
    f, block_rows, ncols = poseidon_placement()
    n = 4 * block_rows
    z = Zeroed(ctx, ncols, n)
    good = records([(1, 3, 5, 7)])
    recs = ctx.alloc(104 * 3).upload(np.concatenate([good, good, good]))
    keys = ctx.alloc(91 * 3 * 32).upload(round_keys_array())
    L = flat(f, POSEIDON_FIELDS)
    call = lambda **kw: lib.ss_trace_poseidon(*[kw.get(k, v) for k, v in (("ctx", h), ("cols", z.ptrs()), ("ncols", ncols), ("col_rows", n), ("layout", L),
                                                                         ("keys", keys.ptr), ("inst", recs.ptr), ("n_given", 1), ("n_blocks", 4),
                                                                         ("block_rows", block_rows), ("begin", 100), ("pool_addr", z.pool_addr.ptr),
                                                                         ("status", z.status.ptr))])
    refused = refusals_common(ncols, block_rows)
    refused.update({"NULL round keys": dict(keys=None), "NULL round keys, nothing given": dict(keys=None, n_given=0)})
    refused["a full-round cell leaves the block"] = dict(layout=flat(changed(f, "off_full", 64, 1), POSEIDON_FIELDS))
    refused["a full-round square leaves the block"] = dict(layout=flat(changed(f, "off_full_sq", 64, 2), POSEIDON_FIELDS))
    refused["a full-round stride that leaves the block"] = dict(layout=flat(changed(f, "full_stride", 128), POSEIDON_FIELDS))
    refused["a partial-round cell leaves the block"] = dict(layout=flat(changed(f, "off_partial_sq", 8), POSEIDON_FIELDS))
    refused["more partial rounds than there are"] = dict(layout=flat(changed(f, "n_partial", 84), POSEIDON_FIELDS))
    refused["a tail beyond the rounds"] = dict(layout=flat(changed(f, "tail_first", 84), POSEIDON_FIELDS))
    refused["a tail that leaves the block"] = dict(layout=flat(changed(f, "tail_first", 40), POSEIDON_FIELDS))
    refused["a pair leaves the block"] = dict(layout=flat(changed(f, "off_pair", block_rows, 5), POSEIDON_FIELDS))
    refused["an odd pool offset"] = dict(layout=flat(changed(f, "off_pair", 39, 0), POSEIDON_FIELDS))
    refused["a NULL column in the table"] = dict(cols=(C.c_void_p * ncols)(*[c.ptr for c in z.cols[:-1]] + [None]))
    for what, kw in refused.items():
        assert call(**kw) != 0, "poseidon: " + what
        assert lib.ss_last_error(), "poseidon: " + what
    ctx.sync()
    assert all(not c.any() for c in z.columns()), "a refused Poseidon call wrote"
    recs.upload(np.concatenate([records([(4, 1, 2, 3)]), good, records([(2, 1, 2, 1 << 252)])]))
    assert call(n_given=3) == 0
    assert z.read_status()[0] == ERR_POSEIDON_INSTANCE
    got = z.columns()
    for c in range(ncols):
        assert not got[c][:block_rows].any() and not got[c][2 * block_rows:].any(), "column %d: a skipped Poseidon instance was written" % c
    assert got[f["col_full"]][block_rows:2 * block_rows].any() and got[f["col_partial"]][block_rows:2 * block_rows].any()
    z.free()
    recs.free()
    keys.free()


# ---- 3. whole generations with every slot a real instance
def saturated_input(layout, log_steps):
    """every bitwise slot - and, in the starknet layout, every Poseidon and Pedersen slot - a distinct seeded instance -> (rows, counts)"""
    from sandstorm_amd import examples
    priv = {"bitwise": examples.seeded_bitwise_instances(examples.bitwise_slots(layout, log_steps))}
    if layout == "starknet":
        priv["poseidon"] = examples.seeded_poseidon_instances(examples.poseidon_slots(log_steps))
        priv["pedersen"] = examples.seeded_pedersen_instances(examples.pedersen_slots(layout, log_steps))
    return priv, {name: len(rows) for name, rows in priv.items()}


def assert_all_on_device(stats, counts):
    for name in ("bitwise", "poseidon", "pedersen"):
        assert stats[name + "_on_host"] == 0, (name, stats)
        assert stats[name + "_on_device"] == counts.get(name, 0), (name, stats)


@pytest.mark.parametrize("layout", ["recursive", "starknet"])
def test_saturated_generation_uploads_inputs_not_templates(ctx, layout):
    """the recursive example run (2^14 steps, 2048 bitwise slots) and the padded starknet statement at 2^17 steps (2048 bitwise, 4096
    Poseidon and 4096 Pedersen slots, all at once), every slot a distinct seeded instance handed over packed: the host generator's
    columns cell for cell; nothing traced on the host, everything on the device; no template more than the bare statement's; the
    uploads grow by the instances' 72 / 104 / 72 bytes each (64 KB of slack for the allocation granules and the round keys)"""
    from sandstorm_amd import hostlib
    trace_bin, memory_bin, pi = statement(layout)
    priv, counts = saturated_input(layout, log_steps_of(layout))
    _, bare = device_columns(ctx, layout, trace_bin, memory_bin, pi, None)
    packed = {name: hostlib.pack_instances(name, rows) for name, rows in priv.items()}
    got, stats = device_columns(ctx, layout, trace_bin, memory_bin, pi, packed)
    print("%s: %s instances, uploads %d B bare, %d B saturated, stats %s" % (layout, counts, bare["bytes_uploaded"], stats["bytes_uploaded"], stats))
    assert_same_columns(got, host_generator(layout)(trace_bin, memory_bin, pi, priv))
    assert_all_on_device(bare, {})
    assert_all_on_device(stats, counts)
    assert stats["templates_uploaded"] == bare["templates_uploaded"]
    assert stats["bytes_uploaded"] <= bare["bytes_uploaded"] + 72 * counts["bitwise"] + 104 * counts.get("poseidon", 0) + 72 * counts.get("pedersen", 0) + (64 << 10)


# ---- 4. the reference's bootloader run
def test_bootloader_run_traces_its_bitwise_and_poseidon_instances_on_the_device(ctx):
    """example/bootloader of the reference (starknet layout, 2^17 steps) with real instances of every builtin on top: cell for cell; the
    bitwise and Poseidon instances go to the device, and a run given its own Pedersen instances plus those uploads no template more
    than the run without them"""
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
    got, stats = device_columns(ctx, "starknet", trace_bin, memory_bin, pi, both)
    assert_same_columns(got, hostlib.starknet_base_trace(trace_bin, memory_bin, pi, both))
    assert stats["bitwise_on_host"] == 0 and stats["bitwise_on_device"] == len(real["bitwise"])
    assert stats["poseidon_on_host"] == 0 and stats["poseidon_on_device"] == len(real["poseidon"])
    # (the run reads its hashes: without its own Pedersen instances it is no valid statement)
    _, own = device_columns(ctx, "starknet", trace_bin, memory_bin, pi, {"pedersen": priv["pedersen"]})
    with_two = {"pedersen": priv["pedersen"], "bitwise": real["bitwise"], "poseidon": real["poseidon"]}
    got, two = device_columns(ctx, "starknet", trace_bin, memory_bin, pi, with_two)
    assert_same_columns(got, hostlib.starknet_base_trace(trace_bin, memory_bin, pi, with_two))
    assert two["templates_uploaded"] <= own["templates_uploaded"]
    assert two["bitwise_on_device"] == len(real["bitwise"]) and two["poseidon_on_device"] == len(real["poseidon"])


# ---- 5. refusals
def test_refusals_are_the_generators(ctx):
    """an index beyond the slots and an index given twice, for both builtins: the host generator's message from both generators, nothing
    counted as traced, the context usable afterwards.  A Poseidon input >= p keeps the template path: the same columns from both
    generators, counted poseidon_on_host.  A bitwise input with bit 251 set - 2^251 is below p, p - 1 is the largest field element, and
    every input >= p below 2^252 has the bit too - reaches the check of bitwise_instance_trace (its last top segment, shifted by 8, does
    not fit 64 bits): "top segment does not fit" from both generators, before anything is uploaded"""
    from sandstorm_amd import examples, hostlib
    from sandstorm_amd._lib import SandstormHipError
    for layout, name, slots, values in (("recursive", "bitwise", examples.bitwise_slots("recursive", 14), (1, 2)),
                                        ("starknet", "bitwise", examples.bitwise_slots("starknet", 17), (1, 2)),
                                        ("starknet", "poseidon", examples.poseidon_slots(17), (1, 2, 3))):
        trace_bin, memory_bin, pi = statement(layout)
        cases = [({name: [(slots,) + values]}, "beyond the trace"), ({name: [(3,) + values, (3,) + values[::-1]]}, "given twice")]
        if name == "bitwise":
            cases += [({name: [(2, 5, 6), (3, 1 << 251, 2)]}, "top segment does not fit"), ({name: [(3, 1, P - 1)]}, "top segment does not fit"),
                      ({name: [(3, P, 2)]}, "top segment does not fit"), ({name: [(3, 1, (1 << 256) - 1)]}, "top segment does not fit")]
        for priv, message in cases:
            with pytest.raises(SandstormHipError, match=message):
                host_generator(layout)(trace_bin, memory_bin, pi, priv)
            with pytest.raises(SandstormHipError, match=message):
                device_columns(ctx, layout, trace_bin, memory_bin, pi, priv)
            stats = hostlib.trace_last_stats()
            assert stats[name + "_on_device"] == 0 and stats[name + "_on_host"] == 0
        priv = {name: [(3,) + values]}
        got, stats = device_columns(ctx, layout, trace_bin, memory_bin, pi, priv)
        assert_same_columns(got, host_generator(layout)(trace_bin, memory_bin, pi, priv))
        assert stats[name + "_on_device"] == 1 and stats[name + "_on_host"] == 0
    trace_bin, memory_bin, pi = statement("starknet")
    priv = {"poseidon": [(3, 1, P, 2), (4, P - 1, 0, 1), (9, 1, 2, P + 5)]}
    got, stats = device_columns(ctx, "starknet", trace_bin, memory_bin, pi, priv)
    assert_same_columns(got, hostlib.starknet_base_trace(trace_bin, memory_bin, pi, priv))
    assert stats["poseidon_on_host"] == 2 and stats["poseidon_on_device"] == 1


# ---- 6. hardware only
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
    """the starknet 2^17-step statement with every bitwise, Poseidon and Pedersen slot filled, through hostlib.prove_files_device: the
    proof is accepted, a flipped byte is not, and the bytes are those hostlib.prove writes from the HOST generator's columns"""
    from sandstorm_amd import backend as be, hostlib
    from sandstorm_amd._lib import SandstormHipError
    trace_bin, memory_bin, pi = statement("starknet")
    priv, counts = saturated_input("starknet", 17)
    log_n = 21
    n = 1 << log_n
    dev = [ctx.alloc(32 * n) for _ in range(9)]
    air, seed, build_extension, keep = starknet_prover(ctx, pi, log_n, dev)
    raw, times = hostlib.prove_files_device(ctx, "starknet", trace_bin, memory_bin, pi, priv, dev, air, be.TREE_KECCAK_M20, 0, be.COIN_SOLIDITY, seed, build_extension)
    assert_all_on_device(hostlib.trace_last_stats(), counts)
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
@pytest.mark.parametrize("layout", ["starknet", "recursive"])
def test_saturated_columns_at_2p20_steps(ctx, layout):
    """2^20 steps: starknet with 16384 bitwise, 32768 Poseidon and 32768 Pedersen instances, recursive with all 131072 bitwise slots
    filled - every cell of every column against the host generator, column by column"""
    from sandstorm_amd import hostlib
    trace_bin, memory_bin, pi = padded_statement(layout, 20)
    priv, counts = saturated_input(layout, 20)
    assert counts["bitwise"] == (16384 if layout == "starknet" else 131072)
    n = 16 << 20
    packed = {name: hostlib.pack_instances(name, rows) for name, rows in priv.items()}
    cols = hostlib.device_base_trace(ctx, layout, trace_bin, memory_bin, pi, packed)
    assert_all_on_device(hostlib.trace_last_stats(), counts)
    want = host_generator(layout)(trace_bin, memory_bin, pi, packed)
    for c, col in enumerate(cols):
        got = col.download(np.uint64, (n, 4))
        assert np.array_equal(got, want[c]), "column %d" % c
        col.free()
        want[c] = None
