"""The base-trace kernels of csrc/trace.hip, each entry point ALONE through the C ABI (ss_trace_memory_image, _cpu_cells, _builtin,
_rc_pool, _rc_builtin, _ordered_runs, _patch, _ordered_memory) against references written here in Python integers mod p, from what
include/sandstorm_hip.h documents - not against the C++ host generator, which tests/test_gpu_device_trace.py does, on runs whose
cycles are almost all the idle `jmp rel 0`.  Here every instruction form is traced (2 304 of them, shuffled over 18 workgroups), with
operands from the top of the field, every input-error bit is provoked, and the ordered memory is driven through its LDS table's
collisions, its chunked prefix sums and its gap bookkeeping.  Every comparison is exact; output buffers start as all ones and the
cells a call does not own must still be all ones afterwards.

Checked against deliberately wrong kernels (scratch copies of the host build of the device code; what failed):
  res = fp_add for res_logic mul; the op0 * op1 cell = fp_add; rec[c ^ 1] for rec[c]; the jnz inverse of -dst
        -> every_instruction_form (all tables and sizes; -dst from 127 cycles on), both status-bit tests
           (+ test_gpu_device_trace.py::test_columns_of_the_synthetic_run, both layouts, for the first three)
  status_error(.., cyc + 1)                      -> both status-bit tests
  the image kernel drops its last record         -> memory_image[1, 255, 256, 257]
  tmpl_of_block[0] for [i]; addr_mult * (i + 1)  -> builtin_templates (7 and 300 cells, 5 and 1000 blocks; all nine)
  padding index h for pad0 + h                   -> rc_pool[pad0 > 0, pad0 beyond the padding]
  part k for part 7 - k                          -> rc_builtin (all six)
  k > first[0] for >=; a dilution mask bit lost  -> ordered_runs (all three; 300 and 65536)
  rows[k] <= col_rows                            -> patch
  the LDS table's fallback counts once           -> ordered_memory_valid[n = 2^13, n = 2^15] (dropped altogether, the wrong kernel reads out of
                                                    bounds at n = 2^13)
  TRACE_ST_GAPS not subtracted                   -> every ordered-memory case with a gap (+ the synthetic run)
  one chunk sum of the prefix scan off by one    -> ordered_memory_valid[n = 2^15]
(`k > first[n_values]` for `>=` in run_value changes nothing: the run search returns the last value there too.)

Runs on the MI355X (`-m gpu`) and, in the CPU suite, on the host build of the device code (tests/test_device_code_on_host.py)."""
import ctypes as C
import os
import random
import sys
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import edge_values as ev                                         # noqa: E402

pytestmark = pytest.mark.gpu
P = 2**251 + 17 * 2**192 + 1
M64 = 1 << 64
ONES = np.uint64(M64 - 1)
# include/sandstorm_hip.h
NPC_PAD, NPC_PUBLIC, NPC_PC, NPC_OP0, NPC_DST, NPC_OP1 = range(6)
RC_FILL, RC_ZERO, RC_OFF_DST, RC_OFF_OP0, RC_OFF_OP1 = range(5)
AUX_ZERO, AUX_AP, AUX_FP, AUX_TMP0, AUX_TMP1, AUX_MUL, AUX_RES = range(7)
(ERR_MISSING_CELL, ERR_NOT_INSTRUCTION, ERR_BAD_OP1_SOURCE, ERR_BAD_RES_LOGIC, ERR_NOT_AN_ADDRESS, ERR_ADDRESS_RANGE, ERR_PUBLIC_ZERO, ERR_PUBLIC_CELLS,
 ERR_NO_ONES, ERR_NOT_SINGLE_VALUED, ERR_NOT_CONTINUOUS, ERR_TOO_MANY_GAPS, ERR_FILL) = (1 << k for k in range(13))
CELL_VALUE, CELL_ADDRESS = 0, 1


@pytest.fixture(scope="module")
def ctx():
    from sandstorm_amd import backend as be
    c = be.Context(0)
    yield c
    c.close()


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
_MONT = {}


def mont(values):
    """python ints -> (len, 4) uint64 Montgomery limbs (oracle.to_mont, one conversion per distinct value)"""
    from oracle import oracle_py
    todo = [v for v in set(values) if v not in _MONT]
    if todo:
        for v, limbs in zip(todo, oracle_py.to_mont(todo)):
            _MONT[v] = limbs
    out = np.empty((len(values), 4), dtype=np.uint64)
    for k, v in enumerate(values):
        out[k] = _MONT[v]
    return out


def felt_arg(v):
    """a felt passed by pointer (pad_value[4]): Montgomery limbs"""
    a = np.ascontiguousarray(mont([v])[0])
    return a, a.ctypes.data_as(C.POINTER(C.c_uint64))


def ones_buffer(ctx, nbytes):
    """a device buffer pre-filled with the sentinel: all ones (no field element, no valid address)"""
    assert nbytes % 8 == 0
    return ctx.alloc(nbytes).upload(np.full(nbytes // 8, ONES, dtype=np.uint64))


def uploaded(ctx, arr):
    a = np.ascontiguousarray(arr)
    return ctx.alloc(max(a.nbytes, 8)).upload(a)


def status_block(ctx):
    st = ctx.alloc(64)
    assert ctx.lib.ss_dev_zero(ctx.handle, st.ptr, 64) == 0
    return st


def read_status(ctx, st):
    out = (C.c_uint32 * 16)()
    assert ctx.lib.ss_trace_status(ctx.handle, st.ptr, out) == 0
    return list(out)


def free(*bufs):
    for b in bufs:
        if b is not None:
            b.free()


def draw_value(rng):
    """half from the edge list (the top of the field, Montgomery images of +-1, ...), half uniform on [0, p)"""
    return rng.choice(ev.EDGE) if rng.random() < 0.5 else rng.randrange(P)


# ---- ss_trace_memory_image -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_records", [0, 1, 255, 256, 257])
def test_memory_image(ctx, n_records):
    """records in shuffled order, a fifth of them at addresses >= cells (dropped), one at cells - 1: the named cells hold their words,
    every other cell of the image reads back as all ones, nothing behind the image is touched"""
    cells, behind = 300, 16
    rng = random.Random(100 + n_records)
    inside = [cells - 1] + rng.sample(range(cells - 1), 250)
    beyond = [cells, cells + 1, 1 << 20, (1 << 32) + 5, M64 - 1] + rng.sample(range(cells + 2, cells + 5000), 80)
    addrs = inside[:max(1, n_records - n_records // 5)] + beyond[:n_records // 5]
    addrs = addrs[:n_records]
    rng.shuffle(addrs)
    words = [draw_value(rng) if rng.random() < 0.8 else rng.getrandbits(255) for _ in addrs]
    rec = np.zeros((max(n_records, 1), 5), dtype=np.uint64)
    for k, (a, w) in enumerate(zip(addrs, words)):
        rec[k, 0] = a
        rec[k, 1:] = ev.to_limbs([w])[0]
    d_rec = uploaded(ctx, rec)
    mark = np.uint64(0x5A5A5A5A5A5A5A5A)                       # not all ones: "no record names it" must be WRITTEN by the call
    d_image = ctx.alloc(32 * (cells + behind)).upload(np.full(4 * (cells + behind), mark, dtype=np.uint64))
    assert ctx.lib.ss_trace_memory_image(ctx.handle, d_rec.ptr, n_records, d_image.ptr, cells) == 0, ctx.lib.ss_last_error()
    got = d_image.download(np.uint64, (cells + behind, 4))
    free(d_rec, d_image)
    want = np.full((cells, 4), ONES, dtype=np.uint64)
    kept = 0
    for a, w in zip(addrs, words):
        if a < cells:
            want[a] = ev.to_limbs([w])[0]
            kept += 1
    if n_records:
        assert kept >= 1 and (want[cells - 1] != ONES).any()
    assert n_records < 5 or kept < n_records
    assert np.array_equal(got[:cells], want)
    assert (got[cells:] == mark).all(), "cells behind the image were written"


# ---- ss_trace_cpu_cells ----------------------------------------------------------------------------------------------------------
IMAGE_CELLS = 1 << 17
OFFSET_EDGES = (0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF)
R256 = ev.R256
FORMS = [(d, o, s, r, pcu, apu, opc) for d in (0, 1) for o in (0, 1) for s in (0, 1, 2, 4) for r in (0, 1, 2) for pcu in (0, 1, 2, 4) for apu in (0, 1, 2)
         for opc in (0, 1, 2, 4)]
assert len(FORMS) == 2304
# the value slots of a cycle: 0 .. 15 the flag prefixes, then
(S_OFF_DST, S_OFF_OP0, S_OFF_OP1, S_AP, S_FP, S_TMP0, S_TMP1, S_MUL, S_RES, S_PC, S_INST, S_OP0_ADDR, S_OP0, S_DST_ADDR, S_DST, S_OP1_ADDR, S_OP1, S_ZERO, S_ONE,
 S_PAD, S_FILL) = range(16, 37)
N_SLOTS = 37


def form_flags(form):
    d, o, s, r, pcu, apu, opc = form
    return d | o << 1 | s << 2 | r << 5 | pcu << 7 | apu << 10 | opc << 12


def form_of_flags(flags):
    return (flags & 1, (flags >> 1) & 1, (flags >> 2) & 7, (flags >> 5) & 3, (flags >> 7) & 7, (flags >> 10) & 3, (flags >> 12) & 7)


def cycle_reference(image, cells, ap, fp, pc):
    """one cycle as the header documents ss_trace_cpu_cells (binary/src/lib.rs:565-721 for the word): -> (error bits, the cycle's value
    slots as integers, its pool addresses (pc, op0, dst, op1)).  A cell the image does not hold reads as zero and sets MISSING_CELL."""
    bits = 0

    def read(a):
        nonlocal bits
        if a >= cells or a not in image:
            bits |= ERR_MISSING_CELL
            return 0
        return image[a]
    word = read(pc)
    w = word % M64
    if word >> 64 or w >> 63:
        bits |= ERR_NOT_INSTRUCTION
    flag = lambda f: (w >> (48 + f)) & 1
    off_dst, off_op0, off_op1 = w & 0xFFFF, (w >> 16) & 0xFFFF, (w >> 32) & 0xFFFF
    dst_addr = (off_dst + (fp if flag(0) else ap) - 0x8000) % M64
    op0_addr = (off_op0 + (fp if flag(1) else ap) - 0x8000) % M64
    op0, dst = read(op0_addr), read(dst_addr)
    src = flag(2) + 2 * flag(3) + 4 * flag(4)
    base = 0
    if src == 0:
        if op0 >> 64:
            bits |= ERR_NOT_AN_ADDRESS
        base = op0 % M64
    elif src in (1, 2, 4):
        base = {1: pc, 2: fp, 4: ap}[src]
    else:
        bits |= ERR_BAD_OP1_SOURCE
    op1_addr = (off_op1 + base - 0x8000) % M64
    op1 = read(op1_addr)
    pc_update, res_logic = flag(7) + 2 * flag(8) + 4 * flag(9), flag(5) + 2 * flag(6)
    res = 0
    if pc_update == 4:
        res = pow(dst, -1, P) if dst % P else 0
    elif res_logic == 0:
        res = op1 % P
    elif res_logic == 1:
        res = (op0 + op1) % P
    elif res_logic == 2:
        res = op0 * op1 % P
    else:
        bits |= ERR_BAD_RES_LOGIC
    jnz = flag(9)
    slots = [0 if f == 15 else (w >> (48 + f)) & ((1 << (15 - f)) - 1) for f in range(16)]
    sat = lambda a: min(a, 0xFFFFFFFF)
    slots += [off_dst, off_op0, off_op1, ap, fp, dst % P if jnz else 0, dst * res % P if jnz else 0, op0 * op1 % P, res,
              sat(pc), word % P, sat(op0_addr), op0 % P, sat(dst_addr), dst % P, sat(op1_addr), op1 % P]
    return bits, slots, (sat(pc), sat(op0_addr), sat(dst_addr), sat(op1_addr))


class Batch:
    """cycles (ap, fp, pc) over a small memory image, one per instruction form; every cycle reads four cells of its own"""

    def __init__(self, forms, seed):
        rng = random.Random(seed)
        self.forms, self.states, self.image = list(forms), [], {}
        jumps = 0
        for form in self.forms:
            d, o, s, r, pcu, apu, opc = form
            while True:
                offs = [rng.choice(OFFSET_EDGES) if rng.random() < 0.5 else rng.randrange(1 << 16) for _ in range(3)]
                ap, fp, pc = rng.randrange(0x18000), rng.randrange(0x18000), rng.randrange(0x8000, 0x18000)
                dst_addr, op0_addr = offs[0] + (fp if d else ap) - 0x8000, offs[1] + (fp if o else ap) - 0x8000
                # "op1 from op0": op0 holds an address of the image
                op0 = rng.randrange(0x8000, 0x18000) if s == 0 else draw_value(rng)
                op1_addr = offs[2] + {0: op0, 1: pc, 2: fp, 4: ap}[s] - 0x8000
                addrs = (pc, op0_addr, dst_addr, op1_addr)
                if len(set(addrs)) == 4 and all(0 <= a < IMAGE_CELLS and a not in self.image for a in addrs):
                    break
            if pcu == 4:                      # a conditional jump: dst is zero, or a value whose inverse is an edge case, or random
                dst = (0, P - 1, 1, 2**251, R256, rng.randrange(1, P), draw_value(rng), 0)[jumps % 8]
                jumps += 1
            else:
                dst = draw_value(rng)
            # a register no address of this cycle is made from may hold any u64 (it is still a cell of the auxiliary column)
            if not (d == 0 or o == 0 or s == 4) and rng.random() < 0.5:
                ap = rng.choice((M64 - 1, 1 << 63, rng.getrandbits(64)))
            if not (d == 1 or o == 1 or s == 2) and rng.random() < 0.5:
                fp = rng.choice((M64 - 1, 1 << 63, rng.getrandbits(64)))
            word = offs[0] | offs[1] << 16 | offs[2] << 32 | form_flags(form) << 48
            self.image.update({pc: word, op0_addr: op0, dst_addr: dst, op1_addr: draw_value(rng)})
            self.states.append((ap, fp, pc))
        assert jumps == sum(1 for f in self.forms if f[4] == 4)

    def __len__(self):
        return len(self.states)


def image_array(image):
    arr = np.full((IMAGE_CELLS, 4), ONES, dtype=np.uint64)
    addrs = sorted(image)
    arr[addrs] = ev.to_limbs([image[a] for a in addrs])
    return arr


def layout_table(mod):
    """a layout's placement table from its Python enums (the cpu_layout() of host/trace_{recursive,starknet}.cpp restated)"""
    npc, rc, aux = [NPC_PAD] * 8, [RC_FILL] * 16, [AUX_ZERO] * 16
    N, R, A = mod.Npc, mod.RangeCheck, mod.Auxiliary
    npc[N.PC // 2], npc[N.MEM_OP0_ADDR // 2], npc[N.MEM_DST_ADDR // 2], npc[N.MEM_OP1_ADDR // 2] = NPC_PC, NPC_OP0, NPC_DST, NPC_OP1
    for o in range(0, 16, mod.PUBLIC_MEMORY_STEP):
        npc[(o + N.PUB_MEM_ADDR) // 2] = NPC_PUBLIC
    rc[R.OFF_DST], rc[R.OFF_OP0], rc[R.OFF_OP1] = RC_OFF_DST, RC_OFF_OP0, RC_OFF_OP1
    if hasattr(mod, "DilutedCheck"):          # starknet: the diluted pool's cells share the range-check column and start as zero
        for o in range(0, 16, mod.DILUTED_CHECK_STEP):
            rc[o + mod.DilutedCheck.UNORDERED] = rc[o + mod.DilutedCheck.ORDERED] = RC_ZERO
    aux[A.AP], aux[A.FP], aux[A.TMP0], aux[A.TMP1], aux[A.OP0_MUL_OP1], aux[A.RES] = AUX_AP, AUX_FP, AUX_TMP0, AUX_TMP1, AUX_MUL, AUX_RES
    return npc, rc, aux


def placement_tables():
    from sandstorm_amd.layouts import recursive as rec, starknet as sk
    rng = random.Random(77)
    permuted = ([NPC_OP1, NPC_DST, NPC_PAD, NPC_OP0, NPC_PUBLIC, NPC_PC, NPC_PC, NPC_OP1],
                [rng.randrange(5) for _ in range(16)], [AUX_RES, AUX_MUL, AUX_TMP1, AUX_TMP0, AUX_FP, AUX_AP, AUX_ZERO] + [rng.randrange(7) for _ in range(9)])
    return {"recursive": layout_table(rec), "starknet": layout_table(sk), "permuted": permuted}


def slot_maps(table):
    """-> per column (flags, pool, range check, auxiliary) the value slot of each of a cycle's 16 rows, and the pool pairs' address kinds"""
    npc, rc, aux = table
    rc_slot = {RC_FILL: S_FILL, RC_ZERO: S_ZERO, RC_OFF_DST: S_OFF_DST, RC_OFF_OP0: S_OFF_OP0, RC_OFF_OP1: S_OFF_OP1}
    aux_slot = {AUX_ZERO: S_ZERO, AUX_AP: S_AP, AUX_FP: S_FP, AUX_TMP0: S_TMP0, AUX_TMP1: S_TMP1, AUX_MUL: S_MUL, AUX_RES: S_RES}
    pair_slot = {NPC_PAD: (S_ONE, S_PAD), NPC_PUBLIC: (S_ZERO, S_ZERO), NPC_PC: (S_PC, S_INST), NPC_OP0: (S_OP0_ADDR, S_OP0), NPC_DST: (S_DST_ADDR, S_DST),
                 NPC_OP1: (S_OP1_ADDR, S_OP1)}
    return (list(range(16)), [pair_slot[npc[o >> 1]][o & 1] for o in range(16)], [rc_slot[k] for k in rc], [aux_slot[k] for k in aux])


class CpuReference:
    """the reference of a batch, computed once: every cycle's value slots as Montgomery limbs, its pool addresses, its error bits"""

    def __init__(self, batch, pad_value, rc_fill, image=None, states=None):
        image, states = batch.image if image is None else image, batch.states if states is None else states
        ints, self.addrs, self.bits = [], [], []
        for ap, fp, pc in states:
            bits, slots, addrs = cycle_reference(image, IMAGE_CELLS, ap, fp, pc)
            ints += slots + [0, 1, pad_value, rc_fill]
            self.addrs.append(addrs)
            self.bits.append(bits)
        self.values = mont(ints).reshape(len(states), N_SLOTS, 4)

    def columns(self, table, num_cycles):
        """-> the four columns' [16 * num_cycles, 4] cells and the 8 * num_cycles pool addresses for a placement table"""
        cols = [self.values[:num_cycles, m, :].reshape(16 * num_cycles, 4) for m in slot_maps(table)]
        kinds = table[0]
        pool_addr = np.array([[1 if k == NPC_PAD else 0 if k == NPC_PUBLIC else a[k - NPC_PC] for k in kinds] for a in self.addrs[:num_cycles]], dtype=np.uint32)
        return cols, pool_addr.reshape(-1)


def run_cpu_cells(ctx, table, states, d_image, num_cycles, pad_value, rc_fill, rows):
    """one call of the entry point into sentinel-filled buffers of `rows` rows -> (the four columns, the pool addresses, the status words)"""
    lay = (C.c_uint8 * 40)(*(table[0] + table[1] + table[2]))
    d_states = uploaded(ctx, np.array(states, dtype=np.uint64))
    cols = [ones_buffer(ctx, 32 * rows) for _ in range(4)]
    d_addr = ones_buffer(ctx, 4 * (rows // 2))
    st = status_block(ctx)
    _keep, pad = felt_arg(pad_value)
    rc = ctx.lib.ss_trace_cpu_cells(ctx.handle, lay, d_states.ptr, num_cycles, d_image.ptr, IMAGE_CELLS, pad, rc_fill, cols[0].ptr, cols[1].ptr, cols[2].ptr,
                                    cols[3].ptr, d_addr.ptr, st.ptr)
    assert rc == 0, ctx.lib.ss_last_error()
    status = read_status(ctx, st)
    got = [c.download(np.uint64, (rows, 4)) for c in cols]
    got_addr = d_addr.download(np.uint32, (rows // 2,))
    free(d_states, d_addr, st, *cols)
    return got, got_addr, status


def cycles_that_agree(got, got_addr, want, want_addr, num_cycles):
    """-> bool per cycle: all 64 cells and all 8 pool addresses of the cycle are the reference's"""
    ok = np.ones(num_cycles, dtype=bool)
    for g, w in zip(got, want):
        ok &= (g[:16 * num_cycles] == w).reshape(num_cycles, 64).all(axis=1)
    ok &= (got_addr[:8 * num_cycles] == want_addr).reshape(num_cycles, 8).all(axis=1)
    return ok


def assert_untouched(got, got_addr, num_cycles):
    for c, g in enumerate(got):
        assert (g[16 * num_cycles:] == ONES).all(), "column %d: rows behind the last cycle were written" % c
    assert (got_addr[8 * num_cycles:] == 0xFFFFFFFF).all(), "pool addresses behind the last cycle were written"


PAD_VALUE, RC_FILL_VALUE = 2**251 + 0x1234567, 0xABCD


@pytest.fixture(scope="module")
def every_form_batch():
    """the shuffled every-form batch and its reference, built without a device"""
    forms = list(FORMS)
    random.Random(2304).shuffle(forms)
    batch = Batch(forms, seed=11)
    return batch, CpuReference(batch, PAD_VALUE, RC_FILL_VALUE)


@pytest.fixture(scope="module")
def every_form(ctx, every_form_batch):
    batch, ref = every_form_batch
    d_image = uploaded(ctx, image_array(batch.image))
    yield batch, ref, d_image
    d_image.free()


def test_the_every_form_batch_is_what_it_claims(every_form_batch):
    """(no device) the batch holds each of the 2 304 forms once, is clean, wraps an address sum below zero, uses huge idle registers, and
    its conditional jumps test zero, p - 1, 1, 2^251 and R256"""
    batch, ref = every_form_batch
    assert sorted(form_of_flags(batch.image[pc] >> 48) for _, _, pc in batch.states) == sorted(FORMS)
    assert not any(ref.bits)
    assert any(ap < 0x8000 or fp < 0x8000 for ap, fp, _ in batch.states) and any(ap >> 63 for ap, _, _ in batch.states) and any(fp >> 63 for _, fp, _ in batch.states)
    jump_dst = Counter()
    for (ap, fp, pc), form in zip(batch.states, batch.forms):
        if form[4] == 4:
            w = batch.image[pc]
            jump_dst[batch.image[(w & 0xFFFF) + (fp if form[0] else ap) - 0x8000]] += 1
    assert all(jump_dst[v] >= 72 for v in (P - 1, 1, 2**251, R256)) and jump_dst[0] >= 144
    big = sum(1 for v in batch.image.values() if v >= 2**251)
    assert big > 500, big


@pytest.mark.parametrize("num_cycles", [1, 127, 128, 129, 2304])
@pytest.mark.parametrize("table", ["recursive", "starknet", "permuted"])
def test_cpu_cells_of_every_instruction_form(ctx, every_form, table, num_cycles):
    """every cell of the flags, memory-pool, range-check and auxiliary columns and every d_pool_addr word of the first num_cycles cycles of
    the shuffled every-form batch, under the two layouts' placement tables and a permuted one; status word 0 stays zero; rows behind the
    last cycle keep the sentinel.  Counts the compared forms: all 2 304 where the batch is whole."""
    batch, ref, d_image = every_form
    tab = placement_tables()[table]
    rows = 16 * (len(batch) + 1)
    got, got_addr, status = run_cpu_cells(ctx, tab, batch.states, d_image, num_cycles, PAD_VALUE, RC_FILL_VALUE, rows)
    want, want_addr = ref.columns(tab, num_cycles)
    ok = cycles_that_agree(got, got_addr, want, want_addr, num_cycles)
    compared = set()
    for c in range(num_cycles):
        assert ok[c], "cycle %d (form %s: dst_reg, op0_reg, op1_src, res_logic, pc_update, ap_update, opcode) differs" % (c, batch.forms[c])
        compared.add(batch.forms[c])
    assert len(compared) == num_cycles
    if num_cycles == len(batch):
        assert len(compared) == 2304
    assert status[0] == 0 and status[1] == 0
    assert_untouched(got, got_addr, num_cycles)


# ---- ss_trace_cpu_cells: the status bits
N_CLEAN = 300


@pytest.fixture(scope="module")
def clean_batch():
    forms = list(FORMS)
    random.Random(300).shuffle(forms)
    # the first 300 forms of another shuffle: the plants pick their cycles by form
    batch = Batch(forms[:N_CLEAN], seed=12)
    ref = CpuReference(batch, PAD_VALUE, RC_FILL_VALUE)
    assert not any(ref.bits)
    return batch, ref


def cycle_addresses(batch, k):
    ap, fp, pc = batch.states[k]
    _, _, (_, op0_addr, dst_addr, op1_addr) = cycle_reference(batch.image, IMAGE_CELLS, ap, fp, pc)
    return pc, op0_addr, dst_addr, op1_addr


def plant(batch, what, start):
    """-> (k, the image with one error planted in cycle k >= start, the bit the header documents for it)"""
    image = dict(batch.image)
    pick = lambda cond: next(k for k in range(start, len(batch)) if cond(batch.forms[k]))
    if what.startswith("missing"):
        k = pick(lambda f: True)
        del image[cycle_addresses(batch, k)[("pc", "op0", "dst", "op1").index(what.split()[1])]]
        return k, image, ERR_MISSING_CELL
    if what == "bit 63":
        k = pick(lambda f: True)
        image[batch.states[k][2]] |= 1 << 63
        return k, image, ERR_NOT_INSTRUCTION
    if what == "high limb":
        k = pick(lambda f: True)
        image[batch.states[k][2]] |= 1 << (64 + 17 * (k % 11))
        return k, image, ERR_NOT_INSTRUCTION
    if what.startswith("op1 source"):
        # the base of such an op1 address is undefined: the word's offset is pointed at a cell the image holds whatever the base (zero)
        src = int(what.split()[2])
        k = pick(lambda f: True)
        pc = batch.states[k][2]
        held = next(a for a in sorted(image) if a < 0x8000 and a != pc)
        w = image[pc] & ~(7 << 50) & ~(0xFFFF << 32)
        image[pc] = w | src << 50 | (held + 0x8000) << 32
        return k, image, ERR_BAD_OP1_SOURCE
    if what == "res logic 3":
        k = pick(lambda f: f[4] != 4)
        image[batch.states[k][2]] |= 3 << 53
        return k, image, ERR_BAD_RES_LOGIC
    assert what == "op0 no address"
    k = pick(lambda f: f[2] == 0)
    image[cycle_addresses(batch, k)[1]] += 1 << (64 + 13 * (k % 14))          # the low 64 bits still name the cell op1 sits in
    return k, image, ERR_NOT_AN_ADDRESS


PLANTS = ["missing pc", "missing op0", "missing dst", "missing op1", "bit 63", "high limb", "op1 source 3", "op1 source 5", "op1 source 6", "op1 source 7",
          "res logic 3", "op0 no address"]


def check_planted(ctx, batch, ref, image, planted):
    """planted: [(k, bit)].  Runs the batch over the image: exactly those bits, word 1 names the smallest k, every other cycle's cells right"""
    from sandstorm_amd.layouts import recursive as rec
    tab = layout_table(rec)
    bad_ref = CpuReference(batch, PAD_VALUE, RC_FILL_VALUE, image=image)
    want_bits = 0
    for k, bit in planted:
        assert bad_ref.bits[k] == bit, "the plant in cycle %d sets %#x in the reference, not just %#x" % (k, bad_ref.bits[k], bit)
        want_bits |= bit
    assert sum(1 for b in bad_ref.bits if b) == len(planted)
    d_image = uploaded(ctx, image_array(image))
    n = len(batch)
    got, got_addr, status = run_cpu_cells(ctx, tab, batch.states, d_image, n, PAD_VALUE, RC_FILL_VALUE, 16 * (n + 1))
    d_image.free()
    assert status[0] == want_bits, "status %#x, planted %#x" % (status[0], want_bits)
    assert status[1] == ~min(k for k, _ in planted) & 0xFFFFFFFF
    want, want_addr = ref.columns(tab, n)              # the CLEAN reference: the other cycles read none of the planted cells
    ok = cycles_that_agree(got, got_addr, want, want_addr, n)
    others = [c for c in range(n) if c not in [k for k, _ in planted]]
    assert ok[others].all(), "cycle %d is not planted and differs" % others[int(np.argmin(ok[others]))]
    assert_untouched(got, got_addr, n)


@pytest.mark.parametrize("what", PLANTS)
def test_cpu_cells_status_bit_of_one_planted_error(ctx, clean_batch, what):
    """one error in one cycle k of a clean 300-cycle batch (k in the first, second and third workgroup over the cases): exactly the
    documented bit, status word 1 = ~k, every cell of every other cycle still right"""
    batch, ref = clean_batch
    k, image, bit = plant(batch, what, start=(37 * PLANTS.index(what) + 5) % (N_CLEAN - 30))
    check_planted(ctx, batch, ref, image, [(k, bit)])


def test_cpu_cells_status_of_two_planted_errors(ctx, clean_batch):
    """two different errors in cycles k1 < k2 of different workgroups: both bits, word 1 names k1"""
    batch, ref = clean_batch
    k2, image, bit2 = plant(batch, "missing dst", start=200)
    k1, image1, bit1 = plant(batch, "res logic 3", start=40)
    pc1 = batch.states[k1][2]
    image[pc1] = image1[pc1]
    assert k1 < 128 <= k2 and bit1 != bit2
    check_planted(ctx, batch, ref, image, [(k1, bit1), (k2, bit2)])


# ---- ss_trace_builtin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_blocks", [1, 5, 1000])
@pytest.mark.parametrize("n_cells", [1, 7, 300])
def test_builtin_templates(ctx, n_cells, n_blocks):
    """random cell tables of both kinds over two columns; one template with d_template_of_block NULL, three with an explicit map;
    addr_per_block 0 and 3: block i's cell e is template value e or the felt of addr_begin + addr_per_block * i + arg, the address cells'
    integers are in d_pool_addr, nothing else is written"""
    from sandstorm_amd import backend as be
    rng = random.Random(1000 * n_cells + n_blocks)
    block_rows, ncols = 256, 2
    rows = n_blocks * block_rows + 32
    for n_templates, addr_per_block in ((1, 0), (1, 3), (3, 0), (3, 3)):
        # distinct (column, offset) per cell; address cells on even rows of column 0, the memory pool
        even0 = rng.sample(range(0, block_rows, 2), min(n_cells, 100))
        n_addr = rng.randrange(1, min(len(even0), n_cells - 1) + 1) if n_cells > 1 else int(n_templates == 3)
        addr_cells = [(0, off, CELL_ADDRESS, rng.randrange(0, 50)) for off in even0[:n_addr]]
        taken = {(0, off) for _, off, _, _ in addr_cells} | {(0, off + 1) for _, off, _, _ in addr_cells}
        spots = [(c, off) for c in range(ncols) for off in range(block_rows) if (c, off) not in taken]
        value_cells = [(c, off, CELL_VALUE, rng.getrandbits(32)) for c, off in rng.sample(spots, n_cells - len(addr_cells))]
        cells = addr_cells + value_cells
        rng.shuffle(cells)
        assert len(cells) == n_cells
        values = ev.edge_column(n_templates * n_cells, seed=n_cells + n_blocks)        # any stored value < p: the kernel copies
        of_block = np.array([rng.randrange(n_templates) for _ in range(n_blocks)], dtype=np.uint32)
        addr_begin = rng.randrange(1, 1 << 20)
        cols = [ones_buffer(ctx, 32 * rows) for _ in range(ncols)]
        d_addr = ones_buffer(ctx, 4 * (rows // 2))
        d_cells, d_values = uploaded(ctx, np.array(cells, dtype=np.uint32)), uploaded(ctx, values)
        d_map = uploaded(ctx, of_block) if n_templates == 3 else None
        rc = ctx.lib.ss_trace_builtin(ctx.handle, be._ptr_array(cols), ncols, d_cells.ptr, n_cells, d_values.ptr, n_templates, d_map.ptr if d_map else None,
                                      n_blocks, block_rows, addr_begin, addr_per_block, d_addr.ptr)
        assert rc == 0, ctx.lib.ss_last_error()
        got = [c.download(np.uint64, (rows, 4)) for c in cols]
        got_addr = d_addr.download(np.uint32, (rows // 2,))
        free(d_cells, d_values, d_map, d_addr, *cols)
        want = [np.full((rows, 4), ONES, dtype=np.uint64) for _ in range(ncols)]
        want_addr = np.full(rows // 2, 0xFFFFFFFF, dtype=np.uint32)
        base = np.arange(n_blocks, dtype=np.int64) * block_rows
        tmpl = of_block.astype(np.int64) if n_templates == 3 else np.zeros(n_blocks, dtype=np.int64)
        for e, (col, off, kind, arg) in enumerate(cells):
            if kind == CELL_VALUE:
                want[col][base + off] = values[tmpl * n_cells + e]
            else:
                a = [addr_begin + addr_per_block * i + arg for i in range(n_blocks)]
                want[col][base + off] = mont(a)
                want_addr[(base + off) // 2] = a
        for c in range(ncols):
            assert np.array_equal(got[c], want[c]), "column %d (%d templates, %d addresses a block)" % (c, n_templates, addr_per_block)
        assert np.array_equal(got_addr, want_addr)


# ---- ss_trace_rc_pool / ss_trace_rc_builtin --------------------------------------------------------------------------------------
class RcPlan(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_slots", "n_given", "slot_rows", "addr_begin", "n_padding", "pad0")] + \
               [(k, C.c_uint32) for k in ("part_stride", "part_off", "pair_off", "rc_lo", "rc_hi", "ordered_step", "ordered_off", "unused_off")]


def rc_pool_inputs(values):
    """d_first and d_padding as the header defines them, and the reference's ordered list"""
    from sandstorm_amd.layouts import recursive as rec
    ordered, padding = rec._rc_ordered_with_padding(values)
    lo, hi = min(values), max(values)
    count = Counter(values)
    first = [0]
    for v in range(lo, hi + 1):
        first.append(first[-1] + max(count[v], 1))
    assert first[-1] == len(ordered) and padding == [v for v in range(lo, hi + 1) if not count[v]]
    return lo, hi, first, padding, ordered


def rc_layouts():
    """(ordered_step, ordered_off, unused_off, slot_rows, part_stride, part_off, pair_off) of the two layouts (host/trace_{recursive,starknet}.cpp)"""
    from sandstorm_amd.layouts import recursive as rec, starknet as sk
    # The host's rc_plan, by the Python enums of the same cells.  ordered_step / ordered_off / unused_off are RANGE_CHECK_STEP / RC_ORDERED /
    # RC_UNUSED in both; slot_rows is RANGE_CHECK_BUILTIN_RATIO * CYCLE_HEIGHT; pair_off is NPC_RANGE_CHECK128_ADDR.  part_stride is
    # CYCLE_HEIGHT (16) in trace_recursive.cpp and 32 in trace_starknet.cpp.  part_off is RC16_COMPONENT in trace_starknet.cpp; trace_recursive.cpp
    # writes it as RC_UNUSED, the same cell (12) that recursive.py names RangeCheck.RC16_COMPONENT: the parts take the unused cell of their cycle.
    assert rec.RangeCheck.RC16_COMPONENT == rec.RangeCheck.UNUSED
    return {"recursive": (rec.RANGE_CHECK_STEP, rec.RangeCheck.ORDERED, rec.RangeCheck.UNUSED, 16 * rec.RANGE_CHECK_BUILTIN_RATIO, 16, rec.RangeCheck.RC16_COMPONENT,
                          rec.Npc.RANGE_CHECK128_ADDR),
            "starknet": (sk.RANGE_CHECK_STEP, sk.RangeCheck.ORDERED, sk.RangeCheck.UNUSED, 16 * sk.RANGE_CHECK_BUILTIN_RATIO, 32, sk.RangeCheck.RC16_COMPONENT,
                         sk.Npc.RANGE_CHECK128_ADDR)}


def rc_multisets():
    rng = random.Random(16)
    return {
        "rc_lo == rc_hi": ([777] * 50, 0),
        "the whole 16-bit range": ([0, 65535] + [rng.randrange(65536) for _ in range(700)], 0),
        "no padding at all": ([v for v in range(32000, 32100) for _ in range(rng.randrange(1, 4))], 0),
        "padding runs out before the odd cycles": ([100, 100, 103, 104, 104, 110] * 3, 0),
        "a pool shorter than the slots": ([5, 9, 9, 12], 0),
        "pad0 > 0": ([rng.randrange(1000, 1400) for _ in range(120)], 37),
        "pad0 beyond the padding": ([rng.randrange(1000, 1040) for _ in range(12)], 500),
    }


@pytest.mark.parametrize("case", list(rc_multisets()))
def test_rc_pool(ctx, case):
    """the ordered values (sorted(values + padding), then rc_hi) at every ordered_step-th row and padding value pad0 + cycle / 2 (then rc_hi)
    on the odd cycles, for 1, 2, 64 and 1000 cycles; every other row keeps the sentinel"""
    values, pad0 = rc_multisets()[case]
    lo, hi, first, padding, ordered = rc_pool_inputs(values)
    step, ordered_off, unused_off = rc_layouts()["recursive"][:3]
    assert rc_layouts()["starknet"][:3] == (step, ordered_off, unused_off)          # both layouts place the pool alike
    d_first, d_padding = uploaded(ctx, np.array(first, dtype=np.uint32)), uploaded(ctx, np.array(padding + [0], dtype=np.uint16))
    for num_cycles in (1, 2, 64, 1000):
        plan = RcPlan(n_padding=len(padding), pad0=pad0, rc_lo=lo, rc_hi=hi, ordered_step=step, ordered_off=ordered_off, unused_off=unused_off)
        rows = 16 * (num_cycles + 1)
        col = ones_buffer(ctx, 32 * rows)
        rc = ctx.lib.ss_trace_rc_pool(ctx.handle, C.byref(plan), d_first.ptr, d_padding.ptr if padding else None, num_cycles, col.ptr)
        assert rc == 0, ctx.lib.ss_last_error()
        got = col.download(np.uint64, (rows, 4))
        col.free()
        want = np.full((rows, 4), ONES, dtype=np.uint64)
        at, vals = [], []
        for cyc in range(num_cycles):
            for j in range(16 // step):
                g = cyc * (16 // step) + j
                at.append(16 * cyc + step * j + ordered_off)
                vals.append(ordered[g] if g < len(ordered) else hi)
            if cyc % 2:
                at.append(16 * cyc + unused_off)
                vals.append(padding[pad0 + cyc // 2] if pad0 + cyc // 2 < len(padding) else hi)
        want[at] = mont(vals)
        assert np.array_equal(got, want), "%d cycles" % num_cycles
    free(d_first, d_padding)


@pytest.mark.parametrize("n_given", ["none", "some", "all"])
@pytest.mark.parametrize("layout", ["recursive", "starknet"])
def test_rc_builtin(ctx, layout, n_given):
    """300 slots: the given instances (2^128 - 1 and 0 among them, indices in any order), then dummies whose eight parts are the next
    padding values - the list ends in the middle of a dummy, rc_hi from there: the parts, most significant first, in the range-check
    column, (addr_begin + index, value) in the pool, the addresses in d_pool_addr; nothing else written"""
    rng = random.Random(len(layout) + len(n_given))
    ordered_step, ordered_off, unused_off, slot_rows, part_stride, part_off, pair_off = rc_layouts()[layout]
    n_slots = 300
    given_n = {"none": 0, "some": 23, "all": n_slots}[n_given]
    dummies = n_slots - given_n
    hi = 40000
    padding = sorted(rng.sample(range(100, hi), max(0, 8 * dummies - 8 * (dummies // 3) - 3)))      # ends inside a dummy (or is empty)
    given_values = ([M64 * M64 - 1, 0, 1 << 127, (1 << 64) - 1, 1 << 64] + [rng.getrandbits(128) for _ in range(given_n)])[:given_n]
    indices = rng.sample(range(5 * n_slots), given_n)
    given = np.array([[i, v % M64, v >> 64] for i, v in zip(indices, given_values)], dtype=np.uint64).reshape(-1, 3)
    addr_begin = 123456
    plan = RcPlan(n_slots=n_slots, n_given=given_n, slot_rows=slot_rows, addr_begin=addr_begin, n_padding=len(padding), part_stride=part_stride, part_off=part_off,
                  pair_off=pair_off, rc_lo=100, rc_hi=hi, ordered_step=ordered_step, ordered_off=ordered_off, unused_off=unused_off)
    rows = n_slots * slot_rows + 32
    rc_col, pool = ones_buffer(ctx, 32 * rows), ones_buffer(ctx, 32 * rows)
    d_addr = ones_buffer(ctx, 4 * (rows // 2))
    d_given = uploaded(ctx, given) if given_n else None
    d_padding = uploaded(ctx, np.array(padding, dtype=np.uint16)) if padding else None
    rc = ctx.lib.ss_trace_rc_builtin(ctx.handle, C.byref(plan), d_given.ptr if d_given else None, d_padding.ptr if d_padding else None, rc_col.ptr, pool.ptr,
                                     d_addr.ptr)
    assert rc == 0, ctx.lib.ss_last_error()
    got_rc, got_pool, got_addr = rc_col.download(np.uint64, (rows, 4)), pool.download(np.uint64, (rows, 4)), d_addr.download(np.uint32, (rows // 2,))
    free(rc_col, pool, d_addr, d_given, d_padding)
    want_rc, want_pool = np.full((rows, 4), ONES, dtype=np.uint64), np.full((rows, 4), ONES, dtype=np.uint64)
    want_addr = np.full(rows // 2, 0xFFFFFFFF, dtype=np.uint32)
    part_rows, part_vals, pair_rows, pair_vals = [], [], [], []
    straddles = False
    for s in range(n_slots):
        if s < given_n:
            index, value = indices[s], given_values[s]
        else:
            index, js = s, range(8 * (s - given_n), 8 * (s - given_n) + 8)
            parts = [padding[j] if j < len(padding) else hi for j in js]
            straddles |= js[0] < len(padding) <= js[-1]
            value = sum(p << (16 * (7 - k)) for k, p in enumerate(parts))
        base = s * slot_rows
        for k in range(8):
            part_rows.append(base + part_stride * k + part_off)
            part_vals.append((value >> (16 * (7 - k))) & 0xFFFF)
        pair_rows += [base + pair_off, base + pair_off + 1]
        pair_vals += [addr_begin + index, value]
        want_addr[(base + pair_off) // 2] = addr_begin + index
    assert straddles or not dummies
    want_rc[part_rows] = mont(part_vals)
    want_pool[pair_rows] = mont(pair_vals)
    assert np.array_equal(got_rc, want_rc)
    assert np.array_equal(got_pool, want_pool)
    assert np.array_equal(got_addr, want_addr)


# ---- ss_trace_ordered_runs -------------------------------------------------------------------------------------------------------
def dilute(v):
    return sum(((v >> i) & 1) << (4 * i) for i in range(16))


@pytest.mark.parametrize("n_values", [1, 300, 65536])
def test_ordered_runs(ctx, n_values):
    """slot k -> d_col[k * stride + offset]: zero before first[0], value lo + j inside run j, the last value behind the pool; plain and diluted
    (0xffff -> 0x1111111111111111), strides (1, 0) and the starknet diluted pool's (8, 5); 1, 255, 257 and 5000 slots"""
    from sandstorm_amd.layouts import starknet as sk
    assert dilute(0xFFFF) == 0x1111111111111111
    rng = random.Random(n_values)
    saw_all_ones_diluted = False
    for slots in (1, 255, 257, 5000):
        for zeros_before in (0, 3):
            # runs of random length (many of them empty where there are more values than slots), ending before the slots do
            total = max(0, slots - zeros_before - rng.randrange(1, 40)) if slots > 1 else 0
            cuts = sorted(rng.randrange(total + 1) for _ in range(n_values - 1))
            first = [zeros_before + c for c in [0] + cuts + [total]]
            assert len(first) == n_values + 1
            d_first = uploaded(ctx, np.array(first, dtype=np.uint32))
            for stride, offset in ((1, 0), (sk.DILUTED_CHECK_STEP, sk.DilutedCheck.ORDERED)):
                for diluted in (0, 1):
                    lo = 0 if diluted or n_values == 65536 else 4000
                    rows = slots * stride + 8
                    col = ones_buffer(ctx, 32 * rows)
                    rc = ctx.lib.ss_trace_ordered_runs(ctx.handle, col.ptr, stride, offset, slots, d_first.ptr, n_values, lo, diluted)
                    assert rc == 0, ctx.lib.ss_last_error()
                    got = col.download(np.uint64, (rows, 4))
                    col.free()
                    vals, j = [], 0
                    for k in range(slots):
                        if k < first[0]:
                            vals.append(0)
                            continue
                        while j < n_values - 1 and first[j + 1] <= k:          # the run that holds k; behind the pool: the last value
                            j += 1
                        v = lo + j
                        vals.append(dilute(v) if diluted else v)
                    saw_all_ones_diluted |= diluted and 0x1111111111111111 in vals
                    want = np.full((rows, 4), ONES, dtype=np.uint64)
                    want[np.arange(slots) * stride + offset] = mont(vals)
                    assert np.array_equal(got, want), "%d slots, stride %d, offset %d, diluted %d, %d zeros" % (slots, stride, offset, diluted, zeros_before)
            d_first.free()
    assert saw_all_ones_diluted == (n_values == 65536)


# ---- ss_trace_patch --------------------------------------------------------------------------------------------------------------
def test_patch(ctx):
    """d_col[d_rows[k]] = felt(d_values[k]) for distinct rows: nothing for count 0, rows >= col_rows skipped, the last row written"""
    col_rows, behind = 1000, 64
    rng = random.Random(9)
    inside = rng.sample(range(1, col_rows - 1), 300) + [col_rows - 1, 0]
    outside = [col_rows, col_rows + 1, col_rows + behind - 1, 1 << 40, M64 - 1]
    rows = inside + outside
    rng.shuffle(rows)
    assert len(set(rows)) == len(rows)        # one lane a row, stored in no order: two patches of one row would race
    values = [rng.choice((0, 1, M64 - 1, 1 << 63, rng.getrandbits(64), rng.getrandbits(16))) for _ in rows]
    d_rows, d_values = uploaded(ctx, np.array(rows, dtype=np.uint64)), uploaded(ctx, np.array(values, dtype=np.uint64))
    for count in (0, len(rows)):
        col = ones_buffer(ctx, 32 * (col_rows + behind))
        assert ctx.lib.ss_trace_patch(ctx.handle, col.ptr, col_rows, d_rows.ptr, d_values.ptr, count) == 0, ctx.lib.ss_last_error()
        got = col.download(np.uint64, (col_rows + behind, 4))
        col.free()
        want = np.full((col_rows + behind, 4), ONES, dtype=np.uint64)
        if count:
            keep = [(r, v) for r, v in zip(rows, values) if r < col_rows]
            want[[r for r, _ in keep]] = mont([v for _, v in keep])
            assert (want[col_rows - 1] != ONES).any()
        assert np.array_equal(got, want), "count %d" % count
    free(d_rows, d_values)


# ---- ss_trace_ordered_memory -----------------------------------------------------------------------------------------------------
UNUSED_OFF = 14                               # Npc::UnusedAddr of both layouts: pair 7 of a cycle


class MemoryCase:
    """the inputs of one call: the pool's n / 2 (address, value) pairs, the public entries, public_cells, pad_value"""

    def __init__(self, n, pairs, public, public_cells, pad_value):
        assert len(pairs) == n // 2
        self.n, self.pairs, self.public, self.public_cells, self.pad_value = n, list(pairs), list(public), public_cells, pad_value


def memory_value(a, pad_value):
    """the one value of address a in the generated memories (address 1 holds the padding value)"""
    if a == 1:
        return pad_value
    rng = random.Random(a)
    return rng.choice(ev.EDGE) if a % 3 == 0 else rng.randrange(P)


def valid_memory(n, top, gaps, public_only=(), public_at_one=0, public_shared=(), n_public_padding=3, hot=None, hot_count=0, triples=(), seed=0):
    """a continuous, single-valued memory on addresses 1 .. top: pair 1 of every cycle is a public-memory slot (0, 0), pair 7 the padding
    pair the gap fillers take, the other six hold the accessed addresses - every address of 2 .. top that is neither a gap nor only in
    the public list at least once, in shuffled order, `hot` hot_count times, each of `triples` (a, a + 1024, a + 2048) in pairs of one
    cycle, the rest repeats.  -> MemoryCase"""
    rng = random.Random(seed)
    pad_value = P - 5 - seed
    cycles = n // 16
    val = lambda a: memory_value(a, pad_value)
    skip = set(gaps) | set(public_only)
    must = [a for a in range(2, top + 1) if a not in skip and a != hot and not any(a in t for t in triples)]
    rng.shuffle(must)
    free_pairs = 6 * cycles
    fill = []
    for t in triples:
        fill += list(t)
    pad_to_six = (-len(fill)) % 6
    fill += [rng.choice(must) for _ in range(pad_to_six)]                          # (the triples stay inside cycles)
    fill += [hot] * hot_count
    fill += must
    assert len(fill) <= free_pairs, "%d accesses for %d free pairs" % (len(fill), free_pairs)
    pool_of = must + ([hot] if hot else []) + [1]
    fill += [rng.choice(pool_of) for _ in range(free_pairs - len(fill))]
    head = len(triples) * 3 + pad_to_six
    tail = fill[head:]
    rng.shuffle(tail)
    fill = fill[:head] + tail
    pairs, it = [], iter(fill)
    for _ in range(cycles):
        for j in range(8):
            a = 0 if j == 1 else 1 if j == 7 else next(it)
            pairs.append((a, 0 if a == 0 else val(a)))
    public = [(a, val(a)) for a in public_only] + [(1, pad_value)] * public_at_one + [(a, val(a)) for a in public_shared]
    rng.shuffle(public)
    return MemoryCase(n, pairs, public, cycles if len(public) + n_public_padding <= cycles else len(public), pad_value)


def ordered_memory_reference(case):
    """-> (the pool's pairs after the gap fillers, the memory column's pairs), from the pool's integer addresses, its values and the public
    entries alone (the five steps of the header's description)"""
    n, half = case.n, case.n // 2
    count, value = Counter(), {}
    for a, v in case.pairs + case.public:
        if a:
            count[a] += 1
            value.setdefault(a, v)
    everything = [a for a, _ in case.pairs + case.public]
    gaps = [a for a in range(max(min(everything) + 1, 2), max(everything)) if not count[a]]
    pairs = list(case.pairs)
    for g, a in enumerate(gaps):
        assert pairs[(16 * g + UNUSED_OFF) // 2][0] == 1, "a gap filler takes a padding pair"
        pairs[(16 * g + UNUSED_OFF) // 2] = (a, 0)
        count[a], value[a] = 1, 0
    count[1] += case.public_cells - len(case.public) - len(gaps)
    value[1] = case.pad_value
    memory = [(a, value[a]) for a in range(1, max(everything) + 1) for _ in range(count[a])]
    return pairs, memory, gaps


def run_ordered_memory(ctx, case):
    """-> (pool pairs as rows [n, 4], memory column [n, 4], pool addresses, status words); the buffers behind them must keep the sentinel"""
    n, half = case.n, case.n // 2
    flat = [x for a, v in case.pairs for x in (a, v)]
    d_pool = ctx.alloc(32 * (n + 16)).upload(np.concatenate([mont(flat), np.full((16, 4), ONES, dtype=np.uint64)]))
    d_addr = ctx.alloc(4 * (half + 8)).upload(np.array([min(a, 0xFFFFFFFF) for a, _ in case.pairs] + [0xFFFFFFFF] * 8, dtype=np.uint32))
    d_mem = ones_buffer(ctx, 32 * (n + 16))
    d_pub_addr = uploaded(ctx, np.array([a for a, _ in case.public] + [0], dtype=np.uint32))
    d_pub_val = uploaded(ctx, mont([v for _, v in case.public] + [0]))
    st = status_block(ctx)
    _keep, pad = felt_arg(case.pad_value)
    rc = ctx.lib.ss_trace_ordered_memory(ctx.handle, n, d_pool.ptr, d_mem.ptr, d_addr.ptr, d_pub_addr.ptr, d_pub_val.ptr, len(case.public), case.public_cells, pad,
                                         UNUSED_OFF, st.ptr)
    assert rc == 0, ctx.lib.ss_last_error()
    status = read_status(ctx, st)
    pool, mem, addr = d_pool.download(np.uint64, (n + 16, 4)), d_mem.download(np.uint64, (n + 16, 4)), d_addr.download(np.uint32, (half + 8,))
    free(d_pool, d_addr, d_mem, d_pub_addr, d_pub_val, st)
    assert (pool[n:] == ONES).all() and (mem[n:] == ONES).all() and (addr[half:] == 0xFFFFFFFF).all(), "a cell behind the columns was written"
    return pool[:n], mem[:n], addr[:half], status


def check_valid_memory(ctx, case, want_gaps=None):
    pairs, memory, gaps = ordered_memory_reference(case)
    if want_gaps is not None:
        assert len(gaps) == want_gaps
    assert len(memory) == case.n // 2, "the generated case is not a valid memory"
    pool, mem, addr, status = run_ordered_memory(ctx, case)
    assert status[0] == 0, "status %#x, word 1 names %d" % (status[0], ~status[1] & 0xFFFFFFFF)
    assert np.array_equal(addr, np.array([a for a, _ in pairs], dtype=np.uint32)), "d_pool_addr"
    assert np.array_equal(pool, mont([x for p in pairs for x in p])), "the pool's gap pairs"
    assert np.array_equal(mem, mont([x for p in memory for x in p])), "the ordered memory column"
    return gaps


def small_valid_case():
    return valid_memory(256, top=70, gaps=[9, 10, 40], public_only=[20, 21], public_at_one=2, public_shared=[5, 6], seed=1)


def big_valid_case():
    """n = 2^15: four counting workgroups, five scan chunks; see test_ordered_memory_valid"""
    rng = random.Random(15)
    top = 5200
    gaps = set(range(4088, 4104)) | set(rng.sample(range(2100, 4000), 900)) | set(rng.sample(range(4200, 5100), 500))
    hot = 2000
    triples = [(hot, hot + 1024, hot + 2048), (50, 1074, 2098), (51, 1075, 2099), (1023, 2047, 3071), (1024, 2048, 3072)]
    gaps -= {x for t in triples for x in t}
    return valid_memory(1 << 15, top=top, gaps=sorted(gaps), public_only=[4150, 4151], public_at_one=3, public_shared=[2, 3, 5199], hot=hot, hot_count=8300,
                        triples=triples, seed=2), len(gaps)


def test_the_big_memory_case_is_what_it_claims():
    """(no device) one address has over half of the accesses; the triples a, a + 1024, a + 2048 share one counting workgroup's 4096 accesses;
    the gaps' ranks run across the 4096-entry boundary of the address array; more than one gap-rank chunk and five start chunks"""
    case, n_gaps = big_valid_case()
    addrs = [a for a, _ in case.pairs]
    assert Counter(addrs)[2000] > len(addrs) // 2
    for t in ((2000, 3024, 4048), (50, 1074, 2098), (1023, 2047, 3071)):
        assert all(a in addrs[:4096] for a in t)
    _, _, gaps = ordered_memory_reference(case)
    assert len(gaps) == n_gaps and 4095 in gaps and 4096 in gaps and 0 < gaps.index(4096) == gaps.index(4095) + 1
    assert (case.n // 2 + 2 + 4095) // 4096 == 5 and len(addrs) // 4096 == 4


VALID_MEMORIES = ["n = 16", "n = 2^8", "n = 2^13", "n = 2^15", "as many gaps as cycles", "top address n / 2", "public entries"]


@pytest.mark.parametrize("which", VALID_MEMORIES)
def test_ordered_memory_valid(ctx, which):
    """valid inputs: status word 0 stays zero, the gap fillers' pairs, d_pool_addr and the whole memory column are the reference's"""
    if which == "n = 16":
        check_valid_memory(ctx, valid_memory(16, top=7, gaps=[4], n_public_padding=0, seed=3), want_gaps=1)
    elif which == "n = 2^8":
        check_valid_memory(ctx, small_valid_case(), want_gaps=3)
    elif which == "n = 2^13":                # cap + 2 = 4098 entries: one scan chunk and two entries
        check_valid_memory(ctx, valid_memory(1 << 13, top=2900, gaps=list(range(100, 500, 3)) + [2899], public_only=[2000], public_at_one=1, seed=4))
    elif which == "n = 2^15":
        case, n_gaps = big_valid_case()
        check_valid_memory(ctx, case, want_gaps=n_gaps)
    elif which == "as many gaps as cycles":
        check_valid_memory(ctx, valid_memory(512, top=150, gaps=list(range(60, 92)), seed=5), want_gaps=32)
    elif which == "top address n / 2":       # every address 1 .. n / 2 once, no public memory at all
        n = 1 << 10
        order = list(range(1, n // 2 + 1))
        random.Random(6).shuffle(order)
        pad_value = 2**251 + 99
        check_valid_memory(ctx, MemoryCase(n, [(a, memory_value(a, pad_value)) for a in order], [], 0, pad_value), want_gaps=0)
    else:                                    # entries only in the public list, entries at address 1, fewer entries than cells
        case = valid_memory(1 << 10, top=300, gaps=[17], public_only=list(range(200, 230)), public_at_one=5, public_shared=[2, 299, 300], n_public_padding=20, seed=7)
        assert 0 < len(case.public) < case.public_cells
        check_valid_memory(ctx, case, want_gaps=1)


def broken_memory(which):
    """-> (MemoryCase, the bits that must be set, status word 1 where the header names the place, or None)"""
    case = small_valid_case()
    n, half, pad = case.n, case.n // 2, case.pad_value
    free_pair = next(k for k, (a, _) in enumerate(case.pairs) if a > 1 and k % 8 not in (1, 7) and Counter(a for a, _ in case.pairs)[a] > 1)
    if which == "a pool address above n / 2":
        case.pairs[free_pair] = (half + 5, 7)
        return case, ERR_ADDRESS_RANGE | ERR_FILL, None
    if which == "a public address above n / 2":
        case.public.append((half + 1, 7))
        return case, ERR_ADDRESS_RANGE | ERR_FILL, None
    if which == "a public entry at address 0":
        case.public.append((0, 0))
        return case, ERR_PUBLIC_ZERO | ERR_FILL, 0
    if which == "one zero-address pair too many":
        case.pairs[free_pair] = (0, 0)
        return case, ERR_PUBLIC_CELLS | ERR_FILL, 0
    if which == "one zero-address pair too few":
        case.pairs[1] = (1, pad)
        return case, ERR_PUBLIC_CELLS | ERR_FILL, 0
    if which == "the lowest address above 1":
        # addresses 2 .. 7 * cycles + 1 once each, no padding pair anywhere, the public memory full: nothing at address 1
        cycles, it = n // 16, iter(range(2, half))
        pairs = []
        for _ in range(cycles):
            for j in range(8):
                a = 0 if j == 1 else next(it)
                pairs.append((a, 0 if a == 0 else memory_value(a, pad)))
        return MemoryCase(n, pairs, [(a, memory_value(a, pad)) for a in range(2, 2 + cycles)], cycles, pad), ERR_NO_ONES | ERR_NOT_CONTINUOUS, 1
    if which == "pool against pool":
        a, v = case.pairs[free_pair]
        case.pairs[free_pair] = (a, (v + 1) % P)
        return case, ERR_NOT_SINGLE_VALUED, a
    if which == "pool against public":
        k = next(k for k, (a, _) in enumerate(case.public) if a in (5, 6))
        a, v = case.public[k]
        case.public[k] = (a, (v + 1) % P)
        return case, ERR_NOT_SINGLE_VALUED, a
    if which == "address 1 against pad_value":
        case.pairs[free_pair] = (1, (pad + 1) % P)
        return case, ERR_NOT_SINGLE_VALUED, 1
    assert which == "one gap more than cycles"
    case = valid_memory(512, top=150, gaps=list(range(60, 92)) + [120], seed=5)
    return case, ERR_TOO_MANY_GAPS, 120


BROKEN_MEMORIES = ["a pool address above n / 2", "a public address above n / 2", "a public entry at address 0", "one zero-address pair too many",
                   "one zero-address pair too few", "the lowest address above 1", "pool against pool", "pool against public", "address 1 against pad_value",
                   "one gap more than cycles"]


@pytest.mark.parametrize("which", BROKEN_MEMORIES)
def test_ordered_memory_errors(ctx, which):
    """one broken input per case: the named bits are set (FILL where the broken input also leaves the column short or long), word 1 names
    the place where the header says which; the single-valuedness cases set nothing else.  A valid case on the same context passes after"""
    case, bits, where = broken_memory(which)
    _, _, _, status = run_ordered_memory(ctx, case)
    assert status[0] & bits == bits, "status %#x lacks %#x" % (status[0], bits & ~status[0])
    if bits == ERR_NOT_SINGLE_VALUED:
        assert status[0] == bits
    if where is not None:
        assert status[1] == ~where & 0xFFFFFFFF, "word 1 names %d" % (~status[1] & 0xFFFFFFFF)
    check_valid_memory(ctx, small_valid_case(), want_gaps=3)
