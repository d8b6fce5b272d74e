"""The plain layout's base trace over the 64-bit field made ON the device (csrc/trace.hip trace_gl64_* / mem_*_gl64 behind
ss_trace_gl64_*; host/trace_plain.cpp; goldilocks.plain_base_trace_on_device / prove_files) against its specification,
sandstorm_amd/layouts/plain.py base_trace, cell for cell: the example run and a busy program (tests/gl64_programs.py) at sizes below,
at and above one workgroup of the CPU kernel (CPU_CYC = 128 cycles: 16, 128, 512, 1024 cycles) - one and many chunks of the ordered
memory's scans -, each kernel alone against Python integers with all-ones sentinels around what it owns, every refusal with
base_trace's message and location, the proof from the files against the proof from host-made columns, and the bytes a generation
uploads.  Every comparison is exact.

Checked against deliberately wrong kernels (scratch copies of the host build of the device code, lanes shuffled; what failed):
  res = gl_add(op0, op1) for res_logic mul      -> example_run (all four sizes), busy_program (both), cpu_cells_alone, both proofs
  the padding value on odd cycles only          -> busy_program (both), rc_pool_alone (all three: an even cycle's row 12 keeps the sentinel);
                                                   example_run stays green - its pool has no unused value, every row 12 is rc_hi
  the gap cells at rows 12, 13 (one pair off)   -> example_run (all four), busy_program (both), the two-valued-memory refusal, the
                                                   permutations, both proofs, upload_accounting (the generation is refused: the op1 pair is gone)
  tmp1 = dst * res without the reduction mod p  -> busy_program (both), cpu_cells_alone (the jnz on 2^63 + 12345 and on p - 1)
  no barrier between the cycles' records and    -> example_run (all four), busy_program (both), cpu_cells_alone, the permutations, both
  the workgroup's row writes                       proofs, upload_accounting

Runs on the MI355X (`-m gpu`) and, in the CPU suite, on the host build of the device code (tests/test_gl64_trace_on_host.py)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gl64_programs as gp                                       # noqa: E402
from sandstorm_amd import binary as bn                           # noqa: E402
from sandstorm_amd.layouts import plain as pl                    # noqa: E402

pytestmark = pytest.mark.gpu
P = pl.P
ONES = np.uint64(2**64 - 1)
EMULATED = os.environ.get("SS_TEST_HIPEMU") == "1"               # the host build of the device code: torch CPU tensors are the "device" buffers
SIZES = (16, 128, 512, 1024)                                     # cycles: below one workgroup of the CPU kernel, exactly one, several
(ERR_MISSING_CELL, ERR_NOT_INSTRUCTION, ERR_BAD_OP1_SOURCE, ERR_BAD_RES_LOGIC, ERR_NOT_AN_ADDRESS, ERR_ADDRESS_RANGE, ERR_PUBLIC_ZERO, ERR_PUBLIC_CELLS,
 ERR_NO_ONES, ERR_NOT_SINGLE_VALUED, ERR_NOT_CONTINUOUS, ERR_TOO_MANY_GAPS, ERR_FILL) = (1 << k for k in range(13))
ST_GL_CYCLE = 7                                                  # include/sandstorm_hip.h SS_TRACE_STATUS_GL_CYCLE


@pytest.fixture(scope="module")
def env():
    """(context, torch device): the context on the stream torch works on"""
    import torch
    from sandstorm_amd import backend as be
    if EMULATED:
        ctx, dev = be.Context(0), torch.device("cpu")
        yield ctx, dev
        ctx.close()
        return
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx = be.Context(0, stream=stream.cuda_stream)
    yield ctx, dev
    ctx.close()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))


# ---- runs and their reference, made once ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def run_of(name, cycles):
    """-> (program, states, memory, public input, trace.bin, memory.bin): the program idles in `jmp rel 0`, so running it for `cycles`
    steps is the run padded with its final state"""
    prog = {"example": lambda: pl.example_program(2), "busy": gp.busy_program, "wide": gp.wide_offsets_program, "long": gp.long_program,
            "holes": gp.holes_program}[name]()
    states, memory = pl.run(prog, cycles)
    pi = pl.public_input_of(prog, states, memory)
    return prog, states, memory, pi, bn.write_register_states(states), bn.write_memory(memory)


@functools.lru_cache(maxsize=None)
def reference(name, cycles):
    _, states, memory, pi, _, _ = run_of(name, cycles)
    return tuple(np.array(c, dtype=np.uint64) for c in pl.base_trace(states, memory, pi))


def host(cols):
    return [c.cpu().numpy().view(np.uint64) for c in cols]


def assert_columns(got, want):
    for c, (g, w) in enumerate(zip(got, want)):
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "column %d: %d cells differ, first at row %d (cycle %d, offset %d): %d for %d" % (
            c, bad.size, bad[0], bad[0] // 16, bad[0] % 16, int(g[bad[0]]), int(w[bad[0]]))


# ---- the entry points driven from here (the plan in Python integers) -------------------------------------------------------------------
class RcPlan(C.Structure):
    """ss_trace_rc_plan"""
    _fields_ = [(k, C.c_uint64) for k in ("n_slots", "n_given", "slot_rows", "addr_begin", "n_padding", "pad0")] + \
               [(k, C.c_uint32) for k in ("part_stride", "part_off", "pair_off", "rc_lo", "rc_hi", "ordered_step", "ordered_off", "unused_off")]


def rc_plan(lo, hi, n_padding, pad0=0, **kw):
    p = RcPlan(n_padding=n_padding, pad0=pad0, rc_lo=lo, rc_hi=hi, ordered_step=4, ordered_off=2, unused_off=12)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def ones_buffer(ctx, words, dtype=np.uint64):
    return ctx.alloc(max(8, words * np.dtype(dtype).itemsize)).upload(np.full(max(words, 1), ~dtype(0), dtype=dtype))


def uploaded(ctx, arr):
    a = np.ascontiguousarray(arr)
    return ctx.alloc(max(a.nbytes, 8)).upload(a) if a.nbytes else None


def ptr(buf):
    return buf.ptr if buf is not None else None


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


def rc_pool_plan(states, memory):
    """(lo, hi, first, padding) from the run's offsets, as the header documents d_first / d_padding"""
    count = {}
    for st in states:
        w = bn.Word(memory[st.pc])
        for v in (w.off_dst, w.off_op0, w.off_op1):
            count[v] = count.get(v, 0) + 1
    lo, hi = min(count), max(count)
    first, padding = [0], []
    for v in range(lo, hi + 1):
        first.append(first[-1] + max(count.get(v, 0), 1))
        if v not in count:
            padding.append(v)
    return lo, hi, np.array(first, dtype=np.uint32), np.array(padding, dtype=np.uint16)


def memory_image(ctx, memory_bin, cells):
    rec = uploaded(ctx, np.frombuffer(memory_bin, dtype=np.uint64))
    image = ctx.alloc(8 * cells)
    assert ctx.lib.ss_trace_gl64_memory_image(ctx.handle, ptr(rec), len(memory_bin) // 40, image.ptr, cells) == 0, ctx.lib.ss_last_error()
    return image, rec


def generate_by_entry_points(ctx, name, cycles, tail=32):
    """the four entry points in the driver's order on sentinel-filled columns of 16 * cycles + tail rows
    -> (five columns, pool addresses, status words), tails included"""
    _, states, memory, pi, trace_bin, memory_bin = run_of(name, cycles)
    n = 16 * cycles
    cols = [ones_buffer(ctx, n + tail) for _ in range(5)]
    pool_addr = ones_buffer(ctx, n // 2 + tail, np.uint32)
    st = status_block(ctx)
    d_states = uploaded(ctx, np.frombuffer(trace_bin, dtype=np.uint64))
    cells = n // 2 + 2
    image, rec = memory_image(ctx, memory_bin, cells)
    lo, hi, first, padding = rc_pool_plan(states, memory)
    d_first, d_padding = uploaded(ctx, first), uploaded(ctx, padding)
    pad_value = pi.public_memory_padding()[1] % P
    lib, h = ctx.lib, ctx.handle
    assert lib.ss_trace_gl64_cpu_cells(h, d_states.ptr, cycles, image.ptr, cells, pad_value, hi, n, cols[pl.COL_FLAGS].ptr, cols[pl.COL_NPC].ptr,
                                       cols[pl.COL_RANGE_CHECK].ptr, cols[pl.COL_AUXILIARY].ptr, pool_addr.ptr, st.ptr) == 0, lib.ss_last_error()
    plan = rc_plan(lo, hi, len(padding))
    assert lib.ss_trace_gl64_rc_pool(h, C.byref(plan), d_first.ptr, ptr(d_padding), cycles, n, cols[pl.COL_RANGE_CHECK].ptr) == 0, lib.ss_last_error()
    d_pa = uploaded(ctx, np.array([a for a, _ in pi.public_memory], dtype=np.uint32))
    d_pv = uploaded(ctx, np.array([v % P for _, v in pi.public_memory], dtype=np.uint64))
    assert lib.ss_trace_gl64_ordered_memory(h, n, n, cols[pl.COL_NPC].ptr, cols[pl.COL_MEMORY].ptr, pool_addr.ptr, ptr(d_pa), ptr(d_pv), len(pi.public_memory),
                                            pad_value, st.ptr) == 0, lib.ss_last_error()
    status = read_status(ctx, st)
    got = [c.download(np.uint64, (n + tail,)) for c in cols]
    addrs = pool_addr.download(np.uint32, (n // 2 + tail,))
    free(*cols, pool_addr, st, d_states, image, rec, d_first, d_padding, d_pa, d_pv)
    return got, addrs, status


# ---- 1, 2: whole generations, cell for cell ----------------------------------------------------------------------------------------------
def check_generation(env, name, cycles):
    ctx, dev = env
    from sandstorm_amd import goldilocks as gs
    want = reference(name, cycles)
    n = 16 * cycles
    # the entry points alone: the columns, the pool's addresses, and nothing behind either
    got, addrs, status = generate_by_entry_points(ctx, name, cycles)
    assert status[0] == 0, "error bits %#x" % status[0]
    assert_columns([g[:n] for g in got], want)
    assert all((g[n:] == ONES).all() for g in got), "rows behind the columns were written"
    assert np.array_equal(addrs[:n // 2].astype(np.uint64), want[pl.COL_NPC][0::2]), "d_pool_addr is not the pool's even rows"
    assert (addrs[n // 2:] == np.uint32(0xFFFFFFFF)).all(), "words behind d_pool_addr were written"
    # the public interface: files -> five device tensors
    _, _, _, pi, trace_bin, memory_bin = run_of(name, cycles)
    cols = gs.plain_base_trace_on_device(ctx, trace_bin, memory_bin, pi)
    assert len(cols) == 5 and all(c.shape == (n,) and c.device.type == dev.type for c in cols)
    assert_columns(host(cols), want)


@pytest.mark.parametrize("cycles", SIZES)
def test_example_run_cell_for_cell(env, cycles):
    """plain.example_program(2) padded with its final state to each size: all five device columns equal plain.base_trace exactly, and
    d_pool_addr is the pool's even rows"""
    check_generation(env, "example", cycles)


BUSY_CYCLES = 256                                                # the smallest power of two that holds busy_program's 223 cycles


@pytest.mark.parametrize("cycles", [BUSY_CYCLES, 4 * BUSY_CYCLES])
def test_busy_program_cell_for_cell(env, cycles):
    """every instruction form, operands at the top of the field, 40 memory holes, 24 unused range-check values"""
    assert 200 <= gp.busy_cycles() <= BUSY_CYCLES < 2 * gp.busy_cycles()
    _, states, memory, pi, _, _ = run_of("busy", cycles)
    want = reference("busy", cycles)
    assert sum(1 for r in range(0, 16 * cycles, 16) if want[pl.COL_NPC][r + pl.Npc.GAP_ADDR] != 1) >= 30
    assert len(rc_pool_plan(states, memory)[3]) >= 20
    d = states[10]                                               # the jnz on 2^63 + 12345: the device's inverse against pow(d, -1, P)
    assert bn.Word(memory[d.pc]).pc_update == 4 and memory[d.ap - 2] >= 2**63
    assert int(want[pl.COL_RANGE_CHECK][16 * 10 + 15]) == pow(memory[d.ap - 2], -1, P)
    check_generation(env, "busy", cycles)


# ---- 3: each kernel alone ------------------------------------------------------------------------------------------------------------------
def test_memory_image_alone(env):
    """named cells, a cell no record names, words that are no field elements (a nonzero upper byte; a low word >= p), records at and
    beyond `cells`: the image holds the named words, all ones elsewhere, and nothing behind it is touched"""
    ctx, _ = env
    cells, behind = 300, 16
    rec = {0: 0, 7: P - 1, 8: 2**63, 299: 12345, 5: 77}
    bad = {20: 1 << 64, 21: (1 << 255) | 3, 22: P, 23: 2**64 - 1}
    beyond = {300: 1, 301: 2, 1 << 20: 3, 2**64 - 1: 4}
    blob = b"".join(int(a).to_bytes(8, "little") + int(w).to_bytes(32, "little") for a, w in list(rec.items()) + list(bad.items()) + list(beyond.items()))
    mark = np.uint64(0x5A5A5A5A5A5A5A5A)
    d_rec = uploaded(ctx, np.frombuffer(blob, dtype=np.uint64))
    image = ctx.alloc(8 * (cells + behind)).upload(np.full(cells + behind, mark, dtype=np.uint64))
    assert ctx.lib.ss_trace_gl64_memory_image(ctx.handle, d_rec.ptr, len(blob) // 40, image.ptr, cells) == 0, ctx.lib.ss_last_error()
    got = image.download(np.uint64, (cells + behind,))
    free(d_rec, image)
    want = np.full(cells, ONES, dtype=np.uint64)
    for a, w in rec.items():
        want[a] = w
    assert np.array_equal(got[:cells], want)
    assert (got[cells:] == mark).all(), "cells behind the image were written"


def cpu_cells_reference(states, memory, pad_value, rc_fill):
    """what ss_trace_gl64_cpu_cells alone writes: the four columns whole - the pool with its padding pairs, the range-check column with
    the filler where the pool's own cells go - and the pool's addresses"""
    n = 16 * len(states)
    flags, npc, rc, aux = ([0] * n for _ in range(4))
    addrs = []
    for c, st in enumerate(states):
        r, w = 16 * c, bn.Word(memory[st.pc])
        da, a0, a1 = w.dst_addr(st.ap, st.fp), w.op0_addr(st.ap, st.fp), w.op1_addr(st.pc, st.ap, st.fp, memory)
        dst, op0, op1 = memory[da] % P, memory[a0] % P, memory[a1] % P
        if w.pc_update == 4:
            res = pow(dst, -1, P) if dst else 0
        else:
            res = (op1, (op0 + op1) % P, op0 * op1 % P)[w.res_logic]
        tmp0 = dst if w.flag(bn.PC_JNZ) else 0
        flags[r:r + 16] = [w.flag_prefix(f) for f in range(16)]
        pairs = [(st.pc, memory[st.pc]), (0, 0), (a0, op0), (1, pad_value), (da, dst), (0, 0), (a1, op1), (1, pad_value)]
        npc[r:r + 16] = [v for p in pairs for v in p]
        addrs += [p[0] for p in pairs]
        rc[r:r + 16] = [w.off_dst, rc_fill, rc_fill, st.ap, w.off_op1, rc_fill, rc_fill, op0 * op1 % P, w.off_op0, rc_fill, rc_fill, st.fp, rc_fill, rc_fill,
                        rc_fill, res]
        aux[r], aux[r + 8] = tmp0, tmp0 * res % P
    return [np.array(c, dtype=np.uint64) for c in (flags, npc, rc, aux)], np.array(addrs, dtype=np.uint32)


def test_cpu_cells_alone_at_a_ragged_last_workgroup(env):
    """the first 165 cycles of the busy run (one workgroup and 37 cycles): the four columns whole, the pool's addresses, the fifth
    column and everything behind 16 * 165 rows untouched"""
    ctx, _ = env
    _, states, memory, pi, trace_bin, memory_bin = run_of("busy", BUSY_CYCLES)
    cycles, tail = 165, 48
    n = 16 * cycles
    pad_value, rc_fill = pi.public_memory_padding()[1] % P, 40000
    want, want_addr = cpu_cells_reference(states[:cycles], memory, pad_value, rc_fill)
    cols = [ones_buffer(ctx, n + tail) for _ in range(4)]
    pool_addr = ones_buffer(ctx, n // 2 + tail, np.uint32)
    st = status_block(ctx)
    d_states = uploaded(ctx, np.frombuffer(trace_bin[:24 * cycles], dtype=np.uint64))
    cells = 8 * BUSY_CYCLES + 2
    image, rec = memory_image(ctx, memory_bin, cells)
    assert ctx.lib.ss_trace_gl64_cpu_cells(ctx.handle, d_states.ptr, cycles, image.ptr, cells, pad_value, rc_fill, n, cols[0].ptr, cols[1].ptr, cols[2].ptr,
                                           cols[3].ptr, pool_addr.ptr, st.ptr) == 0, ctx.lib.ss_last_error()
    status = read_status(ctx, st)
    got = [c.download(np.uint64, (n + tail,)) for c in cols]
    addrs = pool_addr.download(np.uint32, (n // 2 + tail,))
    free(*cols, pool_addr, st, d_states, image, rec)
    assert status[0] == 0
    assert_columns([g[:n] for g in got], want)
    assert all((g[n:] == ONES).all() for g in got)
    assert np.array_equal(addrs[:n // 2], want_addr) and (addrs[n // 2:] == np.uint32(0xFFFFFFFF)).all()


@pytest.mark.parametrize("n_padding", [0, 5, 40], ids=["no padding", "some", "more than cycles"])
def test_rc_pool_alone(env, n_padding):
    """32 cycles, values 100 .. 100 + span with every other one unused: the ordered values at rows 4 j + 2, padding value c at row 12 of
    EVERY cycle c (then rc_hi forever), every other cell still the sentinel"""
    ctx, _ = env
    cycles, lo = 32, 100
    n = 16 * cycles
    unused = [lo + 1 + 2 * k for k in range(n_padding)]
    hi = lo + 2 * n_padding + 3
    first = [0]
    for v in range(lo, hi + 1):
        first.append(first[-1] + (1 if v in unused or v % 5 else 3))
    assert first[-1] < n // 4                                     # the pool ends inside the column: the rest is rc_hi
    ordered = [v for v in range(lo, hi + 1) for _ in range(first[v - lo + 1] - first[v - lo])]
    col = ones_buffer(ctx, n + 16)
    d_first, d_padding = uploaded(ctx, np.array(first, dtype=np.uint32)), uploaded(ctx, np.array(unused, dtype=np.uint16))
    plan = rc_plan(lo, hi, n_padding)
    assert ctx.lib.ss_trace_gl64_rc_pool(ctx.handle, C.byref(plan), d_first.ptr, ptr(d_padding), cycles, n, col.ptr) == 0, ctx.lib.ss_last_error()
    got = col.download(np.uint64, (n + 16,))
    free(col, d_first, d_padding)
    want = np.full(n + 16, ONES, dtype=np.uint64)
    for k in range(n // 4):
        want[4 * k + 2] = ordered[k] if k < len(ordered) else hi
    for c in range(cycles):
        want[16 * c + 12] = unused[c] if c < len(unused) else hi
    assert np.array_equal(got, want)


def test_ordered_memory_alone_with_a_repeated_public_entry_and_no_gap(env):
    """a pool of 64 cycles whose accesses cover addresses 1 .. 300 without a hole, a public memory of (1, pad), (5, value of 5) - the
    second repeats a pool access - and (301, v), which only the public memory names: the sorted pairs fill the memory column, the
    pool is left as it was (no gap cell taken), no error bit"""
    ctx, _ = env
    cycles = 64
    n, half = 16 * cycles, 8 * cycles
    value = lambda a: (a * 0x9E3779B97F4A7C15 + (P - 1)) % P
    pad = value(1)
    pairs = []
    for j in range(half):
        pairs.append((0, 0) if j % 8 in (1, 5) else (1, pad))
    free_slots = [j for j in range(half) if j % 8 not in (1, 5)]
    accesses = [(a, value(a)) for a in range(2, 301)] + [(7, value(7))] * 3 + [(300, value(300))]
    assert len(accesses) < len(free_slots)
    step = len(free_slots) // len(accesses)                       # spread over the pool: more than one chunk of the counting kernel's LDS table
    for k, acc in enumerate(accesses):
        pairs[free_slots[k * step]] = acc
    public = [(1, pad), (5, value(5)), (301, value(301))]
    pool_h = np.array([v for p in pairs for v in p], dtype=np.uint64)
    pool = ctx.alloc(8 * n).upload(pool_h)
    pool_addr = uploaded(ctx, np.array([a for a, _ in pairs], dtype=np.uint32))
    mem = ones_buffer(ctx, n + 16)
    st = status_block(ctx)
    d_pa, d_pv = uploaded(ctx, np.array([a for a, _ in public], dtype=np.uint32)), uploaded(ctx, np.array([v for _, v in public], dtype=np.uint64))
    assert ctx.lib.ss_trace_gl64_ordered_memory(ctx.handle, n, n, pool.ptr, mem.ptr, pool_addr.ptr, d_pa.ptr, d_pv.ptr, len(public), pad, st.ptr) == 0, \
        ctx.lib.ss_last_error()
    status = read_status(ctx, st)
    got, pool_after = mem.download(np.uint64, (n + 16,)), pool.download(np.uint64, (n,))
    free(pool, pool_addr, mem, st, d_pa, d_pv)
    assert status[0] == 0, "error bits %#x" % status[0]
    acc = [p for p in pairs if p[0] != 0] + [(1, pad)] * (n // 8 - len(public)) + public
    acc.sort(key=lambda e: e[0])
    assert len(acc) == half
    assert np.array_equal(got[:n], np.array([v for p in acc for v in p], dtype=np.uint64))
    assert (got[n:] == ONES).all()
    assert np.array_equal(pool_after, pool_h), "a gap cell was taken though memory has no hole"


# ---- 4: refusals ---------------------------------------------------------------------------------------------------------------------------
def refusal_of_python(states, memory, pi):
    with pytest.raises(ValueError) as e:
        pl.base_trace(states, memory, pi)
    return str(e.value)


def refusal_of_device(env, trace_bin, memory_bin, pi):
    from sandstorm_amd import goldilocks as gs
    from sandstorm_amd._lib import SandstormHipError
    with pytest.raises(SandstormHipError) as e:
        gs.plain_base_trace_on_device(env[0], trace_bin, memory_bin, pi)
    return str(e.value)


@pytest.mark.parametrize("name,message", [("wide", "range-check values do not fit the trace"), ("long", "public memory does not fit"),
                                          ("holes", "more memory holes than gap cells")])
def test_refusals_of_runs_that_do_not_fit(env, name, message):
    _, states, memory, pi, trace_bin, memory_bin = run_of(name, 16)
    assert refusal_of_python(states, memory, pi) == message
    assert message in refusal_of_device(env, trace_bin, memory_bin, pi)


def test_refusal_of_an_instruction_with_bit_63(env):
    import copy
    prog, states, memory, pi, trace_bin, _ = run_of("example", 16)
    k = 3                                                        # the instruction the fourth cycle runs
    pc = states[k].pc
    memory, pi = list(memory), copy.deepcopy(pi)
    memory[pc] |= 1 << 63
    assert memory[pc] < P
    pi.public_memory = [(a, memory[pc] if a == pc else v) for a, v in pi.public_memory]
    message = refusal_of_python(states, memory, pi)
    assert message == "instruction at pc %d has bit 63 set" % pc
    assert message in refusal_of_device(env, trace_bin, bn.write_memory(memory), pi)


def test_refusal_of_a_run_that_reads_a_cell_the_file_does_not_hold(env):
    """(Python has no message for it: the text and the address are include/sandstorm_hip.h's and host/trace_plain.cpp's)"""
    _, states, memory, pi, trace_bin, _ = run_of("example", 16)
    w = bn.Word(memory[states[2].pc])                            # the third cycle's destination: written there, read by no earlier cycle
    gone = w.dst_addr(states[2].ap, states[2].fp)
    assert gone not in [a for a, _ in pi.public_memory]
    memory = list(memory)
    memory[gone] = None
    assert "the run reads address %d, which memory.bin does not hold" % gone in refusal_of_device(env, trace_bin, bn.write_memory(memory), pi)


def test_refusal_of_a_public_memory_entry_at_address_zero(env):
    import copy
    _, states, memory, pi, trace_bin, memory_bin = run_of("example", 16)
    pi = copy.deepcopy(pi)
    pi.public_memory = pi.public_memory + [(0, 5)]
    message = refusal_of_python(states, memory, pi)
    assert message == "the public-memory cells must be the only accesses of address 0, and memory starts at 1"
    assert message in refusal_of_device(env, trace_bin, memory_bin, pi)


def test_refusal_of_memory_with_two_values_at_an_address(env):
    import copy
    _, states, memory, pi, trace_bin, memory_bin = run_of("example", 16)
    pi = copy.deepcopy(pi)
    a, v = pi.public_memory[4]
    assert a != 1
    pi.public_memory[4] = (a, (v + 1) % P)
    message = refusal_of_python(states, memory, pi)
    assert message == "memory is not continuous and single-valued at address %d" % a
    assert message in refusal_of_device(env, trace_bin, memory_bin, pi)


def test_bad_arguments_are_refused_and_nothing_is_written(env):
    """NULL context, NULL column, and columns shorter than 16 * cycles: an error, and every sentinel still in place"""
    ctx, dev = env
    import torch
    from sandstorm_amd import hostlib
    from sandstorm_amd._lib import SandstormHipError
    _, states, memory, pi, trace_bin, memory_bin = run_of("example", 16)
    n = 256
    sentinel = lambda: torch.full((n,), -1, dtype=torch.int64, device=dev)
    cols = [sentinel() for _ in range(5)]
    with pytest.raises(SandstormHipError, match="NULL argument"):
        hostlib.gl_base_trace_device(None, trace_bin, memory_bin, pi, cols)
    with pytest.raises(SandstormHipError, match="NULL column"):
        hostlib.gl_base_trace_device(ctx, trace_bin, memory_bin, pi, cols[:2] + [0] + cols[3:])
    assert all(bool((c == -1).all()) for c in cols)
    lib, h = ctx.lib, ctx.handle
    bufs = [ones_buffer(ctx, n) for _ in range(5)]
    pool_addr, st = ones_buffer(ctx, n // 2, np.uint32), status_block(ctx)
    d_states = uploaded(ctx, np.frombuffer(trace_bin, dtype=np.uint64))
    image, rec = memory_image(ctx, memory_bin, n // 2 + 2)
    d_first = uploaded(ctx, np.array([0, 1], dtype=np.uint32))
    plan = rc_plan(5, 5, 0)
    p = [b.ptr for b in bufs]
    assert lib.ss_trace_gl64_cpu_cells(h, d_states.ptr, 16, image.ptr, n // 2 + 2, 0, 5, n - 1, p[0], p[1], p[3], p[4], pool_addr.ptr, st.ptr) != 0
    assert lib.ss_trace_gl64_cpu_cells(h, d_states.ptr, 16, image.ptr, n // 2 + 2, 0, 5, n, p[0], None, p[3], p[4], pool_addr.ptr, st.ptr) != 0
    assert lib.ss_trace_gl64_cpu_cells(None, d_states.ptr, 16, image.ptr, n // 2 + 2, 0, 5, n, p[0], p[1], p[3], p[4], pool_addr.ptr, st.ptr) != 0
    assert lib.ss_trace_gl64_rc_pool(h, C.byref(plan), d_first.ptr, None, 16, n - 1, p[3]) != 0
    wrong = rc_plan(5, 5, 0, unused_off=13)
    assert lib.ss_trace_gl64_rc_pool(h, C.byref(wrong), d_first.ptr, None, 16, n, p[3]) != 0
    assert lib.ss_trace_gl64_ordered_memory(h, n, n - 1, p[1], p[2], pool_addr.ptr, None, None, 0, 0, st.ptr) != 0
    assert lib.ss_trace_gl64_ordered_memory(h, n, n, p[1], None, pool_addr.ptr, None, None, 0, 0, st.ptr) != 0
    assert lib.ss_trace_gl64_memory_image(h, None, 3, image.ptr, n // 2 + 2) != 0
    assert read_status(ctx, st) == [0] * 16
    assert all((b.download(np.uint64, (n,)) == ONES).all() for b in bufs)
    assert (pool_addr.download(np.uint32, (n // 2,)) == np.uint32(0xFFFFFFFF)).all()
    free(*bufs, pool_addr, st, d_states, image, rec, d_first)


# ---- 5: closing the loop ---------------------------------------------------------------------------------------------------------------------
LOOP_CYCLES = 1024


def test_device_made_columns_close_the_permutations(env):
    """with device-made columns, plain_extension_on_device(check=True) closes the range-check product and its memory total is
    plain.public_memory_quotient"""
    ctx, _ = env
    from sandstorm_amd import goldilocks as gs
    _, _, _, pi, trace_bin, memory_bin = run_of("example", LOOP_CYCLES)
    cols = gs.plain_base_trace_on_device(ctx, trace_bin, memory_bin, pi)
    challenges = [(3, 1, 4), (1, 5, 9), (2, 6, 5)]
    _, last_mem = gs.plain_extension_on_device(ctx, cols, challenges, check=True)
    assert last_mem == pl.public_memory_quotient(challenges[pl.MEM_Z], challenges[pl.MEM_A], 16 * LOOP_CYCLES, pi)


@pytest.mark.parametrize("sha256", [0, 1])
def test_proof_from_the_files_is_the_proof_from_host_made_columns(env, sha256):
    """goldilocks.prove_files: accepted by goldilocks.verify, and array for array the proof Prover.prove writes from base_trace_np's
    columns with the same seed and statement"""
    ctx, dev = env
    import torch
    from sandstorm_amd import goldilocks as gs
    _, states, memory, pi, trace_bin, memory_bin = run_of("example", LOOP_CYCLES)
    air, seed = gs.plain_air(), bytes(range(32))
    opt = gs.Options(num_queries=20, grinding=8, hash="sha256" if sha256 else "blake2s")
    proof = gs.prove_files(ctx, trace_bin, memory_bin, pi, seed, opt)
    gs.verify(proof, air, seed, statement=pi, expected_options=opt, required_security_bits=28)
    base = [torch.from_numpy(c.view(np.int64)).to(dev) for c in pl.base_trace_np(states, memory, pi)]
    want = gs.proof_to_arrays(gs.Prover(ctx, air, opt).prove(seed, base, lambda ch: gs.plain_extension_on_device(ctx, base, ch)[0], statement=pi))
    got = gs.proof_to_arrays(proof)
    assert set(got) == set(want)
    for k in sorted(want):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k


# ---- 6: what a generation uploads ----------------------------------------------------------------------------------------------------------
def test_upload_accounting(env):
    """a generation uploads the two files, 12 bytes per public-memory entry, the range-check plan (at most 65 537 u32 + 65 536 u16) and
    nothing of the size of the columns: a bound derived from what the driver needs, not measured"""
    ctx, _ = env
    from sandstorm_amd import goldilocks as gs, hostlib
    _, _, _, pi, trace_bin, memory_bin = run_of("example", LOOP_CYCLES)
    gs.plain_base_trace_on_device(ctx, trace_bin, memory_bin, pi)
    uploaded_bytes = hostlib.gl_trace_last_stats()["bytes_uploaded"]
    status_block_bytes = 16 * 4
    assert 0 < uploaded_bytes <= len(trace_bin) + len(memory_bin) + 12 * len(pi.public_memory) + 65537 * 4 + 65536 * 2 + status_block_bytes
    assert uploaded_bytes < 5 * 8 * (16 * LOOP_CYCLES) // 4
