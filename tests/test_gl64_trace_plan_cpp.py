"""host/trace_plain.cpp's parsing, planning and refusals alone, without a device, as a stand-alone program under AddressSanitizer and
UBSan (tests/cpp/trace_plain_plan_test.cpp: its own main, the C ABI stubbed): the range-check plan against one counted here from the
run's offsets, the files' own refusals, and the message each status block asks for - the location that belongs to the bit reported."""
import os
import shutil
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gl64_programs as gp                                       # noqa: E402
from sandstorm_amd import binary as bn                           # noqa: E402
from sandstorm_amd.layouts import plain as pl                    # noqa: E402


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("plan") / "trace_plain_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "trace_plain_plan_test.cpp"), os.path.join(ROOT, "sandstorm_amd", "host", "trace_plain.cpp")])
    return exe


def run(program, tmp_path, trace_bin, memory_bin, public_memory, n_steps, status=None):
    paths = [str(tmp_path / name) for name in ("trace.bin", "memory.bin", "public.bin")]
    for path, blob in zip(paths, (trace_bin, memory_bin, b"".join(struct.pack("<QQ", a, v) for a, v in public_memory))):
        with open(path, "wb") as f:
            f.write(blob)
    out = subprocess.run([program] + paths + [str(n_steps)] + [str(v) for v in (status or [])], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.strip().splitlines()


def files(prog, cycles):
    states, memory = pl.run(prog, cycles)
    return states, memory, pl.public_input_of(prog, states, memory), bn.write_register_states(states), bn.write_memory(memory)


def test_plan_of_the_busy_run(program, tmp_path):
    states, memory, pi, trace_bin, memory_bin = files(gp.busy_program(), 256)
    count = {}
    for st in states:
        w = bn.Word(memory[st.pc])
        for v in (w.off_dst, w.off_op0, w.off_op1):
            count[v] = count.get(v, 0) + 1
    lo, hi = min(count), max(count)
    first = [0]
    for v in range(lo, hi + 1):
        first.append(first[-1] + max(count.get(v, 0), 1))
    lines = run(program, tmp_path, trace_bin, memory_bin, pi.public_memory, 256)
    assert lines[0] == "n 4096 cells 2050 lo %d hi %d pad_value %d" % (lo, hi, pi.public_memory_padding()[1])
    assert lines[1] == "first " + " ".join(str(v) for v in first)
    assert lines[2] == "padding " + " ".join(str(v) for v in range(lo, hi + 1) if v not in count)
    assert lines[3] == "public " + " ".join("%d:%d" % (a, v % pl.P) for a, v in pi.public_memory)


def test_refusals_from_the_files_alone(program, tmp_path):
    states, memory, pi, trace_bin, memory_bin = files(pl.example_program(2), 16)
    refused = lambda *a: run(program, tmp_path, *a)[-1]
    assert refused(trace_bin[:-24], memory_bin, pi.public_memory, 15) == "refused: trace: the number of cycles must be a power of two"
    assert refused(trace_bin[:-24], memory_bin, pi.public_memory, 16) == "refused: trace: trace file does not hold the run's cycles"
    assert refused(trace_bin, memory_bin[:-1], pi.public_memory, 16) == "refused: trace: memory file is not a sequence of (u64 address, 32-byte word) records"
    assert refused(trace_bin, memory_bin, [e for e in pi.public_memory if e[0] != 1], 16).startswith("refused: trace: the public memory holds no value at address 1")
    for prog, message in ((gp.wide_offsets_program(), "range-check values do not fit the trace"), (gp.long_program(), "public memory does not fit")):
        _, _, pi2, t2, m2 = files(prog, 16)
        assert refused(t2, m2, pi2.public_memory, 16) == "refused: trace: " + message


def test_each_status_bit_is_reported_with_its_own_location(program, tmp_path):
    """the CPU's bits name cycles in words 7 .. 11, the memory's bits an address in word 1; with several bits set the message is the first
    base_trace would raise, and its location is that bit's"""
    states, memory, pi, trace_bin, memory_bin = files(pl.example_program(2), 16)
    inv = lambda v: (~v) & 0xFFFFFFFF

    def refusal(bits, where=0, cycles=()):
        st = [bits, inv(where)] + [0] * 14
        for bit, cyc in cycles:
            st[7 + bit] = inv(cyc)
        return run(program, tmp_path, trace_bin, memory_bin, pi.public_memory, 16, st)[-1]
    assert refusal(0) == "refusal:"                               # (the lines are stripped)
    assert refusal(2, cycles=[(1, 5)]) == "refusal: instruction at pc %d has bit 63 set" % states[5].pc
    # a missing cell at cycle 7 (the file holds every cell: the cycle's last access is named), whatever else is set and wherever
    w = bn.Word(memory[states[7].pc])
    op1 = w.op1_addr(states[7].pc, states[7].ap, states[7].fp, memory)
    assert refusal(1 | 2 | 512, where=3, cycles=[(0, 7), (1, 2)]) == "refusal: the run reads address %d, which memory.bin does not hold" % op1
    assert refusal(2048 | 2 | 1024, where=9, cycles=[(1, 4)]) == "refusal: more memory holes than gap cells"
    assert refusal(2 | 512, where=9, cycles=[(1, 4)]) == "refusal: instruction at pc %d has bit 63 set" % states[4].pc
    for bits in (64, 128, 256):
        assert refusal(bits | 512, where=9) == "refusal: the public-memory cells must be the only accesses of address 0, and memory starts at 1"
    for bits in (512, 1024, 32):
        assert refusal(bits, where=9) == "refusal: memory is not continuous and single-valued at address 9"
    assert refusal(4096, where=9) == "refusal: the ordered memory does not fill its column"
