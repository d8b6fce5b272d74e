"""Derived columns of the generated constraint kernels (tools/gen_quotient.py derived_column_of): a scratch value that is a fixed
integer combination of cells of ONE trace column - the 16 decoded flags of the CPU constraints, c_j - 2 c_(j+1) - is not recomputed
at every read but read as one cell of a column F the launch builds once (sandstorm_amd/csrc/quotient_derive.h).

Here, without a GPU: which recipes the generator groups into a derived column and which it leaves rematerialised; bodies generated
with derived columns on, compiled with the existing host harness (so through the fallback definition of QG_DERIVED_RAW that each
body carries) against the oracle's constraint VM; and the device's definition - a read of an array filled by the library's row
function, whole domain and row block - against that fallback (tests/cpp/quotient_gen_derived_host_test.cpp).  Results are field
elements: equality, no tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_quotient_gen_fuzz import (ACC, CONST, NCOLS, NCONSTS, NTABLES, OP_ADD, OP_MOV, OP_MUL, OP_OUT, OP_RSUB, OP_ST, OP_SUB, SLOT, TRACE,
                                          Builder, _add_mod_p)
from tests.test_quotient_gen_host import CPP, ROOT, _extreme, run_host
from tests.test_layout_starknet import P

sys.path.insert(0, os.path.join(ROOT, "tools"))

CPP_DERIVED = os.path.join(ROOT, "tests", "cpp", "quotient_gen_derived_host_test.cpp")
FLAGS = (0, ((0, 1), (1, -2)))                   # the derived column of the decoded flags: + column 0 at offset 0, - 2 x column 0 at offset 1
NSLOTS = 24
EDGE = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2]


def cell(col, off):
    return (TRACE, (col << 24) | off)


def decode_program(nflags=16, extras=True):
    """the shape of the CPU decode: flags f_j = c_j - 2 c_(j+1) over column 0 parked in slots, bit constraints f^2 - f, flags as
    factors of products; with `extras` three more parked values: one that names a constant, one over two columns (both read twice)
    and one over a single column that is read once"""
    ins = []
    e = lambda op, d, kind=0, w1=0: ins.append((op, d, kind, int(w1)))
    for j in range(nflags):
        e(OP_MOV, 3, *cell(0, j + 1))
        e(OP_ADD, 3, *cell(0, j + 1))
        e(OP_RSUB, 3, *cell(0, j))
        e(OP_ST, 3, 0, j)
    if extras:
        e(OP_MOV, 3, *cell(0, 3)); e(OP_ADD, 3, CONST, 1); e(OP_ST, 3, 0, 16)                  # names a constant
        e(OP_MOV, 3, *cell(1, 0)); e(OP_SUB, 3, *cell(2, 1)); e(OP_ST, 3, 0, 17)               # two columns
        e(OP_MOV, 3, *cell(3, 0)); e(OP_ADD, 3, *cell(3, 2)); e(OP_ST, 3, 0, 18)               # one column, read once
    started = False

    def constraint_done(k):
        nonlocal started
        e(OP_MUL, 2, CONST, k % NCONSTS)
        e(OP_ADD if started else OP_MOV, 1, ACC, 2)
        started = True
    for j in range(nflags):                                                                      # f^2 - f
        e(OP_MOV, 2, SLOT, j); e(OP_MUL, 2, ACC, 2); e(OP_SUB, 2, SLOT, j)
        constraint_done(j)
    for j in range(0, nflags - 1, 3):                                                            # f_j x cell - f_(j+1) x cell' + f_j
        e(OP_MOV, 2, SLOT, j); e(OP_MUL, 2, *cell(1 + j % 4, j % 3))
        e(OP_MOV, 3, SLOT, j + 1); e(OP_MUL, 3, *cell(2, 1)); e(OP_SUB, 2, ACC, 3); e(OP_ADD, 2, SLOT, j)
        constraint_done(j + 5)
    if extras:
        for s in (16, 17):
            e(OP_MOV, 2, SLOT, s); e(OP_MUL, 2, *cell(4, 0)); e(OP_SUB, 2, SLOT, s)
            constraint_done(s)
        e(OP_MOV, 2, *cell(5, 1)); e(OP_MUL, 2, SLOT, 18)
        constraint_done(18)
    e(OP_MOV, 0, ACC, 1)
    e(OP_OUT, 0)
    return ins


def planted(rng):
    """a random program of the fuzz test's generator with a few decoded flags planted in it: defined in front (slots 6 ..), used in
    bit constraints and as factors behind the program's own groups"""
    ins = Builder(rng).program(False)
    assert ins[-1][0] == OP_OUT and ins[-1][1] == 0
    nflags = int(rng.integers(2, 6))
    head, tail = [], []
    for j in range(nflags):
        head += [(OP_MOV, 3, *cell(0, j + 1)), (OP_ADD, 3, *cell(0, j + 1)), (OP_RSUB, 3, *cell(0, j)), (OP_ST, 3, 0, 6 + j)]
    for j in range(nflags):
        tail += [(OP_MOV, 2, SLOT, 6 + j), (OP_MUL, 2, ACC, 2), (OP_SUB, 2, SLOT, 6 + j), (OP_MUL, 2, CONST, int(rng.integers(NCONSTS))), (OP_ADD, 0, ACC, 2)]
    for j in range(nflags - 1):
        tail += [(OP_MOV, 2, SLOT, 6 + j), (OP_MUL, 2, SLOT, 7 + j), (OP_RSUB, 2, *cell(int(rng.integers(NCOLS)), 2)),
                 (OP_MUL, 2, CONST, int(rng.integers(NCONSTS))), (OP_ADD, 0, ACC, 2)]
    return head + ins[:-1] + tail + [ins[-1]]


def with_derived(gen_quotient, ins, min_saved=0):
    """what generate() does to a part that rematerialises -> (program, derived columns).  The bodies under test are small: by default
    without the floor on loads saved, which is about whether a column pays for its pass and not about what the body computes"""
    found = {}
    gen_quotient.rematerialize_cheap_slots(ins, found=found)
    derived = gen_quotient.choose_derived_columns(found, min_saved=min_saved)
    return gen_quotient.rematerialize_cheap_slots(ins, derived=derived), derived


def test_recipes_over_one_column_become_one_derived_column():
    import gen_quotient as g
    ins = decode_program()
    found = {}
    plain = g.rematerialize_cheap_slots(ins, found=found)
    assert plain == g.rematerialize_cheap_slots(ins)                       # collecting changes nothing, and the default is today's program
    assert not any(kind == g.SRC_DERIVED for _, _, kind, _ in plain)
    # the 16 flags are one column; the one-column value read once is found too but not kept; constants and two columns never are
    assert set(found) == {FLAGS, (3, ((0, 1), (2, 1)))}
    assert found[(3, ((0, 1), (2, 1)))][0] == 1
    assert found[FLAGS][0] == sum(1 for op, _, kind, w1 in ins if op <= OP_MUL and kind == SLOT and w1 < 16)
    assert g.choose_derived_columns(found) == [FLAGS]
    out, derived = with_derived(g, ins, min_saved=None)                    # with the generator's own floor
    assert derived == [FLAGS]
    loads = [(op, d, w1) for op, d, kind, w1 in out if kind == g.SRC_DERIVED and op <= OP_MUL]
    assert all(w1 >> 24 == 0 for _, _, w1 in loads)
    assert set(w1 & 0xffffff for _, _, w1 in loads) == set(range(16))      # flag j is the column's cell at row offset j
    # every definition became one load (its three instructions and the store are gone), every read one load
    assert out[:16] == [(OP_MOV, 3, g.SRC_DERIVED, j) for j in range(16)]
    assert len(loads) == 16 + found[FLAGS][0]
    assert not any(kind == TRACE and w1 >> 24 == 0 and op in (OP_ADD, OP_RSUB) for op, _, kind, w1 in out)
    assert not any(op == OP_ST and w1 < 16 for op, _, _, w1 in out)
    # the others are rematerialised as before: replayed into the generator's own accumulator in front of their reads
    temp = [(op, kind, w1) for op, d, kind, w1 in out if d == g.TEMP_ACC]
    assert temp.count((OP_ADD, CONST, 1)) == 2                             # names a constant: at both reads
    assert temp.count((OP_SUB, TRACE, (2 << 24) | 1)) == 2                 # two columns: at both reads
    assert temp.count((OP_ADD, TRACE, (3 << 24) | 2)) == 1                 # read once
    assert not any(op == OP_ST for op, _, _, _ in out)


def test_a_column_read_once_is_not_kept_and_the_cap_holds():
    import gen_quotient as g
    assert g.choose_derived_columns({FLAGS: [1, 200]}) == []
    assert g.choose_derived_columns({FLAGS: [9, g.MIN_DERIVED_LOADS_SAVED - 1]}) == []              # saves less than its pass is worth
    many = {(c, ((0, 1), (1, -2))): [2 + c, g.MIN_DERIVED_LOADS_SAVED + 2 * c] for c in range(4)}
    assert g.choose_derived_columns(many) == [(3, ((0, 1), (1, -2))), (2, ((0, 1), (1, -2)))]      # by loads saved, two at the most
    assert g.derived_column_of([(OP_MOV, 3, *cell(0, 4)), (OP_ADD, 3, *cell(0, 4)), (OP_RSUB, 3, *cell(0, 3))]) == (FLAGS, 3)
    assert g.derived_column_of([(OP_MOV, 3, *cell(0, 4)), (OP_SUB, 3, *cell(0, 4))]) is None       # cancels
    assert g.derived_column_of([(OP_MOV, 3, *cell(0, 4)), (OP_SUB, 3, CONST, 2)]) is None


def _tables(rng, log_n, gen):
    tabs, desc, off = [], [], 0
    for t in range(NTABLES):
        length = 1 << int(rng.integers(1, log_n + 2))
        desc += [off, length.bit_length() - 1]
        off += length
        tabs.append(gen(rng, length))
    return np.concatenate(tabs), desc


def _felts(values):
    return np.array([[(v >> (64 * k)) & ((1 << 64) - 1) for k in range(4)] for v in values], dtype=np.uint64)


def _build(g, tmp, programs, cpp, derived_h=None):
    """the programs' bodies with derived columns on, as the parts of one kernel, compiled with harness `cpp` -> (exe, derived lists)"""
    os.makedirs(tmp, exist_ok=True)
    with open(os.path.join(tmp, "qg_scaled.h"), "w") as f:
        f.write("static const uint32_t QG_N_TABLES = %du, QG_N_SCALED = 0u;\nstatic const uint32_t QG_SCALED_TABLES[] = {0u};\n" % NTABLES)
    lists = []
    with open(os.path.join(tmp, "qg_parts.h"), "w") as f:
        for j, ins in enumerate(programs):
            part, derived = with_derived(g, ins)
            part, n_slots = g.compact_slots(part)
            lists.append(derived)
            g.generate_body("derived", part, NCONSTS, n_slots, NTABLES, NCOLS, 2 + j % 3, "derived_p%d.inc" % j, True, "QG_OUT" if j == 0 else "QG_OUT_ACC",
                            0, True, j % 2 == 0, j % 2 == 0, 1, (), derived=derived)
            f.write("static void run_lane_p%d(HostArgs &a, uint64_t lane, uint64_t lanes) {\n    QG_LANE_PRELUDE\n#include \"%s\"\n}\n"
                    % (j, os.path.join(tmp, "derived_p%d.inc" % j)))
        f.write("static const part_fn PARTS[] = {%s};\n" % ", ".join("run_lane_p%d" % j for j in range(len(programs))))
    flags = ["-DQG_PARTS_H=\"qg_parts.h\"", "-DQG_SCALED_H=\"qg_scaled.h\""]
    if derived_h is not None:
        with open(os.path.join(tmp, "qg_derived.h"), "w") as f:
            f.write("static const uint32_t QG_N_DERIVED = %du;\nstatic const ss::QGenDerived QG_DERIVED[] = {%s};\n" % (len(derived_h), ", ".join(
                "{%du, %du, {%s}, {%s}}" % (col, len(terms), ", ".join("%du" % o for o, _ in terms), ", ".join("%d" % c for _, c in terms)) for col, terms in derived_h)))
        flags.append("-DQG_DERIVED_H=\"qg_derived.h\"")
    exe = os.path.join(tmp, "qg_derived")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fopenmp", "-I", tmp] + flags + ["-o", exe, cpp])
    return exe, lists


def _vm(oracle, g, programs, consts, tab, desc, lde, log_n, offset):
    want = None
    for ins in programs:
        v = oracle.eval_program(g.encode(ins), consts, tab, desc, NSLOTS, lde, log_n, 1, offset)
        want = v if want is None else _add_mod_p(want, v)
    return want


def test_bodies_with_derived_columns_through_the_fallback(oracle, tmp_path, monkeypatch):
    import gen_quotient as g
    tmp = str(tmp_path)
    monkeypatch.setattr(g, "OUT_DIR", tmp)
    rng = np.random.default_rng(4107)
    programs = [decode_program()] + [planted(rng) for _ in range(5)]
    exe, lists = _build(g, tmp, programs, CPP)
    assert all(FLAGS in derived for derived in lists)
    for j in range(len(programs)):
        with open(os.path.join(tmp, "derived_p%d.inc" % j)) as f:
            text = f.read()
        assert "#ifndef QG_DERIVED_RAW" in text and "QG_DERIVED_RAW(0, " in text
        assert "fp_sub(QG_TRACE_RAW(0, (off) + 0u, idx), fp_dbl(QG_TRACE_RAW(0, (off) + 1u, idx)))" in text
    log_n = 6
    N = 2 << log_n
    g3 = oracle.to_mont([3])[0]
    w = oracle.to_mont([pow(3, (P - 1) // N, P)])[0]
    rand = lambda r, count: _felts([int.from_bytes(r.bytes(40), "little") % P for _ in range(count)])
    for gen in (rand, _extreme):                                           # random columns, then columns of edge values
        tab, desc = _tables(rng, log_n, gen)
        lde = [gen(rng, N) for _ in range(NCOLS)]
        consts = gen(rng, NCONSTS)
        want = _vm(oracle, g, programs, consts, tab, desc, lde, log_n, g3)
        got = run_host(exe, tmp, lde, tab, desc, consts, N, 0, N - 1, 1, 24, g3, w)
        assert np.array_equal(got, want)


def test_a_body_without_derived_columns_is_todays(tmp_path, monkeypatch):
    """the keyword's default reproduces the body of before: no macro block, no derived operand"""
    import gen_quotient as g
    monkeypatch.setattr(g, "OUT_DIR", str(tmp_path))
    part, n_slots = g.compact_slots(g.rematerialize_cheap_slots(decode_program()))
    g.generate_body("derived", part, NCONSTS, n_slots, NTABLES, NCOLS, 3, "plain.inc", True, "QG_OUT", 0, True, True, True, 1, ())
    with open(os.path.join(str(tmp_path), "plain.inc")) as f:
        assert "DERIVED" not in f.read()


def test_the_device_definition_against_the_fallback(oracle, tmp_path, monkeypatch):
    """QG_DERIVED_RAW as the device defines it - a read of the column that quotient_derive.h's row function built - gives what the
    fallback gives, at 2^10 points and log_blowup 1, on the whole domain (the column wraps with the mask) and on a row block with its
    halo (the column ends where the launch ends it; the harness's reads are bounds-checked).  Column 0 is drawn from 0, 1, p - 1,
    (p - 1) / 2, (p + 1) / 2, and rows N - 2, N - 1, 0, 1 - the pairs a flag read joins across the end of the domain - take every
    pair of those values in turn: every wrap of the subtraction meets every wrap of the index."""
    import gen_quotient as g
    tmp = str(tmp_path)
    monkeypatch.setattr(g, "OUT_DIR", os.path.join(tmp, "fallback"))
    rng = np.random.default_rng(977)
    programs = [decode_program()] + [planted(rng) for _ in range(2)]
    fallback, lists = _build(g, os.path.join(tmp, "fallback"), programs, CPP)
    assert all(derived == [FLAGS] for derived in lists)
    monkeypatch.setattr(g, "OUT_DIR", os.path.join(tmp, "device"))
    device, _ = _build(g, os.path.join(tmp, "device"), programs, CPP_DERIVED, derived_h=[FLAGS])
    log_n = 9
    N = 2 << log_n
    g3 = oracle.to_mont([3])[0]
    w = oracle.to_mont([pow(3, (P - 1) // N, P)])[0]
    tab, desc = _tables(rng, log_n, _extreme)
    lde = [_extreme(rng, N) for _ in range(NCOLS)]
    consts = _extreme(rng, NCONSTS)
    edge = _felts(EDGE)
    lde[0] = edge[rng.integers(0, len(EDGE), size=N)]
    halo = 16 << 1                                                         # the flags' farthest row: offset 16, log_blowup 1
    B = N // 4
    for k, (x, y) in enumerate((x, y) for x in range(len(EDGE)) for y in range(len(EDGE))):
        col0 = lde[0].copy()
        col0[N - 2], col0[0] = edge[x], edge[y]                           # F[N - 2] = c[N - 2] - 2 c[0]
        col0[N - 1], col0[1] = edge[y], edge[x]                           # F[N - 1] = c[N - 1] - 2 c[1]
        cols = [col0] + lde[1:]
        whole = run_host(fallback, tmp, cols, tab, desc, consts, N, 0, N - 1, 1, 96, g3, w)
        assert np.array_equal(run_host(device, tmp, cols, tab, desc, consts, N, 0, N - 1, 1, 96, g3, w), whole)
        if k == 0:
            assert np.array_equal(whole, _vm(oracle, g, programs, consts, tab, desc, cols, log_n, g3))
        if k % 6 == 0:                                                     # the row block that wraps around the end of the domain
            idx = (3 * B + np.arange(B + halo)) % N
            block = run_host(device, tmp, [c[idx] for c in cols], tab, desc, consts, B, 3 * B, 0xffffffff, 1, 64, g3, w)
            assert np.array_equal(block, whole[3 * B:])
