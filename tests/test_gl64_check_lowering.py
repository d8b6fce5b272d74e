"""The 64-bit field's trace check without a device: air_program.lower_checks on the plain layout's 47 constraints (layouts/plain.py
check_program) - the program interpreted in Python integers over Fq3, row by row, against plain.failing_rows; a sub-expression two
constraints share is computed once; and lower(), which shares its code generator with the new lowering, still emits the words it
emitted (the 252-bit layouts' digests from the commit before any lower_checks existed, the plain layout's compiled-kernel hash)."""
import hashlib
import json
import os
import random
import re
import sys

import pytest

from sandstorm_amd import air_program as ap
from sandstorm_amd.layouts import plain as pl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
P = pl.P
rng = random.Random(20261019)
CH = [tuple(rng.randrange(P) for _ in range(3)) for _ in range(pl.NUM_CHALLENGES)]           # random elements of Fq3


@pytest.fixture(scope="module")
def run16():
    """the example run at 16 cycles (n = 256): base columns, extension coordinate columns for CH, the check program"""
    prog = pl.example_program(2)
    states, memory = pl.run(prog, 16)
    pi = pl.public_input_of(prog, states, memory)
    cols = pl.base_trace(states, memory, pi)
    ext, _ = pl.extension_columns(cols, CH)
    n = len(cols[0])
    assert n == 256
    hints = pl.Hints.from_public_input(pi, CH, n)
    return pi, cols, ext, n, hints, pl.check_program(n, hints, CH)


def run_check_program(prog, cols8, r, n):
    """the two-word program at trace row r in Python integers over Fq3 -> {check index: accumulator at its CHECK}"""
    code, consts = prog.code, prog.consts
    x = (pow(pl.root_of_unity(n.bit_length() - 1), r, P), 0, 0)
    acc, slots, seen = [(0, 0, 0)] * 4, [(0, 0, 0)] * prog.n_slots, {}
    for w0, w1 in zip(code[0::2], code[1::2]):
        op, d, kind = w0 & 0xFF, (w0 >> 8) & 0xF, (w0 >> 12) & 0xF
        if op <= 4:
            assert kind != ap.SRC.TABLE, "the plain layout's check reads no table"
            src = (acc[w1] if kind == ap.SRC.ACC else slots[w1] if kind == ap.SRC.SLOT else tuple(consts[w1]) if kind == ap.SRC.CONST
                   else (cols8[w1 >> 24][(r + (w1 & 0xFFFFFF)) % n], 0, 0) if kind == ap.SRC.TRACE else x)
            acc[d] = (src if op == 0 else pl.add3(acc[d], src) if op == 1 else pl.sub3(acc[d], src) if op == 2 else pl.sub3(src, acc[d]) if op == 3
                      else pl.mul3(acc[d], src))
        elif op == ap.OP.INV:
            acc[d] = pl.inv3(acc[d])
        elif op == ap.OP.ST:
            slots[w1] = acc[d]
        elif op == ap.OP.CHECK:
            assert w1 not in seen
            seen[w1] = acc[d]
        else:
            raise AssertionError("opcode %d in a check program" % op)
    return seen


def report_of_program(prog, domains_rows, cols8, n):
    """{constraint: sorted violating rows of its domain} from the interpreted program"""
    values = [run_check_program(prog, cols8, r, n) for r in range(n)]
    out = {}
    for k, rows in enumerate(domains_rows):
        bad = [r for r in rows if any(values[r][k])]
        if bad:
            out[k] = bad
    return out


def test_check_program_shape(run16):
    pi, cols, ext, n, hints, (prog, domains, names, domain_names) = run16
    cs = pl.constraints(hints, CH)
    assert len(domains) == len(names) == len(domain_names) == len(cs) == 47
    assert names == [c.name for c in cs] and domain_names == [c.domain.name for c in cs]
    assert domains == [(list(map(tuple, c.domain.num(n))), list(map(tuple, c.domain.den(n)))) for c in cs]
    ops = [w & 0xFF for w in prog.code[0::2]]
    assert [w1 for w0, w1 in zip(prog.code[0::2], prog.code[1::2]) if w0 & 0xFF == ap.OP.CHECK] == list(range(47))      # CHECK k in order, each once
    assert ap.OP.OUT not in ops and ap.OP.INV not in ops                     # no OUT; bare numerators: no zerofier inverse
    assert not any((w >> 12) & 0xF in (ap.SRC.TABLE, ap.SRC.X) and (w & 0xFF) <= 4 for w in prog.code[0::2])         # no multiplier
    assert all(len(c) == 3 for c in prog.consts)                             # constants of the extension
    # no power of a composition coefficient: the constants are the challenges, the hints, the basis X, X^2 and base-field values
    known = [tuple(v) for v in CH] + [pl.f3(h) for h in (hints.memory_quotient, hints.range_check_product)] + [(0, 1, 0), (0, 0, 1)]
    for c in prog.consts:
        assert tuple(c) in known or (c[1] == c[2] == 0)


def test_a_domain_with_too_many_factors_is_refused_by_name(monkeypatch):
    from sandstorm_amd.layouts import recursive as rec
    wide = rec.Domain("seventeen rows", lambda n: range(17), lambda n: [], lambda n: [(1, k) for k in range(17)])
    monkeypatch.setattr(pl, "constraints", lambda hints, challenges=None: [rec.Constraint("too/wide", pl.npc(0), wide)])
    with pytest.raises(ValueError, match="too/wide.*seventeen rows.*17 denominator"):
        pl.check_program(256, pl.Hints(0, 0, 0, 0), CH)


def test_interpreted_check_program_reproduces_failing_rows(run16):
    """clean trace and three corruptions: the violating rows the program finds are failing_rows', for all 47 constraints"""
    pi, cols, ext, n, hints, (prog, domains, names, domain_names) = run16
    cs = pl.constraints(hints, CH)
    rows = [list(c.domain.rows(n)) for c in cs]
    corruptions = [None,
                   (pl.COL_RANGE_CHECK, 16 * 2 + pl.Auxiliary.RES[1]),       # `res` of a cycle of the loop
                   (pl.COL_NPC, n - 16 + pl.Npc.PC),                          # the last cycle's pc
                   (pl.NUM_BASE_COLUMNS + 1, 6)]                              # coordinate 1 of the permutation column, a memory row
    for cell in corruptions:
        cols8 = [list(c) for c in cols + ext]
        if cell is not None:
            cols8[cell[0]][cell[1]] = (cols8[cell[0]][cell[1]] + 1) % P
        want = {}
        for k, c in enumerate(cs):
            bad = pl.failing_rows(c, cols8, n, limit=n)
            if bad:
                want[k] = sorted(bad)
        assert (cell is None) == (not want), cell
        assert report_of_program(prog, rows, cols8, n) == want, cell


def test_a_shared_subexpression_is_stored_once(run16):
    """memory/diff_is_bit and memory/is_func both read address_diff = mem(ADDRESS, 1) - mem(ADDRESS): lowered together it is computed
    once, parked in a slot across the first CHECK and read back for the second; lowered apart it is computed twice"""
    pi, cols, ext, n, hints, _ = run16
    cs = {c.name: c for c in pl.constraints(hints, CH)}
    a, b = cs["memory/diff_is_bit"].numerator, cs["memory/is_func"].numerator
    next_address = ap.trace_payload(pl.COL_MEMORY, pl.MEMORY_STEP + pl.Mem.ADDRESS)

    def reads(prog, payload):
        return sum(1 for w0, w1 in zip(prog.code[0::2], prog.code[1::2]) if (w0 & 0xFF) <= 4 and (w0 >> 12) & 0xF == ap.SRC.TRACE and w1 == payload)
    both = ap.lower_checks([a, b], P, ext=True)
    apart = [ap.lower_checks([e], P, ext=True) for e in (a, b)]
    assert reads(both, next_address) == 1 and [reads(p_, next_address) for p_ in apart] == [1, 1]
    assert both.n_instr < apart[0].n_instr + apart[1].n_instr
    ops = [(w0 & 0xFF, (w0 >> 12) & 0xF) for w0 in both.code[0::2]]
    first_check = ops.index((ap.OP.CHECK, 0))
    assert any(op <= 4 and kind == ap.SRC.SLOT for op, kind in ops[first_check + 1:])         # the slot outlives the first CHECK
    # a root that is also a later root's sub-expression, and the same root twice
    twice = ap.lower_checks([a, a * b, a], P, ext=True)
    assert reads(twice, next_address) == 1 and [w1 for w0, w1 in zip(twice.code[0::2], twice.code[1::2]) if w0 & 0xFF == ap.OP.CHECK] == [0, 1, 2]
    # and both programs compute what the expressions are
    cols8 = cols + ext
    for r in (0, 2, 100, n - 2):
        got = run_check_program(twice, cols8, r, n)
        ev = lambda e: tuple(ap.evaluate_ext(e, P, (0, 0, 0), lambda c, o: (cols8[c][(r + o) % n], 0, 0), None))
        assert [got[0], got[1], got[2]] == [ev(a), ev(a * b), ev(a)]


def _fnv1a(words):
    h = 0xcbf29ce484222325
    for w in words:
        for b in range(4):
            h = ((h ^ ((w >> (8 * b)) & 0xFF)) * 0x100000001b3) & (2**64 - 1)
    return h


def test_lower_emits_the_words_it_emitted():
    """lower() shares its code generator with lower_checks now: (a) the plain layout's composition still hashes to the compiled
    kernel's program (csrc/quotient_gen_plain_gl.inc: ss_eval_quotient_gl64x3 picks the compiled kernel by this hash), for two
    statements; (b) the C++ host's lower() still writes the 252-bit layouts' words (tests/golden/air_program_code_digests.json)"""
    with open(os.path.join(ROOT, "sandstorm_amd", "csrc", "quotient_gen_plain_gl.inc")) as f:
        inc = f.read()
    want_hash = int(re.search(r"GL3_PLAIN_CODE_HASH\s*=\s*(0x[0-9a-fA-F]+)", inc).group(1), 16)
    want_instr = int(re.search(r"GL3_PLAIN_N_INSTR\s*=\s*(\d+)", inc).group(1))
    for loops, steps in ((2, 16), (10, 64)):
        prog = pl.example_program(loops)
        states, memory = pl.run(prog, steps)
        pi = pl.public_input_of(prog, states, memory)
        n = 16 * steps
        tables = pl.Tables(n, 1)
        root = pl.composition(n, pl.Hints.from_public_input(pi, CH, n), CH, (3, 5, 7), tables)
        low = ap.lower(root, P, ext=True, symbols=tables.symbols)
        assert low.n_instr == want_instr and _fnv1a(low.code) == want_hash
        assert low.code[-2] & 0xFF == ap.OP.OUT and [w & 0xFF for w in low.code[0::2]].count(ap.OP.OUT) == 1
    from test_constraint_check_host import CHALLENGES, host_air
    from sandstorm_amd import backend as be, hostlib
    with open(os.path.join(ROOT, "tests", "golden", "air_program_code_digests.json")) as f:
        want = json.load(f)
    for layout in ("recursive", "starknet"):
        air, _, _, log_n = host_air(layout)
        assert log_n == want[layout]["log_n"]
        low, _, _ = hostlib.prover_air(air).build_program(1 << log_n, [be.felt(c) for c in CHALLENGES], be.felt(12345))
        assert len(low.code) // 2 == want[layout]["n_instr"]
        assert hashlib.sha256(low.code.astype("<u4").tobytes()).hexdigest() == want[layout]["sha256"], layout
        air.close()
