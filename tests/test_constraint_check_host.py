"""The trace check's host side, without a device: the check program the C++ AIRs lower (one CHECK per constraint over its bare
numerator - LayoutAir::build_check_program, lower_checks) and the per-check domain descriptors, against the Python mirror
(sandstorm_amd/layouts/{recursive,starknet}.py); the composition program's words, which the new lowering must leave alone; the
generated name table."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

P = 2**251 + 17 * 2**192 + 1
CHALLENGES = [pow(7, 11 + 3 * i, P) for i in range(6)]


def host_air(layout):
    """-> (C++ AIR without a context, the mirror's module, its public input, log2 of the layout's smallest trace length here)"""
    from sandstorm_amd import hostlib, public_input
    if layout == "recursive":
        from sandstorm_amd.layouts import recursive as L
        pi = public_input.AirPublicInput.from_json(os.path.join(ROOT, "tests", "golden", "air_public_input_array_sum.json"))
        return hostlib.RecursiveHostAir(None, pi, 18), L, pi, 18
    from sandstorm_amd.layouts import starknet as L
    from test_layout_starknet import bootloader_run
    spi = bootloader_run()[2]
    return hostlib.StarknetHostAir(None, spi, 21), L, spi, 21


def rows_of_descriptor(num, den, n):
    """the membership rule of ss_check_constraints: row r is in the domain iff some den factor (p, e) has p r = e (mod n) and no
    num factor has"""
    r = np.arange(n, dtype=np.uint64)
    in_num, in_den = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for p_, e in num:
        in_num |= (np.uint64(p_) * r - np.uint64(e)) % np.uint64(n) == 0
    for p_, e in den:
        in_den |= (np.uint64(p_) * r - np.uint64(e)) % np.uint64(n) == 0
    return np.nonzero(in_den & ~in_num)[0]


@pytest.mark.parametrize("layout,count", [("recursive", 93), ("starknet", 195)])
def test_check_domains_are_the_mirrors_row_sets(layout, count):
    """(a) number and order of the checks = the mirror's constraints; every check's descriptor selects exactly the rows the mirror
    enforces that constraint on, at the layout's smallest trace length"""
    from sandstorm_amd import backend as be, _lib
    air, L, pi, log_n = host_air(layout)
    n = 1 << log_n
    code, consts, n_slots, desc, domains = air.check_program(n, [be.felt(c) for c in CHALLENGES])
    constraints = L.constraints(L.Hints.from_public_input(pi, CHALLENGES, n), CHALLENGES)
    assert len(domains) == len(constraints) == count
    ops = code[0::2] & 0xFF
    assert [int(w) for w in code[1::2][ops == _lib.OP_CHECK]] == list(range(count))       # CHECK k in order, each once
    assert not (ops == 7).any()                                                           # no OUT
    seen = {}
    for k, ((num, den), c) in enumerate(zip(domains, constraints)):
        assert len(num) <= _lib.CHECK_MAX_FACTORS and len(den) <= _lib.CHECK_MAX_FACTORS
        key = (tuple(num), tuple(den), c.domain.name)
        if key in seen:
            continue
        seen[key] = k
        want = np.fromiter(c.domain.rows(n), dtype=np.int64)
        got = rows_of_descriptor(num, den, n)
        assert len(set(want.tolist())) == len(want)
        assert np.array_equal(np.sort(want), got), (k, c.name, c.domain.name)
    assert len(seen) >= 20
    air.close()


def run_check_program(code, consts, n_slots, cols, r, n, table_at):
    """the two-word program at trace row r in Python integers -> {check index: accumulator at its CHECK}"""
    g = pow(3, (P - 1) // n, P)
    acc, slots, seen = [0, 0, 0, 0], [0] * n_slots, {}
    for w0, w1 in zip(code[0::2].tolist(), code[1::2].tolist()):
        op, d, kind = w0 & 0xFF, (w0 >> 8) & 0xF, (w0 >> 12) & 0xF
        if op <= 4:
            src = (acc[w1] if kind == 0 else slots[w1] if kind == 1 else consts[w1] if kind == 2
                   else cols[w1 >> 24][(r + (w1 & 0xFFFFFF)) % n] if kind == 3 else table_at(w1, r) if kind == 4 else pow(g, r, P))
            acc[d] = (src if op == 0 else acc[d] + src if op == 1 else acc[d] - src if op == 2 else src - acc[d] if op == 3 else acc[d] * src) % P
        elif op == 5:
            acc[d] = pow(acc[d], P - 2, P)
        elif op == 6:
            slots[w1] = acc[d]
        elif op == 10:
            assert w1 not in seen
            seen[w1] = acc[d]
        else:
            raise AssertionError("opcode %d in a check program" % op)
    return seen


def test_check_program_computes_the_mirrors_numerators():
    """(b) the lowered check program, interpreted in Python integers on the example run's trace (the Python generator's base columns,
    the oracle's extension columns), leaves at every CHECK the value the mirror's numerator has there - at the first row, the last
    row and an excluded neighbour of every domain, for all 93 checks at each of those rows"""
    from sandstorm_amd import air_program as ap, backend as be
    from sandstorm_amd.examples import load_run
    from sandstorm_amd.layouts import recursive as rec
    from test_layout_recursive import with_extension
    states, memory, pi = load_run()
    cols, _ = with_extension(rec, rec.base_trace(states, memory, pi), CHALLENGES)
    n = len(cols[0])
    air, _, _, log_n = host_air("recursive")
    assert n == 1 << log_n
    code, consts_mont, n_slots, desc, domains = air.check_program(n, [be.felt(c) for c in CHALLENGES])
    air.close()
    r_inv = pow(1 << 256, -1, P)
    consts = [sum(int(v) << (64 * j) for j, v in enumerate(c)) * r_inv % P for c in consts_mont]
    assert desc == [0, 11, 2048, 11]                                     # the two Pedersen columns, a period of 2048 rows each
    constraints = rec.constraints(rec.Hints.from_public_input(pi, CHALLENGES, n), CHALLENGES)
    rows = set()
    for c in constraints:
        dom = sorted(c.domain.rows(n))
        inside = set(dom)
        rows.update((dom[0], dom[-1]))
        rows.add(next(r % n for r in (dom[0] + 1, dom[0] + 2, dom[-1] + 1, dom[-1] + 2, dom[0] + 3) if r % n not in inside))
    assert len(rows) >= 20
    for r in sorted(rows):
        got = run_check_program(code, consts, n_slots, cols, r, n, lambda t, row: rec.periodic_value(t, row))
        assert sorted(got) == list(range(len(constraints)))
        for k, c in enumerate(constraints):
            want = ap.evaluate(c.numerator, P, None, lambda col, o: cols[col][(r + o) % n], lambda t: rec.periodic_value(t, r))
            assert got[k] == want % P, (r, k, c.name)


def test_composition_program_words_are_the_parents():
    """(c) lower(g, root) is untouched by the multi-root lowering: ssh_air_program returns the words it returned before (the compiled
    constraint kernels are selected by a hash of them) - digests committed from the parent commit"""
    from sandstorm_amd import backend as be, hostlib
    with open(os.path.join(ROOT, "tests", "golden", "air_program_code_digests.json")) as f:
        want = json.load(f)
    for layout in ("recursive", "starknet"):
        air, _, _, log_n = host_air(layout)
        assert log_n == want[layout]["log_n"]
        prog, _, _ = hostlib.prover_air(air).build_program(1 << log_n, [be.felt(c) for c in CHALLENGES], be.felt(12345))
        assert len(prog.code) // 2 == want[layout]["n_instr"]
        assert hashlib.sha256(prog.code.astype("<u4").tobytes()).hexdigest() == want[layout]["sha256"], layout
        air.close()


def test_constraint_name_table_is_not_stale():
    """(d) host/constraint_names.inc is what tools/gen_constraint_names.py writes from the mirror today"""
    import gen_constraint_names as g
    with open(g.OUT) as f:
        assert f.read() == g.render(), "sandstorm_amd/host/constraint_names.inc is stale: run python tools/gen_constraint_names.py"
    assert len(g.names("recursive")) == 93 and len(g.names("starknet")) == 195
