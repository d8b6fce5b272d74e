"""The 64-bit field's trace against the plain AIR on the device (ss_check_constraints_gl64x3: the checking instantiation of
csrc/goldilocks.hip's Fq3 interpreter; goldilocks.check_trace above it; `validate` in goldilocks.Prover and in the C++ host's provers).
Everything compares exactly: the kernel's (first row, count) per constraint against Python integers over Fq3 for a hand-written
program, and against layouts/plain.py failing_rows (with a limit that does not truncate) for whole traces with one corrupted cell.

Runs on the MI355X (`-m gpu`); the kernel-level cases below the two-sweep size and the n = 256 plain cases also run in the CPU suite
on the host build of the device code (tests/test_gl64_constraint_check_on_host.py)."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gl64_programs as gp                                       # noqa: E402
from sandstorm_amd import air_program as ap                      # noqa: E402
from sandstorm_amd import binary as bn                           # noqa: E402
from sandstorm_amd.layouts import plain as pl                    # noqa: E402

pytestmark = pytest.mark.gpu
P = pl.P
NONE = 2**64 - 1
K = (0x123456789ABCDEF, P - 5, 0xFEDCBA9876543)                  # a constant with non-zero upper coordinates
CH = [(11, 22, 33), (5, 6, 7), (9, 8, 7)]


@pytest.fixture(scope="module")
def ctx():
    from sandstorm_amd import backend as be
    c = be.Context(0)
    yield c
    c.close()


def in_domain(num, den, r, n):
    """the membership rule of ss_check_constraints on factor lists"""
    return any((p_ * r - e) % n == 0 for p_, e in den) and not any((p_ * r - e) % n == 0 for p_, e in num)


# ------------------------------------------------------------------------------------------------ the kernel alone
# nine columns, six constraints (a hand-written program: every accumulator, a slot, a constant with non-zero upper coordinates,
# shifted cells, a bare cell as root):
#   0  c0^2 - c0                               every row                       den X^n - 1
#   1  c1[r+1] - c1[r] - 1                     every row but the last          num X - w^(n-1), den X^n - 1
#   2  K (K c2)  (through a slot)              row n - 4                       den X - w^(n-4)
#   3  c3 - c0 * c1[r+1]                       even rows but n - 2             num X - w^(n-2), den X^(n/4) - 1, X^(n/4) - w^(n/2)
#   4  c4  (the root is a bare cell)           every 8th row                   den X^(n/8) - 1
#   5  c5 + X c6 + X^2 c7 - K c8[r+1]          every row (row n - 1 reads c8[0])   den X^n - 1
C1_START, C8_VALUES = 1000, 251
KTAB = [np.array([k * v % P for v in range(C8_VALUES + 2)], dtype=np.uint64) for k in K]


def kernel_program():
    T = ap.trace_payload
    prog = ap.Program()
    one, k, u1, u2 = (prog.const_index(c) for c in ((1, 0, 0), K, (0, 1, 0), (0, 0, 1)))
    I, O, S = ap.instr, ap.OP, ap.SRC
    prog.code = (I(O.MOV, 0, S.TRACE, T(0, 0)) + I(O.MUL, 0, S.ACC, 0) + I(O.SUB, 0, S.TRACE, T(0, 0)) + I(O.CHECK, 0, 0, 0)
                 + I(O.MOV, 1, S.TRACE, T(1, 1)) + I(O.SUB, 1, S.TRACE, T(1, 0)) + I(O.SUB, 1, S.CONST, one) + I(O.CHECK, 1, 0, 1)
                 + I(O.MOV, 0, S.TRACE, T(2, 0)) + I(O.MUL, 0, S.CONST, k) + I(O.ST, 0, 0, 0) + I(O.MOV, 2, S.CONST, k) + I(O.MUL, 2, S.SLOT, 0)
                 + I(O.CHECK, 2, 0, 2)
                 + I(O.MOV, 0, S.TRACE, T(0, 0)) + I(O.MUL, 0, S.TRACE, T(1, 1)) + I(O.RSUB, 0, S.TRACE, T(3, 0)) + I(O.CHECK, 0, 0, 3)
                 + I(O.MOV, 3, S.TRACE, T(4, 0)) + I(O.CHECK, 3, 0, 4)
                 + I(O.MOV, 3, S.TRACE, T(6, 0)) + I(O.MUL, 3, S.CONST, u1) + I(O.MOV, 1, S.TRACE, T(7, 0)) + I(O.MUL, 1, S.CONST, u2)
                 + I(O.ADD, 3, S.ACC, 1) + I(O.ADD, 3, S.TRACE, T(5, 0)) + I(O.MOV, 0, S.TRACE, T(8, 1)) + I(O.MUL, 0, S.CONST, k)
                 + I(O.SUB, 3, S.ACC, 0) + I(O.CHECK, 3, 0, 5))
    prog.n_slots = 1
    return prog


def kernel_domains(n):
    return [([], [(n, 0)]), ([(1, n - 1)], [(n, 0)]), ([], [(1, n - 4)]), ([(1, n - 2)], [(n // 4, 0), (n // 4, n // 2)]), ([], [(n // 8, 0)]),
            ([], [(n, 0)])]


DOMAIN_HAS = [lambda r, n: True, lambda r, n: r != n - 1, lambda r, n: r == n - 4, lambda r, n: r % 2 == 0 and r != n - 2, lambda r, n: r % 8 == 0,
              lambda r, n: True]


def clean_columns(n):
    """numpy columns from closed forms on which every constraint holds on its domain and fails on the rows just outside it"""
    ri = np.arange(n, dtype=np.int64)
    r = ri.astype(np.uint64)
    c0 = ((r * np.uint64(2654435761)) >> np.uint64(7)) & np.uint64(1)
    c1 = np.uint64(C1_START) + r                                             # the step fails at the excluded last row (wrap-around)
    c2 = np.where(ri == n - 4, 0, 7).astype(np.uint64)
    c3 = np.where((ri % 2 == 0) & (ri != n - 2), (c0 * np.roll(c1, -1)).astype(np.int64), 12345).astype(np.uint64)
    c4 = np.where(ri % 8 == 0, 0, 9).astype(np.uint64)
    c8 = (r * np.uint64(48271) + np.uint64(11)) % np.uint64(C8_VALUES) + np.uint64(1)
    nxt = np.roll(c8, -1).astype(np.int64)
    return [c0, c1, c2, c3, c4, KTAB[0][nxt], KTAB[1][nxt], KTAB[2][nxt], c8]


def numerators(cols, r, n):
    """the six numerators at row r in Python integers over Fq3"""
    c = lambda j, o=0: int(cols[j][(r + o) % n])
    return [((c(0) * c(0) - c(0)) % P, 0, 0), ((c(1, 1) - c(1) - 1) % P, 0, 0), pl.mul3(K, pl.mul3(K, (c(2), 0, 0))),
            ((c(3) - c(0) * c(1, 1)) % P, 0, 0), (c(4) % P, 0, 0),
            pl.sub3((c(5) % P, c(6) % P, c(7) % P), pl.scale3(K, c(8, 1)))]


def python_report(cols, n, rows=None):
    """(first row, count) per constraint from Python integers - over every row, or over `rows` where nothing else can have changed"""
    bad = [[] for _ in range(6)]
    for r in (range(n) if rows is None else sorted(set(rows))):
        for k, v in enumerate(numerators(cols, r, n)):
            if DOMAIN_HAS[k](r, n) and any(v):
                bad[k].append(r)
    return [b[0] if b else NONE for b in bad], [len(b) for b in bad]


def device_report(ctx, cols, n, program=None, domains=None):
    prog = program or kernel_program()
    dev = [ctx.column(c) for c in cols]
    try:
        first, count = ctx.check_constraints_gl64x3(np.array(prog.code, dtype=np.uint32), np.array(prog.consts, dtype=np.uint64).reshape(-1, 3),
                                                    prog.n_slots, None, [], dev, n.bit_length() - 1, domains or kernel_domains(n))
    finally:
        for d in dev:
            d.free()
    return [int(v) for v in first], [int(v) for v in count]


SIZES = [pytest.param(4, id="2p4"), pytest.param(7, id="2p7"), pytest.param(10, id="2p10"), pytest.param(21, id="2p21_two_sweeps")]


@pytest.mark.parametrize("log_n", SIZES)
def test_kernel_reports_what_python_integers_give(ctx, log_n):
    """n = 2^4 (less than one wave), 2^7 (a partial workgroup), 2^10, 2^21 (two sweeps of the launch's 2^20 lanes).  A clean trace
    reports nothing - the violations at excluded rows are not reported.  Then violations planted at row 0, rows 63 / 64 (one wave and
    the next), 255 / 256, the last row and in the second sweep; one that lives only in coordinate 1 of an Fq3 numerator and one only in
    coordinate 2; one at the last row reached through wrap-around; one only at an excluded row.  Then every row violating constraint 0.
    At 2^21 the expected report is evaluated at the rows that read a corrupted cell (every other row is a clean one)."""
    n = 1 << log_n
    small = n <= 1 << 10
    cols = clean_columns(n)
    if small:
        for k, dom in enumerate(kernel_domains(n)):                            # the descriptors say what the predicates say
            assert [in_domain(dom[0], dom[1], r, n) for r in range(n)] == [DOMAIN_HAS[k](r, n) for r in range(n)]
        assert python_report(cols, n) == ([NONE] * 6, [0] * 6)
    assert device_report(ctx, cols, n) == ([NONE] * 6, [0] * 6)

    def report_after(cells):
        """corrupt the cells {(column, row): new value} of a clean trace -> (expected, device)"""
        c = clean_columns(n)
        for (j, r), v in cells.items():
            c[j][r] = v
        touched = [(r - o) % n for (_, r) in cells for o in (0, 1)]
        want = python_report(c, n, touched)
        if small:
            assert want == python_report(c, n)
        return want, device_report(ctx, c, n)
    # only coordinate 1, only coordinate 2 of the numerator of constraint 5
    for col, row in ((6, 5), (7, n - 2)):
        want, got = report_after({(col, row): (int(cols[col][row]) + 1) % P})
        assert want == ([NONE] * 5 + [row], [0] * 5 + [1]) and got == want, (col, want, got)
    # the last row, reached through wrap-around: c8[0] is read by row n - 1 alone
    want, got = report_after({(8, 0): C8_VALUES + 1})
    assert want == ([NONE] * 5 + [n - 1], [0] * 5 + [1]) and got == want, (want, got)
    # many at once
    planted = [r for r in (0, n - 1, 63, 64, 255, 256, (1 << 20) + 12345, (1 << 20) + 64 * 1000 + 63) if r < n]
    cells = {(0, r): 2 + r for r in planted}                     # constraint 0 at r, constraint 3 where r is an even row of its domain
    cells[(1, n // 2)] = int(cols[1][n // 2]) + 3                # the step into and out of row n / 2
    cells[(2, n - 4)] = 5
    cells[(2, n - 3)] = 11                                       # only at a row no constraint covers: not reported
    cells[(4, 8 * (n // 16))] = 1
    cells[(4, n - 1)] = 0                                        # (an excluded row that now holds: nothing changes)
    cells[(6, 5)] = (int(cols[6][5]) + 1) % P
    cells[(7, n - 2)] = (int(cols[7][n - 2]) + 1) % P
    cells[(8, 0)] = C8_VALUES + 1
    want, got = report_after(cells)
    assert want[1][0] == len(planted) and want[0][0] == 0 and want[1][1] == 2 and want[0][2] == n - 4 and want[1][4] == 1
    assert want[0][5] == 5 and want[1][5] == 3
    assert got == want, (want, got)
    # every row violates constraint 0 (and constraint 3 on all of its domain: 2 c1 is never c0 c1): the counts are the domains' sizes
    c = clean_columns(n)
    c[0][:] = 2
    want = ([0, NONE, NONE, 0, NONE, NONE], [n, 0, 0, n // 2 - 1, 0, 0])
    if small:
        assert python_report(c, n) == want
    assert device_report(ctx, c, n) == want


def test_kernel_refusals(ctx):
    """an OUT in the program, a missing check index, a repeated one, one out of range, a domain of 17 factors, a constant that is no
    element of the field - and a CHECK program handed to ss_eval_quotient_gl64x3: all refused by message, nothing launched"""
    from sandstorm_amd._lib import SandstormHipError, CHECK_MAX_FACTORS
    n = 16
    cols = clean_columns(n)
    doms = kernel_domains(n)

    def run(code, domains=doms, consts=None):
        prog = kernel_program()
        prog.code = code
        if consts is not None:
            prog.consts = consts
        return device_report(ctx, cols, n, prog, domains)
    good = kernel_program().code
    assert run(good)[1] == [0] * 6
    with pytest.raises(SandstormHipError, match="OUT in a check program"):
        run(good + ap.instr(ap.OP.OUT, 0, 0, 0))
    with pytest.raises(SandstormHipError, match="check 5 does not appear"):
        run(good[:-2])
    with pytest.raises(SandstormHipError, match="check 3 appears twice"):
        run(good[:-1] + [3])
    with pytest.raises(SandstormHipError, match="check 6 out of range"):
        run(good[:-1] + [6])
    wide = ([], [(1, k) for k in range(CHECK_MAX_FACTORS + 1)])
    assert len(wide[1]) == 17
    with pytest.raises(SandstormHipError, match="17 denominator factors exceeds SS_CHECK_MAX_FACTORS"):
        run(good, doms[:5] + [wide])
    with pytest.raises(SandstormHipError, match="constant 1 is not an element of the extension"):
        run(good, consts=[(1, 0, 0), (K[0], P, K[2]), (0, 1, 0), (0, 0, 1)])
    dev = [ctx.column(c) for c in cols]
    out = ctx.alloc(24 * 2 * n)
    prog = kernel_program()
    with pytest.raises(SandstormHipError, match="bad opcode"):
        ctx.eval_quotient_gl64x3(np.array(prog.code, dtype=np.uint32), np.array(prog.consts, dtype=np.uint64), prog.n_slots, None, [], dev, 4, 0, 7, out)
    out.free()
    for d in dev:
        d.free()


# ------------------------------------------------------------------------------------------------ the plain layout
RUNS = {"example_16": ("example", 16), "example_64": ("example", 64), "busy_64": ("busy", 64)}


@functools.lru_cache(maxsize=None)
def run_of(key):
    """-> (public input, the 8 component columns as lists of ints for CH, n, states, memory): made once, never changed"""
    name, cycles = RUNS[key]
    prog = pl.example_program(2 if cycles == 16 else 10) if name == "example" else gp.busy_program(6)
    if name == "busy":
        assert gp.busy_cycles(6) < cycles
    states, memory = pl.run(prog, cycles)
    pi = pl.public_input_of(prog, states, memory)
    cols = pl.base_trace(states, memory, pi)
    ext, _ = pl.extension_columns(cols, CH)
    return pi, tuple(tuple(c) for c in cols + ext), len(cols[0]), states, memory


def corruptions(n):
    """(name, component column, row): spread over every base column, every extension coordinate column, the first row, the last
    cycle, a range-check ordered value and `res` of the loop's multiplication"""
    B = pl.NUM_BASE_COLUMNS
    return [("flags", pl.COL_FLAGS, 16 * 3 + 2), ("npc", pl.COL_NPC, 16 * 5 + pl.Npc.MEM_DST), ("memory", pl.COL_MEMORY, 2 * 20 + pl.Mem.VALUE),
            ("range_check", pl.COL_RANGE_CHECK, 16 * 4 + pl.RangeCheck.OFF_OP1), ("auxiliary", pl.COL_AUXILIARY, 16 * 2 + pl.Auxiliary.TMP0[1]),
            ("perm_c0", B, 8), ("perm_c1", B + 1, 13), ("perm_c2", B + 2, n - 2),
            ("first_row", pl.COL_NPC, 0), ("last_cycle", pl.COL_RANGE_CHECK, n - 16 + pl.Auxiliary.AP[1]),
            ("rc_ordered", pl.COL_RANGE_CHECK, 4 * 9 + pl.RangeCheck.ORDERED), ("res", pl.COL_RANGE_CHECK, 16 * 2 + pl.Auxiliary.RES[1])]


def mirror_report(pi, cols8, n, challenges):
    """plain.failing_rows over all 47 constraints, with a limit that does not truncate -> [(index, name, domain, first row, count)]"""
    out = []
    for k, c in enumerate(pl.constraints(pl.Hints.from_public_input(pi, challenges, n), challenges)):
        bad = sorted(pl.failing_rows(c, cols8, n, limit=n + 1))
        if bad:
            out.append((k, c.name, c.domain.name, bad[0], len(bad)))
    return out


def device_check(ctx, pi, cols8):
    from sandstorm_amd import goldilocks as gs
    dev = [ctx.column(np.array(c, dtype=np.uint64)) for c in cols8]
    try:
        return gs.check_trace(ctx, gs.plain_air(), dev, CH, pi)
    finally:
        for d in dev:
            d.free()


@pytest.mark.parametrize("key", list(RUNS))
def test_plain_clean_trace_satisfies_the_air(ctx, key):
    pi, cols8, n, _, _ = run_of(key)
    assert device_check(ctx, pi, cols8) == []


@pytest.mark.parametrize("case", range(12), ids=[c[0] for c in corruptions(256)])
@pytest.mark.parametrize("key", list(RUNS))
def test_plain_corrupted_cell_is_reported_as_the_mirror_reports_it(ctx, key, case):
    pi, cols8, n, _, _ = run_of(key)
    _, col, row = corruptions(n)[case]
    bad = [list(c) for c in cols8]
    bad[col][row] = (bad[col][row] + 1) % P
    want = mirror_report(pi, bad, n, CH)
    assert want, "the corrupted cell is read by no constraint"
    assert device_check(ctx, pi, bad) == want


def test_cpp_host_reports_what_the_python_host_reports(ctx):
    """hostlib.gl_check_trace (ssh_gl_check_trace: the check program through the callback's blob, gl::check_trace) on a clean and on a
    corrupted trace"""
    from sandstorm_amd import goldilocks as gs, hostlib
    pi, cols8, n, _, _ = run_of("example_64")
    bad = [list(c) for c in cols8]
    bad[pl.COL_RANGE_CHECK][16 * 2 + pl.Auxiliary.RES[1]] += 1
    for cols, clean in ((cols8, True), (bad, False)):
        dev = [ctx.column(np.array(c, dtype=np.uint64)) for c in cols]
        got = hostlib.gl_check_trace(ctx, gs.plain_air(), dev, CH, pi)
        assert got == gs.check_trace(ctx, gs.plain_air(), dev, CH, pi) and (got == []) == clean
        for d in dev:
            d.free()
    assert "cpu/operands/res" in [g[1] for g in got]


# ------------------------------------------------------------------------------------------------ the provers
@pytest.fixture(scope="module")
def env():
    """(context, torch device): the context on the stream torch works on"""
    import torch
    from sandstorm_amd import backend as be
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    c = be.Context(0, stream=stream.cuda_stream)
    yield c, dev
    c.close()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))


SEED = bytes(range(32))


def golden_arrays():
    """the proof of the example run the parent commit writes (tests/golden/goldilocks_plain_proof.npz: made on the MI355X)"""
    with np.load(os.path.join(ROOT, "tests", "golden", "goldilocks_plain_proof.npz")) as f:
        return {k: f[k] for k in f.files}


def assert_same_arrays(proof, want):
    from sandstorm_amd import goldilocks as gs
    got = gs.proof_to_arrays(proof)
    assert set(got) == set(want)
    for k in sorted(want):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k


def prove_columns(env, columns, pi, seen=None, **kw):
    """Prover.prove on host-made columns; `seen` collects the challenges the proof drew"""
    import torch
    from sandstorm_amd import goldilocks as gs
    c, dev = env
    base = [torch.from_numpy(np.array(col, dtype=np.uint64).view(np.int64)).to(dev) for col in columns]

    def extension(ch):
        if seen is not None:
            seen.append([tuple(int(v) for v in x) for x in ch])
        return gs.plain_extension_on_device(c, base, ch)[0]
    opt = gs.Options(num_queries=20, grinding=8)
    return gs.Prover(c, gs.plain_air(), opt, **kw.pop("init", {})).prove(SEED, base, extension, statement=pi, **kw)


def test_provers_clean_run_writes_the_same_proof_with_and_without_validation(env):
    """Prover.prove and prove_files, validation off and on: array for array the proof the parent commit wrote for this run"""
    from sandstorm_amd import goldilocks as gs
    c, dev = env
    pi, cols8, n, states, memory = run_of("example_64")
    want = golden_arrays()
    opt = gs.Options(num_queries=20, grinding=8)
    assert_same_arrays(prove_columns(env, cols8[:5], pi), want)                                    # validate=False: the parent's arrays
    assert_same_arrays(prove_columns(env, cols8[:5], pi, init={"validate": True}), want)
    assert_same_arrays(prove_columns(env, cols8[:5], pi, validate=True), want)
    trace_bin, memory_bin = bn.write_register_states(states), bn.write_memory(memory)
    assert_same_arrays(gs.prove_files(c, trace_bin, memory_bin, pi, SEED, opt), want)
    assert_same_arrays(gs.prove_files(c, trace_bin, memory_bin, pi, SEED, opt, validate=True), want)


def test_provers_stop_at_a_corrupted_cell_and_name_it(env):
    """the value the loop's first multiplication writes, changed in memory: the trace generators (host and device) make the same base
    columns from it, the permutations close, and `dst = res` fails.  Both provers stop before the extension commitment with the message
    naming the mirror's first failing constraint, row and count for the proof's own challenges; no proof exists; the same context then
    proves the clean statement"""
    from sandstorm_amd import goldilocks as gs
    from sandstorm_amd._lib import SandstormHipError
    c, dev = env
    pi, cols8, n, states, memory = run_of("example_64")
    address = cols8[pl.COL_NPC][16 * 2 + pl.Npc.MEM_DST_ADDR]
    assert address not in [a for a, _ in pi.public_memory]
    wrong = list(memory)                                         # (indexed by address)
    wrong[address] = (wrong[address] + 1) % P
    base = pl.base_trace(states, wrong, pi)
    assert [list(x) for x in base] != [list(x) for x in cols8[:5]]
    seen = []
    proof = None
    with pytest.raises(ValueError) as e:
        proof = prove_columns(env, base, pi, seen, validate=True)
    assert proof is None and len(seen) == 1
    ext, _ = pl.extension_columns(base, seen[0], check=False)
    mirror = mirror_report(pi, [list(x) for x in base] + ext, n, seen[0])
    assert mirror
    message = gs.describe_failures(mirror)
    assert message.startswith("trace does not satisfy the AIR: %d constraint" % len(mirror)) and "; first: #%d %s (%s) at row %d, %d row" % mirror[0] in message
    assert str(e.value) == message
    opt = gs.Options(num_queries=20, grinding=8)
    with pytest.raises(SandstormHipError) as e:
        proof = gs.prove_files(c, bn.write_register_states(states), bn.write_memory(wrong), pi, SEED, opt, validate=True)
    assert proof is None and str(e.value).endswith(message), str(e.value)
    # nothing was committed that is in the way: the clean statement is proved as before, by both
    want = golden_arrays()
    assert_same_arrays(prove_columns(env, cols8[:5], pi, validate=True), want)
    assert_same_arrays(gs.prove_files(c, bn.write_register_states(states), bn.write_memory(memory), pi, SEED, opt, validate=True), want)
