"""The trace against its AIR on the device (ss_check_constraints: the checking instantiation of csrc/quotient.hip's interpreter;
ssh::check_trace above it; Air::validate_trace in the provers).  Everything compares exactly: the kernel's (first row, count) per
constraint against Python integers for hand-written programs, and against the layouts' Python mirror
(sandstorm_amd/layouts/{recursive,starknet}.py) for whole traces with one corrupted cell.

Runs on the MI355X (`-m gpu`); the kernel-level cases and the recursive layout's also run in the CPU suite on the host build of the
device code (tests/test_constraint_check_on_host.py)."""
import gzip
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

P = 2**251 + 17 * 2**192 + 1
R = (1 << 256) % P
R_INV = pow(1 << 256, -1, P)
NONE = 2**64 - 1
CHALLENGES = [pow(7, 11 + 3 * i, P) for i in range(6)]


@pytest.fixture(scope="module")
def ctx():
    from sandstorm_amd import backend as be
    c = be.Context(0)
    yield c
    c.close()


def to_mont(values):
    """python ints -> uint64[n, 4] Montgomery limbs (few distinct values, or a long run of them: both cheap)"""
    cache = {}
    raw = bytearray()
    for v in values:
        b = cache.get(v)
        if b is None:
            b = cache[v] = (v % P * R % P).to_bytes(32, "little")
        raw += b
    return np.frombuffer(bytes(raw), dtype="<u8").astype(np.uint64).reshape(-1, 4)


def from_limbs(limbs):
    return sum(int(v) << (64 * j) for j, v in enumerate(limbs)) * R_INV % P


def poke(ctx, ptr, row, value):
    a = to_mont([value])
    from sandstorm_amd import backend as be
    be.check(ctx.lib.ss_upload(ctx.handle, be._ptr_of(ptr) + 32 * row, a.ctypes.data, 32))


def peek(ctx, ptr, row):
    from sandstorm_amd import backend as be
    a = np.empty(4, dtype=np.uint64)
    be.check(ctx.lib.ss_download(ctx.handle, a.ctypes.data, be._ptr_of(ptr) + 32 * row, 32))
    return from_limbs(a)


def in_domain(num, den, r, n):
    """the membership rule of ss_check_constraints on the mirror's factor lists"""
    return any((p_ * r - e) % n == 0 for p_, e in den) and not any((p_ * r - e) % n == 0 for p_, e in num)


# ------------------------------------------------------------------------------------------------ the kernel alone
# five columns, five constraints (a hand-written program: every accumulator, a slot, a constant, shifted cells, a bare cell):
#   0  c0^2 - c0                    every row                                  den X^n - 1
#   1  c1[r+1] - c1[r] - 1          every row but the last                     num X - g^(n-1), den X^n - 1
#   2  c2                           row n - 4                                  den X - g^(n-4)
#   3  c3 - c0 * c1[r+1]            even rows but n - 2                        num X - g^(n-2), den X^(n/4) - 1, X^(n/4) - g^(n/2)
#   4  c4  (the root is a bare cell)  every 8th row                            den X^(n/8) - 1
C1_START = 1000


def kernel_program():
    from sandstorm_amd import air_program as ap
    T = ap.trace_payload
    prog = ap.Program()
    one = prog.const_index(1)
    I, O, S = ap.instr, ap.OP, ap.SRC
    prog.code = (I(O.MOV, 0, S.TRACE, T(0, 0)) + I(O.MUL, 0, S.ACC, 0) + I(O.SUB, 0, S.TRACE, T(0, 0)) + I(O.CHECK, 0, 0, 0)
                 + I(O.MOV, 1, S.TRACE, T(1, 1)) + I(O.SUB, 1, S.TRACE, T(1, 0)) + I(O.SUB, 1, S.CONST, one) + I(O.CHECK, 1, 0, 1)
                 + I(O.MOV, 0, S.TRACE, T(2, 0)) + I(O.ST, 0, 0, 0) + I(O.MOV, 2, S.SLOT, 0) + I(O.CHECK, 2, 0, 2)
                 + I(O.MOV, 0, S.TRACE, T(0, 0)) + I(O.MUL, 0, S.TRACE, T(1, 1)) + I(O.RSUB, 0, S.TRACE, T(3, 0)) + I(O.CHECK, 0, 0, 3)
                 + I(O.MOV, 3, S.TRACE, T(4, 0)) + I(O.CHECK, 3, 0, 4))
    prog.n_slots = 1
    return prog


def kernel_domains(n):
    return [([], [(n, 0)]), ([(1, n - 1)], [(n, 0)]), ([], [(1, n - 4)]), ([(1, n - 2)], [(n // 4, 0), (n // 4, n // 2)]), ([], [(n // 8, 0)])]


def kernel_domain_rows(n):
    return [range(n), range(n - 1), [n - 4], [r for r in range(0, n, 2) if r != n - 2], range(0, n, 8)]


def clean_columns(n):
    """python-int columns on which every constraint holds on its domain and fails on the rows just outside it"""
    c0 = [(r * 2654435761 >> 7) & 1 for r in range(n)]
    c1 = [C1_START + r for r in range(n)]                                    # the step fails at the excluded last row (wrap-around)
    c2 = [0 if r == n - 4 else 7 for r in range(n)]
    c3 = [c0[r] * c1[(r + 1) % n] if r % 2 == 0 and r != n - 2 else 12345 for r in range(n)]
    c4 = [0 if r % 8 == 0 else 9 for r in range(n)]
    return [c0, c1, c2, c3, c4]


def python_report(cols, n):
    c0, c1, c2, c3, c4 = cols
    numerators = [lambda r: c0[r] * c0[r] - c0[r], lambda r: c1[(r + 1) % n] - c1[r] - 1, lambda r: c2[r],
                  lambda r: c3[r] - c0[r] * c1[(r + 1) % n], lambda r: c4[r]]
    first, count = [], []
    for rows, f in zip(kernel_domain_rows(n), numerators):
        bad = [r for r in rows if f(r) % P]
        first.append(bad[0] if bad else NONE)
        count.append(len(bad))
    return first, count


def device_report(ctx, cols, n):
    dev = [ctx.column(to_mont(c)) for c in cols]
    first, count = ctx.check_constraints(kernel_program(), None, [], dev, n.bit_length() - 1, kernel_domains(n))
    for d in dev:
        d.free()
    return [int(v) for v in first], [int(v) for v in count]


SIZES = [pytest.param(4, id="2p4"), pytest.param(7, id="2p7"), pytest.param(10, id="2p10"), pytest.param(19, id="2p19_two_sweeps")]


@pytest.mark.parametrize("log_n", SIZES)
def test_kernel_reports_what_python_integers_give(ctx, log_n):
    """n = 2^4 (a partly filled wave), 2^7 (half a workgroup), 2^10, 2^19 (two sweeps of the 2^18-lane grid): a clean trace reports
    nothing - the violations at excluded rows (the step at row n - 1, c3 at n - 2 and at odd rows, c2 and c4 off their rows) are not
    reported; then violations planted at row 0, row n - 1, rows 63 / 64 and 255 / 256 and in the second sweep, plus one only at an
    excluded row; then every row violating constraint 0"""
    n = 1 << log_n
    cols = clean_columns(n)
    for rows, dom in zip(kernel_domain_rows(n), kernel_domains(n)):            # the descriptors say what the row lists say
        if n <= 1 << 10:
            assert [r for r in range(n) if in_domain(dom[0], dom[1], r, n)] == list(rows)
    want = python_report(cols, n)
    assert want == ([NONE] * 5, [0] * 5)
    assert device_report(ctx, cols, n) == want
    planted = [r for r in (0, n - 1, 63, 64, 255, 256, (1 << 18) + 12345, (1 << 18) + 64 * 1000 + 63) if r < n]
    for r in planted:
        cols[0][r] = 2 + r                                  # constraint 0 at r, constraint 3 where r is an even row of its domain
    cols[1][n // 2] += 3                                    # the step into and out of row n / 2
    cols[2][n - 4] = 5
    cols[2][n - 3] = 11                                     # only at a row no constraint covers: not reported
    cols[4][8 * (n // 16)] = 1
    cols[4][n - 1] = 0                                      # (an excluded row that now holds: nothing changes)
    want = python_report(cols, n)
    assert want[1][0] == len(planted) and want[0][0] == 0 and want[1][1] == 2 and want[0][2] == n - 4 and want[1][4] == 1
    assert device_report(ctx, cols, n) == want
    cols = clean_columns(n)
    cols[0] = [2] * n                                       # every row violates constraint 0: count = |domain|
    want = python_report(cols, n)
    assert want[1][0] == n and want[0][0] == 0
    assert device_report(ctx, cols, n) == want


def test_kernel_refusals(ctx):
    """a CHECK index out of range, a duplicated check, a missing one, a program with OUT, a domain beyond SS_CHECK_MAX_FACTORS - and a
    CHECK program handed to ss_eval_quotient: all refused by name, nothing launched"""
    from sandstorm_amd import air_program as ap, backend as be
    from sandstorm_amd._lib import SandstormHipError, CHECK_MAX_FACTORS
    n = 16
    dev = [ctx.column(to_mont(c)) for c in clean_columns(n)]
    doms = kernel_domains(n)

    def run(code, domains=doms):
        prog = kernel_program()
        prog.code = code
        return ctx.check_constraints(prog, None, [], dev, 4, domains)
    good = kernel_program().code
    assert [int(v) for v in run(good)[1]] == [0] * 5
    with pytest.raises(SandstormHipError, match="check 5 out of range"):
        run(good[:-1] + [5])
    with pytest.raises(SandstormHipError, match="check 3 appears twice"):
        run(good[:-1] + [3])
    with pytest.raises(SandstormHipError, match="check 4 does not appear"):
        run(good[:-2])
    with pytest.raises(SandstormHipError, match="OUT in a check program"):
        run(good + ap.instr(ap.OP.OUT, 0, 0, 0))
    wide = ([], [(1, k) for k in range(CHECK_MAX_FACTORS + 1)])
    with pytest.raises(SandstormHipError, match="SS_CHECK_MAX_FACTORS"):
        run(good, doms[:4] + [wide])
    out = ctx.alloc(32 * 2 * n)
    with pytest.raises(SandstormHipError, match="bad opcode"):
        ctx.eval_quotient(kernel_program(), None, [], dev, 4, 0, be.felt(3), out)
    with pytest.raises(SandstormHipError, match="bad opcode"):
        ctx.eval_quotient_rows(kernel_program(), None, [], dev, 4, 0, be.felt(3), 0, 8, 16, out)
    out.free()
    for d in dev:
        d.free()


# ------------------------------------------------------------------------------------------------ whole layouts
def mask_of(expr):
    cells, seen, stack = set(), set(), [expr]
    while stack:
        e = stack.pop()
        if e._id in seen:
            continue
        seen.add(e._id)
        if e.kind == "trace":
            cells.add(tuple(e.args))
        elif e.kind in ("add", "sub", "mul", "inv"):
            stack.extend(e.args)
    return cells


class DeviceTrace:
    """base + extension columns in HBM and the mirror's constraints; cells are read from the device on demand (exact integers)"""

    def __init__(self, ctx, L, air, cols, n, constraints):
        self.ctx, self.L, self.air, self.cols, self.n, self.constraints = ctx, L, air, cols, n, constraints
        self.cache, self.masks = {}, [mask_of(c.numerator) for c in constraints]

    def cell(self, c, r):
        if (c, r) not in self.cache:
            self.cache[(c, r)] = peek(self.ctx, self.cols[c], r)
        return self.cache[(c, r)]

    def report(self):
        from sandstorm_amd import backend as be, hostlib
        return hostlib.check_trace(self.ctx, self.air, self.cols, self.n.bit_length() - 1, [be.felt(c) for c in CHALLENGES])

    def expected_after(self, col, row, value):
        """what the mirror says of the trace with cell (col, row) replaced by `value`: per constraint, the rows of its domain that
        read that cell through its own mask and where its numerator is then not zero - no other row can have changed"""
        from sandstorm_amd import air_program as ap
        n, out = self.n, []
        for k, c in enumerate(self.constraints):
            cand = sorted({(row - off) % n for cc, off in self.masks[k] if cc == col})
            num, den = c.domain.num(n), c.domain.den(n)
            bad = []
            for r in cand:
                if not in_domain(num, den, r, n):
                    continue
                v = ap.evaluate(c.numerator, P, None, lambda cc, o: value if (cc, (r + o) % n) == (col, row) else self.cell(cc, (r + o) % n),
                                lambda t: self.L.periodic_value(t, r))
                if v % P:
                    bad.append(r)
            if bad:
                out.append((k, c.name, c.domain.name, bad[0], len(bad)))
        return out

    def corrupt_and_compare(self, col, row):
        old = self.cell(col, row)
        new = (old + 5) % P
        want = self.expected_after(col, row, new)
        poke(self.ctx, self.cols[col], row, new)
        try:
            got = self.report()
        finally:
            poke(self.ctx, self.cols[col], row, old)
        assert got == want, (col, row)
        return want


@pytest.fixture(scope="module")
def recursive_trace(ctx):
    """the reference's example run (2^14 steps, n = 2^18: the smallest size the layout's pools admit): the base trace made on the
    device, the extension columns by the C++ host's build_extension_columns at fixed challenges"""
    from sandstorm_amd import backend as be, hostlib
    from sandstorm_amd.layouts import recursive as rec
    from test_gpu_device_trace import example_files
    trace_bin, memory_bin, pi = example_files()
    n = 16 * (len(trace_bin) // 24)
    dev = hostlib.device_base_trace(ctx, "recursive", trace_bin, memory_bin, pi, None)
    aux = [dev[c] for c in (rec.COL_NPC, rec.COL_MEMORY, rec.COL_RANGE_CHECK, rec.COL_DILUTED_UNORDERED, rec.COL_DILUTED_ORDERED)]
    ext = hostlib.build_extension_columns(ctx, "recursive", aux, n, [be.felt(c) for c in CHALLENGES])
    air = hostlib.RecursiveHostAir(ctx, pi, n.bit_length() - 1)
    constraints = rec.constraints(rec.Hints.from_public_input(pi, CHALLENGES, n), CHALLENGES)
    yield DeviceTrace(ctx, rec, air, dev + ext.cols, n, constraints)
    air.close()
    ext.close()
    for d in dev:
        d.free()


def test_recursive_example_run_satisfies_all_93_constraints(recursive_trace):
    assert recursive_trace.n == 1 << 18 and len(recursive_trace.constraints) == 93
    assert recursive_trace.report() == []


def recursive_cells():
    from sandstorm_amd.layouts import recursive as rec
    cycle_row = 16 * 1234
    cells = [(rec.COL_AUXILIARY, rec.Auxiliary.RES), (rec.COL_AUXILIARY, rec.Auxiliary.AP), (rec.COL_NPC, rec.Npc.PC),
             (rec.COL_RANGE_CHECK, rec.RangeCheck.OFF_OP0), (rec.COL_FLAGS, 3), (rec.COL_MEMORY, 1), (rec.COL_RANGE_CHECK, rec.RangeCheck.ORDERED),
             (rec.COL_MEM_RC_PERMUTATION, 0), (rec.COL_NPC, rec.Npc.UNUSED_ADDR)]
    # ... and AUX_AP of cycle 0, which the ..._EXCEPT_LAST constraints read at their excluded last cycle through wrap-around
    return [(col, cycle_row + cell) for col, cell in cells] + [(rec.COL_AUXILIARY, rec.Auxiliary.AP)]


@pytest.mark.parametrize("case", range(10))
def test_recursive_corrupted_cell_is_reported_as_the_mirror_predicts(recursive_trace, case):
    """the nine cells of tests/test_layout_recursive.py test_a_corrupted_cell_trips_its_constraints, and the first cycle's ap: index,
    name, domain, first row and count of every failing constraint; every other constraint clean"""
    col, row = recursive_cells()[case]
    want = recursive_trace.corrupt_and_compare(col, row)
    assert want, "the mirror trips no constraint for this cell"
    if case == 9:
        assert all(first != recursive_trace.n - 16 for _, _, _, first, _ in want)          # the excluded last cycle is not reported


STARKNET_BUILTINS = ["pedersen/", "rc_builtin/", "ecdsa/", "bitwise/", "ec_op/", "poseidon/"]


def starknet_cell(trace, prefix):
    """a cell of the builtin's own columns (not the memory pair): of the first constraint of that builtin that is enforced on more
    than two rows and reads such a cell, at the second row of its domain"""
    import itertools
    L, n = trace.L, trace.n
    for k, c in enumerate(trace.constraints):
        own = sorted(cell for cell in trace.masks[k] if cell[0] not in (L.COL_NPC, L.COL_MEMORY))
        if not c.name.startswith(prefix) or not own or all(p_ == 1 for p_, _ in c.domain.den(n)):
            continue
        second = next(itertools.islice(iter(c.domain.rows(n)), 1, 2))
        col, off = own[-1]
        return col, (second + off) % n
    raise AssertionError(prefix)


@pytest.fixture(scope="module")
def starknet_trace(ctx):
    """the reference's bootloader run (2^17 steps, the smallest the layout admits) with real instances of every builtin"""
    from sandstorm_amd import backend as be, hostlib
    from sandstorm_amd.layouts import starknet as sk
    from test_layout_starknet import real_instances, bootloader_run
    g = os.path.join(ROOT, "tests", "golden")
    with gzip.open(os.path.join(g, "bootloader", "trace.bin.gz")) as f:
        trace_bin = f.read()
    with gzip.open(os.path.join(g, "bootloader", "memory.bin.gz")) as f:
        memory_bin = f.read()
    _, _, pi, priv = bootloader_run()
    both = dict(real_instances(), pedersen=priv["pedersen"])
    n = 16 * (len(trace_bin) // 24)
    dev = hostlib.device_base_trace(ctx, "starknet", trace_bin, memory_bin, pi, both)
    ext = hostlib.build_extension_columns(ctx, "starknet", [dev[sk.COL_NPC], dev[sk.COL_MEMORY], dev[sk.COL_RANGE_CHECK]], n, [be.felt(c) for c in CHALLENGES])
    air = hostlib.StarknetHostAir(ctx, pi, n.bit_length() - 1)
    constraints = sk.constraints(sk.Hints.from_public_input(pi, CHALLENGES, n), CHALLENGES)
    yield DeviceTrace(ctx, sk, air, dev + ext.cols, n, constraints)
    air.close()
    ext.close()
    for d in dev:
        d.free()


def test_starknet_bootloader_run_satisfies_all_195_constraints(starknet_trace):
    assert starknet_trace.n == 1 << 21 and len(starknet_trace.constraints) == 195
    assert starknet_trace.report() == []


@pytest.mark.parametrize("prefix", STARKNET_BUILTINS)
def test_starknet_corrupted_builtin_cell_is_reported_as_the_mirror_predicts(starknet_trace, prefix):
    col, row = starknet_cell(starknet_trace, prefix)
    want = starknet_trace.corrupt_and_compare(col, row)
    assert want and any(name.startswith(prefix) for _, name, _, _, _ in want), (prefix, col, row, want)


# ------------------------------------------------------------------------------------------------ the provers
def test_prover_with_validation(ctx):
    """recursive, 2^14 steps, files -> proof through the device generator: with validation on a clean proof is the proof with it off,
    byte for byte; with a cell patched on the device after the base commitment the proof is refused with the
    constraint, domain, row and count the mirror names, and nothing is written; the sharded prover refuses an AIR with validation on.
    (The Eth claim's parts - Keccak trees, Solidity coin: a Pedersen-topped tree would build the library's process-wide 23.6 GB Pedersen
    table in front of the full-size tests that run later in the same process and need the whole card.)"""
    from sandstorm_amd import backend as be, binary, hostlib, public_input
    from sandstorm_amd._lib import SandstormHipError
    from sandstorm_amd.examples import recursive_example
    from sandstorm_amd.layouts import recursive as rec
    states, memory, pi = recursive_example(14)
    trace_bin, memory_bin = binary.write_register_states(states), binary.write_memory(memory)
    log_n = 18
    n = 1 << log_n
    dev = [ctx.alloc(32 * n) for _ in range(7)]
    air = hostlib.RecursiveHostAir(ctx, pi, log_n)
    seed = public_input.public_coin_seed(pi, be.COIN_SOLIDITY)
    aux_idx = (rec.COL_NPC, rec.COL_MEMORY, rec.COL_RANGE_CHECK, rec.COL_DILUTED_UNORDERED, rec.COL_DILUTED_ORDERED)
    keep, patch, seen = [], {}, {}

    def build_extension(challenges):
        keep.append(hostlib.build_extension_columns(ctx, "recursive", [dev[c] for c in aux_idx], n, challenges))
        seen["challenges"] = [from_limbs(c) for c in challenges]
        seen["cols"] = dev + keep[-1].cols
        for (col, row), delta in patch.items():              # after the base commitment, before the check: a bad cell of the witness
            poke(ctx, dev[col], row, (peek(ctx, dev[col], row) + delta) % P)
        return keep[-1].cols

    def prove():
        return hostlib.prove_files_device(ctx, "recursive", trace_bin, memory_bin, pi, None, dev, air, be.TREE_KECCAK, 0, be.COIN_SOLIDITY, seed, build_extension)[0]
    off = prove()
    air.set_validation(True)
    on = prove()
    assert off == on and len(off) > 100_000
    assert hostlib.verify(air, be.TREE_KECCAK, be.COIN_SOLIDITY, seed, on)           # (and it is a proof: the C++ verifier accepts it)
    # cpu/operands/res reads aux RES of its own cycle only, and no extension column is made from the auxiliary column
    col, row = rec.COL_AUXILIARY, 16 * 1234 + rec.Auxiliary.RES
    patch[(col, row)] = 5
    with pytest.raises(SandstormHipError) as err:
        prove()
    constraints = rec.constraints(rec.Hints.from_public_input(pi, seen["challenges"], n), seen["challenges"])
    trace = DeviceTrace(ctx, rec, air, seen["cols"], n, constraints)
    new = peek(ctx, dev[col], row)
    want = trace.expected_after(col, row, new)
    assert want and want[0][1] == "cpu/operands/res"
    k, name, domain, first, count = want[0]
    message = "trace does not satisfy the AIR: %d constraint%s; first: #%d %s (%s) at row %d, %d row%s" % (
        len(want), " fails" if len(want) == 1 else "s fail", k, name, domain, first, count, "" if count == 1 else "s")
    assert str(err.value).endswith(message), (str(err.value), message)
    patch.clear()
    assert prove() == off                                # the context and the AIR stay usable
    group = hostlib.LocalGroup(1)
    with pytest.raises(SandstormHipError, match="sharded prover does not check the trace"):
        hostlib.prove_files_sharded_device(ctx, "recursive", trace_bin, memory_bin, pi, None, air, be.TREE_KECCAK, 0, be.COIN_SOLIDITY, seed, 0, 1, group)
    air.set_validation(False)
    group.close()
    for m in keep:
        m.close()
    air.close()
    for d in dev:
        d.free()
