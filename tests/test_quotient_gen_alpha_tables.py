"""The compiled constraint kernels with their zerofier groups' coefficients folded into per-constraint copies of the periodic
multiplier tables (tools/gen_quotient.py fold_alpha_tables; csrc/quotient.hip qg_copy_tables_kernel), on the device, bit for bit:

  * both layouts' real programs - starknet at 2^16 trace rows (two instances of its longest period, 32768), recursive at 2^13 - on
    random columns and tables, compiled against the interpreter (quotient_vm_kernel, SS_QUOTIENT_INTERPRET) at every point; the
    programs' hashes are the committed kernels', and the two paths are told apart by the quotient stage's launch count;
  * with two different composition coefficients, evaluated A, B, A on one context: the copies are made from the call's own constant
    table at every call, so a copy left over from the call before would show;
  * on a row block whose first row is no multiple of the longest period (the copies are indexed by the global row);
  * with one (baked) constant changed: same code words, not the kernels' program - interpreted, and equal to the interpreter;
  * the copy kernel alone (ss_table_copies): tables of 1, 2, 32 and 2^17 entries, every limb form of the factor, against Python
    integers; coefficients 0, 1 and p - 1 and table entries at p - 1 included."""
import os
import sys

import numpy as np
import pytest

from tests.test_gpu_real_quotient import _rand
from tests.test_layout_recursive import load_run
from tests.test_layout_starknet import CHALLENGES, P, starknet_example
from tests.test_quotient_gen_small_multiples import baked_constants

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_NS = {"starknet": 16, "recursive": 13}
ALPHAS = (pow(3, 99, P), pow(7, 1055, P))
R = 1 << 256


class _Prog:
    def __init__(self, code, consts_mont, n_slots):
        self.code, self.consts_mont, self.n_slots = code, np.ascontiguousarray(consts_mont, dtype=np.uint64).reshape(-1, 4), n_slots


def _copies(layout):
    import re
    with open(os.path.join(ROOT, "sandstorm_amd", "csrc", "quotient_gen_%s.hip" % layout)) as f:
        listed = re.search(r"QGenAlpha alpha\[\] = \{(.*)\};", f.read()).group(1)
    return [tuple(int(v) for v in m) for m in re.findall(r"\{(\d+)u, (\d+)u, (\d+)u\}", listed)]


class _State:
    """one layout's program with two composition coefficients, random tables and columns on the device; the interpreter's
    composition for both coefficients is computed once and shared by the tests below"""

    def __init__(self, oracle, layout):
        from sandstorm_amd import backend as be, hostlib
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import gen_quotient
        log_n = LOG_NS[layout]
        if layout == "starknet":
            from sandstorm_amd.layouts import starknet as lay
            _, _, pi = starknet_example(11)
            cpp = hostlib.StarknetHostAir(None, pi, log_n)
        else:
            from sandstorm_amd.layouts import recursive as lay
            _, _, pi = load_run()
            cpp = hostlib.RecursiveHostAir(None, pi, log_n)
        self.be, self.layout, self.log_n = be, layout, log_n
        n, self.N = 1 << log_n, 2 << log_n
        self.consts = []
        for alpha in ALPHAS:
            code, consts, n_slots, specs = cpp.dump(n, [oracle.to_mont([c])[0] for c in CHALLENGES], oracle.to_mont([alpha])[0])
            self.consts.append(np.array(consts, dtype=np.uint64).reshape(-1, 4))
        cpp.close()
        with open(os.path.join(ROOT, "sandstorm_amd", "csrc", "quotient_gen_%s.hip" % layout)) as f:
            assert ("0x%016x" % gen_quotient.code_hash(code)) in f.read(), "the committed kernel was generated from another program"
        self.code, self.n_slots = code, n_slots
        self.copies = _copies(layout)
        assert len(self.copies) >= 50
        differ = [c for _, c, _ in self.copies if not np.array_equal(self.consts[0][c], self.consts[1][c])]
        assert len(differ) >= len(self.copies) - 1              # (alpha^0 = 1 is the one coefficient that does not move)
        self.halo = max((int(c) & 0xffffff) for c in code[1::2][(code[0::2] >> 12) & 0xf == 3]) << 1
        tables = lay.Tables(n)
        rng = np.random.default_rng(43)
        tabs, self.desc, off = [], [], 0
        for spec in specs:
            t = _rand(rng, tables.length(spec))
            self.desc += [off, len(t).bit_length() - 1]
            off += len(t)
            tabs.append(t)
        self.longest = max(1 << self.desc[2 * t + 1] for t, _, _ in self.copies)
        self.lde = [_rand(rng, self.N) for _ in range(10)]
        self.g = oracle.to_mont([3])[0]
        self.ctx = be.Context(0)
        self.m = be.Matrix.from_host(self.ctx, self.lde)
        self.d_tab = self.ctx.column(np.concatenate(tabs))
        self.ctx.profile(True)
        self.interpreted, self.interpreted_launches = zip(*[self.run(c, interpret=True) for c in self.consts])

    def run(self, consts, interpret=False):
        """-> (the composition at every point, launches of the quotient stage)"""
        ctx = self.ctx
        out = ctx.alloc(32 * self.N)
        ctx.zero(out)
        ctx.profile_reset()
        if interpret:
            os.environ["SS_QUOTIENT_INTERPRET"] = "1"
        try:
            ctx.eval_quotient(_Prog(self.code, consts, self.n_slots), self.d_tab, self.desc, self.m.cols, self.log_n, 1, self.g, out)
        finally:
            os.environ.pop("SS_QUOTIENT_INTERPRET", None)
        return out.download(np.uint64, (self.N, 4)), ctx.profile_read(self.be.PROF_QUOTIENT)[1]


@pytest.fixture(scope="module")
def states(oracle):
    made = {}

    def get(layout):
        if layout not in made:
            made[layout] = _State(oracle, layout)
        return made[layout]
    yield get
    for s in made.values():
        s.ctx.close()


@pytest.mark.parametrize("layout", ["starknet", "recursive"])
def test_compiled_is_the_interpreter_for_two_coefficients(states, layout):
    s = states(layout)
    if layout == "starknet":
        assert s.longest == 2 * 32768 and s.N == 2 * s.longest
    assert not np.array_equal(s.interpreted[0], s.interpreted[1])
    for k in (0, 1, 0):                                         # A, B, A again: nothing of the call before may survive in the copies
        got, launches = s.run(s.consts[k])
        assert launches != s.interpreted_launches[k], "the launch count does not tell the two paths apart"
        assert launches >= 1 + (6 if layout == "starknet" else 1)                   # the derived column and the parts (the copies' launch
                                                                                    # is inside the first part's clock)
        assert got.any() and np.array_equal(got, s.interpreted[k]), "coefficient %d" % k


@pytest.mark.parametrize("layout", ["starknet", "recursive"])
def test_row_block_that_starts_inside_a_period(states, layout):
    s = states(layout)
    B = s.N // 8
    row0 = 5 * B + 37
    assert row0 % s.longest != 0 and row0 % 64 != 0
    idx = (row0 + np.arange(B + s.halo)) % s.N
    blocks = [s.ctx.column(c[idx]) for c in s.lde]
    out = s.ctx.alloc(32 * B)
    s.ctx.profile_reset()
    s.ctx.eval_quotient_rows(_Prog(s.code, s.consts[1], s.n_slots), s.d_tab, s.desc, blocks, s.log_n, 1, s.g, row0, B, B + s.halo, out)
    assert s.ctx.profile_read(s.be.PROF_QUOTIENT)[1] != s.interpreted_launches[1]  # served by the compiled kernels
    assert np.array_equal(out.download(np.uint64, (B, 4)), s.interpreted[1][row0:row0 + B])


@pytest.mark.parametrize("layout", ["starknet", "recursive"])
def test_a_changed_constant_is_interpreted_and_agrees(states, layout):
    s = states(layout)
    baked = baked_constants(layout)
    assert baked
    k = baked[len(baked) // 2][0]
    patched = s.consts[0].copy()
    patched[k] = s.consts[0][(k + 1) % len(patched)] if not np.array_equal(patched[k], s.consts[0][(k + 1) % len(patched)]) else s.consts[0][(k + 2) % len(patched)]
    got, launches = s.run(patched)
    want, interpreted_launches = s.run(patched, interpret=True)
    assert launches == interpreted_launches == s.interpreted_launches[0]          # not the compiled kernels
    assert np.array_equal(got, want) and not np.array_equal(got, s.interpreted[0])


def _felts(values):
    return np.array([[(v >> (64 * k)) & ((1 << 64) - 1) for k in range(4)] for v in values], dtype=np.uint64)


def test_the_copy_kernel_alone():
    from sandstorm_amd import backend as be
    rng = np.random.default_rng(9)
    rand = lambda: int.from_bytes(rng.bytes(40), "little") % P
    lens = [1, 2, 32, 1 << 17]
    table, firsts = [], []
    for length in lens:
        firsts.append(len(table))
        t = [rand() for _ in range(length)]
        t[0] = P - 1                                            # every table holds p - 1 (and the longer ones 0 and 1 as well)
        if length >= 32:
            t[5], t[length - 1], t[length // 2] = 0, 1, P - 1
        table += t
    coefficients = [0, 1, P - 1, rand()]
    # the factor of QG_ALPHA_R280, _R280_UP, _R280_UPN for coefficient c (quotient_derive.h qg_alpha_factor) - and c itself: factors 0, 1, p - 1
    forms = [lambda c: c << 24, lambda c: c << 48, lambda c: -(c << 48), lambda c: c]
    copies = []                                                 # (first, length, factor as an integer mod p)
    for first, length in zip(firsts, lens):
        for c in (coefficients if length <= 32 else coefficients[2:]):
            for form in forms:
                copies.append((first, length, form(c) % P))
    ctx = be.Context(0)
    try:
        d_tab = ctx.column(_felts([v * R % P for v in table]))
        total = sum(length for _, length, _ in copies)
        out = ctx.alloc(32 * total)
        ctx.zero(out)
        ctx.table_copies(d_tab, [c[0] for c in copies], [c[1] for c in copies], _felts([c[2] * R % P for c in copies]), out)
        got = out.download(np.uint64, (total, 4))
    finally:
        ctx.close()
    want = []
    for first, length, factor in copies:
        want += [table[first + k] * factor % P * R % P for k in range(length)]
    assert np.array_equal(got, _felts(want))
