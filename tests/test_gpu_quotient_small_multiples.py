"""The compiled constraint kernels with small structural multiples as shifts and adds and repeated operands as one load
(tools/gen_quotient.py), on the device, at the smallest sizes at which the real programs are the compiled ones - 2^15 trace rows (a
2^16-point domain) for recursive, 2^16 for starknet: its program at 2^15 rows has another shape and other code words (a single
ECDSA instance), is not the program the kernels were generated from and is interpreted whatever the kernels hold; the hash is checked:

  * both layouts' real programs, compiled against the interpreter (SS_QUOTIENT_INTERPRET) at every point, on a trace whose cells are
    the values at the edges of the limb forms (0, 1, p - 1, p - 2, 2^251) in seeded positions between random cells - so that the scaled
    values reach their bounds on the device's own code path;
  * the same program with ONE baked constant changed in the constant table (same code words, same hash): served by the interpreter -
    told by the quotient stage's launch count - and equal to the interpreter's result for those constants;
  * the row-block entry on the last block of the domain, whose rows behind it wrap around the end, against the whole-domain result."""
import os

import numpy as np
import pytest

from tests.test_gpu_real_quotient import _rand
from tests.test_layout_recursive import load_run
from tests.test_layout_starknet import CHALLENGES, P, starknet_example
from tests.test_quotient_gen_small_multiples import baked_constants

pytestmark = pytest.mark.gpu
LOG_NS = {"starknet": 16, "recursive": 15}
EDGES = [0, 1, P - 1, P - 2, 1 << 251]


class _Prog:
    def __init__(self, code, consts_mont, n_slots):
        self.code, self.consts_mont, self.n_slots = code, np.ascontiguousarray(consts_mont, dtype=np.uint64).reshape(-1, 4), n_slots


def _edge_column(rng, count):
    """random cells with an edge value in about every fourth position"""
    col = _rand(rng, count)
    table = np.array([[(v >> (64 * k)) & ((1 << 64) - 1) for k in range(4)] for v in EDGES], dtype=np.uint64)
    where = np.flatnonzero(rng.random(count) < 0.25)
    col[where] = table[rng.integers(0, len(EDGES), size=len(where))]
    return col


class _State:
    """one layout's program, tables and edge-value trace on the device, its composition by the compiled kernels and by the interpreter
    (computed once, shared by the tests below) and the quotient stage's launch counts of both"""

    def __init__(self, oracle, layout):
        import sys
        from sandstorm_amd import backend as be, hostlib
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
        import gen_quotient
        if layout == "starknet":
            from sandstorm_amd.layouts import starknet as lay
            _, _, pi = starknet_example(11)
            cpp = hostlib.StarknetHostAir(None, pi, LOG_NS[layout])
        else:
            from sandstorm_amd.layouts import recursive as lay
            _, _, pi = load_run()
            cpp = hostlib.RecursiveHostAir(None, pi, LOG_NS[layout])
        self.be, self.layout, self.log_n = be, layout, LOG_NS[layout]
        LOG_N = self.log_n
        n, self.N = 1 << LOG_N, 2 << LOG_N
        code, consts, n_slots, specs = cpp.dump(n, [oracle.to_mont([c])[0] for c in CHALLENGES], oracle.to_mont([pow(3, 99, P)])[0])
        cpp.close()
        with open(os.path.join(gen_quotient.ROOT, "sandstorm_amd", "csrc", "quotient_gen_%s.hip" % layout)) as f:
            assert ("0x%016x" % gen_quotient.code_hash(code)) in f.read(), "the committed kernel was generated from another program"
        self.code, self.consts, self.n_slots = code, np.array(consts, dtype=np.uint64).reshape(-1, 4), n_slots
        self.halo = max((int(c) & 0xffffff) for c in code[1::2][(code[0::2] >> 12) & 0xf == 3]) << 1
        tables = lay.Tables(n)
        rng = np.random.default_rng(41)
        tabs, self.desc, off = [], [], 0
        for spec in specs:
            t = _rand(rng, tables.length(spec))
            self.desc += [off, len(t).bit_length() - 1]
            off += len(t)
            tabs.append(t)
        self.lde = [_edge_column(rng, self.N) for _ in range(10)]
        self.g = oracle.to_mont([3])[0]
        self.ctx = be.Context(0)
        self.m = be.Matrix.from_host(self.ctx, self.lde)
        self.d_tab = self.ctx.column(np.concatenate(tabs))
        self.ctx.profile(True)
        self.compiled, self.compiled_launches = self.run(self.consts)
        self.interpreted, self.interpreted_launches = self.run(self.consts, interpret=True)

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
        got = out.download(np.uint64, (self.N, 4))
        return got, self.ctx.profile_read(self.be.PROF_QUOTIENT)[1]


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
def test_edge_value_trace_compiled_is_the_interpreter(states, layout):
    s = states(layout)
    assert s.compiled_launches != s.interpreted_launches, "the launch count does not tell the two paths apart"
    assert s.compiled_launches >= 1 + (6 if layout == "starknet" else 1)            # the parts (and the derived column's pass)
    assert s.compiled.any() and np.array_equal(s.compiled, s.interpreted)


@pytest.mark.parametrize("layout", ["starknet", "recursive"])
def test_patched_baked_constant_is_interpreted(states, layout):
    s = states(layout)
    baked = baked_constants(layout)
    assert baked
    for k, image in baked:                                      # the kernel table's list is this program's constant table
        assert sum(int(w) << (64 * j) for j, w in enumerate(s.consts[k])) == image
    k = baked[len(baked) // 2][0]
    patched = s.consts.copy()
    patched[k] = s.consts[(k + 1) % len(s.consts)] if not np.array_equal(s.consts[k], s.consts[(k + 1) % len(s.consts)]) else s.consts[(k + 2) % len(s.consts)]
    got, launches = s.run(patched)
    want, interpreted_launches = s.run(patched, interpret=True)
    assert launches == interpreted_launches == s.interpreted_launches           # not the compiled kernels: they hold the old value as code
    assert np.array_equal(got, want) and not np.array_equal(got, s.compiled)
    again, launches = s.run(s.consts)                            # the unpatched program is still theirs
    assert launches == s.compiled_launches and np.array_equal(again, s.compiled)


@pytest.mark.parametrize("layout", ["starknet", "recursive"])
def test_row_block_that_wraps_around_the_domain(states, layout):
    s = states(layout)
    B = s.N // 4
    row0 = s.N - B                                               # the last block: the rows behind it are the domain's first
    idx = (row0 + np.arange(B + s.halo)) % s.N
    blocks = [s.ctx.column(c[idx]) for c in s.lde]
    out = s.ctx.alloc(32 * B)
    s.ctx.profile_reset()
    s.ctx.eval_quotient_rows(_Prog(s.code, s.consts, s.n_slots), s.d_tab, s.desc, blocks, s.log_n, 1, s.g, row0, B, B + s.halo, out)
    assert s.ctx.profile_read(s.be.PROF_QUOTIENT)[1] == s.compiled_launches     # the compiled kernels serve the row-block entry too
    assert np.array_equal(out.download(np.uint64, (B, 4)), s.compiled[row0:])
