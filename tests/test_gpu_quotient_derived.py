"""The derived flag column of the compiled constraint kernels on the device (csrc/quotient_derive.h, csrc/quotient.hip
qg_derive_column_kernel, csrc/capi.hip eval_quotient_compiled): both layouts' real programs at 2^18 trace rows - the size at which
the program's hash is the committed kernel's, checked here - compiled against interpreted (SS_QUOTIENT_INTERPRET=1) at every point:
column 0 at the values where the flag's subtraction wraps, also across the end of the domain; two evaluations on one context with
column 0 overwritten in between (the column is rebuilt at every call); and the row-block entry point, whose derived column ends
with the block's rows.  The library takes the interpreter by itself for a program whose counts differ from the kernel's: every
evaluation here counts its profiled launches, so "compiled" is the parts' kernels behind the derive kernel and not the interpreter twice."""
import glob
import os
import sys

import numpy as np
import pytest

from tests.test_gpu_real_quotient import _Prog, _rand
from tests.test_layout_recursive import load_run
from tests.test_layout_starknet import CHALLENGES, P, starknet_example

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_N = 18
EDGE = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2]


def _felts(values):
    return np.array([[(v >> (64 * k)) & ((1 << 64) - 1) for k in range(4)] for v in values], dtype=np.uint64)


class _Case:
    """one layout's program, tables and random columns on one context; the interpreter's result on them, computed once"""

    def __init__(self, oracle, layout):
        from sandstorm_amd import backend as be, hostlib
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import gen_quotient
        if layout == "starknet":
            from sandstorm_amd.layouts import starknet as lay
            _, _, pi = starknet_example(11)
            cpp = hostlib.StarknetHostAir(None, pi, LOG_N)
        else:
            from sandstorm_amd.layouts import recursive as lay
            _, _, pi = load_run()
            cpp = hostlib.RecursiveHostAir(None, pi, LOG_N)
        n, self.N = 1 << LOG_N, 2 << LOG_N
        code, consts, n_slots, specs = cpp.dump(n, [oracle.to_mont([c])[0] for c in CHALLENGES], oracle.to_mont([pow(3, 99, P)])[0])
        cpp.close()
        with open(os.path.join(ROOT, "sandstorm_amd", "csrc", "quotient_gen_%s.hip" % layout)) as f:
            text = f.read()
        assert ("0x%016x" % gen_quotient.code_hash(code)) in text, "the committed kernel was generated from another program"
        assert "scaled, 1u, {{0u, 2u, {0u, 1u}, {1, -2}}}}" in text, "the committed kernel reads other derived columns than the flags'"
        # launches of a compiled evaluation: one per part behind one per derived column; the interpreter is one
        self.compiled_launches = len(glob.glob(os.path.join(ROOT, "sandstorm_amd", "csrc", "quotient_gen_%s_p[0-9].hip" % layout))) + 1
        code = np.asarray(code)
        trace = (code[0::2] & 0xff <= 4) & ((code[0::2] >> 12) & 0xf == 3)
        self.halo = int(max(int(w1) & 0xffffff for w1 in code[1::2][trace])) << 1       # the layout's largest row offset, LDE rows
        tables = lay.Tables(n)
        self.rng = rng = np.random.default_rng(41)
        tabs, self.desc, off = [], [], 0
        for spec in specs:
            t = _rand(rng, tables.length(spec))
            self.desc += [off, len(t).bit_length() - 1]
            off += len(t)
            tabs.append(t)
        self.lde = [_rand(rng, self.N) for _ in range(10)]
        self.g = oracle.to_mont([3])[0]
        self.ctx = be.Context(0)
        self.m = be.Matrix.from_host(self.ctx, self.lde)
        self.d_tab = self.ctx.column(np.concatenate(tabs))
        self.prog = _Prog(code, [int(v) for v in oracle.from_mont(consts)], n_slots)
        self.out = self.ctx.alloc(32 * self.N)
        self.interpreted = None
        self.ctx.profile(True)

    def launches(self, evaluate):
        """run one evaluation and hold the quotient stage's launch count to the path that was asked for"""
        from sandstorm_amd import backend as be
        self.ctx.profile_reset()
        evaluate()
        self.ctx.sync()
        return self.ctx.profile_read(be.PROF_QUOTIENT)[1]

    def whole(self, interpret):
        """the composition over the whole domain of what the context's columns hold now (the interpreter's: once per contents)"""
        if interpret and self.interpreted is not None:
            return self.interpreted
        if interpret:
            os.environ["SS_QUOTIENT_INTERPRET"] = "1"
        try:
            self.ctx.zero(self.out)
            n = self.launches(lambda: self.ctx.eval_quotient(self.prog, self.d_tab, self.desc, self.m.cols, LOG_N, 1, self.g, self.out))
            assert n == (1 if interpret else self.compiled_launches), (interpret, n)
            got = self.out.download(np.uint64, (self.N, 4))
        finally:
            os.environ.pop("SS_QUOTIENT_INTERPRET", None)
        if interpret:
            self.interpreted = got
        return got

    def set_column0(self, col0):
        """overwrite column 0 in place: the same device buffer, other contents"""
        self.lde[0], self.interpreted = col0, None
        self.m.cols[0].upload(col0)


@pytest.fixture(scope="module", params=["starknet", "recursive"])
def case(request, oracle):
    c = _Case(oracle, request.param)
    yield c
    c.ctx.close()


def test_edge_values_in_column_0(case):
    """column 0 drawn from 0, 1, p - 1, (p - 1) / 2, (p + 1) / 2 at random, and laid out explicitly in the last and the first 32 rows:
    a flag joins rows i and i + 2 (one trace row on), the flags read up to 16 trace rows on, so the last rows' flags are read
    across the end of the domain and two of them are MADE across it.  The explicit rows run through all 25 ordered pairs of the
    values at distance 2, the pair across the end among them."""
    edge = _felts(EDGE)
    col0 = edge[case.rng.integers(0, len(EDGE), size=case.N)]
    cycle = [0, 0, 1, 0, 2, 0, 3, 0, 4, 1, 1, 2, 1, 3, 1, 4, 2, 2, 3, 2, 4, 3, 3, 4, 4]      # every ordered pair of 5 symbols, cyclically
    seam = np.array([cycle[(t // 2) % 25] for t in range(64)])                               # rows N - 32 .. N - 1, 0 .. 31
    assert len(set((int(seam[t]), int(seam[t + 2])) for t in range(62))) == 25
    col0[-32:], col0[:32] = edge[seam[:32]], edge[seam[32:]]
    case.set_column0(col0)
    compiled = case.whole(False)
    assert compiled.any() and np.array_equal(compiled, case.whole(True))


def test_no_stale_derived_column(case):
    """two evaluations on one context, column 0 overwritten in place between them: the second is the interpreter's on the new
    contents (the derived column is rebuilt at every call, nothing is kept by pointer)"""
    first = case.whole(False)
    case.set_column0(_rand(case.rng, case.N))
    second = case.whole(False)
    assert not np.array_equal(first, second)
    assert np.array_equal(second, case.whole(True))


@pytest.mark.parametrize("extra", [0, 1], ids=["halo-exact", "halo-plus-one-row"])
def test_row_blocks_assemble_to_the_whole_domain(case, extra):
    """ss_eval_quotient_rows with the rows behind each block exactly the layout's largest row offset (and with one row more): the
    derived column has the block's rows less its reach, every row the kernels read; the last block wraps around the end of the domain"""
    want = case.whole(True)
    R = 4
    B = case.N // R
    rows = B + case.halo + extra
    got = np.empty_like(want)
    for r in range(R):
        idx = (r * B + np.arange(rows)) % case.N
        blocks = [case.ctx.column(c[idx]) for c in case.lde]
        out = case.ctx.alloc(32 * B)
        n = case.launches(lambda: case.ctx.eval_quotient_rows(case.prog, case.d_tab, case.desc, blocks, LOG_N, 1, case.g, r * B, B, rows, out))
        assert n == case.compiled_launches, (r, n)
        got[r * B:(r + 1) * B] = out.download(np.uint64, (B, 4))
    assert np.array_equal(got, want)
