"""The 64-bit field's claim (sandstorm_amd/goldilocks.py, host/goldilocks_prover.cpp) at LDE blowup 4, 8 and 16, not only 2.

The plain AIR's constraints have degree 2, so the composition has 2n coefficients whatever the blowup is: both provers evaluate the
constraints on the 2n-point coset OFFSET * <w_2n> - every 2^(lb-1)-th row of the LDE, copied out as contiguous columns by
ss_subsample_rows_gl64 -, interpolate there, split into H0 / H1 and extend the six coordinate columns to N = n 2^lb rows; the AIR's
tables are those of that coset (make_tables(n, 1)) at every blowup.  What holds this:

  1  ss_subsample_rows_gl64 against numpy slicing: odd sizes, every stride, more columns than one launch takes, words >= p, the tail
  2  proofs of the example (n = 1024) at log_blowup 2, 3, 4, folds 2 / 8 / 16, both hashes: goldilocks.Prover and hostlib.gl_prove
     write the same arrays, and goldilocks.verify accepts them
  3  the same prover over the CPU oracle (a context whose sub-sampling is numpy slicing) writes those arrays
  4  an independent route: the constraints on ALL N rows (ss_eval_quotient_gl64x3 at log_blowup = lb with tables of that coset: code
     this feature leaves as it was) equal H0(x^2) + x H1(x^2) built from the six committed columns, at every row
  5  files -> proof (goldilocks.prove_files, hostlib.gl_prove_files) at lb = 2, with validation on, and a broken cell named
  6  the verifier: another log_blowup in the options, 0 and 5, and the security rule at 32 / 31 queries

Runs on the MI355X (`-m gpu`) and, in the CPU suite, on the host build of the device code (tests/test_gl64_lde_blowup_on_host.py)."""
import copy
import dataclasses
import os

import numpy as np
import pytest

from tests.gl64_edge_values import EDGE, P
from tests.test_fri_options_on_host import SEED, gl_example

pytestmark = pytest.mark.gpu
EMULATED = os.environ.get("SS_TEST_HIPEMU") == "1"          # (the device code on the CPU: torch CPU tensors are its device buffers)
OFFSET = 7
# (log_blowup, queries, fold, hash): every blowup at fold 8, folds 2 and 16 at blowup 4, SHA-256 once
CASES = [(2, 10, 8, "blake2s"), (3, 7, 8, "blake2s"), (4, 5, 8, "blake2s"), (4, 5, 2, "blake2s"), (4, 5, 16, "blake2s"), (2, 10, 8, "sha256")]
CASE_IDS = ["lb%d-q%d-fold%d-%s" % c for c in CASES]


def options(lb, queries, fold=8, hash_name="blake2s", grinding=8):
    from sandstorm_amd import goldilocks as gs
    return gs.Options(num_queries=queries, log_blowup=lb, grinding=grinding, fold=fold, hash=hash_name)


@pytest.fixture(scope="module")
def ctx():
    from sandstorm_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def env():
    """-> (context, torch device): ONE stream for torch's tensor ops and the C ABI's kernels, as tests/test_goldilocks_stark.py sets up"""
    import torch
    from sandstorm_amd import backend as be
    if EMULATED:
        c, dev = be.Context(0), torch.device("cpu")
    else:
        dev = torch.device("cuda", 0)
        stream = torch.cuda.Stream(dev)
        torch.cuda.set_stream(stream)
        c = be.Context(0, stream=stream.cuda_stream)
    yield c, dev
    c.close()
    if not EMULATED:
        torch.cuda.set_stream(torch.cuda.default_stream(dev))


def tensors(cols, dev):
    import torch
    return [torch.from_numpy(np.array(c, dtype=np.uint64).view(np.int64)).to(dev) for c in cols]


def assert_same_arrays(proof, want, what=""):
    from sandstorm_amd import goldilocks as gs
    got = gs.proof_to_arrays(proof)
    assert set(got) == set(want), what
    for k in sorted(want):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k)


# ------------------------------------------------------------------------------------------------------ 1. the sub-sampling kernel
ROWS = [1, 2, 3, 255, 256, 257, 1000, 4097]
STRIDES = [0, 1, 2, 3, 4]
NCOLS = [1, 3, 16, 17]
SENTINEL = 0xA5A5A5A5A5A5A5A5
# what is no field element passes through as it is: p, p + 1, the largest word, the lazy words just below 2^64
WORDS = np.array(EDGE + [P, P + 1, 2**64 - 1, 2**64 - 2, 2**64 - 2**32, 2**64 - 2**32 + 2], dtype=np.uint64)


@pytest.fixture(scope="module")
def words():
    """one pool of 64-bit words for every shape (the kernel moves bits: they need not be field elements): uniform over all of 2^64,
    the edge words at about a third of the positions and at its head"""
    rng = np.random.default_rng(0x61DE)
    pool = rng.integers(0, 1 << 64, size=max(NCOLS) * (max(ROWS) << max(STRIDES)), dtype=np.uint64)
    at = rng.random(len(pool)) < 1 / 3
    pool[at] = WORDS[rng.integers(0, len(WORDS), size=int(at.sum()))]
    pool[:len(WORDS)] = WORDS
    pool.setflags(write=False)
    return pool


@pytest.mark.parametrize("log_stride", STRIDES)
@pytest.mark.parametrize("nrows_out", ROWS)
def test_subsample_rows_gl64_against_numpy_slicing(ctx, words, nrows_out, log_stride):
    """d_out[c][j] = d_in[c][j << log_stride] for j < nrows_out, bit for bit, and nothing else: 1, 3, 16 and 17 columns (17: two
    launches), the inputs exactly nrows_out << log_stride words long (no case reads outside its allocation), the outputs one word
    longer and pre-filled - the tail must come back untouched"""
    in_len = nrows_out << log_stride
    fill = np.full(nrows_out + 1, SENTINEL, dtype=np.uint64)
    for ncols in NCOLS:
        host = [words[c * in_len:(c + 1) * in_len] for c in range(ncols)]
        d_in = [ctx.column(h) for h in host]
        d_out = [ctx.column(fill) for _ in range(ncols)]
        ctx.subsample_rows_gl64(d_in, nrows_out, log_stride, d_out)
        for c in range(ncols):
            got = d_out[c].download(np.uint64, (nrows_out + 1,))
            assert np.array_equal(got[:nrows_out], host[c][::1 << log_stride]), (ncols, c)
            assert got[nrows_out] == SENTINEL, (ncols, c, "tail")
        for d in d_in + d_out:
            d.free()


def test_subsample_rows_gl64_into_a_destination_that_is_not_16_byte_aligned(ctx, words):
    """an output column that starts 8 bytes into a buffer (a view): the same words, the word before and the word after untouched"""
    from sandstorm_amd import backend as be
    for nrows_out in (1, 2, 257, 1000):
        host = words[:nrows_out << 1]
        d_in = ctx.column(host)
        buf = ctx.column(np.full(nrows_out + 2, SENTINEL, dtype=np.uint64))
        ctx.subsample_rows_gl64([d_in], nrows_out, 1, [be.DeviceView(buf, 8, 8 * nrows_out)])
        got = buf.download(np.uint64, (nrows_out + 2,))
        assert np.array_equal(got[1:-1], host[::2]) and got[0] == SENTINEL and got[-1] == SENTINEL, nrows_out
        d_in.free()
        buf.free()


def test_subsample_rows_gl64_refuses_what_it_cannot_serve(ctx):
    import ctypes as C
    from sandstorm_amd._lib import SandstormHipError, check
    a, b = ctx.alloc(8 * 64), ctx.alloc(8 * 64)
    with pytest.raises(SandstormHipError, match="log_stride"):
        ctx.subsample_rows_gl64([a], 2, 5, [b])
    with pytest.raises(SandstormHipError):
        ctx.subsample_rows_gl64([a], 0, 1, [b])
    with pytest.raises(SandstormHipError, match="NULL"):
        ctx.subsample_rows_gl64([a], 4, 1, [0])
    with pytest.raises(SandstormHipError, match="NULL"):
        ctx.subsample_rows_gl64([0], 4, 1, [b])
    one = (C.c_void_p * 1)(a.ptr)
    with pytest.raises(SandstormHipError, match="NULL"):
        check(ctx.lib.ss_subsample_rows_gl64(None, one, 1, 4, 1, one))
    with pytest.raises(SandstormHipError, match="NULL"):
        check(ctx.lib.ss_subsample_rows_gl64(ctx.handle, None, 1, 4, 1, one))
    with pytest.raises(SandstormHipError, match="NULL"):
        check(ctx.lib.ss_subsample_rows_gl64(ctx.handle, one, 1, 4, 1, None))
    ctx.subsample_rows_gl64([a], 4, 4, [b])           # the largest stride: 4 rows out of 64


# ------------------------------------------------------------------------------------------------------ 2. whole proofs
_proofs = {}


def python_proof(env, case):
    """goldilocks.Prover on the device, once per case"""
    from sandstorm_amd import goldilocks as gs
    if case not in _proofs:
        c, dev = env
        pi, cols = gl_example()
        base = tensors(cols, dev)
        _proofs[case] = gs.Prover(c, gs.plain_air(), options(*case)).prove(SEED, base, lambda ch: gs.plain_extension_on_device(c, base, ch)[0], statement=pi)
    return _proofs[case]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_both_hosts_prove_the_example_above_blowup_2(env, case):
    """n = 1024 at N = 4096, 8192 and 16384: goldilocks.Prover and hostlib.gl_prove write the same proof, array for array; the verifier -
    which recomputes the AIR at z from the layout's DAG - accepts it under the expected options, and refuses it with one composition
    value altered (out of domain, and in an opened row)"""
    from sandstorm_amd import goldilocks as gs, hostlib
    c, dev = env
    lb, queries, fold, hash_name = case
    opt = options(*case)
    pi, cols = gl_example()
    proof = python_proof(env, case)
    want = gs.proof_to_arrays(proof)
    assert int(want["options"][1]) == lb and proof.base.paths.shape[1] == 10 + lb
    base = tensors(cols, dev)
    cpp = hostlib.gl_prove(c, gs.plain_air(), opt, SEED, base, lambda ch: gs.plain_extension_on_device(c, base, ch)[0], statement=pi)
    assert_same_arrays(cpp, want, "hostlib.gl_prove")
    bits = queries * lb + 8
    for p in (proof, cpp):
        positions = gs.verify(p, gs.plain_air(), SEED, statement=pi, expected_options=opt, required_security_bits=bits)
        assert 1 <= len(positions) <= queries and all(q < 1024 << lb for q in positions)
    again = gs.proof_from_arrays(want)
    assert again.options == opt
    gs.verify(again, gs.plain_air(), SEED, statement=pi, expected_options=opt, required_security_bits=bits)
    for mutate in (lambda p: p.ood_comp.__setitem__((4, 1), (int(p.ood_comp[4, 1]) + 1) % P),
                   lambda p: p.comp.rows.__setitem__((0, 3), (int(p.comp.rows[0, 3]) + 1) % P)):
        bad = copy.deepcopy(proof)
        mutate(bad)
        with pytest.raises(gs.VerificationError):
            gs.verify(bad, gs.plain_air(), SEED, statement=pi, required_security_bits=bits)


# ------------------------------------------------------------------------------------------------------ 3. the oracle pipeline
def oracle_context():
    """oracle/gl_cpu_context.py with the one call it lacks: the sub-sampling is numpy slicing"""
    from oracle.gl_cpu_context import GlCpuContext, _np

    class Ctx(GlCpuContext):
        def subsample_rows_gl64(self, cols_in, nrows_out, log_stride, cols_out):
            for src, dst in zip(cols_in, cols_out):
                _np(dst)[:nrows_out] = _np(src)[::1 << log_stride][:nrows_out]
    return Ctx()


@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=[CASE_IDS[0], CASE_IDS[2]])
def test_oracle_pipeline_writes_the_device_made_proof(env, case):
    """the prover of sandstorm_amd/goldilocks.py with the oracle standing in for every kernel, at lb = 2 and 4: the arrays of test 2"""
    import torch
    from sandstorm_amd import goldilocks as gs
    want = gs.proof_to_arrays(python_proof(env, case))
    octx = oracle_context()
    pi, cols = gl_example()
    base = tensors(cols, torch.device("cpu"))
    proof = gs.Prover(octx, gs.plain_air(), options(*case)).prove(SEED, base, lambda ch: gs.plain_extension_on_device(octx, base, ch)[0], statement=pi)
    assert_same_arrays(proof, want, "the oracle pipeline")


# ------------------------------------------------------------------------------------------------------ 4. an independent route
@pytest.mark.parametrize("lb", [2, 3])
def test_the_split_is_the_composition_on_every_lde_row(env, oracle, lb):
    """With fixed challenges the constraints are evaluated on ALL N LDE rows by ss_eval_quotient_gl64x3 at log_blowup = lb with tables
    built for that coset (make_tables(n, lb)) - the wasteful route, code this feature leaves alone.  The six composition columns come
    from Prover.composition_columns (sub-sampled rows, tables of the 2n-point coset).  On the host each committed column is
    interpolated over its N points (the oracle's transform; coefficients n .. N - 1 are zero) and evaluated on OFFSET^2 <w_(N/2)>, where
    x_i^2 lies: q[i] = H0(x_i^2) + x_i H1(x_i^2) in every coordinate, at every row"""
    import torch
    from sandstorm_amd import air_program as ap, goldilocks as gs
    from sandstorm_amd.layouts import plain as pl
    c, dev = env
    pi, cols = gl_example()
    n, log_n = len(cols[0]), 10
    N = n << lb
    ch, alpha = [(11, 22, 33), (5, 6, 7), (9, 8, 7)], (123456789, 987654321, 55555)
    ext, _ = pl.extension_columns(cols, ch)
    trace = tensors(list(cols) + ext, dev)
    trace_ev = [torch.empty(N, dtype=torch.int64, device=dev) for _ in trace]
    c.lde_gl64(trace, log_n, lb, OFFSET, trace_ev)
    air = gs.plain_air()

    def lowered(tables):
        prog = ap.lower(air.composition(n, ch, alpha, tables, pi), P, ext=True, symbols=tables.symbols)
        tvals, tdesc = tables.device_tables()
        return prog, torch.from_numpy(tvals.view(np.int64)).to(dev), tdesc
    prog, d_tables, tdesc = lowered(air.make_tables(n, lb))
    q = torch.empty((N, 3), dtype=torch.int64, device=dev)
    c.eval_quotient_gl64x3(np.array(prog.code, dtype=np.uint32), np.array(prog.consts, dtype=np.uint64).reshape(-1, 3), prog.n_slots, d_tables, tdesc,
                           trace_ev, log_n, lb, OFFSET, q)
    q = q.cpu().numpy().view(np.uint64)
    prog, d_tables, tdesc = lowered(air.make_tables(n, 1))
    comp_co, comp_ev = gs.Prover(c, air, options(lb, 8)).composition_columns(trace_ev, log_n, prog, d_tables, tdesc)
    assert len(comp_co) == len(comp_ev) == 6 and all(v.shape == (N,) for v in comp_ev) and all(v.shape == (n,) for v in comp_co)
    squares = []                                                                    # squares[k][j] = column k's polynomial at OFFSET^2 w_(N/2)^j
    for col in comp_ev:
        coeffs = oracle.gl_ntt(col.cpu().numpy().view(np.uint64), inverse=True, offset=OFFSET)
        assert coeffs[:n].any() and not coeffs[n:].any()
        squares.append([int(v) for v in oracle.gl_ntt(coeffs[:N // 2], offset=OFFSET * OFFSET % P)])
    wN = pl.root_of_unity(log_n + lb)
    x = OFFSET
    for i in range(N):
        j = i % (N // 2)
        for t in range(3):
            assert int(q[i, t]) == (squares[t][j] + x * squares[3 + t][j]) % P, (i, t)
        x = x * wN % P


# ------------------------------------------------------------------------------------------------------ 5. files -> proof
def example_files():
    from sandstorm_amd import binary as bn
    from sandstorm_amd.layouts import plain as pl
    prog = pl.example_program(10)
    states, memory = pl.run(prog, 64)
    return states, memory, pl.public_input_of(prog, states, memory), bn


def test_files_to_proof_at_blowup_4(env):
    """lb = 2: goldilocks.prove_files and hostlib.gl_prove_files (the base trace made on the device, the extension column and the proof
    by the C++ host), validation off and on, write the proof Prover writes from layouts/plain.py's host-made columns"""
    import torch
    from sandstorm_amd import goldilocks as gs, hostlib
    c, dev = env
    case = CASES[0]
    opt = options(*case)
    want = gs.proof_to_arrays(python_proof(env, case))
    states, memory, pi, bn = example_files()
    trace_bin, memory_bin = bn.write_register_states(states), bn.write_memory(memory)
    out = lambda: [torch.empty(1024, dtype=torch.int64, device=dev) for _ in range(5)]
    assert_same_arrays(gs.prove_files(c, trace_bin, memory_bin, pi, SEED, opt, out=out()), want, "goldilocks.prove_files")
    assert_same_arrays(gs.prove_files(c, trace_bin, memory_bin, pi, SEED, opt, out=out(), validate=True), want, "goldilocks.prove_files, validate")
    proof, times = hostlib.gl_prove_files(c, gs.plain_air(), opt, SEED, trace_bin, memory_bin, pi, out())
    assert_same_arrays(proof, want, "hostlib.gl_prove_files")
    assert times["total_s"] >= times["trace_gen_s"] > 0


def test_a_broken_cell_is_named_at_blowup_4(env):
    """lb = 2, validation on: the value the loop's first multiplication writes, changed in memory - Prover.prove, hostlib.gl_prove and
    prove_files stop with the constraint's name, as they do at blowup 2"""
    import torch
    from sandstorm_amd import goldilocks as gs, hostlib
    from sandstorm_amd._lib import SandstormHipError
    from sandstorm_amd.layouts import plain as pl
    c, dev = env
    opt = options(*CASES[0])
    states, memory, pi, bn = example_files()
    good = pl.base_trace(states, memory, pi)
    address = good[pl.COL_NPC][16 * 2 + pl.Npc.MEM_DST_ADDR]
    assert address not in [a for a, _ in pi.public_memory]
    wrong = list(memory)
    wrong[address] = (wrong[address] + 1) % P
    base = tensors(pl.base_trace(states, wrong, pi), dev)
    ext = lambda ch: gs.plain_extension_on_device(c, base, ch)[0]
    name = "trace does not satisfy the AIR: .*cpu/"
    with pytest.raises(ValueError, match=name) as e:
        gs.Prover(c, gs.plain_air(), opt, validate=True).prove(SEED, base, ext, statement=pi)
    message = str(e.value)
    with pytest.raises(SandstormHipError) as e:
        hostlib.gl_prove(c, gs.plain_air(), opt, SEED, base, ext, statement=pi, validate=True)
    assert str(e.value).endswith(message)
    with pytest.raises(SandstormHipError) as e:
        gs.prove_files(c, bn.write_register_states(states), bn.write_memory(wrong), pi, SEED, opt,
                       out=[torch.empty(1024, dtype=torch.int64, device=dev) for _ in range(5)], validate=True)
    assert str(e.value).endswith(message)


# ------------------------------------------------------------------------------------------------------ 6. the verifier, refusals
def test_verifier_refuses_a_proof_under_another_blowup(env):
    """a proof made at lb = 2 whose options say 1 or 3: the transcript, the domain and the tree depths are another proof's"""
    from sandstorm_amd import goldilocks as gs
    pi, _ = gl_example()
    proof = python_proof(env, CASES[0])
    for other in (1, 3):
        forged = dataclasses.replace(proof, options=dataclasses.replace(proof.options, log_blowup=other))
        with pytest.raises(gs.VerificationError):
            gs.verify(forged, gs.plain_air(), SEED, statement=pi, required_security_bits=8)


@pytest.mark.parametrize("lb", [0, 5])
def test_log_blowup_0_and_5_are_refused_by_name(env, lb):
    """both provers and the files path before any launch (the profiler counts none; pre-filled base columns come back as they were), and the
    verifier - each names the option"""
    import torch
    from sandstorm_amd import goldilocks as gs, hostlib
    from sandstorm_amd._lib import SandstormHipError
    c, dev = env
    opt = options(lb, 10)
    pi, cols = gl_example()
    base = tensors(cols, dev)
    ext = lambda ch: gs.plain_extension_on_device(c, base, ch)[0]
    states, memory, _, bn = example_files()
    out = [torch.full((1024,), 0x5A5A5A5A, dtype=torch.int64, device=dev) for _ in range(5)]
    c.profile(True)
    try:
        c.profile_reset()
        with pytest.raises(ValueError, match="log_blowup refused"):
            gs.Prover(c, gs.plain_air(), opt).prove(SEED, base, ext, statement=pi)
        with pytest.raises(SandstormHipError, match="log_blowup refused"):
            hostlib.gl_prove(c, gs.plain_air(), opt, SEED, base, ext, statement=pi)
        with pytest.raises(SandstormHipError, match="log_blowup refused"):
            gs.prove_files(c, bn.write_register_states(states), bn.write_memory(memory), pi, SEED, opt, out=out)
        assert sum(c.profile_read(kind)[1] for kind in range(8)) == 0
    finally:
        c.profile(False)
    assert all(bool((col == 0x5A5A5A5A).all()) for col in out), "a base column was written by a refused call"
    forged = dataclasses.replace(python_proof(env, CASES[0]), options=opt)
    with pytest.raises(gs.VerificationError, match="log_blowup"):
        gs.verify(forged, gs.plain_air(), SEED, statement=pi, required_security_bits=8)


def test_32_queries_at_blowup_4_clear_the_default_security_bar(env):
    """32 queries x 2 bits + 16 grinding bits = 80: accepted by a default verify(); 31 queries conjecture 78 and are refused"""
    from sandstorm_amd import goldilocks as gs
    c, dev = env
    pi, cols = gl_example()
    base = tensors(cols, dev)
    ext = lambda ch: gs.plain_extension_on_device(c, base, ch)[0]
    opt = options(2, 32, grinding=16)
    assert gs.conjectured_security_bits(opt, 1024) == 80
    proof = gs.Prover(c, gs.plain_air(), opt).prove(SEED, base, ext, statement=pi)
    assert gs.verify(proof, gs.plain_air(), SEED, statement=pi, expected_options=opt)
    opt31 = options(2, 31, grinding=16)
    assert gs.conjectured_security_bits(opt31, 1024) == 78
    proof31 = gs.Prover(c, gs.plain_air(), opt31).prove(SEED, base, ext, statement=pi)
    gs.verify(proof31, gs.plain_air(), SEED, statement=pi, expected_options=opt31, required_security_bits=78)      # a sound proof ...
    with pytest.raises(gs.VerificationError, match="78 bits of security, 80 required"):
        gs.verify(proof31, gs.plain_air(), SEED, statement=pi, expected_options=opt31)                              # ... below the bar
