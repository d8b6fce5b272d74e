"""Proofs with an LDE blowup factor of 4, 8 and 16 (`--lde-blowup-factor`, cli/src/main.rs:53-54), not only 2.

The AIRs have degree 2, so the composition polynomial has 2n coefficients whatever the blowup is: the provers evaluate the constraints
on the 2n-point coset offset * <w_2n> - every 2^(lb-1)-th row of the LDE, copied out as contiguous columns by ss_subsample_rows -
interpolate there, split, and extend the two composition columns to N = n 2^lb rows.  What holds this:

  1  ss_subsample_rows against numpy slicing: odd sizes, every stride, more columns than one launch takes, the tail of the output
  2  DEEP at log_blowup 2, 3, 4 against the oracle (pointwise and rational path): written for a general blowup, never run above 1 before
  3  whole proofs of the shipped recursive example (both claims) and of the starknet statement: BOTH verifiers - which this feature
     does not touch - accept the bytes, refuse them after one composition value is altered, and the host-generated path writes the same
  4  an independent route to the composition columns: the constraints on ALL 4n rows (an AIR built for that coset: the old, wasteful
     route), interpolated at size 4n - the upper half of the coefficients is zero, and the even / odd halves at z^2 are the proof's
     two composition out-of-domain values
  5  the sharded prover on 1, 2 and 4 ranks writes the single-device bytes
  6  blowup 1, 3 and 32 are refused by name of the accepted set, and the context proves afterwards

Runs on the MI355X (`-m gpu`) and, in the CPU suite, on the host build of the device code (tests/test_lde_blowup_on_host.py)."""
import os

import numpy as np
import pytest

from tests.util import P, random_column

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
N_FRIENDLY = 22
# (blowup, queries): queries * log2(blowup) + 16 grinding bits >= 80 each (cli/src/main.rs:203)
PAIRS = [(4, 32), (8, 22), (16, 16)]


@pytest.fixture(scope="module")
def ctx():
    from sandstorm_amd.backend import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def be():
    from sandstorm_amd import backend
    return backend


# ------------------------------------------------------------------------------------------------------ 1. the sub-sampling kernel
ROWS = [1, 255, 256, 257, 4096 + 48]
STRIDES = [0, 1, 2, 3]
NCOLS = [1, 3, 16, 17]
TAIL = 64


@pytest.fixture(scope="module")
def cells():
    """one pool of random 32-byte cells for every shape (the kernel moves bits: they need not be field elements), every 97th all ones"""
    rng = np.random.default_rng(0x1DE)
    pool = rng.integers(0, 1 << 64, size=(max(NCOLS) * (max(ROWS) << max(STRIDES)), 4), dtype=np.uint64)
    pool[::97] = np.uint64(0xFFFFFFFFFFFFFFFF)
    pool.setflags(write=False)
    return pool


@pytest.mark.parametrize("log_stride", STRIDES)
@pytest.mark.parametrize("nrows_out", ROWS)
def test_subsample_rows_against_numpy_slicing(ctx, cells, nrows_out, log_stride):
    """d_out[c][j] = d_in[c][j << log_stride] for j < nrows_out and nothing else: 1, 3, 16 and 17 columns (17: two launches), the
    inputs exactly nrows_out << log_stride cells long (no case reads outside its allocation), the outputs 64 cells longer and
    pre-filled - the tail must come back untouched"""
    in_len = nrows_out << log_stride
    fill = np.full((nrows_out + TAIL, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    for ncols in NCOLS:
        host = [cells[c * in_len:(c + 1) * in_len] for c in range(ncols)]
        d_in = [ctx.column(h) for h in host]
        d_out = [ctx.column(fill) for _ in range(ncols)]
        ctx.subsample_rows(d_in, nrows_out, log_stride, d_out)
        for c in range(ncols):
            got = d_out[c].download(np.uint64, (nrows_out + TAIL, 4))
            assert np.array_equal(got[:nrows_out], host[c][::1 << log_stride]), (ncols, c)
            assert np.array_equal(got[nrows_out:], fill[nrows_out:]), (ncols, c, "tail")


def test_subsample_rows_refuses_what_it_cannot_serve(ctx):
    from sandstorm_amd._lib import SandstormHipError
    a, b = ctx.alloc(32 * 64), ctx.alloc(32 * 64)
    with pytest.raises(SandstormHipError, match="log_stride"):
        ctx.subsample_rows([a], 2, 5, [b])
    with pytest.raises(SandstormHipError):
        ctx.subsample_rows([a], 0, 1, [b])
    with pytest.raises(SandstormHipError, match="NULL"):
        ctx.subsample_rows([a], 4, 1, [0])
    ctx.subsample_rows([a], 4, 4, [b])           # the largest stride: 4 rows out of 64


# ------------------------------------------------------------------------------------------------------ 2. DEEP above blowup 2
def _deep_case(ctx, be, oracle, log_n, lb, ncols, mask, seed):
    n, N = 1 << log_n, 1 << (log_n + lb)
    g = oracle.to_mont([3])[0]
    cols = [random_column(n, c + seed) for c in range(ncols)]
    m = be.Matrix.from_host(ctx, cols)
    ev, co = m.lde(lb, g)
    comp_coeffs = [random_column(n, seed + 20 + k) for k in range(2)]
    cm = be.Matrix.from_host(ctx, [np.concatenate([c, np.zeros((N - n, 4), dtype=np.uint64)]) for c in comp_coeffs])
    cm.evaluate(g)
    z = 0x1357924680ACE ** 5 % P
    zm = oracle.to_mont([z])[0]
    mc, mo = [c for c, _ in mask], [o for _, o in mask]
    ood_t = ctx.ood_eval(co.cols, log_n, mc, mo, zm)
    ood_c = np.stack([oracle.poly_eval(c, oracle.to_mont([z * z % P])[0]) for c in comp_coeffs])
    alpha = 987654321987654321
    ct = oracle.to_mont([pow(alpha, j, P) for j in range(len(mask))])
    cc = oracle.to_mont([pow(alpha, len(mask) + k, P) for k in range(2)])
    args = (log_n, lb, g, mc, mo, ood_t, ct, ood_c, cc, zm)
    want = oracle.deep_compose(ev.to_host(), cm.to_host(), *args)
    return ev, cm, args, want, n, N


@pytest.mark.parametrize("lb", [2, 3, 4])
@pytest.mark.parametrize("log_n", [4, 10])
def test_deep_compose_above_blowup_2_vs_oracle(ctx, be, oracle, log_n, lb):
    """tests/test_gpu_parity.py::test_deep_compose_vs_oracle's recipe at log_blowup 2, 3, 4: ss_deep_compose reads every 2^lb-th row and
    extends the n sub-coset values to N"""
    n = 1 << log_n
    mask = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 5 % n), (0, n - 1), (2, 1)]
    ev, cm, args, want, n, N = _deep_case(ctx, be, oracle, log_n, lb, 3, mask, 70)
    out = ctx.alloc(32 * N)
    ctx.deep_compose(ev.cols, cm.cols, *args, out)
    assert np.array_equal(out.download(np.uint64, (N, 4)), want)
    ctx.deep_prepare(2, log_n, args[2], args[-1])            # the tables queued ahead (as the provers do) are the ones it uses
    out2 = ctx.alloc(32 * N)
    ctx.deep_compose(ev.cols, cm.cols, *args, out2)
    assert np.array_equal(out2.download(np.uint64, (N, 4)), want)
    # consistent out-of-domain values => a polynomial of degree < n on all N points
    ctx.ntt([out], log_n + lb, be.INVERSE, args[2])
    assert not np.any(out.download(np.uint64, (N, 4))[n:])


def test_deep_rational_path_at_blowup_4(ctx, be, oracle, monkeypatch):
    """the rational path (large mask columns as A_c(x) / B(x): from 2^20 points on) forced at 2^10 rows the way
    tests/test_gpu_parity.py::test_deep_compose_of_a_layout_sized_mask forces it, at log_blowup 2: the taps' values and the oracle's"""
    log_n, lb = 10, 2
    n = 1 << log_n
    rng = np.random.default_rng(1042)
    pick = lambda k, hi: sorted({int(v) for v in rng.integers(0, hi, size=3 * k)} | {0, 1})[:k]
    offs = [pick(40, n), pick(26, min(n, 600)), [0, 1, n - 1], [5]]
    mask = [(c, o) for c in range(4) for o in offs[c]] + [(0, offs[0][3]), (1, offs[1][2] + n)]
    ev, cm, args, want, n, N = _deep_case(ctx, be, oracle, log_n, lb, 4, mask, 700)
    out, out_taps = ctx.alloc(32 * N), ctx.alloc(32 * N)
    monkeypatch.setenv("SS_DEEP_RATIONAL_MIN_LOG", "8")
    ctx.deep_compose(ev.cols, cm.cols, *args, out)
    monkeypatch.setenv("SS_DEEP_TAPS", "1")
    ctx.deep_compose(ev.cols, cm.cols, *args, out_taps)
    got = out.download(np.uint64, (N, 4))
    assert np.array_equal(got, out_taps.download(np.uint64, (N, 4)))
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------ 3. whole proofs
def example_files():
    """the reference's example run as `cairo-run` wrote it (2^14 steps) and its public input"""
    from sandstorm_amd import public_input
    with open(os.path.join(GOLD, "example", "trace.bin"), "rb") as f:
        trace_bin = f.read()
    with open(os.path.join(GOLD, "example", "memory.bin"), "rb") as f:
        memory_bin = f.read()
    return trace_bin, memory_bin, public_input.AirPublicInput.from_json(os.path.join(GOLD, "air_public_input_array_sum.json"))


def claim_parts(be, claim):
    return (be.TREE_FRIENDLY, N_FRIENDLY, be.COIN_CAIRO) if claim == "cairo" else (be.TREE_KECCAK, 0, be.COIN_SOLIDITY)


class RecursiveExample:
    """the shipped example on one context: files -> proof through the device generator or the host generator"""

    def __init__(self):
        from sandstorm_amd import backend as be, hostlib
        self.trace_bin, self.memory_bin, self.pi = example_files()
        self.n = 16 * (len(self.trace_bin) // 24)
        self.log_n = self.n.bit_length() - 1
        self.ctx = be.Context(0)
        self.dev = [self.ctx.alloc(32 * self.n) for _ in range(7)]
        self.air = hostlib.RecursiveHostAir(self.ctx, self.pi, self.log_n)           # tables of the 2n-point coset, whatever the blowup
        self.keep = []

    def build_extension(self, challenges):
        from sandstorm_amd import hostlib
        from sandstorm_amd.layouts import recursive as rec
        aux = (rec.COL_NPC, rec.COL_MEMORY, rec.COL_RANGE_CHECK, rec.COL_DILUTED_UNORDERED, rec.COL_DILUTED_ORDERED)
        for m in self.keep:
            m.close()
        self.keep = [hostlib.build_extension_columns(self.ctx, "recursive", [self.dev[c] for c in aux], self.n, challenges)]
        return self.keep[-1].cols

    def seed(self, claim):
        from sandstorm_amd import backend as be, public_input
        return public_input.public_coin_seed(self.pi, claim_parts(be, claim)[2])

    def prove(self, claim, options, host_generator=False):
        from sandstorm_amd import backend as be, hostlib
        tree, nf, coin = claim_parts(be, claim)
        if host_generator:
            views = [np.zeros((self.n, 4), dtype=np.uint64) for _ in range(7)]
            return hostlib.prove_files(self.ctx, "recursive", self.trace_bin, self.memory_bin, self.pi, None, views, self.dev, self.air, tree, nf, coin,
                                       self.seed(claim), self.build_extension, options)[0]
        return hostlib.prove_files_device(self.ctx, "recursive", self.trace_bin, self.memory_bin, self.pi, None, self.dev, self.air, tree, nf, coin,
                                          self.seed(claim), self.build_extension, options)[0]

    def close(self):
        for m in self.keep:
            m.close()
        self.air.close()
        self.dev = None
        self.ctx.close()


@pytest.fixture(scope="module")
def example():
    e = RecursiveExample()
    yield e
    e.close()


def both_verifiers(raw, air_cpp, air_py, tree, coin, seed, opt, nf, bits=80):
    from sandstorm_amd import hostlib, verifier
    pos = hostlib.verify(air_cpp, tree, coin, seed, raw, required_security_bits=bits, expected_options=opt, n_friendly_layers=nf)
    assert verifier.verify(raw, air_py, tree, coin, seed, required_security_bits=bits, expected_options=opt, n_friendly_layers=nf) == pos
    return pos


def both_reject(raw, air_cpp, air_py, tree, coin, seed, opt, nf, bits=80):
    from sandstorm_amd import hostlib, verifier
    from sandstorm_amd._lib import SandstormHipError
    with pytest.raises(SandstormHipError):
        hostlib.verify(air_cpp, tree, coin, seed, raw, required_security_bits=bits, expected_options=opt, n_friendly_layers=nf)
    with pytest.raises(verifier.VerificationError):
        verifier.verify(raw, air_py, tree, coin, seed, required_security_bits=bits, expected_options=opt, n_friendly_layers=nf)


def altered_copies(raw, tree):
    """-> the proof with one composition out-of-domain value altered, and with one opened composition row altered"""
    from sandstorm_amd import wire
    a = wire.parse(raw, tree)
    a.ood_composition[1] = (a.ood_composition[1] + 1) % P
    b = wire.parse(raw, tree)
    b.composition_rows[len(b.composition_rows) // 2] = (b.composition_rows[len(b.composition_rows) // 2] + 1) % P
    return wire.serialize(a), wire.serialize(b)


@pytest.mark.parametrize("claim", ["cairo", "eth"])
@pytest.mark.parametrize("blowup,queries", PAIRS)
def test_recursive_example_proofs_verify(example, claim, blowup, queries):
    """tests/golden/example/{trace,memory}.bin, 2^14 steps, under the CairoVerifierClaim and under Keccak trees + the Solidity coin,
    through hostlib.prove_files_device: the C++ verifier and verifier.py accept the bytes, the options byte is the request, an altered
    composition value (out of domain, or in an opened row) is refused by both, and the host-generated path writes the same bytes"""
    from sandstorm_amd import backend as be, wire
    from sandstorm_amd.layouts import recursive as rec
    from sandstorm_amd.prover import ProofOptions
    opt = ProofOptions(num_queries=queries, lde_blowup_factor=blowup)
    tree, nf, coin = claim_parts(be, claim)
    seed = example.seed(claim)
    raw = example.prove(claim, opt)
    assert raw[1] == blowup and raw[0] == queries
    parsed = wire.parse(raw, tree)
    assert parsed.options[1] == blowup and parsed.trace_len == example.n and len(parsed.ood_composition) == 2
    assert wire.serialize(parsed) == raw
    args = (example.air, rec.verifier_air(example.pi), tree, coin, seed, opt, nf)
    pos = both_verifiers(raw, *args)
    assert len(pos) == len(parsed.base_openings) and all(p < example.n * blowup for p in pos)
    for bad in altered_copies(raw, tree):
        both_reject(bad, *args)
    assert example.prove(claim, opt, host_generator=True) == raw


def test_starknet_statement_at_blowup_4():
    """the statement tests/test_gpu_reference_proof.py proves (the reference's array-sum run under the starknet layout, 2^17 steps,
    masked Keccak trees + the Solidity coin), base trace by the device generator, at blowup 4 with 32 queries: both verifiers accept,
    and refuse the altered copies"""
    from sandstorm_amd import backend as be, binary, hostlib, public_input, wire
    from sandstorm_amd.layouts import starknet as sk
    from sandstorm_amd.prover import ProofOptions
    from tests.test_layout_starknet import starknet_example
    states, memory, spi = starknet_example(17)
    log_n = 21
    n = 1 << log_n
    ctx = be.Context(0)
    cols = hostlib.device_base_trace(ctx, "starknet", binary.write_register_states(states), binary.write_memory(memory), spi)
    del states, memory
    air = hostlib.StarknetHostAir(ctx, spi, log_n)
    seed = public_input.public_coin_seed(spi, be.COIN_SOLIDITY)
    keep = []

    def build_extension(challenges):
        keep.append(hostlib.build_extension_columns(ctx, "starknet", [cols[sk.COL_NPC], cols[sk.COL_MEMORY], cols[sk.COL_RANGE_CHECK]], n, challenges))
        return keep[-1].cols
    opt = ProofOptions(num_queries=32, lde_blowup_factor=4)
    try:
        raw = hostlib.prove(ctx, air, be.TREE_KECCAK_M20, 0, be.COIN_SOLIDITY, seed, cols, log_n, build_extension, opt, wire=True)
        assert raw[1] == 4 and wire.parse(raw).trace_len == n
        args = (air, sk.verifier_air(spi), be.TREE_KECCAK_M20, be.COIN_SOLIDITY, seed, opt, 0)
        both_verifiers(raw, *args)
        for bad in altered_copies(raw, be.TREE_KECCAK_M20):
            both_reject(bad, *args)
    finally:
        for m in keep:
            m.close()
        air.close()
        del cols
        ctx.close()


@pytest.mark.parametrize("blowup,queries", [(4, 12), (16, 6)])
def test_mini_air_cpp_host_writes_the_python_mirrors_bytes(ctx, oracle, blowup, queries):
    """tests/mini_air.py: the C++ host on this device (sub-sampled LDE rows) and sandstorm_amd/prover.py on the CPU oracle (which
    evaluates the kept coefficient columns on the 2n-point coset instead) write the same wire bytes, and both verifiers accept them"""
    import dataclasses
    from sandstorm_amd import backend as be, hostlib
    from tests import sharded_host_cases as cases
    from tests.test_cpu_pipeline import cpu_mini_proof
    from tests.test_verifier import mini_verifier_air
    log_n = 6
    _, case = cases.mini_case(log_n, 4)
    tree, nf, coin, opt, host, _ = case
    opt = dataclasses.replace(opt, num_queries=queries, lde_blowup_factor=blowup)
    raw = cases.single_device_mini(ctx, (tree, nf, coin, opt, host, log_n))
    assert raw[1] == blowup
    assert raw == cpu_mini_proof(oracle, log_n, opt, bytes(range(32)))
    cpp = hostlib.HostAir(None, hostlib.AIR_MINI, log_n)
    try:
        both_verifiers(raw, cpp, mini_verifier_air(), tree, coin, bytes(range(32)), opt, nf, bits=16)
    finally:
        cpp.close()


# ------------------------------------------------------------------------------------------------------ 4. an independent route
def test_composition_columns_by_the_wasteful_route(example, oracle):
    """blowup 4, recursive 2^14 steps.  With the proof's challenges and composition coefficient the constraints are evaluated on ALL
    4n LDE rows by ss_eval_quotient at log_blowup = 2 with an AIR whose tables are built for that coset - code this feature leaves as
    it was - and interpolated at size 4n on the device.  On the host: coefficients 2n .. 4n - 1 are zero (degree-2 constraints), and
    the even and the odd coefficients, evaluated at z^2 with Python integers, are the proof's two composition out-of-domain values."""
    from sandstorm_amd import backend as be, hostlib
    from sandstorm_amd.prover import ProofOptions
    ctx, n, log_n = example.ctx, example.n, example.log_n
    g = oracle.to_mont([3])[0]
    opt = ProofOptions(num_queries=32, lde_blowup_factor=4)
    hostlib.device_base_trace(ctx, "recursive", example.trace_bin, example.memory_bin, example.pi, None, example.dev)
    proof = hostlib.prove(ctx, example.air, be.TREE_KECCAK, 0, be.COIN_SOLIDITY, example.seed("eth"), example.dev, log_n, example.build_extension, opt)
    ext = example.build_extension(proof.challenges)
    ev, _ = be.Matrix(ctx, list(example.dev) + list(ext), n).lde(2, g, keep_coeffs=False)
    air4 = hostlib.RecursiveHostAir(ctx, example.pi, log_n, 2)                      # tables over the 4n-point coset
    try:
        program, tables, desc = hostlib.prover_air(air4).build_program(n, proof.challenges, proof.composition_coeff)
        out = ctx.alloc(32 * 4 * n)
        ctx.eval_quotient(program, tables, desc, ev.cols, log_n, 2, g, out)
        ctx.ntt([out], log_n + 2, be.INVERSE, g)                                    # natural-order coefficients of H
        coeffs = out.download(np.uint64, (4 * n, 4))
    finally:
        air4.close()
    assert np.any(coeffs[:2 * n]) and not np.any(coeffs[2 * n:])
    h = oracle.from_mont(coeffs[:2 * n])
    z2 = pow(int(oracle.from_mont(proof.z[None, :])[0]), 2, P)
    for k in range(2):
        acc = 0
        for c in h[k::2][::-1]:
            acc = (acc * z2 + int(c)) % P
        assert acc == int(oracle.from_mont(proof.ood_composition[k][None, :])[0]), k


# ------------------------------------------------------------------------------------------------------ 5. sharded
@pytest.fixture(scope="module")
def single_device_blowup_4(example):
    from sandstorm_amd.prover import ProofOptions
    return example.prove("cairo", ProofOptions(num_queries=32, lde_blowup_factor=4))


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_from_files_writes_the_single_device_bytes(world, single_device_blowup_4, monkeypatch):
    """two and four ranks - threads of this process, each with its own context on the one device - at blowup 4, from the files
    (hostlib.prove_files_sharded_device): every rank sub-samples its row block and halo, the coefficient exchange is the one of blowup 2"""
    from sandstorm_amd import backend as be, hostlib
    from sandstorm_amd.prover import ProofOptions
    from tests.test_gpu_sharded_files import proof_of, run_file_ranks
    monkeypatch.setenv("SSH_FRI_SPREAD_MIN_LOG", "6")          # the ranks fold these small FRI layers together too (sharded.cpp)
    trace_bin, memory_bin, pi = example_files()
    from sandstorm_amd import public_input
    seed = public_input.public_coin_seed(pi, be.COIN_CAIRO)
    log_n = (len(trace_bin) // 24).bit_length() - 1 + 4
    opt = ProofOptions(num_queries=32, lde_blowup_factor=4)

    def prove(rank, world, ctx, group):
        air = hostlib.RecursiveHostAir(ctx, pi, log_n)
        try:
            return hostlib.prove_files_sharded_device(ctx, "recursive", trace_bin, memory_bin, pi, None, air, be.TREE_FRIENDLY, N_FRIENDLY, be.COIN_CAIRO, seed,
                                                      rank, world, group, opt)
        finally:
            air.close()
    out, errs, _ = run_file_ranks(world, prove)
    assert proof_of(out, errs) == single_device_blowup_4


def test_sharded_driver_with_one_rank_writes_the_single_device_bytes(example, single_device_blowup_4):
    """hostlib.prove_sharded with a group of one (ss_eval_quotient on the whole sub-sampled columns)"""
    from sandstorm_amd import backend as be, hostlib
    from sandstorm_amd.prover import ProofOptions
    opt = ProofOptions(num_queries=32, lde_blowup_factor=4)
    ctx = example.ctx
    hostlib.device_base_trace(ctx, "recursive", example.trace_bin, example.memory_bin, example.pi, None, example.dev)
    group = hostlib.LocalGroup(1)
    try:
        raw = hostlib.prove_sharded(ctx, example.air, be.TREE_FRIENDLY, N_FRIENDLY, be.COIN_CAIRO, example.seed("cairo"), 0, 1, group,
                                    dict(enumerate(example.dev)), example.log_n,
                                    lambda ch: {7 + k: c for k, c in enumerate(example.build_extension(ch))}, opt)
    finally:
        group.close()
    assert raw == single_device_blowup_4


# ------------------------------------------------------------------------------------------------------ 6. refusals
@pytest.mark.parametrize("blowup", [1, 3, 32])
def test_other_blowup_factors_are_refused(example, blowup):
    """the message names the accepted set, and the refusal comes before any device work: the base columns, pre-filled, come back as
    they were - neither the device generator nor an upload of the host generator has written them; the context proves at blowup 2
    afterwards (the committed proof)"""
    from sandstorm_amd._lib import SandstormHipError
    from sandstorm_amd.prover import ProofOptions
    fill = np.full((example.n, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    for col in example.dev:
        col.upload(fill)
    with pytest.raises(SandstormHipError, match="2, 4, 8 or 16"):
        example.prove("cairo", ProofOptions(lde_blowup_factor=blowup))
    with pytest.raises(SandstormHipError, match="2, 4, 8 or 16"):
        example.prove("cairo", ProofOptions(lde_blowup_factor=blowup), host_generator=True)
    for c, col in enumerate(example.dev):
        assert np.array_equal(col.download(np.uint64, (example.n, 4)), fill), "base column %d was written by a refused call" % c
    with open(os.path.join(GOLD, "array_sum_recursive_cairo.proof"), "rb") as f:
        assert example.prove("cairo", ProofOptions()) == f.read()


def test_an_air_built_for_the_lde_blowup_is_refused(example):
    """an AIR whose tables are laid out over the 4n-point coset (log_ce_blowup = 2) handed to a prover at blowup 4: refused by name of
    the quantity, not proven with the wrong tables"""
    from sandstorm_amd import backend as be, hostlib
    from sandstorm_amd._lib import SandstormHipError
    from sandstorm_amd.prover import ProofOptions
    air4 = hostlib.RecursiveHostAir(example.ctx, example.pi, example.log_n, 2)
    assert air4.log_ce_blowup == 2 and example.air.log_ce_blowup == 1 and hostlib.prover_air(air4).log_ce_blowup == 2
    try:
        with pytest.raises(SandstormHipError, match="log_ce_blowup"):
            hostlib.prove(example.ctx, air4, be.TREE_KECCAK, 0, be.COIN_SOLIDITY, example.seed("eth"), example.dev, example.log_n, example.build_extension,
                          ProofOptions(num_queries=32, lde_blowup_factor=4), wire=True)
    finally:
        air4.close()
