"""Every FRI folding factor through every prover, on the device: the Python host and the C++ host on one device, the sharded prover
with its layers spread over the ranks (and with a folding factor below the number of ranks, where nothing spreads), and both hosts of
the 64-bit field - at folds 2, 4 and 16, which no proof of this library had been built with.  The reference of every device-made
proof is the same host code over the CPU oracle (tests/test_fri_options_on_host.py), run in the same test and compared bit for bit;
the sizes are the smallest that reach two layers and the spread branch.  A geometry the verifiers refuse is refused by every prover
before its first launch."""
import os
import threading

import numpy as np
import pytest

from tests.sharded_host_cases import mini_case, run_ranks, single_device_mini
from tests.test_fri_options_on_host import (REFUSED, SEED, check_gl_proof, check_mini_proof, gl_example, gl_options, gl_proof, mini_options, mini_proof,
                                            oracle_gl_proof, oracle_mini_proof)

pytestmark = pytest.mark.gpu
EMULATED = os.environ.get("SS_TEST_HIPEMU") == "1"          # (the device code on the CPU: torch CPU tensors are its device buffers)
N_PROFILE_KINDS = 8                                         # SS_PROF_KINDS of include/sandstorm_hip.h


@pytest.fixture(scope="module")
def ctx():
    from sandstorm_amd import backend as be
    c = be.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gl_ctx():
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


@pytest.fixture(autouse=True)
def spread_small_fri_layers(monkeypatch):
    """the ranks fold FRI layers above 2^21 values together: make these small proofs do it too (sharded.cpp)"""
    monkeypatch.setenv("SSH_FRI_SPREAD_MIN_LOG", "6")


def launches(c):
    return sum(c.profile_read(kind)[1] for kind in range(N_PROFILE_KINDS))


def cpp_case(fold, log_n, max_remainder, flavour="eth"):
    """the statement of mini_proof for the C++ hosts (tests/sharded_host_cases.py: same trace, seed, queries and grinding bits)"""
    make, case = mini_case(log_n, max_remainder, flavour)
    case[3].fri_folding_factor = fold                       # (the options object the ranks' closures share)
    return make, case


def cpp_transcript(ctx, case):
    """the same statement through hostlib.prove's flat dump, which keeps the transcript's values -> the parsed Proof"""
    from sandstorm_amd import backend as be, hostlib
    from sandstorm_amd.coin import canonical
    from tests import mini_air
    tree, nf, coin, opt, host, log_n = case
    air = hostlib.HostAir(ctx, hostlib.AIR_MINI, log_n)
    base = [ctx.column(host[0]), ctx.column(host[1])]
    c0 = [canonical(v) for v in host[0]]
    keep = []

    def ext(challenges):
        keep.append(ctx.column(np.stack([be.felt(v) for v in mini_air.extension_trace(c0, canonical(challenges[0]))])))
        return [keep[-1]]
    try:
        return hostlib.prove(ctx, air, tree, nf, coin, SEED, base, log_n, ext, opt)
    finally:
        air.close()


# ------------------------------------------------------------------------------------------------------ 252-bit field, one device
@pytest.mark.parametrize("fold,log_n,flavour", [(f, l, "eth") for f in (2, 4, 16) for l in (5, 9)] + [(16, 6, "cairo")])
def test_both_hosts_write_the_oracle_pipelines_proof(ctx, oracle, fold, log_n, flavour):
    """rows of 2, 4 and 16 values under the Keccak-masked tree (and of 16 under masked Blake2s + Pedersen), bit-reversed column order
    over 1, 2 and 4 bits, layer offsets offset^(fold^i), positions folded by q >> log2 fold - in prover.py and in host/prover.cpp, over
    the kernels: the bytes of the same host code over the CPU oracle, accepted by both verifiers"""
    from sandstorm_amd import backend as be
    want, want_proof = oracle_mini_proof(oracle, fold, log_n, 4, flavour)
    options = mini_options(fold, 4)
    _, case = cpp_case(fold, log_n, 4, flavour)
    # A friendly tree makes its context build the Pedersen window tables - up to 23.6 GB, kept by the process until no context uses them
    # and one is trimmed: a context of its own, closed here, so that the tests at the device's capacity later in the session find the room
    own = be.Context(0) if flavour == "cairo" else None
    c = own or ctx
    try:
        raw, proof = mini_proof(c, oracle, log_n, options, flavour)
        cpp_raw, cpp_proof = single_device_mini(c, case), cpp_transcript(c, case)
    finally:
        if own is not None:
            own.close()
            ctx.trim()
    assert raw == want
    assert cpp_raw == want
    check_mini_proof(raw, proof, log_n, options, flavour, tamper=False)
    # The wire format carries no challenge, and a layer folded with (draw * offset) over the domain offset * <w> does not depend on the
    # offset: a wrong layer offset shows in the challenges alone (and in a proof made with Conventions.fri_alpha_times_offset off)
    for name, p in (("prover.py", proof), ("host/prover.cpp", cpp_proof)):
        assert len(p.fri_alphas) == len(want_proof.fri_alphas) == len(want_proof.fri_layers) >= 1, name
        for li, (got, exp) in enumerate(zip(p.fri_alphas, want_proof.fri_alphas)):
            assert np.array_equal(np.asarray(got, dtype=np.uint64), np.asarray(exp, dtype=np.uint64)), (name, "challenge of layer %d" % li)


# -------------------------------------------------------------------------------------------------------- the sharded prover
@pytest.mark.parametrize("fold,world", [(16, 2), (16, 8), (4, 4), (2, 2), (2, 4), (4, 8)])
def test_sharded_prover_writes_the_single_device_proof(oracle, fold, world):
    """2^9 rows, layers above 2^6 values spread: fold 16 on 2 and 8 ranks (8 and 2 columns of a layer per rank; on 8 ranks ONE spread
    layer, the second is too short for 8 x 8 row blocks), fold 4 on 4 ranks (one column each), fold 2 on 2 - and fold 2 on 4 ranks,
    fold 4 on 8: fewer columns than ranks, nothing spreads and rank 0 folds every layer.  The single-device proof, byte for byte"""
    want, _ = oracle_mini_proof(oracle, fold, 9, 4)
    make, _ = cpp_case(fold, 9, 4)
    assert run_ranks(world, make(world)) == want


# --------------------------------------------------------------------------------------------------------------- 64-bit field
@pytest.mark.parametrize("fold,hash_name", [(2, "blake2s"), (4, "blake2s"), (16, "blake2s"), (16, "sha256")])
def test_both_hosts_of_the_64_bit_field_write_the_oracle_pipelines_proof(gl_ctx, fold, hash_name):
    """goldilocks.Prover and hostlib.gl_prove over the kernels: rows of `fold` Fq3 values through ss_hash_rows_gl64, the trees, the
    gathers and ss_fri_fold_gl64x3 with offsets 7^(fold^i) - the arrays of the same prover over the oracle, array for array"""
    import torch
    from sandstorm_amd import goldilocks as gs, hostlib
    c, dev = gl_ctx
    options = gl_options(fold, 16, hash_name)
    want = gs.proof_to_arrays(oracle_gl_proof(fold, 16, hash_name))
    proof = gl_proof(c, options, dev)
    pi, cols = gl_example()
    base = [torch.from_numpy(np.array(col, dtype=np.uint64).view(np.int64)).to(dev) for col in cols]
    cpp = hostlib.gl_prove(c, gs.plain_air(), options, SEED, base, lambda ch: gs.plain_extension_on_device(c, base, ch)[0], statement=pi)
    for name, p in (("goldilocks.Prover", proof), ("hostlib.gl_prove", cpp)):
        got = gs.proof_to_arrays(p)
        assert set(got) == set(want), name
        for k in sorted(want):
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (name, k)
        check_gl_proof(p, options, tamper=False)


@pytest.mark.parametrize("nseg", [2, 4, 16])
def test_rows_of_fri_layers_of_the_64_bit_field_against_hashlib(ctx, nseg):
    """ss_hash_rows_gl64 at (segments, words per segment) = (fold, 3), the rows FRI commits at folds 2, 4 and 16: 48, 96 and 384 bytes
    - 384 is six whole SHA-256 / Blake2s blocks, where the padding opens a block of its own and Blake2s's last block is a full one.
    300 rows: more than one workgroup, and not a whole number of them"""
    import hashlib
    from sandstorm_amd import backend as be
    from sandstorm_amd.coin import keccak256
    rng = np.random.default_rng(300 + nseg)
    nrows, seg_len = 300, 3
    segs = [rng.integers(0, 2**64 - 2**32 + 1, size=nrows * seg_len, dtype=np.uint64) for _ in range(nseg)]
    segs[0][:3] = 2**64 - 2**32                              # the field's largest word in the first row
    d_segs = [ctx.column(s) for s in segs]
    rows = [b"".join(int(s[i * seg_len + e]).to_bytes(8, "little") for s in segs for e in range(seg_len)) for i in range(nrows)]
    for kind, h in ((be.HASH_KECCAK, keccak256), (be.HASH_SHA256, lambda d: hashlib.sha256(d).digest()), (be.HASH_BLAKE2S, lambda d: hashlib.blake2s(d).digest())):
        out = ctx.alloc(32 * nrows)
        ctx.hash_rows_gl64(d_segs, seg_len, nrows, out, kind)
        got = out.download(np.uint8, (nrows, 32))
        assert [bytes(r) for r in got] == [h(r) for r in rows], kind


# ----------------------------------------------------------------------------------------------------- refusal on the device
@pytest.mark.parametrize("log_n,fold,max_remainder", REFUSED)
def test_no_prover_launches_anything_for_a_geometry_the_verifiers_refuse(ctx, gl_ctx, oracle, log_n, fold, max_remainder):
    """the two geometries that used to end in a Merkle tree of one row (after five commitments) and in a shift by 2^32 - 1: every
    prover raises the rule's error, and the profiler has counted no launch - Python and C++ on one device, the sharded prover on two
    ranks, and both hosts of the 64-bit field (there: 16-fold layers down to a bound of 1, which 2048 points do not reach)"""
    import torch
    from sandstorm_amd import backend as be, goldilocks as gs, hostlib
    from sandstorm_amd._lib import SandstormHipError
    rule = "FRI geometry refused: .*trace length %d, folding factor %d, max remainder coefficients %d" % (1 << log_n, fold, max_remainder)
    options = mini_options(fold, max_remainder)
    ctx.profile(True)
    try:
        ctx.profile_reset()
        with pytest.raises(ValueError, match=rule):
            mini_proof(ctx, oracle, log_n, options)
        make, case = cpp_case(fold, log_n, max_remainder)
        with pytest.raises(SandstormHipError, match=rule):
            single_device_mini(ctx, case)
        assert launches(ctx) == 0
        mini_proof(ctx, oracle, 5, mini_options(8, 4))      # (the counter does count: a geometry that is taken launches)
        assert launches(ctx) > 0
    finally:
        ctx.profile(False)
    # the sharded prover: two ranks as threads, each with a context of its own
    world, group, seen = 2, hostlib.LocalGroup(2), [None, None]

    def body(rank):
        c = be.Context(0)
        try:
            c.profile(True)
            c.profile_reset()
            air, tree, nf, coin, seed, mine, _, ext, opt = make(world)(rank, c)
            try:
                hostlib.prove_sharded(c, air, tree, nf, coin, seed, rank, world, group, mine, log_n, ext, opt)
                seen[rank] = "proved"
            except SandstormHipError as e:
                seen[rank] = (str(e), launches(c))
            finally:
                air.close()
                del mine
        except BaseException as e:          # noqa: BLE001 - reported below
            seen[rank] = e
        finally:
            c.close()
    threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    group.close()
    for s in seen:
        assert isinstance(s, tuple) and "FRI geometry refused" in s[0] and "trace length %d" % (1 << log_n) in s[0] and s[1] == 0, seen
    # the 64-bit field
    c, dev = gl_ctx
    bad = gl_options(16, 1)
    pi, cols = gl_example()
    base = [torch.from_numpy(np.array(col, dtype=np.uint64).view(np.int64)).to(dev) for col in cols]
    c.profile(True)
    try:
        c.profile_reset()
        with pytest.raises(ValueError, match="FRI geometry refused: .*LDE domain 2048, folding factor 16, max remainder 1"):
            gl_proof(c, bad, dev)
        with pytest.raises(SandstormHipError, match="FRI geometry refused: .*LDE domain 2048, folding factor 16, max remainder 1"):
            hostlib.gl_prove(c, gs.plain_air(), bad, SEED, base, lambda ch: gs.plain_extension_on_device(c, base, ch)[0], statement=pi)
        assert launches(c) == 0
    finally:
        c.profile(False)
