"""Files -> proof over several ranks in ONE call (hostlib.prove_files_sharded_device; host_capi.cpp ssh_prove_files_sharded_device): every
rank is handed the run's trace.bin / memory.bin, makes the base trace on its device, keeps its columns and its rows of the auxiliary
columns, and proves with the others.  The bytes must be the single-device proofs: the committed fixtures, the reference's own proof,
and what hostlib.prove_files_device writes for the same inputs.  Equality is byte for byte.

The ranks are threads of this process, each with its own context (the pattern of tests/sharded_host_cases.run_ranks), an RCCL group of
one, or two processes over gloo (tests/dist_files_sharded_worker.py).  Runs on the MI355X (`-m gpu`) and, in the CPU suite, on the host
build of the device code (tests/test_sharded_files_on_host.py)."""
import copy
import os
import subprocess
import sys
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

pytestmark = pytest.mark.gpu
EMULATED = os.environ.get("SS_TEST_HIPEMU") == "1"
N_FRIENDLY = 22
JOIN_S = 1500 if EMULATED else 300          # no thread may be left waiting: a rank still alive after this fails the test


@pytest.fixture(autouse=True)
def spread_small_fri_layers(monkeypatch):
    """the ranks fold FRI layers above 2^21 values together: make these small proofs do it too (sharded.cpp)"""
    monkeypatch.setenv("SSH_FRI_SPREAD_MIN_LOG", "6")


def example_files():
    """the reference's example run as `cairo-run` wrote it (2^14 steps) and its public input"""
    from sandstorm_amd import public_input
    with open(os.path.join(GOLD, "example", "trace.bin"), "rb") as f:
        trace_bin = f.read()
    with open(os.path.join(GOLD, "example", "memory.bin"), "rb") as f:
        memory_bin = f.read()
    return trace_bin, memory_bin, public_input.AirPublicInput.from_json(os.path.join(GOLD, "air_public_input_array_sum.json"))


def golden_recursive_proof():
    with open(os.path.join(GOLD, "array_sum_recursive_cairo.proof"), "rb") as f:
        return f.read()


def recursive_statement(trace_bin, memory_bin, pi, priv=None):
    """-> prove(rank, world, ctx, group) for the CairoVerifierClaim (FriendlyMerkleTree<22> + the Cairo coin), default options"""
    from sandstorm_amd import backend as be, hostlib, public_input
    seed = public_input.public_coin_seed(pi, be.COIN_CAIRO)
    log_n = (len(trace_bin) // 24).bit_length() - 1 + 4

    def prove(rank, world, ctx, group):
        air = hostlib.RecursiveHostAir(ctx, pi, log_n, 1)
        try:
            return hostlib.prove_files_sharded_device(ctx, "recursive", trace_bin, memory_bin, pi, priv, air, be.TREE_FRIENDLY, N_FRIENDLY, be.COIN_CAIRO, seed,
                                                      rank, world, group)
        finally:
            air.close()
    return prove


def run_file_ranks(world, prove, ctxs=None, group=None, after=None):
    """one thread per rank, each with its own context (or ctxs[rank]); prove(rank, world, ctx, group) -> (bytes / None, times).
    -> (what every rank returned, what every rank raised, after(rank)'s results).  A thread still alive after JOIN_S fails the test."""
    from sandstorm_amd import backend as be, hostlib
    own_group = group is None
    if own_group:
        group = hostlib.LocalGroup(world)
    out, errs, extra = [None] * world, [None] * world, [None] * world

    def body(rank):
        ctx = None
        try:
            ctx = ctxs[rank] if ctxs else be.Context(0)
            out[rank] = prove(rank, world, ctx, group)
            if after:
                extra[rank] = after(rank)              # (on the rank's thread: the generator's stats are per thread)
        except BaseException as e:                     # noqa: BLE001 - handed to the caller
            errs[rank] = e
        finally:
            if ctx is not None and not ctxs:
                ctx.close()
    threads = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_S)
    stuck = [r for r, t in enumerate(threads) if t.is_alive()]
    assert not stuck, "ranks %s are still waiting" % stuck
    if own_group:
        group.close()
    return out, errs, extra


def proof_of(out, errs):
    for e in sorted((e for e in errs if e is not None), key=lambda e: "another rank failed" in str(e)):
        raise e                                        # the rank that failed first, not the ones it released from their barriers
    assert all(o[0] is None for o in out[1:])
    for _, times in out:
        assert 0 < times["trace_gen_s"] <= times["total_s"]
    return out[0][0]


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_recursive_example_from_its_files(world):
    """tests/golden/example/{trace,memory}.bin under the CLI's claim for the recursive layout: tests/golden/array_sum_recursive_cairo.proof
    (the single-device C++ host's).  2 ranks: the seventh base column is left over and spread; 8 ranks: one rank owns no base column"""
    trace_bin, memory_bin, pi = example_files()
    out, errs, _ = run_file_ranks(world, recursive_statement(trace_bin, memory_bin, pi))
    assert proof_of(out, errs) == golden_recursive_proof()


@pytest.mark.parametrize("world", [2, 4])
def test_real_builtin_instances_are_traced_on_every_rank(world):
    """the same run with real Pedersen (one at the top of the field), bitwise and range-check instances: the bytes
    hostlib.prove_files_device writes for the same inputs on one context, and on every rank the given Pedersen and bitwise instances
    traced on the device from their inputs"""
    from sandstorm_amd import backend as be, hostlib, public_input
    from sandstorm_amd.layouts import recursive as rec
    from test_gpu_device_trace import recursive_private
    trace_bin, memory_bin, pi = example_files()
    priv = recursive_private()
    n = 16 * (len(trace_bin) // 24)
    ctx = be.Context(0)
    dev = [ctx.alloc(32 * n) for _ in range(7)]
    air = hostlib.RecursiveHostAir(ctx, pi, n.bit_length() - 1)
    keep = []

    def build_extension(challenges):
        aux = (rec.COL_NPC, rec.COL_MEMORY, rec.COL_RANGE_CHECK, rec.COL_DILUTED_UNORDERED, rec.COL_DILUTED_ORDERED)
        keep.append(hostlib.build_extension_columns(ctx, "recursive", [dev[c] for c in aux], n, challenges))
        return keep[-1].cols
    want, _ = hostlib.prove_files_device(ctx, "recursive", trace_bin, memory_bin, pi, priv, dev, air, be.TREE_FRIENDLY, N_FRIENDLY, be.COIN_CAIRO,
                                         public_input.public_coin_seed(pi, be.COIN_CAIRO), build_extension)
    for m in keep:
        m.close()
    air.close()
    del dev
    ctx.close()
    assert want != golden_recursive_proof()            # (the instances are part of the trace)
    out, errs, stats = run_file_ranks(world, recursive_statement(trace_bin, memory_bin, pi, priv), after=lambda rank: hostlib.trace_last_stats())
    assert proof_of(out, errs) == want
    for s in stats:
        assert s["pedersen_on_device"] == len(priv["pedersen"]) == 3 and s["pedersen_on_host"] == 0, s
        assert s["bitwise_on_device"] == len(priv["bitwise"]) == 9 and s["bitwise_on_host"] == 0, s


def test_the_references_own_proof_from_the_files_two_ranks():
    """tests/golden/reference_array_sum_starknet.proof (the reference's proof of its example under the starknet layout, 2^17 steps): its
    options, its proof-of-work nonce - and two ranks write that file, byte for byte"""
    from sandstorm_amd import backend as be, binary, examples, hostlib, public_input, wire
    from sandstorm_amd.prover import ProofOptions
    with open(os.path.join(GOLD, "reference_array_sum_starknet.proof"), "rb") as f:
        ref_raw = f.read()
    ref = wire.parse(ref_raw)
    states, memory, spi = examples.starknet_example(17)
    trace_bin, memory_bin = binary.write_register_states(states), binary.write_memory(memory)
    del states, memory
    seed = public_input.public_coin_seed(spi, be.COIN_SOLIDITY)

    def prove(rank, world, ctx, group):
        air = hostlib.StarknetHostAir(ctx, spi, 21)
        try:
            return hostlib.prove_files_sharded_device(ctx, "starknet", trace_bin, memory_bin, spi, None, air, be.TREE_KECCAK_M20, 0, be.COIN_SOLIDITY, seed,
                                                      rank, world, group, ProofOptions(*ref.options), pow_nonce=ref.pow_nonce)
        finally:
            air.close()
    out, errs, _ = run_file_ranks(2, prove)
    same = proof_of(out, errs)
    assert len(same) == len(ref_raw)
    assert same == ref_raw, "first differing byte at offset %d" % next(i for i, (a, b) in enumerate(zip(same, ref_raw)) if a != b)


def test_refused_files_release_every_rank():
    """what the generator refuses is refused on every rank before any rank enters a collective: a trace.bin that is not a power of two
    of cycles (a host check), a memory.bin without a cell the run reads (a status bit of the device's kernels).  Nobody is left
    waiting, and the same contexts then prove over a new group"""
    from sandstorm_amd import backend as be
    from sandstorm_amd._lib import SandstormHipError
    trace_bin, memory_bin, pi = example_files()
    pc0 = int.from_bytes(trace_bin[16:24], "little")
    missing = b"".join(memory_bin[o:o + 40] for o in range(0, len(memory_bin), 40) if int.from_bytes(memory_bin[o:o + 8], "little") != pc0)
    ctxs = [be.Context(0) for _ in range(2)]
    try:
        for files, what in (((trace_bin[:24 * 3000], memory_bin), "power of two"), ((trace_bin, missing), "does not hold")):
            out, errs, _ = run_file_ranks(2, recursive_statement(files[0], files[1], pi), ctxs=ctxs)
            assert out == [None, None]
            for e in errs:
                assert isinstance(e, SandstormHipError) and what in str(e), repr(e)
        out, errs, _ = run_file_ranks(2, recursive_statement(trace_bin, memory_bin, pi), ctxs=ctxs)
        assert proof_of(out, errs) == golden_recursive_proof()
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.skipif(EMULATED, reason="the emulated device has no RCCL")
def test_rccl_group_of_one_proves_from_the_files_twice():
    """the RCCL transport as far as one GPU takes it (tests/test_gpu_sharded_host.py test_rccl_transport_with_a_group_of_one): one
    communicator, two proofs from the files"""
    from sandstorm_amd import backend as be, hostlib
    trace_bin, memory_bin, pi = example_files()
    prove = recursive_statement(trace_bin, memory_bin, pi)
    ctx = be.Context(0)
    grp = hostlib.RcclGroup(ctx, hostlib.rccl_unique_id(), 0, 1)
    try:
        for _ in range(2):
            raw, times = prove(0, 1, ctx, grp)
            assert raw == golden_recursive_proof()
            assert 0 < times["trace_gen_s"] <= times["total_s"]
    finally:
        grp.close()                                    # everything that lives in the context's pool goes before the context does
        ctx.close()


def test_two_processes_over_gloo_prove_from_the_files(tmp_path):
    """the ranks as two PROCESSES under torch.distributed.run (tests/dist_files_sharded_worker.py), meeting in the driver's
    CallbackTransport over gloo: every process reads the files itself; the committed proof comes out on rank 0"""
    from tests.hipemu.extra_sharded_host_procs import free_port
    out_path = os.path.join(str(tmp_path), "proof.bin")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(OMP_NUM_THREADS="1")
    env.pop("HIPEMU_THREADS", None)                    # the worker sizes the emulator's pool for its number of ranks
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.join(ROOT, "tests", "dist_files_sharded_worker.py"), out_path]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500 if EMULATED else 600)
    assert out.returncode == 0 and "SHARDED_PROOF_WRITTEN" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    with open(out_path, "rb") as f:
        assert f.read() == golden_recursive_proof()


def test_arguments_that_do_not_fit_the_group_are_refused():
    """a group of another size, another rank of a group, a NULL seed: an error with a message, nothing launched, the context as good
    as before"""
    from sandstorm_amd import backend as be, hostlib, public_input
    from sandstorm_amd._lib import SandstormHipError
    trace_bin, memory_bin, pi = example_files()
    seed = public_input.public_coin_seed(pi, be.COIN_CAIRO)
    ctx = be.Context(0)
    air = hostlib.RecursiveHostAir(ctx, pi, 18, 1)

    def call(rank, world, group, seed=seed):
        return hostlib.prove_files_sharded_device(ctx, "recursive", trace_bin, memory_bin, pi, None, air, be.TREE_FRIENDLY, N_FRIENDLY, be.COIN_CAIRO, seed,
                                                  rank, world, group)
    try:
        two = hostlib.LocalGroup(2)
        with pytest.raises(SandstormHipError, match="another number of ranks"):
            call(0, 4, two)
        with pytest.raises(SandstormHipError, match="rank 2 of 2"):
            call(2, 2, two)
        two.close()
        other = hostlib.CallbackGroup(1, 2, lambda send, sc, rc: b"", lambda mine: bytes(mine) * 2)      # this process is rank 1 of it
        with pytest.raises(SandstormHipError, match="another rank of it"):
            call(0, 2, other)
        other.close()
        one = hostlib.LocalGroup(1)
        with pytest.raises(SandstormHipError, match="NULL argument"):
            call(0, 1, one, seed=None)
        one.close()
        one = hostlib.LocalGroup(1)                    # (a group a rank gave up on stays failed)
        raw, _ = call(0, 1, one)
        one.close()
        assert raw == golden_recursive_proof()
    finally:
        air.close()
        ctx.close()
