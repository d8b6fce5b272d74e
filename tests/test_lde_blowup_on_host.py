"""No GPU: LDE blowup factors above 2 (tests/test_gpu_lde_blowup.py) on the host build of the device code (tests/hipemu, test
infrastructure: see tests/test_device_code_on_host.py), the Python mirror over the CPU oracle, and the row sub-sampling kernel under
AddressSanitizer / UBSan in a stand-alone program."""
import os
import shutil
import subprocess

import pytest

from tests.test_device_code_on_host import CLANG, emulated_library, heavy, run_gpu_tests_on_host  # noqa: F401  (emulated_library: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE = "tests/test_gpu_lde_blowup.py"


def test_subsampling_and_deep_above_blowup_2(emulated_library):
    """ss_subsample_rows over every shape (20 shapes x 1 / 3 / 16 / 17 columns, the tail of the output, its refusals) and DEEP at
    log_blowup 2, 3, 4 (pointwise and rational path) against the oracle, lane by lane on the CPU"""
    out = run_gpu_tests_on_host(emulated_library, [FILE, "-k", "subsample or deep"])
    assert "28 passed" in out, out[-500:]                    # 20 shapes + the refusals + 6 DEEP sizes + the rational path


def test_cpp_host_and_python_mirror_write_the_same_bytes(emulated_library):
    """the mini AIR at blowup 4 and 16: the C++ prover on the emulated library (ss_subsample_rows) and sandstorm_amd/prover.py on
    oracle/cpu_context.py (ctx.evaluate of the coefficient columns) write the same wire bytes; both verifiers accept"""
    out = run_gpu_tests_on_host(emulated_library, [FILE, "-k", "mini_air"])
    assert "2 passed" in out, out[-500:]


def test_python_mirror_proves_at_every_blowup_on_the_cpu_oracle(oracle):
    """sandstorm_amd/prover.py over oracle/cpu_context.py alone (no device code at all): proofs at blowup 4, 8 and 16 that both
    verifiers accept and that carry the blowup in their options byte; blowup 3 is refused by name of the accepted set"""
    from sandstorm_amd import backend as be, hostlib
    from sandstorm_amd.prover import ProofOptions
    from tests.test_cpu_pipeline import cpu_mini_proof
    from tests.test_verifier import mini_verifier_air, pv
    seed, log_n = bytes(range(32)), 6
    cpp = hostlib.HostAir(None, hostlib.AIR_MINI, log_n)
    for blowup, queries in ((4, 12), (8, 8), (16, 6)):
        opt = ProofOptions(num_queries=queries, lde_blowup_factor=blowup, grinding_factor=8, fri_max_remainder_coeffs=4)
        raw = cpu_mini_proof(oracle, log_n, opt, seed)
        assert raw[1] == blowup
        pos = pv(raw, mini_verifier_air(), be.TREE_KECCAK_M20, be.COIN_SOLIDITY, seed)
        assert len(pos) >= 1 and all(p < (blowup << log_n) for p in pos)
        assert hostlib.verify(cpp, be.TREE_KECCAK_M20, be.COIN_SOLIDITY, seed, raw, required_security_bits=16, expected_options=opt) == pos
    cpp.close()
    with pytest.raises(ValueError, match="2, 4, 8 or 16"):
        cpu_mini_proof(oracle, log_n, ProofOptions(num_queries=8, lde_blowup_factor=3, grinding_factor=8, fri_max_remainder_coeffs=4), seed)


def test_python_mirror_refuses_an_air_built_for_another_coset(oracle):
    """prover.Air.log_ce_blowup: the mirror guards it as the C++ provers do (an AIR laid out for the LDE's blowup would give a wrong
    composition with no message), the layouts' make_air carries it, and hostlib.HostAir checks the request against what the handle holds"""
    import dataclasses
    import inspect
    from oracle.cpu_context import CpuContext
    from sandstorm_amd import backend as be, hostlib
    from sandstorm_amd._lib import SandstormHipError
    from sandstorm_amd.layouts import recursive as rec, starknet as sk
    from sandstorm_amd.prover import Claim, ProofOptions, Prover
    from tests import mini_air
    ctx = CpuContext()
    c0, c1 = mini_air.base_trace(32)
    base = be.Matrix.from_host(ctx, [oracle.to_mont(c0), oracle.to_mont(c1)])
    air = dataclasses.replace(mini_air.make_air(oracle.to_mont), log_ce_blowup=2)
    with pytest.raises(ValueError, match="log_ce_blowup"):
        Prover(ctx, Claim(air, be.LeafVariantMerkleTree, be.COIN_SOLIDITY), ProofOptions(num_queries=8, lde_blowup_factor=4, grinding_factor=4)).prove(
            bytes(32), base, lambda ch: None)
    for make in (rec.make_air, sk.make_air, rec.verifier_air, sk.verifier_air):
        assert "log_ce_blowup" in inspect.signature(make).parameters and "log_blowup" not in inspect.signature(make).parameters
    with pytest.raises(SandstormHipError, match="log_ce_blowup"):
        hostlib.HostAir(None, hostlib.AIR_MINI, 5, 2)
    ok = hostlib.HostAir(None, hostlib.AIR_MINI, 5)
    assert ok.log_ce_blowup == 1
    ok.close()


def test_recursive_example_proofs_at_blowup_4_8_16(emulated_library):
    """the shipped recursive example, 2^14 steps, both claims, (blowup, queries) = (4, 32), (8, 22), (16, 16): files -> proof through
    the emulated device code, both verifiers, the altered copies, the host-generated path's bytes"""
    heavy()
    out = run_gpu_tests_on_host(emulated_library, [FILE, "-k", "recursive_example_proofs_verify"], timeout=3400)
    assert "6 passed" in out, out[-500:]


def test_sharded_on_two_ranks_at_blowup_4(emulated_library):
    """two thread-ranks at blowup 4 from the files: a rank's block and halo sub-sampled, ss_eval_quotient_rows on the 2n-point coset,
    the single-device bytes"""
    heavy()
    os.environ["HIPEMU_THREADS"] = "1"           # the emulator's worker pool serves one launching thread: the ranks are the parallelism
    try:
        out = run_gpu_tests_on_host(emulated_library, [FILE, "-k", "sharded_from_files and 2"], timeout=2400)
    finally:
        del os.environ["HIPEMU_THREADS"]
    assert "1 passed" in out, out[-500:]


def test_subsampling_kernel_under_the_sanitizers(tmp_path):
    """tests/cpp/subsample_rows_host_test.cpp: a program of its own - csrc/deep.hip's host build, the emulated runtime and a main that
    drives the kernel over case 1's shapes with heap blocks of exactly the documented sizes - built with
    -fsanitize=address,undefined.  (Leak checking is off: the emulated runtime keeps its lanes' stacks for the next launch.)"""
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no clang++ to build the host emulation with (%s)" % CLANG)
    exe = str(tmp_path / "subsample_rows_host_test")
    emu = os.path.join(ROOT, "tests", "hipemu")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O1", "-g1", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", emu, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "sandstorm_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "subsample_rows_host_test.cpp"), os.path.join(ROOT, "sandstorm_amd", "csrc", "deep.hip"),
                           os.path.join(emu, "hipemu.cpp"), "-pthread", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and "60 launches, 0 mismatches" in out.stdout, out.stdout[-1000:] + out.stderr[-3000:]
