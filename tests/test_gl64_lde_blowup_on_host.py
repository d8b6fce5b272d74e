"""No GPU: the 64-bit field's claim at LDE blowup 4, 8 and 16 (tests/test_gpu_gl64_lde_blowup.py) on the host build of the device code
(tests/hipemu, test infrastructure: see tests/test_device_code_on_host.py) - the same tests, lane by lane on the CPU -, the verifier's
rules, which need no device at all, and the row sub-sampling kernel under AddressSanitizer / UBSan in a stand-alone program."""
import dataclasses
import os
import shutil
import subprocess

import pytest

from tests.test_device_code_on_host import CLANG, emulated_library, run_gpu_tests_on_host  # noqa: F401  (emulated_library: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE = "tests/test_gpu_gl64_lde_blowup.py"


def test_subsampling_kernel_against_numpy_slicing(emulated_library):
    """ss_subsample_rows_gl64 over every shape (8 sizes x 5 strides, each with 1 / 3 / 16 / 17 columns and the output's tail), a
    destination that is not 16-byte aligned, and its refusals"""
    out = run_gpu_tests_on_host(emulated_library, [FILE, "-k", "subsample"])
    assert "42 passed" in out, out[-500:]                    # 40 shapes + the unaligned destination + the refusals


def test_both_hosts_prove_above_blowup_2_and_the_oracle_pipeline_agrees(emulated_library):
    """goldilocks.Prover and hostlib.gl_prove over the emulated device code at log_blowup 2, 3, 4 (folds 2, 8, 16; SHA-256 once): the same
    arrays, accepted by the verifier; the prover over the CPU oracle writes them too (lb = 2 and 4)"""
    out = run_gpu_tests_on_host(emulated_library, [FILE, "-k", "both_hosts or oracle_pipeline"])
    assert "8 passed" in out, out[-500:]                     # 6 cases + the oracle pipeline at lb = 2 and 4


def test_the_split_is_the_composition_files_to_proof_and_refusals(emulated_library):
    """the constraints on all N rows against H0(x^2) + x H1(x^2) from the committed columns (lb = 2, 3); files -> proof at lb = 2 with and
    without validation, a broken cell named; another blowup in the options, log_blowup 0 and 5, the security rule at 32 / 31 queries"""
    out = run_gpu_tests_on_host(emulated_library, [FILE, "-k", "split or files or broken or verifier or refused or security"])
    assert "8 passed" in out, out[-500:]                     # 2 + 2 + the forged blowups + log_blowup 0 and 5 + the security rule


def test_verifier_and_prover_rules_need_no_device():
    """log_blowup 0 and 5: check_log_blowup (what Prover.prove asks first) and the verifier name the option; 1 .. 4 pass the rule; the
    security rule counts log_blowup bits per query; the verifier's tables do not depend on the blowup"""
    import numpy as np
    from sandstorm_amd import goldilocks as gs
    from sandstorm_amd.layouts import plain as pl
    for lb in (1, 2, 3, 4, np.int64(2)):
        gs.check_log_blowup(lb)
    for lb in (0, 5, -1, True, 2.0, None):
        with pytest.raises(ValueError, match="log_blowup refused"):
            gs.check_log_blowup(lb)
    assert gs.conjectured_security_bits(gs.Options(num_queries=32, log_blowup=2), 1 << 24) == 80
    assert gs.conjectured_security_bits(gs.Options(num_queries=31, log_blowup=2), 1 << 24) == 78
    assert gs.conjectured_security_bits(gs.Options(num_queries=22, log_blowup=3), 1 << 24) == 82
    assert gs.conjectured_security_bits(gs.Options(num_queries=16, log_blowup=4), 1 << 24) == 80
    with np.load(os.path.join(ROOT, "tests", "golden", "goldilocks_plain_proof.npz")) as f:
        proof = gs.proof_from_arrays({k: f[k] for k in f.files})
    prog = pl.example_program(10)
    states, memory = pl.run(prog, 64)
    pi = pl.public_input_of(prog, states, memory)
    for lb in (0, 5):
        forged = dataclasses.replace(proof, options=dataclasses.replace(proof.options, log_blowup=lb))
        with pytest.raises(gs.VerificationError, match="log_blowup"):
            gs.verify(forged, gs.plain_air(), bytes(range(32)), statement=pi, required_security_bits=8)
    for lb in (2, 3, 4):                                      # no longer "written for blowup 2": refused as another proof's transcript
        forged = dataclasses.replace(proof, options=dataclasses.replace(proof.options, log_blowup=lb))
        with pytest.raises(gs.VerificationError) as e:
            gs.verify(forged, gs.plain_air(), bytes(range(32)), statement=pi, required_security_bits=8)
        assert "written for" not in str(e.value)
    z = (3, 5, 8)
    t1, t4 = pl.Tables(1024, 1), pl.Tables(1024, 4)
    gs.plain_air().composition(1024, [(11, 22, 33), (5, 6, 7), (9, 8, 7)], (1, 2, 3), t1, pi)
    gs.plain_air().composition(1024, [(11, 22, 33), (5, 6, 7), (9, 8, 7)], (1, 2, 3), t4, pi)
    assert t1.specs == t4.specs and all(t1.value_at(s, z) == t4.value_at(s, z) for s in t1.specs)


def test_subsampling_kernel_under_the_sanitizers(tmp_path):
    """tests/cpp/subsample_rows_gl64_host_test.cpp: a program of its own - csrc/goldilocks.hip's host build, the emulated runtime and a
    main that drives the kernel over the shapes above with heap blocks of exactly the documented sizes - built with
    -fsanitize=address,undefined.  (Leak checking is off: the emulated runtime keeps its lanes' stacks for the next launch.)"""
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no clang++ to build the host emulation with (%s)" % CLANG)
    exe = str(tmp_path / "subsample_rows_gl64_host_test")
    emu = os.path.join(ROOT, "tests", "hipemu")
    subprocess.check_call([CLANG, "-x", "c++", "-std=c++17", "-O1", "-g1", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", emu, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "sandstorm_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "subsample_rows_gl64_host_test.cpp"), os.path.join(ROOT, "sandstorm_amd", "csrc", "goldilocks.hip"),
                           os.path.join(emu, "hipemu.cpp"), "-pthread", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert out.returncode == 0 and "160 launches, 0 mismatches" in out.stdout, out.stdout[-1000:] + out.stderr[-3000:]
