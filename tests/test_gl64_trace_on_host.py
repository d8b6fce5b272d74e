"""tests/test_gpu_gl64_device_trace.py - the plain layout's base trace over the 64-bit field made by the DEVICE CODE from the raw files -
in the CPU suite: on the host build of sandstorm_amd/csrc/*.hip (tests/hipemu/, as tests/test_ecdsa_trace_on_host.py runs the ECDSA
tests), with the lanes of a workgroup scheduled in a different order every pass - the CPU kernel hands every cycle's values from the
lane that computed them to the sixteen lanes that write its rows through LDS, and the ordered memory counts through an LDS table, so a
missing barrier shows.  Every test of the file runs here: the example and the busy run cell for cell, each kernel alone, the
refusals, the proof from the files (both hashes) and the upload accounting; none is hardware only.  TEST INFRASTRUCTURE: nothing under
sandstorm_amd/ can load the emulation."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")


@pytest.fixture(scope="module")
def emulated_library():
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no clang++ to build the host emulation with (%s)" % CLANG)
    out = subprocess.run(["bash", os.path.join(ROOT, "tests", "hipemu", "build.sh")], capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.strip().splitlines()[-1]


def test_plain_base_trace_made_by_the_device_code(emulated_library):
    env = dict(os.environ, SS_TEST_HIPEMU="1", SS_TEST_HIPEMU_LIB=emulated_library, HIPEMU_ORDER="shuffle")
    out = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_gl64_device_trace.py"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=2400)
    tail = out.stdout[-3000:] + out.stderr[-2000:]
    assert out.returncode == 0, tail
    # 4 example sizes, 2 busy sizes, 6 kernels alone (3 rc-pool cases), 8 refusals, the permutations, 2 proofs, the upload accounting
    assert "24 passed" in out.stdout and "skipped" not in out.stdout, tail
