"""tests/test_gpu_builtin_trace.py - real bitwise and Poseidon builtin instances traced by the DEVICE CODE from their inputs - in the CPU
suite: on the host build of sandstorm_amd/csrc/*.hip (tests/hipemu/, as tests/test_pedersen_trace_on_host.py runs the Pedersen tests),
with the lanes of a workgroup scheduled in a different order every pass.  The entry points alone (bitwise for both layouts' placements
and all three masks, Poseidon against the Python mirror too), their refusals and skips, whole saturated generations with the upload
statistics, the reference's bootloader run, the generators' refusals; the whole proof and the 2^20-step statements are hardware only.
TEST INFRASTRUCTURE: nothing under sandstorm_amd/ can load the emulation."""
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


def test_bitwise_and_poseidon_instances_traced_by_the_device_code(emulated_library):
    env = dict(os.environ, SS_TEST_HIPEMU="1", SS_TEST_HIPEMU_LIB=emulated_library, HIPEMU_ORDER="shuffle")
    out = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_builtin_trace.py"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=2400)
    tail = out.stdout[-3000:] + out.stderr[-2000:]
    assert out.returncode == 0, tail
    # bitwise entry point x 2 layouts, Poseidon entry point, their refusals, saturated x 2, bootloader, refusals; proof + 2^20 x 2: hardware
    assert "8 passed, 3 skipped" in out.stdout, tail
