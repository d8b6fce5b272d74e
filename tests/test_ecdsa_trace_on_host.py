"""tests/test_gpu_ecdsa_trace.py - real ECDSA builtin instances traced by the DEVICE CODE from their inputs - in the CPU suite: on the
host build of sandstorm_amd/csrc/*.hip (tests/hipemu/, as tests/test_ec_op_trace_on_host.py runs the EC-op tests), with the lanes of a
workgroup scheduled in a different order every pass - the kernel's phases hand values from one lane to the others through LDS and the
instance's own cells, and the key's second root runs over the cells of the first, so a missing barrier shows.  The entry point alone
against the host generator and the Python mirror, its refusals, skips and findings, a whole saturated generation with the upload
statistics, the switch and the reference's bootloader run; the whole proof is hardware only.  TEST INFRASTRUCTURE: nothing under
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


def test_ecdsa_instances_traced_by_the_device_code(emulated_library):
    env = dict(os.environ, SS_TEST_HIPEMU="1", SS_TEST_HIPEMU_LIB=emulated_library, HIPEMU_ORDER="shuffle")
    out = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "tests/test_gpu_ecdsa_trace.py"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=2400)
    tail = out.stdout[-3000:] + out.stderr[-2000:]
    assert out.returncode == 0, tail
    # the entry point, its refusals, the saturated generation, the switch with the bootloader run; the proof: hardware
    assert "4 passed, 1 skipped" in out.stdout, tail
