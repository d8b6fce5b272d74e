"""tests/test_gpu_gl64_constraint_check.py on the CPU: the checking instantiation of the Fq3 interpreter (csrc/goldilocks.hip) compiled for
the host over tests/hipemu, where __shfl_xor is a workgroup barrier - a lane that skipped a CHECK's reduction (the ragged wave at
n = 2^4, the partial workgroup at 2^7) would hang or misreport here.  The kernel-level cases below the two-sweep size, the refusals,
and the plain layout's example run at n = 256 with its corrupted cells; the larger runs and the provers need the hardware."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_device_code_on_host import emulated_library, run_gpu_tests_on_host  # noqa: E402,F401


def test_kernel_level_cases(emulated_library):
    out = run_gpu_tests_on_host(emulated_library, ["tests/test_gpu_gl64_constraint_check.py", "-k", "kernel and not two_sweeps"])
    assert "4 passed" in out, out[-500:]                      # 2^4, 2^7, 2^10 and the refusals


def test_plain_layout_at_256_rows(emulated_library):
    out = run_gpu_tests_on_host(emulated_library, ["tests/test_gpu_gl64_constraint_check.py", "-k", "plain and example_16"])
    assert "13 passed" in out, out[-500:]                     # the clean example run + twelve corrupted cells
