"""No GPU: files -> proof over several ranks (host_capi.cpp ssh_prove_files_sharded_device) on the host build of the device code -
tests/test_gpu_sharded_files.py's thread-rank cases in a process of their own (tests/test_device_code_on_host.py has the plumbing):
ownership arithmetic, the auxiliary blocks' offsets, the order the columns are released in and the failure paths, checked on the CPU.
The reference's own 2^17-step proof is left to the MI355X (2^21 rows are too slow emulated)."""
import os

from tests.test_device_code_on_host import emulated_library, heavy, run_gpu_tests_on_host  # noqa: F401 - emulated_library is a fixture


def run(lib, selection):
    os.environ["HIPEMU_THREADS"] = "1"           # the emulator's worker pool serves one launching thread: the ranks are the parallelism
    try:
        return run_gpu_tests_on_host(lib, ["tests/test_gpu_sharded_files.py", "-k", selection], timeout=2400)
    finally:
        del os.environ["HIPEMU_THREADS"]


def test_recursive_example_from_its_files_on_two_and_eight_ranks(emulated_library):  # noqa: F811
    """the committed proof's bytes; 2 ranks: the seventh base column is spread; 8 ranks: a rank without a base column"""
    heavy()
    out = run(emulated_library, "test_recursive_example_from_its_files and (2 or 8)")
    assert "2 passed" in out, out[-500:]


def test_real_instances_and_refused_files_on_two_ranks(emulated_library):  # noqa: F811
    """real Pedersen / bitwise / range-check instances against the single-context call, traced on the device code on both ranks; files
    the host checks refuse and files only the device code's status bits refuse, on both ranks, nobody left waiting"""
    heavy()
    out = run(emulated_library, "(test_real_builtin_instances and 2) or test_refused_files")
    assert "2 passed" in out, out[-500:]
