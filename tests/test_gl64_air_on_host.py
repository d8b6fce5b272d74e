"""tests/test_gpu_gl64_air.py on the host build of the device code (tests/test_device_code_on_host.py): the 64-bit field's claim proved
through the plain AIR the C++ host lowers itself, every kernel executed lane by lane on the CPU - the runs of 16 and 128 cycles; the
1024-cycle run is the card's."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_device_code_on_host import emulated_library, run_gpu_tests_on_host  # noqa: E402,F401  (emulated_library: a fixture)

FILE = "tests/test_gpu_gl64_air.py"


def test_same_proof_as_the_python_lowering(emulated_library):  # noqa: F811
    """files -> proof and resident columns -> proof with no callback, against goldilocks.prove_files and goldilocks.Prover: blowups 2 and 4,
    folds 2 and 8, both hashes, validation off and on; both verifiers accept"""
    out = run_gpu_tests_on_host(emulated_library, [FILE, "-k", "same_proof"])
    assert "12 passed" in out, out[-500:]                    # 3 runs x 4 cases


def test_same_check_report_and_validation_messages(emulated_library):  # noqa: F811
    out = run_gpu_tests_on_host(emulated_library, [FILE, "-k", "check_report or validating"])
    assert "11 passed" in out, out[-500:]                    # 2 runs x (clean + 4 broken cells) + the validating prove calls


def test_same_refusals_and_handle_hygiene(emulated_library):  # noqa: F811
    out = run_gpu_tests_on_host(emulated_library, [FILE, "-k", "refused or handle"])
    assert "12 passed" in out, out[-500:]                    # 3 refused files + the open permutation + 5 option sets + 3 of the handle
