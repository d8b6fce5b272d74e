"""The parser of the 64-bit field's check callback blob (sandstorm_amd/host/gl_check_blob.hpp) as a program of its own under the host
sanitizers: tests/cpp/gl_check_blob_test.cpp feeds it a good blob, every truncation of it and a list of inconsistent ones; each must
be refused by message, and none may be read past its end."""
import os
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_device_code_on_host import CLANG  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_blob_parser_under_the_sanitizers(tmp_path):
    if not (os.path.exists(CLANG) or shutil.which(CLANG)):
        pytest.skip("no clang++ to build the program with (%s)" % CLANG)
    exe = str(tmp_path / "gl_check_blob_test")
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "sandstorm_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "gl_check_blob_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "prefixes refused, 0 failures" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
