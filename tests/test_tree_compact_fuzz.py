"""ASan/UBSan build of the stable-erase index map (prysm_amd/csrc/tree_compact.hpp,
the function k_tree_compact runs per destination): built host-only with
-fsanitize=address,undefined and checked against a naive filtered copy by the
stand-alone tests/c_abi/tree_compact_fuzz.cpp (nothing sanitized is loaded
into Python)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prysm_amd", "csrc")


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fuzz") / "tree_compact_fuzz")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "c_abi", "tree_compact_fuzz.cpp"), "-o", out], check=True)
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_tree_compact_fuzz_sanitized(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_exe, str(seed), "400"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    m = re.search(r"(\d+) cases clean, (\d+) block destinations", r.stderr)
    assert m and int(m.group(1)) > 300 * 300 and int(m.group(2)) > 0, r.stderr[-300:]


def test_index_map_has_no_hip_and_is_the_kernels():
    """One function for the kernel and the fuzz: the header includes no HIP, the kernel file includes the header."""
    with open(os.path.join(CSRC, "tree_compact.hpp")) as f:
        src = f.read()
    assert "#include <hip" not in src and "runtime.hpp" not in src
    with open(os.path.join(CSRC, "kernels_tree.hip")) as f:
        kern = f.read()
    assert '#include "tree_compact.hpp"' in kern
    body = kern[kern.index("void k_tree_compact("):]
    assert "compact_skip_in(" in body and "compact_skip(" in body
