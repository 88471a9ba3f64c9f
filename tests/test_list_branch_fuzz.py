"""ASan/UBSan build of the list-tree proof arithmetic (prysm_amd/csrc/list_branch.hpp,
what k_list_tree_branches and k_verify_list_branches index with): built
host-only with -fsanitize=address,undefined and checked against a naive model
of every level's count by the stand-alone tests/c_abi/list_branch_fuzz.cpp
(nothing sanitized is loaded into Python)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prysm_amd", "csrc")


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fuzz") / "list_branch_fuzz")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "c_abi", "list_branch_fuzz.cpp"), "-o", out], check=True)
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_list_branch_fuzz_sanitized(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_exe, str(seed), "1500"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    m = re.search(r"(\d+) cases clean, (\d+) node indices, (\d+) gathers replayed", r.stderr)
    assert m and int(m.group(1)) > 20000 and int(m.group(2)) > 50000 and int(m.group(3)) > 10000, r.stderr[-300:]


def test_arithmetic_has_no_hip_and_is_the_kernels():
    """One header for the kernels, the host side and the fuzz: it includes no HIP, and both kernels use it."""
    with open(os.path.join(CSRC, "list_branch.hpp")) as f:
        src = f.read()
    assert "#include <hip" not in src and "runtime.hpp" not in src
    with open(os.path.join(CSRC, "kernels_tree.hip")) as f:
        kern = f.read()
    assert '#include "list_branch.hpp"' in kern
    gather = kern[kern.index("void k_list_tree_branches("):]
    assert "branch_window(" in gather and "branch_sibling(" in gather
    verify = kern[kern.index("void k_verify_list_branches("):]
    assert "branch_window(" in verify and "branch_level_count(" in verify
