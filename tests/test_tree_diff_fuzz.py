"""ASan/UBSan build of the rule of two resident trees' diff
(prysm_amd/csrc/tree_diff.hpp, what k_trees_diff and mk_dev_ssz_trees_diff walk
by): built host-only with -fsanitize=address,undefined and
replayed on exact-size buffers of a naive model of both trees by the
stand-alone tests/c_abi/tree_diff_fuzz.cpp (nothing sanitized is loaded into
Python)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prysm_amd", "csrc")


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fuzz") / "tree_diff_fuzz")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "c_abi", "tree_diff_fuzz.cpp"), "-o", out], check=True)
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_tree_diff_fuzz_sanitized(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_exe, str(seed), "600"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    m = re.search(r"(\d+) cases clean, (\d+) nodes read, (\d+) work items, (\d+) wide checks, (\d+) collisions met",
                  r.stderr)
    assert m, r.stderr[-300:]
    cases, reads, items, wide, collisions = (int(x) for x in m.groups())
    assert cases == 602 and reads > 20000 and items > 2000 and wide > 20000 and collisions >= 2, r.stderr[-300:]


def test_arithmetic_has_no_hip_and_is_the_kernels():
    """One header for the kernel, the host side and the fuzz: it includes no HIP, and all of them use it."""
    with open(os.path.join(CSRC, "tree_diff.hpp")) as f:
        src = f.read()
    assert "#include <hip" not in src and "runtime.hpp" not in src
    with open(os.path.join(CSRC, "kernels_tree.hip")) as f:
        kern = f.read()
    assert '#include "tree_diff.hpp"' in kern
    diff = kern[kern.index("void k_trees_diff("):]
    diff = diff[:diff.index("\n}\n")]
    for fn in ("diff_shape(", "diff_items(", "diff_comparable(", "diff_visited(", "diff_node_a(", "diff_node_b("):
        assert fn in diff, fn
    with open(os.path.join(CSRC, "tree_diff_api.cpp")) as f:
        host = f.read()
    assert '#include "tree_diff.hpp"' in host and "diff_items(" in host and "diff_shape(" in host
    with open(os.path.join(ROOT, "tests", "c_abi", "tree_diff_fuzz.cpp")) as f:
        fuzz = f.read()
    assert '#include "tree_diff.hpp"' in fuzz and "diff_walk(" in fuzz
