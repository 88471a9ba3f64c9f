"""ASan/UBSan build of the piece map of a resident tree's copy
(prysm_amd/csrc/tree_copy.hpp, what k_trees_copy and mk_dev_ssz_trees_copy cut a
tree into): built host-only with -fsanitize=address,undefined
and replayed into exact-size buffers of a naive model of the layout rule by the
stand-alone tests/c_abi/tree_copy_fuzz.cpp (nothing sanitized is loaded into
Python)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prysm_amd", "csrc")


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fuzz") / "tree_copy_fuzz")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "c_abi", "tree_copy_fuzz.cpp"), "-o", out], check=True)
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_tree_copy_fuzz_sanitized(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_exe, str(seed), "600"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    m = re.search(r"(\d+) cases clean, (\d+) pieces replayed, (\d+) level offsets compared", r.stderr)
    assert m and int(m.group(1)) > 4000 and int(m.group(2)) > 1000000 and int(m.group(3)) > 50000, r.stderr[-300:]


def test_arithmetic_has_no_hip_and_is_the_kernels():
    """One header for the kernel, the host side and the fuzz: it includes no HIP, and all of them use it."""
    with open(os.path.join(CSRC, "tree_copy.hpp")) as f:
        src = f.read()
    assert "#include <hip" not in src and "runtime.hpp" not in src
    with open(os.path.join(CSRC, "kernels_tree.hip")) as f:
        kern = f.read()
    assert '#include "tree_copy.hpp"' in kern
    copy = kern[kern.index("void k_trees_copy("):]
    copy = copy[:copy.index("\n}\n")]
    for fn in ("copy_shape(", "copy_seg_first(", "copy_seg_offs(", "copy_piece_in("):
        assert fn in copy, fn
    with open(os.path.join(CSRC, "tree_copy_api.cpp")) as f:
        host = f.read()
    assert '#include "tree_copy.hpp"' in host and "copy_pieces(" in host and "copy_level_off(" in host
