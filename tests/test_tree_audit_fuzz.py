"""ASan/UBSan build of the work-item map of a resident tree's audit
(prysm_amd/csrc/tree_audit.hpp, what k_trees_audit and mk_dev_ssz_trees_audit
number a tree's checks with): built host-only with
-fsanitize=address,undefined and replayed into exact-size buffers of a naive
model of the layout rule by the stand-alone tests/c_abi/tree_audit_fuzz.cpp
(nothing sanitized is loaded into Python)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prysm_amd", "csrc")


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fuzz") / "tree_audit_fuzz")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "c_abi", "tree_audit_fuzz.cpp"), "-o", out], check=True)
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_tree_audit_fuzz_sanitized(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_exe, str(seed), "600"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    m = re.search(r"(\d+) cases clean, (\d+) items replayed, (\d+) level offsets compared", r.stderr)
    assert m and int(m.group(1)) > 2500 and int(m.group(2)) > 100000 and int(m.group(3)) > 50000, r.stderr[-300:]


def test_arithmetic_has_no_hip_and_is_the_kernels():
    """One header for the kernel, the host side and the fuzz: it includes no HIP, restates neither the
    counts nor the offsets, and all of them use it."""
    with open(os.path.join(CSRC, "tree_audit.hpp")) as f:
        src = f.read()
    assert "#include <hip" not in src and "runtime.hpp" not in src
    assert '#include "list_branch.hpp"' in src and '#include "tree_copy.hpp"' in src
    for fn in ("branch_shape(", "branch_window(", "branch_window_padded(", "branch_level_count(", "copy_level_off("):
        assert fn in src, fn
    with open(os.path.join(CSRC, "kernels_tree.hip")) as f:
        kern = f.read()
    assert '#include "tree_audit.hpp"' in kern
    audit = kern[kern.index("void k_trees_audit("):]
    audit = audit[:audit.index("\n}\n")]
    for fn in ("audit_shape(", "audit_slot_first(", "audit_slot_child(", "audit_slot_node(", "audit_item_in("):
        assert fn in audit, fn
    assert "g_arrive" not in audit
    assert "g_arrive" not in kern  # the arrival counters stay with the fused tops (kernels_top.hip)
    with open(os.path.join(CSRC, "tree_audit_api.cpp")) as f:
        host = f.read()
    assert '#include "tree_audit.hpp"' in host and "audit_items(" in host and "audit_shape(" in host
