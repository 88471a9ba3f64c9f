"""ASan/UBSan build of the undo journal's slot map (prysm_amd/csrc/tree_journal.hpp,
what k_trees_journal, k_trees_restore and mk_dev_ssz_trees_journal place a
piece by): built host-only with -fsanitize=address,undefined and checked by the
stand-alone tests/c_abi/tree_journal_fuzz.cpp -- every slot inside the reported
size, no two pieces on one byte, every ancestor the old tree has saved, against
a naive walk (nothing sanitized is loaded into Python)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prysm_amd", "csrc")


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fuzz") / "tree_journal_fuzz")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "c_abi", "tree_journal_fuzz.cpp"), "-o", out], check=True)
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_tree_journal_fuzz_sanitized(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_exe, str(seed), "3000"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    m = re.search(r"(\d+) cases clean, (\d+) pieces, (\d+) ancestors", r.stderr)
    assert m and int(m.group(1)) == 3000 and int(m.group(2)) > 100000 and int(m.group(3)) > 10000, r.stderr[-300:]


def test_slot_map_has_no_hip_and_is_the_kernels():
    """One slot map for the kernels, the host side and the fuzz: the header includes no HIP, the kernel file
    and the device entries include the header."""
    with open(os.path.join(CSRC, "tree_journal.hpp")) as f:
        src = f.read()
    assert "#include <hip" not in src and "runtime.hpp" not in src
    with open(os.path.join(CSRC, "kernels_tree.hip")) as f:
        kern = f.read()
    assert '#include "tree_journal.hpp"' in kern
    body = kern[kern.index("void journal_run("):]
    assert "journal_piece(" in body and "journal_value(" in body and "journal_node_off(" in body
    assert "void k_trees_journal(" in body and "void k_trees_restore(" in body
    with open(os.path.join(CSRC, "tree_journal_api.cpp")) as f:
        host = f.read()
    assert '#include "tree_journal.hpp"' in host and "journal_tree_bytes(" in host and "journal_pieces(" in host
