"""ASan/UBSan build of the rules of the deposit trie's roll back, fork point,
audit and copy (prysm_amd/csrc/trie_admin.hpp, what the kernels of
kernels_trie_admin.hip and trie_admin_api.cpp go by): built
host-only with -fsanitize=address,undefined and replayed on exact-size heap
arrays against a naive model by the stand-alone tests/c_abi/trie_admin_fuzz.cpp
(nothing sanitized is loaded into Python).  Dead nodes hold poison and a read
of one aborts the run."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prysm_amd", "csrc")


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fuzz") / "trie_admin_fuzz")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I" + CSRC,
                    os.path.join(ROOT, "tests", "c_abi", "trie_admin_fuzz.cpp"), "-o", out], check=True)
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_trie_admin_fuzz_sanitized(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_exe, str(seed), "800"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    m = re.search(r"(\d+) cases clean, (\d+) roll backs, (\d+) nodes read, (\d+) hashes", r.stderr)
    assert m, r.stderr[-300:]
    cases, rollbacks, reads, hashes = (int(x) for x in m.groups())
    assert cases == 800 and rollbacks > 100 and reads > 20000 and hashes > 20000, r.stderr[-300:]


def test_rules_have_no_hip_and_are_the_kernels():
    """One header for the kernels, the host side and the fuzz: it includes no HIP, and all of them use it."""
    with open(os.path.join(CSRC, "trie_admin.hpp")) as f:
        src = f.read()
    assert "#include <hip" not in src and "runtime.hpp" not in src and "merkle_kernels" not in src
    with open(os.path.join(CSRC, "kernels_trie_admin.hip")) as f:
        kern = f.read()
    assert '#include "trie_admin.hpp"' in kern and "MK_KERNEL_UNIT" in kern
    for fn in ("ta_chain_first(", "ta_path_right(", "ta_fork_has(", "ta_fork_sub(", "ta_audit_first(",
               "ta_audit_right(", "ta_copy_first("):
        assert fn in kern, fn
    with open(os.path.join(CSRC, "trie_admin_api.cpp")) as f:
        host = f.read()
    assert '#include "trie_admin.hpp"' in host and "ta_audit_items(" in host and "ta_copy_first(" in host
    with open(os.path.join(CSRC, "merkle_kernels.hip")) as f:
        unit = f.read()
    assert '#include "kernels_trie_admin.hip"' in unit
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    parts = re.search(r"^KERNEL_PARTS := (.*)$", mk, re.M).group(1).split()
    objs = re.search(r"^OBJS := (.*)$", mk, re.M).group(1)
    assert "kernels_trie_admin.hip" in parts and "kernels_trie_admin" not in objs
    with open(os.path.join(ROOT, "tests", "c_abi", "trie_admin_fuzz.cpp")) as f:
        fuzz = f.read()
    assert '#include "trie_admin.hpp"' in fuzz
    for fn in ("ta_truncate(", "ta_fork_point(", "ta_audit(", "ta_copy_first("):
        assert fn in fuzz, fn


def test_every_kernel_file_is_a_part_of_the_one_unit():
    """The kernel files and the Makefile agree: what merkle_kernels.hip includes is KERNEL_PARTS, in the same
    order, every kernels_*.hip on disk is among them, none is an object of its own, and each refuses to compile
    outside the unit."""
    with open(os.path.join(CSRC, "merkle_kernels.hip")) as f:
        unit = f.read()
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    parts = re.search(r"^KERNEL_PARTS := (.*)$", mk, re.M).group(1).split()
    objs = re.search(r"^OBJS := (.*)$", mk, re.M).group(1)
    included = re.findall(r'^#include "(kernels_\w+\.hip)"$', unit, re.M)
    assert len(set(parts)) == len(parts)
    assert included == parts
    assert sorted(parts) == sorted(f for f in os.listdir(CSRC) if f.endswith(".hip") and f != "merkle_kernels.hip")
    assert unit.index("#define MK_KERNEL_UNIT 1") < unit.index("#include ")  # ahead of the first include
    for part in parts:
        assert part[:-4] not in objs, part
        with open(os.path.join(CSRC, part)) as f:
            src = f.read()
        guard = '#ifndef MK_KERNEL_UNIT\n#error "%s is built through merkle_kernels.hip"\n#endif\n' % part
        assert guard in src and "__global__" not in src[:src.index(guard)], part
        assert "#define MK_KERNEL_UNIT" not in src, part
    assert "g_arrive" not in unit  # the arrival counters stay in the one file that defines them
    for part in parts:
        with open(os.path.join(CSRC, part)) as f:
            assert ("g_arrive" in f.read()) == (part == "kernels_top.hip"), part
