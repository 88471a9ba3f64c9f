"""ASan/UBSan build of the tree set's host side (prysm_amd/csrc/tree_set_plan.cpp,
plain C++): the pending changes of every tree and the plan of a flush, built
host-only with -fsanitize=address,undefined and fuzzed against a naive model
by the stand-alone tests/c_abi/tree_set_plan_fuzz.cpp (nothing sanitized is
loaded into Python)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fuzz") / "tree_set_plan_fuzz")
    csrc = os.path.join(ROOT, "prysm_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I" + csrc,
                    os.path.join(ROOT, "tests", "c_abi", "tree_set_plan_fuzz.cpp"),
                    os.path.join(csrc, "tree_set_plan.cpp"), "-o", out], check=True)
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_tree_set_plan_fuzz_sanitized(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_exe, str(seed), "400"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "cases clean" in r.stderr
    m = re.search(r"(\d+) flushes, (\d+) climbs, (\d+) rebuilds, (\d+) grows", r.stderr)
    assert m and all(int(x) > 0 for x in m.groups()), r.stderr[-300:]  # every decision was reached


def test_plan_source_has_no_hip():
    """The plan is a function of the pending changes alone: no device call in its translation unit."""
    for name in ("tree_set_plan.cpp", "tree_set_plan.hpp"):
        with open(os.path.join(ROOT, "prysm_amd", "csrc", name)) as f:
            src = f.read()
        assert "#include <hip" not in src and "runtime.hpp" not in src, name
