"""ASan/UBSan build of the struct layout parser (prysm_amd/csrc/struct_spec.cpp,
plain C++) fuzzed by tests/c_abi/struct_list_spec_fuzz.cpp with layouts that
hold MK_FIELD_LIST entries.  The parser must refuse an array or produce a
program whose replay reads only inside the record, writes only inside the
thread's LDS column and keeps each list's node stack inside its budget."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fuzz") / "struct_list_spec_fuzz")
    csrc = os.path.join(ROOT, "prysm_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Werror", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "struct_list_spec_fuzz.cpp"),
                    os.path.join(csrc, "struct_spec.cpp"), os.path.join(csrc, "planner.cpp"), "-o", out], check=True)
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_struct_list_spec_fuzz_sanitized(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_exe, str(seed), "6000"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    m = re.search(r"(\d+) cases clean: (\d+) accepted with a list, (\d+) refused, (\d+) with a stored count", r.stderr)
    assert m, r.stderr[-300:]
    cases, accepted, refused, counts_bad = map(int, m.groups())
    assert cases == 6000 and accepted > 500 and refused > 500 and counts_bad > 50
