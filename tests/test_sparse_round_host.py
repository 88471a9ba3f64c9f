"""The sparse round 0 of prysm_amd/csrc/keccak_sparse.hpp on the host: the
header's own instruction sequence over a plain C++ ops policy
(tests/c_abi/sparse_round_host.cpp), built with ASan/UBSan, against a
textbook Keccak-f round on the zero-extended input: 10^4 random fills of the
live lanes per seed, the 64-B node form and the 17-lane first-block form.
The lanes the sparse forms must not read are poisoned.  The device policy's
asm wrappers are not compiled here; the GPU root tests cover them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sparse") / "sparse_round_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "prysm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_abi", "sparse_round_host.cpp"), "-o", out], check=True)
    return out


@pytest.mark.parametrize("seed", [1, 0x5EED])
def test_sparse_round0_matches_full_round(exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(seed), "10000"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "10000 cases clean" in r.stderr
