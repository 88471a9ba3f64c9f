"""Compiled resource figures of the library's kernels: VGPRs, SGPRs, scratch
(private segment) and static LDS per kernel, read from the code object's
metadata note.

    python tools/kernel_resources.py [--match SUBSTR] [--compare profiles/kernel_split/resources.json] [--out FILE]
    python tools/kernel_resources.py --text-sha256 [--lib prysm_amd/lib/merkle_kernels.o]

Unbundles the gfx950 code object from prysm_amd/lib/libprysm_merkle.so with
clang-offload-bundler and parses `llvm-readelf --notes`.  --compare checks
every kernel that both sides name (after --match) for equal figures and exits
1 when one differs.  --text-sha256 prints one line, the sha256 of the code
object's .text: a move of kernel source that is a pure cut leaves it as it was
(profiles/kernel_split/text_identity.json)."""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
KEYS = {".vgpr_count": "vgpr_count", ".sgpr_count": "sgpr_count", ".private_segment_fixed_size": "private_segment_fixed_size",
        ".group_segment_fixed_size": "group_segment_fixed_size"}


def code_object(lib, tmp):
    """The gfx950 code object of a library or an object file, unbundled into the directory tmp."""
    co, fat = os.path.join(tmp, "gfx950.co"), os.path.join(tmp, "lib.hipfb")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat],
                   check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
    return co


def text_sha256(lib):
    with tempfile.TemporaryDirectory() as tmp:
        text = os.path.join(tmp, "text.bin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.text",
                        code_object(lib, tmp), text], check=True)
        with open(text, "rb") as f:
            return hashlib.sha256(f.read()).hexdigest()


def kernel_resources(lib):
    with tempfile.TemporaryDirectory() as tmp:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", code_object(lib, tmp)], check=True,
                               capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2).strip().strip("'\"")
        if key == ".args":  # a new kernel's block begins with its argument list
            cur = {}
        elif key == ".name" and cur is not None and re.match(r"^\s{4}\.name", line):
            out[val] = cur  # the keys after .name (they are sorted) still go into this dict
        elif key in KEYS and cur is not None:
            cur[KEYS[key]] = int(val)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "prysm_amd", "lib", "libprysm_merkle.so"))
    ap.add_argument("--match", default="")
    ap.add_argument("--compare")
    ap.add_argument("--out")
    ap.add_argument("--text-sha256", action="store_true")
    a = ap.parse_args()
    if a.text_sha256:
        print(text_sha256(a.lib))
        return
    res = {k: v for k, v in kernel_resources(a.lib).items() if a.match in k}
    rows = [dict(name=k, **v) for k, v in sorted(res.items())]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
    bad = 0
    if a.compare:
        with open(a.compare) as f:
            old = json.load(f)
        old = old["kernels"] if isinstance(old, dict) else old
        for o in old:
            if o["name"] not in res:
                continue
            new = res[o["name"]]
            same = all(new.get(k) == o[k] for k in KEYS.values() if k in o)
            bad += not same
            print(("same     " if same else "DIFFERENT"), o["name"], {k: new.get(k) for k in KEYS.values()})
    else:
        for r in rows:
            print(json.dumps(r))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
