#!/usr/bin/env python3
"""The resident deposit trie rolled back, audited, compared and cloned on the
device, each beside the only way to the same answer without
it, on a trie of 2^20 deposits of 280 bytes at depth 32.

  python tools/trie_admin_probe.py [--out profiles/trie_admin/probe.json] [--quick]

  rollback    mk_dev_deposit_trie_truncate to count - 1 (the longest chain), to
              2^19 and to count, against mk_deposit_trie_build of the surviving
              deposits from host data (upload + build + synchronise) and against
              the device build alone (mk_dev_deposit_trie_append from count 0)
  audit       mk_dev_deposit_trie_audit against mk_dev_deposit_trie_levels(0 ->
              depth) into a scratch array plus a flat device compare of the two
  fork_point  mk_dev_deposit_trie_fork_point of two tries that part at one leaf,
              against a flat device compare of the two level-0 arrays and
              against the read-back of both
  clone       mk_deposit_trie_clone of a handle against mk_deposit_trie_build
              from host data
Device forms are timed with device events on the call's stream, calls that
upload or synchronise themselves with host wall time.  One process, warm,
`rounds` interleaved rounds after one that is dropped; `ms` is the median,
`ms_min` / `ms_max` the spread.  The clocks are not pinned.  Every result is
checked (the roots against the build's, the fork point against where the tries
were made to part).  Prints one JSON line and writes it to --out.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x5EED000000000000 + 0x7A0B
DEP, DEPTH = 280, 32


def stat(xs):
    return {"ms": round(statistics.median(xs), 4), "ms_min": round(min(xs), 4), "ms_max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trie_admin", "probe.json"))
    ap.add_argument("--quick", action="store_true", help="a small trie (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D
    from prysm_amd.hashutil import _ptr

    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise SystemExit("trie_admin_probe needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    n = 1 << (12 if args.quick else 20)
    rounds = args.rounds

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    mk = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)  # noqa: E731
    data = mk(n * DEP)
    D.synth_fill(data, SEED)
    other = mk(n * DEP)
    D.synth_fill(other, SEED + 1)
    host = data.cpu().numpy()
    offs = np.arange(n + 1, dtype=np.uint64) * DEP
    cap = n
    lvb = D.deposit_trie_levels_bytes(cap, DEPTH)
    lv, root = mk(lvb), mk(32)
    D.deposit_trie_append(lv, cap, 0, data, n, DEP, DEPTH, root)
    torch.cuda.synchronize()
    full_root = root.clone()
    scratch, sroot, wroot = mk(lvb), mk(32), mk(32)

    def host_build(c):
        out = ctypes.create_string_buffer(32)
        _lib.invoke("mk_deposit_trie_build", _ptr(host), _ptr(offs), c, DEPTH, None, out)
        return out.raw

    out = {"probe": "trie_admin", "deposits": n, "deposit_len": DEP, "depth": DEPTH, "rounds": rounds,
           "quick": bool(args.quick)}

    # ---- roll back, each time of a fresh copy of the full trie (the copy is not timed)
    cases = {"to_count_minus_1": n - 1, "to_half": n // 2, "to_count": n}
    t = {k: {"truncate": [], "host_build": [], "device_build": []} for k in cases}
    work = mk(lvb)
    for r in range(rounds + 1):
        for k, c in cases.items():
            work.copy_(lv)
            t[k]["truncate"].append(events(lambda: D.deposit_trie_truncate(work, cap, n, c, DEPTH, wroot)))
            ms, want = wall(lambda: host_build(c))
            t[k]["host_build"].append(ms)
            assert wroot.cpu().numpy().tobytes() == want, k
            t[k]["device_build"].append(
                events(lambda: D.deposit_trie_append(scratch, cap, 0, data, c, DEP, DEPTH, sroot)))
            assert torch.equal(sroot, wroot), k
    out["rollback"] = {k: dict(new_count=cases[k], **{w: stat(v[1:]) for w, v in t[k].items()}) for k in cases}
    del work

    # ---- audit against levels 1 .. depth built again from level 0 and compared
    scratch[:32 * n] = lv[:32 * n]
    ta, tl, tc = [], [], []
    rep = mk(24)
    for r in range(rounds + 1):
        ta.append(events(lambda: D.deposit_trie_audit(lv, cap, n, DEPTH, root, rep)))
        tl.append(events(lambda: D.deposit_trie_levels(scratch, cap, n, 0, DEPTH, DEPTH, sroot)))
        tc.append(events(lambda: (scratch != lv).any()))
    assert D.audit_reports(rep)[0] == (0, _lib.MK_AUDIT_NONE, 2**64 - 1) and torch.equal(scratch, lv)
    nodes = sum(-(-n // (1 << d)) for d in range(1, DEPTH + 1))
    both = [a + b for a, b in zip(tl[1:], tc[1:])]
    out["audit"] = {"nodes": nodes, "audit": stat(ta[1:]), "levels_again": stat(tl[1:]), "flat_compare": stat(tc[1:]),
                    "levels_again_plus_compare": stat(both),
                    "audit_hashes_per_s": round(nodes / statistics.median(ta[1:]) * 1e3)}

    # ---- fork point: B is A rolled back to `at` and continued with other deposits
    at = n // 2 + 12345 % (n // 2)
    lvB, rootB = lv.clone(), mk(32)
    D.deposit_trie_truncate(lvB, cap, n, at, DEPTH, rootB)
    D.deposit_trie_append(lvB, cap, at, other, n - at, DEP, DEPTH, rootB)
    fork = torch.zeros(1, dtype=torch.int64, device=dev)
    tf, tc, tr = [], [], []
    for r in range(rounds + 1):
        tf.append(events(lambda: D.deposit_trie_fork_point(lv, cap, n, lvB, cap, n, DEPTH, fork)))
        tc.append(events(lambda: (lv[:32 * n] != lvB[:32 * n]).any()))
        tr.append(wall(lambda: (lv[:32 * n].cpu(), lvB[:32 * n].cpu()))[0])
    assert int(fork.item()) == at
    out["fork_point"] = {"at": at, "fork_point": stat(tf[1:]), "flat_compare_level0": stat(tc[1:]),
                         "read_back_both_level0": stat(tr[1:])}
    del lvB

    # ---- clone of a handle against the build from host data
    h = ctypes.c_void_p()
    _lib.invoke("mk_deposit_trie_new", DEPTH, n, ctypes.byref(h))
    _lib.invoke("mk_deposit_trie_append", h, _ptr(host), _ptr(offs), n)
    tcl, tb = [], []
    for r in range(rounds + 1):
        c = ctypes.c_void_p()
        tcl.append(wall(lambda: _lib.invoke("mk_deposit_trie_clone", h, ctypes.byref(c)))[0])
        got = ctypes.create_string_buffer(32)
        _lib.invoke("mk_deposit_trie_root", c, got)
        _lib.load().mk_deposit_trie_free(c)
        ms, want = wall(lambda: host_build(n))
        tb.append(ms)
        assert got.raw == want == full_root.cpu().numpy().tobytes()
    _lib.load().mk_deposit_trie_free(h)
    out["clone"] = {"clone": stat(tcl[1:]), "host_build": stat(tb[1:]), "upload_bytes": n * DEP}

    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
