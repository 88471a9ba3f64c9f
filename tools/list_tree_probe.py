#!/usr/bin/env python3
"""Device-resident list tree: build, update and append times beside the
one-shot merkleHash of the same list, in one process.

  python tools/list_tree_probe.py [--out profiles/list_tree/probe.json] [--quick]

Per list (2^24 x 32 B, 2^20 x 8 B): the full hash (mk_dev_ssz_merkle_hash,
the baseline), list_tree_build, list_tree_update for k random in-place
indices (1, 256, 65 536 and the powers of two from 2^10 up, to find where an
update stops being cheaper than a build) and for 4 096 appended items.  Every
variant is warmed up, then timed in `rounds` interleaved rounds of `reps`
back-to-back calls between device events; the figure is the median round's
ms per call.  `wall_ms` is one synchronised call on the host clock (launch
and sync included).  Every timed root is checked against the full hash.
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x5EED000000000000 + 4242


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_tree", "probe.json"))
    ap.add_argument("--quick", action="store_true", help="small lists (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D

    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise SystemExit("list_tree_probe needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    lists = [(1 << 14, 32), (1 << 12, 8)] if args.quick else [(1 << 24, 32), (1 << 20, 8)]
    rng = np.random.default_rng(1)

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def wall(fn):
        torch.cuda.synchronize()
        ts = []
        for _ in range(10):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    result = {"tool": "list_tree_probe", "version": _lib.load().mk_version().decode(), "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "lists": []}
    for n, L in lists:
        items = torch.empty(n * L, dtype=torch.uint8, device=dev)
        D.synth_fill(items, SEED + L)
        lv = torch.empty(D.list_tree_levels_bytes(n, L), dtype=torch.uint8, device=dev)
        root = torch.zeros(32, dtype=torch.uint8, device=dev)
        full = torch.zeros(32, dtype=torch.uint8, device=dev)
        mws = D.merkle_workspace(n, L, dev)
        ks = sorted({1, 256, 65536} | {1 << e for e in range(10, 23) if (1 << e) <= n // 4})
        idx = {k: torch.from_numpy(np.sort(rng.choice(n, k, replace=False)).astype(np.int64)).to(dev) for k in ks}
        ws = torch.empty(D.list_tree_update_workspace_bytes(max(max(ks), 4096)), dtype=torch.uint8, device=dev)
        napp = min(4096, n // 2)

        variants = {"full_hash": lambda: D.merkle_hash(items, n, L, out=full, ws=mws),
                    "build": lambda: D.list_tree_build(items, n, n, L, lv, root, ws=ws)}
        for k in ks:
            variants[f"update_k{k}"] = (lambda k=k: D.list_tree_update(items, n, n, n, L, lv, root, idx[k], k, None,
                                                                       ws=ws))
        variants[f"append_{napp}"] = lambda: D.list_tree_update(items, n - napp, n, n, L, lv, root, None, 0, None,
                                                                ws=ws)
        variants["build"]()  # the updates below climb a built tree
        variants["full_hash"]()
        torch.cuda.synchronize()
        want = bytes(full.cpu().numpy())
        reps = {}
        for name, fn in variants.items():  # warm-up, a root check, and a repeat count for >= ~50 ms per round
            root.zero_()
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            if name != "full_hash":
                assert bytes(root.cpu().numpy()) == want, f"{name}: root differs from the full hash"
            ms = timed(fn, 3)
            reps[name] = max(3, min(200, int(50.0 / max(ms, 1e-3))))
        samples = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                samples[name].append(timed(fn, reps[name]))
        row = {"n": n, "item_len": L, "ms": {}, "ms_min": {}, "ms_max": {}, "wall_ms": {}, "reps": reps}
        for name, fn in variants.items():
            row["ms"][name] = round(statistics.median(samples[name]), 5)
            row["ms_min"][name] = round(min(samples[name]), 5)
            row["ms_max"][name] = round(max(samples[name]), 5)
        for name in ("full_hash", "build", "update_k1", "update_k256"):
            row["wall_ms"][name] = round(wall(variants[name]), 5)
        below = [k for k in ks if row["ms"][f"update_k{k}"] < row["ms"]["build"]]
        row["largest_k_cheaper_than_build"] = max(below) if below else 0
        row["k1_faster_than_full_hash"] = row["ms"]["update_k1"] < row["ms"]["full_hash"]
        result["lists"].append(row)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
