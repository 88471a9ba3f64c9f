#!/usr/bin/env python3
"""Resident trees copied on the device: what clone and reserve
cost, beside the only way to the same state before them.

  python tools/tree_copy_probe.py [--out profiles/tree_copy/probe.json] [--quick]

  registry_clone  StructListTree of 2^20 ValidatorRecords: clone() against
                  assign() of the same records from host arrays
  list_clone      ListTree of 2^24 x 32-B items: the same pair
  set_clone       BeaconTreeSet of a 2^20-validator state: clone() against
                  assign_state() + root() of the same state
  reserve         the registry tree at capacity == count: reserve(2 n) against
                  an append of one record, which crosses the capacity and
                  rebuilds (today's path), each on a freshly assigned tree
  device          mk_dev_ssz_trees_copy of the registry tree in torch buffers
                  against one flat device-to-device copy_ of the same number of
                  bytes, and against one copy_ per live extent
The handle calls upload or synchronise themselves: host wall time
(time.perf_counter).  The device forms are timed with device events on the
stream of the call.  One process, `rounds` interleaved rounds; `ms` is the
median, `ms_min` / `ms_max` the spread.  The clocks are not pinned.  Every clone
is held against its source's root.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x5EED000000000000 + 4848


def stat(xs):
    return {"ms": round(statistics.median(xs), 4), "ms_min": round(min(xs), 4), "ms_max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_copy", "probe.json"))
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()

    import numpy as np
    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D
    from prysm_amd import listtree as LT
    from prysm_amd import registry as R
    from prysm_amd import state as ST

    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise SystemExit("tree_copy_probe needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    nreg = 1 << (12 if args.quick else 20)
    nlist = 1 << (14 if args.quick else 24)
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

    out = {"probe": "tree_copy", "rounds": rounds, "quick": bool(args.quick)}

    # ---- one handle: clone against assign
    def clone_vs_assign(make, values):
        src = make()
        src.assign(values)
        spare = make()
        want = src.root()
        tc, ta = [], []
        for r in range(rounds + 1):  # the first round warms up and is dropped
            ms, c = wall(src.clone)
            assert c.root() == want
            del c
            tc.append(ms)
            ms, _ = wall(lambda: spare.assign(values))
            ta.append(ms)
        assert spare.root() == want
        return {"clone": stat(tc[1:]), "assign": stat(ta[1:])}

    recs = R.synthetic_registry(nreg, SEED).records
    out["registry_clone"] = dict(n=nreg, **clone_vs_assign(lambda: LT.StructListTree(160, R.VALIDATOR_FIELDS), recs))
    items = np.random.default_rng(5).integers(0, 256, nlist * 32, dtype=np.uint8)
    out["list_clone"] = dict(n=nlist, **clone_vs_assign(lambda: LT.ListTree(32), items))
    del items

    # ---- the whole state
    st = ST.synthetic_state(nreg, SEED + 1, n_attestations=128, n_batched=16, n_votes=4,
                            lists_len=64 if args.quick else 8192, shards=64 if args.quick else 1024)
    ts = ST.beacon_tree_set(st)
    spare = ST.beacon_tree_set()
    want = ts.root()
    tc, ta = [], []
    for r in range(rounds + 1):
        ms, c = wall(ts.clone)
        assert c.root() == want
        del c
        tc.append(ms)

        def again():
            spare.assign_state(st)
            return spare.root()
        ms, got = wall(again)
        assert got == want
        ta.append(ms)
    out["set_clone"] = {"validators": nreg, "clone": stat(tc[1:]), "assign": stat(ta[1:])}
    del ts, spare

    # ---- reserve against the append that crosses the capacity
    tr, tp = [], []
    for r in range(rounds + 1):
        a = LT.StructListTree(160, R.VALIDATOR_FIELDS, capacity=nreg)
        a.assign(recs)
        root = a.root()
        ms, _ = wall(lambda: a.reserve(2 * nreg))
        assert a.root() == root and a.capacity == 2 * nreg
        tr.append(ms)
        b = LT.StructListTree(160, R.VALIDATOR_FIELDS, capacity=nreg)
        b.assign(recs)
        ms, _ = wall(lambda: b.append(recs[:1]))
        assert b.capacity == 2 * nreg
        tp.append(ms)
        del a, b
    out["reserve"] = {"n": nreg, "reserve_2n": stat(tr[1:]), "append_across_capacity": stat(tp[1:])}

    # ---- the device entry against the card's own copy of the same bytes
    n, cap = nreg, nreg
    lvb = D.list_tree_levels_bytes(cap, 32)
    mk = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)  # noqa: E731
    s_items, s_l0, s_lv, s_root = mk(cap * 160 + 16), mk(32 * cap), mk(lvb), mk(32)
    d_items, d_l0, d_lv, d_root = mk(2 * cap * 160 + 16), mk(64 * cap), mk(D.list_tree_levels_bytes(2 * cap, 32)), mk(32)
    s_items[: n * 160] = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(dev)
    D.struct_list_tree_build(s_items, n, cap, 160, R.VALIDATOR_FIELDS, s_l0, s_lv, s_root)
    live = [n * 160, 32 * n, 32]
    c = -(-n // 4)
    while c > 1:
        c = (c + 1) // 2
        live.append(32 * c)
    moved = sum(live)
    flat_s, flat_d = mk(moved), mk(moved)
    parts = [(mk(b), mk(b)) for b in live]
    desc = D.TreeCopyArgs(_lib.MK_TREE_STRUCT, 160, n, cap, 2 * cap, s_items, s_lv, s_root, d_items, d_lv, d_root,
                          src_level0=s_l0, dst_level0=d_l0)
    tk, tf, tp = [], [], []
    for r in range(rounds + 1):
        tk.append(events(lambda: D.trees_copy([desc])))
        tf.append(events(lambda: flat_d.copy_(flat_s)))
        tp.append(events(lambda: [d.copy_(s) for s, d in parts]))
    assert torch.equal(d_items[: n * 160], s_items[: n * 160]) and torch.equal(d_root, s_root)
    gbs = lambda ms: round(2 * moved / ms / 1e6, 1)  # noqa: E731  read + written
    out["device"] = {"n": n, "bytes_moved": moved, "trees_copy": stat(tk[1:]), "flat_copy": stat(tf[1:]),
                     "per_extent_copies": stat(tp[1:]), "extents": len(live),
                     "trees_copy_gbs": gbs(statistics.median(tk[1:])), "flat_copy_gbs": gbs(statistics.median(tf[1:]))}

    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
