#!/usr/bin/env python3
"""Shrinking a resident tree on the device: what truncate and
the stable erase cost, beside the only way to the same list before them.

  python tools/tree_shrink_probe.py [--out profiles/tree_shrink/probe.json] [--quick]

  attestations   a StructListTree of 2^14 PendingAttestationRecords losing its
                 older half (CleanupAttestations: a scattered half): erase of
                 the dropped positions against assign of the survivors, the
                 same handle, the same process, interleaved.  Host wall time
                 (time.perf_counter): both calls upload and synchronise, and
                 the upload is what differs.
  bytes_erase    mk_dev_ssz_bytes_list_tree_erase on 2^20 x 32-B elements
                 losing 1, 256 and 2^16 scattered elements (first = the lowest)
  list_truncate  mk_dev_ssz_list_tree_erase on 2^24 x 32-B items truncated by
                 one item and by half
  climb_vs_build the climb over a dirty suffix of T items (the form a shrink
                 uses: mk_dev_ssz_list_tree_update with n_old = n - T) against
                 the level build, 2^20 x 32-B items -- which side of the kind's
                 rebuild divisor is right for a shrink
The device entries are timed with device events on the stream of the call,
buffers restored (untimed) between samples.  `rounds` interleaved rounds; `ms`
is the median, `ms_min` / `ms_max` the spread.  The clocks are not pinned.
Every shrunk root is held against the one-shot build of the same list.  Prints
one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x5EED000000000000 + 4747


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_shrink", "probe.json"))
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D
    from prysm_amd import listtree as LT
    from prysm_amd import state as ST

    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise SystemExit("tree_shrink_probe needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    q = args.quick
    rng = np.random.default_rng(4)

    def stats(samples):
        return {"ms": round(statistics.median(samples), 4), "ms_min": round(min(samples), 4),
                "ms_max": round(max(samples), 4)}

    def timed(fn):
        """ms of fn() on the current stream, by device events."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    result = {}

    # ---- the attestation handle: erase against assign of the survivors ----------------------------
    na = 1 << 10 if q else 1 << 14
    st = ST.synthetic_state(0, SEED, n_attestations=na, n_batched=0, n_votes=0, lists_len=1, shards=1)
    rec, fields = ST.pack_attestations(st.attestations, 48)
    med = int(np.sort(st.attestations.slot)[na // 2])
    drop = np.nonzero(st.attestations.slot < med)[0].astype(np.uint64)
    keep = np.nonzero(st.attestations.slot >= med)[0]
    survivors = np.ascontiguousarray(rec[keep])
    tree = LT.StructListTree(rec.shape[1], fields, capacity=na)
    samples = {"erase": [], "assign_survivors": []}
    roots = set()
    for r in range(args.rounds + 1):  # round 0 warms up
        for name in samples:
            tree.assign(rec)
            t0 = time.perf_counter()
            tree.erase(drop) if name == "erase" else tree.assign(survivors)
            dt = 1e3 * (time.perf_counter() - t0)
            roots.add(tree.root())
            assert len(tree) == len(keep)
            if r:
                samples[name].append(dt)
    assert len(roots) == 1, "erase and assign of the survivors disagree"
    result["attestations"] = {"records": na, "dropped": int(drop.size), "record_len": int(rec.shape[1]),
                              **{k: stats(v) for k, v in samples.items()}}
    del tree

    # ---- device entries ------------------------------------------------------------------------------
    def dev_tree(kind, n, L):
        items = torch.empty(n * L + 16, dtype=torch.uint8, device=dev)
        D.synth_fill(items[: (n * L) // 8 * 8], SEED + n)
        len0 = L if kind == _lib.MK_TREE_LIST else 32
        level0 = None if kind == _lib.MK_TREE_LIST else torch.empty(32 * n, dtype=torch.uint8, device=dev)
        lv = torch.empty(D.list_tree_levels_bytes(n, len0), dtype=torch.uint8, device=dev)
        root = torch.empty(32, dtype=torch.uint8, device=dev)
        if kind == _lib.MK_TREE_LIST:
            D.list_tree_build(items, n, n, L, lv, root)
        else:
            D.bytes_list_tree_build(items, n, n, L, level0, lv, root)
        return items, level0, lv, root

    def one_shot(kind, items, n, n_cap, L):
        """The root of the first n values of `items` by a fresh build."""
        len0 = L if kind == _lib.MK_TREE_LIST else 32
        lv = torch.empty(D.list_tree_levels_bytes(n_cap, len0), dtype=torch.uint8, device=dev)
        if kind == _lib.MK_TREE_LIST:
            r = D.list_tree_build(items, n, n_cap, L, lv)
        else:
            r = D.bytes_list_tree_build(items, n, n_cap, L, torch.empty(32 * n_cap, dtype=torch.uint8, device=dev), lv)
        return bytes(r.cpu().numpy())

    # bytes tree: scattered erases
    nb = 1 << 14 if q else 1 << 20
    items, level0, lv, root = dev_tree(_lib.MK_TREE_BYTES, nb, 32)
    saved = (items.clone(), level0.clone(), lv.clone())
    cases = {}
    for k in (1, 256, 1 << 10 if q else 1 << 16):
        rm = np.sort(rng.choice(nb, k, replace=False)).astype(np.int64)
        d_rm = torch.from_numpy(rm).to(dev)
        first = int(rm[0])
        ws = torch.empty(D.tree_erase_workspace_bytes(_lib.MK_TREE_BYTES, nb - k - first, 32), dtype=torch.uint8,
                         device=dev)
        cases[k] = (d_rm, first, ws, rm)
    samples = {k: [] for k in cases}
    for r in range(args.rounds + 1):
        for k, (d_rm, first, ws, rm) in cases.items():
            for buf, was in zip((items, level0, lv), saved):
                buf.copy_(was)
            dt = timed(lambda: D.tree_erase(_lib.MK_TREE_BYTES, items, nb, nb - k, nb, 32, lv, root, d_rm, k, first,
                                            level0=level0, ws=ws))
            if r:
                samples[k].append(dt)
            else:
                keep_mask = np.ones(nb, dtype=bool)
                keep_mask[rm] = False
                want = saved[0][: nb * 32].reshape(nb, 32)[torch.from_numpy(keep_mask).to(dev)].reshape(-1).contiguous()
                assert bytes(root.cpu().numpy()) == one_shot(_lib.MK_TREE_BYTES, want, nb - k, nb, 32), k
    result["bytes_erase"] = {"elements": nb, "elem_len": 32,
                             "removed": {str(k): {"first": cases[k][1], **stats(v)} for k, v in samples.items()}}
    del items, level0, lv, saved, cases

    # list: truncates
    nl = 1 << 16 if q else 1 << 24
    items, _, lv, root = dev_tree(_lib.MK_TREE_LIST, nl, 32)
    saved_lv = lv.clone()
    ws = torch.empty(D.tree_erase_workspace_bytes(_lib.MK_TREE_LIST, 0, 32), dtype=torch.uint8, device=dev)
    samples = {"by_one": [], "by_half": []}
    for r in range(args.rounds + 1):
        for name, n_new in (("by_one", nl - 1), ("by_half", nl // 2)):
            lv.copy_(saved_lv)
            dt = timed(lambda: D.tree_erase(_lib.MK_TREE_LIST, items, nl, n_new, nl, 32, lv, root, ws=ws))
            if r:
                samples[name].append(dt)
            else:
                assert bytes(root.cpu().numpy()) == one_shot(_lib.MK_TREE_LIST, items, n_new, nl, 32), name
    result["list_truncate"] = {"items": nl, "item_len": 32, **{k: stats(v) for k, v in samples.items()}}
    del items, lv, saved_lv

    # the climb over a dirty suffix against the level build
    nc = 1 << 14 if q else 1 << 20
    items, _, lv, root = dev_tree(_lib.MK_TREE_LIST, nc, 32)
    Ts = [1 << e for e in range(0, (12 if q else 18), 2)]
    wsu = torch.empty(D.list_tree_update_workspace_bytes(max(Ts)), dtype=torch.uint8, device=dev)
    wsb = torch.empty(_lib.load().mk_ssz_list_tree_build_workspace_bytes(nc, 32), dtype=torch.uint8, device=dev)
    samples = {f"climb_{T}": [] for T in Ts}
    samples["build"] = []
    want = bytes(root.cpu().numpy())
    for r in range(args.rounds + 1):
        for T in Ts:
            dt = timed(lambda: D.list_tree_update(items, nc - T, nc, nc, 32, lv, root, ws=wsu))
            assert bytes(root.cpu().numpy()) == want
            if r:
                samples[f"climb_{T}"].append(dt)
        dt = timed(lambda: D.list_tree_build(items, nc, nc, 32, lv, root, ws=wsb))
        if r:
            samples["build"].append(dt)
    result["climb_vs_build"] = {"items": nc, "item_len": 32, "rebuild_div": {
        "list": _lib.LIST_TREE_REBUILD_DIV, "struct": _lib.STRUCT_TREE_REBUILD_DIV, "bytes": _lib.BYTES_TREE_REBUILD_DIV},
        **{k: stats(v) for k, v in samples.items()}}

    out = {"tool": "tree_shrink_probe", "version": _lib.load().mk_version().decode(), "rounds": args.rounds,
           "quick": q, "device": torch.cuda.get_device_name(0), "clocks_pinned": False, **result}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
