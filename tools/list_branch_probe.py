#!/usr/bin/env python3
"""Resident list trees: batched Merkle proofs and the batched verifier, each
beside what a caller had before them, in one process (the
conventions of tools/trie_branch_probe.py).

  python tools/list_branch_probe.py [--out profiles/list_branches/probe.json] [--quick]

  dev_*    device forms on the current stream, between device events
  host_*   handle / host-buffer forms, which synchronize themselves: wall clock
a  16 proofs out of a 2^20-record registry tree (StructListTree.branches)
                                     | the whole list read back (records(); the
   caller would then hash 2^20 structs and build the tree on the CPU: not timed)
b  16 proofs out of a 2^24 x 32-B list tree (ListTree.branches)
                                     | the whole list read back (items())
c  2^16 proofs in one mk_dev_ssz_list_tree_branches over the 2^24 x 32-B tree:
   GB/s of proof bytes written (no yardstick exists)
d  mk_dev_verify_list_branches / mk_verify_list_branches at 16 and 2^16 proofs
                                     | mk_verify_merkle_branches at the same depth
   (host form: it has no device form)
Every variant is warmed up, then timed in `rounds` interleaved rounds of `reps`
back-to-back calls; `ms` is the median round's ms per call, `ms_min` / `ms_max`
the spread.  The process reads no oracle: results are cross-checked against
each other (handle records against the device form's, every produced proof
accepted, a flipped value rejected).  Prints one JSON line and writes it to
--out.
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

SEED = 0x5EED000000000000 + 5252


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_branches", "probe.json"))
    ap.add_argument("--quick", action="store_true", help="2^12-value trees (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D
    from prysm_amd import registry as RG
    from prysm_amd.listtree import ListTree, StructListTree, verify_branches

    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise SystemExit("list_branch_probe needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    nreg = 1 << (12 if args.quick else 20)
    nlist = 1 << (12 if args.quick else 24)
    kbulk = min(1 << 16, nlist)
    u8 = dict(dtype=torch.uint8, device=dev)

    def ev_timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def wall_timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / reps

    def _vp(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    rng = np.random.default_rng(1)
    # a: the registry
    reg = StructListTree(160, RG.VALIDATOR_FIELDS, capacity=nreg)
    reg.assign(RG.synthetic_registry(nreg, SEED).records)
    ridx = np.sort(rng.choice(nreg, 16, replace=False)).astype(np.uint64)
    # b, c, d: the 2^24 x 32-B list, as a handle and as device buffers (the same bytes)
    items = D.synth_fill(torch.empty(nlist * 32, **u8), SEED + 1)
    levels = torch.zeros(max(D.list_tree_levels_bytes(nlist, 32), 16), **u8)
    root = torch.zeros(32, **u8)
    D.list_tree_build(items, nlist, nlist, 32, levels, root=root)
    host_items = items.cpu().numpy()
    lt = ListTree(32, capacity=nlist)
    lt.assign(host_items)
    lidx = np.sort(rng.choice(nlist, 16, replace=False)).astype(np.uint64)
    stride = D.list_branch_bytes(nlist, 32)
    depth = (stride - 256) // 32 + 1
    d_bulk = torch.from_numpy(rng.integers(0, nlist, size=kbulk).astype(np.int64)).to(dev)
    out_bulk = torch.zeros(kbulk * stride, **u8)
    ok = torch.zeros(kbulk, **u8)

    def dev_bulk():
        D.list_tree_branches(items, nlist, nlist, 32, levels, d_bulk, out=out_bulk)

    dev_bulk()
    d_vals = items.view(nlist, 32)[d_bulk].contiguous().view(-1)
    torch.cuda.synchronize()
    h_bulk = d_bulk.cpu().numpy().astype(np.uint64)
    h_vals = d_vals.cpu().numpy()
    h_br = out_bulk.cpu().numpy()
    h_root = bytes(root.cpu().numpy())
    h_roots = np.tile(np.frombuffer(h_root, dtype=np.uint8), kbulk)
    h_ok = np.zeros(kbulk, dtype=np.uint8)
    # the old verifier's inputs at the same depth: the timing does not depend on the verdicts
    o_leaves = h_vals[:kbulk * 32]
    o_br = np.ascontiguousarray(h_br.reshape(kbulk, stride)[:, :depth * 32]).reshape(-1)

    def dev_verify(nv):
        D.verify_list_branches(d_vals, d_bulk, nv, nlist, 32, out_bulk, root, out=ok)

    def host_verify_new(nv):
        _lib.invoke("mk_verify_list_branches", _vp(h_vals), _vp(h_bulk), nv, nlist, 32, _vp(h_br), _vp(h_roots), 0,
                    None, 0, 0, _vp(h_ok))

    def host_verify_old(nv):
        _lib.invoke("mk_verify_merkle_branches", _vp(o_leaves), _vp(o_br), _vp(h_bulk), nv, depth, depth, _vp(h_roots),
                    _vp(h_ok))

    ev = {"dev_branches_bulk": dev_bulk}
    wall = {"host_registry_branches16": lambda: reg.branches(ridx),
            "host_registry_records_all": lambda: reg.records(),
            "host_list_branches16": lambda: lt.branches(lidx),
            "host_list_items_all": lambda: lt.items()}
    nvs = (16, kbulk)
    for nv in nvs:
        ev[f"dev_verify_list_branches_n{nv}"] = (lambda nv=nv: dev_verify(nv))
        wall[f"host_verify_list_branches_n{nv}"] = (lambda nv=nv: host_verify_new(nv))
        wall[f"host_verify_merkle_branches_n{nv}"] = (lambda nv=nv: host_verify_old(nv))

    # cross-checks (no oracle in this process)
    assert lt.root() == h_root, "the handle's root differs from the device tree's"
    vals16, br16 = lt.branches(lidx)
    d16 = D.list_tree_branches(items, nlist, nlist, 32, levels, torch.from_numpy(lidx.astype(np.int64)).to(dev))
    torch.cuda.synchronize()
    assert br16.tobytes() == d16.cpu().numpy().tobytes(), "handle records differ from the device form's"
    assert verify_branches(vals16, lidx, nlist, 32, br16, h_root).all(), "a list proof did not verify"
    rv, rb = reg.branches(ridx)
    assert verify_branches(rv, ridx, nreg, 32, rb, reg.root()).all(), "a registry proof did not verify"
    bad = rv.copy()
    bad[3, 5] ^= 1
    assert verify_branches(bad, ridx, nreg, 32, rb, reg.root()).tolist() == [g != 3 for g in range(16)]
    for nv in nvs:
        ok.zero_()
        dev_verify(nv)
        torch.cuda.synchronize()
        assert bool(ok[:nv].all()), "a bulk proof did not verify on the device"
        host_verify_new(nv)
        assert h_ok[:nv].all(), "a bulk proof did not verify from host buffers"

    reps, samples = {}, {}
    for table, timed in ((ev, ev_timed), (wall, wall_timed)):
        for name, fn in table.items():  # warm-up and a repeat count for >= ~30 ms per round
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            ms = timed(fn, 2)
            reps[name] = max(2, min(200, int(30.0 / max(ms, 1e-3))))
            samples[name] = []
    for _ in range(args.rounds):
        for table, timed in ((ev, ev_timed), (wall, wall_timed)):
            for name, fn in table.items():
                samples[name].append(timed(fn, reps[name]))
    res = {"tool": "list_branch_probe", "version": _lib.load().mk_version().decode(), "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "registry_records": nreg, "list_items": nlist, "item_len": 32,
           "record_bytes": int(stride), "registry_record_bytes": int(D.list_branch_bytes(nreg, 32)),
           "verify_depth": int(depth), "k_bulk": kbulk, "reps": reps,
           "ms": {k: round(statistics.median(v), 5) for k, v in samples.items()},
           "ms_min": {k: round(min(v), 5) for k, v in samples.items()},
           "ms_max": {k: round(max(v), 5) for k, v in samples.items()}}
    res["bulk_gb_per_s"] = round(kbulk * stride / 1e9 / (res["ms"]["dev_branches_bulk"] * 1e-3), 1)

    def wins(new, old):  # a win only by more than the larger spread of the two
        sp = max(res["ms_max"][new] - res["ms_min"][new], res["ms_max"][old] - res["ms_min"][old])
        return res["ms"][old] - res["ms"][new] > sp

    res["beats_yardstick"] = {
        "registry_branches16": wins("host_registry_branches16", "host_registry_records_all"),
        "list_branches16": wins("host_list_branches16", "host_list_items_all"),
        **{f"host_verify_n{nv}": wins(f"host_verify_list_branches_n{nv}", f"host_verify_merkle_branches_n{nv}")
           for nv in nvs}}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
