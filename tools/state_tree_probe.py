#!/usr/bin/env python3
"""Resident BeaconState: one slot's changes to the ten list trees and the
state root, in one launch against the composition of the existing entry points,
in one process (the method of tools/bytes_tree_probe.py).

  python tools/state_tree_probe.py [--out profiles/state_tree/probe.json] [--quick]

The state is synthetic_state(2^20 validators) resident on the device
(prysm_amd.state.ResidentBeaconState).  The change set of one slot: one block
root and one randao mix, three balances, two validator records, one appended
attestation, one crosslink, the Slot scalar; the other five lists unchanged.
  a  trees_update     mk_dev_ssz_trees_update over the ten trees: every stage 0,
                      then all climbs and the 536-B state hash in one launch
  b  ten_updates      the ten existing mk_dev_ssz_*_tree_update calls back to
                      back on the same stream, their roots written straight
                      into the 536-B message, then mk_dev_hash_batch over it
                      (what a caller can compose without the new entry)
Both get the same index and value buffers (the values are scattered in by the
calls).  Every variant is warmed up, then timed in `rounds` interleaved rounds
of `reps` back-to-back calls between device events; `ms` is the median round's
ms per call, `ms_min` / `ms_max` the spread of the rounds.  The clocks are not
pinned.  The two state roots must be equal, and equal to the one-shot
BeaconState.tree_hash_ssz() of the same state.  Also recorded: the host wall
time of ResidentBeaconState.root() after a slot's changes, and of
tree_hash_ssz().  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x5EED000000000000 + 4646


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_tree", "probe.json"))
    ap.add_argument("--quick", action="store_true", help="a small registry (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D
    from prysm_amd import state as ST

    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise SystemExit("state_tree_probe needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    nv = 1 << 12 if args.quick else 1 << 20
    st = ST.synthetic_state(nv, SEED)
    donor = ST.synthetic_state(64, SEED + 1, n_attestations=32, n_batched=0, lists_len=64, shards=64)
    rs = ST.ResidentBeaconState(dev)
    rs.assign(st)
    assert rs.root() == st.tree_hash_ssz(), "the resident root differs from the one-shot root"
    # room for the appended attestation without a rebuild: one append doubles the capacity
    att = rs.trees["attestations"]
    att.append(ST.pack_attestations(donor.attestations, 48)[0][:1])
    rs.root()  # grows the attestation tree; every tree is built and clean after this
    rng = np.random.default_rng(3)

    def u8(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    def idx(a):
        return torch.from_numpy(np.sort(np.asarray(a, dtype=np.int64))).to(dev)

    # the slot's change set: (indices, values, appended) per tree
    natt = att.n
    change = {
        "registry": (idx(rng.choice(nv, 2, replace=False)), u8(donor.registry.records[:2]), 0),
        "balances": (idx(rng.choice(nv, 3, replace=False)), u8(donor.balances[:3].astype("<u8")), 0),
        "randao_mixes": (idx([4242]), u8(donor.randao_mixes[0]), 0),
        "crosslinks": (idx([517]), u8(ST.pack_crosslinks(donor.crosslink_epochs[:1], donor.crosslink_roots[:1])), 0),
        "latest_block_roots": (idx([4242]), u8(donor.latest_block_roots[0]), 0),
        "attestations": (None, u8(ST.pack_attestations(donor.attestations, 48)[0][1:2]), 1),  # re-appends the last one
    }
    slot_bytes = torch.from_numpy(np.array([st.scalars["Slot"] + 1], dtype="<u8").view(np.uint8).copy()).to(dev)
    slot_off = ST.CONTAINER_OFF["Slot"]

    def tree_args(name, root, coff):
        t = rs.trees[name]
        ix, vals, napp = change.get(name, (None, None, 0))
        return D.TreeArgs(t.kind, t.items, t.n - napp, t.n, t.cap, t.item_len, t.levels, root, level0=t.level0,
                          idx=ix, k_idx=0 if ix is None else ix.numel(), values=vals, spec=t.spec,
                          container_off=coff)

    names = [attr for attr, *_ in ST.RESIDENT_TREES]
    # (a): the roots in their own tensors, the container written by the kernel
    cont_a = rs.container.clone()
    root_a = torch.zeros(32, dtype=torch.uint8, device=dev)
    trees_a = [tree_args(n, rs.trees[n].root, rs._off[n]) for n in names]
    ws_a = torch.empty(D.trees_update_workspace_bytes(trees_a), dtype=torch.uint8, device=dev)

    def many():
        cont_a[slot_off:slot_off + 8] = slot_bytes
        D.trees_update(trees_a, cont_a, ST.CONTAINER_LEN, root_a, ws_a)

    # (b): every root written straight into the message by its own update call
    cont_b = rs.container.clone()
    root_b = torch.zeros(32, dtype=torch.uint8, device=dev)
    trees_b = [tree_args(n, cont_b[rs._off[n]:rs._off[n] + 32], None) for n in names]
    ws_b = [torch.empty(D.trees_update_workspace_bytes([t]), dtype=torch.uint8, device=dev) for t in trees_b]

    def ten():
        cont_b[slot_off:slot_off + 8] = slot_bytes
        for t, ws in zip(trees_b, ws_b):
            if t.kind == _lib.MK_TREE_LIST:
                D.list_tree_update(t.items, t.n_old, t.n_new, t.capacity, t.item_len, t.levels, t.root, t.idx,
                                   t.k_idx, t.values, ws=ws)
            elif t.kind == _lib.MK_TREE_STRUCT:
                D.struct_list_tree_update(t.items, t.n_old, t.n_new, t.capacity, t.item_len, t.spec, t.level0,
                                          t.levels, t.root, t.idx, t.k_idx, t.values, ws=ws)
            else:
                D.bytes_list_tree_update(t.items, t.n_old, t.n_new, t.capacity, t.item_len, t.level0, t.levels,
                                         t.root, t.idx, t.k_idx, t.values, ws=ws)
        D.hash_batch(cont_b, 1, ST.CONTAINER_LEN, out=root_b)

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    variants = {"trees_update": many, "ten_updates": ten}
    reps = {}
    for name, fn in variants.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = timed(fn, 3)
        reps[name] = max(3, min(200, int(50.0 / max(ms, 1e-3))))
    ra, rb = bytes(root_a.cpu().numpy()), bytes(root_b.cpu().numpy())
    assert ra == rb, "the state roots of the two configurations differ"
    assert np.array_equal(cont_a.cpu().numpy(), cont_b.cpu().numpy()), "the two 536-B messages differ"
    samples = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            samples[name].append(timed(fn, reps[name]))
    row = {"validators": nv, "ms": {}, "ms_min": {}, "ms_max": {}, "reps": reps}
    for name in variants:
        row["ms"][name] = round(statistics.median(samples[name]), 5)
        row["ms_min"][name] = round(min(samples[name]), 5)
        row["ms_max"][name] = round(max(samples[name]), 5)
    spread = max(row["ms_max"][n] - row["ms_min"][n] for n in variants)
    row["one_launch_beats_ten_updates"] = row["ms"]["ten_updates"] - row["ms"]["trees_update"] > spread

    # host wall time: root() after one slot's changes (the changes themselves are not timed), and the one-shot
    wall = []
    for s in range(10):
        at = (st.scalars["Slot"] + s) % 8192
        rs.update("latest_block_roots", [at], donor.latest_block_roots[s:s + 1])
        rs.update("randao_mixes", [at], donor.randao_mixes[s:s + 1])
        rs.update("balances", rng.choice(nv, 3, replace=False), donor.balances[:3].astype("<u8"))
        rs.update("registry", rng.choice(nv, 2, replace=False), donor.registry.records[2 * s:2 * s + 2])
        rs.append("attestations", ST.pack_attestations(donor.attestations, 48)[0][s + 2:s + 3])
        rs.update("crosslinks", [s], ST.pack_crosslinks(donor.crosslink_epochs[s:s + 1],
                                                        donor.crosslink_roots[s:s + 1]))
        rs.set_scalar("Slot", st.scalars["Slot"] + s + 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rs.root()
        wall.append(1e3 * (time.perf_counter() - t0))
    shot = []
    for _ in range(3):
        t0 = time.perf_counter()
        st.tree_hash_ssz()
        shot.append(1e3 * (time.perf_counter() - t0))
    row["host_wall_ms"] = {"resident_root": round(statistics.median(wall), 3),
                           "resident_root_min": round(min(wall), 3), "resident_root_max": round(max(wall), 3),
                           "tree_hash_ssz": round(statistics.median(shot), 3),
                           "tree_hash_ssz_min": round(min(shot), 3), "tree_hash_ssz_max": round(max(shot), 3)}
    result = {"tool": "state_tree_probe", "version": _lib.load().mk_version().decode(), "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "clocks_pinned": False,
              "state": row}
    line = json.dumps(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
