#!/usr/bin/env python3
"""mk_tree_set: host wall time of one slot of a resident BeaconState behind one
C handle, beside what a host caller could do before it (the
method of tools/state_tree_probe.py).

  python tools/tree_set_probe.py [--out profiles/tree_set/probe.json] [--quick]

The state is synthetic_state(2^20 validators); the change set of one slot is
§5h's: one block root and one randao mix, three balances, two validator
records, one appended attestation, one crosslink, the Slot scalar.
  set_root       mk_tree_set_root alone, after the slot's update / append / put
                 calls (host only, not timed)
  set_slot       those calls and the root
  ten_handles    the ten single handles: mk_*_tree_update / append for the six
                 changed lists, ten mk_*_tree_root, mk_hash_batch of the 536-B
                 message assembled on the host (a cgo caller's only way so far)
  resident_root  ResidentBeaconState.root() after the same changes (the device
                 caller's form, torch tensors; its changes are not timed)
time.perf_counter, `rounds` interleaved rounds of `slots` slots each; `ms` is
the median round's ms per slot, `ms_min` / `ms_max` the spread of the rounds.
The clocks are not pinned.  All roots of a slot must be equal.  Prints one JSON
line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x5EED000000000000 + 4646


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_set", "probe.json"))
    ap.add_argument("--quick", action="store_true", help="a small registry (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slots", type=int, default=8)
    args = ap.parse_args()

    import numpy as np
    import torch

    from prysm_amd import _lib
    from prysm_amd import hashutil as H
    from prysm_amd import listtree as LT
    from prysm_amd import state as ST

    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise SystemExit("tree_set_probe needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    nv = 1 << 12 if args.quick else 1 << 20
    st = ST.synthetic_state(nv, SEED)
    donor = ST.synthetic_state(64, SEED + 1, n_attestations=64, n_batched=0, lists_len=64, shards=64)
    att_rows = ST.pack_attestations(donor.attestations, 48)[0]

    # the three holders of the same state
    ts = ST.beacon_tree_set(st)
    rs = ST.ResidentBeaconState(dev)
    rs.assign(st)
    u8 = lambda a: np.ascontiguousarray(a).view(np.uint8)  # noqa: E731  (the single handles take bytes)
    lists = {"registry": st.registry.records, "balances": u8(st.balances.astype("<u8")),
             "randao_mixes": st.randao_mixes, "crosslinks": ST.pack_crosslinks(st.crosslink_epochs, st.crosslink_roots),
             "latest_block_roots": st.latest_block_roots, "batched_block_roots": st.batched_block_roots,
             "penalized_balances": u8(st.penalized_balances.astype("<u8")),
             "attestations": ST.pack_attestations(st.attestations, 48)[0], "index_roots": st.index_roots,
             "eth1_votes": ST.pack_eth1_votes(st.eth1_votes, st.eth1_vote_counts)}
    handles = {}
    for attr, _, kind, item_len, spec in ST.RESIDENT_TREES:
        if kind == _lib.MK_TREE_LIST:
            handles[attr] = LT.ListTree(item_len)
        elif kind == _lib.MK_TREE_STRUCT:
            handles[attr] = LT.StructListTree(item_len, spec)
        else:
            handles[attr] = LT.BytesListTree(item_len)
        handles[attr].assign(lists[attr])
    msg = bytearray(rs.container[:ST.CONTAINER_LEN].cpu().numpy().tobytes())  # the small fields as assign() put them
    off = {attr: ST.CONTAINER_OFF[name] for attr, name, *_ in ST.RESIDENT_TREES}
    rng = np.random.default_rng(3)
    slot_no = [0]

    def change():
        """The next slot's change set: [(list, indices or None, rows)], the Slot scalar."""
        s = slot_no[0]
        slot_no[0] += 1
        at = (st.scalars["Slot"] + s) % 8192
        return [("latest_block_roots", [at], donor.latest_block_roots[s % 64:s % 64 + 1]),
                ("randao_mixes", [at], donor.randao_mixes[s % 64:s % 64 + 1]),
                ("balances", rng.choice(nv, 3, replace=False), u8(donor.balances[:3].astype("<u8"))),
                ("registry", rng.choice(nv, 2, replace=False), donor.registry.records[2 * (s % 32):2 * (s % 32) + 2]),
                ("attestations", None, att_rows[s % 64:s % 64 + 1]),
                ("crosslinks", [s % 1024], ST.pack_crosslinks(donor.crosslink_epochs[s % 64:s % 64 + 1],
                                                              donor.crosslink_roots[s % 64:s % 64 + 1]))], \
            st.scalars["Slot"] + s + 1

    def apply_set(ch, slot):
        for name, idx, rows in ch:
            ts.append(name, rows) if idx is None else ts.update(name, idx, rows)
        ts.set_scalar("Slot", slot)

    def slot_set_root(ch, slot):
        apply_set(ch, slot)
        t0 = time.perf_counter()
        r = ts.root()
        return r, time.perf_counter() - t0

    def slot_set(ch, slot):
        t0 = time.perf_counter()
        apply_set(ch, slot)
        r = ts.root()
        return r, time.perf_counter() - t0

    def slot_handles(ch, slot):
        t0 = time.perf_counter()
        for name, idx, rows in ch:
            handles[name].append(rows) if idx is None else handles[name].update(idx, rows)
        for attr in handles:
            msg[off[attr]:off[attr] + 32] = handles[attr].root()
        o = ST.CONTAINER_OFF["Slot"]
        msg[o:o + 8] = struct.pack("<Q", slot)
        r = bytes(H.hash_batch(np.frombuffer(bytes(msg), np.uint8).reshape(1, -1), len(msg))[0])
        return r, time.perf_counter() - t0

    def slot_resident(ch, slot):
        for name, idx, rows in ch:
            rs.append(name, rows) if idx is None else rs.update(name, idx, rows)
        rs.set_scalar("Slot", slot)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = rs.root()
        return r, time.perf_counter() - t0

    variants = {"set_root": slot_set_root, "set_slot": slot_set, "ten_handles": slot_handles,
                "resident_root": slot_resident}

    def one_slot(timed_name):
        """Every holder takes the slot (they must stay the same state); only `timed_name`'s time is kept."""
        ch, slot = change()
        roots, t = {}, None
        for name, fn in (("set", variants[timed_name] if timed_name.startswith("set") else slot_set),
                         ("ten_handles", slot_handles), ("resident_root", slot_resident)):
            roots[name], dt = fn(ch, slot)
            if name == timed_name or (name == "set" and timed_name.startswith("set")):
                t = dt
        assert len(set(roots.values())) == 1, f"the roots of slot {slot} differ: {roots}"
        return t

    for _ in range(3):  # warm-up; the attestation trees double their capacity here
        one_slot("set_slot")
    samples = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name in variants:
            samples[name].append(1e3 * statistics.mean(one_slot(name) for _ in range(args.slots)))
    row = {"validators": nv, "slots_per_round": args.slots, "ms": {}, "ms_min": {}, "ms_max": {}}
    for name in variants:
        row["ms"][name] = round(statistics.median(samples[name]), 4)
        row["ms_min"][name] = round(min(samples[name]), 4)
        row["ms_max"][name] = round(max(samples[name]), 4)

    def beats(a, b):
        spread = max(row["ms_max"][n] - row["ms_min"][n] for n in (a, b))
        return row["ms"][b] - row["ms"][a] > spread

    row["set_slot_beats_ten_handles"] = beats("set_slot", "ten_handles")
    row["ten_handles_beats_set_slot"] = beats("ten_handles", "set_slot")
    row["set_root_beats_resident_root"] = beats("set_root", "resident_root")
    row["resident_root_beats_set_root"] = beats("resident_root", "set_root")
    result = {"tool": "tree_set_probe", "version": _lib.load().mk_version().decode(), "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "clocks_pinned": False, "state": row}
    line = json.dumps(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
