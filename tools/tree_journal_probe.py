#!/usr/bin/env python3
"""Checkpoints of a tree set: what journaling costs a slot, what a roll back
costs beside copy_from of a clone, and the HBM the journal holds (DESIGN.md
§5r; the state and the slot of tools/tree_set_probe.py).

  python tools/tree_journal_probe.py [--parent-lib PATH] [--out profiles/tree_journal/probe.json] [--quick]

The state is synthetic_state(2^20 validators), the change set of one slot §5h's.
  parent_slot / this_slot   ms per slot of mk_tree_set_root with NO checkpoint open, the parent commit's
                            library (--parent-lib, named to a child by PRYSM_MERKLE_LIB) and this one's in
                            alternation: a child process per library and round, because one Python process
                            binds one library.  The bar: this_slot's median is not above parent_slot's maximum.
  slot_no_checkpoint        the same slot in this process, as the base of the next line
  slot_checkpoint_open      the same slot with one checkpoint open: the difference is the cost of journaling
  rollback_1 / rollback_32  mk_tree_set_rollback over 1 and over 32 slots
  copy_from_1 / _32         mk_tree_set_copy from a clone taken before the slots: what the parent can do instead
  journal_bytes_32          journal_bytes() after 32 slots, beside 32 x the bytes of one clone (from the capacities)
time.perf_counter, `rounds` interleaved rounds; `ms` is the median round, `ms_min` / `ms_max` the spread.  The
clocks are not pinned.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x5EED000000000000 + 5151


def make(quick):
    import numpy as np

    from prysm_amd import state as ST

    nv = 1 << 12 if quick else 1 << 20
    st = ST.synthetic_state(nv, SEED)
    donor = ST.synthetic_state(64, SEED + 1, n_attestations=64, n_batched=0, lists_len=64, shards=64)
    att_rows = ST.pack_attestations(donor.attestations, 48)[0]
    ts = ST.beacon_tree_set(st)
    ts.reserve("attestations", ts.count("attestations") + 4096)  # no slot of the probe outgrows a tree
    u8 = lambda a: np.ascontiguousarray(a).view(np.uint8)  # noqa: E731
    rng = np.random.default_rng(3)
    no = [0]

    def slot(timed=True):
        """The next slot applied; the seconds of its root()."""
        s = no[0]
        no[0] += 1
        at = (st.scalars["Slot"] + s) % 8192
        ts.update("latest_block_roots", [at], donor.latest_block_roots[s % 64:s % 64 + 1])
        ts.update("randao_mixes", [at], donor.randao_mixes[s % 64:s % 64 + 1])
        ts.update("balances", rng.choice(nv, 3, replace=False), u8(donor.balances[:3].astype("<u8")))
        ts.update("registry", rng.choice(nv, 2, replace=False), donor.registry.records[2 * (s % 32):2 * (s % 32) + 2])
        ts.append("attestations", att_rows[s % 64:s % 64 + 1])
        ts.update("crosslinks", [s % 1024], ST.pack_crosslinks(donor.crosslink_epochs[s % 64:s % 64 + 1],
                                                               donor.crosslink_roots[s % 64:s % 64 + 1]))
        ts.set_scalar("Slot", st.scalars["Slot"] + s + 1)
        t0 = time.perf_counter()
        ts.root()
        return time.perf_counter() - t0

    for _ in range(4):
        slot()
    return ts, slot, nv


def child(args):
    """One round of the no-checkpoint slot with the library the environment names: ms per slot on stdout."""
    ts, slot, _nv = make(args.quick)
    print(json.dumps({"ms": 1e3 * statistics.mean(slot() for _ in range(args.slots))}))


def stats(xs):
    return {"ms": round(statistics.median(xs), 4), "ms_min": round(min(xs), 4), "ms_max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_journal", "probe.json"))
    ap.add_argument("--parent-lib", default=None, help="libprysm_merkle.so built from the parent commit")
    ap.add_argument("--quick", action="store_true", help="a small registry (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)

    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D
    from prysm_amd import state as ST

    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise SystemExit("tree_journal_probe needs a gfx950 device (no CPU fallback)")

    # 1. no checkpoint open: the parent's library and this one's, a child each, in alternation
    ab = {"parent_slot": [], "this_slot": []}
    if args.parent_lib:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--slots", str(args.slots)] + (["--quick"] if args.quick else [])
        for _ in range(args.rounds):
            for name, lib in (("parent_slot", os.path.abspath(args.parent_lib)), ("this_slot", None)):
                env = dict(os.environ)
                env.pop("PRYSM_MERKLE_LIB", None)
                if lib:
                    env["PRYSM_MERKLE_LIB"] = lib
                out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, check=True).stdout
                ab[name].append(json.loads(out.strip().splitlines()[-1])["ms"])

    # 2-4. this process
    ts, slot, nv = make(args.quick)
    clone = ts.clone()
    samples = {k: [] for k in ("slot_no_checkpoint", "slot_checkpoint_open", "rollback_1", "copy_from_1", "rollback_32",
                               "copy_from_32")}
    held = []

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)

    for _ in range(args.rounds):
        samples["slot_no_checkpoint"].append(1e3 * statistics.mean(slot() for _ in range(args.slots)))
        cp = ts.checkpoint()
        samples["slot_checkpoint_open"].append(1e3 * statistics.mean(slot() for _ in range(args.slots)))
        ts.release(cp)
        for n in (1, 32):
            cp, root = ts.checkpoint(), ts.root()
            for _ in range(n):
                slot()
            if n == 32:
                held.append(ts.journal_bytes())
            samples[f"rollback_{n}"].append(timed(lambda: ts.rollback(cp)))
            assert ts.root() == root, "the roll back did not return to the checkpoint's root"
            clone.copy_from(ts)
            for _ in range(n):
                slot()
            samples[f"copy_from_{n}"].append(timed(lambda: ts.copy_from(clone)))
            assert ts.root() == root, "copy_from did not return to the clone's root"
    clone_bytes = 0
    for attr, _name, kind, item_len, _spec in ST.RESIDENT_TREES:
        cap = ts.capacity(attr)
        leaf = item_len if kind == _lib.MK_TREE_LIST else 32
        clone_bytes += cap * item_len + (0 if kind == _lib.MK_TREE_LIST else 32 * cap) + D.list_tree_levels_bytes(cap, leaf)
    row = {"validators": nv, "slots_per_round": args.slots}
    for k, xs in list(ab.items()) + list(samples.items()):
        row[k] = stats(xs) if xs else None
    if ab["parent_slot"]:
        row["this_median_not_above_parent_max"] = row["this_slot"]["ms"] <= row["parent_slot"]["ms_max"]
    row["journaling_ms_per_slot"] = round(row["slot_checkpoint_open"]["ms"] - row["slot_no_checkpoint"]["ms"], 4)
    row["journal_bytes_32"] = int(statistics.median(held))
    row["clone_bytes"] = int(clone_bytes)
    row["clone_bytes_x32"] = int(32 * clone_bytes)
    result = {"tool": "tree_journal_probe", "version": _lib.load().mk_version().decode(), "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "clocks_pinned": False, "state": row}
    line = json.dumps(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
