#!/usr/bin/env python3
"""Resident trees audited on the device: what the audit costs,
beside the build of the same tree and the read-back of the same list.

  python tools/tree_audit_probe.py [--out profiles/tree_audit/probe.json] [--quick]

  registry  2^20 ValidatorRecords in torch buffers: mk_dev_ssz_trees_audit
            against mk_dev_ssz_struct_list_tree_build of the same tree (device
            events), and records() of a StructListTree of the same records
            (host wall time)
  list      2^24 x 32-B items: mk_dev_ssz_trees_audit against
            mk_dev_ssz_list_tree_build, and items() of a ListTree
  set       BeaconTreeSet of a 2^20-validator state: audit() (host wall time,
            flush, launch chain, one read-back) against items("registry"), the
            read-back of its registry alone
The condition fixed before the run: set.audit is faster than set.registry_readback.
The audit-to-build ratio is reported, not gated.  One process, `rounds`
interleaved rounds after one dropped warm-up round; `ms` is the median, `ms_min`
/ `ms_max` the spread.  The clocks are not pinned.  Every audit timed is a clean
one, checked.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x5EED000000000000 + 4949


def stat(xs):
    return {"ms": round(statistics.median(xs), 4), "ms_min": round(min(xs), 4), "ms_max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_audit", "probe.json"))
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
        raise SystemExit("tree_audit_probe needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    nreg = 1 << (12 if args.quick else 20)
    nlist = 1 << (14 if args.quick else 24)
    rounds = args.rounds
    clean = (0, _lib.MK_AUDIT_NONE, (1 << 64) - 1)

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

    mk = lambda nbytes: torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=dev)  # noqa: E731
    out = {"probe": "tree_audit", "rounds": rounds, "quick": bool(args.quick)}

    def device_pair(desc, build, read):
        """audit and build of one tree in torch buffers (device events), the handle's read-back (wall)."""
        ws = mk(D.trees_audit_workspace_bytes([desc]))
        reports = mk(48)
        ta, tb, tr = [], [], []
        for r in range(rounds + 1):  # the first round warms up and is dropped
            tb.append(events(build))
            ta.append(events(lambda: D.trees_audit([desc], reports=reports, ws=ws)))
            assert D.audit_reports(reports) == [clean, clean]
            tr.append(wall(read)[0])
        a, b = statistics.median(ta[1:]), statistics.median(tb[1:])
        return {"audit": stat(ta[1:]), "build": stat(tb[1:]), "readback": stat(tr[1:]), "audit_to_build": round(a / b, 3)}

    # ---- the registry tree
    recs = R.synthetic_registry(nreg, SEED).records
    items, l0, lv, root = mk(nreg * 160 + 16), mk(32 * nreg), mk(D.list_tree_levels_bytes(nreg, 32)), mk(32)
    items[: nreg * 160] = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(dev)
    bws = mk(D.struct_list_tree_build_workspace_bytes(nreg, R.VALIDATOR_FIELDS))
    h = LT.StructListTree(160, R.VALIDATOR_FIELDS, capacity=nreg)
    h.assign(recs)
    out["registry"] = dict(n=nreg, **device_pair(
        D.TreeAuditArgs(_lib.MK_TREE_STRUCT, items, nreg, nreg, 160, lv, root, level0=l0, spec=R.VALIDATOR_FIELDS),
        lambda: D.struct_list_tree_build(items, nreg, nreg, 160, R.VALIDATOR_FIELDS, l0, lv, root, ws=bws),
        h.records))
    assert h.audit() == clean
    del h, items, l0, lv, bws

    # ---- a list of 32-byte items
    host = np.random.default_rng(5).integers(0, 256, nlist * 32, dtype=np.uint8)
    items, lv, root = mk(nlist * 32 + 16), mk(D.list_tree_levels_bytes(nlist, 32)), mk(32)
    items[: nlist * 32] = torch.from_numpy(host).to(dev)
    bws = mk(_lib.load().mk_ssz_list_tree_build_workspace_bytes(nlist, 32))
    h = LT.ListTree(32, capacity=nlist)
    h.assign(host)
    out["list"] = dict(n=nlist, **device_pair(
        D.TreeAuditArgs(_lib.MK_TREE_LIST, items, nlist, nlist, 32, lv, root),
        lambda: D.list_tree_build(items, nlist, nlist, 32, lv, root, ws=bws), h.items))
    del h, items, lv, host, bws

    # ---- the whole state, handle form
    st = ST.synthetic_state(nreg, SEED + 1, n_attestations=128, n_batched=16, n_votes=4,
                            lists_len=64 if args.quick else 8192, shards=64 if args.quick else 1024)
    ts = ST.beacon_tree_set(st)
    ts.root()
    ta, tr = [], []
    for r in range(rounds + 1):
        ms, got = wall(ts.audit)
        assert got == [clean] * (len(ts) + 1)
        ta.append(ms)
        tr.append(wall(lambda: ts.items("registry"))[0])
    a, rb = statistics.median(ta[1:]), statistics.median(tr[1:])
    out["set"] = {"validators": nreg, "audit": stat(ta[1:]), "registry_readback": stat(tr[1:]),
                  "audit_faster_than_readback": bool(a < rb)}

    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not args.quick and not a < rb:
        raise SystemExit("the set's audit is not faster than the read-back of its registry")


if __name__ == "__main__":
    main()
