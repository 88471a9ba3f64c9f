#!/usr/bin/env python3
"""Two resident trees diffed on the device: what the descent
costs, beside the read-back of one side, a clone and a flat device compare.

  python tools/tree_diff_probe.py [--out profiles/tree_diff/probe.json] [--quick]

  registry  2^20 ValidatorRecords in torch buffers against a copy with 16
            scattered records changed: mk_dev_ssz_trees_diff (device events);
            the same pair with every 32nd record changed (the dense end); a
            flat compare of the two level-0 arrays, torch.ne(...).nonzero()
  list      2^24 x 32-B items against a copy with 16 scattered items changed:
            mk_dev_ssz_trees_diff and the flat compare of the items
  set       BeaconTreeSet of a 2^20-validator state against its clone after one
            slot's changes: diff() (host wall time: two flushes, one launch,
            one read-back) against items("registry") of one side and clone()
The condition fixed before the run: set.diff is faster than
set.registry_readback.  The ratios to the flat compare and to clone() are
reported, not gated.  One process, `rounds` interleaved rounds after one dropped
warm-up round; `ms` is the median, `ms_min` / `ms_max` the spread.  The clocks
are not pinned.  Every diff timed is checked against the changed indices.
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

SEED = 0x5EED000000000000 + 5050


def stat(xs):
    return {"ms": round(statistics.median(xs), 4), "ms_min": round(min(xs), 4), "ms_max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_diff", "probe.json"))
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()

    import numpy as np
    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D
    from prysm_amd import registry as R
    from prysm_amd import state as ST

    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise SystemExit("tree_diff_probe needs a gfx950 device (no CPU fallback)")
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

    mk = lambda nbytes: torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=dev)  # noqa: E731
    out = {"probe": "tree_diff", "rounds": rounds, "quick": bool(args.quick)}

    def scattered(n, k=16):
        return sorted({int(x) for x in np.random.default_rng(n + k).integers(0, n, size=k)})

    def timed(desc_of, sides, flat):
        """{name: (a, b, want)}: the diff of each pair (device events), checked, and the flat compare."""
        reports = mk(16)
        slots = torch.zeros(max(max(len(w) for _, _, w in sides.values()), 1), dtype=torch.int64, device=dev)
        t = {name: [] for name in sides}
        tf = []
        for r in range(rounds + 1):  # the first round warms up and is dropped
            for name, (a, b, want) in sides.items():
                desc = desc_of(a, b, slots)
                t[name].append(events(lambda: D.trees_diff([desc], reports=reports)))
                total, first = D.diff_reports(reports)[0]
                assert total == len(want) and first == want[0], (name, total, first)
                assert sorted(int(x) for x in slots[:total].cpu().numpy()) == want, name
            tf.append(events(flat))
        res = {name: stat(v[1:]) for name, v in t.items()}
        res["flat_compare"] = stat(tf[1:])
        for name in sides:
            res[f"flat_to_{name}"] = round(res["flat_compare"]["ms"] / res[name]["ms"], 2)
        return res

    # ---- the registry tree: 16 scattered records, and every 32nd
    recs = R.synthetic_registry(nreg, SEED).records
    bws = mk(D.struct_list_tree_build_workspace_bytes(nreg, R.VALIDATOR_FIELDS))

    def reg_tree(changed):
        x = recs.copy()
        x["exit_epoch"][np.asarray(changed, dtype=np.int64)] ^= 1
        items, l0, lv, root = mk(nreg * 160 + 16), mk(32 * nreg), mk(D.list_tree_levels_bytes(nreg, 32)), mk(32)
        items[: nreg * 160] = torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).to(dev)
        D.struct_list_tree_build(items, nreg, nreg, 160, R.VALIDATOR_FIELDS, l0, lv, root, ws=bws)
        return items, l0, lv

    few, dense = scattered(nreg), list(range(5, nreg, 32))
    base, tfew, tdense = reg_tree([]), reg_tree(few), reg_tree(dense)
    reg_desc = lambda a, b, slots: D.TreeDiffArgs(_lib.MK_TREE_STRUCT, 160, a[0], a[2], nreg, nreg, b[0], b[2], nreg,  # noqa: E731
                                                  nreg, idx_out=slots, a_level0=a[1], b_level0=b[1])
    va, vb = base[1][: 32 * nreg].view(-1, 32), tfew[1][: 32 * nreg].view(-1, 32)
    out["registry"] = dict(n=nreg, **timed(reg_desc, {"diff_16": (base, tfew, few), "diff_every_32nd": (base, tdense, dense)},
                                           lambda: torch.ne(va, vb).any(dim=1).nonzero()))
    del base, tfew, tdense, va, vb, bws

    # ---- a list of 32-byte items
    host = np.random.default_rng(5).integers(0, 256, nlist * 32, dtype=np.uint8)
    lws = mk(_lib.load().mk_ssz_list_tree_build_workspace_bytes(nlist, 32))

    def list_tree(changed):
        x = host.copy().reshape(nlist, 32)
        x[np.asarray(changed, dtype=np.int64), 3] ^= 1
        items, lv, root = mk(nlist * 32 + 16), mk(D.list_tree_levels_bytes(nlist, 32)), mk(32)
        items[: nlist * 32] = torch.from_numpy(x.reshape(-1)).to(dev)
        D.list_tree_build(items, nlist, nlist, 32, lv, root, ws=lws)
        return items, lv

    few = scattered(nlist)
    base, tfew = list_tree([]), list_tree(few)
    list_desc = lambda a, b, slots: D.TreeDiffArgs(_lib.MK_TREE_LIST, 32, a[0], a[1], nlist, nlist, b[0], b[1], nlist,  # noqa: E731
                                                   nlist, idx_out=slots)
    va, vb = base[0][: 32 * nlist].view(-1, 32), tfew[0][: 32 * nlist].view(-1, 32)
    out["list"] = dict(n=nlist, **timed(list_desc, {"diff_16": (base, tfew, few)},
                                        lambda: torch.ne(va, vb).any(dim=1).nonzero()))
    del base, tfew, va, vb, host, lws

    # ---- the whole state against its clone after one slot's changes, handle form
    st = ST.synthetic_state(nreg, SEED + 1, n_attestations=128, n_batched=16, n_votes=4,
                            lists_len=64 if args.quick else 8192, shards=64 if args.quick else 1024)
    ts = ST.beacon_tree_set(st)
    ts.root()
    c = ts.clone()
    bi = np.array(scattered(nreg, 8))
    c.update("balances", bi, (st.balances[bi] + 1).astype("<u8"))
    rec = st.registry.records.copy()
    ri = scattered(nreg, 4)
    rec["exit_epoch"][ri] ^= 1
    c.update("registry", ri, rec[ri])
    slot = st.scalars["Slot"] % len(st.latest_block_roots)
    c.update("latest_block_roots", [slot], np.full((1, 32), 0x77, dtype=np.uint8))
    c.update("randao_mixes", [slot % len(st.randao_mixes)], np.full((1, 32), 0x55, dtype=np.uint8))
    c.set_scalar("Slot", st.scalars["Slot"] + 1)
    c.root()
    td, tr, tc = [], [], []
    for r in range(rounds + 1):
        ms, got = wall(lambda: ts.diff(c))
        assert [int(x) for x in got[ts.tree["registry"]][0]] == ri and got[ts.tree["balances"]][1] == len(bi)
        assert got[ts.tree["latest_block_roots"]][1] == 1 and got["container"][0] >= 1
        td.append(ms)
        tr.append(wall(lambda: ts.items("registry"))[0])
        ms, k = wall(ts.clone)
        tc.append(ms)
        del k
    d, rb = statistics.median(td[1:]), statistics.median(tr[1:])
    out["set"] = {"validators": nreg, "diff": stat(td[1:]), "registry_readback": stat(tr[1:]), "clone": stat(tc[1:]),
                  "readback_to_diff": round(rb / d, 2), "clone_to_diff": round(statistics.median(tc[1:]) / d, 2),
                  "diff_faster_than_readback": bool(d < rb)}

    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if not args.quick and not d < rb:
        raise SystemExit("the set's diff is not faster than the read-back of its registry")


if __name__ == "__main__":
    main()
