#!/usr/bin/env python3
"""Device-resident registry tree: update, append and build times beside the
composition of the existing entry points and the one-shot struct list root,
in one process (the method of tools/list_tree_probe.py).

  python tools/struct_tree_probe.py [--out profiles/struct_tree/probe.json] [--quick]

n = 2^20 ValidatorRecords; k random in-place records (1, 16, 256, 4096,
65536, and the powers of two between, to find where an update stops being
cheaper than a build) and an append of 4096:
  a  tree_update_k*   mk_dev_ssz_struct_list_tree_update (records pre-written)
  b  composed_k*      mk_dev_ssz_struct_roots over the k records, then
                      mk_dev_ssz_list_tree_update with those roots as d_values
  c  list_root        mk_dev_ssz_struct_list_root of the whole list
  d  tree_build       mk_dev_ssz_struct_list_tree_build
Every variant is warmed up, then timed in `rounds` interleaved rounds of
`reps` back-to-back calls between device events; `ms` is the median round's
ms per call, `ms_min` / `ms_max` the spread of the rounds.  Every timed root
is checked against the one-shot root.  Prints one JSON line and writes it to
--out.  PRYSM_MERKLE_LIB selects a variant build; `version` records which
one ran.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x5EED000000000000 + 4343


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "struct_tree", "probe.json"))
    ap.add_argument("--quick", action="store_true", help="a small list (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D
    from prysm_amd import registry as R

    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise SystemExit("struct_tree_probe needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    n = 1 << 14 if args.quick else 1 << 20
    spec, RL = R.VALIDATOR_FIELDS, 160
    rng = np.random.default_rng(1)

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    recs = R.synthetic_registry_device(n, SEED, dev)
    roots = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    lv = torch.empty(D.list_tree_levels_bytes(n, 32), dtype=torch.uint8, device=dev)
    root = torch.zeros(32, dtype=torch.uint8, device=dev)
    full = torch.zeros(32, dtype=torch.uint8, device=dev)
    ks = sorted({1, 16, 256, 4096, 65536} | {1 << e for e in range(9, 17)})
    ks = [k for k in ks if k <= n // 4]
    napp = min(4096, n // 2)
    kmax = max(max(ks), napp)
    idx = {k: torch.from_numpy(np.sort(rng.choice(n, k, replace=False)).astype(np.int64)).to(dev) for k in ks}
    ws = torch.empty(D.struct_list_tree_update_workspace_bytes(kmax, spec), dtype=torch.uint8, device=dev)
    bws = torch.empty(D.struct_list_tree_build_workspace_bytes(n, spec), dtype=torch.uint8, device=dev)
    fws = torch.empty(_lib.load().mk_ssz_struct_list_workspace_bytes(n, R._fields(spec), len(spec)) + 256,
                      dtype=torch.uint8, device=dev)
    # (b): the k records side by side, as a caller of today's entry points holds them
    krec = {k: recs.view(n, RL)[idx[k]].reshape(-1).contiguous() for k in ks}
    kroots = torch.empty(32 * kmax, dtype=torch.uint8, device=dev)
    sws = torch.empty(max(256, 144 * kmax), dtype=torch.uint8, device=dev)
    lws = torch.empty(D.list_tree_update_workspace_bytes(kmax), dtype=torch.uint8, device=dev)

    def composed(k):
        D.struct_roots(krec[k], k, RL, spec, out=kroots, ws=sws)
        D.list_tree_update(roots, n, n, n, 32, lv, root, idx[k], k, kroots, ws=lws)

    variants = {"list_root": lambda: D.struct_list_root(recs, n, RL, spec, out=full, ws=fws),
                "tree_build": lambda: D.struct_list_tree_build(recs, n, n, RL, spec, roots, lv, root, ws=bws)}
    for k in ks:
        variants[f"tree_update_k{k}"] = (lambda k=k: D.struct_list_tree_update(recs, n, n, n, RL, spec, roots, lv,
                                                                               root, idx[k], k, None, ws=ws))
        variants[f"composed_k{k}"] = (lambda k=k: composed(k))
    variants[f"tree_append_{napp}"] = lambda: D.struct_list_tree_update(recs, n - napp, n, n, RL, spec, roots, lv,
                                                                        root, None, 0, None, ws=ws)
    variants["tree_build"]()  # the updates below climb a built tree
    variants["list_root"]()
    torch.cuda.synchronize()
    want = bytes(full.cpu().numpy())
    reps = {}
    for name, fn in variants.items():  # warm-up, a root check, and a repeat count for >= ~50 ms per round
        root.zero_()
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        if name != "list_root":
            assert bytes(root.cpu().numpy()) == want, f"{name}: root differs from the one-shot root"
        ms = timed(fn, 3)
        reps[name] = max(3, min(200, int(50.0 / max(ms, 1e-3))))
    samples = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            samples[name].append(timed(fn, reps[name]))
    row = {"n": n, "record_len": RL, "ms": {}, "ms_min": {}, "ms_max": {}, "reps": reps}
    for name in variants:
        row["ms"][name] = round(statistics.median(samples[name]), 5)
        row["ms_min"][name] = round(min(samples[name]), 5)
        row["ms_max"][name] = round(max(samples[name]), 5)
    # (a) beats (b) by more than the rounds' spread: the whole range of a below the whole range of b
    row["tree_beats_composed"] = {str(k): row["ms_max"][f"tree_update_k{k}"] < row["ms_min"][f"composed_k{k}"]
                                  for k in ks}
    below = [k for k in ks if row["ms"][f"tree_update_k{k}"] < row["ms"]["tree_build"]]
    row["largest_k_cheaper_than_build"] = max(below) if below else 0
    row["k1_faster_than_list_root"] = row["ms"]["tree_update_k1"] < row["ms"]["list_root"]
    result = {"tool": "struct_tree_probe", "version": _lib.load().mk_version().decode(), "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "registry": row}
    line = json.dumps(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
