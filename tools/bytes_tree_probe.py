#!/usr/bin/env python3
"""Device-resident bytes tree ([][32]byte): update, append and build times
beside the composition of the existing entry points and the one-shot
TreeHash, in one process (the method of
tools/struct_tree_probe.py).

  python tools/bytes_tree_probe.py [--out profiles/bytes_tree/probe.json] [--quick]

Two lists of 32-B elements: 2^24 elements, and the 8 192 of the state's root
arrays.  k random in-place elements (1, 16, 256, 4096, 16384, 32768, 65536,
and the powers of two from 2^9 to 2^18, to find where an update stops being
cheaper than a build) and an append of 4096:
  a  tree_update_k*   mk_dev_ssz_bytes_list_tree_update (elements pre-written)
  b  existing_k*      mk_dev_hash_batch over the k 36-B messages le32(32) || e,
                      then mk_dev_ssz_list_tree_update with those digests as
                      d_values (what a caller could do before this tree)
  c  one_shot         mk_dev_ssz_tree_hash_bytes_list of the whole list
  d  tree_build       mk_dev_ssz_bytes_list_tree_build
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

SEED = 0x5EED000000000000 + 4545
KS = (1, 16, 256, 4096, 16384, 32768, 65536)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bytes_tree", "probe.json"))
    ap.add_argument("--quick", action="store_true", help="small lists (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D

    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise SystemExit("bytes_tree_probe needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    EL = 32

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def measure(n):
        rng = np.random.default_rng(1)
        elems = D.synth_fill(torch.empty(n * EL, dtype=torch.uint8, device=dev), SEED)
        digs = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
        lv = torch.empty(D.list_tree_levels_bytes(n, 32), dtype=torch.uint8, device=dev)
        root = torch.zeros(32, dtype=torch.uint8, device=dev)
        full = torch.zeros(32, dtype=torch.uint8, device=dev)
        ks = sorted(set(KS) | {1 << e for e in range(9, 19)})
        ks = [k for k in ks if k <= n // 4]
        napp = min(4096, n // 2)
        kmax = max(max(ks), napp)
        idx = {k: torch.from_numpy(np.sort(rng.choice(n, k, replace=False)).astype(np.int64)).to(dev) for k in ks}
        ws = torch.empty(D.bytes_list_tree_update_workspace_bytes(kmax, EL), dtype=torch.uint8, device=dev)
        bws = torch.empty(D.bytes_list_tree_build_workspace_bytes(n, EL), dtype=torch.uint8, device=dev)
        fws = D.tree_hash_bytes_list_workspace(n, EL, dev)
        # (b): the k messages le32(32) || e side by side, as a caller of the existing entry points holds them
        kmsg = {}
        for k in ks:
            msg = torch.zeros((k, 4 + EL), dtype=torch.uint8, device=dev)
            msg[:, 0] = EL
            msg[:, 4:] = elems.view(n, EL)[idx[k]]
            kmsg[k] = msg.reshape(-1).contiguous()
        kdig = torch.empty(32 * kmax, dtype=torch.uint8, device=dev)
        lws = torch.empty(D.list_tree_update_workspace_bytes(kmax), dtype=torch.uint8, device=dev)

        def existing(k):
            D.hash_batch(kmsg[k], k, 4 + EL, out=kdig)
            D.list_tree_update(digs, n, n, n, 32, lv, root, idx[k], k, kdig, ws=lws)

        def update(k):
            D.bytes_list_tree_update(elems, n, n, n, EL, digs, lv, root, idx[k], k, None, ws=ws)

        variants = {"one_shot": lambda: D.tree_hash_bytes_list(elems, n, EL, out=full, ws=fws),
                    "tree_build": lambda: D.bytes_list_tree_build(elems, n, n, EL, digs, lv, root, ws=bws)}
        for k in ks:
            variants[f"tree_update_k{k}"] = (lambda k=k: update(k))
            if k in KS:
                variants[f"existing_k{k}"] = (lambda k=k: existing(k))
        variants[f"tree_append_{napp}"] = lambda: D.bytes_list_tree_update(elems, n - napp, n, n, EL, digs, lv, root,
                                                                           None, 0, None, ws=ws)
        variants["tree_build"]()  # the updates below climb a built tree
        variants["one_shot"]()
        torch.cuda.synchronize()
        want = bytes(full.cpu().numpy())
        reps = {}
        for name, fn in variants.items():  # warm-up, a root check, and a repeat count for >= ~50 ms per round
            root.zero_()
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            if name != "one_shot":
                assert bytes(root.cpu().numpy()) == want, f"{name}: root differs from the one-shot root"
            ms = timed(fn, 3)
            reps[name] = max(3, min(200, int(50.0 / max(ms, 1e-3))))
        samples = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                samples[name].append(timed(fn, reps[name]))
        row = {"n": n, "elem_len": EL, "ms": {}, "ms_min": {}, "ms_max": {}, "reps": reps}
        for name in variants:
            row["ms"][name] = round(statistics.median(samples[name]), 5)
            row["ms_min"][name] = round(min(samples[name]), 5)
            row["ms_max"][name] = round(max(samples[name]), 5)

        def spread(name):
            return row["ms_max"][name] - row["ms_min"][name]

        # the tree's update against (b): a win only by more than the larger spread of the two
        row["tree_beats_existing"] = {
            str(k): row["ms"][f"existing_k{k}"] - row["ms"][f"tree_update_k{k}"] > max(spread(f"existing_k{k}"),
                                                                                    spread(f"tree_update_k{k}"))
            for k in ks if k in KS}
        below = [k for k in ks if row["ms"][f"tree_update_k{k}"] < row["ms"]["tree_build"]]
        row["largest_k_cheaper_than_build"] = max(below) if below else 0
        row["k1_faster_than_one_shot"] = (row["ms"]["one_shot"] - row["ms"]["tree_update_k1"]
                                          > max(spread("one_shot"), spread("tree_update_k1")))
        return row

    sizes = [1 << 14, 1 << 10] if args.quick else [1 << 24, 8192]
    result = {"tool": "bytes_tree_probe", "version": _lib.load().mk_version().decode(), "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "lists": [measure(n) for n in sizes]}
    line = json.dumps(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
