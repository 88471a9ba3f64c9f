#!/usr/bin/env python3
"""hashutil.RepeatHash in batches: what a batch of chains costs
in each kernel form, beside the two routes that existed before it.

  python tools/repeat_hash_probe.py [--out profiles/repeat_hash/probe.json] [--quick]

Shapes: n in {1, 64, 1024, 2^14, 2^20} x layers in {1, 16}, layers 1024 for
n <= 1024, uniform; one skewed case, layers[i] = i % 32 at n = 2^14; and a scan
of n between 1024 and 2^14 at 16 layers, forced forms only, to place the
MK_REPEAT_AUTO threshold where they cross.  Per shape, in one process:
  lane, wave, auto   mk_dev_repeat_hash forced to each form and as AUTO picks
  base_a             the only route without it: `layers` successive
                     mk_dev_hash_batch(msg_len = 32) launches on one stream,
                     ping-pong between two buffers (the skewed case: max(layers)
                     launches over all n chains -- that route cannot mask)
  base_b             the oracle's C Keccak on one core for the same chains (at
                     most 2^17 hashes are run and the time scaled to the shape:
                     `cpu_scaled`)
Device events around `reps` back-to-back calls (reps sized so a window is
>= ~4 ms), `rounds` interleaved rounds after one dropped warm-up round; `ms`
is the median per call, `ms_min` / `ms_max` the spread.  The clocks are not
pinned.  Every form's output is compared with base_a's on the device and with
the oracle on the first chains.
The gate, fixed before the run: at every shape AUTO is no slower than base_a.
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x5EED000000000000 + 7171
CPU_HASHES = 1 << 17


def stat(xs):
    return {"ms": round(statistics.median(xs), 5), "ms_min": round(min(xs), 5), "ms_max": round(max(xs), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repeat_hash", "probe.json"))
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()

    import numpy as np
    import torch

    from oracle import oracle as O
    from prysm_amd import _lib
    from prysm_amd import device as D

    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise SystemExit("repeat_hash_probe needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    rounds = args.rounds
    big = 1 << (12 if args.quick else 20)
    mid = 1 << (10 if args.quick else 14)
    deep = 64 if args.quick else 1024

    shapes = []  # (name, n, layers or "mod32", forms)
    all_forms = ("lane", "wave", "auto")
    for n in (1, 64, 1024, mid, big):
        for layers in (1, 16) + ((deep,) if n <= 1024 else ()):
            shapes.append((f"n{n}_l{layers}", n, layers, all_forms))
    shapes.append((f"n{mid}_mod32", mid, "mod32", all_forms))
    scan = [] if args.quick else [2048, 4096, 8192]
    for n in scan:
        shapes.append((f"scan_n{n}_l16", n, 16, ("lane", "wave")))
    form_of = {"lane": _lib.MK_REPEAT_LANE, "wave": _lib.MK_REPEAT_WAVE, "auto": _lib.MK_REPEAT_AUTO}

    def events(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    seeds_all = torch.empty(big * 32, dtype=torch.uint8, device=dev)
    D.synth_fill(seeds_all, SEED)
    out = {"probe": "repeat_hash", "rounds": rounds, "quick": bool(args.quick), "shapes": {}}
    failed = []
    for name, n, layers, forms in shapes:
        lay_np = (np.arange(n) % 32 if layers == "mod32" else np.full(n, layers)).astype(np.int32)
        lmax = int(lay_np.max())
        seeds = seeds_all[: n * 32]
        d_lay = torch.from_numpy(lay_np).to(dev)
        res = torch.empty(n * 32, dtype=torch.uint8, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ping = [torch.empty(n * 32, dtype=torch.uint8, device=dev) for _ in range(2)]

        def chain(form):
            D.repeat_hash(seeds, d_lay, n, lmax, form, out=res, status=status)

        def base_a():
            src = seeds
            for t in range(lmax):
                D.hash_batch(src, n, 32, out=ping[t & 1])
                src = ping[t & 1]

        # ---- results first: every form against base_a (uniform shapes) and the oracle
        base_a()
        want_dev = ping[(lmax - 1) & 1].clone()
        k = min(n, 64)
        host_seeds = seeds[: k * 32].cpu().numpy().reshape(k, 32)
        want = host_seeds.copy()
        for t in range(lmax):
            nxt = O.keccak256_batch(np.ascontiguousarray(want), 32).reshape(k, 32)
            live = lay_np[:k] > t
            want[live] = nxt[live]
        for f in forms:
            res.zero_()
            chain(form_of[f])
            torch.cuda.synchronize()
            assert int(status.item()) == 0, (name, f)
            assert np.array_equal(res[: k * 32].cpu().numpy().reshape(k, 32), want), (name, f)
            if layers != "mod32":
                assert torch.equal(res, want_dev), (name, f)

        # ---- timings
        variants = {f: (lambda f=f: chain(form_of[f])) for f in forms}
        if "auto" in forms:
            variants["base_a"] = base_a
        one = max(events(fn, 1) for fn in variants.values())
        reps = int(min(400, max(1, math.ceil(4.0 / max(one, 1e-3)))))
        t = {v: [] for v in variants}
        for r in range(rounds + 1):  # the first round warms up and is dropped
            for v, fn in variants.items():
                t[v].append(events(fn, reps))
        row = {"n": n, "layers": layers, "hashes": int(lay_np.sum()), "reps": reps}
        row.update({v: stat(x[1:]) for v, x in t.items()})
        if "auto" in forms:
            # one core of the CPU, the oracle's C port: at most CPU_HASHES hashes, scaled
            kc = max(1, min(n, CPU_HASHES // max(lmax, 1)))
            x0 = seeds[: kc * 32].cpu().numpy().reshape(kc, 32)
            tc = []
            for _ in range(3):
                x = x0
                t0 = time.perf_counter()
                for _t in range(lmax):
                    x = O.keccak256_batch(x, 32)
                tc.append((time.perf_counter() - t0) * 1e3)
            ran = kc * lmax
            total = int(lay_np.sum())
            row["base_b"] = {"ms": round(statistics.median(tc) * total / ran, 4), "cpu_scaled": total != ran,
                             "hashes_run": ran}
            row["base_a_to_auto"] = round(row["base_a"]["ms"] / row["auto"]["ms"], 2)
            row["base_b_to_auto"] = round(row["base_b"]["ms"] / row["auto"]["ms"], 1)
            row["gate_ok"] = bool(row["auto"]["ms"] <= row["base_a"]["ms"])
            if not row["gate_ok"]:
                failed.append(name)
        row["wave_to_lane"] = round(row["wave"]["ms"] / row["lane"]["ms"], 3)
        out["shapes"][name] = row
        print(name, json.dumps(row), file=sys.stderr, flush=True)

    # where the forced forms cross at 16 layers: the largest probed n at which the wave form is not slower
    at16 = sorted((r["n"], r["wave_to_lane"]) for r in out["shapes"].values() if r["layers"] == 16)
    not_slower = [n for n, ratio in at16 if ratio <= 1.0]
    out["crossing_l16"] = {"wave_to_lane": at16, "wave_not_slower_up_to": max(not_slower) if not_slower else 0}
    out["gate"] = {"rule": "auto.ms <= base_a.ms at every shape", "pass": not failed, "failed": failed}

    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    if failed and not args.quick:
        raise SystemExit(f"AUTO slower than the per-layer launches at {failed}")


if __name__ == "__main__":
    main()
