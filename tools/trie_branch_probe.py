#!/usr/bin/env python3
"""Deposit trie: batched branches as of a past count, and the batched deposit
verifier, each beside what a caller had before them, in one process
(the method of tools/bytes_tree_probe.py).

  python tools/trie_branch_probe.py [--out profiles/trie_branches/probe.json] [--quick]

A 2^20-deposit trie of 280-B deposits at depth 32, resident on the device.
  dev_*    device forms on the current stream, between device events
  host_*   handle / host-buffer forms, which synchronize themselves: wall clock
a  16 branches at as_of == count, one call   | 16 single-branch calls
b  16 branches + root at as_of = count - 1, count / 2 + 1 (odd: the longest
   chain, 32 permutations) and count / 2 (a power of two: the chain starts at
   level 19, 13 permutations)                | mk_dev_deposit_trie_build over
   the first as_of deposits, then 16 single-branch calls on that trie
c  2^16 branches in one call, GB/s of branch bytes written, with no chain
   (as_of == count) and with the longest one (every workgroup walks it)
d  mk_dev_verify_deposits, n = 16 and 2^16   | mk_dev_hash_batch_var alone (the
   existing verifier has no device form), and as host forms mk_verify_deposits
   | mk_hash_batch_var + mk_verify_merkle_branches
Every variant is warmed up, then timed in `rounds` interleaved rounds of `reps`
back-to-back calls; `ms` is the median round's ms per call, `ms_min` / `ms_max`
the spread.  The process reads no oracle: results are only cross-checked
against each other (batched against single branches, rebuilt tries' roots
against root_at, every verified deposit accepted).  Prints one JSON line and
writes it to --out.
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

SEED = 0x5EED000000000000 + 3232
DL, DEPTH = 280, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trie_branches", "probe.json"))
    ap.add_argument("--quick", action="store_true", help="a 2^12-deposit trie (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D

    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise SystemExit("trie_branch_probe needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    n = 1 << (12 if args.quick else 20)
    kbulk = min(1 << 16, n)
    u8 = dict(dtype=torch.uint8, device=dev)

    def ev_timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def _vp(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def wall_timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / reps

    data = D.synth_fill(torch.empty(n * DL, **u8), SEED)
    lv = torch.zeros(D.deposit_trie_levels_bytes(n, DEPTH), **u8)
    lv2 = torch.zeros(D.deposit_trie_levels_bytes(n, DEPTH), **u8)
    root, root2, root_at = (torch.zeros(32, **u8) for _ in range(3))
    D.deposit_trie_build(lv, n, data, n, DL, DEPTH, DEPTH, root)
    rng = np.random.default_rng(1)
    as_ofs = {"count": n, "count-1": n - 1, "count/2+1": n // 2 + 1, "count/2": n // 2}
    idx16 = {name: np.sort(rng.choice(c, 16, replace=False)).astype(np.int64) for name, c in as_ofs.items()}
    d_idx16 = {name: torch.from_numpy(v).to(dev) for name, v in idx16.items()}
    out16 = torch.zeros(16 * DEPTH * 32, **u8)
    one16 = torch.zeros(16 * DEPTH * 32, **u8)
    d_bulk = torch.from_numpy(rng.integers(0, n, size=kbulk).astype(np.int64)).to(dev)
    out_bulk = torch.zeros(kbulk * DEPTH * 32, **u8)

    def batched(name):
        D.deposit_trie_branches(lv, n, n, DEPTH, as_ofs[name], d_idx16[name], out=out16, root_at=root_at)

    def singles(levels, count, name):
        for j, i in enumerate(idx16[name]):
            D.deposit_trie_branch(levels, n, count, DEPTH, int(i), out=one16[j * DEPTH * 32:(j + 1) * DEPTH * 32])

    def rebuild_then_singles(name):
        D.deposit_trie_build(lv2, n, data, as_ofs[name], DL, DEPTH, DEPTH, root2)
        singles(lv2, as_ofs[name], name)

    # the handle over the same deposits (host data in, host branches out)
    host = data.cpu().numpy()
    offs = (np.arange(n + 1, dtype=np.uint64) * DL)
    h = ctypes.c_void_p()
    _lib.invoke("mk_deposit_trie_new", DEPTH, n, ctypes.byref(h))
    _lib.invoke("mk_deposit_trie_append", h, _vp(host), _vp(offs), n)
    h_idx16 = {name: v.astype(np.uint64) for name, v in idx16.items()}
    h_out16 = np.zeros(16 * DEPTH * 32, dtype=np.uint8)
    h_one16 = np.zeros(16 * DEPTH * 32, dtype=np.uint8)
    h_root_at = np.zeros(32, dtype=np.uint8)

    def host_batched(name):
        _lib.invoke("mk_deposit_trie_branches", h, as_ofs[name], _vp(h_idx16[name]), 16, _vp(h_out16), _vp(h_root_at))

    def host_singles():
        for j, i in enumerate(idx16["count"]):
            _lib.invoke("mk_deposit_trie_branch", h, int(i), _vp(h_one16[j * DEPTH * 32:]))

    # verifier inputs: the first nv deposits, their branches as of `count`, the shared root
    nvs = (16, kbulk)
    d_offs = torch.from_numpy(offs[:kbulk + 1].astype(np.int64)).to(dev)
    d_vidx = torch.arange(kbulk, dtype=torch.int64, device=dev)
    vbr = D.deposit_trie_branches(lv, n, n, DEPTH, n, d_vidx)
    digs = torch.zeros(kbulk * 32, **u8)
    ok = torch.zeros(kbulk, **u8)
    h_vbr = vbr.cpu().numpy()
    h_root = bytes(root.cpu().numpy())
    h_idx = np.arange(kbulk, dtype=np.uint64)
    h_roots = np.tile(np.frombuffer(h_root, dtype=np.uint8), kbulk)
    h_leaves = np.zeros(kbulk * 32, dtype=np.uint8)
    h_ok = np.zeros(kbulk, dtype=np.uint8)

    def dev_verify(nv):
        D.verify_deposits(data, d_offs, vbr, d_vidx, nv, DEPTH, root, 0, out=ok)

    def dev_hash_var(nv):
        _lib.invoke("mk_dev_hash_batch_var", D._p(data), D._p(d_offs), nv, D._p(digs), D._stream(dev), device=0)

    def host_verify_new(nv):
        _lib.invoke("mk_verify_deposits", _vp(host), _vp(offs), _vp(h_vbr), _vp(h_idx), nv, DEPTH, DEPTH, _vp(h_roots),
                    0, _vp(h_ok))
        return h_ok[:nv]

    def host_verify_old(nv):
        _lib.invoke("mk_hash_batch_var", _vp(host), _vp(offs), nv, _vp(h_leaves))
        _lib.invoke("mk_verify_merkle_branches", _vp(h_leaves), _vp(h_vbr), _vp(h_idx), nv, DEPTH, DEPTH, _vp(h_roots),
                    _vp(h_ok))
        return h_ok[:nv]

    ev, wall = {}, {}
    ev["dev_branches16_at_count"] = lambda: batched("count")
    ev["dev_single_x16_at_count"] = lambda: singles(lv, n, "count")
    for name in ("count-1", "count/2+1", "count/2"):
        ev[f"dev_branches16_root_at_{name}"] = (lambda name=name: batched(name))
        ev[f"dev_rebuild_single_x16_at_{name}"] = (lambda name=name: rebuild_then_singles(name))
    ev["dev_bulk_no_chain"] = lambda: D.deposit_trie_branches(lv, n, n, DEPTH, n, d_bulk, out=out_bulk)
    ev["dev_bulk_longest_chain"] = lambda: D.deposit_trie_branches(lv, n, n, DEPTH, n // 2 + 1, d_bulk, out=out_bulk)
    for nv in nvs:
        ev[f"dev_verify_deposits_n{nv}"] = (lambda nv=nv: dev_verify(nv))
        ev[f"dev_hash_batch_var_n{nv}"] = (lambda nv=nv: dev_hash_var(nv))
        wall[f"host_verify_deposits_n{nv}"] = (lambda nv=nv: host_verify_new(nv))
        wall[f"host_hash_var_then_verify_branches_n{nv}"] = (lambda nv=nv: host_verify_old(nv))
    wall["host_branches16_at_count"] = lambda: host_batched("count")
    wall["host_single_x16_at_count"] = host_singles
    for name in ("count-1", "count/2+1", "count/2"):
        wall[f"host_branches16_at_{name}"] = (lambda name=name: host_batched(name))

    # cross-checks (no oracle in this process)
    batched("count")
    singles(lv, n, "count")
    torch.cuda.synchronize()
    assert torch.equal(out16, one16), "batched branches differ from 16 single branches"
    host_batched("count")
    host_singles()
    assert np.array_equal(h_out16, out16.cpu().numpy()) and np.array_equal(h_one16, h_out16), "handle form differs"
    assert bytes(h_root_at) == h_root, "root_at(count) differs from the root"
    for name in ("count-1", "count/2+1", "count/2"):
        batched(name)
        rebuild_then_singles(name)
        torch.cuda.synchronize()
        assert torch.equal(out16, one16) and torch.equal(root_at, root2), f"as_of {name}: differs from the rebuilt trie"
    for nv in nvs:
        ok.zero_()
        dev_verify(nv)
        torch.cuda.synchronize()
        assert bool(ok[:nv].all()), "a deposit of the trie did not verify"
        assert host_verify_new(nv).all() and host_verify_old(nv).all()

    reps, samples = {}, {}
    for table, timed in ((ev, ev_timed), (wall, wall_timed)):
        for name, fn in table.items():  # warm-up and a repeat count for >= ~30 ms per round
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ms = timed(fn, 3)
            reps[name] = max(3, min(200, int(30.0 / max(ms, 1e-3))))
            samples[name] = []
    for _ in range(args.rounds):
        for table, timed in ((ev, ev_timed), (wall, wall_timed)):
            for name, fn in table.items():
                samples[name].append(timed(fn, reps[name]))
    res = {"tool": "trie_branch_probe", "version": _lib.load().mk_version().decode(), "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0), "deposits": n, "depth": DEPTH, "k_bulk": kbulk, "reps": reps,
           "ms": {k: round(statistics.median(v), 5) for k, v in samples.items()},
           "ms_min": {k: round(min(v), 5) for k, v in samples.items()},
           "ms_max": {k: round(max(v), 5) for k, v in samples.items()}}
    gb = kbulk * DEPTH * 32 / 1e9
    res["bulk_gb_per_s"] = {k: round(gb / (res["ms"][k] * 1e-3), 1) for k in ("dev_bulk_no_chain", "dev_bulk_longest_chain")}

    def wins(new, old):  # a win only by more than the larger spread of the two
        sp = max(res["ms_max"][new] - res["ms_min"][new], res["ms_max"][old] - res["ms_min"][old])
        return res["ms"][old] - res["ms"][new] > sp

    res["batch_beats_yardstick"] = {
        "dev_at_count": wins("dev_branches16_at_count", "dev_single_x16_at_count"),
        "host_at_count": wins("host_branches16_at_count", "host_single_x16_at_count"),
        **{f"dev_at_{name}": wins(f"dev_branches16_root_at_{name}", f"dev_rebuild_single_x16_at_{name}")
           for name in ("count-1", "count/2+1", "count/2")},
        **{f"host_verify_n{nv}": wins(f"host_verify_deposits_n{nv}", f"host_hash_var_then_verify_branches_n{nv}")
           for nv in nvs}}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    _lib.load().mk_deposit_trie_free(h)


if __name__ == "__main__":
    main()
