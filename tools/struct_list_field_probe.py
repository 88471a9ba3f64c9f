#!/usr/bin/env python3
"""Records with list fields (MK_FIELD_LIST, k_struct_list) beside the only
route to the same roots without them, in one process.

  python tools/struct_list_field_probe.py [--out profiles/struct_list_field/probe.json] [--quick]
  python tools/struct_list_field_probe.py --attestations-only --out FILE   # the old path's timing alone

Three lists of 2^14 records:
  votes_uniform   SlashableVote, indices_cap 256, counts uniform in 0..256
  votes_full      the same, every count 256
  deposits        Deposit, branch counts uniform in 0..32, deposit data 0..64 B
For each: `list_root` = mk_dev_ssz_struct_list_root over the packed records
between device events (warmed up, `rounds` rounds of `reps` back-to-back
calls; median, min and max ms per call), checked against the host entry
point's root; `generic` = prysm_amd.ssz.tree_hash of the same values as typed
structs (the breadth-first evaluator, one batched launch per type level; host
wall time, one warm-up and `rounds` calls).  `perms` is the Keccak-f count of
the list by the message lengths; `valu_fraction` = perms x 4320 int32 ops
 / list_root time / 78.6e12.
`attestations`: LatestAttestations (2^14 PendingAttestationRecords, 48-byte
bitfield slots) through the same entry point -- the path this layout kind does
not touch; run it with PRYSM_MERKLE_LIB pointing at another build of the
library to compare.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 4646
PEAK = 78.6e12
OPS_PER_PERM = 4320


def perms_of(mlen):
    return mlen // 136 + 1


def list_perms(count, out_len, elem_perms):
    """Keccak-f calls of merkleHash over `count` element hashes (hash.go:194-239)."""
    ipc = 128 // out_len
    total = count * elem_perms
    chunks = max(1, -(-count // ipc))
    if chunks == 1:
        return total + perms_of((count * out_len if count else 128) + 32)
    last = (count - 1) % ipc + 1
    m = -(-chunks // 2)
    total += (m - 1) * perms_of(256) + perms_of(last * out_len + 128)  # the last pair: 128 B beside the short chunk
    while m > 1:
        total += (m // 2) * perms_of(64) + (m % 2) * perms_of(160)
        m = -(-m // 2)
    return total + perms_of(64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "struct_list_field", "probe.json"))
    ap.add_argument("--quick", action="store_true", help="small lists (a rehearsal, not a measurement)")
    ap.add_argument("--attestations-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D
    from prysm_amd import ssz as S
    from prysm_amd import state as ST

    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise SystemExit("struct_list_field_probe needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    L = _lib.load()
    n = 1 << (10 if args.quick else 14)
    rng = np.random.default_rng(SEED)

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def stats(samples):
        return {"ms": round(statistics.median(samples), 5), "ms_min": round(min(samples), 5),
                "ms_max": round(max(samples), 5)}

    def device_time(rec, fields):
        R = rec.shape[1]
        d_rec = torch.from_numpy(rec.reshape(-1)).to(dev)
        out = torch.zeros(32, dtype=torch.uint8, device=dev)
        ws = torch.empty(L.mk_ssz_struct_list_workspace_bytes(len(rec), ST.R._fields(fields), len(fields)) + 256,
                         dtype=torch.uint8, device=dev)

        def fn():
            D.struct_list_root(d_rec, len(rec), R, fields, out=out, ws=ws)

        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps = max(3, min(200, int(50.0 / max(timed(fn, 3), 1e-3))))
        samples = [timed(fn, reps) for _ in range(args.rounds)]
        return stats(samples), bytes(out.cpu().numpy()), reps

    def host_time(vals, typ):
        got = S.tree_hash(vals, typ)
        samples = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            S.tree_hash(vals, typ)
            samples.append((time.perf_counter() - t0) * 1e3)
        return stats(samples), got

    def rb(k):
        return rng.integers(0, 256, k, dtype=np.uint8).tobytes()

    def vote(count):
        return {"ValidatorIndices": rng.integers(0, 1 << 63, count, dtype=np.uint64).tolist(),
                "CustodyBitfield": rb(int(rng.integers(0, 33))),
                "Data": {"Slot": int(rng.integers(1 << 40)), "Shard": int(rng.integers(1024)),
                         "BeaconBlockRootHash32": rb(32), "EpochBoundaryRootHash32": rb(32),
                         "ShardBlockRootHash32": rb(32), "LatestCrosslinkRootHash32": rb(32),
                         "JustifiedEpoch": int(rng.integers(1 << 30)), "JustifiedBlockRootHash32": rb(32),
                         "JustifiedSlot": int(rng.integers(1 << 40))},
                "AggregateSignature": rb(96)}

    def row(name, vals, rec, fields, typ, perms):
        dstat, root, reps = device_time(rec, fields)
        assert root == ST.struct_list_root_packed(rec, fields), name
        hstat, hroot = host_time(vals, S.Slice(S.Ptr(typ)))
        assert hroot == root, f"{name}: the generic evaluator's root differs"
        return {"records": len(rec), "record_len": int(rec.shape[1]), "reps": reps, "list_root": dstat,
                "generic": hstat, "perms": int(perms),
                "valu_fraction": round(perms * OPS_PER_PERM / (dstat["ms"] * 1e-3) / PEAK, 4),
                "speedup": round(hstat["ms"] / dstat["ms"], 1)}

    result = {"tool": "struct_list_field_probe", "version": L.mk_version().decode(), "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0)}
    att = ST.synthetic_state(8, SEED, n_attestations=n, n_batched=1, n_votes=1, lists_len=8, shards=8).attestations
    arec, afields = ST.pack_attestations(att, 48)
    astat, _, areps = device_time(arec, afields)
    result["attestations"] = {"records": n, "record_len": int(arec.shape[1]), "reps": areps, "list_root": astat}
    if not args.attestations_only:
        tree = lambda k: list_perms(k, 32, 0)  # noqa: E731  the list of record roots
        for name, counts in (("votes_uniform", rng.integers(0, 257, n)), ("votes_full", np.full(n, 256))):
            vals = [vote(int(c)) for c in counts]
            rec, fields = ST.pack_slashable_votes(vals, 256, 32)
            # per record: the index list, the bitfield, AttestationData (5 x 36 B, its 192-B message), the
            # signature (100 B), the 128-B record message
            per = [list_perms(int(c), 8, 0) + 1 + 5 + perms_of(192) + 1 + 1 for c in counts]
            result[name] = row(name, vals, rec, fields, ST.SLASHABLE_VOTE_SSZ, sum(per) + tree(n))
        counts = rng.integers(0, 33, n)
        vals = [{"MerkleBranchHash32S": [rb(32) for _ in range(int(c))], "MerkleTreeIndex": int(rng.integers(1 << 32)),
                 "DepositData": rb(int(rng.integers(0, 65)))} for c in counts]
        rec, fields = ST.pack_deposits(vals, 64)
        per = [list_perms(int(c), 32, 1) + 1 + 1 for c in counts]
        result["deposits"] = row("deposits", vals, rec, fields, ST.DEPOSIT_SSZ, sum(per) + tree(n))
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
