#!/usr/bin/env python3
"""Nested struct hashing (MK_FIELD_STRUCT / MK_FIELD_VARBYTES, k_struct_nested)
beside what the earlier entry points could compose, in one process (DESIGN.md
§5g; the method of tools/bytes_tree_probe.py).

  python tools/struct_nested_probe.py [--out profiles/struct_nested/probe.json] [--quick]

Lists of 4 096 and 65 536 PendingAttestationRecords (bitfields of 16..47
bytes in 48-byte slots, 304-B records):
  a  nested_list_root   mk_dev_ssz_struct_list_root over the packed records:
                        k_struct_nested, then merkleHash over the roots
  b  composed           what a device-resident caller could compose before:
                        mk_dev_hash_batch over the 5 a 36-B messages
                        le32(32) || root, mk_dev_hash_batch_var over the 2 a
                        bitfield messages, mk_dev_hash_batch_var over the a
                        192-B AttestationData messages, mk_dev_hash_batch_var
                        over the a 104-B record messages, mk_dev_ssz_merkle_hash
                        over the a roots.  Every message buffer is assembled
                        beforehand (the gathers between the steps are left
                        out), so (b) is flattered and its root is not checked.
  c  host wall time of the three struct lists of BeaconState.tree_hash_ssz
     (LatestCrosslinks, LatestAttestations, Eth1DataVotes) for the
     synthetic_state default shape: `host_packed` = this tree's packers and
     struct-list calls, `host_parent` = the per-row Python path they replace
     (restated here from the parent's tree_hash_ssz: two dependent
     hash_batch_var round trips and one for the bitfields, then the lists'
     merkleHash).  Both produce the same three roots (checked).
(a) and (b) are warmed up, then timed in `rounds` interleaved rounds of `reps`
back-to-back calls between device events; `ms` is the median round's ms per
call, `ms_min` / `ms_max` the spread.  (c) is time.perf_counter around the
whole host path, the same rounds.  (a)'s root is checked against the host
entry point's.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import struct as _st
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x5EED000000000000 + 4646


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "struct_nested", "probe.json"))
    ap.add_argument("--quick", action="store_true", help="small lists (a rehearsal, not a measurement)")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch

    from prysm_amd import _lib
    from prysm_amd import device as D
    from prysm_amd import state as ST
    from prysm_amd.hashutil import hash_batch, hash_batch_var

    if not torch.cuda.is_available() or _lib.device_count() < 1:
        raise SystemExit("struct_nested_probe needs a gfx950 device (no CPU fallback)")
    dev = torch.device("cuda:0")
    L = _lib.load()

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

    def hash_var_dev(msgs, offs, n, out):
        _lib.invoke("mk_dev_hash_batch_var", D._p(msgs), D._p(offs), n, D._p(out), D._stream(dev), device=0)

    def measure(a):
        att = ST.synthetic_state(8, SEED, n_attestations=a, n_batched=1, n_votes=1, lists_len=8,
                                 shards=8).attestations
        rec, fields = ST.pack_attestations(att, 48)
        R = rec.shape[1]
        d_rec = torch.from_numpy(rec.reshape(-1)).to(dev)
        out = torch.zeros(32, dtype=torch.uint8, device=dev)
        ws = torch.empty(L.mk_ssz_struct_list_workspace_bytes(a, ST.R._fields(fields), len(fields)) + 256,
                         dtype=torch.uint8, device=dev)
        # (b): pre-assembled message buffers of the right shapes
        m36 = torch.zeros(5 * a * 36, dtype=torch.uint8, device=dev)
        bits = [_st.pack("<I", len(x)) + x for x in att.aggregation_bitfield + att.custody_bitfield]
        boffs = torch.from_numpy(np.cumsum([0] + [len(x) for x in bits]).astype(np.uint64).view(np.int64)).to(dev)
        bmsg = torch.from_numpy(np.frombuffer(b"".join(bits), np.uint8).copy()).to(dev)
        m192 = torch.zeros(a * 192, dtype=torch.uint8, device=dev)
        o192 = torch.arange(0, (a + 1) * 192, 192, dtype=torch.int64, device=dev)
        m104 = torch.zeros(a * 104, dtype=torch.uint8, device=dev)
        o104 = torch.arange(0, (a + 1) * 104, 104, dtype=torch.int64, device=dev)
        h36 = torch.empty(5 * a * 32, dtype=torch.uint8, device=dev)
        hbits = torch.empty(2 * a * 32, dtype=torch.uint8, device=dev)
        hdata = torch.empty(a * 32, dtype=torch.uint8, device=dev)
        hrec = torch.empty(a * 32, dtype=torch.uint8, device=dev)
        out_b = torch.zeros(32, dtype=torch.uint8, device=dev)
        mws = D.merkle_workspace(a, 32, dev)

        def nested():
            D.struct_list_root(d_rec, a, R, fields, out=out, ws=ws)

        def composed():
            D.hash_batch(m36, 5 * a, 36, out=h36)
            hash_var_dev(bmsg, boffs, 2 * a, hbits)
            hash_var_dev(m192, o192, a, hdata)
            hash_var_dev(m104, o104, a, hrec)
            D.merkle_hash(hrec, a, 32, out=out_b, ws=mws)

        variants = {"nested_list_root": nested, "composed": composed}
        want = ST.struct_list_root_packed(rec, fields)
        reps = {}
        for name, fn in variants.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ms = timed(fn, 3)
            reps[name] = max(3, min(200, int(50.0 / max(ms, 1e-3))))
        assert bytes(out.cpu().numpy()) == want, "nested_list_root differs from the host entry point's root"
        samples = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                samples[name].append(timed(fn, reps[name]))
        row = {"attestations": a, "record_len": R, "reps": reps}
        for name in variants:
            row[name] = stats(samples[name])
        sp = max(row[n]["ms_max"] - row[n]["ms_min"] for n in variants)
        d = row["nested_list_root"]["ms"] - row["composed"]["ms"]
        row["nested_vs_composed"] = "slower" if d > sp else ("faster" if -d > sp else "within the spread")
        return row

    def host_paths():
        st = ST.synthetic_state(1024, SEED)
        att = st.attestations
        a, v = len(att), len(st.eth1_votes)

        def packed():
            rec, fields = ST.pack_attestations(att)
            return (ST.struct_list_root_packed(ST.pack_crosslinks(st.crosslink_epochs, st.crosslink_roots),
                                               ST.CROSSLINK_FIELDS),
                    ST.struct_list_root_packed(rec, fields),
                    ST.struct_list_root_packed(ST.pack_eth1_votes(st.eth1_votes, st.eth1_vote_counts),
                                               ST.ETH1_VOTE_FIELDS))

        def parent():  # the per-row path of the parent's tree_hash_ssz, the three struct lists only
            b32 = np.concatenate([st.crosslink_roots, att.roots.reshape(-1, 32), att.justified_root,
                                  st.eth1_votes.reshape(-1, 32)])
            msgs = np.empty((len(b32), 36), dtype=np.uint8)
            msgs[:, :4] = np.frombuffer(_st.pack("<I", 32), dtype=np.uint8)
            msgs[:, 4:] = b32
            h = hash_batch(msgs, 36)
            cut = np.cumsum([0, len(st.crosslink_roots), 4 * a, a, 2 * v])
            h_cross, h_att4, h_just, h_votes = (h[cut[i]:cut[i + 1]] for i in range(4))
            h_att4 = h_att4.reshape(a, 128)
            bits = hash_batch_var([_st.pack("<I", len(x)) + x for x in att.aggregation_bitfield + att.custody_bitfield])
            le = lambda x: np.ascontiguousarray(x, dtype="<u8").reshape(-1, 1).view(np.uint8)  # noqa: E731
            cross_msg = np.concatenate([le(st.crosslink_epochs), h_cross], axis=1)
            att_msg = np.concatenate([le(att.slot), le(att.shard), h_att4, le(att.justified_epoch), h_just,
                                      le(att.justified_slot)], axis=1)
            eth1_msg = h_votes.reshape(v, 64)
            r3 = hash_batch_var([bytes(r) for r in cross_msg] + [bytes(r) for r in att_msg] +
                                [bytes(r) for r in eth1_msg])
            cross_roots = b"".join(r3[:len(cross_msg)])
            att_data, vote_eth1 = r3[len(cross_msg):len(cross_msg) + a], r3[len(cross_msg) + a:]
            rec_msgs = [att_data[i] + bits[i] + bits[a + i] + _st.pack("<Q", int(att.slot_included[i]))
                        for i in range(a)]
            vote_msgs = [vote_eth1[i] + _st.pack("<Q", int(st.eth1_vote_counts[i])) for i in range(v)]
            r4 = hash_batch_var(rec_msgs + vote_msgs)
            lists = [(np.frombuffer(cross_roots, np.uint8), len(cross_msg)),
                     (np.frombuffer(b"".join(r4[:a]), np.uint8), a), (np.frombuffer(b"".join(r4[a:]), np.uint8), v)]
            buf, offs, pos = [], [], 0
            for arr, _ in lists:
                pad = (-pos) % 16
                buf.append(np.zeros(pad, np.uint8))
                pos += pad
                offs.append(pos)
                buf.append(arr)
                pos += arr.size
            return tuple(ST._merkle_many_mixed(np.concatenate(buf), offs, [x[1] for x in lists], [32, 32, 32]))

        assert packed() == parent(), "the packed path and the parent's path disagree"
        samples = {"host_packed": [], "host_parent": []}
        fns = {"host_packed": packed, "host_parent": parent}
        for _ in range(args.rounds):
            for name, fn in fns.items():
                t0 = time.perf_counter()
                for _ in range(5):
                    fn()
                samples[name].append((time.perf_counter() - t0) * 1e3 / 5)
        row = {"attestations": a, "crosslinks": len(st.crosslink_epochs), "votes": v}
        for name in fns:
            row[name] = stats(samples[name])
        return row

    sizes = [256, 1024] if args.quick else [4096, 65536]
    result = {"tool": "struct_nested_probe", "version": L.mk_version().decode(), "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0), "lists": [measure(a) for a in sizes], "host": host_paths()}
    line = json.dumps(result)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
