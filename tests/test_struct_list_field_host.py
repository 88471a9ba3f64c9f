"""List fields inside flat records (MK_FIELD_LIST) without a GPU: the packers
of prysm_amd.state and the slot format (tests/struct_list_ref.py) against the
oracle's reflective TreeHash of the same values, the layouts the parser takes
and every refusal, and the reference's own struct vectors with slice fields
expressed as flat records."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from oracle import ssz_ref
from prysm_amd import _lib
from prysm_amd import state as ST
from tests import struct_list_ref as SL

B, R, V, S, L = _lib.MK_FIELD_BYTES, _lib.MK_FIELD_RAW, _lib.MK_FIELD_VARBYTES, _lib.MK_FIELD_STRUCT, _lib.MK_FIELD_LIST
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

U64, BY = ("uint", 64), ("bytes",)
ATT_DATA_T = ("struct", "pb.AttestationData", [
    ("Slot", U64), ("Shard", U64), ("BeaconBlockRootHash32", BY), ("EpochBoundaryRootHash32", BY),
    ("ShardBlockRootHash32", BY), ("LatestCrosslinkRootHash32", BY), ("JustifiedEpoch", U64),
    ("JustifiedBlockRootHash32", BY), ("JustifiedSlot", U64)])
VOTE_T = ("struct", "pb.SlashableVote", [
    ("ValidatorIndices", ("slice", U64)), ("CustodyBitfield", BY), ("Data", ("ptr", ATT_DATA_T)),
    ("AggregateSignature", BY)])
SLASHING_T = ("struct", "pb.AttesterSlashing", [("SlashableVote_1", ("ptr", VOTE_T)), ("SlashableVote_2", ("ptr", VOTE_T))])
DEPOSIT_T = ("struct", "pb.Deposit", [("MerkleBranchHash32S", ("slice", BY)), ("MerkleTreeIndex", U64), ("DepositData", BY)])


def rand_vote(rng, count, bitfield_cap=8):
    rb = lambda n: bytes(rng.getrandbits(8) for _ in range(n))
    return {"ValidatorIndices": [rng.getrandbits(64) for _ in range(count)],
            "CustodyBitfield": rb(rng.randint(0, bitfield_cap)),
            "Data": {"Slot": rng.getrandbits(64), "Shard": rng.getrandbits(64), "BeaconBlockRootHash32": rb(32),
                     "EpochBoundaryRootHash32": rb(32), "ShardBlockRootHash32": rb(32),
                     "LatestCrosslinkRootHash32": rb(32), "JustifiedEpoch": rng.getrandbits(64),
                     "JustifiedBlockRootHash32": rb(32), "JustifiedSlot": rng.getrandbits(64)},
            "AggregateSignature": rb(rng.choice([0, 48, 96]))}


def rand_deposit(rng, count, data_cap=64):
    rb = lambda n: bytes(rng.getrandbits(8) for _ in range(n))
    return {"MerkleBranchHash32S": [rb(32) for _ in range(count)], "MerkleTreeIndex": rng.getrandbits(64),
            "DepositData": rb(rng.randint(0, data_cap))}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def _f(spec):
    arr = (_lib.Field * len(spec))()
    for i, (k, o, n) in enumerate(spec):
        arr[i].kind, arr[i].offset, arr[i].len = k, o, n
    return arr


def _counts(rng, cap, n):
    return [0, cap, 1] + [rng.randint(0, cap) for _ in range(n - 3)]


# ---- the packers and the slot format against the typed TreeHash --------------------------------
def test_slashable_votes_match_typed_hash():
    rng = random.Random(11)
    votes = [rand_vote(rng, c) for c in _counts(rng, 40, 8)]
    rec, fields = ST.pack_slashable_votes(votes, 40, 8)
    assert rec.shape == (8, ST.slashable_vote_record_len(40, 8)) and len(fields) == 14
    roots = SL.record_roots(rec, fields)
    for v, r in zip(votes, roots):
        assert bytes(r) == ssz_ref.tree_hash(VOTE_T, v)
    assert SL.list_root(rec, fields) == ssz_ref.tree_hash(("slice", ("ptr", VOTE_T)), votes)


def test_attester_slashings_match_typed_hash():
    rng = random.Random(12)
    cs = _counts(rng, 20, 6)
    sl = [{"SlashableVote_1": rand_vote(rng, a), "SlashableVote_2": rand_vote(rng, b)} for a, b in zip(cs, cs[::-1])]
    rec, fields = ST.pack_attester_slashings(sl, 20, 8)
    assert len(fields) == 30
    for v, r in zip(sl, SL.record_roots(rec, fields)):
        assert bytes(r) == ssz_ref.tree_hash(SLASHING_T, v)


def test_deposits_match_typed_hash():
    rng = random.Random(13)
    deps = [rand_deposit(rng, c) for c in _counts(rng, 32, 9)]
    rec, fields = ST.pack_deposits(deps, 64)
    assert rec.shape[1] == ST.deposit_record_len(64) and len(fields) == 4
    for v, r in zip(deps, SL.record_roots(rec, fields)):
        assert bytes(r) == ssz_ref.tree_hash(DEPOSIT_T, v)


def test_generic_flattening_agrees_with_the_packers():
    """tests/struct_list_ref.flatten lays the same types out on its own; both
    records hash to the same roots."""
    rng = random.Random(14)
    votes = [rand_vote(rng, c) for c in (0, 5, 17)]
    fields, rec_len, pack = SL.flatten(VOTE_T, [17, 8, 32, 32, 32, 32, 32, 96])
    rec = np.frombuffer(b"".join(pack(v) for v in votes), dtype=np.uint8).reshape(3, rec_len)
    for v, r in zip(votes, SL.record_roots(rec, fields)):
        assert bytes(r) == ssz_ref.tree_hash(VOTE_T, v)


def test_packers_refuse_values_above_capacity():
    rng = random.Random(15)
    with pytest.raises(ValueError):
        ST.pack_slashable_votes([rand_vote(rng, 5)], 4, 8)
    v = rand_vote(rng, 2)
    v["CustodyBitfield"] = b"\1" * 9
    with pytest.raises(ValueError):
        ST.pack_slashable_votes([v], 4, 8)
    with pytest.raises(ValueError):
        ST.pack_attester_slashings([{"SlashableVote_1": rand_vote(rng, 1), "SlashableVote_2": rand_vote(rng, 5)}], 4, 8)
    with pytest.raises(ValueError):
        ST.pack_deposits([rand_deposit(rng, 33)], 64)
    d = rand_deposit(rng, 3)
    d["DepositData"] = b"\2" * 65
    with pytest.raises(ValueError):
        ST.pack_deposits([d], 64)


def test_slot_garbage_beyond_count_is_ignored():
    rng = random.Random(16)
    deps = [rand_deposit(rng, c, 16) for c in (0, 3, 31)]
    rec, fields = ST.pack_deposits(deps, 64)
    dirty = rec.copy()
    for i, d in enumerate(deps):
        dirty[i, 4 + 32 * len(d["MerkleBranchHash32S"]):4 + 32 * 32] = 0xA5
    assert (SL.record_roots(dirty, fields) == SL.record_roots(rec, fields)).all()


# ---- the reference's own vectors with slices inside structs -----------------------------------
def _has_slice(t):
    if t[0] in ("slice", "array"):
        return True
    if t[0] == "ptr":
        return _has_slice(t[1])
    if t[0] == "struct":
        return any(_has_slice(ft) for _, ft in t[2])
    return False


def _tup(t):
    return tuple(_tup(x) if isinstance(x, list) else x for x in t) if isinstance(t, list) else t


def _struct_slice_vectors():
    with open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")) as f:
        doc = json.load(f)
    found = []

    def walk(x):
        if isinstance(x, dict):
            if "type" in x and "output" in x and x.get("error") is None and isinstance(x["type"], list):
                t = _tup(x["type"])
                if t and t[0] == "struct" and _has_slice(t):
                    found.append((t, x["value"], x["output"]))
            for v in x.values():
                walk(v)
        elif isinstance(x, list):
            for v in x:
                walk(v)
    walk(doc)
    return found


def test_reference_vectors_with_slice_fields(lib):
    vecs = _struct_slice_vectors()
    assert vecs, "reference_vectors.json holds a struct with a slice field (hash_test.go:107)"
    done = 0
    for t, value, output in vecs:
        try:
            fields, rec_len, pack = SL.flatten(t, [8] * 16)
        except (AssertionError, ValueError):
            continue  # a slice of slices, or a kind flat records do not carry
        rec = np.frombuffer(pack(value), dtype=np.uint8).reshape(1, rec_len)
        assert SL.record_root(rec[0].tobytes(), fields).hex() == output
        assert lib.mk_ssz_struct_msg_len(_f(fields), len(fields)) > 0
        done += 1
    assert done >= 1


# ---- the parser: what it takes, what it refuses ----------------------------------------------
ACCEPTED = [
    ("uint64 items", [(L, 0, 256), (R, 8, 8)], 32),
    ("bool items, 256 chunks", [(L, 0, 128 * 256), (R, 1, 1)], 32),
    ("[32]byte items", [(R, 0, 8), (L, 8, 32), (B, 32, 32)], 8 + 32),
    ("[48]byte items, padded cells", [(L, 0, 5), (B, 64, 48), (R, 324, 4)], 32 + 4),
    ("struct items", [(L, 0, 9), (S, 12, 2), (R, 0, 8), (R, 8, 2)], 32),
    ("struct items with a varbytes child", [(L, 0, 9), (S, 24, 2), (R, 0, 8), (V, 8, 12)], 32),
    ("struct items with a nested struct", [(L, 0, 4), (S, 16, 3), (R, 0, 8), (S, 0, 1), (R, 8, 8)], 32),
    ("two lists", [(L, 0, 4), (R, 8, 8), (L, 36, 4), (B, 32, 32)], 64),
    ("list in a nested struct", [(R, 0, 8), (S, 0, 3), (L, 8, 4), (R, 4, 4), (R, 28, 4)], 8 + 32),
    ("slashable vote", ST.slashable_vote_fields(256, 32), 32 * 4),
    ("attester slashing", ST.attester_slashing_fields(256, 32), 64),
    ("deposit", ST.deposit_fields(512), 72),
]


@pytest.mark.parametrize("what,spec,top", ACCEPTED, ids=[a[0] for a in ACCEPTED])
def test_accepted_layouts(lib, what, spec, top):
    got = lib.mk_ssz_struct_msg_len(_f(spec), len(spec))
    assert got >= top > 0, what
    if not any(k == S for k, _, _ in spec):
        assert got == top
    assert lib.mk_ssz_struct_list_workspace_bytes(1000, _f(spec), len(spec)) > 0


_DEEP_ITEM = [(S, 0, 5), (S, 0, 4), (S, 0, 3), (L, 0, 2), (S, 8, 1), (R, 0, 8)]   # the item struct would be depth 5
_DEPTH4_ITEM = [(S, 0, 4), (S, 0, 3), (L, 0, 2), (S, 8, 1), (R, 0, 8)]           # the item struct is depth 4
# top message 9 x 32 B, then the chunk pair and 8 stack levels: 288 + 256 + 256 > 640
_LDS = [(B, 32 * k, 32) for k in range(8)] + [(L, 256, 128 * 256), (R, 1, 1)]
REFUSED = [
    ("list in a list item", [(L, 0, 4), (S, 64, 2), (L, 0, 4), (R, 8, 8)]),
    ("list of lists", [(L, 0, 4), (L, 64, 4), (R, 8, 8)]),
    ("cap == 0", [(L, 0, 0), (R, 8, 8)]),
    ("more than 256 chunks", [(L, 0, 16 * 256 + 1), (R, 8, 8)]),
    ("more than 256 chunks of byte items", [(L, 0, 4 * 256 + 1), (B, 32, 32)]),
    ("raw stride != len", [(L, 0, 4), (R, 16, 8)]),
    ("bytes stride below len", [(L, 0, 4), (B, 28, 32)]),
    ("bytes stride % 4", [(L, 0, 4), (B, 34, 32)]),
    ("bytes len % 4", [(L, 0, 4), (B, 32, 30)]),
    ("struct stride % 4", [(L, 0, 4), (S, 10, 1), (R, 0, 8)]),
    ("item child past the cell", [(L, 0, 4), (S, 12, 2), (R, 0, 8), (R, 8, 8)]),
    ("unaligned slot", [(R, 0, 2), (L, 2, 4), (R, 8, 8)]),
    ("missing item descriptor", [(R, 0, 8), (L, 8, 4)]),
    ("missing item descriptor in a struct", [(S, 0, 2), (R, 0, 8), (L, 8, 4), (R, 8, 8)]),
    ("varbytes item", [(L, 0, 4), (V, 36, 32)]),
    ("more than 32 entries", [(L, 0, 4), (R, 8, 8)] + [(R, 40 + 8 * k, 8) for k in range(31)]),
    ("depth above 4", _DEEP_ITEM),
    ("LDS need over budget", _LDS),
]


@pytest.mark.parametrize("what,spec", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_layouts(lib, what, spec):
    assert lib.mk_ssz_struct_msg_len(_f(spec), len(spec)) == 0, what
    call = _lib.Call(-1, 0, b"")
    rc = lib.mk_dev_ssz_struct_list_tree_build(ctypes.byref(call), None, 10, 10, 1 << 20, _f(spec), len(spec), None,
                                               None, None, None, 1 << 30, None)
    assert rc == _lib.MK_EINVAL and call.err != b"", what


def test_limits_are_tight(lib):
    assert lib.mk_ssz_struct_msg_len(_f(_DEPTH4_ITEM), len(_DEPTH4_ITEM)) > 0
    ok32 = [(L, 0, 4), (R, 8, 8)] + [(R, 40 + 8 * k, 8) for k in range(30)]
    assert len(ok32) == 32 and lib.mk_ssz_struct_msg_len(_f(ok32), 32) > 0
    assert lib.mk_ssz_struct_msg_len(_f([(L, 0, 16 * 256), (R, 8, 8)]), 2) == 32
    # 4 x 32 B of message, the pair and 8 levels: 128 + 512 = 640 B, the limit at 64 threads
    fits = [(B, 32 * k, 32) for k in range(3)] + [(L, 96, 128 * 256), (R, 1, 1)]
    assert lib.mk_ssz_struct_msg_len(_f(fits), len(fits)) == 128
    over = [(B, 32 * k, 32) for k in range(3)] + [(R, 96, 4), (L, 100, 128 * 256), (R, 1, 1)]
    assert lib.mk_ssz_struct_msg_len(_f(over), len(over)) == 0


def test_slot_past_the_record_is_refused(lib):
    spec = [(L, 0, 4), (R, 8, 8)]
    call = _lib.Call(-1, 0, b"")
    args = (None, None, None, None, 1 << 30, None)
    rc = lib.mk_dev_ssz_struct_list_tree_build(ctypes.byref(call), None, 10, 10, 32, _f(spec), 2, *args)
    assert rc == _lib.MK_EINVAL and b"exceeds the record" in call.err
    rc = lib.mk_dev_ssz_struct_list_tree_build(ctypes.byref(call), None, 10, 10, 36, _f(spec), 2, *args)
    assert rc != _lib.MK_EINVAL or b"null pointer" in call.err
