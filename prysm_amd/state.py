"""State tree hash: ssz.TreeHash of a whole
``pb.BeaconState`` on the engine.

The reference roots a state with ``Keccak(proto.Marshal(state))``
(beacon-chain/core/state/state.go:168-174) and leaves "Replace by state tree
hashing algorithm" TODOs at beacon-chain/blockchain/service.go:115 and :273.
This module is that replacement: the reference's own reflective TreeHash
(shared/ssz/hash.go:23-239) of the state struct, field by field in
declaration order (proto/beacon/p2p/v1/types.pb.go:50-79, the XXX_ fields
skipped as structFields does, ssz_utils_cache.go:100), computed with a fixed
number of batched library calls instead of one Keccak per field element:

  1. every 32-B bytes field that is a list element or a state field (randao
     mixes, block / batched / index roots, seeds): hashedEncoding
     K(le32(32) || b), one 36-B batch;
  2. the validator registry: typed struct roots + merkleHash
     (mk_ssz_struct_list_root, the Hashable fast path of registry.py);
  3. the three struct lists (CrosslinkRecord, PendingAttestationRecord with
     its nested AttestationData and variable-length bitfields, Eth1DataVote
     with its nested Eth1Data) packed into flat record arrays with numpy and
     rooted by one mk_ssz_struct_list_root each (MK_FIELD_STRUCT,
     MK_FIELD_VARBYTES); LatestEth1Data as a one-record struct root;
  4. every other list of the state (balances, the 8192-entry root arrays,
     penalized balances) in ONE segmented merkleHash call (mk_ssz_merkle_many);
  5. the state struct: K(concatenation of the 25 field outputs).

SSZ legality: ``Validator.StatusFlags`` is an int32 enum,
which makeEncoder rejects (encode.go:107-108), so it is widened to uint64;
``LatestEth1Data`` and ``Fork`` are pointers, which must be non-nil
(hash.go:172-173).  ``STATE_SSZ`` is the same type for the reflective mirror
(prysm_amd.ssz.tree_hash), and the tests check both paths against the
oracle's restatement (oracle/ssz_ref.py).
"""
from __future__ import annotations

import struct as _st
from dataclasses import dataclass, field
from typing import List

import numpy as np

from . import _lib
from . import registry as R
from . import ssz as S
from .hashutil import _ptr, hash_batch, hash_batch_var

# shared/params/config.go:96-105
SHARD_COUNT = 1024
LATEST_BLOCK_ROOTS_LENGTH = 8192
LATEST_RANDAO_MIXES_LENGTH = 8192
LATEST_PENALIZED_EXIT_LENGTH = 8192
LATEST_INDEX_ROOTS_LENGTH = 8192

_U64 = S.Uint(64)
_B = S.Bytes()

CROSSLINK_SSZ = S.Struct("pb.CrosslinkRecord", [("Epoch", _U64), ("ShardBlockRootHash32", _B)])
ATTESTATION_DATA_SSZ = S.Struct("pb.AttestationData", [
    ("Slot", _U64), ("Shard", _U64), ("BeaconBlockRootHash32", _B), ("EpochBoundaryRootHash32", _B),
    ("ShardBlockRootHash32", _B), ("LatestCrosslinkRootHash32", _B), ("JustifiedEpoch", _U64),
    ("JustifiedBlockRootHash32", _B), ("JustifiedSlot", _U64)])
PENDING_ATTESTATION_SSZ = S.Struct("pb.PendingAttestationRecord", [
    ("Data", S.Ptr(ATTESTATION_DATA_SSZ)), ("AggregationBitfield", _B), ("CustodyBitfield", _B),
    ("SlotIncluded", _U64)])
ETH1_DATA_SSZ = S.Struct("pb.Eth1Data", [("DepositRootHash32", _B), ("BlockHash32", _B)])
ETH1_VOTE_SSZ = S.Struct("pb.Eth1DataVote", [("Eth1Data", S.Ptr(ETH1_DATA_SSZ)), ("VoteCount", _U64)])
FORK_SSZ = S.Struct("pb.Fork", [("PreviousVersion", _U64), ("CurrentVersion", _U64), ("Epoch", _U64)])

# pb.BeaconState field order (types.pb.go:50-79); XXX_ fields present and skipped
STATE_FIELDS = [
    ("ValidatorRegistry", S.Slice(S.Ptr(R.VALIDATOR_SSZ))),
    ("ValidatorRegistryUpdateEpoch", _U64),
    ("ValidatorBalances", S.Slice(_U64)),
    ("LatestRandaoMixesHash32S", S.Slice(_B)),
    ("PreviousEpochStartShard", _U64),
    ("CurrentEpochStartShard", _U64),
    ("PreviousCalculationEpoch", _U64),
    ("CurrentCalculationEpoch", _U64),
    ("PreviousEpochSeedHash32", _B),
    ("CurrentEpochSeedHash32", _B),
    ("PreviousJustifiedEpoch", _U64),
    ("JustifiedEpoch", _U64),
    ("JustificationBitfield", _U64),
    ("FinalizedEpoch", _U64),
    ("LatestCrosslinks", S.Slice(S.Ptr(CROSSLINK_SSZ))),
    ("LatestBlockRootHash32S", S.Slice(_B)),
    ("BatchedBlockRootHash32S", S.Slice(_B)),
    ("LatestPenalizedBalances", S.Slice(_U64)),
    ("LatestAttestations", S.Slice(S.Ptr(PENDING_ATTESTATION_SSZ))),
    ("LatestIndexRootHash32S", S.Slice(_B)),
    ("LatestEth1Data", S.Ptr(ETH1_DATA_SSZ)),
    ("Eth1DataVotes", S.Slice(S.Ptr(ETH1_VOTE_SSZ))),
    ("GenesisTime", _U64),
    ("Fork", S.Ptr(FORK_SSZ)),
    ("Slot", _U64),
    ("XXX_NoUnkeyedLiteral", S.Unsupported("struct {}")),
    ("XXX_unrecognized", _B),
    ("XXX_sizecache", S.Unsupported("int32")),
]
STATE_SSZ = S.Struct("pb.BeaconState", STATE_FIELDS)

_SCALARS = ["ValidatorRegistryUpdateEpoch", "PreviousEpochStartShard", "CurrentEpochStartShard",
            "PreviousCalculationEpoch", "CurrentCalculationEpoch", "PreviousJustifiedEpoch", "JustifiedEpoch",
            "JustificationBitfield", "FinalizedEpoch", "GenesisTime", "Slot"]


@dataclass
class Attestations:
    """[]*PendingAttestationRecord as columns (AttestationData inlined)."""
    slot: np.ndarray            # u64 (a,)
    shard: np.ndarray           # u64 (a,)
    roots: np.ndarray           # (a, 4, 32): beacon block / epoch boundary / shard block / latest crosslink
    justified_epoch: np.ndarray
    justified_root: np.ndarray  # (a, 32)
    justified_slot: np.ndarray
    aggregation_bitfield: List[bytes]
    custody_bitfield: List[bytes]
    slot_included: np.ndarray

    def __len__(self):
        return len(self.slot)


# ---- typed layouts of the state's struct lists (mk_field: (kind, offset, len)) ----------------
_BY, _RAW, _VAR, _STRUCT = _lib.MK_FIELD_BYTES, _lib.MK_FIELD_RAW, _lib.MK_FIELD_VARBYTES, _lib.MK_FIELD_STRUCT

CROSSLINK_FIELDS = [(_RAW, 0, 8), (_BY, 8, 32)]                    # 40-B records
ETH1_DATA_FIELDS = [(_BY, 0, 32), (_BY, 32, 32)]                   # 64-B records
ETH1_VOTE_FIELDS = [(_STRUCT, 0, 2)] + ETH1_DATA_FIELDS + [(_RAW, 64, 8)]  # 72-B records
# AttestationData at record offset 0 (192 B)
_ATT_DATA_FIELDS = [(_RAW, 0, 8), (_RAW, 8, 8), (_BY, 16, 32), (_BY, 48, 32), (_BY, 80, 32), (_BY, 112, 32),
                    (_RAW, 144, 8), (_BY, 152, 32), (_RAW, 184, 8)]


def pending_attestation_fields(bitfield_cap: int):
    """The PendingAttestationRecord layout for bitfield slots of
    ``bitfield_cap`` bytes (a multiple of 4): AttestationData, the two
    bitfield slots (le32 length + capacity), SlotIncluded; 13 entries."""
    if bitfield_cap % 4:
        raise ValueError("bitfield capacity must be a multiple of 4")
    slot = 4 + bitfield_cap
    return ([(_STRUCT, 0, len(_ATT_DATA_FIELDS))] + _ATT_DATA_FIELDS +
            [(_VAR, 192, bitfield_cap), (_VAR, 192 + slot, bitfield_cap), (_RAW, 192 + 2 * slot, 8)])


def pending_attestation_record_len(bitfield_cap: int) -> int:
    return 192 + 2 * (4 + bitfield_cap) + 8


PENDING_ATTESTATION_FIELDS = pending_attestation_fields(48)  # synthetic_state's bitfields: 16..47 bytes


def _le64(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype="<u8").reshape(-1, 1).view(np.uint8)


def _put_bitfields(rec: np.ndarray, off: int, cap: int, fields: List[bytes]) -> None:
    """le32(len) || bytes into the slot at column ``off`` of every record."""
    lens = np.fromiter((len(x) for x in fields), dtype=np.int64, count=len(fields))
    if len(fields) and lens.max() > cap:
        raise ValueError(f"bitfield of {int(lens.max())} bytes in a {cap}-byte slot")
    rec[:, off:off + 4] = lens.astype("<u4").reshape(-1, 1).view(np.uint8)
    flat = np.frombuffer(b"".join(fields), dtype=np.uint8)
    row = np.repeat(np.arange(len(fields)), lens)
    col = np.arange(flat.size) - np.repeat(np.cumsum(lens) - lens, lens)
    rec[row, off + 4 + col] = flat


def pack_attestations(att: "Attestations", bitfield_cap: int = None):
    """[]*PendingAttestationRecord as flat records: (records (a, record_len)
    uint8, fields).  The bitfield slots are sized to the longest bitfield
    rounded up to 4 (at least 4) unless ``bitfield_cap`` is given."""
    a = len(att)
    if bitfield_cap is None:
        longest = max([len(x) for x in att.aggregation_bitfield] + [len(x) for x in att.custody_bitfield] + [1])
        bitfield_cap = (longest + 3) & ~3
    slot = 4 + bitfield_cap
    rec = np.zeros((a, pending_attestation_record_len(bitfield_cap)), dtype=np.uint8)
    rec[:, 0:8] = _le64(att.slot)
    rec[:, 8:16] = _le64(att.shard)
    rec[:, 16:144] = np.asarray(att.roots, dtype=np.uint8).reshape(a, 128)
    rec[:, 144:152] = _le64(att.justified_epoch)
    rec[:, 152:184] = np.asarray(att.justified_root, dtype=np.uint8).reshape(a, 32)
    rec[:, 184:192] = _le64(att.justified_slot)
    _put_bitfields(rec, 192, bitfield_cap, att.aggregation_bitfield)
    _put_bitfields(rec, 192 + slot, bitfield_cap, att.custody_bitfield)
    rec[:, 192 + 2 * slot:] = _le64(att.slot_included)
    return rec, pending_attestation_fields(bitfield_cap)


# ---- records with list fields (MK_FIELD_LIST): le32(count), then `cap` item cells ------------
_LIST = _lib.MK_FIELD_LIST

# types.pb.go field order; the values are dicts (or objects) keyed by the Go field names
SLASHABLE_VOTE_SSZ = S.Struct("pb.SlashableVote", [
    ("ValidatorIndices", S.Slice(_U64)), ("CustodyBitfield", _B), ("Data", S.Ptr(ATTESTATION_DATA_SSZ)),
    ("AggregateSignature", _B)])
ATTESTER_SLASHING_SSZ = S.Struct("pb.AttesterSlashing", [
    ("SlashableVote_1", S.Ptr(SLASHABLE_VOTE_SSZ)), ("SlashableVote_2", S.Ptr(SLASHABLE_VOTE_SSZ))])
DEPOSIT_SSZ = S.Struct("pb.Deposit", [
    ("MerkleBranchHash32S", S.Slice(_B)), ("MerkleTreeIndex", _U64), ("DepositData", _B)])
DEPOSIT_BRANCH_CAP = 32  # DepositContractTreeDepth nodes of 32 bytes


def _shift(fields, base: int):
    """The layout moved to record offset ``base`` (struct entries and item
    descriptors keep their offset member: 0, or a stride)."""
    out, skip = [], False
    for kind, off, ln in fields:
        out.append((kind, off if kind == _STRUCT or skip else off + base, ln))
        skip = kind == _LIST  # the next entry is the item descriptor
    return out


def slashable_vote_record_len(indices_cap: int, bitfield_cap: int, signature_cap: int = 96) -> int:
    return 4 + 8 * indices_cap + 4 + bitfield_cap + 192 + 4 + signature_cap


def slashable_vote_fields(indices_cap: int, bitfield_cap: int, signature_cap: int = 96):
    """The SlashableVote layout: the validator indices as a list slot of
    ``indices_cap`` uint64 cells, the custody bitfield slot, AttestationData
    (192 B), the aggregate signature slot; 14 entries."""
    if bitfield_cap % 4 or signature_cap % 4:
        raise ValueError("bitfield and signature capacities must be multiples of 4")
    o1 = 4 + 8 * indices_cap
    o2 = o1 + 4 + bitfield_cap
    return ([(_LIST, 0, indices_cap), (_RAW, 8, 8), (_VAR, o1, bitfield_cap), (_STRUCT, 0, len(_ATT_DATA_FIELDS))] +
            _shift(_ATT_DATA_FIELDS, o2) + [(_VAR, o2 + 192, signature_cap)])


def _put_var(rec: np.ndarray, off: int, cap: int, b: bytes, what: str) -> None:
    if len(b) > cap:
        raise ValueError(f"{what} of {len(b)} bytes in a {cap}-byte slot")
    rec[off:off + 4] = np.frombuffer(_st.pack("<I", len(b)), dtype=np.uint8)
    rec[off + 4:off + 4 + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)


def _put_vote(rec: np.ndarray, v, indices_cap: int, bitfield_cap: int, signature_cap: int) -> None:
    idx = np.asarray(S._field(v, "ValidatorIndices"), dtype="<u8").reshape(-1)
    if idx.size > indices_cap:
        raise ValueError(f"{idx.size} validator indices in a slot of {indices_cap}")
    rec[0:4] = np.frombuffer(_st.pack("<I", idx.size), dtype=np.uint8)
    rec[4:4 + 8 * idx.size] = idx.view(np.uint8)
    o1 = 4 + 8 * indices_cap
    o2 = o1 + 4 + bitfield_cap
    _put_var(rec, o1, bitfield_cap, S._field(v, "CustodyBitfield"), "custody bitfield")
    d = S._field(v, "Data")
    data = rec[o2:o2 + 192]
    for name, off in (("Slot", 0), ("Shard", 8), ("JustifiedEpoch", 144), ("JustifiedSlot", 184)):
        data[off:off + 8] = np.frombuffer(_st.pack("<Q", int(S._field(d, name))), dtype=np.uint8)
    for name, off in (("BeaconBlockRootHash32", 16), ("EpochBoundaryRootHash32", 48), ("ShardBlockRootHash32", 80),
                      ("LatestCrosslinkRootHash32", 112), ("JustifiedBlockRootHash32", 152)):
        b = bytes(S._field(d, name))
        if len(b) != 32:
            raise ValueError(f"{name} of {len(b)} bytes in a 32-byte field")
        data[off:off + 32] = np.frombuffer(b, dtype=np.uint8)
    _put_var(rec, o2 + 192, signature_cap, S._field(v, "AggregateSignature"), "aggregate signature")


def pack_slashable_votes(votes, indices_cap: int, bitfield_cap: int, signature_cap: int = 96):
    """[]*SlashableVote as flat records: (records (n, record_len) uint8, fields)."""
    fields = slashable_vote_fields(indices_cap, bitfield_cap, signature_cap)
    rec = np.zeros((len(votes), slashable_vote_record_len(indices_cap, bitfield_cap, signature_cap)), dtype=np.uint8)
    for i, v in enumerate(votes):
        _put_vote(rec[i], v, indices_cap, bitfield_cap, signature_cap)
    return rec, fields


def attester_slashing_fields(indices_cap: int, bitfield_cap: int, signature_cap: int = 96):
    """AttesterSlashing: its two SlashableVotes by value, one behind the
    other (a list inside a nested struct); 30 entries."""
    vote = slashable_vote_fields(indices_cap, bitfield_cap, signature_cap)
    vlen = slashable_vote_record_len(indices_cap, bitfield_cap, signature_cap)
    return [(_STRUCT, 0, len(vote))] + vote + [(_STRUCT, 0, len(vote))] + _shift(vote, vlen)


def pack_attester_slashings(slashings, indices_cap: int, bitfield_cap: int, signature_cap: int = 96):
    """[]*AttesterSlashing as flat records: (records, fields)."""
    vlen = slashable_vote_record_len(indices_cap, bitfield_cap, signature_cap)
    rec = np.zeros((len(slashings), 2 * vlen), dtype=np.uint8)
    for i, s in enumerate(slashings):
        _put_vote(rec[i, :vlen], S._field(s, "SlashableVote_1"), indices_cap, bitfield_cap, signature_cap)
        _put_vote(rec[i, vlen:], S._field(s, "SlashableVote_2"), indices_cap, bitfield_cap, signature_cap)
    return rec, attester_slashing_fields(indices_cap, bitfield_cap, signature_cap)


_DEP_INDEX = 8 + 32 * DEPOSIT_BRANCH_CAP  # the branch slot (4 + 1024 B) rounded up to 8


def deposit_record_len(data_cap: int) -> int:
    return _DEP_INDEX + 8 + 4 + data_cap


def deposit_fields(data_cap: int):
    """Deposit: the Merkle branch as a list slot of 32 cells of 32 bytes,
    the tree index, the deposit data slot; 4 entries."""
    if data_cap % 4:
        raise ValueError("deposit data capacity must be a multiple of 4")
    return [(_LIST, 0, DEPOSIT_BRANCH_CAP), (_BY, 32, 32), (_RAW, _DEP_INDEX, 8), (_VAR, _DEP_INDEX + 8, data_cap)]


def pack_deposits(deposits, data_cap: int):
    """[]*Deposit as flat records: (records, fields)."""
    rec = np.zeros((len(deposits), deposit_record_len(data_cap)), dtype=np.uint8)
    for i, d in enumerate(deposits):
        branch = [bytes(b) for b in S._field(d, "MerkleBranchHash32S")]
        if len(branch) > DEPOSIT_BRANCH_CAP:
            raise ValueError(f"Merkle branch of {len(branch)} nodes in a slot of {DEPOSIT_BRANCH_CAP}")
        if any(len(b) != 32 for b in branch):
            raise ValueError("Merkle branch nodes must be 32 bytes")
        rec[i, 0:4] = np.frombuffer(_st.pack("<I", len(branch)), dtype=np.uint8)
        rec[i, 4:4 + 32 * len(branch)] = np.frombuffer(b"".join(branch), dtype=np.uint8)
        rec[i, _DEP_INDEX:_DEP_INDEX + 8] = np.frombuffer(_st.pack("<Q", int(S._field(d, "MerkleTreeIndex"))),
                                                          dtype=np.uint8)
        _put_var(rec[i], _DEP_INDEX + 8, data_cap, S._field(d, "DepositData"), "deposit data")
    return rec, deposit_fields(data_cap)


def pack_eth1_votes(votes: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """[]*Eth1DataVote as (v, 72) uint8 records of ETH1_VOTE_FIELDS."""
    v = len(votes)
    rec = np.empty((v, 72), dtype=np.uint8)
    rec[:, :64] = np.asarray(votes, dtype=np.uint8).reshape(v, 64)
    rec[:, 64:] = _le64(counts)
    return rec


def pack_crosslinks(epochs: np.ndarray, roots: np.ndarray) -> np.ndarray:
    """[]*CrosslinkRecord as (s, 40) uint8 records of CROSSLINK_FIELDS."""
    s = len(epochs)
    rec = np.empty((s, 40), dtype=np.uint8)
    rec[:, :8] = _le64(epochs)
    rec[:, 8:] = np.asarray(roots, dtype=np.uint8).reshape(s, 32)
    return rec


def struct_list_root_packed(rec: np.ndarray, fields) -> bytes:
    """TreeHash of a list of packed records ((n, record_len) uint8)."""
    import ctypes

    rec = np.ascontiguousarray(rec, dtype=np.uint8)
    out = ctypes.create_string_buffer(32)
    _lib.invoke("mk_ssz_struct_list_root", _ptr(rec) if rec.size else None, rec.shape[0], rec.shape[1],
                R._fields(fields), len(fields), out)
    return out.raw


def struct_roots_packed(rec: np.ndarray, fields) -> np.ndarray:
    """Struct root of every packed record -> (n, 32) uint8."""
    rec = np.ascontiguousarray(rec, dtype=np.uint8)
    out = np.empty((rec.shape[0], 32), dtype=np.uint8)
    _lib.invoke("mk_ssz_struct_roots", _ptr(rec) if rec.size else None, rec.shape[0], rec.shape[1],
                R._fields(fields), len(fields), _ptr(out))
    return out


@dataclass
class BeaconState:
    """A synthetic, SSZ-legal pb.BeaconState with its lists as flat arrays."""
    registry: R.ValidatorRegistry
    balances: np.ndarray                 # u64 (n,)
    randao_mixes: np.ndarray             # (8192, 32)
    seeds: np.ndarray                    # (2, 32): previous, current epoch seed
    crosslink_epochs: np.ndarray         # u64 (1024,)
    crosslink_roots: np.ndarray          # (1024, 32)
    latest_block_roots: np.ndarray       # (8192, 32)
    batched_block_roots: np.ndarray      # (m, 32)
    penalized_balances: np.ndarray       # u64 (8192,)
    attestations: Attestations
    index_roots: np.ndarray              # (8192, 32)
    eth1_data: np.ndarray                # (2, 32): deposit root, block hash
    eth1_votes: np.ndarray               # (v, 2, 32)
    eth1_vote_counts: np.ndarray         # u64 (v,)
    fork: np.ndarray                     # u64 (3,)
    scalars: dict = field(default_factory=dict)

    # ---------------------------------------------------------------- the engine path
    def tree_hash_ssz(self) -> bytes:
        """ssz.TreeHash(state): a fixed number of library calls, no per-element Python work."""
        # 1. hashedEncoding of the 32-B list elements and state fields, one fixed-length batch
        b32 = np.concatenate([self.randao_mixes, self.seeds, self.latest_block_roots, self.batched_block_roots,
                              self.index_roots])
        msgs = np.empty((len(b32), 36), dtype=np.uint8)
        msgs[:, :4] = np.frombuffer(_st.pack("<I", 32), dtype=np.uint8)
        msgs[:, 4:] = b32
        h = hash_batch(msgs, 36)
        cut = np.cumsum([0, len(self.randao_mixes), 2, len(self.latest_block_roots), len(self.batched_block_roots),
                         len(self.index_roots)])
        h_randao, h_seeds, h_block, h_batched, h_index = (h[cut[i]:cut[i + 1]] for i in range(5))
        # 2. the registry (typed Hashable path: struct kernel + merkleHash)
        reg_root = self.registry.tree_hash_ssz()
        # 3. the struct lists from packed records: nested structs and bitfields hash on the device
        cross_root = struct_list_root_packed(pack_crosslinks(self.crosslink_epochs, self.crosslink_roots),
                                             CROSSLINK_FIELDS)
        att_rec, att_fields = pack_attestations(self.attestations)
        att_root = struct_list_root_packed(att_rec, att_fields)
        votes_root = struct_list_root_packed(pack_eth1_votes(self.eth1_votes, self.eth1_vote_counts),
                                             ETH1_VOTE_FIELDS)
        eth1_root = bytes(struct_roots_packed(np.ascontiguousarray(self.eth1_data, dtype=np.uint8).reshape(1, 64),
                                              ETH1_DATA_FIELDS)[0])
        # 4. every other list of the state in one segmented merkleHash call
        lists = [(self.balances.astype("<u8").view(np.uint8), len(self.balances), 8),
                 (h_randao, len(h_randao), 32), (h_block, len(h_block), 32), (h_batched, len(h_batched), 32),
                 (self.penalized_balances.astype("<u8").view(np.uint8), len(self.penalized_balances), 8),
                 (h_index, len(h_index), 32)]
        buf, offs, pos = [], [], 0
        for arr, _, _ in lists:
            pad = (-pos) % 16
            buf.append(np.zeros(pad, np.uint8))
            pos += pad
            offs.append(pos)
            flat = np.ascontiguousarray(arr, dtype=np.uint8).reshape(-1)
            buf.append(flat)
            pos += flat.size
        roots = _merkle_many_mixed(np.concatenate(buf), offs, [x[1] for x in lists], [x[2] for x in lists])
        bal_root, randao_root, block_root, batched_root, pen_root, index_root = roots
        # 5. the state struct: field outputs in declaration order
        sc = self.scalars
        u = lambda name: _st.pack("<Q", int(sc[name]))  # noqa: E731
        fork_root = hash_batch_var([b"".join(_st.pack("<Q", int(x)) for x in self.fork)])[0]
        msg = b"".join([
            reg_root, u("ValidatorRegistryUpdateEpoch"), bal_root, randao_root, u("PreviousEpochStartShard"),
            u("CurrentEpochStartShard"), u("PreviousCalculationEpoch"), u("CurrentCalculationEpoch"),
            bytes(h_seeds[0]), bytes(h_seeds[1]), u("PreviousJustifiedEpoch"), u("JustifiedEpoch"),
            u("JustificationBitfield"), u("FinalizedEpoch"), cross_root, block_root, batched_root, pen_root,
            att_root, index_root, eth1_root, votes_root, u("GenesisTime"), fork_root, u("Slot")])
        return hash_batch_var([msg])[0]

    TreeHashSSZ = tree_hash_ssz

    # ---------------------------------------------------------------- reflective form
    def as_value(self) -> dict:
        """The same state as a value of STATE_SSZ (dicts / lists / bytes) for the
        reflective mirror and the oracle."""
        att = self.attestations
        b = lambda a: [bytes(r) for r in a]  # noqa: E731
        d = {
            "ValidatorRegistry": self.registry.as_dicts(),
            "ValidatorBalances": [int(x) for x in self.balances],
            "LatestRandaoMixesHash32S": b(self.randao_mixes),
            "PreviousEpochSeedHash32": bytes(self.seeds[0]), "CurrentEpochSeedHash32": bytes(self.seeds[1]),
            "LatestCrosslinks": [{"Epoch": int(e), "ShardBlockRootHash32": bytes(r)}
                                 for e, r in zip(self.crosslink_epochs, self.crosslink_roots)],
            "LatestBlockRootHash32S": b(self.latest_block_roots),
            "BatchedBlockRootHash32S": b(self.batched_block_roots),
            "LatestPenalizedBalances": [int(x) for x in self.penalized_balances],
            "LatestAttestations": [{
                "Data": {"Slot": int(att.slot[i]), "Shard": int(att.shard[i]),
                         "BeaconBlockRootHash32": bytes(att.roots[i, 0]),
                         "EpochBoundaryRootHash32": bytes(att.roots[i, 1]),
                         "ShardBlockRootHash32": bytes(att.roots[i, 2]),
                         "LatestCrosslinkRootHash32": bytes(att.roots[i, 3]),
                         "JustifiedEpoch": int(att.justified_epoch[i]),
                         "JustifiedBlockRootHash32": bytes(att.justified_root[i]),
                         "JustifiedSlot": int(att.justified_slot[i])},
                "AggregationBitfield": att.aggregation_bitfield[i], "CustodyBitfield": att.custody_bitfield[i],
                "SlotIncluded": int(att.slot_included[i])} for i in range(len(att))],
            "LatestIndexRootHash32S": b(self.index_roots),
            "LatestEth1Data": {"DepositRootHash32": bytes(self.eth1_data[0]), "BlockHash32": bytes(self.eth1_data[1])},
            "Eth1DataVotes": [{"Eth1Data": {"DepositRootHash32": bytes(x[0]), "BlockHash32": bytes(x[1])},
                               "VoteCount": int(c)} for x, c in zip(self.eth1_votes, self.eth1_vote_counts)],
            "Fork": {"PreviousVersion": int(self.fork[0]), "CurrentVersion": int(self.fork[1]),
                     "Epoch": int(self.fork[2])},
            "XXX_NoUnkeyedLiteral": None, "XXX_unrecognized": b"", "XXX_sizecache": 0,
        }
        for name in _SCALARS:
            d[name] = int(self.scalars[name])
        return d


def _merkle_many_mixed(buf: np.ndarray, offs, ns, item_lens) -> List[bytes]:
    """mk_ssz_merkle_many with per-list item lengths (host buffer)."""
    from . import _lib
    from .hashutil import _ptr

    k = len(ns)
    o = np.ascontiguousarray(offs, dtype=np.uint64)
    n = np.ascontiguousarray(ns, dtype=np.uint64)
    il = np.ascontiguousarray(item_lens, dtype=np.uint32)
    out = np.empty((k, 32), dtype=np.uint8)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    _lib.invoke("mk_ssz_merkle_many", _ptr(buf), _ptr(o), _ptr(n), _ptr(il), k, _ptr(out))
    return [bytes(r) for r in out]


def synthetic_state(n_validators: int, seed: int, n_attestations: int = 128, n_batched: int = 16,
                    n_votes: int = 4, lists_len: int = LATEST_BLOCK_ROOTS_LENGTH,
                    shards: int = SHARD_COUNT) -> BeaconState:
    """A synthetic BeaconState from the SplitMix64 stream:
    the registry and balances of registry.py, the 8192-entry root arrays,
    1024 crosslinks, `n_attestations` pending attestations with bitfields of
    16..48 bytes, `n_batched` batched block roots and `n_votes` eth1 votes."""
    words = iter(range(1, 1 << 20))

    def rnd(nbytes: int) -> np.ndarray:
        w = R.splitmix_words(seed + 1000 * next(words), 0, (nbytes + 7) // 8)
        return w.view(np.uint8)[:nbytes].copy()

    def u64(count: int, mask: int = (1 << 40) - 1) -> np.ndarray:
        return R.splitmix_words(seed + 1000 * next(words), 0, count) & np.uint64(mask)

    a = n_attestations
    agg_len = 16 + (u64(a, 31) & np.uint64(31)).astype(np.int64)
    cust_len = 16 + (u64(a, 31) & np.uint64(31)).astype(np.int64)
    att = Attestations(
        slot=u64(a), shard=u64(a, shards - 1), roots=rnd(a * 128).reshape(a, 4, 32), justified_epoch=u64(a),
        justified_root=rnd(a * 32).reshape(a, 32), justified_slot=u64(a),
        aggregation_bitfield=[bytes(rnd(int(L))) for L in agg_len],
        custody_bitfield=[bytes(rnd(int(L))) for L in cust_len], slot_included=u64(a))
    st = BeaconState(
        registry=R.synthetic_registry(n_validators, seed), balances=R.synthetic_balances(n_validators, seed),
        randao_mixes=rnd(lists_len * 32).reshape(lists_len, 32), seeds=rnd(64).reshape(2, 32),
        crosslink_epochs=u64(shards), crosslink_roots=rnd(shards * 32).reshape(shards, 32),
        latest_block_roots=rnd(lists_len * 32).reshape(lists_len, 32),
        batched_block_roots=rnd(n_batched * 32).reshape(n_batched, 32),
        penalized_balances=u64(lists_len, (1 << 45) - 1), attestations=att,
        index_roots=rnd(lists_len * 32).reshape(lists_len, 32), eth1_data=rnd(64).reshape(2, 32),
        eth1_votes=rnd(n_votes * 64).reshape(n_votes, 2, 32), eth1_vote_counts=u64(n_votes, 1023),
        fork=u64(3, 15))
    sc = u64(len(_SCALARS))
    st.scalars = {name: int(x) for name, x in zip(_SCALARS, sc)}
    return st


# ---------------------------------------------------------------- the resident state
# offset of every field output in the state's 536-B hash message (tree_hash_ssz step 5)
def _container_layout():
    offs, pos = {}, 0
    for name, typ in STATE_FIELDS[:25]:
        offs[name] = pos
        pos += 8 if typ is _U64 else 32
    return offs, pos


CONTAINER_OFF, CONTAINER_LEN = _container_layout()

# the ten list fields in STATE_FIELDS order: (BeaconState attribute, state field, tree kind, item length, layout)
_K_LIST, _K_STRUCT, _K_BYTES = _lib.MK_TREE_LIST, _lib.MK_TREE_STRUCT, _lib.MK_TREE_BYTES
RESIDENT_TREES = [
    ("registry", "ValidatorRegistry", _K_STRUCT, R.VALIDATOR_DTYPE.itemsize, R.VALIDATOR_FIELDS),
    ("balances", "ValidatorBalances", _K_LIST, 8, None),
    ("randao_mixes", "LatestRandaoMixesHash32S", _K_BYTES, 32, None),
    ("crosslinks", "LatestCrosslinks", _K_STRUCT, 40, CROSSLINK_FIELDS),
    ("latest_block_roots", "LatestBlockRootHash32S", _K_BYTES, 32, None),
    ("batched_block_roots", "BatchedBlockRootHash32S", _K_BYTES, 32, None),
    ("penalized_balances", "LatestPenalizedBalances", _K_LIST, 8, None),
    ("attestations", "LatestAttestations", _K_STRUCT, pending_attestation_record_len(48), PENDING_ATTESTATION_FIELDS),
    ("index_roots", "LatestIndexRootHash32S", _K_BYTES, 32, None),
    ("eth1_votes", "Eth1DataVotes", _K_STRUCT, 72, ETH1_VOTE_FIELDS),
]
# the dirty share from which each kind's host handle rebuilds instead of climbing
_REBUILD_DIV = {_K_LIST: _lib.LIST_TREE_REBUILD_DIV, _K_STRUCT: _lib.STRUCT_TREE_REBUILD_DIV,
                _K_BYTES: _lib.BYTES_TREE_REBUILD_DIV}


def widen_attestation_records(rec: np.ndarray, old_cap: int, new_cap: int) -> np.ndarray:
    """Packed PendingAttestationRecords moved to bitfield slots of ``new_cap`` bytes."""
    so, sn = 4 + old_cap, 4 + new_cap
    out = np.zeros((rec.shape[0], pending_attestation_record_len(new_cap)), dtype=np.uint8)
    out[:, :192] = rec[:, :192]
    out[:, 192:192 + so] = rec[:, 192:192 + so]
    out[:, 192 + sn:192 + sn + so] = rec[:, 192 + so:192 + 2 * so]
    out[:, 192 + 2 * sn:] = rec[:, 192 + 2 * so:]
    return out


class _ResidentTree:
    """One list of the resident state: its items, level 0, levels and root in
    HBM, and the changes made since the last root (host side)."""

    def __init__(self, kind: int, item_len: int, spec, device):
        self.kind, self.item_len, self.spec, self.device = kind, item_len, spec, device
        self.n = self.cap = 0
        self.items = self.level0 = self.levels = None
        import torch

        self.root = torch.zeros(32, dtype=torch.uint8, device=device)
        self.pending = {}    # index -> row, the last value of a repeated index
        self.appended = []   # rows

    def __len__(self):
        return self.n + len(self.appended)

    def _rows(self, values) -> np.ndarray:
        a = np.ascontiguousarray(values)
        a = a.view(np.uint8) if a.dtype != np.uint8 else a
        if a.size % self.item_len:
            raise ValueError(f"{a.size} bytes are not a whole number of {self.item_len}-byte items")
        return a.reshape(-1, self.item_len)

    def _alloc(self, cap: int) -> None:
        import torch

        from . import device as D

        self.cap = cap
        self.items = torch.zeros(cap * self.item_len + 16, dtype=torch.uint8, device=self.device)
        len0 = self.item_len
        if self.kind != _K_LIST:
            self.level0 = torch.zeros(32 * cap + 16, dtype=torch.uint8, device=self.device)
            len0 = 32
        self.levels = torch.zeros(max(D.list_tree_levels_bytes(cap, len0), 16), dtype=torch.uint8, device=self.device)

    def _build(self) -> None:
        from . import device as D

        if self.kind == _K_LIST:
            D.list_tree_build(self.items, self.n, self.cap, self.item_len, self.levels, self.root)
        elif self.kind == _K_STRUCT:
            D.struct_list_tree_build(self.items, self.n, self.cap, self.item_len, self.spec, self.level0, self.levels,
                                     self.root)
        else:
            D.bytes_list_tree_build(self.items, self.n, self.cap, self.item_len, self.level0, self.levels, self.root)

    def replace(self, values) -> None:
        """Any new content, through the build entry."""
        import torch

        rows = self._rows(values)
        n = rows.shape[0]
        if self.items is None or n > self.cap:
            self._alloc(max(n, 1))
        if n:
            self.items[:n * self.item_len].copy_(torch.from_numpy(rows.reshape(-1)))
        self.n = n
        self.pending, self.appended = {}, []
        self._build()

    def update(self, indices, values) -> None:
        idx = [int(i) for i in np.asarray(indices).reshape(-1)]
        rows = self._rows(values)
        if len(idx) != rows.shape[0]:
            raise ValueError("one value per index")
        for i in idx:
            if i < 0 or i >= len(self):
                raise IndexError(f"index {i} beyond {len(self)} items")
        for i, row in zip(idx, rows):
            if i >= self.n:
                self.appended[i - self.n] = row.copy()
            else:
                self.pending[i] = row.copy()

    def append(self, values) -> None:
        self.appended.extend(r.copy() for r in self._rows(values))

    def _write_through(self) -> None:
        """The pending changes straight into the item buffer (then a build follows)."""
        import torch

        view = self.items[:self.cap * self.item_len].view(self.cap, self.item_len)
        if self.pending:
            idx = sorted(self.pending)
            vals = np.stack([self.pending[i] for i in idx])
            view[torch.tensor(idx, dtype=torch.int64, device=self.device)] = torch.from_numpy(vals).to(self.device)
        if self.appended:
            view[self.n:self.n + len(self.appended)] = torch.from_numpy(np.stack(self.appended)).to(self.device)
        self.n += len(self.appended)
        self.pending, self.appended = {}, []

    def flush(self, container_off: int):
        """This tree's entry of the next trees_update.  A list that outgrew its
        capacity (doubled, moved) or is dirty enough for its host handle to
        rebuild goes through the build entry and enters with nothing dirty."""
        import torch

        from . import device as D

        n_new, dirty = len(self), len(self.pending) + len(self.appended)
        if n_new > self.cap:
            old, n = self.items, self.n
            self._alloc(max(2 * self.cap, n_new))
            self.items[:n * self.item_len].copy_(old[:n * self.item_len])
            self._write_through()
            self._build()
        elif dirty and n_new // _REBUILD_DIV[self.kind] <= dirty:
            self._write_through()
            self._build()
        idx = vals = None
        k = len(self.pending)
        if self.pending or self.appended:
            order = sorted(self.pending)
            rows = [self.pending[i] for i in order] + self.appended
            vals = torch.from_numpy(np.stack(rows).reshape(-1)).to(self.device)
            if k:
                idx = torch.tensor(order, dtype=torch.int64, device=self.device)
        t = D.TreeArgs(self.kind, self.items, self.n, len(self), self.cap, self.item_len, self.levels, self.root,
                       level0=self.level0, idx=idx, k_idx=k, values=vals, spec=self.spec, container_off=container_off)
        self.n = len(self)
        self.pending, self.appended = {}, []
        return t


class ResidentBeaconState:
    """A whole ``BeaconState`` kept in HBM: the ten lists as
    resident trees (registry, crosslinks, attestations and votes as struct
    trees, the balances as list trees, the four root arrays as bytes trees),
    the 536-B hash message of the state struct beside them.  Changes are
    collected on the host; ``root()`` is ONE ``device.trees_update`` over the
    ten trees -- every climb and the state hash in one launch -- and one 32-B
    read-back.  Everything runs on torch's current stream of ``device``.

    Values are packed rows: ``VALIDATOR_DTYPE`` records, u64 balances, (k, 32)
    roots, ``pack_crosslinks`` / ``pack_eth1_votes`` records; attestations go
    in as an ``Attestations``."""

    def __init__(self, device="cuda"):
        import torch

        self.device = torch.device(device)
        self.trees = {attr: _ResidentTree(kind, item_len, spec, self.device)
                      for attr, _, kind, item_len, spec in RESIDENT_TREES}
        self._off = {attr: CONTAINER_OFF[field_name] for attr, field_name, _, _, _ in RESIDENT_TREES}
        self.container = torch.zeros(CONTAINER_LEN + 8, dtype=torch.uint8, device=self.device)
        self.state_root = torch.zeros(32, dtype=torch.uint8, device=self.device)
        self._ws = None
        self._att_cap = 48

    # ---- the small fields: written into the message when they are set
    def _put(self, off: int, data: bytes) -> None:
        import torch

        self.container[off:off + len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))

    def set_scalar(self, name: str, value: int) -> None:
        if name not in _SCALARS:
            raise KeyError(name)
        self._put(CONTAINER_OFF[name], _st.pack("<Q", int(value)))

    def set_seeds(self, previous: bytes, current: bytes) -> None:
        msgs = np.empty((2, 36), dtype=np.uint8)
        msgs[:, :4] = np.frombuffer(_st.pack("<I", 32), dtype=np.uint8)
        msgs[0, 4:] = np.frombuffer(bytes(previous), dtype=np.uint8)
        msgs[1, 4:] = np.frombuffer(bytes(current), dtype=np.uint8)
        h = hash_batch(msgs, 36)
        self._put(CONTAINER_OFF["PreviousEpochSeedHash32"], bytes(h[0]) + bytes(h[1]))

    def set_eth1_data(self, eth1_data) -> None:
        rec = np.ascontiguousarray(eth1_data, dtype=np.uint8).reshape(1, 64)
        self._put(CONTAINER_OFF["LatestEth1Data"], bytes(struct_roots_packed(rec, ETH1_DATA_FIELDS)[0]))

    def set_fork(self, fork) -> None:
        msg = b"".join(_st.pack("<Q", int(x)) for x in fork)
        self._put(CONTAINER_OFF["Fork"], hash_batch_var([msg])[0])

    # ---- the lists
    def _att_rows(self, att: "Attestations") -> np.ndarray:
        """``att`` packed for the attestation tree; bitfields longer than its
        slots widen the layout: the resident records are repacked and the tree
        rebuilt."""
        longest = max([len(x) for x in att.aggregation_bitfield] + [len(x) for x in att.custody_bitfield] + [0])
        t = self.trees["attestations"]
        if longest > self._att_cap:
            new_cap = max(2 * self._att_cap, (longest + 3) & ~3)
            rows = np.zeros((t.n, t.item_len), np.uint8)
            if t.n:  # the resident records with their pending changes, then the pending appends
                rows = t.items[:t.n * t.item_len].cpu().numpy().reshape(t.n, t.item_len).copy()
            for i, row in t.pending.items():
                rows[i] = row
            rows = np.concatenate([rows] + [r.reshape(1, -1) for r in t.appended])
            rows = widen_attestation_records(rows, self._att_cap, new_cap)
            self._att_cap = new_cap
            t.item_len, t.spec = pending_attestation_record_len(new_cap), pending_attestation_fields(new_cap)
            t.items = None  # another record length: new buffers
            t.replace(rows)
        return pack_attestations(att, self._att_cap)[0]

    def _rows(self, name: str, values):
        if name == "attestations" and isinstance(values, Attestations):
            return self._att_rows(values)
        return values

    def assign(self, state: BeaconState) -> None:
        """Every tree built from ``state`` (the build entry points), every small field set."""
        for name in _SCALARS:
            self.set_scalar(name, state.scalars[name])
        self.set_seeds(bytes(state.seeds[0]), bytes(state.seeds[1]))
        self.set_eth1_data(state.eth1_data)
        self.set_fork(state.fork)
        self.replace("registry", state.registry.records)
        self.replace("balances", state.balances.astype("<u8"))
        self.replace("randao_mixes", state.randao_mixes)
        self.replace("crosslinks", pack_crosslinks(state.crosslink_epochs, state.crosslink_roots))
        self.replace("latest_block_roots", state.latest_block_roots)
        self.replace("batched_block_roots", state.batched_block_roots)
        self.replace("penalized_balances", state.penalized_balances.astype("<u8"))
        self.replace("attestations", state.attestations)
        self.replace("index_roots", state.index_roots)
        self.replace("eth1_votes", pack_eth1_votes(state.eth1_votes, state.eth1_vote_counts))

    def count(self, name: str) -> int:
        """Items of list ``name``, pending appends included."""
        return len(self.trees[name])

    def update(self, name: str, indices, values) -> None:
        """list[indices[j]] = values[j] in order (of a repeated index the last
        value wins); an index >= len raises and changes nothing."""
        t = self.trees[name]
        for i in np.asarray(indices).reshape(-1):  # before anything changes (packing may widen the attestation slots)
            if int(i) < 0 or int(i) >= len(t):
                raise IndexError(f"{name}: index {int(i)} beyond {len(t)} items")
        t.update(indices, self._rows(name, values))

    def append(self, name: str, values) -> None:
        """Append; past the capacity the list doubles it and is rebuilt."""
        rows = self._rows(name, values)
        self.trees[name].append(rows)

    def replace(self, name: str, values) -> None:
        """Any new content for a list, a shorter one included, through the build entry."""
        if name == "attestations" and isinstance(values, Attestations):
            t = self.trees[name]
            t.n, t.pending, t.appended = 0, {}, []  # nothing to carry over should the slots widen
            values = self._att_rows(values)
        self.trees[name].replace(values)

    def root(self) -> bytes:
        """The state root: one trees_update over the ten trees (a rebuilt tree
        enters with nothing dirty, so its root still reaches the message), one
        32-B read-back."""
        import torch

        from . import device as D

        with torch.cuda.device(self.device):
            trees = [self.trees[attr].flush(self._off[attr]) for attr, *_ in RESIDENT_TREES]
            need = D.trees_update_workspace_bytes(trees)
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            D.trees_update(trees, self.container, CONTAINER_LEN, self.state_root, self._ws)
            return bytes(self.state_root.cpu().numpy())


# ---------------------------------------------------------------- the resident state behind one C handle
from .listtree import TreeSet  # noqa: E402


class BeaconTreeSet(TreeSet):
    """A ``listtree.TreeSet`` with the ten trees of ``RESIDENT_TREES`` at
    ``CONTAINER_OFF`` in a ``CONTAINER_LEN`` message (``mk_tree_set``, DESIGN.md
    §5j): what a cgo caller holds for a ``pb.BeaconState``.  A tree goes by its
    number or its ``RESIDENT_TREES`` attribute name; values are packed rows as
    for ``ResidentBeaconState`` (an ``Attestations`` is packed into 48-byte
    bitfield slots)."""

    def __init__(self, device: int = -1):
        super().__init__(CONTAINER_LEN, device=device)
        self.tree = {attr: self.add(kind, item_len, fields=spec, container_off=CONTAINER_OFF[field_name])
                     for attr, field_name, kind, item_len, spec in RESIDENT_TREES}

    def _tree(self, tree) -> int:
        return self.tree[tree] if isinstance(tree, str) else int(tree)

    def _flat(self, tree: int, values) -> np.ndarray:
        if isinstance(values, Attestations):
            values = pack_attestations(values, 48)[0]
        return super()._flat(tree, values)

    # ---- the small fields: their outputs into the message
    def set_scalar(self, name: str, value: int) -> None:
        if name not in _SCALARS:
            raise KeyError(name)
        self.put(CONTAINER_OFF[name], _st.pack("<Q", int(value)))

    def set_seeds(self, previous: bytes, current: bytes) -> None:
        msgs = np.empty((2, 36), dtype=np.uint8)
        msgs[:, :4] = np.frombuffer(_st.pack("<I", 32), dtype=np.uint8)
        msgs[0, 4:] = np.frombuffer(bytes(previous), dtype=np.uint8)
        msgs[1, 4:] = np.frombuffer(bytes(current), dtype=np.uint8)
        h = hash_batch(msgs, 36)
        self.put(CONTAINER_OFF["PreviousEpochSeedHash32"], bytes(h[0]) + bytes(h[1]))

    def set_eth1_data(self, eth1_data) -> None:
        rec = np.ascontiguousarray(eth1_data, dtype=np.uint8).reshape(1, 64)
        self.put(CONTAINER_OFF["LatestEth1Data"], bytes(struct_roots_packed(rec, ETH1_DATA_FIELDS)[0]))

    def set_fork(self, fork) -> None:
        msg = b"".join(_st.pack("<Q", int(x)) for x in fork)
        self.put(CONTAINER_OFF["Fork"], hash_batch_var([msg])[0])

    def clone(self) -> "BeaconTreeSet":
        """A second resident state (``TreeSet.clone``) that knows
        its trees by the same names: run a block's transition on it, compare
        ``root()`` with the block's state root, keep it or drop it."""
        return super().clone()

    def verify_randao(self, proposer_indices, reveals, max_layers: int = _lib.MK_REPEAT_MAX_LAYERS) -> np.ndarray:
        """verifyBlockRandao (block_operations.go:109-123) for a batch of blocks
        against the resident registry: verdict j is 1 where
        ``RepeatHash(reveals[j], proposer.RandaoLayers) ==
        proposer.RandaoCommitmentHash32`` for validator ``proposer_indices[j]``,
        0 where not, 2 where RandaoLayers exceeds ``max_layers``
        (``TreeSet.verify_repeat_hash`` with the ValidatorRecord's offsets; no
        record is read back, pending registry updates are seen)."""
        return self.verify_repeat_hash("registry", proposer_indices, reveals, R.RANDAO_COMMITMENT_OFF,
                                       R.RANDAO_LAYERS_OFF, max_layers)

    def assign_state(self, state: BeaconState) -> None:
        """Every small field put, every list assigned from ``state``."""
        for name in _SCALARS:
            self.set_scalar(name, state.scalars[name])
        self.set_seeds(bytes(state.seeds[0]), bytes(state.seeds[1]))
        self.set_eth1_data(state.eth1_data)
        self.set_fork(state.fork)
        self.assign("registry", state.registry.records)
        self.assign("balances", state.balances.astype("<u8"))
        self.assign("randao_mixes", state.randao_mixes)
        self.assign("crosslinks", pack_crosslinks(state.crosslink_epochs, state.crosslink_roots))
        self.assign("latest_block_roots", state.latest_block_roots)
        self.assign("batched_block_roots", state.batched_block_roots)
        self.assign("penalized_balances", state.penalized_balances.astype("<u8"))
        self.assign("attestations", state.attestations)
        self.assign("index_roots", state.index_roots)
        self.assign("eth1_votes", pack_eth1_votes(state.eth1_votes, state.eth1_vote_counts))


def beacon_tree_set(state: BeaconState = None, device: int = -1) -> BeaconTreeSet:
    """The tree set of a ``pb.BeaconState`` (filled from ``state`` when given):
    ``root()`` is ssz.TreeHash of the state -- one upload, one update over the
    ten trees, one 32-B read-back."""
    s = BeaconTreeSet(device=device)
    if state is not None:
        s.assign_state(state)
    return s
