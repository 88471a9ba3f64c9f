"""Nested structs and variable-length byte fields on the device
(MK_FIELD_STRUCT, MK_FIELD_VARBYTES; k_struct_nested): struct roots, list
roots, the registry tree and the state's packers against the oracle's
reflective hasher (oracle/ssz_ref.py, shared/ssz/hash.go:23-239) over the same
values as dicts -- never against the library itself.

A test type is a list of fields: ("u", bits) a scalar, ("b", n) a []byte of
fixed length n, ("v", cap) a []byte of varying length in a slot of capacity
cap, ("s", [fields]) a pointer to a struct.  From one such description come
the mk_field layout, the packed records, the oracle's type and its values."""
import numpy as np
import pytest

from prysm_amd import _lib

pytestmark = pytest.mark.gpu

B, R, V, S = _lib.MK_FIELD_BYTES, _lib.MK_FIELD_RAW, _lib.MK_FIELD_VARBYTES, _lib.MK_FIELD_STRUCT
SEED = 0x5EED000000000000 + 2900
H32, U64 = ("b", 32), ("u", 64)
CAP = 136                                       # bitfield slot capacity of the test layouts
VAR_LENS = [0, 1, 3, 4, 131, 132, 133, CAP]     # 4 + L crosses the 136-B rate; mixed within a wave
N_MAX = 257
SIZES = [1, 2, 63, 64, 65, 257]

ATT_DATA = [U64, U64, H32, H32, H32, H32, U64, H32, U64]
TYPES = {
    # pb.PendingAttestationRecord: message 104 B, AttestationData 192 B (two blocks)
    "attestation": [("s", ATT_DATA), ("v", CAP), ("v", CAP), U64],
    # pb.Eth1DataVote
    "eth1_vote": [("s", [H32, H32]), U64],
    # depth 4, scalars of 1 / 2 / 4 bytes at odd offsets, a 5-byte and a 200-byte (two-block) []byte
    "depth4": [("u", 8), ("s", [("u", 16), ("s", [("v", 8), ("s", [("b", 5), ("u", 8)]), ("u", 32)]), ("b", 200)]),
               U64],
    # nested messages of exactly 136 B (four hashes and a u64: pad in a block of its own) and of 137 B;
    # the top-level message is 2 * 32 + 9 * 8 = 136 B as well
    "rate136": [("s", [H32, H32, H32, H32, U64]), ("s", [H32, H32, H32, H32, U64, ("u", 8)])] + [U64] * 9,
    # a top-level message of 168 B (two blocks) over a 136-B nested one
    "rate168": [("s", [H32, H32, H32, H32, U64]), H32, H32, H32, H32, U64],
    # no nested struct: a flat layout with a variable-length field takes the same kernel
    "flat_var": [U64, ("v", 20), H32, ("u", 16)],
}


def _align4(x):
    return (x + 3) & ~3


def layout(t, off=0):
    """(mk_field entries in pre-order, end offset) of a type at record offset off."""
    ents = []
    for f in t:
        if f[0] == "u":
            ents.append((R, off, f[1] // 8))
            off += f[1] // 8
        elif f[0] == "b":
            off = _align4(off)
            ents.append((B, off, f[1]))
            off += f[1]
        elif f[0] == "v":
            off = _align4(off)
            ents.append((V, off, f[1]))
            off += 4 + f[1]
        else:
            sub, off = layout(f[1], off)
            ents.append((S, 0, len(sub)))
            ents += sub
    return ents, off


def ref_type(t, name="T"):
    """The oracle's type tuple (oracle/ssz_ref.py)."""
    fields = []
    for i, f in enumerate(t):
        if f[0] == "u":
            ft = ("uint", f[1])
        elif f[0] in ("b", "v"):
            ft = ("bytes",)
        else:
            ft = ("ptr", ref_type(f[1], f"{name}_{i}"))
        fields.append((f"F{i}", ft))
    return ("struct", name, fields)


def rand_value(t, rng, i, salt=0):
    """Record i's value as the oracle's dict; var field j of the record has length VAR_LENS[(i + 3 j + salt) % 8]."""
    nvar = [0]

    def go(t):
        d = {}
        for k, f in enumerate(t):
            if f[0] == "u":
                d[f"F{k}"] = int(rng.integers(0, 1 << min(f[1], 62)))
            elif f[0] == "b":
                d[f"F{k}"] = rng.integers(0, 256, f[1], dtype=np.uint8).tobytes()
            elif f[0] == "v":
                L = min(VAR_LENS[(i + 3 * nvar[0] + salt) % len(VAR_LENS)], f[1])
                nvar[0] += 1
                d[f"F{k}"] = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
            else:
                d[f"F{k}"] = go(f[1])
        return d

    return go(t)


def pack(t, val, rec, off=0):
    """The value into the record (uint8 row) as layout() lays it out; slack of a var slot is 0xEE."""
    for k, f in enumerate(t):
        v = val[f"F{k}"]
        if f[0] == "u":
            n = f[1] // 8
            rec[off:off + n] = np.frombuffer(int(v).to_bytes(n, "little"), np.uint8)
            off += n
        elif f[0] == "b":
            off = _align4(off)
            rec[off:off + f[1]] = np.frombuffer(v, np.uint8)
            off += f[1]
        elif f[0] == "v":
            off = _align4(off)
            rec[off:off + 4] = np.frombuffer(len(v).to_bytes(4, "little"), np.uint8)
            rec[off + 4:off + 4 + len(v)] = np.frombuffer(v, np.uint8)
            rec[off + 4 + len(v):off + 4 + f[1]] = 0xEE
            off += 4 + f[1]
        else:
            off = pack(f[1], v, rec, off)
    return off


class Case:
    """N_MAX records of one type: values, packed records, oracle struct roots (computed once, never changed)."""

    def __init__(self, name):
        from oracle import ssz_ref as OS

        self.t = TYPES[name]
        self.fields, end = layout(self.t)
        self.R = _align4(end)
        self.ref = ref_type(self.t)
        rng = np.random.default_rng(SEED + sum(map(ord, name)))
        self.vals = [rand_value(self.t, rng, i) for i in range(N_MAX)]
        self.rec = np.full((N_MAX, self.R), 0xDD, dtype=np.uint8)
        for i, v in enumerate(self.vals):
            pack(self.t, v, self.rec[i])
        self.roots = np.stack([np.frombuffer(OS.tree_hash(self.ref, v), np.uint8) for v in self.vals])
        self.rec.setflags(write=False)
        self.roots.setflags(write=False)

    def list_root(self, n):
        from oracle import ssz_ref as OS

        return OS.tree_hash(("slice", ("ptr", self.ref)), self.vals[:n])


_CASES = {}


def case(name) -> Case:
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def _dev_records(gpu, rec, shift, tail=64):
    """The records on the device at a base that is 16-B aligned (shift 0) or only 4-B aligned (shift 4), followed by
    a canary of `tail` bytes."""
    import torch

    flat = np.ascontiguousarray(rec).reshape(-1)
    buf = torch.full((16 + flat.size + tail,), 0xA5, dtype=torch.uint8, device=gpu)
    assert buf.data_ptr() % 16 == 0
    view = buf[shift:shift + flat.size]
    view.copy_(torch.from_numpy(flat.copy()).to(gpu))
    return buf, view


def test_layouts_cover_the_rate_boundary(gpu):
    L = _lib.load()
    from tests.test_struct_nested_host import _f

    want = {"attestation": 104 + 192, "eth1_vote": 40 + 64, "rate136": 136 + 136 + 137, "rate168": 168 + 136,
            "flat_var": 8 + 32 + 32 + 2}
    for name, tot in want.items():
        f = layout(TYPES[name])[0]
        assert L.mk_ssz_struct_msg_len(_f(f), len(f)) == tot, name
    assert len(layout(TYPES["attestation"])[0]) == 13


@pytest.mark.parametrize("shift", [0, 4], ids=["base16", "base4"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(TYPES))
def test_struct_roots(gpu, name, n, shift):
    import torch

    from prysm_amd import device as D

    c = case(name)
    buf, view = _dev_records(gpu, c.rec[:n], shift)
    out = torch.full((32 * n + 32,), 0x5A, dtype=torch.uint8, device=gpu)
    D.struct_roots(view, n, c.R, c.fields, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:32 * n].reshape(n, 32), c.roots[:n]), (name, n)
    assert (got[32 * n:] == 0x5A).all()
    assert (buf.cpu().numpy()[shift + n * c.R:] == 0xA5).all()


@pytest.mark.parametrize("name", ["attestation", "depth4", "flat_var"])
def test_host_struct_roots(gpu, name):
    from prysm_amd import state as ST

    c = case(name)
    got = ST.struct_roots_packed(c.rec[:65], c.fields)
    assert np.array_equal(got, c.roots[:65])


def test_device_clamps_a_stored_length(gpu):
    """A stored L above the capacity on a device entry point: hashed as the
    capacity, nothing read or written outside the buffers."""
    import torch

    from oracle import ssz_ref as OS
    from prysm_amd import device as D

    c = case("attestation")
    n, bad = 65, 64  # the last record of the buffer
    rec = c.rec[:n].copy()
    off = c.fields[10][1]  # the first bitfield slot
    assert c.fields[10] == (V, off, CAP) and c.fields[11] == (V, off + 4 + CAP, CAP)
    for slot in (off, off + 4 + CAP):
        rec[bad, slot:slot + 4] = np.frombuffer((CAP + 1000).to_bytes(4, "little"), np.uint8)
    val = dict(c.vals[bad])
    val["F1"] = rec[bad, off + 4:off + 4 + CAP].tobytes()
    val["F2"] = rec[bad, off + 8 + CAP:off + 8 + 2 * CAP].tobytes()
    want = c.roots[:n].copy()
    want[bad] = np.frombuffer(OS.tree_hash(c.ref, val), np.uint8)
    buf, view = _dev_records(gpu, rec, 4)
    out = torch.full((32 * n + 32,), 0x5A, dtype=torch.uint8, device=gpu)
    D.struct_roots(view, n, c.R, c.fields, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:32 * n].reshape(n, 32), want)
    assert (got[32 * n:] == 0x5A).all()
    assert (buf.cpu().numpy()[4 + n * c.R:] == 0xA5).all() and (buf.cpu().numpy()[:4] == 0xA5).all()
    # the host entry points refuse the same records
    from prysm_amd import state as ST

    for fn in (ST.struct_roots_packed, ST.struct_list_root_packed):
        with pytest.raises(_lib.MerkleError) as e:
            fn(rec, c.fields)
        assert e.value.code == _lib.MK_EINVAL


@pytest.mark.parametrize("n", [0, 1, 2, 65, 257])
@pytest.mark.parametrize("name", ["attestation", "eth1_vote", "depth4"])
def test_list_roots(gpu, name, n):
    import torch

    from prysm_amd import device as D
    from prysm_amd import state as ST

    c = case(name)
    want = c.list_root(n)
    assert ST.struct_list_root_packed(c.rec[:n], c.fields) == want
    _, view = _dev_records(gpu, c.rec[:max(n, 1)], 0)
    got = D.struct_list_root(view, n, c.R, c.fields)
    torch.cuda.synchronize()
    assert bytes(got.cpu().numpy()) == want


def test_struct_list_tree(gpu):
    """The registry tree over PendingAttestationRecords: assign, an update of a
    few records with one bitfield length changed, an append past the capacity,
    the root after each step; an oversized L is MK_EINVAL and changes nothing."""
    from oracle import ssz_ref as OS
    from prysm_amd.listtree import StructListTree

    c = case("attestation")
    slice_t = ("slice", ("ptr", c.ref))
    tree = StructListTree(c.R, c.fields, capacity=64)
    assert tree.root() == OS.tree_hash(slice_t, [])
    vals = list(c.vals[:50])
    tree.assign(c.rec[:50])
    assert len(tree) == 50 and tree.root() == OS.tree_hash(slice_t, vals)
    # records 3, 17, 49 change; 17 only in the length of its first bitfield (132 -> 3 bytes or 3 -> 132)
    rng = np.random.default_rng(SEED + 77)
    idx = [17, 3, 49]
    new = [dict(c.vals[17]), rand_value(c.t, rng, 200), rand_value(c.t, rng, 205)]
    old = new[0]["F1"]
    new[0]["F1"] = old[:3] if len(old) > 3 else rng.integers(0, 256, 132, dtype=np.uint8).tobytes()
    assert len(new[0]["F1"]) != len(old)
    rec = np.full((3, c.R), 0xDD, dtype=np.uint8)
    for j, v in enumerate(new):
        pack(c.t, v, rec[j])
        vals[idx[j]] = v
    tree.update(idx, rec)
    assert tree.root() == OS.tree_hash(slice_t, vals)
    # an oversized stored length: refused, tree unchanged
    bad = rec.copy()
    off = c.fields[11][1]
    bad[1, off:off + 4] = np.frombuffer((CAP + 1).to_bytes(4, "little"), np.uint8)
    for call in (lambda: tree.update(idx, bad), lambda: tree.append(bad), lambda: tree.assign(bad)):
        with pytest.raises(_lib.MerkleError) as e:
            call()
        assert e.value.code == _lib.MK_EINVAL
        assert len(tree) == 50 and tree.root() == OS.tree_hash(slice_t, vals)
    assert np.array_equal(tree.records(3, 1)[0], rec[1])
    # past the capacity of 64: doubles and rebuilds
    tree.append(c.rec[100:130])
    vals += c.vals[100:130]
    assert len(tree) == 80 and tree.root() == OS.tree_hash(slice_t, vals)
    # a short append climbs from the appended records only
    tree.append(c.rec[200:201])
    vals += c.vals[200:201]
    assert tree.root() == OS.tree_hash(slice_t, vals)
    # and a one-record update climbs from that record (81 / 32 > 1 dirty)
    tree.update([80], c.rec[201:202])
    vals[80] = c.vals[201]
    assert len(tree) == 81 and tree.root() == OS.tree_hash(slice_t, vals)


@pytest.mark.parametrize("k", [0, 1, 130])
def test_packers_vs_state_value(gpu, k):
    """pack_attestations / pack_eth1_votes / pack_crosslinks against
    BeaconState.as_value() through the oracle."""
    from oracle import ssz_ref as OS
    from prysm_amd import ssz as SZ
    from prysm_amd import state as ST
    from tests.ssz_types import to_ref_type

    st = ST.synthetic_state(8, SEED + k, n_attestations=k, n_batched=2, n_votes=k, lists_len=16, shards=max(k, 1))
    val = st.as_value()
    rec, fields = ST.pack_attestations(st.attestations)
    longest = max([len(x) for x in st.attestations.aggregation_bitfield + st.attestations.custody_bitfield] + [1])
    assert rec.shape == (k, ST.pending_attestation_record_len(_align4(longest))) and len(fields) == 13
    want = OS.tree_hash(to_ref_type(SZ.Slice(SZ.Ptr(ST.PENDING_ATTESTATION_SSZ))), val["LatestAttestations"])
    assert ST.struct_list_root_packed(rec, fields) == want
    votes = ST.pack_eth1_votes(st.eth1_votes, st.eth1_vote_counts)
    want = OS.tree_hash(to_ref_type(SZ.Slice(SZ.Ptr(ST.ETH1_VOTE_SSZ))), val["Eth1DataVotes"])
    assert ST.struct_list_root_packed(votes, ST.ETH1_VOTE_FIELDS) == want
    cross = ST.pack_crosslinks(st.crosslink_epochs, st.crosslink_roots)
    want = OS.tree_hash(to_ref_type(SZ.Slice(SZ.Ptr(ST.CROSSLINK_SSZ))), val["LatestCrosslinks"])
    assert ST.struct_list_root_packed(cross, ST.CROSSLINK_FIELDS) == want
    want = OS.tree_hash(to_ref_type(ST.ETH1_DATA_SSZ), val["LatestEth1Data"])
    assert bytes(ST.struct_roots_packed(st.eth1_data.reshape(1, 64), ST.ETH1_DATA_FIELDS)[0]) == want
