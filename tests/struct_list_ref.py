"""TEST INFRASTRUCTURE: the flat-record format with list fields
(MK_FIELD_LIST, include/prysm_merkle.h), restated with the oracle alone.

``record_roots(records, fields)`` is the struct root of every packed record by
the slot rules: it reads the records exactly as the header describes them and
hashes with ``oracle.keccak256`` / ``oracle.merkle_hash``.

``flatten(typ, caps)`` lays an oracle type tuple (oracle/ssz_ref.py) out as a
flat record: (fields, record_len, pack(value) -> bytes).  Slices take their
capacity from ``caps`` in declaration order, byte strings their slot size.
"""
import struct

import numpy as np

from oracle import oracle as O

BYTES, RAW, VARBYTES, STRUCT, LIST = 1, 2, 3, 4, 5


def _span(fields, f):
    kind, _, ln = fields[f]
    if kind == STRUCT:
        return 1 + ln
    if kind == LIST:
        return 1 + _span(fields, f + 1)
    return 1


def _le32(rec, off):
    return struct.unpack_from("<I", rec, off)[0]


def _struct_msg(rec, base, fields, f0, f1):
    """Concatenated field outputs of the struct whose children are entries
    [f0, f1); offsets count from ``base``."""
    out, f = [], f0
    while f < f1:
        kind, off, ln = fields[f]
        if kind == RAW:
            out.append(rec[base + off:base + off + ln])
        elif kind == BYTES:
            out.append(O.keccak256(struct.pack("<I", ln) + rec[base + off:base + off + ln]))
        elif kind == VARBYTES:
            L = _le32(rec, base + off)
            assert L <= ln, "stored length above the slot"
            out.append(O.keccak256(rec[base + off:base + off + 4 + L]))
        elif kind == STRUCT:
            out.append(O.keccak256(_struct_msg(rec, base, fields, f + 1, f + 1 + ln)))
        elif kind == LIST:
            ikind, stride, ilen = fields[f + 1]
            count = _le32(rec, base + off)
            assert count <= ln, "count above the capacity"
            elems = []
            for j in range(count):
                cell = base + off + 4 + j * stride
                if ikind == RAW:
                    elems.append(rec[cell:cell + ilen])
                elif ikind == BYTES:
                    elems.append(O.keccak256(struct.pack("<I", ilen) + rec[cell:cell + ilen]))
                else:
                    assert ikind == STRUCT
                    elems.append(O.keccak256(_struct_msg(rec, cell, fields, f + 2, f + 2 + ilen)))
            out.append(O.merkle_hash(elems))
        else:
            raise ValueError(kind)
        f += _span(fields, f)
    return b"".join(out)


def record_root(rec: bytes, fields) -> bytes:
    return O.keccak256(_struct_msg(bytes(rec), 0, fields, 0, len(fields)))


def record_roots(records: np.ndarray, fields) -> np.ndarray:
    records = np.ascontiguousarray(records, dtype=np.uint8)
    out = np.empty((records.shape[0], 32), dtype=np.uint8)
    for i in range(records.shape[0]):
        out[i] = np.frombuffer(record_root(records[i].tobytes(), fields), dtype=np.uint8)
    return out


def list_root(records: np.ndarray, fields) -> bytes:
    """TreeHash of the list of records: merkleHash over their roots."""
    return O.merkle_hash([bytes(r) for r in record_roots(records, fields)])


# ---- an oracle type as a flat record ---------------------------------------------------------
def _align4(x):
    return (x + 3) & ~3


def _lay(t, caps, off, in_item):
    """-> (entries, size, put(buf, base, value)); entry offsets count from the
    record (from the cell inside a list item), starting at ``off``."""
    k = t[0]
    if k == "ptr":
        return _lay(t[1], caps, off, in_item)
    if k in ("bool", "uint"):
        n = 1 if k == "bool" else t[1] // 8

        def put(buf, base, v, off=off, n=n):
            buf[base + off:base + off + n] = int(v).to_bytes(n, "little")
        return [(RAW, off, n)], off + n, put
    if k == "bytearray":
        off = _align4(off)

        def put(buf, base, v, off=off, n=t[1]):
            buf[base + off:base + off + n] = bytes(v)
        return [(BYTES, off, t[1])], (off + t[1]), put
    if k == "bytes":
        off, cap = _align4(off), caps.pop(0)

        def put(buf, base, v, off=off, cap=cap):
            assert len(v) <= cap
            buf[base + off:base + off + 4] = struct.pack("<I", len(v))
            buf[base + off + 4:base + off + 4 + len(v)] = bytes(v)
        return [(VARBYTES, off, cap)], off + 4 + cap, put
    if k == "struct":
        entries, puts, cur = [], [], off
        for name, ft in t[2]:
            if "XXX" in name:
                continue
            e, end, p = _lay(ft, caps, cur, in_item)
            entries += e
            puts.append((name, p))
            cur = end

        def put(buf, base, v, puts=puts):
            for name, p in puts:
                p(buf, base, v[name])
        return [(STRUCT, 0, len(entries))] + entries, cur, put
    if k in ("slice", "array"):
        assert not in_item
        off, cap = _align4(off), caps.pop(0)
        e, size, p = _lay(t[1], caps, 0, True)
        if e[0][0] == RAW:
            stride, desc = e[0][2], [(RAW, e[0][2], e[0][2])]
        elif e[0][0] == BYTES:
            stride, desc = _align4(size), [(BYTES, _align4(size), e[0][2])]
        else:
            assert e[0][0] == STRUCT
            stride = _align4(size)
            desc = [(STRUCT, stride, e[0][2])] + e[1:]

        def put(buf, base, v, off=off, cap=cap, stride=stride, p=p):
            assert len(v) <= cap
            buf[base + off:base + off + 4] = struct.pack("<I", len(v))
            for j, x in enumerate(v):
                p(buf, base + off + 4 + j * stride, x)
        return [(LIST, off, cap)] + desc, off + 4 + cap * stride, put
    raise ValueError(t)


def flatten(typ, caps):
    """(fields, record_len, pack) for a struct type; ``caps``: the capacities
    of its slices and []byte fields in declaration order (depth first)."""
    assert typ[0] in ("struct", "ptr")
    entries, size, put = _lay(typ, list(caps), 0, False)
    rec_len = _align4(size)

    def pack(v, fill=None):
        """``fill``: rec_len bytes the record starts from (the padding, the slots'
        unused tails and the cells beyond a count keep them); None: zeros."""
        buf = bytearray(rec_len) if fill is None else bytearray(fill)
        assert len(buf) == rec_len
        put(buf, 0, v)
        return bytes(buf)
    return entries[1:], rec_len, pack  # without the top-level struct's own entry
