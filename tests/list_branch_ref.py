"""The list-tree proof rule of DESIGN.md §5l in plain Python: ``prove`` builds
the record of item i from the list's bytes and every level of its merkleHash
tree, ``verify`` folds a value through a record to the root.  K is
``oracle.keccak256``; nothing of the library is used, so the GPU tests can
compare records byte for byte and verdicts one by one with this file.

For n items of s bytes (1 <= s <= 128): p = 128 // s items per chunk, cb =
p * s, nchunks = ceil(n / p), total = n * s, D the smallest d with
ceil(nchunks / 2^d) == 1."""
from __future__ import annotations

from oracle import oracle as O

Z32 = bytes(32)
Z128 = bytes(128)


def shape(n: int, s: int):
    """(p, cb, nchunks, total, D)"""
    assert 1 <= s <= 128
    p = 128 // s
    cb = p * s
    nchunks = -(-n // p)
    D, c = 0, nchunks
    while c > 1:
        c = (c + 1) // 2
        D += 1
    return p, cb, nchunks, n * s, D


def stride(n: int, s: int) -> int:
    return 256 + 32 * max(shape(n, s)[4] - 1, 0)


def levels(data: bytes, n: int, s: int):
    """lv[d] for d = 1 .. D: the nodes of level d of the list's tree (lv[0] unused)."""
    p, cb, nchunks, total, D = shape(n, s)
    data = bytes(data[:total])
    lv = [None]
    if nchunks < 2:
        return lv
    cur = []
    for j in range((nchunks + 1) // 2):
        w = data[2 * j * cb:min(total, (2 * j + 2) * cb)]
        cur.append(O.keccak256(w + (Z128 if 2 * j + 1 == nchunks else b"")))
    lv.append(cur)
    while len(cur) > 1:
        nxt = []
        for q in range((len(cur) + 1) // 2):
            nxt.append(O.keccak256(cur[2 * q] + (cur[2 * q + 1] if 2 * q + 1 < len(cur) else Z128)))
        lv.append(nxt)
        cur = nxt
    assert len(lv) == D + 1
    return lv


def list_root(data: bytes, n: int, s: int) -> bytes:
    p, cb, nchunks, total, D = shape(n, s)
    lv = levels(data, n, s)
    if nchunks == 0:
        top = Z128  # merkleHash([]): the empty chunk
    elif nchunks == 1:
        top = bytes(data[:total])
    else:
        top = lv[D][0]
    return O.keccak256(top + n.to_bytes(8, "little") + bytes(24))


def prove(data: bytes, n: int, s: int, i: int, lv=None) -> bytes:
    """The record of item i; all zeros for i >= n."""
    p, cb, nchunks, total, D = shape(n, s)
    size = stride(n, s)
    if i >= n:
        return bytes(size)
    if lv is None:
        lv = levels(data, n, s)
    if nchunks >= 2:
        j = (i // p) // 2
        win = bytes(data[2 * j * cb:min(total, (2 * j + 2) * cb)])
    else:
        j = 0
        win = bytes(data[:total])
    rec = win + bytes(256 - len(win))
    for d in range(1, D):
        sib = (j >> (d - 1)) ^ 1
        rec += lv[d][sib] if sib < len(lv[d]) else Z32
    assert len(rec) == size
    return rec


def verify(value: bytes, i: int, n: int, s: int, record: bytes, root: bytes, container: bytes = None,
           container_off: int = None) -> bool:
    if i >= n:
        return False
    p, cb, nchunks, total, D = shape(n, s)
    j = (i // p) // 2 if nchunks >= 2 else 0
    pos = i * s - (2 * j * cb if nchunks >= 2 else 0)
    win = bytearray(record[:256])
    win[pos:pos + s] = value
    if nchunks <= 1:
        top = bytes(win[:total])
    else:
        wl = min(total, (2 * j + 2) * cb) - 2 * j * cb
        node = O.keccak256(bytes(win[:wl]) + (Z128 if 2 * j + 1 == nchunks else b""))
        for d in range(1, D):
            q = j >> (d - 1)
            cnt = -(-nchunks // (1 << d))
            sib = bytes(record[256 + 32 * (d - 1):256 + 32 * d])
            if q & 1:
                node = O.keccak256(sib + node)
            elif q + 1 < cnt:
                node = O.keccak256(node + sib)
            else:
                node = O.keccak256(node + Z128)
        top = node
    got = O.keccak256(top + n.to_bytes(8, "little") + bytes(24))
    if container is not None:
        msg = bytearray(container)
        msg[container_off:container_off + 32] = got
        got = O.keccak256(bytes(msg))
    return got == bytes(root)
