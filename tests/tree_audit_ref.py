"""The rule of a resident tree's audit (include/prysm_merkle.h)
in plain numpy over host copies of a tree's buffers: which stored nodes are not
the hash of what is stored below them.  Every count comes from n; the capacity
only places the levels; nothing at or beyond a level's count and no level-0
byte at or beyond n * len0 is looked at.  Returns the full set of mismatch keys
(level, index); `report` turns a set into what a mk_audit_report holds."""
import numpy as np

ROOT, CONTAINER, NONE = 64, 65, 0xFFFFFFFF
NO_INDEX = (1 << 64) - 1


def per(len0):
    return 128 // len0 if len0 < 128 else 1


def chunks(n, len0):
    return -(-n // per(len0))


def level_layout(n, capacity, len0):
    """[(first node in the level array, live nodes)] of levels 1 .. D."""
    c, cc, off, out = chunks(n, len0), chunks(capacity, len0), 0, []
    while c > 1:
        c, cc = (c + 1) // 2, (cc + 1) // 2
        out.append((off, c))
        off += cc
    return out


def _k(msgs):
    from oracle import oracle as O

    return O.keccak256_var([bytes(m) for m in msgs])


def tree_mismatches(level0, levels, root, n, capacity, len0):
    """Levels 1 .. D and the root of one tree: {(level, index)}.  level0: the
    level-0 bytes (the items of a list tree, the 32-B roots / digests of the
    other kinds), levels: the level array laid out for `capacity` values, root:
    32 bytes."""
    level0 = np.asarray(level0, dtype=np.uint8).reshape(-1)
    levels = np.asarray(levels, dtype=np.uint8).reshape(-1)
    total, cb, nch = n * len0, per(len0) * len0, chunks(n, len0)
    lay = level_layout(n, capacity, len0)
    bad = set()

    def stored(d):  # the live nodes of level d
        off, c = lay[d - 1]
        return levels[32 * off:32 * (off + c)].reshape(c, 32)

    if lay:
        c1 = lay[0][1]
        msgs = []
        for j in range(c1):
            m = bytes(level0[2 * j * cb:min(total, (2 * j + 2) * cb)])
            msgs.append(m + (bytes(128) if 2 * j + 1 == nch else b""))
        want = _k(msgs)
        bad |= {(1, int(j)) for j in np.flatnonzero((want != stored(1)).any(axis=1))}
        for d in range(2, len(lay) + 1):
            below = stored(d - 1)
            cnt = lay[d - 1][1]
            msgs = [bytes(below[2 * j]) + (bytes(below[2 * j + 1]) if 2 * j + 1 < len(below) else bytes(128))
                    for j in range(cnt)]
            bad |= {(d, int(j)) for j in np.flatnonzero((_k(msgs) != stored(d)).any(axis=1))}
        top = bytes(stored(len(lay))[0])
    else:
        top = bytes(level0[:total]) if n else bytes(128)
    want = _k([top + int(n).to_bytes(8, "little") + bytes(24)])[0]
    if bytes(want) != bytes(np.asarray(root, dtype=np.uint8).reshape(-1)[:32]):
        bad.add((ROOT, 0))
    return bad


def level0_mismatches(level0, want0, n):
    """Level 0 of a struct / bytes tree: the stored 32-B entries against the
    n freshly hashed ones (want0, from the oracle): {(0, i)}."""
    a = np.asarray(level0, dtype=np.uint8).reshape(-1)[:32 * n].reshape(n, 32)
    b = np.asarray(want0, dtype=np.uint8).reshape(-1)[:32 * n].reshape(n, 32)
    return {(0, int(i)) for i in np.flatnonzero((a != b).any(axis=1))}


def container_mismatches(message, container_root, roots_and_offsets):
    """The container checks: index 0 the hash of the message, 1 + i tree i's 32
    bytes of it (roots_and_offsets[i] = (root, offset or None))."""
    message = bytes(message)
    bad = set()
    if bytes(_k([message])[0]) != bytes(container_root)[:32]:
        bad.add((CONTAINER, 0))
    for i, (root, off) in enumerate(roots_and_offsets):
        if off is not None and message[off:off + 32] != bytes(root)[:32]:
            bad.add((CONTAINER, 1 + i))
    return bad


def report(bad):
    """(bad, first_level, first_index) of a mismatch set."""
    if not bad:
        return 0, NONE, NO_INDEX
    lvl, idx = min(bad)
    return len(bad), lvl, idx
