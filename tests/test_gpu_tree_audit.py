"""Resident trees audited on the device: the device entry
mk_dev_ssz_trees_audit and audit() of ListTree, StructListTree and
BytesListTree.

The kinds, their pools of rows and the buffers are those of
tests/test_gpu_tree_copy.py / test_gpu_tree_shrink.py, plus a struct with bytes
that belong to no field.  What a report must hold comes from the numpy model of
the rule (tests/tree_audit_ref.py) over host copies of the SAME buffers, with
level 0 of a struct / bytes tree from the oracle's struct hash / element
digests: the number of mismatches and the smallest (level, index) among them,
compared exactly."""
import numpy as np
import pytest

from prysm_amd import _lib
from tests import tree_audit_ref as A
from tests.test_gpu_tree_copy import FILL, Bufs, desc, kind_of
from tests.test_gpu_tree_shrink import POOL, Kind, _rand, rows

pytestmark = pytest.mark.gpu

CLEAN = (0, A.NONE, A.NO_INDEX)
GAP_FIELDS = [(_lib.MK_FIELD_BYTES, 0, 32), (_lib.MK_FIELD_RAW, 40, 8)]  # bytes 32..39 and 48..63: no field's
_gap = []


def gap_kind():
    """A 64-byte record of which 24 bytes belong to no field."""
    if not _gap:
        from oracle import oracle as O
        from prysm_amd.listtree import StructListTree

        pool = _rand(POOL * 64, 4242)
        _gap.append(Kind("struct-gap", _lib.MK_TREE_STRUCT, 64, lambda cap: StructListTree(64, GAP_FIELDS, capacity=cap),
                         "records", pool, O.struct_roots(pool, POOL, 64, GAP_FIELDS), fields=GAP_FIELDS))
    return _gap[0]


def kind(name):
    return gap_kind() if name == "struct-gap" else kind_of(name)


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def args(b, n, container_off=None):
    from prysm_amd import device as D

    return D.TreeAuditArgs(b.k.tree_kind, b.items, n, b.cap, b.k.L, b.lv, b.root, level0=b.level0, spec=b.k.fields,
                           container_off=container_off)


def audit(trees, **kw):
    from prysm_amd import device as D

    return D.audit_reports(D.trees_audit(trees, **kw))


def fresh_level0(k, records, n):
    """Level 0 as the oracle hashes it from the records as they are now (None for a list tree)."""
    from oracle import oracle as O

    if k.tree_kind == _lib.MK_TREE_LIST:
        return None
    rec = np.ascontiguousarray(records[:n * k.L])
    if k.tree_kind == _lib.MK_TREE_BYTES:
        return O.elem_digests(rec, n, k.L)
    return O.struct_roots(rec, n, k.L, k.fields)


def model(b, n, shift=0):
    """The report the rule gives on the buffers as the device holds them."""
    items, l0, lv, root = b.host()
    items = items[shift:]
    k = b.k
    bad = A.tree_mismatches(items if l0 is None else l0, lv, root, n, b.cap, k.len0)
    if l0 is not None and n:
        bad |= A.level0_mismatches(l0, fresh_level0(k, items, n), n)
    return A.report(bad)


CLEAN_KINDS = ["list-1", "list-8", "list-32", "list-48", "list-100", "list-128", "struct-validator",
               "struct-attestation", "struct-gap", "bytes-32", "bytes-48"]


def counts(k):
    p = k.per
    return [0, 1, p, p + 1, 2 * p, 2 * p + 1, 37 * p, 64 * p + 1]


@pytest.mark.parametrize("name", CLEAN_KINDS)
def test_clean(gpu, name):
    """Every shape built into buffers full of 0xA5, the sixteen trees of a kind in ONE call: nothing to report."""
    k = kind(name)
    built = []
    for n in counts(k):
        for cap in (n, 2 * n + 3):
            built.append((Bufs(gpu, k, cap, FILL).build(rows(n, 1)), n))
    assert len(built) == _lib.MK_TREES_MAX
    got = audit([args(b, n) for b, n in built])
    assert got == [CLEAN] * 17, [(b.cap, n, r) for (b, n), r in zip(built, got) if r != CLEAN]
    if name != "struct-attestation":  # (its nested layout is beyond the C oracle's struct hash)
        for b, n in built[-2:]:  # and the model agrees on the largest
            assert model(b, n) == CLEAN
    assert audit([args(*built[-1])]) == [CLEAN] * 2  # one tree alone


def flip(t, at, mask=0x01):
    t[at] ^= mask


LOCAL = ["list-8", "list-100", "struct-validator", "struct-gap", "bytes-32"]


@pytest.mark.parametrize("name", LOCAL)
def test_exact_localisation(gpu, name):
    """A 37-chunk tree (D = 6): one byte of every stored node in turn, the root, the values, bytes beyond."""
    import torch

    k = kind(name)
    n = 37 * k.per
    cap = 2 * n + 3
    b = Bufs(gpu, k, cap, FILL).build(rows(n, 2))
    lay = A.level_layout(n, cap, k.len0)
    assert [c for _, c in lay] == [19, 10, 5, 3, 2, 1]
    a = [args(b, n)]
    assert audit(a) == [CLEAN, CLEAN]
    pristine = [t.clone() if t is not None else None for t in (b.items_all, b.level0, b.lv, b.root)]

    def check(what, want_keys=None):
        got = audit(a)[0]
        want = model(b, n)
        assert got == want, f"{name} {what}: {got} != {want}"
        if want_keys is not None:
            assert want == A.report(want_keys), f"{name} {what}: the model gives {want}"
        for t, p in zip((b.items_all, b.level0, b.lv, b.root), pristine):  # read-only, then back to the built tree
            if t is not None:
                t.copy_(p)

    D = len(lay)
    for d, (off, c) in enumerate(lay, 1):
        for j in range(c):
            flip(b.lv, 32 * (off + j) + (5 * j + d) % 32, 0x40)
            check(f"node ({d}, {j})", {(d, j), (A.ROOT, 0) if d == D else (d + 1, j >> 1)})
        nxt = lay[d][0] if d < D else b.lv.numel() // 32
        assert off + c < nxt  # the capacity leaves room behind every level
        flip(b.lv, 32 * (off + c) + 9, 0xFF)
        check(f"a node beyond level {d}'s count", set())
    flip(b.root, 17)
    check("the root", {(A.ROOT, 0)})
    if k.tree_kind == _lib.MK_TREE_LIST:
        i = 3 * k.per  # the first item of chunk 3: window 1
        flip(b.items, i * k.L + k.L // 2)
        check("an item", {(1, 1)})
        flip(b.items, n * k.L)
        check("the first byte beyond the list", set())
    else:
        i = 21
        flip(b.items, i * k.L + 5)  # inside the first field
        check("a record byte inside a hashed field", {(0, i)})
        flip(b.level0, 32 * i + 31)
        check("a level-0 entry", {(0, i), (1, i // 8)})
        flip(b.level0, 32 * n + 1)
        flip(b.items, n * k.L + 3)
        check("level 0 and the values beyond the list", set())
        if name == "struct-gap":
            flip(b.items, i * k.L + 35)
            flip(b.items, (n - 1) * k.L + 63)
            check("record bytes outside every field", set())
    # fifty random flips anywhere in the live nodes, level 0 and the values
    rng = np.random.default_rng(11)
    live = [(b.lv, 32 * off, 32 * c) for off, c in lay] + [(b.items, 0, n * k.L)]
    if b.level0 is not None:
        live.append((b.level0, 0, 32 * n))
    for _ in range(50):
        t, lo, size = live[int(rng.integers(len(live)))]
        flip(t, lo + int(rng.integers(size)), 1 << int(rng.integers(8)))
    got, want = audit(a)[0], model(b, n)
    assert got == want and got[0] >= 10, f"{name} fifty flips: {got} != {want}"
    torch.cuda.synchronize()


def test_unaligned_and_short_windows(gpu):
    """Item buffers at odd byte offsets and item lengths whose windows are no 256 bytes: the byte path."""
    for name, n, shift in (("list-8", 593, 8), ("list-32", 149, 4), ("list-1", 4099, 1), ("list-48", 75, 16),
                           ("list-100", 37, 2), ("list-128", 38, 3)):
        k = kind(name)
        b = Bufs(gpu, k, n + 5, FILL, shift=shift).build(rows(n, 3))
        assert audit([args(b, n)]) == [CLEAN, CLEAN], name
        flip(b.items, (n - 1) * k.L)
        last = A.level_layout(n, n + 5, k.len0)[0][1] - 1
        got = audit([args(b, n)])[0]
        assert got == model(b, n, shift) == (1, 1, last), (name, got)


def test_container(gpu):
    """Three trees and the message that holds two of their roots: a message byte, a root's 32 bytes in it, the
    container root, each reported in the extra report only."""
    import torch

    from oracle import oracle as O

    shapes = [("list-8", 593, 0), ("struct-validator", 149, None), ("bytes-32", 33, 40)]
    built = [(Bufs(gpu, kind(nm), n + 3, FILL).build(rows(n, j)), n, off) for j, (nm, n, off) in enumerate(shapes)]
    torch.cuda.synchronize()
    msg = bytearray(_rand(80, 9).tobytes())
    for b, n, off in built:
        if off is not None:
            msg[off:off + 32] = bytes(b.root.cpu().numpy())
    d_msg = torch.tensor(list(msg) + [FILL] * 16, dtype=torch.uint8, device=gpu)
    d_croot = torch.tensor(list(O.keccak256(bytes(msg))), dtype=torch.uint8, device=gpu)
    trees = [args(b, n, off) for b, n, off in built]
    kw = dict(container=d_msg, container_len=80, container_root=d_croot)

    def want():
        m, cr = d_msg.cpu().numpy()[:80], d_croot.cpu().numpy()
        return A.report(A.container_mismatches(m, cr, [(b.root.cpu().numpy(), off) for b, n, off in built]))

    assert audit(trees, **kw) == [CLEAN] * 4
    flip(d_msg, 35)  # between the two roots
    assert audit(trees, **kw) == [CLEAN] * 3 + [(1, A.CONTAINER, 0)] == [CLEAN] * 3 + [want()]
    flip(d_msg, 35)
    flip(d_msg, 41)  # inside tree 2's root
    assert audit(trees, **kw) == [CLEAN] * 3 + [(2, A.CONTAINER, 0)] == [CLEAN] * 3 + [want()]
    flip(d_msg, 41)
    flip(d_msg, 80)  # beyond the message
    assert audit(trees, **kw) == [CLEAN] * 4
    flip(d_croot, 0)
    assert audit(trees, **kw) == [CLEAN] * 3 + [(1, A.CONTAINER, 0)]
    flip(d_croot, 0)
    flip(built[0][0].root, 3)  # a tree's root: the tree's own report, and its place in the message
    got = audit(trees, **kw)
    assert got == [(1, A.ROOT, 0), CLEAN, CLEAN, (1, A.CONTAINER, 1)] and got[3] == want()
    flip(built[0][0].root, 3)
    assert audit(trees, **kw) == [CLEAN] * 4


def test_after_every_device_mutation(gpu):
    """Update, append, truncate, erase and a copy into another capacity: what each leaves behind is sound,
    and what a shrink leaves to the right of the new end is not looked at."""
    import torch

    from prysm_amd import device as D

    for name in ("list-8", "list-48", "struct-validator", "struct-attestation", "bytes-32"):
        k = kind(name)
        n0 = 1025
        b = Bufs(gpu, k, 2 * n0 + 3, FILL).build(rows(n0))
        b.update(n0, n0, [0, 7, 1024], k.pool[[3, 4, 5]])
        assert audit([args(b, n0)])[0] == CLEAN, f"{name}: update"
        b.update(n0, n0 + 9, [5], k.pool[[6] + list(range(10, 19))])
        n = n0 + 9
        assert audit([args(b, n)])[0] == CLEAN, f"{name}: append"
        D.tree_erase(k.tree_kind, b.items, n, 600, b.cap, k.L, b.lv, b.root, level0=b.level0, spec=k.fields)
        n = 600
        assert audit([args(b, n)])[0] == CLEAN, f"{name}: truncate"
        rm = torch.tensor([1, 2, 77, 300, 598], dtype=torch.int64, device=gpu)
        D.tree_erase(k.tree_kind, b.items, n, n - 5, b.cap, k.L, b.lv, b.root, level0=b.level0, spec=k.fields, rm=rm,
                     k_rm=5, first=1)
        n -= 5
        assert audit([args(b, n)])[0] == CLEAN, f"{name}: erase"
        dst = Bufs(gpu, k, n + 1, FILL)
        D.trees_copy([desc(b, dst, n)])
        assert audit([args(dst, n), args(b, n)]) == [CLEAN] * 3, f"{name}: copy"
        # the audit of the longer list the buffers no longer hold must fail: it is n that is audited
        assert audit([args(b, n + 5)])[0][0] > 0, f"{name}: the stale tail"


def test_read_only_and_capture(gpu):
    """Every input byte is what it was, and one captured call replayed gives the same reports."""
    import torch

    from prysm_amd import device as D

    built = [(Bufs(gpu, kind(nm), n + 7, FILL).build(rows(n, 4)), n) for nm, n in
             (("list-100", 259), ("struct-validator", 70001 // 64), ("bytes-48", 77))]
    flip(built[1][0].lv, 32 * 3 + 1)
    flip(built[2][0].level0, 32 * 5)
    msg = torch.full((64,), 7, dtype=torch.uint8, device=gpu)
    croot = torch.full((32,), 9, dtype=torch.uint8, device=gpu)
    trees = [args(b, n, off) for (b, n), off in zip(built, (0, None, 32))]
    before = [[t.clone() for t in (b.items_all, b.level0, b.lv, b.root) if t is not None] for b, _ in built]
    kw = dict(container=msg, container_len=64, container_root=croot)
    ws = torch.empty(max(D.trees_audit_workspace_bytes(trees), 16), dtype=torch.uint8, device=gpu)
    reports = torch.zeros(24 * 4, dtype=torch.uint8, device=gpu)
    first = D.audit_reports(D.trees_audit(trees, reports=reports, ws=ws, **kw))
    assert first[0] == CLEAN and first[1] == (2, 1, 3) and first[2] == (2, 0, 5)
    assert first[3] == (3, A.CONTAINER, 0)  # the made-up message holds no root and is not what croot hashes
    for (b, _), keep in zip(built, before):
        now = [t for t in (b.items_all, b.level0, b.lv, b.root) if t is not None]
        assert all(torch.equal(x, y) for x, y in zip(now, keep))
    assert bool((msg == 7).all()) and bool((croot == 9).all())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.trees_audit(trees, reports=reports, ws=ws, **kw)
    for rep in range(2):
        reports.fill_(0x33)
        g.replay()
        torch.cuda.synchronize()
        assert D.audit_reports(reports) == first, f"replay {rep}"


def test_level0_in_pieces(gpu):
    """More values than one piece of the workspace holds (2^18): a flip in the second piece is found."""
    from prysm_amd import device as D

    k = kind("bytes-32")
    piece = 1 << 18
    n = piece + 300
    b = Bufs(gpu, k, n, FILL).build((np.arange(n) * 37 % POOL).tolist())
    assert D.trees_audit_workspace_bytes([args(b, n)]) == D.trees_audit_workspace_bytes([args(b, piece)])
    assert audit([args(b, n)]) == [CLEAN, CLEAN]
    flip(b.items, (piece + 17) * 32 + 4)
    flip(b.items, (piece + 299) * 32)
    assert audit([args(b, n)])[0] == (2, 0, piece + 17)


def test_refused_calls_write_nothing(gpu):
    import torch

    from prysm_amd import device as D

    k = kind("bytes-32")
    b = Bufs(gpu, k, 300, FILL).build(rows(257))
    reports = torch.full((48,), FILL, dtype=torch.uint8, device=gpu)
    small = args(b, 257)
    small.capacity = 256
    for what, a, kw in (("n above the capacity", small, {}),
                        ("a short workspace", args(b, 257), {"ws": torch.empty(64, dtype=torch.uint8, device=gpu)}),
                        ("a container offset without a container", args(b, 257, 0), {})):
        with pytest.raises(_lib.MerkleError) as e:
            D.trees_audit([a], reports=reports, **kw)
        assert e.value.code in (_lib.MK_EINVAL, _lib.MK_ENOMEM), what
        torch.cuda.synchronize()
        assert bool((reports == FILL).all()), what


# ---- the handles ---------------------------------------------------------------------------------
HANDLE_KINDS = ["list-8", "list-100", "struct-validator", "struct-attestation", "bytes-32", "bytes-48"]


@pytest.mark.parametrize("name", HANDLE_KINDS)
def test_handle_sequence(gpu, name):
    """assign / update / append / erase / truncate / clone / reserve: after each, the handle's tree is sound."""
    k = kind(name)
    t = k.make(0)
    assert t.audit() == CLEAN  # the empty tree
    steps = [("assign", lambda: t.assign(k.pool[rows(1025)])),
             ("update", lambda: t.update([0, 1024, 77], k.pool[[1, 2, 3]])),
             ("append past the capacity", lambda: t.append(k.pool[rows(700, 3)])),
             ("a large update (a rebuild)", lambda: t.update(list(range(0, 1700, 3)), k.pool[rows(567, 5)])),
             ("erase", lambda: t.erase([0, 5, 6, 1000, 1724])),
             ("truncate", lambda: t.truncate(601)),
             ("append again", lambda: t.append(k.pool[rows(9, 7)])),
             ("reserve", lambda: t.reserve(5000)),
             ("update in the new layout", lambda: t.update([609], k.pool[[9]])),
             ("truncate to one chunk", lambda: t.truncate(k.per)),
             ("truncate to nothing", lambda: t.truncate(0))]
    for what, step in steps:
        step()
        assert t.audit() == CLEAN, f"{name}: {what}"
        if what == "reserve":
            c = t.clone()
            assert c.audit() == CLEAN and c.root() == t.root(), f"{name}: the clone"
            c.append(k.pool[rows(3, 8)])
            assert c.audit() == CLEAN and t.audit() == CLEAN
    root = t.root()
    assert t.audit() == CLEAN and t.root() == root
