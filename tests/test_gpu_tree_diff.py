"""Two resident trees diffed on the device: the device entry
mk_dev_ssz_trees_diff over the three kinds.

The kinds, their pools of rows and the buffers are those of
tests/test_gpu_tree_copy.py / test_gpu_tree_shrink.py: a tree is built by its
kind's build entry into buffers full of 0xA5, tree a at capacity n_a + 3 and
tree b at 2 n_b + 5, so no level of the two starts at the same node.  The
expected answer needs no tree: [i < m : leaf_a[i] != leaf_b[i]] in numpy over
the pools' level-0 rows (the items, the oracle's struct roots / element
digests).  Sixteen pairs go into one call.  With h = 10 a work item spans
H = 2^10 p values; the counts are the smallest at which the kernel takes
another path: nothing, one value, a chunk, one more, 37 chunks, and one work
item less one, exactly, plus one, and two items and a bit."""
import numpy as np
import pytest

from prysm_amd import _lib
from tests import tree_diff_ref as R
from tests.test_gpu_tree_copy import FILL, Bufs, kind_of
from tests.test_gpu_tree_shrink import POOL, Kind, _rand

pytestmark = pytest.mark.gpu

KINDS = ["list-1", "list-8", "list-32", "list-100", "struct-validator", "bytes-32"]
SLOT = -0x5A5A5A5A5A5A5A5B  # what an index slot holds before the call (as int64)
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def base_rows(n):
    return (37 * np.arange(n, dtype=np.int64) + 11) % POOL


_alt = {}


def other_rows(k):
    """For every pool row, one whose level-0 entry differs (one-byte items repeat within the pool)."""
    if k.name not in _alt:
        alt = np.empty(POOL, dtype=np.int64)
        for r in range(POOL):
            alt[r] = next(q % POOL for q in range(r + 1, r + POOL) if not np.array_equal(k.pool0[q % POOL], k.pool0[r]))
        _alt[k.name] = alt
    return _alt[k.name]


def changed_rows(k, n, idx):
    rows = base_rows(n)
    at = np.asarray(idx, dtype=np.int64)
    rows[at] = other_rows(k)[rows[at]]
    return rows


def span(k):
    return (1 << R.H) * k.per


def counts(k):
    p, H = k.per, span(k)
    return [0, 1, p, p + 1, 2 * p + 1, 37 * p, H - 1, H, H + 1, 2 * H + 3]


def change_sets(k, m, which):
    """name -> indices below m."""
    p, H = k.per, span(k)
    rng = np.random.default_rng(1000 * m + p)
    sets = {"none": []}
    if m:
        sets["first"] = [0]
        sets["last"] = [m - 1]
        sets["per-chunk"] = list(range(min(p, m) - 1, m, p)) if m <= 37 * p else [m // 2]
        sets["children"] = sorted({0, min(p, m - 1), min(2 * p, m - 1), min(3 * p, m - 1)})  # both children, twice
        sets["dense"] = list(range(min(H, m)))
        sets["random"] = sorted({int(x) for x in rng.integers(0, m, size=50)})
    return {name: sets[name] for name in which if name in sets}


ALL = ("none", "first", "last", "per-chunk", "children", "dense", "random")


def cases(k):
    """(n_a, n_b, changed indices): every count with n_a == n_b and every change set; n_a < n_b by one value and
    by more than a work item (m = n_a inside a chunk, at a chunk end, at a work-item end: the counts' own)."""
    H = span(k)
    out = []
    for n in counts(k):
        for name, idx in change_sets(k, n, ALL).items():
            out.append((n, n, idx, f"{n}=={n} {name}"))
        for name, idx in change_sets(k, n, ("none", "last", "random")).items():
            out.append((n, n + 1, idx, f"{n}<{n + 1} {name}"))
        for name, idx in change_sets(k, n, ("none", "first", "last", "dense")).items():
            out.append((n + H + 7, n, idx, f"{n + H + 7}>{n} {name}"))
    return out


class Pair:
    def __init__(self, gpu, k, a, n_a, n_b, idx, what, max_out=None):
        import torch

        self.k, self.a, self.n_a, self.n_b, self.what = k, a, n_a, n_b, what
        rows_b = changed_rows(k, n_b, idx)
        self.b = Bufs(gpu, k, 2 * n_b + 5, FILL).build(rows_b)
        m = min(n_a, n_b)
        ne = (k.pool0[base_rows(n_a)[:m]] != k.pool0[rows_b[:m]]).any(axis=1)
        self.want = [int(i) for i in np.flatnonzero(ne)]
        assert self.want == sorted(int(i) for i in idx if i < m), what
        self.max_out = len(self.want) + 3 if max_out is None else max_out
        self.out = torch.full((self.max_out,), SLOT, dtype=torch.int64, device=gpu) if self.max_out else None

    def args(self):
        from prysm_amd import device as D

        a, b, k = self.a, self.b, self.k
        return D.TreeDiffArgs(k.tree_kind, k.L, a.items, a.lv, self.n_a, a.cap, b.items, b.lv, self.n_b, b.cap,
                              idx_out=self.out, max_out=self.max_out, a_level0=a.level0, b_level0=b.level0)

    def check(self, report):
        total, first = report
        assert total == len(self.want), f"{self.k.name} {self.what}: total {total}, want {len(self.want)}"
        assert first == (self.want[0] if self.want else NONE), f"{self.k.name} {self.what}: first_index {first}"
        if self.out is None:
            return
        got = self.out.cpu().numpy()
        w = min(total, self.max_out)
        assert (got[w:] == SLOT).all(), f"{self.k.name} {self.what}: a slot beyond the written ones changed"
        wrote = sorted(int(x) for x in got[:w])
        if total <= self.max_out:
            assert wrote == self.want, f"{self.k.name} {self.what}"
        else:  # some max_out of them, each once
            assert len(set(wrote)) == w and set(wrote) <= set(self.want), f"{self.k.name} {self.what}"


def run(pairs):
    from prysm_amd import device as D

    for lo in range(0, len(pairs), _lib.MK_TREES_MAX):
        part = pairs[lo:lo + _lib.MK_TREES_MAX]
        reports = D.diff_reports(D.trees_diff([p.args() for p in part]))
        for p, r in zip(part, reports):
            p.check(r)


_a = {}


def tree_a(gpu, k, n):
    if (k.name, n) not in _a:
        _a[(k.name, n)] = Bufs(gpu, k, n + 3, FILL).build(base_rows(n))
    return _a[(k.name, n)]


@pytest.mark.parametrize("name", KINDS)
def test_counts_and_change_sets(gpu, name):
    import torch

    k = kind_of(name)
    pairs = [Pair(gpu, k, tree_a(gpu, k, na), na, nb, idx, what) for na, nb, idx, what in cases(k)]
    assert len(pairs) > 3 * _lib.MK_TREES_MAX
    bufs = {id(t): t for p in pairs[:32] for x in (p.a, p.b) for t in (x.items_all, x.level0, x.lv) if t is not None}
    before = {i: t.clone() for i, t in bufs.items()}
    run(pairs)
    # read-only on its inputs
    assert all(torch.equal(bufs[i], before[i]) for i in bufs)
    _a.clear()


@pytest.mark.parametrize("name", ["list-8", "struct-validator"])
def test_fewer_slots_than_differences(gpu, name):
    """max_out below total: total exact, the written indices a subset of the answer; max_out 0 with no buffer."""
    k = kind_of(name)
    H = span(k)
    n = 2 * H + 3
    a = tree_a(gpu, k, n)
    dense = list(range(H // 2, H + H // 2))  # across two work items
    pairs = [Pair(gpu, k, a, n, n, dense, "dense, 100 slots", max_out=100),
             Pair(gpu, k, a, n, n + 9, dense, "dense, one slot", max_out=1),
             Pair(gpu, k, a, n, n, dense, "dense, no buffer", max_out=0),
             Pair(gpu, k, a, n, n, [], "nothing, no buffer", max_out=0),
             Pair(gpu, k, a, n, n, [5, n - 1], "two of two", max_out=2),
             Pair(gpu, k, a, n, n, [5, 6 * k.per, n - 1], "two of three", max_out=2)]
    run(pairs)
    _a.clear()


def test_zero_pad_collision(gpu):
    """s = 32: a = x[0:k], b = x[0:k] and zero items up to the next chunk's end.  For k = 12 the level-1 node
    over chunk 2 is K(c2 || 0^128) in both trees; it is a straddler and is descended, not compared."""
    import torch

    from prysm_amd import device as D

    k = kind_of("list-32")
    x = torch.from_numpy(k.pool[base_rows(64)].reshape(-1).copy()).to(gpu)
    trees, wants = [], []
    outs = []
    for na, nb, flip in ((4, 8, None), (8, 16, None), (12, 16, None), (12, 16, 10), (20, 24, None), (20, 24, 19)):
        a = Bufs(gpu, k, na + 3, FILL)
        a.items[:na * 32] = x[:na * 32]
        D.list_tree_build(a.items, na, a.cap, 32, a.lv, a.root)
        b = Bufs(gpu, k, 2 * nb + 5, FILL)
        b.items[:nb * 32] = 0
        b.items[:na * 32] = x[:na * 32]
        if flip is not None:
            b.items[flip * 32 + 9] ^= 0x04
        D.list_tree_build(b.items, nb, b.cap, 32, b.lv, b.root)
        if (na, nb) == (12, 16) and flip is None:  # the collision is real: the two stored nodes are byte-equal
            na_off, nb_off = R.level_off(a.cap, 32, 1) + 1, R.level_off(b.cap, 32, 1) + 1
            assert torch.equal(a.lv[32 * na_off:32 * na_off + 32], b.lv[32 * nb_off:32 * nb_off + 32])
        out = torch.full((4,), SLOT, dtype=torch.int64, device=gpu)
        outs.append(out)
        trees.append(D.TreeDiffArgs(k.tree_kind, 32, a.items, a.lv, na, a.cap, b.items, b.lv, nb, b.cap, idx_out=out))
        wants.append([] if flip is None else [flip])
    got = D.diff_reports(D.trees_diff(trees))
    for r, w, out in zip(got, wants, outs):
        assert r == (len(w), w[0] if w else NONE)
        assert [int(v) for v in out.cpu().numpy()[:len(w)]] == w


def test_list_items_at_odd_byte_offsets(gpu):
    """Item lengths 1 and 100 with the two sides' values at byte offsets that agree mod 16 (the wide path with
    byte loads around it), that differ (byte loads), and 16-B aligned."""
    for name in ("list-1", "list-100"):
        k = kind_of(name)
        n = span(k) + 2 * k.per + 1
        idx = sorted({0, 1, k.per, n // 2, n - 2, n - 1})
        pairs = []
        for sa, sb in ((3, 19), (1, 2), (0, 7), (16, 0)):
            a = Bufs(gpu, k, n + 3, FILL, shift=sa).build(base_rows(n))
            p = Pair.__new__(Pair)
            import torch

            p.k, p.a, p.n_a, p.n_b, p.what = k, a, n, n, f"shifts {sa}, {sb}"
            p.b = Bufs(gpu, k, 2 * n + 5, FILL, shift=sb).build(changed_rows(k, n, idx))
            p.want, p.max_out = idx, len(idx) + 2
            p.out = torch.full((p.max_out,), SLOT, dtype=torch.int64, device=gpu)
            pairs.append(p)
        run(pairs)


VAR_FIELDS = [(_lib.MK_FIELD_BYTES, 0, 32), (_lib.MK_FIELD_VARBYTES, 32, 20), (_lib.MK_FIELD_RAW, 56, 8)]
VAR_LEN = 72  # bytes 64 .. 71 belong to no field; the VARBYTES slot is bytes 32 .. 55


def test_struct_fields_and_slack(gpu):
    """A record layout with a VARBYTES field: bytes of a slot beyond its length and bytes outside every field
    are no difference; a byte inside a field is."""
    import torch

    from prysm_amd import device as D

    n = 4 * 37 + 1
    rec = _rand(n * VAR_LEN, 777).reshape(n, VAR_LEN).copy()
    lens = (np.arange(n) * 7) % 21
    rec[:, 32:36] = lens.astype("<u4").view(np.uint8).reshape(n, 4)
    k = Kind.__new__(Kind)
    k.name, k.tree_kind, k.L, k.fields, k.len0, k.per = "struct-var", _lib.MK_TREE_STRUCT, VAR_LEN, VAR_FIELDS, 32, 4

    def build(records, cap):
        b = Bufs(gpu, k, cap, FILL)
        b.items[:n * VAR_LEN] = torch.from_numpy(records.reshape(-1).copy()).to(gpu)
        D.struct_list_tree_build(b.items, n, cap, VAR_LEN, VAR_FIELDS, b.level0, b.lv, b.root)
        return b

    a = build(rec, n + 3)
    slack = rec.copy()
    for i in range(n):
        slack[i, 36 + lens[i]:56] ^= 0xFF  # the slot beyond its length (nothing for a full one)
        slack[i, 64:72] ^= 0x3C            # outside every field
    field = slack.copy()
    field[3, 5] ^= 1                       # the BYTES field
    field[77, 60] ^= 1                     # the RAW field
    j = int(np.flatnonzero(lens > 2)[5])
    field[j, 36 + 1] ^= 1                  # inside the VARBYTES value
    want = sorted({3, 77, j})
    trees, outs = [], []
    for other in (slack, field):
        b = build(other, 2 * n + 5)
        out = torch.full((8,), SLOT, dtype=torch.int64, device=gpu)
        outs.append(out)
        trees.append(D.TreeDiffArgs(k.tree_kind, VAR_LEN, a.items, a.lv, n, a.cap, b.items, b.lv, n, b.cap, idx_out=out,
                                    a_level0=a.level0, b_level0=b.level0))
    got = D.diff_reports(D.trees_diff(trees))
    assert got[0] == (0, NONE) and bool((outs[0] == SLOT).all())
    assert got[1] == (3, want[0]) and sorted(int(v) for v in outs[1].cpu().numpy()[:3]) == want


@pytest.mark.parametrize("name", ["list-8", "bytes-32"])
def test_garbage_beyond_the_counts_after_a_shrink(gpu, name):
    """Both trees are built long, then built again shorter in the same buffers (what a shrink leaves to the
    right of the new end), and every node between a level's count and the next level is overwritten through a
    view of the level array: nothing beyond a count is read."""
    import torch

    k = kind_of(name)
    H = span(k)
    n_long, na, nb = 2 * H + 40 * k.per, H + 5 * k.per + 1, H + 9 * k.per
    idx = [0, k.per + 1, H - 1, H, na - 1]
    a = Bufs(gpu, k, n_long + 3, FILL).build(base_rows(n_long)).build(base_rows(na))
    p = Pair.__new__(Pair)
    p.k, p.a, p.n_a, p.n_b, p.what = k, a, na, nb, "after a shrink"
    p.b = Bufs(gpu, k, 2 * n_long + 5, FILL).build(changed_rows(k, n_long, [7, H + 2]))
    p.b.build(changed_rows(k, nb, idx))
    p.want, p.max_out = idx, 16
    p.out = torch.full((16,), SLOT, dtype=torch.int64, device=gpu)
    run([p])
    for t, n in ((p.a, na), (p.b, nb)):
        nodes = t.lv[:t.lv.numel() // 32 * 32].view(-1, 32)
        D_ = R.depth(n, k.len0)
        for d in range(1, R.depth(t.cap, k.len0) + 1):
            lo = R.level_off(t.cap, k.len0, d) + (R.level_count(n, k.len0, d) if d <= D_ else 0)
            nodes[lo:R.level_off(t.cap, k.len0, d + 1)] = 0x5A
        if t.level0 is not None:
            t.level0[32 * n:] = 0x5A
        t.items[n * k.L:] = 0x5A
    p.out.fill_(SLOT)
    run([p])


def test_same_buffers_on_both_sides_and_a_captured_call(gpu):
    import torch

    from prysm_amd import device as D

    k = kind_of("struct-validator")
    H = span(k)
    n = H + 9
    a = tree_a(gpu, k, n)
    idx = [1, H - 1, H + 8]
    p = Pair(gpu, k, a, n, n, idx, "captured")
    same = D.TreeDiffArgs(k.tree_kind, k.L, a.items, a.lv, n, a.cap, a.items, a.lv, n, a.cap, idx_out=None, max_out=0,
                          a_level0=a.level0, b_level0=a.level0)
    trees = [p.args(), same]
    reports = torch.zeros(32, dtype=torch.uint8, device=gpu)
    first = D.diff_reports(D.trees_diff(trees, reports=reports))
    assert first == [(3, 1), (0, NONE)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        D.trees_diff(trees, reports=reports)
    for rep in range(2):
        reports.fill_(0x33)
        p.out.fill_(SLOT)
        g.replay()
        torch.cuda.synchronize()
        assert D.diff_reports(reports) == first, f"replay {rep}"
        p.check(first[0])
    _a.clear()
