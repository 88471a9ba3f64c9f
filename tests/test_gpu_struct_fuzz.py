"""Seeded fuzz of struct hashing beyond the flat grammar on the GPU: nested
structs, []byte slots and list fields (k_struct_nested at 256 and 128 threads,
k_struct_list at 128 and 64) at layouts nobody wrote by hand, through the
device entry point, the host entry points, the resident StructListTree and
TreeSet.  The plan (layouts, records, lives, tree sets) is
tests/struct_fuzz_plan.py's and is checked without a device by
test_struct_fuzz_host.py, which also ties the reference used here,
tests/struct_list_ref.py on the packed records, to the oracle's typed TreeHash.
Nothing is compared with the library itself.

Measured on one MI355X at the default seed (wall time of the test function;
the reference roots of all planned records are a module fixture, 1.8 s with
the first use of the device):
  test_fuzz_struct_roots_nested_and_lists          165 accepted layouts (22 flat, 29 + 41 nested at 256 / 128
                                                   threads, 6 + 67 list at 128 / 64), 8736 records     0.28 s
  test_fuzz_struct_host_entry_points               a third of them and every clamp variant             0.07 s
  test_fuzz_struct_list_tree_lives                 33 lives, 215 steps                                 0.23 s
  test_fuzz_tree_set_with_nested_and_list_layouts  10 tree sets                                        0.11 s
PRYSM_FUZZ_SEED draws another plan, PRYSM_FUZZ_SCALE multiplies the random layouts."""
import random

import numpy as np
import pytest

from oracle import oracle as O
from prysm_amd import _lib
from prysm_amd import state as ST
from tests import struct_fuzz_plan as P
from tests import struct_list_ref as SL

pytestmark = pytest.mark.gpu

CANARY, GUARD = 0xA5, 0x5A


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def plan():
    return P.plan()


@pytest.fixture(scope="module")
def roots(plan):
    """The reference root of every planned record, computed once and left unchanged."""
    out = {lay.name: SL.record_roots(lay.records, lay.fields) for lay in plan.accepted}
    for r in out.values():
        r.setflags(write=False)
    return out


def merkle(leaves):
    return O.merkle_hash([bytes(x) for x in leaves])


def dev_roots(gpu, rec, fields, base_off):
    """Struct roots on the device entry point: the records between canaries at
    a base of ``base_off`` mod 16, 32 guard bytes behind the roots."""
    import torch

    from prysm_amd import device as D

    n, R = rec.shape
    flat = np.ascontiguousarray(rec).reshape(-1)
    lo = 16 + base_off
    host = np.full(lo + flat.size + 64, CANARY, np.uint8)
    host[lo:lo + flat.size] = flat
    buf = torch.from_numpy(host).to(gpu)
    view = buf[lo:lo + flat.size]
    assert view.data_ptr() % 16 == base_off
    out = torch.full((32 * n + 32,), GUARD, dtype=torch.uint8, device=gpu)
    D.struct_roots(view, n, R, fields, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[32 * n:] == GUARD).all(), "bytes behind the roots were written"
    assert np.array_equal(buf.cpu().numpy(), host), "the records or the bytes around them were written"
    return got[:32 * n].reshape(n, 32)


def test_fuzz_struct_roots_nested_and_lists(gpu, plan, roots):
    for lay in plan.accepted:
        assert lay.base_off in (0, 4)
        got = dev_roots(gpu, lay.records, lay.fields, lay.base_off)
        bad = [i for i in range(lay.n) if not np.array_equal(got[i], roots[lay.name][i])]
        assert not bad, (f"{len(bad)} of {lay.n} roots differ, first at records {bad[:8]}", lay.describe(bad[0]))
        if lay.clamp is not None:  # a stored length or count above its slot hashes as the capacity
            wrong, clamped = lay.clamp
            got = dev_roots(gpu, wrong, lay.fields, lay.base_off)
            assert np.array_equal(got, SL.record_roots(clamped, lay.fields)), ("clamp", lay.describe())
    assert {lay.base_off for lay in plan.accepted} == {0, 4}
    print(plan.line())


def test_fuzz_struct_host_entry_points(gpu, plan, roots):
    ran = 0
    for i, lay in enumerate(plan.accepted):
        if i % 3 and lay.clamp is None:
            continue
        ran += 1
        want = roots[lay.name]
        assert np.array_equal(ST.struct_roots_packed(lay.records, lay.fields), want), lay.describe()
        assert ST.struct_list_root_packed(lay.records, lay.fields) == merkle(want), lay.describe()
        assert ST.struct_list_root_packed(lay.records[:0], lay.fields) == O.merkle_hash([]), lay.describe()
        if lay.clamp is None:
            continue
        wrong = lay.clamp[0]
        mixed = np.concatenate([lay.records[:2], wrong[1:2], lay.records[:1]])
        for fn in (ST.struct_roots_packed, ST.struct_list_root_packed):
            for rec in (wrong, wrong[2:3], mixed):
                with pytest.raises(_lib.MerkleError) as e:
                    fn(rec, lay.fields)
                assert e.value.code == _lib.MK_EINVAL, lay.describe()
        assert np.array_equal(ST.struct_roots_packed(lay.records, lay.fields), want), lay.describe()
        assert ST.struct_list_root_packed(lay.records, lay.fields) == merkle(want), lay.describe()
    assert ran >= len(plan.accepted) // 3


MUTATING = ("update", "append", "erase", "truncate", "clone_diverge", "copy_from", "reserve")


def test_fuzz_struct_list_tree_lives(gpu, plan):
    from prysm_amd.listtree import StructListTree, verify_branches

    def check_diff(tree, twin, want, what):
        idx, na, nb = want
        d, total, ga, gb = tree.diff(twin)
        assert list(d) == list(idx) and total == len(idx) and (ga, gb) == (na, nb), what

    for lay in plan.lives:
        life = lay.life
        m = P.LifeModel(life, SL.record_roots(life.pool, lay.fields))
        tree = StructListTree(lay.rec_len, lay.fields, capacity=life.n0)
        if life.n0:
            tree.assign(life.pool[:life.n0])
        assert len(tree) == life.n0 and tree.root() == merkle(m.roots), lay.describe()
        twin = None
        for s, step in enumerate(life.steps):
            kind, arg, first, take = step
            what = (lay.describe(), f"step {s}", step[:2])
            new = life.pool[first:first + take]
            if kind in ("diff", "clone_diverge") and (twin is None or kind == "clone_diverge"):
                twin = tree.clone()
                assert twin.root() == tree.root() and len(twin) == len(tree), what
            seen = m.apply(step)
            if kind == "update":
                tree.update(arg, new)
            elif kind == "append":
                tree.append(new)
            elif kind == "erase":
                tree.erase(arg)
            elif kind == "truncate":
                tree.truncate(arg)
            elif kind == "clone_diverge":
                twin.update(arg, new)
                assert twin.root() == merkle(m.twin[1]) and twin.audit()[0] == 0, what
                check_diff(tree, twin, seen, what)
            elif kind == "copy_from":
                tree.copy_from(twin)
            elif kind == "reserve":
                tree.reserve(arg)
                assert tree.capacity >= arg, what
            elif kind == "audit":
                assert tree.audit()[0] == 0, what
            elif kind == "diff":
                check_diff(tree, twin, seen, what)
            elif kind == "branches":
                values, br = tree.branches(arg)
                assert np.array_equal(values, seen), what
                assert verify_branches(values, arg, len(m), 32, br, tree.root()).all(), what
            assert len(tree) == len(m) and tree.root() == merkle(m.roots), what
            if kind in MUTATING:
                assert tree.audit()[0] == 0, what
        assert np.array_equal(tree.records(), m.rec), lay.describe()


def _leaves(what, x, vals):
    if what == "struct":
        return SL.record_roots(vals, x.fields)
    if what == "list":
        return vals
    return np.array([np.frombuffer(O.keccak256(x.to_bytes(4, "little") + bytes(e)), np.uint8) for e in vals],
                    dtype=np.uint8).reshape(-1, 32)


def test_fuzz_tree_set_with_nested_and_list_layouts(gpu, plan):
    from prysm_amd.listtree import TreeSet

    kind_of = {"struct": _lib.MK_TREE_STRUCT, "list": _lib.MK_TREE_LIST, "bytes": _lib.MK_TREE_BYTES}
    for si, sp in enumerate(plan.sets):
        rng = random.Random(P.SEED + 7000 + si)
        nt = len(sp.trees)
        msg = bytearray(rng.randbytes(sp.container_len))
        s = TreeSet(container_len=sp.container_len)
        pools, leaves, cur = [], [], []
        edge = 0
        for t, (what, x, n0, off) in enumerate(sp.trees):
            L = x.rec_len if what == "struct" else x
            assert s.add(kind_of[what], L, fields=x.fields if what == "struct" else None, container_off=off) == t
            if off > edge:
                s.put(edge, msg[edge:off])
            edge = off + 32
            pools.append(P.set_pool(sp, t, 16 * si + t))
            leaves.append(_leaves(what, x, pools[t]))
            cur.append((pools[t][:n0].copy(), leaves[t][:n0].copy()))
            if n0:
                s.assign(t, pools[t][:n0])
        if sp.container_len > edge:
            s.put(edge, msg[edge:])

        def want(state):
            m = bytearray(msg)
            for (_, _, _, off), (_, lv) in zip(sp.trees, state):
                m[off:off + 32] = merkle(lv)
            return O.keccak256(bytes(m))

        def apply(handle, state, op):
            t, kind, arg, first, take = op
            vals, lv = state[t]
            nv, nl = pools[t][first:first + take], leaves[t][first:first + take]
            if kind == "update":
                handle.update(t, arg, nv)
                vals, lv = vals.copy(), lv.copy()
                vals[arg], lv[arg] = nv, nl
            elif kind == "append":
                handle.append(t, nv)
                vals, lv = np.concatenate([vals, nv]), np.concatenate([lv, nl])
            else:
                handle.erase(t, arg)
                vals, lv = np.delete(vals, arg, axis=0), np.delete(lv, arg, axis=0)
            state[t] = (vals, lv)

        what = f"tree set {si}: {[(w, x.name if w == 'struct' else x, n0, off) for w, x, n0, off in sp.trees]}"
        assert s.root() == want(cur), what
        for r, (ops, clone) in enumerate(sp.rounds):
            for op in ops:
                apply(s, cur, op)
            assert s.root() == want(cur), (what, r, ops)
            assert [s.count(t) for t in range(nt)] == [len(v) for v, _ in cur], (what, r)
            if clone is None:
                continue
            other, twin = list(cur), s.clone()
            apply(twin, other, clone)
            assert twin.root() == want(other) and s.root() == want(cur), (what, r, clone)
            d = s.diff(twin)
            for t in range(nt):
                idx = np.nonzero((cur[t][1] != other[t][1]).any(axis=1))[0]
                assert list(d[t][0]) == list(idx) and d[t][1] == len(idx), (what, r, clone, t)
            assert d["container"] == (0, None), (what, r)
        assert all(rep[0] == 0 for rep in s.audit()), what
