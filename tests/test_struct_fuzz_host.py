"""The struct-hashing fuzz's plan (tests/struct_fuzz_plan.py) without a device:
the parser's verdict on every planned layout against the header's rules as the
plan restates them, the flat reference (tests/struct_list_ref.py, what the
device is compared with) against the oracle's typed TreeHash on every planned
record, the model of every resident life, the coverage the committed seed
reaches, and two deliberately wrong variants of the reference that the planned
records must tell from the right one."""
import os
import struct

import numpy as np
import pytest

from oracle import oracle as O
from oracle import ssz_ref
from prysm_amd import _lib
from tests import struct_fuzz_plan as P
from tests import struct_list_ref as SL
from tests.struct_list_ref import BYTES, LIST, STRUCT
from tests.test_struct_list_field_host import _f

needs_default_seed = pytest.mark.skipif(P.FUZZ_SEED != 0, reason="coverage is asserted for the committed seed")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module")
def plan():
    return P.plan()


@pytest.fixture(scope="module")
def roots(plan):
    """The flat reference's root of every planned record, computed once."""
    return {lay.name: SL.record_roots(lay.records, lay.fields) for lay in plan.accepted}


# ---- the parser against the header ---------------------------------------------------------------------
def test_verdicts_and_scratch_sizes(lib, plan):
    for lay in plan.layouts:
        got = lib.mk_ssz_struct_msg_len(_f(lay.fields), len(lay.fields))
        assert (got > 0) == lay.accepted, (lay.describe(), lay.why, got)
        if lay.accepted:
            want = P.scratch_bytes(lay.fields) if any(k == STRUCT for k, _, _ in lay.fields) else \
                P.msg_len(lay.fields, 0, len(lay.fields))
            assert got == want, lay.describe()
    for kind, over in (("nested", 324), ("list", 644)):
        aimed = [lay for lay in plan.layouts if lay.aimed == over and lay.kind == kind]
        assert len(aimed) >= P.PEAK_LAYOUTS and all(lay.peak == over and not lay.accepted for lay in aimed), (kind, over)
    for kind, at in (("nested", 160), ("nested", 164), ("nested", 320), ("list", 320), ("list", 324), ("list", 640)):
        aimed = [lay for lay in plan.layouts if lay.aimed == at and lay.kind == kind]
        assert len(aimed) >= P.PEAK_LAYOUTS and all(lay.peak == at and lay.accepted for lay in aimed), (kind, at)


def test_few_random_layouts_are_dropped(plan):
    assert plan.drawn >= 100
    assert len(plan.dropped) <= 0.05 * plan.drawn, plan.dropped


def test_sizes_stay_small(plan):
    for lay in plan.layouts:
        assert lay.rec_len <= P.MAX_RECORD and lay.rec_len % 4 == 0, lay.describe()
        assert lay.n in [0] + P.RECORD_COUNTS and lay.n * lay.rec_len <= max(P.RECORDS_BYTES, lay.rec_len)
        if lay.life is not None:
            assert 4 <= len(lay.life.steps) <= 8 and lay.life.pool_n <= P.LIFE_CAP


# ---- the two references -----------------------------------------------------------------------------------
def test_flat_reference_matches_typed_hash(plan, roots):
    for lay in plan.accepted:
        for i, v in enumerate(lay.values):
            assert bytes(roots[lay.name][i]) == ssz_ref.tree_hash(lay.typ, v), lay.describe(i)
        want = ssz_ref.tree_hash(("slice", ("ptr", lay.typ)), lay.values)
        assert O.merkle_hash([bytes(r) for r in roots[lay.name]]) == want, lay.describe()
    lay = plan.accepted[0]
    assert SL.list_root(lay.records, lay.fields) == ssz_ref.tree_hash(("slice", ("ptr", lay.typ)), lay.values)


def test_records_carry_garbage_and_diverge(plan):
    """The bytes no field owns are random, not zero, and neighbouring records differ in their counts."""
    for lay in plan.accepted:
        clean = np.frombuffer(b"".join(lay.pack(v) for v in lay.values[:4]), np.uint8).reshape(-1, lay.rec_len)
        ones = np.frombuffer(b"".join(lay.pack(v, b"\xff" * lay.rec_len) for v in lay.values[:4]), np.uint8)
        spare = clean.reshape(-1) != ones  # bytes that pack() leaves alone
        if spare.sum() >= 16:
            assert (lay.records[:4].reshape(-1)[spare] != 0).any(), lay.describe()
        nlists = sum(k == LIST for k, _, _ in lay.fields)
        for j in range(nlists):
            if lay.n >= 64 and lay.fields[[f for f, e in enumerate(lay.fields) if e[0] == LIST][j]][2] >= 3:
                for a in range(0, lay.n - 63, 32):
                    assert len({c[0][j] for c in lay.counts[a:a + 64]}) >= 4, lay.describe(a)


def test_clamp_variants(plan, roots):
    seen = 0
    for lay in plan.accepted:
        if lay.clamp is None:
            continue
        bad, clamped = lay.clamp
        seen += 1
        assert (bad != clamped).any(axis=1).all()
        SL.record_roots(clamped, lay.fields)  # inside every slot
        for i in range(len(bad)):
            with pytest.raises(AssertionError, match="above the"):
                SL.record_root(bad[i].tobytes(), lay.fields)
    with_words = sum(bool(P.clamp_words(lay.fields)) for lay in plan.accepted)
    assert seen >= 1 and 0.05 * with_words <= seen <= 0.2 * with_words, (seen, with_words)


# ---- resident lives ---------------------------------------------------------------------------------------
def test_life_models(plan):
    assert len(plan.lives) >= 0.15 * sum(lay.kind != "flat" for lay in plan.accepted)
    for lay in plan.lives:
        life = lay.life
        pool_roots = SL.record_roots(life.pool, lay.fields)
        m = P.LifeModel(life, pool_roots)
        for step in life.steps:
            kind, arg, first, take = step
            assert first + take <= life.pool_n
            before = len(m)
            seen = m.apply(step)
            assert len(m.rec) == len(m.roots) <= P.LIFE_CAP, (lay.name, step)
            if kind in ("update", "clone_diverge", "erase", "branches"):
                assert len(arg) >= 1 and max(arg) < before, (lay.name, step)
            if kind == "erase":
                assert len(m) == before - len(set(arg))
            if kind == "append":
                assert len(m) == before + take and take >= 1
            if kind == "truncate":
                assert len(m) == arg <= before
            if kind == "clone_diverge":
                idx, na, nb = seen
                # a new record whose live bytes equal the old one's (an empty list for an empty list) is no difference
                same = [i for i in arg if m.roots[i].tobytes() == m.twin[1][i].tobytes()]
                assert na == nb == before and list(idx) == sorted(set(arg) - set(same)), (lay.name, step)
            if kind == "diff":
                idx, na, nb = seen
                k = min(na, nb)
                a, b = SL.record_roots(m.rec[:k], lay.fields), SL.record_roots(m.twin[0][:k], lay.fields)
                naive = [i for i in range(k) if a[i].tobytes() != b[i].tobytes()]
                assert list(idx) == naive, (lay.name, step)
            if kind == "branches":
                assert np.array_equal(seen, SL.record_roots(m.rec[arg], lay.fields))
        # the incremental model against the reference from scratch
        assert np.array_equal(m.roots, SL.record_roots(m.rec, lay.fields)), lay.name
        assert O.merkle_hash([bytes(r) for r in m.roots]) == SL.list_root(m.rec, lay.fields)


def test_tree_sets_are_legal(plan):
    assert len(plan.sets) >= 8
    for sp in plan.sets:
        assert 2 <= len(sp.trees) <= 4
        kinds = [x.kind for what, x, _, _ in sp.trees if what == "struct"]
        assert "nested" in kinds and "list" in kinds and any(what != "struct" for what, _, _, _ in sp.trees)
        offs = sorted(off for _, _, _, off in sp.trees)
        assert all(b - a >= 32 for a, b in zip(offs, offs[1:])) and offs[-1] + 32 <= sp.container_len
        assert all(o % 4 == 0 for o in offs)


# ---- coverage of the committed seed ---------------------------------------------------------------------
@needs_default_seed
def test_plan_coverage(plan):
    cov = plan.cov
    for form in P.FORMS:
        assert cov["form", form] >= 5, (form, cov["form", form])
    for kind, peak in (("nested", 160), ("nested", 320), ("list", 320), ("list", 640)):
        assert cov["peak", kind, peak] >= 1, (kind, peak)
    for what in ("nested depth 4", "list at depth 3, item struct at depth 4", "three lists", "list first", "list last"):
        assert cov[what] >= 1, what
    for n in (124, 128, 132, 136, "odd", ">=200"):
        assert cov["bytes", "list_top", n] >= 1, ("top-level bytes of", n)
    for where in ("item", "in_item"):
        for n in (128, 132, 136):
            assert cov["bytes", where, n] >= 1, (where, n)
    for where in ("nested", "list_top", "in_item"):
        for tag in P.VAR_LENGTHS:
            assert cov["var", where, tag] >= 1, (where, tag)
    for where in ("nested", "item"):  # 136 = 4 x 32 + 8 is reachable with the drawn field kinds
        for tag in ("<136", "136", ">136", ">272"):
            assert cov["msg", where, tag] >= 1, (where, tag)
    for ik in ("raw1", "raw2", "raw4", "raw8", "bytes", "struct"):
        for tag in P.COUNT_TAGS:
            assert cov["count", ik, tag] >= 1, (ik, tag)
    assert [P._odd_levels(c) for c in (4, 5, 6, 11)] == [0, 2, 1, 2]
    assert cov["odd2"] >= 1, "no list with an odd number of nodes at two levels"
    for lv in range(6):
        assert cov["levels", lv] >= 1, ("stack levels", lv)
    for kind in P.LIFE_STEPS:
        assert cov["step", kind] >= 10, (kind, cov["step", kind])
    assert cov["erase_all"] >= 1 and cov["append_from_empty"] >= 1
    assert cov["clamp", "var"] >= 1 and cov["clamp", "count"] >= 1


# ---- the plan would notice a wrong kernel -----------------------------------------------------------------
def py_merkle_hash(elems, drop_pad=False):
    """merkleHash restated (hash.go:194-239); drop_pad: the wrong variant that
    leaves the 128 zero bytes beside an odd node out."""
    n = len(elems)
    if n == 0:
        chunks = [bytes(128)]
    else:
        per = max(128 // len(elems[0]), 1)
        chunks = [b"".join(elems[i:i + per]) for i in range(0, n, per)]
    while len(chunks) > 1:
        if len(chunks) % 2:
            chunks.append(b"" if drop_pad else bytes(128))
        chunks = [O.keccak256(chunks[i] + chunks[i + 1]) for i in range(0, len(chunks), 2)]
    return O.keccak256(chunks[0] + n.to_bytes(8, "little") + bytes(24))


class _NoPad:
    keccak256 = staticmethod(O.keccak256)

    @staticmethod
    def merkle_hash(elems):
        return py_merkle_hash(elems, drop_pad=True)


class _NoPrefix132:
    """struct_list_ref packs a length prefix only for MK_FIELD_BYTES."""
    unpack_from = staticmethod(struct.unpack_from)

    @staticmethod
    def pack(fmt, *args):
        return b"" if args == (132,) else struct.pack(fmt, *args)


def test_restated_merkle_hash_is_the_oracles():
    for L, n in [(1, 0), (1, 300), (8, 17), (8, 81), (32, 4), (32, 5), (32, 21), (32, 43)]:
        elems = [bytes([i & 255]) * L for i in range(n)]
        assert py_merkle_hash(elems) == O.merkle_hash(elems), (L, n)


@pytest.mark.parametrize("what,attr,shim", [("no zero chunk beside an odd node", "O", _NoPad),
                                            ("132-byte field without its length prefix", "struct", _NoPrefix132)])
def test_plan_tells_a_wrong_reference(plan, roots, monkeypatch, what, attr, shim):
    def touched(lay):
        if attr == "struct":
            return any(k == BYTES and ln == 132 for k, _, ln in lay.fields)
        return any(k == LIST and P.list_chunks(lay.fields, f) >= 3 for f, (k, _, _) in enumerate(lay.fields))
    monkeypatch.setattr(SL, attr, shim)
    caught = 0
    for lay in plan.accepted:
        if touched(lay):
            caught += bool((SL.record_roots(lay.records, lay.fields) != roots[lay.name]).any())
    assert caught >= 10, (what, caught)
