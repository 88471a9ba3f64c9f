"""CPU self-test of tests/guarded_arena.py, and the part of the workspace
contract (tests/test_gpu_ws_contract.py) that needs no GPU: the shapes meant
for the wide generic leaf pass plan as that pass."""
import pytest
import torch

from tests.guarded_arena import FILL, GUARD, GuardedArena


def _arena():
    ar = GuardedArena("cpu", [("in", 1000, 256, 0), ("ws", 4096 + 32, 16, 8)], capacity=GUARD + 512)
    out = ar.region("out", 96, 64, 1)
    assert out.numel() == 96 and ar.view("ws").numel() == 4096 + 32
    return ar


def test_layout():
    ar = _arena()
    assert ar.ptr("in") % 256 == 0 and ar.ptr("ws") % 16 == 8 and ar.ptr("out") % 64 == 1
    spans = sorted((lo, hi) for _f, lo, hi, _b in ar._regions.values())
    assert spans[0][0] >= GUARD and ar.buf.numel() - spans[-1][1] >= GUARD
    for (_lo0, hi0), (lo1, _hi1) in zip(spans, spans[1:]):
        assert lo1 - hi0 >= GUARD
    assert bool((ar.buf == FILL).all())
    ar.check_guards()
    with pytest.raises(ValueError):
        ar.region("huge", 1 << 20)
    with pytest.raises(ValueError):
        ar.region("ws", 8)


def test_poison_and_views():
    ar = _arena()
    ar.poison("ws", 0x5A)
    assert bool((ar.view("ws") == 0x5A).all())
    ar.assert_poison("ws", 0x5A)
    ar.check_guards()  # poisoning a region never touches a guard
    ar.view("ws")[100] = 0
    ar.view("ws")[107] = 1
    with pytest.raises(AssertionError, match=r"region 'ws'.*offset 100, 8 bytes"):
        ar.assert_poison("ws", 0x5A)
    ar.assert_poison("ws", 0x5A, 108)
    ar.assert_poison("ws", 0x5A, 0, 100)


@pytest.mark.parametrize("name,side,dist", [("ws", "back", 0), ("ws", "back", GUARD - 1), ("ws", "front", 0),
                                            ("in", "front", GUARD - 1), ("out", "back", 31)])
def test_check_guards_reports_one_flipped_byte(name, side, dist):
    """One flipped guard byte is reported with its region, side and distance; a
    check_guards that checks nothing fails here."""
    ar = _arena()
    _f, lo, hi, _b = ar._regions[name]
    pos = hi + dist if side == "back" else lo - 1 - dist
    ar.buf[pos] ^= 0xFF
    with pytest.raises(AssertionError) as e:
        ar.check_guards("case X: ")
    msg = str(e.value)
    assert msg.startswith("case X: ") and f"{side} guard" in msg and f"first damaged byte {dist} bytes" in msg
    assert "damaged length 1 " in msg
    # a guard shared by two neighbours is reported for one of them; a far one never
    assert f"region {name!r}" in msg or (dist == GUARD - 1 and "region" in msg)
    ar.buf[pos] ^= 0xFF
    ar.check_guards()


def test_check_guards_reports_an_overrun_length():
    ar = _arena()
    _f, _lo, hi, _b = ar._regions["ws"]
    ar.buf[hi:hi + 32768] = 0  # a workgroup's 1024 nodes past the end of the workspace
    with pytest.raises(AssertionError, match=r"region 'ws', back guard, first damaged byte 0 bytes past the end.*"
                                             r"damaged length 32768 "):
        ar.check_guards()


def test_snapshot_reports_a_changed_input():
    ar = _arena()
    ar.view("in").copy_(torch.arange(1000, dtype=torch.int64).to(torch.uint8))
    ar.snapshot("in")
    ar.assert_unchanged("in")
    ar.view("in")[777] ^= 1
    with pytest.raises(AssertionError, match=r"region 'in' changed: first at offset 777, 1 bytes"):
        ar.assert_unchanged("in", "call Y: ")
    ar.view("in")[777] ^= 1
    ar.assert_unchanged("in")
    ar.check_guards()


def test_wide_generic_shapes_plan_as_the_generic_pass(tmp_path):
    """The host side of test_merkle_hash_wide_generic: every shape's pass 0 is
    k_reduce<true, false, NI> as a whole pass (no wave, no fast workgroups)."""
    from tests import test_gpu_ws_contract as C

    passes = C.build_plan_probe(tmp_path)
    for item_len, c1, shift in C.WIDE:
        C.wide_plan_ok(passes, item_len, c1, shift)
    # and the shapes that docstrings used to credit with that pass are k_wave3 leaf passes
    p0 = passes(70_001, 32, False)[0]
    assert p0["wave"] == 1 and p0["sp"] == 0 and p0["c1"] == 8751
