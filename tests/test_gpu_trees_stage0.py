"""Stage 0 batched across the trees of one mk_dev_ssz_trees_update
(k_trees_stage0) held to the per-tree one: every call below has
six trees with their values given -- list trees of 8-B (scatter unit 8) and 5-B
(unit 1) items, bytes trees of 32-B elements (staged at a 16-B aligned source:
the fast digest) and 33-B elements, struct trees of 40-B and 144-B records --
and is run on twin copies of the same built buffers; one goes through the
multi-tree call, the other through its kind's own single-tree update with the
same arguments.  Items, level 0, every level and the root must be equal byte
for byte, and the roots equal to the oracle's (Case / Twin / run_call are
test_gpu_trees_update.py's)."""
import numpy as np
import pytest

from prysm_amd import _lib
from prysm_amd import state as ST
from tests.test_gpu_trees_update import BYTES, LIST, STRUCT, Case, _rand, run_call

pytestmark = pytest.mark.gpu

# a 144-B record: epoch, four 32-B roots, a slot
REC144_FIELDS = [(_lib.MK_FIELD_RAW, 0, 8)] + [(_lib.MK_FIELD_BYTES, 8 + 32 * i, 32) for i in range(4)] + \
    [(_lib.MK_FIELD_RAW, 136, 8)]


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def _case(kind, L, n_old, cap, idx=(), n_app=0, salt=0, spec=None):
    from oracle import oracle as O

    m = n_old + len(idx) + n_app
    pool = _rand(max(m, 1) * L, 9000 + salt).reshape(-1, L)[:m]
    pool0 = None
    if kind == BYTES:
        pool0 = O.elem_digests(pool.reshape(-1), m, L) if m else np.zeros((0, 32), np.uint8)
    elif kind == STRUCT:
        pool0 = O.struct_roots(pool, m, L, spec) if m else np.zeros((0, 32), np.uint8)
    return Case(kind, L, pool, pool0, n_old, cap, idx, n_app, spec=spec)


# name -> six trees (L8, L5, B32, B33, S40, S144); shared, never changed
@pytest.fixture(scope="module")
def calls():
    X, R144 = ST.CROSSLINK_FIELDS, REC144_FIELDS
    wide_idx = list(range(3, 903, 3))  # 300 work items: the grid is larger than every other tree's segment
    return {
        # one tree with 300 work items, the others 1; a tree with nothing dirty (no values) in the middle
        "wide": [_case(LIST, 8, 1000, 1024, wide_idx, salt=1), _case(LIST, 5, 100, 128, [77], salt=2),
                 _case(BYTES, 32, 64, 64, salt=3), _case(BYTES, 33, 37, 64, [36], salt=4),
                 _case(STRUCT, 40, 50, 64, [49], salt=5, spec=X), _case(STRUCT, 144, 9, 16, [0], salt=6, spec=R144)],
        "wide bytes": [_case(LIST, 8, 9, 16, [8], salt=7), _case(BYTES, 32, 1000, 1024, wide_idx, salt=8),
                       _case(STRUCT, 144, 20, 32, salt=9, spec=R144), _case(LIST, 5, 26, 64, [25], salt=10),
                       _case(BYTES, 33, 6, 8, [5], salt=11), _case(STRUCT, 40, 6, 8, [0], salt=12, spec=X)],
        "wide struct": [_case(STRUCT, 40, 1000, 1024, wide_idx, salt=13, spec=X), _case(LIST, 8, 40, 64, [0], salt=14),
                        _case(LIST, 5, 30, 64, salt=15), _case(BYTES, 32, 9, 16, [8], salt=16),
                        _case(BYTES, 33, 9, 16, [1], salt=17), _case(STRUCT, 144, 300, 512, wide_idx[:100], salt=18,
                                                                     spec=R144)],
        # listed indices >= n_old: nothing may be written for them (items, level 0, levels)
        "ignored": [_case(LIST, 8, 100, 128, [100, 5000], salt=20), _case(LIST, 5, 30, 64, [7, 30, 63], salt=21),
                    _case(BYTES, 32, 10, 16, [10, 15], salt=22), _case(BYTES, 33, 3, 8, [1, 3, 7], salt=23),
                    _case(STRUCT, 40, 50, 64, [3, 50, 63], salt=24, spec=X),
                    _case(STRUCT, 144, 3, 8, [3], salt=25, spec=R144)],
        # appends across a chunk boundary (16 / 25 items, 4 digests or roots per chunk)
        "appends": [_case(LIST, 8, 15, 64, [14], 3, salt=30), _case(LIST, 5, 24, 64, [0], 3, salt=31),
                    _case(BYTES, 32, 7, 16, [6], 3, salt=32), _case(BYTES, 33, 8, 16, n_app=1, salt=33),
                    _case(STRUCT, 40, 3, 16, [2], 6, salt=34, spec=X), _case(STRUCT, 144, 12, 16, n_app=1, salt=35,
                                                                            spec=R144)],
        # lists of 0, 1, 4 and 5 records or digests: the one-chunk rule and the first list with levels
        "0 1 4 5": [_case(LIST, 8, 0, 8, n_app=1, salt=40), _case(LIST, 5, 1, 8, [0], salt=41),
                    _case(BYTES, 32, 4, 8, [3], salt=42), _case(BYTES, 33, 5, 8, [4], salt=43),
                    _case(STRUCT, 40, 1, 8, [0], salt=44, spec=X), _case(STRUCT, 144, 5, 8, [0, 4], salt=45,
                                                                        spec=R144)],
        "to 1 4 5": [_case(BYTES, 32, 0, 8, n_app=1, salt=50), _case(BYTES, 33, 0, 8, n_app=4, salt=51),
                     _case(STRUCT, 40, 0, 8, n_app=5, salt=52, spec=X), _case(STRUCT, 144, 4, 8, [1], 1, salt=53,
                                                                         spec=R144),
                     _case(LIST, 8, 0, 8, salt=54), _case(LIST, 5, 4, 8, [3], 1, salt=55)],
        "from 4 and 5": [_case(STRUCT, 144, 0, 4, n_app=1, salt=60, spec=R144), _case(STRUCT, 40, 4, 4, [0, 3], salt=61,
                                                                                    spec=X),
                         _case(BYTES, 33, 1, 4, [0], 3, salt=62), _case(BYTES, 32, 5, 8, [0], salt=63),
                         _case(LIST, 5, 0, 1, salt=64), _case(LIST, 8, 5, 5, [4], salt=65)],
    }


NAMES = ["wide", "wide bytes", "wide struct", "ignored", "appends", "0 1 4 5", "to 1 4 5", "from 4 and 5"]


def test_every_shape_in_every_call(calls):
    assert list(calls) == NAMES
    for name, cs in calls.items():
        assert sorted((c.kind, c.L) for c in cs) == sorted([(LIST, 8), (LIST, 5), (BYTES, 32), (BYTES, 33),
                                                            (STRUCT, 40), (STRUCT, 144)]), name


@pytest.mark.parametrize("name", NAMES)
def test_batched_stage0_equals_single_tree(gpu, calls, name):
    twins = run_call(gpu, calls[name], name)
    for t in twins:  # the staged 32-B elements sit at a 16-B aligned source: the fast digest path
        if t.c.kind == BYTES and t.c.L == 32 and t.d_vals is not None:
            assert t.d_vals.data_ptr() % 16 == 0


def test_with_the_container(gpu, calls):
    """The six roots in a 232-B message, hashed in the same launch."""
    import torch

    from oracle import oracle as O
    from prysm_amd import device as D
    from tests.test_gpu_trees_update import Twin, check_twins

    cs = calls["appends"]
    offs = [0, 40, 72, 104, 136, 200]
    msg = _rand(232, 70)
    a, b = [Twin(gpu, c) for c in cs], [Twin(gpu, c) for c in cs]
    container = torch.from_numpy(msg.copy()).to(gpu)
    croot = torch.zeros(32, dtype=torch.uint8, device=gpu)
    D.trees_update([t.args(o) for t, o in zip(a, offs)], container, 232, croot)
    for t in b:
        t.single()
    torch.cuda.synchronize()
    want = msg.copy()
    for i, (x, y, o) in enumerate(zip(a, b, offs)):
        check_twins(x, y, f"tree {i}")
        want[o:o + 32] = np.frombuffer(cs[i].want_root, np.uint8)
    assert np.array_equal(container.cpu().numpy(), want)
    assert bytes(croot.cpu().numpy()) == O.keccak256(bytes(want))


def test_the_library_has_the_kernel():
    with open(_lib.LIB_PATH, "rb") as f:
        assert b"k_trees_stage0" in f.read()
