"""Host half of the resident-tree fuzz (test_gpu_tree_fuzz.py): the lives of
a tree (shape, capacity, placement), the steps of each life and the coverage
they reach, drawn from seeded streams without a device.  test_tree_fuzz_host.py
checks this plan on the CPU; the GPU test runs exactly the same plan.

A life is one tree: built with n0 items, then 6 to 12 steps.  A step is what
one mk_dev_ssz_*_tree_update call gets: a strictly ascending index list (an
entry >= n_old is the contract's ignored index, never a disordered one) and
n_new.  The values are drawn when the step runs.

Sizes are the smallest at which the climb can still go wrong: 0 to 2100
chunks, at most 300 KB of items per tree, and most lives below 40 chunks,
where a pad, a ragged chunk and the top meet in the same few nodes."""
import os
import random
from collections import Counter

import numpy as np

from prysm_amd import _lib
from tests.test_gpu_fuzz import _item_len, _layout

# PRYSM_FUZZ_SEED shifts every stream, PRYSM_FUZZ_SCALE multiplies the number
# of lives (as in test_gpu_fuzz.py).  The coverage conditions are asserted for
# the committed run, PRYSM_FUZZ_SEED unset or 0.
FUZZ_SEED = int(os.environ.get("PRYSM_FUZZ_SEED", "0"))
SEED = 0x5EED000000000000 + 4100 + 1000 * FUZZ_SEED
SCALE = max(1, int(os.environ.get("PRYSM_FUZZ_SCALE", "1")))

LIST, STRUCT, BYTES = _lib.MK_TREE_LIST, _lib.MK_TREE_STRUCT, _lib.MK_TREE_BYTES
KIND_NAME = {LIST: "list", STRUCT: "struct", BYTES: "bytes"}

MAX_CHUNKS = 2100
MAX_BYTES = 300 * 1024
SMALL_CHUNKS = 39  # "stays below 40 chunks"

ITEM_LENS = [1, 2, 3, 4, 7, 8, 16, 31, 32, 33, 48, 64, 96, 100, 128, 129, 200, 255, 280, 300]  # _item_len's list
ELEM_LENS = [1, 3, 4, 31, 32, 33, 48, 131, 132, 133, 200]
LIST_OFFS, LIST_VAL_OFFS = [0, 8, 4, 1, 3], [0, 1]
BYTES_OFFS, BYTES_VAL_OFFS = [0, 4, 16, 1], [0, 1]
STRUCT_OFFS, STRUCT_VAL_OFFS = [0, 4, 8, 12], [0, 4]  # records and new records are 4-B aligned
VALIDATOR_LEN = 160

# default number of lives per test: test_gpu_tree_fuzz.py's docstring has the measured times
LIVES = {"list": 360, "bytes": 180, "struct": 180, "calls": 42}

# ---- steps ----------------------------------------------------------------------------------------
STEP_WEIGHTS = [
    ("scattered", 10),          # a few scattered indices
    ("dense_run", 6),           # a dense run that starts in an odd chunk
    ("level1_pair", 6),         # both children of one level-1 node
    ("first_last", 5),          # the first and the last item together
    ("every", 3),               # every item
    ("nothing", 5),             # nothing: the root must be written again
    ("append_in_chunk", 6),     # an append that stays inside the last chunk
    ("append_chunk", 6),        # ... across a chunk boundary
    ("append_pair", 6),         # ... across a pair boundary (a new level-1 node)
    ("append_taller", 8),       # ... across a power of two of chunks (a new top level)
    ("append_from_0", 10),      # ... to an empty list
    ("append_1_to_2", 10),      # ... from one chunk to two
    ("update_append", 6),       # updates and an append in one call
    ("ignored_behind", 5),      # indices >= n_old behind valid ones
    ("ignored_alone", 4),       # only indices >= n_old
    ("ignored_empty", 8),       # indices with n_old == 0, no append
    ("ignored_empty_append", 8),  # indices with n_old == 0 and an append
    ("ignored_append", 5),      # valid and ignored indices and an append
]
STEP_KINDS = [k for k, _ in STEP_WEIGHTS]


def per_of(kind, L):
    """Items per 128-B chunk of the tree's level 0 (struct roots and digests are 32-B items)."""
    if kind != LIST:
        return 4
    return 128 // L if L < 128 else 1


def chunks_of(n, per):
    return -(-n // per)


def max_chunks(kind, L):
    return min(MAX_CHUNKS, MAX_BYTES // (per_of(kind, L) * L))


def _pow2_at_least(x):
    p = 1
    while p < x:
        p <<= 1
    return p


class Step:
    def __init__(self, kind, idx, n_old, n_new, with_values, val_off):
        self.kind, self.n_old, self.n_new = kind, n_old, n_new
        self.idx = np.asarray(idx, dtype=np.int64)
        self.with_values, self.val_off = with_values, val_off

    @property
    def k(self):
        return len(self.idx)

    @property
    def work(self):  # values the step carries: one per index, then the appended items
        return self.k + self.n_new - self.n_old


def feasible(kind, n, cap, per):
    nch = chunks_of(n, per)
    room = cap > n
    return {
        "scattered": n >= 1,
        "dense_run": nch >= 2,
        "level1_pair": nch >= 2,
        "first_last": n >= 2,
        "every": n >= 1,
        "nothing": True,
        "append_in_chunk": n >= 1 and n % per != 0 and room,
        "append_chunk": n >= 1 and cap >= nch * per + 1,
        "append_pair": n >= 1 and cap >= (nch + (nch & 1)) * per + 1,
        "append_taller": nch >= 2 and cap >= _pow2_at_least(nch) * per + 1,
        "append_from_0": n == 0 and cap >= 1,
        "append_1_to_2": nch == 1 and cap >= per + 1,
        "update_append": n >= 1 and room,
        "ignored_behind": n >= 1,
        "ignored_alone": n >= 1,
        "ignored_empty": n == 0,
        "ignored_empty_append": n == 0 and cap >= 1,
        "ignored_append": n >= 1 and room,
    }[kind]


def _scattered(rng, n, kmax=12):
    return sorted(rng.sample(range(n), rng.randint(1, min(n, kmax))))


def _ignored(rng, n, cap, per):
    """1 to 3 ascending indices >= n: just behind the list, inside the capacity, far outside."""
    first = n + rng.choice([0, 0, 1, rng.randint(0, 2 * per), max(cap - 1 - n, 0), cap - n + 5, 1 << 40])
    out = [first]
    for _ in range(rng.randint(0, 2)):
        out.append(out[-1] + rng.choice([1, 1, per, 1 << 33]))
    return out


def draw_step(rng, n, cap, per, val_offs, force=None):
    """One step of a tree that holds n items with room for cap."""
    nch = chunks_of(n, per)
    if force is not None and feasible(force, n, cap, per):
        kind = force
    else:
        pool = [(k, w) for k, w in STEP_WEIGHTS if feasible(k, n, cap, per)]
        kind = rng.choices([k for k, _ in pool], [w for _, w in pool])[0]
    idx, n_new = [], n
    if kind == "scattered":
        idx = _scattered(rng, n)
    elif kind == "dense_run":
        c = 2 * rng.randrange(nch // 2) + 1  # an odd chunk
        idx = list(range(c * per, min(c * per + rng.randint(2, max(6 * per, 40)), n)))
    elif kind == "level1_pair":
        j = rng.randrange(nch // 2)  # chunks 2 j and 2 j + 1 both exist
        idx = [2 * j * per + rng.randrange(per), min((2 * j + 1) * per + rng.randrange(per), n - 1)]
    elif kind == "first_last":
        idx = [0, n - 1]
    elif kind == "every":
        idx = range(n)
    elif kind == "append_in_chunk":
        n_new = rng.randint(n + 1, min(cap, nch * per))
    elif kind == "append_chunk":
        n_new = rng.randint(nch * per + 1, min(cap, (nch + 3) * per))
    elif kind == "append_pair":
        e = nch + (nch & 1)
        n_new = rng.randint(e * per + 1, min(cap, (e + 2) * per))
    elif kind == "append_taller":
        p2 = _pow2_at_least(nch)
        n_new = rng.randint(p2 * per + 1, min(cap, (p2 + 2) * per))
    elif kind == "append_from_0":
        n_new = rng.randint(1, min(cap, 6 * per))
    elif kind == "append_1_to_2":
        n_new = rng.randint(per + 1, min(cap, 2 * per))
    elif kind == "update_append":
        idx = _scattered(rng, n)
        n_new = n + rng.randint(1, min(cap - n, 3 * per))
    elif kind == "ignored_behind":
        idx = _scattered(rng, n, 6) + _ignored(rng, n, cap, per)
    elif kind == "ignored_alone":
        idx = _ignored(rng, n, cap, per)
    elif kind == "ignored_empty":
        idx = _ignored(rng, 0, cap, per)
    elif kind == "ignored_empty_append":
        idx = _ignored(rng, 0, cap, per)
        n_new = rng.randint(1, min(cap, 6 * per))
    elif kind == "ignored_append":
        idx = _scattered(rng, n, 6) + _ignored(rng, n, cap, per)
        n_new = n + rng.randint(1, min(cap - n, 3 * per))
    return Step(kind, idx, n, n_new, rng.random() < 0.5, rng.choice(val_offs))


def apply_step(rows, step, vals):
    """The model: rows is the (cap, L) host copy of the list, vals the step's (work, L) values."""
    k = step.k
    valid = step.idx < step.n_old
    rows[step.idx[valid]] = vals[:k][valid]
    rows[step.n_old:step.n_new] = vals[k:]


# ---- lives ----------------------------------------------------------------------------------------
LIFE_SHAPES = [("empty", 12), ("one_chunk", 12), ("small", 25), ("pow2", 13), ("k1024", 13), ("large", 25)]
CALL_SHAPES = [("empty", 10), ("one_chunk", 12), ("small", 40), ("pow2", 18), ("k1024", 5), ("large", 15)]


class Life:
    def __init__(self, kind, L, spec, off, val_offs, shape, n0, cap):
        self.kind, self.L, self.spec, self.off, self.val_offs = kind, L, spec, off, val_offs
        self.shape, self.n0, self.cap, self.per = shape, n0, cap, per_of(kind, L)
        self.small = chunks_of(cap, self.per) <= SMALL_CHUNKS
        self.steps = []

    def name(self):
        return f"{KIND_NAME[self.kind]} L={self.L} off={self.off} {self.shape} n0={self.n0} cap={self.cap}"


def draw_life(rng, kind, L, spec, off, val_offs, shapes, exact, nsteps=None):
    per, top = per_of(kind, L), max_chunks(kind, L)
    shape = rng.choices([s for s, _ in shapes], [w for _, w in shapes])[0]
    if shape == "k1024" and top < 1030:
        shape = "large"
    if shape == "empty":
        nch = 0
    elif shape == "one_chunk":
        nch = 1
    elif shape == "small":
        nch = rng.randint(2, SMALL_CHUNKS)
    elif shape == "pow2":  # at or one below a power of two of chunks
        nch = (1 << rng.randint(1, 5)) - rng.choice([0, 0, 1])
    elif shape == "k1024":
        nch = rng.choice([1023, 1024, 1024, 1025])
    else:
        nch = rng.randint(SMALL_CHUNKS + 1, top)
    n = nch * per - (rng.randrange(per) if nch else 0)
    limit = top if shape in ("k1024", "large") else SMALL_CHUNKS
    # exact (every fourth life): capacity == n; the k1024 lives always have room to cross 1024 chunks
    if exact and shape != "k1024":
        cap = n
    else:  # up to twice the chunks (8 more for a list shorter than that)
        cap_ch = min(nch + rng.randint(1, max(nch, 8)), limit)
        if shape == "k1024":
            cap_ch = max(cap_ch, 1030)
        cap = max(n, cap_ch * per - rng.randrange(per))
    life = Life(kind, L, spec, off, val_offs, shape, n, cap)
    cur = n
    for s in range(rng.randint(6, 12) if nsteps is None else nsteps):
        force = None
        if s == 0:  # what only a life's first step can reach (an empty list, a single chunk) is not left to luck
            if shape == "k1024" and nch <= 1024:
                force = "append_taller"
            elif shape == "empty":
                force = rng.choice(["ignored_empty_append", "append_from_0", "ignored_empty", None])
            elif shape == "one_chunk":
                force = rng.choice(["append_1_to_2", None])
        st = draw_step(rng, cur, cap, per, val_offs, force)
        life.steps.append(st)
        cur = st.n_new
    return life


def _struct_layout(rng):
    fields, rl = _layout(rng)
    return [tuple(f) for f in fields], rl


def plan_list(nlives=None):
    rng = random.Random(SEED + 1)
    return [draw_life(rng, LIST, _item_len(rng), None, rng.choice(LIST_OFFS), LIST_VAL_OFFS, LIFE_SHAPES, i % 4 == 3)
            for i in range((nlives or LIVES["list"]) * SCALE)]


def plan_bytes(nlives=None):
    rng = random.Random(SEED + 2)
    return [draw_life(rng, BYTES, rng.choice(ELEM_LENS), None, rng.choice(BYTES_OFFS), BYTES_VAL_OFFS, LIFE_SHAPES,
                      i % 4 == 3)
            for i in range((nlives or LIVES["bytes"]) * SCALE)]


def plan_struct(nlives=None):
    rng = random.Random(SEED + 3)
    out = []
    for i in range((nlives or LIVES["struct"]) * SCALE):
        fields, rl = _struct_layout(rng)
        out.append(draw_life(rng, STRUCT, rl, fields, rng.choice(STRUCT_OFFS), STRUCT_VAL_OFFS, LIFE_SHAPES,
                             i % 4 == 3))
    return out


class Call:
    """One mk_dev_ssz_trees_update: the container's length, its base and root
    placement and each tree's root offset in it (None: no field of it)."""

    def __init__(self, length, base_off, root_off, offs):
        self.length, self.base_off, self.root_off, self.offs = length, base_off, root_off, offs


def draw_call(rng, ntrees):
    length = rng.choice([rng.randint(32, 4096), rng.randint(32, 4096), rng.randint(32, 300), 135, 136, 4095, 4096])
    take = [i for i in range(ntrees) if rng.random() < 0.75] or [rng.randrange(ntrees)]
    take = sorted(rng.sample(take, min(len(take), length // 32)))
    # disjoint 4-B aligned root ranges: the slack, in words, spread over the gaps
    slack = (length - 32 * len(take)) // 4
    cuts = sorted(rng.randint(0, slack) for _ in take)
    offs = [None] * ntrees
    for j, i in enumerate(take):
        offs[i] = 4 * cuts[j] + 32 * j
    order = [offs[i] for i in take]
    rng.shuffle(order)  # the trees need not lie in the container in their order in the call
    for j, i in enumerate(take):
        offs[i] = order[j]
    return Call(length, rng.choice([0, 4, 8, 12]), rng.choice([0, 4]), offs)


class CallLife:
    """1 to 16 trees of mixed kinds that live together: every step is one call over all of them."""

    def __init__(self, lives, calls):
        self.lives, self.calls = lives, calls


def plan_calls(nlives=None):
    rng = random.Random(SEED + 4)
    out = []
    for g in range((nlives or LIVES["calls"]) * SCALE):
        ntrees, nsteps = rng.randint(1, 16), rng.randint(6, 12)
        if g < 2:  # the two ends of 1 .. MK_TREES_MAX, whatever the seed
            ntrees = (16, 1)[g]
        lives = []
        for i in range(ntrees):
            kind = rng.choice([LIST, STRUCT, BYTES])
            if kind == LIST:
                args = (_item_len(rng), None, rng.choice(LIST_OFFS), LIST_VAL_OFFS)
            elif kind == BYTES:
                args = (rng.choice(ELEM_LENS), None, rng.choice(BYTES_OFFS), BYTES_VAL_OFFS)
            else:
                fields, rl = _struct_layout(rng)
                args = (rl, fields, rng.choice(STRUCT_OFFS), STRUCT_VAL_OFFS)
            lives.append(draw_life(rng, kind, *args, CALL_SHAPES, (g + i) % 4 == 3, nsteps))
        out.append(CallLife(lives, [draw_call(rng, ntrees) for _ in range(nsteps)]))
    return out


# ---- coverage -------------------------------------------------------------------------------------
def scatter_case(life, step):
    """The row of the issue's table a LIST step reaches, or None (k_list_tree_scatter does not run)."""
    if life.kind != LIST or not step.with_values or step.work == 0:
        return None
    if life.L % 8:
        return "length not a multiple of 8: unit 1"
    if life.off % 8 == 0 and step.val_off % 8 == 0:
        return "aligned, multiple of 8: unit 8"
    return "misaligned, multiple of 8: unit 1"


def fast32_case(life, step):
    """The branch of k_bytes_tree_digest a 32-B BYTES step reaches, or None."""
    if life.kind != BYTES or life.L != 32 or step.work == 0 or chunks_of(step.n_new, 4) <= 1:
        return None
    return "fast32" if life.off % 16 == 0 else "misaligned 32-B elements"


def level1_case(life, step):
    """Which level-1 forms of lt_update a LIST step can reach (a chunk pair of 256 B at a 16-B aligned base
    takes hash_window3; this names the 256-B pair at another base, which no other test reaches)."""
    if life.kind != LIST or step.work == 0 or chunks_of(step.n_new, life.per) <= 2:
        return None
    if life.per * life.L == 128 and life.off % 16:
        return "256-B pair, misaligned"
    return None


class Coverage:
    def __init__(self, lives):
        self.lives = len(lives)
        self.steps = sum(len(lf.steps) for lf in lives)
        self.step_kinds = Counter(st.kind for lf in lives for st in lf.steps)
        self.lens = Counter(lf.L for lf in lives)
        self.pairs = {(lf.kind, lf.L, lf.off) for lf in lives}
        self.scatter = Counter(c for lf in lives for st in lf.steps if (c := scatter_case(lf, st)))
        self.fast32 = Counter(c for lf in lives for st in lf.steps if (c := fast32_case(lf, st)))
        self.level1 = Counter(c for lf in lives for st in lf.steps if (c := level1_case(lf, st)))
        self.small = sum(lf.small for lf in lives)
        self.exact = sum(lf.cap == lf.n0 for lf in lives)
        self.k1024 = sum(lf.shape == "k1024" and lf.steps[0].kind == "append_taller" for lf in lives)
        self.validator = sum(lf.kind == STRUCT and lf.L == VALIDATOR_LEN for lf in lives)
        self.with_values = sum(st.with_values for lf in lives for st in lf.steps)

    def line(self):
        return (f"{self.lives} lives, {self.steps} steps, {len(self.pairs)} distinct (kind, item_len, offset), "
                f"{self.small} lives below 40 chunks, {self.exact} with capacity == n")

    def check_common(self):
        """What every fuzz test must reach (asserted for the committed seed)."""
        missing = [k for k in STEP_KINDS if not self.step_kinds[k]]
        assert not missing, f"step kinds never drawn: {missing}"
        assert 3 * self.small >= self.lives, f"{self.small} of {self.lives} lives below 40 chunks"
        assert 0.15 * self.lives <= self.exact <= 0.3 * self.lives, f"{self.exact} of {self.lives}: capacity == n"
        assert self.k1024 >= 1, "no life appends across 1024 chunks"
        assert 0.4 * self.steps <= self.with_values <= 0.6 * self.steps, "steps that pass d_values: about half"

    def check_list(self):
        self.check_common()
        assert sorted(self.lens) == ITEM_LENS, f"item lengths drawn: {sorted(self.lens)}"
        assert len(self.scatter) == 3, f"scatter cases reached: {dict(self.scatter)}"
        assert self.level1["256-B pair, misaligned"], "no 256-B level-1 pair at a misaligned base"

    def check_bytes(self):
        self.check_common()
        assert sorted(self.lens) == ELEM_LENS, f"element lengths drawn: {sorted(self.lens)}"
        assert len(self.fast32) == 2, f"fast32 branches reached: {dict(self.fast32)}"

    def check_struct(self):
        self.check_common()
        assert self.validator >= 1, "the validator layout was never drawn"
        assert len(self.lens) >= 5, f"record lengths drawn: {sorted(self.lens)}"


def flatten_calls(call_lives):
    return [lf for cl in call_lives for lf in cl.lives]
