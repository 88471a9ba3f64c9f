"""Seeded, stateful, model-based fuzz of the device-resident trees
(mk_dev_ssz_list_tree_* / struct_list_tree_* / bytes_list_tree_* and
mk_dev_ssz_trees_update) through prysm_amd.device, bit-exact against the CPU
oracle.  The plan (lives, steps, placement) is tests/tree_fuzz_plan.py's and
is checked without a device by test_tree_fuzz_host.py; the comparison is
oracle_tree / split_levels / compare_tree of test_gpu_list_tree.py.

The model is a host numpy copy of each tree's whole item allocation.  After
every step: the root against O.merkle_hash_flat, the whole item allocation
(canaries in front and behind, the unused capacity) against the model and, for
STRUCT and BYTES trees, the canary behind the used part of level 0.  After the
build, every third step and the last step also every stored node of every level
and level 0 against O.struct_roots / O.elem_digests.

The default numbers of lives (tree_fuzz_plan.LIVES) were chosen on one MI355X
so that every test function stays at a few seconds; measured there at the
default seed (wall time of the test function, oracle included):
  test_fuzz_list_tree         360 lives, 3246 steps,  99 (item_len, offset)   3.6 s
  test_fuzz_bytes_list_tree   180 lives, 1622 steps,  43 (elem_len, offset)   3.8 s
  test_fuzz_struct_list_tree  180 lives, 1616 steps,  94 (record_len, offset) 3.7 s
  test_fuzz_trees_update      340 lives in 42 groups, 385 calls, 3102 steps   3.6 s
  test_container_lengths      25 cases, under 5 ms each
PRYSM_FUZZ_SCALE multiplies the lives for a longer run by hand."""
import numpy as np
import pytest

from tests import tree_fuzz_plan as P
from tests.test_gpu_list_tree import compare_tree, split_levels
from tests.tree_fuzz_plan import BYTES, LIST, STRUCT

pytestmark = pytest.mark.gpu

CANARY, FILL = 0xA5, 0xC3  # guard bytes; the capacity behind the list
FRONT = BACK = 64


@pytest.fixture(scope="module")
def gpu():
    import torch

    from prysm_amd import _lib

    assert torch.cuda.is_available()
    assert _lib.device_count() >= 1
    return torch.device("cuda:0")


def _rand(nbytes, salt):
    from oracle import oracle as O

    return O.splitmix_bytes((nbytes + 7) // 8 * 8, P.SEED + salt)[:nbytes].copy()


class DevTree:
    """A device tree of one life and its host model."""

    def __init__(self, gpu, life, salt):
        import torch

        from prysm_amd import device as D

        self.life, self.salt, self.n = life, salt, life.n0
        kind, L, cap = life.kind, life.L, life.cap
        self.len0 = L if kind == LIST else 32
        self.lo = FRONT + life.off
        self.model = np.full(self.lo + cap * L + BACK, CANARY, np.uint8)
        body = self.model[self.lo:self.lo + cap * L]
        body[:] = FILL
        body[:self.n * L] = _rand(self.n * L, salt)
        self.rows = body.reshape(cap, L)
        self.base = torch.from_numpy(self.model.copy()).to(gpu)
        self.items = self.base[self.lo:]
        assert self.items.data_ptr() % 16 == life.off % 16
        self.level0 = (torch.full((32 * cap + BACK,), CANARY, dtype=torch.uint8, device=gpu)
                       if kind != LIST else None)
        self.lv = torch.zeros(max(D.list_tree_levels_bytes(cap, self.len0), 32), dtype=torch.uint8, device=gpu)
        self.root = torch.zeros(32, dtype=torch.uint8, device=gpu)
        if kind == LIST:
            D.list_tree_build(self.items, self.n, cap, L, self.lv, self.root)
        elif kind == STRUCT:
            D.struct_list_tree_build(self.items, self.n, cap, L, life.spec, self.level0, self.lv, self.root)
        else:
            D.bytes_list_tree_build(self.items, self.n, cap, L, self.level0, self.lv, self.root)

    def stage(self, step, s):
        """Upload step s (indices, values), bring the model up to date and
        return (d_idx, d_values): d_values None for a step that writes the new
        bytes into the item buffer itself, on the same stream, before the call."""
        import torch

        gpu, L, k = self.base.device, self.life.L, step.k
        assert step.n_old == self.n
        vals = _rand(step.work * L, self.salt + 1 + s).reshape(step.work, L)
        d_idx = torch.from_numpy(step.idx).to(gpu) if k else None
        d_vals = None
        if step.with_values:
            vbuf = torch.empty(step.val_off + vals.size + 16, dtype=torch.uint8, device=gpu)
            d_vals = vbuf[step.val_off:]
            d_vals[:vals.size].copy_(torch.from_numpy(vals.reshape(-1)))
            assert d_vals.data_ptr() % 8 == step.val_off % 8
        elif step.work:
            valid = step.idx < step.n_old
            if valid.any():
                rows = self.items[:step.n_old * L].view(step.n_old, L)
                rows[torch.from_numpy(step.idx[valid]).to(gpu)] = torch.from_numpy(vals[:k][valid]).to(gpu)
            if step.n_new > step.n_old:
                self.items[step.n_old * L:step.n_new * L] = torch.from_numpy(vals[k:].reshape(-1)).to(gpu)
        P.apply_step(self.rows, step, vals)
        self.n = step.n_new
        return d_idx, d_vals

    def update(self, step, s):
        """The step through this kind's own update entry."""
        from prysm_amd import device as D

        lf = self.life
        d_idx, d_vals = self.stage(step, s)
        if lf.kind == LIST:
            D.list_tree_update(self.items, step.n_old, step.n_new, lf.cap, lf.L, self.lv, self.root, d_idx, step.k,
                               d_vals)
        elif lf.kind == STRUCT:
            D.struct_list_tree_update(self.items, step.n_old, step.n_new, lf.cap, lf.L, lf.spec, self.level0,
                                      self.lv, self.root, d_idx, step.k, d_vals)
        else:
            D.bytes_list_tree_update(self.items, step.n_old, step.n_new, lf.cap, lf.L, self.level0, self.lv,
                                     self.root, d_idx, step.k, d_vals)

    def args(self, step, s, container_off):
        """The step as one tree of a trees_update call."""
        from prysm_amd import device as D

        lf = self.life
        d_idx, d_vals = self.stage(step, s)
        return D.TreeArgs(lf.kind, self.items, step.n_old, step.n_new, lf.cap, lf.L, self.lv, self.root,
                          level0=self.level0, idx=d_idx, k_idx=step.k, values=d_vals, spec=lf.spec,
                          container_off=container_off)

    def want_level0(self):
        from oracle import oracle as O

        lf, n = self.life, self.n
        rows = self.rows[:n]
        if lf.kind == LIST:
            return rows.reshape(-1)
        if n == 0:
            return np.zeros(0, np.uint8)
        if lf.kind == STRUCT:
            return O.struct_roots(rows, n, lf.L, lf.spec).reshape(-1)
        return O.elem_digests(rows, n, lf.L).reshape(-1)

    def check(self, what, full):
        """After a synchronize.  Returns the oracle's root."""
        from oracle import oracle as O

        lf, n = self.life, self.n
        what = f"{lf.name()}: {what}"
        want0 = self.want_level0()
        want_root = O.merkle_hash_flat(want0, n, self.len0)
        root = self.root.cpu().numpy()
        assert bytes(root) == want_root, f"{what}: root"
        got = self.base.cpu().numpy()
        assert (got[:self.lo] == CANARY).all(), f"{what}: bytes in front of the items"
        assert (got[len(got) - BACK:] == CANARY).all(), f"{what}: bytes behind the items"
        bad = np.flatnonzero(got != self.model)
        assert bad.size == 0, f"{what}: item allocation differs at bytes {bad[:8] - self.lo} of the item buffer"
        got0 = got[self.lo:]
        if lf.kind != LIST:
            got0 = self.level0.cpu().numpy()
            assert (got0[32 * n:] == CANARY).all(), f"{what}: bytes behind the used part of level 0"
        if full:
            if lf.kind != LIST:
                bad = np.flatnonzero((got0[:32 * n] != want0).reshape(n, 32).any(axis=1))
                assert bad.size == 0, f"{what}: level 0 entries {bad[:8]} of {n}"
            levels = split_levels(self.lv.cpu().numpy(), n, lf.cap, self.len0)
            compare_tree(got0, levels, root, want0, n, self.len0, what)
        return want_root


def _full(s, nsteps):
    return s % 3 == 2 or s == nsteps - 1


def run_lives(gpu, lives, salt0):
    import torch

    for i, lf in enumerate(lives):
        t = DevTree(gpu, lf, salt0 + 100 * i)
        torch.cuda.synchronize()
        t.check("build", True)
        for s, st in enumerate(lf.steps):
            t.update(st, s)
            torch.cuda.synchronize()
            t.check(f"step {s} {st.kind} idx={st.idx[:6]} n {st.n_old} -> {st.n_new} "
                    f"values={st.with_values}+{st.val_off}", _full(s, len(lf.steps)))


def test_fuzz_list_tree(gpu):
    lives = P.plan_list()
    cov = P.Coverage(lives)
    print("list tree:", cov.line(), dict(cov.scatter), dict(cov.level1))
    if P.FUZZ_SEED == 0:
        cov.check_list()
    run_lives(gpu, lives, 100_000)


def test_fuzz_bytes_list_tree(gpu):
    lives = P.plan_bytes()
    cov = P.Coverage(lives)
    print("bytes tree:", cov.line(), dict(cov.fast32))
    if P.FUZZ_SEED == 0:
        cov.check_bytes()
    run_lives(gpu, lives, 200_000)


def test_fuzz_struct_list_tree(gpu):
    lives = P.plan_struct()
    cov = P.Coverage(lives)
    print("struct tree:", cov.line(), f"{cov.validator} validator lives, {len(cov.lens)} record lengths")
    if P.FUZZ_SEED == 0:
        cov.check_struct()
    run_lives(gpu, lives, 300_000)


# ---- several trees and their container in one call ------------------------------------------------
class Container:
    """A container message of exactly `length` bytes at base + base_off and its
    32-B root at root_off of its own allocation, canaries behind both."""

    def __init__(self, gpu, length, base_off, root_off, salt):
        import torch

        self.length, self.base_off, self.root_off = length, base_off, root_off
        self.msg = _rand(length, salt)
        host = np.full(base_off + length + BACK, CANARY, np.uint8)
        host[base_off:base_off + length] = self.msg
        self.buf = torch.from_numpy(host).to(gpu)
        self.rootbuf = torch.full((root_off + 32 + BACK,), CANARY, dtype=torch.uint8, device=gpu)
        self.d_msg, self.d_root = self.buf[base_off:], self.rootbuf[root_off:]

    def check(self, roots, what):
        """roots: [(offset, oracle root)] of the trees that are fields of the container."""
        from oracle import oracle as O

        want = self.msg.copy()
        for off, r in roots:
            want[off:off + 32] = np.frombuffer(r, np.uint8)
        got = self.buf.cpu().numpy()
        assert (got[:self.base_off] == CANARY).all(), f"{what}: bytes in front of the container"
        assert (got[self.base_off + self.length:] == CANARY).all(), f"{what}: bytes behind the container"
        bad = np.flatnonzero(got[self.base_off:self.base_off + self.length] != want)
        assert bad.size == 0, f"{what}: container message differs at bytes {bad[:8]}"
        got = self.rootbuf.cpu().numpy()
        assert (got[:self.root_off] == CANARY).all() and (got[self.root_off + 32:] == CANARY).all(), \
            f"{what}: bytes around the container root"
        assert bytes(got[self.root_off:self.root_off + 32]) == O.keccak256(bytes(want)), f"{what}: container root"


def test_fuzz_trees_update(gpu):
    import torch

    from prysm_amd import device as D

    call_lives = P.plan_calls()
    cov = P.Coverage(P.flatten_calls(call_lives))
    ncalls = sum(len(cl.calls) for cl in call_lives)
    print("trees_update:", cov.line(), f"{len(call_lives)} groups of trees, {ncalls} calls")
    if P.FUZZ_SEED == 0:
        cov.check_common()
        assert {lf.kind for lf in P.flatten_calls(call_lives)} == {LIST, STRUCT, BYTES}
        assert {len(cl.lives) for cl in call_lives} >= {1, 16}, "tree counts 1 and 16 per call"
        assert any(o is None for cl in call_lives for c in cl.calls for o in c.offs)
    for g, cl in enumerate(call_lives):
        trees = [DevTree(gpu, lf, 400_000 + 10_000 * g + 100 * i) for i, lf in enumerate(cl.lives)]
        torch.cuda.synchronize()
        for t in trees:
            t.check(f"group {g} build", True)
        for s, call in enumerate(cl.calls):
            box = Container(gpu, call.length, call.base_off, call.root_off, 900_000 + 100 * g + s)
            args = [t.args(t.life.steps[s], s, off) for t, off in zip(trees, call.offs)]
            D.trees_update(args, box.d_msg, call.length, box.d_root)
            torch.cuda.synchronize()
            roots = []
            for i, (t, off) in enumerate(zip(trees, call.offs)):
                st = t.life.steps[s]
                r = t.check(f"group {g} call {s} tree {i}/{len(trees)} {st.kind} idx={st.idx[:6]} "
                            f"n {st.n_old} -> {st.n_new} values={st.with_values}+{st.val_off}",
                            _full(s, len(cl.calls)))
                if off is not None:
                    roots.append((off, r))
            box.check(roots, f"group {g} call {s}: container of {call.length} bytes at +{call.base_off}, "
                             f"offsets {call.offs}")


# ---- the container hash at every length class -----------------------------------------------------
CONTAINER_LENS = [32, 33, 34, 35, 37, 67, 103, 133, 134, 135, 136, 137, 139, 168, 271, 272, 273, 407, 408, 409, 680,
                  4093, 4094, 4095, 4096]


def container_offsets(length):
    """Offset 0, the last legal 4-B aligned offset and one in the middle: as many of them as fit without overlap."""
    last = (length - 32) & ~3
    offs = [0]
    if last >= 32:
        offs.append(last)
        mid = (last // 2) & ~3
        if mid >= 32 and mid + 32 <= last:
            offs.append(mid)
    return offs


@pytest.mark.parametrize("length", CONTAINER_LENS)
def test_container_lengths(gpu, length):
    """Three small trees, one of each kind, 2 to 9 chunks each and one dirty
    item each, as fields of a container of exactly `length` bytes that lies at
    a 4-B, not 8-B, aligned address, as does its root."""
    import random

    import torch

    from prysm_amd import device as D
    from prysm_amd import registry as R

    rng = random.Random(P.SEED + length)
    offs = container_offsets(length)
    assert len(offs) == (3 if length >= 96 else 2 if length >= 64 else 1)
    shapes = [(LIST, 8, None, 0, P.LIST_VAL_OFFS), (STRUCT, P.VALIDATOR_LEN, R.VALIDATOR_FIELDS, 4, P.STRUCT_VAL_OFFS),
              (BYTES, 48, None, 1, P.BYTES_VAL_OFFS)]
    trees = []
    for i, (kind, L, spec, off, val_offs) in enumerate(shapes[:len(offs)]):
        per = P.per_of(kind, L)
        n = rng.randint(2, 9) * per - rng.randrange(per)
        lf = P.Life(kind, L, spec, off, val_offs, "container", n, n + rng.randrange(2 * per))
        lf.steps.append(P.Step("scattered", [rng.randrange(n)], n, n, rng.random() < 0.5, rng.choice(val_offs)))
        trees.append(DevTree(gpu, lf, 700_000 + 1000 * length + 100 * i))
    box = Container(gpu, length, 4, 4, 800_000 + length)
    assert box.d_msg.data_ptr() % 8 == 4 and box.d_root.data_ptr() % 8 == 4
    D.trees_update([t.args(t.life.steps[0], 0, off) for t, off in zip(trees, offs)], box.d_msg, length, box.d_root)
    torch.cuda.synchronize()
    roots = [(off, t.check(f"container of {length} bytes, tree {i}", True))
             for i, (t, off) in enumerate(zip(trees, offs))]
    box.check(roots, f"container of {length} bytes, roots at {offs}")
