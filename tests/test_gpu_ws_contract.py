"""The memory contract of the one-shot device entry points (the calls bench.py
times and a cgo caller reaches first), through ``_lib.invoke`` with the
library's own sizes -- no wrapper of prysm_amd/device.py pads anything here.

Every buffer of a call is a region of one guarded arena (tests/guarded_arena.py):
the workspace is exactly as large as the entry's documented query says, 64 KiB
of 0xA5 lie on both sides of every region, and the inputs are snapshotted.
Per case (``_run``):

1. exact size: the call returns MK_OK, the output equals the oracle's, every
   guard byte is intact, the inputs are unchanged;
2. stale scratch: the same call with the workspace and the output poisoned
   with 0x00, then 0xFF, gives the same bytes;
3. one byte short: MK_ENOMEM with both sizes in the text, and neither the
   workspace nor the output loses its poison (nothing was launched).  Not for
   shapes that need no workspace at all: merkleHash of at most one chunk
   (``p.small``) and a finisher of at most 64 nodes (one k_wave3 workgroup
   straight from the input) -- their queries return a 256-byte floor the
   library never reads;
4. output extent: a frontier writes 32 * nodes_out bytes of its 32 << k, a
   pair finisher its slot, the struct root at [64, 96) and the arrival word
   the header places at [96, 100), nothing else.

``test_ws_alignment`` gives the entries whose header states a workspace
alignment a workspace shifted by 8.

Sizes used for the two subtree entries: mk_ssz_merkle_workspace_bytes(shard_n,
item_len), the rule include/prysm_merkle.h states (tests/c_abi/planner_fuzz.cpp
holds it as a property of the planner).
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from tests.guarded_arena import GuardedArena

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED000000000000 + 0xC0A7
NT = 16  # oracle threads

# ---- shapes (the smallest that reach each planner branch; planner.cpp, merkle_api.cpp) -----------
# 32-B items, n = 8 * windows
MERKLE_N = [
    0, 1, 4,                    # no chunk / one chunk (p.small)
    5, 9,                       # two chunks, odd third
    129, 8 * 4096,              # the list-tree fast path's edges, 16 < c1 <= 4096
    8 * 4096 + 1,               # first k_wave3 leaf pass, ragged
    1 << 20,                    # last wave width (c1 = 2^17)
    (1 << 20) + 1,              # first k_reduce NI = 1, tail workgroup of one 32-B item
    (1 << 21) - 8,              # top of NI = 1 (c1 = 2^18 - 1)
    (1 << 21) + 9,              # first NI = 2, ragged
    257 * 32768 + 3,            # locked leaf pass: 257 groups and a ragged tail
]
SHARD_N = [n for n in MERKLE_N if n >= 129]  # below, shard_plan(n, 32, 4) does not shard


def _n_for_c1(c1: int, item_len: int) -> int:
    """The smallest n whose first level has c1 windows."""
    per = 128 // item_len if item_len < 128 else 1
    return (2 * c1 - 2) * per + 1


# the wide generic leaf pass, k_reduce<true, false, NI> as a whole pass: (item_len, c1, pointer shift)
WIDE = [(il, c1, 0) for il in (48, 200, 129, 3) for c1 in ((1 << 17) + 1, (1 << 18) + 1)] + \
       [(32, (1 << 18) + 1, 8), (32, (1 << 18) + 1, 1), (8, (1 << 17) + 1, 4)]

NODE_COUNTS = [2, 3, 1025, 1 << 18, (1 << 18) + 3, (1 << 23) + (1 << 15) + 7]

MANY_EXTRA = [(140_001, 48)]  # a generic list above kManyBigChunks beside the 32-B ones of _SHAPES

BYTES_LIST = [(32, 7, 0), (32, 7, 1), (32, 8 * 4096 + 8, 0), (32, 8 * 4096 + 8, 1), (32, (1 << 20) + 8, 0),
              (32, (1 << 20) + 8, 1), (48, 1000, 0)]


@pytest.fixture(scope="module")
def gpu():
    import torch

    from prysm_amd import _lib

    assert torch.cuda.is_available()
    _lib.init(0)
    return torch.device("cuda:0")


def build_plan_probe(tmpdir):
    """tests/c_abi/plan_probe.cpp over the host planner: the passes of a merkleHash plan."""
    exe = os.path.join(str(tmpdir), "plan_probe")
    csrc = os.path.join(ROOT, "prysm_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Werror", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "plan_probe.cpp"), os.path.join(csrc, "planner.cpp"),
                    "-o", exe], check=True)

    def passes(n, item_len, aligned16):
        r = subprocess.run([exe, str(n), str(item_len), "1" if aligned16 else "0"], capture_output=True, text=True,
                           check=True)
        out = []
        for line in r.stdout.splitlines():
            f = line.split()
            if f[0] == "pass":
                out.append({f[i]: int(f[i + 1]) for i in range(2, len(f), 2)})
        return out

    return passes


@pytest.fixture(scope="module")
def plan_probe(tmp_path_factory):
    return build_plan_probe(tmp_path_factory.mktemp("probe"))


# ---- inputs and oracle values, computed once ------------------------------------------------------
@functools.lru_cache(maxsize=3)
def _stream_bytes(nbytes: int, seed: int) -> np.ndarray:
    from oracle import oracle as O

    return O.splitmix_bytes(max(8, nbytes + (-nbytes) % 8), seed)[:nbytes]


@functools.lru_cache(maxsize=None)
def _merkle_root_of(n: int, item_len: int, seed: int) -> bytes:
    from oracle import oracle as O

    return O.merkle_hash_flat(_stream_bytes(n * item_len, seed), n, item_len, nthreads=NT)


def _shards(n: int, item_len: int = 32, world: int = 4):
    from prysm_amd import device as D

    return D.shard_plan(n, item_len, world)


# ---- the contract runner ---------------------------------------------------------------------------
class Case:
    """One call: ``inputs`` [(region, array, align, shift)], the exact
    ``ws_bytes``, the output region's size, ``call(ar, ws_ptr, ws_bytes)``,
    and ``check(ar, out, poison)`` -> the bytes the two poisoned runs must
    agree on (it compares them with the oracle and the rest with the poison)."""

    def __init__(self, name, inputs, ws_bytes, out_bytes, call, check, short=True, ws_align=256, ws_shift=0,
                 out_align=256, extra=(), prepare=None, out_poisoned=((0, None),)):
        self.name, self.inputs, self.ws_bytes, self.out_bytes = name, inputs, int(ws_bytes), out_bytes
        self.call, self.check, self.short = call, check, short
        self.ws_align, self.ws_shift, self.out_align = ws_align, ws_shift, out_align
        self.extra = list(extra)      # further output regions [(name, nbytes, align)]
        self.prepare = prepare        # prepare(ar, poison): after poisoning, before the call
        self.out_poisoned = out_poisoned  # the output's byte ranges that hold the poison when a call is refused


def _arena(dev, c):
    import torch

    regs = [(nm, a.size, al, sh) for nm, a, al, sh in c.inputs]
    regs.append(("ws", c.ws_bytes, c.ws_align, c.ws_shift))
    regs.append(("out", c.out_bytes, c.out_align, 0))
    regs += [(nm, nb, al, 0) for nm, nb, al in c.extra]
    ar = GuardedArena(dev, regs)
    for nm, a, _al, _sh in c.inputs:
        if a.size:
            ar.view(nm).copy_(torch.from_numpy(np.ascontiguousarray(a)))
        ar.snapshot(nm)
    return ar


def _poison_all(ar, c, byte):
    for nm in ["ws", "out"] + [e[0] for e in c.extra]:
        ar.poison(nm, byte)
    if c.prepare:
        c.prepare(ar, byte)


def _run(dev, c):
    import torch

    from prysm_amd import _lib

    ar = _arena(dev, c)
    seen = []
    for poison in (0x00, 0xFF):
        what = f"{c.name}, exact workspace of {c.ws_bytes} bytes poisoned 0x{poison:02X}: "
        _poison_all(ar, c, poison)
        c.call(ar, ar.ptr("ws"), c.ws_bytes)  # raises unless MK_OK
        torch.cuda.synchronize()
        seen.append(c.check(ar, ar.view("out").cpu().numpy(), poison))
        ar.check_guards(what)
        for nm, _a, _al, _sh in c.inputs:
            ar.assert_unchanged(nm, what)
    assert seen[0] == seen[1], f"{c.name}: the result depends on what the workspace and the output held before"
    if c.short and c.ws_bytes:
        what = f"{c.name}, workspace one byte short ({c.ws_bytes - 1}): "
        _poison_all(ar, c, 0x5A)
        with pytest.raises(_lib.MerkleError) as e:
            c.call(ar, ar.ptr("ws"), c.ws_bytes - 1)
        torch.cuda.synchronize()
        assert e.value.code == _lib.MK_ENOMEM, what + str(e.value)
        assert str(c.ws_bytes - 1) in str(e.value) and str(c.ws_bytes) in str(e.value), what + str(e.value)
        for nm in ["ws"] + [x[0] for x in c.extra]:
            ar.assert_poison(nm, 0x5A, what=what)
        for lo, hi in c.out_poisoned:
            ar.assert_poison("out", 0x5A, lo, hi, what=what)
        ar.check_guards(what)
    return seen[0]


def _root_check(want: bytes, name: str):
    def check(ar, out, poison):
        assert out[:32].tobytes() == want, f"{name}: {out[:32].tobytes().hex()} != oracle {want.hex()}"
        assert (out[32:] == poison).all(), f"{name}: bytes past the 32-B result changed"
        return out[:32].tobytes()

    return check


def _stream(dev):
    from prysm_amd import device as D

    return D._stream(dev)


def _vp(x):
    return ctypes.c_void_p(x)


# ---- mk_dev_ssz_merkle_hash ------------------------------------------------------------------------
def _merkle_case(dev, n, item_len, shift, seed, ws_shift=0):
    from prysm_amd import _lib

    arr = _stream_bytes(n * item_len, seed)
    want = _merkle_root_of(n, item_len, seed)
    ws = _lib.load().mk_ssz_merkle_workspace_bytes(n, item_len)
    chunks = -(-n * item_len // ((128 // item_len) * item_len if item_len < 128 else item_len)) if n else 0
    name = f"mk_dev_ssz_merkle_hash(n={n}, item_len={item_len}, items shifted {shift}, ws shifted {ws_shift})"

    def call(ar, wsp, wsb):
        _lib.invoke("mk_dev_ssz_merkle_hash", _vp(ar.ptr("items")), n, item_len, _vp(ar.ptr("out")), _vp(wsp), wsb,
                    _stream(dev), device=0)

    return Case(name, [("items", arr, 256, shift)], ws, 32, call, _root_check(want, name), short=chunks > 1,
                ws_shift=ws_shift)


@pytest.mark.parametrize("n", MERKLE_N)
def test_merkle_hash(gpu, n):
    _run(gpu, _merkle_case(gpu, n, 32, 0, SEED + 1))


def _wide_id(w):
    return f"len{w[0]}-c1_{w[1]}-shift{w[2]}"


def wide_plan_ok(passes, item_len, c1, shift):
    """Pass 0 is the generic throughput pass as a whole pass, with the NI the width implies."""
    p0 = passes(_n_for_c1(c1, item_len), item_len, shift % 16 == 0)[0]
    want_ni = 1 if c1 < (1 << 18) else 2
    assert p0["leaf"] == 1 and p0["wave"] == 0 and p0["sp"] == 0 and p0["nlock"] == 0, p0
    assert p0["nfast"] == 0 and p0["ni"] == want_ni and p0["c1"] == c1, p0
    assert p0["nwg"] == -(-c1 // (512 * want_ni)) and p0["nwg"] > 1, p0


@pytest.mark.parametrize("w", WIDE, ids=_wide_id)
def test_merkle_hash_wide_generic(gpu, plan_probe, w):
    """k_reduce<true, false, 1> and <true, false, 2> as whole leaf passes:
    chunk sizes other than 128 B, and item pointers that are not 16-B
    aligned, above kLeafWaveMaxC1 = 2^17 windows.  The plan is asserted, so a
    later threshold change cannot quietly move a case back onto k_wave3."""
    item_len, c1, shift = w
    wide_plan_ok(plan_probe, item_len, c1, shift)
    _run(gpu, _merkle_case(gpu, _n_for_c1(c1, item_len), item_len, shift, SEED + 2 + item_len))


# ---- the subtree and frontier forms ----------------------------------------------------------------
@pytest.mark.parametrize("which", ["first", "last"])
@pytest.mark.parametrize("n", SHARD_N)
def test_merkle_subtree(gpu, n, which):
    from oracle import oracle as O
    from prysm_amd import _lib

    il, seed = 32, SEED + 1
    h, ne, begin = _shards(n)
    assert ne > 1
    s = 0 if which == "first" else ne - 1
    sn = begin[s + 1] - begin[s]
    arr = _stream_bytes(n * il, seed)[begin[s] * il:begin[s + 1] * il]
    want = O.merkle_subtree_gen(n, il, seed, s, h, nthreads=NT)
    ws = _lib.load().mk_ssz_merkle_workspace_bytes(sn, il)
    name = f"mk_dev_ssz_merkle_subtree(n={n}, shard {s} of {ne}: {sn} items, height {h})"

    def call(ar, wsp, wsb):
        _lib.invoke("mk_dev_ssz_merkle_subtree", _vp(ar.ptr("items")), sn, il, h, 1, _vp(ar.ptr("out")), _vp(wsp),
                    wsb, _stream(gpu), device=0)

    _run(gpu, Case(name, [("items", arr, 256, 0)], ws, 32, call, _root_check(want, name)))


@pytest.mark.parametrize("kk", ["k1", "kmax"])
@pytest.mark.parametrize("n", SHARD_N)
def test_merkle_subtree_frontier(gpu, n, kk):
    """Every shard's frontier 1 level, and height - 1 levels, below its root:
    32 * nodes_out bytes of the 32 << k are written, a ragged last shard and
    a lone node under pad_at_one included.  The shards' frontiers in order
    are a level of the whole tree: the oracle finishes it to the root."""
    from oracle import oracle as O
    from prysm_amd import _lib
    from prysm_amd import parallel as P

    il, seed = 32, SEED + 1
    h, ne, begin = _shards(n)
    k = 1 if kk == "k1" else h - 1
    if kk == "kmax" and k == 1:
        k = 0  # nothing new
    if k == 0 or k >= h:
        return
    level = []
    for s in range(ne):
        sn = begin[s + 1] - begin[s]
        arr = _stream_bytes(n * il, seed)[begin[s] * il:begin[s + 1] * il]
        ws = _lib.load().mk_ssz_merkle_workspace_bytes(sn, il)
        want_nodes = P.frontier_count(sn, il, h, k)
        got_nodes = ctypes.c_uint64(0)
        name = f"mk_dev_ssz_merkle_subtree_frontier(n={n}, shard {s}: {sn} items, height {h}, frontier {k})"

        def call(ar, wsp, wsb):
            _lib.invoke("mk_dev_ssz_merkle_subtree_frontier", _vp(ar.ptr("items")), sn, il, h, k, 1,
                        _vp(ar.ptr("out")), ctypes.byref(got_nodes), _vp(wsp), wsb, _stream(gpu), device=0)

        def check(ar, out, poison):
            assert got_nodes.value == want_nodes, (name, got_nodes.value, want_nodes)
            assert (out[32 * want_nodes:] == poison).all(), f"{name}: wrote past its {want_nodes} nodes"
            return out[:32 * want_nodes].tobytes()

        try:
            level.append(_run(gpu, Case(name, [("items", arr, 256, 0)], ws, 32 << k, call, check)))
        except _lib.MerkleError as e:
            # the planner takes no single-level throughput pass (a frontier one level above the
            # chunks of a wide shard): refused on the host for every shard alike, nothing to compare
            assert e.code == _lib.MK_EINVAL and "single-level" in str(e) and h - k == 1 and s == 0, (name, str(e))
            return
    nodes = np.frombuffer(b"".join(level), dtype=np.uint8)
    assert O.merkle_nodes(nodes, nodes.size // 32, n, nthreads=NT) == _merkle_root_of(n, il, seed)


# ---- the node entries ------------------------------------------------------------------------------
def _levels_to_one(c):
    lv = 0
    while c > 1:
        c = (c + 1) // 2
        lv += 1
    return lv


def _nodes(count):
    return _stream_bytes(32 * count, SEED + 5)


@functools.lru_cache(maxsize=None)
def _nodes_root(count, n_total):
    from oracle import oracle as O

    return O.merkle_nodes(_nodes(count), count, n_total, nthreads=NT)


@pytest.mark.parametrize("count", NODE_COUNTS)
def test_finish_nodes(gpu, count):
    from prysm_amd import _lib

    n_total = 4 * count - 1
    ws = _lib.load().mk_ssz_merkle_finish_workspace_bytes(count)
    name = f"mk_dev_ssz_merkle_finish_nodes(count={count})"

    def call(ar, wsp, wsb):
        _lib.invoke("mk_dev_ssz_merkle_finish_nodes", _vp(ar.ptr("nodes")), count, n_total, _vp(ar.ptr("out")),
                    _vp(wsp), wsb, _stream(gpu), device=0)

    _run(gpu, Case(name, [("nodes", _nodes(count), 256, 0)], ws, 32, call,
                   _root_check(_nodes_root(count, n_total), name), short=count > 64))


@pytest.mark.parametrize("count", NODE_COUNTS)
def test_finish_nodes_pair(gpu, count):
    """The pair block (MK_PAIR_BLOCK_BYTES = 128): one finisher writes its slot
    and zeroes the struct root at [64, 96); the second of the epoch writes the
    struct root.  [96, 100) is the arrival word the header gives the
    finishers (zero before the first use); [100, 128) is never touched."""
    import torch

    from oracle import oracle as O
    from prysm_amd import _lib

    slot = count % 2
    n_tot = [4 * count - 1, 4 * count - 2]  # of the finisher in slot `slot`, and of the other one
    roots = [_nodes_root(count, n_tot[0]), _nodes_root(count, n_tot[1])]
    ws = _lib.load().mk_ssz_merkle_finish_workspace_bytes(count)
    name = f"mk_dev_ssz_merkle_finish_nodes_pair(count={count}, slot={slot})"
    state = {"epoch": 0}

    def prepare(ar, poison):  # the header: the arrival word is zero before the block's first use
        ar.view("out")[96:100].zero_()
        state["epoch"] += 1
        state["both"] = poison == 0x00

    def one(ar, s, nt, wsp, wsb):
        _lib.invoke("mk_dev_ssz_merkle_finish_nodes_pair", _vp(ar.ptr("nodes")), count, nt, _vp(ar.ptr("out")), s,
                    state["epoch"], _vp(wsp), wsb, _stream(gpu), device=0)

    def call(ar, wsp, wsb):
        one(ar, slot, n_tot[0], wsp, wsb)
        if state["both"] and wsb == ws:  # the second run completes the pair (same stream: ordered)
            torch.cuda.synchronize()
            ar.check_guards(name + ", first finisher: ")
            one(ar, 1 - slot, n_tot[1], wsp, wsb)

    def check(ar, out, poison):
        assert out[32 * slot:32 * slot + 32].tobytes() == roots[0], name
        assert (out[100:128] == poison).all(), f"{name}: bytes [100, 128) of the pair block changed"
        if poison == 0xFF:  # one finisher only: the other slot untouched, the struct root zeroed
            assert (out[32 * (1 - slot):32 * (1 - slot) + 32] == poison).all(), f"{name}: the other slot changed"
            assert (out[64:96] == 0).all(), name
        else:
            assert out[32 * (1 - slot):32 * (1 - slot) + 32].tobytes() == roots[1], name
            pair = [roots[0], roots[1]] if slot == 0 else [roots[1], roots[0]]
            assert out[64:96].tobytes() == O.keccak256(pair[0] + pair[1]), f"{name}: struct root"
        return out[32 * slot:32 * slot + 32].tobytes()

    c = Case(name, [("nodes", _nodes(count), 256, 0)], ws, 128, call, check, short=count > 64, out_align=16,
             prepare=prepare, out_poisoned=((0, 96), (100, 128)))
    _run(gpu, c)


@pytest.mark.parametrize("pair", [False, True], ids=["one", "pair"])
@pytest.mark.parametrize("count", [c for c in NODE_COUNTS if c <= 1 << 20])
def test_top_fused(gpu, count, pair):
    """One list (a 32-B root) and two lists side by side (a pair block whose
    arrival word is not used: [96, 128) keeps its poison)."""
    from oracle import oracle as O
    from prysm_amd import _lib

    c1 = 3 if pair else 0
    n0, n1 = 4 * count - 1, 4 * c1
    nodes1 = _stream_bytes(32 * max(c1, 1), SEED + 6)
    ws = _lib.load().mk_ssz_merkle_top_fused_workspace_bytes(count, c1)
    assert ws > 0
    name = f"mk_dev_ssz_merkle_top_fused(count0={count}, count1={c1})"
    r0 = _nodes_root(count, n0)
    r1 = O.merkle_nodes(nodes1, c1, n1) if pair else b""

    def call(ar, wsp, wsb):
        _lib.invoke("mk_dev_ssz_merkle_top_fused", _vp(ar.ptr("nodes")), count, n0,
                    _vp(ar.ptr("nodes1")) if pair else None, c1, n1, _vp(ar.ptr("out")), 7, _vp(wsp), wsb,
                    _stream(gpu), device=0)

    def check(ar, out, poison):
        if not pair:
            return _root_check(r0, name)(ar, out, poison)
        assert out[:32].tobytes() == r0 and out[32:64].tobytes() == r1, name
        assert out[64:96].tobytes() == O.keccak256(r0 + r1), f"{name}: struct root"
        assert (out[96:] == poison).all(), f"{name}: bytes [96, 128) of the pair block changed"
        return out[:96].tobytes()

    inputs = [("nodes", _nodes(count), 8, 0)] + ([("nodes1", nodes1, 8, 0)] if pair else [])
    _run(gpu, Case(name, inputs, ws, 128 if pair else 32, call, check, ws_align=16, out_align=16))


@pytest.mark.parametrize("kk", ["top", "k1", "kmax"])
@pytest.mark.parametrize("count", NODE_COUNTS)
def test_node_frontier(gpu, count, kk):
    """`count` nodes reduced height = levels_to_one(count) levels with
    pad_at_one, to the top node (frontier 0) and to the frontiers 1 and
    height - 1 levels below it: the oracle continues each to the root."""
    from oracle import oracle as O
    from prysm_amd import _lib

    height = _levels_to_one(count)
    k = {"top": 0, "k1": 1, "kmax": height - 1}[kk]
    if (kk != "top" and (k < 1 or k >= height)) or (kk == "kmax" and k == 1):
        return  # no such frontier at this height, or the same as k1
    n_total = 4 * count - 1
    ws = _lib.load().mk_ssz_merkle_node_frontier_workspace_bytes(count, height, k)
    if ws == 0:
        # the planner takes no single-level throughput pass (the frontier one level above a level
        # too wide for k_wave3): the query says 0 and the call is MK_EINVAL on the host
        assert height - k == 1 and count > 1 << 18, (count, height, k)
        ar = GuardedArena(gpu, [("nodes", 32, 256, 0), ("ws", 256, 256, 0), ("out", 32, 256, 0)])
        with pytest.raises(_lib.MerkleError) as e:
            _lib.invoke("mk_dev_ssz_merkle_node_frontier", _vp(ar.ptr("nodes")), count, height, k, 1,
                        _vp(ar.ptr("out")), None, _vp(ar.ptr("ws")), 256, _stream(gpu), device=0)
        assert e.value.code == _lib.MK_EINVAL and "single-level" in str(e.value)
        return
    assert ws >= 256
    want_nodes = max(1, -(-count // (1 << (height - k)))) if k else 1
    got_nodes = ctypes.c_uint64(0)
    name = f"mk_dev_ssz_merkle_node_frontier(count={count}, height={height}, frontier={k})"

    def call(ar, wsp, wsb):
        _lib.invoke("mk_dev_ssz_merkle_node_frontier", _vp(ar.ptr("nodes")), count, height, k, 1, _vp(ar.ptr("out")),
                    ctypes.byref(got_nodes), _vp(wsp), wsb, _stream(gpu), device=0)

    def check(ar, out, poison):
        assert got_nodes.value == want_nodes, (name, got_nodes.value, want_nodes)
        assert (out[32 * want_nodes:] == poison).all(), f"{name}: wrote past its {want_nodes} nodes"
        lvl = out[:32 * want_nodes]
        if want_nodes == 1:  # the top node: the mix-in is all the reference adds
            got = O.keccak256(lvl.tobytes() + n_total.to_bytes(8, "little") + bytes(24))
        else:
            got = O.merkle_nodes(lvl, want_nodes, n_total, nthreads=NT)
        assert got == _nodes_root(count, n_total), name
        return lvl.tobytes()

    _run(gpu, Case(name, [("nodes", _nodes(count), 256, 0)], ws, 32 << k, call, check))


# ---- mk_dev_ssz_merkle_many ------------------------------------------------------------------------
@pytest.mark.parametrize("align", [16, 1])
def test_merkle_many(gpu, align):
    """The lists of test_gpu_merkle_many._SHAPES (two of them above
    kManyBigChunks, so the big lists' shared workspace at off_big is used) and
    one generic big list, at 16-B aligned and at odd offsets."""
    from oracle import oracle as O
    from prysm_amd import _lib
    from tests.test_gpu_merkle_many import _SHAPES

    shapes = list(_SHAPES) + MANY_EXTRA
    assert sum(1 for n, il in shapes if -(-n * il // ((128 // il) * il if il < 128 else il)) > 1 << 15) >= 3
    data = [O.splitmix_bytes(max(8, n * il + (-(n * il)) % 8), SEED + 40 + i)[:n * il]
            for i, (n, il) in enumerate(shapes)]
    offs, pos, parts = [], 0, []
    for a in data:
        pad = (-pos) % align + (3 if align == 1 else 0)
        parts.append(np.zeros(pad, np.uint8))
        pos += pad
        offs.append(pos)
        parts.append(a)
        pos += a.size
    buf = np.concatenate(parts)
    k = len(shapes)
    o = np.ascontiguousarray(offs, dtype=np.uint64)
    ns = np.ascontiguousarray([n for n, _ in shapes], dtype=np.uint64)
    ils = np.ascontiguousarray([il for _, il in shapes], dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    ws = _lib.load().mk_ssz_merkle_many_workspace_bytes(p(ns), p(ils), k)
    want = b"".join(O.merkle_hash_flat(a, n, il, nthreads=NT) for a, (n, il) in zip(data, shapes))
    name = f"mk_dev_ssz_merkle_many({k} lists at alignment {align})"

    def call(ar, wsp, wsb):
        _lib.invoke("mk_dev_ssz_merkle_many", _vp(ar.ptr("items")), p(o), p(ns), p(ils), k, _vp(ar.ptr("out")),
                    _vp(wsp), wsb, _stream(gpu), device=0)

    def check(ar, out, poison):
        got = out.tobytes()
        for i, (n, il) in enumerate(shapes):
            assert got[32 * i:32 * i + 32] == want[32 * i:32 * i + 32], f"{name}: list {i} ({n} x {il} B)"
        return got

    _run(gpu, Case(name, [("items", buf, 256, 0)], ws, 32 * k, call, check))


# ---- mk_dev_ssz_tree_hash_bytes_list ---------------------------------------------------------------
@pytest.mark.parametrize("b", BYTES_LIST, ids=lambda b: f"len{b[0]}-n{b[1]}-shift{b[2]}")
def test_tree_hash_bytes_list(gpu, b):
    """Aligned elements: the query.  Other alignments take the two-phase form
    and the size the header documents for it: the query plus n * 32 rounded
    up to 256."""
    from oracle import oracle as O
    from prysm_amd import _lib

    el, n, shift = b
    arr = _stream_bytes(n * el, SEED + 7 + el)
    want = O.tree_hash_bytes_list(arr, n, el, nthreads=NT)
    ws = _lib.load().mk_ssz_tree_hash_bytes_list_workspace_bytes(n, el)
    if shift % 16:
        ws += -(-n * 32 // 256) * 256
    name = f"mk_dev_ssz_tree_hash_bytes_list(n={n}, elem_len={el}, elements shifted {shift})"

    def call(ar, wsp, wsb):
        _lib.invoke("mk_dev_ssz_tree_hash_bytes_list", _vp(ar.ptr("elems")), n, el, _vp(ar.ptr("out")), _vp(wsp), wsb,
                    _stream(gpu), device=0)

    _run(gpu, Case(name, [("elems", arr, 256, shift)], ws, 32, call, _root_check(want, name)))


# ---- struct roots and the struct list root ---------------------------------------------------------
def _layout(layout):
    from prysm_amd import registry as R
    from tests.test_gpu_parity import _STRUCT_LAYOUTS

    return (160, [tuple(f) for f in R.VALIDATOR_FIELDS]) if layout == "validator" else _STRUCT_LAYOUTS[layout]


@functools.lru_cache(maxsize=None)
def _struct_want(layout, n):
    from oracle import oracle as O

    rec_len, spec = _layout(layout)
    return O.struct_roots(_stream_bytes(n * rec_len, SEED + 8 + rec_len), n, rec_len, spec, nthreads=NT)


@pytest.mark.parametrize("n", [1, 257, 16384])
@pytest.mark.parametrize("layout", ["validator", "fallback_u16"])
def test_struct_roots(gpu, layout, n):
    from prysm_amd import _lib
    from prysm_amd.registry import _fields

    rec_len, spec = _layout(layout)
    arr = _stream_bytes(n * rec_len, SEED + 8 + rec_len)
    f = _fields(spec)
    ws = n * _lib.load().mk_ssz_struct_msg_len(f, len(spec))  # the header: at least n * msg_len bytes
    want = _struct_want(layout, n).reshape(-1).tobytes()
    name = f"mk_dev_ssz_struct_roots({layout}, n={n})"

    def call(ar, wsp, wsb):
        _lib.invoke("mk_dev_ssz_struct_roots", _vp(ar.ptr("records")), n, rec_len, f, len(spec), _vp(ar.ptr("out")),
                    _vp(wsp), wsb, _stream(gpu), device=0)

    def check(ar, out, poison):
        assert out.tobytes() == want, name
        return out.tobytes()

    _run(gpu, Case(name, [("records", arr, 256, 0)], ws, 32 * n, call, check))


@pytest.mark.parametrize("n", [1, 257, 16384])
@pytest.mark.parametrize("layout", ["validator", "fallback_u16"])
def test_struct_list_root(gpu, layout, n):
    from oracle import oracle as O
    from prysm_amd import _lib
    from prysm_amd.registry import _fields

    rec_len, spec = _layout(layout)
    arr = _stream_bytes(n * rec_len, SEED + 8 + rec_len)
    f = _fields(spec)
    ws = _lib.load().mk_ssz_struct_list_workspace_bytes(n, f, len(spec))
    want = O.merkle_hash_flat(_struct_want(layout, n).reshape(-1), n, 32, nthreads=NT)
    name = f"mk_dev_ssz_struct_list_root({layout}, n={n})"

    def call(ar, wsp, wsb):
        _lib.invoke("mk_dev_ssz_struct_list_root", _vp(ar.ptr("records")), n, rec_len, f, len(spec),
                    _vp(ar.ptr("out")), _vp(wsp), wsb, _stream(gpu), device=0)

    _run(gpu, Case(name, [("records", arr, 256, 0)], ws, 32, call, _root_check(want, name)))


# ---- mk_merkle_root's device form ------------------------------------------------------------------
@pytest.mark.parametrize("leaves", [True, False], ids=["leaves", "no_leaves"])
@pytest.mark.parametrize("n", [1, 3, 8192])
def test_dev_merkle_root(gpu, n, leaves):
    from oracle import oracle as O
    from prysm_amd import _lib

    vlen = 40
    arr = _stream_bytes(n * vlen, SEED + 9)
    want = O.merkle_root([arr[i * vlen:(i + 1) * vlen].tobytes() for i in range(n)])
    want_leaves = O.keccak256_batch(arr, vlen, nthreads=NT).reshape(-1).tobytes()
    heap = _lib.load().mk_merkle_root_workspace_bytes(n)
    name = f"mk_dev_merkle_root(n={n}, leaves {'present' if leaves else 'absent'})"

    def call(ar, wsp, wsb):
        _lib.invoke("mk_dev_merkle_root", _vp(ar.ptr("data")), None, n, vlen, _vp(wsp), wsb,
                    _vp(ar.ptr("leaves")) if leaves else None, _vp(ar.ptr("out")), _stream(gpu), device=0)

    def check(ar, out, poison):
        lv = ar.view("leaves").cpu().numpy()
        if leaves:
            assert lv.tobytes() == want_leaves, f"{name}: leaf hashes"
        else:
            assert (lv == poison).all(), f"{name}: the absent leaves output was written"
        return _root_check(want, name)(ar, out, poison) + (lv.tobytes() if leaves else b"")

    _run(gpu, Case(name, [("data", arr, 256, 0)], heap, 32, call, check, extra=[("leaves", 32 * n, 256)]))


# ---- workspace alignment ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 8 * 4096])
def test_ws_alignment_merkle_hash(gpu, n):
    """The list-tree fast path inside mk_dev_ssz_merkle_hash wants a 16-B
    aligned workspace and silently takes the planner's passes otherwise: the
    same root by both routes (and the oracle's), the same memory contract."""
    a = _run(gpu, _merkle_case(gpu, n, 32, 0, SEED + 1))
    b = _run(gpu, _merkle_case(gpu, n, 32, 0, SEED + 1, ws_shift=8))
    assert a == b == _merkle_root_of(n, 32, SEED + 1)


@pytest.mark.parametrize("count", [3, 1025, 1 << 18])
def test_ws_alignment_top_fused(gpu, count):
    """mk_dev_ssz_merkle_top_fused documents a 16-B aligned workspace: shifted
    by 8 it is the documented MK_EINVAL before any launch (or, should a later
    version take it, the right root) -- never a wrong root."""
    import torch

    from prysm_amd import _lib

    n0 = 4 * count - 1
    ws = _lib.load().mk_ssz_merkle_top_fused_workspace_bytes(count, 0)
    ar = GuardedArena(gpu, [("nodes", 32 * count, 8, 0), ("ws", ws, 16, 8), ("out", 32, 16, 0)])
    ar.view("nodes").copy_(torch.from_numpy(_nodes(count)))
    ar.poison("ws", 0x5A)
    ar.poison("out", 0x5A)
    try:
        _lib.invoke("mk_dev_ssz_merkle_top_fused", _vp(ar.ptr("nodes")), count, n0, None, 0, 0, _vp(ar.ptr("out")), 7,
                    _vp(ar.ptr("ws")), ws, _stream(gpu), device=0)
    except _lib.MerkleError as e:
        assert e.code == _lib.MK_EINVAL and "16-B aligned" in str(e), str(e)
        torch.cuda.synchronize()
        ar.assert_poison("ws", 0x5A)
        ar.assert_poison("out", 0x5A)
    else:
        torch.cuda.synchronize()
        assert ar.view("out").cpu().numpy().tobytes() == _nodes_root(count, n0)
    ar.check_guards()
