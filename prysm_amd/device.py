"""Device-resident entry points (inputs already in HBM), torch as plumbing.

torch provides device memory, the current HIP stream and torch.distributed;
every hash is computed by the HIP kernels behind the C-ABI
(``mk_dev_*`` in include/prysm_merkle.h).  Work is enqueued on torch's
current stream of the tensor's device and is not synchronised here.  Every
call passes its device in its own ``mk_call`` context (``_lib.invoke``).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib


def _stream(dev: torch.device):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _p(t: torch.Tensor):
    return ctypes.c_void_p(t.data_ptr())


def _np(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def _dev(t: torch.Tensor) -> int:
    """Device index of a GPU tensor (passed in every call's context)."""
    if t.device.type != "cuda":
        raise _lib.MerkleError(_lib.MK_EINVAL, "device entry points need a GPU tensor")
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def synth_fill(dst: torch.Tensor, seed: int, word0: int = 0) -> torch.Tensor:
    """Fill ``dst`` (uint8, nbytes % 8 == 0) with bytes [8*word0, ...) of the
    SplitMix64 stream."""
    _lib.invoke("mk_dev_synth_fill", _p(dst), dst.numel() * dst.element_size(), seed, word0, _stream(dst.device),
                device=_dev(dst))
    return dst


def struct_roots(records: torch.Tensor, n: int, record_len: int, spec, out: torch.Tensor = None,
                 ws: torch.Tensor = None) -> torch.Tensor:
    """Struct root of each of n records (makeStructHasher per element,
    shared/ssz/hash.go:141-159; ``spec`` = [(kind, offset, len)] as in
    registry.VALIDATOR_FIELDS).  Returns an (n*32,) uint8 device tensor."""
    from .registry import _fields

    dev = _dev(records)
    if records.numel() < n * record_len:
        raise ValueError("records tensor shorter than n*record_len")
    f = _fields(spec)
    L = _lib.load()
    if out is None:
        out = torch.empty(max(32, 32 * n), dtype=torch.uint8, device=records.device)
    if ws is None:
        ws = torch.empty(max(256, n * L.mk_ssz_struct_msg_len(f, len(spec))), dtype=torch.uint8,
                         device=records.device)
    _lib.invoke("mk_dev_ssz_struct_roots", _p(records), n, record_len, f, len(spec), _p(out), _p(ws), ws.numel(),
                _stream(records.device), device=dev)
    return out


def struct_list_root(records: torch.Tensor, n: int, record_len: int, spec, out: torch.Tensor = None,
                     ws: torch.Tensor = None) -> torch.Tensor:
    """TreeHash of a list of n flat records (struct roots + merkleHash)."""
    from .registry import _fields

    dev = _dev(records)
    f = _fields(spec)
    if out is None:
        out = torch.empty(32, dtype=torch.uint8, device=records.device)
    if ws is None:
        ws = torch.empty(_lib.load().mk_ssz_struct_list_workspace_bytes(n, f, len(spec)), dtype=torch.uint8,
                         device=records.device)
    _lib.invoke("mk_dev_ssz_struct_list_root", _p(records), n, record_len, f, len(spec), _p(out), _p(ws), ws.numel(),
                _stream(records.device), device=dev)
    return out


def struct_list_level1_ok(records: torch.Tensor, n: int, record_len: int, spec) -> bool:
    """Whether struct_list_level1 takes these records (the ValidatorRecord
    layout at a 16-B aligned address, n >= 2^18)."""
    from .registry import _fields

    return bool(_lib.load().mk_ssz_struct_list_level1_ok(_p(records), n, record_len, _fields(spec), len(spec)))


def struct_list_level1(records: torch.Tensor, n: int, record_len: int, spec, roots: torch.Tensor,
                       nodes: torch.Tensor, values: torch.Tensor = None, nvalues: int = 0, value_len: int = 8,
                       value_nodes: torch.Tensor = None) -> torch.Tensor:
    """The list root's first tree level in the struct-roots launch: the n
    struct roots into ``roots`` and the ceil(n/8) level-1 nodes of their
    merkleHash into ``nodes`` (finish with merkle_finish_nodes(nodes,
    ceil(n/8), n)); with ``values`` also the ceil(nvalues * value_len / 256)
    level-1 nodes of a second list's merkleHash into ``value_nodes``."""
    from .registry import _fields

    if roots.numel() < 32 * n or nodes.numel() < 32 * -(-n // 8):
        raise ValueError("roots / nodes buffers too small")
    if nvalues and (values is None or value_nodes is None or
                    value_nodes.numel() < 32 * -(-nvalues * value_len // 256)):
        raise ValueError("second list: values / value_nodes missing or too small")
    _lib.invoke("mk_dev_ssz_struct_list_level1", _p(records), n, record_len, _fields(spec), len(spec), _p(roots),
                _p(nodes), _p(values) if nvalues else None, nvalues, value_len,
                _p(value_nodes) if nvalues else None, _stream(records.device), device=_dev(records))
    return nodes


def struct_pipe_ok(records: torch.Tensor, n: int, record_len: int, spec) -> bool:
    """Whether struct_list_level1_pipe takes these records on the current
    stream (struct_list_level1_ok with 4 groups of 1024 per workgroup)."""
    from .registry import _fields

    return bool(_lib.load().mk_ssz_struct_pipe_ok(_p(records), n, record_len, _fields(spec), len(spec),
                                                  _stream(records.device)))


def struct_pipe_levels_bytes(n: int, nvalues: int = 0, value_len: int = 8, which: int = 0) -> int:
    """Bytes of one tree's slot-levels buffer (which 0: the registry of n
    records, 1: the second list of nvalues x value_len)."""
    return int(_lib.load().mk_ssz_struct_pipe_levels_bytes(n, nvalues, value_len, which))


def struct_pipe_top_workspace(n: int, device, nvalues: int = 0, value_len: int = 8, which: int = 0) -> torch.Tensor:
    nb = int(_lib.load().mk_ssz_struct_pipe_top_workspace_bytes(n, nvalues, value_len, which))
    return torch.empty(max(256, nb), dtype=torch.uint8, device=device)


def struct_list_level1_pipe(records: torch.Tensor, n: int, record_len: int, spec, roots: torch.Tensor,
                            nodes: torch.Tensor, prev_nodes, prev_levels, values: torch.Tensor = None,
                            nvalues: int = 0, value_len: int = 8, value_nodes: torch.Tensor = None,
                            prev_value_nodes=None, prev_value_levels=None) -> torch.Tensor:
    """struct_list_level1, and in the same launch levels 2..10 of the
    PREVIOUS state's registry tree (its level-1 ``prev_nodes``; None for the
    first state) into ``prev_levels`` and levels 2..4 of its second list's
    tree (``prev_value_nodes``) into ``prev_value_levels``."""
    from .registry import _fields

    if roots.numel() < 32 * n or nodes.numel() < 32 * -(-n // 8):
        raise ValueError("roots / nodes buffers too small")
    if prev_nodes is not None and (prev_nodes.numel() < 32 * -(-n // 8) or prev_levels is None or
                                   prev_levels.numel() < struct_pipe_levels_bytes(n)):
        raise ValueError("previous state's nodes / levels buffers too small")
    if nvalues and (values is None or value_nodes is None or
                    value_nodes.numel() < 32 * -(-nvalues * value_len // 256)):
        raise ValueError("second list: values / value_nodes missing or too small")
    if prev_value_nodes is not None and (
            prev_value_levels is None or
            prev_value_levels.numel() < struct_pipe_levels_bytes(n, nvalues, value_len, 1)):
        raise ValueError("previous state's second-list levels buffer too small")
    vp = lambda t: _p(t) if t is not None else None  # noqa: E731
    _lib.invoke("mk_dev_ssz_struct_list_level1_pipe", _p(records), n, record_len, _fields(spec), len(spec),
                _p(roots), _p(nodes), vp(values) if nvalues else None, nvalues, value_len,
                vp(value_nodes) if nvalues else None, vp(prev_nodes), vp(prev_levels) if prev_nodes is not None else None,
                vp(prev_value_nodes), vp(prev_value_levels) if prev_value_nodes is not None else None,
                _stream(records.device), device=_dev(records))
    return nodes


def struct_pipe_top(nodes: torch.Tensor, n: int, levels: torch.Tensor, pair_block: torch.Tensor, slot: int,
                    epoch: int, ws: torch.Tensor, nvalues: int = 0, value_len: int = 8, which: int = 0) -> None:
    """One tree's root of a state whose slot levels the next pipelined launch
    built (which 0: the registry, 1: the second list), into slot ``slot`` of a
    pair block (merkle_finish_nodes_pair semantics)."""
    if pair_block.numel() < 128:
        raise ValueError("pair block of 128 bytes")
    _lib.invoke("mk_dev_ssz_struct_pipe_top", _p(nodes), n, nvalues, value_len, which, _p(levels), _p(pair_block),
                slot, epoch, _p(ws), ws.numel(), _stream(nodes.device), device=_dev(nodes))


def merkle_workspace(n: int, item_len: int, device) -> torch.Tensor:
    nbytes = _lib.load().mk_ssz_merkle_workspace_bytes(n, item_len)
    return torch.empty(max(256, nbytes), dtype=torch.uint8, device=device)


def merkle_hash(items: torch.Tensor, n: int, item_len: int, out: torch.Tensor = None,
                ws: torch.Tensor = None) -> torch.Tensor:
    """ssz.merkleHash of n items of item_len bytes held in ``items`` (uint8,
    device).  Returns a (32,) uint8 device tensor."""
    dev = _dev(items)
    if items.numel() < n * item_len:
        raise ValueError("items tensor shorter than n*item_len")
    if out is None:
        out = torch.empty(32, dtype=torch.uint8, device=items.device)
    if ws is None:
        ws = merkle_workspace(n, item_len, items.device)
    _lib.invoke("mk_dev_ssz_merkle_hash", _p(items), n, item_len, _p(out), _p(ws), ws.numel(), _stream(items.device),
                device=dev)
    return out


def tree_hash_bytes_list_workspace(n: int, elem_len: int, device, aligned16: bool = True) -> torch.Tensor:
    """Workspace of mk_dev_ssz_tree_hash_bytes_list.  The library's query
    plans for 16-B aligned elements; elements at another address take the
    two-phase form (element digests in the workspace first), which needs
    n x 32 more bytes (rounded to 256)."""
    nb = _lib.load().mk_ssz_tree_hash_bytes_list_workspace_bytes(n, elem_len)
    if not aligned16:
        nb += -(-n * 32 // 256) * 256
    return torch.empty(max(nb, 256), dtype=torch.uint8, device=device)


def tree_hash_bytes_list(elems: torch.Tensor, n: int, elem_len: int, out: torch.Tensor = None,
                         ws: torch.Tensor = None) -> torch.Tensor:
    """ssz.TreeHash of a list of n byte strings of elem_len bytes each
    (makeSliceHasher + hashedEncoding, shared/ssz/hash.go:100-107, 118-139):
    merkleHash over K(le32(elem_len) || element_i), in one call with the
    element digests fused into the leaf pass (32-B elements)."""
    if out is None:
        out = torch.empty(32, dtype=torch.uint8, device=elems.device)
    if ws is None:
        ws = tree_hash_bytes_list_workspace(n, elem_len, elems.device, aligned16=elems.data_ptr() % 16 == 0)
    _lib.invoke("mk_dev_ssz_tree_hash_bytes_list", _p(elems), n, elem_len, _p(out), _p(ws), ws.numel(),
                _stream(elems.device), device=_dev(elems))
    return out


def merkle_many(items: torch.Tensor, offs, ns, item_lens, out: torch.Tensor = None,
                ws: torch.Tensor = None) -> torch.Tensor:
    """merkleHash of many lists in one call (list i = ns[i] items of
    item_lens[i] bytes at byte offset offs[i] of ``items``): an (nlists*32,)
    uint8 device tensor of roots."""
    dev = _dev(items)
    k = len(ns)
    o = np.ascontiguousarray(offs, dtype=np.uint64)
    n = np.ascontiguousarray(ns, dtype=np.uint64)
    il = np.ascontiguousarray(item_lens, dtype=np.uint32)
    if out is None:
        out = torch.empty(max(32, 32 * k), dtype=torch.uint8, device=items.device)
    if ws is None:
        ws = torch.empty(max(256, many_workspace_bytes(n, il)), dtype=torch.uint8, device=items.device)
    _lib.invoke("mk_dev_ssz_merkle_many", _p(items), _np(o), _np(n), _np(il), k, _p(out), _p(ws), ws.numel(),
                _stream(items.device), device=dev)
    return out[:32 * k]


def many_workspace_bytes(ns, item_lens) -> int:
    n = np.ascontiguousarray(ns, dtype=np.uint64)
    il = np.ascontiguousarray(item_lens, dtype=np.uint32)
    return _lib.load().mk_ssz_merkle_many_workspace_bytes(_np(n), _np(il), len(n))


def shard_plan(n: int, item_len: int, nshards: int):
    """(height, nonempty, item_begin[nshards+1]) of the subtree sharding."""
    h = ctypes.c_uint32()
    ne = ctypes.c_uint32()
    begin = (ctypes.c_uint64 * (nshards + 1))()
    _lib.invoke("mk_ssz_merkle_shard_plan", n, item_len, nshards, ctypes.byref(h), ctypes.byref(ne), begin)
    return h.value, ne.value, list(begin)


def subtree_workspace(shard_n: int, item_len: int, device) -> torch.Tensor:
    # the header's rule: the merkleHash query of the shard's own items bounds every subtree and
    # frontier plan over them (held by tests/c_abi/planner_fuzz.cpp), and the entries refuse less
    nbytes = _lib.load().mk_ssz_merkle_workspace_bytes(max(shard_n, 1), item_len)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def merkle_subtree(items: torch.Tensor, shard_n: int, item_len: int, height: int, pad_at_one: bool,
                   out: torch.Tensor = None, ws: torch.Tensor = None) -> torch.Tensor:
    """32-B root of one shard at `height` levels above its chunks."""
    dev = _dev(items)
    if out is None:
        out = torch.empty(32, dtype=torch.uint8, device=items.device)
    if ws is None:
        ws = subtree_workspace(shard_n, item_len, items.device)
    _lib.invoke("mk_dev_ssz_merkle_subtree", _p(items), shard_n, item_len, height, int(pad_at_one), _p(out), _p(ws),
                ws.numel(), _stream(items.device), device=dev)
    return out


def merkle_subtree_frontier(items: torch.Tensor, shard_n: int, item_len: int, height: int, frontier_log2: int,
                            pad_at_one: bool, out: torch.Tensor = None, ws: torch.Tensor = None) -> torch.Tensor:
    """The shard's tree level `frontier_log2` levels below its root: a
    (nodes*32,) uint8 device tensor (nodes = parallel.frontier_count(...))."""
    from .parallel import frontier_count

    dev = _dev(items)
    nodes = frontier_count(shard_n, item_len, height, frontier_log2)
    if out is None:
        out = torch.empty(32 << frontier_log2, dtype=torch.uint8, device=items.device)
    if out.numel() < 32 * nodes:
        raise ValueError("frontier output buffer too small")
    if ws is None:
        ws = subtree_workspace(shard_n, item_len, items.device)
    got = ctypes.c_uint64()
    _lib.invoke("mk_dev_ssz_merkle_subtree_frontier", _p(items), shard_n, item_len, height, frontier_log2,
                int(pad_at_one), _p(out), ctypes.byref(got), _p(ws), ws.numel(), _stream(items.device), device=dev)
    assert got.value == nodes, (got.value, nodes)
    return out[:32 * nodes]


def merkle_node_frontier(nodes: torch.Tensor, count: int, height: int, frontier_log2: int, pad_at_one: bool,
                         out: torch.Tensor = None, ws: torch.Tensor = None) -> torch.Tensor:
    """A subtree continued from one of its node levels: `count` 32-B nodes
    reduced `height` levels (odd rule, hash.go:225-235), stopping
    `frontier_log2` levels below the top; returns the (nodes*32,) level."""
    dev = _dev(nodes)
    lib = _lib.load()
    want = max(1, -(-count // (1 << (height - frontier_log2)))) if frontier_log2 else 1
    if out is None:
        out = torch.empty(32 << frontier_log2, dtype=torch.uint8, device=nodes.device)
    if out.numel() < 32 * want:
        raise ValueError("node frontier output buffer too small")
    if ws is None:
        ws = torch.empty(max(256, lib.mk_ssz_merkle_node_frontier_workspace_bytes(count, height, frontier_log2)),
                         dtype=torch.uint8, device=nodes.device)
    got = ctypes.c_uint64()
    _lib.invoke("mk_dev_ssz_merkle_node_frontier", _p(nodes), count, height, frontier_log2, int(pad_at_one), _p(out),
                ctypes.byref(got), _p(ws), ws.numel(), _stream(nodes.device), device=dev)
    assert got.value == want, (got.value, want)
    return out[:32 * want]


def finish_workspace(count: int, device) -> torch.Tensor:
    return torch.empty(max(256, _lib.load().mk_ssz_merkle_finish_workspace_bytes(count)), dtype=torch.uint8,
                       device=device)


def merkle_finish_nodes_pair(nodes: torch.Tensor, count: int, n_total: int, pair_block: torch.Tensor, slot: int,
                             epoch: int, ws: torch.Tensor = None) -> None:
    """merkle_finish_nodes for one list field of a two-field struct: the list
    root goes to pair_block[32 slot:32 slot + 32]; whichever of the pair's two
    finishers (slot 0 and 1, the same ``epoch``, any streams) completes
    second writes the struct root Keccak(pair_block[0:64]) to
    pair_block[64:96].  ``pair_block``: 128 bytes, zeroed before its first
    use; ``epoch``: 1 .. 2^30 - 1, a new one per pair."""
    dev = _dev(nodes)
    if pair_block.numel() < 128:
        raise ValueError("pair block of 128 bytes")
    if ws is None:
        ws = finish_workspace(count, nodes.device)
    _lib.invoke("mk_dev_ssz_merkle_finish_nodes_pair", _p(nodes), count, n_total, _p(pair_block), slot, epoch, _p(ws),
                ws.numel(), _stream(nodes.device), device=dev)


def top_fused_workspace(count0: int, count1: int, device) -> torch.Tensor:
    nb = _lib.load().mk_ssz_merkle_top_fused_workspace_bytes(count0, count1)
    if nb == 0:
        raise ValueError(f"fused top: bad counts {count0}, {count1}")
    return torch.empty(nb, dtype=torch.uint8, device=device)


def merkle_top_fused(nodes0: torch.Tensor, count0: int, n0: int, out: torch.Tensor, nodes1: torch.Tensor = None,
                     count1: int = 0, n1: int = 0, epoch: int = 0, ws: torch.Tensor = None) -> torch.Tensor:
    """The level loop + length mix-in of one list (count1 == 0: ``out`` gets
    the 32-B root) or of two lists side by side (``out`` a 128-B pair block,
    merkle_finish_nodes_pair semantics: the struct root at out[64:96],
    ``epoch`` 1 .. 2^30 - 1 a new one per pair), from a complete node level of
    each, in one launch (mk_dev_ssz_merkle_top_fused)."""
    dev = _dev(nodes0)
    if count1 and out.numel() < 128:
        raise ValueError("pair block of 128 bytes")
    if ws is None:
        ws = top_fused_workspace(count0, count1, nodes0.device)
    _lib.invoke("mk_dev_ssz_merkle_top_fused", _p(nodes0), count0, n0, _p(nodes1) if nodes1 is not None else None,
                count1, n1, _p(out), epoch, _p(ws), ws.numel(), _stream(nodes0.device), device=dev)
    return out


def merkle_finish_nodes(nodes: torch.Tensor, count: int, n_total: int, out: torch.Tensor = None,
                        ws: torch.Tensor = None) -> torch.Tensor:
    """Reference level loop over one gathered tree level of `count` nodes +
    length mix-in (the finisher of the frontier sharding)."""
    dev = _dev(nodes)
    if out is None:
        out = torch.empty(32, dtype=torch.uint8, device=nodes.device)
    if ws is None:
        ws = finish_workspace(count, nodes.device)
    _lib.invoke("mk_dev_ssz_merkle_finish_nodes", _p(nodes), count, n_total, _p(out), _p(ws), ws.numel(),
                _stream(nodes.device), device=dev)
    return out


def merkle_finish(roots: torch.Tensor, nroots: int, n_total: int, out: torch.Tensor = None) -> torch.Tensor:
    """Reference level loop over gathered shard roots + length mix-in."""
    dev = _dev(roots)
    if out is None:
        out = torch.empty(32, dtype=torch.uint8, device=roots.device)
    _lib.invoke("mk_dev_ssz_merkle_finish", _p(roots), nroots, n_total, _p(out), _stream(roots.device), device=dev)
    return out


def merkle_hash_multi(shards, n: int, item_len: int, out: torch.Tensor, streams=None) -> torch.Tensor:
    """Single-process multi-device merkleHash (the cgo caller's form):
    shards[d] on device d holds shard d of shard_plan(n, item_len,
    len(shards)); RCCL all-gather of the frontiers, device 0 finishes into
    ``out`` (a (32,) tensor on device 0)."""
    k = len(shards)
    ptrs = (ctypes.c_void_p * k)(*[s.data_ptr() for s in shards])
    sts = (ctypes.c_void_p * k)(*[(streams[d] if streams else torch.cuda.current_stream(shards[d].device)).cuda_stream
                                  for d in range(k)])
    _lib.invoke("mk_dev_ssz_merkle_hash_multi", ptrs, n, item_len, k, _p(out), sts, device=0)
    return out


def hash_batch(msgs: torch.Tensor, n: int, msg_len: int, out: torch.Tensor = None) -> torch.Tensor:
    """Batched Hash of n fixed-length messages resident on the device."""
    dev = _dev(msgs)
    if out is None:
        out = torch.empty(n * 32, dtype=torch.uint8, device=msgs.device)
    _lib.invoke("mk_dev_hash_batch", _p(msgs), n, msg_len, _p(out), _stream(msgs.device), device=dev)
    return out


def _nbytes(t: torch.Tensor) -> int:
    return t.numel() * t.element_size()


def _same_dev(dev: int, **tensors) -> None:
    """Every tensor given (None: absent) lies on GPU ``dev``: a kernel must not be handed a pointer of
    another device or of the host."""
    for name, t in tensors.items():
        if t is not None and _dev(t) != dev:
            raise ValueError(f"{name} is on {t.device}, not on cuda:{dev}")


def repeat_hash(seeds: torch.Tensor, layers: torch.Tensor, n: int, max_layers: int,
                form: int = _lib.MK_REPEAT_AUTO, out: torch.Tensor = None, status: torch.Tensor = None):
    """``out[i] = RepeatHash(seeds[i], layers[i])`` for n chains resident on the
    device (hashutil.RepeatHash, hash.go:29-34): ``seeds`` n x 32
    bytes, ``layers`` n 32-bit counts.  Returns ``(out, status)``: the host
    cannot see the counts, so a chain whose count exceeds ``max_layers`` gets 32
    zero bytes and sets the one-word ``status`` tensor (int32) to 1.  A
    ``status`` passed in is only ever set, never cleared: clear it once, check
    it after any number of calls; without one the call makes a zeroed word."""
    dev = _dev(seeds)
    _same_dev(dev, layers=layers, out=out, status=status)
    if _nbytes(seeds) < 32 * n:
        raise ValueError("seeds shorter than n x 32 bytes")
    if layers.element_size() != 4 or layers.numel() < n:
        raise ValueError("layers: at least n 32-bit integers")
    if out is None:
        out = torch.empty(n * 32, dtype=torch.uint8, device=seeds.device)
    elif _nbytes(out) < 32 * n:
        raise ValueError("out shorter than n x 32 bytes")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=seeds.device)
    elif status.element_size() != 4 or status.numel() < 1:
        raise ValueError("status: one 32-bit word")
    _lib.invoke("mk_dev_repeat_hash", _p(seeds), _p(layers), n, max_layers, form, _p(out), _p(status),
                _stream(seeds.device), device=dev)
    return out, status


def hash_onion(seeds: torch.Tensor, n: int, layers: int, form: int = _lib.MK_REPEAT_AUTO,
               out: torch.Tensor = None) -> torch.Tensor:
    """The hash onions of n seeds resident on the device, every layer kept:
    n x (layers + 1) x 32 bytes, ``out[i][t] = RepeatHash(seeds[i], t)``, row 0
    the seed (mk_dev_hash_onion)."""
    dev = _dev(seeds)
    _same_dev(dev, out=out)
    if _nbytes(seeds) < 32 * n:
        raise ValueError("seeds shorter than n x 32 bytes")
    if layers < 0:
        raise ValueError("layers < 0")
    if out is None:
        out = torch.empty(n * (layers + 1) * 32, dtype=torch.uint8, device=seeds.device)
    elif _nbytes(out) < n * (layers + 1) * 32:
        raise ValueError("out shorter than n x (layers + 1) x 32 bytes")
    _lib.invoke("mk_dev_hash_onion", _p(seeds), n, layers, form, _p(out), _stream(seeds.device), device=dev)
    return out


def verify_repeat_hash(records: torch.Tensor, n_records: int, stride: int, commit_off: int, layers_off: int,
                       indices: torch.Tensor, reveals: torch.Tensor, m: int, max_layers: int,
                       form: int = _lib.MK_REPEAT_AUTO, out: torch.Tensor = None) -> torch.Tensor:
    """verifyBlockRandao (block_operations.go:109-123) for m proposals against
    records resident on the device: (m,) uint8, ``MK_REPEAT_OK`` where
    ``RepeatHash(reveals[j], le64(rec + layers_off)) == rec[commit_off:+32]``,
    rec = record ``indices[j]``; ``MK_REPEAT_BAD`` where not; ``MK_REPEAT_TOO_DEEP``
    where the record's 64-bit layer count exceeds ``max_layers`` (the chain is
    not run); ``MK_REPEAT_NO_RECORD`` where ``indices[j] >= n_records``."""
    dev = _dev(reveals)
    _same_dev(dev, records=records, indices=indices, out=out)
    if _nbytes(records) < n_records * stride:
        raise ValueError("records shorter than n_records x stride bytes")
    if indices.element_size() != 8 or indices.numel() < m:
        raise ValueError("indices: at least m 64-bit integers")
    if _nbytes(reveals) < 32 * m:
        raise ValueError("reveals shorter than m x 32 bytes")
    if out is None:
        out = torch.empty(m, dtype=torch.uint8, device=reveals.device)
    elif _nbytes(out) < m:
        raise ValueError("out shorter than m bytes")
    _lib.invoke("mk_dev_verify_repeat_hash", _p(records), n_records, stride, commit_off, layers_off, _p(indices),
                _p(reveals), m, max_layers, form, _p(out), _stream(reveals.device), device=dev)
    return out


def deposit_trie_levels_bytes(capacity: int, depth: int) -> int:
    return _lib.load().mk_deposit_trie_levels_bytes(capacity, depth)


def deposit_trie_append(levels: torch.Tensor, capacity: int, count: int, data: torch.Tensor, k: int,
                        fixed_len: int, depth: int, root: torch.Tensor, offs: torch.Tensor = None) -> None:
    """Append k deposits (fixed_len-byte records in ``data``, or variable
    length with device ``offs``) to the device trie holding ``count``
    deposits: UpdateDepositTrie (deposit_trie.go:29-40) batched, right edge
    of every level only; count == 0 is the batch build."""
    dev = _dev(levels)
    if offs is None and data.numel() < k * fixed_len:
        raise ValueError(f"deposit buffer holds {data.numel()} bytes < {k} x {fixed_len}")
    if levels.numel() < deposit_trie_levels_bytes(capacity, depth):
        raise ValueError("level buffer smaller than mk_deposit_trie_levels_bytes(capacity, depth)")
    _lib.invoke("mk_dev_deposit_trie_append", _p(levels), capacity, count, _p(data),
                _p(offs) if offs is not None else None, k, fixed_len, depth, _p(root), _stream(levels.device),
                device=dev)


def deposit_trie_build(levels: torch.Tensor, capacity: int, data: torch.Tensor, n: int, deposit_len: int,
                       d_to: int, depth: int, root: torch.Tensor = None) -> torch.Tensor:
    """Batch build front (deposit_trie.go:29-40): Hash of n fixed-length
    deposits into level 0 of an empty trie and levels 1..d_to (the root too
    when d_to == depth).  Returns ``levels``."""
    dev = _dev(levels)
    if n > capacity or levels.numel() < deposit_trie_levels_bytes(capacity, depth):
        raise ValueError("level array smaller than the capacity layout")
    if data.numel() * data.element_size() < n * deposit_len:
        raise ValueError("deposit buffer shorter than n * deposit_len")
    if d_to == depth and root is None:
        root = torch.empty(32, dtype=torch.uint8, device=levels.device)
    _lib.invoke("mk_dev_deposit_trie_build", _p(levels), capacity, _p(data), None, n, deposit_len, d_to, depth,
                _p(root) if root is not None else None, _stream(levels.device), device=dev)
    return levels


def deposit_trie_pipe_ok(data: torch.Tensor, n: int, deposit_len: int, depth: int) -> bool:
    """Whether deposit_trie_build_pipe takes this stream shape."""
    return bool(_lib.load().mk_deposit_trie_pipe_ok(_p(data), n, deposit_len, depth, _stream(data.device)))


def deposit_trie_build_pipe(levels: torch.Tensor, prev_levels, capacity: int, data: torch.Tensor, n: int,
                            deposit_len: int, depth: int) -> None:
    """Levels 0..2 of this trie and levels 3..7 of the previous trie of the
    stream (``prev_levels``, None for the first) in one launch
    (mk_dev_deposit_trie_build_pipe)."""
    _lib.invoke("mk_dev_deposit_trie_build_pipe", _p(levels), None if prev_levels is None else _p(prev_levels),
                capacity, _p(data), n, deposit_len, depth, _stream(levels.device), device=_dev(levels))


def deposit_trie_pipe_top(levels: torch.Tensor, capacity: int, count: int, depth: int, root: torch.Tensor) -> None:
    """Levels 8 .. depth and the root of a pipelined front's previous trie,
    in launches that fit beside the next front (mk_dev_deposit_trie_pipe_top)."""
    _lib.invoke("mk_dev_deposit_trie_pipe_top", _p(levels), capacity, count, depth, _p(root), _stream(levels.device),
                device=_dev(levels))


def deposit_trie_levels(levels: torch.Tensor, capacity: int, count: int, d_from: int, d_to: int, depth: int,
                        root: torch.Tensor = None) -> None:
    """Levels d_from+1 .. d_to of the batch build (level d_from complete);
    the root to ``root`` when d_to == depth."""
    dev = _dev(levels)
    _lib.invoke("mk_dev_deposit_trie_levels", _p(levels), capacity, count, d_from, d_to, depth,
                _p(root) if root is not None else None, _stream(levels.device), device=dev)


def deposit_trie_branch(levels: torch.Tensor, capacity: int, count: int, depth: int, index: int,
                        out: torch.Tensor = None) -> torch.Tensor:
    """GenerateMerkleBranch(index) of a device trie: (depth*32,) uint8."""
    dev = _dev(levels)
    if out is None:
        out = torch.empty(32 * depth, dtype=torch.uint8, device=levels.device)
    _lib.invoke("mk_dev_deposit_trie_branch", _p(levels), capacity, count, depth, index, _p(out),
                _stream(levels.device), device=dev)
    return out


def deposit_trie_branches(levels: torch.Tensor, capacity: int, count: int, depth: int, as_of: int,
                          indices: torch.Tensor, k: int = None, out: torch.Tensor = None,
                          root_at: torch.Tensor = None) -> torch.Tensor:
    """GenerateMerkleBranch for the k device ``indices`` (int64 / uint64, any
    order) as of ``as_of`` <= count deposits, one launch: (k*depth*32,) uint8;
    the root of that moment to ``root_at`` (32 B) when given
    (mk_dev_deposit_trie_branches).  Nothing is read on the host, so a captured
    call follows the indices tensor's contents at replay."""
    dev = _dev(levels)
    if k is None:
        k = indices.numel()
    if indices.element_size() != 8 or indices.numel() < k:
        raise ValueError("indices: at least k 64-bit integers")
    if out is None:
        out = torch.empty(32 * depth * k, dtype=torch.uint8, device=levels.device)
    elif out.numel() * out.element_size() < 32 * depth * k:
        raise ValueError("branch buffer smaller than k x depth x 32 bytes")
    _lib.invoke("mk_dev_deposit_trie_branches", _p(levels), capacity, count, depth, as_of, _p(indices), k, _p(out),
                _p(root_at) if root_at is not None else None, _stream(levels.device), device=dev)
    return out


def _trie_fits(levels: torch.Tensor, capacity: int, depth: int) -> None:
    if capacity and 0 < depth < 64 and levels.numel() * levels.element_size() < deposit_trie_levels_bytes(capacity, depth):
        raise ValueError("level buffer smaller than mk_deposit_trie_levels_bytes(capacity, depth)")


def deposit_trie_truncate(levels: torch.Tensor, capacity: int, count: int, new_count: int, depth: int,
                          root: torch.Tensor) -> None:
    """Roll the device trie of ``count`` deposits back to its first
    ``new_count``: one single-wave launch stores the at most ``depth`` nodes
    that straddle ``new_count`` and the root; nothing else of ``levels`` is
    written (mk_dev_deposit_trie_truncate)."""
    _trie_fits(levels, capacity, depth)
    _lib.invoke("mk_dev_deposit_trie_truncate", _p(levels), capacity, count, new_count, depth, _p(root),
                _stream(levels.device), device=_dev(levels))


def deposit_trie_fork_point(levels_a: torch.Tensor, capacity_a: int, count_a: int, levels_b: torch.Tensor,
                            capacity_b: int, count_b: int, depth: int, out: torch.Tensor = None) -> torch.Tensor:
    """The smallest leaf index below min(count_a, count_b) at which two device
    tries of one depth differ, that minimum when none does: one int64 on the
    device (mk_dev_deposit_trie_fork_point)."""
    _trie_fits(levels_a, capacity_a, depth)
    _trie_fits(levels_b, capacity_b, depth)
    if out is None:
        out = torch.empty(1, dtype=torch.int64, device=levels_a.device)
    elif out.numel() * out.element_size() < 8:
        raise ValueError("out shorter than 8 bytes")
    _lib.invoke("mk_dev_deposit_trie_fork_point", _p(levels_a), capacity_a, count_a, _p(levels_b), capacity_b,
                count_b, depth, _p(out), _stream(levels_a.device), device=_dev(levels_a))
    return out


def deposit_trie_audit(levels: torch.Tensor, capacity: int, count: int, depth: int, root: torch.Tensor,
                       report: torch.Tensor = None) -> torch.Tensor:
    """Every stored node of level 1 .. depth of a device trie against the
    level below it, and ``root`` against the top node, read-only
    (mk_dev_deposit_trie_audit).  Returns ``report``, 24 bytes on the device:
    one mk_audit_report; ``audit_reports`` turns it into a tuple."""
    _trie_fits(levels, capacity, depth)
    if report is None:
        report = torch.empty(24, dtype=torch.uint8, device=levels.device)
    elif report.numel() * report.element_size() < 24:
        raise ValueError("report shorter than 24 bytes")
    _lib.invoke("mk_dev_deposit_trie_audit", _p(levels), capacity, count, depth, _p(root), _p(report),
                _stream(levels.device), device=_dev(levels))
    return report


def deposit_trie_copy(src_levels: torch.Tensor, src_capacity: int, count: int, dst_levels: torch.Tensor,
                      dst_capacity: int, depth: int, src_root: torch.Tensor = None,
                      dst_root: torch.Tensor = None) -> None:
    """The live nodes of a device trie from the layout of ``src_capacity``
    into that of ``dst_capacity`` >= count, and the root when both root
    tensors are given: one launch, no hashing (mk_dev_deposit_trie_copy)."""
    _trie_fits(src_levels, src_capacity, depth)
    _trie_fits(dst_levels, dst_capacity, depth)
    _lib.invoke("mk_dev_deposit_trie_copy", _p(src_levels), src_capacity, count, _p(dst_levels), dst_capacity, depth,
                _p(src_root) if src_root is not None else None, _p(dst_root) if dst_root is not None else None,
                _stream(src_levels.device), device=_dev(src_levels))


def verify_deposits(data: torch.Tensor, offs: torch.Tensor, branches: torch.Tensor, indices: torch.Tensor, n: int,
                    depth: int, roots: torch.Tensor, root_stride: int = 0, tree_depth: int = 32,
                    out: torch.Tensor = None) -> torch.Tensor:
    """verifyDeposit for n deposits resident on the device (deposit i =
    data[offs[i], offs[i+1]), ``offs`` n + 1 64-bit offsets): (n,) uint8, 1
    where Hash(deposit) folds through its branch to the root -- ``roots``'
    first 32 bytes for all of them (root_stride 0) or root i (root_stride 32)
    (mk_dev_verify_deposits)."""
    dev = _dev(branches)
    if offs.element_size() != 8 or offs.numel() < n + 1 or indices.element_size() != 8 or indices.numel() < n:
        raise ValueError("offs: n + 1 and indices: n 64-bit integers")
    if branches.numel() * branches.element_size() < 32 * depth * n:
        raise ValueError("branch buffer smaller than n x depth x 32 bytes")
    if roots.numel() * roots.element_size() < (32 * n if root_stride else 32):
        raise ValueError("root buffer too small")
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=branches.device)
    _lib.invoke("mk_dev_verify_deposits", _p(data), _p(offs), _p(branches), _p(indices), n, depth, tree_depth,
                _p(roots), root_stride, _p(out), _stream(branches.device), device=dev)
    return out


def list_tree_levels_bytes(capacity: int, item_len: int) -> int:
    """Bytes of the level array of a list tree with room for ``capacity`` items."""
    return _lib.load().mk_ssz_list_tree_levels_bytes(capacity, item_len)


def list_tree_update_workspace_bytes(k: int) -> int:
    """Workspace of list_tree_update for k = changed + appended items."""
    return _lib.load().mk_ssz_list_tree_update_workspace_bytes(k)


def list_tree_build(items: torch.Tensor, n: int, capacity: int, item_len: int, levels: torch.Tensor,
                    root: torch.Tensor = None, ws: torch.Tensor = None) -> torch.Tensor:
    """Every level (into ``levels``) and the root of merkleHash over the n
    items in ``items`` (hash.go:194-239), laid out for ``capacity`` items.
    Returns the (32,) uint8 root tensor."""
    dev = _dev(items)
    if items.numel() * items.element_size() < n * item_len:
        raise ValueError("item buffer shorter than n * item_len")
    if levels.numel() < list_tree_levels_bytes(capacity, item_len):
        raise ValueError("level buffer smaller than mk_ssz_list_tree_levels_bytes(capacity, item_len)")
    if root is None:
        root = torch.empty(32, dtype=torch.uint8, device=items.device)
    if ws is None:
        ws = torch.empty(_lib.load().mk_ssz_list_tree_build_workspace_bytes(n, item_len), dtype=torch.uint8,
                         device=items.device)
    _lib.invoke("mk_dev_ssz_list_tree_build", _p(items), n, capacity, item_len, _p(levels), _p(root), _p(ws),
                ws.numel(), _stream(items.device), device=dev)
    return root


def list_tree_update(items: torch.Tensor, n_old: int, n_new: int, capacity: int, item_len: int,
                     levels: torch.Tensor, root: torch.Tensor, idx: torch.Tensor = None, k_idx: int = 0,
                     values: torch.Tensor = None, ws: torch.Tensor = None) -> torch.Tensor:
    """Re-hash a built list tree after ``k_idx`` items changed (``idx``:
    ascending int64/uint64 device indices < n_old) and n_new - n_old were
    appended: only the ancestors of the changed chunks.  ``values`` (the k_idx
    new items, then the appended ones) are scattered into ``items`` first;
    None: ``items`` already holds the new bytes.  Returns ``root``."""
    dev = _dev(items)
    if items.numel() * items.element_size() < n_new * item_len:
        raise ValueError("item buffer shorter than n_new * item_len")
    if k_idx and (idx is None or idx.numel() < k_idx or idx.element_size() != 8):
        raise ValueError("idx: k_idx 64-bit device indices")
    k = k_idx + max(n_new - n_old, 0)
    if values is not None and values.numel() * values.element_size() < k * item_len:
        raise ValueError("values shorter than (k_idx + appended) * item_len")
    if ws is None:
        ws = torch.empty(_lib.load().mk_ssz_list_tree_update_workspace_bytes(k), dtype=torch.uint8,
                         device=items.device)
    _lib.invoke("mk_dev_ssz_list_tree_update", _p(items), n_old, n_new, capacity, item_len, _p(levels),
                _p(idx) if k_idx else None, k_idx, _p(values) if values is not None else None, _p(root), _p(ws),
                ws.numel(), _stream(items.device), device=dev)
    return root


def list_branch_bytes(n: int, item_len: int) -> int:
    """Bytes of one proof record of a list of n item_len-byte items (0: item_len 0 or above 128)."""
    return _lib.load().mk_ssz_list_branch_bytes(n, item_len)


def list_tree_branches(level0: torch.Tensor, n: int, capacity: int, item_len: int, levels: torch.Tensor,
                       indices: torch.Tensor, k: int = None, out: torch.Tensor = None) -> torch.Tensor:
    """Merkle proofs of the items at the k device ``indices`` (int64 / uint64,
    any order) of a built resident tree, one launch: (k * list_branch_bytes(n,
    item_len),) uint8 (mk_dev_ssz_list_tree_branches).
    ``level0``: the item buffer of a list tree, or the struct roots / element
    digests of the other two kinds with item_len = 32.  An index >= n gives a
    zero record.  Nothing is read on the host, so a captured call follows the
    tensors' contents at replay."""
    dev = _dev(level0)
    if k is None:
        k = indices.numel()
    if indices.element_size() != 8 or indices.numel() < k:
        raise ValueError("indices: at least k 64-bit integers")
    if level0.numel() * level0.element_size() < n * item_len:
        raise ValueError("level 0 shorter than n * item_len")
    if levels.numel() * levels.element_size() < list_tree_levels_bytes(capacity, item_len):
        raise ValueError("level buffer smaller than mk_ssz_list_tree_levels_bytes(capacity, item_len)")
    need = list_branch_bytes(n, item_len) * k
    if out is None:
        out = torch.empty(need, dtype=torch.uint8, device=level0.device)
    elif out.numel() * out.element_size() < need:
        raise ValueError("branch buffer smaller than k records")
    _lib.invoke("mk_dev_ssz_list_tree_branches", _p(level0), n, capacity, item_len, _p(levels), _p(indices), k,
                _p(out), _stream(level0.device), device=dev)
    return out


def verify_list_branches(values: torch.Tensor, indices: torch.Tensor, k: int, n: int, item_len: int,
                         branches: torch.Tensor, roots: torch.Tensor, root_stride: int = 0,
                         container: torch.Tensor = None, container_off: int = 0,
                         out: torch.Tensor = None) -> torch.Tensor:
    """Verify k list-tree proofs resident on the device: (k,) uint8, 1 where
    ``values[g]`` at index ``indices[g]`` of a list of n items folds through
    record g to the root -- ``roots``' first 32 bytes (root_stride 0) or root
    g (32).  With ``container`` (the struct's hash message) the list root is
    substituted at ``container_off`` and the message's hash is compared
    (mk_dev_verify_list_branches)."""
    dev = _dev(branches)
    if indices.element_size() != 8 or indices.numel() < k:
        raise ValueError("indices: at least k 64-bit integers")
    if values.numel() * values.element_size() < k * item_len:
        raise ValueError("values shorter than k * item_len")
    if branches.numel() * branches.element_size() < list_branch_bytes(n, item_len) * k:
        raise ValueError("branch buffer smaller than k records")
    if roots.numel() * roots.element_size() < (32 * k if root_stride else 32):
        raise ValueError("root buffer too small")
    if out is None:
        out = torch.empty(k, dtype=torch.uint8, device=branches.device)
    clen = container.numel() * container.element_size() if container is not None else 0
    _lib.invoke("mk_dev_verify_list_branches", _p(values), _p(indices), k, n, item_len, _p(branches), _p(roots),
                root_stride, _p(container) if container is not None else None, clen, container_off, _p(out),
                _stream(branches.device), device=dev)
    return out


def struct_list_tree_build_workspace_bytes(n: int, spec) -> int:
    from .registry import _fields

    return _lib.load().mk_ssz_struct_list_tree_build_workspace_bytes(n, _fields(spec), len(spec))


def struct_list_tree_update_workspace_bytes(k: int, spec) -> int:
    """Workspace of struct_list_tree_update for k = changed + appended records."""
    from .registry import _fields

    return _lib.load().mk_ssz_struct_list_tree_update_workspace_bytes(k, _fields(spec), len(spec))


def struct_list_tree_build(records: torch.Tensor, n: int, capacity: int, record_len: int, spec,
                           roots: torch.Tensor, levels: torch.Tensor, root: torch.Tensor = None,
                           ws: torch.Tensor = None) -> torch.Tensor:
    """Every struct root (into ``roots``, capacity x 32 B), every level (into
    ``levels``, the layout of ``list_tree_levels_bytes(capacity, 32)``) and the
    root of TreeHash over the n records in ``records`` (hash.go:118-159,
    194-239).  Returns the (32,) uint8 root tensor."""
    from .registry import _fields

    dev = _dev(records)
    if records.numel() * records.element_size() < n * record_len:
        raise ValueError("record buffer shorter than n * record_len")
    if roots.numel() < 32 * capacity:
        raise ValueError("roots buffer shorter than 32 * capacity")
    if levels.numel() < list_tree_levels_bytes(capacity, 32):
        raise ValueError("level buffer smaller than mk_ssz_list_tree_levels_bytes(capacity, 32)")
    if root is None:
        root = torch.empty(32, dtype=torch.uint8, device=records.device)
    if ws is None:
        ws = torch.empty(struct_list_tree_build_workspace_bytes(n, spec), dtype=torch.uint8, device=records.device)
    _lib.invoke("mk_dev_ssz_struct_list_tree_build", _p(records), n, capacity, record_len, _fields(spec), len(spec),
                _p(roots), _p(levels), _p(root), _p(ws), ws.numel(), _stream(records.device), device=dev)
    return root


def struct_list_tree_update(records: torch.Tensor, n_old: int, n_new: int, capacity: int, record_len: int, spec,
                            roots: torch.Tensor, levels: torch.Tensor, root: torch.Tensor,
                            idx: torch.Tensor = None, k_idx: int = 0, values: torch.Tensor = None,
                            ws: torch.Tensor = None) -> torch.Tensor:
    """Re-hash a built registry tree after ``k_idx`` records changed (``idx``:
    ascending int64/uint64 device indices < n_old) and n_new - n_old were
    appended: those records' struct roots and their ancestors only.
    ``values`` (the k_idx new records, then the appended ones) are scattered
    into ``records`` first; None: ``records`` already holds them.  Returns
    ``root``."""
    from .registry import _fields

    dev = _dev(records)
    if records.numel() * records.element_size() < n_new * record_len:
        raise ValueError("record buffer shorter than n_new * record_len")
    if k_idx and (idx is None or idx.numel() < k_idx or idx.element_size() != 8):
        raise ValueError("idx: k_idx 64-bit device indices")
    k = k_idx + max(n_new - n_old, 0)
    if values is not None and values.numel() * values.element_size() < k * record_len:
        raise ValueError("values shorter than (k_idx + appended) * record_len")
    if ws is None:
        ws = torch.empty(struct_list_tree_update_workspace_bytes(k, spec), dtype=torch.uint8, device=records.device)
    _lib.invoke("mk_dev_ssz_struct_list_tree_update", _p(records), n_old, n_new, capacity, record_len, _fields(spec),
                len(spec), _p(roots), _p(levels), _p(idx) if k_idx else None, k_idx,
                _p(values) if values is not None else None, _p(root), _p(ws), ws.numel(), _stream(records.device),
                device=dev)
    return root


def bytes_list_tree_build_workspace_bytes(n: int, elem_len: int) -> int:
    return _lib.load().mk_ssz_bytes_list_tree_build_workspace_bytes(n, elem_len)


def bytes_list_tree_update_workspace_bytes(k: int, elem_len: int) -> int:
    """Workspace of bytes_list_tree_update for k = changed + appended elements."""
    return _lib.load().mk_ssz_bytes_list_tree_update_workspace_bytes(k, elem_len)


def bytes_list_tree_build(elems: torch.Tensor, n: int, capacity: int, elem_len: int, digests: torch.Tensor,
                          levels: torch.Tensor, root: torch.Tensor = None, ws: torch.Tensor = None) -> torch.Tensor:
    """Every element digest K(le32(elem_len) || e_i) (into ``digests``,
    capacity x 32 B), every level (into ``levels``, the layout of
    ``list_tree_levels_bytes(capacity, 32)``) and the root of TreeHash over the
    n byte strings in ``elems`` (hash.go:100-107, 118-139, 194-239).  Returns
    the (32,) uint8 root tensor."""
    dev = _dev(elems)
    if elems.numel() * elems.element_size() < n * elem_len:
        raise ValueError("element buffer shorter than n * elem_len")
    if digests.numel() < 32 * capacity:
        raise ValueError("digest buffer shorter than 32 * capacity")
    if levels.numel() < list_tree_levels_bytes(capacity, 32):
        raise ValueError("level buffer smaller than mk_ssz_list_tree_levels_bytes(capacity, 32)")
    if root is None:
        root = torch.empty(32, dtype=torch.uint8, device=elems.device)
    if ws is None:
        ws = torch.empty(bytes_list_tree_build_workspace_bytes(n, elem_len), dtype=torch.uint8, device=elems.device)
    _lib.invoke("mk_dev_ssz_bytes_list_tree_build", _p(elems), n, capacity, elem_len, _p(digests), _p(levels),
                _p(root), _p(ws), ws.numel(), _stream(elems.device), device=dev)
    return root


def bytes_list_tree_update(elems: torch.Tensor, n_old: int, n_new: int, capacity: int, elem_len: int,
                           digests: torch.Tensor, levels: torch.Tensor, root: torch.Tensor,
                           idx: torch.Tensor = None, k_idx: int = 0, values: torch.Tensor = None,
                           ws: torch.Tensor = None) -> torch.Tensor:
    """Re-hash a built bytes tree after ``k_idx`` elements changed (``idx``:
    ascending int64/uint64 device indices < n_old) and n_new - n_old were
    appended: those elements' digests and their ancestors only.  ``values``
    (the k_idx new elements, then the appended ones) are scattered into
    ``elems`` first; None: ``elems`` already holds them.  Returns ``root``."""
    dev = _dev(elems)
    if elems.numel() * elems.element_size() < n_new * elem_len:
        raise ValueError("element buffer shorter than n_new * elem_len")
    if digests.numel() < 32 * n_new:
        raise ValueError("digest buffer shorter than 32 * n_new")
    if k_idx and (idx is None or idx.numel() < k_idx or idx.element_size() != 8):
        raise ValueError("idx: k_idx 64-bit device indices")
    k = k_idx + max(n_new - n_old, 0)
    if values is not None and values.numel() * values.element_size() < k * elem_len:
        raise ValueError("values shorter than (k_idx + appended) * elem_len")
    if ws is None:
        ws = torch.empty(bytes_list_tree_update_workspace_bytes(k, elem_len), dtype=torch.uint8, device=elems.device)
    _lib.invoke("mk_dev_ssz_bytes_list_tree_update", _p(elems), n_old, n_new, capacity, elem_len, _p(digests),
                _p(levels), _p(idx) if k_idx else None, k_idx, _p(values) if values is not None else None, _p(root),
                _p(ws), ws.numel(), _stream(elems.device), device=dev)
    return root


def tree_erase_workspace_bytes(kind: int, moved: int, item_len: int) -> int:
    """Workspace of ``tree_erase`` of a tree of ``kind`` (``_lib.MK_TREE_*``):
    moved = n_new - first values of an erase, 0 for a truncate."""
    name = {_lib.MK_TREE_LIST: "list", _lib.MK_TREE_STRUCT: "struct_list", _lib.MK_TREE_BYTES: "bytes_list"}[kind]
    return getattr(_lib.load(), f"mk_ssz_{name}_tree_erase_workspace_bytes")(moved, item_len)


def tree_erase(kind: int, items: torch.Tensor, n_old: int, n_new: int, capacity: int, item_len: int,
               levels: torch.Tensor, root: torch.Tensor, rm: torch.Tensor = None, k_rm: int = 0, first: int = 0,
               level0: torch.Tensor = None, spec=None, ws: torch.Tensor = None) -> torch.Tensor:
    """Shrink a built tree of ``kind`` on the device (``mk_dev_ssz_*_tree_erase``,
    DESIGN.md §5k): the values at the ``k_rm`` strictly ascending 64-bit device
    indices ``rm`` (all >= ``first``) leave and the survivors close the gaps in
    order (n_new == n_old - k_rm); ``k_rm == 0``: the first n_new <= n_old
    values stay.  ``level0``: the struct roots / element digests, which move
    with their values; ``spec``: a struct tree's field layout.  Returns ``root``."""
    from .registry import _fields

    dev = _dev(items)
    if k_rm and (rm is None or rm.numel() < k_rm or rm.element_size() != 8):
        raise ValueError("rm: k_rm 64-bit device indices")
    if (kind != _lib.MK_TREE_LIST) != (level0 is not None):
        raise ValueError("level0 goes with a struct or bytes tree")
    if ws is None:
        ws = torch.empty(tree_erase_workspace_bytes(kind, n_new - first if k_rm else 0, item_len), dtype=torch.uint8,
                         device=items.device)
    tail = (_p(levels), _p(rm) if k_rm else None, k_rm, first, _p(root), _p(ws), ws.numel(), _stream(items.device))
    head = (_p(items), n_old, n_new, capacity, item_len)
    if kind == _lib.MK_TREE_LIST:
        _lib.invoke("mk_dev_ssz_list_tree_erase", *head, *tail, device=dev)
    elif kind == _lib.MK_TREE_STRUCT:
        _lib.invoke("mk_dev_ssz_struct_list_tree_erase", *head, _fields(spec), len(spec), _p(level0), *tail, device=dev)
    else:
        _lib.invoke("mk_dev_ssz_bytes_list_tree_erase", *head, _p(level0), *tail, device=dev)
    return root


class TreeArgs:
    """One tree of ``trees_update`` (mk_tree_update): the arguments of that
    kind's own ``*_tree_update`` wrapper.  ``kind`` is _lib.MK_TREE_LIST /
    STRUCT / BYTES; ``level0`` the struct roots (STRUCT) or element digests
    (BYTES); ``spec`` the field layout (STRUCT); ``container_off`` the byte
    offset of the tree's root in the container message, None: not a field of
    it."""

    def __init__(self, kind: int, items: torch.Tensor, n_old: int, n_new: int, capacity: int, item_len: int,
                 levels: torch.Tensor, root: torch.Tensor, level0: torch.Tensor = None, idx: torch.Tensor = None,
                 k_idx: int = 0, values: torch.Tensor = None, spec=None, container_off: int = None):
        self.kind, self.items, self.n_old, self.n_new, self.capacity = kind, items, n_old, n_new, capacity
        self.item_len, self.levels, self.root, self.level0, self.idx = item_len, levels, root, level0, idx
        self.k_idx, self.values, self.spec, self.container_off = k_idx, values, spec, container_off


def _tree_table(trees, lists: bool = True):
    """The mk_tree_update array of ``trees`` (and what it points to, kept alive by the caller).
    ``lists`` False: without the index arrays and the values (``trees_restore`` reads neither)."""
    from .registry import _fields

    arr = (_lib.TreeUpdate * max(len(trees), 1))()
    keep = []
    for a, t in zip(arr, trees):
        if t.items.numel() * t.items.element_size() < t.n_new * t.item_len:
            raise ValueError("item buffer shorter than n_new * item_len")
        if lists and t.k_idx and (t.idx is None or t.idx.numel() < t.k_idx or t.idx.element_size() != 8):
            raise ValueError("idx: k_idx 64-bit device indices")
        k = t.k_idx + max(t.n_new - t.n_old, 0)
        if lists and t.values is not None and t.values.numel() * t.values.element_size() < k * t.item_len:
            raise ValueError("values shorter than (k_idx + appended) * item_len")
        if t.level0 is not None and t.level0.numel() < 32 * t.n_new:
            raise ValueError("level-0 buffer shorter than 32 * n_new")
        a.kind, a.item_len = t.kind, t.item_len
        a.d_items = t.items.data_ptr()
        a.d_level0 = t.level0.data_ptr() if t.level0 is not None else None
        a.d_levels = t.levels.data_ptr() if t.levels is not None else None
        a.n_old, a.n_new, a.capacity = t.n_old, t.n_new, t.capacity
        a.d_idx = t.idx.data_ptr() if lists and t.k_idx else None
        a.k_idx = t.k_idx
        a.d_values = t.values.data_ptr() if lists and t.values is not None else None
        if t.spec is not None:
            f = _fields(t.spec)
            keep.append(f)
            a.fields, a.nfields = ctypes.cast(f, ctypes.c_void_p), len(t.spec)
        a.container_off = _lib.MK_NO_CONTAINER if t.container_off is None else t.container_off
        a.d_root32 = t.root.data_ptr()
    return arr, keep


def trees_update_workspace_bytes(trees) -> int:
    """Workspace of ``trees_update`` over ``trees`` (0: a list it would refuse)."""
    arr, _keep = _tree_table(trees)
    return _lib.load().mk_ssz_trees_update_workspace_bytes(arr, len(trees))


def trees_update(trees, container: torch.Tensor = None, container_len: int = 0,
                 container_root: torch.Tensor = None, ws: torch.Tensor = None) -> None:
    """Update up to 16 resident trees (``TreeArgs``) in one call: each tree's
    stage 0, then one launch in which all of them climb.  Every tree ends as
    its own ``*_tree_update`` would leave it, its root in ``t.root``.  With
    ``container_len`` > 0, ``container`` is the hash message of the struct
    that holds the trees: each root is also written at its ``container_off``
    and Keccak(container[:container_len]) lands in ``container_root``, all
    in the same launch (mk_dev_ssz_trees_update)."""
    if not trees:
        raise ValueError("no trees")
    dev = _dev(trees[0].items)
    arr, _keep = _tree_table(trees)
    if ws is None:
        ws = torch.empty(_lib.load().mk_ssz_trees_update_workspace_bytes(arr, len(trees)), dtype=torch.uint8,
                         device=trees[0].items.device)
    if container_len and (container is None or container.numel() < container_len or container_root is None or
                          container_root.numel() < 32):
        raise ValueError("container shorter than container_len, or no 32-B container root")
    _lib.invoke("mk_dev_ssz_trees_update", arr, len(trees), _p(container) if container_len else None, container_len,
                _p(container_root) if container_len else None, _p(ws), ws.numel(), _stream(trees[0].items.device),
                device=dev)


def trees_journal_bytes(trees, container_len: int = 0) -> int:
    """Bytes of the undo journal of one ``trees_update`` over ``trees`` (0: a list it would refuse)."""
    arr, _keep = _tree_table(trees)
    return _lib.load().mk_ssz_trees_journal_bytes(arr, len(trees), container_len)


def _trees_journal_call(name, trees, container, container_len, container_root, journal):
    if not trees:
        raise ValueError("no trees")
    if container_len and (container is None or container.numel() < container_len or container_root is None or
                          container_root.numel() < 32):
        raise ValueError("container shorter than container_len, or no 32-B container root")
    arr, _keep = _tree_table(trees, lists=name.endswith("journal"))
    _lib.invoke(name, arr, len(trees), _p(container) if container_len else None, container_len,
                _p(container_root) if container_len else None, _p(journal), journal.numel() * journal.element_size(),
                _stream(trees[0].items.device), device=_dev(trees[0].items))


def trees_journal(trees, journal: torch.Tensor, container: torch.Tensor = None, container_len: int = 0,
                  container_root: torch.Tensor = None) -> None:
    """Save into ``journal`` (16-B aligned, ``trees_journal_bytes`` long) what
    the ``trees_update`` of the same ``trees`` (and container) is about to
    overwrite of the old state: enqueue it before that update, on the same
    stream.  One launch, nothing hashed (mk_dev_ssz_trees_journal, DESIGN.md
    §5r)."""
    _trees_journal_call("mk_dev_ssz_trees_journal", trees, container, container_len, container_root, journal)


def trees_restore(trees, journal: torch.Tensor, container: torch.Tensor = None, container_len: int = 0,
                  container_root: torch.Tensor = None) -> None:
    """Take the update of ``trees`` back out of the ``journal`` that
    ``trees_journal`` filled for it: every tree is again what its ``n_old``
    values specify, the container and its root what they were.  ``idx`` and
    ``values`` of the trees are not read.  One launch
    (mk_dev_ssz_trees_restore); several journals are undone newest first."""
    _trees_journal_call("mk_dev_ssz_trees_restore", trees, container, container_len, container_root, journal)


class TreeCopyArgs:
    """One tree of ``trees_copy`` (mk_tree_copy): the ``n`` values of a built
    tree of ``kind`` laid out for ``src_capacity`` values in ``src_*`` go into
    the layout of ``dst_capacity`` values in ``dst_*``.  ``*_level0``: the struct
    roots / element digests of a STRUCT / BYTES tree (None for a list tree)."""

    def __init__(self, kind: int, item_len: int, n: int, src_capacity: int, dst_capacity: int,
                 src_items: torch.Tensor, src_levels: torch.Tensor, src_root: torch.Tensor,
                 dst_items: torch.Tensor, dst_levels: torch.Tensor, dst_root: torch.Tensor,
                 src_level0: torch.Tensor = None, dst_level0: torch.Tensor = None):
        self.kind, self.item_len, self.n = kind, item_len, n
        self.src_capacity, self.dst_capacity = src_capacity, dst_capacity
        self.src = (src_items, src_level0, src_levels, src_root)
        self.dst = (dst_items, dst_level0, dst_levels, dst_root)


def trees_copy(trees, extra_src: torch.Tensor = None, extra_dst: torch.Tensor = None) -> None:
    """Copy up to 16 built resident trees (``TreeCopyArgs``) between the
    layouts of two capacities, and optionally 32 more bytes (``extra_src`` ->
    ``extra_dst``: a container root), in one launch on the current stream
    (mk_dev_ssz_trees_copy).  Nothing is hashed, uploaded or
    allocated: the call can be captured.  Only the live part of each tree is
    read and written; the rest of the destination buffers stays as it was."""
    arr = (_lib.TreeCopy * max(len(trees), 1))()
    for a, t in zip(arr, trees):
        leaf = t.item_len if t.kind == _lib.MK_TREE_LIST else 32
        for side, cap in ((t.src, t.src_capacity), (t.dst, t.dst_capacity)):
            items, level0, levels, root = side
            if items is not None and items.numel() * items.element_size() < t.n * t.item_len:
                raise ValueError("value buffer shorter than n * item_len")
            if level0 is not None and level0.numel() * level0.element_size() < 32 * t.n:
                raise ValueError("level-0 buffer shorter than 32 * n")
            if levels is not None and levels.numel() * levels.element_size() < list_tree_levels_bytes(cap, leaf):
                raise ValueError("level buffer smaller than mk_ssz_list_tree_levels_bytes(capacity, leaf length)")
            if root is not None and root.numel() * root.element_size() < 32:
                raise ValueError("root buffer shorter than 32 bytes")
        a.kind, a.item_len, a.n = t.kind, t.item_len, t.n
        a.src_capacity, a.dst_capacity = t.src_capacity, t.dst_capacity
        for name, x in zip(("items", "level0", "levels", "root32"), t.src):
            setattr(a, f"d_src_{name}", x.data_ptr() if x is not None else None)
        for name, x in zip(("items", "level0", "levels", "root32"), t.dst):
            setattr(a, f"d_dst_{name}", x.data_ptr() if x is not None else None)
    if (extra_src is None) != (extra_dst is None):
        raise ValueError("the 32-byte extra needs a source and a destination")
    some = next((x for t in trees for x in t.dst + t.src if x is not None), extra_dst)
    if some is None:
        return  # no tree and no extra: nothing to do
    _lib.invoke("mk_dev_ssz_trees_copy", arr, len(trees), _p(extra_src) if extra_src is not None else None,
                _p(extra_dst) if extra_dst is not None else None, _stream(some.device), device=_dev(some))


class TreeAuditArgs:
    """One tree of ``trees_audit`` (mk_tree_audit): the ``n`` values of a built
    tree of ``kind`` laid out for ``capacity`` values.  ``level0``: the struct
    roots / element digests of a STRUCT / BYTES tree (None for a list tree);
    ``spec`` the field layout (STRUCT); ``container_off`` the byte offset of the
    tree's root in the container message, None: not a field of it."""

    def __init__(self, kind: int, items: torch.Tensor, n: int, capacity: int, item_len: int, levels: torch.Tensor,
                 root: torch.Tensor, level0: torch.Tensor = None, spec=None, container_off: int = None):
        self.kind, self.items, self.n, self.capacity, self.item_len = kind, items, n, capacity, item_len
        self.levels, self.root, self.level0, self.spec, self.container_off = levels, root, level0, spec, container_off


def _audit_table(trees):
    from .registry import _fields

    arr = (_lib.TreeAudit * max(len(trees), 1))()
    keep = []
    for a, t in zip(arr, trees):
        leaf = t.item_len if t.kind == _lib.MK_TREE_LIST else 32
        if t.items is not None and t.items.numel() * t.items.element_size() < t.n * t.item_len:
            raise ValueError("value buffer shorter than n * item_len")
        if t.level0 is not None and t.level0.numel() * t.level0.element_size() < 32 * t.n:
            raise ValueError("level-0 buffer shorter than 32 * n")
        if t.levels is not None and t.levels.numel() * t.levels.element_size() < list_tree_levels_bytes(t.capacity, leaf):
            raise ValueError("level buffer smaller than mk_ssz_list_tree_levels_bytes(capacity, leaf length)")
        if t.root is not None and t.root.numel() * t.root.element_size() < 32:
            raise ValueError("root buffer shorter than 32 bytes")
        a.kind, a.item_len, a.n, a.capacity = t.kind, t.item_len, t.n, t.capacity
        a.d_items = t.items.data_ptr() if t.items is not None else None
        a.d_level0 = t.level0.data_ptr() if t.level0 is not None else None
        a.d_levels = t.levels.data_ptr() if t.levels is not None else None
        a.d_root32 = t.root.data_ptr() if t.root is not None else None
        if t.spec is not None:
            f = _fields(t.spec)
            keep.append(f)
            a.fields, a.nfields = ctypes.cast(f, ctypes.c_void_p), len(t.spec)
        a.container_off = _lib.MK_NO_CONTAINER if t.container_off is None else t.container_off
    return arr, keep


def trees_audit_workspace_bytes(trees) -> int:
    """Workspace of ``trees_audit`` over ``trees`` (0: list trees only, or a list it would refuse)."""
    arr, _keep = _audit_table(trees)
    return _lib.load().mk_ssz_trees_audit_workspace_bytes(arr, len(trees))


def trees_audit(trees, container: torch.Tensor = None, container_len: int = 0, container_root: torch.Tensor = None,
                reports: torch.Tensor = None, ws: torch.Tensor = None) -> torch.Tensor:
    """Audit up to 16 built resident trees (``TreeAuditArgs``) and, with
    ``container_len`` > 0, the hash message that holds their roots: every
    stored node against what is stored below it, read-only, on the current
    stream (mk_dev_ssz_trees_audit).  Returns ``reports``, a
    device tensor of 24 * (len(trees) + 1) bytes -- one mk_audit_report per
    tree, then the container's; ``audit_reports`` turns it into tuples.
    Nothing is allocated when ``reports`` and ``ws`` are given: the call can
    be captured."""
    if not trees:
        raise ValueError("no trees")
    dev_t = trees[0].root.device
    arr, _keep = _audit_table(trees)
    if ws is None:
        ws = torch.empty(max(_lib.load().mk_ssz_trees_audit_workspace_bytes(arr, len(trees)), 16), dtype=torch.uint8,
                         device=dev_t)
    if reports is None:
        reports = torch.empty(24 * (len(trees) + 1), dtype=torch.uint8, device=dev_t)
    if reports.numel() * reports.element_size() < 24 * (len(trees) + 1):
        raise ValueError("reports shorter than 24 * (len(trees) + 1) bytes")
    if container_len and (container is None or container.numel() < container_len or container_root is None or
                          container_root.numel() < 32):
        raise ValueError("container shorter than container_len, or no 32-B container root")
    _lib.invoke("mk_dev_ssz_trees_audit", arr, len(trees), _p(container) if container_len else None, container_len,
                _p(container_root) if container_len else None, _p(reports), _p(ws), ws.numel(), _stream(dev_t),
                device=_dev(trees[0].root))
    return reports


def audit_reports(reports: torch.Tensor):
    """``trees_audit``'s device reports as host tuples ``(bad, first_level, first_index)`` (synchronises)."""
    raw = np.ascontiguousarray(reports.cpu().numpy()).view(np.uint8).reshape(-1, 24)
    out = []
    for r in raw:
        bad, idx = (int(x) for x in r[:16].copy().view(np.uint64))
        out.append((bad, int(r[16:20].copy().view(np.uint32)[0]), idx))
    return out


class TreeDiffArgs:
    """One pair of ``trees_diff`` (mk_tree_diff): two built trees of ``kind`` and
    ``item_len``, ``n_a`` values laid out for ``capacity_a`` against ``n_b`` for
    ``capacity_b``.  ``*_level0``: the struct roots / element digests of a
    STRUCT / BYTES tree (None for a list tree; its ``*_items`` are not read).
    ``idx_out``: a uint64 device tensor whose ``max_out`` (default: all) slots
    take the differing indices; None with ``max_out`` 0."""

    def __init__(self, kind: int, item_len: int, a_items: torch.Tensor, a_levels: torch.Tensor, n_a: int,
                 capacity_a: int, b_items: torch.Tensor, b_levels: torch.Tensor, n_b: int, capacity_b: int,
                 idx_out: torch.Tensor = None, max_out: int = None, a_level0: torch.Tensor = None,
                 b_level0: torch.Tensor = None):
        self.kind, self.item_len = kind, item_len
        self.a = (a_items, a_level0, a_levels, n_a, capacity_a)
        self.b = (b_items, b_level0, b_levels, n_b, capacity_b)
        self.idx_out = idx_out
        self.max_out = (idx_out.numel() if idx_out is not None else 0) if max_out is None else max_out


def trees_diff(trees, reports: torch.Tensor = None, stream=None) -> torch.Tensor:
    """Diff up to 16 pairs of built resident trees (``TreeDiffArgs``) by Merkle
    descent, read-only, in one launch on ``stream`` (default: the current one;
    mk_dev_ssz_trees_diff).  Pair i's differing indices below
    min(n_a, n_b) go to its ``idx_out`` in no particular order, only into slots
    below ``max_out``.  Returns ``reports``, a device tensor of 16 * len(trees)
    bytes -- (total, first_index) per pair, ``total`` exact; ``diff_reports``
    turns it into tuples.  Nothing is allocated when ``reports`` is given: the
    call can be captured."""
    if not trees:
        raise ValueError("no trees")
    arr = (_lib.TreeDiff * len(trees))()
    some = None
    for d, t in zip(arr, trees):
        leaf = t.item_len if t.kind == _lib.MK_TREE_LIST else 32
        d.kind, d.item_len = t.kind, t.item_len
        for side, (items, level0, levels, n, cap) in (("a", t.a), ("b", t.b)):
            if items is not None and items.numel() * items.element_size() < n * t.item_len:
                raise ValueError("value buffer shorter than n * item_len")
            if level0 is not None and level0.numel() * level0.element_size() < 32 * n:
                raise ValueError("level-0 buffer shorter than 32 * n")
            if levels is not None and levels.numel() * levels.element_size() < list_tree_levels_bytes(cap, leaf):
                raise ValueError("level buffer smaller than mk_ssz_list_tree_levels_bytes(capacity, leaf length)")
            for name, x in (("items", items), ("level0", level0), ("levels", levels)):
                setattr(d, f"d_{side}_{name}", x.data_ptr() if x is not None else None)
                some = x if some is None and x is not None else some
            setattr(d, f"n_{side}", n)
            setattr(d, f"capacity_{side}", cap)
        if t.idx_out is not None and (t.idx_out.element_size() != 8 or t.idx_out.is_floating_point()):
            raise ValueError("idx_out must be a 64-bit integer tensor")
        if t.max_out and (t.idx_out is None or t.idx_out.numel() < t.max_out):
            raise ValueError("idx_out shorter than max_out")
        d.d_idx_out = t.idx_out.data_ptr() if t.idx_out is not None and t.max_out else None
        d.max_out = t.max_out
    if reports is None:
        if some is None:
            raise ValueError("no device buffer to take the device from: pass reports")
        reports = torch.empty(16 * len(trees), dtype=torch.uint8, device=some.device)
    if reports.numel() * reports.element_size() < 16 * len(trees):
        raise ValueError("reports shorter than 16 * len(trees) bytes")
    st = _stream(reports.device) if stream is None else ctypes.c_void_p(getattr(stream, "cuda_stream", stream))
    _lib.invoke("mk_dev_ssz_trees_diff", arr, len(trees), _p(reports), st, device=_dev(reports))
    return reports


def diff_reports(reports: torch.Tensor):
    """``trees_diff``'s device reports as host tuples ``(total, first_index)`` (synchronises)."""
    raw = np.ascontiguousarray(reports.cpu().numpy()).view(np.uint8).reshape(-1, 16)
    return [tuple(int(x) for x in r.copy().view(np.uint64)) for r in raw]


def prof_enable(on: bool = True) -> None:
    _lib.check(_lib.load().mk_prof_enable(int(on)), "mk_prof_enable")


def prof_read():
    """(summed ms, launches, algorithmic permutations, digests) of the recorded leaf passes."""
    ms = ctypes.c_double()
    cnt = ctypes.c_uint64()
    perms = ctypes.c_double()
    hashes = ctypes.c_double()
    _lib.invoke("mk_prof_read", ctypes.byref(ms), ctypes.byref(cnt), ctypes.byref(perms), ctypes.byref(hashes))
    return ms.value, cnt.value, perms.value, hashes.value
