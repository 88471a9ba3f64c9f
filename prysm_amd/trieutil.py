"""Host mirror of ``shared/trieutil`` (deposit sparse Merkle trie) over the
HIP engine.

Reference: shared/trieutil/deposit_trie.go:13-81, depth 32 from
shared/params/config.go:109.  ``DepositTrie`` keeps the reference's
incremental API (UpdateDepositTrie / GenerateMerkleBranch / Root) over a
device-resident trie handle (``mk_deposit_trie_*``): every level stays in
HBM, and the deposits queued by UpdateDepositTrie are appended at the next
read by one library call that hashes the new leaves and recomputes only the
right edge of each level (<= k/2^d + 2 nodes at level d for k new
deposits).  The live caller, powchain's ``saveInTrie``
(beacon-chain/powchain/service.go:379-386), reads Root() before every
update, so each log costs one leaf hash plus ``depth`` node hashes — the
reference's own O(depth) per deposit — instead of a rebuild.  A batch of
updates followed by one read is the batch build (leaf batch + one launch per
wide level).  Empty nodes are 0^32 (Go map miss); the root of an empty trie
is 0^32.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .hashutil import _flatten, _ptr

DEPOSIT_CONTRACT_TREE_DEPTH = 32  # shared/params/config.go:109
ZERO = bytes(32)


def build_levels(deposits: Sequence[bytes], depth: int = DEPOSIT_CONTRACT_TREE_DEPTH):
    """Batch build: returns (root, levels) with levels[d] an (c_d, 32) uint8
    array of the nodes at height d (d = 0: Hash(deposit))."""
    n = len(deposits)
    root = ctypes.create_string_buffer(32)
    if n == 0:
        _lib.invoke("mk_deposit_trie_build", None, None, 0, depth, None, root)
        return root.raw, []
    data, offs = _flatten(deposits)
    nbytes = _lib.load().mk_deposit_trie_levels_bytes(n, depth)
    lv = np.empty(nbytes, dtype=np.uint8)
    _lib.invoke("mk_deposit_trie_build", _ptr(data), _ptr(offs), n, depth, _ptr(lv), root)
    levels, pos, c = [], 0, n
    for _ in range(depth + 1):
        levels.append(lv[pos * 32:(pos + c) * 32].reshape(c, 32))
        pos += c
        c = (c + 1) // 2
    return root.raw, levels


class DepositTrie:
    """trieutil.DepositTrie (deposit_trie.go:13-16) over a device trie handle."""

    def __init__(self, depth: int = DEPOSIT_CONTRACT_TREE_DEPTH, capacity: int = 0, device: int = -1):
        self.depth = depth
        self.deposit_count = 0
        self._queue: List[bytes] = []
        self._handle: Optional[ctypes.c_void_p] = None
        self._capacity = capacity
        self._device = device

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and _lib is not None:
            try:
                _lib.load().mk_deposit_trie_free(h)
            except Exception:
                pass

    # NewDepositTrie (deposit_trie.go:20-26)
    @classmethod
    def new(cls) -> "DepositTrie":
        return cls()

    @classmethod
    def build(cls, deposits: Sequence[bytes], depth: int = DEPOSIT_CONTRACT_TREE_DEPTH) -> "DepositTrie":
        """Batch constructor: equals NewDepositTrie + UpdateDepositTrie for each."""
        t = cls(depth, capacity=len(deposits))
        for d in deposits:
            t.update_deposit_trie(d)
        return t

    def update_deposit_trie(self, deposit_data: bytes) -> None:
        """UpdateDepositTrie (deposit_trie.go:29-40): queued, appended on the next read."""
        self._queue.append(bytes(deposit_data))
        self.deposit_count += 1

    UpdateDepositTrie = update_deposit_trie

    def _flush(self):
        if not self._queue:
            return
        if self._handle is None:
            h = ctypes.c_void_p()
            _lib.invoke("mk_deposit_trie_new", self.depth, max(self._capacity, len(self._queue)), ctypes.byref(h),
                        device=self._device)
            self._handle = h
        data, offs = _flatten(self._queue)
        _lib.invoke("mk_deposit_trie_append", self._handle, _ptr(data), _ptr(offs), len(self._queue),
                    device=self._device)
        self._queue = []

    def save_logs(self, deposits: Sequence[bytes], log_roots: Sequence[bytes]) -> List[bool]:
        """powchain's ProcessDepositLog -> saveInTrie loop over a batch of logs
        (beacon-chain/powchain/service.go:248-258, 379-386) in one device call:
        in log order, deposit j is appended iff Root() before it equals
        log_roots[j], else the log is skipped.  Returns the per-log accept
        flags; the roots are computed on the device in parallel."""
        if len(deposits) != len(log_roots):
            raise ValueError("one merkle root per log")
        self._flush()
        k = len(deposits)
        if k == 0:
            return []
        if self._handle is None:
            h = ctypes.c_void_p()
            _lib.invoke("mk_deposit_trie_new", self.depth, max(self._capacity, k), ctypes.byref(h),
                        device=self._device)
            self._handle = h
        data, offs = _flatten([bytes(d) for d in deposits])
        roots = b"".join(bytes(r) for r in log_roots)
        if len(roots) != 32 * k:
            raise ValueError("log roots are 32 bytes")
        acc = ctypes.create_string_buffer(k)
        _lib.invoke("mk_deposit_trie_save_logs", self._handle, _ptr(data), _ptr(offs), k, roots, acc,
                    device=self._device)
        flags = [b == 1 for b in acc.raw]
        self.deposit_count += sum(flags)
        return flags

    SaveLogs = save_logs

    def generate_merkle_branch(self, index: int, count: Optional[int] = None) -> List[bytes]:
        """GenerateMerkleBranch (deposit_trie.go:43-58): the sibling at each of
        the `depth` levels; missing nodes read as 0^32.  ``count``: the branch
        as of that many deposits (see generate_merkle_branches); None: now."""
        self._flush()
        if count is not None:
            raw = self.generate_merkle_branches([index], count).tobytes()
            return [raw[32 * d:32 * d + 32] for d in range(self.depth)]
        if self._handle is None:
            return [ZERO] * self.depth
        out = ctypes.create_string_buffer(32 * self.depth)
        _lib.invoke("mk_deposit_trie_branch", self._handle, index, out, device=self._device)
        raw = out.raw
        return [raw[32 * d:32 * d + 32] for d in range(self.depth)]

    GenerateMerkleBranch = generate_merkle_branch

    def _as_of(self, count: Optional[int]) -> int:
        if count is None:
            return self.deposit_count
        if not 0 <= count <= self.deposit_count:
            raise _lib.MerkleError(_lib.MK_EINVAL, f"count {count} outside 0..{self.deposit_count} deposits")
        return count

    def generate_merkle_branches(self, indices: Sequence[int], count: Optional[int] = None,
                                 out: Optional[np.ndarray] = None) -> np.ndarray:
        """GenerateMerkleBranch for every index in one device call, as of
        ``count`` deposits (None: now): what the reference's trie answered
        right after its count-th UpdateDepositTrie, so the branches verify
        against the root of that moment (``root_at(count)``) -- the
        state.LatestEth1Data.DepositRootHash32 that verifyDeposit checks
        (core/blocks/block_operations.go:624-641) -- however many deposits
        powchain has appended since.  Indices in any order, repeats allowed.
        Returns (k, depth, 32) uint8 (``out``, when given: C-contiguous, that
        shape); nothing is written when ``count`` is out of range."""
        self._flush()
        c = self._as_of(count)
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        k = idx.size
        if out is None:
            out = np.empty((k, self.depth, 32), dtype=np.uint8)
        elif out.dtype != np.uint8 or out.shape != (k, self.depth, 32) or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous (k, depth, 32) uint8 array")
        if self._handle is None:
            out[...] = 0
            return out
        _lib.invoke("mk_deposit_trie_branches", self._handle, c, _ptr(idx), k, _ptr(out), None, device=self._device)
        return out

    GenerateMerkleBranches = generate_merkle_branches

    def root_at(self, count: Optional[int] = None) -> bytes:
        """Root() as of ``count`` deposits (None: now); 0^32 for count 0."""
        self._flush()
        c = self._as_of(count)
        if self._handle is None:
            return ZERO
        out = ctypes.create_string_buffer(32)
        _lib.invoke("mk_deposit_trie_root_at", self._handle, c, out, device=self._device)
        return out.raw

    RootAt = root_at

    def root(self) -> bytes:
        """Root (deposit_trie.go:61-63): node 1, 0^32 when empty."""
        self._flush()
        if self._handle is None:
            return ZERO
        out = ctypes.create_string_buffer(32)
        _lib.invoke("mk_deposit_trie_root", self._handle, out, device=self._device)
        return out.raw

    Root = root

    def leaf(self, index: int) -> bytes:
        """Hash(deposit index) (the leaf the trie stores), 0^32 past the end."""
        self._flush()
        if self._handle is None or index >= self.deposit_count:
            return ZERO
        out = ctypes.create_string_buffer(32)
        _lib.invoke("mk_deposit_trie_leaves", self._handle, index, 1, out, device=self._device)
        return out.raw

    # ---- roll back, fork point, audit, clone / copy / reserve ----
    def _ensure_handle(self):
        if self._handle is None:
            h = ctypes.c_void_p()
            _lib.invoke("mk_deposit_trie_new", self.depth, self._capacity, ctypes.byref(h), device=self._device)
            self._handle = h
        return self._handle

    def truncate(self, n: int) -> None:
        """Roll back to the first ``n`` deposits (an ETH1 reorganisation: the
        deposit index of the first removed log).  No deposit data is needed:
        the at most ``depth`` nodes that straddle ``n`` are recomputed from the
        stored ones in one launch.  ``n`` beyond the count raises and nothing
        changes."""
        self._flush()
        if not 0 <= n <= self.deposit_count:
            raise _lib.MerkleError(_lib.MK_EINVAL, f"truncate to {n} outside 0..{self.deposit_count} deposits")
        if self._handle is not None:
            _lib.invoke("mk_deposit_trie_truncate", self._handle, n, device=self._device)
        self.deposit_count = n

    Rollback = truncate

    def fork_point(self, other: "DepositTrie") -> int:
        """The smallest deposit index at which this trie and ``other`` hold
        different leaves, min of the two counts when none does."""
        self._flush()
        other._flush()
        if other.depth != self.depth:
            raise _lib.MerkleError(_lib.MK_EINVAL, f"fork_point: tries of depth {self.depth} and {other.depth}")
        if self._handle is None or other._handle is None:
            return 0
        out = ctypes.c_uint64()
        _lib.invoke("mk_deposit_trie_fork_point", self._handle, other._handle, ctypes.byref(out),
                    device=self._device)
        return int(out.value)

    ForkPoint = fork_point

    def audit(self):
        """Check every stored node of level 1 .. depth against the level below
        it and the root against the top node, on the device, read-only:
        ``(bad, first_level, first_index)`` as the list trees' ``audit()``;
        ``(0, _lib.MK_AUDIT_NONE, 2**64 - 1)`` for a sound trie.  Level 0 is
        not checked: the trie keeps no deposit data."""
        self._flush()
        if self._handle is None:
            return 0, _lib.MK_AUDIT_NONE, 2**64 - 1
        out = _lib.AuditReport()
        _lib.invoke("mk_deposit_trie_audit", self._handle, ctypes.byref(out), device=self._device)
        return out.astuple()

    Audit = audit

    def clone(self) -> "DepositTrie":
        """A new trie holding the same deposits: one copy launch in HBM, no
        hashing.  The two share nothing afterwards (a candidate ETH1 view)."""
        self._flush()
        t = DepositTrie(self.depth, self._capacity, self._device)
        t.deposit_count = self.deposit_count
        if self._handle is not None:
            h = ctypes.c_void_p()
            _lib.invoke("mk_deposit_trie_clone", self._handle, ctypes.byref(h), device=self._device)
            t._handle = h
        return t

    Clone = clone

    def copy_from(self, other: "DepositTrie") -> None:
        """Make this trie a copy of ``other`` (the same depth, else it raises
        and nothing changes); it grows only when ``other``'s deposits do not fit."""
        if other is self:
            return
        other._flush()
        if other.depth != self.depth:
            raise _lib.MerkleError(_lib.MK_EINVAL, f"copy_from: tries of depth {self.depth} and {other.depth}")
        self._queue = []
        if other._handle is None:
            if self._handle is not None:
                _lib.invoke("mk_deposit_trie_truncate", self._handle, 0, device=self._device)
        else:
            _lib.invoke("mk_deposit_trie_copy", self._ensure_handle(), other._handle, device=self._device)
        self.deposit_count = other.deposit_count

    def reserve(self, capacity: int) -> None:
        """Room for ``capacity`` deposits: the next appends up to it move nothing."""
        self._flush()
        _lib.invoke("mk_deposit_trie_reserve", self._ensure_handle(), int(capacity), device=self._device)

    @property
    def capacity(self) -> int:
        """Deposits the trie has room for before an append moves it."""
        self._flush()
        return int(_lib.load().mk_deposit_trie_capacity(self._handle)) if self._handle is not None else 0


def verify_merkle_branches(leaves: Sequence[bytes], branches: Sequence[Sequence[bytes]], depth: int,
                           indices: Sequence[int], roots: Sequence[bytes],
                           tree_depth: int = DEPOSIT_CONTRACT_TREE_DEPTH) -> List[bool]:
    """Batched VerifyMerkleBranch: one GPU thread folds one branch."""
    n = len(leaves)
    if n == 0:
        return []
    lv = np.frombuffer(b"".join(bytes(x) for x in leaves), dtype=np.uint8)
    rt = np.frombuffer(b"".join(bytes(x) for x in roots), dtype=np.uint8)
    br = np.frombuffer(b"".join(bytes(b[i]) for b in branches for i in range(depth)) or b"\0", dtype=np.uint8)
    idx = np.asarray(indices, dtype=np.uint64)
    ok = np.zeros(n, dtype=np.uint8)
    _lib.invoke("mk_verify_merkle_branches", _ptr(lv), _ptr(br), _ptr(idx), n, depth, tree_depth, _ptr(rt), _ptr(ok))
    return [bool(x) for x in ok]


def verify_merkle_branch(leaf: bytes, branch: Sequence[bytes], depth: int, index: int, root: bytes,
                         tree_depth: int = DEPOSIT_CONTRACT_TREE_DEPTH) -> bool:
    """VerifyMerkleBranch (deposit_trie.go:68-81)."""
    return verify_merkle_branches([leaf], [branch], depth, [index], [root], tree_depth)[0]


VerifyMerkleBranch = verify_merkle_branch


def verify_deposits(deposit_datas: Sequence[bytes], branches, indices: Sequence[int], root_or_roots, depth: int,
                    tree_depth: int = DEPOSIT_CONTRACT_TREE_DEPTH) -> List[bool]:
    """verifyDeposit (core/blocks/block_operations.go:624-641) for a batch,
    one GPU thread per deposit: Hash(deposit data), the fold of its branch,
    the compare -- no leaf hashes cross the bus.  ``branches``: the
    (k, depth, 32) array generate_merkle_branches returns, or a list of lists
    of 32-byte siblings.  ``root_or_roots``: one 32-byte root for the whole
    batch (a block's deposits against the state's deposit root) or one per
    deposit."""
    n = len(deposit_datas)
    if n == 0:
        return []
    if isinstance(branches, np.ndarray):
        br = np.ascontiguousarray(branches, dtype=np.uint8).reshape(-1)
    else:
        br = np.frombuffer(b"".join(bytes(b[i]) for b in branches for i in range(depth)), dtype=np.uint8)
    if br.size != 32 * depth * n:
        raise ValueError(f"branches hold {br.size} bytes, not {n} x {depth} x 32")
    shared = isinstance(root_or_roots, (bytes, bytearray, memoryview))
    roots = bytes(root_or_roots) if shared else b"".join(bytes(r) for r in root_or_roots)
    if len(roots) != (32 if shared else 32 * n):
        raise ValueError("one 32-byte root, or one per deposit")
    rt = np.frombuffer(roots, dtype=np.uint8)
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    if idx.size != n:
        raise ValueError("one index per deposit")
    data, offs = _flatten(deposit_datas)
    ok = np.zeros(n, dtype=np.uint8)
    _lib.invoke("mk_verify_deposits", _ptr(data), _ptr(offs), _ptr(br) if depth else None, _ptr(idx), n, depth,
                tree_depth, _ptr(rt), 0 if shared else 32, _ptr(ok))
    return [bool(x) for x in ok]


VerifyDeposits = verify_deposits
