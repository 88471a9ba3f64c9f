"""Host mirror of the device-resident list tree (``mk_list_tree_*``).

``ssz.merkleHash`` (shared/ssz/hash.go:194-239) is one-shot: the whole list
in, the root out.  A beacon node's long lists (the validator registry, the
balances) live for the life of the process and change in a few places between
two state roots.  ``ListTree`` keeps such a list and every level of its tree
in HBM; ``update`` and ``append`` upload only the changed items and re-hash
only the ancestors of the changed chunks, and ``root()`` always equals
``merkleHash`` of the current items.  There is no CPU fallback.

A list of STRUCTS (the validator registry itself) has a handle of its own,
``StructListTree`` (``mk_struct_list_tree_*``): it owns the
records as well as their 32-B struct roots and the levels over them, so a
changed ``ValidatorRecord`` goes in as a record and costs its own struct hash
plus its ancestors::

    tree = StructListTree(160, VALIDATOR_FIELDS, capacity=n)
    tree.assign(reg.records)                                  # once
    ...
    tree.update(indices, changed_records)                     # per state root
    root = tree.root()           # == registry.struct_list_root(all records)

(device-resident callers use ``device.struct_list_tree_build`` /
``struct_list_tree_update`` and never leave the GPU;
``registry.ResidentState`` pairs the registry with a ``ListTree(8)`` of the
balances and returns the State root).

A list of BYTE STRINGS (``[][N]byte``: the state's randao mixes, block roots
and index roots, where one element changes per slot) has ``BytesListTree``
(``mk_bytes_list_tree_*``): it owns the elements, their digests
``K(le32(N) || e_i)`` and the levels over them::

    tree = BytesListTree(32, capacity=8192)
    tree.assign(block_roots)                                  # once
    tree.update([slot % 8192], new_root)                      # per slot
    root = tree.root()           # == ssz.tree_hash_bytes_list(all elements)
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .hashutil import _ptr

DIFF_FIRST = 4096  # index slots of a diff()'s first call when the caller sets no bound


class _Tree:
    """What the three handles share: a list of ``_len``-byte values behind the
    ``mk_<_prefix>_*`` entry points (one handle core in C: csrc/tree_handle.cpp)."""

    _prefix = ""    # C symbol prefix: mk_<_prefix>_new, _assign, ...
    _noun = ""      # what a value is called in messages
    _one = ""       # ValueError text of update(): "one ... per index"
    _reader = ""    # name of the read-back entry point and method
    _leaf32 = False  # level 0 is a 32-B root / digest per value, not the value itself

    def __init__(self, value_len: int, *new_args, device: int = -1):
        self._len = int(value_len)
        self._device = device
        self._handle = None
        h = ctypes.c_void_p()
        _lib.invoke(f"mk_{self._prefix}_new", self._len, *new_args, ctypes.byref(h), device=device)
        self._handle = h

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and _lib is not None:
            try:
                getattr(_lib.load(), f"mk_{self._prefix}_free")(h)
            except Exception:
                pass

    def __len__(self) -> int:
        return int(getattr(_lib.load(), f"mk_{self._prefix}_count")(self._handle))

    def _bytes(self, values) -> np.ndarray:
        return np.ascontiguousarray(values, dtype=np.uint8)

    def _flat(self, values) -> np.ndarray:
        a = self._bytes(values).reshape(-1)
        if a.size % self._len:
            raise ValueError(f"{a.size} bytes are not a whole number of {self._len}-byte {self._noun}")
        return a

    def _call(self, op: str, *args):
        _lib.invoke(f"mk_{self._prefix}_{op}", self._handle, *args, device=self._device)

    def assign(self, values) -> None:
        """Replace the whole list (uint8 array of n * value_len bytes, any
        shape; a StructListTree also takes a structured array)."""
        a = self._flat(values)
        self._call("assign", _ptr(a), a.size // self._len)

    def update(self, indices, values) -> None:
        """``list[indices[j]] = values[j]`` for every j in order (any order,
        repeats allowed: the last value wins).  An index >= len(self) raises
        and changes nothing."""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        a = self._flat(values)
        if a.size != idx.size * self._len:
            raise ValueError(self._one)
        self._call("update", _ptr(idx), _ptr(a), idx.size)

    def append(self, values) -> None:
        """Append values; past the capacity the tree doubles it and rebuilds."""
        a = self._flat(values)
        self._call("append", _ptr(a), a.size // self._len)

    def truncate(self, n: int) -> None:
        """Keep the first ``n`` values (on the device: nothing is uploaded);
        ``n`` > len(self) raises and changes nothing."""
        self._call("truncate", int(n))

    def erase(self, indices) -> None:
        """Remove the values at ``indices`` (any order, a repeat counts once)
        and close the gaps in order, on the device: only the indices are
        uploaded, and no survivor is hashed again.  An index >= len(self)
        raises and changes nothing."""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        self._call("erase", _ptr(idx), idx.size)

    def root(self) -> bytes:
        """merkleHash (ListTree) / TreeHash (the other two) of the current list."""
        out = ctypes.create_string_buffer(32)
        self._call("root", out)
        return out.raw

    def _read(self, first: int = 0, count: int = None) -> np.ndarray:
        """Values [first, first + count) read back as a (count, value_len) uint8 array."""
        if count is None:
            count = len(self) - first
        out = np.empty((max(count, 0), self._len), dtype=np.uint8)
        self._call(self._reader, first, count, _ptr(out))
        return out

    def branches(self, indices):
        """Merkle proofs of the values at ``indices`` (any order, repeats
        allowed; an index >= len(self) raises): ``(values, branches)``, the
        (k, leaf_len) level-0 values -- the items of a ListTree, the 32-B struct
        roots / element digests of the other two -- and the (k, stride) proof
        records that ``verify_branches`` takes with ``root()``.
        One upload of the indices, one launch, one read-back."""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        leaf = 32 if self._leaf32 else self._len
        stride = int(_lib.load().mk_ssz_list_branch_bytes(len(self), leaf))
        values = np.zeros((idx.size, leaf), dtype=np.uint8)
        out = np.zeros((idx.size, stride), dtype=np.uint8)
        self._call("branches", _ptr(idx), idx.size, _ptr(values), _ptr(out))
        return values, out

    # ---- a second resident tree, or more room, without uploading or hashing anything
    @property
    def capacity(self) -> int:
        """Values the tree has room for before an append rebuilds it."""
        return int(getattr(_lib.load(), f"mk_{self._prefix}_capacity")(self._handle))

    def clone(self):
        """A new tree of the same kind, value length, layout and capacity
        holding this list: one copy launch in HBM.  The two share nothing
        afterwards (a candidate block's post-state, the other side of a fork)."""
        h = ctypes.c_void_p()
        self._call("clone", ctypes.byref(h))
        t = object.__new__(type(self))
        t.__dict__.update(self.__dict__)
        t._handle = h
        return t

    def copy_from(self, other) -> None:
        """Make this tree a copy of ``other`` (the same kind, value length and
        layout, else it raises and nothing changes).  It keeps its capacity
        when ``other``'s values fit and takes ``other``'s otherwise."""
        if type(other) is not type(self):
            raise _lib.MerkleError(_lib.MK_EINVAL, f"copy_from: a {type(other).__name__} into a {type(self).__name__}")
        self._call("copy", other._handle)

    def reserve(self, capacity: int) -> None:
        """Room for ``capacity`` values: the tree moves into the layout of the
        new capacity on the device; root, count and values stay.  A smaller
        ``capacity`` than the current one does nothing."""
        self._call("reserve", int(capacity))

    def audit(self):
        """Check every stored node of the tree against what is stored below it
        -- level 0 against the values, each level against the one below, the
        root against the top and the length -- on the device, read-only
        (DESIGN.md §5n): ``(bad, first_level, first_index)``, the number of
        mismatches and the smallest (level, index) among them;
        ``(0, _lib.MK_AUDIT_NONE, 2**64 - 1)`` for a sound tree.  Level
        ``_lib.MK_AUDIT_ROOT`` is the root."""
        out = _lib.AuditReport()
        self._call("audit", ctypes.byref(out))
        return out.astuple()

    def diff(self, other, max_out: int = None):
        """Which values differ between this tree and ``other`` (the same kind,
        value length and layout, else it raises)?  Found in HBM by walking
        down from the top only through stored nodes that differ (DESIGN.md
        §5o): ``(indices, total, n_self, n_other)`` -- the differing indices
        below min(n_self, n_other) as an ascending uint64 array, their exact
        number and the two counts.  A StructListTree compares the records'
        roots, a BytesListTree the elements' digests.  With ``max_out`` the
        array holds at most that many of them (``total`` says how many there
        are); None: all of them, with a second call when there are more than
        ``DIFF_FIRST``.  One launch and one read-back per call."""
        if type(other) is not type(self):
            raise _lib.MerkleError(_lib.MK_EINVAL, f"diff: a {type(other).__name__} against a {type(self).__name__}")
        want = DIFF_FIRST if max_out is None else int(max_out)
        while True:
            out = np.empty(want, dtype=np.uint64)
            total, na, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            self._call("diff", other._handle, _ptr(out) if want else None, want, ctypes.byref(total), ctypes.byref(na),
                       ctypes.byref(nb))
            if max_out is None and total.value > want:
                want = int(total.value)
                max_out = want  # once: the trees may change between the two calls
                continue
            return out[:min(total.value, want)].copy(), int(total.value), int(na.value), int(nb.value)


def verify_branches(values, indices, n: int, item_len: int, branches, root, container=None,
                    container_off: int = None, device: int = -1) -> np.ndarray:
    """Verify list-tree proofs from host buffers on the GPU
    (mk_verify_list_branches): a bool array, True where ``values[g]`` at index
    ``indices[g]`` of a list of ``n`` ``item_len``-byte leaves folds through
    ``branches[g]`` to ``root`` -- one 32-byte root for the batch, or one per
    proof.  With ``container`` (the message ``TreeSet.branches`` returns) the
    list root is substituted at ``container_off`` and the hash of the message
    is what is compared (``TreeSet.root()``)."""
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    k = idx.size
    vals = np.ascontiguousarray(values, dtype=np.uint8).reshape(-1)
    br = np.ascontiguousarray(branches, dtype=np.uint8).reshape(-1)
    roots = np.frombuffer(bytes(root), dtype=np.uint8) if isinstance(root, (bytes, bytearray)) else \
        np.ascontiguousarray(root, dtype=np.uint8).reshape(-1)
    stride = int(_lib.load().mk_ssz_list_branch_bytes(n, item_len))
    if vals.size != k * item_len or br.size != k * stride:
        raise ValueError("one item_len-byte value and one proof record per index")
    if roots.size not in (32, 32 * k):
        raise ValueError("one 32-byte root, or one per proof")
    root_stride = 32 if (roots.size == 32 * k and k != 1) else 0
    cont = None
    if container is not None and len(container):
        if container_off is None:
            raise ValueError("a container needs the tree's container_off")
        cont = np.frombuffer(bytes(container), dtype=np.uint8)
    ok = np.zeros(k, dtype=np.uint8)
    _lib.invoke("mk_verify_list_branches", _ptr(vals), _ptr(idx), k, int(n), int(item_len), _ptr(br), _ptr(roots),
                root_stride, _ptr(cont) if cont is not None else None, cont.size if cont is not None else 0,
                int(container_off or 0), _ptr(ok), device=device)
    return ok.astype(bool)


def _verify_repeat_hash(call, head, indices, reveals, commit_off, layers_off, max_layers) -> np.ndarray:
    """What StructListTree.verify_repeat_hash and TreeSet.verify_repeat_hash share."""
    idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
    rev = np.ascontiguousarray(reveals, dtype=np.uint8).reshape(-1)
    if rev.size != 32 * idx.size:
        raise ValueError("one 32-byte reveal per index")
    ok = np.zeros(idx.size, dtype=np.uint8)
    call("verify_repeat_hash", *head, int(commit_off), int(layers_off), _ptr(idx), _ptr(rev), idx.size,
         int(max_layers), _ptr(ok))
    return ok


class ListTree(_Tree):
    """A list of fixed-length items and its merkleHash tree, device-resident."""

    _prefix, _noun, _one, _reader = "list_tree", "items", "one item_len-byte value per index", "items"
    items = _Tree._read

    def __init__(self, item_len: int, capacity: int = 0, device: int = -1):
        super().__init__(item_len, int(capacity), device=device)
        self.item_len = self._len


class StructListTree(_Tree):
    """A list of flat fixed-layout records (``fields`` = [(kind, offset, len)]
    as in ``registry.VALIDATOR_FIELDS``) and the tree of its TreeHash,
    device-resident: records, struct roots and levels."""

    _prefix, _noun, _one, _reader = "struct_list_tree", "records", "one record per index", "records"
    _leaf32 = True
    records = _Tree._read

    def __init__(self, record_len: int, fields, capacity: int = 0, device: int = -1):
        from .registry import _fields

        self.fields = list(fields)
        super().__init__(record_len, _fields(self.fields), len(self.fields), int(capacity), device=device)
        self.record_len = self._len

    def _bytes(self, records) -> np.ndarray:  # a structured array as its bytes: no dtype conversion
        return np.ascontiguousarray(records).view(np.uint8)

    def verify_repeat_hash(self, indices, reveals, commit_off: int, layers_off: int,
                           max_layers: int = _lib.MK_REPEAT_MAX_LAYERS) -> np.ndarray:
        """verifyBlockRandao (block_operations.go:109-123) for m proposals
        against the records the tree holds on the device: (m,) uint8, 1 where
        ``RepeatHash(reveals[j], le64(rec[layers_off:+8])) ==
        rec[commit_off:+32]`` for record ``indices[j]``, 0 where not, 2 where
        the record's 64-bit layer count exceeds ``max_layers`` (the chain is not
        run).  Only the indices and the reveals go up and m bytes come back; the
        tree is not changed.  An index >= len(self) or an offset past the record
        raises."""
        return _verify_repeat_hash(self._call, (), indices, reveals, commit_off, layers_off, max_layers)


class BytesListTree(_Tree):
    """A list of byte strings of ``elem_len`` bytes each (``[][N]byte``) and
    the tree of its TreeHash, device-resident: elements, element digests and
    levels."""

    _prefix, _noun, _one, _reader = "bytes_list_tree", "elements", "one elem_len-byte element per index", "elems"
    _leaf32 = True
    elems = _Tree._read

    def __init__(self, elem_len: int, capacity: int = 0, device: int = -1):
        super().__init__(elem_len, int(capacity), device=device)
        self.elem_len = self._len


class TreeSet:
    """Up to ``_lib.MK_TREES_MAX`` resident trees of the three kinds and the
    hash message of the struct that holds them behind one handle
    (``mk_tree_set_*``).  ``update`` / ``append`` / ``put`` only
    record the change on the host; ``root()`` uploads every tree's changes in
    one copy, runs the update over all the trees (every climb and the hash of
    the message in one launch) and reads 32 bytes back::

        s = TreeSet(container_len=72)
        bal = s.add(_lib.MK_TREE_LIST, 8, container_off=0)
        roots = s.add(_lib.MK_TREE_BYTES, 32, container_off=32)
        s.put(64, slot_le64)                                      # the other fields
        s.assign(bal, balances); s.assign(roots, block_roots)     # once
        s.update(bal, [17], new_balance); s.append(roots, r)      # per slot
        root = s.root()              # == TreeHash of the whole struct

    numpy in, bytes out; there is no CPU fallback."""

    def __init__(self, container_len: int = 0, device: int = -1):
        self.container_len = int(container_len)
        self._device = device
        self._handle = None
        self._len = []  # value length of every tree
        self._leaf = []  # length of its level-0 entries: the value's (a list tree) or 32
        self._coff = []  # where its root goes in the message (None: nowhere)
        h = ctypes.c_void_p()
        _lib.invoke("mk_tree_set_new", self.container_len, ctypes.byref(h), device=device)
        self._handle = h

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and _lib is not None:
            try:
                _lib.load().mk_tree_set_free(h)
            except Exception:
                pass

    def __len__(self) -> int:
        return len(self._len)

    def _call(self, op: str, *args):
        _lib.invoke(f"mk_tree_set_{op}", self._handle, *args, device=self._device)

    def _tree(self, tree) -> int:
        """The number of a tree (a subclass may know its trees by name)."""
        return int(tree)

    def _flat(self, tree: int, values) -> np.ndarray:
        a = np.ascontiguousarray(values)
        a = (a.view(np.uint8) if a.dtype != np.uint8 else a).reshape(-1)
        L = self._len[tree]
        if a.size % L:
            raise ValueError(f"{a.size} bytes are not a whole number of {L}-byte values")
        return a

    def add(self, kind: int, value_len: int, fields=None, capacity: int = 0, container_off: int = None) -> int:
        """A new, empty tree; returns its number.  ``fields``: the record
        layout of a ``MK_TREE_STRUCT`` tree; ``container_off``: where its root
        goes in the message (None: it is no field of it)."""
        from .registry import _fields

        out = ctypes.c_uint32()
        off = _lib.MK_NO_CONTAINER if container_off is None else int(container_off)
        spec = list(fields) if fields is not None else []
        self._call("add", int(kind), int(value_len), _fields(spec) if fields is not None else None, len(spec),
                   int(capacity), off, ctypes.byref(out))
        self._len.append(int(value_len))
        self._leaf.append(int(value_len) if int(kind) == _lib.MK_TREE_LIST else 32)
        self._coff.append(None if container_off is None else int(container_off))
        return int(out.value)

    def put(self, off: int, data) -> None:
        """Bytes of the message outside every tree's root: the other fields' outputs."""
        a = np.frombuffer(bytes(data), dtype=np.uint8)
        self._call("put", int(off), _ptr(a), a.size)

    def assign(self, tree, values) -> None:
        """Replace the whole list of a tree (through the build entry, at once)."""
        tree = self._tree(tree)
        a = self._flat(tree, values)
        self._call("assign", tree, _ptr(a), a.size // self._len[tree])

    def update(self, tree, indices, values) -> None:
        """``list[indices[j]] = values[j]`` in order, recorded on the host; an
        index >= count(tree) raises and changes nothing."""
        tree = self._tree(tree)
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        a = self._flat(tree, values)
        if a.size != idx.size * self._len[tree]:
            raise ValueError("one value per index")
        self._call("update", tree, _ptr(idx), _ptr(a), idx.size)

    def append(self, tree, values) -> None:
        tree = self._tree(tree)
        a = self._flat(tree, values)
        self._call("append", tree, _ptr(a), a.size // self._len[tree])

    def truncate(self, tree, n: int) -> None:
        """Keep the first ``n`` values of a tree.  Not recorded: whatever the
        set has pending is flushed, then the tree shrinks on the device at
        once (``BeaconTreeSet``: ``truncate("eth1_votes", 0)`` at the end of a
        voting period)."""
        self._call("truncate", self._tree(tree), int(n))

    def erase(self, tree, indices) -> None:
        """Remove the values at ``indices`` (any order, a repeat counts once)
        of a tree and close the gaps in order, at once as ``truncate``
        (``BeaconTreeSet``: ``erase("attestations", dropped)`` is
        CleanupAttestations)."""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        self._call("erase", self._tree(tree), _ptr(idx), idx.size)

    def count(self, tree) -> int:
        """Items of a tree, pending appends included."""
        return int(_lib.load().mk_tree_set_count(self._handle, self._tree(tree)))

    def root(self) -> bytes:
        """The hash of the message with every tree's root in place."""
        out = ctypes.create_string_buffer(32)
        self._call("root", out)
        return out.raw

    def tree_root(self, tree) -> bytes:
        out = ctypes.create_string_buffer(32)
        self._call("tree_root", self._tree(tree), out)
        return out.raw

    def items(self, tree, first: int = 0, count: int = None) -> np.ndarray:
        """Values [first, first + count) of a tree as a (count, value_len) uint8 array."""
        tree = self._tree(tree)
        if count is None:
            count = self.count(tree) - first
        out = np.empty((max(count, 0), self._len[tree]), dtype=np.uint8)
        self._call("items", tree, first, count, _ptr(out))
        return out

    # ---- a second resident state, or more room for one tree
    def capacity(self, tree) -> int:
        """Values a tree has room for before a flush has to rebuild it."""
        return int(_lib.load().mk_tree_set_capacity(self._handle, self._tree(tree)))

    def clone(self):
        """A new set of the same trees holding this one's lists and message,
        pending changes included (they are flushed first, as ``root()`` does):
        one copy launch over all the trees and the container root, nothing
        uploaded, nothing hashed.  The two share nothing afterwards; a subclass
        keeps its type and whatever it knows its trees by."""
        h = ctypes.c_void_p()
        self._call("clone", ctypes.byref(h))
        s = object.__new__(type(self))
        s.__dict__.update({k: (v.copy() if isinstance(v, (list, dict)) else v) for k, v in self.__dict__.items()})
        s._handle = h
        return s

    def copy_from(self, other) -> None:
        """Make this set a copy of ``other`` (flushed first), dropping what
        this one has pending: the way back after a block that failed.  The sets
        must agree in container length and, tree by tree, in kind, value length,
        layout and container offset, else it raises and nothing changes."""
        self._call("copy", other._handle)

    def reserve(self, tree, capacity: int) -> None:
        """Room for ``capacity`` values in one tree; pending changes stay pending."""
        self._call("reserve", self._tree(tree), int(capacity))

    # ---- checkpoints: a change taken back through an undo journal
    def checkpoint(self) -> int:
        """Flush what is pending and open a checkpoint; the id ``rollback`` and
        ``release`` take.  While one is open every flush saves what it
        overwrites (about changed x depth nodes) before it updates.  At most
        ``_lib.MK_CHECKPOINTS_MAX`` are open at a time."""
        cp = ctypes.c_uint64()
        self._call("checkpoint", ctypes.byref(cp))
        return int(cp.value)

    def rollback(self, cp: int) -> None:
        """Back to the state at checkpoint ``cp``: pending changes dropped,
        every record since undone newest first, nothing re-hashed but the roots'
        mix-ins and the message.  Closes ``cp`` and every later checkpoint; an
        unknown or closed id raises and nothing changes."""
        self._call("rollback", int(cp))

    def release(self, cp: int) -> None:
        """Forget checkpoint ``cp`` and every earlier one (the finalised case)
        and free what only they needed."""
        self._call("release", int(cp))

    def journal_bytes(self) -> int:
        """Bytes of HBM the open checkpoints hold."""
        return int(_lib.load().mk_tree_set_journal_bytes(self._handle))

    def journal_capacity(self) -> int:
        """Bytes allocated for the journals (what ``release`` frees is used again before this grows)."""
        return int(_lib.load().mk_tree_set_journal_capacity(self._handle))

    def journal_reserve(self, nbytes: int) -> None:
        """Room for ``nbytes`` of journal, so that no flush of a slot grows it."""
        self._call("journal_reserve", int(nbytes))

    def audit(self):
        """Is every tree what its values say, and the message what the trees
        say?  Whatever is pending is flushed first, as ``root()`` does; then
        every stored node of every tree, every root, the roots' 32 bytes in the
        message and the hash of the message are checked in HBM
        and len(self) + 1 reports ``(bad, first_level, first_index)`` come
        back, tree by tree and the container's last (index 0: the hash of the
        message, 1 + i: tree i's root in it).  All ``(0, MK_AUDIT_NONE, ...)``:
        the resident state is sound, and a state root that does not match
        ``root()`` is the block's fault."""
        out = (_lib.AuditReport * (len(self) + 1))()
        self._call("audit", out)
        return [r.astuple() for r in out]

    def diff(self, other, max_out: int = None):
        """Which values differ between this set and ``other`` (sets that agree as
        ``copy_from`` requires, else it raises and nothing changes)?  Both are
        flushed first, as ``root()`` does; one launch walks all the trees down
        from their tops through the stored nodes that differ
        and one read-back follows.  A dict: tree number -> ``(indices, total,
        n_self, n_other)`` as ``_Tree.diff``, and ``"container"`` -> ``(total,
        first_offset)``, the bytes of the two messages outside every tree's
        root that differ (what ``put`` wrote) and the first such offset (None:
        none).  ``max_out`` bounds the indices per tree; None: all of them,
        with a second call when a tree has more than ``DIFF_FIRST``."""
        nt = len(self)
        per = DIFF_FIRST if max_out is None else int(max_out)
        while True:
            reports = (_lib.DiffReport * (nt + 1))()
            out = np.empty((nt, per), dtype=np.uint64)
            self._call("diff", other._handle, reports, _ptr(out) if out.size else None, per)
            most = max((int(r.total) for r in reports[:nt]), default=0)
            if max_out is None and most > per:
                per = max_out = most  # once
                continue
            break
        res = {}
        for i in range(nt):
            total = int(reports[i].total)
            res[i] = (out[i, :min(total, per)].copy(), total, self.count(i), other.count(i))
        total, first = reports[nt].astuple()
        res["container"] = (total, first if total else None)
        return res

    def leaf_len(self, tree) -> int:
        """Bytes of a level-0 entry of a tree: what ``branches`` proves."""
        return self._leaf[self._tree(tree)]

    def container_off(self, tree):
        """Where a tree's root lies in the message (None: it is no field of it)."""
        return self._coff[self._tree(tree)]

    def branches(self, tree, indices):
        """Merkle proofs of the values at ``indices`` of one tree, whatever is
        pending flushed first as ``root()`` does: ``(values, branches,
        container)`` -- ``_Tree.branches``' pair and the hash message with
        every tree's root in place (b"" for a set without a container).
        ``verify_branches(values, indices, count(tree), leaf_len(tree),
        branches, root(), container, container_off(tree))`` checks them against
        the root of the whole struct; a tree that is no field of the container
        verifies against ``tree_root(tree)`` with no container."""
        tree = self._tree(tree)
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        leaf = self._leaf[tree]
        stride = int(_lib.load().mk_ssz_list_branch_bytes(self.count(tree), leaf))
        values = np.zeros((idx.size, leaf), dtype=np.uint8)
        out = np.zeros((idx.size, stride), dtype=np.uint8)
        msg = np.zeros(self.container_len, dtype=np.uint8)
        self._call("branches", tree, _ptr(idx), idx.size, _ptr(values), _ptr(out), _ptr(msg))
        return values, out, msg.tobytes()

    def verify_repeat_hash(self, tree, indices, reveals, commit_off: int, layers_off: int,
                           max_layers: int = _lib.MK_REPEAT_MAX_LAYERS) -> np.ndarray:
        """``StructListTree.verify_repeat_hash`` against the records of one
        ``MK_TREE_STRUCT`` tree of the set (any other kind raises), whatever is
        pending flushed first as ``root()`` does: an update not yet flushed is
        seen."""
        return _verify_repeat_hash(self._call, (self._tree(tree),), indices, reveals, commit_off, layers_off,
                                   max_layers)
