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


class ListTree:
    """A list of fixed-length items and its merkleHash tree, device-resident."""

    def __init__(self, item_len: int, capacity: int = 0, device: int = -1):
        self.item_len = int(item_len)
        self._device = device
        self._handle = None
        h = ctypes.c_void_p()
        _lib.invoke("mk_list_tree_new", self.item_len, int(capacity), ctypes.byref(h), device=device)
        self._handle = h

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and _lib is not None:
            try:
                _lib.load().mk_list_tree_free(h)
            except Exception:
                pass

    def __len__(self) -> int:
        return int(_lib.load().mk_list_tree_count(self._handle))

    def _flat(self, values) -> np.ndarray:
        a = np.ascontiguousarray(values, dtype=np.uint8).reshape(-1)
        if a.size % self.item_len:
            raise ValueError(f"{a.size} bytes are not a whole number of {self.item_len}-byte items")
        return a

    def assign(self, items) -> None:
        """Replace the whole list (uint8 array of n * item_len bytes, any shape)."""
        a = self._flat(items)
        _lib.invoke("mk_list_tree_assign", self._handle, _ptr(a), a.size // self.item_len, device=self._device)

    def update(self, indices, values) -> None:
        """``list[indices[j]] = values[j]`` for every j in order (any order,
        repeats allowed: the last value wins).  An index >= len(self) raises
        and changes nothing."""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        a = self._flat(values)
        if a.size != idx.size * self.item_len:
            raise ValueError("one item_len-byte value per index")
        _lib.invoke("mk_list_tree_update", self._handle, _ptr(idx), _ptr(a), idx.size, device=self._device)

    def append(self, items) -> None:
        """Append items; past the capacity the tree doubles it and rebuilds."""
        a = self._flat(items)
        _lib.invoke("mk_list_tree_append", self._handle, _ptr(a), a.size // self.item_len, device=self._device)

    def root(self) -> bytes:
        """merkleHash of the current items."""
        out = ctypes.create_string_buffer(32)
        _lib.invoke("mk_list_tree_root", self._handle, out, device=self._device)
        return out.raw

    def items(self, first: int = 0, count: int = None) -> np.ndarray:
        """Items [first, first + count) read back as a (count, item_len) uint8 array."""
        if count is None:
            count = len(self) - first
        out = np.empty((max(count, 0), self.item_len), dtype=np.uint8)
        _lib.invoke("mk_list_tree_items", self._handle, first, count, _ptr(out), device=self._device)
        return out


class StructListTree:
    """A list of flat fixed-layout records (``fields`` = [(kind, offset, len)]
    as in ``registry.VALIDATOR_FIELDS``) and the tree of its TreeHash,
    device-resident: records, struct roots and levels."""

    def __init__(self, record_len: int, fields, capacity: int = 0, device: int = -1):
        from .registry import _fields

        self.record_len = int(record_len)
        self.fields = list(fields)
        self._device = device
        self._handle = None
        h = ctypes.c_void_p()
        _lib.invoke("mk_struct_list_tree_new", self.record_len, _fields(self.fields), len(self.fields),
                    int(capacity), ctypes.byref(h), device=device)
        self._handle = h

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and _lib is not None:
            try:
                _lib.load().mk_struct_list_tree_free(h)
            except Exception:
                pass

    def __len__(self) -> int:
        return int(_lib.load().mk_struct_list_tree_count(self._handle))

    def _flat(self, records) -> np.ndarray:
        a = np.ascontiguousarray(records).view(np.uint8).reshape(-1)
        if a.size % self.record_len:
            raise ValueError(f"{a.size} bytes are not a whole number of {self.record_len}-byte records")
        return a

    def assign(self, records) -> None:
        """Replace the whole list (n records: a structured or uint8 array)."""
        a = self._flat(records)
        _lib.invoke("mk_struct_list_tree_assign", self._handle, _ptr(a), a.size // self.record_len,
                    device=self._device)

    def update(self, indices, records) -> None:
        """``list[indices[j]] = records[j]`` for every j in order (any order,
        repeats allowed: the last value wins).  An index >= len(self) raises
        and changes nothing."""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        a = self._flat(records)
        if a.size != idx.size * self.record_len:
            raise ValueError("one record per index")
        _lib.invoke("mk_struct_list_tree_update", self._handle, _ptr(idx), _ptr(a), idx.size, device=self._device)

    def append(self, records) -> None:
        """Append records; past the capacity the tree doubles it and rebuilds."""
        a = self._flat(records)
        _lib.invoke("mk_struct_list_tree_append", self._handle, _ptr(a), a.size // self.record_len,
                    device=self._device)

    def root(self) -> bytes:
        """TreeHash of the current list of records."""
        out = ctypes.create_string_buffer(32)
        _lib.invoke("mk_struct_list_tree_root", self._handle, out, device=self._device)
        return out.raw

    def records(self, first: int = 0, count: int = None) -> np.ndarray:
        """Records [first, first + count) read back as a (count, record_len) uint8 array."""
        if count is None:
            count = len(self) - first
        out = np.empty((max(count, 0), self.record_len), dtype=np.uint8)
        _lib.invoke("mk_struct_list_tree_records", self._handle, first, count, _ptr(out), device=self._device)
        return out


class BytesListTree:
    """A list of byte strings of ``elem_len`` bytes each (``[][N]byte``) and
    the tree of its TreeHash, device-resident: elements, element digests and
    levels."""

    def __init__(self, elem_len: int, capacity: int = 0, device: int = -1):
        self.elem_len = int(elem_len)
        self._device = device
        self._handle = None
        h = ctypes.c_void_p()
        _lib.invoke("mk_bytes_list_tree_new", self.elem_len, int(capacity), ctypes.byref(h), device=device)
        self._handle = h

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and _lib is not None:
            try:
                _lib.load().mk_bytes_list_tree_free(h)
            except Exception:
                pass

    def __len__(self) -> int:
        return int(_lib.load().mk_bytes_list_tree_count(self._handle))

    def _flat(self, elems) -> np.ndarray:
        a = np.ascontiguousarray(elems, dtype=np.uint8).reshape(-1)
        if a.size % self.elem_len:
            raise ValueError(f"{a.size} bytes are not a whole number of {self.elem_len}-byte elements")
        return a

    def assign(self, elems) -> None:
        """Replace the whole list (uint8 array of n * elem_len bytes, any shape)."""
        a = self._flat(elems)
        _lib.invoke("mk_bytes_list_tree_assign", self._handle, _ptr(a), a.size // self.elem_len,
                    device=self._device)

    def update(self, indices, elems) -> None:
        """``list[indices[j]] = elems[j]`` for every j in order (any order,
        repeats allowed: the last value wins).  An index >= len(self) raises
        and changes nothing."""
        idx = np.ascontiguousarray(indices, dtype=np.uint64).reshape(-1)
        a = self._flat(elems)
        if a.size != idx.size * self.elem_len:
            raise ValueError("one elem_len-byte element per index")
        _lib.invoke("mk_bytes_list_tree_update", self._handle, _ptr(idx), _ptr(a), idx.size, device=self._device)

    def append(self, elems) -> None:
        """Append elements; past the capacity the tree doubles it and rebuilds."""
        a = self._flat(elems)
        _lib.invoke("mk_bytes_list_tree_append", self._handle, _ptr(a), a.size // self.elem_len,
                    device=self._device)

    def root(self) -> bytes:
        """TreeHash of the current list of byte strings."""
        out = ctypes.create_string_buffer(32)
        _lib.invoke("mk_bytes_list_tree_root", self._handle, out, device=self._device)
        return out.raw

    def elems(self, first: int = 0, count: int = None) -> np.ndarray:
        """Elements [first, first + count) read back as a (count, elem_len) uint8 array."""
        if count is None:
            count = len(self) - first
        out = np.empty((max(count, 0), self.elem_len), dtype=np.uint8)
        _lib.invoke("mk_bytes_list_tree_elems", self._handle, first, count, _ptr(out), device=self._device)
        return out
