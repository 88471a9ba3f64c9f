"""ctypes binding of libprysm_merkle.so (include/prysm_merkle.h).

This is the Python-side twin of the cgo binding a Go maintainer would add
(INTEGRATION.md).  The library is built in-tree (``prysm_amd/lib/``) by
``__graft_entry__.build()`` / ``make -C prysm_amd/csrc``.  There is no CPU
fallback anywhere in the product path: if the library is missing, or no
gfx950 device is visible, calls raise ``MerkleError`` loudly.
"""
from __future__ import annotations

import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libprysm_merkle.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "prysm_merkle.h")

MK_OK = 0
MK_EINVAL = -22
MK_ENODEV = -19
MK_ENOMEM = -12
MK_EHIP = -5
MK_ECOMM = -71


class MerkleError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{msg} (code {code})")
        self.code = code


_c = ctypes
_vp = _c.c_void_p
_u64, _u32, _int = _c.c_uint64, _c.c_uint32, _c.c_int


class Call(ctypes.Structure):
    """mk_call: per-call device selection and error detail (include/prysm_merkle.h)."""
    _fields_ = [("device", ctypes.c_int32), ("code", ctypes.c_int32), ("err", ctypes.c_char * 256)]


_cp = _c.POINTER(Call)

# name -> (restype, argtypes); entry points taking a per-call context list it first
_SIGS = {
    "mk_init": (_int, [_int]),
    "mk_device_count": (_int, []),
    "mk_strerror": (_c.c_char_p, [_int]),
    "mk_last_error": (_c.c_char_p, []),
    "mk_version": (_c.c_char_p, []),
    "mk_hash": (_int, [_cp, _vp, _u64, _vp]),
    "mk_hash_batch": (_int, [_cp, _vp, _u64, _u32, _vp]),
    "mk_hash_batch_var": (_int, [_cp, _vp, _vp, _u64, _vp]),
    "mk_dev_hash_batch": (_int, [_cp, _vp, _u64, _u32, _vp, _vp]),
    "mk_dev_hash_batch_var": (_int, [_cp, _vp, _vp, _u64, _vp, _vp]),
    "mk_ssz_merkle_hash": (_int, [_cp, _vp, _u64, _u32, _vp]),
    "mk_ssz_merkle_workspace_bytes": (_u64, [_u64, _u32]),
    "mk_dev_ssz_merkle_hash": (_int, [_cp, _vp, _u64, _u32, _vp, _vp, _u64, _vp]),
    "mk_ssz_tree_hash_bytes_list_workspace_bytes": (_u64, [_u64, _u32]),
    "mk_dev_ssz_tree_hash_bytes_list": (_int, [_cp, _vp, _u64, _u32, _vp, _vp, _u64, _vp]),
    "mk_ssz_tree_hash_bytes_list": (_int, [_cp, _vp, _u64, _u32, _vp]),
    "mk_ssz_merkle_many_workspace_bytes": (_u64, [_vp, _vp, _u32]),
    "mk_dev_ssz_merkle_many": (_int, [_cp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _u64, _vp]),
    "mk_ssz_merkle_many": (_int, [_cp, _vp, _vp, _vp, _vp, _u32, _vp]),
    "mk_ssz_merkle_shard_plan": (_int, [_cp, _u64, _u32, _u32, _vp, _vp, _vp]),
    "mk_dev_ssz_merkle_subtree": (_int, [_cp, _vp, _u64, _u32, _u32, _int, _vp, _vp, _u64, _vp]),
    "mk_dev_ssz_merkle_finish": (_int, [_cp, _vp, _u64, _u64, _vp, _vp]),
    "mk_dev_ssz_merkle_subtree_frontier": (_int, [_cp, _vp, _u64, _u32, _u32, _u32, _int, _vp, _vp, _vp, _u64,
                                                  _vp]),
    "mk_ssz_merkle_node_frontier_workspace_bytes": (_u64, [_u64, _u32, _u32]),
    "mk_dev_ssz_merkle_node_frontier": (_int, [_cp, _vp, _u64, _u32, _u32, _int, _vp, _vp, _vp, _u64, _vp]),
    "mk_ssz_merkle_finish_workspace_bytes": (_u64, [_u64]),
    "mk_dev_ssz_merkle_finish_nodes": (_int, [_cp, _vp, _u64, _u64, _vp, _vp, _u64, _vp]),
    "mk_dev_ssz_merkle_finish_nodes_pair": (_int, [_cp, _vp, _u64, _u64, _vp, _u32, _u32, _vp, _u64, _vp]),
    "mk_ssz_merkle_top_fused_workspace_bytes": (_u64, [_u64, _u64]),
    "mk_dev_ssz_merkle_top_fused": (_int, [_cp, _vp, _u64, _u64, _vp, _u64, _u64, _vp, _u32, _vp, _u64, _vp]),
    "mk_ssz_merkle_hash_multi": (_int, [_cp, _vp, _u64, _u32, _int, _vp, _vp]),
    "mk_dev_ssz_merkle_hash_multi": (_int, [_cp, _vp, _u64, _u32, _int, _vp, _vp]),
    "mk_ssz_struct_msg_len": (_u64, [_vp, _u32]),
    "mk_ssz_struct_roots": (_int, [_cp, _vp, _u64, _u32, _vp, _u32, _vp]),
    "mk_ssz_struct_list_workspace_bytes": (_u64, [_u64, _vp, _u32]),
    "mk_dev_ssz_struct_list_root": (_int, [_cp, _vp, _u64, _u32, _vp, _u32, _vp, _vp, _u64, _vp]),
    "mk_dev_ssz_struct_roots": (_int, [_cp, _vp, _u64, _u32, _vp, _u32, _vp, _vp, _u64, _vp]),
    "mk_ssz_struct_list_level1_ok": (_int, [_vp, _u64, _u32, _vp, _u32]),
    "mk_dev_ssz_struct_list_level1": (_int, [_cp, _vp, _u64, _u32, _vp, _u32, _vp, _vp, _vp, _u64, _u32, _vp, _vp]),
    "mk_ssz_struct_pipe_ok": (_int, [_vp, _u64, _u32, _vp, _u32, _vp]),
    "mk_ssz_struct_pipe_levels_bytes": (_u64, [_u64, _u64, _u32, _u32]),
    "mk_ssz_struct_pipe_top_workspace_bytes": (_u64, [_u64, _u64, _u32, _u32]),
    "mk_dev_ssz_struct_list_level1_pipe": (_int, [_cp, _vp, _u64, _u32, _vp, _u32, _vp, _vp, _vp, _u64, _u32, _vp,
                                                  _vp, _vp, _vp, _vp, _vp]),
    "mk_dev_ssz_struct_pipe_top": (_int, [_cp, _vp, _u64, _u64, _u32, _u32, _vp, _vp, _u32, _u32, _vp, _u64, _vp]),
    "mk_ssz_struct_list_root": (_int, [_cp, _vp, _u64, _u32, _vp, _u32, _vp]),
    "mk_merkle_root": (_int, [_cp, _vp, _vp, _u64, _vp, _vp]),
    "mk_merkle_root_workspace_bytes": (_u64, [_u64]),
    "mk_dev_merkle_root": (_int, [_cp, _vp, _vp, _u64, _u32, _vp, _u64, _vp, _vp, _vp]),
    "mk_deposit_trie_levels_bytes": (_u64, [_u64, _u32]),
    "mk_deposit_trie_build": (_int, [_cp, _vp, _vp, _u64, _u32, _vp, _vp]),
    "mk_dev_deposit_trie_append": (_int, [_cp, _vp, _u64, _u64, _vp, _vp, _u64, _u32, _u32, _vp, _vp]),
    "mk_dev_deposit_trie_branch": (_int, [_cp, _vp, _u64, _u64, _u32, _u64, _vp, _vp]),
    "mk_deposit_trie_pipe_ok": (_int, [_vp, _u64, _u32, _u32, _vp]),
    "mk_dev_deposit_trie_build_pipe": (_int, [_cp, _vp, _vp, _u64, _vp, _u64, _u32, _u32, _vp]),
    "mk_dev_deposit_trie_pipe_top": (_int, [_cp, _vp, _u64, _u64, _u32, _vp, _vp]),
    "mk_dev_deposit_trie_levels": (_int, [_cp, _vp, _u64, _u64, _u32, _u32, _u32, _vp, _vp]),
    "mk_dev_deposit_trie_build": (_int, [_cp, _vp, _u64, _vp, _vp, _u64, _u32, _u32, _u32, _vp, _vp]),
    "mk_deposit_trie_new": (_int, [_cp, _u32, _u64, _vp]),
    "mk_deposit_trie_free": (None, [_vp]),
    "mk_deposit_trie_count": (_u64, [_vp]),
    "mk_deposit_trie_append": (_int, [_cp, _vp, _vp, _vp, _u64]),
    "mk_deposit_trie_save_logs": (_int, [_cp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "mk_deposit_trie_root": (_int, [_cp, _vp, _vp]),
    "mk_deposit_trie_branch": (_int, [_cp, _vp, _u64, _vp]),
    "mk_deposit_trie_leaves": (_int, [_cp, _vp, _u64, _u64, _vp]),
    "mk_dev_deposit_trie_branches": (_int, [_cp, _vp, _u64, _u64, _u32, _u64, _vp, _u64, _vp, _vp, _vp]),
    "mk_deposit_trie_branches": (_int, [_cp, _vp, _u64, _vp, _u64, _vp, _vp]),
    "mk_deposit_trie_root_at": (_int, [_cp, _vp, _u64, _vp]),
    "mk_dev_deposit_trie_truncate": (_int, [_cp, _vp, _u64, _u64, _u64, _u32, _vp, _vp]),
    "mk_dev_deposit_trie_fork_point": (_int, [_cp, _vp, _u64, _u64, _vp, _u64, _u64, _u32, _vp, _vp]),
    "mk_dev_deposit_trie_audit": (_int, [_cp, _vp, _u64, _u64, _u32, _vp, _vp, _vp]),
    "mk_dev_deposit_trie_copy": (_int, [_cp, _vp, _u64, _u64, _vp, _u64, _u32, _vp, _vp, _vp]),
    "mk_deposit_trie_truncate": (_int, [_cp, _vp, _u64]),
    "mk_deposit_trie_fork_point": (_int, [_cp, _vp, _vp, _vp]),
    "mk_deposit_trie_audit": (_int, [_cp, _vp, _vp]),
    "mk_deposit_trie_clone": (_int, [_cp, _vp, _vp]),
    "mk_deposit_trie_copy": (_int, [_cp, _vp, _vp]),
    "mk_deposit_trie_reserve": (_int, [_cp, _vp, _u64]),
    "mk_deposit_trie_capacity": (_u64, [_vp]),
    "mk_dev_verify_deposits": (_int, [_cp, _vp, _vp, _vp, _vp, _u64, _u32, _u32, _vp, _u32, _vp, _vp]),
    "mk_verify_deposits": (_int, [_cp, _vp, _vp, _vp, _vp, _u64, _u32, _u32, _vp, _u32, _vp]),
    "mk_ssz_list_tree_levels_bytes": (_u64, [_u64, _u32]),
    "mk_ssz_list_tree_build_workspace_bytes": (_u64, [_u64, _u32]),
    "mk_dev_ssz_list_tree_build": (_int, [_cp, _vp, _u64, _u64, _u32, _vp, _vp, _vp, _u64, _vp]),
    "mk_ssz_list_tree_update_workspace_bytes": (_u64, [_u64]),
    "mk_dev_ssz_list_tree_update": (_int, [_cp, _vp, _u64, _u64, _u64, _u32, _vp, _vp, _u64, _vp, _vp, _vp, _u64,
                                           _vp]),
    "mk_ssz_list_tree_erase_workspace_bytes": (_u64, [_u64, _u32]),
    "mk_dev_ssz_list_tree_erase": (_int, [_cp, _vp, _u64, _u64, _u64, _u32, _vp, _vp, _u64, _u64, _vp, _vp, _u64,
                                          _vp]),
    "mk_list_tree_new": (_int, [_cp, _u32, _u64, _vp]),
    "mk_list_tree_free": (None, [_vp]),
    "mk_list_tree_count": (_u64, [_vp]),
    "mk_list_tree_assign": (_int, [_cp, _vp, _vp, _u64]),
    "mk_list_tree_update": (_int, [_cp, _vp, _vp, _vp, _u64]),
    "mk_list_tree_append": (_int, [_cp, _vp, _vp, _u64]),
    "mk_list_tree_truncate": (_int, [_cp, _vp, _u64]),
    "mk_list_tree_erase": (_int, [_cp, _vp, _vp, _u64]),
    "mk_list_tree_root": (_int, [_cp, _vp, _vp]),
    "mk_list_tree_items": (_int, [_cp, _vp, _u64, _u64, _vp]),
    "mk_ssz_struct_list_tree_build_workspace_bytes": (_u64, [_u64, _vp, _u32]),
    "mk_dev_ssz_struct_list_tree_build": (_int, [_cp, _vp, _u64, _u64, _u32, _vp, _u32, _vp, _vp, _vp, _vp, _u64,
                                                 _vp]),
    "mk_ssz_struct_list_tree_update_workspace_bytes": (_u64, [_u64, _vp, _u32]),
    "mk_dev_ssz_struct_list_tree_update": (_int, [_cp, _vp, _u64, _u64, _u64, _u32, _vp, _u32, _vp, _vp, _vp, _u64,
                                                  _vp, _vp, _vp, _u64, _vp]),
    "mk_ssz_struct_list_tree_erase_workspace_bytes": (_u64, [_u64, _u32]),
    "mk_dev_ssz_struct_list_tree_erase": (_int, [_cp, _vp, _u64, _u64, _u64, _u32, _vp, _u32, _vp, _vp, _vp, _u64,
                                                 _u64, _vp, _vp, _u64, _vp]),
    "mk_struct_list_tree_new": (_int, [_cp, _u32, _vp, _u32, _u64, _vp]),
    "mk_struct_list_tree_free": (None, [_vp]),
    "mk_struct_list_tree_count": (_u64, [_vp]),
    "mk_struct_list_tree_assign": (_int, [_cp, _vp, _vp, _u64]),
    "mk_struct_list_tree_update": (_int, [_cp, _vp, _vp, _vp, _u64]),
    "mk_struct_list_tree_append": (_int, [_cp, _vp, _vp, _u64]),
    "mk_struct_list_tree_truncate": (_int, [_cp, _vp, _u64]),
    "mk_struct_list_tree_erase": (_int, [_cp, _vp, _vp, _u64]),
    "mk_struct_list_tree_root": (_int, [_cp, _vp, _vp]),
    "mk_struct_list_tree_records": (_int, [_cp, _vp, _u64, _u64, _vp]),
    "mk_ssz_bytes_list_tree_build_workspace_bytes": (_u64, [_u64, _u32]),
    "mk_dev_ssz_bytes_list_tree_build": (_int, [_cp, _vp, _u64, _u64, _u32, _vp, _vp, _vp, _vp, _u64, _vp]),
    "mk_ssz_bytes_list_tree_update_workspace_bytes": (_u64, [_u64, _u32]),
    "mk_dev_ssz_bytes_list_tree_update": (_int, [_cp, _vp, _u64, _u64, _u64, _u32, _vp, _vp, _vp, _u64, _vp, _vp,
                                                 _vp, _u64, _vp]),
    "mk_ssz_bytes_list_tree_erase_workspace_bytes": (_u64, [_u64, _u32]),
    "mk_dev_ssz_bytes_list_tree_erase": (_int, [_cp, _vp, _u64, _u64, _u64, _u32, _vp, _vp, _vp, _u64, _u64, _vp,
                                                _vp, _u64, _vp]),
    "mk_bytes_list_tree_new": (_int, [_cp, _u32, _u64, _vp]),
    "mk_bytes_list_tree_free": (None, [_vp]),
    "mk_bytes_list_tree_count": (_u64, [_vp]),
    "mk_bytes_list_tree_assign": (_int, [_cp, _vp, _vp, _u64]),
    "mk_bytes_list_tree_update": (_int, [_cp, _vp, _vp, _vp, _u64]),
    "mk_bytes_list_tree_append": (_int, [_cp, _vp, _vp, _u64]),
    "mk_bytes_list_tree_truncate": (_int, [_cp, _vp, _u64]),
    "mk_bytes_list_tree_erase": (_int, [_cp, _vp, _vp, _u64]),
    "mk_bytes_list_tree_root": (_int, [_cp, _vp, _vp]),
    "mk_bytes_list_tree_elems": (_int, [_cp, _vp, _u64, _u64, _vp]),
    "mk_ssz_trees_update_workspace_bytes": (_u64, [_vp, _u32]),
    "mk_dev_ssz_trees_update": (_int, [_cp, _vp, _u32, _vp, _u32, _vp, _vp, _u64, _vp]),
    "mk_tree_set_new": (_int, [_cp, _u32, _vp]),
    "mk_tree_set_free": (None, [_vp]),
    "mk_tree_set_add": (_int, [_cp, _vp, _u32, _u32, _vp, _u32, _u64, _u32, _vp]),
    "mk_tree_set_put": (_int, [_cp, _vp, _u32, _vp, _u32]),
    "mk_tree_set_assign": (_int, [_cp, _vp, _u32, _vp, _u64]),
    "mk_tree_set_update": (_int, [_cp, _vp, _u32, _vp, _vp, _u64]),
    "mk_tree_set_append": (_int, [_cp, _vp, _u32, _vp, _u64]),
    "mk_tree_set_truncate": (_int, [_cp, _vp, _u32, _u64]),
    "mk_tree_set_erase": (_int, [_cp, _vp, _u32, _vp, _u64]),
    "mk_tree_set_count": (_u64, [_vp, _u32]),
    "mk_tree_set_root": (_int, [_cp, _vp, _vp]),
    "mk_tree_set_tree_root": (_int, [_cp, _vp, _u32, _vp]),
    "mk_tree_set_items": (_int, [_cp, _vp, _u32, _u64, _u64, _vp]),
    "mk_ssz_list_branch_bytes": (_u64, [_u64, _u32]),
    "mk_dev_ssz_list_tree_branches": (_int, [_cp, _vp, _u64, _u64, _u32, _vp, _vp, _u64, _vp, _vp]),
    "mk_dev_verify_list_branches": (_int, [_cp, _vp, _vp, _u64, _u64, _u32, _vp, _vp, _u32, _vp, _u32, _u32, _vp,
                                           _vp]),
    "mk_verify_list_branches": (_int, [_cp, _vp, _vp, _u64, _u64, _u32, _vp, _vp, _u32, _vp, _u32, _u32, _vp]),
    "mk_list_tree_branches": (_int, [_cp, _vp, _vp, _u64, _vp, _vp]),
    "mk_struct_list_tree_branches": (_int, [_cp, _vp, _vp, _u64, _vp, _vp]),
    "mk_bytes_list_tree_branches": (_int, [_cp, _vp, _vp, _u64, _vp, _vp]),
    "mk_tree_set_branches": (_int, [_cp, _vp, _u32, _vp, _u64, _vp, _vp, _vp]),
    "mk_dev_ssz_trees_copy": (_int, [_cp, _vp, _u32, _vp, _vp, _vp]),
    "mk_list_tree_clone": (_int, [_cp, _vp, _vp]),
    "mk_list_tree_copy": (_int, [_cp, _vp, _vp]),
    "mk_list_tree_reserve": (_int, [_cp, _vp, _u64]),
    "mk_list_tree_capacity": (_u64, [_vp]),
    "mk_struct_list_tree_clone": (_int, [_cp, _vp, _vp]),
    "mk_struct_list_tree_copy": (_int, [_cp, _vp, _vp]),
    "mk_struct_list_tree_reserve": (_int, [_cp, _vp, _u64]),
    "mk_struct_list_tree_capacity": (_u64, [_vp]),
    "mk_bytes_list_tree_clone": (_int, [_cp, _vp, _vp]),
    "mk_bytes_list_tree_copy": (_int, [_cp, _vp, _vp]),
    "mk_bytes_list_tree_reserve": (_int, [_cp, _vp, _u64]),
    "mk_bytes_list_tree_capacity": (_u64, [_vp]),
    "mk_tree_set_clone": (_int, [_cp, _vp, _vp]),
    "mk_tree_set_copy": (_int, [_cp, _vp, _vp]),
    "mk_tree_set_reserve": (_int, [_cp, _vp, _u32, _u64]),
    "mk_tree_set_capacity": (_u64, [_vp, _u32]),
    "mk_ssz_trees_journal_bytes": (_u64, [_vp, _u32, _u32]),
    "mk_dev_ssz_trees_journal": (_int, [_cp, _vp, _u32, _vp, _u32, _vp, _vp, _u64, _vp]),
    "mk_dev_ssz_trees_restore": (_int, [_cp, _vp, _u32, _vp, _u32, _vp, _vp, _u64, _vp]),
    "mk_tree_set_checkpoint": (_int, [_cp, _vp, _vp]),
    "mk_tree_set_rollback": (_int, [_cp, _vp, _u64]),
    "mk_tree_set_release": (_int, [_cp, _vp, _u64]),
    "mk_tree_set_journal_bytes": (_u64, [_vp]),
    "mk_tree_set_journal_capacity": (_u64, [_vp]),
    "mk_tree_set_journal_reserve": (_int, [_cp, _vp, _u64]),
    "mk_ssz_trees_audit_workspace_bytes": (_u64, [_vp, _u32]),
    "mk_dev_ssz_trees_audit": (_int, [_cp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _u64, _vp]),
    "mk_list_tree_audit": (_int, [_cp, _vp, _vp]),
    "mk_struct_list_tree_audit": (_int, [_cp, _vp, _vp]),
    "mk_bytes_list_tree_audit": (_int, [_cp, _vp, _vp]),
    "mk_tree_set_audit": (_int, [_cp, _vp, _vp]),
    "mk_dev_ssz_trees_diff": (_int, [_cp, _vp, _u32, _vp, _vp]),
    "mk_list_tree_diff": (_int, [_cp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "mk_struct_list_tree_diff": (_int, [_cp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "mk_bytes_list_tree_diff": (_int, [_cp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "mk_tree_set_diff": (_int, [_cp, _vp, _vp, _vp, _vp, _u64]),
    "mk_dev_repeat_hash": (_int, [_cp, _vp, _vp, _u64, _u32, _u32, _vp, _vp, _vp]),
    "mk_dev_hash_onion": (_int, [_cp, _vp, _u64, _u32, _u32, _vp, _vp]),
    "mk_dev_verify_repeat_hash": (_int, [_cp, _vp, _u64, _u64, _u32, _u32, _vp, _vp, _u64, _u32, _u32, _vp, _vp]),
    "mk_repeat_hash_batch": (_int, [_cp, _vp, _vp, _u64, _u32, _vp]),
    "mk_repeat_hash": (_int, [_cp, _vp, _u64, _vp]),
    "mk_hash_onion": (_int, [_cp, _vp, _u64, _u32, _vp]),
    "mk_verify_repeat_hash": (_int, [_cp, _vp, _u64, _u64, _u32, _u32, _vp, _vp, _u64, _u32, _vp]),
    "mk_struct_list_tree_verify_repeat_hash": (_int, [_cp, _vp, _u32, _u32, _vp, _vp, _u64, _u32, _vp]),
    "mk_tree_set_verify_repeat_hash": (_int, [_cp, _vp, _u32, _u32, _u32, _vp, _vp, _u64, _u32, _vp]),
    "mk_verify_merkle_branches":(_int, [_cp, _vp, _vp, _vp, _u64, _u32, _u32, _vp, _vp]),
    "mk_dev_synth_fill": (_int, [_cp, _vp, _u64, _u64, _u64, _vp]),
    "mk_prof_enable": (_int, [_int]),
    "mk_prof_read": (_int, [_cp, _vp, _vp, _vp, _vp]),
}

MK_FIELD_BYTES = 1
MK_FIELD_RAW = 2
MK_FIELD_VARBYTES = 3  # le32(L) || L bytes in a slot of 4 + len bytes
MK_FIELD_STRUCT = 4    # a nested struct: len = the entries that follow and belong to it
MK_FIELD_LIST = 5      # le32(count) || len cells; the next entry describes one item, its offset the stride


class Field(ctypes.Structure):
    """mk_field: one field of a fixed-layout record."""
    _fields_ = [("kind", ctypes.c_uint32), ("offset", ctypes.c_uint32), ("len", ctypes.c_uint32)]


MK_TREE_LIST = 1    # mk_dev_ssz_list_tree_update's tree
MK_TREE_STRUCT = 2  # mk_dev_ssz_struct_list_tree_update's tree
MK_TREE_BYTES = 3   # mk_dev_ssz_bytes_list_tree_update's tree
MK_TREES_MAX = 16
MK_NO_CONTAINER = 0xFFFFFFFF
MK_CONTAINER_MAX = 4096
MK_CHECKPOINTS_MAX = 64
# hashutil.RepeatHash in batches: the cap on any call's max_layers, the kernel forms, the verdicts
MK_REPEAT_MAX_LAYERS = 1 << 20
MK_REPEAT_AUTO, MK_REPEAT_LANE, MK_REPEAT_WAVE = 0, 1, 2
MK_REPEAT_BAD, MK_REPEAT_OK, MK_REPEAT_TOO_DEEP, MK_REPEAT_NO_RECORD = 0, 1, 2, 3
# the dirty share from which a resident tree's host handle rebuilds instead of climbing: count / DIV
# (MK_*_TREE_REBUILD_DIV in csrc/list_tree_api.cpp, struct_tree_api.cpp, bytes_tree_api.cpp)
LIST_TREE_REBUILD_DIV = 512
STRUCT_TREE_REBUILD_DIV = 32
BYTES_TREE_REBUILD_DIV = 256


class TreeUpdate(ctypes.Structure):
    """mk_tree_update: one tree of mk_dev_ssz_trees_update."""
    _fields_ = [("kind", _u32), ("item_len", _u32), ("d_items", _vp), ("d_level0", _vp), ("d_levels", _vp),
                ("n_old", _u64), ("n_new", _u64), ("capacity", _u64), ("d_idx", _vp), ("k_idx", _u64),
                ("d_values", _vp), ("fields", _vp), ("nfields", _u32), ("container_off", _u32), ("d_root32", _vp)]


class TreeCopy(ctypes.Structure):
    """mk_tree_copy: one tree of mk_dev_ssz_trees_copy."""
    _fields_ = [("kind", _u32), ("item_len", _u32), ("n", _u64), ("src_capacity", _u64), ("dst_capacity", _u64),
                ("d_src_items", _vp), ("d_src_level0", _vp), ("d_src_levels", _vp), ("d_src_root32", _vp),
                ("d_dst_items", _vp), ("d_dst_level0", _vp), ("d_dst_levels", _vp), ("d_dst_root32", _vp)]


MK_AUDIT_ROOT = 64            # a mismatch's level: the list root
MK_AUDIT_CONTAINER = 65       # ... the container checks (the extra report)
MK_AUDIT_NONE = 0xFFFFFFFF    # no mismatch


class TreeAudit(ctypes.Structure):
    """mk_tree_audit: one tree of mk_dev_ssz_trees_audit."""
    _fields_ = [("kind", _u32), ("item_len", _u32), ("d_items", _vp), ("d_level0", _vp), ("d_levels", _vp),
                ("d_root32", _vp), ("n", _u64), ("capacity", _u64), ("fields", _vp), ("nfields", _u32),
                ("container_off", _u32)]


class AuditReport(ctypes.Structure):
    """mk_audit_report: mismatches and the smallest (level, index) among them."""
    _fields_ = [("bad", _u64), ("first_index", _u64), ("first_level", _u32), ("pad", _u32)]

    def astuple(self):
        return int(self.bad), int(self.first_level), int(self.first_index)


class TreeDiff(ctypes.Structure):
    """mk_tree_diff: one pair of trees of mk_dev_ssz_trees_diff."""
    _fields_ = [("kind", _u32), ("item_len", _u32), ("d_a_items", _vp), ("d_a_level0", _vp), ("d_a_levels", _vp),
                ("d_b_items", _vp), ("d_b_level0", _vp), ("d_b_levels", _vp), ("n_a", _u64), ("capacity_a", _u64),
                ("n_b", _u64), ("capacity_b", _u64), ("d_idx_out", _vp), ("max_out", _u64)]


class DiffReport(ctypes.Structure):
    """mk_diff_report: the number of differing indices and the smallest (2^64 - 1: none)."""
    _fields_ = [("total", _u64), ("first_index", _u64)]

    def astuple(self):
        return int(self.total), int(self.first_index)


_lib = None


def header_symbols():
    """Every mk_* function declared in include/prysm_merkle.h."""
    with open(HEADER) as f:
        txt = f.read()
    return sorted(set(re.findall(r"^\s*(?:int|uint64_t|void|const char\*)\s+(mk_[a-z0-9_]+)\s*\(", txt, re.M)))


def load():
    """Load the HIP library (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    # PRYSM_MERKLE_LIB: another build of the same library (A/B tooling, e.g.
    # prysm_amd/lib/variants/); never a different implementation
    path = os.environ.get("PRYSM_MERKLE_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise MerkleError(MK_ENODEV, f"{path} missing: run __graft_entry__.build() "
                                     "(no CPU fallback exists)")
    L = ctypes.CDLL(path)
    for name, (res, args) in _SIGS.items():
        # an older build named by PRYSM_MERKLE_LIB (a parent commit's, for A/B timing) may lack the newest entries;
        # the shipped library may not (__graft_entry__.build() checks every header symbol)
        if path != LIB_PATH and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(rc: int, what: str = "", call: "Call" = None) -> None:
    """Raise MerkleError for a failed call; the detail comes from the call's
    own context (never from another call on this thread)."""
    if rc != MK_OK:
        L = load()
        detail = call.err.decode(errors="replace") if call is not None else L.mk_last_error().decode(errors="replace")
        raise MerkleError(rc, f"{what}: {L.mk_strerror(rc).decode()}: {detail}")


def invoke(name: str, *args, device: int = -1) -> None:
    """Call entry point `name` with a fresh per-call context (device: -1 =
    the stream's / thread's current device) and raise on failure."""
    call = Call(device, 0, b"")
    rc = getattr(load(), name)(ctypes.byref(call), *args)
    check(rc, name, call)


def device_count() -> int:
    return load().mk_device_count()


def init(device: int = 0) -> None:
    check(load().mk_init(device), "mk_init")
