"""The locked leaf pass (k_leaf_lock_sc) with its division-free staging
addresses and the sparse round 0 (keccak_sparse.hpp), bit-exact against
oracle.merkle_hash_flat at the smallest trees that reach it.

One locked group is 4096 windows = 32,768 items of 32 B, and the persistent
grid is 256 workgroups (MK_LOCK_GRID, one per CU).  The planner gives a leaf
pass to k_leaf_lock_sc from 2^20 full windows on (planner.cpp,
MK_LEAF_LOCK_MIN_LOG2 = 20), which is exactly 256 groups, so:

  256 groups  every workgroup runs one group; no next group, so the last
              window's next-region pointer is null and no phase A is issued
  257 groups  workgroup 0 runs two: the pending store of its first node after
              the next wait, and a non-null next region on that group's last
              window
  255 groups  CONTROL ONLY, none of the locked kernel's code runs: one
              below the threshold, so the planner keeps the free-running
              k_reduce for the whole pass.  A locked grid with an idle
              workgroup cannot be reached through the API (the launch is
              min(groups, 256) workgroups and the planner needs >= 256
              groups), so that case has no test

Each thread of a locked group runs 4 x 2 window permutations (the first of
each window starts with round0_block17) and 3 node permutations
(round0_node), the same node round k_node_lock runs."""
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED0000000000C7
GROUP_ITEMS = 32_768
GRID = 256


@pytest.fixture(scope="module")
def gpu():
    import torch

    from prysm_amd import _lib

    assert torch.cuda.is_available()
    _lib.init(0)
    return torch.device("cuda:0")


@pytest.mark.parametrize("ngroups", [GRID - 1, GRID, GRID + 1])
def test_leaf_lock_groups_vs_oracle(gpu, ngroups):
    import torch

    from oracle import oracle as O
    from prysm_amd import device as D

    n = ngroups * GROUP_ITEMS
    items = torch.empty(n * 32, dtype=torch.uint8, device=gpu)
    D.synth_fill(items, SEED + ngroups)
    root = D.merkle_hash(items, n, 32)
    torch.cuda.synchronize()
    want = O.merkle_hash_flat(O.splitmix_bytes(n * 32, SEED + ngroups), n, 32)
    assert bytes(root.cpu().numpy()) == want
