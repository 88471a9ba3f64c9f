"""hashutil.RepeatHash (shared/hashutil/hash.go:29-34) by the oracle: a plain
loop of ``oracle.keccak256_batch(x, 32)``.  The expected values of
tests/test_gpu_repeat_hash.py; pinned by tests/test_repeat_hash_host.py."""
import numpy as np

from oracle import oracle as O


def _rows(seeds) -> np.ndarray:
    return np.ascontiguousarray(seeds, dtype=np.uint8).reshape(-1, 32)


def repeat(x: bytes, k: int) -> bytes:
    """RepeatHash(x, k) of one 32-byte value."""
    return onion(np.frombuffer(bytes(x), dtype=np.uint8), k)[0, k].tobytes()


def onion(seeds, layers: int) -> np.ndarray:
    """(n, layers + 1, 32): row t of chain i is RepeatHash(seeds[i], t)."""
    x = _rows(seeds)
    out = np.empty((x.shape[0], layers + 1, 32), dtype=np.uint8)
    out[:, 0] = x
    for t in range(layers):
        out[:, t + 1] = O.keccak256_batch(np.ascontiguousarray(out[:, t]), 32).reshape(-1, 32)
    return out


def chains(seeds, layers) -> np.ndarray:
    """(n, 32): RepeatHash(seeds[i], layers[i])."""
    x = _rows(seeds)
    lay = np.broadcast_to(np.asarray(layers, dtype=np.int64).reshape(-1), (x.shape[0],))
    on = onion(x, int(lay.max()) if lay.size else 0)
    return on[np.arange(x.shape[0]), lay].copy()


def verify(records: np.ndarray, stride: int, commit_off: int, layers_off: int, idx, reveals, max_layers: int):
    """The verdict bytes of mk_dev_verify_repeat_hash, record by record."""
    rec = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1)
    n_records = rec.size // stride
    rev = _rows(reveals)
    out = []
    for j, r in enumerate(int(i) for i in idx):
        if r >= n_records:
            out.append(3)
            continue
        row = rec[r * stride:(r + 1) * stride]
        cnt = int.from_bytes(row[layers_off:layers_off + 8].tobytes(), "little")
        if cnt > max_layers:
            out.append(2)
            continue
        out.append(int(repeat(rev[j].tobytes(), cnt) == row[commit_off:commit_off + 32].tobytes()))
    return np.array(out, dtype=np.uint8)
