"""numpy restatement of the ID mattes (include/mipt.h pt_set_matte), exact in float32 and uint32, used by tests/test_gpu_matte.py and checked
on its own by tests/test_matte_host.py.

  fix             Cryptomatte's exponent fix of a 32-bit id
  murmur3_32      MurmurHash3_x86_32 in pure Python
  matte_id        fix(murmur3_32(name, 0));  default_id(kind, i) = matte_id of "instance_<i>" / "material_<i>"
  fold_sample     one sample's record into the (ids, cov) ranks of every pixel that hold n samples (through adaptive_ref.blend)
  sort_ranks      non-empty before empty, coverage descending, id ascending as unsigned
  fold_call       a call: its records in sample order, then the sort.  first < 0: the call does not accumulate
  fold            the states after calls of one sample each: entry n - 1 after n samples
  pack / unpack   (ids, cov) <-> the K / 2 float32 layers (H, W, 4) = (id_2j bits, cov_2j, id_2j+1 bits, cov_2j+1)
  extract         the sequential float32 sum over the ranks of the coverages whose id is in a set
"""
import numpy as np

from tests import adaptive_ref as ar

f32, u32 = np.float32, np.uint32
INSTANCE, MATERIAL = 0, 1


def fix(h):
    h = int(h) & 0xffffffff
    e = (h >> 23) & 0xff
    return h ^ (1 << 23) if e in (0, 255) else h


def murmur3_32(data, seed=0):
    data = bytes(data)
    M = 0xffffffff
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & M
    h = seed & M
    n = len(data) // 4
    for i in range(n):
        k = int.from_bytes(data[4 * i:4 * i + 4], "little")
        k = (k * 0xcc9e2d51) & M; k = rotl(k, 15); k = (k * 0x1b873593) & M
        h ^= k; h = rotl(h, 13); h = (h * 5 + 0xe6546b64) & M
    tail = data[4 * n:]
    if tail:
        k = int.from_bytes(tail, "little")
        k = (k * 0xcc9e2d51) & M; k = rotl(k, 15); k = (k * 0x1b873593) & M
        h ^= k
    h ^= len(data)
    h ^= h >> 16; h = (h * 0x85ebca6b) & M; h ^= h >> 13; h = (h * 0xc2b2ae35) & M; h ^= h >> 16
    return h


def matte_id(name):
    return fix(murmur3_32(name.encode() if isinstance(name, str) else name, 0))


def default_id(kind, i):
    return matte_id(("material_%d" if kind == MATERIAL else "instance_%d") % i)


def id_table(kind, rows, user_ids=()):
    """The id of every table row: fix(user_ids[i]) for the rows the caller named, the default names' ids for the rest."""
    return np.array([fix(user_ids[i]) if i < len(user_ids) else default_id(kind, i) for i in range(rows)], u32)


def empty_state(shape, K):
    return np.zeros(tuple(shape) + (K,), u32), np.zeros(tuple(shape) + (K,), f32)


def _blend(c, n, x):
    """c + (1 / (n + 1)) * (x - c) on every rank, three at a time through adaptive_ref.blend (the AOVs' and the output's running mean)."""
    out = np.empty_like(c)
    for g in range(0, c.shape[-1], 3):
        w = min(3, c.shape[-1] - g)
        h4 = np.zeros(c.shape[:-1] + (4,), f32); L = np.zeros(c.shape[:-1] + (3,), f32)
        h4[..., :w] = c[..., g:g + w]; L[..., :w] = x[..., g:g + w]
        out[..., g:g + w] = ar.blend(h4, n, L)[..., :w]
    return out


def fold_sample(ids, cov, h, n):
    """ids, cov: (..., K); h: (...) uint32 records (0 = miss); n: samples already in the state.  Returns the new, unsorted state."""
    ids, cov, h = np.asarray(ids, u32), np.asarray(cov, f32), np.asarray(h, u32)
    K = ids.shape[-1]
    if n == 0:
        ids2, cov2 = empty_state(h.shape, K)
        ids2[..., 0] = h
        cov2[..., 0] = np.where(h != 0, f32(1), f32(0))
        return ids2, cov2
    b = f32(1.0) / f32(n + 1)
    nonempty = ids != 0
    holds = nonempty & (ids == h[..., None]) & (h[..., None] != 0)
    cov2 = np.where(nonempty, _blend(cov, n, holds.astype(f32)), cov).astype(f32)
    ids2 = ids.copy()
    place = (h != 0) & ~holds.any(axis=-1) & (~nonempty).any(axis=-1)      # no empty rank: the id is dropped
    where = np.argmax(~nonempty, axis=-1)                                  # an empty rank (they are all alike)
    idx = np.nonzero(place)
    ids2[idx + (where[idx],)] = h[idx]
    cov2[idx + (where[idx],)] = b
    return ids2, cov2


def sort_ranks(ids, cov):
    ids, cov = np.asarray(ids, u32), np.asarray(cov, f32)
    assert np.all(cov >= 0) and np.all(np.isfinite(cov))
    covbits = cov.view(u32).astype(np.int64)                               # monotone in the value for non-negative floats
    order = np.lexsort((ids.astype(np.int64), -covbits, (ids == 0).astype(np.int64)), axis=-1)     # the last key is the first criterion
    return np.take_along_axis(ids, order, axis=-1), np.take_along_axis(cov, order, axis=-1)


def fold_call(ids, cov, records, first):
    """One pt_trace: records[k] = the (...) uint32 records of the call's sample k; first = the samples already in the state, or < 0 for a
    call without FLAG_ACCUMULATE (every sample is then the first)."""
    for k, h in enumerate(records):
        ids, cov = fold_sample(ids, cov, h, 0 if first < 0 else first + k)
    return sort_ranks(ids, cov)


def fold(records, K):
    """The states after 1, 2, ... samples traced one call each: a list of (ids, cov)."""
    out = []
    ids, cov = empty_state(np.asarray(records[0]).shape, K)
    for n, h in enumerate(records):
        ids, cov = fold_call(ids, cov, [h], n)
        out.append((ids.copy(), cov.copy()))
    return out


def pack(ids, cov):
    """The K / 2 layers (..., 4) float32 of a state."""
    K = ids.shape[-1]
    layers = []
    for j in range(K // 2):
        l = np.zeros(ids.shape[:-1] + (4,), u32)
        l[..., 0] = ids[..., 2 * j]; l[..., 1] = cov[..., 2 * j].view(u32); l[..., 2] = ids[..., 2 * j + 1]; l[..., 3] = cov[..., 2 * j + 1].view(u32)
        layers.append(l.view(f32))
    return layers


def unpack(layers):
    ids = np.stack([np.ascontiguousarray(l, f32).view(u32)[..., c] for l in layers for c in (0, 2)], axis=-1)
    cov = np.stack([np.ascontiguousarray(l, f32)[..., c] for l in layers for c in (1, 3)], axis=-1)
    return ids, cov


def extract(ids, cov, id_set):
    """mask = ((0 + cov_r0) + cov_r1) + ... over the ranks, in rank order, whose id is among fix(id_set)."""
    want = np.array([fix(i) for i in id_set], u32)
    mask = np.zeros(ids.shape[:-1], f32)
    for r in range(ids.shape[-1]):
        hit = np.isin(ids[..., r], want)
        mask = np.where(hit, mask + cov[..., r], mask).astype(f32)
    return mask
