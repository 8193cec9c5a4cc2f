"""The host restatement of grb_random_walk and grb_sample_neighbors, written from the definitions in include/grb_hip.h: the
counter-based draw, the walk in both modes with its record, and the sample with its record.  Everything is exact integer
arithmetic; the GPU tests compare with it for equality.  No GPU, no library."""
import numpy as np

U32 = np.uint32
UNIFORM, WEIGHTED = 0, 1
INT32_MAX = 2 ** 31 - 1


def mix(x):
    """the 32-bit finaliser, on a uint32 array or a Python int (unsigned 32-bit arithmetic that wraps)"""
    if isinstance(x, (int, np.integer)):
        x = int(x) & 0xffffffff
        x ^= x >> 16
        x = (x * 0x85ebca6b) & 0xffffffff
        x ^= x >> 13
        x = (x * 0xc2b2ae35) & 0xffffffff
        x ^= x >> 16
        return x
    x = np.asarray(x).astype(np.uint64) & np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85ebca6b)) & np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xc2b2ae35)) & np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(16))
    return x.astype(U32)


def draw(seed, a, b):
    """draw(seed, a, b) = mix(mix(mix((seed + 0x9e3779b9) ^ a) + b) ^ seed); a and b ints or arrays"""
    seed = int(seed) & 0xffffffff
    if isinstance(a, (int, np.integer)) and isinstance(b, (int, np.integer)):
        x = mix(((seed + 0x9e3779b9) & 0xffffffff) ^ (int(a) & 0xffffffff))
        x = mix((x + (int(b) & 0xffffffff)) & 0xffffffff)
        return mix(x ^ seed)
    a, b = np.broadcast_arrays(np.atleast_1d(a), np.atleast_1d(b))
    a = a.astype(np.uint64) & np.uint64(0xffffffff)
    b = b.astype(np.uint64) & np.uint64(0xffffffff)
    x = mix(np.uint64((seed + 0x9e3779b9) & 0xffffffff) ^ a).astype(np.uint64)
    x = mix((x + b) & np.uint64(0xffffffff)).astype(np.uint64)
    return mix(x ^ np.uint64(seed))


def pick(r, m):
    """(uint64(r) * uint64(m)) >> 32: a number in 0 .. m - 1"""
    if isinstance(r, (int, np.integer)) and isinstance(m, (int, np.integer)):
        return (int(r) * int(m)) >> 32
    return ((np.asarray(r).astype(np.uint64) * np.asarray(m).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)


def weights_of(val):
    """the integer weights of stored values under the rule (i32 >= 0; f32 a non-negative integer value <= 2^24, -0.0 = +0.0),
    or None when one of them breaks it"""
    val = np.asarray(val)
    if val.dtype.kind == "f":
        with np.errstate(invalid="ignore"):
            ok = (val >= 0) & (val <= 2.0 ** 24) & (val == np.trunc(val))
        if not ok.all():
            return None
        return val.astype(np.int64)
    if (val < 0).any():
        return None
    return val.astype(np.int64)


class WalkResult:
    def __init__(self, walks, steps, dead_ends, walkers):
        self.walks, self.steps, self.dead_ends, self.walkers = walks, steps, dead_ends, walkers


def walk(ptr, ind, val, starts, length, mode, seed):
    """the walks and the record; None when weighted mode meets a bad weight or a row sum above 2^31 - 1.  starts None: every
    vertex in order.  Vectorised over the walkers, a step at a time."""
    ptr = np.asarray(ptr, np.int64)
    ind = np.asarray(ind, np.int64)
    n = ptr.size - 1
    starts = np.arange(n, dtype=np.int64) if starts is None else np.asarray(starts, np.int64).ravel()
    ns = starts.size
    pre = None
    if mode == WEIGHTED:
        w = weights_of(val)
        if w is None:
            return None
        cs = np.concatenate([[0], np.cumsum(w)])
        pre = cs[1:] - np.repeat(cs[ptr[:-1]], np.diff(ptr))          # the inclusive prefix sum inside the row
        if ((cs[ptr[1:]] - cs[ptr[:-1]]) > INT32_MAX).any():
            return None
        gpre = cs[1:]                                                 # ... and over all entries: ascending, for the search
    out = np.full((ns, length + 1), -1, np.int32)
    if ns == 0:
        return WalkResult(out.ravel(), 0, 0, 0)
    out[:, 0] = starts
    cur = starts.copy()
    alive = np.ones(ns, bool)
    who = np.arange(ns, dtype=np.int64)
    steps = 0
    for t in range(length):
        b, e = ptr[cur], ptr[cur + 1]
        d = e - b
        if mode == WEIGHTED:
            S = np.where(d > 0, cs[e] - cs[b], 0)
            alive &= S > 0
        else:
            alive &= d > 0
        if not alive.any():
            break
        idx = np.flatnonzero(alive)
        r = draw(seed, who[idx], t)
        if mode == WEIGHTED:
            x = pick(r, S[idx])
            # the first entry of the row whose inclusive prefix exceeds x
            p = np.searchsorted(gpre, cs[b[idx]] + x, side="right")
            assert (p >= b[idx]).all() and (p < e[idx]).all() and (pre[p] > x).all()
        else:
            p = b[idx] + pick(r, d[idx])
        cur[idx] = ind[p]
        out[idx, t + 1] = cur[idx]
        steps += idx.size
    reached = (out >= 0).sum(axis=1) - 1
    return WalkResult(out.ravel(), int(steps), int((reached < length).sum()), ns)


class SampleResult:
    def __init__(self, ptr, ind, val, full_rows):
        self.ptr, self.ind, self.val, self.full_rows = ptr, ind, val, full_rows
        self.rows, self.entries = ptr.size - 1, int(ind.size)


def sample(ptr, ind, val, seeds, fanout, seed):
    """C's CSR (pointers, columns, values with A's bits) and the record"""
    ptr = np.asarray(ptr, np.int64)
    ind = np.asarray(ind)
    val = np.asarray(val)
    seeds = np.asarray(seeds if seeds is not None else [], np.int64).ravel()
    optr = np.zeros(seeds.size + 1, np.int64)
    keep_all = []
    full = 0
    for k, row in enumerate(seeds.tolist()):
        b, e = int(ptr[row]), int(ptr[row + 1])
        d = e - b
        if d <= fanout:
            full += 1
            keep = np.arange(b, e)
        else:
            keys = draw(seed, k, np.arange(d, dtype=np.int64))
            assert np.unique(keys).size == d
            keep = b + np.sort(np.argsort(keys, kind="stable")[:fanout])
        keep_all.append(keep)
        optr[k + 1] = optr[k] + keep.size
    at = np.concatenate(keep_all).astype(np.int64) if keep_all else np.zeros(0, np.int64)
    return SampleResult(optr.astype(np.int32), ind[at].astype(np.int32), val[at], full)
