"""The definition of grb_louvain (include/grb_hip.h) restated on the host in numpy integer arrays: the reference the GPU tests
compare with, bit for bit.  Written from the definition, not from the kernel: a round is a handful of sorts over the
(vertex, neighbouring community) pairs, nothing is parallel and nothing is atomic.

    run(n, rows, cols, weights, max_levels, max_rounds) -> Result

rows / cols / weights are the stored entries of A, each once as stored (both directions of an edge, the diagonal once);
weights are non-negative integers (all ones for weighted = 0).  Not a test module."""
import numpy as np

I64 = np.int64
W_MAX = 2 ** 31 - 1


class Result:
    """labels: the smallest original vertex of every vertex's community.  trace[level] = [(proposals, moves, qn after the
    round), ...], one tuple a round, the round without proposals included.  level_qn[level] = QN of the level's input graph
    under the identity partition, computed on that (contracted) graph."""

    def __init__(self):
        self.labels = None
        self.levels = self.rounds = self.moves = self.proposals = self.communities = 0
        self.qn = self.w = 0
        self.modularity = 0.0
        self.trace = []
        self.level_qn = []


def _first_of_runs(keys):
    """the positions where a run of equal keys begins, in a sorted array"""
    if keys.size == 0:
        return np.zeros(0, dtype=I64)
    return np.flatnonzero(np.concatenate(([True], keys[1:] != keys[:-1])))


def qn_of(n, rows, cols, w, c, W):
    """QN = W * sum_x in(x) - sum_x tot(x)^2 of the partition c, in Python integers"""
    same = c[rows] == c[cols]
    inner = int(w[same].sum())
    k = np.zeros(n, dtype=I64)
    np.add.at(k, rows, w)
    tot = np.zeros(n, dtype=I64)
    np.add.at(tot, c, k)
    return int(W) * inner - sum(int(t) * int(t) for t in tot[tot != 0])


def one_level(n, rows, cols, w, W, max_rounds):
    """c after the level, and its trace"""
    k = np.zeros(n, dtype=I64)
    np.add.at(k, rows, w)
    c = np.arange(n, dtype=I64)
    tot = k.copy()
    off = rows != cols
    r, u, wo = rows[off], cols[off], w[off]
    trace = []
    while True:
        # 1. propose: e(v, x) for every (v, x) with a stored off-diagonal entry from v into community x
        x = c[u]
        key = r * n + x
        order = np.argsort(key, kind="stable")
        ks = key[order]
        heads = _first_of_runs(ks)
        e = np.add.reduceat(wo[order], heads) if heads.size else np.zeros(0, dtype=I64)
        pv, px = ks[heads] // n, ks[heads] % n
        ea = np.zeros(n, dtype=I64)
        own = px == c[pv]
        ea[pv[own]] = e[own]
        stay = W * ea - k * (tot[c] - k)
        gv, gx, ge = pv[~own], px[~own], e[~own]
        gain = W * ge - k[gv] * tot[gx] - stay[gv]
        o2 = np.lexsort((gx, -gain, gv))                 # per v: the largest gain, then the smallest x
        gv, gx, gain = gv[o2], gx[o2], gain[o2]
        h2 = _first_of_runs(gv)
        bv, bd, bg = gv[h2], gx[h2], gain[h2]
        good = bg > 0
        bv, bd, bg = bv[good], bd[good], bg[good]
        if bv.size == 0:
            trace.append((0, 0, qn_of(n, rows, cols, w, c, W)))
            break
        ba = c[bv]
        # 2. claim: both ends of every proposal
        comm = np.concatenate((ba, bd))
        cg = np.concatenate((bg, bg))
        cv = np.concatenate((bv, bv))
        o3 = np.lexsort((cv, -cg, comm))
        h3 = _first_of_runs(comm[o3])
        winner = np.full(n, -1, dtype=I64)
        winner[comm[o3][h3]] = cv[o3][h3]
        K = np.zeros(n, dtype=I64)
        np.add.at(K, bd, k[bv])
        dest = np.full(n, -1, dtype=I64)
        dest[bv] = bd
        # 3. accept
        wd = winner[bd]
        enters = dest[wd] == bd                          # d's winner proposes to enter d
        ok = (winner[ba] == bv) & ((wd == bv) | (enters & (bg > k[bv] * (K[bd] - k[bv]))))
        mv, md, ma = bv[ok], bd[ok], ba[ok]
        # 4. apply
        c[mv] = md
        np.subtract.at(tot, ma, k[mv])
        np.add.at(tot, md, k[mv])
        trace.append((int(bv.size), int(mv.size), qn_of(n, rows, cols, w, c, W)))
        if len(trace) >= max_rounds:
            break
    return c, trace


def contract(n, rows, cols, w, c):
    """map = the rank of c's values; the community graph with loops kept and PLUS"""
    uniq, m = np.unique(c, return_inverse=True)
    m = m.astype(I64)
    nc = int(uniq.size)
    key = m[rows] * nc + m[cols]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    heads = _first_of_runs(ks)
    ws = np.add.reduceat(w[order], heads) if heads.size else np.zeros(0, dtype=I64)
    return nc, ks[heads] // nc, ks[heads] % nc, ws.astype(I64), m


def run(n, rows, cols, weights, max_levels=1 << 30, max_rounds=1 << 30):
    rows = np.asarray(rows, dtype=I64)
    cols = np.asarray(cols, dtype=I64)
    w = np.asarray(weights, dtype=I64)
    assert rows.shape == cols.shape == w.shape and (w >= 0).all()
    W = int(w.sum())
    assert W <= W_MAX
    res = Result()
    res.w = W
    comp = np.arange(n, dtype=I64)                       # the original vertices' vertex of the current level
    if n == 0 or rows.size == 0 or W == 0:
        res.levels = res.rounds = 1
        res.trace = [[(0, 0, 0)]]
        res.level_qn = [0]
        res.communities = n
        res.labels = comp.astype(np.int32)
        return res
    gn, gr, gc, gw = n, rows, cols, w
    while True:
        res.level_qn.append(qn_of(gn, gr, gc, gw, np.arange(gn, dtype=I64), W))
        c, trace = one_level(gn, gr, gc, gw, W, max_rounds)
        res.trace.append(trace)
        res.levels += 1
        res.rounds += len(trace)
        res.proposals += sum(t[0] for t in trace)
        moved = sum(t[1] for t in trace)
        res.moves += moved
        res.qn = trace[-1][2]
        if moved == 0:
            break
        gn, gr, gc, gw, m = contract(gn, gr, gc, gw, c)
        comp = m[comp]
        if res.levels >= max_levels:
            break
    res.communities = gn
    first = np.full(gn, n, dtype=I64)
    np.minimum.at(first, comp, np.arange(n, dtype=I64))
    res.labels = first[comp].astype(np.int32)
    res.modularity = float(res.qn) / (float(W) * float(W))   # the header's expression, as doubles
    return res


def modularity_of(n, rows, cols, weights, labels):
    """Q of any labelling by the same formula (labels: any integers)"""
    rows = np.asarray(rows, dtype=I64)
    cols = np.asarray(cols, dtype=I64)
    w = np.asarray(weights, dtype=I64)
    W = int(w.sum())
    if W == 0:
        return 0.0
    _, c = np.unique(np.asarray(labels), return_inverse=True)
    return qn_of(n, rows, cols, w, c.astype(I64), W) / (W * W)
