"""tests/louvain_model.py, the host restatement of grb_louvain's definition that the GPU tests compare with: QN strictly
increases in every round that moves a vertex, QN is the same number on every contracted level, the labels are a "smallest
member" labelling, and on loop-free unweighted graphs the quality is within a tenth of networkx's Louvain.  No GPU."""
import numpy as np
import pytest

import louvain_model as lm


def _coo(n, edges, loops=()):
    """both directions of every edge once, and the loops"""
    e = sorted({(min(a, b), max(a, b)) for a, b in edges if a != b})
    r = [a for a, b in e] + [b for a, b in e] + list(loops)
    c = [b for a, b in e] + [a for a, b in e] + list(loops)
    return n, np.array(r, dtype=np.int64), np.array(c, dtype=np.int64)


def _ring_of_cliques(cliques, size):
    edges = []
    for q in range(cliques):
        base = q * size
        edges += [(base + i, base + j) for i in range(size) for j in range(i + 1, size)]
        edges.append((base + size - 1, ((q + 1) % cliques) * size))
    return cliques * size, edges


def _grid(h, w):
    edges = [(i * w + j, i * w + j + 1) for i in range(h) for j in range(w - 1)]
    edges += [(i * w + j, (i + 1) * w + j) for i in range(h - 1) for j in range(w)]
    return h * w, edges


def _numpy_inputs():
    rng = np.random.default_rng(11)
    out = {}
    out["ring_of_cliques"] = _ring_of_cliques(8, 5)
    out["grid_12"] = _grid(12, 12)
    out["path_50"] = (50, [(i, i + 1) for i in range(49)])
    out["star_20"] = (21, [(0, i) for i in range(1, 21)])
    out["k33"] = (6, [(i, 3 + j) for i in range(3) for j in range(3)])
    n = 150
    blocks = np.arange(n) // 30
    p = np.where(blocks[:, None] == blocks[None, :], 0.4, 0.02)
    m = np.triu(rng.random((n, n)) < p, 1)
    out["planted"] = (n, list(zip(*np.nonzero(m))))
    # preferential attachment, four edges a new vertex: heavy-tailed, many co-entrants enter one hub (no networkx needed)
    ends, edges = list(range(4)), []
    for v in range(4, 600):
        for u in set(rng.choice(ends, size=4).tolist()):
            edges.append((u, v))
            ends += [u, v]
    out["preferential_600"] = (600, edges)
    return out


INPUTS = _numpy_inputs()


def _weighted_cases():
    """(name, n, rows, cols, weights): the unweighted inputs, and weighted ones with loops and stored zeros"""
    cases = []
    for name, (n, edges) in INPUTS.items():
        n, r, c = _coo(n, edges)
        cases.append((name, n, r, c, np.ones(r.size, dtype=np.int64)))
    rng = np.random.default_rng(5)
    n, edges = INPUTS["planted"]
    n, r, c = _coo(n, edges, loops=range(0, n, 7))
    half = (r.size - len(range(0, n, 7))) // 2
    w = rng.integers(0, 9, size=half)
    cases.append(("planted_weighted_loops", n, r, c, np.concatenate((w, w, rng.integers(0, 5, size=r.size - 2 * half)))))
    return cases


CASES = _weighted_cases()


def _check_trace(n, r, c, w, res):
    """QN strictly increases in every round with a move and is the same number on every contracted level; the record"""
    assert res.levels == len(res.trace) == len(res.level_qn) and res.levels >= 1
    prev = res.level_qn[0]
    assert prev == lm.qn_of(n, r, c, w, np.arange(n, dtype=np.int64), res.w)
    for level, trace in enumerate(res.trace):
        assert res.level_qn[level] == prev, "QN of the contracted graph under the identity partition = QN before the contraction"
        for proposals, moves, qn in trace:
            assert moves <= proposals
            if proposals > 0:
                assert moves >= 1, "the globally best proposal is always accepted"
            if moves > 0:
                assert qn > prev
            else:
                assert qn == prev
            prev = qn
        assert trace[-1][0] == 0, "a level ends with a round without proposals"
    assert res.trace[-1] == [(0, 0, res.qn)], "the call ends with a level that moves nothing"
    assert res.rounds == sum(len(t) for t in res.trace)
    # the record formula on the original graph
    _, comm = np.unique(res.labels, return_inverse=True)
    assert res.qn == lm.qn_of(n, r, c, w, comm.astype(np.int64), res.w)
    assert res.modularity == float(res.qn) / (float(res.w) * float(res.w))
    assert res.communities == np.unique(res.labels).size


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_qn_strictly_increases_and_survives_contraction(case):
    _, n, r, c, w = case
    _check_trace(n, r, c, w, lm.run(n, r, c, w))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_labels_are_the_smallest_members(case):
    _, n, r, c, w = case
    lab = lm.run(n, r, c, w).labels
    assert lab.dtype == np.int32 and lab.shape == (n,)
    assert (lab[lab] == lab).all() and (lab <= np.arange(n)).all()
    for x in np.unique(lab):
        assert np.flatnonzero(lab == x).min() == x


def test_star_ends_in_three_rounds_and_one_community():
    n, r, c = _coo(*INPUTS["star_20"])
    res = lm.run(n, r, c, np.ones(r.size, dtype=np.int64))
    assert res.communities == 1 and (res.labels == 0).all() and res.qn == 0
    assert len(res.trace[0]) == 3


def test_truncation_and_degenerate_inputs():
    n, r, c = _coo(*INPUTS["grid_12"])
    w = np.ones(r.size, dtype=np.int64)
    full = lm.run(n, r, c, w)
    one = lm.run(n, r, c, w, max_levels=1)
    assert one.levels == 1 and one.trace[0] == full.trace[0] and one.qn == full.trace[0][-1][2]
    cut = lm.run(n, r, c, w, max_rounds=1)
    assert all(len(t) == 1 for t in cut.trace) and cut.trace[0][0] == full.trace[0][0]
    for res in (lm.run(0, [], [], []), lm.run(4, [], [], []), lm.run(3, [0, 1], [1, 0], [0, 0])):
        assert (res.levels, res.rounds, res.moves, res.proposals, res.qn) == (1, 1, 0, 0, 0)
        assert (res.labels == np.arange(res.labels.size)).all() and res.modularity == 0.0
    diag = lm.run(3, [0, 1, 2], [0, 1, 2], [2, 0, 5])
    assert (diag.levels, diag.rounds, diag.moves) == (1, 1, 0) and diag.w == 7 and diag.qn == 7 * 7 - (4 + 25)


def _nx_cases():
    nx = pytest.importorskip("networkx")
    return nx, [
        ("karate", lambda: nx.karate_club_graph()),
        ("ring_of_cliques", lambda: nx.ring_of_cliques(8, 5)),
        ("grid_12", lambda: nx.convert_node_labels_to_integers(nx.grid_2d_graph(12, 12))),
        ("path_50", lambda: nx.path_graph(50)),
        ("planted", lambda: nx.planted_partition_graph(6, 30, 0.4, 0.02, seed=3)),
        ("ba_400", lambda: nx.barabasi_albert_graph(400, 4, seed=2)),
        ("gnp_300", lambda: nx.gnp_random_graph(300, 0.03, seed=5)),
        ("ba_3000", lambda: nx.barabasi_albert_graph(3000, 5, seed=2)),
        ("plc_3000", lambda: nx.powerlaw_cluster_graph(3000, 6, 0.3, seed=4)),
        ("grid_40", lambda: nx.convert_node_labels_to_integers(nx.grid_2d_graph(40, 40))),
    ]


NX_NAMES = ["karate", "ring_of_cliques", "grid_12", "path_50", "planted", "ba_400", "gnp_300", "ba_3000", "plc_3000", "grid_40"]


@pytest.mark.parametrize("name", NX_NAMES)
def test_quality_against_networkx(name):
    """the issue's ten graphs, loop-free and unweighted: QN strictly increases in every round with a move and survives every
    contraction (the heavy-tailed ones are where many co-entrants enter one hub), the labels are the smallest members, and
    the model's Q >= 0.9 x Q of louvain_communities(seed=1)"""
    nx, cases = _nx_cases()
    G = dict(cases)[name]()
    n, r, c = _coo(G.number_of_nodes(), list(G.edges()))
    res = lm.run(n, r, c, np.ones(r.size, dtype=np.int64))
    _check_trace(n, r, c, np.ones(r.size, dtype=np.int64), res)
    assert any(moves > 1 for t in res.trace for _, moves, _ in t)
    lab = res.labels
    assert (lab[lab] == lab).all() and (lab <= np.arange(n)).all()
    parts = nx.community.louvain_communities(G, weight=None, seed=1)
    q_nx = nx.community.modularity(G, parts, weight=None)
    lab = np.zeros(n, dtype=np.int64)
    for i, p in enumerate(parts):
        lab[list(p)] = i
    assert abs(lm.modularity_of(n, r, c, np.ones(r.size, dtype=np.int64), lab) - q_nx) < 1e-9, "the same formula"
    print("%s: model Q %.4f, networkx Q %.4f" % (name, res.modularity, q_nx))
    assert res.modularity >= 0.9 * q_nx
