"""The host reference of tests/spmspv_cases.py against the oracle's push product (oracle/ops.py:_spmspv_merge under
mxvmode = 1), which sorts the expanded edges and folds every output sequentially: the 13 commutative semirings, both
types, both orientations, no mask / dense / dense + scmp / sparse, key-value and structure-only, on the patterns S,
E0, E1 and the three degenerate ones.  The data are exact, so the order of a fold is free and the comparison is bit
for bit.  Then the facts every pattern exists for, from the route model, for the large ones too (T: more than 256 scan
tiles, B: more than 256 bitmap tiles, D: more than 2048 chunks), and the model's constants against the headers they
mirror.  No GPU."""
import os
import re

import numpy as np
import pytest

import spmspv_cases as sc
from oracle import ops
from oracle.semiring import Semiring

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphblast_amd", "csrc")


def _oracle(case, A, orient, sr_name, dtype, fval, mask_kind, mask, sparse_mask, scmp, struconly):
    d = ops.Descriptor()
    d.loadArgs(mxvmode=1, struconly=struconly)
    if scmp:
        d.set(ops.GrB_MASK, ops.GrB_SCMP)
    u, w = ops.Vector(case.nrows, dtype), ops.Vector(case.ncols, dtype)
    assert u.build_sparse(case.fidx, fval) == 0
    mk = None
    if mask_kind == "dense":
        mk = ops.Vector(case.ncols, dtype)
        mk.build_dense(mask)
    elif mask_kind == "sparse":
        mk = ops.Vector(case.ncols, dtype)
        assert mk.build_sparse(*sparse_mask) == 0
    sr = Semiring(sr_name, dtype)
    info = ops.vxm(w, mk, None, sr, u, A, d) if orient == "vxm" else ops.mxv(w, mk, None, sr, A, u, d)
    assert info == 0
    assert w.getStorage() == ops.GrB_SPARSE and d.lastmxv_ == ops.GrB_PUSHONLY
    ind, val = w.extractTuples_sparse()
    assert w.nvals() == ind.size
    return ind, val


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=["f32", "i32"])
@pytest.mark.parametrize("name", sc.ORACLE_CASES)
def test_reference_equals_the_oracle(name, dtype):
    case = sc.CASES[name]()
    for sr in sc.COMMUTATIVE:
        (vals, fval, mask, sparse_mask), folded = sc.prepared(case, sr, dtype)
        for orient in sc.ORIENTS:
            nrows, ncols, ptr, ind, v = case.matrix_arrays(orient, vals)
            A = ops.Matrix(nrows, ncols, dtype)
            A.build_csr(ptr, ind, v)
            for mask_name in sc.MASKS:
                mask_kind, scmp = sc.MASK_ARGS[mask_name]
                for struconly in (0, 1):
                    what = (name, sr, dtype.__name__, orient, mask_name, struconly)
                    ref_i, ref_v = _oracle(case, A, orient, sr, dtype, fval, mask_kind, mask, sparse_mask, scmp, struconly)
                    got_i, got_v = sc.want(case, orient, sr, dtype, vals, case.fidx, fval, mask_kind, mask, scmp,
                                           struconly, folded)
                    assert got_i.dtype == ref_i.dtype and np.array_equal(got_i, ref_i), what
                    assert np.all(np.diff(got_i) > 0), what
                    if struconly:
                        assert got_v is None
                    else:
                        assert got_v.dtype == ref_v.dtype and np.array_equal(got_v, ref_v), what
            if case.total == 0:
                assert got_i.size == 0


def test_want_folds_by_itself_what_it_is_given_folded():
    case = sc.small()
    vals, fval, mask, _ = sc.operands(case, "PlusMinus", np.float32)
    a = sc.want(case, "mxv", "PlusMinus", np.float32, vals, case.fidx, fval, "dense", mask, 1, 0)
    b = sc.want(case, "mxv", "PlusMinus", np.float32, vals, case.fidx, fval, "dense", mask, 1, 0,
                sc.fold(case, "PlusMinus", np.float32, vals, fval))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].size


def test_route_facts_of_every_pattern():
    """what the kernels' routes depend on, pattern by pattern (asserted inside the builders too)"""
    f = {name: sc.routes(build()) for name, build in sc.CASES.items()}
    S = f["S"]
    assert (S["scan_tiles"], S["chunks"], S["word_tiles"], S["unstaged"], S["nf"]) == (1, 1, 1, 0, 37)
    for variant, name in enumerate(("E0", "E1")):
        E, case = f[name], sc.CASES[name]()
        assert (case.nrows, case.ncols) == (6000, 20011) and case.ncols % 32 and 4400 <= case.nf <= 5100
        assert E["scan_tiles"] >= 5 and E["word_tiles"] == 3
        assert E["unstaged"] >= 1 and E["zero_tile"]            # a chunk with count > 2048, a scan tile of sum 0
        assert E["total_mod"] == variant and E["total"] // sc.EDGE_CHUNK == 7
        assert E["single_row"] >= 3 and E["tile_edge_staged"] >= 1
        deg = case.deg
        assert deg[0] == 0 and deg[-1] == 0 and np.sort(deg)[-2:].tolist() == [2048, 5000]
        run = np.diff(np.nonzero(np.concatenate([[1], deg, [1]]))[0]) - 1      # lengths of the runs of empty rows
        assert run.max() >= 2500
        hub = int(np.argmax(deg))
        assert case.scan[hub] % sc.EDGE_CHUNK and np.count_nonzero(E["chunk_owner"][:-1] == hub) == 3
        assert np.any((E["count"] == 1) & (E["chunk_owner"][:-1] == hub))          # a whole chunk is the hub's alone
        assert case.scan[int(np.nonzero(deg == 2048)[0][0])] % sc.EDGE_CHUNK == 0
        assert sc.EDGE_CHUNK in case.scan[deg > 0]              # some total of exactly 2048 at a row boundary
    T = f["T"]
    assert T["nf"] >= 300000 and T["scan_tiles"] > 256 and T["scan_carry"] and T["zero_tile"] and T["unstaged"] >= 1
    B = f["B"]
    assert sc.many_bitmap_tiles().ncols == 2200001 and B["word_tiles"] > 256 and B["word_carry"]
    assert B["last_word_bits"] == 1
    D = f["D"]
    assert D["total"] == 2100 * 2100 and D["chunks"] > 2048 and D["past_grid"] and D["single_row"] > 0
    assert (f["Z1"]["nf"], f["Z1"]["total"]) == (1, 1) and (f["Z0"]["nf"], f["Z0"]["total"]) == (1, 0)
    assert f["Zn"]["nf"] > 1 and f["Zn"]["total"] == 0
    # no pattern reaches what is out of scope: the partition kernel's grid loop, a 32-bit total
    assert all(r["chunks"] + 1 <= 1024 * 256 and r["total"] < 2 ** 31 for r in f.values())


def test_operands_hold_what_they_are_for():
    """the identity on both sides for every semiring and type, negative values for the min / max semirings, masks
    with zeros, a zero-prune that really drops entries, MultipliesMultiplies results that are not constant"""
    case = sc.chunk_edges_0()
    for sr in sc.COMMUTATIVE:
        for dtype in sc.DTYPES:
            ident = Semiring(sr, dtype).identity()
            vals, fval, mask, (sm_idx, sm_val) = sc.operands(case, sr, dtype)
            assert np.any(vals == ident) and np.any(fval == ident) and np.any(vals != ident) and np.any(fval != ident)
            if sr.startswith(("Minimum", "Maximum")):
                assert np.any(vals < 0) and np.any(fval < 0)
            assert 0.3 < np.mean(mask == 0) < 0.7 and np.any(mask < 0)
            assert np.all(np.diff(sm_idx) > 0) and np.any(sm_val == 0) and np.any(sm_val != 0)
    vals, fval, mask, _ = sc.operands(case, "PlusMultiplies", np.float32)
    args = (case, "vxm", "PlusMultiplies", np.float32, vals, case.fidx, fval, "dense", mask, 1)
    assert sc.want(*args, 0)[0].size < sc.want(*args, 1)[0].size
    for name in ("E0", "T", "D"):
        case = sc.CASES[name]()
        vals, fval, _, _ = sc.operands(case, "MultipliesMultiplies", np.int32)
        res = sc.want(case, "vxm", "MultipliesMultiplies", np.int32, vals, case.fidx, fval)[1]
        # D: every output takes every frontier value, the 2s among them too: no 1, but several powers of two
        assert np.any(res == 0) and (np.any(res == 1) or name == "D") and np.unique(res).size >= 3, name


def _constant(text, name):
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*([^;]+);" % name, text)
    assert m, name
    return m.group(1).strip()


def test_constants_match_the_headers():
    """a retuned kernel constant fails here instead of silently emptying a route of the GPU tests"""
    with open(os.path.join(CSRC, "common.hpp")) as f:
        common = f.read()
    with open(os.path.join(CSRC, "push_common.hpp")) as f:
        push = f.read()
    kblock = int(_constant(common, "kBlock"))
    assert _constant(push, "kDegTile") == "kBlock * kDegItems" and _constant(push, "kEdgeChunk") == "kBlock * kEdgeItems"
    assert _constant(push, "kSegMax") == "kEdgeChunk"
    assert kblock * int(_constant(push, "kDegItems")) == sc.DEG_TILE
    assert kblock * int(_constant(push, "kEdgeItems")) == sc.EDGE_CHUNK == sc.SEG_MAX
    assert kblock == sc.WORD_TILE == sc.SCAN_BLOCK
    m = re.search(r"egrid\s*=\s*max_chunks\s*<\s*(\d+)\s*\?\s*max_chunks\s*:\s*(\d+)\s*;", push)
    assert m and int(m.group(1)) == int(m.group(2)) == sc.MAX_GRID
    # the partition kernel's grid, which the out-of-scope bound of test_route_facts_of_every_pattern restates
    assert re.search(r"if\s*\(pgrid\s*>\s*1024\)\s*pgrid\s*=\s*1024;", push)
