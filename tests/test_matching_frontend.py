"""The C++ frontend's matching driver (include/graphblas/algorithm/matching.hpp) compiles: float and int A, const and
non-const, a null descriptor, a null C, with and without the result record.  And the Python mirror is there: api.matching
with its parameter names and docstring, the three mode constants, _lib's declaration with the argument count of the
prototype in include/grb_hip.h, and the header's grb_matching_result field for field.  No GPU."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r"""
#define GRB_USE_CUDA
#include <vector>
#include "graphblas/graphblas.hpp"
#include "graphblas/algorithm/matching.hpp"

template <typename A>
static graphblas::Info all(graphblas::Vector<int>* mate, graphblas::Matrix<A>* c, graphblas::Matrix<A>* a, graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<A>* ca = a;
  grb_matching_result rec;
  Info i = GrB_SUCCESS;
  i = algorithm::matching(mate, c, a, GRB_MATCH_HEAVIEST, 0u, desc);                            // non-const A, no record
  i = algorithm::matching(mate, c, ca, GRB_MATCH_LIGHTEST, 0u, desc, &rec);                     // const A, the record
  i = algorithm::matching<A>(mate, c, ca, GRB_MATCH_HASHED, 7u, desc);                          // the spelled-out template argument
  i = algorithm::matching(mate, c, ca, 0, 0u, static_cast<Descriptor*>(NULL));                  // a null descriptor
  i = algorithm::matching(mate, static_cast<Matrix<A>*>(NULL), a, 2, 1u, desc, &rec);           // a null C
  i = algorithm::matching(mate, static_cast<Matrix<A>*>(NULL), ca, 1, 0u, static_cast<Descriptor*>(NULL), &rec);
  i = algorithm::matching(mate, a, a, 0, 0u, desc);                                             // in place
  return i == GrB_SUCCESS && rec.edges >= 0 && rec.matched >= 0 && rec.weight >= 0. && rec.exposed >= 0 && rec.isolated >= 0 &&
                 rec.rounds >= 0 && rec.passes >= 0 && rec.evaluations >= 0 && rec.launches >= 0 && rec.loop_ms >= 0.f ? GrB_SUCCESS : i;
}

int main() {
  graphblas::Matrix<float> fa(4, 4), fc(4, 4);
  graphblas::Matrix<int> ia(4, 4), ic(4, 4);
  graphblas::Vector<int> mate(4);
  graphblas::Descriptor desc;
  graphblas::Info i = all(&mate, &fc, &fa, &desc);
  i = all(&mate, &ic, &ia, &desc);
  return i == graphblas::GrB_SUCCESS && GRB_MATCH_HEAVIEST == 0 && GRB_MATCH_LIGHTEST == 1 && GRB_MATCH_HASHED == 2 ? 0 : 1;
}
"""


def _syntax_only(path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_matching_driver_compiles(tmp_path):
    src = tmp_path / "matching_frontend.cpp"
    src.write_text(TU)
    _syntax_only(src)


def test_matching_test_tool_compiles():
    """tests/tools/matching.cpp, which the GPU suite builds and runs"""
    _syntax_only(os.path.join(ROOT, "tests", "tools", "matching.cpp"))


def _prototype_args(name):
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        m = re.search(r"grb_info\s+%s\s*\(([^)]*)\)\s*;" % name, f.read())
    assert m is not None, name
    return len(m.group(1).split(","))


def test_python_mirror_declares_it():
    from graphblast_amd import _lib, api
    import graphblast_amd
    assert callable(getattr(api, "matching", None)) and graphblast_amd.matching is api.matching
    assert (api.GRB_MATCH_HEAVIEST, api.GRB_MATCH_LIGHTEST, api.GRB_MATCH_HASHED) == (0, 1, 2)
    assert graphblast_amd.GRB_MATCH_HASHED == 2
    assert list(inspect.signature(api.matching).parameters) == ["mate", "Cm", "A", "mode", "seed", "desc"]
    assert all(p.default is inspect.Parameter.empty for p in inspect.signature(api.matching).parameters.values())
    doc = api.matching.__doc__
    assert doc and "grb_matching" in doc
    for phrase in ("(p, min(u, v), max(u, v))", "-0.0 and +0.0", "greedy scan", "both ends are still free", "maximal", "Cm may be A",
                   "NaN", "mix(mix(min + seed) ^ max)", "0x85ebca6b", "0xc2b2ae35", "or -1", "GRB_MATCH_HEAVIEST = 0",
                   "GRB_MATCH_LIGHTEST = 1", "GRB_MATCH_HASHED = 2", "row of min(u, v)", "exposed", "evaluations"):
        assert phrase in doc, phrase
    for code in ("GrB_UNINITIALIZED_OBJECT", "GrB_DIMENSION_MISMATCH", "GrB_NOT_IMPLEMENTED", "GrB_DOMAIN_MISMATCH", "GrB_INVALID_VALUE",
                 "GrB_OUT_OF_MEMORY", "GrB_PANIC"):
        assert code in doc, code
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "grb_matrix_eWiseMult" in v)
    assert "grb_matching" in table
    assert len(table["grb_matching"]) == _prototype_args("grb_matching") == 7
    assert table["grb_matching"][3] is ctypes.c_int and table["grb_matching"][4] is ctypes.c_uint32
    assert table["grb_matching"][-1] is ctypes.POINTER(_lib.MatchingResult)


C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}


def _record(hdr, name):
    m = re.search(r"typedef struct \{([^{}]*)\} %s;" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S)   # (comments may hold braces)
    assert m is not None, name
    decls = [x.split() for x in m.group(1).split(";") if x.strip()]
    return [d[-1] for d in decls], [d[0] for d in decls]


def test_header_declares_the_result_record():
    """grb_matching_result, field for field and type for type what the Python mirror reads: 56 bytes, as its comment says"""
    from graphblast_amd import _lib
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = f.read()
    fields, types = _record(hdr, "grb_matching_result")
    assert fields == ["edges", "matched", "weight", "exposed", "isolated", "rounds", "passes", "evaluations", "launches", "loop_ms"]
    assert types == ["int64_t", "int64_t", "double"] + ["int32_t"] * 6 + ["float"]
    assert [f[0] for f in _lib.MatchingResult._fields_] == fields
    assert [f[1] for f in _lib.MatchingResult._fields_] == [C_TYPES[t] for t in types]
    assert ctypes.sizeof(_lib.MatchingResult) == 56
    assert re.search(r"\}\s*grb_matching_result;\s*/\*\s*56 bytes\s*\*/", hdr)
    for name, value in (("GRB_MATCH_HEAVIEST", 0), ("GRB_MATCH_LIGHTEST", 1), ("GRB_MATCH_HASHED", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name


def test_header_states_the_contract():
    """the definition, in full, is in the header: the graph, the key and its three kinds, the zeros, NaN, what mate and C
    receive, the symmetry rule, the errors, the bounds on an input taken on the caller's word, and the working memory"""
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = re.sub(r"\s*\n \*\s*", " ", f.read())
    block = hdr[hdr.index("Greedy weighted and maximal matching (csrc/matching.hip)"):hdr.index("} grb_matching_result;")]
    for phrase in ("Diagonal entries take no part", "(p, min(u, v), max(u, v))", "compared lexicographically", "descending weight",
                   "compared as signed integers", "-0.0 and +0.0 are the same weight", "+-inf are allowed",
                   "a NaN off the diagonal is GRB_INVALID_VALUE", "A stored zero or a negative weight is an edge like any other",
                   "the same, ascending", "the values are never compared", "mix(mix(min + seed) ^ max)", "0x85ebca6b", "0xc2b2ae35",
                   "The smaller p goes first", "seed is ignored in the other modes", "keep an edge when both ends are still free",
                   "M is unique, and it is maximal", "at least half the maximum weight matching's", "reproducible from seed",
                   "same inputs give the same bits", "mate(v) = v's partner, or -1", "may be NULL", "at most one entry a row",
                   "from the row of min(u, v)", "The CSC is a copy of the CSR", "C may be A", "no descriptor field is read",
                   "the exact 64-bit integer sum", "no floating-point atomics", "only the CSR is read",
                   "in modes 0 and 1 also values", "compared as bits after -0 has been mapped to +0", "without a CSC of its own",
                   "taken on the caller's word", "bounded by n / 2 + 1", "clamped to n", "bounded spins", "launches is 1 whatever the graph",
                   "locally dominant edge", "enters the list exactly once", "The worst case is equal weights", "Working memory",
                   "24 bytes per vertex", "nothing is proportional to nvals", "both keep what they held", "GRB_UNINITIALIZED_OBJECT",
                   "GRB_DIMENSION_MISMATCH", "GRB_NOT_IMPLEMENTED", "GRB_DOMAIN_MISMATCH", "GRB_INVALID_VALUE", "mode outside 0..2",
                   "GRB_OUT_OF_MEMORY", "GRB_PANIC", "n = 0 is a success with a zero record", "mate = -1 everywhere and an empty C"):
        assert phrase in block, phrase
