"""The C++ frontend's Louvain driver (include/graphblas/algorithm/louvain.hpp) compiles: float and int A, const and non-const,
a null descriptor, with and without the result record.  And the Python mirror is there: api.louvain with its parameter names
and docstring, _lib's declaration with the argument count of the prototype in include/grb_hip.h, and the header's
grb_louvain_result field for field.  No GPU."""
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
#include "graphblas/algorithm/louvain.hpp"

template <typename A>
static graphblas::Info all(graphblas::Vector<int>* labels, graphblas::Matrix<A>* a, graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<A>* ca = a;
  grb_louvain_result rec;
  Info i = GrB_SUCCESS;
  i = algorithm::louvain(labels, a, 1, 10, 100, desc);                              // non-const A, no record
  i = algorithm::louvain(labels, ca, 0, 10, 100, desc, &rec);                       // const A, the record
  i = algorithm::louvain<A>(labels, ca, 1, 10, 100, desc);                          // the spelled-out template argument
  i = algorithm::louvain(labels, ca, 1, 10, 100, static_cast<Descriptor*>(NULL));   // a null descriptor
  i = algorithm::louvain(labels, a, 1, 1, 1, static_cast<Descriptor*>(NULL), &rec);
  return i == GrB_SUCCESS && rec.qn >= 0 && rec.w >= 0 && rec.moves >= 0 && rec.proposals >= 0 && rec.modularity >= 0. &&
                 rec.levels >= 0 && rec.rounds >= 0 && rec.communities >= 0 && rec.passes >= 0 && rec.launches >= 0 &&
                 rec.loop_ms >= 0.f ? GrB_SUCCESS : i;
}

int main() {
  graphblas::Matrix<float> fa(4, 4);
  graphblas::Matrix<int> ia(4, 4);
  graphblas::Vector<int> labels(4);
  graphblas::Descriptor desc;
  graphblas::Info i = all(&labels, &fa, &desc);
  i = all(&labels, &ia, &desc);
  return i == graphblas::GrB_SUCCESS ? 0 : 1;
}
"""


def _syntax_only(path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_louvain_driver_compiles(tmp_path):
    src = tmp_path / "louvain_frontend.cpp"
    src.write_text(TU)
    _syntax_only(src)


def test_louvain_test_tool_compiles():
    """tests/tools/louvain.cpp, which the GPU suite builds and runs"""
    _syntax_only(os.path.join(ROOT, "tests", "tools", "louvain.cpp"))


def _header():
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        return f.read()


def _prototype_args(name):
    m = re.search(r"grb_info\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m is not None, name
    return len(m.group(1).split(","))


def test_python_mirror_declares_it():
    from graphblast_amd import _lib, api
    import graphblast_amd
    assert callable(getattr(api, "louvain", None)) and graphblast_amd.louvain is api.louvain
    assert list(inspect.signature(api.louvain).parameters) == ["labels", "A", "weighted", "max_levels", "max_rounds", "desc"]
    assert all(p.default is inspect.Parameter.empty for p in inspect.signature(api.louvain).parameters.values())
    doc = api.louvain.__doc__
    assert doc and "grb_louvain" in doc
    for phrase in ("QN = W * sum in(x) - sum tot(x)^2", "the smallest x on a tie", "the smallest v on a tie", "g > k(v) (K(d) - k(v))",
                   "strictly increases QN", "smallest original vertex", "2^31 - 1", "<= 2^24", "labels unchanged on every error",
                   "the same on any number"):
        assert phrase in doc, phrase
    for code in ("GrB_UNINITIALIZED_OBJECT", "GrB_DIMENSION_MISMATCH", "GrB_NOT_IMPLEMENTED", "GrB_INVALID_VALUE", "GrB_INVALID_OBJECT",
                 "GrB_OUT_OF_MEMORY", "GrB_PANIC"):
        assert code in doc, code
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "grb_matrix_eWiseMult" in v)
    assert "grb_louvain" in table
    assert len(table["grb_louvain"]) == _prototype_args("grb_louvain") == 7
    assert table["grb_louvain"][-1] is ctypes.POINTER(_lib.LouvainResult)


C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}


def _record(hdr, name):
    m = re.search(r"typedef struct \{([^{}]*)\} %s;" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S)   # (comments may hold braces)
    assert m is not None, name
    decls = [x.split() for x in m.group(1).split(";") if x.strip()]
    return [d[-1] for d in decls], [d[0] for d in decls]


def test_header_declares_the_result_record():
    """grb_louvain_result, field for field and type for type what the Python mirror reads: 64 bytes"""
    from graphblast_amd import _lib
    hdr = _header()
    fields, types = _record(hdr, "grb_louvain_result")
    assert fields == ["qn", "w", "moves", "proposals", "modularity", "levels", "rounds", "communities", "passes", "launches", "loop_ms"]
    assert types == ["int64_t"] * 4 + ["double"] + ["int32_t"] * 5 + ["float"]
    assert [f[0] for f in _lib.LouvainResult._fields_] == fields
    assert [f[1] for f in _lib.LouvainResult._fields_] == [C_TYPES[t] for t in types]
    assert ctypes.sizeof(_lib.LouvainResult) == 64
    assert re.search(r"\} grb_louvain_result;\s*/\* 64 bytes \*/", hdr)


def test_header_states_the_contract():
    """the definition is in the header: the input rule, QN, the four steps of a round, the levels, the label convention,
    every error, the degenerate successes, and what has not been measured"""
    hdr = re.sub(r"\s*\n \*\s*", " ", _header())
    block = hdr[hdr.index("Louvain community detection (csrc/louvain.hip)"):hdr.index("} grb_louvain_result;")]
    for phrase in ("symmetric structure and values", "weighted = 0 never reads the values", "A stored zero is an entry of weight 0",
                   "a loop of that weight", "W must be <= 2^31 - 1", "QN = W * sum_x in(x) - sum_x tot(x)^2", "invariant under contraction",
                   "1. Propose.", "the smallest x on a tie", "2. Claim.", "the smallest v on a tie", "3. Accept.", "g > k(v) (K(d) - k(v))",
                   "4. Apply.", "A round without proposals ends the level and counts in rounds", "The globally best proposal is always accepted",
                   "grb_contract(G, map, GRB_OP_PLUS, loops = 1)", "the first level that accepted no move",
                   "the smallest original vertex number", "taken on the caller's word", "ONE co-resident launch", "GRB_NUM_CU is honoured",
                   "No floating-point atomics", "nothing is allocated inside a level", "None of the constants has been measured",
                   "The worst case is a path", "(double)qn / ((double)w * (double)w)", "labels keeps what it held",
                   "GRB_UNINITIALIZED_OBJECT", "GRB_DIMENSION_MISMATCH", "GRB_NOT_IMPLEMENTED", "GRB_INVALID_VALUE", "GRB_INVALID_OBJECT",
                   "GRB_OUT_OF_MEMORY", "GRB_PANIC", "labels(v) = v, levels = 1, rounds = 1, qn = 0"):
        assert phrase in block, phrase
