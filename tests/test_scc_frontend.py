"""The C++ frontend's strongly-connected-components driver (include/graphblas/algorithm/scc.hpp) compiles: float and int A,
const and non-const, a null descriptor, with and without the result record.  And the Python mirror is there: api.scc with
its parameter names and docstring, _lib's declaration with the argument count of the prototype in include/grb_hip.h, and
the header's grb_scc_result field for field.  No GPU."""
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
#include "graphblas/algorithm/scc.hpp"

template <typename A>
static graphblas::Info all(graphblas::Vector<int>* v, graphblas::Matrix<A>* a, graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<A>* ca = a;
  grb_scc_result rec;
  Info i = GrB_SUCCESS;
  i = algorithm::scc(v, a, desc);                                              // non-const A, no record
  i = algorithm::scc(v, ca, desc, &rec);                                       // const A, the record
  i = algorithm::scc<A>(v, ca, desc);                                          // the spelled-out template argument
  i = algorithm::scc(v, ca, static_cast<Descriptor*>(NULL));                   // a null descriptor
  i = algorithm::scc(v, a, static_cast<Descriptor*>(NULL), &rec);
  return i == GrB_SUCCESS && rec.edges >= 0 && rec.components >= 0 && rec.largest >= 0 && rec.trivial >= 0 && rec.trimmed >= 0 &&
                 rec.rounds >= 0 && rec.passes >= 0 && rec.launches >= 0 && rec.loop_ms >= 0.f ? GrB_SUCCESS : i;
}

int main() {
  graphblas::Matrix<float> fa(4, 4);
  graphblas::Matrix<int> ia(4, 4);
  graphblas::Vector<int> v(4);
  graphblas::Descriptor desc;
  graphblas::Info i = all(&v, &fa, &desc);
  i = all(&v, &ia, &desc);
  return i == graphblas::GrB_SUCCESS ? 0 : 1;
}
"""


def _syntax_only(path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_scc_driver_compiles(tmp_path):
    src = tmp_path / "scc_frontend.cpp"
    src.write_text(TU)
    _syntax_only(src)


def test_scc_test_tool_compiles():
    """tests/tools/scc.cpp, which the GPU suite builds and runs"""
    _syntax_only(os.path.join(ROOT, "tests", "tools", "scc.cpp"))


def _prototype_args(name):
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        m = re.search(r"grb_info\s+%s\s*\(([^)]*)\)\s*;" % name, f.read())
    assert m is not None, name
    return len(m.group(1).split(","))


def test_python_mirror_declares_it():
    from graphblast_amd import _lib, api
    import graphblast_amd
    assert callable(getattr(api, "scc", None)) and graphblast_amd.scc is api.scc
    assert list(inspect.signature(api.scc).parameters) == ["v", "A", "desc"]
    assert all(p.default is inspect.Parameter.empty for p in inspect.signature(api.scc).parameters.values())
    doc = api.scc.__doc__
    assert doc and "grb_scc" in doc and "smallest vertex number" in doc
    for code in ("GrB_UNINITIALIZED_OBJECT", "GrB_DIMENSION_MISMATCH", "GrB_NOT_IMPLEMENTED", "GrB_INVALID_OBJECT", "GrB_OUT_OF_MEMORY",
                 "GrB_PANIC"):
        assert code in doc, code
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "grb_matrix_eWiseMult" in v)
    assert "grb_scc" in table
    assert len(table["grb_scc"]) == _prototype_args("grb_scc") == 4
    assert table["grb_scc"][-1] is ctypes.POINTER(_lib.SccResult)


C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def _record(hdr, name):
    m = re.search(r"typedef struct \{([^{}]*)\} %s;" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S)   # (comments may hold braces)
    assert m is not None, name
    decls = [x.split() for x in m.group(1).split(";") if x.strip()]
    return [d[-1] for d in decls], [d[0] for d in decls]


def test_header_declares_the_result_record():
    """grb_scc_result, field for field and type for type what the Python mirror reads: 40 bytes"""
    from graphblast_amd import _lib
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = f.read()
    fields, types = _record(hdr, "grb_scc_result")
    assert fields == ["edges", "components", "largest", "trivial", "trimmed", "rounds", "passes", "launches", "loop_ms"]
    assert types == ["int64_t"] + ["int32_t"] * 7 + ["float"]
    assert [f[0] for f in _lib.SccResult._fields_] == fields
    assert [f[1] for f in _lib.SccResult._fields_] == [C_TYPES[t] for t in types]
    assert ctypes.sizeof(_lib.SccResult) == 40


def test_header_states_the_contract():
    """the definition, in full, is in the header: the graph, the relation, the label, the CSC rule, the errors, the
    working memory, and which fields of the record depend on scheduling"""
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = re.sub(r"\s*\n \*\s*", " ", f.read())
    block = hdr[hdr.index("The strongly connected components (csrc/scc.hip)"):hdr.index("} grb_scc_result;")]
    for phrase in ("A(i, j) stored, i != j", "a directed path runs from u to v and one from v to u, or u = v",
                   "the smallest vertex number in v's component", "same inputs give the same bits", "A and its transpose give the same vector",
                   "Diagonal entries take no part", "a stored zero is an edge", "no descriptor field is read",
                   "the CSR (out-edges) and the CSC (in-edges) are both read","without a CSC of its own", "GRB_INVALID_OBJECT",
                   "GRB_PANIC", "GRB_OUT_OF_MEMORY", "GRB_DIMENSION_MISMATCH", "GRB_NOT_IMPLEMENTED", "GRB_UNINITIALIZED_OBJECT",
                   "bounded spins", "Working memory", "24 bytes per vertex", "quadratic in passes", "connected components, labelled by their smallest member",
                   "n = 0 is a success with a zero record", "components = trivial = n", "largest = 1 when n > 0",
                   "edges, components, largest and trivial are exact", "scc keeps what it held"):
        assert phrase in block, phrase
