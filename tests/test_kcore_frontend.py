"""The C++ frontend's k-core drivers (include/graphblas/algorithm/kcore.hpp) compile: float and int A, const and
non-const, a null descriptor, with and without the result record.  And the Python mirror is there: api.coreness and
api.kcore with their parameter names and docstrings, _lib's declarations with the argument counts of the prototypes in
include/grb_hip.h, and the header's grb_kcore_result field for field.  No GPU."""
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
#include "graphblas/algorithm/kcore.hpp"

template <typename A>
static graphblas::Info all(graphblas::Vector<int>* v, graphblas::Matrix<A>* a, graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<A>* ca = a;
  grb_kcore_result rec;
  Info i = GrB_SUCCESS;
  i = algorithm::coreness(v, a, desc);                                         // non-const A, no record
  i = algorithm::coreness(v, ca, desc, &rec);                                  // const A, the record
  i = algorithm::coreness<A>(v, ca, desc);                                     // the spelled-out template argument
  i = algorithm::coreness(v, ca, static_cast<Descriptor*>(NULL));              // a null descriptor
  i = algorithm::coreness(v, a, static_cast<Descriptor*>(NULL), &rec);
  i = algorithm::kcore(v, a, 3, desc);
  i = algorithm::kcore(v, ca, 0, desc, &rec);
  i = algorithm::kcore<A>(v, ca, 2, desc);
  i = algorithm::kcore(v, ca, 1, static_cast<Descriptor*>(NULL));
  i = algorithm::kcore(v, a, 1, static_cast<Descriptor*>(NULL), &rec);
  return i == GrB_SUCCESS && rec.edges >= 0 && rec.result_edges >= 0 && rec.kmax >= 0 && rec.levels >= 0 && rec.result_vertices >= 0 &&
                 rec.rounds >= 0 && rec.launches >= 0 && rec.loop_ms >= 0.f ? GrB_SUCCESS : i;
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


def test_kcore_drivers_compile(tmp_path):
    src = tmp_path / "kcore_frontend.cpp"
    src.write_text(TU)
    _syntax_only(src)


def test_kcore_test_tool_compiles():
    """tests/tools/kcore.cpp, which the GPU suite builds and runs"""
    _syntax_only(os.path.join(ROOT, "tests", "tools", "kcore.cpp"))


def _prototype_args(name):
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        m = re.search(r"grb_info\s+%s\s*\(([^)]*)\)\s*;" % name, f.read())
    assert m is not None, name
    return len(m.group(1).split(","))


def test_python_mirror_declares_both():
    from graphblast_amd import _lib, api
    import graphblast_amd
    assert callable(getattr(api, "coreness", None)) and graphblast_amd.coreness is api.coreness
    assert callable(getattr(api, "kcore", None)) and graphblast_amd.kcore is api.kcore
    assert list(inspect.signature(api.coreness).parameters) == ["v", "A", "desc"]
    assert list(inspect.signature(api.kcore).parameters) == ["v", "A", "k", "desc"]
    for f in (api.coreness, api.kcore):
        assert all(p.default is inspect.Parameter.empty for p in inspect.signature(f).parameters.values())
    doc = api.coreness.__doc__
    assert doc and "grb_coreness" in doc and "at least k neighbours inside the subgraph" in doc and "degeneracy" in doc
    assert "GrB_INVALID_VALUE" in doc and "GrB_DIMENSION_MISMATCH" in doc and "GrB_NOT_IMPLEMENTED" in doc and "GrB_PANIC" in doc
    doc = api.kcore.__doc__
    assert doc and "grb_kcore" in doc and "k < 0 -> GrB_INVALID_VALUE" in doc and "plain degrees" in doc
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "grb_matrix_eWiseMult" in v)
    assert "grb_coreness" in table and "grb_kcore" in table
    assert len(table["grb_coreness"]) == _prototype_args("grb_coreness") == 4
    assert len(table["grb_kcore"]) == _prototype_args("grb_kcore") == 5
    assert table["grb_coreness"][-1] is ctypes.POINTER(_lib.KcoreResult)
    assert table["grb_kcore"][-1] is ctypes.POINTER(_lib.KcoreResult)


C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def _record(hdr, name):
    m = re.search(r"typedef struct \{([^{}]*)\} %s;" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S)   # (comments may hold braces)
    assert m is not None, name
    decls = [x.split() for x in m.group(1).split(";") if x.strip()]
    return [d[-1] for d in decls], [d[0] for d in decls]


def test_header_declares_the_result_record():
    """grb_kcore_result, field for field and type for type what the Python mirror reads: 40 bytes"""
    from graphblast_amd import _lib
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = f.read()
    fields, types = _record(hdr, "grb_kcore_result")
    assert fields == ["edges", "result_edges", "kmax", "levels", "result_vertices", "rounds", "launches", "loop_ms"]
    assert types == ["int64_t", "int64_t", "int32_t", "int32_t", "int32_t", "int32_t", "int32_t", "float"]
    assert [f[0] for f in _lib.KcoreResult._fields_] == fields
    assert [f[1] for f in _lib.KcoreResult._fields_] == [C_TYPES[t] for t in types]
    assert ctypes.sizeof(_lib.KcoreResult) == 40


def test_header_states_the_contract():
    """the definition, in full, is in the header: the graph, the k-core, core(v), kmax, both calls, the structure rule, the
    errors, the working memory"""
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = re.sub(r"\s*\n \*\s*", " ", f.read())
    block = hdr[hdr.index("The k-core decomposition (csrc/kcore.hip)"):hdr.index("} grb_kcore_result;")]
    for phrase in ("simple undirected graph", "at least k neighbours inside the subgraph", "It is unique".lower(), "largest k such that v is in the k-core",
                   "the degeneracy", "0 for an isolated vertex", "k = 0 gives the plain degrees", "k > kmax is a success",
                   "only the CSR is read", "GRB_INVALID_VALUE", "GRB_PANIC", "GRB_OUT_OF_MEMORY", "GRB_DIMENSION_MISMATCH",
                   "GRB_NOT_IMPLEMENTED", "GRB_UNINITIALIZED_OBJECT", "k < 0", "levels = 1 when n > 0", "Working memory",
                   "same inputs give the same bits", "bounded spins"):
        assert phrase in block, phrase
