"""The C++ frontend's minimum-spanning-forest driver (include/graphblas/algorithm/msf.hpp) compiles: float and int A, const
and non-const, a null descriptor, a null comp, with and without the result record.  And the Python mirror is there: api.msf
with its parameter names and docstring, _lib's declaration with the argument count of the prototype in include/grb_hip.h,
and the header's grb_msf_result field for field.  No GPU."""
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
#include "graphblas/algorithm/msf.hpp"

template <typename A>
static graphblas::Info all(graphblas::Matrix<A>* c, graphblas::Vector<int>* comp, graphblas::Matrix<A>* a, graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<A>* ca = a;
  grb_msf_result rec;
  Info i = GrB_SUCCESS;
  i = algorithm::msf(c, comp, a, desc);                                             // non-const A, no record
  i = algorithm::msf(c, comp, ca, desc, &rec);                                      // const A, the record
  i = algorithm::msf<A>(c, comp, ca, desc);                                         // the spelled-out template argument
  i = algorithm::msf(c, comp, ca, static_cast<Descriptor*>(NULL));                  // a null descriptor
  i = algorithm::msf(c, static_cast<Vector<int>*>(NULL), a, desc, &rec);            // a null comp
  i = algorithm::msf(c, static_cast<Vector<int>*>(NULL), ca, static_cast<Descriptor*>(NULL), &rec);
  i = algorithm::msf(a, comp, a, desc);                                             // in place
  return i == GrB_SUCCESS && rec.edges >= 0 && rec.forest_edges >= 0 && rec.weight >= 0. && rec.components >= 0 && rec.isolated >= 0 &&
                 rec.rounds >= 0 && rec.passes >= 0 && rec.launches >= 0 && rec.loop_ms >= 0.f ? GrB_SUCCESS : i;
}

int main() {
  graphblas::Matrix<float> fa(4, 4), fc(4, 4);
  graphblas::Matrix<int> ia(4, 4), ic(4, 4);
  graphblas::Vector<int> comp(4);
  graphblas::Descriptor desc;
  graphblas::Info i = all(&fc, &comp, &fa, &desc);
  i = all(&ic, &comp, &ia, &desc);
  return i == graphblas::GrB_SUCCESS ? 0 : 1;
}
"""


def _syntax_only(path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_msf_driver_compiles(tmp_path):
    src = tmp_path / "msf_frontend.cpp"
    src.write_text(TU)
    _syntax_only(src)


def test_msf_test_tool_compiles():
    """tests/tools/msf.cpp, which the GPU suite builds and runs"""
    _syntax_only(os.path.join(ROOT, "tests", "tools", "msf.cpp"))


def _prototype_args(name):
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        m = re.search(r"grb_info\s+%s\s*\(([^)]*)\)\s*;" % name, f.read())
    assert m is not None, name
    return len(m.group(1).split(","))


def test_python_mirror_declares_it():
    from graphblast_amd import _lib, api
    import graphblast_amd
    assert callable(getattr(api, "msf", None)) and graphblast_amd.msf is api.msf
    assert list(inspect.signature(api.msf).parameters) == ["Cm", "comp", "A", "desc"]
    assert all(p.default is inspect.Parameter.empty for p in inspect.signature(api.msf).parameters.values())
    doc = api.msf.__doc__
    assert doc and "grb_msf" in doc
    for phrase in ("(w, min(u, v), max(u, v))", "-0.0 and +0.0", "Kruskal", "smallest vertex number", "Cm may be A", "NaN"):
        assert phrase in doc, phrase
    for code in ("GrB_UNINITIALIZED_OBJECT", "GrB_DIMENSION_MISMATCH", "GrB_NOT_IMPLEMENTED", "GrB_DOMAIN_MISMATCH", "GrB_INVALID_VALUE",
                 "GrB_OUT_OF_MEMORY", "GrB_PANIC"):
        assert code in doc, code
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "grb_matrix_eWiseMult" in v)
    assert "grb_msf" in table
    assert len(table["grb_msf"]) == _prototype_args("grb_msf") == 5
    assert table["grb_msf"][-1] is ctypes.POINTER(_lib.MsfResult)


C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}


def _record(hdr, name):
    m = re.search(r"typedef struct \{([^{}]*)\} %s;" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S)   # (comments may hold braces)
    assert m is not None, name
    decls = [x.split() for x in m.group(1).split(";") if x.strip()]
    return [d[-1] for d in decls], [d[0] for d in decls]


def test_header_declares_the_result_record():
    """grb_msf_result, field for field and type for type what the Python mirror reads: 48 bytes"""
    from graphblast_amd import _lib
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = f.read()
    fields, types = _record(hdr, "grb_msf_result")
    assert fields == ["edges", "forest_edges", "weight", "components", "isolated", "rounds", "passes", "launches", "loop_ms"]
    assert types == ["int64_t", "int64_t", "double"] + ["int32_t"] * 5 + ["float"]
    assert [f[0] for f in _lib.MsfResult._fields_] == fields
    assert [f[1] for f in _lib.MsfResult._fields_] == [C_TYPES[t] for t in types]
    assert ctypes.sizeof(_lib.MsfResult) == 48


def test_header_states_the_contract():
    """the definition, in full, is in the header: the graph, the key order, the zeros, NaN, what C and comp receive, the
    structure rule, the errors, the bounds on an input taken on the caller's word, and the working memory"""
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = re.sub(r"\s*\n \*\s*", " ", f.read())
    block = hdr[hdr.index("The minimum spanning forest (csrc/msf.hip)"):hdr.index("} grb_msf_result;")]
    for phrase in ("symmetric in structure and in values", "Diagonal entries take no part", "A stored zero is an edge of weight 0",
                   "The weights ARE read", "(w, min(u, v), max(u, v))", "compared lexicographically", "compared as a signed integer",
                   "-0.0 and +0.0 are the same weight", "+-inf are allowed", "a NaN anywhere off the diagonal is GRB_INVALID_VALUE",
                   "the forest Kruskal builds when it takes the edges in key order", "same inputs give the same bits",
                   "only up to the tie-break", "columns ascending, empty rows for isolated vertices", "The CSC is a copy of the CSR",
                   "C may be A", "a -0.0 stays -0.0, taken from the row of min(u, v)", "the smallest vertex number in v's connected component",
                   "no descriptor field is read", "the exact 64-bit integer sum", "no floating-point atomics", "only the CSR is read",
                   "compared as bits after -0 has been mapped to +0", "without a CSC of its own", "taken on the caller's word",
                   "bounded by 32", "clamped to n - 1", "The NaN scan runs in both cases", "bounded spins", "launches is 1 whatever the graph",
                   "Ties are never broken by CSR position", "mutual pairs", "Working memory", "56 bytes per vertex",
                   "nothing is proportional to nvals", "both keep what they held", "GRB_UNINITIALIZED_OBJECT", "GRB_DIMENSION_MISMATCH",
                   "GRB_NOT_IMPLEMENTED", "GRB_DOMAIN_MISMATCH", "GRB_INVALID_VALUE", "GRB_OUT_OF_MEMORY", "GRB_PANIC",
                   "n = 0 is a success with a zero record", "components = isolated = n and weight 0"):
        assert phrase in block, phrase
