"""The C++ frontend's LCC driver (include/graphblas/algorithm/lcc.hpp) compiles: float and int A, const and non-const, a
null descriptor, with and without the result record.  And the Python mirror is there: api.lcc with its parameter names,
defaults and docstring, _lib's declaration with the argument count of the prototype in include/grb_hip.h, and the header's
grb_lcc_result field for field.  No GPU."""
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
#include "graphblas/algorithm/lcc.hpp"

template <typename A>
static graphblas::Info all(graphblas::Vector<float>* l, graphblas::Matrix<A>* a, graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<A>* ca = a;
  grb_lcc_result rec;
  Info i = GrB_SUCCESS;
  i = algorithm::lcc(l, a, false, desc);                                       // non-const A, no record
  i = algorithm::lcc(l, ca, true, desc, &rec);                                 // const A, the record
  i = algorithm::lcc<A>(l, ca, true, desc);                                    // the spelled-out template argument
  i = algorithm::lcc(l, ca, false, static_cast<Descriptor*>(NULL));            // a null descriptor
  i = algorithm::lcc(l, a, true, static_cast<Descriptor*>(NULL), &rec);
  return i == GrB_SUCCESS && rec.edges >= 0 && rec.triangles >= 0 && rec.closed >= 0 && rec.wedges >= 0 && rec.max_degree >= 0 &&
                 rec.loop_ms >= 0.f ? GrB_SUCCESS : i;
}

int main() {
  graphblas::Matrix<float> fa(4, 4);
  graphblas::Matrix<int> ia(4, 4);
  graphblas::Vector<float> l(4);
  graphblas::Descriptor desc;
  graphblas::Info i = all(&l, &fa, &desc);
  i = all(&l, &ia, &desc);
  return i == graphblas::GrB_SUCCESS ? 0 : 1;
}
"""


def test_lcc_driver_compiles(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    src = tmp_path / "lcc_frontend.cpp"
    src.write_text(TU)
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_lcc_test_tool_compiles():
    """tests/tools/lcc.cpp, which the GPU suite builds and runs"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "tools", "lcc.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def _prototype_args(name):
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        m = re.search(r"grb_info\s+%s\s*\(([^)]*)\)\s*;" % name, f.read())
    assert m is not None, name
    return len(m.group(1).split(","))


def test_python_mirror_declares_lcc():
    from graphblast_amd import _lib, api
    import graphblast_amd
    assert callable(getattr(api, "lcc", None)) and graphblast_amd.lcc is api.lcc
    sig = inspect.signature(api.lcc)
    assert list(sig.parameters) == ["v", "A", "desc", "directed"]
    assert sig.parameters["directed"].default is False
    assert all(sig.parameters[p].default is inspect.Parameter.empty for p in ("v", "A", "desc"))
    doc = api.lcc.__doc__
    assert doc and "grb_lcc" in doc and "num(x) / (d(x) (d(x) - 1))" in doc and "SET" in doc and "directed=True" in doc
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "grb_matrix_eWiseMult" in v)
    assert "grb_lcc" in table
    assert len(table["grb_lcc"]) == _prototype_args("grb_lcc") == 5
    assert table["grb_lcc"][-1] is ctypes.POINTER(_lib.LccResult)


C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def _record(hdr, name):
    m = re.search(r"typedef struct \{([^{}]*)\} %s;" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S)   # (comments may hold braces)
    assert m is not None, name
    decls = [x.split() for x in m.group(1).split(";") if x.strip()]
    return [d[-1] for d in decls], [d[0] for d in decls]


def test_header_declares_the_result_record():
    """grb_lcc_result, field for field what the Python mirror reads; grb_cdlp_result and grb_truss_result are as they were"""
    from graphblast_amd import _lib
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = f.read()
    fields, types = _record(hdr, "grb_lcc_result")
    assert fields == ["edges", "triangles", "closed", "wedges", "max_degree", "loop_ms"]
    assert types == ["int64_t", "int64_t", "int64_t", "int64_t", "int32_t", "float"]
    assert [f[0] for f in _lib.LccResult._fields_] == fields
    assert [f[1] for f in _lib.LccResult._fields_] == [C_TYPES[t] for t in types]
    assert ctypes.sizeof(_lib.LccResult) == 40
    fields, types = _record(hdr, "grb_cdlp_result")
    assert fields == ["iterations", "changed", "evaluated", "communities", "loop_ms"]
    assert types == ["int32_t", "int32_t", "int64_t", "int32_t", "float"]
    assert [f[0] for f in _lib.CdlpResult._fields_] == fields
    fields, _ = _record(hdr, "grb_truss_result")
    assert fields == ["rounds", "supports", "edges", "result_edges", "kmax", "loop_ms"]
    assert [f[0] for f in _lib.TrussResult._fields_] == fields


def test_header_states_the_contract():
    """the definition, in full, is in the header: the set N(v), the directed numerator, the quotient, both structure cases"""
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = re.sub(r"\s*\n \*\s*", " ", f.read())
    for phrase in ("a SET", "multiset", "num(v) / (d(v) (d(v) - 1))", "exactly 0", "directed == 0", "directed == 1",
                   "GRB_INVALID_OBJECT", "rounded to f32 once", "Working memory"):
        assert phrase in hdr[hdr.index("The local clustering coefficient (csrc/lcc.hip)"):hdr.index("} grb_lcc_result;")], phrase
