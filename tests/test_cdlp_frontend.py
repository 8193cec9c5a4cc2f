"""The C++ frontend's CDLP driver (include/graphblas/algorithm/cdlp.hpp) compiles: float and int A, const and non-const, a
NULL init, in place, with and without the result record.  And the Python mirror is there: api.cdlp and api.cdlp_set_skip with
their parameter names and docstrings, _lib's declaration with the argument count of the prototype in include/grb_hip.h, and
the header's grb_cdlp_result.  No GPU."""
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
#include "graphblas/algorithm/cdlp.hpp"

template <typename A>
static graphblas::Info all(graphblas::Vector<int>* l, graphblas::Vector<int>* init, graphblas::Matrix<A>* a, graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<A>* ca = a;
  const Vector<int>* cinit = init;
  grb_cdlp_result rec;
  Info i = GrB_SUCCESS;
  i = algorithm::cdlp(l, a, init, false, 10, desc);                                       // non-const A, no record
  i = algorithm::cdlp(l, ca, cinit, true, 10, desc, &rec);                                // const A and init, the record
  i = algorithm::cdlp<A>(l, ca, cinit, true, 3, desc);                                    // the spelled-out template argument
  i = algorithm::cdlp(l, a, static_cast<const Vector<int>*>(NULL), false, 10, desc);      // a NULL init: L(v) = v
  i = algorithm::cdlp(l, ca, static_cast<Vector<int>*>(NULL), true, 10, desc, &rec);
  i = algorithm::cdlp(l, a, l, false, 10, desc);                                          // in place
  i = algorithm::cdlp(init, ca, init, false, 1, desc, &rec);
  i = algorithm::cdlp(l, ca, cinit, false, 10, static_cast<Descriptor*>(NULL));           // a null descriptor
  i = algorithm::cdlp(l, a, init, false, 10, static_cast<Descriptor*>(NULL), &rec);
  return i == GrB_SUCCESS && rec.iterations >= 1 && rec.changed >= 0 && rec.evaluated >= 0 && rec.communities >= 0 &&
                 rec.loop_ms >= 0.f ? GrB_SUCCESS : i;
}

int main() {
  graphblas::Matrix<float> fa(4, 4);
  graphblas::Matrix<int> ia(4, 4);
  graphblas::Vector<int> l(4), init(4);
  graphblas::Descriptor desc;
  graphblas::Info i = all(&l, &init, &fa, &desc);
  i = all(&l, &init, &ia, &desc);
  return i == graphblas::GrB_SUCCESS ? 0 : 1;
}
"""


def test_cdlp_driver_compiles(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    src = tmp_path / "cdlp_frontend.cpp"
    src.write_text(TU)
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def _prototype_args(name):
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        m = re.search(r"grb_info\s+%s\s*\(([^)]*)\)\s*;" % name, f.read())
    assert m is not None, name
    return len(m.group(1).split(","))


def test_python_mirror_declares_cdlp():
    from graphblast_amd import _lib, api
    assert callable(getattr(api, "cdlp", None)) and callable(getattr(api, "cdlp_set_skip", None))
    sig = inspect.signature(api.cdlp)
    assert list(sig.parameters) == ["v", "A", "desc", "init", "directed", "max_iter"]
    assert sig.parameters["init"].default is None and sig.parameters["directed"].default is False
    assert sig.parameters["max_iter"].default == 10
    sig = inspect.signature(api.cdlp_set_skip)
    assert list(sig.parameters) == ["on"] and sig.parameters["on"].default == -1
    assert api.cdlp.__doc__ and api.cdlp_set_skip.__doc__
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "grb_matrix_eWiseMult" in v)
    assert "grb_cdlp" in table and "grb_cdlp_set_skip" in table
    assert len(table["grb_cdlp"]) == _prototype_args("grb_cdlp") == 7
    assert len(table["grb_cdlp_set_skip"]) == 1
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        assert re.search(r"int\s+grb_cdlp_set_skip\s*\(\s*int\s+on\s*\)\s*;", f.read())


def test_header_declares_the_result_record():
    """grb_cdlp_result, with the five fields the Python mirror reads, in the header's order; grb_truss_result is as it was"""
    from graphblast_amd import _lib
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = f.read()
    m = re.search(r"typedef struct \{([^{}]*)\} grb_cdlp_result;", hdr, re.S)
    assert m is not None
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    decls = [x.split() for x in body.split(";") if x.strip()]
    fields = [d[-1] for d in decls]
    assert fields == ["iterations", "changed", "evaluated", "communities", "loop_ms"]
    assert [d[0] for d in decls] == ["int32_t", "int32_t", "int64_t", "int32_t", "float"]
    assert [f[0] for f in _lib.CdlpResult._fields_] == fields
    m = re.search(r"typedef struct \{([^{}]*)\} grb_truss_result;", hdr, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [x.split()[-1] for x in body.split(";") if x.strip()] == ["rounds", "supports", "edges", "result_edges", "kmax", "loop_ms"]
