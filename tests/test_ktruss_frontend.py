"""The C++ frontend's k-truss drivers (include/graphblas/algorithm/ktruss.hpp) compile: float and int, const and non-const
A, in place, with and without the result record.  And the Python mirror is there: api.ktruss and api.trussness with their
parameter names and docstrings, _lib's declarations with the argument counts of the prototypes in include/grb_hip.h, and the
header's grb_truss_result.  No GPU."""
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
#include "graphblas/algorithm/ktruss.hpp"

template <typename C, typename A>
static graphblas::Info all(graphblas::Matrix<C>* c, graphblas::Matrix<A>* a, graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<A>* ca = a;
  grb_truss_result rec;
  Info i = GrB_SUCCESS;
  i = algorithm::ktruss(c, a, 3, desc);                  // non-const A, no record
  i = algorithm::ktruss(c, ca, 4, desc, &rec);           // const A, the record
  i = algorithm::ktruss<C, A>(c, ca, 2, desc);           // spelled-out template arguments
  i = algorithm::ktruss(a, a, 3, desc);                  // in place
  i = algorithm::ktruss(a, ca, 3, desc, &rec);
  i = algorithm::trussness(c, a, desc);
  i = algorithm::trussness(c, ca, desc, &rec);
  i = algorithm::trussness<C, A>(c, ca, desc);
  i = algorithm::trussness(a, a, desc, &rec);            // in place
  i = algorithm::trussness(c, ca, static_cast<Descriptor*>(NULL));   // a null descriptor: the defaults
  return i == GrB_SUCCESS && rec.rounds >= 0 && rec.kmax >= 0 ? GrB_SUCCESS : i;
}

int main() {
  graphblas::Matrix<float> fa(4, 4), fc(4, 4);
  graphblas::Matrix<int> ia(4, 4), ic(4, 4);
  graphblas::Descriptor desc;
  graphblas::Info i = all(&fc, &fa, &desc);
  i = all(&ic, &ia, &desc);
  i = all(&fc, &ia, &desc);                              // C's type is independent of A's
  i = all(&ic, &fa, &desc);
  return i == graphblas::GrB_SUCCESS ? 0 : 1;
}
"""


def test_ktruss_drivers_compile(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    src = tmp_path / "ktruss_frontend.cpp"
    src.write_text(TU)
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def _prototype_args(name):
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        m = re.search(r"grb_info\s+%s\s*\(([^)]*)\)\s*;" % name, f.read())
    assert m is not None, name
    return len(m.group(1).split(","))


def test_python_mirror_declares_ktruss_and_trussness():
    from graphblast_amd import _lib, api
    assert callable(getattr(api, "ktruss", None)) and callable(getattr(api, "trussness", None))
    assert list(inspect.signature(api.ktruss).parameters) == ["Cm", "A", "k", "desc"]
    assert list(inspect.signature(api.trussness).parameters) == ["Cm", "A", "desc"]
    assert api.ktruss.__doc__ and api.trussness.__doc__
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "grb_matrix_eWiseMult" in v)
    assert "grb_ktruss" in table and "grb_trussness" in table
    assert len(table["grb_ktruss"]) == _prototype_args("grb_ktruss") == 5
    assert len(table["grb_trussness"]) == _prototype_args("grb_trussness") == 4


def test_header_declares_the_result_record():
    """grb_truss_result, with the six fields the Python mirror reads, in the header's order; grb_algo_result is as it was"""
    from graphblast_amd import _lib
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = f.read()
    m = re.search(r"typedef struct \{([^{}]*)\} grb_truss_result;", hdr, re.S)
    assert m is not None
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [x.split()[-1] for x in body.split(";") if x.strip()]
    assert fields == ["rounds", "supports", "edges", "result_edges", "kmax", "loop_ms"]
    assert [f[0] for f in _lib.TrussResult._fields_] == fields
    m = re.search(r"typedef struct \{([^{}]*)\} grb_algo_result;", hdr, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [x.split()[-1] for x in body.split(";") if x.strip()] == ["iterations", "tight_ms", "last_value"]
