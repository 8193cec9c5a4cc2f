"""The C++ frontend's betweenness-centrality driver (include/graphblas/algorithm/bc.hpp) compiles: float and int A, const
and non-const, with and without the result record, a NULL source list and a NULL descriptor.  And the Python mirror is
there: api.bc with its parameter names and docstring, _lib's declaration with the argument count of the prototype in
include/grb_hip.h, and the header's grb_bc_result.  No GPU."""
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
#include "graphblas/algorithm/bc.hpp"

template <typename A>
static graphblas::Info all(graphblas::Vector<float>* v, graphblas::Matrix<A>* a, graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<A>* ca = a;
  std::vector<Index> src(3, 0);
  const std::vector<Index>* csrc = &src;
  grb_bc_result rec;
  Info i = GrB_SUCCESS;
  i = algorithm::bc(v, a, &src, desc);                   // non-const A, no record
  i = algorithm::bc(v, ca, csrc, desc, &rec);            // const A, a const list, the record
  i = algorithm::bc<A>(v, ca, &src, desc);               // the spelled-out template argument
  i = algorithm::bc(v, a, static_cast<const std::vector<Index>*>(NULL), desc);          // every vertex a source
  i = algorithm::bc(v, ca, static_cast<const std::vector<Index>*>(NULL), desc, &rec);
  i = algorithm::bc(v, ca, &src, static_cast<Descriptor*>(NULL));                       // a null descriptor
  i = algorithm::bc(v, ca, static_cast<const std::vector<Index>*>(NULL), static_cast<Descriptor*>(NULL), &rec);
  return i == GrB_SUCCESS && rec.sources >= 0 && rec.batches >= 0 && rec.levels >= 0 && rec.reached >= 0 && rec.loop_ms >= 0.f
             ? GrB_SUCCESS : i;
}

int main() {
  graphblas::Matrix<float> fa(4, 4);
  graphblas::Matrix<int> ia(4, 4);
  graphblas::Vector<float> v(4);
  graphblas::Descriptor desc;
  graphblas::Info i = all(&v, &fa, &desc);
  i = all(&v, &ia, &desc);
  return i == graphblas::GrB_SUCCESS ? 0 : 1;
}
"""


def test_bc_driver_compiles(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    src = tmp_path / "bc_frontend.cpp"
    src.write_text(TU)
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def _prototype_args(name):
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        m = re.search(r"grb_info\s+%s\s*\(([^)]*)\)\s*;" % name, f.read())
    assert m is not None, name
    return len(m.group(1).split(","))


def test_python_mirror_declares_bc():
    from graphblast_amd import _lib, api
    assert callable(getattr(api, "bc", None))
    assert list(inspect.signature(api.bc).parameters) == ["v", "A", "sources", "desc"]
    assert api.bc.__doc__
    assert "grb_bc" in _lib._SIGS
    assert len(_lib._SIGS["grb_bc"]) == _prototype_args("grb_bc") == 6


def test_header_declares_the_result_record():
    """grb_bc_result, with the five fields the Python mirror reads, in the header's order"""
    from graphblast_amd import _lib
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = f.read()
    m = re.search(r"typedef struct \{([^{}]*)\} grb_bc_result;", hdr, re.S)
    assert m is not None
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [x.split()[-1] for x in body.split(";") if x.strip()]
    assert fields == ["sources", "batches", "levels", "reached", "loop_ms"]
    assert [f[0] for f in _lib.BcResult._fields_] == fields
