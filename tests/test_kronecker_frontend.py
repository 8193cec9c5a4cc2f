"""The C++ frontend's kronecker overload (include/graphblas/graphblas.hpp: GraphBLAS's GrB_kronecker) compiles: template
arguments spelled out or deduced, GrB_NULL mask and accum, const or non-const operands, in place, float and int, a built-in
and a registered semiring.  And the Python mirror is there: api.kronecker, and _lib's declaration of grb_kronecker with the
seven arguments of include/grb_hip.h.  No GPU."""
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

namespace graphblas {
REGISTER_SEMIRING(MaxMinusSemiring, MaximumMonoid, minus)
}  // namespace graphblas

template <typename T>
static graphblas::Info all(graphblas::Matrix<T>* C, graphblas::Matrix<T>* A, graphblas::Matrix<T>* B, graphblas::Matrix<T>* M,
                           graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<T>* cA = A;
  const Matrix<T>* cB = B;
  const Matrix<T>* cM = M;
  Info i = GrB_SUCCESS;
  // spelled-out template arguments, a null mask and accum
  i = kronecker<T, T, T, T>(C, GrB_NULL, GrB_NULL, PlusMultipliesSemiring<T>(), A, B, desc);
  i = kronecker<T, T, T, T>(C, GrB_NULL, GrB_NULL, MinimumPlusSemiring<T>(), cA, cB, desc);
  // deduced, non-const and const operands, a mask
  i = kronecker(C, M, GrB_NULL, PlusMultipliesSemiring<T>(), A, B, desc);
  i = kronecker(C, cM, GrB_NULL, LogicalOrAndSemiring<T>(), cA, B, desc);
  i = kronecker(C, cM, GrB_NULL, MaxMinusSemiring<T>(), A, cB, desc);
  // in place: C is A, C is B, C is both
  i = kronecker(A, cM, GrB_NULL, PlusMultipliesSemiring<T>(), A, cB, desc);
  i = kronecker(B, cM, GrB_NULL, PlusMultipliesSemiring<T>(), cA, B, desc);
  i = kronecker(A, cM, GrB_NULL, PlusDividesSemiring<T>(), A, A, desc);
  return i;
}

int main() {
  graphblas::Matrix<float> fa(2, 2), fb(2, 3), fc(4, 6), fm(4, 6);
  graphblas::Matrix<int> ia(2, 2), ib(2, 3), ic(4, 6), im(4, 6);
  graphblas::Descriptor desc;
  graphblas::Info i = all(&fc, &fa, &fb, &fm, &desc);
  i = all(&ic, &ia, &ib, &im, &desc);
  return i == graphblas::GrB_SUCCESS ? 0 : 1;
}
"""


def test_kronecker_overload_compiles(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    src = tmp_path / "kronecker_frontend.cpp"
    src.write_text(TU)
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_python_mirror_declares_kronecker():
    """api.kronecker(Cm, mask, accum, op, A, B, desc); _lib's argument list has the seven arguments of the prototype in
    include/grb_hip.h"""
    from graphblast_amd import _lib, api
    assert callable(getattr(api, "kronecker", None))
    assert list(inspect.signature(api.kronecker).parameters) == ["Cm", "mask", "accum", "op", "A", "B", "desc"]
    assert api.kronecker.__doc__
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "grb_matrix_eWiseMult" in v)
    assert "grb_kronecker" in table and len(table["grb_kronecker"]) == 7
    assert table["grb_kronecker"] == table["grb_matrix_eWiseMult"]          # the same seven kinds of argument
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        m = re.search(r"grb_info\s+grb_kronecker\s*\(([^)]*)\)\s*;", f.read())
    assert m is not None
    assert len(m.group(1).split(",")) == 7
