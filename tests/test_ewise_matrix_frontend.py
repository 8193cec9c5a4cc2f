"""The C++ frontend's matrix eWiseAdd / eWiseMult / transpose (include/graphblas/graphblas.hpp) compile, and a matrix
operand of eWiseMult takes the matrix overload rather than the matrix x broadcast-scalar one, const pointer or not,
template arguments spelled out or deduced; the scalar and vector forms still compile as before.  Syntax only: no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r"""
#define GRB_USE_CUDA
#include "graphblas/graphblas.hpp"

template <typename T>
static graphblas::Info all_three(graphblas::Matrix<T>* C, graphblas::Matrix<T>* A, graphblas::Matrix<T>* B,
                                 graphblas::Matrix<T>* M, graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<T>* cA = A;
  const Matrix<T>* cB = B;
  const Matrix<T>* cM = M;
  Info i = GrB_SUCCESS;
  // spelled-out template arguments, a null mask (the reference's way of calling)
  i = eWiseAdd<T, T, T, T>(C, GrB_NULL, GrB_NULL, PlusMultipliesSemiring<T>(), A, B, desc);
  i = eWiseMult<T, T, T, T>(C, GrB_NULL, GrB_NULL, PlusMultipliesSemiring<T>(), A, B, desc);
  i = transpose<T, T, T>(C, GrB_NULL, GrB_NULL, A, desc);
  // deduced, non-const and const operands, a mask
  i = eWiseAdd(C, M, GrB_NULL, MinimumPlusSemiring<T>(), A, B, desc);
  i = eWiseMult(C, M, GrB_NULL, PlusMultipliesSemiring<T>(), A, B, desc);
  i = eWiseMult(C, cM, GrB_NULL, MaximumMultipliesSemiring<T>(), cA, cB, desc);
  i = eWiseAdd(C, cM, GrB_NULL, PlusMultipliesSemiring<T>(), cA, cB, desc);
  i = transpose(C, M, GrB_NULL, A, desc);
  i = transpose(C, cM, GrB_NULL, cA, desc);
  return i;
}

template <typename T>
static graphblas::Info existing_forms(graphblas::Matrix<T>* A, graphblas::Vector<T>* v, graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Vector<T>* cv = v;
  Info i = GrB_SUCCESS;
  // matrix x broadcast scalar, in place
  i = eWiseMult<T, T, T, T>(A, GrB_NULL, GrB_NULL, PlusMultipliesSemiring<T>(), A, static_cast<T>(2), desc);
  i = eWiseMult(A, static_cast<const Matrix<T>*>(NULL), GrB_NULL, PlusMultipliesSemiring<T>(), A, 0.5, desc);
  // matrix x broadcast vector, in place
  i = eWiseMult<T, T, T, T>(A, GrB_NULL, GrB_NULL, PlusMultipliesSemiring<T>(), A, v, desc);
  i = eWiseMult(A, static_cast<const Matrix<T>*>(NULL), GrB_NULL, PlusMultipliesSemiring<T>(), A, cv, desc);
  i = eWiseMult(A, static_cast<const Matrix<T>*>(NULL), GrB_NULL, PlusMultipliesSemiring<T>(), A, v, desc);
  // vector forms
  i = eWiseMult<T, T, T, T>(v, GrB_NULL, GrB_NULL, PlusMultipliesSemiring<T>(), cv, cv, desc);
  i = eWiseAdd<T, T, T, T>(v, GrB_NULL, GrB_NULL, PlusMultipliesSemiring<T>(), cv, cv, desc);
  i = eWiseAdd<T, T, T, T>(v, GrB_NULL, GrB_NULL, PlusMultipliesSemiring<T>(), cv, static_cast<T>(1), desc);
  return i;
}

int main() {
  graphblas::Matrix<float> fa(4, 4), fb(4, 4), fc(4, 4), fm(4, 4);
  graphblas::Matrix<int> ia(4, 4), ib(4, 4), ic(4, 4), im(4, 4);
  graphblas::Vector<float> fv(4);
  graphblas::Vector<int> iv(4);
  graphblas::Descriptor desc;
  graphblas::Info i = all_three(&fc, &fa, &fb, &fm, &desc);
  i = all_three(&ic, &ia, &ib, &im, &desc);
  i = existing_forms(&fa, &fv, &desc);
  i = existing_forms(&ia, &iv, &desc);
  return i == graphblas::GrB_SUCCESS ? 0 : 1;
}
"""


def test_frontend_overloads_compile(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    src = tmp_path / "ewise_matrix_frontend.cpp"
    src.write_text(TU)
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
