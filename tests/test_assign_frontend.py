"""The C++ frontend's four matrix assign overloads (include/graphblas/graphblas.hpp; operations.hpp:441-551 of the
reference: submatrix, column, row, constant) compile with the reference's signatures: template arguments spelled out or
deduced, const or non-const operands, given lists or typed null lists, GrB_NULL or graphblas::plus<T>() as the accum,
C == A, float and int; a functor type without an operator code is GrB_NOT_IMPLEMENTED, not a compile error.  Syntax only:
no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r"""
#define GRB_USE_CUDA
#include <vector>
#include "graphblas/graphblas.hpp"

struct my_accum {                      // a user's functor: no operator code for the device
  float operator()(float a, float b) const { return a + b; }
};

template <typename T>
static graphblas::Info all_four(graphblas::Matrix<T>* C, graphblas::Matrix<T>* A, graphblas::Matrix<T>* M,
                                graphblas::Vector<T>* u, graphblas::Vector<T>* vm, graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<T>* cA = A;
  const Matrix<T>* cM = M;
  const Vector<T>* cu = u;
  const Vector<T>* cvm = vm;
  const Vector<T>* nomask = NULL;
  std::vector<Index> rows(2, 0), cols(3, 1);
  rows[1] = 1; cols[1] = 2; cols[2] = 3;
  const std::vector<Index>* crows = &rows;
  const std::vector<Index>* ccols = &cols;
  const std::vector<Index>* none = NULL;
  const Index one = 1;
  const T val = static_cast<T>(3);
  Info i = GrB_SUCCESS;
  // spelled-out template arguments, a null mask and accum (the reference's way of calling), given and null lists
  i = assign<T, T, T>(C, GrB_NULL, GrB_NULL, A, &rows, 2, &cols, 3, desc);
  i = assign<T, T, T>(C, GrB_NULL, GrB_NULL, A, GrB_ALL, 4, GrB_ALL, 4, desc);
  i = assign<T, T, T>(C, GrB_NULL, GrB_NULL, val, &rows, 2, &cols, 3, desc);
  i = assign<T, T, T>(C, GrB_NULL, GrB_NULL, val, GrB_ALL, 4, GrB_ALL, 4, desc);
  i = assign<T, T, T>(C, GrB_NULL, GrB_NULL, u, crows, 2, one, desc);
  i = assign<T, T, T>(C, GrB_NULL, GrB_NULL, u, one, ccols, 3, desc);
  i = assign<T, T, T>(C, GrB_NULL, GrB_NULL, u, none, 4, one, desc);
  i = assign<T, T, T>(C, GrB_NULL, GrB_NULL, u, one, none, 4, desc);
  i = assign<T, T, T>(C, GrB_NULL, graphblas::plus<T>(), A, &rows, 2, &cols, 3, desc);
  i = assign<T, T, T>(C, GrB_NULL, graphblas::plus<T>(), val, &rows, 2, &cols, 3, desc);
  i = assign<T, T, T>(C, GrB_NULL, graphblas::plus<T>(), u, crows, 2, one, desc);
  i = assign<T, T, T>(C, GrB_NULL, graphblas::plus<T>(), u, one, ccols, 3, desc);
  // deduced, non-const and const operands and lists, a mask
  i = assign(C, M, GrB_NULL, A, &rows, 2, &cols, 3, desc);
  i = assign(C, cM, GrB_NULL, cA, crows, 2, none, 4, desc);
  i = assign(C, cM, graphblas::plus<T>(), cA, none, 4, ccols, 3, desc);
  i = assign(C, M, graphblas::first<T>(), A, none, 4, none, 4, desc);
  i = assign(C, M, GrB_NULL, val, &rows, 2, &cols, 3, desc);
  i = assign(C, cM, graphblas::plus<T>(), val, none, 4, ccols, 3, desc);
  i = assign(C, cM, GrB_NULL, 1, crows, 2, none, 4, desc);
  i = assign(C, vm, GrB_NULL, u, crows, 2, one, desc);
  i = assign(C, cvm, graphblas::plus<T>(), cu, none, 4, one, desc);
  i = assign(C, nomask, GrB_NULL, cu, crows, 2, one, desc);
  i = assign(C, vm, GrB_NULL, u, one, ccols, 3, desc);
  i = assign(C, cvm, graphblas::plus<T>(), cu, one, none, 4, desc);
  i = assign(C, nomask, GrB_NULL, cu, one, ccols, 3, desc);
  // in place
  i = assign(A, cM, GrB_NULL, A, none, 4, none, 4, desc);
  i = assign(A, cM, graphblas::plus<T>(), cA, crows, 2, crows, 2, desc);
  i = assign(M, M, GrB_NULL, A, none, 4, none, 4, desc);
  // a functor without an operator code compiles and answers GrB_NOT_IMPLEMENTED
  i = assign(C, cM, my_accum(), cA, none, 4, none, 4, desc);
  i = assign(C, cM, my_accum(), val, none, 4, none, 4, desc);
  i = assign(C, cvm, my_accum(), cu, none, 4, one, desc);
  i = assign(C, cvm, my_accum(), cu, one, none, 4, desc);
  return i;
}

int main() {
  graphblas::Matrix<float> fa(4, 4), fc(4, 4), fm(4, 4);
  graphblas::Matrix<int> ia(4, 4), ic(4, 4), im(4, 4);
  graphblas::Vector<float> fu(4), fv(4);
  graphblas::Vector<int> iu(4), iv(4);
  graphblas::Descriptor desc;
  graphblas::Info i = all_four(&fc, &fa, &fm, &fu, &fv, &desc);
  i = all_four(&ic, &ia, &im, &iu, &iv, &desc);
  // the vector assign (a constant under a mask) is what it was
  i = graphblas::assign<float, float, float, graphblas::Index>(&fu, &fv, GrB_NULL, 1.f, GrB_ALL, 4, &desc);
  return i == graphblas::GrB_SUCCESS ? 0 : 1;
}
"""


def test_assign_overloads_compile(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    src = tmp_path / "assign_frontend.cpp"
    src.write_text(TU)
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
