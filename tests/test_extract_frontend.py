"""The C++ frontend's three extract overloads (include/graphblas/graphblas.hpp; operations.hpp:355-410 of the reference:
subvector, submatrix, matrix column) compile with the reference's signatures: template arguments spelled out or deduced,
const or non-const operands, null (GrB_ALL) or given index lists, float and int.  Syntax only: no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r"""
#define GRB_USE_CUDA
#include <vector>
#include "graphblas/graphblas.hpp"

template <typename T>
static graphblas::Info all_three(graphblas::Matrix<T>* C, graphblas::Matrix<T>* A, graphblas::Matrix<T>* M,
                                 graphblas::Vector<T>* w, graphblas::Vector<T>* u, graphblas::Vector<T>* vm,
                                 graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<T>* cA = A;
  const Matrix<T>* cM = M;
  const Vector<T>* cu = u;
  const Vector<T>* cvm = vm;
  std::vector<Index> rows(2, 0), cols(3, 1);
  const std::vector<Index>* crows = &rows;
  const std::vector<Index>* none = NULL;
  Info i = GrB_SUCCESS;
  // spelled-out template arguments, a null mask (the reference's way of calling), given and null lists
  i = extract<T, T, T>(w, GrB_NULL, GrB_NULL, u, &rows, 2, desc);
  i = extract<T, T, T>(w, GrB_NULL, GrB_NULL, u, GrB_ALL, 4, desc);
  i = extract<T, T, T>(C, GrB_NULL, GrB_NULL, A, &rows, 2, &cols, 3, desc);
  i = extract<T, T, T>(C, GrB_NULL, GrB_NULL, A, GrB_ALL, 4, GrB_ALL, 4, desc);
  i = extract<T, T, T>(w, GrB_NULL, GrB_NULL, A, &rows, 2, 1, desc);
  i = extract<T, T, T>(w, GrB_NULL, GrB_NULL, A, GrB_ALL, 4, static_cast<Index>(0), desc);
  // deduced, non-const and const operands and lists, a mask
  i = extract(w, vm, GrB_NULL, u, &rows, 2, desc);
  i = extract(w, cvm, GrB_NULL, cu, crows, 2, desc);
  i = extract(w, cvm, GrB_NULL, cu, none, 4, desc);
  i = extract(C, M, GrB_NULL, A, &rows, 2, &cols, 3, desc);
  i = extract(C, cM, GrB_NULL, cA, crows, 2, none, 4, desc);
  i = extract(C, cM, GrB_NULL, cA, none, 4, crows, 2, desc);
  i = extract(w, vm, GrB_NULL, A, &rows, 2, 1, desc);
  i = extract(w, cvm, GrB_NULL, cA, crows, 2, 3, desc);
  i = extract(w, cvm, GrB_NULL, cA, none, 4, 0, desc);
  // in place
  i = extract(A, cM, GrB_NULL, A, none, 4, none, 4, desc);
  i = extract(u, cvm, GrB_NULL, u, none, 4, desc);
  return i;
}

int main() {
  graphblas::Matrix<float> fa(4, 4), fc(4, 4), fm(4, 4);
  graphblas::Matrix<int> ia(4, 4), ic(4, 4), im(4, 4);
  graphblas::Vector<float> fw(4), fu(4), fv(4);
  graphblas::Vector<int> iw(4), iu(4), iv(4);
  graphblas::Descriptor desc;
  graphblas::Info i = all_three(&fc, &fa, &fm, &fw, &fu, &fv, &desc);
  i = all_three(&ic, &ia, &im, &iw, &iu, &iv, &desc);
  return i == graphblas::GrB_SUCCESS ? 0 : 1;
}
"""


def test_extract_overloads_compile(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    src = tmp_path / "extract_frontend.cpp"
    src.write_text(TU)
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
