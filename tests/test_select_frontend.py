"""The C++ frontend's two select overloads (include/graphblas/graphblas.hpp: GraphBLAS's GrB_select with the predefined
index-unary operators) compile: template arguments spelled out or deduced, GrB_NULL mask and accum, const or non-const
operands, in place, float and int, every SelectOp enumerator by name.  And api.SELECT_OPS names the C enumerators of
include/grb_hip.h in their order.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["TRIL", "TRIU", "DIAG", "OFFDIAG", "ROWLE", "ROWGT", "COLLE", "COLGT",
         "VALUEEQ", "VALUENE", "VALUELT", "VALUELE", "VALUEGT", "VALUEGE"]

TU = r"""
#define GRB_USE_CUDA
#include <vector>
#include "graphblas/graphblas.hpp"

template <typename T>
static graphblas::Info both(graphblas::Matrix<T>* C, graphblas::Matrix<T>* A, graphblas::Matrix<T>* M,
                            graphblas::Vector<T>* w, graphblas::Vector<T>* u, graphblas::Vector<T>* vm,
                            graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<T>* cA = A;
  const Matrix<T>* cM = M;
  const Vector<T>* cu = u;
  const Vector<T>* cvm = vm;
  Info i = GrB_SUCCESS;
  // spelled-out template arguments, a null mask and accum
  i = select<T, T, T>(C, GrB_NULL, GrB_NULL, GrB_SEL_TRIL, A, 0, desc);
  i = select<T, T, T>(w, GrB_NULL, GrB_NULL, GrB_SEL_ROWLE, u, 2, desc);
  i = select<T, T, T>(C, GrB_NULL, GrB_NULL, GrB_SEL_VALUENE, cA, 0.0, desc);
  i = select<T, T, T>(w, GrB_NULL, GrB_NULL, GrB_SEL_VALUENE, cu, 0.0, desc);
  // deduced, non-const and const operands, a mask
  i = select(C, M, GrB_NULL, GrB_SEL_TRIU, A, 1, desc);
  i = select(C, cM, GrB_NULL, GrB_SEL_DIAG, cA, -1, desc);
  i = select(w, vm, GrB_NULL, GrB_SEL_ROWGT, u, 1, desc);
  i = select(w, cvm, GrB_NULL, GrB_SEL_VALUEGE, cu, 2.5, desc);
  // in place
  i = select(A, cM, GrB_NULL, GrB_SEL_OFFDIAG, A, 0, desc);
  i = select(u, cvm, GrB_NULL, GrB_SEL_VALUELT, u, 3, desc);
  // every enumerator by name
  const SelectOp ops[] = {%s};
  for (unsigned k = 0; k < sizeof(ops) / sizeof(ops[0]); ++k) {
    i = select(C, cM, GrB_NULL, ops[k], cA, 1, desc);
    i = select(w, cvm, GrB_NULL, ops[k], cu, 1, desc);
  }
  return i;
}

int main() {
  graphblas::Matrix<float> fa(4, 4), fc(4, 4), fm(4, 4);
  graphblas::Matrix<int> ia(4, 4), ic(4, 4), im(4, 4);
  graphblas::Vector<float> fw(4), fu(4), fv(4);
  graphblas::Vector<int> iw(4), iu(4), iv(4);
  graphblas::Descriptor desc;
  graphblas::Info i = both(&fc, &fa, &fm, &fw, &fu, &fv, &desc);
  i = both(&ic, &ia, &im, &iw, &iu, &iv, &desc);
%s
  return i == graphblas::GrB_SUCCESS ? 0 : 1;
}
""" % (", ".join("GrB_SEL_" + n for n in NAMES),
       "\n".join('  static_assert(static_cast<int>(graphblas::GrB_SEL_%s) == static_cast<int>(GRB_SEL_%s) && GRB_SEL_%s == %d, '
                 '"SelectOp follows grb_select_op");' % (n, n, n, k) for k, n in enumerate(NAMES)))


def test_select_overloads_compile(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    src = tmp_path / "select_frontend.cpp"
    src.write_text(TU)
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_select_ops_follow_the_c_enum(tmp_path):
    """api.SELECT_OPS: 14 names, each at the position that is its C enumerator's value (the C++ enum's values are asserted in the
    translation unit above)"""
    from graphblast_amd import api
    assert len(api.SELECT_OPS) == 14 and api.SELECT_OPS == [n.lower() for n in NAMES]
    lines = ["#include <stdio.h>", '#include "grb_hip.h"', "int main(void) {"]
    lines += ['  printf("%s %%d\\n", (int)GRB_SEL_%s);' % (n.lower(), n) for n in NAMES]
    lines += ['  printf("count %d\\n", (int)GRB_N_SELECT_OPS);', "  return 0;", "}"]
    src = tmp_path / "select_enum.c"
    src.write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "select_enum")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(ln.split() for ln in subprocess.check_output([exe]).decode().splitlines())
    assert int(got.pop("count")) == 14
    assert {k: int(v) for k, v in got.items()} == {name: k for k, name in enumerate(api.SELECT_OPS)}
