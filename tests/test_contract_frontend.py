"""The C++ frontend's contraction driver (include/graphblas/algorithm/contract.hpp) compiles: float and int A, const and
non-const, a null descriptor, a null sizes, with and without the result record, relabel with and without the count.  And the
Python mirror is there: api.relabel and api.contract with their parameter names and docstrings, the two kind constants,
_lib's declarations with the argument counts of the prototypes in include/grb_hip.h, and the header's grb_contract_result
field for field.  No GPU."""
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
#include "graphblas/algorithm/contract.hpp"

template <typename A>
static graphblas::Info all(graphblas::Matrix<A>* c, graphblas::Vector<int>* sizes, graphblas::Matrix<A>* a, graphblas::Vector<int>* map,
                           graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<A>* ca = a;
  const Vector<int>* cmap = map;
  grb_contract_result rec;
  Info i = GrB_SUCCESS;
  i = algorithm::contract(c, sizes, a, map, GRB_OP_PLUS, 0, desc);                                   // non-const A, no record
  i = algorithm::contract(c, sizes, ca, cmap, GRB_OP_MINIMUM, 1, desc, &rec);                        // const A and map, the record
  i = algorithm::contract<A>(c, sizes, ca, map, GRB_OP_MAXIMUM, 0, desc);                            // the spelled-out template argument
  i = algorithm::contract(c, sizes, ca, map, GRB_OP_FIRST, 1, static_cast<Descriptor*>(NULL));       // a null descriptor
  i = algorithm::contract(c, static_cast<Vector<int>*>(NULL), a, map, GRB_OP_PLUS, 0, desc, &rec);   // a null sizes
  i = algorithm::contract(c, static_cast<Vector<int>*>(NULL), ca, cmap, GRB_OP_PLUS, 1, static_cast<Descriptor*>(NULL), &rec);
  i = algorithm::contract(a, sizes, a, map, GRB_OP_PLUS, 1, desc);                                   // in place
  return i == GrB_SUCCESS && rec.kept >= 0 && rec.loops >= 0 && rec.entries >= 0 && rec.clusters >= 0 && rec.dropped >= 0 &&
                 rec.largest >= 0 && rec.launches >= 0 && rec.loop_ms >= 0.f ? GrB_SUCCESS : i;
}

int main() {
  graphblas::Matrix<float> fa(4, 4), fc(4, 4);
  graphblas::Matrix<int> ia(4, 4), ic(4, 4);
  graphblas::Vector<int> map(4), sizes(4), labels(4);
  const graphblas::Vector<int>* clabels = &labels;
  graphblas::Descriptor desc;
  int count = 0;
  graphblas::Info i = all(&fc, &sizes, &fa, &map, &desc);
  i = all(&ic, &sizes, &ia, &map, &desc);
  i = graphblas::algorithm::relabel(&map, &labels, GRB_RELABEL_LABELS);                              // no count
  i = graphblas::algorithm::relabel(&map, clabels, GRB_RELABEL_MATE, &count);                        // const labels, the count
  i = graphblas::algorithm::relabel(&labels, &labels, 0, &count);                                    // in place
  return i == graphblas::GrB_SUCCESS && GRB_RELABEL_LABELS == 0 && GRB_RELABEL_MATE == 1 ? 0 : 1;
}
"""


def _syntax_only(path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_contract_driver_compiles(tmp_path):
    src = tmp_path / "contract_frontend.cpp"
    src.write_text(TU)
    _syntax_only(src)


def test_contract_test_tool_compiles():
    """tests/tools/contract.cpp, which the GPU suite builds and runs"""
    _syntax_only(os.path.join(ROOT, "tests", "tools", "contract.cpp"))


def _prototype_args(name):
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        m = re.search(r"grb_info\s+%s\s*\(([^)]*)\)\s*;" % name, f.read())
    assert m is not None, name
    return len(m.group(1).split(","))


def test_python_mirror_declares_them():
    from graphblast_amd import _lib, api
    import graphblast_amd
    assert callable(getattr(api, "relabel", None)) and graphblast_amd.relabel is api.relabel
    assert callable(getattr(api, "contract", None)) and graphblast_amd.contract is api.contract
    assert (api.GRB_RELABEL_LABELS, api.GRB_RELABEL_MATE) == (0, 1) and graphblast_amd.GRB_RELABEL_MATE == 1
    assert list(inspect.signature(api.relabel).parameters) == ["map", "labels", "kind"]
    assert list(inspect.signature(api.contract).parameters) == ["Cm", "sizes", "A", "map", "op", "loops", "desc"]
    for f in (api.relabel, api.contract):
        assert all(p.default is inspect.Parameter.empty for p in inspect.signature(f).parameters.values())
    doc = " ".join((api.relabel.__doc__ or "").split())
    assert "grb_relabel" in doc
    for phrase in ("all n values stored", "GRB_RELABEL_LABELS (0)", "GRB_RELABEL_MATE (1)", "min(v, labels[v])", "becomes dense",
                   "the number of distinct values of L smaller than L(v)", "map may be labels", "same bits", "before map is written",
                   "GrB_UNINITIALIZED_OBJECT", "GrB_DIMENSION_MISMATCH", "GrB_NOT_IMPLEMENTED", "GrB_INVALID_VALUE", "GrB_INVALID_INDEX"):
        assert phrase in doc, phrase
    doc = " ".join((api.contract.__doc__ or "").split())
    assert "grb_contract" in doc
    for phrase in ("S^T A S", "only its CSR is read", "stored zeros are entries", "-1 .. nc - 1", "-1 drops the vertex", "loops = 0 drops",
                   "columns ascend", '"plus"', '"minimum"', '"maximum"', '"first"', "wraps", "rounds once", "no floating-point atomics",
                   "-NaN < -inf", "-0.0 < +0.0", "+inf < +NaN", "the winner's bits", "smallest (i, j)", "the transpose of that CSR",
                   "Cm may be A when nc = n", "sizes[a]", "No descriptor field is read", "unchanged on every error", "kept", "clusters",
                   "dropped", "largest", "launches", "loop_ms"):
        assert phrase in doc, phrase
    for code in ("GrB_UNINITIALIZED_OBJECT", "GrB_DIMENSION_MISMATCH", "GrB_NOT_IMPLEMENTED", "GrB_DOMAIN_MISMATCH", "GrB_INVALID_VALUE",
                 "GrB_INVALID_INDEX", "GrB_OUT_OF_MEMORY"):
        assert code in doc, code
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "grb_matrix_eWiseMult" in v)
    assert "grb_relabel" in table and "grb_contract" in table
    assert len(table["grb_relabel"]) == _prototype_args("grb_relabel") == 5
    assert len(table["grb_contract"]) == _prototype_args("grb_contract") == 8
    assert table["grb_relabel"][2] is ctypes.c_int and table["grb_relabel"][3] is ctypes.POINTER(ctypes.c_int32)
    assert table["grb_contract"][4] is ctypes.c_int and table["grb_contract"][5] is ctypes.c_int
    assert table["grb_contract"][-1] is ctypes.POINTER(_lib.ContractResult)


C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}


def _record(hdr, name):
    m = re.search(r"typedef struct \{([^{}]*)\} %s;" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S)   # (comments may hold braces)
    assert m is not None, name
    decls = [x.split() for x in m.group(1).split(";") if x.strip()]
    return [d[-1] for d in decls], [d[0] for d in decls]


def test_header_declares_the_result_record():
    """grb_contract_result, field for field and type for type what the Python mirror reads: 48 bytes, as its comment says"""
    from graphblast_amd import _lib
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = f.read()
    fields, types = _record(hdr, "grb_contract_result")
    assert fields == ["kept", "loops", "entries", "clusters", "dropped", "largest", "launches", "loop_ms"]
    assert types == ["int64_t"] * 3 + ["int32_t"] * 4 + ["float"]
    assert [f[0] for f in _lib.ContractResult._fields_] == fields
    assert [f[1] for f in _lib.ContractResult._fields_] == [C_TYPES[t] for t in types]
    assert ctypes.sizeof(_lib.ContractResult) == 48
    assert re.search(r"\}\s*grb_contract_result;\s*/\*\s*48 bytes\s*\*/", hdr)
    for name, value in (("GRB_RELABEL_LABELS", 0), ("GRB_RELABEL_MATE", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name


def test_header_states_the_contract():
    """the definitions, in full, are in the header: the two kinds, the map's range, loops, the four operators and their value
    rules, what C and sizes receive, the errors and the working memory"""
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = re.sub(r"\s*\n \*\s*", " ", f.read())
    block = hdr[hdr.index("Graph contraction (csrc/contract.hip)"):hdr.index("} grb_contract_result;")]
    for phrase in ("with all n values stored", "every value is in 0 .. n - 1", "every value is in -1 .. n - 1", "min(v, labels(v))",
                   "The involution is not checked", "the number of distinct values of L smaller than L(v)", "map may be labels",
                   "Errors are found before map is written", "C = S^T A S with S(v, map(v)) = 1", "Only the CSR is read",
                   "Stored zeros are entries", "each in -1 .. nc - 1", "map(v) = -1 drops vertex v", "checked on the device before anything is written",
                   "0 drops every entry with map(i) = map(j)", "1 keeps them", "Columns ascend in every row", "never a second fold",
                   "C may be A when nc = n", "two's-complement wrap-around", "an f64 sum rounded to f32 once", "not of GRB_NUM_CU or of scheduling",
                   "No floating-point atomic", "-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN", "The winner's bits are copied",
                   "the contributing entry with the smallest (i, j)", "sizes(a) = |{v : map(v) = a}|", "no descriptor field is read",
                   "no level loop, no grid barrier", "not a serial chain", "nothing is read or written out of bounds", "Working memory",
                   "both keep what they held", "GRB_UNINITIALIZED_OBJECT", "GRB_DIMENSION_MISMATCH", "GRB_NOT_IMPLEMENTED",
                   "GRB_DOMAIN_MISMATCH", "GRB_INVALID_VALUE", "GRB_INVALID_INDEX", "GRB_OUT_OF_MEMORY", "success with an empty C"):
        assert phrase in block, phrase
