"""The C++ frontend's maximum flow driver (include/graphblas/algorithm/maxflow.hpp) compiles: float and int A, const and
non-const, a null descriptor, a null F, a null side, with and without the result record.  And the Python mirror is there:
api.maxflow with its parameter names and docstring, the two mode constants, _lib's declaration with the argument count of
the prototype in include/grb_hip.h, and the header's grb_maxflow_result field for field.  No GPU."""
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
#include "graphblas/algorithm/maxflow.hpp"

template <typename A>
static graphblas::Info all(graphblas::Matrix<A>* f, graphblas::Vector<int>* side, graphblas::Matrix<A>* a, graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<A>* ca = a;
  grb_maxflow_result rec;
  Info i = GrB_SUCCESS;
  i = algorithm::maxflow(f, side, a, 0, 3, GRB_FLOW_CAPACITY, desc);                                // non-const A, no record
  i = algorithm::maxflow(f, side, ca, 0, 3, GRB_FLOW_UNIT, desc, &rec);                             // const A, the record
  i = algorithm::maxflow<A>(f, side, ca, 1, 2, GRB_FLOW_CAPACITY, desc);                            // the spelled-out template argument
  i = algorithm::maxflow(f, side, ca, 0, 3, 0, static_cast<Descriptor*>(NULL));                     // a null descriptor
  i = algorithm::maxflow(static_cast<Matrix<A>*>(NULL), side, a, 0, 3, 1, desc, &rec);              // a null F
  i = algorithm::maxflow(f, static_cast<Vector<int>*>(NULL), ca, 0, 3, 0, desc, &rec);              // a null side
  i = algorithm::maxflow(static_cast<Matrix<A>*>(NULL), static_cast<Vector<int>*>(NULL), ca, 0, 3, 0, static_cast<Descriptor*>(NULL), &rec);
  i = algorithm::maxflow(a, side, a, 0, 3, 0, desc);                                                // in place
  return i == GrB_SUCCESS && rec.value >= 0 && rec.arcs >= 0 && rec.flow_arcs >= -1 && rec.sink_side >= 0 && rec.cut_arcs >= 0 &&
                 rec.cut_capacity >= 0 && rec.rounds >= 0 && rec.global_relabels >= 0 && rec.passes >= 0 && rec.launches >= 0 &&
                 rec.loop_ms >= 0.f ? GrB_SUCCESS : i;
}

int main() {
  graphblas::Matrix<float> fa(4, 4), ff(4, 4);
  graphblas::Matrix<int> ia(4, 4), iff(4, 4);
  graphblas::Vector<int> side(4);
  graphblas::Descriptor desc;
  graphblas::Info i = all(&ff, &side, &fa, &desc);
  i = all(&iff, &side, &ia, &desc);
  return i == graphblas::GrB_SUCCESS && GRB_FLOW_CAPACITY == 0 && GRB_FLOW_UNIT == 1 ? 0 : 1;
}
"""


def _syntax_only(path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_maxflow_driver_compiles(tmp_path):
    src = tmp_path / "maxflow_frontend.cpp"
    src.write_text(TU)
    _syntax_only(src)


def test_maxflow_test_tool_compiles():
    """tests/tools/maxflow.cpp, which the GPU suite builds and runs"""
    _syntax_only(os.path.join(ROOT, "tests", "tools", "maxflow.cpp"))


def _prototype_args(name):
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        m = re.search(r"grb_info\s+%s\s*\(([^)]*)\)\s*;" % name, f.read())
    assert m is not None, name
    return len(m.group(1).split(","))


def test_python_mirror_declares_it():
    from graphblast_amd import _lib, api
    import graphblast_amd
    assert callable(getattr(api, "maxflow", None)) and graphblast_amd.maxflow is api.maxflow
    assert (api.GRB_FLOW_CAPACITY, api.GRB_FLOW_UNIT) == (0, 1)
    assert graphblast_amd.GRB_FLOW_UNIT == 1
    assert list(inspect.signature(api.maxflow).parameters) == ["F", "side", "A", "source", "sink", "mode", "desc"]
    assert all(p.default is inspect.Parameter.empty for p in inspect.signature(api.maxflow).parameters.values())
    doc = api.maxflow.__doc__
    assert doc and "grb_maxflow" in doc
    for phrase in ("capacity of the arc i -> j", "diagonal entries take no part", "antiparallel arcs are two arcs", "0 .. 2^24",
                   "GRB_FLOW_CAPACITY = 0", "GRB_FLOW_UNIT = 1", "a NaN is fine", "no floating-point atomics", "64-bit integer",
                   "smallest sink side", "side[sink] = 1, side[source] = 0", "cancelled form", "never both F(i, j) and F(j, i)",
                   "F may be A", "same inputs give the same bits", "not converted to a flow", "cut_capacity", "flow_arcs",
                   "global_relabels"):
        assert phrase in doc, phrase
    for code in ("GrB_UNINITIALIZED_OBJECT", "GrB_DIMENSION_MISMATCH", "GrB_INDEX_OUT_OF_BOUNDS", "GrB_INVALID_VALUE", "GrB_NOT_IMPLEMENTED",
                 "GrB_DOMAIN_MISMATCH", "GrB_INVALID_OBJECT", "GrB_OUT_OF_MEMORY", "GrB_PANIC"):
        assert code in doc, code
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "grb_matrix_eWiseMult" in v)
    assert "grb_maxflow" in table
    assert len(table["grb_maxflow"]) == _prototype_args("grb_maxflow") == 8
    assert table["grb_maxflow"][3] is ctypes.c_int64 and table["grb_maxflow"][4] is ctypes.c_int64 and table["grb_maxflow"][5] is ctypes.c_int
    assert table["grb_maxflow"][-1] is ctypes.POINTER(_lib.MaxflowResult)


C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}


def _record(hdr, name):
    m = re.search(r"typedef struct \{([^{}]*)\} %s;" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S)   # (comments may hold braces)
    assert m is not None, name
    decls = [x.split() for x in m.group(1).split(";") if x.strip()]
    return [d[-1] for d in decls], [d[0] for d in decls]


def test_header_declares_the_result_record():
    """grb_maxflow_result, field for field and type for type what the Python mirror reads: 72 bytes, as its comment says"""
    from graphblast_amd import _lib
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = f.read()
    fields, types = _record(hdr, "grb_maxflow_result")
    assert fields == ["value", "arcs", "flow_arcs", "sink_side", "cut_arcs", "cut_capacity", "rounds", "global_relabels", "passes", "launches",
                      "loop_ms"]
    assert types == ["int64_t"] * 6 + ["int32_t"] * 4 + ["float"]
    assert [f[0] for f in _lib.MaxflowResult._fields_] == fields
    assert [f[1] for f in _lib.MaxflowResult._fields_] == [C_TYPES[t] for t in types]
    assert ctypes.sizeof(_lib.MaxflowResult) == 72
    assert re.search(r"\}\s*grb_maxflow_result;\s*/\*\s*72 bytes\s*\*/", hdr)
    for name, value in (("GRB_FLOW_CAPACITY", 0), ("GRB_FLOW_UNIT", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name


def test_header_states_the_contract():
    """the definition, in full, is in the header: the network, the two modes, the exact arithmetic, what value, side and F are,
    the algorithm and what bounds it, the errors and the working memory"""
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        hdr = re.sub(r"\s*\n \*\s*", " ", f.read())
    block = hdr[hdr.index("Maximum flow and minimum cut (csrc/maxflow.hip)"):hdr.index("} grb_maxflow_result;")]
    for phrase in ("A(i, j) is the capacity of the arc i -> j", "No symmetry is asked for", "Diagonal entries take no part",
                   "are two arcs", "A stored 0 is an arc of capacity 0", "i32 must be >= 0", "an integer value in 0 .. 2^24",
                   "negative, fractional, NaN, +-inf, above 2^24", "the values are never read", "A NaN is fine",
                   "32-bit residual capacities", "64-bit integer excesses and value", "no floating-point atomic",
                   "Integer atomic adds commute", "It is unique", "the smallest sink side of any minimum cut",
                   "for every maximum preflow", "side(sink) = 1, side(source) = 0", "their capacities sum to value",
                   "cancelled form", "0 < F(i, j) <= capacity", "never both F(i, j) and F(j, i)", "Columns ascending",
                   "F may be A", "not unique as a mathematical object", "the same bits on any number of CUs",
                   "the preflow is not converted to a flow", "no descriptor field is read", "push-relabel", "global relabeling",
                   "ONE co-resident launch", "GRB_NUM_CU is honoured", "bounded spins", "launches is 1 whatever the network",
                   "as they stood at the start of the round", "only one direction of an arc pair can be admissible",
                   "one 64-bit integer atomicAdd", "exclusive prefix sum", "staged per wave in LDS",
                   "backward BFS from the sink", "offset by n", "never of timing or the CU count", "heights never exceed 2 n",
                   "panic flag", "The host reads one record", "Working memory", "44 bytes per vertex", "16 bytes per residual slot",
                   "proportional to nvals", "long thin network", "both keep what they held", "GRB_UNINITIALIZED_OBJECT",
                   "GRB_DIMENSION_MISMATCH", "GRB_INDEX_OUT_OF_BOUNDS", "n = 0 cannot name two terminals", "GRB_INVALID_VALUE",
                   "GRB_NOT_IMPLEMENTED", "GRB_DOMAIN_MISMATCH", "GRB_INVALID_OBJECT", "GRB_OUT_OF_MEMORY", "GRB_PANIC",
                   "No path from source to sink is a success with value 0"):
        assert phrase in block, phrase
