"""The C++ frontend's random-walk and neighbour-sampling drivers (include/graphblas/algorithm/random_walk.hpp and
sample_neighbors.hpp) compile: float and int A, const and non-const, a null descriptor, a null list, with and without the
result record.  And the Python mirror is there: api.random_walk and api.sample_neighbors with their parameter names and
docstrings, _lib's declarations with the argument counts of the prototypes in include/grb_hip.h, and the header's
grb_walk_result and grb_sample_result field for field.  No GPU."""
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
#include "graphblas/algorithm/random_walk.hpp"
#include "graphblas/algorithm/sample_neighbors.hpp"

template <typename A>
static graphblas::Info all(graphblas::Vector<int>* walks, graphblas::Matrix<A>* c, graphblas::Matrix<A>* a, graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<A>* ca = a;
  std::vector<Index> list(2, 1);
  const std::vector<Index>* none = NULL;
  grb_walk_result wrec;
  grb_sample_result srec;
  Info i = GrB_SUCCESS;
  i = algorithm::random_walk(walks, a, &list, 3, GRB_WALK_UNIFORM, 7u, desc);                          // non-const A, no record
  i = algorithm::random_walk(walks, ca, &list, 3, GRB_WALK_WEIGHTED, 7u, desc, &wrec);                 // const A, the record
  i = algorithm::random_walk<A>(walks, ca, none, 1, 0, 7u, desc);                                      // every vertex
  i = algorithm::random_walk(walks, a, &list, 3, 1, 0xffffffffu, static_cast<Descriptor*>(NULL), &wrec);   // a null descriptor
  i = algorithm::sample_neighbors(c, a, &list, 5, 7u, desc);
  i = algorithm::sample_neighbors(c, ca, &list, 5, 7u, desc, &srec);
  i = algorithm::sample_neighbors<A>(c, ca, none, 5, 7u, static_cast<Descriptor*>(NULL));
  i = algorithm::sample_neighbors(a, a, &list, 1, 0u, static_cast<Descriptor*>(NULL), &srec);           // C may be A
  return i == GrB_SUCCESS && wrec.walkers >= 0 && wrec.steps >= 0 && wrec.dead_ends >= 0 && wrec.launches >= 0 && wrec.loop_ms >= 0.f &&
                 srec.rows >= 0 && srec.entries >= 0 && srec.full_rows >= 0 && srec.launches >= 0 && srec.loop_ms >= 0.f ? GrB_SUCCESS : i;
}

int main() {
  graphblas::Matrix<float> fa(4, 4), fc(2, 4);
  graphblas::Matrix<int> ia(4, 4), ic(2, 4);
  graphblas::Vector<int> walks(8);
  graphblas::Descriptor desc;
  graphblas::Info i = all(&walks, &fc, &fa, &desc);
  i = all(&walks, &ic, &ia, &desc);
  return i == graphblas::GrB_SUCCESS && GRB_WALK_UNIFORM == 0 && GRB_WALK_WEIGHTED == 1 ? 0 : 1;
}
"""


def _syntax_only(path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_drivers_compile(tmp_path):
    src = tmp_path / "sample_frontend.cpp"
    src.write_text(TU)
    _syntax_only(src)


def test_sample_test_tool_compiles():
    """tests/tools/sample.cpp, which the GPU suite builds and runs"""
    _syntax_only(os.path.join(ROOT, "tests", "tools", "sample.cpp"))


def _header():
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        return f.read()


def _prototype_args(name):
    m = re.search(r"grb_info\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m is not None, name
    return [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]


WALK_PHRASES = ("draw(seed, a, b) = mix(mix(mix((seed + 0x9e3779b9) ^ a) + b) ^ seed)", "x *= 0x85ebca6b", "x *= 0xc2b2ae35",
                "pick(r, m) = (uint64(r) * uint64(m)) >> 32", "walks[w * (length + 1) + t]", "r = draw(seed, w, t)",
                "entry pick(r, d) of the row in stored order", "exceeds pick(r, S(v))", "An entry of weight 0 is never taken",
                "every later position of that walker is -1", "<= 2^24", "<= 2^31 - 1", "the same on any number of CUs")
SAMPLE_PHRASES = ("the fanout entries with the smallest draw(seed, k, p)", "The key takes the list position k, not the vertex",
                  "stored zeros, -0.0 and NaN are copied", "the columns ascend", "may be A", "the same on any number of CUs")


def test_python_mirror_declares_them():
    from graphblast_amd import _lib, api
    import graphblast_amd
    assert callable(getattr(api, "random_walk", None)) and graphblast_amd.random_walk is api.random_walk
    assert callable(getattr(api, "sample_neighbors", None)) and graphblast_amd.sample_neighbors is api.sample_neighbors
    assert list(inspect.signature(api.random_walk).parameters) == ["walks", "A", "starts", "length", "mode", "seed", "desc"]
    assert list(inspect.signature(api.sample_neighbors).parameters) == ["C", "A", "seeds", "fanout", "seed", "desc"]
    for f in (api.random_walk, api.sample_neighbors):
        assert all(p.default is inspect.Parameter.empty for p in inspect.signature(f).parameters.values())
    assert (api.GRB_WALK_UNIFORM, api.GRB_WALK_WEIGHTED) == (0, 1) == (graphblast_amd.GRB_WALK_UNIFORM, graphblast_amd.GRB_WALK_WEIGHTED)
    doc = re.sub(r"\s+", " ", api.random_walk.__doc__)
    assert "grb_random_walk" in doc
    for phrase in WALK_PHRASES + ("walks unchanged on every error",):
        assert phrase.replace("An entry", "an entry") in doc, phrase       # (mid-sentence in the docstring)
    for code in ("GrB_UNINITIALIZED_OBJECT", "GrB_DIMENSION_MISMATCH", "GrB_INVALID_INDEX", "GrB_INVALID_VALUE", "GrB_NOT_IMPLEMENTED",
                 "GrB_OUT_OF_MEMORY"):
        assert code in doc, code
    doc = re.sub(r"\s+", " ", api.sample_neighbors.__doc__)
    assert "grb_sample_neighbors" in doc
    for phrase in SAMPLE_PHRASES + ("C unchanged on every error",):
        assert phrase in doc, phrase
    for code in ("GrB_UNINITIALIZED_OBJECT", "GrB_DIMENSION_MISMATCH", "GrB_INDEX_OUT_OF_BOUNDS", "GrB_INVALID_VALUE", "GrB_NOT_IMPLEMENTED",
                 "GrB_OUT_OF_MEMORY"):
        assert code in doc, code
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "grb_matrix_eWiseMult" in v)
    assert _prototype_args("grb_random_walk") == ["walks", "A", "starts", "ns", "length", "mode", "seed", "desc", "result"]
    assert _prototype_args("grb_sample_neighbors") == ["C", "A", "seeds", "ns", "fanout", "seed", "desc", "result"]
    assert len(table["grb_random_walk"]) == 9 and len(table["grb_sample_neighbors"]) == 8
    assert table["grb_random_walk"][3] is ctypes.c_int64 and table["grb_random_walk"][6] is ctypes.c_uint32
    assert table["grb_sample_neighbors"][3] is ctypes.c_int and table["grb_sample_neighbors"][5] is ctypes.c_uint32
    assert table["grb_random_walk"][-1] is ctypes.POINTER(_lib.WalkResult)
    assert table["grb_sample_neighbors"][-1] is ctypes.POINTER(_lib.SampleResult)


C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}


def _record(hdr, name):
    m = re.search(r"typedef struct \{([^{}]*)\} %s;" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S)   # (comments may hold braces)
    assert m is not None, name
    decls = [x.split() for x in m.group(1).split(";") if x.strip()]
    return [d[-1] for d in decls], [d[0] for d in decls]


@pytest.mark.parametrize("name, mirror, want", [
    ("grb_walk_result", "WalkResult", ["walkers", "steps", "dead_ends", "launches", "loop_ms"]),
    ("grb_sample_result", "SampleResult", ["rows", "entries", "full_rows", "launches", "loop_ms"])])
def test_header_declares_the_result_records(name, mirror, want):
    """field for field and type for type what the Python mirror reads: 32 bytes each"""
    from graphblast_amd import _lib
    hdr = _header()
    fields, types = _record(hdr, name)
    rec = getattr(_lib, mirror)
    assert fields == want and types == ["int64_t"] * 3 + ["int32_t", "float"]
    assert [f[0] for f in rec._fields_] == fields
    assert [f[1] for f in rec._fields_] == [C_TYPES[t] for t in types]
    assert ctypes.sizeof(rec) == 32
    assert re.search(r"\} %s;\s*/\* 32 bytes \*/" % name, hdr)


def test_header_states_the_contract():
    """the definitions are in the header: the draw, both walk modes, dead ends, the sample's rule, every error, what is out of
    scope and what has not been measured"""
    hdr = re.sub(r"\s*\n \*\s*", " ", _header())
    block = hdr[hdr.index("Random walks and neighbour sampling (csrc/sample.hip)"):hdr.index("} grb_sample_result;")]
    for phrase in WALK_PHRASES + SAMPLE_PHRASES + (
            "All arithmetic is unsigned 32-bit and wraps", "draw is a bijection of b", "starts == NULL means every vertex",
            "duplicates are allowed, they are different walkers", "a diagonal entry is an ordinary step", "Only the CSR is read",
            "A dead end is a row with d = 0, or in weighted mode S(v) = 0", "walks keeps what it held", "GRB_INVALID_INDEX, as grb_bc",
            "ns * (length + 1) > INT32_MAX", "ns = 0 is a success with nothing written", "if d <= fanout, the whole row",
            "uniform sampling without replacement", "with no counting pass", "the transposition behind grb_transpose",
            "aliased in the CSR-only format", "C keeps what it held", "GRB_INDEX_OUT_OF_BOUNDS, as grb_matrix_extract",
            "fanout < 1, or ns < 0: GRB_INVALID_VALUE", "ns = 0 gives an empty 0 x ncols C", "a 32-step bisection",
            "second-order (node2vec p / q) walks", "restarts", "weighted sampling without replacement", "sampling with replacement",
            "the multi-hop loop", "None of the constants has been measured", "GRB_UNINITIALIZED_OBJECT", "GRB_DIMENSION_MISMATCH",
            "GRB_NOT_IMPLEMENTED", "GRB_INVALID_VALUE", "GRB_OUT_OF_MEMORY", "#define GRB_WALK_UNIFORM 0", "#define GRB_WALK_WEIGHTED 1"):
        assert phrase in block, phrase
