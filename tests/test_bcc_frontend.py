"""The C++ frontend's biconnected-components driver (include/graphblas/algorithm/bcc.hpp) compiles: float and int A, const
and non-const, a null descriptor, a null C, a null art, with and without the result record.  And the Python mirror is there:
api.bcc with its parameter names and docstring, the two mode constants, _lib's declaration with the argument count of the
prototype in include/grb_hip.h, and the header's grb_bcc_result field for field.  No GPU."""
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
#include "graphblas/algorithm/bcc.hpp"

template <typename A>
static graphblas::Info all(graphblas::Matrix<int>* c, graphblas::Vector<int>* art, graphblas::Matrix<A>* a, graphblas::Descriptor* desc) {
  using namespace graphblas;
  const Matrix<A>* ca = a;
  grb_bcc_result rec;
  Info i = GrB_SUCCESS;
  i = algorithm::bcc(c, art, a, GRB_BCC_BLOCKS, desc);                              // non-const A, no record
  i = algorithm::bcc(c, art, ca, GRB_BCC_BRIDGES, desc, &rec);                      // const A, the record
  i = algorithm::bcc<A>(c, art, ca, GRB_BCC_BLOCKS, desc);                          // the spelled-out template argument
  i = algorithm::bcc(c, art, ca, GRB_BCC_BLOCKS, static_cast<Descriptor*>(NULL));   // a null descriptor
  i = algorithm::bcc(c, static_cast<Vector<int>*>(NULL), a, GRB_BCC_BLOCKS, desc, &rec);                 // a null art
  i = algorithm::bcc(static_cast<Matrix<int>*>(NULL), art, ca, GRB_BCC_BLOCKS, desc, &rec);              // a null C
  i = algorithm::bcc(static_cast<Matrix<int>*>(NULL), static_cast<Vector<int>*>(NULL), ca, GRB_BCC_BRIDGES,
                     static_cast<Descriptor*>(NULL), &rec);                         // the record alone
  return i == GrB_SUCCESS && rec.edges >= 0 && rec.largest >= 0 && rec.blocks >= 0 && rec.bridges >= 0 && rec.articulation >= 0 &&
                 rec.components >= 0 && rec.isolated >= 0 && rec.levels >= 0 && rec.rounds >= 0 && rec.passes >= 0 &&
                 rec.launches >= 0 && rec.loop_ms >= 0.f ? GrB_SUCCESS : i;
}

int main() {
  graphblas::Matrix<float> fa(4, 4);
  graphblas::Matrix<int> ia(4, 4), ic(4, 4);
  graphblas::Vector<int> art(4);
  graphblas::Descriptor desc;
  graphblas::Info i = all(&ic, &art, &fa, &desc);
  i = all(&ic, &art, &ia, &desc);
  i = graphblas::algorithm::bcc(&ia, &art, &ia, GRB_BCC_BLOCKS, &desc);             // in place
  return i == graphblas::GrB_SUCCESS ? 0 : 1;
}
"""


def _syntax_only(path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is required for the frontend's compile check")
    r = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_bcc_driver_compiles(tmp_path):
    src = tmp_path / "bcc_frontend.cpp"
    src.write_text(TU)
    _syntax_only(src)


def test_bcc_test_tool_compiles():
    """tests/tools/bcc.cpp, which the GPU suite builds and runs"""
    _syntax_only(os.path.join(ROOT, "tests", "tools", "bcc.cpp"))


def _header():
    with open(os.path.join(ROOT, "include", "grb_hip.h")) as f:
        return f.read()


def _prototype_args(name):
    m = re.search(r"grb_info\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m is not None, name
    return len(m.group(1).split(","))


def test_python_mirror_declares_it():
    from graphblast_amd import _lib, api
    import graphblast_amd
    assert callable(getattr(api, "bcc", None)) and graphblast_amd.bcc is api.bcc
    assert list(inspect.signature(api.bcc).parameters) == ["Cm", "art", "A", "mode", "desc"]
    assert all(p.default is inspect.Parameter.empty for p in inspect.signature(api.bcc).parameters.values())
    doc = api.bcc.__doc__
    assert doc and "grb_bcc" in doc
    for phrase in ("(min(u, v), max(u, v))", "ascending order of their smallest edge key", "number of blocks that contain v",
                   "GRB_BCC_BLOCKS = 0", "GRB_BCC_BRIDGES = 1", "Cm may be A when A is i32", "never read", "Both may be None"):
        assert phrase in doc, phrase
    for code in ("GrB_UNINITIALIZED_OBJECT", "GrB_DIMENSION_MISMATCH", "GrB_NOT_IMPLEMENTED", "GrB_DOMAIN_MISMATCH", "GrB_INVALID_VALUE",
                 "GrB_OUT_OF_MEMORY", "GrB_PANIC"):
        assert code in doc, code
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "grb_matrix_eWiseMult" in v)
    assert "grb_bcc" in table
    assert len(table["grb_bcc"]) == _prototype_args("grb_bcc") == 6
    assert table["grb_bcc"][-1] is ctypes.POINTER(_lib.BccResult)


def test_mode_constants_everywhere():
    """GRB_BCC_BLOCKS = 0 and GRB_BCC_BRIDGES = 1 in api, in the package and in the header"""
    from graphblast_amd import api
    import graphblast_amd
    hdr = _header()
    for name, value in (("GRB_BCC_BLOCKS", 0), ("GRB_BCC_BRIDGES", 1)):
        assert getattr(api, name) == value and getattr(graphblast_amd, name) == value
        m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, hdr, re.M)
        assert m is not None and int(m.group(1)) == value, name


C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}


def _record(hdr, name):
    m = re.search(r"typedef struct \{([^{}]*)\} %s;" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S)   # (comments may hold braces)
    assert m is not None, name
    decls = [x.split() for x in m.group(1).split(";") if x.strip()]
    return [d[-1] for d in decls], [d[0] for d in decls]


def test_header_declares_the_result_record():
    """grb_bcc_result, field for field and type for type what the Python mirror reads: 56 bytes"""
    from graphblast_amd import _lib
    hdr = _header()
    fields, types = _record(hdr, "grb_bcc_result")
    assert fields == ["edges", "largest", "blocks", "bridges", "articulation", "components", "isolated", "levels", "rounds", "passes",
                      "launches", "loop_ms"]
    assert types == ["int64_t", "int64_t"] + ["int32_t"] * 9 + ["float"]
    assert [f[0] for f in _lib.BccResult._fields_] == fields
    assert [f[1] for f in _lib.BccResult._fields_] == [C_TYPES[t] for t in types]
    assert ctypes.sizeof(_lib.BccResult) == 56
    assert re.search(r"\} grb_bcc_result;\s*/\* 56 bytes \*/", hdr)


def test_header_states_the_contract():
    """the definition, in full, is in the header: the graph, the blocks, the key order and the numbering, art, both modes, the
    structure rule, every error, the bounds on an input taken on the caller's word, the one launch and the working memory"""
    hdr = re.sub(r"\s*\n \*\s*", " ", _header())
    block = hdr[hdr.index("Biconnected components, articulation points and bridges (csrc/bcc.hip)"):hdr.index("} grb_bcc_result;")]
    for phrase in ("LAGraph does not ship", "Its structure is symmetric", "Its values are never read, so a stored zero is an edge",
                   "Diagonal entries take no part", "two edges lie on a common simple cycle, or are equal", "A bridge is a block of one edge",
                   "Every edge is in exactly one block", "(min(u, v), max(u, v))", "compared lexicographically",
                   "numbered in ascending order of their smallest edge key", "same inputs give the same bits on any number of CUs",
                   "the number of blocks that contain v", "2 or more exactly when v is an articulation point", "block-cut tree",
                   "may be NULL.  Otherwise n x n and i32", "GRB_BCC_BLOCKS", "GRB_BCC_BRIDGES", "whatever A's type", "the value is the block number of that edge",
                   "only the entries whose block is a single edge", "The CSC is a copy of the CSR", "C may be A when A is i32",
                   "no descriptor field is read", "only the record is filled", "only the CSR is read", "without a CSC of its own",
                   "taken on the caller's word", "the levels are bounded by n", "nothing is read or written out of bounds",
                   "Tarjan-Vishkin on a BFS forest", "ONE co-resident launch", "GRB_NUM_CU is honoured", "bounded spins",
                   "launches is 1 whatever the graph", "No floating point appears anywhere", "Working memory", "76 bytes per vertex",
                   "nothing is proportional to nvals", "a path of a million vertices", "both keep what they held",
                   "GRB_UNINITIALIZED_OBJECT", "GRB_DIMENSION_MISMATCH", "GRB_NOT_IMPLEMENTED", "GRB_DOMAIN_MISMATCH", "GRB_INVALID_VALUE",
                   "GRB_OUT_OF_MEMORY", "GRB_PANIC", "n = 0 is a success with a zero record", "art = 0 everywhere, blocks = 0",
                   "components = isolated = n"):
        assert phrase in block, phrase
