// Test driver: algorithm::bcc through the drop-in frontend.  Reads an .mtx file with readMtx, keeps its off-diagonal entries
// in both directions, and runs the biconnected components on a float matrix (a descriptor, art, the record, both modes) and
// on a const int matrix (a NULL descriptor, a NULL art, no record; a NULL C; then in place).  Prints, a line each,
//   "blocks B bridges R articulation P largest M edges E components K isolated I levels L launches N"
//   "csr | pointers | indices | values"         C's CSR in GRB_BCC_BLOCKS mode
//   "bridges | pointers | indices | values"     C's CSR in GRB_BCC_BRIDGES mode
//   "art ..."                                   the number of blocks at every vertex
// and "ok" when the int runs agree with the float run; tests/test_gpu_bcc.py compares the lines with networkx.
#define GRB_USE_CUDA
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>
#include "graphblas/graphblas.hpp"
#include "graphblas/algorithm/bcc.hpp"

static int dump(const char* name, graphblas::Matrix<int>* m, graphblas::Index nr) {
  const grb_index *ptr, *ind;
  const void* val;
  grb_index nv = 0;
  grb_matrix_nvals(m->handle(), &nv);
  if (grb_matrix_host_csr(m->handle(), &ptr, &ind, &val) != 0) return 1;
  printf("%s |", name);
  for (graphblas::Index i = 0; i <= nr; ++i) printf(" %d", ptr[i]);
  printf(" |");
  for (grb_index i = 0; i < nv; ++i) printf(" %d", ind[i]);
  printf(" |");
  for (grb_index i = 0; i < nv; ++i) printf(" %d", static_cast<const int*>(val)[i]);
  printf("\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  using namespace graphblas;
  std::vector<Index> r, c;
  std::vector<float> v;
  Index nr, nc, nv;
  readMtx(argv[1], &r, &c, &v, &nr, &nc, &nv, 1, false, NULL);
  if (nr != nc) return 2;
  std::set<std::pair<Index, Index> > both;
  for (Index i = 0; i < nv; ++i)
    if (r[i] != c[i]) {
      both.insert(std::make_pair(r[i], c[i]));
      both.insert(std::make_pair(c[i], r[i]));
    }
  std::vector<Index> sr, sc;
  std::vector<float> sf;
  std::vector<int> si;
  for (std::set<std::pair<Index, Index> >::const_iterator it = both.begin(); it != both.end(); ++it) {
    sr.push_back(it->first);
    sc.push_back(it->second);
    sf.push_back(0.f);                                                              // a stored zero is an edge
    si.push_back(7);
  }
  const Index ne = static_cast<Index>(sr.size());

  Matrix<float> a(nr, nr);
  Matrix<int> blocks(nr, nr), bridges(nr, nr);
  if (a.build(&sr, &sc, &sf, ne, GrB_NULL) != GrB_SUCCESS) return 3;
  Vector<int> art(nr);
  Descriptor desc;
  grb_bcc_result rec, brec;
  if (algorithm::bcc(&blocks, &art, &a, GRB_BCC_BLOCKS, &desc, &rec) != GrB_SUCCESS) return 4;
  if (algorithm::bcc(&bridges, static_cast<Vector<int>*>(NULL), &a, GRB_BCC_BRIDGES, &desc, &brec) != GrB_SUCCESS) return 4;
  printf("blocks %d bridges %d articulation %d largest %lld edges %lld components %d isolated %d levels %d launches %d\n", rec.blocks,
         rec.bridges, rec.articulation, static_cast<long long>(rec.largest), static_cast<long long>(rec.edges), rec.components,
         rec.isolated, rec.levels, rec.launches);
  if (dump("csr", &blocks, nr) || dump("bridges", &bridges, nr)) return 5;
  if (brec.blocks != rec.blocks || brec.bridges != rec.bridges || brec.articulation != rec.articulation) return 6;
  std::vector<int> h(nr, -1);
  Index size = nr;
  if (art.extractTuples(&h, &size) != GrB_SUCCESS || size != nr) return 7;
  printf("art");
  for (Index i = 0; i < nr; ++i) printf(" %d", h[i]);
  printf("\n");

  Matrix<int> b(nr, nr), iblocks(nr, nr);
  if (b.build(&sr, &sc, &si, ne, GrB_NULL) != GrB_SUCCESS) return 8;
  const Matrix<int>* cb = &b;
  if (algorithm::bcc(&iblocks, static_cast<Vector<int>*>(NULL), cb, GRB_BCC_BLOCKS, static_cast<Descriptor*>(NULL)) != GrB_SUCCESS) return 9;
  grb_index inv = 0, fnv = 0, bnv = 0;
  grb_matrix_nvals(iblocks.handle(), &inv);
  grb_matrix_nvals(blocks.handle(), &fnv);
  grb_bcc_result nrec, irec;
  if (algorithm::bcc(static_cast<Matrix<int>*>(NULL), static_cast<Vector<int>*>(NULL), cb, GRB_BCC_BLOCKS, &desc, &nrec) != GrB_SUCCESS)
    return 10;                                                                      // the record alone
  if (algorithm::bcc(&b, &art, cb, GRB_BCC_BLOCKS, &desc, &irec) != GrB_SUCCESS) return 10;   // in place: b becomes its blocks
  grb_matrix_nvals(b.handle(), &bnv);
  if (inv != fnv || bnv != fnv || irec.blocks != rec.blocks || nrec.blocks != rec.blocks || irec.largest != rec.largest ||
      nrec.articulation != rec.articulation)
    return 11;
  Matrix<float> wrong(nr, nr);                                                      // C not int
  if (to_info(grb_bcc(wrong.handle(), NULL, a.handle(), GRB_BCC_BLOCKS, NULL, NULL)) != GrB_DOMAIN_MISMATCH) return 12;
  if (to_info(grb_bcc(blocks.handle(), NULL, a.handle(), 2, NULL, NULL)) != GrB_INVALID_VALUE) return 13;
  printf("ok\n");
  return 0;
}
