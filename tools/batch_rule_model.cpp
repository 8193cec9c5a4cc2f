// batch_rule_model.cpp -- the bit-parallel sweep's levels on the host, decided by the library's own rule.
//
//   batch_rule_model GRAPH [switchpoint budget finish_limit tail_edges max_niter]
//
// GRAPH is what tools/batch_rule_model.py writes: int64 {n, nnz, k}, int32 sources[k], int32 optr[n + 1], oind[nnz],
// iptr[n + 1], iind[nnz].  The directions of every level come from batch_decide.hpp -- the header the host loop and the
// totals kernel of csrc/bfs_batch.hip use -- so this is the rule itself, not a restatement.  Per level of the host loop:
// sources pulled and pushed, in-entries inspected by the pull (exact: up to the entry that completes a row; quotas: as
// batch_pull_kernel takes them, the hint, four serial probes, then 32, 128, 512 ... entries a round, a big row in
// 4096-entry slices read 256 entries a step), out-edges pushed, and U, the in-edges of the rows the pull left open --
// what GRB_BATCH_TRACE prints for the same graph and sources.  Levels inside a light-level launch are one line.
#include "batch_decide.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef unsigned long long u64;

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s GRAPH [switchpoint budget finish_limit tail_edges max_niter]\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int64_t head[3];
  if (fread(head, sizeof(int64_t), 3, f) != 3) return 2;
  const int64_t n = head[0], nnz = head[1];
  const int k = (int)head[2];
  if (n < 1 || nnz < 0 || k < 1 || k > 64) { fprintf(stderr, "bad header\n"); return 2; }
  std::vector<int32_t> src(k), optr(n + 1), oind(nnz), iptr(n + 1), iind(nnz);
  auto rd = [&](std::vector<int32_t>& v) { return v.empty() || fread(v.data(), sizeof(int32_t), v.size(), f) == v.size(); };
  if (!rd(src) || !rd(optr) || !rd(oind) || !rd(iptr) || !rd(iind)) { fprintf(stderr, "short file\n"); return 2; }
  fclose(f);

  grb::BatchRule rule;
  rule.k = k; rule.n = n; rule.nvals = nnz; rule.mode = grb::kDecidePushPull;
  rule.switchpoint = argc > 2 ? (float)atof(argv[2]) : 0.01f;
  rule.budget = argc > 3 ? atof(argv[3]) : 0.15;
  rule.finish_limit = argc > 4 ? atof(argv[4]) : 0.01;
  rule.tail_limit = argc > 5 ? atof(argv[5]) : 1048576.0;
  const int max_niter = argc > 6 ? atoi(argv[6]) : 1 << 30;
  const int kBig = 4096, kSlice = 4096, kSerial = 4;

  // the pull hint: a vertex's in-neighbour of largest out-degree (the first of equals)
  std::vector<int32_t> hint(n, 0);
  for (int64_t v = 0; v < n; ++v) {
    int64_t best = -1;
    for (int32_t p = iptr[v]; p < iptr[v + 1]; ++p) {
      const int64_t d = optr[iind[p] + 1] - optr[iind[p]];
      if (d > best) { best = d; hint[v] = iind[p]; }
    }
  }
  std::vector<u64> seen(n, 0), fcur(n, 0), fnext(n, 0);
  u64 nf[64] = {0}, mf[64] = {0};
  for (int s = 0; s < k; ++s) {
    seen[src[s]] |= 1ull << s;
    fcur[src[s]] |= 1ull << s;
    nf[s] = 1;
    mf[s] = (u64)(optr[src[s] + 1] - optr[src[s]]);
  }
  long long open_u = grb::kOpenUnknown;
  // one level: pull the bits Q, push the bits P; returns the pairs discovered
  struct Level { u64 exact = 0, quota = 0, pushed = 0, U = 0, pairs = 0; };
  auto run_level = [&](u64 Q, u64 P) {
    Level L;
    for (int64_t v = 0; v < n; ++v) fnext[v] = 0;
    if (Q)
      for (int64_t v = 0; v < n; ++v) {
        const u64 need = ~seen[v] & Q;
        const int32_t p0 = iptr[v], e = iptr[v + 1];
        if (!need || p0 == e) continue;
        u64 acc = fcur[hint[v]];
        ++L.exact; ++L.quota;
        int32_t p = p0;
        for (; p < e && (acc & need) != need; ++p) { acc |= fcur[iind[p]]; ++L.exact; }
        // the same row as the kernels walk it
        u64 a2 = fcur[hint[v]];
        int32_t q = p0;
        for (int t = 0; t < kSerial && q < e && (a2 & need) != need; ++t) { a2 |= fcur[iind[q++]]; ++L.quota; }
        if (e - p0 >= kBig) {                               // slices, each on its own: 256 entries a step until the row is covered
          u64 got = a2;                                     // (the slices of a row run side by side: what one finds does not stop another)
          for (int32_t s0 = p0; s0 < e; s0 += kSlice) {
            u64 g = 0;
            const int32_t s1 = s0 + kSlice < e ? s0 + kSlice : e;
            for (int32_t c = s0; c < s1 && ((g | a2) & need) != need; c += 256) {
              const int32_t c1 = c + 256 < s1 ? c + 256 : s1;
              for (int32_t x = c; x < c1; ++x) g |= fcur[iind[x]];
              L.quota += (u64)(c1 - c);
            }
            got |= g;
          }
          a2 = got;
        } else {
          for (int32_t quota = 32; q < e && (a2 & need) != need;) {
            const int32_t c1 = e - q < quota ? e : q + quota;  // a round's entries are all read, then the row is tested
            L.quota += (u64)(c1 - q);
            for (; q < c1; ++q) a2 |= fcur[iind[q]];
            if (quota < (1 << 20)) quota *= 4;
          }
        }
        const u64 newb = acc & need;
        fnext[v] |= newb;
        if (need & ~newb) L.U += (u64)(e - p0);
      }
    if (P)
      for (int64_t u = 0; u < n; ++u) {
        const u64 fw = fcur[u] & P;
        if (!fw) continue;
        L.pushed += (u64)(optr[u + 1] - optr[u]);
        for (int32_t p = optr[u]; p < optr[u + 1]; ++p) fnext[oind[p]] |= fw & ~seen[oind[p]];
      }
    for (int s = 0; s < 64; ++s) nf[s] = mf[s] = 0;
    for (int64_t v = 0; v < n; ++v) {
      const u64 nb = fnext[v] & ~seen[v];
      fnext[v] = nb;
      if (!nb) continue;
      seen[v] |= nb;
      const u64 d = (u64)(optr[v + 1] - optr[v]);
      for (u64 t = nb; t; t &= t - 1) { const int s = __builtin_ctzll(t); ++nf[s]; mf[s] += d; ++L.pairs; }
    }
    fcur.swap(fnext);
    return L;
  };
  for (int iter = 1; iter <= max_niter; ++iter) {
    const grb::BatchDecision d = grb::batch_decide(nf, mf, rule, true, open_u);
    if (d.kind == grb::kDecideDone) break;
    if (d.kind == grb::kDecideLight) {                      // every live source pushed, level after level, while the out-edges stay under the limit
      const int first = iter;
      u64 pairs = 0;
      int status = 0;
      for (;;) {
        const Level L = run_level(0, ~0ull);
        pairs += L.pairs;
        u64 edges = 0;
        for (int s = 0; s < k; ++s) edges += mf[s];
        if (L.pairs == 0) { status = 0; break; }
        if (iter >= max_niter) { status = 1; break; }
        if ((double)edges > rule.tail_limit) { status = 2; break; }
        ++iter;
      }
      printf("levels %d..%d: one launch (light levels), status %d, pairs %llu\n", first, iter, status, pairs);
      open_u = grb::kOpenUnknown;
      if (status == 0) break;
      continue;
    }
    const Level L = run_level(d.qmask, d.pmask);
    const bool complete = d.pmask == 0 && d.qmask != 0;
    printf("level %d: pull %d sources, push %d (%.0f edges) -> pairs %llu, inspected %llu exact %llu by quotas, qmask %llx pmask %llx, U %llu%s\n",
           iter, __builtin_popcountll(d.qmask), __builtin_popcountll(d.pmask), d.pushed_edges, L.pairs, L.exact, L.quota, d.qmask, d.pmask,
           L.U, complete ? "" : " (not complete)");
    open_u = complete ? (long long)L.U : grb::kOpenUnknown;
    if (L.pairs == 0) break;
  }
  return 0;
}
