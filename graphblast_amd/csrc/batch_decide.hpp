// batch_decide.hpp -- the bit-parallel sweep's direction rule (bfs_batch.hip), once, for the host loop and for the
// device's totals kernel.  Plain C++: no HIP header, a host compiler accepts it (tests/test_batch_decide_model.py).
//
// Per source s of the k: nf_s = the pairs its frontier holds, mf_s = their out-degrees.  A live source (nf_s > 0) is
//   pulled  when its own frontier passed the reference's switch point (nf_s > switchpoint * n), or
//           when the out-edges of all sources under that point exceed budget * nvals: then the heaviest of them are
//           pulled as well, in the order mf descending, source index ascending, until the rest fits;
//   pushed  otherwise.
// The serial form of the second clause -- walk the order, pull while the running sum is over the budget, take the
// pulled source's mf off it -- pulls a PREFIX of that order (the sum only falls), so source s is pulled exactly when
// (sum over all sources under the point) - (sum over those of them before s in the order) is over the budget.  That form
// needs no sorted array: a lane per source counts its predecessors.  Every sum is a sum of integers below 2^53 (at most
// 64 * nvals), exact in doubles in any order and equal to the integer sum: both forms compare the same doubles.
//
// The finishing rule, after the per-source decisions.  A source near its END is under the switch point too, because almost
// nothing is left for it to find -- and pushing it costs a pass over all n frontier words and a pass to count what arrived,
// for a few thousand edges.  The rows that still lack its bit are rows the level's pull walks anyway.  U = the in-edges of
// the rows that the pull of the level before left open (lacking a bit of some source it pulled), known and complete only
// when that level pulled EVERY live source.  When the rule is push-pull, the per-source decisions pull some sources and
// push others, U is known and U <= finish_limit * nvals, the pushed sources are pulled as well: q |= p, p = 0.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GRB_DECIDE_HD __host__ __device__
#else
#define GRB_DECIDE_HD
#endif

namespace grb {

enum BatchDecideMode { kDecidePushPull = 0, kDecidePushOnly = 1, kDecidePullOnly = 2 };
enum BatchDecideKind {
  kDecideDone = 0,    // no live source, or no iteration left: the label pass follows
  kDecideLight = 1,   // every live source pushed and few edges to push: the light-level launch
  kDecideHost = 2     // a level of the host loop: pull kernels for qmask, push kernels for pmask
};

struct BatchRule {
  int k;
  long long n, nvals;
  int mode;             // BatchDecideMode
  float switchpoint;
  double budget;        // share of nvals that may be pushed in one level
  double tail_limit;    // out-edges a level may push inside the light-level launch; 0: no such launch
  double finish_limit = -1.0;   // the finishing rule: the share of nvals up to which the open rows' in-edges make a level
                                // pull its pushed sources too; below 0: no such rule
};

constexpr long long kOpenUnknown = -1;   // U of the level before: not counted, or that level did not pull every live source

struct BatchDecision {
  unsigned long long qmask, pmask;   // bits pulled / pushed
  double pushed_edges;               // the out-edges of the pushed sources
  int kind;                          // BatchDecideKind
  unsigned long long stash;          // a heavy host level: pmask (batch_decide_stash), else 0
};

// source s is live and under the switch point: pushed, if the budget allows
GRB_DECIDE_HD inline bool batch_decide_under(const unsigned long long* nf_s, int s, const BatchRule& r) {
  return s < r.k && nf_s[s] != 0 && !((double)nf_s[s] > (double)r.switchpoint * (double)r.n);
}

// source s alone: 0 dead, 1 pushed, 2 pulled.  `under`: bit t = batch_decide_under(t), for every source (the device
// gets it from one ballot).  The two sums are kept as integers and turned into a double once: the same number.
GRB_DECIDE_HD inline int batch_decide_source(const unsigned long long* nf_s, const unsigned long long* mf_s, int s,
                                             const BatchRule& r, unsigned long long under) {
  if (s >= r.k || nf_s[s] == 0) return 0;
  if (r.mode == kDecidePullOnly) return 2;
  if (r.mode == kDecidePushOnly) return 1;
  if (!((under >> s) & 1ull)) return 2;
  const unsigned long long mine = mf_s[s];
  unsigned long long pushed = 0, before = 0;
  for (int t = 0; t < r.k; ++t) {
    if (!((under >> t) & 1ull)) continue;
    const unsigned long long m = mf_s[t];
    pushed += m;
    if (m > mine || (m == mine && t < s)) before += m;
  }
  return (double)(pushed - before) > r.budget * (double)r.nvals ? 2 : 1;
}

// what kind of level the masks make
GRB_DECIDE_HD inline int batch_decide_kind(unsigned long long qmask, unsigned long long pmask, double pushed_edges,
                                           const BatchRule& r, bool iteration_left) {
  if (!iteration_left || (qmask | pmask) == 0) return kDecideDone;
  if (r.tail_limit > 0 && qmask == 0 && pushed_edges <= r.tail_limit) return kDecideLight;
  return kDecideHost;
}

// A host level is HEAVY when its pushed sources bring more out-edges than half the vertices: the push kernels then only
// claim in `seen`, and the commit pass tells the new bits from the old by the pushed sources' old seen-bits, which the
// pull pass in front has stashed in the level's own words.  `stash` = the bit columns that carry them: pmask on a heavy
// level of the host loop, 0 on every other level.  pushed_edges is an integer below 2^53 whoever summed it.
GRB_DECIDE_HD inline bool batch_decide_heavy(double pushed_edges, long long n) { return pushed_edges > 0.5 * (double)n; }
GRB_DECIDE_HD inline unsigned long long batch_decide_stash(unsigned long long pmask, double pushed_edges, long long n, int kind) {
  return kind == kDecideHost && pmask != 0 && batch_decide_heavy(pushed_edges, n) ? pmask : 0ull;
}

// the finishing rule: the level that would pull q and push p pulls both
GRB_DECIDE_HD inline bool batch_decide_finish(unsigned long long qmask, unsigned long long pmask, const BatchRule& r, long long open_u) {
  return r.mode == kDecidePushPull && qmask != 0 && pmask != 0 && open_u >= 0 && r.finish_limit >= 0 &&
         (double)open_u <= r.finish_limit * (double)r.nvals;
}

GRB_DECIDE_HD inline BatchDecision batch_decide(const unsigned long long* nf_s, const unsigned long long* mf_s,
                                                const BatchRule& r, bool iteration_left, long long open_u = kOpenUnknown) {
  BatchDecision d;
  d.qmask = 0; d.pmask = 0; d.pushed_edges = 0;
  unsigned long long under = 0;
  for (int s = 0; s < r.k; ++s)
    if (batch_decide_under(nf_s, s, r)) under |= 1ull << s;
  for (int s = 0; s < r.k; ++s) {
    const int w = batch_decide_source(nf_s, mf_s, s, r, under);
    if (w == 2) d.qmask |= 1ull << s;
    if (w == 1) { d.pmask |= 1ull << s; d.pushed_edges += (double)mf_s[s]; }
  }
  if (batch_decide_finish(d.qmask, d.pmask, r, open_u)) { d.qmask |= d.pmask; d.pmask = 0; d.pushed_edges = 0; }
  d.kind = batch_decide_kind(d.qmask, d.pmask, d.pushed_edges, r, iteration_left);
  d.stash = batch_decide_stash(d.pmask, d.pushed_edges, r.n, d.kind);
  return d;
}

// The sweep's first level as a plain launch (batch_first_level_kernel): source s's row is cut into pieces of `piece`
// edges, pre[s] .. pre[s + 1] are its pieces, pre[k] is the grid's wave count.  An empty row has no piece; a vertex
// named twice has its pieces twice.  k <= 64, pre holds k + 1 entries (the rest, up to 65, is zeroed).
template <typename I>
inline void first_level_pieces(const I* row_ptr, const I* sources, int k, int piece, unsigned int* pre) {
  unsigned int at = 0;
  for (int s = 0; s <= 64; ++s) {
    pre[s] = at;
    if (s < k) {
      const long long deg = (long long)row_ptr[(long long)sources[s] + 1] - (long long)row_ptr[sources[s]];
      at += (unsigned int)((deg + piece - 1) / piece);
    }
  }
}

}  // namespace grb
