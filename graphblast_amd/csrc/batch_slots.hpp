// batch_slots.hpp -- the word arrays of the bit-parallel sweep (bfs_batch.hip): which one a level reads, which it writes,
// which are kept for the label pass and which are known all-zero.  Plain C++ over slot indices: no HIP header, a host
// compiler accepts it (tests/test_batch_slots_model.py); the caller turns an index into a pointer.
//
// Slots 0 .. nstore are KEPT for the label pass, in order: the i-th kept level lives in slot i (slot 0 the seeds, or
// level 1 when the first level is the plain launch), and which level that is is recorded as the slot is taken.  Four
// more ROTATE (nstore + 1 .. nstore + 4): a level beyond the kept ones, which labels as it discovers, and the three
// arrays of a light-level launch.  A rotating array is CLEAN when it is known all-zero: the light-level launch needs
// its three so and leaves them so, and the knowledge survives from one sweep to the next.
//
// Where a level's words go is a PLAN until the level is known to be one of the host loop's: the pull kernels launched
// ahead write by it, and when the level turns out to be none (they then wrote nothing) the plan is dropped.  plan()
// changes nothing; commit() does.
#pragma once

namespace grb {

constexpr int kSlotsKeptMax = 17;       // at most (the seeds and 16 levels)
constexpr int kSlotsRotating = 4;

struct SlotPlan {
  bool keep;                            // a kept slot; else a rotating one (the level labels directly)
  int slot;
};

class BatchSlots {
 public:
  // a sweep starts: the seeds are kept level 0, in slot 0, and the frontier; clean[i]: rotating array i is all-zero
  void begin(int nstore, const bool* clean) {
    nstore_ = nstore;
    for (int i = 0; i < kSlotsRotating; ++i) clean_[i] = clean[i];
    nkept_ = 1;
    kept_level_[0] = 0;
    any_direct_ = false;
    frontier_ = 0;
  }
  // the first level needs no seed words (the seed kernel writes the sources' own labels): no frontier array, and slot 0
  // goes to level 1
  void first_plain() {
    nkept_ = 0;
    frontier_ = -1;
    any_direct_ = true;
  }

  int frontier() const { return frontier_; }                 // the slot the next level reads (-1: none)
  int nkept() const { return nkept_; }
  int kept_level(int i) const { return kept_level_[i]; }      // the iteration that wrote kept slot i (0: the seeds)
  bool any_direct() const { return any_direct_; }             // some label was written outside the label pass
  bool clean(int slot) const { return clean_[slot - nstore_ - 1]; }
  const bool* clean_flags() const { return clean_; }          // per rotating array, for the next sweep

  // where the level that reads the frontier writes: a kept slot while there are any, else a rotating array -- a dirty
  // one if there is one, so that the clean ones stay clean
  SlotPlan plan() const {
    SlotPlan p;
    p.keep = nkept_ <= nstore_;
    p.slot = p.keep ? nkept_ : pick(-1, -1, false);
    return p;
  }
  // iteration `iter` is a level of the host loop and writes by plan p; what it writes is the next frontier
  void commit(const SlotPlan& p, int iter) {
    if (p.keep) {
      kept_level_[nkept_] = iter;
      ++nkept_;
    } else {
      clean_[p.slot - nstore_ - 1] = false;
      any_direct_ = true;
    }
    frontier_ = p.slot;
  }

  // the three arrays of a light-level launch: distinct, none of them the frontier, clean ones first (a clean one needs no
  // memset)
  void light_pick(int x[3]) const {
    x[0] = pick(-1, -1, true);
    x[1] = pick(x[0], -1, true);
    x[2] = pick(x[0], x[1], true);
  }
  // the launch ran `done` >= 1 levels on x and ended with `status`: level j wrote x[j % 3], the last of them is the new
  // frontier, and every other array was left all-zero -- the frontier's too when the status is 0 (nothing new was found)
  void light_done(const int x[3], int done, int status) {
    for (int i = 0; i < 3; ++i) clean_[x[i] - nstore_ - 1] = true;
    frontier_ = x[(done - 1) % 3];
    if (status != 0) clean_[frontier_ - nstore_ - 1] = false;
    any_direct_ = true;
  }

 private:
  // a rotating slot other than the frontier, x and y: one whose cleanness is as wanted if there is one
  int pick(int x, int y, bool want_clean) const {
    int other = -1;
    for (int i = 0; i < kSlotsRotating; ++i) {
      const int slot = nstore_ + 1 + i;
      if (slot == frontier_ || slot == x || slot == y) continue;
      if (clean_[i] == want_clean) return slot;
      if (other < 0) other = slot;
    }
    return other;
  }

  int nstore_ = 1, nkept_ = 1, frontier_ = 0;
  int kept_level_[kSlotsKeptMax] = {0};
  bool clean_[kSlotsRotating] = {false, false, false, false};
  bool any_direct_ = false;
};

}  // namespace grb
