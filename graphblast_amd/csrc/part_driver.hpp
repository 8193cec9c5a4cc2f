// part_driver.hpp -- the launch rule of the partitioned traversals whose loop runs on the device (bfs_part_run.hip,
// sssp_part_run.hip), once.  Plain C++: no HIP header, a host compiler accepts it (tests/test_part_driver_model.py).
//
// A traversal is a chain of launches on one stream, launch k followed by its exchange.  The host sees ONE 8-byte word of
// pinned memory, which every launch of rank 0 overwrites when it has finished (one relaxed system-scope store: the data is
// the flag):  low half = launches completed, k + 1;  high half = 0 while the traversal goes on, e + 1 once launch e has
// ended it, 0xffffffff when a grid barrier gave up (distress).
// The rule: launch k goes out when launch k - 2 has reported and had not ended the traversal, so the device always has
// launch k - 1 queued behind the one that runs and never waits for the host.  It reads only what launch k - 2 computed --
// the same on every rank -- so every rank enqueues the same number of launches and collectives: (the ending launch's
// index) + 2; a launch that finds the traversal finished exits at once.  One-shot (one rank whose first launch may run
// every level): launch 0 alone goes out and the word is not read here.
// A word that does not advance: every 4096 reads the clock is looked at; once limit_seconds have passed since the loop
// began, stall() is called, once -- it waits for the stream, after which every enqueued launch has reported -- and a word
// that still lags at the next look is GRB_PANIC.
#pragma once
#include <chrono>
#include "grb_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GRB_PART_HD __host__ __device__
#else
#define GRB_PART_HD
#endif

namespace grb {

struct PartMailWord { int launches_done, done_at; };   // done_at: the launch that ended the traversal; -1 none yet; -2 distress
GRB_PART_HD inline PartMailWord part_mail_decode(unsigned long long g) {
  const unsigned int hi = (unsigned int)(g >> 32);
  return {(int)(g & 0xffffffffull), hi == 0xffffffffu ? -2 : (int)hi - 1};
}
GRB_PART_HD inline unsigned long long part_mail_encode(int k, int done_at, bool bad) {   // what launch k leaves
  const unsigned long long hi = bad ? 0xffffffffull : (unsigned long long)(unsigned)(done_at + 1);
  return (hi << 32) | (unsigned long long)(unsigned)(k + 1);
}

// peek() -> the word; enqueue(k) -> grb_info: launch k of every rank and its exchange; stall() -> grb_info.  GRB_SUCCESS:
// *launches went out.  GRB_PANIC: distress, or a lagging word; whatever else enqueue or stall returned ends the loop.
template <typename Peek, typename Enqueue, typename Stall>
inline grb_info part_drive(Peek peek, Enqueue enqueue, Stall stall, int limit_seconds, bool one_shot, int* launches) {
  const auto t0 = std::chrono::steady_clock::now();
  int k = 0;
  for (;;) {
    if (k >= 2) {
      unsigned spins = 0;
      bool stalled = false;
      PartMailWord m;
      for (;;) {
        m = part_mail_decode(peek());
        if (m.launches_done >= k - 1) break;
        if ((++spins & 4095u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(limit_seconds)) {
          if (stalled) return GRB_PANIC;
          if (const grb_info si = stall()) return si;
          stalled = true;
        }
      }
      if (m.done_at == -2) return GRB_PANIC;
      if (m.done_at >= 0 && m.done_at <= k - 2) break;
    }
    if (const grb_info ei = enqueue(k)) return ei;
    ++k;
    if (one_shot) break;
    if (k > (1 << 28)) return GRB_PANIC;
  }
  *launches = k;
  return GRB_SUCCESS;
}

}  // namespace grb
