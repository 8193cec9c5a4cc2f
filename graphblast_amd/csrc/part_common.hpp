// part_common.hpp -- the HIP side of what the two partitioned traversals with their loop on the device share
// (bfs_part_run.hip, sssp_part_run.hip); the launch rule and the mail word are part_driver.hpp's.  The carry and state
// structs stay with their kernels: their fields differ.
#pragma once
#include "part_driver.hpp"
#include "persist_common.hpp"

namespace grb {

// the group runs' stand-in for the all-gather: every rank's send buffer into slot r of every rank's receive buffer, one
// launch (all ranks live on this device)
constexpr int kLoopMaxRanks = 16;
struct LoopbackPtrs {
  const unsigned int* send[kLoopMaxRanks];
  unsigned int* recv[kLoopMaxRanks];
};
static __global__ __launch_bounds__(kBlock) void loopback_allgather_kernel(LoopbackPtrs p, int world, int nwords) {
  const long long total = (long long)world * nwords;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
    const int r = (int)(i / nwords);
    const unsigned int x = p.send[r][i - (long long)r * nwords];
    for (int q = 0; q < world; ++q) p.recv[q][i] = x;
  }
}
static inline grb_info loopback_allgather(const LoopbackPtrs& p, int world, int nwords, hipStream_t s) {
  hipLaunchKernelGGL(loopback_allgather_kernel, dim3(stream_grid((long long)world * nwords)), dim3(kBlock), 0, s, p, world, nwords);
  GRB_HIP_TRY(hipGetLastError());
  return GRB_SUCCESS;
}

// a real run of a world > 1: the library's communicator is this partition's
inline bool part_comm_matches(int rank, int world) {
  int r = -1, w = 0;
  grb_comm_info(&r, &w);
  return w == world && r == rank;
}

// a rank's mailbox: 256 pinned bytes -- the mail word, and from byte 64 the carry record as the ending launch leaves it --
// and the two events around a traversal's device work
struct PartMail {
  unsigned long long *h_mail = nullptr, *d_mail = nullptr;   // pinned, and its device-side address
  hipEvent_t ev0 = nullptr, ev1 = nullptr;

  grb_info create() {
    if (hipHostMalloc((void**)&h_mail, 256, hipHostMallocMapped) != hipSuccess) return GRB_OUT_OF_MEMORY;
    memset(h_mail, 0, 256);
    if (hipHostGetDevicePointer((void**)&d_mail, h_mail, 0) != hipSuccess) return GRB_PANIC;
    return hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess ? GRB_PANIC : GRB_SUCCESS;
  }
  void destroy() {
    if (h_mail) (void)hipHostFree(h_mail);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
  // before a traversal's first launch (nothing of this device is in flight: every run ends synchronised)
  void reset() { __atomic_store_n(h_mail, 0ull, __ATOMIC_RELEASE); }
  unsigned long long peek() const { return __atomic_load_n(h_mail, __ATOMIC_ACQUIRE); }
  template <typename Carry>
  Carry* d_carry() const { return reinterpret_cast<Carry*>(d_mail + 8); }
  // after the final synchronisation: the record of the launch that ended the traversal; GRB_PANIC when none did
  template <typename Carry>
  grb_info read_carry(Carry* cy) const {
    static_assert(sizeof(Carry) <= 256 - 64, "the result record follows the mail word in pinned memory");
    memcpy(cy, h_mail + 8, sizeof(Carry));
    return part_mail_decode(peek()).done_at < 0 || !cy->done ? GRB_PANIC : GRB_SUCCESS;
  }
  // the launch loop on this mailbox, behind the first event; a word that lags past the limit gets one wait for the stream
  template <typename Enqueue>
  grb_info drive(hipStream_t s, Enqueue enqueue, int limit_seconds, bool one_shot, int* launches) const {
    GRB_HIP_TRY(hipEventRecord(ev0, s));
    auto wait_stream = [&]() -> grb_info { GRB_HIP_TRY(hipStreamSynchronize(s)); return GRB_SUCCESS; };
    return part_drive([&] { return peek(); }, enqueue, wait_stream, limit_seconds, one_shot, launches);
  }
  grb_info elapsed_ms(hipStream_t s, float* ms) const {    // the second event; waits for everything enqueued on s
    GRB_HIP_TRY(hipEventRecord(ev1, s));
    GRB_HIP_TRY(hipEventSynchronize(ev1));
    GRB_HIP_TRY(hipEventElapsedTime(ms, ev0, ev1));
    return GRB_SUCCESS;
  }
};

// device: launch k has finished, with the carry y -- one 8-byte word, the data is the flag.  (The carry by reference, as the
// kernels' own lambdas took it: by value the BFS kernel spills a register.)
template <typename Carry>
__device__ __forceinline__ void part_report(unsigned long long* mail, int k, const Carry& y, bool bad) {
  __hip_atomic_store(mail, part_mail_encode(k, y.done_at, bad), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace grb
