// What the persistent kernels (bblock.hip, bblockx3.hip, bneckx3.hip, conv_tt.hip, the fused heads) share: buffer descriptors and the
// LDS-DMA piece, the phase clock of the tuning traces, the per-XCD shares and the re-arming of ticket words, the LDS counters' polls
// on the device; the grid, the large-LDS opt-in, the trace scope and the profiling-event guard on the host (host parts: api.cpp).
#pragma once
#include "common.hpp"

namespace sncal {

// ---- device half ----------------------------------------------------------------------------------------------------------------------
// Word 3 of a buffer descriptor: a raw buffer of 32-bit data; offsets at or beyond the descriptor's size read zeros and drop stores.
constexpr int BUF_FLAGS = 0x00020000;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, BUF_FLAGS);
}
// Offsets that are out of range of every descriptor a kernel builds -- how a lane opts out of a load (zeros) or a store (dropped).
// BUF_OOB is for descriptors below 2 GB.  bblockx3's descriptors span the whole batch (the launcher accepts up to 0xf0000000 bytes):
// BUF_OOB_WIDE lies beyond those and leaves room for the instruction's constant and scalar offsets (< 512) without wrapping.
constexpr unsigned BUF_OOB = 0x80000000u, BUF_OOB_WIDE = 0xfffffe00u;

// One LDS-DMA piece (64 lanes x 16 bytes -> 1 KB at LDS byte address `lds_addr`) as inline assembly, with its descriptor as four plain
// words.  The builtin form (__builtin_amdgcn_raw_ptr_buffer_load_lds) makes hipcc's wait-count pass treat every later ds_read as a
// possible reader of the DMA's destination and put `s_waitcnt vmcnt(0)` in front of it, i.e. wait for the NEXT tile's / slice's pieces
// before multiplying this one's (bblock48: ~3k of 13k clk per tile; bblockx3: in front of the loader waves' counter polls).  The pass
// does not see the assembly: a kernel that uses dma_piece orders its DMA by explicit s_waitcnt + barriers / LDS counters.
typedef int i32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void dma_piece(i32x4_t rsrc, unsigned lds_addr, unsigned voff, unsigned soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" : : "s"(lds_addr), "v"(voff), "s"(rsrc), "s"(soff) : "memory", "m0");
}
__device__ __forceinline__ i32x4_t raw_rsrc(const void* base, unsigned bytes) {
    const unsigned long long a = reinterpret_cast<unsigned long long>(base);
    return i32x4_t{(int)(unsigned)a, (int)(unsigned)((a >> 32) & 0xffffu), (int)bytes, BUF_FLAGS};
}

// Phase clock of the tuning traces (SNCAL_*_TRACE): lap(k) adds the clocks since the previous stamp to slot k.  What the slots mean
// and where a wave's slots go in the trace is the kernel's business (documented there; read by tools/*_trace.py), and so is the loop
// that writes `sum` out: behind a call hipcc lays bblock48 out differently (profiles/persist_frame.md).  The fused heads keep a clock of
// their own for the same reason (head32.hip, headx3.hip).
struct PhaseClock {
    unsigned long long sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, prev = 0;
    const bool on;
    __device__ __forceinline__ explicit PhaseClock(const void* trace) : on(trace != nullptr) {}
    __device__ __forceinline__ void start() { if (on) prev = __builtin_amdgcn_s_memtime(); }
    __device__ __forceinline__ void lap(int k) { if (on) { const unsigned long long now = __builtin_amdgcn_s_memtime(); sum[k] += now - prev; prev = now; } }
};

// Workgroup b runs on XCD b % 8: the XCD's contiguous share [lo, hi) of n work items cut into eight.
__device__ __forceinline__ void xcd_share(int n, int xcd, int& lo, int& hi) {
    lo = (int)((long)n * xcd / 8);
    hi = (int)((long)n * (xcd + 1) / 8);
}

// Leaving a ticket queue (one lane per leaver, `per_wg` leavers in every workgroup of the launch).  The queue is `n_words` device words,
// the last of them the count of leavers.  Every leaver holds exactly one failing ticket, so once all of them have been counted nobody
// touches the words any more and the last one re-arms them for the next launch on this stream.  (conv_tt counts its leavers per XCD:
// conv_tt_kernel.hpp.)
__device__ __forceinline__ void ticket_leave(unsigned* words, int n_words, unsigned per_wg) {
    if (atomicAdd(words + n_words - 1, 1u) == gridDim.x * per_wg - 1u) {
#pragma unroll
        for (int i = 0; i < n_words; ++i) words[i] = 0u;
        __threadfence();
    }
}

// Counters in LDS that the waves of a workgroup hand work over with: a relaxed read, and a wait until the counter has reached `target`.
__device__ __forceinline__ unsigned poll(unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void spin_until(unsigned* p, unsigned target) {
    while ((int)(poll(p) - target) < 0) __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");
}

// ---- host half ------------------------------------------------------------------------------------------------------------------------
// Grid of a persistent launch: one workgroup per CU, rounded down to a multiple of the 8 XCDs; 256 when the CU count is unknown.
inline int persistent_grid(int n_cus) { return n_cus >= 8 ? n_cus / 8 * 8 : 256; }

// More than 64 KB of dynamic LDS needs an opt-in per kernel: done by the first call, once per process (not per device), for every
// kernel named.  False when the runtime refuses (the reason is in set_error; the call after it tries again): a launcher that returns
// a status returns SNCAL_ERR_HIP, one that cannot goes on and the launch that follows fails its check.
bool opt_in_lds_kernel(const void* kernel, int bytes);
template <auto... Kernels>
bool opt_in_lds(int bytes) {
    static bool done = false;
    if (!done) done = (opt_in_lds_kernel(reinterpret_cast<const void*>(Kernels), bytes) && ...);
    return done;
}

// Phase trace of ONE launch: with a dump file named (null: no trace), `words` is n zeroed 64-bit device words on `stream` for the
// kernel's `trace` parameter (null when the allocation fails); leaving the scope synchronises the stream, writes the words to the
// file -- every launch overwrites it: the file holds the last traced launch of the run -- and frees them.  Whether to trace (the
// SNCAL_*_TRACE switch, read once per process, and any further condition) is the caller's.
struct TraceScope {
    unsigned long long* words = nullptr;
    TraceScope(const char* file, size_t n, hipStream_t stream);
    ~TraceScope();
    TraceScope(const TraceScope&) = delete;
    TraceScope& operator=(const TraceScope&) = delete;
private:
    const char* file_;
    size_t n_;
    hipStream_t stream_;
};

// Takes the armed profiling event pair (launch_events) away while helper kernels in front of an op's own launch run -- the pair times
// that launch, not them -- and gives it back on every way out of the scope.
struct LaunchEventsHold {
    const LaunchEvents armed;
    LaunchEventsHold() : armed(launch_events()) { launch_events() = LaunchEvents{}; }
    ~LaunchEventsHold() { launch_events() = armed; }
    LaunchEventsHold(const LaunchEventsHold&) = delete;
    LaunchEventsHold& operator=(const LaunchEventsHold&) = delete;
};

}  // namespace sncal
