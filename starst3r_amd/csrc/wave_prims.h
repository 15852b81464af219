// Wave64 and workgroup primitives shared by the scans (scan.h, gs_isect.hip) and the radix sort (radix_sort.hip): the one
// place that spells the shuffle ladder, the 4-wave block scan and the ballot match.  Every caller runs whole waves through
// them (no divergent call), and threadIdx.x is the thread's only coordinate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct WaveAdd { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct WaveMax { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return max(a, b); } };

// inclusive scan over the 64 lanes of a wave (Op: WaveAdd -- prefix sum --, WaveMax -- prefix maximum)
template <typename Op = WaveAdd, typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(v, off);
        if (lane >= off) v = Op()(v, t);
    }
    return v;
}

// the value of the lane below; `first` in lane 0 (an inclusive scan shifted into an exclusive one)
template <typename T>
__device__ __forceinline__ T wave_prev(T v, T first) {
    const T t = __shfl_up(v, 1);
    return (threadIdx.x & 63) == 0 ? first : t;
}

// inclusive scan of one value per thread over a workgroup of 256 threads (4 waves); *total receives the workgroup's sum.
// Two barriers: the second one lets the next call reuse the wave sums.
template <typename T>
__device__ __forceinline__ T block_incl_scan(T v, T* total) {
    __shared__ T wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const T inc = wave_incl_scan(v);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    T base = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) base += i < w ? wsum[i] : T(0);
    *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    return inc + base;
}

// "match-any" on the low `nbits` bits of `digit`: declares `m`, the ballot mask of the valid lanes of the wave that hold this
// lane's digit (one ballot per digit bit; an invalid lane gets the mask of the valid lanes that share ITS digit and must not
// use it).  A macro, not a function: every function form tried -- forced or plain inline, template or run-time bit count,
// result returned or stored -- left k_rs_pass<uint32_t, 512, 8> (radix_sort.hip) with the instructions of its look-back loop
// in another order and two more VGPRs; the expanded text compiles to the kernels the hand-written loops gave.
#define WAVE_MATCH(m, valid, digit, nbits)                 \
    unsigned long long m = __ballot(valid);                \
    for (int b_ = 0; b_ < (nbits); ++b_) {                 \
        const bool bit = ((digit) >> b_) & 1u;             \
        const unsigned long long bal = __ballot(bit);      \
        m &= bit ? bal : ~bal;                             \
    }
