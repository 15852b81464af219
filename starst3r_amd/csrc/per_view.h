// What the per-view kernels share: the fixed-order block sum of doubles (gs_pose_bwd.hip, gs_blend_depth.hip and the
// two files below), the scaffold of the streaming per-view kernels (loss_depth.hip, gs_exposure.hip, gs_alpha.hip) with the
// weight sums of the weighted losses (loss_depth.hip, loss.hip, gs_alpha.hip), a two-switch kernel launch, and the core of
// the per-view Adam kernels (gs_pose_step.hip, gs_exposure.hip).  The device helpers are of the form DESIGN.md's "What
// the projection kernels share" arrives at: references in the order of first use, no arrays by value.
#pragma once
#include "stages.h"

// Sum of v[k] over the 256 threads of a workgroup in a fixed order (wave butterfly, then the four waves in order):
// thread k < NV returns the sum of v[k], the other threads 0.  red: 4 * NV doubles of LDS that no thread still reads
// (a loop around the call needs a barrier between one call's reads and the next call's writes).
template <int NV>
__device__ __forceinline__ double block_sum_fixed(double (&v)[NV], double* red) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) red[wv * NV + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x >= NV) return 0.0;
    const int k = threadIdx.x;
    return ((red[k] + red[NV + k]) + red[2 * NV + k]) + red[3 * NV + k];
}

// ---- streaming per-view kernels ----
// Nothing is re-read, so the arrangement is all there is to them.  A view's HW pixels are dealt to workgroups of
// STREAM_T threads in contiguous chunks, a multiple of STREAM_ALIGN pixels: four pixels per thread and access, so 16-byte
// accesses stay aligned whenever HW is a multiple of 4 and the buffers are (kernel<true>); otherwise -- an odd HW puts
// every second view on an unaligned base -- one pixel per thread and 4-byte accesses (kernel<false>).  The grid is
// (blocks, C), at most 2048 workgroups in all: eight per CU on the 256 CUs, one resident round of the chip and no partly
// filled second one.  A thread strides through its chunk.  Sums: every thread adds its pixels in double, the workgroup
// meets in block_sum_fixed, one partial of NV doubles per (view, workgroup); k_stream_finish, one workgroup per view,
// adds a view's partials the same way.  No atomics, a fixed order for a given shape: the same inputs give the same bits.
#define STREAM_T 256          // threads per workgroup
#define STREAM_ALIGN 1024     // chunk granularity in pixels: one 16-byte access per thread

// workgroups per view and pixels per workgroup: at least four pixels per thread, at most 256 x 8 workgroups in all (one
// resident round of the chip; the count is C times a per-view count, so it is not an exact multiple of 256)
static inline void stream_grid(int C, int64_t HW, int* blocks, int64_t* chunk) {
    int64_t want = (C * HW + STREAM_ALIGN - 1) / STREAM_ALIGN;
    if (want > 256 * 8) want = 256 * 8;
    int64_t b = want / C;
    if (b < 1) b = 1;
    int64_t ch = (HW + b - 1) / b;
    ch = (ch + STREAM_ALIGN - 1) / STREAM_ALIGN * STREAM_ALIGN;
    *chunk = ch;
    *blocks = (int)((HW + ch - 1) / ch);
}

// every pointer on a 16-byte boundary (NULL counts as aligned)
template <typename... P>
static inline bool aligned16(const P*... p) { return ((... | (uintptr_t)p) & 15) == 0; }

// the pixels [lo, hi) of its view that this workgroup walks
__device__ __forceinline__ void stream_chunk(const int64_t& chunk, const int64_t& HW, int64_t& lo, int64_t& hi) {
    lo = (int64_t)blockIdx.x * chunk; hi = min(HW, lo + chunk);
}

// kernel<true> if vec, else kernel<false>, on the grid of stream_grid; on failure the enclosing function returns
// the error code
#define STREAM_LAUNCH(kernel, vec, blocks, C, s, ...)                                                           \
    do {                                                                                                        \
        if (vec) hipLaunchKernelGGL(kernel<true>, dim3(blocks, C), dim3(STREAM_T), 0, s, __VA_ARGS__);          \
        else hipLaunchKernelGGL(kernel<false>, dim3(blocks, C), dim3(STREAM_T), 0, s, __VA_ARGS__);             \
        LAUNCH_CHECK();                                                                                         \
    } while (0)
// the same for a kernel with two switches, on any grid: kernel<a, b>
#define LAUNCH_BOOL2(kernel, a, b, grid, block, s, ...)                                                         \
    do {                                                                                                        \
        if (a) {                                                                                                \
            if (b) hipLaunchKernelGGL((kernel<true, true>), grid, block, 0, s, __VA_ARGS__);                    \
            else hipLaunchKernelGGL((kernel<true, false>), grid, block, 0, s, __VA_ARGS__);                     \
        } else {                                                                                                \
            if (b) hipLaunchKernelGGL((kernel<false, true>), grid, block, 0, s, __VA_ARGS__);                   \
            else hipLaunchKernelGGL((kernel<false, false>), grid, block, 0, s, __VA_ARGS__);                    \
        }                                                                                                       \
        LAUNCH_CHECK();                                                                                         \
    } while (0)

// one workgroup per view: its n_part partials of NV doubles in a fixed order -> out[c * stride + k] as OUT;
// at_least_one: max(sum, 1)
template <int NV, typename OUT>
__global__ __launch_bounds__(STREAM_T) void k_stream_finish(int n_part, const double* __restrict__ part,
                                                            OUT* __restrict__ out, int stride, int at_least_one) {
    __shared__ double red[4 * NV];
    const int c = blockIdx.x;
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
    for (int b = threadIdx.x; b < n_part; b += STREAM_T) {
        const double* p = part + ((int64_t)c * n_part + b) * NV;
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[k] += p[k];
    }
    const double t = block_sum_fixed(acc, red);
    if (threadIdx.x < NV) out[(int64_t)c * stride + threadIdx.x] = (OUT)(at_least_one ? fmax(t, 1.0) : t);
}

template <int NV, typename OUT>
static int stream_finish(hipStream_t s, int C, int blocks, const double* part, OUT* out, int stride, int at_least_one) {
    hipLaunchKernelGGL((k_stream_finish<NV, OUT>), dim3(C), dim3(STREAM_T), 0, s, blocks, part, out, stride, at_least_one);
    LAUNCH_CHECK();
    return ST3R_OK;
}

// The sums of a per-pixel weight map that normalise a weighted loss (loss_depth.hip, loss.hip): part[(c, workgroup)] =
// sum_p w of one chunk of view c, the weights that count (w > 0; a negative or NaN weight is 0) in double; INTERIOR: and
// after it sum_{p in I} w over the interior I of the SSIM term, the pixels WEIGHT_SUM_BORDER away from every edge -- that
// test needs the pixel's row and column, a division per access, which the plain sum does not pay (H and W: INTERIOR only).
#define WEIGHT_SUM_BORDER 5   // (loss.hip: HALO)
template <bool VEC, bool INTERIOR>
__global__ __launch_bounds__(STREAM_T) void k_weight_sums(int64_t HW, int64_t chunk, int H, int W,
                                                          const float* __restrict__ weight, double* __restrict__ part) {
    constexpr int NV = INTERIOR ? 2 : 1, B = WEIGHT_SUM_BORDER;
    __shared__ double red[4 * NV];
    const int c = blockIdx.y;
    const float* w = weight + (int64_t)c * HW;
    int64_t lo, hi;
    stream_chunk(chunk, HW, lo, hi);
    double acc[NV] = {};
    auto take = [&](int row, int col, float v) {
        const double d = (double)(v > 0.f ? v : 0.f);
        acc[0] += d;
        if constexpr (INTERIOR) {
            if (row >= B && row < H - B && col >= B && col < W - B) acc[1] += d;
        }
    };
    if (VEC) {
        for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi; i += 4 * STREAM_T) {
            const float4 v = *reinterpret_cast<const float4*>(w + i);
            const float e[4] = {v.x, v.y, v.z, v.w};
            int row = INTERIOR ? (int)(i / W) : 0, col = INTERIOR ? (int)(i - (int64_t)row * W) : 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                take(row, col, e[k]);
                if (INTERIOR && ++col == W) { col = 0; ++row; }
            }
        }
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += STREAM_T) {
            const int row = INTERIOR ? (int)(i / W) : 0;
            take(row, INTERIOR ? (int)(i - (int64_t)row * W) : 0, w[i]);
        }
    }
    const double t = block_sum_fixed(acc, red);
    if (threadIdx.x < NV) part[((int64_t)c * gridDim.x + blockIdx.x) * NV + (NV > 1 ? threadIdx.x : 0)] = t;
}

// ---- per-view Adam ----
// One thread per view, torch's formulas in double on float32 storage, behind the device-side guard of k_adam: a step
// that outgrew its buffers moves nothing.  A view with mask[c] == 0 keeps every bit.  Non-finite gradients are NOT
// filtered (torch's Adam does not filter them either).
struct PerViewAdamK {
    double lr, b1, b2, eps, bc1, bc2;
    const float* mask;
    const int32_t* count_dev;
    uint32_t count_cap;
};

// the view this thread updates, or -1: a guarded step, a thread past C, a frozen view
__device__ __forceinline__ int per_view_adam_view(const PerViewAdamK& k, const int& C) {
    if (k.count_dev && (uint32_t)k.count_dev[0] > k.count_cap) return -1;   // (see k_adam)
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return -1;
    if (k.mask && k.mask[c] == 0.0f) return -1;
    return c;
}

// the moments m, v of one scalar take its gradient g; returns delta = -lr mhat / (sqrt(vhat) + eps).
// Each update is a sum of two products, of which hipcc fuses one into an fma -- in the first moment not the same one in
// the two kernels, as they were written before they shared this function.  The fma is therefore spelled out, and M_LAST
// keeps each kernel's bits: true rounds (1 - b1) g and fuses b1 m (k_pose_adam), false the other way round
// (k_exposure_adam).  The second moment rounds b2 v in both.
template <bool M_LAST>
__device__ __forceinline__ double per_view_adam_delta(const PerViewAdamK& k, float& m, const double& g, float& v) {
    const double w1 = 1.0 - k.b1;
    const double mi = M_LAST ? fma(k.b1, (double)m, w1 * g) : fma(w1, g, k.b1 * (double)m);
    const double vi = fma((1.0 - k.b2) * g, g, k.b2 * (double)v);
    m = (float)mi; v = (float)vi;
    return -k.lr * (mi / k.bc1) / (sqrt(vi / k.bc2) + k.eps);
}

// launches kernel(C, k, args...), one thread per view, with the constants of Adam step `step` and the guard
template <typename... KA, typename... A>
static int per_view_adam_launch(st3r_ctx* ctx, hipStream_t s, void (*kernel)(int, PerViewAdamK, KA...), int C, double lr,
                                double b1, double b2, double eps, int step, const float* mask, A... args) {
    PerViewAdamK k;
    k.lr = lr; k.b1 = b1; k.b2 = b2; k.eps = eps;
    k.bc1 = 1.0 - pow(b1, (double)step); k.bc2 = 1.0 - pow(b2, (double)step);
    k.mask = mask;
    // an asynchronous step is in flight and its count not yet settled: guard the update with it (see k_adam)
    st3r_adam_guard(ctx, &k.count_dev, &k.count_cap);
    hipLaunchKernelGGL(kernel, dim3(ceil_div(C, 64)), dim3(64), 0, s, C, k, args...);
    LAUNCH_CHECK();
    return ST3R_OK;
}
