// Per-view exposure: an affine colour transform between the render and the loss (the `exposure` of the original 3DGS
// code, `app_opt` of gsplat's trainer), forward, backward and its Adam step.
//     E_c = [A_c | t_c]  [3,4] float32, row major         y_j = fmaf(A[j][2], b, fmaf(A[j][1], g, fmaf(A[j][0], r, t[j])))
//     v_x_i    = A[0][i] v_y_0 + A[1][i] v_y_1 + A[2][i] v_y_2      (float32, that order; v_x may be written over v_y)
//     v_A[j][i] = sum_p v_y_j(p) x_i(p)      v_t[j] = sum_p v_y_j(p)
//
// Two streaming kernels: 12 bytes in and 12 out per pixel forward, 24 in and 12 out backward, nothing re-read.  They are
// arranged as loss_depth.hip: a view's pixels are dealt to workgroups in contiguous chunks (a multiple of 1024 pixels: four
// pixels = three 16-byte accesses per thread stay aligned whenever H * W is a multiple of 4 and the buffers are; otherwise
// -- an odd H * W puts every second view on an unaligned base -- one pixel per thread and 4-byte accesses), the grid is at
// most 2048 workgroups (one resident round of the chip; st3r_stream_grid), a thread strides through its chunk.
// The twelve sums of a view: every product is (double)v_y * (double)x, every thread adds its pixels in double, the wave
// meets in a butterfly, the four waves in order, one 12-double partial per (view, workgroup); a second launch (one
// workgroup per view) adds a view's partials the same way and stores float32.  No atomics, a fixed order for a given
// shape: the same inputs give the same bits.
//
// Exposure Adam (k_exposure_adam) is k_pose_adam without the retraction: one thread per view, torch's formulas in double,
// behind the same device-side guard, a masked view keeps E, m and v bit for bit.  Non-finite gradients are NOT filtered.
#include "stages.h"

#define EX_T 256          // threads per workgroup

struct ExposureK { float a[12]; };   // one view's E, row major: a[4 j + i] = A[j][i], a[4 j + 3] = t[j]

__device__ __forceinline__ ExposureK ex_load(const float* __restrict__ exposure, int c) {
    ExposureK k;
#pragma unroll
    for (int i = 0; i < 12; ++i) k.a[i] = exposure[12 * c + i];
    return k;
}

__device__ __forceinline__ void ex_fwd_pixel(const ExposureK& k, float r, float g, float b, float* y) {
#pragma unroll
    for (int j = 0; j < 3; ++j) y[j] = fmaf(k.a[4 * j + 2], b, fmaf(k.a[4 * j + 1], g, fmaf(k.a[4 * j], r, k.a[4 * j + 3])));
}

template <bool VEC>
__global__ __launch_bounds__(EX_T) void k_exposure_fwd(int64_t HW, int64_t chunk, const float* __restrict__ rgb,
                                                       const float* __restrict__ exposure, float* __restrict__ out) {
    const int c = blockIdx.y;
    const ExposureK k = ex_load(exposure, c);
    const float* x = rgb + (int64_t)c * HW * 3;
    float* y = out + (int64_t)c * HW * 3;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = min(HW, lo + chunk);
    if (VEC) {
        for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi; i += 4 * EX_T) {   // pixels i .. i + 3: 12 floats
            alignas(16) float v[12], w[12];
            const float4* src = reinterpret_cast<const float4*>(x + 3 * i);
            *reinterpret_cast<float4*>(v) = src[0]; *reinterpret_cast<float4*>(v + 4) = src[1];
            *reinterpret_cast<float4*>(v + 8) = src[2];
#pragma unroll
            for (int p = 0; p < 4; ++p) ex_fwd_pixel(k, v[3 * p], v[3 * p + 1], v[3 * p + 2], w + 3 * p);
            float4* dst = reinterpret_cast<float4*>(y + 3 * i);
            dst[0] = *reinterpret_cast<float4*>(w); dst[1] = *reinterpret_cast<float4*>(w + 4);
            dst[2] = *reinterpret_cast<float4*>(w + 8);
        }
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += EX_T) {
            float w[3];
            ex_fwd_pixel(k, x[3 * i], x[3 * i + 1], x[3 * i + 2], w);
            y[3 * i] = w[0]; y[3 * i + 1] = w[1]; y[3 * i + 2] = w[2];
        }
    }
}

// one pixel of the backward: v_x out (vy may be the same three floats), its twelve terms added to acc
__device__ __forceinline__ void ex_bwd_pixel(const ExposureK& k, const float* x, const float* vy, float* vx, double* acc) {
    const float v0 = vy[0], v1 = vy[1], v2 = vy[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double vj = (double)(j == 0 ? v0 : (j == 1 ? v1 : v2));
        acc[4 * j] += vj * (double)x[0]; acc[4 * j + 1] += vj * (double)x[1]; acc[4 * j + 2] += vj * (double)x[2];
        acc[4 * j + 3] += vj;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) vx[i] = (k.a[i] * v0 + k.a[4 + i] * v1) + k.a[8 + i] * v2;
}

// twelve block sums: butterfly per wave, the four waves in order; red: [4][12]
__device__ __forceinline__ void ex_block_sum12(double* acc, double* red) {
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        double v = acc[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * 12 + q] = v;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = ((red[q] + red[12 + q]) + red[24 + q]) + red[36 + q];
}

// v_out and v_rgb may be the same buffer: a thread reads its pixels' v_y before it writes their v_x, and nobody else
// touches them (no __restrict__ on the two)
template <bool VEC>
__global__ __launch_bounds__(EX_T) void k_exposure_bwd(int64_t HW, int64_t chunk, const float* __restrict__ rgb,
                                                       const float* __restrict__ exposure, const float* v_out, float* v_rgb,
                                                       double* __restrict__ part) {
    __shared__ double red[48];
    const int c = blockIdx.y;
    const ExposureK k = ex_load(exposure, c);
    const int64_t base = (int64_t)c * HW * 3;
    const float* x = rgb + base;
    const float* vy = v_out + base;
    float* vx = v_rgb + base;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = min(HW, lo + chunk);
    double acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.0;
    if (VEC) {
        for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi; i += 4 * EX_T) {
            alignas(16) float xv[12], gv[12], ov[12];
            const float4* sx = reinterpret_cast<const float4*>(x + 3 * i);
            const float4* sg = reinterpret_cast<const float4*>(vy + 3 * i);
            *reinterpret_cast<float4*>(xv) = sx[0]; *reinterpret_cast<float4*>(xv + 4) = sx[1];
            *reinterpret_cast<float4*>(xv + 8) = sx[2];
            *reinterpret_cast<float4*>(gv) = sg[0]; *reinterpret_cast<float4*>(gv + 4) = sg[1];
            *reinterpret_cast<float4*>(gv + 8) = sg[2];
#pragma unroll
            for (int p = 0; p < 4; ++p) ex_bwd_pixel(k, xv + 3 * p, gv + 3 * p, ov + 3 * p, acc);
            float4* dst = reinterpret_cast<float4*>(vx + 3 * i);
            dst[0] = *reinterpret_cast<float4*>(ov); dst[1] = *reinterpret_cast<float4*>(ov + 4);
            dst[2] = *reinterpret_cast<float4*>(ov + 8);
        }
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += EX_T) {
            const float xs[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
            const float gs[3] = {vy[3 * i], vy[3 * i + 1], vy[3 * i + 2]};
            float os[3];
            ex_bwd_pixel(k, xs, gs, os, acc);
            vx[3 * i] = os[0]; vx[3 * i + 1] = os[1]; vx[3 * i + 2] = os[2];
        }
    }
    ex_block_sum12(acc, red);
    if (threadIdx.x < 12) {
        double t = acc[0];
#pragma unroll
        for (int q = 1; q < 12; ++q) t = threadIdx.x == q ? acc[q] : t;
        part[((int64_t)c * gridDim.x + blockIdx.x) * 12 + threadIdx.x] = t;
    }
}

// one workgroup per view: its n_part 12-double partials in a fixed order -> v_exposure[c] as float32
__global__ __launch_bounds__(EX_T) void k_exposure_finish(int n_part, const double* __restrict__ part,
                                                          float* __restrict__ v_exposure) {
    __shared__ double red[48];
    const int c = blockIdx.x;
    double acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.0;
    for (int b = threadIdx.x; b < n_part; b += EX_T) {
        const double* p = part + ((int64_t)c * n_part + b) * 12;
#pragma unroll
        for (int q = 0; q < 12; ++q) acc[q] += p[q];
    }
    ex_block_sum12(acc, red);
    if (threadIdx.x < 12) {
        double t = acc[0];
#pragma unroll
        for (int q = 1; q < 12; ++q) t = threadIdx.x == q ? acc[q] : t;
        v_exposure[12 * c + threadIdx.x] = (float)t;
    }
}

static bool ex_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int st3r_exposure_fwd_impl(hipStream_t s, int C, int H, int W, const float* rgb, const float* exposure, float* out) {
    const int64_t HW = (int64_t)H * W;
    int blocks; int64_t chunk;
    st3r_stream_grid(C, HW, &blocks, &chunk);
    if (HW % 4 == 0 && ex_al16(rgb) && ex_al16(out))
        hipLaunchKernelGGL(k_exposure_fwd<true>, dim3(blocks, C), dim3(EX_T), 0, s, HW, chunk, rgb, exposure, out);
    else
        hipLaunchKernelGGL(k_exposure_fwd<false>, dim3(blocks, C), dim3(EX_T), 0, s, HW, chunk, rgb, exposure, out);
    LAUNCH_CHECK();
    return ST3R_OK;
}

int st3r_exposure_bwd_impl(st3r_ctx* ctx, hipStream_t s, int C, int H, int W, const float* rgb, const float* exposure,
                           const float* v_out, float* v_rgb, float* v_exposure) {
    const int64_t HW = (int64_t)H * W;
    int blocks; int64_t chunk;
    st3r_stream_grid(C, HW, &blocks, &chunk);
    ARENA_GET(SLOT_EXPOSURE_PART, double, (size_t)C * blocks * 12, part);
    if (HW % 4 == 0 && ex_al16(rgb) && ex_al16(v_out) && ex_al16(v_rgb))
        hipLaunchKernelGGL(k_exposure_bwd<true>, dim3(blocks, C), dim3(EX_T), 0, s, HW, chunk, rgb, exposure, v_out, v_rgb,
                           part);
    else
        hipLaunchKernelGGL(k_exposure_bwd<false>, dim3(blocks, C), dim3(EX_T), 0, s, HW, chunk, rgb, exposure, v_out, v_rgb,
                           part);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_exposure_finish, dim3(C), dim3(EX_T), 0, s, blocks, (const double*)part, v_exposure);
    LAUNCH_CHECK();
    return ST3R_OK;
}

// The registered exposures that belong to the C views at `gt` (fused_step.hip): out->exposure = NULL if none applies (no
// registration, another image size, or not a whole-view offset into the registered images).
void st3r_exposure_for(st3r_ctx* ctx, const float* gt, int C, int H, int W, ExposureReg* out) {
    *out = ExposureReg{};
    if (!ctx->ex_exposure || H != ctx->ex_h || W != ctx->ex_w) return;
    const int64_t img = (int64_t)H * W * 3;
    if (gt < ctx->ex_gt || (gt - ctx->ex_gt) % img != 0) return;
    const int64_t c0 = (gt - ctx->ex_gt) / img;
    if (c0 + C > ctx->ex_c) return;
    *out = ExposureReg{ctx->ex_exposure + 12 * c0, ctx->ex_v_exposure + 12 * c0};
}

ST3R_EXPORT int st3r_ctx_set_exposure(st3r_ctx* ctx, const float* gt, const float* exposure, float* v_exposure, int C,
                                      int height, int width) {
    ARG_CHECK(ctx);
    if (!gt || !exposure || !v_exposure) {
        ctx->ex_gt = nullptr; ctx->ex_exposure = nullptr; ctx->ex_v_exposure = nullptr;
        ctx->ex_c = ctx->ex_h = ctx->ex_w = 0;
        return ST3R_OK;
    }
    ARG_CHECK(C > 0 && height > 0 && width > 0);
    ctx->ex_gt = gt; ctx->ex_exposure = exposure; ctx->ex_v_exposure = v_exposure;
    ctx->ex_c = C; ctx->ex_h = height; ctx->ex_w = width;
    return ST3R_OK;
}

ST3R_EXPORT int st3r_exposure_fwd(st3r_ctx* ctx, void* stream, int C, int height, int width, const float* rgb,
                                  const float* exposure, float* out) {
    ARG_CHECK(ctx && C > 0 && C <= 65535 && height > 0 && width > 0 && rgb && exposure && out);
    return st3r_exposure_fwd_impl((hipStream_t)stream, C, height, width, rgb, exposure, out);
}

ST3R_EXPORT int st3r_exposure_bwd(st3r_ctx* ctx, void* stream, int C, int height, int width, const float* rgb,
                                  const float* exposure, const float* v_out, float* v_rgb, float* v_exposure) {
    ARG_CHECK(ctx && C > 0 && C <= 65535 && height > 0 && width > 0 && rgb && exposure && v_out && v_rgb && v_exposure);
    return st3r_exposure_bwd_impl(ctx, (hipStream_t)stream, C, height, width, rgb, exposure, v_out, v_rgb, v_exposure);
}

struct ExposureAdamK {
    double lr, b1, b2, eps, bc1, bc2;
};

__global__ __launch_bounds__(64) void k_exposure_adam(int C, float* __restrict__ exposure,
                                                      const float* __restrict__ v_exposure, float* __restrict__ m,
                                                      float* __restrict__ v, ExposureAdamK k,
                                                      const float* __restrict__ mask, const int32_t* __restrict__ count_dev,
                                                      uint32_t count_cap) {
    if (count_dev && (uint32_t)count_dev[0] > count_cap) return;   // (see k_adam)
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    if (mask && mask[c] == 0.0f) return;   // a frozen view keeps E, m and v bit for bit
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        const int i = 12 * c + q;
        const double g = (double)v_exposure[i];
        const double mi = k.b1 * (double)m[i] + (1.0 - k.b1) * g;
        const double vi = k.b2 * (double)v[i] + ((1.0 - k.b2) * g) * g;
        m[i] = (float)mi; v[i] = (float)vi;
        exposure[i] = (float)((double)exposure[i] - k.lr * (mi / k.bc1) / (sqrt(vi / k.bc2) + k.eps));
    }
}

ST3R_EXPORT int st3r_exposure_adam_step(st3r_ctx* ctx, void* stream, int C, float* exposure, const float* v_exposure,
                                        float* m, float* v, double lr, double beta1, double beta2, double eps, int step,
                                        const float* mask) {
    ARG_CHECK(ctx && C > 0 && step >= 1 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0);
    ARG_CHECK(exposure && v_exposure && m && v);
    ExposureAdamK k;
    k.lr = lr; k.b1 = beta1; k.b2 = beta2; k.eps = eps;
    k.bc1 = 1.0 - pow(beta1, (double)step); k.bc2 = 1.0 - pow(beta2, (double)step);
    // an asynchronous step is in flight and its count not yet settled: guard the update with it (see k_adam)
    const int32_t* count_dev; uint32_t count_cap;
    st3r_adam_guard(ctx, &count_dev, &count_cap);
    hipLaunchKernelGGL(k_exposure_adam, dim3(ceil_div(C, 64)), dim3(64), 0, (hipStream_t)stream, C, exposure, v_exposure, m,
                       v, k, mask, count_dev, count_cap);
    LAUNCH_CHECK();
    return ST3R_OK;
}
