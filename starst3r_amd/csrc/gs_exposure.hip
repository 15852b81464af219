// Per-view exposure: an affine colour transform between the render and the loss (the `exposure` of the original 3DGS
// code, `app_opt` of gsplat's trainer), forward, backward and its Adam step.
//     E_c = [A_c | t_c]  [3,4] float32, row major         y_j = fmaf(A[j][2], b, fmaf(A[j][1], g, fmaf(A[j][0], r, t[j])))
//     v_x_i    = A[0][i] v_y_0 + A[1][i] v_y_1 + A[2][i] v_y_2      (float32, that order; v_x may be written over v_y)
//     v_A[j][i] = sum_p v_y_j(p) x_i(p)      v_t[j] = sum_p v_y_j(p)
//
// Two streaming kernels (per_view.h: chunks, grid, launch pair, sums): 12 bytes in and 12 out per pixel forward, 24 in
// and 12 out backward; four pixels are three 16-byte accesses per thread.  The twelve sums of a view: every product is
// (double)v_y * (double)x, one 12-double partial per (view, workgroup), the view's total stored as float32.
//
// Exposure Adam (k_exposure_adam) is the per-view Adam of per_view.h on the twelve scalars of a view.
#include "per_view.h"

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
__global__ __launch_bounds__(STREAM_T) void k_exposure_fwd(int64_t HW, int64_t chunk, const float* __restrict__ rgb,
                                                       const float* __restrict__ exposure, float* __restrict__ out) {
    const int c = blockIdx.y;
    const ExposureK k = ex_load(exposure, c);
    const float* x = rgb + (int64_t)c * HW * 3;
    float* y = out + (int64_t)c * HW * 3;
    int64_t lo, hi;
    stream_chunk(chunk, HW, lo, hi);
    if (VEC) {
        for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi; i += 4 * STREAM_T) {   // pixels i .. i + 3: 12 floats
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
        for (int64_t i = lo + threadIdx.x; i < hi; i += STREAM_T) {
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

// v_out and v_rgb may be the same buffer: a thread reads its pixels' v_y before it writes their v_x, and nobody else
// touches them (no __restrict__ on the two)
template <bool VEC>
__global__ __launch_bounds__(STREAM_T) void k_exposure_bwd(int64_t HW, int64_t chunk, const float* __restrict__ rgb,
                                                       const float* __restrict__ exposure, const float* v_out, float* v_rgb,
                                                       double* __restrict__ part) {
    __shared__ double red[48];
    const int c = blockIdx.y;
    const ExposureK k = ex_load(exposure, c);
    const int64_t base = (int64_t)c * HW * 3;
    const float* x = rgb + base;
    const float* vy = v_out + base;
    float* vx = v_rgb + base;
    int64_t lo, hi;
    stream_chunk(chunk, HW, lo, hi);
    double acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.0;
    if (VEC) {
        for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi; i += 4 * STREAM_T) {
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
        for (int64_t i = lo + threadIdx.x; i < hi; i += STREAM_T) {
            const float xs[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
            const float gs[3] = {vy[3 * i], vy[3 * i + 1], vy[3 * i + 2]};
            float os[3];
            ex_bwd_pixel(k, xs, gs, os, acc);
            vx[3 * i] = os[0]; vx[3 * i + 1] = os[1]; vx[3 * i + 2] = os[2];
        }
    }
    const double t = block_sum_fixed(acc, red);
    if (threadIdx.x < 12) part[((int64_t)c * gridDim.x + blockIdx.x) * 12 + threadIdx.x] = t;
}

int st3r_exposure_fwd_impl(hipStream_t s, int C, int H, int W, const float* rgb, const float* exposure, float* out) {
    const int64_t HW = (int64_t)H * W;
    int blocks; int64_t chunk;
    stream_grid(C, HW, &blocks, &chunk);
    STREAM_LAUNCH(k_exposure_fwd, HW % 4 == 0 && aligned16(rgb, out), blocks, C, s, HW, chunk, rgb, exposure, out);
    return ST3R_OK;
}

int st3r_exposure_bwd_impl(st3r_ctx* ctx, hipStream_t s, int C, int H, int W, const float* rgb, const float* exposure,
                           const float* v_out, float* v_rgb, float* v_exposure) {
    const int64_t HW = (int64_t)H * W;
    int blocks; int64_t chunk;
    stream_grid(C, HW, &blocks, &chunk);
    ARENA_GET(SLOT_EXPOSURE_PART, double, (size_t)C * blocks * 12, part);
    STREAM_LAUNCH(k_exposure_bwd, HW % 4 == 0 && aligned16(rgb, v_out, v_rgb), blocks, C, s, HW, chunk, rgb, exposure,
                  v_out, v_rgb, part);
    return stream_finish<12>(s, C, blocks, part, v_exposure, 12, 0);
}

// The registered exposures that belong to the C views at `gt` (fused_step.hip): out->exposure = NULL if none applies
// (view_reg_first).
void st3r_exposure_for(st3r_ctx* ctx, const float* gt, int C, int H, int W, ExposureReg* out) {
    const int64_t c0 = view_reg_first(ctx->ex, gt, C, H, W);
    *out = c0 < 0 ? ExposureReg{} : ExposureReg{ctx->ex_exposure + 12 * c0, ctx->ex_v_exposure + 12 * c0};
}

ST3R_EXPORT int st3r_ctx_set_exposure(st3r_ctx* ctx, const float* gt, const float* exposure, float* v_exposure, int C,
                                      int height, int width) {
    ARG_CHECK(ctx);
    const bool on = gt && exposure && v_exposure;
    int rc = view_reg_set(&ctx->ex, on, gt, C, height, width);
    if (rc) return rc;
    ctx->ex_exposure = on ? exposure : nullptr; ctx->ex_v_exposure = on ? v_exposure : nullptr;
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

__global__ __launch_bounds__(64) void k_exposure_adam(int C, PerViewAdamK k, float* __restrict__ exposure,
                                                      const float* __restrict__ v_exposure, float* __restrict__ m,
                                                      float* __restrict__ v) {
    const int c = per_view_adam_view(k, C);
    if (c < 0) return;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        const int i = 12 * c + q;
        exposure[i] = (float)((double)exposure[i] + per_view_adam_delta<false>(k, m[i], (double)v_exposure[i], v[i]));
    }
}

ST3R_EXPORT int st3r_exposure_adam_step(st3r_ctx* ctx, void* stream, int C, float* exposure, const float* v_exposure,
                                        float* m, float* v, double lr, double beta1, double beta2, double eps, int step,
                                        const float* mask) {
    ARG_CHECK(ctx && C > 0 && step >= 1 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0);
    ARG_CHECK(exposure && v_exposure && m && v);
    return per_view_adam_launch(ctx, (hipStream_t)stream, k_exposure_adam, C, lr, beta1, beta2, eps, step, mask, exposure,
                                v_exposure, m, v);
}
