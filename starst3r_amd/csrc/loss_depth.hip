// Depth-prior loss of C views: a weighted L1 between the expected depth of the render and a per-pixel prior (the depth
// maps of the alignment, or a sensor's), forward and backward in one pass.
//     ED(p)  = D(p) / max(alpha(p), 1e-10)            gsplat's "ED", as render_3dgs forms it
//     n_c    = max(sum_p w_c(p), 1)
//     loss_c = depth_fac * sum_p w_c(p) |ED(p) - Z_c(p)| / n_c
//     v_D(p) = g / max(alpha, 1e-10),  v_alpha(p) = -g ED / alpha where alpha >= 1e-10, else 0 (torch's clamp gradient),
//     g      = depth_fac w_c(p) sign(ED - Z) / n_c
// A pixel with w == 0 (or a NaN weight) contributes nothing and gets zero gradients whatever D, alpha and Z hold there.
//
// A streaming kernel with one reduction (per_view.h: chunks, grid, launch pair, sums): four inputs and two outputs of 4
// bytes per pixel, one double partial per (view, workgroup).
// n_c depends on the weights alone: the fused step computes it once per registration (st3r_ctx_set_depth_prior).
#include "per_view.h"

#define DP_MIN_ALPHA 1e-10f

// one pixel: gradients out, its term of the sum returned
__device__ __forceinline__ double dp_pixel(float d, float a, float z, float w, float k, float& v_d, float& v_a) {
    v_d = 0.f; v_a = 0.f;
    if (!(w > 0.f)) return 0.0;
    const float ac = fmaxf(a, DP_MIN_ALPHA);
    const float ed = d / ac;
    const double diff = (double)ed - (double)z;
    const float g = k * w * (diff > 0.0 ? 1.0f : (diff < 0.0 ? -1.0f : 0.0f));
    v_d = g / ac;
    v_a = a >= DP_MIN_ALPHA ? -(g * ed) / ac : 0.f;
    return (double)w * fabs(diff);
}

template <bool VEC>
__global__ __launch_bounds__(STREAM_T) void k_dprior_loss(int64_t HW, int64_t chunk, const float* __restrict__ depth,
                                                          const float* __restrict__ alpha, const float* __restrict__ prior,
                                                          const float* __restrict__ weight, const double* __restrict__ norm,
                                                          int norm_stride, float depth_fac, float* __restrict__ v_depth,
                                                          float* __restrict__ v_alpha, double* __restrict__ part) {
    __shared__ double red[4];
    const int c = blockIdx.y;
    const int64_t base = (int64_t)c * HW;
    int64_t lo, hi;
    stream_chunk(chunk, HW, lo, hi);
    const float k = (float)((double)depth_fac / norm[(int64_t)c * norm_stride]);
    double acc[1] = {0.0};
    if (VEC) {
        for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi; i += 4 * STREAM_T) {
            const float4 d = *reinterpret_cast<const float4*>(depth + base + i);
            const float4 a = *reinterpret_cast<const float4*>(alpha + base + i);
            const float4 z = *reinterpret_cast<const float4*>(prior + base + i);
            const float4 w = *reinterpret_cast<const float4*>(weight + base + i);
            float4 vd, va;
            acc[0] += dp_pixel(d.x, a.x, z.x, w.x, k, vd.x, va.x);
            acc[0] += dp_pixel(d.y, a.y, z.y, w.y, k, vd.y, va.y);
            acc[0] += dp_pixel(d.z, a.z, z.z, w.z, k, vd.z, va.z);
            acc[0] += dp_pixel(d.w, a.w, z.w, w.w, k, vd.w, va.w);
            *reinterpret_cast<float4*>(v_depth + base + i) = vd;
            *reinterpret_cast<float4*>(v_alpha + base + i) = va;
        }
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += STREAM_T) {
            float vd, va;
            acc[0] += dp_pixel(depth[base + i], alpha[base + i], prior[base + i], weight[base + i], k, vd, va);
            v_depth[base + i] = vd; v_alpha[base + i] = va;
        }
    }
    const double t = block_sum_fixed(acc, red);
    if (threadIdx.x == 0) part[(int64_t)c * gridDim.x + blockIdx.x] = t;
}

// out[c * stride] = sum_p w of the C views at `weight` and, interior, out[c * stride + 1] = sum_{p in I} w
// (k_weight_sums); at_least_one: max(., 1) of each.  slot: the arena slot of the partials.
int st3r_weight_norms(st3r_ctx* ctx, hipStream_t s, int C, int H, int W, const float* weight, double* out, int stride,
                      int at_least_one, bool interior, int slot) {
    const int64_t HW = (int64_t)H * W;
    int blocks; int64_t chunk;
    stream_grid(C, HW, &blocks, &chunk);
    ARENA_GET(slot, double, (size_t)C * blocks * (interior ? 2 : 1), part);
    LAUNCH_BOOL2(k_weight_sums, HW % 4 == 0 && aligned16(weight), interior, dim3(blocks, C), dim3(STREAM_T), s, HW, chunk,
                 H, W, weight, part);
    return interior ? stream_finish<2>(s, C, blocks, part, out, stride, at_least_one)
                    : stream_finish<1>(s, C, blocks, part, out, stride, at_least_one);
}

// The norms of a registration (those of all its reg.c views, 1 or 2 doubles each, in the arena slot norm_slot), computed
// by the first call that gets here, on its stream: *valid says that the slot holds this registration's.
int st3r_registered_weight_norms(st3r_ctx* ctx, hipStream_t s, const ViewReg& reg, const float* weight, int at_least_one,
                                 bool interior, int part_slot, int norm_slot, int* valid, const double** norms) {
    const int stride = interior ? 2 : 1;
    void* p = nullptr; int grown = 0;
    int rc = st3r_arena_get2(ctx, norm_slot, sizeof(double) * stride * (size_t)reg.c, &p, &grown);
    if (rc) return rc;
    if (grown || !*valid) {
        rc = st3r_weight_norms(ctx, s, reg.c, reg.h, reg.w, weight, (double*)p, stride, at_least_one, interior, part_slot);
        if (rc) return rc;
        *valid = 1;
    }
    *norms = (const double*)p;
    return ST3R_OK;
}

// the pass itself: sums[c * sums_stride] = sum_p w |ED - Z| of view c; norm holds n_c already
int st3r_depth_prior_loss_impl(st3r_ctx* ctx, hipStream_t s, int C, int H, int W, const float* depth, const float* alpha,
                               const float* prior, const float* weight, const double* norm, int norm_stride,
                               float depth_fac, double* sums, int sums_stride, float* v_depth, float* v_alpha) {
    const int64_t HW = (int64_t)H * W;
    int blocks; int64_t chunk;
    stream_grid(C, HW, &blocks, &chunk);
    ARENA_GET(SLOT_DPRIOR_PART, double, (size_t)C * blocks, part);
    STREAM_LAUNCH(k_dprior_loss, HW % 4 == 0 && aligned16(depth, alpha, prior, weight, v_depth, v_alpha), blocks, C, s, HW,
                  chunk, depth, alpha, prior, weight, norm, norm_stride, depth_fac, v_depth, v_alpha, part);
    return stream_finish<1>(s, C, blocks, part, sums, sums_stride, 0);
}

ST3R_EXPORT int st3r_ctx_set_depth_prior(st3r_ctx* ctx, const float* gt, const float* depth, const float* weight, int C,
                                         int height, int width, float depth_fac) {
    ARG_CHECK(ctx);
    return target_reg_set(&ctx->dp, gt, depth, weight, C, height, width, depth_fac, depth_fac == depth_fac);   // no NaN
}

ST3R_EXPORT int st3r_loss_depth_prior(st3r_ctx* ctx, void* stream, int C, int height, int width, const float* depth,
                                      const float* alpha, const float* prior, const float* weight, float depth_fac,
                                      double* sums, float* v_depth, float* v_alpha) {
    ARG_CHECK(ctx && C > 0 && height > 0 && width > 0);
    ARG_CHECK(depth && alpha && prior && weight && sums && v_depth && v_alpha);
    hipStream_t s = (hipStream_t)stream;
    int rc = st3r_weight_norms(ctx, s, C, height, width, weight, sums + 1, 2, 1, false, SLOT_DPRIOR_PART);   // n_c
    if (rc) return rc;
    return st3r_depth_prior_loss_impl(ctx, s, C, height, width, depth, alpha, prior, weight, sums + 1, 2, depth_fac, sums, 2,
                                      v_depth, v_alpha);
}
