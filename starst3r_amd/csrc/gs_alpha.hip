// Backgrounds and alpha supervision of C views: a background colour under the render (`backgrounds` of
// gsplat.rasterization) and a weighted L1 between the accumulated opacity of the render and a per-view target map.
//     composite   y_j     = fmaf(1 - a, b_j, x_j)                       float32; b = backgrounds[c], a = alpha(p)
//     background  t_bg    = -fmaf(b_2, v_2, fmaf(b_1, v_1, b_0 * v_0))  v = d loss / d y (which is d loss / d x as well)
//                 v_b[c][j] = sum_p (1 - a) v_j                         the float32 factor 1 - a, products and sums in double
//     alpha term  n_c     = max(sum_p w, 1)
//                 loss_c  = alpha_fac * sum_p w |a - M| / n_c
//                 t_a     = k w sign(a - M),  k = (float)((double)alpha_fac / n_c),  sign(0) = 0
//     output      v_alpha = ((v_alpha_in or 0) + t_bg) + t_a            in that order; an absent term is +0
// A pixel with w <= 0 (or a NaN weight) contributes nothing to the sum and gets t_a = 0 whatever M holds there: dp_pixel's
// rule (loss_depth.hip).
//
// Two streaming kernels (per_view.h: chunks, grid, launch pair, sums).  The composite reads 16 bytes and writes 12 per
// pixel.  k_alpha_grad takes its switches as template parameters -- background term, alpha term, accumulate, vector form
// -- so that a call loads only what it uses: 4 (alpha) + 12 (v) + 8 (M, w) + 4 (v_alpha_in) bytes in at most, 4 out.  Its
// sums: three doubles (v_b) and one (sum_p w |a - M|) per (view, workgroup), in two arrays of one arena slot, finished by
// k_stream_finish.  No atomics, a fixed order for a given shape: the same inputs give the same bits.
// The switches decide the loads, not all of the arithmetic: with the background term on, a pixel forms its three double
// products for v_b also when the caller wants no v_b (part_b NULL: the fused step, whose colours are fixed) and only the
// reduction is skipped.  A fifth switch would double the instantiations for three multiply-adds per pixel of a kernel that
// waits for memory (4.5 TB/s, profiles/alpha_step.md).
// n_c depends on the weights alone: the fused step computes it once per registration (st3r_ctx_set_alpha_target).
#include "per_view.h"

// out may be rgb itself: a thread reads its pixels before it writes them, and nobody else touches them (no __restrict__
// on the two)
template <bool VEC>
__global__ __launch_bounds__(STREAM_T) void k_composite_fwd(int64_t HW, int64_t chunk, const float* rgb,
                                                            const float* __restrict__ alpha,
                                                            const float* __restrict__ backgrounds, float* out) {
    const int c = blockIdx.y;
    const float b[3] = {backgrounds[3 * c], backgrounds[3 * c + 1], backgrounds[3 * c + 2]};
    const float* x = rgb + (int64_t)c * HW * 3;
    const float* a = alpha + (int64_t)c * HW;
    float* y = out + (int64_t)c * HW * 3;
    int64_t lo, hi;
    stream_chunk(chunk, HW, lo, hi);
    if (VEC) {
        for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi; i += 4 * STREAM_T) {   // pixels i .. i + 3: 12 + 4 floats
            alignas(16) float v[12], w[12], av[4];
            const float4* src = reinterpret_cast<const float4*>(x + 3 * i);
            *reinterpret_cast<float4*>(v) = src[0]; *reinterpret_cast<float4*>(v + 4) = src[1];
            *reinterpret_cast<float4*>(v + 8) = src[2];
            *reinterpret_cast<float4*>(av) = *reinterpret_cast<const float4*>(a + i);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float om = 1.0f - av[p];
#pragma unroll
                for (int j = 0; j < 3; ++j) w[3 * p + j] = fmaf(om, b[j], v[3 * p + j]);
            }
            float4* dst = reinterpret_cast<float4*>(y + 3 * i);
            dst[0] = *reinterpret_cast<float4*>(w); dst[1] = *reinterpret_cast<float4*>(w + 4);
            dst[2] = *reinterpret_cast<float4*>(w + 8);
        }
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += STREAM_T) {
            const float om = 1.0f - a[i];
            const float x0 = x[3 * i], x1 = x[3 * i + 1], x2 = x[3 * i + 2];
            y[3 * i] = fmaf(om, b[0], x0); y[3 * i + 1] = fmaf(om, b[1], x1); y[3 * i + 2] = fmaf(om, b[2], x2);
        }
    }
}

// what k_alpha_grad reads and writes; the pointers a switch leaves out are not looked at
struct AlphaGradK {
    const float *alpha, *backgrounds, *v_out, *target, *weight;
    const double* norm; int norm_stride;
    float alpha_fac;
    const float* v_alpha_in;   // may be v_alpha itself
    float* v_alpha;
    double *part_b, *part_a;   // [C, workgroups, 3] and [C, workgroups]
};

// one pixel: d loss / d alpha out; its terms of the sums added to acc (acc[0..2]: v_b, acc[3]: sum w |a - M|)
template <bool BG, bool AT>
__device__ __forceinline__ float ag_pixel(float a, const float* b, const float* v, float m, float w, float k, float vin,
                                          double* acc) {
    float t_bg = 0.f, t_a = 0.f;
    if (BG) {
        t_bg = -fmaf(b[2], v[2], fmaf(b[1], v[1], b[0] * v[0]));
        const double om = (double)(1.0f - a);
        acc[0] += om * (double)v[0]; acc[1] += om * (double)v[1]; acc[2] += om * (double)v[2];
    }
    if (AT) {
        if (w > 0.f) {
            const double diff = (double)a - (double)m;
            t_a = k * w * (diff > 0.0 ? 1.0f : (diff < 0.0 ? -1.0f : 0.0f));
            acc[3] += (double)w * fabs(diff);
        }
    }
    return (vin + t_bg) + t_a;
}

// v_alpha_in and v_alpha may be the same buffer (see k_composite_fwd)
template <bool BG, bool AT, bool ACC, bool VEC>
__global__ __launch_bounds__(STREAM_T) void k_alpha_grad(int64_t HW, int64_t chunk, AlphaGradK g) {
    __shared__ double red[16];
    const int c = blockIdx.y;
    const int64_t base = (int64_t)c * HW;
    int64_t lo, hi;
    stream_chunk(chunk, HW, lo, hi);
    float b[3] = {0.f, 0.f, 0.f};
    if (BG) { b[0] = g.backgrounds[3 * c]; b[1] = g.backgrounds[3 * c + 1]; b[2] = g.backgrounds[3 * c + 2]; }
    const float k = AT ? (float)((double)g.alpha_fac / g.norm[(int64_t)c * g.norm_stride]) : 0.f;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (VEC) {
        for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi; i += 4 * STREAM_T) {
            alignas(16) float av[4], vv[12] = {}, mv[4] = {}, wv[4] = {}, iv[4] = {}, ov[4];
            *reinterpret_cast<float4*>(av) = *reinterpret_cast<const float4*>(g.alpha + base + i);
            if (BG) {
                const float4* sv = reinterpret_cast<const float4*>(g.v_out + 3 * (base + i));
                *reinterpret_cast<float4*>(vv) = sv[0]; *reinterpret_cast<float4*>(vv + 4) = sv[1];
                *reinterpret_cast<float4*>(vv + 8) = sv[2];
            }
            if (AT) {
                *reinterpret_cast<float4*>(mv) = *reinterpret_cast<const float4*>(g.target + base + i);
                *reinterpret_cast<float4*>(wv) = *reinterpret_cast<const float4*>(g.weight + base + i);
            }
            if (ACC) *reinterpret_cast<float4*>(iv) = *reinterpret_cast<const float4*>(g.v_alpha_in + base + i);
#pragma unroll
            for (int p = 0; p < 4; ++p) ov[p] = ag_pixel<BG, AT>(av[p], b, vv + 3 * p, mv[p], wv[p], k, iv[p], acc);
            *reinterpret_cast<float4*>(g.v_alpha + base + i) = *reinterpret_cast<float4*>(ov);
        }
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += STREAM_T) {
            float vs[3] = {0.f, 0.f, 0.f};
            if (BG) { vs[0] = g.v_out[3 * (base + i)]; vs[1] = g.v_out[3 * (base + i) + 1]; vs[2] = g.v_out[3 * (base + i) + 2]; }
            const float m = AT ? g.target[base + i] : 0.f, w = AT ? g.weight[base + i] : 0.f;
            const float vin = ACC ? g.v_alpha_in[base + i] : 0.f;
            g.v_alpha[base + i] = ag_pixel<BG, AT>(g.alpha[base + i], b, vs, m, w, k, vin, acc);
        }
    }
    if (g.part_b || AT) {   // (uniform over the workgroup)
        const double t = block_sum_fixed(acc, red);
        const int64_t wg = (int64_t)c * gridDim.x + blockIdx.x;
        if (BG && g.part_b && threadIdx.x < 3) g.part_b[wg * 3 + threadIdx.x] = t;
        if (AT && threadIdx.x == 3) g.part_a[wg] = t;
    }
}

int st3r_composite_fwd_impl(hipStream_t s, int C, int H, int W, const float* rgb, const float* alpha,
                            const float* backgrounds, float* out) {
    const int64_t HW = (int64_t)H * W;
    int blocks; int64_t chunk;
    stream_grid(C, HW, &blocks, &chunk);
    STREAM_LAUNCH(k_composite_fwd, HW % 4 == 0 && aligned16(rgb, alpha, out), blocks, C, s, HW, chunk, rgb, alpha,
                  backgrounds, out);
    return ST3R_OK;
}

// k_alpha_grad<BG, AT, ACC, .> in its 16-byte or 4-byte form, on the grid of stream_grid (STREAM_LAUNCH takes a kernel of
// one switch)
template <bool BG, bool AT, bool ACC>
static int alpha_grad_launch(hipStream_t s, bool vec, int blocks, int C, int64_t HW, int64_t chunk, const AlphaGradK& g) {
    const auto kernel = vec ? k_alpha_grad<BG, AT, ACC, true> : k_alpha_grad<BG, AT, ACC, false>;
    hipLaunchKernelGGL(kernel, dim3(blocks, C), dim3(STREAM_T), 0, s, HW, chunk, g);
    LAUNCH_CHECK();
    return ST3R_OK;
}

// The pass itself.  backgrounds != NULL (with v_out): the background term; target != NULL (with weight, norm, sums): the
// alpha term, norm holding n_c already and sums[c * sums_stride] receiving sum_p w |a - M| of view c; v_alpha_in != NULL:
// accumulate onto it; v_backgrounds != NULL: [C,3], written whole.
int st3r_alpha_grad_impl(st3r_ctx* ctx, hipStream_t s, int C, int H, int W, const float* alpha, const float* backgrounds,
                         const float* v_out, const float* target, const float* weight, const double* norm, int norm_stride,
                         float alpha_fac, const float* v_alpha_in, double* sums, int sums_stride, float* v_alpha,
                         float* v_backgrounds) {
    const int64_t HW = (int64_t)H * W;
    const bool bg = backgrounds != nullptr, at = target != nullptr, acc = v_alpha_in != nullptr;
    int blocks; int64_t chunk;
    stream_grid(C, HW, &blocks, &chunk);
    ARENA_GET(SLOT_AGRAD_PART, double, (size_t)C * blocks * 4, part);
    AlphaGradK g{alpha, backgrounds, v_out, target, weight, norm, norm_stride, alpha_fac, v_alpha_in, v_alpha,
                 bg && v_backgrounds ? part : nullptr, part + (size_t)C * blocks * 3};
    const bool vec = HW % 4 == 0 && aligned16(alpha, v_out, target, weight, v_alpha_in, v_alpha);
    int rc;
    if (bg && at) rc = acc ? alpha_grad_launch<true, true, true>(s, vec, blocks, C, HW, chunk, g)
                           : alpha_grad_launch<true, true, false>(s, vec, blocks, C, HW, chunk, g);
    else if (bg) rc = acc ? alpha_grad_launch<true, false, true>(s, vec, blocks, C, HW, chunk, g)
                          : alpha_grad_launch<true, false, false>(s, vec, blocks, C, HW, chunk, g);
    else rc = acc ? alpha_grad_launch<false, true, true>(s, vec, blocks, C, HW, chunk, g)
                  : alpha_grad_launch<false, true, false>(s, vec, blocks, C, HW, chunk, g);
    if (!rc && g.part_b) rc = stream_finish<3>(s, C, blocks, g.part_b, v_backgrounds, 3, 0);
    if (!rc && at) rc = stream_finish<1>(s, C, blocks, g.part_a, sums, sums_stride, 0);
    return rc;
}

// The registered backgrounds that belong to the C views at `gt` (fused_step.hip): out->colors = NULL if none applies
// (view_reg_first).
void st3r_background_for(st3r_ctx* ctx, const float* gt, int C, int H, int W, Background* out) {
    const int64_t c0 = view_reg_first(ctx->bg, gt, C, H, W);
    *out = c0 < 0 ? Background{} : Background{ctx->bg_colors + 3 * c0};
}

ST3R_EXPORT int st3r_ctx_set_background(st3r_ctx* ctx, const float* gt, const float* backgrounds, int C, int height,
                                        int width) {
    ARG_CHECK(ctx);
    const bool on = gt && backgrounds;
    int rc = view_reg_set(&ctx->bg, on, gt, C, height, width);
    if (rc) return rc;
    ctx->bg_colors = on ? backgrounds : nullptr;
    return ST3R_OK;
}

ST3R_EXPORT int st3r_ctx_set_alpha_target(st3r_ctx* ctx, const float* gt, const float* target, const float* weight, int C,
                                          int height, int width, float alpha_fac) {
    ARG_CHECK(ctx);
    return target_reg_set(&ctx->at, gt, target, weight, C, height, width, alpha_fac, alpha_fac - alpha_fac == 0.f);   // finite
}

ST3R_EXPORT int st3r_composite_fwd(st3r_ctx* ctx, void* stream, int C, int height, int width, const float* rgb,
                                   const float* alpha, const float* backgrounds, float* out) {
    ARG_CHECK(ctx && C > 0 && C <= 65535 && height > 0 && width > 0 && rgb && alpha && backgrounds && out);
    return st3r_composite_fwd_impl((hipStream_t)stream, C, height, width, rgb, alpha, backgrounds, out);
}

ST3R_EXPORT int st3r_alpha_grad(st3r_ctx* ctx, void* stream, int C, int height, int width, const float* alpha,
                                const float* backgrounds, const float* v_out, const float* target, const float* weight,
                                float alpha_fac, const float* v_alpha_in, double* sums, float* v_alpha,
                                float* v_backgrounds) {
    ARG_CHECK(ctx && C > 0 && C <= 65535 && height > 0 && width > 0 && alpha && v_alpha);
    const bool bg = backgrounds && v_out, at = target && weight && sums;
    ARG_CHECK(bg || at);                                       // at least one of the two terms
    ARG_CHECK(bg || (!backgrounds && !v_out && !v_backgrounds));   // a term is given whole or not at all
    ARG_CHECK(at || (!target && !weight && !sums));
    ARG_CHECK(!at || alpha_fac - alpha_fac == 0.f);
    hipStream_t s = (hipStream_t)stream;
    if (at) {
        int rc = st3r_weight_norms(ctx, s, C, height, width, weight, sums + 1, 2, 1, false, SLOT_ATARGET_PART);   // n_c
        if (rc) return rc;
    }
    return st3r_alpha_grad_impl(ctx, s, C, height, width, alpha, bg ? backgrounds : nullptr, v_out, at ? target : nullptr,
                                weight, sums ? sums + 1 : nullptr, 2, alpha_fac, v_alpha_in, sums, 2, v_alpha, v_backgrounds);
}
