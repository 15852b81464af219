// Depth-prior loss of C views: a weighted L1 between the expected depth of the render and a per-pixel prior (the depth
// maps of the alignment, or a sensor's), forward and backward in one pass.
//     ED(p)  = D(p) / max(alpha(p), 1e-10)            gsplat's "ED", as render_3dgs forms it
//     n_c    = max(sum_p w_c(p), 1)
//     loss_c = depth_fac * sum_p w_c(p) |ED(p) - Z_c(p)| / n_c
//     v_D(p) = g / max(alpha, 1e-10),  v_alpha(p) = -g ED / alpha where alpha >= 1e-10, else 0 (torch's clamp gradient),
//     g      = depth_fac w_c(p) sign(ED - Z) / n_c
// A pixel with w == 0 (or a NaN weight) contributes nothing and gets zero gradients whatever D, alpha and Z hold there.
//
// A streaming kernel with one reduction: four inputs and two outputs of 4 bytes per pixel, nothing re-read.  A view's
// pixels are dealt to workgroups in contiguous chunks (a multiple of 1024 pixels: 16-byte accesses stay aligned whenever
// H * W is a multiple of 4 and the buffers are), the grid is at most 2048 workgroups -- eight per CU on the 256 CUs, so the
// whole launch is resident at once and there is no partly filled second round -- and a thread strides through its chunk.
// Sums: every thread adds its pixels in double, the wave meets in a butterfly, the four waves in order, one double partial
// per workgroup; a second launch (one workgroup per view) adds a view's partials the same way.  No atomics, a fixed order for a given shape: the same inputs give the same bits.
// n_c depends on the weights alone: the fused step computes it once per registration (st3r_ctx_set_depth_prior).
#include "stages.h"

#define DP_T 256          // threads per workgroup
#define DP_ALIGN 1024     // chunk granularity in pixels: one 16-byte access per thread
#define DP_MIN_ALPHA 1e-10f

__device__ __forceinline__ double dp_block_sum(double v, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// sum of the weights that count (w > 0) of one chunk
template <bool VEC>
__global__ __launch_bounds__(DP_T) void k_dprior_wsum(int64_t HW, int64_t chunk, const float* __restrict__ weight,
                                                      double* __restrict__ part) {
    __shared__ double red[4];
    const int c = blockIdx.y;
    const float* w = weight + (int64_t)c * HW;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = min(HW, lo + chunk);
    double acc = 0.0;
    if (VEC) {
        for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi; i += 4 * DP_T) {
            const float4 v = *reinterpret_cast<const float4*>(w + i);
            acc += (double)(v.x > 0.f ? v.x : 0.f); acc += (double)(v.y > 0.f ? v.y : 0.f);
            acc += (double)(v.z > 0.f ? v.z : 0.f); acc += (double)(v.w > 0.f ? v.w : 0.f);
        }
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += DP_T) {
            const float v = w[i];
            acc += (double)(v > 0.f ? v : 0.f);
        }
    }
    const double t = dp_block_sum(acc, red);
    if (threadIdx.x == 0) part[(int64_t)c * gridDim.x + blockIdx.x] = t;
}

// one workgroup per view: its n_part partials in a fixed order -> out[c * stride]; at_least_one: max(sum, 1) (n_c)
__global__ __launch_bounds__(DP_T) void k_dprior_finish(int n_part, const double* __restrict__ part,
                                                        double* __restrict__ out, int stride, int at_least_one) {
    __shared__ double red[4];
    const int c = blockIdx.x;
    double acc = 0.0;
    for (int b = threadIdx.x; b < n_part; b += DP_T) acc += part[(int64_t)c * n_part + b];
    const double t = dp_block_sum(acc, red);
    if (threadIdx.x == 0) out[(int64_t)c * stride] = at_least_one ? fmax(t, 1.0) : t;
}

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
__global__ __launch_bounds__(DP_T) void k_dprior_loss(int64_t HW, int64_t chunk, const float* __restrict__ depth,
                                                      const float* __restrict__ alpha, const float* __restrict__ prior,
                                                      const float* __restrict__ weight, const double* __restrict__ norm,
                                                      int norm_stride, float depth_fac, float* __restrict__ v_depth,
                                                      float* __restrict__ v_alpha, double* __restrict__ part) {
    __shared__ double red[4];
    const int c = blockIdx.y;
    const int64_t base = (int64_t)c * HW;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = min(HW, lo + chunk);
    const float k = (float)((double)depth_fac / norm[(int64_t)c * norm_stride]);
    double acc = 0.0;
    if (VEC) {
        for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi; i += 4 * DP_T) {
            const float4 d = *reinterpret_cast<const float4*>(depth + base + i);
            const float4 a = *reinterpret_cast<const float4*>(alpha + base + i);
            const float4 z = *reinterpret_cast<const float4*>(prior + base + i);
            const float4 w = *reinterpret_cast<const float4*>(weight + base + i);
            float4 vd, va;
            acc += dp_pixel(d.x, a.x, z.x, w.x, k, vd.x, va.x);
            acc += dp_pixel(d.y, a.y, z.y, w.y, k, vd.y, va.y);
            acc += dp_pixel(d.z, a.z, z.z, w.z, k, vd.z, va.z);
            acc += dp_pixel(d.w, a.w, z.w, w.w, k, vd.w, va.w);
            *reinterpret_cast<float4*>(v_depth + base + i) = vd;
            *reinterpret_cast<float4*>(v_alpha + base + i) = va;
        }
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += DP_T) {
            float vd, va;
            acc += dp_pixel(depth[base + i], alpha[base + i], prior[base + i], weight[base + i], k, vd, va);
            v_depth[base + i] = vd; v_alpha[base + i] = va;
        }
    }
    const double t = dp_block_sum(acc, red);
    if (threadIdx.x == 0) part[(int64_t)c * gridDim.x + blockIdx.x] = t;
}

// workgroups per view and pixels per workgroup: at least four pixels per thread, at most 256 x 8 workgroups in all (one
// resident round of the chip; the count is C times a per-view count, so it is not an exact multiple of 256)
// (stages.h: gs_exposure.hip deals its pixels the same way)
void st3r_stream_grid(int C, int64_t HW, int* blocks, int64_t* chunk) {
    int64_t want = (C * HW + DP_ALIGN - 1) / DP_ALIGN;
    if (want > 256 * 8) want = 256 * 8;
    int64_t b = want / C;
    if (b < 1) b = 1;
    int64_t ch = (HW + b - 1) / b;
    ch = (ch + DP_ALIGN - 1) / DP_ALIGN * DP_ALIGN;
    *chunk = ch;
    *blocks = (int)((HW + ch - 1) / ch);
}

static bool dp_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int dp_partials(st3r_ctx* ctx, int C, int blocks, double** part) {
    ARENA_GET(SLOT_DPRIOR_PART, double, (size_t)C * blocks, p);
    *part = p;
    return ST3R_OK;
}

// norm[c * stride] = n_c of the views at `weight`
static int dp_norms(st3r_ctx* ctx, hipStream_t s, int C, int64_t HW, const float* weight, double* norm, int stride) {
    int blocks; int64_t chunk;
    st3r_stream_grid(C, HW, &blocks, &chunk);
    double* part;
    int rc = dp_partials(ctx, C, blocks, &part);
    if (rc) return rc;
    if (HW % 4 == 0 && dp_al16(weight))
        hipLaunchKernelGGL(k_dprior_wsum<true>, dim3(blocks, C), dim3(DP_T), 0, s, HW, chunk, weight, part);
    else
        hipLaunchKernelGGL(k_dprior_wsum<false>, dim3(blocks, C), dim3(DP_T), 0, s, HW, chunk, weight, part);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_dprior_finish, dim3(C), dim3(DP_T), 0, s, blocks, (const double*)part, norm, stride, 1);
    LAUNCH_CHECK();
    return ST3R_OK;
}

// the pass itself: sums[c * sums_stride] = sum_p w |ED - Z| of view c; norm holds n_c already
int st3r_depth_prior_loss_impl(st3r_ctx* ctx, hipStream_t s, int C, int H, int W, const float* depth, const float* alpha,
                               const float* prior, const float* weight, const double* norm, int norm_stride,
                               float depth_fac, double* sums, int sums_stride, float* v_depth, float* v_alpha) {
    const int64_t HW = (int64_t)H * W;
    int blocks; int64_t chunk;
    st3r_stream_grid(C, HW, &blocks, &chunk);
    double* part;
    int rc = dp_partials(ctx, C, blocks, &part);
    if (rc) return rc;
    const bool vec = HW % 4 == 0 && dp_al16(depth) && dp_al16(alpha) && dp_al16(prior) && dp_al16(weight) &&
                     dp_al16(v_depth) && dp_al16(v_alpha);
    if (vec)
        hipLaunchKernelGGL(k_dprior_loss<true>, dim3(blocks, C), dim3(DP_T), 0, s, HW, chunk, depth, alpha, prior, weight,
                           norm, norm_stride, depth_fac, v_depth, v_alpha, part);
    else
        hipLaunchKernelGGL(k_dprior_loss<false>, dim3(blocks, C), dim3(DP_T), 0, s, HW, chunk, depth, alpha, prior, weight,
                           norm, norm_stride, depth_fac, v_depth, v_alpha, part);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(k_dprior_finish, dim3(C), dim3(DP_T), 0, s, blocks, (const double*)part, sums, sums_stride, 0);
    LAUNCH_CHECK();
    return ST3R_OK;
}

// The registered prior that belongs to the C views at `gt` (fused_step.hip): out->prior = NULL if there is none (no registration,
// depth_fac == 0, another image size, or not a whole-view offset into the registered images).  The n_c of the
// registration are computed by the first call that gets here, on its stream.
int st3r_depth_prior_for(st3r_ctx* ctx, hipStream_t s, const float* gt, int C, int H, int W, DepthPrior* out) {
    *out = DepthPrior{};
    if (!ctx->dp_depth || ctx->dp_fac == 0.f || H != ctx->dp_h || W != ctx->dp_w) return ST3R_OK;
    const int64_t img = (int64_t)H * W * 3, HW = (int64_t)H * W;
    if (gt < ctx->dp_gt || (gt - ctx->dp_gt) % img != 0) return ST3R_OK;
    const int64_t c0 = (gt - ctx->dp_gt) / img;
    if (c0 + C > ctx->dp_c) return ST3R_OK;
    void* p = nullptr; int grown = 0;
    int rc = st3r_arena_get2(ctx, SLOT_DPRIOR_NORM, sizeof(double) * (size_t)ctx->dp_c, &p, &grown);
    if (rc) return rc;
    if (grown || !ctx->dp_norm_valid) {
        rc = dp_norms(ctx, s, ctx->dp_c, HW, ctx->dp_weight, (double*)p, 1);
        if (rc) return rc;
        ctx->dp_norm_valid = 1;
    }
    *out = DepthPrior{ctx->dp_depth + c0 * HW, ctx->dp_weight + c0 * HW, (const double*)p + c0, ctx->dp_fac};
    return ST3R_OK;
}

ST3R_EXPORT int st3r_ctx_set_depth_prior(st3r_ctx* ctx, const float* gt, const float* depth, const float* weight, int C,
                                         int height, int width, float depth_fac) {
    ARG_CHECK(ctx);
    ctx->dp_norm_valid = 0;
    if (!gt || !depth || !weight) {
        ctx->dp_gt = nullptr; ctx->dp_depth = nullptr; ctx->dp_weight = nullptr;
        ctx->dp_c = ctx->dp_h = ctx->dp_w = 0; ctx->dp_fac = 0.f;
        return ST3R_OK;
    }
    ARG_CHECK(C > 0 && height > 0 && width > 0 && depth_fac == depth_fac);
    ctx->dp_gt = gt; ctx->dp_depth = depth; ctx->dp_weight = weight;
    ctx->dp_c = C; ctx->dp_h = height; ctx->dp_w = width; ctx->dp_fac = depth_fac;
    return ST3R_OK;
}

ST3R_EXPORT int st3r_loss_depth_prior(st3r_ctx* ctx, void* stream, int C, int height, int width, const float* depth,
                                      const float* alpha, const float* prior, const float* weight, float depth_fac,
                                      double* sums, float* v_depth, float* v_alpha) {
    ARG_CHECK(ctx && C > 0 && height > 0 && width > 0);
    ARG_CHECK(depth && alpha && prior && weight && sums && v_depth && v_alpha);
    hipStream_t s = (hipStream_t)stream;
    int rc = dp_norms(ctx, s, C, (int64_t)height * width, weight, sums + 1, 2);
    if (rc) return rc;
    return st3r_depth_prior_loss_impl(ctx, s, C, height, width, depth, alpha, prior, weight, sums + 1, 2, depth_fac, sums, 2,
                                      v_depth, v_alpha);
}
