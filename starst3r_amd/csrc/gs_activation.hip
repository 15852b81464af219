// The canonical 3DGS parameterisation (scene.activations): the scales tensor holds log-scales, the opacities tensor logits.
//     activate    S = expf(s)                       float32, precise expf (not __expf), over the flat 3N floats
//                 O = 1 / (1 + expf(-o))            float32, correctly rounded add and divide, over the N floats
//                 reg_sums[0] = sum O, reg_sums[1] = sum S     the STORED float32 values, added in double
//     backward    v_s = (v_S + reg_s_k) * S         two float32 roundings, in that order
//                 v_o = ((v_O + reg_o_k) * O) * (1 - O)        four, in that order (1 - O is rounded on its own)
// The backward reads the stored activated values: no transcendental, no second rounding of the activation, and
// reg_*_k = 0 is the plain chain rule.  Its outputs may be its inputs v_S / v_O (the fused step runs it in place on the
// scales and opacities blocks of the gradient buffer): a thread reads its elements before it writes them and nobody else
// touches them, so those pointers carry no __restrict__.  A logit of -90 gives expf(90) = inf and O = 0, one of +90 gives
// O = 1; both gradients are then exactly 0 -- the saturated sigmoid has no NaN.
//
// Two streaming kernels on the scaffold of per_view.h (chunks, grid, sums): the Gaussians are dealt to the workgroups of
// stream_grid(1, N) in contiguous chunks, a multiple of 1024, at most 2048 workgroups: one resident round of the chip.  A
// thread takes four Gaussians per access: one 16-byte access of the opacities and three of the scales, as k_composite_fwd
// takes four pixels.  That is the form of aligned pointers (kernel<true>); the up to three Gaussians behind the last
// multiple of four are taken one by one by the first threads of the last workgroup.  A pointer off the 16-byte grid (a view
// that starts one float into a buffer; the gradient blocks at 7N and 10N floats when N is no multiple of four) selects
// the 4-byte form (kernel<false>): gs_alpha.hip's rule.  Traffic: 32 bytes per Gaussian forward, 48 backward.
// Sums: every thread adds its stored values in double, the workgroup meets in block_sum_fixed, one partial of two doubles
// per workgroup; k_stream_finish, one workgroup, adds the partials in a fixed order (more than 256 partials, N > 256 * 1024:
// a second trip of its loop).  No atomics: the same inputs give the same bits.
// No contraction in this file: the backward's roundings are the ones written above.
#include "per_view.h"
#pragma clang fp contract(off)

__device__ __forceinline__ float act_scale(float s) { return expf(s); }
__device__ __forceinline__ float act_opacity(float o) { return 1.0f / (1.0f + expf(-o)); }
__device__ __forceinline__ float act_scale_bwd(float v, float k, float S) { return (v + k) * S; }
__device__ __forceinline__ float act_opacity_bwd(float v, float k, float O) { return ((v + k) * O) * (1.0f - O); }

// the Gaussians [lo, hi4) of this workgroup that go four at a time and, for the last workgroup of the VEC form, the tail
// [N4, N) that goes one at a time; the 4-byte form walks [lo, hi) one at a time
template <bool VEC>
__device__ __forceinline__ void act_chunk(const int64_t& chunk, const int64_t& N, int64_t& lo, int64_t& hi, int64_t& hi4) {
    stream_chunk(chunk, N, lo, hi);
    hi4 = VEC ? min(hi, N & ~(int64_t)3) : lo;   // (chunk is a multiple of 4, so lo is)
}

template <bool VEC, bool SUMS>
__global__ __launch_bounds__(STREAM_T) void k_param_activate(int64_t N, int64_t chunk, const float* __restrict__ scales,
                                                             const float* __restrict__ opacities,
                                                             float* __restrict__ act_scales,
                                                             float* __restrict__ act_opacities,
                                                             double* __restrict__ part) {
    __shared__ double red[8];
    int64_t lo, hi, hi4;
    act_chunk<VEC>(chunk, N, lo, hi, hi4);
    double acc[2] = {0.0, 0.0};   // sum O, sum S
    if (VEC) {
        for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi4; i += 4 * STREAM_T) {   // Gaussians i .. i + 3
            alignas(16) float sv[12], ov[4];
            const float4* src = reinterpret_cast<const float4*>(scales + 3 * i);
            *reinterpret_cast<float4*>(sv) = src[0]; *reinterpret_cast<float4*>(sv + 4) = src[1];
            *reinterpret_cast<float4*>(sv + 8) = src[2];
            *reinterpret_cast<float4*>(ov) = *reinterpret_cast<const float4*>(opacities + i);
#pragma unroll
            for (int k = 0; k < 12; ++k) { sv[k] = act_scale(sv[k]); if (SUMS) acc[1] += (double)sv[k]; }
#pragma unroll
            for (int k = 0; k < 4; ++k) { ov[k] = act_opacity(ov[k]); if (SUMS) acc[0] += (double)ov[k]; }
            float4* dst = reinterpret_cast<float4*>(act_scales + 3 * i);
            dst[0] = *reinterpret_cast<float4*>(sv); dst[1] = *reinterpret_cast<float4*>(sv + 4);
            dst[2] = *reinterpret_cast<float4*>(sv + 8);
            *reinterpret_cast<float4*>(act_opacities + i) = *reinterpret_cast<float4*>(ov);
        }
    }
    for (int64_t i = hi4 + threadIdx.x; i < hi; i += STREAM_T) {   // the 4-byte form, or the tail behind the last four
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float S = act_scale(scales[3 * i + k]);
            act_scales[3 * i + k] = S;
            if (SUMS) acc[1] += (double)S;
        }
        const float O = act_opacity(opacities[i]);
        act_opacities[i] = O;
        if (SUMS) acc[0] += (double)O;
    }
    if (SUMS) {
        const double t = block_sum_fixed(acc, red);
        if (threadIdx.x < 2) part[2 * (int64_t)blockIdx.x + threadIdx.x] = t;
    }
}

// v_scales may be v_act_scales and v_opacities may be v_act_opacities (in place)
template <bool VEC>
__global__ __launch_bounds__(STREAM_T) void k_param_activate_bwd(int64_t N, int64_t chunk, const float* __restrict__ act_scales,
                                                                 const float* __restrict__ act_opacities,
                                                                 const float* v_act_scales, const float* v_act_opacities,
                                                                 float reg_s_k, float reg_o_k, float* v_scales,
                                                                 float* v_opacities) {
    int64_t lo, hi, hi4;
    act_chunk<VEC>(chunk, N, lo, hi, hi4);
    if (VEC) {
        for (int64_t i = lo + 4 * (int64_t)threadIdx.x; i < hi4; i += 4 * STREAM_T) {
            alignas(16) float Sv[12], gv[12], Ov[4], hv[4];
            const float4* sS = reinterpret_cast<const float4*>(act_scales + 3 * i);
            const float4* sg = reinterpret_cast<const float4*>(v_act_scales + 3 * i);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                *reinterpret_cast<float4*>(Sv + 4 * q) = sS[q]; *reinterpret_cast<float4*>(gv + 4 * q) = sg[q];
            }
            *reinterpret_cast<float4*>(Ov) = *reinterpret_cast<const float4*>(act_opacities + i);
            *reinterpret_cast<float4*>(hv) = *reinterpret_cast<const float4*>(v_act_opacities + i);
#pragma unroll
            for (int k = 0; k < 12; ++k) gv[k] = act_scale_bwd(gv[k], reg_s_k, Sv[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) hv[k] = act_opacity_bwd(hv[k], reg_o_k, Ov[k]);
            float4* dst = reinterpret_cast<float4*>(v_scales + 3 * i);
#pragma unroll
            for (int q = 0; q < 3; ++q) dst[q] = *reinterpret_cast<float4*>(gv + 4 * q);
            *reinterpret_cast<float4*>(v_opacities + i) = *reinterpret_cast<float4*>(hv);
        }
    }
    for (int64_t i = hi4 + threadIdx.x; i < hi; i += STREAM_T) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v_scales[3 * i + k] = act_scale_bwd(v_act_scales[3 * i + k], reg_s_k, act_scales[3 * i + k]);
        v_opacities[i] = act_opacity_bwd(v_act_opacities[i], reg_o_k, act_opacities[i]);
    }
}

// reg_sums != NULL: double[2] on the device, written whole -- sum O, sum S of the stored values
int st3r_param_activate_impl(st3r_ctx* ctx, hipStream_t s, int N, const float* scales, const float* opacities,
                             float* act_scales, float* act_opacities, double* reg_sums) {
    int blocks; int64_t chunk;
    stream_grid(1, (int64_t)N, &blocks, &chunk);
    double* part = nullptr;
    if (reg_sums) {
        ARENA_GET(SLOT_ACT_PART, double, 2 * (size_t)blocks, p);
        part = p;
    }
    LAUNCH_BOOL2(k_param_activate, aligned16(scales, opacities, act_scales, act_opacities), reg_sums != nullptr, dim3(blocks),
                 dim3(STREAM_T), s, (int64_t)N, chunk, scales, opacities, act_scales, act_opacities, part);
    return reg_sums ? stream_finish<2>(s, 1, blocks, part, reg_sums, 2, 0) : ST3R_OK;
}

int st3r_param_activate_bwd_impl(hipStream_t s, int N, const float* act_scales, const float* act_opacities,
                                 const float* v_act_scales, const float* v_act_opacities, float reg_s_k, float reg_o_k,
                                 float* v_scales, float* v_opacities) {
    int blocks; int64_t chunk;
    stream_grid(1, (int64_t)N, &blocks, &chunk);
    const bool vec = aligned16(act_scales, act_opacities, v_act_scales, v_act_opacities, v_scales, v_opacities);
    if (vec) hipLaunchKernelGGL(k_param_activate_bwd<true>, dim3(blocks), dim3(STREAM_T), 0, s, (int64_t)N, chunk, act_scales,
                                act_opacities, v_act_scales, v_act_opacities, reg_s_k, reg_o_k, v_scales, v_opacities);
    else hipLaunchKernelGGL(k_param_activate_bwd<false>, dim3(blocks), dim3(STREAM_T), 0, s, (int64_t)N, chunk, act_scales,
                            act_opacities, v_act_scales, v_act_opacities, reg_s_k, reg_o_k, v_scales, v_opacities);
    LAUNCH_CHECK();
    return ST3R_OK;
}

// the activated copies of a call's scales and opacities in the ctx's scratch (fused_step.hip)
int st3r_activated_params(st3r_ctx* ctx, hipStream_t s, const GsParams& g, double* reg_sums, GsParams* out) {
    ARENA_GET(SLOT_ACT_SCALES, float, 3 * (size_t)g.N, as);
    ARENA_GET(SLOT_ACT_OPACITIES, float, (size_t)g.N, ao);
    int rc = st3r_param_activate_impl(ctx, s, g.N, g.scales, g.opacities, as, ao, reg_sums);
    *out = g;
    out->scales = as; out->opacities = ao;
    return rc;
}

ST3R_EXPORT int st3r_ctx_set_activation(st3r_ctx* ctx, int on) {
    ARG_CHECK(ctx && (on == 0 || on == 1));
    ctx->activation = on;
    return ST3R_OK;
}

ST3R_EXPORT int st3r_ctx_get_activation(st3r_ctx* ctx, int* on) {
    ARG_CHECK(ctx && on);
    *on = ctx->activation;
    return ST3R_OK;
}

ST3R_EXPORT int st3r_param_activate(st3r_ctx* ctx, void* stream, int N, const float* scales, const float* opacities,
                                    float* act_scales, float* act_opacities, double* reg_sums) {
    ARG_CHECK(ctx && N > 0 && scales && opacities && act_scales && act_opacities);
    return st3r_param_activate_impl(ctx, (hipStream_t)stream, N, scales, opacities, act_scales, act_opacities, reg_sums);
}

ST3R_EXPORT int st3r_param_activate_bwd(st3r_ctx* ctx, void* stream, int N, const float* act_scales,
                                        const float* act_opacities, const float* v_act_scales, const float* v_act_opacities,
                                        float reg_s_k, float reg_o_k, float* v_scales, float* v_opacities) {
    ARG_CHECK(ctx && N > 0 && act_scales && act_opacities && v_act_scales && v_act_opacities && v_scales && v_opacities);
    ARG_CHECK(reg_s_k - reg_s_k == 0.f && reg_o_k - reg_o_k == 0.f);   // finite
    return st3r_param_activate_bwd_impl((hipStream_t)stream, N, act_scales, act_opacities, v_act_scales, v_act_opacities,
                                        reg_s_k, reg_o_k, v_scales, v_opacities);
}
