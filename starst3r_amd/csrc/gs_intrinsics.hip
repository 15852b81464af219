// Intrinsics backward: the gradient of a render loss with respect to each camera's (fx, fy, cx, cy), its Adam step and
// the registration that makes the fused training step write it (self-calibrating few-view training: the focal the
// alignment estimated is good, not exact, and no pose update can remove a focal error).
//
// Input: the per-pair gradients v_splats that st3r_gs_blend_bwd writes (v_means2d 0:2, v_conic 3:6) -- what
// st3r_gs_viewmat_bwd consumes; colour (6:9) and depth (float 9) do not depend on K.  Per visible pair (camera c,
// Gaussian g), in the float32 arithmetic of k_project_sh_bwd and k_viewmat_bwd_part:
//     p = R m + t = (x, y, z),  S = R Sigma R^T,  J = [[a, 0, cj], [0, b, d]]
//     a = fx / z,  cj = -fx tx / z^2,  b = fy / z,  d = -fy ty / z^2,   tx = z clamp(x / z, -lim_xn, lim_xp)
//     mean2d = (fx x / z + cx, fy y / z + cy)
//     v_fx = vm2x x / z + vJ00 / z + vJ02 dcj/dfx          v_cx = vm2x + vJ02 dcj/dcx          (y alike)
// The clamp limits depend on K -- lim_xp = (1.15 W - cx) / fx, lim_xn = (0.15 W + cx) / fx -- and the gradient is that
// of the forward AS COMPUTED: an unclamped pair has cj = -fx x / z^2, so dcj/dfx = -x / z^2 and dcj/dcx = 0; a pair
// clamped high has cj = -(1.15 W - cx) / z, one clamped low cj = (0.15 W + cx) / z: dcj/dfx = 0 and dcj/dcx = 1 / z on
// both sides.  The tile rectangle and the culling stay non-differentiable, as everywhere else here.
//
// The conic chain rule (conic_chain) is project_common.h's; covariance and projection are written out as in
// k_viewmat_bwd_part and must be kept equal by hand ("What the projection kernels share").
//
// Reduction as in gs_pose_bwd.hip: grid (blocks of 256 Gaussians, C); each block sums its 256 pairs' four terms in double
// in a fixed order and writes one partial; k_stream_finish, one workgroup per camera, adds that camera's partials in a
// fixed order.  No atomics: the same inputs give the same bits.  v_cx is a plain sum of v_means2d.x over up to 10^6 pairs
// and cancels the way the pose translation does -- hence double.
#include "per_view.h"   // block_sum_fixed, k_stream_finish, per-view Adam
#include "project_common.h"

__global__ __launch_bounds__(256) void k_intrinsics_bwd_part(
    int N, const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
    const float* __restrict__ viewmats, const float* __restrict__ Ks, int W, int H, const float4* __restrict__ splats,
    const float4* __restrict__ v_splats, double* __restrict__ part) {
    __shared__ double red[4 * 4];
    const int c = blockIdx.y;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    float v_fx = 0.f, v_fy = 0.f, v_cx = 0.f, v_cy = 0.f;
    const int64_t pid = (int64_t)c * N + g;
    if (g < N && __float_as_int(splats[pid * 3 + 2].z) > 0) {   // radius word first: culled pairs load nothing else
        const float4 r0 = splats[pid * 3 + 0], r1 = splats[pid * 3 + 1];
        const float4 g0 = v_splats[pid * 3 + 0], g1 = v_splats[pid * 3 + 1];
        const float* V = viewmats + 16 * c;
        const float R[9] = {V[0], V[1], V[2], V[4], V[5], V[6], V[8], V[9], V[10]};
        const float* K = Ks + 9 * c;
        const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
        const float tan_fovx = 0.5f * (float)W / fx, tan_fovy = 0.5f * (float)H / fy;
        const float lim_xp = ((float)W - cx) / fx + 0.3f * tan_fovx, lim_xn = cx / fx + 0.3f * tan_fovx;
        const float lim_yp = ((float)H - cy) / fy + 0.3f * tan_fovy, lim_yn = cy / fy + 0.3f * tan_fovy;
        const float mx = means[3 * g], my = means[3 * g + 1], mz = means[3 * g + 2];
        float qw = quats[4 * g], qx = quats[4 * g + 1], qy = quats[4 * g + 2], qz = quats[4 * g + 3];
        const float sc[3] = {scales[3 * g], scales[3 * g + 1], scales[3 * g + 2]};
        // world covariance Sigma = M M^T, M = Rq diag(s)
        const float inv_norm = 1.0f / sqrtf(((qw * qw + qx * qx) + qy * qy) + qz * qz);
        qw *= inv_norm; qx *= inv_norm; qy *= inv_norm; qz *= inv_norm;
        float cov[6];
        {
            float x2 = qx * qx, y2 = qy * qy, z2 = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz;
            float wx = qw * qx, wy = qw * qy, wz = qw * qz;
            const float Rq[9] = {1.0f - 2.0f * (y2 + z2), 2.0f * (xy - wz), 2.0f * (xz + wy),
                                 2.0f * (xy + wz), 1.0f - 2.0f * (x2 + z2), 2.0f * (yz - wx),
                                 2.0f * (xz - wy), 2.0f * (yz + wx), 1.0f - 2.0f * (x2 + y2)};
            float M[9];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) M[i * 3 + j] = Rq[i * 3 + j] * sc[j];
            cov[0] = M[0] * M[0] + M[1] * M[1] + M[2] * M[2];
            cov[1] = M[0] * M[3] + M[1] * M[4] + M[2] * M[5];
            cov[2] = M[0] * M[6] + M[1] * M[7] + M[2] * M[8];
            cov[3] = M[3] * M[3] + M[4] * M[4] + M[5] * M[5];
            cov[4] = M[3] * M[6] + M[4] * M[7] + M[5] * M[8];
            cov[5] = M[6] * M[6] + M[7] * M[7] + M[8] * M[8];
        }
        const float x = R[0] * mx + R[1] * my + R[2] * mz + V[3];
        const float y = R[3] * mx + R[4] * my + R[5] * mz + V[7];
        const float z = R[6] * mx + R[7] * my + R[8] * mz + V[11];
        float T[9];   // R Sigma
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            T[i * 3 + 0] = R[i * 3] * cov[0] + R[i * 3 + 1] * cov[1] + R[i * 3 + 2] * cov[2];
            T[i * 3 + 1] = R[i * 3] * cov[1] + R[i * 3 + 1] * cov[3] + R[i * 3 + 2] * cov[4];
            T[i * 3 + 2] = R[i * 3] * cov[2] + R[i * 3 + 1] * cov[4] + R[i * 3 + 2] * cov[5];
        }
        const Sym3 S = {T[0] * R[0] + T[1] * R[1] + T[2] * R[2], T[0] * R[3] + T[1] * R[4] + T[2] * R[5],
                        T[0] * R[6] + T[1] * R[7] + T[2] * R[8], T[3] * R[3] + T[4] * R[4] + T[5] * R[5],
                        T[3] * R[6] + T[4] * R[7] + T[5] * R[8], T[6] * R[6] + T[7] * R[7] + T[8] * R[8]};
        const float rz = 1.0f / z, rz2 = rz * rz;
        const float xr = x * rz, yr = y * rz;
        const bool x_in = (xr <= lim_xp) && (xr >= -lim_xn);
        const bool y_in = (yr <= lim_yp) && (yr >= -lim_yn);
        const float tx = z * fminf(lim_xp, fmaxf(-lim_xn, xr));
        const float ty = z * fminf(lim_yp, fmaxf(-lim_yn, yr));
        const float a = fx * rz, cj = -fx * tx * rz2, b = fy * rz, d = -fy * ty * rz2;
        Sym3 vS;
        float vJ00, vJ02, vJ11, vJ12;
        conic_chain(r0, r1, g0, g1, a, cj, b, d, S, vS, vJ00, vJ02, vJ11, vJ12);
        const float vm2x = g0.x, vm2y = g0.y;
        v_fx = vm2x * xr + vJ00 * rz;
        v_fy = vm2y * yr + vJ11 * rz;
        v_cx = vm2x; v_cy = vm2y;
        if (x_in) v_fx += -x * rz2 * vJ02;
        else v_cx += vJ02 * rz;
        if (y_in) v_fy += -y * rz2 * vJ12;
        else v_cy += vJ12 * rz;
    }
    double v[4] = {(double)v_fx, (double)v_fy, (double)v_cx, (double)v_cy};
    const double t = block_sum_fixed(v, red);
    if (threadIdx.x < 4) part[((int64_t)c * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = t;
}

ST3R_EXPORT int st3r_gs_intrinsics_bwd(st3r_ctx* ctx, void* stream, int N, int C, const float* means, const float* quats,
                                       const float* scales, const float* viewmats, const float* Ks, int width, int height,
                                       float eps2d, const float* splats, const float* v_splats, float* v_Ks) {
    ARG_CHECK(ctx && N >= 0 && C > 0 && C <= ST3R_MAX_VIEWS && width > 0 && height > 0);
    ARG_CHECK(means && quats && scales && viewmats && Ks && splats && v_splats && v_Ks);
    (void)eps2d;   // the conic in the splat records already holds it
    hipStream_t s = (hipStream_t)stream;
    const int nb = ceil_div(N, 256);
    double* part = nullptr;
    if (nb > 0) {
        ARENA_GET(SLOT_KGRAD_PART, double, 4 * (size_t)nb * C, p);
        part = p;
        hipLaunchKernelGGL(k_intrinsics_bwd_part, dim3(nb, C), dim3(256), 0, s, N, means, quats, scales, viewmats, Ks,
                           width, height, (const float4*)splats, (const float4*)v_splats, part);
        LAUNCH_CHECK();
    }
    return stream_finish<4>(s, C, nb, (const double*)part, v_Ks, 4, 0);   // (no partials: exact zeros)
}

// The rows of the registered v_Ks that belong to the C views at `gt` (fused_step.hip), or NULL if no registration
// applies (view_reg_first).
float* st3r_intrinsics_grad_for(st3r_ctx* ctx, const float* gt, int C, int H, int W) {
    const int64_t c0 = view_reg_first(ctx->kg, gt, C, H, W);
    return c0 < 0 ? nullptr : ctx->kg_v_Ks + 4 * c0;
}

ST3R_EXPORT int st3r_ctx_set_intrinsics_grad(st3r_ctx* ctx, const float* gt, float* v_Ks, int C, int height, int width) {
    ARG_CHECK(ctx);
    const bool on = gt && v_Ks;
    int rc = view_reg_set(&ctx->kg, on, gt, C, height, width);
    if (rc) return rc;
    ctx->kg_v_Ks = on ? v_Ks : nullptr;
    return ST3R_OK;
}

// Intrinsics Adam: the per-view Adam of per_view.h on q = (log fx, log fy, cx / W, cy / H), so that one learning rate is
// free of the image's scale: g = (fx v_fx, fy v_fy, W v_cx, H v_cy);  fx <- fx exp(delta_0), fy <- fy exp(delta_1),
// cx <- cx + W delta_2, cy <- cy + H delta_3.  mode bit 0 ties the focals (one scalar, gradient g_0 + g_1, moment slot 0;
// both focals take the same factor, slot 1 is not touched), bit 1 trains the principal point (without it cx, cy and
// their moments keep every bit).  Skew and row 2 of K are never written.
// Of the two forms of per_view_adam_delta this is <false>, k_exposure_adam's (rounds b1 m, fuses (1 - b1) g): this
// kernel, like that one, runs behind the training step as a launch of its own.
__global__ __launch_bounds__(64) void k_intrinsics_adam(int C, PerViewAdamK k, float* __restrict__ Ks,
                                                        const float* __restrict__ v_Ks, float* __restrict__ k_m,
                                                        float* __restrict__ k_v, double W, double H, int mode) {
    const int c = per_view_adam_view(k, C);
    if (c < 0) return;   // (a frozen view keeps K, m and v bit for bit)
    float* K = Ks + 9 * c;
    const float* G = v_Ks + 4 * c;
    float* m = k_m + 4 * c;
    float* v = k_v + 4 * c;
    const double fx = (double)K[0], fy = (double)K[4];
    const double g0 = fx * (double)G[0], g1 = fy * (double)G[1];
    if (mode & 1) {
        const double e = exp(per_view_adam_delta<false>(k, m[0], g0 + g1, v[0]));
        K[0] = (float)(fx * e); K[4] = (float)(fy * e);
    } else {
        K[0] = (float)(fx * exp(per_view_adam_delta<false>(k, m[0], g0, v[0])));
        K[4] = (float)(fy * exp(per_view_adam_delta<false>(k, m[1], g1, v[1])));
    }
    if (mode & 2) {
        K[2] = (float)((double)K[2] + W * per_view_adam_delta<false>(k, m[2], W * (double)G[2], v[2]));
        K[5] = (float)((double)K[5] + H * per_view_adam_delta<false>(k, m[3], H * (double)G[3], v[3]));
    }
}

ST3R_EXPORT int st3r_intrinsics_adam_step(st3r_ctx* ctx, void* stream, int C, float* Ks, const float* v_Ks, float* k_m,
                                          float* k_v, double lr, double beta1, double beta2, double eps, int step,
                                          const float* mask, int width, int height, int mode) {
    ARG_CHECK(ctx && C > 0 && step >= 1 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0);
    ARG_CHECK(Ks && v_Ks && k_m && k_v && width > 0 && height > 0 && mode >= 0 && mode <= 3);
    return per_view_adam_launch(ctx, (hipStream_t)stream, k_intrinsics_adam, C, lr, beta1, beta2, eps, step, mask, Ks, v_Ks,
                                k_m, k_v, (double)width, (double)height, mode);
}
