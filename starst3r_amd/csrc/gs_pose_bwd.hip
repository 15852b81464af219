// Pose backward: the gradient of a render loss with respect to each camera's world-to-camera matrix (gsplat returns
// v_viewmats when viewmats require a gradient; render_3dgs stands in for gsplat.rasterization, starster/gs.py:76-87).
//
// Input: the per-pair gradients v_splats that st3r_gs_blend_bwd writes (v_means2d 0:2, v_opacity 2, v_conic 3:6,
// v_colour 6:9).  Per visible pair (camera c, Gaussian g), in the float32 arithmetic of k_project_sh_bwd:
//     p = R m + t,  S = R Sigma R^T         v_p  (camera-space mean),  vS (symmetric, camera covariance)
//     d = m - campos_c                      v_d  (SH view direction, clamp_min(c + 0.5, 0) pass-through)
//     v_t_c += v_p      v_R_c += v_p m^T + 2 vS R Sigma      v_campos_c += -v_d
// Per camera, through campos = inverse(V)[:3, 3]:
//     v_V = [[v_R, v_t], [0, 0]] - (V^-T [v_campos; 0]) (x) inverse(V)[:, 3]
//
// The conic chain rule (conic_chain) is project_common.h's, shared with k_project_sh_bwd.  The rest of the per-pair
// arithmetic is still written out in both kernels and must be kept equal by hand: a shared function for it changes the
// machine code of k_project_sh_bwd, the tuned training kernel ("What the projection kernels share").
//
// Reduction without float atomics (bit-reproducible, like every backward here): grid (blocks of 256 Gaussians, C);
// each block sums its 256 pairs' 15 terms in double in a fixed order (wave butterfly, then the four waves in order) and
// writes one partial; one workgroup per camera then sums that camera's partials in a fixed order and applies the
// finisher.  Translation terms of a photometric loss cancel heavily over up to 10^6 pairs -- hence double.
#include "per_view.h"   // block_sum_fixed
#include "project_common.h"

#define POSE_VALS 15   // v_R (9, row-major), v_t (3), v_campos (3)

// Sum of v over the 256 threads of a workgroup, in a fixed order; the result is in red[0 .. POSE_VALS) after the call.
// red: 5 * POSE_VALS doubles of LDS.
__device__ __forceinline__ void block_sum_pose(double (&v)[POSE_VALS], double* red) {
    const double sum = block_sum_fixed(v, red);
    if (threadIdx.x < POSE_VALS) red[4 * POSE_VALS + threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x < POSE_VALS) red[threadIdx.x] = red[4 * POSE_VALS + threadIdx.x];
    __syncthreads();
}

// DEG: the SH degree in use (st3r_ctx_set_sh_degree); 1 is the kernel as it always was
template <int DEG>
__global__ __launch_bounds__(256) void k_viewmat_bwd_part(
    int N, const float* __restrict__ means, const float* __restrict__ quats, const float* __restrict__ scales,
    const float* __restrict__ sh, int sh_stride, const float* __restrict__ viewmats, const float* __restrict__ Ks,
    const float* __restrict__ campos, int W, int H, const float4* __restrict__ splats,
    const float4* __restrict__ v_splats, double* __restrict__ part) {
    __shared__ double red[5 * POSE_VALS];
    const int c = blockIdx.y;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    float acc[POSE_VALS];
#pragma unroll
    for (int k = 0; k < POSE_VALS; ++k) acc[k] = 0.f;
    const int64_t pid = (int64_t)c * N + g;
    if (g < N && __float_as_int(splats[pid * 3 + 2].z) > 0) {   // radius word first: culled pairs load nothing else
        const float4 r0 = splats[pid * 3 + 0], r1 = splats[pid * 3 + 1], r2 = splats[pid * 3 + 2];
        const float4 g0 = v_splats[pid * 3 + 0], g1 = v_splats[pid * 3 + 1], g2 = v_splats[pid * 3 + 2];
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
        constexpr int KF = 3 * SH_ROWS(DEG);   // coefficient floats read per Gaussian
        float k[KF];
        const float* kp = sh + (int64_t)g * sh_stride;
#pragma unroll
        for (int i = 0; i < KF; ++i) k[i] = kp[i];
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
        // ---- SH backward: v_d, the gradient of the unnormalised direction d = m - campos ----
        if constexpr (DEG == 1) {
            float dx = mx - campos[3 * c], dy = my - campos[3 * c + 1], dz = mz - campos[3 * c + 2];
            float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
            float inrm = 1.0f / nrm;
            float ux = dx * inrm, uy = dy * inrm, uz = dz * inrm;
            const float vcol[3] = {g1.z, g1.w, g2.x};
            const float colf[3] = {r1.z, r1.w, r2.x};
            float vdx = 0.f, vdy = 0.f, vdz = 0.f;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                // clamp_min(c+0.5, 0) passes gradient where the pre-clamp value is >= 0 (as k_project_sh_bwd)
                float pre = SH_C0 * k[ch] + SH_C1 * ((-uy * k[3 + ch] + uz * k[6 + ch]) - ux * k[9 + ch]) + 0.5f;
                float vc = (colf[ch] > 0.0f || pre >= 0.0f) ? vcol[ch] : 0.0f;
                vdx += -SH_C1 * k[9 + ch] * vc;
                vdy += -SH_C1 * k[3 + ch] * vc;
                vdz += SH_C1 * k[6 + ch] * vc;
            }
            float dotp = vdx * ux + vdy * uy + vdz * uz;
            acc[12] = -((vdx - dotp * ux) * inrm);
            acc[13] = -((vdy - dotp * uy) * inrm);
            acc[14] = -((vdz - dotp * uz) * inrm);
        } else {
            float dx = mx - campos[3 * c], dy = my - campos[3 * c + 1], dz = mz - campos[3 * c + 2];
            float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
            float inrm = 1.0f / nrm;
            float ux = dx * inrm, uy = dy * inrm, uz = dz * inrm;
            const float vcol[3] = {g1.z, g1.w, g2.x};
            const float colf[3] = {r1.z, r1.w, r2.x};
            float vdx, vdy, vdz;
            sh_chain<DEG, false>(k, vcol, colf, ux, uy, uz, nullptr, vdx, vdy, vdz);
            float dotp = vdx * ux + vdy * uy + vdz * uz;
            acc[12] = -((vdx - dotp * ux) * inrm);
            acc[13] = -((vdy - dotp * uy) * inrm);
            acc[14] = -((vdz - dotp * uz) * inrm);
        }
        // ---- projection backward: v_p and vS ----
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
        const float S00 = T[0] * R[0] + T[1] * R[1] + T[2] * R[2];
        const float S01 = T[0] * R[3] + T[1] * R[4] + T[2] * R[5];
        const float S02 = T[0] * R[6] + T[1] * R[7] + T[2] * R[8];
        const float S11 = T[3] * R[3] + T[4] * R[4] + T[5] * R[5];
        const float S12 = T[3] * R[6] + T[4] * R[7] + T[5] * R[8];
        const float S22 = T[6] * R[6] + T[7] * R[7] + T[8] * R[8];
        const float rz = 1.0f / z, rz2 = rz * rz, rz3 = rz2 * rz;
        const float xr = x * rz, yr = y * rz;
        const bool x_in = (xr <= lim_xp) && (xr >= -lim_xn);
        const bool y_in = (yr <= lim_yp) && (yr >= -lim_yn);
        const float tx = z * fminf(lim_xp, fmaxf(-lim_xn, xr));
        const float ty = z * fminf(lim_yp, fmaxf(-lim_yn, yr));
        const float a = fx * rz, cj = -fx * tx * rz2, b = fy * rz, d = -fy * ty * rz2;
        const Sym3 S = {S00, S01, S02, S11, S12, S22};
        Sym3 vS;
        float vJ00, vJ02, vJ11, vJ12;
        conic_chain(r0, r1, g0, g1, a, cj, b, d, S, vS, vJ00, vJ02, vJ11, vJ12);
        const float vm2x = g0.x, vm2y = g0.y;
        float vpx = fx * rz * vm2x;
        float vpy = fy * rz * vm2y;
        float vpz = -(fx * x * vm2x + fy * y * vm2y) * rz2;
        vpz += -fx * rz2 * vJ00 - fy * rz2 * vJ11;
        if (x_in) { vpx += -fx * rz2 * vJ02; vpz += 2.0f * fx * x * rz3 * vJ02; }
        else { vpz += fx * tx * rz3 * vJ02; }
        if (y_in) { vpy += -fy * rz2 * vJ12; vpz += 2.0f * fy * y * rz3 * vJ12; }
        else { vpz += fy * ty * rz3 * vJ12; }
        // v_R = v_p m^T + 2 vS (R Sigma),  v_t = v_p
        const float vSm[9] = {vS.xx, vS.xy, vS.xz, vS.xy, vS.yy, vS.yz, vS.xz, vS.yz, vS.zz};
        const float vp[3] = {vpx, vpy, vpz}, m[3] = {mx, my, mz};
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                acc[i * 3 + j] = vp[i] * m[j] +
                                 2.0f * (vSm[i * 3] * T[j] + vSm[i * 3 + 1] * T[3 + j] + vSm[i * 3 + 2] * T[6 + j]);
            acc[9 + i] = vp[i];
        }
    }
    double v[POSE_VALS];
#pragma unroll
    for (int k2 = 0; k2 < POSE_VALS; ++k2) v[k2] = (double)acc[k2];
    block_sum_pose(v, red);
    if (threadIdx.x < POSE_VALS)
        part[((int64_t)c * gridDim.x + blockIdx.x) * POSE_VALS + threadIdx.x] = red[threadIdx.x];
}

// one workgroup per camera: its n_part partials in a fixed order, then the chain through campos = inverse(V)[:3, 3]
__global__ __launch_bounds__(256) void k_viewmat_bwd_finish(int n_part, const float* __restrict__ viewmats,
                                                           const double* __restrict__ part,
                                                           float* __restrict__ v_viewmats) {
    __shared__ double red[5 * POSE_VALS];
    const int c = blockIdx.x;
    double v[POSE_VALS];
#pragma unroll
    for (int k = 0; k < POSE_VALS; ++k) v[k] = 0.0;
    const double* pc = part + (int64_t)c * n_part * POSE_VALS;
    for (int b = threadIdx.x; b < n_part; b += blockDim.x) {
#pragma unroll
        for (int k = 0; k < POSE_VALS; ++k) v[k] += pc[(int64_t)b * POSE_VALS + k];
    }
    block_sum_pose(v, red);
    if (threadIdx.x >= 16) return;
    // 4x4 inverse in double (cofactors over 2x2 minors); thread i writes element i of v_V
    double a[16];
    const float* Vf = viewmats + 16 * c;
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = (double)Vf[i];
    const double s0 = a[0] * a[5] - a[4] * a[1], s1 = a[0] * a[6] - a[4] * a[2], s2 = a[0] * a[7] - a[4] * a[3];
    const double s3 = a[1] * a[6] - a[5] * a[2], s4 = a[1] * a[7] - a[5] * a[3], s5 = a[2] * a[7] - a[6] * a[3];
    const double c5 = a[10] * a[15] - a[14] * a[11], c4 = a[9] * a[15] - a[13] * a[11], c3 = a[9] * a[14] - a[13] * a[10];
    const double c2 = a[8] * a[15] - a[12] * a[11], c1 = a[8] * a[14] - a[12] * a[10], c0 = a[8] * a[13] - a[12] * a[9];
    const double idet = 1.0 / (s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0);
    double inv[16];
    inv[0] = (a[5] * c5 - a[6] * c4 + a[7] * c3) * idet;
    inv[1] = (-a[1] * c5 + a[2] * c4 - a[3] * c3) * idet;
    inv[2] = (a[13] * s5 - a[14] * s4 + a[15] * s3) * idet;
    inv[3] = (-a[9] * s5 + a[10] * s4 - a[11] * s3) * idet;
    inv[4] = (-a[4] * c5 + a[6] * c2 - a[7] * c1) * idet;
    inv[5] = (a[0] * c5 - a[2] * c2 + a[3] * c1) * idet;
    inv[6] = (-a[12] * s5 + a[14] * s2 - a[15] * s1) * idet;
    inv[7] = (a[8] * s5 - a[10] * s2 + a[11] * s1) * idet;
    inv[8] = (a[4] * c4 - a[5] * c2 + a[7] * c0) * idet;
    inv[9] = (-a[0] * c4 + a[1] * c2 - a[3] * c0) * idet;
    inv[10] = (a[12] * s4 - a[13] * s2 + a[15] * s0) * idet;
    inv[11] = (-a[8] * s4 + a[9] * s2 - a[11] * s0) * idet;
    inv[12] = (-a[4] * c3 + a[5] * c1 - a[6] * c0) * idet;
    inv[13] = (a[0] * c3 - a[1] * c1 + a[2] * c0) * idet;
    inv[14] = (-a[12] * s3 + a[13] * s1 - a[14] * s0) * idet;
    inv[15] = (a[8] * s3 - a[9] * s1 + a[10] * s0) * idet;
    const int i = threadIdx.x >> 2, j = threadIdx.x & 3;
    // u = V^-T [v_campos; 0],  w = inverse(V)[:, 3] (= [campos; 1] for a rigid V)
    const double u = inv[i] * red[12] + inv[4 + i] * red[13] + inv[8 + i] * red[14];
    const double w = inv[4 * j + 3];
    const double base = i == 3 ? 0.0 : (j == 3 ? red[9 + i] : red[i * 3 + j]);
    v_viewmats[16 * c + threadIdx.x] = (float)(base - u * w);
}

ST3R_EXPORT int st3r_gs_viewmat_bwd(st3r_ctx* ctx, void* stream, int N, int C, const float* means, const float* quats,
                                    const float* scales, const float* sh, int sh_stride, const float* viewmats,
                                    const float* Ks, const float* campos, int width, int height, float eps2d,
                                    const float* splats, const float* v_splats, float* v_viewmats) {
    ARG_CHECK(ctx && N >= 0 && C > 0 && C <= ST3R_MAX_VIEWS && sh_stride >= 12 && width > 0 && height > 0);
    ARG_CHECK(means && quats && scales && sh && viewmats && Ks && campos && splats && v_splats && v_viewmats);
    GsParams gp{N, means, quats, scales, nullptr, sh, sh_stride};
    const int rc_sh = st3r_sh_setting(ctx, &gp, false);   // (reads the coefficients, writes no coefficient gradient)
    if (rc_sh) return rc_sh;
    (void)eps2d;   // the conic in the splat records already holds it
    hipStream_t s = (hipStream_t)stream;
    const int nb = ceil_div(N, 256);
    double* part = nullptr;
    if (nb > 0) {
        ARENA_GET(SLOT_POSE_PART, double, POSE_VALS * (size_t)nb * C, p);
        part = p;
#define VIEWMAT_PART(DEG)                                                                                                  \
    hipLaunchKernelGGL(k_viewmat_bwd_part<DEG>, dim3(nb, C), dim3(256), 0, s, N, means, quats, scales, sh, sh_stride,          \
                       viewmats, Ks, campos, width, height, (const float4*)splats, (const float4*)v_splats, part)
        switch (gp.sh_active) {
            case 0: VIEWMAT_PART(0); break;
            case 2: VIEWMAT_PART(2); break;
            case 3: VIEWMAT_PART(3); break;
            default: VIEWMAT_PART(1); break;
        }
#undef VIEWMAT_PART
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_viewmat_bwd_finish, dim3(C), dim3(256), 0, s, nb, viewmats, (const double*)part, v_viewmats);
    LAUNCH_CHECK();
    return ST3R_OK;
}
