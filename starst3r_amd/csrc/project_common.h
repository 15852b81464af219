// What gs_project.hip, gs_project_bwd.hip and gs_pose_bwd.hip share: the SH constants, the layout of the per-camera
// block, the conic part of the pair chain rule and SH of the degrees other than 1.  (The fixed-order block sum of
// doubles that gs_pose_bwd.hip has in common with gs_blend_depth.hip is per_view.h's.)
#pragma once
#include <hip/hip_runtime.h>

#define SH_C0 0.2820947917738781f
#define SH_C1 0.48860251190292f

// per-camera block of CAM_STRIDE floats (C blocks of dynamic LDS in k_project_sh_fwd and k_project_sh_bwd):
//   [0..11] view matrix rows 0..2 (R|t), 12 fx, 13 fy, 14 cx, 15 cy,
//   16 lim_x_pos, 17 lim_x_neg, 18 lim_y_pos, 19 lim_y_neg, 20..22 camera position
#define CAM_STRIDE 32

struct Sym3 { float xx, xy, xz, yy, yz, zz; };   // symmetric 3x3: 00 01 02 11 12 22

// The conic part of the pair chain rule, for k_project_sh_bwd and k_viewmat_bwd_part.  In: the pair's record (r0.w r1.x
// r1.y: the conic, which already holds eps2d), its gradient (g0.w g1.x g1.y), the projection Jacobian
// J = [[a, 0, cj], [0, b, d]] and the camera-space covariance S.  Out: vS = J^T G J, the gradient of S, and the four
// entries of v_J = 2 G J S that are not zero.  Everything goes through references and the body is straight-line: in that
// form hipcc leaves k_project_sh_bwd as it is, instruction for instruction ("What the projection kernels
// share").
__device__ __forceinline__ void conic_chain(const float4& r0, const float4& r1, const float4& g0, const float4& g1,
                                            const float& a, const float& cj, const float& b, const float& d,
                                            const Sym3& S, Sym3& vS, float& vJ00, float& vJ02, float& vJ11,
                                            float& vJ12) {
    // conic -> cov2d
    const float A = r0.w, B = r1.x, Cc = r1.y;
    const float vA = g0.w, vB = 0.5f * g1.x, vC = g1.y;
    const float X00 = A * vA + B * vB, X01 = A * vB + B * vC;
    const float X10 = B * vA + Cc * vB, X11 = B * vB + Cc * vC;
    const float G00 = -(X00 * A + X01 * B);
    const float G01 = -0.5f * ((X00 * B + X01 * Cc) + (X10 * A + X11 * B));
    const float G11 = -(X10 * B + X11 * Cc);
    // GJ = G * J
    const float GJ00 = G00 * a, GJ01 = G01 * b, GJ02 = G00 * cj + G01 * d;
    const float GJ10 = G01 * a, GJ11 = G11 * b, GJ12 = G01 * cj + G11 * d;
    vS.xx = a * GJ00; vS.xy = a * GJ01; vS.xz = a * GJ02;
    vS.yy = b * GJ11; vS.yz = b * GJ12; vS.zz = cj * GJ02 + d * GJ12;
    vJ00 = 2.0f * (GJ00 * S.xx + GJ01 * S.xy + GJ02 * S.xz);
    vJ02 = 2.0f * (GJ00 * S.xz + GJ01 * S.yz + GJ02 * S.zz);
    vJ11 = 2.0f * (GJ10 * S.xy + GJ11 * S.yy + GJ12 * S.yz);
    vJ12 = 2.0f * (GJ10 * S.xz + GJ11 * S.yz + GJ12 * S.zz);
}

// ---- SH of degree 0..3 (st3r_ctx_set_sh_degree) ----
// The three kernels are templates on the degree in use.  Their degree-1 instantiation keeps the text it always had (the
// setting's default launches it, and hipcc leaves it instruction for instruction as it was: DESIGN.md, "Spherical
// harmonics of degree 0 to 3"); every other degree goes through the functions below.
#define SH_MAX_DEGREE 3
#define SH_ROWS(deg) (((deg) + 1) * ((deg) + 1))
#define SH_C2_0 1.0925484305920792f
#define SH_C2_1 -1.0925484305920792f
#define SH_C2_2 0.31539156525252005f
#define SH_C2_3 -1.0925484305920792f
#define SH_C2_4 0.5462742152960396f
#define SH_C3_0 -0.5900435899266435f
#define SH_C3_1 2.890611442640554f
#define SH_C3_2 -0.4570457994644658f
#define SH_C3_3 0.3731763325901154f
#define SH_C3_4 -0.4570457994644658f
#define SH_C3_5 1.445305721320277f
#define SH_C3_6 -0.5900435899266435f

// b[i], i >= 4: basis function i (with its constant) at the unit direction (x, y, z).  Rows 0..3 are written out where
// they are used, in the degree-1 kernels' own association.
template <int DEG>
__device__ __forceinline__ void sh_basis_high(const float& x, const float& y, const float& z, float (&b)[16]) {
    const float xx = x * x, yy = y * y, zz = z * z;
    if constexpr (DEG >= 2) {
        b[4] = SH_C2_0 * (x * y);
        b[5] = SH_C2_1 * (y * z);
        b[6] = SH_C2_2 * ((2.0f * zz - xx) - yy);
        b[7] = SH_C2_3 * (x * z);
        b[8] = SH_C2_4 * (xx - yy);
    }
    if constexpr (DEG >= 3) {
        b[9] = SH_C3_0 * (y * (3.0f * xx - yy));
        b[10] = SH_C3_1 * ((x * y) * z);
        b[11] = SH_C3_2 * (y * ((4.0f * zz - xx) - yy));
        b[12] = SH_C3_3 * (z * ((2.0f * zz - 3.0f * xx) - 3.0f * yy));
        b[13] = SH_C3_4 * (x * ((4.0f * zz - xx) - yy));
        b[14] = SH_C3_5 * (z * (xx - yy));
        b[15] = SH_C3_6 * (x * (xx - 3.0f * yy));
    }
}

// The pre-clamp colour of channel ch: sum over the bands in use + 0.5.  k: the Gaussian's 3 SH_ROWS(DEG) coefficients.
// Each band is summed on its own and added to the bands below it, so a Gaussian whose higher rows are zero gets the
// bits of the lower degree (under -ffp-contract=off, as k_project_sh_fwd is compiled).
template <int DEG>
__device__ __forceinline__ float sh_pre_clamp(const float* k, const int ch, const float& x, const float& y, const float& z,
                                              const float (&b)[16]) {
    float r = SH_C0 * k[ch];
    if constexpr (DEG >= 1) r = r + SH_C1 * ((-y * k[3 + ch] + z * k[6 + ch]) - x * k[9 + ch]);
    if constexpr (DEG >= 2) {
        float s = b[4] * k[12 + ch];
#pragma unroll
        for (int i = 5; i < 9; ++i) s = s + b[i] * k[3 * i + ch];
        r = r + s;
    }
    if constexpr (DEG >= 3) {
        float s = b[9] * k[27 + ch];
#pragma unroll
        for (int i = 10; i < 16; ++i) s = s + b[i] * k[3 * i + ch];
        r = r + s;
    }
    return r + 0.5f;
}

// The chain rule of one pair's colour.  vcol: the colour gradient; colf: the stored (clamped) colour.  The clamp's
// pass-through is decided on the full pre-clamp value.  v_k (WANT_K): the coefficient gradients, 3 SH_ROWS(DEG) sums in
// the caller's registers.  (vx, vy, vz): the gradient of the unit direction, each basis function differentiated as a
// polynomial in three free variables -- the caller projects it onto the sphere's tangent, as the degree-1 text does.
template <int DEG, bool WANT_K>
__device__ __forceinline__ void sh_chain(const float* k, const float (&vcol)[3], const float (&colf)[3], const float& x,
                                         const float& y, const float& z, float* v_k, float& vx, float& vy, float& vz) {
    constexpr int K = SH_ROWS(DEG);
    float b[16];
    sh_basis_high<DEG>(x, y, z, b);
    b[0] = SH_C0; b[1] = -SH_C1 * y; b[2] = SH_C1 * z; b[3] = -SH_C1 * x;
    float vc[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float pre = sh_pre_clamp<DEG>(k, ch, x, y, z, b);
        vc[ch] = (colf[ch] > 0.0f || pre >= 0.0f) ? vcol[ch] : 0.0f;
    }
    float t[16];   // t[i] = sum over the channels of k[i][ch] vc[ch]: d colour . vcol / d b[i]
#pragma unroll
    for (int i = 0; i < K; ++i) {
        if (WANT_K) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) v_k[3 * i + ch] += b[i] * vc[ch];
        }
        t[i] = (k[3 * i] * vc[0] + k[3 * i + 1] * vc[1]) + k[3 * i + 2] * vc[2];
    }
    vx = 0.f; vy = 0.f; vz = 0.f;
    if constexpr (DEG >= 1) { vx = -SH_C1 * t[3]; vy = -SH_C1 * t[1]; vz = SH_C1 * t[2]; }
    if constexpr (DEG >= 2) {
        vx += SH_C2_0 * y * t[4] + SH_C2_2 * (-2.0f * x) * t[6] + SH_C2_3 * z * t[7] + SH_C2_4 * (2.0f * x) * t[8];
        vy += SH_C2_0 * x * t[4] + SH_C2_1 * z * t[5] + SH_C2_2 * (-2.0f * y) * t[6] + SH_C2_4 * (-2.0f * y) * t[8];
        vz += SH_C2_1 * y * t[5] + SH_C2_2 * (4.0f * z) * t[6] + SH_C2_3 * x * t[7];
    }
    if constexpr (DEG >= 3) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z;
        vx += SH_C3_0 * (6.0f * xy) * t[9] + SH_C3_1 * yz * t[10] + SH_C3_2 * (-2.0f * xy) * t[11] +
              SH_C3_3 * (-6.0f * xz) * t[12] + SH_C3_4 * ((4.0f * zz - 3.0f * xx) - yy) * t[13] +
              SH_C3_5 * (2.0f * xz) * t[14] + SH_C3_6 * (3.0f * xx - 3.0f * yy) * t[15];
        vy += SH_C3_0 * (3.0f * xx - 3.0f * yy) * t[9] + SH_C3_1 * xz * t[10] +
              SH_C3_2 * ((4.0f * zz - xx) - 3.0f * yy) * t[11] + SH_C3_3 * (-6.0f * yz) * t[12] +
              SH_C3_4 * (-2.0f * xy) * t[13] + SH_C3_5 * (-2.0f * yz) * t[14] + SH_C3_6 * (-6.0f * xy) * t[15];
        vz += SH_C3_1 * xy * t[10] + SH_C3_2 * (8.0f * yz) * t[11] + SH_C3_3 * ((6.0f * zz - 3.0f * xx) - 3.0f * yy) * t[12] +
              SH_C3_4 * (8.0f * xz) * t[13] + SH_C3_5 * (xx - yy) * t[14];
    }
}
