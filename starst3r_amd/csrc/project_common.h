// What gs_project.hip, gs_project_bwd.hip and gs_pose_bwd.hip share: the SH constants, the layout of the per-camera
// block and the conic part of the pair chain rule.  (The fixed-order block sum of doubles that gs_pose_bwd.hip has in
// common with gs_blend_depth.hip is per_view.h's.)
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
