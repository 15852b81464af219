// Pose step: Adam on the cameras of a training call, on the device, and the fused training step that uses it
// (InstantSplat-style joint refinement: the cameras the alignment produced are good, not exact).
//
// Per camera, in double, with V = [R t; 0 1] and G = d loss / d V (st3r_gs_viewmat_bwd; row 3 of G is ignored: the
// bottom row of a rigid V is not varied).  Left perturbation V <- exp(xi^) V, xi = (omega, upsilon):
//     A = G[:3,:3] R^T
//     g_omega   = (A21 - A12, A02 - A20, A10 - A01) + t x G[:3,3]         g_upsilon = G[:3,3]
// Adam on the six scalars (torch's formulas, bias corrected by `step`):  delta = -lr mhat / (sqrt(vhat) + eps)
// Retraction:  E = Rodrigues(delta_omega),  R' = E R,  t' = E t + delta_upsilon,  Gram-Schmidt on the rows of R'
// (row 0 normalised, row 1 minus its projection then normalised, row 2 = row 0 x row 1),  campos' = -R'^T t'.
// V and campos are stored as float32, the bottom row as 0 0 0 1; the moments as float32.
//
// The work is ~300 double operations per camera: one thread per camera, one launch, nothing to reduce.  What matters
// is that it runs on the stream with no synchronisation, behind the same device-side guard as k_adam: a step that
// outgrew its buffers moves no camera either.  Guard, mask, moment update and launch are the per-view Adam of
// per_view.h, which k_exposure_adam shares; the tangent gradient and the retraction are this kernel's.
// Non-finite gradients are NOT filtered (torch's Adam does not filter them either): a NaN or Inf in G goes through the
// moments into V and campos of that camera, and stays.  The loss of such a step is non-finite too and says so.
#include "per_view.h"

__global__ __launch_bounds__(64) void k_pose_adam(int C, PerViewAdamK k, float* __restrict__ viewmats,
                                                  float* __restrict__ campos, const float* __restrict__ v_viewmats,
                                                  float* __restrict__ pose_m, float* __restrict__ pose_v) {
    const int c = per_view_adam_view(k, C);
    if (c < 0) return;   // (a frozen camera keeps V, campos, m and v bit for bit)
    float* V = viewmats + 16 * c;
    const float* Gf = v_viewmats + 16 * c;
    double R[9], t[3], GR[9], Gt[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) { R[i * 3 + j] = (double)V[4 * i + j]; GR[i * 3 + j] = (double)Gf[4 * i + j]; }
        t[i] = (double)V[4 * i + 3]; Gt[i] = (double)Gf[4 * i + 3];
    }
    // ---- tangent gradient
    double A[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            A[i * 3 + j] = (GR[i * 3] * R[j * 3] + GR[i * 3 + 1] * R[j * 3 + 1]) + GR[i * 3 + 2] * R[j * 3 + 2];
    double g[6];
    g[0] = (A[7] - A[5]) + (t[1] * Gt[2] - t[2] * Gt[1]);
    g[1] = (A[2] - A[6]) + (t[2] * Gt[0] - t[0] * Gt[2]);
    g[2] = (A[3] - A[1]) + (t[0] * Gt[1] - t[1] * Gt[0]);
    g[3] = Gt[0]; g[4] = Gt[1]; g[5] = Gt[2];
    // ---- Adam
    double d[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) d[q] = per_view_adam_delta<true>(k, pose_m[6 * c + q], g[q], pose_v[6 * c + q]);
    // ---- retraction: E = I + a K + b K^2,  K = [delta_omega]x,  K^2 = w w^T - |w|^2 I
    const double th2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    double a, b;
    if (th2 < 1e-16) {
        a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0;
    } else {
        const double th = sqrt(th2), hs = sin(0.5 * th) / (0.5 * th);
        a = sin(th) / th; b = 0.5 * hs * hs;   // (1 - cos th) / th^2 without the cancellation
    }
    double E[9];
    E[0] = 1.0 + b * (d[0] * d[0] - th2); E[1] = -a * d[2] + b * d[0] * d[1];  E[2] = a * d[1] + b * d[0] * d[2];
    E[3] = a * d[2] + b * d[0] * d[1];    E[4] = 1.0 + b * (d[1] * d[1] - th2); E[5] = -a * d[0] + b * d[1] * d[2];
    E[6] = -a * d[1] + b * d[0] * d[2];   E[7] = a * d[0] + b * d[1] * d[2];   E[8] = 1.0 + b * (d[2] * d[2] - th2);
    double Rn[9], tn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            Rn[i * 3 + j] = (E[i * 3] * R[j] + E[i * 3 + 1] * R[3 + j]) + E[i * 3 + 2] * R[6 + j];
        tn[i] = ((E[i * 3] * t[0] + E[i * 3 + 1] * t[1]) + E[i * 3 + 2] * t[2]) + d[3 + i];
    }
    // Gram-Schmidt on the rows: the float32 store of every step would otherwise let R drift off SO(3)
    const double n0 = 1.0 / sqrt((Rn[0] * Rn[0] + Rn[1] * Rn[1]) + Rn[2] * Rn[2]);
    Rn[0] *= n0; Rn[1] *= n0; Rn[2] *= n0;
    const double p01 = (Rn[3] * Rn[0] + Rn[4] * Rn[1]) + Rn[5] * Rn[2];
    Rn[3] -= p01 * Rn[0]; Rn[4] -= p01 * Rn[1]; Rn[5] -= p01 * Rn[2];
    const double n1 = 1.0 / sqrt((Rn[3] * Rn[3] + Rn[4] * Rn[4]) + Rn[5] * Rn[5]);
    Rn[3] *= n1; Rn[4] *= n1; Rn[5] *= n1;
    Rn[6] = Rn[1] * Rn[5] - Rn[2] * Rn[4];
    Rn[7] = Rn[2] * Rn[3] - Rn[0] * Rn[5];
    Rn[8] = Rn[0] * Rn[4] - Rn[1] * Rn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        V[4 * i] = (float)Rn[i * 3]; V[4 * i + 1] = (float)Rn[i * 3 + 1]; V[4 * i + 2] = (float)Rn[i * 3 + 2];
        V[4 * i + 3] = (float)tn[i];
        campos[3 * c + i] = (float)(-((Rn[i] * tn[0] + Rn[3 + i] * tn[1]) + Rn[6 + i] * tn[2]));
    }
    V[12] = 0.0f; V[13] = 0.0f; V[14] = 0.0f; V[15] = 1.0f;
}

ST3R_EXPORT int st3r_pose_adam_step(st3r_ctx* ctx, void* stream, int C, float* viewmats, float* campos,
                                    const float* v_viewmats, float* pose_m, float* pose_v, double lr, double beta1,
                                    double beta2, double eps, int step, const float* mask) {
    ARG_CHECK(ctx && C > 0 && step >= 1 && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0);
    ARG_CHECK(viewmats && campos && v_viewmats && pose_m && pose_v);
    return per_view_adam_launch(ctx, (hipStream_t)stream, k_pose_adam, C, lr, beta1, beta2, eps, step, mask, viewmats,
                                campos, v_viewmats, pose_m, pose_v);
}

// st3r_gs_train_step that also moves the cameras.  Order: forward, loss, blend backward; Gaussian gradients AND the
// per-camera pose gradient (both at the poses the call started with); Gaussian Adam; pose Adam.  No host round trip of
// its own: with stats_host == NULL the whole call is asynchronous in steady state, and a step that outgrew its buffers
// updates neither the Gaussians nor the cameras (the next call reports ST3R_ERR_CAPACITY: repeat the step).
ST3R_EXPORT int st3r_gs_train_step_poses(st3r_ctx* ctx, void* stream, int N, int C, float* means, float* quats,
                                         float* scales, float* opacities, float* sh, int sh_stride, float* viewmats,
                                         const float* Ks, float* campos, const float* gt_images, int width, int height,
                                         float ssim_fac, float opac_fac, float scale_fac, float* grads, float* m, float* v,
                                         double lr, double beta1, double beta2, double eps, int step, float* loss_out,
                                         int64_t* stats_host, float* pose_m, float* pose_v, double pose_lr, int pose_step,
                                         const float* pose_mask, float* v_viewmats_out) {
    ARG_CHECK(ctx && grads && m && v && step >= 1 && N > 0 && C > 0 && C <= ST3R_MAX_VIEWS);
    ARG_CHECK(pose_m && pose_v && pose_step >= 1 && viewmats && campos);
    ARG_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0);
    if (ctx->comm) {
        st3r_set_error("st3r_gs_train_step_poses: a communicator is attached -- view-sharded pose training is not "
                       "supported (every rank would have to move the cameras of the other ranks' views)");
        return ST3R_ERR_INVALID;
    }
    float* v_viewmats = v_viewmats_out;
    if (!v_viewmats) {
        ARENA_GET(SLOT_POSE_GRAD, float, 16 * (size_t)C, own);
        v_viewmats = own;
    }
    int rc = st3r_train_fwd_bwd_impl(ctx, (hipStream_t)stream, GsParams{N, means, quats, scales, opacities, sh, sh_stride},
                                     GsViews{C, width, height, viewmats, Ks, campos}, gt_images, ssim_fac, opac_fac,
                                     scale_fac, grads, loss_out, stats_host, v_viewmats);
    if (rc) return rc;
    rc = st3r_adam_step(ctx, stream, N, means, quats, scales, opacities, sh, sh_stride, grads, m, v, lr, beta1, beta2, eps,
                        step);
    if (rc) return rc;
    return per_view_adam_launch(ctx, (hipStream_t)stream, k_pose_adam, C, pose_lr, beta1, beta2, eps, pose_step, pose_mask,
                                viewmats, campos, v_viewmats, pose_m, pose_v);
}
