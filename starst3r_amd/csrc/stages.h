// Internal interface between the translation units of libst3r_hip.so: every function that is defined in one .hip file
// and called from another is declared here, once, and the defining file includes this header too -- a definition that
// drifts from its declaration is a compile error, not a link error.  (radix_sort.h does the same for the sort.)
// A launcher nobody outside its file calls is static there and has no line here.
#pragma once
#include "common.h"

// ---- argument bundles of the internal calls (the exported C functions keep their flat lists and fill these) ----
struct GsParams {   // the Gaussians: [N,3] [N,4] [N,3] [N] [N,sh_stride]
    int N;
    const float *means, *quats, *scales, *opacities, *sh;
    int sh_stride;
    // the SH setting of the call (st3r_sh_setting fills it from the context): SH_ROWS(sh_active) rows are evaluated, the
    // gradients of the rows 4 .. SH_ROWS(sh_degree) - 1 go to v_sh_high [N, 3 (SH_ROWS(sh_degree) - 4)]
    int sh_active = 1, sh_degree = 1;
    float* v_sh_high = nullptr;
};

// The context's SH setting (st3r_ctx_set_sh_degree) onto the Gaussians of a call that evaluates SH, with the two checks
// every such call makes: the rows are there, and a backward call at degree >= 2 has somewhere to write.
static inline int st3r_sh_setting(const st3r_ctx* ctx, GsParams* g, bool backward) {
    const int rows = (ctx->sh_degree + 1) * (ctx->sh_degree + 1);
    ARG_CHECK(g->sh_stride >= 3 * (rows < 4 ? 4 : rows));
    if (backward && ctx->sh_degree >= 2 && !ctx->sh_v_high) {
        st3r_set_error("the SH degree is %d and no v_sh_high is set -- a backward call needs it "
                       "(st3r_ctx_set_sh_degree(ctx, degree, active_degree, v_sh_high))", ctx->sh_degree);
        return ST3R_ERR_INVALID;
    }
    g->sh_active = ctx->sh_active; g->sh_degree = ctx->sh_degree; g->v_sh_high = ctx->sh_v_high;
    return ST3R_OK;
}

struct GsViews {   // C views of W x H pixels: [C,4,4] [C,3,3] [C,3]
    int C, W, H;
    const float *viewmats, *Ks, *campos;
    GsViews slice(int c0, int c1) const { return {c1 - c0, W, H, viewmats + 16 * c0, Ks + 9 * c0, campos + 3 * c0}; }
};

// What the front end of a fused call (project -> scan -> emit -> sort -> offsets, fused_step.hip) leaves for the blend
// kernels; the stand-alone blend entry points fill one from their arguments (cum / rects / rectbase they do not have
// stay NULL, tight 0).
struct RasterOut {
    int C, W, H, tile_w, tile_h;
    const float* splats; const int32_t *offsets, *flat, *cum; const uint64_t *rects, *rectbase;
    int tight;          // `cum` counts the tight rectangles of the fused emission (see k_blend_bwd)
    int64_t n_pairs;    // N * C
    // n_isects: the slot count (sum of the rectangle areas) = capacity of everything indexed by record or slot;
    // n_records: the records emitted (= n_isects on the synchronous path), -1 while the count stays on the device
    int64_t n_isects, n_records, n_isects_ref, n_visible;
};

// the lists of a stand-alone blend call (stage API): no rectangles, and a pair scan only for the backward
static inline RasterOut stage_lists(int C, int W, int H, int tile_w, int tile_h, const float* splats, const int32_t* offsets,
                                    const int32_t* flat, int64_t n_isects, const int32_t* cum = nullptr,
                                    int64_t n_pairs = 0) {
    return RasterOut{C, W, H, tile_w, tile_h, splats, offsets, flat, cum, nullptr, nullptr, 0, n_pairs, n_isects, n_isects,
                     n_isects, -1};
}

// a registered weighted per-pixel target of a set of views -- the depth prior (loss_depth.hip), the alpha targets
// (gs_alpha.hip): map, weight [C,H,W], norm [C] = n_c, fac of its loss term; map == NULL: none applies
struct WeightedTarget { const float* map; const float* weight; const double* norm; float fac; };

// the registered exposures of a set of views (gs_exposure.hip) and where their gradient goes; exposure == NULL: none applies
struct ExposureReg { const float* exposure; float* v_exposure; };

// the per-pixel loss weights of a set of views (loss.hip); weight == NULL: none apply.  weight [C,H,W]; norm: per view
// norm_stride doubles, of which the first two are sum_p w and sum_{p in I} w (clamped to >= 1 or not: the readers clamp);
// sums_stride: doubles per view of the loss kernel's accumulators
struct LossWeight { const float* weight = nullptr; const double* norm = nullptr; int norm_stride = 0; int sums_stride = 2; };

// the registered backgrounds [C,3] of a set of views (gs_alpha.hip); colors == NULL: none apply
struct Background { const float* colors; };

// What a training call's views have registered (st3r_ctx_set_*), resolved once per call (fused_step.hip:
// resolve_options); default-constructed: nothing applies.  dp_sums, at_sums [C]: the per-view sums sum_p w |ED - Z| and
// sum_p w |a - M| of the step; v_Ks [C,4]: the rows of the registered intrinsics gradient (gs_intrinsics.hip).
struct StepOptions {
    WeightedTarget dp{}; double* dp_sums = nullptr;   // depth prior
    ExposureReg ex{};
    LossWeight lw{};
    Background bg{};
    WeightedTarget at{}; double* at_sums = nullptr;   // alpha targets
    float* v_Ks = nullptr;
    // the options of the views from c0 on (HW pixels each): every per-view pointer moves by c0 whole views -- what
    // view_reg_first yields for those views' ground-truth pointer
    StepOptions slice(int c0, int64_t HW) const {
        StepOptions o = *this;
        const auto move = [c0](auto*& p, int64_t per_view) { if (p) p += c0 * per_view; };
        move(o.dp.map, HW); move(o.dp.weight, HW); move(o.dp.norm, 1); move(o.dp_sums, 1);
        move(o.ex.exposure, 12); move(o.ex.v_exposure, 12);
        move(o.lw.weight, HW); move(o.lw.norm, o.lw.norm_stride);
        move(o.bg.colors, 3);
        move(o.at.map, HW); move(o.at.weight, HW); move(o.at.norm, 1); move(o.at_sums, 1);
        move(o.v_Ks, 4);
        return o;
    }
};

// ---- api.hip, fused_step.hip, comm.hip ----
// The 16 device words next to the fused steps: [0] record count of an asynchronous step (k_adam compares it with the
// step's capacity), [4] status word of an exchanged step (comm.hip).  Zeroed when allocated.
int st3r_counts_buffer(st3r_ctx* ctx, hipStream_t s, int32_t** out);
int st3r_count_settle(st3r_ctx* ctx);
// st3r_gs_train_fwd_bwd, and with v_viewmats != NULL ([C,4,4]) the pose gradient of every view next to it
int st3r_train_fwd_bwd_impl(st3r_ctx* ctx, hipStream_t s, const GsParams& g, const GsViews& v, const float* gt_images,
                            float ssim_fac, float opac_fac, float scale_fac, float* grads, float* loss_out,
                            int64_t* stats_host, float* v_viewmats);
int st3r_peer_status_settle(st3r_ctx* ctx);

// ---- gs_project.hip, gs_project_bwd.hip ----
int st3r_project_impl(st3r_ctx* ctx, hipStream_t s, const GsParams& g, const GsViews& v, int tile_size, float eps2d,
                      float near_plane, float far_plane, float radius_clip, float* splats, int32_t* tiles_per_gauss,
                      double* reg_sums, uint64_t* depth_keys, int32_t* depth_vals, int tight, uint32_t key_base, void* rects,
                      int rect32, int reg_overwrite, double* zero_ptr, int zero_n, uint32_t* krange);
int st3r_project_sh_bwd_impl(hipStream_t s, const GsParams& g, const GsViews& v, float eps2d, const float* splats,
                             const float* v_splats, float reg_views, float opac_fac, float scale_fac, float* grads,
                             bool accumulate, int g_begin, int g_end, bool range_major, const st3r_vtile_ref* slots);

// ---- gs_isect.hip, gs_sort.hip ----
int st3r_isect_scan_impl(st3r_ctx* ctx, hipStream_t s, int64_t n_pairs, const int32_t* tiles, int32_t* cum,
                         int64_t* n_isects_host, const void* pack_rects, int rect32, uint64_t* pack_out,
                         int32_t** total_dev_out, int32_t* total_copy, int32_t* total_host);
// host-side decisions, shared with st3r_front_plan: tiles of the single-pass scan, the emission grid, the tiling constants
// (SCAN_TILE, EP, ECH, EMIT_SELF_BASE_MAX, keys per thread of k_isect_offsets32)
int st3r_scan_tiles(int64_t n);
void st3r_emit_grid(int N, int C, int* bpc, int* grid, int* self_base);
void st3r_isect_constants(int64_t out[5]);
// band_tile > 0: the banded emission (records split by the high byte of their key) and, in *band_table, the band starts and
// sort tiles for st3r_radix_sort_u32_banded (radix_sort.h): two arrays of ST3R_BAND_TAB words (gs_isect.hip: k_band_table); tile_keys == NULL
// (banded only, N * C <= 2^24): the packed form, vals = pair id | low key byte << 24 (st3r_radix_sort_u32_banded_packed)
int st3r_isect_emit_chain_impl(st3r_ctx* ctx, hipStream_t s, int N, int C, const int32_t* perm, const void* rects,
                               int rect32, int tile_w, int tile_h, uint32_t* tile_keys, int32_t* vals, int64_t cap,
                               int band_tile, const int32_t* n_dev, const uint32_t** band_table);
int st3r_records_prepare_impl(hipStream_t s, int N, int C, const float* splats, int tile_size, int tile_w, int tile_h,
                              int tight, int32_t* tiles, uint64_t* depth_keys, int32_t* depth_vals, uint32_t key_base,
                              void* rects, int rect32);
int st3r_isect_offsets32_impl(hipStream_t s, int64_t n_isects, const uint32_t* keys, int C, int tile_w, int tile_h,
                              int32_t* offsets, const int32_t* n_dev);
int st3r_sort_tile_end_bit(int end_bit);
int st3r_sort_tile_impl(st3r_ctx* ctx, hipStream_t s, int64_t n, int end_bit, uint32_t* keys_in, int32_t* vals_in,
                        uint32_t* keys_out, int32_t* vals_out, const int32_t* n_dev);
// the banded tile sort (keys of 9 .. 16 bits, unless debug flag 16 asks for the two passes): does it apply?  (Its sort tile
// and its one low-byte pass over the banded stream: radix_sort.h.)
int st3r_sort_tile_banded(int end_bit, int debug_flags);

// ---- gs_blend.hip, gs_blend_cells.hip, gs_blend_depth.hip ----
// end_in_offsets (fused calls): ro.offsets has C * tiles + 1 entries and the last one closes the last tile -- the record
// count may then live on the device, ro.n_isects being a capacity
int st3r_blend_fwd_impl(st3r_ctx* ctx, hipStream_t s, const RasterOut& ro, float* rgb, float* alpha, int32_t* last_ids,
                        bool for_backward, bool end_in_offsets);
int st3r_blend_fwd_cells_impl(st3r_ctx* ctx, hipStream_t s, const RasterOut& ro, float* rgb, float* alpha,
                              int32_t* last_ids, uint64_t* cmask, int64_t cmask_words, int32_t* tile_nb);
int st3r_blend_bwd_impl(st3r_ctx* ctx, hipStream_t s, const RasterOut& ro, const float* alpha, const int32_t* last_ids,
                        const float* v_rgb, const float* v_alpha, float* v_splats, bool end_in_offsets,
                        st3r_vtile_ref* defer);
int st3r_gather_vtile_impl(hipStream_t s, int64_t n_pairs, const st3r_vtile_ref* slots, float* v_splats);
int st3r_blend_depth_fwd_impl(st3r_ctx* ctx, hipStream_t s, const RasterOut& ro, const int32_t* last_ids, float* depth,
                              bool end_in_offsets);
int st3r_blend_depth_bwd_impl(st3r_ctx* ctx, hipStream_t s, const RasterOut& ro, const float* alpha,
                              const int32_t* last_ids, const float* v_depth, float* v_splats, bool end_in_offsets);
int st3r_add_pairs_impl(hipStream_t s, int64_t n_pairs, float* a, const float* b);

// ---- loss.hip, loss_depth.hip ----
int st3r_loss_impl(st3r_ctx* ctx, hipStream_t s, int C, int H, int W, const float* render, const float* gt,
                   float w_l1, float w_ssim, double* sums, float* v_render, bool sums_cleared, const LossWeight& lw);
int st3r_loss_weight_for(st3r_ctx* ctx, hipStream_t s, const float* gt, int C, int H, int W, LossWeight* out);
// the sums of a weight map that normalise either loss (k_weight_sums, per_view.h), and those of a registration
int st3r_weight_norms(st3r_ctx* ctx, hipStream_t s, int C, int H, int W, const float* weight, double* out, int stride,
                      int at_least_one, bool interior, int slot);
int st3r_registered_weight_norms(st3r_ctx* ctx, hipStream_t s, const ViewReg& reg, const float* weight, int at_least_one,
                                 bool interior, int part_slot, int norm_slot, int* valid, const double** norms);
int st3r_depth_prior_loss_impl(st3r_ctx* ctx, hipStream_t s, int C, int H, int W, const float* depth, const float* alpha,
                               const float* prior, const float* weight, const double* norm, int norm_stride,
                               float depth_fac, double* sums, int sums_stride, float* v_depth, float* v_alpha);

// ---- gs_exposure.hip ----
void st3r_exposure_for(st3r_ctx* ctx, const float* gt, int C, int H, int W, ExposureReg* out);
int st3r_exposure_fwd_impl(hipStream_t s, int C, int H, int W, const float* rgb, const float* exposure, float* out);
int st3r_exposure_bwd_impl(st3r_ctx* ctx, hipStream_t s, int C, int H, int W, const float* rgb, const float* exposure,
                           const float* v_out, float* v_rgb, float* v_exposure);

// ---- gs_alpha.hip ----
void st3r_background_for(st3r_ctx* ctx, const float* gt, int C, int H, int W, Background* out);
int st3r_composite_fwd_impl(hipStream_t s, int C, int H, int W, const float* rgb, const float* alpha,
                            const float* backgrounds, float* out);
int st3r_alpha_grad_impl(st3r_ctx* ctx, hipStream_t s, int C, int H, int W, const float* alpha, const float* backgrounds,
                         const float* v_out, const float* target, const float* weight, const double* norm, int norm_stride,
                         float alpha_fac, const float* v_alpha_in, double* sums, int sums_stride, float* v_alpha,
                         float* v_backgrounds);

// ---- gs_activation.hip ----
// S = exp(scales), O = sigmoid(opacities); reg_sums != NULL: double[2] = sum O, sum S of the stored values
int st3r_param_activate_impl(st3r_ctx* ctx, hipStream_t s, int N, const float* scales, const float* opacities,
                             float* act_scales, float* act_opacities, double* reg_sums);
// v_s = (v_S + reg_s_k) S, v_o = (v_O + reg_o_k) O (1 - O); the outputs may be v_act_scales / v_act_opacities
int st3r_param_activate_bwd_impl(hipStream_t s, int N, const float* act_scales, const float* act_opacities,
                                 const float* v_act_scales, const float* v_act_opacities, float reg_s_k, float reg_o_k,
                                 float* v_scales, float* v_opacities);
// *out = g with its scales and opacities replaced by their activated copies in the ctx's scratch
int st3r_activated_params(st3r_ctx* ctx, hipStream_t s, const GsParams& g, double* reg_sums, GsParams* out);

// ---- gs_intrinsics.hip ----
// the rows of the registered intrinsics gradient [C,4] of the C views at `gt`; NULL: none applies
float* st3r_intrinsics_grad_for(st3r_ctx* ctx, const float* gt, int C, int H, int W);

// ---- adam.hip ----
// i0 < 0: the whole buffer.  [g0, g1) a proper sub-range of the Gaussians: that range instead of [i0, i1).
int st3r_adam_impl(hipStream_t s, int N, float* means, float* quats, float* scales, float* opacities, float* sh,
                   int sh_stride, const float* grads, float* m, float* v, double lr, double b1, double b2,
                   double eps, int step, const int32_t* count_dev, uint32_t count_cap, const int32_t* status_dev, int64_t i0,
                   int64_t i1, int64_t g0, int64_t g1, float* pstage, const float* gstage, float* grads_out);
int st3r_params_from_stage_impl(hipStream_t s, int N, float* means, float* quats, float* scales, float* opacities,
                                float* sh, int sh_stride, const float* pstage, int64_t i0, int64_t i1, int64_t lim,
                                const int32_t* count_dev, uint32_t count_cap, const int32_t* status_dev);
int st3r_params_from_peers_impl(hipStream_t s, int N, float* means, float* quats, float* scales, float* opacities,
                                float* sh, int sh_stride, const float* const* tab, int r, int64_t q, int64_t lim,
                                const int32_t* status_dev);
// the device-side guard of an asynchronous step that is still in flight (see k_adam)
void st3r_adam_guard(st3r_ctx* ctx, const int32_t** count_dev, uint32_t* count_cap);
