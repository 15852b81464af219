// The fused train / render steps: they chain the stage kernels on one stream using only ctx scratch.
//   rasterize_front          project -> scan -> emit -> sort -> offsets
//   train_views              one set of views: forward, losses, backward; st3r_train_fwd_bwd_impl walks the view chunks
//   st3r_gs_raster_train     the middle phase of the Gaussian-sharded mode
//   st3r_gs_render           forward only
#include "radix_sort.h"
#include "stages.h"

// The previous asynchronous step left its record count in pinned memory behind an event: pick it up (it completed long
// ago), remember it as the sizing hint, and fail loudly if that step ran out of capacity (its records past the
// capacity were dropped, so its gradients were incomplete).
int st3r_count_settle(st3r_ctx* ctx) {
    if (!ctx->count_pending) return ST3R_OK;
    HIP_TRY(hipEventSynchronize(ctx->count_event));
    ctx->count_pending = 0;
    const int64_t n = (int64_t)((int32_t*)(ctx->pinned + 8))[0];
    if (n < 0) {
        ctx->isect_hint = 0;
        ctx->view_chunks = (ctx->view_chunks > 0 ? ctx->view_chunks : 1) * 2;
        st3r_set_error("the previous step produced more than 2^31 tile intersections: its gradients were incomplete -- "
                       "repeat it (st3r_gs_train_fwd_bwd / st3r_gs_train_step now walk the views in %d chunks)",
                       ctx->view_chunks);
        return ST3R_ERR_CAPACITY;
    }
    if (n > ctx->count_cap) {
        ctx->isect_hint = 0;   // the next call takes the synchronous path and sizes its buffers exactly
        st3r_set_error("the previous step produced %lld tile intersections, more than the %lld its buffers were sized "
                       "for from the step before (+25 %%): its gradients were incomplete and st3r_adam_step / "
                       "st3r_gs_train_step did NOT apply them (the update is guarded on the device) -- repeat that step",
                       (long long)n, (long long)ctx->count_cap);
        return ST3R_ERR_CAPACITY;
    }
    ctx->isect_hint = n;
    return ST3R_OK;
}

// What rasterize_front decides on the host from the shape of a call alone (the sorts', the scan's and the emission's own
// shapes come from the functions that launch them).  with_reg: the projection's reduction is at hand (training calls);
// records: the splat records come from the caller (st3r_gs_raster_train).
struct FrontPlan {
    int tile_w, tile_h;
    bool key32;       // level-1 keys: one 32-bit word (camera | depth code above the near plane's) -- else 64-bit
    bool segments;    // level-1 sort per camera segment on biased keys, pass count from the device
    int rect32;       // 32-bit packed rectangles -- else 64-bit
    bool rectbase;    // slot base | 10-bit rectangle per pair for the blend backward
    uint32_t key_base;
    int l1_end_bit;   // bits of the level-1 key sorted when the sort is not segmented: depth code (29 / 32) + camera bits
    int end_bit;      // bits of the (camera, tile) key
};
static const float k_near_plane = 0.01f, k_far_plane = 1e10f;
static FrontPlan front_plan(int C, int W, int H, int debug_flags, bool with_reg, bool records) {
    FrontPlan p;
    const int tile = 16;
    p.tile_w = (W + tile - 1) / tile; p.tile_h = (H + tile - 1) / tile;
    // Level-1 keys.  Up to 8 local views: one 32-bit word, camera (3 bits) | depth bits minus those of the near plane
    // (the reference's near = 0.01 and far = 1e10 span < 2^29 float codes) -- the same order as (camera | depth) at
    // 8 instead of 12 bytes per pair and one radix pass less.  More views: 64-bit (camera << 32 | depth bits).
    uint32_t near_bits, far_bits;
    memcpy(&near_bits, &k_near_plane, 4); memcpy(&far_bits, &k_far_plane, 4);
    p.key32 = (C <= 8) && (far_bits - near_bits < 0x1FFFFFFFu);
    p.key_base = p.key32 ? near_bits : 0u;
    // packed tile rectangle of every pair (pair-id order; the tile count of a pair is the area of its rectangle, no
    // array of its own): 32-bit entries for tile grids up to 255 x 255 (tile_rect.h), 64-bit beyond -- and under debug
    // flag 64, whose backward reads the 64-bit form
    p.rect32 = (p.tile_w <= 255 && p.tile_h <= 255 && !(debug_flags & 64)) ? 1 : 0;
    // Round 6: with the projection's own reduction at hand (training calls) the level-1 sort runs per camera SEGMENT on keys
    // biased by the smallest depth code of the call -- three 8-bit passes instead of four whenever the scene's depth codes
    // span less than 2^24 (decided on the device: counts[8..10] = bias, sentinel, passes); debug flag 4 keeps the
    // (camera | depth) keys and their four passes
    p.segments = p.key32 && with_reg && !records && !(debug_flags & 4);
    p.l1_end_bit = (p.key32 ? 29 : 32) + bit_length_u32((uint32_t)(C - 1));
    p.rectbase = p.tile_w <= 1023 && p.tile_h <= 1023 && !(debug_flags & 64);   // 10-bit rectangle fields
    p.end_bit = bit_length_u32((uint32_t)((int64_t)C * p.tile_w * p.tile_h - 1));
    return p;
}

// project -> scan -> emit -> sort -> offsets, all in ctx scratch
static int rasterize_front(st3r_ctx* ctx, hipStream_t s, const GsParams& g, const GsViews& v, double* reg_sums, int tight,
                           const float* records_in, bool allow_async, RasterOut* o, double* loss_sums = nullptr) {
    // reg_sums is OVERWRITTEN with the projection's sums, and loss_sums[0 .. 2C) (the loss kernel's accumulators, when
    // given) is cleared along the way -- by the projection's reduction launch, not by memsets of their own
    // records_in != NULL: the splat records were projected elsewhere (Gaussian-sharded mode); the projection is
    // replaced by k_records_prepare and the records are used in place (g's and v's pointers are not looked at)
    const int N = g.N, C = v.C, W = v.W, H = v.H;
    const int tile = 16;
    const FrontPlan fp = front_plan(C, W, H, ctx->debug_flags, reg_sums != nullptr, records_in != nullptr);
    const int tile_w = fp.tile_w, tile_h = fp.tile_h;
    const int64_t n_pairs = (int64_t)N * C;
    float* splats = const_cast<float*>(records_in);
    if (!records_in) {
        ARENA_GET(SLOT_SPLATS, float, n_pairs * ST3R_SPLAT_STRIDE, own);
        splats = own;
    }
    ARENA_GET(SLOT_CUM, int32_t, n_pairs, cum);
    ARENA_GET(SLOT_OFFSETS, int32_t, (int64_t)C * tile_w * tile_h + 1, offsets);   // + the total (closes the last tile)
    // Two-level sort (see gs_isect.hip): pairs by (camera | depth) first, then the emitted records by
    // their 32-bit (camera, tile) key with a stable sort -- the same final order as gsplat's single
    // 64-bit (camera | tile | depth) sort at roughly a quarter of the sort traffic.  (The forms of the level-1 keys, of the
    // packed rectangles and of the level-1 sort: front_plan.)
    const float near_plane = k_near_plane, far_plane = k_far_plane;
    const bool key32 = fp.key32;
    ARENA_GET(SLOT_DKEYS_A, uint64_t, n_pairs, dkeys_a);
    ARENA_GET(SLOT_DKEYS_B, uint64_t, n_pairs, dkeys_b);
    ARENA_GET(SLOT_DVALS_A, int32_t, n_pairs, dvals_a);
    ARENA_GET(SLOT_DVALS_B, int32_t, n_pairs, perm);
    const int rect32 = fp.rect32;
    ARENA_GET(SLOT_RECTS, uint64_t, rect32 ? (n_pairs + 1) / 2 : n_pairs, rects);
    int32_t* counts = nullptr;
    { int rc_ = st3r_counts_buffer(ctx, s, &counts); if (rc_) return rc_; }
    uint32_t* const krange = fp.segments ? (uint32_t*)(counts + 8) : nullptr;   // counts[8..10] = bias, sentinel, passes
    st3r_prof_begin(ctx, s, STG_PROJECT);
    const uint32_t key_base = fp.key_base;
    int rc = records_in
                 ? st3r_records_prepare_impl(s, N, C, splats, tile, tile_w, tile_h, tight, nullptr, dkeys_a, dvals_a,
                                             key_base, rects, rect32)
                 : st3r_project_impl(ctx, s, g, v, tile, 0.3f, near_plane, far_plane, 0.0f, splats, nullptr, reg_sums,
                                     dkeys_a, dvals_a, tight, key_base, rects, rect32, 1, loss_sums, 2 * C, krange);
    if (!rc && records_in && loss_sums) HIP_TRY(hipMemsetAsync(loss_sums, 0, sizeof(double) * 2 * (size_t)C, s));
    st3r_prof_end(ctx, s, STG_PROJECT);
    if (rc) return rc;
    st3r_prof_begin(ctx, s, STG_SORT_DEPTH);
    // (segments: the keys WITHOUT the camera bits, one segment of N pairs per camera, biased and sorted in as many 8-bit
    // passes as the depth range of the call needs -- radix_sort.hip: SEG)
    rc = krange ? st3r_radix_sort_u32_segments(ctx, s, N, C, (uint32_t*)dkeys_a, dvals_a, (uint32_t*)dkeys_b, perm, krange)
         : key32 ? st3r_radix_sort_u32(ctx, s, n_pairs, 0, fp.l1_end_bit, (uint32_t*)dkeys_a, dvals_a, (uint32_t*)dkeys_b, perm, nullptr)
                 : st3r_radix_sort_u64(ctx, s, n_pairs, 0, fp.l1_end_bit, dkeys_a, dvals_a, dkeys_b, perm);
    st3r_prof_end(ctx, s, STG_SORT_DEPTH);
    if (rc) return rc;
    int64_t n_isects = 0;
    st3r_prof_begin(ctx, s, STG_SCAN);
    // pair-id order scan: slot base of every pair for the backward pass's per-(record, tile) partials
    // (the same launch leaves slot base | rectangle as one word per pair for the backward's staging)
    uint64_t* rectbase = nullptr;
    if (fp.rectbase) {
        ARENA_GET(SLOT_RECTBASE, uint64_t, n_pairs, rb);
        rectbase = rb;
    }
    // (its total is the record count; the emit kernel finds the write positions of the depth-ordered records itself)
    // The record count is produced on the device.  Steady state (allow_async and a count from an earlier call): no host
    // round trip -- the buffers are sized from the previous count (+25 %, +1024), every kernel downstream reads the count
    // from device memory (the scan's last workgroup leaves it in the ctx's count word as well), and the count travels to
    // pinned memory behind an event that the NEXT call checks (it also notices, loudly, if this call's count exceeded its
    // capacity).  Otherwise (first call, or the caller wants exact statistics back): copy + synchronise, as in round 1.
    const int64_t sig = ((int64_t)N << 34) ^ ((int64_t)C << 26) ^ ((int64_t)W << 13) ^ (int64_t)H;
    const bool async = allow_async && ctx->isect_hint > 0 && ctx->hint_sig == sig;
    int32_t* total_dev = nullptr;
    rc = st3r_isect_scan_impl(ctx, s, n_pairs, nullptr, cum, nullptr, rects, rect32, rectbase, &total_dev,
                              async ? counts : nullptr, async ? (int32_t*)(ctx->pinned + 8) : nullptr);
    st3r_prof_end(ctx, s, STG_SCAN);
    if (rc) return rc;
    if (async) {
        // (the scan's last workgroup has stored the count into the pinned word itself)
        if (!ctx->count_event) HIP_TRY(hipEventCreateWithFlags(&ctx->count_event, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ctx->count_event, s));
        n_isects = ctx->isect_hint + ctx->isect_hint / 4 + 1024;   // capacity, not the count
        if (ctx->debug_flags & 8) n_isects = ctx->isect_hint / 2;   // test hook: provoke a capacity overflow
        if (n_isects > 2147483647LL) n_isects = 2147483647LL;
        ctx->count_pending = 1; ctx->count_cap = n_isects;
        o->n_visible = -1; o->n_isects_ref = -1;
    } else {
        HIP_TRY(hipMemcpyAsync(ctx->pinned, total_dev, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (reg_sums) HIP_TRY(hipMemcpyAsync(ctx->pinned + 1, reg_sums + 2, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        n_isects = (int64_t)((int32_t*)ctx->pinned)[0];
        if (n_isects < 0) {   // the tile counts are summed in int32
            st3r_set_error("more than 2^31 tile intersections in one call: split the views over more calls / GPUs");
            return ST3R_SPLIT_VIEWS;   // st3r_gs_train_fwd_bwd retries with the views in chunks; others report invalid
        }
        o->n_visible = reg_sums ? (int64_t)((double*)ctx->pinned)[1] : -1;
        o->n_isects_ref = reg_sums ? (int64_t)((double*)ctx->pinned)[2] : n_isects;
        if (allow_async) { ctx->isect_hint = n_isects; ctx->hint_sig = sig; }
    }
    ARENA_GET(SLOT_KEYS_A, uint32_t, n_isects, tkeys_a);
    ARENA_GET(SLOT_KEYS_B, uint32_t, n_isects, tkeys_b);
    ARENA_GET(SLOT_VALS_A, int32_t, n_isects, vals_a);
    ARENA_GET(SLOT_VALS_B, int32_t, n_isects, vals_b);
    // the sort and the offsets read the record count from device memory in both paths: the pair-order scan's total
    o->n_records = async ? -1 : n_isects;
    const int64_t n_keys = (int64_t)C * tile_w * tile_h;
    const uint32_t* band_table = nullptr;
    const uint32_t* band_hist = nullptr;   // packed tile sort: the records of every (band, low key byte)
    int n_bands = 0;
    if (n_isects > 0) {
        // Keys of 9 .. 16 bits: the emission writes the records split by the high byte of their key (the "band"), in
        // (camera, depth) order inside every band, and ONE stable pass on the low byte inside every band is left of the
        // tile sort -- the same (camera, tile, depth) order as the two passes (debug flag 16), bit for bit.
        const int end_bit = fp.end_bit;
        const bool banded = st3r_sort_tile_banded(end_bit, ctx->debug_flags) != 0;
        // Packed form of the banded sort (pair ids below 2^24; debug flag 1024 keeps the two arrays): behind the banded
        // emission a record's position fixes its band, the high key byte, so the emission writes ONE word per record,
        // pair id | low key byte << 24, into vals_a, the pass sorts that word keys-only and stores the bare pair ids, and
        // the offsets come from the band table and the band histograms.  tkeys_a / tkeys_b are not written.
        const bool packed = banded && n_pairs <= (1 << 24) && !(ctx->debug_flags & 1024);
        n_bands = (int)((n_keys - 1) >> 8) + 1;
        st3r_prof_begin(ctx, s, STG_EMIT);
        rc = st3r_isect_emit_chain_impl(ctx, s, N, C, perm, rects, rect32, tile_w, tile_h, packed ? nullptr : tkeys_a, vals_a,
                                        n_isects, banded ? st3r_radix_sort_band_tile(n_isects) : 0, total_dev, &band_table);
        st3r_prof_end(ctx, s, STG_EMIT);
        if (rc) return rc;
        st3r_prof_begin(ctx, s, STG_SORT);
        rc = packed ? st3r_radix_sort_u32_banded_packed(ctx, s, n_isects, n_bands, band_table, (const uint32_t*)vals_a, vals_b,
                                                        &band_hist)
             : banded ? st3r_radix_sort_u32_banded(ctx, s, n_isects, n_bands, band_table, tkeys_a, vals_a, tkeys_b, vals_b)
                      : st3r_sort_tile_impl(ctx, s, n_isects, end_bit, tkeys_a, vals_a, tkeys_b, vals_b, total_dev);
        st3r_prof_end(ctx, s, STG_SORT);
        if (rc) return rc;
    }
    st3r_prof_begin(ctx, s, STG_OFFSETS);
    rc = band_hist ? st3r_radix_band_offsets(s, n_bands, band_table, band_hist, n_keys, offsets)
                   : st3r_isect_offsets32_impl(s, n_isects, tkeys_b, C, tile_w, tile_h, offsets, total_dev);
    st3r_prof_end(ctx, s, STG_OFFSETS);
    if (rc) return rc;
    o->C = C; o->W = W; o->H = H; o->tile_w = tile_w; o->tile_h = tile_h;
    o->splats = splats; o->offsets = offsets; o->flat = vals_b; o->cum = cum; o->rects = rect32 ? nullptr : rects;
    o->rectbase = rectbase;
    o->tight = tight; o->n_pairs = n_pairs;
    o->n_isects = n_isects;
    return ST3R_OK;
}

// one weighted-target term of the loss (depth prior, alpha targets): fac sum_c sums[c] / norm[c]; sums == NULL: none
struct TargetTerm { const double* sums; const double* norm; double fac; };

__global__ void k_finalize_loss(int C, const double* __restrict__ sums, const double* __restrict__ reg_sums,
                                double inv_px, double inv_cnt, double w_l1, double w_ssim, double reg_views,
                                double opac_k, double scale_k, float* __restrict__ loss_out,
                                const double* __restrict__ wnorm, TargetTerm depth, TargetTerm alpha) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double loss = 0;
        if (wnorm)   // per-pixel weights (loss.hip): wnorm[2c], wnorm[2c + 1] = sum_p w, sum_{p in I} w of view c
            for (int c = 0; c < C; ++c)
                loss += w_l1 * sums[2 * c] / (3.0 * fmax(wnorm[2 * c], 1.0)) +
                        w_ssim * (3.0 * wnorm[2 * c + 1] - sums[2 * c + 1]) / (3.0 * fmax(wnorm[2 * c + 1], 1.0));
        else
            for (int c = 0; c < C; ++c) loss += w_l1 * sums[2 * c] * inv_px + w_ssim * (1.0 - sums[2 * c + 1] * inv_cnt);
        loss += reg_views * (opac_k * reg_sums[0] + scale_k * reg_sums[1]);
        if (depth.sums)   // depth prior (loss_depth.hip): depth_fac sum_p w |ED - Z| / n_c per view
            for (int c = 0; c < C; ++c) loss += depth.fac * depth.sums[c] / depth.norm[c];
        if (alpha.sums)   // alpha targets (gs_alpha.hip): alpha_fac sum_p w |a - M| / n_c per view
            for (int c = 0; c < C; ++c) loss += alpha.fac * alpha.sums[c] / alpha.norm[c];
        loss_out[0] = (float)loss;
    }
}

// the per-view sums of a step -> its loss; o: the depth and alpha terms, and the weighted loss, normalised by the sums of
// the views' weights
static int finalize_loss(hipStream_t s, int C, int H, int W, const double* sums, const double* reg_sums, float ssim_fac,
                         double reg_views, double opac_k, double scale_k, float* loss_out, const StepOptions& o) {
    const int Hi = H - 10, Wi = W - 10;
    const double cnt = (Hi > 0 && Wi > 0) ? (double)Hi * Wi * 3 : 0.0;
    hipLaunchKernelGGL(k_finalize_loss, dim3(1), dim3(64), 0, s, C, sums, reg_sums, 1.0 / ((double)H * W * 3),
                       cnt > 0 ? 1.0 / cnt : 0.0, (double)(1.0f - ssim_fac), (double)ssim_fac, reg_views, opac_k, scale_k,
                       loss_out, o.lw.norm, TargetTerm{o.dp_sums, o.dp.norm, (double)o.dp.fac},
                       TargetTerm{o.at_sums, o.at.norm, (double)o.at.fac});
    LAUNCH_CHECK();
    return ST3R_OK;
}

struct LossFacs { float ssim, opac, scale; };

// A set of views with what a training call compares them against, what is registered for them and where their per-view
// results go: the whole call, or one view chunk of it.  v_viewmats may be NULL (no pose gradient wanted).
struct ViewBatch {
    GsViews v;
    const float* gt;      // [C,H,W,3]
    double* sums;         // [C,2]: L1 and SSIM sums
    float* v_viewmats;    // [C,4,4]
    StepOptions opt;
    ViewBatch slice(int c0, int c1) const {
        return {v.slice(c0, c1), gt + (int64_t)c0 * v.H * v.W * 3, sums + 2 * c0,
                v_viewmats ? v_viewmats + 16 * c0 : nullptr, opt.slice(c0, (int64_t)v.H * v.W)};
    }
};

// the images of a step, in ctx scratch (depth, v_depth: with a depth prior only; v_alpha: with a depth prior, backgrounds
// or alpha targets; exposed: with exposures only; composite: with backgrounds only)
struct StepImages { float *rgb, *alpha; int32_t* last; float *v_rgb, *depth, *v_depth, *v_alpha, *exposed, *composite; };

static int step_images(st3r_ctx* ctx, const RasterOut& ro, const StepOptions& o, StepImages* im) {
    const int64_t n_px = (int64_t)ro.C * ro.H * ro.W;
    ARENA_GET(SLOT_RGB, float, n_px * 3, rgb);
    ARENA_GET(SLOT_ALPHA, float, n_px, alpha);
    ARENA_GET(SLOT_LAST, int32_t, n_px, last);
    ARENA_GET(SLOT_VRENDER, float, n_px * 3, v_rgb);
    *im = StepImages{rgb, alpha, last, v_rgb, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (o.ex.exposure) {
        ARENA_GET(SLOT_EXPOSED, float, n_px * 3, exposed);
        im->exposed = exposed;
    }
    if (o.bg.colors) {
        ARENA_GET(SLOT_COMPOSITE, float, n_px * 3, composite);
        im->composite = composite;
    }
    if (o.dp.map) {
        ARENA_GET(SLOT_DEPTH, float, n_px, depth);
        ARENA_GET(SLOT_VDEPTH, float, n_px, v_depth);
        im->depth = depth; im->v_depth = v_depth;
    }
    if (o.dp.map || o.bg.colors || o.at.map) {
        ARENA_GET(SLOT_VALPHA, float, n_px, v_alpha);
        im->v_alpha = v_alpha;
    }
    return ST3R_OK;
}

// Blend forward and the losses of the views in b: their sums go to b.sums (and b.opt.dp_sums, b.opt.at_sums), d loss /
// d image to im.  Of b.opt:
static int forward_and_losses(st3r_ctx* ctx, hipStream_t s, const RasterOut& ro, const ViewBatch& b, float ssim_fac,
                              bool sums_cleared, const StepImages& im) {
    const WeightedTarget &dp = b.opt.dp, &at = b.opt.at;
    const ExposureReg& ex = b.opt.ex;
    const LossWeight& lw = b.opt.lw;
    const Background& bg = b.opt.bg;
    // dp.map != NULL: the step also renders the depth map of the same lists and takes the prior's loss, which sends v_D
    // and v_alpha back
    // bg.colors != NULL: the loss sees the render composited over the views' backgrounds (st3r_composite_fwd, into scratch
    // of its own, before the exposure: scene first, then camera); at.map != NULL: the alpha term.  Either one sends a
    // v_alpha back (st3r_alpha_grad, behind the depth prior, onto whose v_alpha it accumulates)
    // ex.exposure != NULL: the loss compares y = E x with the ground truth (the stand-alone kernels of gs_exposure.hip, in
    // the order of the unfused chain); im.v_rgb leaves as d loss / d x, ex.v_exposure as d loss / d E of these views
    // lw.weight != NULL: the photometric loss takes the views' per-pixel weights (on y with exposures, whose backward then
    // sees the weighted d loss / d y)
    const bool eio = true;   // the fused path's offsets table carries the total as its last entry
    st3r_prof_begin(ctx, s, STG_BLEND_FWD);
    int rc = st3r_blend_fwd_impl(ctx, s, ro, im.rgb, im.alpha, im.last, true, eio);
    if (!rc && dp.map) rc = st3r_blend_depth_fwd_impl(ctx, s, ro, im.last, im.depth, eio);
    st3r_prof_end(ctx, s, STG_BLEND_FWD);
    if (rc) return rc;
    st3r_prof_begin(ctx, s, STG_LOSS);
    const float* x = im.rgb;   // what the camera sees: the render, or the render over its background
    if (bg.colors) {
        rc = st3r_composite_fwd_impl(s, ro.C, ro.H, ro.W, im.rgb, im.alpha, bg.colors, im.composite);
        x = im.composite;
    }
    if (!rc && ex.exposure) rc = st3r_exposure_fwd_impl(s, ro.C, ro.H, ro.W, x, ex.exposure, im.exposed);
    if (!rc)
        rc = st3r_loss_impl(ctx, s, ro.C, ro.H, ro.W, ex.exposure ? im.exposed : x, b.gt, 1.0f - ssim_fac, ssim_fac,
                            b.sums, im.v_rgb, sums_cleared, lw);
    if (!rc && ex.exposure)
        rc = st3r_exposure_bwd_impl(ctx, s, ro.C, ro.H, ro.W, x, ex.exposure, im.v_rgb, im.v_rgb, ex.v_exposure);
    if (!rc && dp.map)
        rc = st3r_depth_prior_loss_impl(ctx, s, ro.C, ro.H, ro.W, im.depth, im.alpha, dp.map, dp.weight, dp.norm, 1, dp.fac,
                                        b.opt.dp_sums, 1, im.v_depth, im.v_alpha);
    if (!rc && (bg.colors || at.map))   // im.v_rgb is d loss / d composite here, and d loss / d render as it stands
        rc = st3r_alpha_grad_impl(ctx, s, ro.C, ro.H, ro.W, im.alpha, bg.colors, bg.colors ? im.v_rgb : nullptr, at.map,
                                  at.weight, at.norm, 1, at.fac, dp.map ? im.v_alpha : nullptr, b.opt.at_sums, 1, im.v_alpha,
                                  nullptr);
    st3r_prof_end(ctx, s, STG_LOSS);
    return rc;
}

// Blend backward of a training step.  The colour backward leaves its stamped (record, tile) slots in *slots (Round 5: the
// projection backward sums them per pair itself -- no 48-byte per-pair records, no k_gather_vtile launch).
// need_pairs (depth prior): the colour backward also receives v_alpha, the depth backward writes slots of its own, and
// both per-pair arrays are materialised by the stand-alone gathers (k_gather_vtile<9>, k_gather_vtile<7>) and added in
// v_pairs -- the kernels and the order of the unfused chain (render_3dgs "RGB+ED" through autograd).
static int blend_backward(st3r_ctx* ctx, hipStream_t s, const RasterOut& ro, const StepImages& im, bool need_pairs,
                          st3r_vtile_ref* slots, float* v_pairs) {
    RasterOut rb = ro;
    if (ctx->debug_flags & 2) { rb.rects = nullptr; rb.rectbase = nullptr; }   // the backward recomputes the rectangles
    const bool eio = true;
    st3r_prof_begin(ctx, s, STG_BLEND_BWD);
    int rc = st3r_blend_bwd_impl(ctx, s, rb, im.alpha, im.last, im.v_rgb, im.v_alpha, nullptr, eio, slots);
    if (!rc && need_pairs) {
        ARENA_GET(SLOT_VSPLATS_D, float, ro.n_pairs * ST3R_SPLAT_STRIDE, v_pairs_d);
        rc = st3r_blend_depth_bwd_impl(ctx, s, rb, im.alpha, im.last, im.v_depth, v_pairs_d, eio);
        if (!rc) {
            if (slots->vtile) rc = st3r_gather_vtile_impl(s, ro.n_pairs, slots, v_pairs);
            else HIP_TRY(hipMemsetAsync(v_pairs, 0, sizeof(float) * ST3R_SPLAT_STRIDE * (size_t)ro.n_pairs, s));   // no records
        }
        if (!rc) rc = st3r_add_pairs_impl(s, ro.n_pairs, v_pairs, v_pairs_d);
    }
    st3r_prof_end(ctx, s, STG_BLEND_BWD);
    return rc;
}

// Projection backward: the per-pair gradients come from v_pairs, or (v_pairs == NULL) are summed from the slots.
// Range-wise exchange (st3r_gs_train_step, comm.hip): one launch per Gaussian range with an event behind each, so that
// a range's gradients can be reduced while the next range is still being computed.
static int project_backward(st3r_ctx* ctx, hipStream_t s, const GsParams& g, const GsViews& v, const RasterOut& ro,
                            const LossFacs& f, const float* v_pairs, const st3r_vtile_ref* slots, bool accumulate,
                            float* grads) {
    ctx->ranges_recorded = 0;
    if (!(ctx->n_ranges > 1 && ctx->comm_stream))
        return st3r_project_sh_bwd_impl(s, g, v, 0.3f, ro.splats, v_pairs, (float)v.C, f.opac, f.scale, grads, accumulate, 0,
                                        -1, false, slots);
    // the gradients of a range go to the ctx's staging buffer in range-major order (one contiguous piece per range);
    // Adam reads them from there and leaves them in the caller's buffer in its block layout (comm.hip).  The later
    // view chunks of a chunked call ADD to the staged gradients and record the range events again (the exchange waits
    // for an event's LAST record): whether a rank walks its views in chunks or not, it stages every range and takes
    // part in the same K collectives (round 3 sent the first chunk to the staging buffer and the others to the
    // caller's buffer, and fell back to one all-reduce on that rank only)
    ARENA_GET(SLOT_GSTAGE, float, (int64_t)23 * g.N, gstage);
    const int K = ctx->n_ranges;
    for (int j = 0; j < K; ++j) {
        const int g0 = (int)((int64_t)g.N * j / K), g1 = (int)((int64_t)g.N * (j + 1) / K);
        int rc = st3r_project_sh_bwd_impl(s, g, v, 0.3f, ro.splats, v_pairs, (float)v.C, f.opac, f.scale, gstage, accumulate,
                                          g0, g1, true, slots);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(ctx->ev_range_bwd[j], s));
    }
    ctx->ranges_recorded = K;
    return ST3R_OK;
}

// the stand-alone pose backward on the per-pair gradients, unchanged: the fused pose gradient is the unfused one
static int pose_backward(st3r_ctx* ctx, hipStream_t s, const GsParams& g, const GsViews& v, const RasterOut& ro,
                         const float* v_pairs, float* v_viewmats) {
    return st3r_gs_viewmat_bwd(ctx, s, g.N, v.C, g.means, g.quats, g.scales, g.sh, g.sh_stride, v.viewmats, v.Ks, v.campos,
                               v.W, v.H, 0.3f, ro.splats, v_pairs, v_viewmats);
}

// The views of b in one training call: rasterize -> loss -> backward; the parameter gradients are written
// (accumulate = false) or added (later view chunks of the same call).  b.opt: what is registered for these views.
// b.v_viewmats != NULL (st3r_gs_train_step_poses): the gradient of these views' world-to-camera matrices is written as well.
static int train_views(st3r_ctx* ctx, hipStream_t s, const GsParams& g, const ViewBatch& b, const LossFacs& f,
                       double* reg_sums, bool allow_async, bool accumulate, float* grads, RasterOut* ro_out) {
    const GsViews& v = b.v;
    // The one decision: with a depth prior the projection backward reads the per-pair array v_pairs (colour + depth
    // gradients, added), without one it sums the colour backward's slots itself (backgrounds and alpha targets hand the
    // colour backward a v_alpha as the depth prior does; its slots then carry the alpha path, and need_pairs stays false).
    const bool need_pairs = b.opt.dp.map != nullptr;
    RasterOut& ro = *ro_out;
    int rc = rasterize_front(ctx, s, g, v, reg_sums, 1, nullptr, allow_async, &ro, b.sums);
    if (rc) return rc;
    StepImages im;
    rc = step_images(ctx, ro, b.opt, &im);
    if (rc) return rc;
    // an intrinsics gradient registered for these views (st3r_ctx_set_intrinsics_grad): it needs the per-pair array as
    // the pose gradient does
    float* const v_Ks = b.opt.v_Ks;
    float* v_pairs = nullptr;   // per-pair gradients [N*C, 12]: the projection backward's input and / or the pose backward's
    if (need_pairs || b.v_viewmats || v_Ks) {
        ARENA_GET(SLOT_VSPLATS, float, ro.n_pairs * ST3R_SPLAT_STRIDE, vp);
        v_pairs = vp;
    }
    rc = forward_and_losses(ctx, s, ro, b, f.ssim, true, im);
    if (rc) return rc;
    st3r_vtile_ref slots{};
    rc = blend_backward(ctx, s, ro, im, need_pairs, &slots, v_pairs);
    if (rc) return rc;
    st3r_prof_begin(ctx, s, STG_PROJECT_BWD);
    rc = project_backward(ctx, s, g, v, ro, f, need_pairs ? v_pairs : nullptr, need_pairs ? nullptr : &slots, accumulate,
                          grads);
    // depth prior, inside the timing bracket: the pose gradient of the summed per-pair gradients first, then the float-9
    // column into the means block and into row 2 of v_viewmats -- the order of _Rasterize.backward
    if (!rc && need_pairs && b.v_viewmats) rc = pose_backward(ctx, s, g, v, ro, v_pairs, b.v_viewmats);
    if (!rc && need_pairs) rc = st3r_gs_depth_bwd(ctx, s, g.N, v.C, g.means, v.viewmats, ro.splats, v_pairs, grads, b.v_viewmats);
    st3r_prof_end(ctx, s, STG_PROJECT_BWD);
    // poses without a depth prior, two launches BEHIND the ones of a call without poses: k_gather_vtile materialises the
    // per-pair sums of the slots (the projection backward above summed the same slots itself and is left as it is)
    if (!rc && !need_pairs && (b.v_viewmats || v_Ks)) {
        rc = st3r_gather_vtile_impl(s, ro.n_pairs, &slots, v_pairs);
        if (!rc && b.v_viewmats) rc = pose_backward(ctx, s, g, v, ro, v_pairs, b.v_viewmats);
    }
    // the stand-alone intrinsics backward on the same per-pair gradients (with a depth prior: the summed ones), behind
    // everything a call without the registration launches
    if (!rc && v_Ks)
        rc = st3r_gs_intrinsics_bwd(ctx, s, g.N, v.C, g.means, g.quats, g.scales, v.viewmats, v.Ks, v.W, v.H, 0.3f,
                                    ro.splats, v_pairs, v_Ks);
    return rc;
}

// More than 2^31 tile intersections in one call (the counts are int32): the views are walked in chunks, each a
// complete rasterize -> loss -> backward whose parameter gradients add up (the loss is a sum over views,
// starster/gs.py:149-152); a view belongs to one chunk, which writes that view's sums and pose gradient.  *chunks is
// doubled until every chunk fits.  stats: visible pairs, records, reference intersections, summed over the chunks.
static int train_chunks(st3r_ctx* ctx, hipStream_t s, const GsParams& g, const ViewBatch& all, const LossFacs& f,
                        double* reg_sums, double* reg_scratch, bool want_stats, float* grads, int* chunks, int64_t stats[3]) {
    const int C = all.v.C;
    for (;;) {
        int rc = ST3R_OK;
        stats[0] = stats[1] = stats[2] = 0;
        bool first = true;
        for (int k = 0; k < *chunks && !rc; ++k) {
            const int c0 = (int)((int64_t)k * C / *chunks), c1 = (int)((int64_t)(k + 1) * C / *chunks);
            if (c1 == c0) continue;
            RasterOut ro;
            // exact statistics need the count on the host: a caller that passes stats_host pays the synchronisation;
            // chunked calls size every chunk exactly (the hint of the steady state belongs to one set of views); with a
            // communicator attached every step is sized exactly too -- a capacity overflow would surface on ONE rank only,
            // at its next call, while the other ranks are already waiting in the gradient all-reduce
            // (reg_scratch: the regulariser sums of the later chunks are repeats)
            rc = train_views(ctx, s, g, all.slice(c0, c1), f, first ? reg_sums : reg_scratch,
                             !want_stats && *chunks == 1 && !ctx->comm, !first, grads, &ro);
            if (!rc) { stats[0] += ro.n_visible; stats[1] += ro.n_records; stats[2] += ro.n_isects_ref; }
            first = false;
        }
        if (rc == ST3R_SPLIT_VIEWS && *chunks < C) {
            *chunks = *chunks * 2 < C ? *chunks * 2 : C;
            continue;
        }
        return rc == ST3R_SPLIT_VIEWS ? ST3R_ERR_INVALID : rc;   // a single view above 2^31 (message set where it was found)
    }
}

// The registered weighted target r (ctx->dp or ctx->at, with its two arena slots) that belongs to the C views at `gt`:
// out->map = NULL if there is none (no registration that applies -- view_reg_first -- or a factor of 0).
static int weighted_target_for(st3r_ctx* ctx, hipStream_t s, TargetReg* r, int part_slot, int norm_slot, const float* gt,
                               int C, int H, int W, WeightedTarget* out) {
    *out = WeightedTarget{};
    const int64_t c0 = view_reg_first(r->reg, gt, C, H, W), HW = (int64_t)H * W;
    if (c0 < 0 || r->fac == 0.f) return ST3R_OK;
    const double* n_c;
    int rc = st3r_registered_weight_norms(ctx, s, r->reg, r->weight, 1, false, part_slot, norm_slot, &r->norm_valid, &n_c);
    if (rc) return rc;
    *out = WeightedTarget{r->map + c0 * HW, r->weight + c0 * HW, n_c + c0, r->fac};
    return ST3R_OK;
}

// Everything registered for the C views at `gt`, each option looked up once, in this order: it is the order of the
// once-per-registration norm launches (st3r_registered_weight_norms).  The view chunks of the call slice the result.
static int resolve_options(st3r_ctx* ctx, hipStream_t s, const float* gt, int C, int H, int W, StepOptions* o) {
    *o = StepOptions{};
    int rc = weighted_target_for(ctx, s, &ctx->dp, SLOT_DPRIOR_PART, SLOT_DPRIOR_NORM, gt, C, H, W, &o->dp);
    if (rc) return rc;
    st3r_exposure_for(ctx, gt, C, H, W, &o->ex);
    o->v_Ks = st3r_intrinsics_grad_for(ctx, gt, C, H, W);
    rc = st3r_loss_weight_for(ctx, s, gt, C, H, W, &o->lw);
    if (rc) return rc;
    st3r_background_for(ctx, gt, C, H, W, &o->bg);
    rc = weighted_target_for(ctx, s, &ctx->at, SLOT_ATARGET_PART, SLOT_ATARGET_NORM, gt, C, H, W, &o->at);
    if (rc) return rc;
    if (o->dp.map) {
        ARENA_GET(SLOT_DPRIOR_SUMS, double, (size_t)C, sums);
        o->dp_sums = sums;
    }
    if (o->at.map) {
        ARENA_GET(SLOT_ATARGET_SUMS, double, (size_t)C, sums);
        o->at_sums = sums;
    }
    return ST3R_OK;
}

int st3r_train_fwd_bwd_impl(st3r_ctx* ctx, hipStream_t s, const GsParams& g, const GsViews& v, const float* gt_images,
                            float ssim_fac, float opac_fac, float scale_fac, float* grads, float* loss_out,
                            int64_t* stats_host, float* v_viewmats) {
    const int N = g.N, C = v.C;
    ARG_CHECK(ctx && N > 0 && C > 0 && C <= ST3R_MAX_VIEWS && v.W > 0 && v.H > 0 && g.sh_stride >= 12);
    ARG_CHECK((int64_t)N * C < 2147483647LL);   // pair ids, tile counts and their scans are int32
    ARG_CHECK(g.means && g.quats && g.scales && g.opacities && g.sh && v.viewmats && v.Ks && v.campos && gt_images && grads &&
              loss_out);
    ARENA_GET(SLOT_SMALL, double, 2 * (size_t)C + 12, small);
    double* sums = small;              // [C,2]
    double* reg_sums = small + 2 * C;  // [4]: sum sigmoid(o), sum exp(s), visible pairs, reference intersections
    StepOptions opt;
    int rc = resolve_options(ctx, s, gt_images, C, v.H, v.W, &opt);
    if (rc) return rc;
    const bool activated = ctx->activation != 0;   // activated parameters (st3r_ctx_set_activation)
    if (ctx->comm) {   // view-sharded training takes none of the options: refuse before anything of the caller's is written
        const struct { bool applies; const char *what, *clear; } refused[] = {
            {opt.dp.map != nullptr, "a depth prior is registered", "st3r_ctx_set_depth_prior(ctx, NULL, ...)"},
            {opt.ex.exposure != nullptr, "exposures are registered", "st3r_ctx_set_exposure(ctx, NULL, ...)"},
            {opt.v_Ks != nullptr, "an intrinsics gradient is registered", "st3r_ctx_set_intrinsics_grad(ctx, NULL, ...)"},
            {opt.lw.weight != nullptr, "loss weights are registered", "st3r_ctx_set_loss_weight(ctx, NULL, ...)"},
            {opt.bg.colors != nullptr, "backgrounds are registered", "st3r_ctx_set_background(ctx, NULL, ...)"},
            {opt.at.map != nullptr, "alpha targets are registered", "st3r_ctx_set_alpha_target(ctx, NULL, ...)"},
            {!(ctx->sh_degree == 1 && ctx->sh_active == 1), "an SH degree other than 1 is set",
             "st3r_ctx_set_sh_degree(ctx, 1, 1, NULL)"},
            {activated, "the activation is on", "st3r_ctx_set_activation(ctx, 0)"},
        };
        for (const auto& r : refused)
            if (r.applies) {
                st3r_set_error("%s and a communicator is attached -- view-sharded training does not support it (clear it "
                               "with %s)", r.what, r.clear);
                return ST3R_ERR_INVALID;
            }
    }
    GsParams gsh = g;
    rc = st3r_sh_setting(ctx, &gsh, true);
    if (rc) return rc;
    st3r_prof_next_step(ctx);
    rc = st3r_count_settle(ctx);
    if (rc) return rc;
    // Activated: the step below runs on exp(scales) and sigmoid(opacities), copies in scratch rebuilt by every call, with
    // both regulariser factors 0 -- every kernel sees activated geometry, unchanged.  The sums the projection still
    // leaves in reg_sums[0..1] are then of the wrong tensors and are not used: the activation's own two, next to
    // reg_sums, take their place in the loss.
    GsParams ga = gsh;
    double* const act_sums = small + 2 * C + 8;   // [2]: sum sigmoid(o), sum exp(s)
    if (activated) {
        rc = st3r_activated_params(ctx, s, gsh, act_sums, &ga);
        if (rc) return rc;
    }
    // the chunk count sticks to the context; debug flag 32 starts at two chunks (tests)
    int chunks = ctx->view_chunks > 0 ? ctx->view_chunks : 1;
    if ((ctx->debug_flags & 32) && chunks < 2) chunks = 2;
    if (chunks > C) chunks = C;
    int64_t stats[3];
    rc = train_chunks(ctx, s, ga, ViewBatch{v, gt_images, sums, v_viewmats, opt},
                      activated ? LossFacs{ssim_fac, 0.f, 0.f} : LossFacs{ssim_fac, opac_fac, scale_fac},
                      reg_sums, reg_sums + 4, stats_host != nullptr, grads, &chunks, stats);
    if (rc) return rc;
    if (chunks > 1) ctx->view_chunks = chunks;
    if (activated) {
        // the chain rule, once, behind the last view chunk, in place on the scales and opacities blocks of grads (block
        // layout: means 3N, quats 4N, scales 3N, opacities N, sh); the regularisers' gradient rides along, its constants
        // formed as the projection backward forms them
        const float reg_o_k = (float)C * opac_fac / (float)N, reg_s_k = (float)C * scale_fac / (3.0f * (float)N);
        float* const v_s = grads + 7 * (size_t)N;
        float* const v_o = grads + 10 * (size_t)N;
        rc = st3r_param_activate_bwd_impl(s, N, ga.scales, ga.opacities, v_s, v_o, reg_s_k, reg_o_k, v_s, v_o);
        if (rc) return rc;
    }
    rc = finalize_loss(s, C, v.H, v.W, sums, activated ? act_sums : reg_sums, ssim_fac, (double)C, (double)opac_fac / N,
                       (double)scale_fac / (3.0 * N), loss_out, opt);
    if (rc) return rc;
    if (stats_host) {
        stats_host[0] = stats[0]; stats_host[1] = stats[1]; stats_host[2] = st3r_ctx_arena_bytes(ctx);
        stats_host[3] = stats[2];   // exact: stats_host selects the synchronous path
    }
    return ST3R_OK;
}

ST3R_EXPORT int st3r_gs_train_fwd_bwd(st3r_ctx* ctx, void* stream, int N, int C, const float* means,
                                      const float* quats, const float* scales, const float* opacities,
                                      const float* sh, int sh_stride, const float* viewmats, const float* Ks,
                                      const float* campos, const float* gt_images, int width, int height,
                                      float ssim_fac, float opac_fac, float scale_fac, float* grads,
                                      float* loss_out, int64_t* stats_host) {
    return st3r_train_fwd_bwd_impl(ctx, (hipStream_t)stream, GsParams{N, means, quats, scales, opacities, sh, sh_stride},
                                   GsViews{C, width, height, viewmats, Ks, campos}, gt_images, ssim_fac, opac_fac,
                                   scale_fac, grads, loss_out, stats_host, nullptr);
}

// Gaussian-sharded multi-GPU mode, middle phase: this rank owns C views and received the splat records of ALL
// Gaussians for them (projected by the ranks that own the Gaussians).  Sort, blend, loss, blend backward; the
// per-record gradients go back to the owners, which run the projection backward and Adam on their shard.
ST3R_EXPORT int st3r_gs_raster_train(st3r_ctx* ctx, void* stream, int N, int C, const float* records,
                                     const float* gt_images, int width, int height, float ssim_fac,
                                     float* v_records, float* loss_out, int64_t* stats_host) {
    ARG_CHECK(ctx && N > 0 && C > 0 && width > 0 && height > 0 && records && gt_images && v_records && loss_out);
    ARG_CHECK(C <= ST3R_MAX_VIEWS && (int64_t)N * C < 2147483647LL);
    hipStream_t s = (hipStream_t)stream;
    ARENA_GET(SLOT_SMALL, double, 2 * (size_t)C + 8, sums);
    double* reg_sums = sums + 2 * C;
    const ViewBatch b{GsViews{C, width, height}, gt_images, sums, nullptr, StepOptions{}};   // (no camera is looked at, no option)
    HIP_TRY(hipMemsetAsync(reg_sums, 0, sizeof(double) * 4, s));  // stays zero: the regularisers belong to the owners
    st3r_prof_next_step(ctx);
    RasterOut ro;
    int rc = st3r_count_settle(ctx);
    if (rc) return rc;
    rc = rasterize_front(ctx, s, GsParams{N}, b.v, nullptr, 1, records, stats_host == nullptr, &ro);
    if (rc == ST3R_SPLIT_VIEWS) rc = ST3R_ERR_INVALID;
    if (rc) return rc;
    StepImages im;
    rc = step_images(ctx, ro, b.opt, &im);
    if (rc) return rc;
    rc = forward_and_losses(ctx, s, ro, b, ssim_fac, false, im);
    if (rc) return rc;
    st3r_prof_begin(ctx, s, STG_BLEND_BWD);
    rc = st3r_blend_bwd_impl(ctx, s, ro, im.alpha, im.last, im.v_rgb, nullptr, v_records, true, nullptr);
    st3r_prof_end(ctx, s, STG_BLEND_BWD);
    if (rc) return rc;
    rc = finalize_loss(s, C, height, width, sums, reg_sums, ssim_fac, 0.0, 0.0, 0.0, loss_out, b.opt);
    if (rc) return rc;
    if (stats_host) {
        stats_host[0] = -1; stats_host[1] = ro.n_records; stats_host[2] = st3r_ctx_arena_bytes(ctx); stats_host[3] = -1;
    }
    return ST3R_OK;
}

ST3R_EXPORT int st3r_gs_render(st3r_ctx* ctx, void* stream, int N, int C, const float* means, const float* quats,
                               const float* scales, const float* opacities, const float* sh, int sh_stride,
                               const float* viewmats, const float* Ks, const float* campos, int width, int height,
                               float* rgb, float* alpha, int64_t* stats_host) {
    ARG_CHECK(ctx && N > 0 && C > 0 && width > 0 && height > 0 && sh_stride >= 12);
    // the projection kernel keeps C * 128 B of camera constants in LDS; pair ids are int32
    ARG_CHECK(C <= ST3R_MAX_VIEWS && (int64_t)N * C < 2147483647LL);
    ARG_CHECK(means && quats && scales && opacities && sh && viewmats && Ks && campos && rgb && alpha);
    hipStream_t s = (hipStream_t)stream;
    RasterOut ro;
    int rc = st3r_count_settle(ctx);
    if (rc) return rc;
    GsParams g{N, means, quats, scales, opacities, sh, sh_stride};
    rc = st3r_sh_setting(ctx, &g, false);
    if (rc) return rc;
    if (ctx->activation) {   // log-scales and logits (st3r_ctx_set_activation): render their activated copies
        rc = st3r_activated_params(ctx, s, g, nullptr, &g);
        if (rc) return rc;
    }
    rc = rasterize_front(ctx, s, g,
                         GsViews{C, width, height, viewmats, Ks, campos}, nullptr, 0, nullptr, false, &ro);
    if (rc == ST3R_SPLIT_VIEWS) rc = ST3R_ERR_INVALID;
    if (rc) return rc;
    ARENA_GET(SLOT_LAST, int32_t, (int64_t)C * height * width, last);
    rc = st3r_blend_fwd_impl(ctx, s, ro, rgb, alpha, last, false, true);
    if (rc) return rc;
    if (stats_host) {
        stats_host[0] = -1; stats_host[1] = ro.n_records; stats_host[2] = st3r_ctx_arena_bytes(ctx); stats_host[3] = 0;
    }
    return ST3R_OK;
}

// The host-side decisions of the front end for a call of this shape, read back for the tests (no context, no GPU): every
// entry comes from the function that takes the decision when the call runs -- front_plan, st3r_scan_tiles, st3r_emit_grid,
// st3r_radix_sort_shape, st3r_sort_tile_end_bit -- so a retuned constant or a moved threshold changes what this reports.
ST3R_EXPORT int st3r_front_plan(int N, int C, int width, int height, int debug_flags, int training, int records,
                                int64_t n_records, int64_t* out, int n_out) {
    ARG_CHECK(N > 0 && C > 0 && C <= ST3R_MAX_VIEWS && width > 0 && height > 0 && n_records >= 0 && out &&
              n_out >= ST3R_FRONT_PLAN_WORDS && !(training && records));
    const FrontPlan fp = front_plan(C, width, height, debug_flags, training != 0, records != 0);
    const int64_t n_pairs = (int64_t)N * C;
    for (int i = 0; i < n_out; ++i) out[i] = 0;
    out[0] = fp.rect32; out[1] = fp.rectbase; out[2] = fp.key32; out[3] = fp.segments;
    out[4] = st3r_scan_tiles(n_pairs);
    int bpc, grid, self_base;
    st3r_emit_grid(N, C, &bpc, &grid, &self_base);
    out[5] = bpc; out[6] = grid; out[7] = self_base;
    int64_t sh[8];
    // the level-1 sort: segments, or the (camera | depth) keys on fp.l1_end_bit bits
    if (fp.segments) st3r_radix_sort_shape(4, n_pairs, N, C, 0, 0, sh);
    else st3r_radix_sort_shape(fp.key32 ? 4 : 8, n_pairs, 0, 0, 0, fp.l1_end_bit, sh);
    out[8] = sh[0]; out[9] = sh[1]; out[10] = sh[2]; out[11] = sh[3]; out[12] = sh[4];
    out[25] = sh[5];
    out[fp.key32 ? 26 : 28] = sh[6]; out[fp.key32 ? 27 : 29] = sh[7];
    st3r_radix_sort_shape(fp.key32 ? 8 : 4, 1, 0, 0, 0, 8, sh);   // (the other key width's two tile sizes)
    out[fp.key32 ? 28 : 26] = sh[6]; out[fp.key32 ? 29 : 27] = sh[7];
    // the tile sort over n_records (camera, tile) keys (a call with the count on the device decides on its capacity)
    out[13] = st3r_sort_tile_end_bit(fp.end_bit);
    if (n_records > 0) {
        st3r_radix_sort_shape(4, n_records, 0, 0, 0, (int)out[13], sh);
        out[14] = sh[0]; out[15] = sh[1]; out[16] = sh[2]; out[17] = sh[4];
    }
    // the banded form of the tile sort (words 14 .. 17 keep describing the two-pass form, which debug flag 16 selects):
    // taken or not, its bands, and the tiles its one pass is launched with
    if (st3r_sort_tile_banded(fp.end_bit, debug_flags)) {
        out[18] = 1;
        out[19] = (((int64_t)C * fp.tile_w * fp.tile_h - 1) >> 8) + 1;
        if (n_records > 0) out[30] = n_records / st3r_radix_sort_band_tile(n_records) + out[19];
    }
    int64_t k[5];
    st3r_isect_constants(k);
    for (int i = 0; i < 5; ++i) out[20 + i] = k[i];
    return ST3R_OK;
}
