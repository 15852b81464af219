// Internal helpers shared by the HIP translation units of libst3r_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/st3r.h"

#define ST3R_EXPORT extern "C" __attribute__((visibility("default")))

void st3r_set_error(const char* fmt, ...);

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            st3r_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));   \
            return ST3R_ERR_HIP;                                                                   \
        }                                                                                          \
    } while (0)

#define ARG_CHECK(cond)                                                                    \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            st3r_set_error("%s:%d: invalid argument: %s", __FILE__, __LINE__, #cond);      \
            return ST3R_ERR_INVALID;                                                       \
        }                                                                                  \
    } while (0)

#define LAUNCH_CHECK() HIP_TRY(hipGetLastError())

// Grow-only scratch arena.  Slots are named so that steady-state iterations never allocate.
enum ArenaSlot {
    SLOT_SPLATS = 0,
    SLOT_TILES,
    SLOT_CUM,
    SLOT_KEYS_A,
    SLOT_KEYS_B,
    SLOT_VALS_A,
    SLOT_VALS_B,
    SLOT_OFFSETS,
    SLOT_RGB,
    SLOT_ALPHA,
    SLOT_LAST,
    SLOT_VRENDER,
    SLOT_VSPLATS,     // fused step with poses: the per-pair gradients k_gather_vtile materialises for the pose backward
    SLOT_SSIM_A,
    SLOT_SORT_TMP,
    SLOT_SCAN_TMP,
    SLOT_SMALL,
    SLOT_CMASK,
    SLOT_TILE_NB,
    SLOT_VTILE,
    SLOT_DKEYS_A,
    SLOT_DKEYS_B,
    SLOT_DVALS_A,
    SLOT_DVALS_B,
    SLOT_CUM_D,
    SLOT_NN_PART,
    SLOT_MCMC_CUM,
    SLOT_MCMC_DEAD,
    SLOT_MCMC_RANK,
    SLOT_MCMC_COUNT,
    SLOT_MCMC_SAMPLED,
    SLOT_MCMC_BINOMS,
    SLOT_REG_PART,
    SLOT_RECTS,
    SLOT_RECTS_D,
    SLOT_RECTBASE,
    SLOT_COUNTS,
    SLOT_PSTAGE,
    SLOT_GSTAGE,
    SLOT_ALIGN_CTL,   // alignment: the chain cache of k_align_update
    SLOT_PAIR_TOUCH,  // blend backward -> projection backward: per-pair stamp "some slot of this pair was written" (gs_blend.hip)
    SLOT_KRANGE_PART, // projection: per-block smallest / largest level-1 key (gs_project.hip)
    SLOT_SCAN_CHAIN,  // single-pass scans (gs_isect.hip): ticket, totals, one status word per tile
    SLOT_POSE_PART,   // pose backward (gs_pose_bwd.hip): one 15-double partial per (camera, block of 256 Gaussians)
    SLOT_VTILE_DEPTH, // depth blend backward (gs_blend_depth.hip): its own stamped per-(record, tile) slots, 32 bytes each
    SLOT_DEPTH_PART,  // depth -> poses (gs_blend_depth.hip): one 4-double partial per (camera, block of 256 Gaussians)
    SLOT_POSE_GRAD,   // fused step with poses (gs_pose_step.hip): v_viewmats [C,4,4] of the step when the caller wants no copy
    SLOT_DEPTH,       // fused step with a depth prior (fused_step.hip): the accumulated depth D [C,H,W] of the step's render
    SLOT_VDEPTH,      // the same: d loss / d D [C,H,W]
    SLOT_VALPHA,      // the same: d loss / d alpha [C,H,W] (the derivative through ED = D / alpha)
    SLOT_VSPLATS_D,   // the same: the per-pair gradients of the depth blend backward, added to SLOT_VSPLATS
    SLOT_DPRIOR_PART, // depth-prior loss (loss_depth.hip): one double partial per (view, workgroup)
    SLOT_DPRIOR_NORM, // the same: n_c = max(sum w_c, 1) of every registered view, computed once per registration
    SLOT_DPRIOR_SUMS, // the same: sum_p w |ED - Z| per view of the fused step
    SLOT_EXPOSURE_PART, // exposure backward (gs_exposure.hip): one 12-double partial per (view, workgroup)
    SLOT_SCAN_CHAIN_B, // the band-counter scan of the banded emission (gs_isect.hip): a control block of its own, so that no clear of it can touch the pair-order scan's total while the step still reads it
    SLOT_EXPOSED,     // fused step with exposures (fused_step.hip): the exposed image y [C,H,W,3] the loss reads (SLOT_RGB keeps the raw render)
    SLOT_KGRAD_PART,  // intrinsics backward (gs_intrinsics.hip): one 4-double partial per (camera, block of 256 Gaussians)
    SLOT_LWEIGHT_PART, // per-pixel loss weights (loss.hip): one 2-double partial per (view, workgroup) of their sums
    SLOT_LWEIGHT_NORM, // the same: (sum_p w, sum_{p in I} w) of every registered view, computed once per registration
    SLOT_COMPOSITE,   // fused step with backgrounds (fused_step.hip): the composited image [C,H,W,3] the exposure / the loss reads (SLOT_RGB keeps the raw render)
    SLOT_AGRAD_PART,  // st3r_alpha_grad (gs_alpha.hip): per (view, workgroup) three doubles (v_backgrounds), then one (sum w |a - M|)
    SLOT_ATARGET_PART, // alpha targets (gs_alpha.hip): one double partial per (view, workgroup) of the weights' sums
    SLOT_ATARGET_NORM, // the same: n_c = max(sum w_c, 1) of every registered view, computed once per registration
    SLOT_ATARGET_SUMS, // the same: sum_p w |a - M| per view of the fused step
    SLOT_ACT_SCALES,  // activated parameters (gs_activation.hip): exp(scales) [N,3] of the fused step / st3r_gs_render
    SLOT_ACT_OPACITIES, // the same: sigmoid(opacities) [N]
    SLOT_ACT_PART,    // the same: one 2-double partial per workgroup of (sum sigmoid, sum exp)
    SLOT_COUNT
};

// Stage ids for the optional per-stage HIP-event timing (st3r_ctx_set_profiling).
enum Stage {
    STG_PROJECT = 0,
    STG_SCAN,
    STG_EMIT,
    STG_SORT,
    STG_OFFSETS,
    STG_BLEND_FWD,
    STG_LOSS,
    STG_BLEND_BWD,
    STG_PROJECT_BWD,
    STG_ADAM,
    STG_SORT_DEPTH,
    STG_COUNT
};
#define PROF_RING 64
#define ST3R_MAX_RANGES 8

#define ST3R_SPLIT_VIEWS 1000   // internal: more than 2^31 tile intersections, the caller may retry with fewer views

// the backward's stamped (record, tile) slots, handed to the kernel that sums them per pair (gs_blend.hip -> gs_project_bwd.hip)
// touch (may be NULL): per pair the stamp of the last backward call in which some (record, tile) of the pair contributed --
// written by k_blend_bwd for scenes of many slots per pair, so that the gather can skip the slots of pairs nobody touched
struct st3r_vtile_ref { const int32_t* cum; const float* vtile; int stamp; unsigned vt_cap; const uint32_t* touch; };

// "Registered for these views": the c images of h x w pixels at gt ([c,h,w,3]); gt == NULL: nothing registered.
struct ViewReg { const float* gt; int c, h, w; };

// The first registered view of a call on the C views of H x W pixels at `gt`, or -1 when the registration does not
// apply: nothing registered, another image size, not a whole-view offset into the registered images (a call on a view
// chunk is one), or more views than are registered.  The one rule that makes view chunks work with every option.
static inline int64_t view_reg_first(const ViewReg& r, const float* gt, int C, int H, int W) {
    if (!r.gt || H != r.h || W != r.w) return -1;
    const int64_t img = (int64_t)H * W * 3;
    if (gt < r.gt || (gt - r.gt) % img != 0) return -1;
    const int64_t c0 = (gt - r.gt) / img;
    return c0 + C <= r.c ? c0 : -1;
}

// the st3r_ctx_set_* calls: `on` false (a NULL pointer among the caller's) clears *r, otherwise the views are checked and stored
static inline int view_reg_set(ViewReg* r, bool on, const float* gt, int C, int height, int width) {
    if (!on) { *r = ViewReg{}; return ST3R_OK; }
    ARG_CHECK(C > 0 && height > 0 && width > 0);
    *r = ViewReg{gt, C, height, width};
    return ST3R_OK;
}

// A weighted per-pixel target registered for a set of views -- the depth prior and the alpha targets are two of these:
// the target and weight maps [c,h,w] (caller-owned), the factor of its loss term (0: none), and norm_valid: the option's
// norm slot holds the n_c = max(sum w_c, 1) of this registration (computed by the first training call that uses it).
struct TargetReg { ViewReg reg; const float* map; const float* weight; float fac; int norm_valid; };

// st3r_ctx_set_depth_prior / st3r_ctx_set_alpha_target; fac_ok: the setter's own check of its factor
static inline int target_reg_set(TargetReg* r, const float* gt, const float* map, const float* weight, int C, int height,
                                 int width, float fac, bool fac_ok) {
    r->norm_valid = 0;
    const bool on = gt && map && weight;
    ARG_CHECK(!on || fac_ok);
    int rc = view_reg_set(&r->reg, on, gt, C, height, width);
    if (rc) return rc;
    r->map = on ? map : nullptr; r->weight = on ? weight : nullptr; r->fac = on ? fac : 0.f;
    return ST3R_OK;
}

struct st3r_ctx {
    int device;
    void* slot_ptr[SLOT_COUNT];
    size_t slot_bytes[SLOT_COUNT];
    int64_t* pinned;  // small pinned host buffer for read-backs
    // profiling: ring of (start, stop) events per stage; elapsed times are harvested lazily
    int debug_flags;  // st3r_ctx_set_debug: bit 0 = blend forward ignores the per-quadrant relevance test; 1: backward
                      // recomputes the tile rectangles; 2 (4): level-1 sort on (camera | depth) keys in four passes; 3: async capacity halved; 4 (16): plain emission and two-pass tile sort instead of the banded form; 8 (256, acts when set): the scans' status-word generations jump to two or three launches before their wrap; 5: training calls start at 2 view chunks;
                      // 6: backward gathers rectangle and slot base separately; 7 (128): training forward on the quadrant
                      // kernel; 9 (512): st3r_gs_render on the cell-list kernel; 10 (1024): the banded tile sort keeps its
                      // two arrays (tile keys next to pair ids, offsets read from the sorted keys) instead of the packed
                      // word (fused_step.hip: rasterize_front); 11 (2048): under a communicator
                      // st3r_gs_train_step behaves as if this rank's forward / backward had failed (comm.hip)
                      // (round 5's experiment switches -- 4096 masked rectangles, 8192 cell-granular backward, 16384 slot sums
                      // in a kernel of their own -- left the library in round 6: tools/experiments/README.md)
    // What the caller registered for a set of views (ViewReg) and each option's payload: caller-owned, valid until cleared.
    // ground-truth moments (st3r_ctx_set_gt_moments, loss.hip)
    ViewReg gtm; const float* gtm_mom;
    // depth prior (st3r_ctx_set_depth_prior, loss_depth.hip) and alpha targets (st3r_ctx_set_alpha_target, gs_alpha.hip);
    // their norms live in SLOT_DPRIOR_NORM and SLOT_ATARGET_NORM
    TargetReg dp, at;
    // exposures (st3r_ctx_set_exposure, gs_exposure.hip)
    ViewReg ex; const float* ex_exposure; float* ex_v_exposure;
    // intrinsics gradient (st3r_ctx_set_intrinsics_grad, gs_intrinsics.hip): where d loss / d (fx, fy, cx, cy) goes
    ViewReg kg; float* kg_v_Ks;
    // per-pixel loss weights (st3r_ctx_set_loss_weight, loss.hip); lw_norm_valid: SLOT_LWEIGHT_NORM holds the sums of this
    // registration (computed by the first training call that uses it)
    ViewReg lw; const float* lw_weight; int lw_norm_valid;
    // backgrounds (st3r_ctx_set_background, gs_alpha.hip): [c,3]
    ViewReg bg; const float* bg_colors;
    // activated parameters (st3r_ctx_set_activation, gs_activation.hip): the fused steps and st3r_gs_render read the scales
    // as logs and the opacities as logits
    int activation;
    // SH degree (st3r_ctx_set_sh_degree, project_common.h): the rows the tensor holds, the rows evaluated, and where the
    // gradients of the rows 4.. go (caller-owned); (1, 1, NULL) unless set
    int sh_degree, sh_active; float* sh_v_high;
    int bwd_stamp;  // generation stamp of the per-(record, tile) partial-gradient slots
    int depth_stamp;  // the same for the depth backward's slots (SLOT_VTILE_DEPTH)
    uint32_t scan_gen;   // single-pass scan (gs_isect.hip): generation of its status words
    uint32_t scan_gen_b; // the same for the band-counter scan's own control block (SLOT_SCAN_CHAIN_B)
    // record count of the fused steps without a host round trip: sizing hint from the last known count, the read-back
    // still in flight (event), and the capacity the in-flight step was given
    int64_t isect_hint, count_cap;
    int64_t hint_sig;   // (N, C, W, H) the hint belongs to: another workload takes the synchronous path
    int count_pending;
    int view_chunks;    // > 1: the training calls walk their views in this many chunks (2^31 intersections per chunk)
    hipEvent_t count_event;
    void* comm;     // ncclComm_t of the view-sharded job (NULL: single replica)
    int comm_owned, comm_rank, comm_size;
    int exchange;   // ST3R_EXCHANGE_*: the form the gradient exchange of st3r_gs_train_step takes (comm.hip)
    int comm_broken;         // a device-side barrier of the direct form timed out: the ranks lost lockstep (comm.hip)
    int peer_pending;        // the status word of the last exchanged step is still to be looked at (comm.hip)
    hipEvent_t peer_event;
    // range-wise exchange (comm.hip): the projection backward runs once per Gaussian range and leaves an event per
    // range; the ranges' all-reduces run on comm_stream behind those events, Adam per range behind the all-reduces
    hipStream_t comm_stream;
    hipEvent_t ev_range_bwd[ST3R_MAX_RANGES], ev_range_red[ST3R_MAX_RANGES];
    void* xwin;              // direct exchange (comm.hip): this rank's exported buffers and the peers' mapped ones
    int n_ranges;            // > 1: train_views splits the projection backward (set by st3r_gs_train_step for one call)
    int ranges_recorded;     // how many ev_range_bwd the last train_views recorded (0: it ran as one launch)
    int prof_enabled;
    hipEvent_t prof_ev[PROF_RING][STG_COUNT][2];
    unsigned char prof_used[PROF_RING][STG_COUNT];
    int prof_slot;          // ring slot of the step being recorded
    double prof_ms[STG_COUNT];
    int64_t prof_n[STG_COUNT];
};

void st3r_prof_begin(st3r_ctx* ctx, hipStream_t s, int stage);
void st3r_prof_end(st3r_ctx* ctx, hipStream_t s, int stage);
void st3r_prof_next_step(st3r_ctx* ctx);

// returns a device pointer with at least `bytes` capacity for `slot` (contents undefined after growth)
int st3r_arena_get(st3r_ctx* ctx, int slot, size_t bytes, void** out);
// same, *grown = 1 when the slot was (re)allocated by this call
int st3r_arena_get2(st3r_ctx* ctx, int slot, size_t bytes, void** out, int* grown);
// declares `type* var` = the scratch of `slot` with room for `count` elements; on failure the enclosing function (which
// has a `ctx`) returns the error code
#define ARENA_GET(slot, type, count, var)                                                    \
    type* var;                                                                               \
    {                                                                                        \
        void* _p;                                                                            \
        int _rc = st3r_arena_get(ctx, slot, sizeof(type) * (size_t)(count), &_p);            \
        if (_rc) return _rc;                                                                 \
        var = (type*)_p;                                                                     \
    }

// the band table of the banded tile sort (gs_isect.hip: k_band_table writes it, radix_sort.hip reads it): two arrays of
// this many words -- up to 256 band starts + the record count, up to 256 first sort tiles + the tiles in use
#define ST3R_BAND_TAB 257

static inline int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static inline int bit_length_u32(uint32_t v) { int n = 0; while (v) { ++n; v >>= 1; } return n; }

