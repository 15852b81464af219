// C-ABI glue: context lifetime, scratch arena, error reporting, per-stage timing, peek / settle / release.
// No device code here; the fused steps that chain the stage kernels are in fused_step.hip.
#include <stdarg.h>

#include "stages.h"

static thread_local char g_err[512] = "";

void st3r_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

ST3R_EXPORT int st3r_version(void) { return ST3R_VERSION; }
ST3R_EXPORT const char* st3r_last_error(void) { return g_err; }

ST3R_EXPORT int st3r_ctx_create(int device, st3r_ctx** out) {
    ARG_CHECK(out);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    ARG_CHECK(device >= 0 && device < ndev);
    HIP_TRY(hipSetDevice(device));
    st3r_ctx* c = new (std::nothrow) st3r_ctx();
    if (!c) { st3r_set_error("out of host memory"); return ST3R_ERR_NOMEM; }
    memset(c, 0, sizeof(*c));
    c->device = device;
    c->sh_degree = c->sh_active = 1;
    hipError_t e = hipHostMalloc((void**)&c->pinned, 64 * sizeof(int64_t), hipHostMallocDefault);
    if (e != hipSuccess) { delete c; st3r_set_error("hipHostMalloc: %s", hipGetErrorString(e)); return ST3R_ERR_HIP; }
    *out = c;
    return ST3R_OK;
}

ST3R_EXPORT int st3r_ctx_destroy(st3r_ctx* ctx) {
    if (!ctx) return ST3R_OK;
    (void)hipSetDevice(ctx->device);
    (void)st3r_comm_destroy(ctx);
    for (int i = 0; i < SLOT_COUNT; ++i)
        if (ctx->slot_ptr[i]) (void)hipFree(ctx->slot_ptr[i]);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->count_event) (void)hipEventDestroy(ctx->count_event);
    if (ctx->peer_event) (void)hipEventDestroy(ctx->peer_event);
    if (ctx->comm_stream) {
        for (int j = 0; j < ST3R_MAX_RANGES; ++j) {
            (void)hipEventDestroy(ctx->ev_range_bwd[j]); (void)hipEventDestroy(ctx->ev_range_red[j]);
        }
        (void)hipStreamDestroy(ctx->comm_stream);
    }
    if (ctx->prof_ev[0][0][0])
        for (int r = 0; r < PROF_RING; ++r)
            for (int st = 0; st < STG_COUNT; ++st)
                for (int k = 0; k < 2; ++k) (void)hipEventDestroy(ctx->prof_ev[r][st][k]);
    delete ctx;
    return ST3R_OK;
}

ST3R_EXPORT int64_t st3r_ctx_arena_bytes(st3r_ctx* ctx) {
    if (!ctx) return 0;
    int64_t t = 0;
    for (int i = 0; i < SLOT_COUNT; ++i) t += (int64_t)ctx->slot_bytes[i];
    return t;
}

int st3r_arena_get(st3r_ctx* ctx, int slot, size_t bytes, void** out) {
    int grown;
    return st3r_arena_get2(ctx, slot, bytes, out, &grown);
}

int st3r_arena_get2(st3r_ctx* ctx, int slot, size_t bytes, void** out, int* grown) {
    *grown = 0;
    if (bytes == 0) bytes = 16;
    if (ctx->slot_bytes[slot] < bytes) {
        // grow with 25% headroom so slowly growing intersection counts do not reallocate every step
        size_t want = bytes + bytes / 4;
        want = (want + 255) & ~(size_t)255;
        if (ctx->slot_ptr[slot]) {
            HIP_TRY(hipDeviceSynchronize());
            HIP_TRY(hipFree(ctx->slot_ptr[slot]));
            ctx->slot_ptr[slot] = nullptr; ctx->slot_bytes[slot] = 0;
        }
        hipError_t e = hipMalloc(&ctx->slot_ptr[slot], want);
        if (e != hipSuccess) {
            st3r_set_error("arena slot %d: hipMalloc(%zu) failed: %s", slot, want, hipGetErrorString(e));
            return ST3R_ERR_NOMEM;
        }
        ctx->slot_bytes[slot] = want;
        *grown = 1;
    }
    *out = ctx->slot_ptr[slot];
    return ST3R_OK;
}

// Debug/test hook: device pointer and capacity of a scratch buffer of the last fused step.
// which: 0 = sorted pair ids ("flatten ids", int32 [n_isects]), 1 = tile offsets (int32 [C*tiles]),
//        2 = splat records (float [C*N*12]), 3 = inclusive tile scan in pair-id order (int32 [C*N])
//        11 / 12 = emitted tile keys / pair ids (the tile sort's input), 13 = sorted tile keys (uint32 / int32 [n_isects])
//        Packed tile sort (banded form, N * C <= 2^24, debug flag 1024 clear): 11 and 13 stay allocated but are NOT written
//        (whatever an earlier step left), 12 = the packed words pair id | low key byte << 24, 0 = clean pair ids.
ST3R_EXPORT int st3r_ctx_peek(st3r_ctx* ctx, void* stream, int which, void* dst, int64_t bytes) {
    ARG_CHECK(ctx && dst && bytes >= 0 && which >= 0 && which <= 13);
    static const int slots[14] = {SLOT_VALS_B, SLOT_OFFSETS, SLOT_SPLATS, SLOT_CUM,
                                  SLOT_MCMC_CUM, SLOT_MCMC_DEAD, SLOT_MCMC_SAMPLED, SLOT_MCMC_COUNT,
                                  SLOT_RGB, SLOT_ALPHA, SLOT_COUNTS, SLOT_KEYS_A, SLOT_VALS_A, SLOT_KEYS_B};
    ARG_CHECK((size_t)bytes <= ctx->slot_bytes[slots[which]]);
    HIP_TRY(hipMemcpyAsync(dst, ctx->slot_ptr[slots[which]], (size_t)bytes, hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
    return ST3R_OK;
}

// ---- per-stage event timing ----
static const char* k_stage_names[STG_COUNT] = {"project", "scan", "emit", "sort", "offsets", "blend_fwd", "loss",
                                               "blend_bwd", "project_bwd", "adam", "sort_depth"};

ST3R_EXPORT const char* st3r_stage_name(int stage) {
    return (stage >= 0 && stage < STG_COUNT) ? k_stage_names[stage] : "";
}

static void prof_harvest_slot(st3r_ctx* ctx, int slot) {
    for (int st = 0; st < STG_COUNT; ++st) {
        if (!ctx->prof_used[slot][st]) continue;
        float ms = 0.f;
        if (hipEventSynchronize(ctx->prof_ev[slot][st][1]) == hipSuccess &&
            hipEventElapsedTime(&ms, ctx->prof_ev[slot][st][0], ctx->prof_ev[slot][st][1]) == hipSuccess) {
            ctx->prof_ms[st] += ms; ctx->prof_n[st] += 1;
        }
        ctx->prof_used[slot][st] = 0;
    }
}

void st3r_prof_begin(st3r_ctx* ctx, hipStream_t s, int stage) {
    if (!((ctx->prof_enabled >> stage) & 1)) return;
    (void)hipEventRecord(ctx->prof_ev[ctx->prof_slot][stage][0], s);
}

void st3r_prof_end(st3r_ctx* ctx, hipStream_t s, int stage) {
    if (!((ctx->prof_enabled >> stage) & 1)) return;
    (void)hipEventRecord(ctx->prof_ev[ctx->prof_slot][stage][1], s);
    ctx->prof_used[ctx->prof_slot][stage] = 1;
}

void st3r_prof_next_step(st3r_ctx* ctx) {
    if (!ctx->prof_enabled) return;
    ctx->prof_slot = (ctx->prof_slot + 1) % PROF_RING;
    prof_harvest_slot(ctx, ctx->prof_slot);  // events from PROF_RING steps ago: long finished
}

ST3R_EXPORT int st3r_ctx_set_debug(st3r_ctx* ctx, int flags) {
    ARG_CHECK(ctx);
    ctx->debug_flags = flags;
    // test hook, acts once when set: the next launch of either single-pass scan is the last one of its 14-bit status-word
    // generation, the one after it clears its control block (gs_isect.hip: chain_ctl)
    // (the two ticket counters of a scan take turns by generation parity, so the parity sequence is kept: two or three
    // launches are left)
    if (flags & 256) {
        ctx->scan_gen = (ctx->scan_gen & 1u) ? 0x3FFDu : 0x3FFEu;
        ctx->scan_gen_b = (ctx->scan_gen_b & 1u) ? 0x3FFDu : 0x3FFEu;
    }
    return ST3R_OK;
}

// The SH degree as a setting of the context (project_common.h); launches nothing.
ST3R_EXPORT int st3r_ctx_set_sh_degree(st3r_ctx* ctx, int degree, int active_degree, float* v_sh_high) {
    ARG_CHECK(ctx && 0 <= active_degree && active_degree <= degree && degree <= 3);
    ARG_CHECK(degree >= 2 || !v_sh_high);
    ctx->sh_degree = degree; ctx->sh_active = active_degree; ctx->sh_v_high = v_sh_high;
    return ST3R_OK;
}

ST3R_EXPORT int st3r_ctx_get_sh_degree(st3r_ctx* ctx, int* degree, int* active_degree, float** v_sh_high) {
    ARG_CHECK(ctx && degree && active_degree && v_sh_high);
    *degree = ctx->sh_degree; *active_degree = ctx->sh_active; *v_sh_high = ctx->sh_v_high;
    return ST3R_OK;
}

// test hook: where the stamp counters of the backward slots stand (blend_common.h: stamped_slots), so that a test can put a
// context next to the restart without two billion calls.  No kernel reads these but through the next call's arguments.
ST3R_EXPORT int st3r_ctx_debug_set_stamps(st3r_ctx* ctx, int colour, int depth) {
    ARG_CHECK(ctx && colour <= 2147483000 && depth <= 2147483000);
    if (colour >= 0) ctx->bwd_stamp = colour;
    if (depth >= 0) ctx->depth_stamp = depth;
    return ST3R_OK;
}

ST3R_EXPORT int st3r_ctx_set_profiling(st3r_ctx* ctx, int enable) {
    ARG_CHECK(ctx && enable >= 0 && enable < 2 + STG_COUNT);
    if (enable && !ctx->prof_ev[0][0][0]) {
        for (int r = 0; r < PROF_RING; ++r)
            for (int st = 0; st < STG_COUNT; ++st)
                for (int k = 0; k < 2; ++k) HIP_TRY(hipEventCreate(&ctx->prof_ev[r][st][k]));
    }
    // prof_enabled is the mask of timed stages: enable = 1 -> all of them, enable = 2 + stage -> that stage only
    ctx->prof_enabled = enable == 0 ? 0 : (enable == 1 ? (1 << STG_COUNT) - 1 : (1 << (enable - 2)));
    return ST3R_OK;
}

ST3R_EXPORT int st3r_ctx_get_stage_ms(st3r_ctx* ctx, double* ms_out, int64_t* counts_out) {
    ARG_CHECK(ctx && ms_out && counts_out);
    HIP_TRY(hipDeviceSynchronize());
    if (ctx->prof_ev[0][0][0])
        for (int r = 0; r < PROF_RING; ++r) prof_harvest_slot(ctx, r);
    for (int st = 0; st < STG_COUNT; ++st) {
        ms_out[st] = ctx->prof_ms[st]; counts_out[st] = ctx->prof_n[st];
        ctx->prof_ms[st] = 0; ctx->prof_n[st] = 0;
    }
    return ST3R_OK;
}

ST3R_EXPORT int st3r_ctx_settle(st3r_ctx* ctx) {
    ARG_CHECK(ctx);
    int rc = st3r_peer_status_settle(ctx);
    if (rc) return rc;
    return st3r_count_settle(ctx);
}

ST3R_EXPORT int st3r_ctx_release_scratch(st3r_ctx* ctx) {
    ARG_CHECK(ctx);
    HIP_TRY(hipDeviceSynchronize());
    const int rc = st3r_ctx_settle(ctx);   // an overflow / a peer's failure of the last asynchronous step is still reported
    for (int i = 0; i < SLOT_COUNT; ++i) {
        if (ctx->slot_ptr[i]) (void)hipFree(ctx->slot_ptr[i]);
        ctx->slot_ptr[i] = nullptr; ctx->slot_bytes[i] = 0;   // (every user of a slot's CONTENTS re-initialises on growth)
    }
    return rc;
}

// the 16 device words next to the fused steps (stages.h)
int st3r_counts_buffer(st3r_ctx* ctx, hipStream_t s, int32_t** out) {
    void* p; int grown = 0;
    int rc = st3r_arena_get2(ctx, SLOT_COUNTS, sizeof(int32_t) * 16, &p, &grown);
    if (rc) return rc;
    if (grown) HIP_TRY(hipMemsetAsync(p, 0, ctx->slot_bytes[SLOT_COUNTS], s));
    *out = (int32_t*)p;
    return ST3R_OK;
}
