// What the three blend translation units share:
//   gs_blend.hip        colour blend, quadrant formulation: the stand-alone entry points and the shared backward;
//   gs_blend_cells.hip  colour forward with 4x4-cell lists: the fused training path;
//   gs_blend_depth.hip  depth blend, forward and backward.
// Here: the tile hand-out (xcd_remap) and the lane -> pixel geometry of a tile (tile_geom), the q-form of a staged record
// and its quadrant relevance, the one exponent expression (blend_power), the mask / DPP helpers of the walks, the layout
// constants of the backward, the gather of the stamped slots (k_gather_vtile<NV>) and, on the host, the hand-off
// buffers, the stamped slot buffers and the argument check of the exports.
#pragma once
#include "stages.h"
#include "tile_rect.h"

#define BLK 256
#define LOG2E 1.4426950408889634f

// Workgroup b runs on XCD b % 8 (each XCD has its own L2).  Tiles are handed out in groups of G consecutive
// tiles per XCD, the groups round-robin over the XCDs: neighbouring tiles (which share Gaussians) meet in one L2.
// A group is one TILE ROW (XCD_GROUP), whatever the number of views: every XCD then gets every eighth row of every camera --
// the dense image centre and the sparse borders are spread over all XCDs.  Rounds 2-5 gave a whole camera to an XCD when the
// views were a multiple of 8; measured in round 6 (alternating same-box A/B, frozen SYNTH-1M scene): rows instead of
// cameras -0.035 +- 0.006 ms on the blend backward (the cameras' record counts differ by a few per cent and the kernel
// ends with its slowest XCD), two rows per group equal, half rows +0.03, quarter rows +1.6 ms (vertical stripes: the XCDs
// that own the centre columns do most of the work), 17 rows +0.16.
#ifndef XCD_GROUP
#define XCD_GROUP(C, n_tiles, tile_w) (tile_w)
#endif
__device__ __forceinline__ int xcd_remap(int bid, int total, int G) {
    const int n_full = (total / (8 * G)) * (8 * G);
    if (bid >= n_full) return bid;
    const int xcd = bid & 7, k = bid >> 3;
    const int round = k / G, within = k - round * G;
    return (round * 8 + xcd) * G + within;
}

// lane -> pixel of the quadrant formulation: wave w owns the 8x8 quadrant (w & 1, w >> 1), lane l its pixel (l & 7, l >> 3)
struct TileGeom {
    int lb, cam, i, j, start, end, tx0, ty0;
    bool inside;
    float px, py;
};

__device__ __forceinline__ TileGeom tile_geom(int C, int W, int H, int tile_w, int tile_h,
                                              const int32_t* __restrict__ offsets, int n_isects) {
    TileGeom g;
    const int n_tiles = tile_w * tile_h, total = C * n_tiles;
    g.lb = xcd_remap(blockIdx.x, total, XCD_GROUP(C, n_tiles, tile_w));
    g.cam = g.lb / n_tiles;
    const int tile = g.lb - g.cam * n_tiles;
    const int ty = tile / tile_w, tx = tile - ty * tile_w;
    g.tx0 = tx * 16; g.ty0 = ty * 16;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    g.j = g.tx0 + ((w & 1) << 3) + (lane & 7);
    g.i = g.ty0 + ((w >> 1) << 3) + (lane >> 3);
    g.inside = (g.i < H) && (g.j < W);
    g.px = (float)g.j + 0.5f; g.py = (float)g.i + 0.5f;
    g.start = offsets[g.lb];
    // n_isects < 0: the offsets array carries one more entry, the total (fused path: the count lives on the device)
    g.end = (g.lb == total - 1 && n_isects >= 0) ? n_isects : offsets[g.lb + 1];
    return g;
}

__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// Stage record `id` into LDS slot t (q-form) and return the 4-bit quadrant relevance.
// q-form of a record in LDS slot t (see the arithmetic note above); forward and backward stage through this one function
// LDS record: 3 x float4 = (x y opacity qa | qb qc r g | b - - -); one address register serves the three reads
__device__ __forceinline__ void stage_qform(const float4& a, const float4& b, const float4& c, int t, float4* sR) {
    sR[3 * t + 0] = make_float4(a.x, a.y, a.z, -0.5f * LOG2E * a.w);
    sR[3 * t + 1] = make_float4(-LOG2E * b.x, -0.5f * LOG2E * b.y, b.z, b.w);
    sR[3 * t + 2] = make_float4(c.x, 0.f, 0.f, 0.f);
}

// The 4-bit quadrant relevance of a record (a = x y opacity conic.a, b = conic.b conic.c . .) for the tile at (tx0, ty0).
// A quadrant (8x8 pixel centres) is relevant iff the ellipse {sigma(p) <= tau}, tau = ln(255 opacity), reaches
// it: either the mean lies inside, or the minimum of sigma over one of its four edges is <= tau (sigma is
// convex, so the minimum over the square sits on the boundary when the mean is outside).  tau is inflated
// (2e-4 relative + 2e-4) so that every pixel of a quadrant declared irrelevant fails the alpha test of the
// blend loop in float arithmetic as well.  Costs ~150 instructions per RECORD (one lane), and removes a
// quarter of the per-(record, quadrant) wave iterations of the axis-aligned-box test it replaces.
__device__ __forceinline__ int quadrant_relevance(const float4& a, const float4& b, int tx0, int ty0) {
    EllipseTest et;
    if (!ellipse_prepare(a.z, a.w, b.x, b.y, &et)) return 0;
    const float rx = ((float)tx0 + 0.5f) - a.x, ry = ((float)ty0 + 0.5f) - a.y;  // first pixel centre - mean
    int rel = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float dx0 = rx + (float)((q & 1) * 8), dy0 = ry + (float)((q >> 1) * 8);
        rel |= ellipse_hits_square(et, dx0, dx0 + 7.0f, dy0, dy0 + 7.0f) ? (1 << q) : 0;
    }
    return rel;
}

// word index of the first 64-record chunk of tile lb in the contribution-mask arrays
// (a tile of `len` records uses 4*ceil(len/256) <= floor(len/64) + 4 words, hence the 4*lb slack)
__device__ __forceinline__ int64_t mask_base(int lb, int start) { return (int64_t)(start >> 6) + 4 * (int64_t)lb; }

// The exponent of a record at a pixel, P = -log2(e) sigma = dx (qa dx + qb dy) + qc dy^2, with ONE fixed association
// and contraction: every blend kernel (forward and backward, quadrant and cell formulation) must take identical
// include / skip decisions, and hipcc contracts the plain expression differently from kernel to kernel (round 3: the
// quadrant forward computed fma(dx, lx, (qc dy) dy), the backward fma(dy, qc dy, dx lx)).
__device__ __forceinline__ float blend_power(float dx, float dy, float qa, float qb, float qc) {
#pragma clang fp contract(off)
    const float lx = __builtin_fmaf(dx, qa, qb * dy);
    return __builtin_fmaf(dx, lx, (qc * dy) * dy);
}

// Compare into a scalar register pair / select under such a mask, spelled out: hipcc keeps a compare result that must
// outlive the next compare in a VGPR (v_cndmask 0/1 + v_cmp_ne to get the ballot back: two extra VALU instructions per
// trip of the forward loop).  "s_nop 1": wait states between a scalar write of the mask and its use by v_cndmask.
__device__ __forceinline__ uint64_t mask_not_less(float a, float b) {   // lanes with !(a < b)
    uint64_t m;
    asm("v_cmp_nlt_f32_e64 %0, %1, %2" : "=s"(m) : "v"(a), "v"(b));
    return m;
}
__device__ __forceinline__ uint64_t mask_not_positive(float a) {        // lanes with !(a > 0)
    uint64_t m;
    asm("v_cmp_nlt_f32_e64 %0, 0, %1" : "=s"(m) : "v"(a));
    return m;
}
__device__ __forceinline__ float zero_unless(uint64_t m, float x) {     // m ? x : 0
    float r;
    asm("s_nop 1\n\tv_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(x), "s"(m));
    return r;
}

// reduce9_rows: sums g[0..8] over the 16 lanes of every DPP row (row = one record of the chunk) with DPP adds only:
//   level 1 (lanes l, l ^ 8)   two values per register -- lanes 0-7 keep the first, lanes 8-15 the second (the writes are
//                              restricted with bank_mask; a bank = four consecutive lanes), 9 instructions -> 5 registers;
//   level 2 (lanes l, l ^ 4)   the same trick with row_shl:4 / row_shr:4: 5 instructions -> 3 registers, every bank now
//                              holds a different value;
//   levels 3, 4                inside the quads (quad_perm), all four lanes end with the total: 6 instructions.
// 20 DPP adds (1.7 ns each on this chip) instead of 8 lane swaps (3.4 ns) + 8 adds + 6 DPP adds of reduce9.
// On return, in bank b (lanes 4b .. 4b+3) of every row: k0 = total of g[{0,2,1,3}[b]], k1 = total of g[{4,6,5,7}[b]],
// k2 (bank 0 only) = total of g[8].
__device__ __forceinline__ void reduce9_rows(float g0, float g1, float g2, float g3, float g4, float g5, float g6,
                                             float g7, float g8, float& k0, float& k1, float& k2) {
    float t0, t1, t2, t3, t4;
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %5, %5 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %1, %7, %7 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %2, %9, %9 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %3, %11, %11 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %4, %13, %13 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %0, %6, %6 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %1, %8, %8 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %2, %10, %10 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %3, %12, %12 row_ror:8 row_mask:0xf bank_mask:0xc"
        : "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&v"(t4)
        : "v"(g0), "v"(g1), "v"(g2), "v"(g3), "v"(g4), "v"(g5), "v"(g6), "v"(g7), "v"(g8));
    float u0, u1, u2;
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %3, %3 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %1, %5, %5 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %2, %7, %7 row_shl:4 row_mask:0xf bank_mask:0x1\n\t"
        "v_add_f32_dpp %0, %4, %4 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %1, %6, %6 row_shr:4 row_mask:0xf bank_mask:0xa"
        : "=&v"(u0), "=&v"(u1), "=&v"(u2)
        : "v"(t0), "v"(t1), "v"(t2), "v"(t3), "v"(t4));
    asm volatile(
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %2, %2, %2 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf"
        : "+v"(u0), "+v"(u1), "+v"(u2));
    k0 = u0; k1 = u1; k2 = u2;
}
// sums per staged record and wave, and floats per (record, tile) slot = the sums + the stamp, in 8-byte stores:
#define ACC_VALS 9                    // colour: S_x S_y S_o S_xx S_xy S_yy S_r S_g S_b
#define VT_STRIDE (ACC_VALS + 1)      //         5 x 8 B
#define DACC_VALS 7                   // depth:  S_x S_y S_o S_xx S_xy S_yy S_z
#define DVT_STRIDE (DACC_VALS + 1)    //         4 x 8 B
#ifndef HB
#define HB 64           // records staged per backward round (a fraction of a forward batch of 256)
#endif
#define HB_WORDS (HB / 64)   // 64-record mask words per round
static_assert(HB == 64, "the backward walks one mask word per round");
#ifndef CHUNK
#define CHUNK 4         // records per transposition chunk (4 or 8); a lane of phase 2 owns CHUNK pixels of one row
#endif
// row layout of phase 2 (lane = part + 16 x record): a record row is 32 + 1 + 32 + 1 float2 -- pixel p sits at p + (p >> 5),
// rows 66 apart -- so that the 32 lanes of a read group (two records x 16 parts, 32-byte stride inside a row) meet in
// 32 different bank pairs
#define PAIR_STRIDE 66
#define PAIR_AT(pix) ((pix) + ((pix) >> 5))

// ---- pieces of the backward shared by k_blend_bwd and k_blend_depth_bwd ----
// Output slot of (record, this tile): u = cum_excl[pid] + index of the tile inside the record's tile rectangle (same
// float ops as the emit kernel => same integers).  Fused path: slot base and rectangle in one gathered word.
__device__ __forceinline__ int slot_of_rectbase(uint64_t r, int tx0, int ty0) {
    const int x0 = (int)(r & 0x3FF), y0 = (int)((r >> 10) & 0x3FF), rw = (int)((r >> 20) & 0x3FF);
    return (int)(r >> 32) + ((ty0 >> 4) - y0) * rw + ((tx0 >> 4) - x0);
}
// The same from the pair scan `cum` and a rectangle (x0, y0, width rw).
__device__ __forceinline__ int slot_of_rect(int cum_excl, int x0, int y0, int rw, int tx0, int ty0) {
    return cum_excl + ((ty0 >> 4) - y0) * rw + ((tx0 >> 4) - x0);
}

// Phase 2: the pixel sums of a lane's run from its index moments.  The lane's pixels are i = 0 .. CHUNK-1 to the right of
// its first one: with d0 = dx of the first pixel, sum g dx = d0 W0 - W1 and sum g dx^2 = d0 (d0 W0 - 2 W1) + W2 for the
// index moments W_k = sum i^k g_i -- 12 VALU instead of 21 for CHUNK = 4 (k_blend_bwd 2.27 -> 2.17 ms); the offsets are
// at most CHUNK-1 pixels, so the cancellation costs a few ulps.  dy is the same for the lane's pixels.
struct RunSums { float So, Sx, Sxx, Sy, Sxy, Syy; };
__device__ __forceinline__ RunSums run_sums(float W0, float W1, float W2, float d0, float dy) {
    const float So = W0, Sx = fmaf(d0, W0, -W1), Sxx = fmaf(d0, Sx - W1, W2);
    const float Sy = So * dy, Sxy = Sx * dy, Syy = Sy * dy;
    return RunSums{So, Sx, Sxx, Sy, Sxy, Syy};
}

__device__ __forceinline__ void wave_lds_sync() {
    // LDS operations of one wave complete in order; this only stops the compiler from moving them across
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---- gather: the stamped slots of a backward call -> per-pair gradient records ----
// how the NV sums of a pair land in its 12-float record: floats 0-1 mean2d, 2 opacity, 3-5 conic, 6-8 colour, 9 depth
__device__ __forceinline__ void store_pair_sums(float4* dst, const float (&acc)[ACC_VALS]) {
    dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    dst[2] = make_float4(acc[8], 0.f, 0.f, 0.f);
}
__device__ __forceinline__ void store_pair_sums(float4* dst, const float (&acc)[DACC_VALS]) {
    dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    dst[1] = make_float4(acc[4], acc[5], 0.f, 0.f);
    dst[2] = make_float4(0.f, acc[6], 0.f, 0.f);
}

// v_splats[pid] = sum over the pair's tiles of the slots stamped by this backward call, in slot order (deterministic
// given the slots).  NV sums per slot, slot stride NV + 1 with the stamp in the last float (NV = 9: colour, 7: depth).
// A workgroup owns 256 consecutive (camera, gaussian) pairs, whose slots are one contiguous range.
// The range is streamed through LDS 256 slots at a time with lane = slot (coalesced reads, no per-lane trip counts on
// the HBM side; the next 256 slots are in flight while the current ones are summed); then lane = pair adds the rows
// of its own slots in slot order.  Measured at SYNTH-1M (NV = 9): 0.26 ms, one thread per pair walking its slots 0.35 ms.
template <int NV>
__global__ __launch_bounds__(256) void k_gather_vtile(int64_t n_pairs, const int32_t* __restrict__ cum,
                                                      const float* __restrict__ vtile, int stamp, unsigned vt_cap,
                                                      float4* __restrict__ v_splats) {
    static_assert(NV & 1, "the stamp closes the slot's last 8-byte word");
    constexpr int ROW = NV;   // odd stride: rows of neighbouring slots fall into different banks
    constexpr int NQ = (NV + 1) / 2;   // 8-byte words per slot
    __shared__ int sCum[257];
    __shared__ float sVal[256 * ROW];
    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * 256;
    const int np = (int)min((int64_t)256, n_pairs - p0);
    if (tid == 0) sCum[0] = p0 == 0 ? 0 : cum[p0 - 1];
    sCum[tid + 1] = cum[p0 + min(tid, np - 1)];
    __syncthreads();
    const int s0 = sCum[0], s1 = sCum[np];
    const int my_start = sCum[tid], my_end = tid < np ? sCum[tid + 1] : sCum[tid];
    float acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.f;
    float2 q[NQ];
    auto fetch = [&](int u) {
#pragma unroll
        for (int k = 0; k < NQ; ++k) q[k] = make_float2(0.f, 0.f);   // stamp 0 = never written
        if (u < s1 && (unsigned)u < vt_cap) {   // (vt_cap: see the flush of k_blend_bwd)
            const float2* src = reinterpret_cast<const float2*>(vtile + (int64_t)u * (NV + 1));
#pragma unroll
            for (int k = 0; k < NQ; ++k) q[k] = src[k];
        }
    };
    fetch(s0 + tid);
    for (int base = s0; base < s1; base += 256) {
        const bool live = __float_as_int(q[NQ - 1].y) == stamp;
        float* row = sVal + tid * ROW;
#pragma unroll
        for (int k = 0; k < NV; ++k) row[k] = live ? ((k & 1) ? q[k >> 1].y : q[k >> 1].x) : 0.f;
        __syncthreads();
        fetch(base + 256 + tid);
        const int lo = max(my_start, base) - base, hi = min(my_end, base + 256) - base;
        for (int r = lo; r < hi; ++r) {
            const float* src = sVal + r * ROW;
#pragma unroll
            for (int k = 0; k < NV; ++k) acc[k] += src[k];
        }
        __syncthreads();
    }
    if (tid < np) store_pair_sums(v_splats + (p0 + tid) * 3, acc);
}

// ---- host set-up shared by the colour and the depth entry points ----
// 64-bit words per wave of the contribution-mask arrays (mask_base: a tile of `len` records uses at most len / 64 + 4)
static inline int64_t cmask_words(int64_t n_isects, int64_t total) { return (n_isects >> 6) + 4 * total + 8; }

// The forward -> backward hand-off scratch of the ctx: four contribution-mask arrays of `words` words and the batch
// count per tile.  allocate: the colour calls size them; !allocate: the depth backward walks what the colour forward
// of the same lists left there.
static int hand_off_buffers(st3r_ctx* ctx, int64_t total, int64_t n_isects, bool allocate, uint64_t** cmask,
                            int64_t* words, int32_t** tile_nb) {
    *words = cmask_words(n_isects, total);
    const size_t cm_bytes = sizeof(uint64_t) * 4 * (size_t)*words, nb_bytes = sizeof(int32_t) * (size_t)total;
    if (allocate) {
        void* p; int rc;
        if ((rc = st3r_arena_get(ctx, SLOT_CMASK, cm_bytes, &p)) || (rc = st3r_arena_get(ctx, SLOT_TILE_NB, nb_bytes, &p)))
            return rc;
    } else if (!ctx->slot_ptr[SLOT_CMASK] || ctx->slot_bytes[SLOT_CMASK] < cm_bytes || !ctx->slot_ptr[SLOT_TILE_NB] ||
               ctx->slot_bytes[SLOT_TILE_NB] < nb_bytes) {
        st3r_set_error("st3r_gs_blend_depth_bwd must follow st3r_gs_blend_fwd of the same lists on the same ctx");
        return ST3R_ERR_INVALID;
    }
    *cmask = (uint64_t*)ctx->slot_ptr[SLOT_CMASK];
    *tile_nb = (int32_t*)ctx->slot_ptr[SLOT_TILE_NB];
    return ST3R_OK;
}

// Per-(record, tile) partial gradients of a backward call: `stride` floats per slot, the last one a stamp.  A slot counts
// only if its stamp equals this call's, so the buffer is never cleared per call: the stamps are zeroed when the buffer is
// (re)allocated and when the counter is about to wrap -- `restarted` (either of the two, not growth alone) tells the
// caller to clear what else it stamps.
struct StampedSlots { float* vtile; int stamp; unsigned cap; bool restarted; };
static int stamped_slots(st3r_ctx* ctx, hipStream_t s, int slot, int stride, int64_t n_isects, int* stamp_counter,
                         StampedSlots* out) {
    void* p; int grown = 0;
    int rc = st3r_arena_get2(ctx, slot, sizeof(float) * stride * (size_t)n_isects, &p, &grown);
    if (rc) return rc;
    const bool restart = grown || *stamp_counter >= 2147483000;
    if (restart) {
        HIP_TRY(hipMemsetAsync(p, 0, ctx->slot_bytes[slot], s));
        *stamp_counter = 0;
    }
    *out = StampedSlots{(float*)p, ++*stamp_counter, (unsigned)(ctx->slot_bytes[slot] / (sizeof(float) * stride)), restart};
    return ST3R_OK;
}

// what every blend export checks first: the image / tile geometry and the lists.  Each export checks its own pointers
// with an ARG_CHECK of its own, so that the message names them and the export's line.
static int check_blend_args(st3r_ctx* ctx, int C, int width, int height, int tile_size, int tile_w, int tile_h,
                            const float* splats, const int32_t* offsets, const int32_t* flatten_ids, int64_t n_isects) {
    ARG_CHECK(ctx && C > 0 && width > 0 && height > 0 && tile_size == 16);
    ARG_CHECK(tile_w == (width + 15) / 16 && tile_h == (height + 15) / 16);
    ARG_CHECK(splats && offsets && n_isects >= 0 && n_isects < 2147483647LL);
    ARG_CHECK(n_isects == 0 || flatten_ids);
    return ST3R_OK;
}
