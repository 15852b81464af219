// Depth maps from the splat renderer, with gradients: gsplat's render_mode "D" / "ED" next to the colour blend of
// gs_blend.hip.  Three entry points:
//   st3r_gs_blend_depth_fwd   D(p) = sum_i w_i(p) z_i over the pixel's depth-sorted records, w_i = alpha_i T_i
//   st3r_gs_blend_depth_bwd   v_D -> per-pair gradients (mean2d, opacity, conic and the depth z_i itself, float 9)
//   st3r_gs_depth_bwd         z = (R m + t)_z: the float-9 column -> means and, when asked for, camera poses
//
// The weights are the colour render's.  Both kernels evaluate the exponent with blend_power on the q-form that
// stage_qform writes (same expressions, hence the same bits) and apply the colour forward's tests (sigma >= 0,
// alpha >= 1/255, clamp 0.999); the walk of a pixel ends at last_ids[pixel], the last record the colour forward blended
// there, which replaces its saturation bookkeeping: every record behind that index either failed the tests or is the one
// that saturated the pixel (not blended).  T and alpha T are formed by the same two multiplications, so D equals, bit for
// bit, channel 0 of a colour render whose colours were overwritten with (z, 0, 0).
//
// Mapping: as gs_blend.hip, through the same functions of blend_common.h -- tile_geom (one workgroup = one 16x16 tile,
// wave w owns the 8x8 quadrant (w&1, w>>1), tiles handed to the XCDs through xcd_remap) and quadrant_relevance.  The forward
// stages 256 records per batch, 32 bytes each (x y opacity qa | qb qc z -: no colour), and walks the set bits only.
//
// Backward: k_blend_bwd's two-phase transposition with one channel whose "colour" is z_i,
//     dL/dalpha_i = (T_i z_i - S_i / (1 - alpha_i)) v_D,     S_i = depth accumulated behind record i
// (no background, no v_alpha term).  Phase 1 (lanes = pixels) leaves (alpha dL/dalpha, alpha T) per (record, pixel) in a
// wave-private LDS buffer; phase 2 (lanes = records x pixel runs) accumulates the seven sums
//     sum g {1, dx, dy, dx^2, dx dy, dy^2}  and  sum (alpha T) v_D
// (run_sums) and meets them in DPP row reductions (reduce9_rows with two idle inputs: a first version, the reduction is not
// tuned for seven values).  Per-(record, tile) results go to stamped 32-byte slots of their own (DVT_STRIDE: 7 sums + stamp;
// slot_of_rectbase / slot_of_rect, stamped_slots) and k_gather_vtile<DACC_VALS> adds a pair's slots in slot order: no
// atomics, fixed summation order, same inputs -> same bits.  It walks the contribution masks the colour forward left in
// the ctx (hand_off_buffers), like st3r_gs_blend_bwd.  What k_blend_depth_bwd still repeats of k_blend_bwd -- that kernel's
// register allocation does not survive the move into a shared function -- is marked `mirrors k_blend_bwd`.
#include <type_traits>

#include "stages.h"
#include "tile_rect.h"
#include "blend_common.h"
#include "per_view.h"   // block_sum_fixed

// q-form of record `id` in LDS slot t, two words: (x y opacity qa | qb qc z -) with qa, qb, qc formed exactly as
// stage_qform forms them; returns the 4-bit quadrant relevance
__device__ __forceinline__ int stage_record_depth(const float4* __restrict__ splats, int64_t id, int t, int tx0, int ty0,
                                                  float4* sR) {
    const float4 a = splats[id * 3 + 0];   // x y opacity conic.a
    const float4 b = splats[id * 3 + 1];   // conic.b conic.c r g
    const float z = reinterpret_cast<const float*>(splats)[id * 12 + 9];
    sR[2 * t + 0] = make_float4(a.x, a.y, a.z, -0.5f * LOG2E * a.w);
    sR[2 * t + 1] = make_float4(-LOG2E * b.x, -0.5f * LOG2E * b.y, z, 0.f);
    return quadrant_relevance(a, b, tx0, ty0);
}

__global__ __launch_bounds__(BLK) void k_blend_depth_fwd(int C, int W, int H, int tile_w, int tile_h,
                                                         const float4* __restrict__ splats,
                                                         const int32_t* __restrict__ offsets,
                                                         const int32_t* __restrict__ flat, int n_isects,
                                                         const int32_t* __restrict__ last_ids,
                                                         float* __restrict__ out_depth) {
    __shared__ float4 sR[BLK * 2];
    __shared__ uint64_t sMask[4][4];  // [quadrant][64-record chunk]
    const TileGeom g = tile_geom(C, W, H, tile_w, tile_h, offsets, n_isects);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t p = ((int64_t)g.cam * H + g.i) * W + g.j;
    // index of the last record the colour forward blended into this pixel (0 for a pixel nothing reached: record 0 then
    // fails the alpha test here as it did there); -1 outside the image
    const int last = g.inside ? last_ids[p] : -1;
    float T = 1.0f, d = 0.f;
    for (int bs = g.start; bs < g.end; bs += BLK) {
        if (__syncthreads_and(last < bs)) break;
        const int idx = bs + threadIdx.x;
        int rel = 0;
        if (idx < g.end) rel = stage_record_depth(splats, flat[idx], threadIdx.x, g.tx0, g.ty0, sR);
        const uint64_t m0 = __ballot(rel & 1), m1 = __ballot(rel & 2), m2 = __ballot(rel & 4), m3 = __ballot(rel & 8);
        if (lane == 0) { sMask[0][w] = m0; sMask[1][w] = m1; sMask[2][w] = m2; sMask[3][w] = m3; }
        __syncthreads();
#pragma unroll 1
        for (int jj = 0; jj < 4; ++jj) {
            uint64_t m64 = uniform_u64(sMask[w][jj]);
            if (__builtin_amdgcn_ballot_w64(last >= bs + jj * 64) == 0) m64 = 0;  // every pixel of this wave is done
#pragma unroll 1
            for (int hh = 0; hh < 2; ++hh) {
                uint32_t m = hh ? (uint32_t)(m64 >> 32) : (uint32_t)m64;
                while (m) {
                    const int bit = __builtin_ctz(m);
                    m &= m - 1;
                    const int t = jj * 64 + hh * 32 + bit;
                    const float4 a = sR[2 * t];
                    const float4 q = sR[2 * t + 1];
                    const float dx = a.x - g.px, dy = a.y - g.py;
                    const float P = blend_power(dx, dy, a.w, q.x, q.y);
                    const float al0 = fminf(0.999f, a.z * __builtin_amdgcn_exp2f(P));
                    const bool ok = !(P > 0.f) && !(al0 < 1.f / 255.f) && (bs + t <= last);
                    const float al = ok ? al0 : 0.f;
                    const float vis = al * T;
                    T = T * (1.0f - al);
                    d = __builtin_fmaf(q.z, vis, d);
                }
            }
        }
    }
    if (g.inside) out_depth[p] = d;
}

int st3r_blend_depth_fwd_impl(st3r_ctx* ctx, hipStream_t s, const RasterOut& ro, const int32_t* last_ids, float* depth,
                              bool end_in_offsets) {
    (void)ctx;
    hipLaunchKernelGGL(k_blend_depth_fwd, dim3(ro.C * ro.tile_w * ro.tile_h), dim3(BLK), 0, s, ro.C, ro.W, ro.H, ro.tile_w,
                       ro.tile_h, (const float4*)ro.splats, ro.offsets, ro.flat, end_in_offsets ? -1 : (int)ro.n_isects,
                       last_ids, depth);
    LAUNCH_CHECK();
    return ST3R_OK;
}

ST3R_EXPORT int st3r_gs_blend_depth_fwd(st3r_ctx* ctx, void* stream, int C, int width, int height, int tile_size,
                                        int tile_w, int tile_h, const float* splats, const int32_t* offsets,
                                        const int32_t* flatten_ids, int64_t n_isects, const float* alpha,
                                        const int32_t* last_ids, float* depth) {
    if (int rc = check_blend_args(ctx, C, width, height, tile_size, tile_w, tile_h, splats, offsets, flatten_ids, n_isects))
        return rc;
    ARG_CHECK(alpha && last_ids && depth);
    (void)alpha;   // (part of the colour render's result the call is bound to; T is rebuilt from the records)
    return st3r_blend_depth_fwd_impl(ctx, (hipStream_t)stream,
                                     stage_lists(C, width, height, tile_w, tile_h, splats, offsets, flatten_ids, n_isects),
                                     last_ids, depth, false);
}

// ------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------
// Phase 2 (see bwd_phase2 of gs_blend.hip): lane = part + 16 * record; each lane walks CHUNK pixels of one row.
__device__ __forceinline__ void depth_bwd_phase2(const float2* __restrict__ pr, unsigned tpack, int cnt, int lane,
                                                 const float4* sA, float* accw, float qxf_lane, float qyf_lane,
                                                 const float (&pvd)[CHUNK]) {
    static_assert(CHUNK == 4, "one DPP row per record of the chunk");
    const int r = lane >> 4, part = lane & 15;
    wave_lds_sync();
    const int t = (tpack >> (8 * r)) & 0xFF;  // rows >= cnt read index 0 (valid); their sums are dropped below
    const float2 mean = *reinterpret_cast<const float2*>(&sA[t]);
    const float dy = mean.y - qyf_lane;
    const float2* src = pr + r * PAIR_STRIDE + PAIR_AT(part * CHUNK);
    // index moments W_k = sum i^k g_i over the lane's pixels (i = 0 .. CHUNK-1 to the right of its first one)
    float W0 = 0.f, W1 = 0.f, W2 = 0.f, Sz = 0.f;
#pragma unroll
    for (int i = 0; i < CHUNK; ++i) {
        const float2 v = src[i];
        W0 += v.x;
        if (i == 1) { W1 = v.x; W2 = v.x; }
        if (i > 1) { W1 = fmaf((float)i, v.x, W1); W2 = fmaf((float)(i * i), v.x, W2); }
        Sz = fmaf(v.y, pvd[i], Sz);
    }
    const RunSums m = run_sums(W0, W1, W2, mean.x - qxf_lane, dy);
    float k0, k1, k2;
    reduce9_rows(m.Sx, m.Sy, m.So, m.Sxx, m.Sxy, m.Syy, Sz, 0.f, 0.f, k0, k1, k2);
    (void)k2;
    if (r < cnt && (lane & 3) == 0) {
        // bank b of the record's row -> slots: k0 -> {0,2,1,3}[b], k1 -> {4,6,5,-}[b]
        const int b = (lane >> 2) & 3;
        const int slot0 = ((b & 1) << 1) | (b >> 1);
        float* acc = accw + t * DACC_VALS;
        acc[slot0] = k0;
        if (slot0 < 3) acc[4 + slot0] = k1;
    }
    wave_lds_sync();
}

__global__ __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(8))) void k_blend_depth_bwd(
    int C, int W, int H, int tile_w, int tile_h, const float4* __restrict__ splats, const int32_t* __restrict__ offsets,
    const int32_t* __restrict__ flat, int n_isects, const float* __restrict__ out_alpha,
    const int32_t* __restrict__ last_ids, const float* __restrict__ v_depth, const uint64_t* __restrict__ cmask,
    int64_t cmask_words, const int32_t* __restrict__ tile_nb, const int32_t* __restrict__ cum,
    const uint64_t* __restrict__ rectbase, int tight, float* __restrict__ vtile, int stamp, unsigned vt_cap) {
    __shared__ float4 sA[HB];   // x y opacity qa
    __shared__ float4 sB[HB];   // qb qc z -
    __shared__ float sAccW[4][HB * DACC_VALS];            // per wave: the sums of the records it met this round
    __shared__ float2 sPair[4][CHUNK * PAIR_STRIDE];      // per wave: (g, fac) of CHUNK records x 64 pixels
    __shared__ uint64_t sClampW;                          // staged records that need the full tests (`hard` below)
    const TileGeom g = tile_geom(C, W, H, tile_w, tile_h, offsets, n_isects);
    const int nb = tile_nb[g.lb];
    if (nb == 0) return;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t p = ((int64_t)g.cam * H + g.i) * W + g.j;
    float T_final = 1.0f, vd = 0.f;
    int bin_final = -1;
    if (g.inside) {
        T_final = 1.0f - out_alpha[p];
        vd = v_depth[p];
        bin_final = last_ids[p];
    }
    float2* pr = sPair[w];
    float* accw = sAccW[w];
    float pvd[CHUNK];
    const int pbase = (lane & 15) * CHUNK;      // (phase-2 lane = part + 16 * record)
    {
        float* px = reinterpret_cast<float*>(pr);
        px[lane] = vd;
        wave_lds_sync();
#pragma unroll
        for (int i = 0; i < CHUNK; ++i) pvd[i] = px[pbase + i];
        wave_lds_sync();
    }
    const float qxf = (float)(g.tx0 + ((w & 1) << 3) + (pbase & 7)) + 0.5f;
    const float qyf_part = (float)(g.ty0 + ((w >> 1) << 3) + (pbase >> 3)) + 0.5f;
    // constants of the easy rounds' alpha test (see k_blend_bwd): 2^64 and -t' 2^64, t' = the float below 1/255
    float k_big = 0x1p64f, k_neg_thr = -__int_as_float(0x3b808080) * 0x1p64f;
    asm volatile("" : "+v"(k_big), "+v"(k_neg_thr));
    float T = T_final;
    float bv = 0.f;   // v_D times the depth blended behind the current record
    const int64_t mbase = mask_base(g.lb, g.start);
    const uint64_t* wmask = cmask + (int64_t)__builtin_amdgcn_readfirstlane(w) * cmask_words + mbase;
    uint64_t m_next = wmask[(BLK / HB) * nb - 1];
    for (int hb = (BLK / HB) * nb - 1; hb >= 0; --hb) {
        const int bs = g.start + hb * HB;
        const int bsz = min(HB, g.end - bs);
        const uint64_t m_cur = m_next;
        if (hb > 0) m_next = wmask[hb - 1];
        if (bsz <= 0) continue;   // the tail of the last forward batch may be empty (uniform over the workgroup)
        // ---- staging: one record per thread (threads 0..HB-1); a record some wave contributed to also fixes its slot
        int my_u = -1, my_cb = 0;
        float my_op = 0.f, my_ca = 0.f, my_cbb = 0.f, my_cc = 0.f;
        if ((int)threadIdx.x < bsz) {
            const int t = threadIdx.x;
            const int64_t my_id = flat[bs + t];
            const int64_t word = mbase + hb;
#pragma unroll
            for (int ww = 0; ww < 4; ++ww) my_cb |= (int)((cmask[ww * cmask_words + word] >> (t & 63)) & 1ull) << ww;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a;
            if (my_cb) {
                a = splats[my_id * 3 + 0];   // x y opacity conic.a
                b = splats[my_id * 3 + 1];   // conic.b conic.c r g
                c = splats[my_id * 3 + 2];   // b depth radius 0
                sA[t] = make_float4(a.x, a.y, a.z, -0.5f * LOG2E * a.w);
                sB[t] = make_float4(-LOG2E * b.x, -0.5f * LOG2E * b.y, c.y, 0.f);
            }
            // mirrors k_blend_bwd: the `hard` record test (records that can reach the 0.999 clamp or fail the sigma >= 0 test)
            const float det_ = a.w * b.y - b.x * b.x;
            const bool hard = my_cb && !(a.z <= 0.998f && a.w > 0.f && b.y > 0.f && det_ >= 2e-3f * (a.w * b.y));
            const uint64_t cw = __builtin_amdgcn_ballot_w64(hard);
            if (t == 0) sClampW = cw;
            if (my_cb) {
                // (fused step: `cum` scans the TIGHT rectangles the emission used -- slot base and rectangle arrive in one
                // word per pair)
                if (rectbase) {
                    my_u = slot_of_rectbase(rectbase[my_id], g.tx0, g.ty0);
                } else {
                    // mirrors k_blend_bwd: the rectangle rebuilt from the record
                    TileRect tr = ref_tile_rect(a.x, a.y, (float)__float_as_int(c.z), 16, tile_w, tile_h);
                    if (tight) tr = tight_tile_rect(tr, a.x, a.y, a.z, a.w, b.x, b.y);
                    const int cum_excl = my_id == 0 ? 0 : cum[my_id - 1];
                    my_u = slot_of_rect(cum_excl, tr.x0, tr.y0, tr.x1 - tr.x0, g.tx0, g.ty0);
                }
                my_op = a.z; my_ca = a.w; my_cbb = b.x; my_cc = b.y;
            }
        }
        __syncthreads();
        // ---- phase 1: lanes are pixels; up to CHUNK records, back to front.  The record-index bound is always tested:
        // last_ids of the stand-alone forward is a real index for every pixel.
        auto walk = [&](auto clamp_tag) {
            constexpr bool CLAMP = decltype(clamp_tag)::value;
            uint64_t m = m_cur;   // HB = 64: one mask word per round
            while (m) {
                unsigned tpack = 0;
                int cnt = 0;
#pragma unroll
                for (int k = 0; k < CHUNK; ++k) {
                    if (m) {
                        const int t = 63 - __builtin_clzll(m);
                        m &= ~(1ull << t);
                        const float4 a = sA[t];
                        const float4 q = sB[t];
                        const float dx = a.x - g.px, dy = a.y - g.py;
                        const float P = blend_power(dx, dy, a.w, q.x, q.y);
                        const float vis0 = __builtin_amdgcn_exp2f(P);
                        const float ov0 = a.z * vis0;
                        // mirrors k_blend_bwd: the phase-1 alpha test, CLAMP / easy-round forms (here always with the index bound)
                        float alpha;
                        if (CLAMP) {
                            const float al0 = fminf(0.999f, ov0);
                            uint64_t okm = mask_not_positive(P) & mask_not_less(al0, 1.f / 255.f);
                            okm &= __builtin_amdgcn_ballot_w64(bs + t <= bin_final);
                            alpha = zero_unless(okm, al0);
                        } else {
                            // step = clamp01((alpha - t') 2^64): exactly 1 for alpha >= 1/255 and exactly 0 below
                            float step;
                            asm("v_fma_f32 %0, %1, %2, %3 clamp" : "=v"(step) : "v"(ov0), "v"(k_big), "v"(k_neg_thr));
                            alpha = ov0 * step;
                            alpha = zero_unless(__builtin_amdgcn_ballot_w64(bs + t <= bin_final), alpha);
                        }
                        // a clamped alpha (opacity*vis > 0.999) passes no gradient to sigma / opacity
                        float alpha_u = alpha;
                        if (CLAMP) alpha_u = ov0 <= 0.999f ? alpha : 0.f;
                        // 1 / (1 - alpha) with one Newton step on v_rcp_f32 (1 ulp -> correctly rounded but for rare cases): the
                        // recurrence T *= ra carries every reciprocal's error through the rest of the list, and with depths
                        // that differ little z T - bv ra cancels to T_final ra -- the bare v_rcp_f32 left the median
                        // relative error of v_means2d at 4 x the division's on tied depths (tests/test_gpu_blend.py, "uneq")
                        const float om = 1.0f - alpha;
                        float ra = __builtin_amdgcn_rcpf(om);
                        ra = __builtin_fmaf(__builtin_fmaf(-om, ra, 1.0f), ra, ra);
                        const float cv = q.z * vd;   // "colour" . cotangent
                        T *= ra;
                        const float fac = alpha * T;
                        const float v_al = cv * T - bv * ra;
                        bv += cv * fac;
                        pr[k * PAIR_STRIDE + PAIR_AT(lane)] = make_float2(alpha_u * v_al, fac);
                        tpack |= (unsigned)t << (8 * k);
                        cnt = k + 1;
                    }
                }
                depth_bwd_phase2(pr, tpack, cnt, lane, sA, accw, qxf, qyf_part, pvd);
            }
        };
        const bool clamp_round = (uniform_u64(sClampW) & m_cur) != 0;
        if (clamp_round) walk(std::true_type{}); else walk(std::false_type{});
        __syncthreads();
        // ---- flush: the (at most four) wave sums of a record -> its stamped slot
        if (my_cb && (unsigned)my_u < vt_cap) {
            float acc[DACC_VALS];
#pragma unroll
            for (int k = 0; k < DACC_VALS; ++k) acc[k] = 0.f;
#pragma unroll
            for (int ww = 0; ww < 4; ++ww) {
                if (my_cb & (1 << ww)) {
#pragma unroll
                    for (int k = 0; k < DACC_VALS; ++k) acc[k] += sAccW[ww][threadIdx.x * DACC_VALS + k];
                }
            }
            // mirrors k_blend_bwd: the flush's geometric part (six sums and the record constants -> three 8-byte words)
            // v_sigma = -opacity g_o;  v_mean2d = v_sigma (a dx + b dy, b dx + c dy);  v_conic = v_sigma (dx^2/2, dx dy, dy^2/2)
            // (the six geometric sums arrive multiplied by the opacity: phase 1 hands over alpha * dL/dalpha)
            const float sx = -acc[0], sy = -acc[1];
            float2* dst = reinterpret_cast<float2*>(vtile + (int64_t)my_u * DVT_STRIDE);
            dst[0] = make_float2(my_ca * sx + my_cbb * sy, my_cbb * sx + my_cc * sy);
            dst[1] = make_float2(my_op != 0.f ? acc[2] / my_op : 0.f, -0.5f * acc[3]);
            dst[2] = make_float2(-acc[4], -0.5f * acc[5]);
            dst[3] = make_float2(acc[6], __int_as_float(stamp));
        }
    }
}

int st3r_blend_depth_bwd_impl(st3r_ctx* ctx, hipStream_t s, const RasterOut& ro, const float* alpha,
                              const int32_t* last_ids, const float* v_depth, float* v_splats, bool end_in_offsets) {
    // ro.rectbase / ro.tight (fused step): `cum` belongs to the tight rectangles of the fused emission (see k_blend_bwd)
    const int C = ro.C, tile_w = ro.tile_w, tile_h = ro.tile_h;
    const int32_t* cum = ro.cum;
    const int64_t n_isects = ro.n_isects, n_pairs = ro.n_pairs;
    if (n_isects == 0) {
        HIP_TRY(hipMemsetAsync(v_splats, 0, sizeof(float) * ST3R_SPLAT_STRIDE * (size_t)n_pairs, s));
        return ST3R_OK;
    }
    // the contribution masks and batch counts st3r_gs_blend_fwd left in the ctx
    uint64_t* cmask; int64_t words; int32_t* tile_nb;
    int rc = hand_off_buffers(ctx, C * tile_w * tile_h, n_isects, false, &cmask, &words, &tile_nb);
    if (rc) return rc;
    // stamped slots of this kernel's own (another stride than the colour backward's, another stamp counter)
    StampedSlots sl;
    rc = stamped_slots(ctx, s, SLOT_VTILE_DEPTH, DVT_STRIDE, n_isects, &ctx->depth_stamp, &sl);
    if (rc) return rc;
    hipLaunchKernelGGL(k_blend_depth_bwd, dim3(C * tile_w * tile_h), dim3(BLK), 0, s, C, ro.W, ro.H, tile_w, tile_h,
                       (const float4*)ro.splats, ro.offsets, ro.flat, end_in_offsets ? -1 : (int)n_isects, alpha, last_ids,
                       v_depth, cmask, words, tile_nb, cum, ro.rectbase, ro.tight, sl.vtile, sl.stamp, sl.cap);
    LAUNCH_CHECK();
    // floats 0-1 mean2d, 2 opacity, 3-5 conic, 9 depth; the colour floats and the padding are written as zeros
    hipLaunchKernelGGL(k_gather_vtile<DACC_VALS>, dim3(ceil_div(n_pairs, 256)), dim3(256), 0, s, n_pairs, cum, sl.vtile,
                       sl.stamp, sl.cap, (float4*)v_splats);
    LAUNCH_CHECK();
    return ST3R_OK;
}

ST3R_EXPORT int st3r_gs_blend_depth_bwd(st3r_ctx* ctx, void* stream, int C, int width, int height, int tile_size,
                                        int tile_w, int tile_h, const float* splats, const int32_t* offsets,
                                        const int32_t* flatten_ids, int64_t n_isects, const float* alpha,
                                        const int32_t* last_ids, const float* v_depth, const int32_t* cum_tiles,
                                        int64_t n_pairs, float* v_splats) {
    if (int rc = check_blend_args(ctx, C, width, height, tile_size, tile_w, tile_h, splats, offsets, flatten_ids, n_isects))
        return rc;
    ARG_CHECK(alpha && last_ids && v_depth && v_splats && cum_tiles && n_pairs >= 0);
    return st3r_blend_depth_bwd_impl(ctx, (hipStream_t)stream,
                                     stage_lists(C, width, height, tile_w, tile_h, splats, offsets, flatten_ids, n_isects,
                                                 cum_tiles, n_pairs),
                                     alpha, last_ids, v_depth, v_splats, false);
}

// a += b over the per-pair gradient records (the colour backward's and the depth backward's: float addition, the bits
// of torch's a.add_(b))
__global__ __launch_bounds__(256) void k_add_pairs(int64_t n4, float4* __restrict__ a, const float4* __restrict__ b) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 x = a[i];
        const float4 y = b[i];
        x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
        a[i] = x;
    }
}

int st3r_add_pairs_impl(hipStream_t s, int64_t n_pairs, float* a, const float* b) {
    const int64_t n4 = n_pairs * (ST3R_SPLAT_STRIDE / 4);
    if (n4 <= 0) return ST3R_OK;
    int blocks = ceil_div(n4, 256);
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(k_add_pairs, dim3(blocks), dim3(256), 0, s, n4, (float4*)a, (const float4*)b);
    LAUNCH_CHECK();
    return ST3R_OK;
}

// ------------------------------------------------------------------------------------
// depth -> parameters
// ------------------------------------------------------------------------------------
// z = (R m + t)_z.  Per visible pair (camera c, Gaussian g) with v_z = v_splats[pair, 9]:
//     v_m += R_c[2, :] v_z        v_t_c[2] += v_z        v_R_c[2, :] += v_z m
// One workgroup owns 256 Gaussians and walks the cameras in index order: a thread adds its Gaussian's camera terms in
// that order INTO grads[3g .. 3g+2]; for the poses the block sums (v_z m, v_z) of each camera in double in a fixed order
// (wave butterfly, then the four waves in order) into one partial, and one workgroup per camera adds that camera's
// partials, in a fixed order, into row 2 of its v_viewmats (the scheme of gs_pose_bwd.hip).
#define DPOSE_VALS 4   // v_R[2, 0:3], v_t[2]

__global__ __launch_bounds__(256) void k_depth_bwd(int N, int C, const float* __restrict__ means,
                                                   const float* __restrict__ viewmats,
                                                   const float* __restrict__ splats, const float* __restrict__ v_splats,
                                                   float* __restrict__ grads, double* __restrict__ part) {
    __shared__ double red[4 * DPOSE_VALS];
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    float mx = 0.f, my = 0.f, mz = 0.f;
    if (g < N) { mx = means[3 * g]; my = means[3 * g + 1]; mz = means[3 * g + 2]; }
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int c = 0; c < C; ++c) {
        const int64_t pid = (int64_t)c * N + g;
        float vz = 0.f;
        if (g < N && __float_as_int(splats[pid * 12 + 10]) > 0) vz = v_splats[pid * 12 + 9];
        const float* V = viewmats + 16 * c;
        ax = fmaf(V[8], vz, ax); ay = fmaf(V[9], vz, ay); az = fmaf(V[10], vz, az);
        if (part) {   // (uniform over the launch)
            double v[DPOSE_VALS] = {(double)vz * (double)mx, (double)vz * (double)my, (double)vz * (double)mz, (double)vz};
            __syncthreads();   // the previous camera's partial has been read
            const double sum = block_sum_fixed(v, red);
            if (threadIdx.x < DPOSE_VALS) part[((int64_t)c * gridDim.x + blockIdx.x) * DPOSE_VALS + threadIdx.x] = sum;
        }
    }
    if (g < N) { grads[3 * g] += ax; grads[3 * g + 1] += ay; grads[3 * g + 2] += az; }
}

// one workgroup per camera: its n_part partials in a fixed order, added into row 2 of v_viewmats
__global__ __launch_bounds__(256) void k_depth_bwd_finish(int n_part, const double* __restrict__ part,
                                                          float* __restrict__ v_viewmats) {
    __shared__ double red[4 * DPOSE_VALS];
    const int c = blockIdx.x;
    double v[DPOSE_VALS] = {0.0, 0.0, 0.0, 0.0};
    const double* pc = part + (int64_t)c * n_part * DPOSE_VALS;
    for (int b = threadIdx.x; b < n_part; b += blockDim.x) {
#pragma unroll
        for (int k = 0; k < DPOSE_VALS; ++k) v[k] += pc[(int64_t)b * DPOSE_VALS + k];
    }
    const double sum = block_sum_fixed(v, red);
    if (threadIdx.x < DPOSE_VALS) {
        const int k = threadIdx.x;
        float* dst = v_viewmats + 16 * c + 8 + k;
        *dst = (float)((double)*dst + sum);
    }
}

ST3R_EXPORT int st3r_gs_depth_bwd(st3r_ctx* ctx, void* stream, int N, int C, const float* means, const float* viewmats,
                                  const float* splats, const float* v_splats, float* grads, float* v_viewmats) {
    ARG_CHECK(ctx && N >= 0 && C > 0 && C <= ST3R_MAX_VIEWS);
    ARG_CHECK(means && viewmats && splats && v_splats && grads);
    hipStream_t s = (hipStream_t)stream;
    const int nb = ceil_div(N, 256);
    if (nb == 0) return ST3R_OK;
    double* part = nullptr;
    if (v_viewmats) {
        ARENA_GET(SLOT_DEPTH_PART, double, DPOSE_VALS * (size_t)nb * C, dpart);
        part = dpart;
    }
    hipLaunchKernelGGL(k_depth_bwd, dim3(nb), dim3(256), 0, s, N, C, means, viewmats, splats, v_splats, grads, part);
    LAUNCH_CHECK();
    if (v_viewmats) {
        hipLaunchKernelGGL(k_depth_bwd_finish, dim3(C), dim3(256), 0, s, nb, (const double*)part, v_viewmats);
        LAUNCH_CHECK();
    }
    return ST3R_OK;
}
