// K4: stable ascending LSD radix sort of (key, int32 value) pairs, hand-written for gfx950.
// Replaces cub::DeviceRadixSort::SortPairs as used by gsplat's isect_tiles (starster/gs.py:76); round 1 called
// rocPRIM here.
//
// Structure ("onesweep", Adinets & Merrill 2022, restated for wave64 and 160 KB of LDS):
//   k_rs_hist        one pass over the keys: 256-bin histograms of ALL digits at once (LDS atomics; a wave whose
//                    lanes agree on a digit -- the rule for the high digits of depth / tile keys -- adds once);
//   (the exclusive scan of each histogram = global base of every bin is taken inside k_rs_pass, by every workgroup)
//   k_rs_pass        one launch per 8-bit digit.  A workgroup (16 waves; 8 for small inputs) owns a tile of 16384 (32-bit keys) or 8192
//                    (64-bit keys) consecutive items.  Ranking is wave-local and stable: wave w holds items
//                    [w*64*IPT, (w+1)*64*IPT) of the tile as IPT rows of 64 consecutive items; per row the lanes
//                    find their equals with 8 ballots (match-any: WAVE_MATCH, wave_prims.h), rank = running wave count of the digit (LDS) +
//                    number of equal lanes below.  The per-digit tile counts then travel through a chained scan with
//                    decoupled look-back: one 8-byte {flag, count} word per (tile, digit), published and polled
//                    with relaxed agent-scope atomics (flag and value in ONE word, so no fences are needed and the
//                    protocol is independent of XCD placement); tiles are handed out by an atomic ticket so that
//                    every predecessor of a running tile is itself running.  Items are regrouped by digit in LDS
//                    and leave in runs that are contiguous in the destination.
//   k_rs_hist_band / k_rs_pass<.., BAND>   the level-2 sort behind the banded emission (gs_isect.hip): the stream is already
//                    split by the high key byte, one stable low-byte pass inside every band is all that is left.
//   k_rs_pass<.., BAND, PACKED> / k_band_offsets   the same pass on one word per record (pair id | low key byte << 24): the
//                    pair ids leave bare, no key does, and the tile offsets come from the band starts and histograms.
// Traffic per pass: one read and one write of keys and values (+ 2 KB of status words per tile); packed: of one word.
#include "radix_sort.h"
#include "wave_prims.h"

namespace {

constexpr int RB = 8;
constexpr int RADIX = 1 << RB;
// Two tile shapes.  Large inputs: 1024 threads x 16 (32-bit keys) / 8 (64-bit keys) items, one workgroup per CU -- the
// per-tile costs (256 status words, the chained scan) dominate, smaller tiles measured 12-25 % slower (tools/experiments/abl3.sh).
// Small inputs (fewer than one large tile per CU: a rank's share of a view-sharded job): 512 threads x 8 / 4 items, so that
// the tiles still cover the chip.
#ifndef RS_THREADS
#define RS_THREADS 1024
#endif
#ifndef RS_SMALL_BELOW
#define RS_SMALL_BELOW 100   // large tiles needed for the large shape (1 M keys: 0.118 -> 0.098 ms; at 200 tiles the large shape wins)
#endif
constexpr int THREADS_L = RS_THREADS, THREADS_S = 512;
constexpr int HIST_THREADS = 256;
constexpr int HIST_ITEMS = 16;
constexpr int MAX_PASSES = 8;
constexpr int HIST_COPIES = 8;   // global histogram copies (workgroup b adds into copy b % 8; 32 copies measured equal)

typedef unsigned long long u64;
constexpr u64 FLAG_AGG = 1ull << 62, FLAG_INC = 2ull << 62, VALUE_MASK = (1ull << 62) - 1;

template <typename K> struct Traits;
#ifndef RS_IPT32
#define RS_IPT32 16
#endif
template <> struct Traits<uint32_t> { static constexpr int IPT = RS_IPT32, IPT_S = 8; };
template <> struct Traits<uint64_t> { static constexpr int IPT = 8, IPT_S = 4; };

// value of lane q of this lane's quad (DPP quad_perm: one VALU move, no LDS)
// value of lane q of this lane's PAIR (lanes 2k, 2k+1)
__device__ __forceinline__ uint32_t pair_lane_u32(uint32_t v, int q) {
    return q == 0 ? (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xA0, 0xf, 0xf, true)
                  : (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xF5, 0xf, 0xf, true);
}
__device__ __forceinline__ uint32_t quad_lane_u32(uint32_t v, int q) {
    switch (q) {
        case 0: return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x00, 0xf, 0xf, true);
        case 1: return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x55, 0xf, 0xf, true);
        case 2: return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xAA, 0xf, 0xf, true);
        default: return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xFF, 0xf, 0xf, true);
    }
}

// The histogram kernels keep one private copy of their WORDS counters per wave (LDS atomics of different waves never meet on
// an address): the clearing of all copies, and the flush -- the copies of the first `count` counters summed and added to dst,
// zeros skipped.  The barriers around them are the kernels'.
template <int WORDS>
__device__ __forceinline__ void hist_clear(uint32_t (*sh)[WORDS]) {
    for (int i = threadIdx.x; i < (HIST_THREADS / 64) * WORDS; i += HIST_THREADS) (&sh[0][0])[i] = 0;
}
template <int WORDS>
__device__ __forceinline__ void hist_flush(const uint32_t (*sh)[WORDS], int count, uint32_t* __restrict__ dst) {
    for (int i = threadIdx.x; i < count; i += HIST_THREADS) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < HIST_THREADS / 64; ++w) t += sh[w][i];
        if (t) atomicAdd(&dst[i], t);
    }
}

template <typename K>
__global__ __launch_bounds__(HIST_THREADS) void k_rs_hist(const K* __restrict__ keys, int64_t n, int begin_bit,
                                                          int end_bit, int passes, uint32_t* __restrict__ hist,
                                                          const int32_t* __restrict__ n_dev) {
    __shared__ uint32_t sh[HIST_THREADS / 64][MAX_PASSES * RADIX];
    if (n_dev) n = min(n, (int64_t)max(*n_dev, 0));   // the item count lives on the device; `n` is the launch capacity
    hist_clear(sh);
    __syncthreads();
    uint32_t* mine = sh[threadIdx.x >> 6];
    constexpr int CH = HIST_THREADS * HIST_ITEMS;
    for (int64_t base = (int64_t)blockIdx.x * CH; base < n; base += (int64_t)gridDim.x * CH) {
        K k[HIST_ITEMS];
#pragma unroll
        for (int i = 0; i < HIST_ITEMS; ++i) {   // all loads of the chunk in flight before the first atomic
            const int64_t idx = base + i * HIST_THREADS + threadIdx.x;
            k[i] = idx < n ? keys[idx] : K(0);
        }
#pragma unroll
        for (int i = 0; i < HIST_ITEMS; ++i) {
            if (base + i * HIST_THREADS + threadIdx.x < n) {
                for (int p = 0; p < passes; ++p) {
                    const int shift = begin_bit + RB * p;
                    const int bits = min(RB, end_bit - shift);
                    atomicAdd(&mine[p * RADIX + ((uint32_t)(k[i] >> shift) & ((1u << bits) - 1u))], 1u);
                }
            }
        }
    }
    __syncthreads();
    hist_flush(sh, passes * RADIX, hist + (blockIdx.x & (HIST_COPIES - 1)) * (MAX_PASSES * RADIX));   // copy b % HIST_COPIES: fewer adds meet on an address
}

// Segmented, biased variant of the histogram (level-1 sort of the fused training calls): segment g = blockIdx.y holds the
// items [g seg_n, (g + 1) seg_n); a key is first mapped to key - krange[0] (the sentinel 0x1FFFFFFF of a culled pair to
// krange[1]), and every segment gets its own histograms of the four digits.
__device__ __forceinline__ uint32_t seg_key(uint32_t raw, uint32_t kmin, uint32_t ktop) {
    return raw == 0x1FFFFFFFu ? ktop : raw - kmin;
}
__global__ __launch_bounds__(HIST_THREADS) void k_rs_hist_seg(const uint32_t* __restrict__ keys, int64_t seg_n,
                                                              uint32_t* __restrict__ hist,
                                                              const uint32_t* __restrict__ krange) {
    __shared__ uint32_t sh[HIST_THREADS / 64][4 * RADIX];
    const uint32_t kmin = krange[0], ktop = krange[1];
    const int passes = (int)krange[2];
    hist_clear(sh);
    __syncthreads();
    uint32_t* mine = sh[threadIdx.x >> 6];
    const uint32_t* kseg = keys + (int64_t)blockIdx.y * seg_n;
    constexpr int CH = HIST_THREADS * HIST_ITEMS;
    for (int64_t base = (int64_t)blockIdx.x * CH; base < seg_n; base += (int64_t)gridDim.x * CH) {
        uint32_t k[HIST_ITEMS];
#pragma unroll
        for (int i = 0; i < HIST_ITEMS; ++i) {
            const int64_t idx = base + i * HIST_THREADS + threadIdx.x;
            k[i] = idx < seg_n ? kseg[idx] : 0u;
        }
#pragma unroll
        for (int i = 0; i < HIST_ITEMS; ++i) {
            if (base + i * HIST_THREADS + threadIdx.x < seg_n) {
                const uint32_t kk = seg_key(k[i], kmin, ktop);
                for (int p = 0; p < passes; ++p) atomicAdd(&mine[p * RADIX + ((kk >> (RB * p)) & (RADIX - 1))], 1u);
            }
        }
    }
    __syncthreads();
    hist_flush(sh, passes * RADIX, hist + blockIdx.y * (MAX_PASSES * RADIX));
}

// SEG (level-1 sort of the fused training calls; K = uint32_t): the input is n_seg segments of seg_n items (one per camera),
// each sorted on its own -- tile t serves segment t / tiles_per_seg, the chained scan restarts at a segment's first tile --,
// the keys are biased on the way in (pass 0: seg_key), and the NUMBER of passes is read from device memory (krange[2], set
// by the projection's reduction from the depth range it saw: three when the biased keys stay below 2^24, else four): launch
// `ps` returns at once when ps >= passes, and source / destination of a pass follow from the pass count so that the last
// pass that runs writes kout / vout (kin = the caller's input, ktmp / vtmp = scratch).
// BAND (the level-2 sort behind the banded emission; K = uint32_t): the input is already split by the high key byte into
// n_bands bands of any length; band_tab holds their starts (entry n_bands = the item count) and, from word BAND_TAB on, the
// first tile of every band and the tiles in use.  A ticketed tile finds its band by a search over the first tiles (the
// table travels through LDS), the chained scan restarts at the band's first tile, hist_base + 256 band is the band's own
// low-byte histogram, and one pass on bits [0, 8) writes the caller's output.  The grid is sized for the capacity
// (n / TILE + n_bands tiles); tickets past the tiles in use return at once.
// PACKED (with BAND): the stream is ONE word per record, pair id | low key byte << 24 (k_isect_emit_b's packed form) -- the
// pass runs keys-only on that word at shift 24 and its store phase writes word & 0x00FFFFFF, the pair id, to vout.  No key
// output (the offsets come from the band histograms: k_band_offsets), no value array in LDS, no value registers.
constexpr int BAND_TAB = ST3R_BAND_TAB;
template <typename K, int THREADS, int IPT, bool SEG = false, bool BAND = false, bool PACKED = false>
__global__ __launch_bounds__(THREADS) void k_rs_pass(const K* __restrict__ kin, const int32_t* __restrict__ vin,
                                                     K* __restrict__ kout, int32_t* __restrict__ vout, int64_t n,
                                                     int shift, int bits, const uint32_t* __restrict__ hist_base,
                                                     u64* status, uint32_t* tile_counter,
                                                     const int32_t* __restrict__ n_dev, int64_t seg_n = 0,
                                                     int tiles_per_seg = 0, const uint32_t* __restrict__ krange = nullptr,
                                                     int ps = 0, K* __restrict__ ktmp = nullptr,
                                                     int32_t* __restrict__ vtmp = nullptr,
                                                     const uint32_t* __restrict__ band_tab = nullptr, int n_bands = 0) {
    static_assert(!(SEG && BAND), "one kind of segment per launch");
    static_assert(!PACKED || (BAND && sizeof(K) == 4), "the packed word is the banded tile sort's");
    if (n_dev) n = min(n, (int64_t)max(*n_dev, 0));   // count on the device, grid sized for the capacity `n`
    constexpr int TILE = THREADS * IPT, WAVES = THREADS / 64;
    uint32_t kmin = 0, ktop = 0;
    bool last_seg_pass = false;
    if constexpr (SEG) {
        const int np = (int)krange[2];
        last_seg_pass = ps == np - 1;
        if (ps >= np) return;                                   // (uniform over the launch)
        const bool to_out = ((np - 1 - ps) & 1) == 0;           // the last pass that runs writes the caller's output
        const K* src_k = ps == 0 ? kin : (to_out ? ktmp : kout);
        const int32_t* src_v = ps == 0 ? vin : (to_out ? vtmp : vout);
        K* dst_k = to_out ? kout : ktmp;
        int32_t* dst_v = to_out ? vout : vtmp;
        kin = src_k; vin = src_v; kout = dst_k; vout = dst_v;
        kmin = krange[0]; ktop = krange[1];
        shift = RB * ps; bits = RB;
    }
    __shared__ K sbuf[TILE];
    __shared__ int32_t svals[PACKED ? 1 : TILE];   // values regroup together with the keys: one trip through LDS, one store phase
    __shared__ uint32_t whist[WAVES][RADIX];
    __shared__ uint32_t lbase[RADIX];
    __shared__ uint32_t tcnt[RADIX];
    __shared__ u64 gexc[RADIX];
    __shared__ long long gofs[RADIX];
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t hsum[4];
    __shared__ uint32_t s_tile;
    __shared__ uint32_t s_btile[BAND ? BAND_TAB : 1];   // BAND: first tile of every band, [n_bands] = tiles in use
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) s_tile = atomicAdd(tile_counter, 1u);
    for (int i = tid; i < WAVES * RADIX; i += THREADS) (&whist[0][0])[i] = 0;
    if constexpr (BAND) { if (tid <= n_bands) s_btile[tid] = band_tab[BAND_TAB + tid]; }
    __syncthreads();
    const uint32_t tile = s_tile;
    uint32_t first_tile = 0;      // first tile of this tile's chain (SEG: of its segment)
    int64_t tbase, seg_base = 0;
    int tcount;
    if constexpr (SEG) {
        const uint32_t sg = tile / (uint32_t)tiles_per_seg;
        first_tile = sg * (uint32_t)tiles_per_seg;
        seg_base = (int64_t)sg * seg_n;
        const int64_t in_seg = (int64_t)(tile - first_tile) * TILE;
        tbase = seg_base + in_seg;
        tcount = (int)min((int64_t)TILE, seg_n - in_seg);
        hist_base += (size_t)sg * (MAX_PASSES * RADIX);
    } else if constexpr (BAND) {
        if (tile >= s_btile[n_bands]) return;   // a ticket past the tiles in use: uniform over the workgroup
        int lo = 0, hi = n_bands;               // the band with first tile <= tile < next first tile (empty bands have no tile)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_btile[mid] <= tile) lo = mid; else hi = mid;
        }
        first_tile = s_btile[lo];
        seg_base = (int64_t)band_tab[lo];
        const int64_t in_band = (int64_t)(tile - first_tile) * TILE;
        tbase = seg_base + in_band;
        tcount = (int)min((int64_t)TILE, (int64_t)band_tab[lo + 1] - seg_base - in_band);
        hist_base += (size_t)lo * RADIX;
    } else {
        if ((int64_t)tile * TILE >= n) return;   // (capacity launch) a ticket past the last tile: uniform over the workgroup
        tbase = (int64_t)tile * TILE;
        tcount = (int)min((int64_t)TILE, n - tbase);
    }
    const uint32_t dmask = (1u << bits) - 1u;
    const int wbase = w * 64 * IPT + lane;

    K key[IPT];
    int32_t val[IPT];
    uint32_t rank[IPT];
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
        const int li = wbase + i * 64;
        key[i] = li < tcount ? kin[tbase + li] : K(0);
        if constexpr (SEG) { if (ps == 0) key[i] = (K)seg_key((uint32_t)key[i], kmin, ktop); }
    }
    // this pass's global digit counts (the HIST_COPIES partial histograms of k_rs_hist; in flight while the keys are ranked).
    // Their exclusive scan -- the global base of every bin -- is taken by every workgroup for itself further down, next to
    // the tile-local one (round 5: it used to be a launch of one workgroup, k_rs_scan_hist, between the histogram and the
    // first pass: 4.6 us twice per step).
    uint32_t hv = 0;
    if (tid < RADIX) {
        if constexpr (SEG || BAND) hv = hist_base[tid];   // (one histogram per segment / band)
        else {
#pragma unroll
            for (int c = 0; c < HIST_COPIES; ++c) hv += hist_base[c * (MAX_PASSES * RADIX) + tid];
        }
    }
    // SEG, pass 0: the values ARE the item indices (pair ids) -- nothing is read, and the projection does not write them
    const bool iota_vals = SEG && ps == 0;
    const bool has_vals = !PACKED && (SEG || vin != nullptr);
    if (iota_vals) {
#pragma unroll
        for (int i = 0; i < IPT; ++i) val[i] = (int32_t)(tbase + wbase + i * 64);
    } else if (has_vals) {   // in flight while the keys are ranked
#pragma unroll
        for (int i = 0; i < IPT; ++i) {
            const int li = wbase + i * 64;
            val[i] = li < tcount ? vin[tbase + li] : 0;
        }
    }
    const u64 lt = (1ull << lane) - 1ull;
    uint32_t* wh = whist[w];
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
        const bool valid = wbase + i * 64 < tcount;
        const uint32_t d = (uint32_t)(key[i] >> shift) & dmask;
        WAVE_MATCH(m, valid, d, RB)
        const uint32_t below = (uint32_t)__popcll(m & lt);
        const uint32_t prev = wh[d];
        if (valid && below == 0) wh[d] = prev + (uint32_t)__popcll(m);
        rank[i] = prev + below;
    }
    __syncthreads();

    // per digit: exclusive scan over the waves (in place), tile count -> published as this tile's aggregate
    uint32_t cnt = 0;
    if (tid < RADIX) {
#pragma unroll
        for (int ww = 0; ww < WAVES; ++ww) {
            const uint32_t c = whist[ww][tid];
            whist[ww][tid] = cnt;
            cnt += c;
        }
        if (tile != first_tile)
            __hip_atomic_store(status + (size_t)tile * RADIX + tid, FLAG_AGG | (u64)cnt, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        tcnt[tid] = cnt;
    }
    // tile-local exclusive scan of the digit counts
    const uint32_t inc = wave_incl_scan(cnt);
    const uint32_t hinc = wave_incl_scan(hv);
    if (tid < RADIX && lane == 63) { wsum[w] = inc; hsum[w] = hinc; }
    __syncthreads();
    uint32_t hexc = 0;   // global base of bin `tid` (threads below RADIX)
    if (tid < RADIX) {
        uint32_t base = 0, hb = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) { base += i < w ? wsum[i] : 0u; hb += i < w ? hsum[i] : 0u; }
        lbase[tid] = base + inc - cnt;
        hexc = hb + hinc - hv;
    }
    // chained scan over the tiles, LB lanes per digit: lane j of a digit's group reads the status word of the
    // (j+1)-th predecessor, then the next LB ...; the group adds aggregates up to the nearest inclusive prefix.
    // Every thread of the workgroup takes part (RADIX * LB == THREADS), so one trip of a few hundred ns covers LB
    // predecessors instead of one.
    {
        constexpr int LB = THREADS / RADIX;
        static_assert(LB == 4 || LB == 2, "the look-back group is a DPP quad or pair");
        const int d = tid / LB, j = tid % LB;
        u64 excl = 0;
        if (tile != first_tile) {
            bool done = false;
            for (int64_t t0 = (int64_t)tile - 1; !done; t0 -= LB) {
                const int64_t t = t0 - j;
                u64 v = FLAG_INC;   // before the first tile: an inclusive prefix of zero
                if (t >= (int64_t)first_tile) {
                    const u64* pt = status + (size_t)t * RADIX + d;
                    v = __hip_atomic_load(pt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    unsigned spins = 0;
                    while ((v >> 62) == 0) {
                        __builtin_amdgcn_s_sleep(1);
                        v = __hip_atomic_load(pt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        // a predecessor always holds an earlier ticket, i.e. it is running: this bound (seconds) can
                        // only trip on a broken device or a protocol bug, and then it must be loud rather than a hang
                        if (++spins > (1u << 26)) __builtin_trap();
                    }
                }
                const uint32_t val = (uint32_t)(v & VALUE_MASK), isinc = (uint32_t)(v >> 62) == 2u;
#pragma unroll
                for (int q = 0; q < LB; ++q) {   // nearest predecessor first
                    const uint32_t vq = LB == 4 ? quad_lane_u32(val, q) : pair_lane_u32(val, q);
                    const uint32_t iq = LB == 4 ? quad_lane_u32(isinc, q) : pair_lane_u32(isinc, q);
                    if (!done) { excl += vq; done = iq != 0; }
                }
            }
        }
        if (j == 0) {
            __hip_atomic_store(status + (size_t)tile * RADIX + d, FLAG_INC | (excl + tcnt[d]), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            gexc[d] = excl;
        }
    }
    __syncthreads();
    if (tid < RADIX) gofs[tid] = (long long)((u64)hexc + gexc[tid]) - (long long)lbase[tid] + seg_base;
    __syncthreads();

    // regroup by digit in LDS, then leave in runs that are contiguous in the destination
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
        if (wbase + i * 64 < tcount) {
            const uint32_t d = (uint32_t)(key[i] >> shift) & dmask;
            const uint32_t pos = lbase[d] + wh[d] + rank[i];
            sbuf[pos] = key[i];
            if (has_vals) svals[pos] = val[i];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < IPT; ++i) {
        const int p = i * THREADS + tid;
        if (p < tcount) {
            const K k = sbuf[p];
            const uint32_t d = (uint32_t)(k >> shift) & dmask;
            const long long o = gofs[d] + p;
            if constexpr (PACKED) {
                vout[o] = (int32_t)((uint32_t)k & 0x00FFFFFFu);   // (nobody reads the tile keys either: k_band_offsets)
            } else {
                if (!(SEG && last_seg_pass)) kout[o] = k;   // (nobody reads the level-1 keys once the pairs are in order)
                if (has_vals) vout[o] = svals[p];
            }
        }
    }
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// The tile shape of a sort of n items (seg_n > 0: n_seg segments of seg_n items each, n = seg_n * n_seg), decided on the
// host here and nowhere else: sort_pairs and sort_pairs_seg launch what it says, st3r_radix_sort_shape reads it back.
struct SortShape { bool small; int64_t tile, ntiles; int tiles_per_seg; };
template <typename K>
SortShape sort_shape(int64_t n, int64_t seg_n = 0, int n_seg = 0) {
    constexpr int TILE_L = THREADS_L * Traits<K>::IPT, TILE_S = THREADS_S * Traits<K>::IPT_S;
    SortShape sh;
    sh.small = (n + TILE_L - 1) / TILE_L < RS_SMALL_BELOW;   // (with a device count: decided on the capacity)
    sh.tile = sh.small ? TILE_S : TILE_L;
    sh.tiles_per_seg = seg_n > 0 ? (int)((seg_n + sh.tile - 1) / sh.tile) : 0;
    sh.ntiles = seg_n > 0 ? (int64_t)sh.tiles_per_seg * n_seg : (n + sh.tile - 1) / sh.tile;
    return sh;
}
// The shape of the one banded pass (below): the rule above unless RS_BAND_SMALL_BELOW says otherwise.  Measured at SYNTH-1M
// (26 M records, 255 bands): see tools/experiments/README.md, round 7.
#ifndef RS_BAND_SMALL_BELOW
#define RS_BAND_SMALL_BELOW RS_SMALL_BELOW
#endif
inline SortShape band_shape(int64_t n) {
    constexpr int TILE_L = THREADS_L * Traits<uint32_t>::IPT, TILE_S = THREADS_S * Traits<uint32_t>::IPT_S;
    SortShape sh = sort_shape<uint32_t>(n);
    sh.small = (n + TILE_L - 1) / TILE_L < RS_BAND_SMALL_BELOW;
    sh.tile = sh.small ? TILE_S : TILE_L;
    return sh;
}
inline int sort_passes(int begin_bit, int end_bit) { return (end_bit - begin_bit + RB - 1) / RB; }

// The scratch of a sort in SLOT_SORT_TMP: hist_words of histograms, MAX_PASSES ticket counters (one per pass), the status words
// of the chained scans of `passes` passes over ntiles tiles and, behind this metadata, optional temporary keys and values.
// The metadata is cleared here, once per sort.
struct SortScratch { uint32_t* hist; uint32_t* counters; u64* status; void* tmp_keys; int32_t* tmp_vals; };
int sort_scratch(st3r_ctx* ctx, hipStream_t s, size_t hist_words, int passes, int64_t ntiles, size_t tmp_key_bytes,
                 size_t tmp_val_bytes, SortScratch* o) {
    const size_t hist_bytes = align256(sizeof(uint32_t) * (hist_words + MAX_PASSES));
    const size_t meta_bytes = hist_bytes + align256(sizeof(u64) * (size_t)passes * (size_t)ntiles * RADIX);
    const size_t tk_bytes = align256(tmp_key_bytes);
    ARENA_GET(SLOT_SORT_TMP, char, meta_bytes + tk_bytes + align256(tmp_val_bytes), base);
    o->hist = (uint32_t*)base;
    o->counters = o->hist + hist_words;
    o->status = (u64*)(base + hist_bytes);
    o->tmp_keys = base + meta_bytes;
    o->tmp_vals = (int32_t*)(base + meta_bytes + tk_bytes);
    HIP_TRY(hipMemsetAsync(base, 0, meta_bytes, s));
    return ST3R_OK;
}

// One launch of k_rs_pass in the tile shape `sh` says: the arguments by name (those a form does not use stay zero), the
// small or the large instantiation.  hist, status and counter are those of this pass.
template <typename K>
struct PassArgs {
    const K* kin; const int32_t* vin; K* kout; int32_t* vout;
    int64_t n; int shift, bits;
    const uint32_t* hist; u64* status; uint32_t* counter;
    const int32_t* n_dev;                                                               // count on the device
    int64_t seg_n; int tiles_per_seg; const uint32_t* krange; int ps; K* ktmp; int32_t* vtmp;   // SEG
    const uint32_t* band_tab; int n_bands;                                              // BAND
};
template <typename K, bool SEG = false, bool BAND = false, bool PACKED = false>
void launch_pass(const SortShape& sh, hipStream_t s, const PassArgs<K>& a) {
    if (sh.small)
        hipLaunchKernelGGL((k_rs_pass<K, THREADS_S, Traits<K>::IPT_S, SEG, BAND, PACKED>), dim3((unsigned)sh.ntiles),
                           dim3(THREADS_S), 0, s, a.kin, a.vin, a.kout, a.vout, a.n, a.shift, a.bits, a.hist, a.status, a.counter,
                           a.n_dev, a.seg_n, a.tiles_per_seg, a.krange, a.ps, a.ktmp, a.vtmp, a.band_tab, a.n_bands);
    else
        hipLaunchKernelGGL((k_rs_pass<K, THREADS_L, Traits<K>::IPT, SEG, BAND, PACKED>), dim3((unsigned)sh.ntiles),
                           dim3(THREADS_L), 0, s, a.kin, a.vin, a.kout, a.vout, a.n, a.shift, a.bits, a.hist, a.status, a.counter,
                           a.n_dev, a.seg_n, a.tiles_per_seg, a.krange, a.ps, a.ktmp, a.vtmp, a.band_tab, a.n_bands);
}

// n_dev != NULL: the item count lives in device memory -- `n` sizes scratch and grids, the kernels sort the first
// min(*n_dev, n) items (no host round trip between the kernel that counts the items and the sort)
template <typename K>
int sort_pairs(st3r_ctx* ctx, hipStream_t s, int64_t n, int begin_bit, int end_bit, const K* keys_in,
               const int32_t* vals_in, K* keys_out, int32_t* vals_out, const int32_t* n_dev) {
    if (n == 0) return ST3R_OK;
    if (end_bit > (int)sizeof(K) * 8) end_bit = (int)sizeof(K) * 8;
    if (begin_bit < 0 || begin_bit >= end_bit) { st3r_set_error("radix sort: empty bit range"); return ST3R_ERR_INVALID; }
    const int passes = sort_passes(begin_bit, end_bit);
    const SortShape sh = sort_shape<K>(n);
    const bool need_tmp = passes > 1;
    SortScratch sc;
    int rc = sort_scratch(ctx, s, HIST_COPIES * MAX_PASSES * RADIX, passes, sh.ntiles, need_tmp ? sizeof(K) * (size_t)n : 0,
                          need_tmp && vals_in ? sizeof(int32_t) * (size_t)n : 0, &sc);
    if (rc) return rc;
    const int hist_blocks = (int)min((int64_t)1024, (n + HIST_THREADS * HIST_ITEMS - 1) / (HIST_THREADS * HIST_ITEMS));
    hipLaunchKernelGGL(k_rs_hist<K>, dim3(hist_blocks), dim3(HIST_THREADS), 0, s, keys_in, n, begin_bit, end_bit, passes,
                       sc.hist, n_dev);
    PassArgs<K> a = {};
    a.kin = keys_in; a.vin = vals_in; a.n = n; a.n_dev = n_dev;
    for (int ps = 0; ps < passes; ++ps) {
        // the last pass writes the caller's output; before that the passes alternate between it and the scratch
        const bool to_out = ((passes - 1 - ps) & 1) == 0;
        a.kout = to_out ? keys_out : (K*)sc.tmp_keys;
        a.vout = !vals_in ? nullptr : to_out ? vals_out : sc.tmp_vals;
        a.shift = begin_bit + RB * ps;
        a.bits = min(RB, end_bit - a.shift);
        a.hist = sc.hist + ps * RADIX; a.status = sc.status + (size_t)ps * sh.ntiles * RADIX; a.counter = sc.counters + ps;
        launch_pass<K>(sh, s, a);
        a.kin = a.kout; a.vin = a.vout;
    }
    LAUNCH_CHECK();
    return ST3R_OK;
}

// n_seg segments of seg_n (key, value) pairs each, every segment sorted on its own by seg_key(key) (see k_rs_pass<.., SEG>);
// krange (device): bias, sentinel key and pass count
int sort_pairs_seg(st3r_ctx* ctx, hipStream_t s, int64_t seg_n, int n_seg, const uint32_t* keys_in, const int32_t* vals_in,
                   uint32_t* keys_out, int32_t* vals_out, const uint32_t* krange) {
    if (seg_n == 0 || n_seg == 0) return ST3R_OK;
    typedef uint32_t K;
    constexpr int PASSES = 4;   // launches; the passes that run: krange[2]
    const int64_t n = seg_n * n_seg;
    const SortShape sh = sort_shape<K>(n, seg_n, n_seg);
    SortScratch sc;
    int rc = sort_scratch(ctx, s, (size_t)n_seg * MAX_PASSES * RADIX, PASSES, sh.ntiles, sizeof(K) * (size_t)n,
                          sizeof(int32_t) * (size_t)n, &sc);
    if (rc) return rc;
    const int hist_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(1024 / n_seg, (seg_n + HIST_THREADS * HIST_ITEMS - 1) / (HIST_THREADS * HIST_ITEMS)));
    hipLaunchKernelGGL(k_rs_hist_seg, dim3(hist_blocks, n_seg), dim3(HIST_THREADS), 0, s, keys_in, seg_n, sc.hist, krange);
    PassArgs<K> a = {};
    a.kin = keys_in; a.vin = vals_in; a.kout = keys_out; a.vout = vals_out; a.n = n; a.bits = RB;
    a.seg_n = seg_n; a.tiles_per_seg = sh.tiles_per_seg; a.krange = krange; a.ktmp = (K*)sc.tmp_keys; a.vtmp = sc.tmp_vals;
    for (int ps = 0; ps < PASSES; ++ps) {
        a.ps = ps;
        a.hist = sc.hist + ps * RADIX; a.status = sc.status + (size_t)ps * sh.ntiles * RADIX; a.counter = sc.counters + ps;
        launch_pass<K, true>(sh, s, a);
    }
    LAUNCH_CHECK();
    return ST3R_OK;
}

// Low-byte histogram of every band of a banded stream: workgroup g owns the contiguous range [g per, (g + 1) per) of the
// stream (not a grid stride), walks the bands that meet it -- one or two when the bands are longer than a range -- and
// flushes 256 counters per band it saw.  hist: [n_bands][256].  shift: where the low key byte sits in a word of the stream
// (0: tile keys, 24: packed words).
__global__ __launch_bounds__(HIST_THREADS) void k_rs_hist_band(const uint32_t* __restrict__ keys, int64_t per,
                                                               const uint32_t* __restrict__ band_tab, int n_bands,
                                                               uint32_t* __restrict__ hist, int shift) {
    __shared__ uint32_t sh[HIST_THREADS / 64][RADIX];
    __shared__ uint32_t s_start[BAND_TAB];
    for (int i = threadIdx.x; i <= n_bands; i += HIST_THREADS) s_start[i] = band_tab[i];
    __syncthreads();
    const int64_t n = s_start[n_bands];
    const int64_t r0 = (int64_t)blockIdx.x * per, r1 = min(r0 + per, n);
    if (r0 >= r1) return;   // uniform
    int lo = 0, hi = n_bands;   // the last band that starts at or before r0 (empty bands in front of it are skipped below)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)s_start[mid] <= r0) lo = mid; else hi = mid;
    }
    uint32_t* mine = sh[threadIdx.x >> 6];
    constexpr int CH = HIST_THREADS * HIST_ITEMS;
    for (int b = lo; b < n_bands && (int64_t)s_start[b] < r1; ++b) {
        const int64_t a0 = max(r0, (int64_t)s_start[b]), a1 = min(r1, (int64_t)s_start[b + 1]);
        if (a0 >= a1) continue;   // uniform
        hist_clear(sh);
        __syncthreads();
        for (int64_t base = a0; base < a1; base += CH) {
            uint32_t k[HIST_ITEMS];
#pragma unroll
            for (int i = 0; i < HIST_ITEMS; ++i) {
                const int64_t idx = base + i * HIST_THREADS + threadIdx.x;
                k[i] = idx < a1 ? keys[idx] : 0u;
            }
#pragma unroll
            for (int i = 0; i < HIST_ITEMS; ++i)
                if (base + i * HIST_THREADS + threadIdx.x < a1) atomicAdd(&mine[(k[i] >> shift) & (RADIX - 1)], 1u);
        }
        __syncthreads();
        hist_flush(sh, RADIX, hist + (size_t)b * RADIX);
        __syncthreads();
    }
}

// Tile offsets of the packed banded sort, from what is known before the pass runs: offsets[b 256 + d] = start of band b +
// the records of the band whose low key byte is below d -- the first sorted position of (camera, tile) key b 256 + d.  One
// workgroup per band, empty bands included (they have no sort tile, so the pass could not write their entries);
// offsets[total] = the record count as k_band_table clamped it.
__global__ __launch_bounds__(RADIX) void k_band_offsets(const uint32_t* __restrict__ band_tab, int n_bands,
                                                        const uint32_t* __restrict__ hist, int64_t total,
                                                        int32_t* __restrict__ offsets) {
    __shared__ uint32_t s_wsum[RADIX / 64];
    const int b = blockIdx.x, d = threadIdx.x, lane = d & 63, w = d >> 6;
    const uint32_t h = hist[(size_t)b * RADIX + d];
    const uint32_t inc = wave_incl_scan(h);
    if (lane == 63) s_wsum[w] = inc;
    __syncthreads();
    uint32_t excl = inc - h;
#pragma unroll
    for (int i = 0; i < RADIX / 64; ++i) excl += i < w ? s_wsum[i] : 0u;
    const int64_t key = (int64_t)b * RADIX + d;
    if (key < total) offsets[key] = (int32_t)(band_tab[b] + excl);
    if (b == n_bands - 1 && d == 0) offsets[total] = (int32_t)band_tab[n_bands];
}

// packed_hist != NULL: the packed form (see k_rs_pass) -- keys_in holds the packed words, vals_in and keys_out are not
// used, vals_out receives the pair ids, and *packed_hist the band histograms for st3r_radix_band_offsets (valid until the
// next sort of this ctx)
int sort_pairs_banded(st3r_ctx* ctx, hipStream_t s, int64_t n, int n_bands, const uint32_t* band_tab, const uint32_t* keys_in,
                      const int32_t* vals_in, uint32_t* keys_out, int32_t* vals_out, const uint32_t** packed_hist = nullptr) {
    if (n == 0) return ST3R_OK;
    typedef uint32_t K;
    if (n_bands < 1 || n_bands > BAND_TAB - 1) { st3r_set_error("banded radix sort: 1 .. 256 bands"); return ST3R_ERR_INVALID; }
    SortShape sh = band_shape(n);
    sh.ntiles = n / sh.tile + n_bands;   // every band may end in a ragged tile
    SortScratch sc;
    int rc = sort_scratch(ctx, s, (size_t)n_bands * RADIX, 1, sh.ntiles, 0, 0, &sc);
    if (rc) return rc;
    constexpr int CH = HIST_THREADS * HIST_ITEMS;
    // (2048 ranges: with 1024 a workgroup walked eight 4096-key chunks plus the ragged ones at its band edges, one latency
    // after the other: 72 us at 26 M keys)
    const int hist_blocks = (int)std::min<int64_t>(2048, (n + CH - 1) / CH);
    const int64_t per = ((n + hist_blocks - 1) / hist_blocks + CH - 1) / CH * CH;
    const bool packed = packed_hist != nullptr;
    hipLaunchKernelGGL(k_rs_hist_band, dim3(hist_blocks), dim3(HIST_THREADS), 0, s, keys_in, per, band_tab, n_bands, sc.hist,
                       packed ? 24 : 0);
    PassArgs<K> a = {};
    a.kin = keys_in; a.vout = vals_out; a.n = n; a.bits = RB; a.hist = sc.hist; a.status = sc.status; a.counter = sc.counters;
    a.band_tab = band_tab; a.n_bands = n_bands;
    if (packed) {   // shift 24, no value input, no key output
        a.shift = 24;
        launch_pass<K, false, true, true>(sh, s, a);
        *packed_hist = sc.hist;
    } else {
        a.vin = vals_in; a.kout = keys_out;
        launch_pass<K, false, true>(sh, s, a);
    }
    LAUNCH_CHECK();
    return ST3R_OK;
}

}  // namespace

int st3r_radix_sort_band_tile(int64_t n_cap) { return (int)band_shape(n_cap).tile; }

int st3r_radix_sort_u32_banded(st3r_ctx* ctx, hipStream_t s, int64_t n_cap, int n_bands, const uint32_t* band_table,
                               const uint32_t* keys_in, const int32_t* vals_in, uint32_t* keys_out, int32_t* vals_out) {
    return sort_pairs_banded(ctx, s, n_cap, n_bands, band_table, keys_in, vals_in, keys_out, vals_out);
}

int st3r_radix_sort_u32_banded_packed(st3r_ctx* ctx, hipStream_t s, int64_t n_cap, int n_bands, const uint32_t* band_table,
                                      const uint32_t* words_in, int32_t* ids_out, const uint32_t** band_hist) {
    *band_hist = nullptr;
    return sort_pairs_banded(ctx, s, n_cap, n_bands, band_table, words_in, nullptr, nullptr, ids_out, band_hist);
}

int st3r_radix_band_offsets(hipStream_t s, int n_bands, const uint32_t* band_table, const uint32_t* band_hist, int64_t total,
                            int32_t* offsets) {
    hipLaunchKernelGGL(k_band_offsets, dim3(n_bands), dim3(RADIX), 0, s, band_table, n_bands, band_hist, total, offsets);
    LAUNCH_CHECK();
    return ST3R_OK;
}

void st3r_radix_sort_shape(int key_bytes, int64_t n, int64_t seg_n, int n_seg, int begin_bit, int end_bit, int64_t out[8]) {
    if (end_bit > 8 * key_bytes) end_bit = 8 * key_bytes;
    const SortShape sh = key_bytes == 4 ? sort_shape<uint32_t>(n, seg_n, n_seg) : sort_shape<uint64_t>(n, seg_n, n_seg);
    out[0] = sh.small ? 1 : 0; out[1] = sh.tile; out[2] = sh.ntiles; out[3] = sh.tiles_per_seg;
    out[4] = seg_n > 0 ? 0 : sort_passes(begin_bit, end_bit);   // (segments: the pass count is decided on the device)
    out[5] = RS_SMALL_BELOW;
    out[6] = key_bytes == 4 ? THREADS_S * Traits<uint32_t>::IPT_S : THREADS_S * Traits<uint64_t>::IPT_S;
    out[7] = key_bytes == 4 ? THREADS_L * Traits<uint32_t>::IPT : THREADS_L * Traits<uint64_t>::IPT;
}

int st3r_radix_sort_u32_segments(st3r_ctx* ctx, hipStream_t s, int64_t seg_n, int n_seg, const uint32_t* keys_in,
                                 const int32_t* vals_in, uint32_t* keys_out, int32_t* vals_out, const uint32_t* krange) {
    return sort_pairs_seg(ctx, s, seg_n, n_seg, keys_in, vals_in, keys_out, vals_out, krange);
}

int st3r_radix_sort_u32(st3r_ctx* ctx, hipStream_t s, int64_t n, int begin_bit, int end_bit, const uint32_t* keys_in,
                        const int32_t* vals_in, uint32_t* keys_out, int32_t* vals_out, const int32_t* n_dev) {
    return sort_pairs<uint32_t>(ctx, s, n, begin_bit, end_bit, keys_in, vals_in, keys_out, vals_out, n_dev);
}

int st3r_radix_sort_u64(st3r_ctx* ctx, hipStream_t s, int64_t n, int begin_bit, int end_bit, const uint64_t* keys_in,
                        const int32_t* vals_in, uint64_t* keys_out, int32_t* vals_out) {
    return sort_pairs<uint64_t>(ctx, s, n, begin_bit, end_bit, keys_in, vals_in, keys_out, vals_out, nullptr);
}
