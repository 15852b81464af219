// K4: stable ascending sort of the (isect key, pair id) stream on bits [0, end_bit).
// Replaces cub::DeviceRadixSort::SortPairs as used by gsplat (starster/gs.py:76).
// The sort itself is the hand-written onesweep radix sort of radix_sort.hip; this file binds it to the 64-bit gsplat
// keys of the stage API and to the level-2 (camera, tile) keys of the fused two-level path (see gs_isect.hip; its level-1
// (camera | depth) sort and the banded forms of its level-2 sort call radix_sort.h directly; whether the banded form applies
// is decided here).
#include "stages.h"
#include "radix_sort.h"

static int st3r_sort_impl(st3r_ctx* ctx, hipStream_t s, int64_t n, int end_bit, int64_t* keys_in, int32_t* vals_in,
                          int64_t* keys_out, int32_t* vals_out) {
    if (end_bit > 64) end_bit = 64;
    // keys are non-negative (camera id in the top bits, sign clear): sort them as unsigned
    return st3r_radix_sort_u64(ctx, s, n, 0, end_bit, reinterpret_cast<const uint64_t*>(keys_in), vals_in,
                               reinterpret_cast<uint64_t*>(keys_out), vals_out);
}

// one view of one tile: the only key is 0 and the callers' end_bit = bit_length(C * tiles - 1) is 0, which the radix
// sort rejects as an empty bit range; one stable pass over bit 0 carries the pairs across in their depth order
int st3r_sort_tile_end_bit(int end_bit) { return end_bit < 1 ? 1 : end_bit; }

// 32-bit (camera, tile) keys, stable: keeps the depth order established by the first level
int st3r_sort_tile_impl(st3r_ctx* ctx, hipStream_t s, int64_t n, int end_bit, uint32_t* keys_in, int32_t* vals_in,
                        uint32_t* keys_out, int32_t* vals_out, const int32_t* n_dev) {
    return st3r_radix_sort_u32(ctx, s, n, 0, st3r_sort_tile_end_bit(end_bit), keys_in, vals_in, keys_out, vals_out, n_dev);
}

// Banded form: the emission has split the records by the high byte of their key (gs_isect.hip), one low-byte pass is left
// (radix_sort.h: st3r_radix_sort_u32_banded and its packed form, called by the fused step itself).
// Keys of at most 8 bits have one pass anyway, keys above 16 bits more than 256 bands: both keep the passes above.
int st3r_sort_tile_banded(int end_bit, int debug_flags) { return end_bit > 8 && end_bit <= 16 && !(debug_flags & 16); }

ST3R_EXPORT int st3r_gs_sort(st3r_ctx* ctx, void* stream, int64_t n_isects, int end_bit, int64_t* isect_ids,
                             int32_t* flatten_ids, int64_t* isect_ids_sorted, int32_t* flatten_ids_sorted) {
    ARG_CHECK(ctx && n_isects >= 0 && end_bit > 0);
    if (n_isects == 0) return ST3R_OK;
    ARG_CHECK(isect_ids && flatten_ids && isect_ids_sorted && flatten_ids_sorted);
    return st3r_sort_impl(ctx, (hipStream_t)stream, n_isects, end_bit, isect_ids, flatten_ids, isect_ids_sorted,
                          flatten_ids_sorted);
}

ST3R_EXPORT int st3r_radix_sort_pairs(st3r_ctx* ctx, void* stream, int key_bytes, int64_t n, int begin_bit, int end_bit,
                                      const void* keys_in, const int32_t* vals_in, void* keys_out, int32_t* vals_out) {
    ARG_CHECK(ctx && n >= 0 && (key_bytes == 4 || key_bytes == 8) && begin_bit >= 0 && end_bit > begin_bit);
    ARG_CHECK(end_bit <= 8 * key_bytes && n < 2147483647LL);
    if (n == 0) return ST3R_OK;
    ARG_CHECK(keys_in && keys_out && ((vals_in == nullptr) == (vals_out == nullptr)));
    if (key_bytes == 4)
        return st3r_radix_sort_u32(ctx, (hipStream_t)stream, n, begin_bit, end_bit, (const uint32_t*)keys_in, vals_in,
                                   (uint32_t*)keys_out, vals_out, nullptr);
    return st3r_radix_sort_u64(ctx, (hipStream_t)stream, n, begin_bit, end_bit, (const uint64_t*)keys_in, vals_in,
                               (uint64_t*)keys_out, vals_out);
}
