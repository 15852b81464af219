// Hand-written LSD radix sort of (key, int32 value) pairs for gfx950: one histogram launch for all digits, then one
// "onesweep" launch per 8-bit digit (chained scan with decoupled look-back, Adinets & Merrill 2022, restated here
// for wave64 / 160 KB LDS).  Replaces cub::DeviceRadixSort::SortPairs as reached from gsplat's isect_tiles
// (starster/gs.py:76); stable, ascending, bits [begin_bit, end_bit).
#pragma once
#include "common.h"

// keys_in/vals_in are left untouched; the result lands in keys_out/vals_out.  vals may be NULL (keys only).
// n_dev (may be NULL): the item count lives in device memory -- n is then the capacity that sizes scratch and grids, and the
// first min(*n_dev, n) items are sorted.
int st3r_radix_sort_u32(st3r_ctx* ctx, hipStream_t s, int64_t n, int begin_bit, int end_bit, const uint32_t* keys_in,
                        const int32_t* vals_in, uint32_t* keys_out, int32_t* vals_out, const int32_t* n_dev);
int st3r_radix_sort_u64(st3r_ctx* ctx, hipStream_t s, int64_t n, int begin_bit, int end_bit, const uint64_t* keys_in,
                        const int32_t* vals_in, uint64_t* keys_out, int32_t* vals_out);
// n_seg segments of seg_n pairs each (the level-1 sort of the fused training calls: one segment per camera), every segment
// sorted on its own by key - krange[0] (the culled pairs' sentinel 0x1FFFFFFF by krange[1]) in krange[2] 8-bit passes -- all
// three read from device memory (written by the projection's reduction: gs_project.hip)
int st3r_radix_sort_u32_segments(st3r_ctx* ctx, hipStream_t s, int64_t seg_n, int n_seg, const uint32_t* keys_in,
                                 const int32_t* vals_in, uint32_t* keys_out, int32_t* vals_out, const uint32_t* krange);
// The host-side decisions of a sort, for st3r_front_plan (fused_step.hip): out = small shape?, items per tile, tiles,
// tiles per segment (seg_n > 0: n_seg segments of seg_n items), passes (0 for segments: decided on the device), then the
// constants RS_SMALL_BELOW and the items per tile of the small and the large shape.  Computed by the code that launches.
void st3r_radix_sort_shape(int key_bytes, int64_t n, int64_t seg_n, int n_seg, int begin_bit, int end_bit, int64_t out[8]);
// One stable pass on the low key byte inside every band of a stream that is already split by the high byte (the banded
// emission of gs_isect.hip).  band_table (device): n_bands + 1 band starts, the last one the item count, then from word ST3R_BAND_TAB
// the first sort tile of every band and the tiles in use, for tiles of st3r_radix_sort_band_tile(n_cap) items.
int st3r_radix_sort_band_tile(int64_t n_cap);
int st3r_radix_sort_u32_banded(st3r_ctx* ctx, hipStream_t s, int64_t n_cap, int n_bands, const uint32_t* band_table,
                               const uint32_t* keys_in, const int32_t* vals_in, uint32_t* keys_out, int32_t* vals_out);
// The same pass on ONE word per record, pair id | low key byte << 24 (pair ids below 2^24): ids_out receives the pair ids
// in sorted order, no keys leave.  *band_hist (device, valid until the next sort of this ctx): the records of every
// (band, low byte), from which st3r_radix_band_offsets writes offsets[k] = first sorted position of key k for k < total and
// offsets[total] = the record count -- before or after the pass, bands without a record included.
int st3r_radix_sort_u32_banded_packed(st3r_ctx* ctx, hipStream_t s, int64_t n_cap, int n_bands, const uint32_t* band_table,
                                      const uint32_t* words_in, int32_t* ids_out, const uint32_t** band_hist);
int st3r_radix_band_offsets(hipStream_t s, int n_bands, const uint32_t* band_table, const uint32_t* band_hist, int64_t total,
                            int32_t* offsets);
