// reduce_plan.h — the arithmetic of a derived resolution level: which rows (and which bands) of
// stored level r a piece of a band of level r + k is made from (pbx_band_write_reduced).
// Device-free: plain integer functions, no context, no HIP call.  runtime.cpp runs them under
// pbx_ctx::reg_mu; scripts/reduce_plan_san.cpp and pbx_test_reduce_plan run them with no device.
//
// The rule is k_downsample's, applied k times: level j has size ((n_{j-1} + 1) / 2) per axis, and
// sample x of level j reads samples 2x and min(2x + 1, n_{j-1} - 1) of level j - 1.  The clamp
// holds at every level, so row y of level r + k depends on rows [y << k, min((y + 1) << k, n_r))
// of level r and on nothing else.
#pragma once
#include <stdint.h>

namespace pbx {

constexpr int32_t REDUCE_MAX_K = 4;

// The size of an axis k levels down.
inline int32_t reduce_size(int32_t n, int32_t k) {
    for (int32_t j = 0; j < k; j++) n = n / 2 + n % 2;  // (n + 1) / 2 without the overflow at 2^31 - 1
    return n;
}

struct ReducePlan {
    int32_t dst_sy;          // rows of level r + k
    int32_t dst_band;        // the destination band that holds the piece
    int32_t src_y0, src_y1;  // the source rows the piece reads, [src_y0, src_y1)
    int32_t band0, band1;    // the source bands that hold them, first and last
};

enum ReducePlanError : int {
    RP_OK = 0,
    RP_BAD_K = 1,       // k outside 1 .. REDUCE_MAX_K
    RP_BAD_BANDS = 2,   // a size or a band height that is not positive
    RP_BAD_ROWS = 3,    // rows outside the destination plane
    RP_CROSS_BAND = 4   // rows that leave their destination band
};

// The plan of rows [y0, y0 + rows) of level r + k, held in bands of dst_band_rows rows, from a
// level r of src_sy rows held in bands of src_band_rows rows (a dense plane: src_band_rows =
// src_sy, one band).
inline int reduce_plan(int32_t k, int32_t src_sy, int32_t src_band_rows, int32_t dst_band_rows, int32_t y0,
                       int32_t rows, ReducePlan* out) {
    if (k < 1 || k > REDUCE_MAX_K) return RP_BAD_K;
    if (src_sy <= 0 || src_band_rows <= 0 || dst_band_rows <= 0) return RP_BAD_BANDS;
    const int32_t dst_sy = reduce_size(src_sy, k);
    if (rows <= 0 || y0 < 0 || (int64_t)y0 + rows > dst_sy) return RP_BAD_ROWS;
    const int32_t band = y0 / dst_band_rows;
    if ((int64_t)y0 + rows > ((int64_t)band + 1) * dst_band_rows) return RP_CROSS_BAND;
    const int64_t s1 = ((int64_t)y0 + rows) << k;
    out->dst_sy = dst_sy;
    out->dst_band = band;
    out->src_y0 = (int32_t)((int64_t)y0 << k);  // < src_sy: y0 <= dst_sy - 1 < src_sy / 2^k
    out->src_y1 = (int32_t)(s1 < src_sy ? s1 : src_sy);
    out->band0 = out->src_y0 / src_band_rows;
    out->band1 = (out->src_y1 - 1) / src_band_rows;
    return RP_OK;
}

}  // namespace pbx
