// kernels_tiff_predictor.hip — TIFF Predictor = 2 (horizontal differencing, TIFF 6.0 section 14)
// for deflate-TIFF tiles of integer samples (pbx_set_tiff_predictor).  The stream of such a tile
// keeps its geometry (h rows of w*bpp big-endian bytes); sample 0 of every row is written as it
// is and sample i > 0 as (s[i] - s[i-1]) mod 2^(8 bpp), subtracted on the sample value and stored
// big-endian.  Every row of every tiled-TIFF sub-tile restarts, and the zero padding of an edge
// sub-tile is differenced like data.  Two kernels write the stream that k_lz77 then reads:
//   k_tiff_pred3  rows of whole 16-byte chunks from 16-byte aligned source rows: one wave per
//                 run of rows, in registers (no LDS, no barrier)
//   k_tiff_pred   everything else: a band of rows staged in LDS, as k_rows does
#include <hip/hip_runtime.h>

#include <mutex>

#include "dev_util.h"
#include "pbx_common.h"
#include "pbx_kernels.h"

namespace pbx {

namespace {

typedef unsigned short tp_u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t tp_sub8(uint32_t a, uint32_t b) {  // bytewise a - b mod 256
    return ((a | 0x80808080u) - (b & 0x7F7F7F7Fu)) ^ ((a ^ ~b) & 0x80808080u);
}
__device__ __forceinline__ uint32_t tp_sub16(uint32_t a, uint32_t b) {  // packed 16-bit a - b
    return __builtin_bit_cast(uint32_t, (tp_u16x2)(__builtin_bit_cast(tp_u16x2, a) - __builtin_bit_cast(tp_u16x2, b)));
}
// a - b per sample, both in the native (little-endian) domain
template <uint32_t BPP>
__device__ __forceinline__ uint32_t tp_sub(uint32_t a, uint32_t b) {
    return BPP == 1 ? tp_sub8(a, b) : BPP == 2 ? tp_sub16(a, b) : a - b;
}

// ---------------------------------------------------------------------------- fast path
// A tile's first wave is in TileDesc::rows_per_blk (blk_first is k_tiff_pred's: the sub-tiles of a
// tiled response lie in both kernels' ranges, and a tile with no wave here shares its key with
// the next one, which the search then picks).
// The previous lane's value (one DPP wave shift); lane 0 takes `first`.  All lanes active.
__device__ __forceinline__ uint32_t tp_prev_lane(uint32_t x, uint32_t first) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)first, (int)x, 0x138, 0xF, 0xF, false);  // wave_shr:1
}

constexpr uint32_t P3_NT = 256;

// One wave's run of TIFF_PRED3_RUN rows: lane l holds 16-byte chunks l and 64 + l of every row,
// the whole run loaded before the first subtraction.  The sample before a chunk's first one is
// the previous lane's last (lane 0: zero for chunk 0, lane 63's chunk-0 tail for chunk 64).
template <uint32_t G, uint32_t BPP>
__device__ __forceinline__ void p3_run(const TileDesc& d, uint32_t wi, uint32_t lane, uint8_t* __restrict__ stream) {
    constexpr uint32_t RUN = TIFF_PRED3_RUN;
    const uint32_t rb = d.rowlen, nc = rb >> 4, h = (uint32_t)d.h;
    const uint32_t r0 = __builtin_amdgcn_readfirstlane((wi - d.rows_per_blk) * RUN);
    const uint32_t r1 = __builtin_amdgcn_readfirstlane(r0 + RUN < h ? r0 + RUN : h);
    // the subtraction runs on native samples: a big-endian plane swaps in, every result swaps out
    const bool be_plane = BPP > 1 && !(d.flags & TF_SWAP);
    const uint8_t* src0 = d.plane + (int64_t)d.y * d.pitch + (int64_t)d.x * BPP;
    uint8_t* out = stream + d.out_off;
    uint4 v[RUN][G];
#pragma unroll
    for (uint32_t k = 0; k < RUN; k++) {  // unconditional loads, clamped to the run's last row
        const uint32_t r = r0 + k < r1 ? r0 + k : r1 - 1;
        const uint8_t* rp = src0 + (int64_t)r * d.pitch;
#pragma unroll
        for (uint32_t g = 0; g < G; g++) {
            const uint32_t c = 64 * g + lane;
            v[k][g] = gload16(rp + 16 * (c < nc ? c : 0u));
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < RUN; k++) {
        uint32_t carry = 0;  // the last dword of the previous group's lane 63
#pragma unroll
        for (uint32_t g = 0; g < G; g++) {
            if (r0 + k >= r1) continue;  // uniform: the run ends inside the tile's last rows
            uint4 x = v[k][g];
            if (be_plane) x = swap16(x, (int)BPP);
            const uint32_t p = tp_prev_lane(x.w, carry);
            carry = (uint32_t)__builtin_amdgcn_readlane((int)x.w, 63);
            uint4 l;  // the left neighbour of every sample of x
            if (BPP == 4) {
                l = make_uint4(p, x.x, x.y, x.z);
            } else {
                constexpr uint32_t sh = 32 - 8 * BPP;  // alignbit(hi, lo, sh): (hi << 8 BPP) | (lo >> sh)
                l = make_uint4(__builtin_amdgcn_alignbit(x.x, p, sh), __builtin_amdgcn_alignbit(x.y, x.x, sh),
                               __builtin_amdgcn_alignbit(x.z, x.y, sh), __builtin_amdgcn_alignbit(x.w, x.z, sh));
            }
            uint4 o = make_uint4(tp_sub<BPP>(x.x, l.x), tp_sub<BPP>(x.y, l.y), tp_sub<BPP>(x.z, l.z), tp_sub<BPP>(x.w, l.w));
            o = swap16(o, (int)BPP);
            const uint32_t c = 64 * g + lane;
            if (c < nc) gstore16(out + (uint64_t)(r0 + k) * rb + 16 * c, o);
        }
    }
}

template <uint32_t G>
__global__ __launch_bounds__(P3_NT) void k_tiff_pred3(const TileDesc* __restrict__ dt, uint32_t ndt,
                                                     uint32_t nwaves, uint8_t* __restrict__ stream) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wi = xcd_remap(blockIdx.x, gridDim.x) * (P3_NT / 64) +
                        __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wi >= nwaves) return;  // a whole wave: no barrier in this kernel
    const uint32_t ti = __builtin_amdgcn_readfirstlane(upper_index(ndt, wi, [&](uint32_t i) { return dt[i].rows_per_blk; }));
    const TileDesc d = dt[ti];
    switch (__builtin_amdgcn_readfirstlane((uint32_t)d.bpp)) {
    case 1: p3_run<G, 1>(d, wi, lane, stream); break;
    case 2: p3_run<G, 2>(d, wi, lane, stream); break;
    default: p3_run<G, 4>(d, wi, lane, stream); break;
    }
}

// ------------------------------------------------------------------------- general path
// One workgroup per band of TIFF_PRED_BAND rows (the band's stream bytes start and end 16-byte
// aligned).  The band's source rows go into LDS big-endian through the realigned loads, each
// behind 16 zero bytes (the left neighbour of its first sample) and with the padding of a
// tiled-TIFF edge sub-tile zeroed; after one barrier every aligned 16-byte stream word is
// assembled from the row's bytes at s and at s - bpp (16 is a multiple of bpp: a stream word
// starts on a sample).  Words that straddle a row end merge the rows they touch with byte
// masks.  Rows over ROWS_MAX_RB bytes do not fit the LDS band: their words are formed byte by
// byte from the plane.
constexpr int PG_NT = 256;

// dword i of the 16 bytes of an LDS row starting at byte s of its data (s >= -20)
__device__ __forceinline__ uint32_t pg_word4(const uint32_t* rowp, int32_t s, uint32_t i) {
    const int32_t b = s + 4 * (int32_t)i;
    const int32_t wdx = b >> 2;  // floor
    return __builtin_amdgcn_alignbit(rowp[wdx + 1], rowp[wdx], (uint32_t)(b & 3) * 8);
}
// bytes [lo, hi) of dword i (byte index within the 16-byte word) as a mask
__device__ __forceinline__ uint32_t pg_byte_mask(int32_t lo, int32_t hi, uint32_t i) {
    const int32_t a = lo - 4 * (int32_t)i, b = hi - 4 * (int32_t)i;
    const uint32_t ma = a <= 0 ? 0xFFFFFFFFu : a >= 4 ? 0u : (0xFFFFFFFFu << (8 * a));
    const uint32_t mb = b >= 4 ? 0xFFFFFFFFu : b <= 0 ? 0u : (0xFFFFFFFFu >> (8 * (4 - b)));
    return ma & mb;
}
// big-endian samples a - b of one dword (bytes in memory order)
__device__ __forceinline__ uint32_t pg_sub_be(uint32_t a, uint32_t b, uint32_t bpp) {
    if (bpp == 1) return tp_sub8(a, b);
    if (bpp == 2) return bswap16x2(tp_sub16(bswap16x2(a), bswap16x2(b)));
    return __builtin_bswap32(__builtin_bswap32(a) - __builtin_bswap32(b));
}

__global__ __launch_bounds__(PG_NT) void k_tiff_pred(const TileDesc* __restrict__ dt, uint32_t ndt,
                                                     uint8_t* __restrict__ stream) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lrow[];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const uint32_t ti = upper_index(ndt, b, [&](uint32_t i) { return dt[i].blk_first; });
    const TileDesc d = dt[ti];
    const uint32_t rowlen = d.rowlen, bpp = (uint32_t)d.bpp;
    const uint32_t r0 = (b - d.blk_first) * TIFF_PRED_BAND;
    const uint32_t nr = (uint32_t)d.h - r0 < TIFF_PRED_BAND ? (uint32_t)d.h - r0 : TIFF_PRED_BAND;
    const uint32_t o0 = r0 * rowlen, nb = nr * rowlen, nw = (nb + 15) >> 4;
    uint8_t* out = stream + d.out_off + o0;
    if (rowlen > ROWS_MAX_RB) {  // uniform: no LDS, no barrier
        TileStream ts;
        ts.init(d, nullptr);
        const uint32_t smask = bpp == 4 ? 0xFFFFFFFFu : (1u << (8 * bpp)) - 1u;
        auto sample = [&](uint32_t r, uint32_t s) {  // the value of sample s of tile row r
            uint32_t v = 0;
            for (uint32_t k = 0; k < bpp; k++) v = (v << 8) | ts.be(r, s * bpp + k);
            return v;
        };
        for (uint32_t k = tid; k < nw; k += PG_NT) {
            const uint32_t o = k << 4;
            uint32_t w[4] = {0, 0, 0, 0};
            for (uint32_t j = 0; j < 16 && o + j < nb; j += bpp) {  // one sample at a time
                const uint32_t p = o + j, q = div_rcp(p, rowlen, d.rowlen_rcp), col = p - q * rowlen;
                const uint32_t s = col >> d.lbpp;
                const uint32_t df = (sample(r0 + q, s) - (s ? sample(r0 + q, s - 1) : 0u)) & smask;
                const uint32_t be = bpp == 1 ? df : bpp == 2 ? (((df & 0xFFu) << 8) | (df >> 8)) : __builtin_bswap32(df);
                const uint32_t m0 = 0u - (uint32_t)(j < 4), m1 = 0u - (uint32_t)(j >= 4 && j < 8),
                               m2 = 0u - (uint32_t)(j >= 8 && j < 12), m3 = 0u - (uint32_t)(j >= 12);
                const uint32_t sv = be << (8 * (j & 3u));
                w[0] |= sv & m0; w[1] |= sv & m1; w[2] |= sv & m2; w[3] |= sv & m3;
            }
            gstore16(out + o, make_uint4(w[0], w[1], w[2], w[3]));
        }
        return;
    }
    const uint32_t nc = (rowlen + 15) >> 4;  // 16-byte chunks per row
    const uint32_t rw = 4 * nc + 4;           // LDS row stride in words: 16 zero bytes, then the data
    uint32_t* rows = lrow + 8 + 4;            // data of row q at rows + q * rw (32 bytes of slack in front)
    // valid bytes per row / rows (the rest is the zero padding of an edge sub-tile)
    const uint32_t vrb = d.vw ? d.vw * bpp : rowlen;
    const uint32_t vh = d.vw ? d.vh : (uint32_t)d.h;
    const bool swap = (d.flags & TF_SWAP) != 0;
    const uint8_t* src0 = d.plane + (int64_t)(d.y + r0) * d.pitch + (int64_t)d.x * bpp;
    for (uint32_t i = tid; i < nr * 4; i += PG_NT) (rows - 4)[(i >> 2) * rw + (i & 3u)] = 0;
    for (uint32_t i = tid; i < nr * nc; i += PG_NT) {
        const uint32_t q = i / nc, c = i - q * nc;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (r0 + q < vh && 16 * c < vrb) {  // (padding is never read from the plane)
            ULoad u;
            uload_issue(u, src0 + (int64_t)q * d.pitch + 16 * c);
            v = uload_finish(u);
            if (swap) v = swap16(v, (int)bpp);
            const int32_t keep = (int32_t)(vrb - 16 * c);  // valid bytes of this chunk
            if (keep < 16)
                v = make_uint4(v.x & pg_byte_mask(0, keep, 0), v.y & pg_byte_mask(0, keep, 1),
                               v.z & pg_byte_mask(0, keep, 2), v.w & pg_byte_mask(0, keep, 3));
        }
        *(uint4*)(rows + q * rw + 4 * c) = v;
    }
    __syncthreads();
    for (uint32_t k = tid; k < nw; k += PG_NT) {
        const uint32_t o = k << 4;
        uint32_t r = div_rcp(o, rowlen, d.rowlen_rcp);
        int32_t s = (int32_t)(o - r * rowlen);  // byte of row r at word byte 0
        const int32_t end = (int32_t)(nb - o) < 16 ? (int32_t)(nb - o) : 16;
        uint32_t w[4] = {0, 0, 0, 0};
        int32_t filled = 0;
        while (filled < end) {  // every row the word touches (one, unless it straddles a row end)
            const uint32_t* rp = rows + r * rw;
            const int32_t hi = (int32_t)rowlen - s < end ? (int32_t)rowlen - s : end;
#pragma unroll
            for (uint32_t i = 0; i < 4; i++)
                w[i] |= pg_sub_be(pg_word4(rp, s, i), pg_word4(rp, s - (int32_t)bpp, i), bpp) & pg_byte_mask(filled, hi, i);
            filled = hi;
            s -= (int32_t)rowlen;
            r++;
        }
        gstore16(out + o, make_uint4(w[0], w[1], w[2], w[3]));
    }
}

}  // namespace

uint32_t tiff_pred3_run_rows() { return TIFF_PRED3_RUN; }

size_t tiff_pred_lds_bytes(uint32_t rb) {
    return 48 + (size_t)TIFF_PRED_BAND * (4 * ((rb + 15) / 16) + 4) * 4 + 32;
}

hipError_t launch_tiff_pred3(hipStream_t st, const TileDesc* d_tiles, uint32_t ntiles, uint32_t nwaves,
                             uint32_t max_rb, uint8_t* stream) {
    if (!ntiles || !nwaves) return hipSuccess;
    if (max_rb > filter3_max_rb()) return hipErrorInvalidValue;
    const uint32_t blocks = (nwaves + P3_NT / 64 - 1) / (P3_NT / 64);
    if (max_rb <= 1024)
        hipLaunchKernelGGL((k_tiff_pred3<1>), dim3(blocks), dim3(P3_NT), 0, st, d_tiles, ntiles, nwaves, stream);
    else
        hipLaunchKernelGGL((k_tiff_pred3<2>), dim3(blocks), dim3(P3_NT), 0, st, d_tiles, ntiles, nwaves, stream);
    return hipGetLastError();
}

hipError_t launch_tiff_pred(hipStream_t st, const TileDesc* d_tiles, uint32_t ntiles, uint32_t nblocks,
                            uint32_t max_rb, uint8_t* stream) {
    if (!ntiles || !nblocks) return hipSuccess;
    if (max_rb > ROWS_MAX_RB) return hipErrorInvalidValue;  // (wider rows take the LDS-free branch: not counted)
    const size_t lds = tiff_pred_lds_bytes(max_rb);
    if (lds > 64 * 1024) {  // bands of rows over 4 KiB: up to 160 KiB of LDS, raised once per device
        constexpr int kMaxDev = 64;
        static std::once_flag once[kMaxDev];
        static hipError_t res[kMaxDev];
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev < 0 || dev >= kMaxDev) return hipErrorInvalidDevice;
        std::call_once(once[dev], [&] {
            res[dev] = hipFuncSetAttribute((const void*)k_tiff_pred, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           160 * 1024);
        });
        if (res[dev] != hipSuccess) return res[dev];
    }
    hipLaunchKernelGGL(k_tiff_pred, dim3(nblocks), dim3(PG_NT), lds, st, d_tiles, ntiles, stream);
    return hipGetLastError();
}

}  // namespace pbx
