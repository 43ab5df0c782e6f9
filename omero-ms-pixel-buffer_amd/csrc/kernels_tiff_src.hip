// kernels_tiff_src.hip — planes loaded from TIFF / OME-TIFF segments (strips or tiles), the step
// before getTileDirect when the reference's pixels service falls back from ZarrPixelsService to
// the Bio-Formats pixel buffers over the original files (config.yaml:18).
//
//   k_tiff_lzw      one wave per strip or tile: TIFF 6.0 §13 LZW (MSB-first codes, Clear = 256,
//                   EOI = 257, first free code 258, "early change" code widths)
//   k_tiff_unpred   one wave per segment row: the inverse of Predictor = 2 (a prefix sum over
//                   the row's samples in the file's byte order, modulo 2^bits)
//   k_tiff_unpred_place   the same sums taken on the way from the decoded segment into a band of
//                   a sparse plane (pbx_band_write_tiff): read once, stored once
//   k_tiff_split_place    chunky segments of 2 .. 4 samples per pixel (RGB, RGBA): the sums with
//                   a stride of S samples and the S interleaved components scattered into S
//                   pitched planes, in one pass (registration and band writes alike)
//   k_tiff_fpunpred_place float and double segments stored with Predictor = 3 (the floating-point
//                   predictor): byte planes summed across their boundaries, interleaved into
//                   samples and stored into the pitched plane, in one pass (registration and
//                   band writes alike)
//
// Zstandard segments (Compression = 50000) go through k_zarr_zstd (kernels_zstd.hip).
// Deflate segments go through k_zarr_inflate2 and stored ones through k_zarr_copy; every kind
// is placed by k_zarr_place (kernels_zarr.hip).  A band write reads stored segments where they
// were uploaded, and with Predictor = 2 k_tiff_unpred_place stands in for k_tiff_unpred +
// k_zarr_place.
//
// LZW as LZ77 sequences.  Between two Clear codes the position of every code in the stream is
// known without decoding: code j (j = 0 right after the Clear) is 9 + [j >= 254] + [j >= 766] +
// [j >= 1790] bits wide, so lane k of a round fetches code j0 + k directly and one ballot cuts
// the round at the first Clear / EOI.  A code < 256 is a literal; a code c >= 258 names table
// entry e = c - 258 = (string of code e) + (first byte of code e + 1), whose bytes are already
// in the output at pos[e]: a match of pos[e + 1] - pos[e] + 1 bytes from there (e = j - 1, the
// KwKwK case, is the overlapping copy).  The dictionary is the array pos[] of output offsets of
// the codes since the last Clear, in LDS.  A code of the round may name an entry made earlier
// in the same round: those lengths are resolved by a scalar walk (readlane + add), and the
// round's sequences go to seq_batch (zarr_dev.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_util.h"
#include "pbx_common.h"
#include "pbx_kernels.h"
#include "zarr_dev.h"

namespace pbx {

constexpr uint32_t LZW_JMAX = 3838;   // codes between two Clears: code values end at 4095 = 257 + 3838
constexpr uint32_t LZW_WAVES = 2;     // streams (waves) per workgroup
constexpr uint32_t LZW_POS = ZR_LZ4 + ZWIN + 64 + 128;            // pos[]: 3840 words
constexpr uint32_t LZW_BYTES = LZW_POS + 4 * 3840 + 320;          // per wave (20.5 KiB: three workgroups, 6 waves, a CU)
static_assert(LZW_BYTES % 256 == 0, "the ring of every wave is 256-byte aligned");
static_assert(LZW_WAVES * LZW_BYTES <= 64 * 1024, "default dynamic LDS limit");

// bits of the codes 0 .. j - 1 after a Clear
__device__ __forceinline__ uint32_t lzw_bits_before(uint32_t j) {
    return 9 * j + (j > 254 ? j - 254 : 0u) + (j > 766 ? j - 766 : 0u) + (j > 1790 ? j - 1790 : 0u);
}

// err[]: 0, or 1 fewer bytes than dlen, 2 a code beyond the next free one, 3 a string past
// dlen (or a match before the stream's start), 4 no Clear before the table is full.
__global__ __launch_bounds__(64 * LZW_WAVES) void k_tiff_lzw(const ZStream* __restrict__ st, uint32_t n,
                                                             const uint8_t* __restrict__ src,
                                                             uint8_t* __restrict__ dst, uint32_t* __restrict__ err) {
    const uint32_t lane = threadIdx.x & 63, w = rfl(threadIdx.x >> 6);  // wave-uniform (SGPR) state
    const uint32_t si = blockIdx.x * LZW_WAVES + w;
    if (si >= n) return;
    const ZStream t = st[si];
    const uint64_t ibits = (uint64_t)rfl(t.csize) * 8;
    const uint32_t wb = w * LZW_BYTES;
    InWin win{src + t.src_off, wb + ZR_LZ4, 0, lane};
    win.load(0);
    OutRing<ZR_LZ4> o{wb, dst + t.dst_off, 0, 0, t.dlen, lane, wb + ZR_LZ4 + ZWIN};
    const uint32_t FLAG = wb + ZR_LZ4 + ZWIN + 64, POS = wb + LZW_POS;
    uint32_t q0 = 0, b0 = 0;  // byte and bit (0..7, from the MSB) of code j0
    uint32_t j0 = 0, bad = 0;
    if (lane == 0) lds32(POS) = 0;  // (a stream need not begin with a Clear)
    for (;;) {
        q0 = rfl(q0); b0 = rfl(b0); j0 = rfl(j0); o.op = rfl(o.op); o.flushed = rfl(o.flushed);
        const uint32_t op0 = o.op;
        if (op0 >= o.olen) break;
        // the window holds the round's 64 codes (<= 96 bytes) and the last one's dword
        if (q0 < win.base || q0 + 104 > win.base + ZWIN) win.load(q0);
        const uint32_t j = j0 + lane;
        const uint32_t wd = 9 + (j >= 254) + (j >= 766) + (j >= 1790);
        const uint32_t rel = b0 + lzw_bits_before(j) - lzw_bits_before(j0);  // < 8 + 64 * 12
        const bool inside = (uint64_t)q0 * 8 + rel + wd <= ibits;
        const uint32_t at = q0 - win.base + (rel >> 3);
        const uint32_t be = __builtin_bswap32(ld_u32_unaligned(zlds + win.wo + (at < ZWIN - 4 ? at : ZWIN - 4)));
        const uint32_t c = (be >> (32 - (rel & 7) - wd)) & ((1u << wd) - 1);
        // the round ends at the first Clear, EOI, end of input (taken as EOI, like a missing
        // one) or full table
        const bool full = j >= LZW_JMAX && c != 256;
        const uint64_t E = __ballot(!inside || c == 256 || c == 257 || full);
        const uint32_t f = E ? (uint32_t)__builtin_ctzll(E) : 64u;
        const bool act = lane < f;
        const uint32_t e = c - 258;  // (c >= 258) the table entry
        const bool lit = c < 256;
        const bool wrong = act && !lit && e >= j;  // not yet defined
        const bool mt = act && !lit && !wrong;
        // lengths: 1, or pos[e + 1] - pos[e] + 1; pos[e + 1] of an entry of this round is not
        // known yet: length of the code that made it + 1
        const uint32_t ec = mt ? e : 0u;
        const uint32_t pe = lds32(POS + 4 * ec), pe1 = lds32(POS + 4 * ec + 4);
        const bool dep = mt && e >= j0;
        uint32_t len = !act ? 0u : (mt && !dep) ? pe1 - pe + 1 : 1u;
        const uint32_t r = dep ? e - j0 : 0u;  // < lane
        uint64_t D = __ballot(dep);
        while (D) {
            const uint32_t k = (uint32_t)__builtin_ctzll(D);
            const uint32_t L = rdl(len, rdl(r, k)) + 1;
            len = lane == k ? L : len;
            D &= D - 1;
        }
        const uint32_t end = wave_incl_add(len, lane), st0 = end - len;
        // the codes up to the one that completes dlen (what follows it is not read: padding,
        // or a stream without EOI)
        const uint32_t rem = o.olen - op0;
        const uint64_t G = __ballot(act && end >= rem);
        const uint32_t nc = G ? (uint32_t)__builtin_ctzll(G) + 1 : f;
        if (__ballot(wrong && lane < nc)) { bad = 2; break; }
        if (nc) {
            // (the shuffle by every lane: inside the ?: only the dep lanes would run it, and it
            // reads nothing from a lane that does not)
            const uint32_t sr = (uint32_t)__shfl((int)st0, (int)r, 64);
            const uint32_t sp = dep ? op0 + sr : pe;  // the entry's bytes
            const uint32_t boff = mt ? op0 + st0 - sp : 0u;
            // the next codes' starts (pos[j0] is there already)
            lds32(lane < nc ? POS + 4 * (j + 1) : FLAG + 64) = op0 + end;
            if (!seq_batch(o, FLAG, lane, nc, lit ? 1u : 0u, mt ? len : 0u, boff, c,
                           [](uint32_t v, uint32_t, bool) -> uint32_t { return v; })) {
                bad = 3;
                break;
            }
        }
        if (rfl(o.op) >= o.olen) break;  // dlen is out: what follows (padding, no EOI) is not read
        if (f == 64) {  // a whole round of codes
            j0 += 64;
            const uint32_t adv = b0 + lzw_bits_before(j0) - lzw_bits_before(j0 - 64);
            q0 += adv >> 3;
            b0 = adv & 7;
            continue;
        }
        // lane f ended the round
        const uint32_t cf = rdl(c, f), inf = rdl((uint32_t)inside, f), fullf = rdl((uint32_t)full, f);
        if (!inf || cf == 257) break;          // EOI: op < olen is the error below
        if (fullf) { bad = 4; break; }
        const uint32_t adv = rdl(rel, f) + rdl(wd, f);  // past the Clear
        q0 += adv >> 3;
        b0 = adv & 7;
        j0 = 0;
        if (lane == 0) lds32(POS) = o.op;
    }
    if (!bad && o.op != o.olen) bad = 1;
    o.finish();
    if (lane == 0) err[si] = bad;
}

// ------------------------------------------------------------------------ un-predictor
// One wave per row of a decoded segment, UP_ROWS rows per workgroup wave: 16 bytes (16 / bpp
// samples) a lane a step, a running sum inside the lane, a wave scan of the lanes' totals and a
// carry from step to step.  Rows are the segment's own (a tile's padded width), so no carry
// crosses a tile.  Sums are taken on the samples' values (byte-swapped in and out for a
// big-endian file) and wrap modulo 2^bits.
constexpr uint32_t UP_WAVES = 4, UP_ROWS = 16;  // rows per workgroup

// One step of a row: the lane's 16 bytes wv (bytes past the row's end zero) become their running
// sums ov, continued from `carry` (the sum of the steps before, updated for the next one).
template <uint32_t BPP>
__device__ __forceinline__ void unpred_group(const uint32_t (&wv)[4], bool be, uint32_t lane, uint32_t& carry,
                                             uint32_t (&ov)[4]) {
    constexpr uint32_t NS = 16 / BPP;
    constexpr uint32_t MASK = BPP == 4 ? 0xffffffffu : (1u << (8 * (BPP & 3))) - 1;
    uint32_t s[NS];
    uint32_t run = 0;
#pragma unroll
    for (uint32_t i = 0; i < NS; i++) {
        uint32_t v;
        if (BPP == 4) {
            v = wv[i];
            v = be ? __builtin_bswap32(v) : v;
        } else if (BPP == 2) {
            v = (wv[i >> 1] >> (16 * (i & 1))) & 0xffffu;
            v = be ? ((v >> 8) | (v << 8)) & 0xffffu : v;
        } else {
            v = (wv[i >> 2] >> (8 * (i & 3))) & 0xffu;
        }
        run += v;
        s[i] = run;
    }
    const uint32_t inc = wave_incl_add(run, lane);
    const uint32_t base = carry + inc - run;
    carry += rdl(inc, 63);
    ov[0] = ov[1] = ov[2] = ov[3] = 0;
#pragma unroll
    for (uint32_t i = 0; i < NS; i++) {
        uint32_t v = (s[i] + base) & MASK;
        if (BPP == 4) {
            ov[i] = be ? __builtin_bswap32(v) : v;
        } else if (BPP == 2) {
            v = be ? ((v >> 8) | (v << 8)) & 0xffffu : v;
            ov[i >> 1] |= v << (16 * (i & 1));
        } else {
            ov[i >> 2] |= v << (8 * (i & 3));
        }
    }
}

// the lane's `have` (0 .. 16) bytes at p, the rest zero
__device__ __forceinline__ void unpred_load(const uint8_t* p, uint32_t have, uint32_t (&wv)[4]) {
    wv[0] = wv[1] = wv[2] = wv[3] = 0;
    if (have == 16) {
        __builtin_memcpy(wv, p, 16);
    } else {
#pragma unroll
        for (uint32_t b = 0; b < 16; b++)
            if (b < have) wv[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
    }
}

template <uint32_t BPP>
__device__ __forceinline__ void unpred_row(uint8_t* row, uint32_t rb, bool be, uint32_t lane) {
    uint32_t carry = 0;
    for (uint32_t k0 = 0; k0 < rb; k0 += 1024) {
        const uint32_t off = k0 + 16 * lane;
        const uint32_t have = off >= rb ? 0u : rb - off < 16 ? rb - off : 16u;  // a multiple of BPP
        uint32_t wv[4], ov[4];
        unpred_load(row + off, have, wv);
        unpred_group<BPP>(wv, be, lane, carry, ov);
        if (have == 16) {
            __builtin_memcpy(row + off, ov, 16);
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 16; b++)
                if (b < have) row[off + b] = (uint8_t)(ov[b >> 2] >> (8 * (b & 3)));
        }
    }
}

__global__ __launch_bounds__(64 * UP_WAVES) void k_tiff_unpred(const TUnpred* __restrict__ sg,
                                                               uint8_t* __restrict__ scratch) {
    const uint32_t lane = threadIdx.x & 63, w = rfl(threadIdx.x >> 6);
    const TUnpred u = sg[blockIdx.x];
    const uint32_t rows = rfl(u.rows), rb = rfl(u.row_bytes), bpp = rfl(u.bpp);
    const bool be = rfl(u.big_endian) != 0;
    const uint32_t r1 = blockIdx.y * UP_ROWS + UP_ROWS < rows ? blockIdx.y * UP_ROWS + UP_ROWS : rows;
    for (uint32_t r = blockIdx.y * UP_ROWS + w; r < r1; r += UP_WAVES) {
        uint8_t* row = scratch + u.off + (uint64_t)r * rb;
        if (bpp == 1) unpred_row<1>(row, rb, false, lane);
        else if (bpp == 2) unpred_row<2>(row, rb, be, lane);
        else unpred_row<4>(row, rb, be, lane);
    }
}

// ------------------------------------------------------------- un-predict and place (bands)
// pbx_band_write_tiff with Predictor = 2: k_tiff_unpred's geometry (a workgroup per segment and
// run of UP_ROWS segment rows, a wave per row at a time), but a row is read once at the
// segment's own pitch -- from scratch, or from the upload buffer for a stored segment -- summed
// in registers and stored straight into the plane.  The row loop is clipped, the same for the
// whole workgroup, to the run, the destination's window [y_lo, y_hi) and the plane: rows a band
// write decodes but does not keep are neither read nor summed.  Only the segment's visible width
// min(seg_w, size_x - x0) is walked: an edge tile's padding is never stored, and the sums stop
// where the plane does.  The plane's base and pitch are 256-byte aligned and a tile's x0 * bpp is
// a multiple of 16 (TileWidth is one), so every whole group is one aligned 16-byte store; the
// row's last, partial group goes byte by byte.
template <uint32_t BPP>
__device__ __forceinline__ void unpred_place_row(const uint8_t* __restrict__ row, uint8_t* __restrict__ out,
                                                 uint32_t vis, bool be, uint32_t lane) {
    uint32_t carry = 0;
    for (uint32_t k0 = 0; k0 < vis; k0 += 1024) {
        const uint32_t off = k0 + 16 * lane;
        const uint32_t have = off >= vis ? 0u : vis - off < 16 ? vis - off : 16u;  // a multiple of BPP
        uint32_t wv[4], ov[4];
        unpred_load(row + off, have, wv);
        unpred_group<BPP>(wv, be, lane, carry, ov);
        if (have == 16) {
            *(uint4*)(out + off) = make_uint4(ov[0], ov[1], ov[2], ov[3]);
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 16; b++)
                if (b < have) out[off + b] = (uint8_t)(ov[b >> 2] >> (8 * (b & 3)));
        }
    }
}

template <uint32_t BPP>
__device__ __forceinline__ void unpred_place_rows(const uint8_t* __restrict__ s, uint32_t rb, uint8_t* __restrict__ o,
                                                  int64_t pitch, int32_t r0, int32_t r1, uint32_t vis, bool be,
                                                  uint32_t lane, uint32_t w) {
    for (int32_t r = r0 + (int32_t)w; r < r1; r += (int32_t)UP_WAVES)
        unpred_place_row<BPP>(s + (uint64_t)r * rb, o + (int64_t)r * pitch, vis, be, lane);
}

__global__ __launch_bounds__(64 * UP_WAVES) void k_tiff_unpred_place(const TPlace* __restrict__ sg, TPlaceDst d,
                                                                     const uint8_t* __restrict__ scratch,
                                                                     const uint8_t* __restrict__ input) {
    const uint32_t lane = threadIdx.x & 63, w = rfl(threadIdx.x >> 6);
    const TPlace u = sg[blockIdx.x];
    const int32_t x0 = (int32_t)rfl((uint32_t)u.x0), y0 = (int32_t)rfl((uint32_t)u.y0);
    const int32_t rows = (int32_t)rfl(u.rows);
    const uint32_t rb = rfl(u.row_bytes);
    // segment rows of this run that lie in the window and in the plane
    int32_t r0 = (int32_t)(blockIdx.y * UP_ROWS), r1 = r0 + (int32_t)UP_ROWS;
    const int32_t top = d.y_lo > 0 ? d.y_lo : 0, bottom = d.y_hi < d.sy ? d.y_hi : d.sy;
    r1 = r1 < rows ? r1 : rows;
    r0 = r0 > top - y0 ? r0 : top - y0;
    r1 = r1 < bottom - y0 ? r1 : bottom - y0;
    if (r0 >= r1 || x0 >= d.sx) return;
    const uint32_t wvis = (uint32_t)(d.sx - x0) * d.bpp;
    const uint32_t vis = wvis < rb ? wvis : rb;
    const uint8_t* s = (rfl(u.from_input) ? input : scratch) + u.src;
    uint8_t* o = d.dev + (int64_t)y0 * d.pitch + (int64_t)x0 * d.bpp;
    const bool be = d.big_endian != 0;
    if (d.bpp == 1) unpred_place_rows<1>(s, rb, o, d.pitch, r0, r1, vis, false, lane, w);
    else if (d.bpp == 2) unpred_place_rows<2>(s, rb, o, d.pitch, r0, r1, vis, be, lane, w);
    else unpred_place_rows<4>(s, rb, o, d.pitch, r0, r1, vis, be, lane, w);
}

// ------------------------------------------------- split and place (SamplesPerPixel 2 .. 4)
// Chunky segments (PlanarConfiguration = 1): a row is seg_w pixels of S interleaved samples, and
// OMERO stores every sample as a channel of its own, so component s of every pixel goes to plane
// dev[s].  k_tiff_unpred_place's geometry and clipping; a lane owns 16 / BPP pixels a step: S
// consecutive 16-byte groups of the chunky row (loaded with unpred_load's guards: strips are
// unaligned and the row's tail is partial), de-interleaved in registers into S groups of 16
// bytes, one per component.  Predictor = 2 differences a sample against the same component of
// the pixel before (TIFF 6.0 section 14), so every component is a row of its own: unpred_group
// with that component's carry, S wave scans a step.  Every wanted component is then stored as
// k_tiff_unpred_place stores its one: whole groups as aligned 16-byte stores, the row's last,
// partial group byte by byte.  A step is 1024 / BPP pixels.
template <uint32_t BPP, uint32_t S>
__device__ __forceinline__ void split_place_row(const uint8_t* __restrict__ row, uint8_t* const (&out)[S],
                                                uint32_t wanted, uint32_t vis, bool pred, bool be,
                                                uint32_t lane) {
    constexpr uint32_t NP = 16 / BPP;  // pixels a lane a step
    constexpr uint32_t MASK = BPP == 4 ? 0xffffffffu : (1u << (8 * (BPP & 3))) - 1;
    uint32_t carry[S];
#pragma unroll
    for (uint32_t s = 0; s < S; s++) carry[s] = 0;
    for (uint32_t k0 = 0; k0 < vis; k0 += 1024) {
        const uint32_t off = k0 + 16 * lane;  // in a component's row
        const uint32_t have = off >= vis ? 0u : vis - off < 16 ? vis - off : 16u;  // a multiple of BPP
        const uint32_t hin = have * S;        // whole pixels of the chunky row
        uint32_t in[4 * S];
#pragma unroll
        for (uint32_t g = 0; g < S; g++) {
            uint32_t wv[4];
            const uint32_t hg = hin <= 16 * g ? 0u : hin - 16 * g < 16 ? hin - 16 * g : 16u;
            unpred_load(row + (uint64_t)off * S + 16 * g, hg, wv);
            in[4 * g] = wv[0]; in[4 * g + 1] = wv[1]; in[4 * g + 2] = wv[2]; in[4 * g + 3] = wv[3];
        }
#pragma unroll
        for (uint32_t s = 0; s < S; s++) {
            uint32_t cv[4] = {0, 0, 0, 0}, ov[4];
#pragma unroll
            for (uint32_t i = 0; i < NP; i++) {
                const uint32_t b = (i * S + s) * BPP;  // the sample's byte in the lane's chunky bytes
                const uint32_t v = BPP == 4 ? in[b >> 2] : (in[b >> 2] >> (8 * (b & 3))) & MASK;
                cv[(i * BPP) >> 2] |= v << (8 * ((i * BPP) & 3));
            }
            if (pred) {
                unpred_group<BPP>(cv, be, lane, carry[s], ov);
            } else {
                ov[0] = cv[0]; ov[1] = cv[1]; ov[2] = cv[2]; ov[3] = cv[3];
            }
            if (!((wanted >> s) & 1)) continue;
            uint8_t* o = out[s];
            if (have == 16) {
                *(uint4*)(o + off) = make_uint4(ov[0], ov[1], ov[2], ov[3]);
            } else {
#pragma unroll
                for (uint32_t b = 0; b < 16; b++)
                    if (b < have) o[off + b] = (uint8_t)(ov[b >> 2] >> (8 * (b & 3)));
            }
        }
    }
}

template <uint32_t BPP, uint32_t S>
__device__ __forceinline__ void split_place_rows(const uint8_t* __restrict__ s, uint32_t rb, const TSplitDst& d,
                                                 int32_t x0, int32_t y0, int32_t r0, int32_t r1, uint32_t vis,
                                                 uint32_t lane, uint32_t w) {
    uint32_t wanted = 0;
#pragma unroll
    for (uint32_t c = 0; c < S; c++) wanted |= d.dev[c] ? 1u << c : 0u;
    wanted = rfl(wanted);
    const bool pred = d.predictor == 2, be = BPP > 1 && d.big_endian != 0;
    for (int32_t r = r0 + (int32_t)w; r < r1; r += (int32_t)UP_WAVES) {
        uint8_t* out[S];
#pragma unroll
        for (uint32_t c = 0; c < S; c++) out[c] = d.dev[c] + (int64_t)(y0 + r) * d.pitch + (int64_t)x0 * BPP;
        split_place_row<BPP, S>(s + (uint64_t)r * rb, out, wanted, vis, pred, be, lane);
    }
}

__global__ __launch_bounds__(64 * UP_WAVES) void k_tiff_split_place(const TPlace* __restrict__ sg,
                                                                    const TSplitDst* __restrict__ dt,
                                                                    const uint8_t* __restrict__ scratch,
                                                                    const uint8_t* __restrict__ input) {
    const uint32_t lane = threadIdx.x & 63, w = rfl(threadIdx.x >> 6);
    const TPlace u = sg[blockIdx.x];
    const TSplitDst d = dt[rfl(u.pad)];
    const int32_t x0 = (int32_t)rfl((uint32_t)u.x0), y0 = (int32_t)rfl((uint32_t)u.y0);
    const int32_t rows = (int32_t)rfl(u.rows);
    const uint32_t rb = rfl(u.row_bytes), bpp = rfl(d.bpp), spp = rfl(d.spp);
    // segment rows of this run that lie in the window and in the plane
    int32_t r0 = (int32_t)(blockIdx.y * UP_ROWS), r1 = r0 + (int32_t)UP_ROWS;
    const int32_t top = d.y_lo > 0 ? d.y_lo : 0, bottom = d.y_hi < d.sy ? d.y_hi : d.sy;
    r1 = r1 < rows ? r1 : rows;
    r0 = r0 > top - y0 ? r0 : top - y0;
    r1 = r1 < bottom - y0 ? r1 : bottom - y0;
    if (r0 >= r1 || x0 >= d.sx || spp < 2 || spp > 4) return;
    // a component's visible bytes of a row: the plane's edge or the segment's
    const uint32_t wvis = (uint32_t)(d.sx - x0) * bpp, segb = rb / spp;
    const uint32_t vis = wvis < segb ? wvis : segb;
    const uint8_t* s = (rfl(u.from_input) ? input : scratch) + u.src;
    switch (bpp * 8 + spp) {  // once per workgroup
#define PBX_SPLIT(B, S) case B * 8 + S: split_place_rows<B, S>(s, rb, d, x0, y0, r0, r1, vis, lane, w); break;
        PBX_SPLIT(1, 2) PBX_SPLIT(1, 3) PBX_SPLIT(1, 4)
        PBX_SPLIT(2, 2) PBX_SPLIT(2, 3) PBX_SPLIT(2, 4)
        PBX_SPLIT(4, 2) PBX_SPLIT(4, 3) PBX_SPLIT(4, 4)
#undef PBX_SPLIT
        default: break;
    }
}

// ------------------------------------ floating-point un-predictor and place (Predictor = 3)
// Adobe TIFF Technical Note 3: a segment row of wc samples of BPP bytes is stored as BPP byte
// planes of wc bytes each, most significant bytes first whatever the file's byte order, and the
// row's BPP * wc bytes are differenced byte by byte straight across the plane boundaries.  Byte b
// (0 = MSB) of sample i is therefore the running sum, modulo 256, of the row's bytes up to
// b * wc + i: (the total of the planes before b) + (the prefix inside plane b up to i).
// k_tiff_unpred_place's geometry and clipping.  A row is walked twice by its wave: the first
// pass adds up the planes 0 .. BPP - 2 over the segment's whole width (an edge tile's padding is
// differenced too and need not be zero), one wave reduction per plane; the second walks the
// visible width only, 64 / BPP samples a lane a step: that many consecutive bytes from each of
// the BPP planes (guarded loads: strips are unaligned), unpred_group<1> on each plane with the
// plane's own carry, a 4 x 4 byte transpose with v_perm_b32 into whole samples in the file's
// byte order, and 64 bytes a lane into the plane: four aligned 16-byte stores, or word by word
// in the row's last, partial group.  A row of at most 256 visible samples (a 256 x 256 tile, the
// usual one) would leave three lanes in four idle at 16 samples a lane: it is walked at four
// samples a lane instead, one step, one or two 16-byte stores a lane.  No LDS, no scratch,
// nothing rewritten in place.
__device__ __forceinline__ void fp_transpose4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t* o) {
    // o[s] = [a.byte s, b.byte s, c.byte s, d.byte s]; perm(hi, lo, sel): bytes 0-3 of lo, 4-7 of hi
    const uint32_t ab0 = __builtin_amdgcn_perm(b, a, 0x05010400u), ab1 = __builtin_amdgcn_perm(b, a, 0x07030602u);
    const uint32_t cd0 = __builtin_amdgcn_perm(d, c, 0x05010400u), cd1 = __builtin_amdgcn_perm(d, c, 0x07030602u);
    o[0] = __builtin_amdgcn_perm(cd0, ab0, 0x05040100u);
    o[1] = __builtin_amdgcn_perm(cd0, ab0, 0x07060302u);
    o[2] = __builtin_amdgcn_perm(cd1, ab1, 0x05040100u);
    o[3] = __builtin_amdgcn_perm(cd1, ab1, 0x07060302u);
}

constexpr uint32_t FP_NARROW = 4;  // samples a lane a step where a row is at most 256 samples wide

// the lane's `have` (0 .. G) bytes at p, the rest zero
template <uint32_t G>
__device__ __forceinline__ void fp_load(const uint8_t* p, uint32_t have, uint32_t (&wv)[4]) {
    wv[0] = wv[1] = wv[2] = wv[3] = 0;
    if (have == G) {
        __builtin_memcpy(wv, p, G);
    } else {
#pragma unroll
        for (uint32_t b = 0; b < G; b++)
            if (b < have) wv[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
    }
}

// G: samples (bytes of every plane) a lane a step, 64 / BPP (64 bytes a lane out) or FP_NARROW
template <uint32_t BPP, bool BE, uint32_t G>
__device__ __forceinline__ void fp_place_row(const uint8_t* __restrict__ row, uint8_t* __restrict__ out,
                                             uint32_t wc, uint32_t nvis, uint32_t lane) {
    constexpr uint32_t PG = G == FP_NARROW ? 4 : 16;  // bytes a lane a step of the first pass
    uint32_t carry[BPP];
    carry[0] = 0;
#pragma unroll
    for (uint32_t b = 0; b + 1 < BPP; b++) {  // the total of plane b, padding included
        uint32_t acc = 0;
        for (uint32_t k0 = 0; k0 < wc; k0 += 64 * PG) {
            const uint32_t off = k0 + PG * lane;
            const uint32_t have = off >= wc ? 0u : wc - off < PG ? wc - off : PG;
            uint32_t wv[4];
            fp_load<PG>(row + (uint64_t)b * wc + off, have, wv);
#pragma unroll
            for (uint32_t j = 0; j < PG / 4; j++)
                acc += (wv[j] & 0xffu) + ((wv[j] >> 8) & 0xffu) + ((wv[j] >> 16) & 0xffu) + (wv[j] >> 24);
        }
        carry[b + 1] = carry[b] + rdl(wave_incl_add(acc, lane), 63);
    }
    for (uint32_t k0 = 0; k0 < nvis; k0 += 64 * G) {
        const uint32_t i0 = k0 + G * lane;
        const uint32_t have = i0 >= nvis ? 0u : nvis - i0 < G ? nvis - i0 : G;  // samples
        uint32_t pv[BPP][4];
#pragma unroll
        for (uint32_t b = 0; b < BPP; b++) {
            uint32_t wv[4];
            fp_load<G>(row + (uint64_t)b * wc + i0, have, wv);
            unpred_group<1>(wv, false, lane, carry[b], pv[BE ? b : BPP - 1 - b]);  // in stored byte order
        }
        uint32_t ow[G * BPP / 4];
#pragma unroll
        for (uint32_t j = 0; j < G / 4; j++) {  // samples 4 j .. 4 j + 3
            if (BPP == 4) {
                fp_transpose4(pv[0][j], pv[1][j], pv[2][j], pv[3][j], ow + 4 * j);
            } else {
                uint32_t lo[4], hi[4];
                fp_transpose4(pv[0][j], pv[1][j], pv[2][j], pv[3][j], lo);
                fp_transpose4(pv[4 % BPP][j], pv[5 % BPP][j], pv[6 % BPP][j], pv[7 % BPP][j], hi);
#pragma unroll
                for (uint32_t s = 0; s < 4; s++) {
                    ow[8 * j + 2 * s] = lo[s];
                    ow[8 * j + 2 * s + 1] = hi[s];
                }
            }
        }
        uint8_t* o = out + (uint64_t)i0 * BPP;
        if (have == G) {
#pragma unroll
            for (uint32_t q = 0; q < G * BPP / 16; q++)
                *(uint4*)(o + 16 * q) = make_uint4(ow[4 * q], ow[4 * q + 1], ow[4 * q + 2], ow[4 * q + 3]);
        } else {
#pragma unroll
            for (uint32_t q = 0; q < G * BPP / 4; q++)
                if (4 * q < have * BPP) *(uint32_t*)(o + 4 * q) = ow[q];
        }
    }
}

template <uint32_t BPP, bool BE>
__device__ __forceinline__ void fp_place_rows(const uint8_t* __restrict__ s, uint32_t rb, uint8_t* __restrict__ o,
                                              int64_t pitch, int32_t r0, int32_t r1, uint32_t nvis, uint32_t lane,
                                              uint32_t w) {
    if (nvis <= 64 * FP_NARROW) {  // one step of four samples a lane covers the row
        for (int32_t r = r0 + (int32_t)w; r < r1; r += (int32_t)UP_WAVES)
            fp_place_row<BPP, BE, FP_NARROW>(s + (uint64_t)r * rb, o + (int64_t)r * pitch, rb / BPP, nvis, lane);
    } else {
        for (int32_t r = r0 + (int32_t)w; r < r1; r += (int32_t)UP_WAVES)
            fp_place_row<BPP, BE, 64 / BPP>(s + (uint64_t)r * rb, o + (int64_t)r * pitch, rb / BPP, nvis, lane);
    }
}

__global__ __launch_bounds__(64 * UP_WAVES) void k_tiff_fpunpred_place(const TPlace* __restrict__ sg,
                                                                       const TPlaceDst* __restrict__ dt,
                                                                       const uint8_t* __restrict__ scratch,
                                                                       const uint8_t* __restrict__ input) {
    const uint32_t lane = threadIdx.x & 63, w = rfl(threadIdx.x >> 6);
    const TPlace u = sg[blockIdx.x];
    const TPlaceDst d = dt[rfl(u.pad)];
    const int32_t x0 = (int32_t)rfl((uint32_t)u.x0), y0 = (int32_t)rfl((uint32_t)u.y0);
    const int32_t rows = (int32_t)rfl(u.rows);
    const uint32_t rb = rfl(u.row_bytes), bpp = rfl(d.bpp);
    // segment rows of this run that lie in the window and in the plane
    int32_t r0 = (int32_t)(blockIdx.y * UP_ROWS), r1 = r0 + (int32_t)UP_ROWS;
    const int32_t top = d.y_lo > 0 ? d.y_lo : 0, bottom = d.y_hi < d.sy ? d.y_hi : d.sy;
    r1 = r1 < rows ? r1 : rows;
    r0 = r0 > top - y0 ? r0 : top - y0;
    r1 = r1 < bottom - y0 ? r1 : bottom - y0;
    if (r0 >= r1 || x0 >= d.sx || (bpp != 4 && bpp != 8)) return;
    const uint32_t wvis = (uint32_t)(d.sx - x0), wc = rb / bpp;
    const uint32_t nvis = wvis < wc ? wvis : wc;  // visible samples of a row
    const uint8_t* s = (rfl(u.from_input) ? input : scratch) + u.src;
    uint8_t* o = d.dev + (int64_t)y0 * d.pitch + (int64_t)x0 * bpp;
    switch (bpp * 2 + (rfl(d.big_endian) ? 1u : 0u)) {  // once per workgroup
        case 8: fp_place_rows<4, false>(s, rb, o, d.pitch, r0, r1, nvis, lane, w); break;
        case 9: fp_place_rows<4, true>(s, rb, o, d.pitch, r0, r1, nvis, lane, w); break;
        case 16: fp_place_rows<8, false>(s, rb, o, d.pitch, r0, r1, nvis, lane, w); break;
        default: fp_place_rows<8, true>(s, rb, o, d.pitch, r0, r1, nvis, lane, w); break;
    }
}

hipError_t launch_tiff_lzw(hipStream_t st, const ZStream* d_streams, uint32_t n, const uint8_t* src,
                           uint8_t* scratch, uint32_t* err) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_tiff_lzw, dim3((n + LZW_WAVES - 1) / LZW_WAVES), dim3(64 * LZW_WAVES),
                       LZW_WAVES * LZW_BYTES, st, d_streams, n, src, scratch, err);
    return hipGetLastError();
}

hipError_t launch_tiff_unpred(hipStream_t st, const TUnpred* d_segs, uint32_t n, uint32_t max_rows,
                              uint8_t* scratch) {
    if (!n || !max_rows) return hipSuccess;
    hipLaunchKernelGGL(k_tiff_unpred, dim3(n, (max_rows + UP_ROWS - 1) / UP_ROWS), dim3(64 * UP_WAVES), 0, st,
                       d_segs, scratch);
    return hipGetLastError();
}

hipError_t launch_tiff_unpred_place(hipStream_t st, const TPlace* d_segs, uint32_t n, uint32_t max_rows,
                                    const TPlaceDst& dst, const uint8_t* scratch, const uint8_t* input) {
    if (!n || !max_rows) return hipSuccess;
    hipLaunchKernelGGL(k_tiff_unpred_place, dim3(n, (max_rows + UP_ROWS - 1) / UP_ROWS), dim3(64 * UP_WAVES), 0, st,
                       d_segs, dst, scratch, input);
    return hipGetLastError();
}

hipError_t launch_tiff_fpunpred_place(hipStream_t st, const TPlace* d_segs, uint32_t n, uint32_t max_rows,
                                      const TPlaceDst* d_dst, const uint8_t* scratch, const uint8_t* input) {
    if (!n || !max_rows) return hipSuccess;
    hipLaunchKernelGGL(k_tiff_fpunpred_place, dim3(n, (max_rows + UP_ROWS - 1) / UP_ROWS), dim3(64 * UP_WAVES), 0,
                       st, d_segs, d_dst, scratch, input);
    return hipGetLastError();
}

hipError_t launch_tiff_split_place(hipStream_t st, const TPlace* d_segs, uint32_t n, uint32_t max_rows,
                                   const TSplitDst* d_dst, const uint8_t* scratch, const uint8_t* input) {
    if (!n || !max_rows) return hipSuccess;
    hipLaunchKernelGGL(k_tiff_split_place, dim3(n, (max_rows + UP_ROWS - 1) / UP_ROWS), dim3(64 * UP_WAVES), 0, st,
                       d_segs, d_dst, scratch, input);
    return hipGetLastError();
}

}  // namespace pbx
