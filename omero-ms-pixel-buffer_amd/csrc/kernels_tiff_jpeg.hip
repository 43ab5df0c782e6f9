// kernels_tiff_jpeg.hip — JPEG-compressed TIFF segments (Compression = 7: baseline sequential
// Huffman streams of 8-bit samples; DESIGN.md §10b "JPEG segments").  The host has read the
// marker segments (tiff_jpeg_plan, runtime.cpp): every byte of entropy-coded data is decoded here.
//
//   k_tiff_jpeg_decode  one wave per stream (strip or tile): entropy decode, dequantisation and
//                       the accurate integer inverse DCT ("islow"), into one 8-bit sample plane
//                       per component in scratch, each at the component's own resolution with
//                       rows and columns padded to whole MCUs
//   k_tiff_jpeg_place   "fancy" (triangle) chroma upsampling, YCbCr -> RGB, split and placement
//                       into the pitched planes in one pass (registration and band writes alike)
//
// The arithmetic is that of the libjpeg 6b lineage (jidctint.c, jdsample.c, jdcolor.c), integer
// throughout, so decoded planes are equal byte for byte to libjpeg-turbo's as long as no IDCT
// sample leaves [-512, 511] before the clamp (there libjpeg's own builds disagree: the C code
// wraps through a table of 1024 entries, the SIMD code saturates; this kernel clamps).
//
// k_tiff_jpeg_decode, per wave, in LDS: the stream's table set (JTabSet: three de-zigzagged
// quantisers, six Huffman decode tables), a buffer of "clean" entropy bytes, and the
// coefficients of a batch of up to 64 blocks.
//   Clean bytes.  64 raw bytes a round, one per lane (guarded: index < the stream's bytes, so no
//   read leaves the stream), each lane with the byte before and after its own: a zero after FF is
//   stuffing, FF before FF or before a marker code is a fill or prefix byte, FF before 00 is data.
//   One ballot finds the round's first marker code, a second (and a popcount of the lanes below)
//   compacts the kept bytes before it into the buffer.  The refill never passes a marker: it
//   records the code (`pend`) and stops, so a restart marker is checked exactly where the decoder
//   stands when an interval ends, and bits asked for past any other marker are an error.
//   Stream state.  A 64-bit bit buffer filled 32 bits at a time from the clean bytes, the DC
//   predictors, the restart countdown and the MCU index are wave-uniform (SGPRs).  A symbol is one
//   9-bit lookup (lut[peek] = length << 8 | symbol), or for longer codes libjpeg's maxcode /
//   valoff walk from 10 bits up.
//   Batch.  Whole MCUs of up to 64 blocks: the serial loop writes each non-zero coefficient (as
//   decoded, int16, in zigzag position) into the block's 132-byte slot (33 dwords: lane-per-block
//   reads fall on 32 different banks); then lane b dequantises and transforms block b entirely in
//   registers (both passes unrolled, zigzag positions compile-time constants) and stores its 8 x 8
//   samples as eight 8-byte rows.  No coefficient goes through HBM.
//   Bounds.  A block's destination follows from its index g < mcux * mcuy * blocks_per_mcu alone:
//   component, MCU and position inside the MCU, i.e. a whole 8 x 8 block inside the component's
//   plane of (mcuy * v * 8) rows of pitch >= mcux * h * 8, which is what the host sized.  Nothing
//   the stream says moves a write.  LDS: coefficient index k <= 63 is checked before the store,
//   the clean buffer is read at min(position, its last dword), written below J_CAP + 64 + J_PAD
//   (at most J_CAP clean bytes, then J_PAD zeros, so that what a block of a cut-short stream
//   reads past the end is zeros in every run and the error it ends in is the same).
//
// err[]: 0, or 1 entropy data ends before the last MCU, 2 a code that is in no table, 3 a run
// that passes coefficient 63, 4 a DC size > 11 or an AC size > 10, 5 a restart marker that is
// missing, out of sequence or misplaced.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_util.h"
#include "pbx_common.h"
#include "pbx_kernels.h"
#include "zarr_dev.h"

namespace pbx {

constexpr uint32_t J_TAB = 0;                          // JTabSet
constexpr uint32_t J_TABSZ = (sizeof(JTabSet) + 255) & ~255u;
constexpr uint32_t J_CLEAN = J_TAB + J_TABSZ;          // clean entropy bytes
constexpr uint32_t J_CAP = 1024;                       // refilled up to here
constexpr uint32_t J_PAD = 320;                        // zeros kept after the clean bytes
constexpr uint32_t J_CLEANSZ = J_CAP + 64 + J_PAD;     // a round past the cap, then the zeros
constexpr uint32_t J_COEF = J_CLEAN + J_CLEANSZ;       // 64 blocks of 33 dwords
constexpr uint32_t J_BLK = 132;
constexpr uint32_t J_BYTES = J_COEF + 64 * J_BLK;
constexpr uint32_t J_LOW = 256;                        // refill below this many clean bytes ahead
static_assert(sizeof(JTabSet) % 16 == 0 && J_CLEAN % 16 == 0 && J_COEF % 16 == 0 && (64 * J_BLK) % 16 == 0,
              "16-byte LDS copies");
static_assert(J_BYTES <= 64 * 1024, "default dynamic LDS limit");
// a block reads at most 27 + 63 * 26 bits past where it began
static_assert(J_LOW * 8 >= 27 + 63 * 26 + 64, "a block never outruns a refilled buffer");
static_assert(J_PAD * 8 >= 27 + 63 * 26 + 64 && J_PAD % 64 == 0, "nor the zeros after the last byte");

constexpr uint32_t J_Q = J_TAB + offsetof(JTabSet, q);
constexpr uint32_t J_H = J_TAB + offsetof(JTabSet, h);
constexpr uint32_t JH_MAX = offsetof(JHuff, maxcode), JH_OFF = offsetof(JHuff, valoff), JH_VAL = offsetof(JHuff, val);

// zigzag position of the coefficient at natural (row-major) position n
// (indexed by unrolled loop counters only: compile-time constants, no table in memory)
__device__ __forceinline__ constexpr uint32_t jzz(uint32_t n) {
    constexpr uint8_t zz[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    return zz[n];
}

struct JBits {
    uint64_t bb;    // the next bits, from bit 63 down
    uint32_t nb;    // how many of them are loaded
    uint32_t cp;    // clean byte the next load takes
    uint32_t cend;  // clean bytes in the buffer
    uint32_t rawp;  // next raw byte of the stream
    uint32_t pend;  // 0, the marker code the refill stopped at, or 0x100 at the stream's end
};

__device__ __forceinline__ void jfill(JBits& s) {
    if (s.nb <= 32) {
        const uint32_t at = s.cp < J_CLEANSZ - 4 ? s.cp : J_CLEANSZ - 4;
        const uint32_t v = __builtin_bswap32(rfl(ld_u32_unaligned(zlds + J_CLEAN + at)));
        s.bb |= (uint64_t)v << (32 - s.nb);
        s.nb += 32;
        s.cp += 4;
    }
}

// Moves what is unread to the buffer's front and appends clean bytes until it holds more than
// J_CAP - 64 of them, a marker or the stream's end.
__device__ __forceinline__ void jrefill(JBits& s, const uint8_t* __restrict__ raw, uint32_t csize, uint32_t lane) {
    const uint32_t posb = s.cp * 8 - s.nb;  // bits consumed
    const uint32_t byte0 = posb >> 3 < s.cend ? posb >> 3 : s.cend;
    const uint32_t skip = posb - byte0 * 8;
    const uint32_t rem = s.cend - byte0;
    if (byte0)
        for (uint32_t k = 0; k < rem; k += 256) {  // forward, a round's reads before its writes
            const uint32_t v = ld_u32_unaligned(zlds + J_CLEAN + byte0 + k + 4 * lane);
            lds32(J_CLEAN + k + 4 * lane) = v;
        }
    uint32_t cend = rem, rawp = s.rawp, pend = s.pend;
    while (!pend && cend <= J_CAP - 64) {
        const uint32_t i = rawp + lane;
        const bool have = i < csize;
        const uint32_t b = have ? raw[i] : 0u;
        const uint32_t prev = have && i > 0 ? raw[i - 1] : 0u;
        const uint32_t next = i + 1 < csize ? raw[i + 1] : 1u;
        const bool marker = have && prev == 0xFF && b != 0 && b != 0xFF;
        const bool keep = have && !marker && !(b == 0 && prev == 0xFF) && (b != 0xFF || next == 0);
        const uint64_t M = __ballot(marker);
        const uint32_t fm = M ? (uint32_t)__builtin_ctzll(M) : 64u;
        const uint64_t K = __ballot(keep && lane < fm);
        const uint32_t at = cend + (uint32_t)__builtin_popcountll(K & ((1ull << lane) - 1));
        if (keep && lane < fm) zlds[J_CLEAN + at] = (uint8_t)b;
        cend += (uint32_t)__builtin_popcountll(K);
        if (M) {
            pend = rdl(b, fm);
            rawp += fm + 1;
        } else if (rawp + 64 >= csize) {
            pend = 0x100;
            rawp = csize;
        } else {
            rawp += 64;
        }
        cend = rfl(cend); rawp = rfl(rawp); pend = rfl(pend);
    }
    // zeros after the data: what a block reads past its end (an error, found when the block is
    // done) is the same in every run
#pragma unroll
    for (uint32_t k = 0; k < J_PAD; k += 64) zlds[J_CLEAN + cend + k + lane] = 0;
    s.cend = cend; s.rawp = rawp; s.pend = pend;
    s.cp = 0; s.bb = 0; s.nb = 0;
    jfill(s);
    s.bb <<= skip;  // < 8
    s.nb -= skip;
}

// One Huffman symbol from table `tab` (LDS offset of a JHuff); 256 for a code in no table.
__device__ __forceinline__ uint32_t jsym(JBits& s, uint32_t tab) {
    jfill(s);
    const uint32_t e = rfl(lds16(tab + 2 * (uint32_t)(s.bb >> 55)));
    uint32_t l, sym;
    if (e) {
        l = e >> 8;
        sym = e & 255;
    } else {
        l = 10;
        while (l <= 16 && (int32_t)(uint32_t)(s.bb >> (64 - l)) > (int32_t)rfl(lds32(tab + JH_MAX + 4 * l))) l++;
        if (l > 16) return 256;
        const uint32_t code = (uint32_t)(s.bb >> (64 - l));
        sym = rfl(zlds[tab + JH_VAL + ((code + rfl(lds32(tab + JH_OFF + 4 * l))) & 255)]);
    }
    s.bb <<= l;
    s.nb -= l;
    return sym;
}

// The next n (1 .. 16) bits as the signed value they encode (T.81 F.2.2.1 EXTEND).
__device__ __forceinline__ int32_t jreceive(JBits& s, uint32_t n) {
    const uint32_t v = (uint32_t)(s.bb >> (64 - n));
    s.bb <<= n;
    s.nb -= n;
    return v < (1u << (n - 1)) ? (int32_t)v - (int32_t)(1u << n) + 1 : (int32_t)v;
}

__device__ __forceinline__ int32_t jdescale(int32_t x, int n) { return (int32_t)((uint32_t)x + (1u << (n - 1))) >> n; }
__device__ __forceinline__ int32_t jmul(int32_t a, int32_t c) { return (int32_t)((uint32_t)a * (uint32_t)c); }
__device__ __forceinline__ int32_t jshl(int32_t a, int n) { return (int32_t)((uint32_t)a << n); }

// jidctint.c's one-dimensional pass over i[0..7], scaled by 2^13: o[0..7] before the descale
__device__ __forceinline__ void jidct1(const int32_t (&i)[8], int32_t (&o)[8]) {
    int32_t z2 = i[2], z3 = i[6];
    int32_t z1 = jmul(z2 + z3, 4433);
    int32_t tmp2 = z1 + jmul(z3, -15137), tmp3 = z1 + jmul(z2, 6270);
    int32_t tmp0 = jshl(i[0] + i[4], 13), tmp1 = jshl(i[0] - i[4], 13);
    const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = i[7]; tmp1 = i[5]; tmp2 = i[3]; tmp3 = i[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int32_t z4 = tmp1 + tmp3;
    const int32_t z5 = jmul(z3 + z4, 9633);
    tmp0 = jmul(tmp0, 2446); tmp1 = jmul(tmp1, 16819); tmp2 = jmul(tmp2, 25172); tmp3 = jmul(tmp3, 12299);
    z1 = jmul(z1, -7373); z2 = jmul(z2, -20995); z3 = jmul(z3, -16069); z4 = jmul(z4, -3196);
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    o[0] = tmp10 + tmp3; o[7] = tmp10 - tmp3;
    o[1] = tmp11 + tmp2; o[6] = tmp11 - tmp2;
    o[2] = tmp12 + tmp1; o[5] = tmp12 - tmp1;
    o[3] = tmp13 + tmp0; o[4] = tmp13 - tmp0;
}

// Block `blk` of the batch (coefficients in zigzag order at cf) times the quantiser at qo, through
// both passes, to 8 rows of 8 samples at out (8-byte aligned) with pitch `pitch`.
__device__ __forceinline__ void jidct_block(uint32_t cf, uint32_t qo, uint8_t* __restrict__ out, uint32_t pitch) {
    int32_t ws[64];
#pragma unroll
    for (uint32_t c = 0; c < 8; c++) {
        int32_t in[8], o[8];
#pragma unroll
        for (uint32_t r = 0; r < 8; r++)
            in[r] = (int32_t)(int16_t)lds16(cf + 2 * jzz(8 * r + c)) * (int32_t)lds16(qo + 2 * (8 * r + c));
        jidct1(in, o);
#pragma unroll
        for (uint32_t r = 0; r < 8; r++) ws[8 * r + c] = jdescale(o[r], 11);
    }
#pragma unroll
    for (uint32_t r = 0; r < 8; r++) {
        int32_t in[8], o[8];
#pragma unroll
        for (uint32_t c = 0; c < 8; c++) in[c] = ws[8 * r + c];
        jidct1(in, o);
        uint32_t w[2] = {0, 0};
#pragma unroll
        for (uint32_t c = 0; c < 8; c++) {
            int32_t v = jdescale(o[c], 18) + 128;
            v = v < 0 ? 0 : v > 255 ? 255 : v;
            w[c >> 2] |= (uint32_t)v << (8 * (c & 3));
        }
        *(uint2*)(out + (uint64_t)r * pitch) = make_uint2(w[0], w[1]);
    }
}

__global__ __launch_bounds__(64) void k_tiff_jpeg_decode(const JStream* __restrict__ st, uint32_t n,
                                                         const JTabSet* __restrict__ tabs,
                                                         const uint8_t* __restrict__ src,
                                                         uint8_t* __restrict__ scratch, uint32_t* __restrict__ err) {
    const uint32_t lane = threadIdx.x, si = blockIdx.x;
    if (si >= n) return;
    const JStream t = st[si];
    const uint32_t csize = rfl(t.csize), ncomp = rfl(t.ncomp) == 3 ? 3u : 1u;
    const uint32_t hs = ncomp == 3 && rfl(t.hs) == 2 ? 2u : 1u, vs = ncomp == 3 && rfl(t.vs) == 2 ? 2u : 1u;
    const uint32_t mcux = rfl(t.mcux), mcuy = rfl(t.mcuy), nmcu = mcux * mcuy;
    const uint32_t ri = rfl(t.restart);
    const uint32_t nluma = hs * vs, bpm = ncomp == 3 ? nluma + 2 : 1u;  // blocks per MCU: 1, 3, 4, 6
    const uint32_t per = 64 / bpm;                                      // MCUs per batch
    {
        const uint4* tp = (const uint4*)(tabs + rfl(t.tabset));
        for (uint32_t i = lane; i < sizeof(JTabSet) / 16; i += 64) *(uint4*)(zlds + J_TAB + 16 * i) = tp[i];
    }
    const uint8_t* raw = src + t.src_off;
    JBits s{0, 0, 0, 0, 0, 0};
    jrefill(s, raw, csize, lane);
    int32_t pred[3] = {0, 0, 0};
    uint32_t todo = ri, rstn = 0, bad = 0;
    for (uint32_t m0 = 0; m0 < nmcu && !bad; m0 += per) {
        const uint32_t m1 = m0 + per < nmcu ? m0 + per : nmcu;
        for (uint32_t i = lane; i < 64 * J_BLK / 16; i += 64) *(uint4*)(zlds + J_COEF + 16 * i) = make_uint4(0, 0, 0, 0);
        uint32_t cf = J_COEF;
        for (uint32_t m = m0; m < m1 && !bad; m++) {
            if (ri && todo == 0) {  // a restart marker stands here, the next in sequence
                if (!s.pend) jrefill(s, raw, csize, lane);
                const uint32_t posb = s.cp * 8 - s.nb;
                if (s.pend != 0xD0 + (rstn & 7) || (posb + 7) >> 3 != s.cend) { bad = 5; break; }
                rstn++;
                todo = ri;
                pred[0] = pred[1] = pred[2] = 0;
                s.pend = 0; s.cend = 0; s.cp = 0; s.nb = 0; s.bb = 0;
                jrefill(s, raw, csize, lane);
            }
            todo--;
            for (uint32_t b = 0; b < bpm && !bad; b++, cf += J_BLK) {
                const uint32_t c = b < nluma ? 0u : b - nluma + 1;
                if (!s.pend && s.cend * 8 < s.cp * 8 - s.nb + J_LOW * 8) jrefill(s, raw, csize, lane);
                const uint32_t dct = J_H + 2 * c * (uint32_t)sizeof(JHuff), act = dct + (uint32_t)sizeof(JHuff);
                const uint32_t sd = jsym(s, dct);
                if (sd > 11) { bad = sd == 256 ? 2 : 4; break; }
                int32_t dc = c == 0 ? pred[0] : c == 1 ? pred[1] : pred[2];
                if (sd) dc += jreceive(s, sd);
                if (c == 0) pred[0] = dc; else if (c == 1) pred[1] = dc; else pred[2] = dc;
                if (lane == 0) lds16(cf) = (uint16_t)dc;
                for (uint32_t k = 1; k < 64; k++) {
                    const uint32_t rs = jsym(s, act);
                    if (rs == 256) { bad = 2; break; }
                    const uint32_t r = rs >> 4, sz = rs & 15;
                    if (!sz) {
                        if (r != 15) break;  // end of block
                        k += 15;
                        if (k > 63) { bad = 3; break; }
                        continue;
                    }
                    k += r;
                    if (k > 63) { bad = 3; break; }
                    if (sz > 10) { bad = 4; break; }
                    jfill(s);
                    const int32_t v = jreceive(s, sz);
                    if (lane == 0) lds16(cf + 2 * k) = (uint16_t)v;
                }
                if (!bad && s.cp * 8 - s.nb > s.cend * 8) bad = 1;  // bits from past the data's end
            }
        }
        bad = rfl(bad);
        if (bad) break;
        // lane b transforms block b of the batch
        const uint32_t nb = (m1 - m0) * bpm;
        if (lane < nb) {
            const uint32_t m = m0 + lane / bpm, r = lane % bpm;
            const uint32_t mx = m % mcux, my = m / mcux;
            const uint32_t c = r < nluma ? 0u : r - nluma + 1;
            uint32_t x, y, pitch;
            uint64_t base = t.dst_off;
            if (c == 0) {
                x = (mx * hs + r % hs) * 8;
                y = (my * vs + r / hs) * 8;
                pitch = t.pitch0;
            } else {
                x = mx * 8;
                y = my * 8;
                pitch = t.pitchc;
                base += c == 1 ? t.offc1 : t.offc2;
            }
            jidct_block(J_COEF + lane * J_BLK, J_Q + c * 128, scratch + base + (uint64_t)y * pitch + x, pitch);
        }
    }
    if (lane == 0) err[si] = bad;
}

// ------------------------------------------------------------------ upsample, convert, place
// k_tiff_split_place's geometry and clipping: a workgroup of four waves per (segment, run of
// UP_ROWS segment rows), rows clipped uniformly to run, window and plane, only the visible width
// walked.  A lane owns 16 consecutive output pixels of a row: 16 luma bytes (one aligned load: the
// component pitches are multiples of 16), and for subsampled chroma the 8 samples under them with
// one neighbour on either side, from the near chroma row and (h2v2) the far one.  Edges are the
// component's own downsampled size -- cw = ceil(w / 2), ch = ceil(rows / 2) of this segment -- so
// the far row above the first and below the last is the edge row itself, never another segment's,
// and the first and last columns take jdsample.c's end rules.  As libjpeg does, a chroma plane at
// most two samples wide is replicated instead (its fancy upsamplers need downsampled_width > 2).
// Every whole group is one aligned 16-byte store per wanted plane; the row's last, partial group
// goes byte by byte.
constexpr uint32_t JP_WAVES = 4, JP_ROWS = 16;

__device__ __forceinline__ uint32_t jclamp(int32_t v) { return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

__device__ __forceinline__ void jstore(uint8_t* __restrict__ o, const uint32_t (&v)[16], uint32_t have) {
    if (!o) return;
    if (have == 16) {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) w[i >> 2] |= v[i] << (8 * (i & 3));
        *(uint4*)o = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 16; i++)
            if (i < have) o[i] = (uint8_t)v[i];
    }
}

__device__ __forceinline__ void jload16(const uint8_t* __restrict__ p, uint32_t (&v)[16]) {
    const uint4 q = *(const uint4*)p;
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) v[i] = (w[i >> 2] >> (8 * (i & 3))) & 255u;
}

// chroma samples ci0 - 1 .. ci0 + 8 of a row (ci0 a multiple of 8), edges replicated at 0 and cw - 1
__device__ __forceinline__ void jload_chroma(const uint8_t* __restrict__ row, uint32_t ci0, uint32_t cw, uint32_t (&v)[10]) {
    const uint2 q = *(const uint2*)(row + ci0);
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) v[i + 1] = ((i < 4 ? q.x : q.y) >> (8 * (i & 3))) & 255u;
    v[0] = ci0 > 0 ? row[ci0 - 1] : v[1];
    v[9] = ci0 + 8 < cw ? row[ci0 + 8] : v[8];
}

// MODE 0: components stored as they are (1 or 3, all 1x1); 1: YCbCr 1x1; 2: h2v1; 3: h2v2
template <uint32_t MODE>
__device__ __forceinline__ void jplace_rows(const TJpegSeg& u, const TSplitDst& d, const uint8_t* __restrict__ scratch,
                                            int32_t r0, int32_t r1, uint32_t vis, uint32_t lane, uint32_t w) {
    const uint8_t* p0 = scratch + u.src;
    const uint8_t* p1 = p0 + u.offc1;
    const uint8_t* p2 = p0 + u.offc2;
    const uint32_t cw = MODE >= 2 ? (u.w + 1) / 2 : u.w, ch = MODE == 3 ? (u.rows + 1) / 2 : u.rows;
    const bool fancy = cw > 2;
    const uint32_t nc = u.ncomp == 3 ? 3u : 1u;
    for (int32_t r = r0 + (int32_t)w; r < r1; r += (int32_t)JP_WAVES) {
        uint8_t* o[3];
#pragma unroll
        for (uint32_t c = 0; c < 3; c++)
            o[c] = c < nc && d.dev[c] ? d.dev[c] + (int64_t)(u.y0 + r) * d.pitch + u.x0 : nullptr;
        const uint32_t cr = MODE == 3 ? (uint32_t)r >> 1 : (uint32_t)r;
        uint32_t fr = cr;  // h2v2: the far chroma row
        if (MODE == 3 && fancy) fr = (r & 1) ? (cr + 1 < ch ? cr + 1 : cr) : (cr > 0 ? cr - 1 : cr);
        for (uint32_t off = 16 * lane; off < vis; off += 1024) {
            const uint32_t have = vis - off < 16 ? vis - off : 16u;
            uint32_t y[16], cb[16], cc[16];
            jload16(p0 + (uint64_t)r * u.pitch0 + off, y);
            if (MODE == 0) {
                jstore(o[0] ? o[0] + off : nullptr, y, have);
                if (nc == 3) {
                    jload16(p1 + (uint64_t)r * u.pitchc + off, cb);
                    jstore(o[1] ? o[1] + off : nullptr, cb, have);
                    jload16(p2 + (uint64_t)r * u.pitchc + off, cc);
                    jstore(o[2] ? o[2] + off : nullptr, cc, have);
                }
                continue;
            }
            if (MODE == 1) {
                jload16(p1 + (uint64_t)r * u.pitchc + off, cb);
                jload16(p2 + (uint64_t)r * u.pitchc + off, cc);
            } else {
                const uint32_t ci0 = off >> 1;
#pragma unroll
                for (uint32_t c = 0; c < 2; c++) {
                    const uint8_t* p = c ? p2 : p1;
                    uint32_t (&out)[16] = c ? cc : cb;
                    uint32_t a[10], b[10];
                    jload_chroma(p + (uint64_t)cr * u.pitchc, ci0, cw, a);
                    if (MODE == 3) {
                        jload_chroma(p + (uint64_t)fr * u.pitchc, ci0, cw, b);
#pragma unroll
                        for (uint32_t i = 0; i < 10; i++) a[i] = 3 * a[i] + b[i];
                    }
#pragma unroll
                    for (uint32_t j = 0; j < 8; j++) {
                        const uint32_t i = ci0 + j, t = a[j + 1];
                        if (!fancy) {
                            out[2 * j] = out[2 * j + 1] = MODE == 3 ? t >> 2 : t;  // (3 t + t) / 4: near == far
                        } else if (MODE == 2) {
                            out[2 * j] = i == 0 ? t : (3 * t + a[j] + 1) >> 2;
                            out[2 * j + 1] = i == cw - 1 ? t : (3 * t + a[j + 2] + 2) >> 2;
                        } else {
                            out[2 * j] = i == 0 ? (4 * t + 8) >> 4 : (3 * t + a[j] + 8) >> 4;
                            out[2 * j + 1] = i == cw - 1 ? (4 * t + 7) >> 4 : (3 * t + a[j + 2] + 7) >> 4;
                        }
                    }
                }
            }
            uint32_t R[16], G[16], B[16];
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) {
                const int32_t Y = (int32_t)y[i], u8 = (int32_t)cb[i] - 128, v8 = (int32_t)cc[i] - 128;
                R[i] = jclamp(Y + ((91881 * v8 + 32768) >> 16));
                G[i] = jclamp(Y + ((-22554 * u8 - 46802 * v8 + 32768) >> 16));
                B[i] = jclamp(Y + ((116130 * u8 + 32768) >> 16));
            }
            jstore(o[0] ? o[0] + off : nullptr, R, have);
            jstore(o[1] ? o[1] + off : nullptr, G, have);
            jstore(o[2] ? o[2] + off : nullptr, B, have);
        }
    }
}

__global__ __launch_bounds__(64 * JP_WAVES) void k_tiff_jpeg_place(const TJpegSeg* __restrict__ sg,
                                                                   const TSplitDst* __restrict__ dt,
                                                                   const uint8_t* __restrict__ scratch) {
    const uint32_t lane = threadIdx.x & 63, w = rfl(threadIdx.x >> 6);
    const TJpegSeg u = sg[blockIdx.x];
    const TSplitDst d = dt[rfl(u.dst)];
    const int32_t x0 = (int32_t)rfl((uint32_t)u.x0), y0 = (int32_t)rfl((uint32_t)u.y0);
    const int32_t rows = (int32_t)rfl(u.rows);
    // segment rows of this run that lie in the window and in the plane
    int32_t r0 = (int32_t)(blockIdx.y * JP_ROWS), r1 = r0 + (int32_t)JP_ROWS;
    const int32_t top = d.y_lo > 0 ? d.y_lo : 0, bottom = d.y_hi < d.sy ? d.y_hi : d.sy;
    r1 = r1 < rows ? r1 : rows;
    r0 = r0 > top - y0 ? r0 : top - y0;
    r1 = r1 < bottom - y0 ? r1 : bottom - y0;
    if (r0 >= r1 || x0 >= d.sx || x0 < 0 || y0 < 0) return;
    const uint32_t wvis = (uint32_t)(d.sx - x0), sw = rfl(u.w);
    const uint32_t vis = wvis < sw ? wvis : sw;
    switch (rfl(u.mode)) {  // once per workgroup
        case 0: jplace_rows<0>(u, d, scratch, r0, r1, vis, lane, w); break;
        case 1: jplace_rows<1>(u, d, scratch, r0, r1, vis, lane, w); break;
        case 2: jplace_rows<2>(u, d, scratch, r0, r1, vis, lane, w); break;
        case 3: jplace_rows<3>(u, d, scratch, r0, r1, vis, lane, w); break;
        default: break;
    }
}

hipError_t launch_tiff_jpeg_decode(hipStream_t st, const JStream* d_streams, uint32_t n, const JTabSet* d_tabs,
                                   const uint8_t* src, uint8_t* scratch, uint32_t* err) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_tiff_jpeg_decode, dim3(n), dim3(64), J_BYTES, st, d_streams, n, d_tabs, src, scratch, err);
    return hipGetLastError();
}

hipError_t launch_tiff_jpeg_place(hipStream_t st, const TJpegSeg* d_segs, uint32_t n, uint32_t max_rows,
                                  const TSplitDst* d_dst, const uint8_t* scratch) {
    if (!n || !max_rows) return hipSuccess;
    hipLaunchKernelGGL(k_tiff_jpeg_place, dim3(n, (max_rows + JP_ROWS - 1) / JP_ROWS), dim3(64 * JP_WAVES), 0, st,
                       d_segs, d_dst, scratch);
    return hipGetLastError();
}

}  // namespace pbx
