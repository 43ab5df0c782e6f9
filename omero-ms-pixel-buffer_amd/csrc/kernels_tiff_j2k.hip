// kernels_tiff_j2k.hip — JPEG 2000 TIFF segments (Compression 33003 / 33004 / 33005 / 34712: one
// codestream of one tile per strip or tile, reversible 5/3 or irreversible 9/7; DESIGN.md §10b
// "JPEG 2000 segments").
// The host has read SIZ, COD and QCD and laid out every sub-band, code block and coefficient
// from them (tiff_j2k_plan, runtime.cpp); packet headers and code-block bytes are read here only.
//
//   k_tiff_j2k_packets  tier 2, one wave per stream: the packet headers of the host's packet
//                       list (tag trees, passes, Lblock, lengths; layers, precincts, SOP / EPH)
//                       into one J2Code per code block, every offset and length checked against
//                       the stream's length before it is stored
//   k_tiff_j2k_gather   a wave per contribution of a block whose bytes lie in several packets:
//                       copies them into the block's one run in the stream's gather area
//   k_tiff_j2k_blocks   tier 1, one wave per code block: the MQ decoder and the three coding
//                       passes over state in LDS, then the block's coefficients, two's
//                       complement int32, row by row into its sub-band's rectangle (9/7:
//                       midpoint magnitudes, dequantised, as float32)
//   k_tiff_j2k_idwt     the inverse 5/3 lifting, one workgroup per component, level by level
//   k_tiff_j2k_idwt97   the inverse 9/7 lifting in float32, same geometry
//   k_tiff_j2k_place    inverse RCT (9/7: ICT, rounding half to even), level shift, clamp, split
//                       and placement, clipped as k_tiff_jpeg_place clips
//   k_tiff_j2k_place_chroma  the same for segments whose second and third components are
//                       subsampled (replicated) and / or YCbCr (converted after the clamp)
//
// The serial halves (tiff_j2k_dev.h) are run by lane 0 of their wave; the lanes together clear
// the state before it and store the coefficients after it.  An arithmetic decoder has one chain of
// dependent decisions per code block, so the parallelism of tier 1 is across code blocks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_util.h"
#include "pbx_common.h"
#include "pbx_kernels.h"
#include "tiff_j2k_dev.h"
#include "zarr_dev.h"

namespace pbx {

__constant__ uint32_t c_j2_mq[J2_MQ_STATES] = {PBX_MQ_TABLE};

__global__ __launch_bounds__(64) void k_tiff_j2k_packets(const J2Stream* __restrict__ st, uint32_t n,
                                                         const J2Packet* __restrict__ packets,
                                                         const J2Band* __restrict__ bands,
                                                         const uint8_t* __restrict__ src, uint32_t* tt, J2Code* code,
                                                         J2Walk* walk, J2Contrib* con, uint32_t* __restrict__ err) {
    const uint32_t si = blockIdx.x;
    if (si >= n || threadIdx.x != 0) return;
    const J2Stream S = st[si];
    err[si] = j2k_packets(S, packets, bands, src, tt, code, walk, con);
}

// One wave per entry of the contribution table (streams of one layer have none): a cleared entry
// ends at once, another's bytes go a byte per lane, stride 64, from the packets to the block's run.
__global__ __launch_bounds__(64) void k_tiff_j2k_gather(const J2Contrib* __restrict__ con, uint32_t n,
                                                        const J2Code* __restrict__ code,
                                                        const J2Block* __restrict__ blocks, uint32_t n_blocks,
                                                        const J2Stream* __restrict__ st, uint32_t n_streams,
                                                        const uint8_t* __restrict__ src, uint8_t* __restrict__ scratch) {
    const uint32_t lane = threadIdx.x, gi = blockIdx.x;
    if (gi >= n) return;
    const J2Contrib G = con[gi];
    if (!G.len || G.block >= n_blocks) return;
    const uint32_t si = blocks[G.block].stream;
    if (si >= n_streams) return;
    const J2Stream S = st[si];
    uint32_t from, to;
    if (!j2k_gather_span(S, code[G.block], G, &from, &to)) return;
    const uint8_t* in = src + S.src_off + from;
    uint8_t* out = scratch + S.gather + to;
    for (uint32_t i = lane; i < G.len; i += 64) out[i] = in[i];
}

// LDS: max_coef magnitudes, max_flag flag bytes (rounded up to 16), the contexts, the MQ table.
__global__ __launch_bounds__(64) void k_tiff_j2k_blocks(const J2Block* __restrict__ blocks, uint32_t n,
                                                        const J2Code* __restrict__ code,
                                                        const J2Stream* __restrict__ st,
                                                        const uint8_t* __restrict__ src, uint8_t* __restrict__ scratch,
                                                        uint32_t max_coef, uint32_t max_flag) {
    const uint32_t lane = threadIdx.x, bi = blockIdx.x;
    if (bi >= n) return;
    const J2Block B = blocks[bi];
    const J2Code C = code[bi];
    const J2Stream S = st[B.stream];
    const uint32_t w = B.w, h = B.h, nco = w * h, nfl = (w + 2) * (h + 2);
    if (nco > max_coef || nfl > max_flag) return;  // (the planner sized both from these blocks)
    const uint32_t flg_off = 4 * max_coef, ctx_off = flg_off + ((max_flag + 15) & ~15u), tab_off = ctx_off + J2_CTX_BYTES;
    int32_t* mag = (int32_t*)zlds;
    uint8_t* flg = zlds + flg_off;
    uint8_t* ctx = zlds + ctx_off;
    uint32_t* tab = (uint32_t*)(zlds + tab_off);
    for (uint32_t i = lane; i < nco; i += 64) mag[i] = 0;
    for (uint32_t i = lane; i < (nfl + 3) / 4; i += 64) lds32(flg_off + 4 * i) = 0;  // (max_flag rounded up to 16)
    if (lane < 19) ctx[lane] = lane == 0 ? 4 << 1 : lane == 17 ? 3 << 1 : lane == 18 ? 46 << 1 : 0;
    if (lane < J2_MQ_STATES) tab[lane] = c_j2_mq[lane];
    __syncthreads();
    const uint32_t planes = (uint32_t)B.mb - C.zbp;
    const bool irr = B.irrev != 0;  // (uniform: one block per workgroup)
    const uint8_t* bytes = j2k_code_bytes(S, C, src + S.src_off, scratch + S.gather);
    const bool ok = C.passes != 0 && C.zbp < B.mb && planes <= (irr ? 30u : 31u) && C.passes <= 3 * planes - 2 && bytes;
    if (ok && lane == 0) {
        if (irr) j2k_block<true>(mag, flg, ctx, tab, bytes, C.len, w, h, B.orient, planes, C.passes);
        else j2k_block<false>(mag, flg, ctx, tab, bytes, C.len, w, h, B.orient, planes, C.passes);
    }
    __syncthreads();
    if (irr) {  // dequantised: twice the midpoint magnitude times half the step
        float* out = (float*)(scratch + B.dst);
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = lane; x < w; x += 64)
                out[(uint64_t)y * B.pitch + x] = j2f_dequant(mag[y * w + x], flg[(y + 1) * (w + 2) + x + 1] & J2F_NEG, B.hstep);
        return;
    }
    int32_t* out = (int32_t*)(scratch + B.dst);
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = lane; x < w; x += 64) {
            const int32_t v = mag[y * w + x];
            out[(uint64_t)y * B.pitch + x] = (flg[(y + 1) * (w + 2) + x + 1] & J2F_NEG) ? -v : v;
        }
}

// ------------------------------------------------------------------------------ inverse 5/3
// One dimension of T.800 F.3 for a signal that starts on an even sample: `nl` low-pass samples
// L(n) at the even places, `nh` = nl or nl - 1 high-pass samples H(n) at the odd ones, extended
// by whole-sample symmetry.  The even output 2n is E(n) = L(n) - ((H(n - 1) + H(n) + 2) >> 2),
// the odd one 2n + 1 is H(n) + ((E(n) + E(n + 1)) >> 1); a thread computes both of a pair and
// recomputes its neighbour's E, so no thread waits for another inside a pass.
template <class FL, class FH>
__device__ __forceinline__ int32_t j2_even(uint32_t n, uint32_t nh, FL L, FH H) {
    if (nh == 0) return L(n);
    const int32_t hm = H(n ? n - 1 : 0u), hp = H(n < nh ? n : nh - 1);
    return (int32_t)((uint32_t)L(n) - (uint32_t)((int32_t)((uint32_t)hm + (uint32_t)hp + 2u) >> 2));
}

constexpr uint32_t J2W_THREADS = 256;

__global__ __launch_bounds__(J2W_THREADS) void k_tiff_j2k_idwt(const J2Comp* __restrict__ comps, uint32_t n,
                                                               uint8_t* __restrict__ scratch) {
    if (blockIdx.x >= n) return;
    const J2Comp c = comps[blockIdx.x];
    if (c.irrev) return;  // k_tiff_j2k_idwt97's
    int32_t* A = (int32_t*)(scratch + c.a);
    int32_t* Bp = (int32_t*)(scratch + c.b);
    const uint64_t W = c.w;
    const uint32_t NL = c.levels < 32 ? c.levels : 32;
    for (uint32_t r = 1; r <= NL; r++) {
        const uint32_t sh = NL - r;  // 0 .. 31
        const uint32_t cw = (uint32_t)((c.w + (1ull << sh) - 1) >> sh), ch = (uint32_t)((c.h + (1ull << sh) - 1) >> sh);
        const uint32_t lw = (cw + 1) / 2, lh = (ch + 1) / 2;  // resolution r - 1
        if (cw == lw && ch == lh) continue;                   // 1 x 1: nothing to undo
        const uint32_t hw = cw - lw, hh = ch - lh;
        // rows: A's [L | H] halves -> B interleaved
        for (uint64_t i = threadIdx.x; i < (uint64_t)ch * lw; i += J2W_THREADS) {
            const uint32_t y = (uint32_t)(i / lw), k = (uint32_t)(i % lw);
            const int32_t* row = A + y * W;
            auto L = [&](uint32_t q) { return row[q]; };
            auto H = [&](uint32_t q) { return row[lw + q]; };
            const int32_t e0 = j2_even(k, hw, L, H);
            Bp[y * W + 2 * k] = e0;
            if (k < hw) {
                const int32_t e1 = k + 1 < lw ? j2_even(k + 1, hw, L, H) : e0;
                Bp[y * W + 2 * k + 1] = (int32_t)((uint32_t)H(k) + (uint32_t)((int32_t)((uint32_t)e0 + (uint32_t)e1) >> 1));
            }
        }
        __syncthreads();
        // columns: B's [L ; H] halves -> A interleaved
        for (uint64_t i = threadIdx.x; i < (uint64_t)lh * cw; i += J2W_THREADS) {
            const uint32_t k = (uint32_t)(i / cw), x = (uint32_t)(i % cw);
            const int32_t* col = Bp + x;
            auto L = [&](uint32_t q) { return col[q * W]; };
            auto H = [&](uint32_t q) { return col[(lh + q) * W]; };
            const int32_t e0 = j2_even(k, hh, L, H);
            A[(2ull * k) * W + x] = e0;
            if (k < hh) {
                const int32_t e1 = k + 1 < lh ? j2_even(k + 1, hh, L, H) : e0;
                A[(2ull * k + 1) * W + x] = (int32_t)((uint32_t)H(k) + (uint32_t)((int32_t)((uint32_t)e0 + (uint32_t)e1) >> 1));
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------ inverse 9/7
// T.800 F.3.8 on float planes, in k_tiff_j2k_idwt's layout: per level the rows (A's [L | H]
// halves -> B interleaved and scaled by K / 1/K, then the four lifting steps in place in B), then
// the columns (B -> A likewise).  Each lifting step updates the samples of one parity from their
// neighbours of the other, so inside a step no thread reads what another writes; between steps the
// workgroup meets at a barrier, the planes staying in HBM (a 256 x 256 tile is 256 KiB a plane,
// above the 160 KiB of LDS, and any tile size has to work: one form, no staged variant beside it).
// The arithmetic is tiff_j2k_dev.h's, the CPU hook's too.
constexpr uint32_t J2W97_THREADS = 1024;

// one lifting step with constant `cst` on the samples of parity `par` of every line of the cw x ch
// region of P: lines are rows (COLS false) or columns (COLS true), each of at least 2 samples
template <bool COLS>
__device__ __forceinline__ void j2_lift97(float* P, uint64_t W, uint32_t cw, uint32_t ch, uint32_t par, float cst) {
    const uint32_t len = COLS ? ch : cw, nl = COLS ? cw : ch;
    const uint32_t cnt = (len + 1 - par) / 2;
    const uint32_t total = nl * cnt;  // (a plane has fewer than 2^29 samples: tiff_j2k_plan)
    for (uint32_t i = threadIdx.x; i < total; i += J2W97_THREADS) {
        const uint32_t line = COLS ? i % nl : i / cnt, k = COLS ? i / nl : i % cnt;
        const uint32_t p = 2 * k + par;  // < len
        const uint32_t pm = p ? p - 1 : 1, pp = p + 1 < len ? p + 1 : len - 2;  // whole-sample symmetry
        float* base = COLS ? P + line : P + line * W;
        const uint64_t st = COLS ? W : 1;
        base[p * st] = j2f_lift(base[p * st], base[pm * st], base[pp * st], cst);
    }
}

__global__ __launch_bounds__(J2W97_THREADS) void k_tiff_j2k_idwt97(const J2Comp* __restrict__ comps, uint32_t n,
                                                                   uint8_t* __restrict__ scratch) {
    if (blockIdx.x >= n) return;
    const J2Comp c = comps[blockIdx.x];
    if (!c.irrev) return;  // k_tiff_j2k_idwt's
    float* A = (float*)(scratch + c.a);
    float* Bp = (float*)(scratch + c.b);
    const uint64_t W = c.w;
    const uint32_t NL = c.levels < 32 ? c.levels : 32;
    auto cs = [](uint32_t k) { return k == 0 ? J2F_DELTA : k == 1 ? J2F_GAMMA : k == 2 ? J2F_BETA : J2F_ALPHA; };
    for (uint32_t r = 1; r <= NL; r++) {
        const uint32_t sh = NL - r;  // 0 .. 31
        const uint32_t cw = (uint32_t)((c.w + (1ull << sh) - 1) >> sh), ch = (uint32_t)((c.h + (1ull << sh) - 1) >> sh);
        const uint32_t lw = (cw + 1) / 2, lh = (ch + 1) / 2;  // resolution r - 1
        if (cw == lw && ch == lh) continue;                   // 1 x 1: nothing to undo
        const uint32_t total = ch * cw;  // < 2^29: 32-bit divisions
        for (uint32_t i = threadIdx.x; i < total; i += J2W97_THREADS) {
            const uint32_t y = i / cw, x = i % cw;
            const float v = A[y * W + x];
            const uint32_t to = x < lw ? 2 * x : 2 * (x - lw) + 1;  // < cw
            Bp[y * W + to] = cw > 1 ? j2f_scale(v, x < lw ? J2F_K : J2F_INVK) : v;
        }
        __syncthreads();
        if (cw > 1)
            for (uint32_t k = 0; k < 4; k++) {
                j2_lift97<false>(Bp, W, cw, ch, k & 1, cs(k));
                __syncthreads();
            }
        for (uint32_t i = threadIdx.x; i < total; i += J2W97_THREADS) {
            const uint32_t y = i / cw, x = i % cw;
            const float v = Bp[y * W + x];
            const uint32_t to = y < lh ? 2 * y : 2 * (y - lh) + 1;  // < ch
            A[to * W + x] = ch > 1 ? j2f_scale(v, y < lh ? J2F_K : J2F_INVK) : v;
        }
        __syncthreads();
        if (ch > 1)
            for (uint32_t k = 0; k < 4; k++) {
                j2_lift97<true>(A, W, cw, ch, k & 1, cs(k));
                __syncthreads();
            }
    }
}

// ------------------------------------------------------------------------------ placement
// k_tiff_jpeg_place's geometry: a workgroup of four waves per (segment, run of J2P_ROWS segment
// rows), rows clipped to run, window and plane, only the visible width walked, a lane per pixel.
constexpr uint32_t J2P_WAVES = 4, J2P_ROWS = 16;

__device__ __forceinline__ uint32_t j2_sample(int32_t v, uint32_t prec) {
    const int32_t hi = (int32_t)((1u << prec) - 1u);
    const int64_t s = (int64_t)v + (int64_t)(1u << (prec - 1));
    return (uint32_t)(s < 0 ? 0 : s > hi ? hi : s);
}

__global__ __launch_bounds__(64 * J2P_WAVES) void k_tiff_j2k_place(const TJ2Seg* __restrict__ sg,
                                                                   const TSplitDst* __restrict__ dt,
                                                                   const uint8_t* __restrict__ scratch) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const TJ2Seg u = sg[blockIdx.x];
    const TSplitDst d = dt[u.dst];
    const uint32_t prec = u.prec == 16 ? 16u : 8u, bpp = prec == 16 ? 2u : 1u;
    if (d.bpp != bpp) return;  // (the host checked the plane's pixel type against the precision)
    const int32_t x0 = u.x0, y0 = u.y0, rows = (int32_t)u.rows;
    int32_t r0 = (int32_t)(blockIdx.y * J2P_ROWS), r1 = r0 + (int32_t)J2P_ROWS;
    const int32_t top = d.y_lo > 0 ? d.y_lo : 0, bottom = d.y_hi < d.sy ? d.y_hi : d.sy;
    r1 = r1 < rows ? r1 : rows;
    r0 = r0 > top - y0 ? r0 : top - y0;
    r1 = r1 < bottom - y0 ? r1 : bottom - y0;
    if (r0 >= r1 || x0 >= d.sx || x0 < 0 || y0 < 0) return;
    const uint32_t wvis = (uint32_t)(d.sx - x0);
    const uint32_t vis = wvis < u.w ? wvis : u.w;
    const uint32_t nc = u.ncomp == 3 ? 3u : 1u;
    const int32_t* p0 = (const int32_t*)(scratch + u.src[0]);
    const int32_t* p1 = (const int32_t*)(scratch + u.src[nc == 3 ? 1 : 0]);
    const int32_t* p2 = (const int32_t*)(scratch + u.src[nc == 3 ? 2 : 0]);
    if (u.rct & J2_SEG_IRREV) {  // float planes: inverse ICT, level shift, round half to even, clamp
        const float* f0 = (const float*)p0;
        const float* f1 = (const float*)p1;
        const float* f2 = (const float*)p2;
        for (int32_t r = r0 + (int32_t)wv; r < r1; r += (int32_t)J2P_WAVES) {
            const uint64_t at = (uint64_t)r * u.w;
            for (uint32_t x = lane; x < vis; x += 64) {
                float v[3];
                v[0] = f0[at + x];
                if (nc == 3) {
                    v[1] = f1[at + x];
                    v[2] = f2[at + x];
                    if (u.rct & 1) j2f_ict(v);
                }
#pragma unroll
                for (uint32_t c = 0; c < 3; c++) {
                    if (c >= nc || !d.dev[c]) continue;
                    uint8_t* o = d.dev[c] + (int64_t)(y0 + r) * d.pitch + ((int64_t)x0 + x) * bpp;
                    const uint32_t s = j2f_sample(v[c], prec);
                    if (bpp == 1) *o = (uint8_t)s;
                    else *(uint16_t*)o = d.big_endian ? (uint16_t)(s >> 8 | s << 8) : (uint16_t)s;
                }
            }
        }
        return;
    }
    for (int32_t r = r0 + (int32_t)wv; r < r1; r += (int32_t)J2P_WAVES) {
        const uint64_t at = (uint64_t)r * u.w;
        for (uint32_t x = lane; x < vis; x += 64) {
            int32_t v[3];
            v[0] = p0[at + x];
            if (nc == 3) {
                v[1] = p1[at + x];
                v[2] = p2[at + x];
                if (u.rct & 1) {  // G = Y - ((U + V) >> 2), R = V + G, B = U + G
                    const int32_t g = (int32_t)((uint32_t)v[0] - (uint32_t)((int32_t)((uint32_t)v[1] + (uint32_t)v[2]) >> 2));
                    const int32_t rr = (int32_t)((uint32_t)v[2] + (uint32_t)g), bb = (int32_t)((uint32_t)v[1] + (uint32_t)g);
                    v[0] = rr;
                    v[1] = g;
                    v[2] = bb;
                }
            }
#pragma unroll
            for (uint32_t c = 0; c < 3; c++) {
                if (c >= nc || !d.dev[c]) continue;
                uint8_t* o = d.dev[c] + (int64_t)(y0 + r) * d.pitch + ((int64_t)x0 + x) * bpp;
                const uint32_t s = j2_sample(v[c], prec);
                if (bpp == 1) *o = (uint8_t)s;
                else *(uint16_t*)o = d.big_endian ? (uint16_t)(s >> 8 | s << 8) : (uint16_t)s;
            }
        }
    }
}

// Segments with J2_SEG_CHROMA bits: three components of precision 8 and no colour transform in
// the stream (tiff_j2k_plan), components 1 and 2 at half width and / or half height in planes of
// their own pitch, and / or YCbCr.  k_tiff_j2k_place's geometry and clipping; a lane reads Y at
// (r, x) and chroma at (r / ys, x / xs) (j2k_chroma_at: replication), shifts, rounds and clamps
// each as k_tiff_j2k_place does, converts with J2_SEG_YCC (j2k_ycc_rgb) and stores the wanted
// samples.  IRR: float planes.  Neighbouring lanes share a chroma dword: the loads of a wave cover
// half the lines the luma's do.
template <bool IRR>
__device__ __forceinline__ void j2_place_chroma(const TJ2Seg& u, const TSplitDst& d, const uint8_t* __restrict__ scratch,
                                                int32_t r0, int32_t r1, uint32_t vis, uint32_t lane, uint32_t wv) {
    const uint32_t* p0 = (const uint32_t*)(scratch + u.src[0]);
    const uint32_t* p1 = (const uint32_t*)(scratch + u.src[1]);
    const uint32_t* p2 = (const uint32_t*)(scratch + u.src[2]);
    for (int32_t r = r0 + (int32_t)wv; r < r1; r += (int32_t)J2P_WAVES) {
        for (uint32_t x = lane; x < vis; x += 64) {
            const uint64_t ac = j2k_chroma_at(1, x, (uint32_t)r, u.w, u.rct);
            const uint32_t raw[3] = {p0[(uint64_t)r * u.w + x], p1[ac], p2[ac]};
            uint32_t v[3];
#pragma unroll
            for (uint32_t c = 0; c < 3; c++) v[c] = IRR ? j2f_sample(__uint_as_float(raw[c]), 8) : j2_sample((int32_t)raw[c], 8);
            if (u.rct & J2_SEG_YCC) j2k_ycc_rgb(v);
#pragma unroll
            for (uint32_t c = 0; c < 3; c++) {
                if (!d.dev[c]) continue;
                d.dev[c][(int64_t)(u.y0 + r) * d.pitch + (int64_t)u.x0 + x] = (uint8_t)v[c];
            }
        }
    }
}

__global__ __launch_bounds__(64 * J2P_WAVES) void k_tiff_j2k_place_chroma(const TJ2Seg* __restrict__ sg,
                                                                          const TSplitDst* __restrict__ dt,
                                                                          const uint8_t* __restrict__ scratch) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const TJ2Seg u = sg[blockIdx.x];
    const TSplitDst d = dt[u.dst];
    // (the host checked: three components of precision 8, no colour transform, a uint8 plane)
    if (d.bpp != 1 || u.ncomp != 3 || u.prec != 8 || (u.rct & 1)) return;
    const int32_t x0 = u.x0, y0 = u.y0, rows = (int32_t)u.rows;
    int32_t r0 = (int32_t)(blockIdx.y * J2P_ROWS), r1 = r0 + (int32_t)J2P_ROWS;
    const int32_t top = d.y_lo > 0 ? d.y_lo : 0, bottom = d.y_hi < d.sy ? d.y_hi : d.sy;
    r1 = r1 < rows ? r1 : rows;
    r0 = r0 > top - y0 ? r0 : top - y0;
    r1 = r1 < bottom - y0 ? r1 : bottom - y0;
    if (r0 >= r1 || x0 >= d.sx || x0 < 0 || y0 < 0) return;
    const uint32_t wvis = (uint32_t)(d.sx - x0);
    const uint32_t vis = wvis < u.w ? wvis : u.w;
    if (u.rct & J2_SEG_IRREV) j2_place_chroma<true>(u, d, scratch, r0, r1, vis, lane, wv);
    else j2_place_chroma<false>(u, d, scratch, r0, r1, vis, lane, wv);
}

// meta (zeroed by the caller): a J2Code and a J2Walk per block, n_con J2Contrib, the tag-tree nodes
hipError_t launch_tiff_j2k_decode(hipStream_t st, const J2Stream* d_streams, uint32_t n_streams,
                                  const J2Packet* d_packets, const J2Band* d_bands, const J2Block* d_blocks,
                                  uint32_t n_blocks, uint32_t n_con, const J2Comp* d_comps, uint32_t n_comps,
                                  uint32_t n_irrev, uint32_t max_coef, uint32_t max_flag, uint8_t* meta,
                                  const uint8_t* src, uint8_t* scratch, uint32_t* err) {
    if (!n_streams) return hipSuccess;
    J2Code* code = (J2Code*)meta;
    J2Contrib* con = (J2Contrib*)(meta + sizeof(J2Code) * (uint64_t)n_blocks);
    J2Walk* walk = (J2Walk*)((uint8_t*)con + sizeof(J2Contrib) * (uint64_t)n_con);
    uint32_t* tt = (uint32_t*)((uint8_t*)walk + sizeof(J2Walk) * (uint64_t)n_blocks);
    hipLaunchKernelGGL(k_tiff_j2k_packets, dim3(n_streams), dim3(64), 0, st, d_streams, n_streams, d_packets, d_bands,
                       src, tt, code, walk, con, err);
    if (n_con)
        hipLaunchKernelGGL(k_tiff_j2k_gather, dim3(n_con), dim3(64), 0, st, con, n_con, code, d_blocks, n_blocks,
                           d_streams, n_streams, src, scratch);
    if (n_blocks) {
        const uint32_t lds = 4 * max_coef + ((max_flag + 15) & ~15u) + J2_CTX_BYTES + J2_TAB_BYTES;
        hipLaunchKernelGGL(k_tiff_j2k_blocks, dim3(n_blocks), dim3(64), lds, st, d_blocks, n_blocks, code, d_streams, src,
                           scratch, max_coef, max_flag);
    }
    if (n_comps > n_irrev)
        hipLaunchKernelGGL(k_tiff_j2k_idwt, dim3(n_comps), dim3(J2W_THREADS), 0, st, d_comps, n_comps, scratch);
    if (n_irrev)
        hipLaunchKernelGGL(k_tiff_j2k_idwt97, dim3(n_comps), dim3(J2W97_THREADS), 0, st, d_comps, n_comps, scratch);
    return hipGetLastError();
}

// d_segs: n segments, the n - n_chroma without J2_SEG_CHROMA bits first
hipError_t launch_tiff_j2k_place(hipStream_t st, const TJ2Seg* d_segs, uint32_t n, uint32_t n_chroma, uint32_t max_rows,
                                 const TSplitDst* d_dst, const uint8_t* scratch) {
    if (!n || !max_rows || n_chroma > n) return hipSuccess;
    const uint32_t gy = (max_rows + J2P_ROWS - 1) / J2P_ROWS;
    if (n > n_chroma)
        hipLaunchKernelGGL(k_tiff_j2k_place, dim3(n - n_chroma, gy), dim3(64 * J2P_WAVES), 0, st, d_segs, d_dst, scratch);
    if (n_chroma)
        hipLaunchKernelGGL(k_tiff_j2k_place_chroma, dim3(n_chroma, gy), dim3(64 * J2P_WAVES), 0, st, d_segs + (n - n_chroma),
                           d_dst, scratch);
    return hipGetLastError();
}

}  // namespace pbx
