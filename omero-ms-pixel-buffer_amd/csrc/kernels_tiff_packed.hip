// kernels_tiff_packed.hip — TIFF segments of bit-packed samples and PackBits streams
// (pbx_planes_register_tiff_packed / pbx_band_write_tiff_packed; DESIGN.md §10b "packed samples
// and PackBits").  Bio-Formats unpacks such samples MSB-first into uint8 (1 .. 8 bits) or uint16
// (9 .. 16 bits) without scaling, and so do these kernels.
//
//   k_tiff_packbits      one wave per strip or tile: TIFF 6.0 section 9 PackBits.  The header
//                        byte n of a run is wave-uniform: 0 .. 127 copies n + 1 literal bytes,
//                        129 .. 255 (-127 .. -1) repeats the next byte 257 - n times, 128 (-128)
//                        does nothing.  The 1 .. 128 bytes of a run are stored by the lanes
//                        together, two a lane at most.
//   k_tiff_unpack_place  segment rows of `bits`-wide samples (1 .. 16), every row padded to a whole
//                        byte, unpacked into uint8 / uint16 samples and placed into the pitched
//                        plane (S = 2 .. 4 chunky samples: into S planes), in one pass.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_util.h"
#include "pbx_common.h"
#include "pbx_kernels.h"
#include "zarr_dev.h"

namespace pbx {

// ------------------------------------------------------------------------------- PackBits
// The input goes through InWin (zarr_dev.h): ZWIN bytes of the stream in LDS, reloaded when a
// run's header and bytes (at most 129) do not lie inside.  Everything about the parse is
// wave-uniform; only the stores of a run's bytes are per lane.
// err[]: 0, or 1 the stream ends before dlen bytes are out (in a header or inside a run), 3 a run
// that would write past dlen.  A stream that has produced dlen bytes is done: what follows is not
// read (libtiff stops at the row count).
constexpr uint32_t PB_WAVES = 4;  // streams (waves) per workgroup

__global__ __launch_bounds__(64 * PB_WAVES) void k_tiff_packbits(const ZStream* __restrict__ st, uint32_t n,
                                                                 const uint8_t* __restrict__ src,
                                                                 uint8_t* __restrict__ dst,
                                                                 uint32_t* __restrict__ err) {
    const uint32_t lane = threadIdx.x & 63, w = rfl(threadIdx.x >> 6);
    const uint32_t si = blockIdx.x * PB_WAVES + w;
    if (si >= n) return;
    const ZStream t = st[si];
    const uint32_t csize = rfl(t.csize), dlen = rfl(t.dlen);
    InWin win{src + t.src_off, w * ZWIN, 0, lane};
    win.load(0);
    uint8_t* __restrict__ out = dst + t.dst_off;
    uint32_t ip = 0, op = 0, bad = 0;
    while (op < dlen) {
        ip = rfl(ip); op = rfl(op);
        if (ip >= csize) { bad = 1; break; }
        if (ip - win.base > ZWIN - 130) win.load(ip);  // (ip never lies below the window's base)
        const uint32_t at = win.wo + ip - win.base;
        const uint32_t h = rfl(zlds[at]);
        ip += 1;
        if (h == 128) continue;
        const bool lit = h < 128;
        const uint32_t cnt = lit ? h + 1 : 257 - h;     // 1 .. 128
        const uint32_t take = lit ? cnt : 1u;           // input bytes after the header
        if (ip + take > csize) { bad = 1; break; }
        if (cnt > dlen - op) { bad = 3; break; }
        // lane l stores bytes l and l + 64 of the run: a literal's from the window, or the one
        // repeated byte
        const uint32_t a = zlds[at + 1 + (lit ? lane : 0u)];
        const uint32_t b = zlds[at + 1 + (lit ? lane + 64 : 0u)];  // (inside the window: at + 129 <= its end)
        if (lane < cnt) out[op + lane] = (uint8_t)a;
        if (lane + 64 < cnt) out[op + lane + 64] = (uint8_t)b;
        ip += take;
        op += cnt;
    }
    if (lane == 0) err[si] = bad;
}

// ----------------------------------------------------------------------- unpack and place
// k_tiff_split_place's geometry and clipping: a workgroup per segment and run of UK_ROWS segment
// rows, a wave per row at a time; rows outside the destination's window [y_lo, y_hi) and the plane
// are neither read nor written, and only the segment's visible width is walked.
// A row is a bit stream, MSB first in II and MM files alike (FillOrder 2: the bits of every byte
// reversed first): sample i (pixel i / S, component i % S) is bits [i * bits, (i + 1) * bits).
// A step is 1024 bytes of every component's output: a lane owns 16 of them (16 / BPP pixels, one
// aligned 16-byte store a component), whose S * 16 / BPP samples lie in (16 / BPP) * S * bits / 8
// whole source bytes, so the wave's 64 spans follow one another from a byte boundary and are at
// most 4096 bytes.  The wave stages them in its own LDS area by 16-byte loads (guarded: strips
// are unaligned and the row's tail is partial), then every lane cuts its samples out of the
// stream: one unaligned LDS dword per sample, byte-swapped, shifted and masked.  No bit cursor
// runs from lane to lane or from sample to sample.
// Values are stored unscaled, uint16 ones in the plane's byte order -- except 16-bit samples,
// which are whole bytes in the FILE's byte order already and keep it (a plain placement, as 8-bit
// ones are: that is how PackBits files of ordinary samples are served).
constexpr uint32_t UK_WAVES = 4, UK_ROWS = 16;  // rows per workgroup
constexpr uint32_t UK_LDS = 4096 + 16;          // a wave's staging area: a step's bytes + a dword's over-read

// the lane's `have` (0 .. 16) bytes at p, the rest zero
__device__ __forceinline__ void packed_load(const uint8_t* p, uint32_t have, uint32_t (&wv)[4]) {
    wv[0] = wv[1] = wv[2] = wv[3] = 0;
    if (have == 16) {
        __builtin_memcpy(wv, p, 16);
    } else {
#pragma unroll
        for (uint32_t b = 0; b < 16; b++)
            if (b < have) wv[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
    }
}

// the bits of every byte of v reversed
__device__ __forceinline__ uint32_t rev_bytes(uint32_t v) { return __builtin_bswap32(__builtin_bitreverse32(v)); }

template <uint32_t BPP, uint32_t S>
__device__ __forceinline__ void unpack_place_row(const uint8_t* __restrict__ row, uint8_t* const (&out)[S],
                                                 uint32_t wanted, uint32_t vis, uint32_t bits, bool rev, bool swap,
                                                 uint32_t lane, uint32_t lo) {
    constexpr uint32_t NP = 16 / BPP;                 // pixels a lane a step
    const uint32_t lbytes = (NP / 8) * S * bits;      // their source bytes
    const uint32_t mask = (1u << bits) - 1;
    for (uint32_t k0 = 0; k0 < vis; k0 += 1024) {     // in a component's row of the plane, bytes
        const uint32_t off = k0 + 16 * lane;
        const uint32_t have = off >= vis ? 0u : vis - off < 16 ? vis - off : 16u;  // a multiple of BPP
        const uint32_t sb0 = (k0 / 16) * lbytes;      // the step's first source byte
        const uint32_t pv = (vis - k0 < 1024 ? vis - k0 : 1024u) / BPP;  // its visible pixels
        const uint32_t need = (pv * S * bits + 7) >> 3;                   // and their source bytes (<= 4096)
        for (uint32_t o0 = 0; o0 < need; o0 += 1024) {
            const uint32_t o = o0 + 16 * lane;
            const uint32_t hv = o >= need ? 0u : need - o < 16 ? need - o : 16u;
            uint32_t wv[4];
            packed_load(row + sb0 + o, hv, wv);
            if (rev) {
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) wv[j] = rev_bytes(wv[j]);
            }
            *(uint4*)(zlds + lo + o) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
        }
        uint32_t b = lane * lbytes * 8;  // the lane's next sample in the staged bytes, in bits
        uint32_t ov[S][4];
#pragma unroll
        for (uint32_t s = 0; s < S; s++) ov[s][0] = ov[s][1] = ov[s][2] = ov[s][3] = 0;
        // four pixels a round (4 * BPP bytes of every component), and the rounds a real loop: unrolled,
        // the 16 / BPP * S offsets and shifts are the same in every step and row, get hoisted out of
        // both loops and cost 128 VGPRs, and all the LDS reads of a step are in flight at once
#pragma unroll 1
        for (uint32_t g = 0; g < NP / 4; g++) {
            uint32_t w0[S], w1[S];
#pragma unroll
            for (uint32_t s = 0; s < S; s++) w0[s] = w1[s] = 0;
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) {
#pragma unroll
                for (uint32_t s = 0; s < S; s++) {
                    const uint32_t be = __builtin_bswap32(ld_u32_unaligned(zlds + lo + (b >> 3)));
                    uint32_t v = (be >> (32 - (b & 7) - bits)) & mask;  // (b & 7) + bits <= 23
                    if (BPP == 2) v = swap ? ((v >> 8) | (v << 8)) & 0xffffu : v;
                    if (BPP == 1) w0[s] |= v << (8 * i);
                    else if (i < 2) w0[s] |= v << (16 * i);
                    else w1[s] |= v << (16 * (i - 2));
                    b += bits;
                }
            }
#pragma unroll
            for (uint32_t s = 0; s < S; s++) {  // (g is wave-uniform; a dynamic index would be scratch)
#pragma unroll
                for (uint32_t q = 0; q < NP / 4; q++) {
                    if (BPP == 1) {
                        ov[s][q] = g == q ? w0[s] : ov[s][q];
                    } else {
                        ov[s][2 * q] = g == q ? w0[s] : ov[s][2 * q];
                        ov[s][2 * q + 1] = g == q ? w1[s] : ov[s][2 * q + 1];
                    }
                }
            }
        }
#pragma unroll
        for (uint32_t s = 0; s < S; s++) {
            if (!((wanted >> s) & 1)) continue;
            uint8_t* o = out[s];
            if (have == 16) {
                *(uint4*)(o + off) = make_uint4(ov[s][0], ov[s][1], ov[s][2], ov[s][3]);
            } else {
#pragma unroll
                for (uint32_t b = 0; b < 16; b++)
                    if (b < have) o[off + b] = (uint8_t)(ov[s][b >> 2] >> (8 * (b & 3)));
            }
        }
    }
}

template <uint32_t BPP, uint32_t S>
__device__ __forceinline__ void unpack_place_rows(const uint8_t* __restrict__ s, uint32_t rb, const TSplitDst& d,
                                                  int32_t x0, int32_t y0, int32_t r0, int32_t r1, uint32_t vis,
                                                  uint32_t bits, bool rev, uint32_t lane, uint32_t w) {
    uint32_t wanted = 0;
#pragma unroll
    for (uint32_t c = 0; c < S; c++) wanted |= d.dev[c] ? 1u << c : 0u;
    wanted = rfl(wanted);
    const bool swap = BPP == 2 && (d.big_endian != 0 || bits == 16);
    for (int32_t r = r0 + (int32_t)w; r < r1; r += (int32_t)UK_WAVES) {
        uint8_t* out[S];
#pragma unroll
        for (uint32_t c = 0; c < S; c++) out[c] = d.dev[c] + (int64_t)(y0 + r) * d.pitch + (int64_t)x0 * BPP;
        unpack_place_row<BPP, S>(s + (uint64_t)r * rb, out, wanted, vis, bits, rev, swap, lane, w * UK_LDS);
    }
}

__global__ __launch_bounds__(64 * UK_WAVES) void k_tiff_unpack_place(const TUnpack* __restrict__ sg,
                                                                     const TSplitDst* __restrict__ dt,
                                                                     const uint8_t* __restrict__ scratch,
                                                                     const uint8_t* __restrict__ input) {
    const uint32_t lane = threadIdx.x & 63, w = rfl(threadIdx.x >> 6);
    const TUnpack u = sg[blockIdx.x];
    const TSplitDst d = dt[rfl(u.dst)];
    const int32_t x0 = (int32_t)rfl((uint32_t)u.x0), y0 = (int32_t)rfl((uint32_t)u.y0);
    const int32_t rows = (int32_t)rfl(u.rows);
    const uint32_t rb = rfl(u.row_bytes), bpp = rfl(d.bpp), spp = rfl(d.spp), bits = rfl(u.bits);
    // segment rows of this run that lie in the window and in the plane
    int32_t r0 = (int32_t)(blockIdx.y * UK_ROWS), r1 = r0 + (int32_t)UK_ROWS;
    const int32_t top = d.y_lo > 0 ? d.y_lo : 0, bottom = d.y_hi < d.sy ? d.y_hi : d.sy;
    r1 = r1 < rows ? r1 : rows;
    r0 = r0 > top - y0 ? r0 : top - y0;
    r1 = r1 < bottom - y0 ? r1 : bottom - y0;
    if (r0 >= r1 || x0 >= d.sx || spp < 1 || spp > 4 || bits < 1 || bits > 16) return;
    if (bpp != (bits > 8 ? 2u : 1u)) return;  // (the planner's rule)
    // a component's visible bytes of a row: the plane's edge or the segment's
    const uint32_t wvis = (uint32_t)(d.sx - x0) * bpp, segb = rfl(u.seg_w) * bpp;
    const uint32_t vis = wvis < segb ? wvis : segb;
    const uint8_t* s = (rfl(u.from_input) ? input : scratch) + u.src;
    const bool rev = rfl(u.fill_order) == 2;
    switch (bpp * 8 + spp) {  // once per workgroup
#define PBX_UNPACK(B, S) case B * 8 + S: unpack_place_rows<B, S>(s, rb, d, x0, y0, r0, r1, vis, bits, rev, lane, w); break;
        PBX_UNPACK(1, 1) PBX_UNPACK(1, 2) PBX_UNPACK(1, 3) PBX_UNPACK(1, 4)
        PBX_UNPACK(2, 1) PBX_UNPACK(2, 2) PBX_UNPACK(2, 3) PBX_UNPACK(2, 4)
#undef PBX_UNPACK
        default: break;
    }
}

hipError_t launch_tiff_packbits(hipStream_t st, const ZStream* d_streams, uint32_t n, const uint8_t* src,
                                uint8_t* scratch, uint32_t* err) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_tiff_packbits, dim3((n + PB_WAVES - 1) / PB_WAVES), dim3(64 * PB_WAVES), PB_WAVES * ZWIN, st,
                       d_streams, n, src, scratch, err);
    return hipGetLastError();
}

hipError_t launch_tiff_unpack_place(hipStream_t st, const TUnpack* d_segs, uint32_t n, uint32_t max_rows,
                                    const TSplitDst* d_dst, const uint8_t* scratch, const uint8_t* input) {
    if (!n || !max_rows) return hipSuccess;
    hipLaunchKernelGGL(k_tiff_unpack_place, dim3(n, (max_rows + UK_ROWS - 1) / UK_ROWS), dim3(64 * UK_WAVES),
                       UK_WAVES * UK_LDS, st, d_segs, d_dst, scratch, input);
    return hipGetLastError();
}

}  // namespace pbx
