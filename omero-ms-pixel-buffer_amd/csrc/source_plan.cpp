// source_plan.cpp — the host-side parsers and planners of the source formats: Zarr chunks (blosc,
// zstd and gzip frames), TIFF strips and tiles, JPEG marker segments and JPEG 2000 codestream
// headers, and the context-free test hooks over them (pbx_test_*_plan, pbx_test_tiff_j2k_decode).
// This is the code that reads file headers as they come.  It is plain C++ built by the host
// compiler alone: no HIP header, no context, no device call, so the sanitizer programs
// (scripts/*_san.cpp, `make san`) build it without the runtime or a kernel.
#include "source_plan.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <tuple>
#include <utility>

#include "tiff_j2k_dev.h"

namespace pbx {

namespace {
thread_local std::string g_err;
}  // namespace

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

std::string& last_error() { return g_err; }

// ------------------------------------------------------------------ NGFF / Zarr planes
namespace {

uint32_t rd_le32(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// One RFC 8878 frame in f[0 .. len) that must decode to cb bytes: the header, then the block
// headers to the frame's end (no block is read).  A frame without a content size passes; the
// decoder's length check decides.
int zstd_frame_check(const uint8_t* f, uint64_t len, uint64_t cb, long long i, const char* what = "chunk") {
    if (len < 6) return fail(PBX_E_BADARG, "%s %lld: short zstd frame", what, i);
    const uint32_t magic = rd_le32(f);
    if ((magic & 0xfffffff0u) == 0x184D2A50u) return fail(PBX_E_BADARG, "%s %lld: skippable zstd frame", what, i);
    if (magic != 0xFD2FB528u) return fail(PBX_E_BADARG, "%s %lld: not a zstd frame", what, i);
    const uint32_t fhd = f[4], fcs_flag = fhd >> 6, single = (fhd >> 5) & 1;
    if (fhd & 3) return fail(PBX_E_BADARG, "%s %lld: zstd frame with a dictionary id", what, i);
    if (fhd & 8) return fail(PBX_E_BADARG, "%s %lld: reserved zstd frame header bit", what, i);
    uint64_t q = 5 + (single ? 0 : 1);
    const uint32_t fcs_size = fcs_flag == 0 ? single : 1u << fcs_flag;
    if (q + fcs_size > len) return fail(PBX_E_BADARG, "%s %lld: short zstd frame", what, i);
    if (fcs_size) {
        uint64_t fcs = 0;
        for (uint32_t k = 0; k < fcs_size; k++) fcs |= (uint64_t)f[q + k] << (8 * k);
        if (fcs_size == 2) fcs += 256;
        if (fcs != cb)
            return fail(PBX_E_BADARG, "%s %lld: zstd content size %llu != %s bytes %llu", what, i,
                        (unsigned long long)fcs, what, (unsigned long long)cb);
    }
    q += fcs_size;
    for (;;) {
        if (q + 3 > len) return fail(PBX_E_BADARG, "%s %lld: truncated zstd frame", what, i);
        const uint32_t bh = (uint32_t)f[q] | (uint32_t)f[q + 1] << 8 | (uint32_t)f[q + 2] << 16;
        const uint32_t type = (bh >> 1) & 3;
        if (type == 3) return fail(PBX_E_BADARG, "%s %lld: reserved zstd block type", what, i);
        q += 3 + (type == 1 ? 1 : bh >> 3);
        if (bh & 1) break;
    }
    if (fhd & 4) q += 4;  // content checksum
    if (q > len) return fail(PBX_E_BADARG, "%s %lld: truncated zstd frame", what, i);
    if (q < len) return fail(PBX_E_BADARG, "%s %lld: %llu bytes after the zstd frame", what, i, (unsigned long long)(len - q));
    return PBX_OK;
}

// One RFC 1952 member in f[0 .. len) that must decode to cb bytes: *body = the first byte of its
// deflate data, *crc = the trailer's CRC-32.  Whether the deflate data ends at the trailer is the
// decoder's to say.
int gzip_member_check(const uint8_t* f, uint64_t len, uint64_t cb, long long i, uint64_t* body, uint32_t* crc) {
    if (len < 18) return fail(PBX_E_BADARG, "chunk %lld: short gzip member", i);
    if (f[0] != 0x1f || f[1] != 0x8b) return fail(PBX_E_BADARG, "chunk %lld: not a gzip member", i);
    if (f[2] != 8) return fail(PBX_E_BADARG, "chunk %lld: gzip compression method %u", i, f[2]);
    const uint32_t flg = f[3];
    if (flg & 0xE0) return fail(PBX_E_BADARG, "chunk %lld: reserved gzip FLG bits 0x%02x", i, flg);
    uint64_t q = 10;
    const uint64_t end = len - 8;  // the trailer
    if (flg & 4) {  // FEXTRA
        if (q + 2 > end) return fail(PBX_E_BADARG, "chunk %lld: truncated gzip header", i);
        q += 2 + ((uint64_t)f[q] | (uint64_t)f[q + 1] << 8);
    }
    for (uint32_t bit : {8u, 16u})  // FNAME, FCOMMENT: zero-terminated
        if (flg & bit) {
            while (q < end && f[q]) q++;
            q++;
        }
    if (flg & 2) q += 2;  // FHCRC
    if (q > end) return fail(PBX_E_BADARG, "chunk %lld: truncated gzip header", i);
    if (rd_le32(f + len - 4) != cb)
        return fail(PBX_E_BADARG, "chunk %lld: gzip ISIZE %u != chunk bytes %llu", i, rd_le32(f + len - 4),
                    (unsigned long long)cb);
    *body = q;
    *crc = rd_le32(f + len - 8);
    return PBX_OK;
}

}  // namespace

// Chunk rows [cy0, cy1) of a plane size_x wide (full width, C order): z->offsets has
// (cy1 - cy0) * gx + 1 entries and z->data holds those chunks only.  Chunk origins are plane
// coordinates.  The whole plane is chunk rows [0, gy).  Every chunk holds `depth` planes
// (slice-major) and gets one ZChunk per wanted plane, all on the one decoded copy.  With
// depth > 1 only the blosc blocks that hold a byte of plane rows [y_lo, y_hi) of a wanted slice
// get streams (include/pbx.h); scratch stays sized and addressed for whole chunks.
int zarr_plan(int32_t size_x, const pbx_zarr_chunks* z, int bpp, uint64_t in_base, int64_t cy0, int64_t cy1,
              int32_t depth, const std::vector<ZarrWant>& want, int64_t y_lo, int64_t y_hi, ZarrPlan& P) {
    const int64_t gx = (size_x + z->chunk_x - 1) / z->chunk_x;
    const int64_t n = gx * (cy1 - cy0);
    const uint64_t pb = (uint64_t)z->chunk_x * z->chunk_y * bpp;  // one plane of the chunk
    if (pb > 0x7fffffffull || pb * (uint64_t)depth > 0x7fffffffull)
        return fail(PBX_E_BADARG, "chunk of %llu bytes too large", (unsigned long long)(pb * (uint64_t)depth));
    const uint64_t cb = pb * (uint64_t)depth, rowb = (uint64_t)z->chunk_x * bpp;
    const uint32_t pe = (uint32_t)z->chunk_x * (uint32_t)z->chunk_y;
    static const bool no_skip = getenv("PBX_ZARR_NO_BLOCK_SKIP") != nullptr;  // A/B: decode every block
    const bool skip = depth > 1 && !no_skip;
    auto emit = [&](ZChunk c) {
        for (const ZarrWant& w : want) {
            c.plane = w.plane;
            c.e0 = w.slice * pe;
            P.chunks.push_back(c);
        }
    };
    const uint64_t total = z->offsets[n];
    for (int64_t i = 0; i < n; i++) {
        const uint64_t o = z->offsets[i];
        uint64_t len = z->offsets[i + 1] - o;
        const uint64_t ob = o + in_base;  // device offset in the launch's upload buffer
        if (z->offsets[i + 1] < o || z->offsets[i + 1] > total)
            return fail(PBX_E_BADARG, "chunk %lld: bad offsets", (long long)i);
        ZChunk c{};
        c.x0 = (int32_t)((i % gx) * z->chunk_x);
        c.y0 = (int32_t)((cy0 + i / gx) * z->chunk_y);
        c.nbytes = (uint32_t)cb;
        c.blocksize = (uint32_t)cb;
        c.typesize = 1;
        if (len == 0) {
            c.flags = ZC_MISSING;
            emit(c);
            continue;
        }
        if (z->flags & PBX_ZARR_F_CRC32C) {  // the last codec of the pipeline: checked on the uploaded bytes
            if (len > 0x7fffffffull) return fail(PBX_E_BADARG, "chunk %lld too large", (long long)i);
            if (len < 4) return fail(PBX_E_BADARG, "chunk %lld: %llu bytes, no room for its crc32c", (long long)i,
                                     (unsigned long long)len);
            len -= 4;
            P.checks[ZK_CRC32C].push_back(ZCheck{ob, (uint32_t)len, rd_le32(z->data + o + len), ZK_INPUT, ZK_CRC32C});
        }
        if (z->codec == PBX_ZARR_RAW) {
            if (len < cb) return fail(PBX_E_BADARG, "chunk %lld: %llu bytes < %llu", (long long)i,
                                      (unsigned long long)len, (unsigned long long)cb);
            c.src = ob;
            c.flags = ZC_INPUT;
            emit(c);
            continue;
        }
        const uint64_t dst = P.scratch;
        if (z->codec == PBX_ZARR_ZLIB || z->codec == PBX_ZARR_ZSTD || z->codec == PBX_ZARR_GZIP) {
            // one stream that decodes to the whole chunk
            if (len > 0xffffffffull) return fail(PBX_E_BADARG, "chunk %lld too large", (long long)i);
            if (z->codec == PBX_ZARR_ZLIB) {
                P.kind[ZS_ZLIB].push_back(ZStream{ob, dst, (uint32_t)len, (uint32_t)cb, ZS_ZLIB, 0});
            } else if (z->codec == PBX_ZARR_ZSTD) {
                if (int rc = zstd_frame_check(z->data + o, len, cb, (long long)i)) return rc;
                P.kind[ZS_ZSTD].push_back(ZStream{ob, dst, (uint32_t)len, (uint32_t)cb, ZS_ZSTD, 0});
            } else {
                uint64_t body = 0;
                uint32_t crc = 0;
                if (int rc = gzip_member_check(z->data + o, len, cb, (long long)i, &body, &crc)) return rc;
                P.kind[ZS_GZIP].push_back(ZStream{ob + body, dst, (uint32_t)(len - body), (uint32_t)cb, ZS_GZIP, 0});
                P.checks[ZK_CRC32].push_back(ZCheck{dst, (uint32_t)cb, crc, ZK_SCRATCH, ZK_CRC32});
            }
            c.src = dst;
            emit(c);
            P.scratch += (cb + 255) & ~255ull;
            continue;
        }
        // blosc 1.x frame
        const uint8_t* f = z->data + o;
        if (len < 16) return fail(PBX_E_BADARG, "chunk %lld: short blosc header", (long long)i);
        const uint32_t ver = f[0], flags = f[2], ts = f[3] ? f[3] : 1;
        const uint32_t nbytes = rd_le32(f + 4), bs = rd_le32(f + 8), cbytes = rd_le32(f + 12);
        if (ver != 2) return fail(PBX_E_BADARG, "chunk %lld: blosc format version %u (c-blosc 1.x writes 2)", (long long)i, ver);
        if (nbytes != cb) return fail(PBX_E_BADARG, "chunk %lld: blosc nbytes %u != chunk bytes %llu",
                                      (long long)i, nbytes, (unsigned long long)cb);
        if (cbytes > len || cbytes < 16) return fail(PBX_E_BADARG, "chunk %lld: blosc cbytes %u", (long long)i, cbytes);
        if (flags & 0x2) {  // memcpyed: the unshuffled chunk follows the header
            if (16ull + nbytes > cbytes) return fail(PBX_E_BADARG, "chunk %lld: short memcpyed frame", (long long)i);
            c.src = ob + 16;
            c.flags = ZC_INPUT;
            emit(c);
            continue;
        }
        const uint32_t codec = flags >> 5;  // 0 blosclz, 1 lz4 / lz4hc, 2 snappy, 3 zlib, 4 zstd
        if (codec != 0 && codec != 1 && codec != 3 && codec != 4)
            return fail(PBX_E_BADARG, "chunk %lld: blosc codec %u not supported (blosclz/lz4/lz4hc/zlib/zstd)",
                        (long long)i, codec);
        static const uint32_t kind_of[5] = {ZS_BLOSCLZ, ZS_LZ4, 0, ZS_ZLIB, ZS_ZSTD};
        if (bs == 0 || bs > nbytes || (bs % ts)) return fail(PBX_E_BADARG, "chunk %lld: blosc blocksize %u", (long long)i, bs);
        const uint32_t nblocks = (nbytes + bs - 1) / bs, leftover = nbytes % bs;
        if (16ull + 4ull * nblocks > cbytes) return fail(PBX_E_BADARG, "chunk %lld: short block table", (long long)i);
        // the chunk's rows of the wanted window, the same in every wanted slice
        const int64_t ra = std::max<int64_t>(y_lo - c.y0, 0), rb = std::min<int64_t>(y_hi - c.y0, z->chunk_y);
        for (uint32_t b = 0; b < nblocks; b++) {
            const bool is_left = leftover && b == nblocks - 1;
            const uint32_t bsize = is_left ? leftover : bs;
            if (skip) {
                const uint64_t b0 = (uint64_t)b * bs, b1 = b0 + bsize;
                bool needed = false;
                for (size_t k = 0; k < want.size() && !needed && ra < rb; k++) {
                    const uint64_t s0 = want[k].slice * pb;
                    needed = b0 < s0 + (uint64_t)rb * rowb && s0 + (uint64_t)ra * rowb < b1;
                }
                if (!needed) {
                    P.skipped++;
                    continue;
                }
            }
            const bool split = !(flags & 0x10) && ts <= 16 && bsize / ts >= 128 && !is_left;
            const uint32_t nsp = split ? ts : 1, neb = bsize / nsp;
            if (neb * nsp != bsize) return fail(PBX_E_BADARG, "chunk %lld: block %u not a multiple of typesize", (long long)i, b);
            uint64_t pos = rd_le32(f + 16 + 4 * b);
            for (uint32_t s = 0; s < nsp; s++) {
                if (pos + 4 > cbytes) return fail(PBX_E_BADARG, "chunk %lld: block %u truncated", (long long)i, b);
                const uint32_t cs = rd_le32(f + pos);
                pos += 4;
                if (pos + cs > cbytes || cs > neb || cs == 0)
                    return fail(PBX_E_BADARG, "chunk %lld: block %u split %u size %u", (long long)i, b, s, cs);
                const uint32_t k = cs == neb ? ZS_COPY : kind_of[codec];
                P.kind[k].push_back(ZStream{ob + pos, dst + (uint64_t)b * bs + (uint64_t)s * neb, cs, neb, k, 0});
                pos += cs;
            }
        }
        c.src = dst;
        c.blocksize = bs;
        if (flags & 0x4) {  // bit shuffle (takes precedence over the byte-shuffle bit)
            c.flags |= ZC_BITSHUF;
            c.typesize = ts;
        } else {
            c.typesize = (flags & 0x1) ? ts : 1;
        }
        emit(c);
        P.scratch += (cb + 255) & ~255ull;
    }
    return PBX_OK;
}

// pbx_zarr_chunks fields that can be checked without the plane.
int zarr_chunks_check(const pbx_zarr_chunks* z) {
    if (!z->offsets || (!z->data && (z->codec != PBX_ZARR_RAW || z->flags))) return fail(PBX_E_BADARG, "null argument");
    if (z->chunk_x <= 0 || z->chunk_y <= 0) return fail(PBX_E_BADARG, "bad chunk shape");
    if (z->codec < PBX_ZARR_RAW || z->codec > PBX_ZARR_GZIP) return fail(PBX_E_BADARG, "bad codec %d", z->codec);
    if (z->flags & ~PBX_ZARR_F_CRC32C) return fail(PBX_E_BADARG, "bad flags 0x%x", (unsigned)z->flags);
    return PBX_OK;
}

// A slice of chunks that hold `depth` planes.
int zarr_slice_check(int32_t depth, int64_t slice) {
    if (depth < 1) return fail(PBX_E_BADARG, "chunk_planes %d < 1", depth);
    if (slice < 0 || slice >= depth) return fail(PBX_E_BADARG, "slice %lld outside chunks of %d planes", (long long)slice, depth);
    return PBX_OK;
}

// ------------------------------------------------------------------ TIFF / OME-TIFF planes
static_assert(sizeof(pbx_tiff_segments) == 40, "pbx_tiff_segments is part of the C-ABI (ctypes mirror PbxTiffSegments)");
// pbx_tiff_segments fields that can be checked without the plane.
// (packed: the pbx_*_tiff_packed calls, which take PackBits too and predictor 1 alone)
static int tiff_segments_check_as(const pbx_tiff_segments* s, bool packed) {
    if (!s->data || !s->offsets) return fail(PBX_E_BADARG, "null argument");
    if (s->seg_w < 1 || s->seg_h < 1) return fail(PBX_E_BADARG, "bad segment shape %d x %d", s->seg_w, s->seg_h);
    if (s->tiled && ((s->seg_w | s->seg_h) & 15))
        return fail(PBX_E_BADARG, "tile %d x %d: TileWidth and TileLength must be multiples of 16 (TIFF 6.0 section 15)",
                    s->seg_w, s->seg_h);
    if (s->compression != PBX_TIFF_NONE && s->compression != PBX_TIFF_LZW && s->compression != PBX_TIFF_DEFLATE &&
        s->compression != PBX_TIFF_ZSTD && !(packed && s->compression == PBX_TIFF_PACKBITS))
        return fail(PBX_E_BADARG, packed ? "bad compression %d (1 none, 5 LZW, 8 deflate, 50000 zstd, 32773 PackBits)"
                                         : "bad compression %d (1 none, 5 LZW, 8 deflate, 50000 zstd)", s->compression);
    if (packed && s->predictor != 1)
        return fail(PBX_E_BADARG, "bad predictor %d (bit-packed samples take 1 only: the predictor is defined on "
                                  "whole-byte samples)", s->predictor);
    if (s->predictor < 1 || s->predictor > 3)
        return fail(PBX_E_BADARG, "bad predictor %d (1, 2, or 3 on float and double planes)", s->predictor);
    if (s->flags) return fail(PBX_E_BADARG, "bad flags 0x%x", (unsigned)s->flags);
    return PBX_OK;
}

int tiff_segments_check(const pbx_tiff_segments* s) { return tiff_segments_check_as(s, false); }

// A sample of chunky segments that hold spp samples per pixel, on a plane of bpp bytes a sample.
int tiff_samples_check(int32_t spp, int64_t sample, int bpp) {
    if (spp < 1 || spp > 4) return fail(PBX_E_BADARG, "samples_per_pixel %d outside 1 .. 4", spp);
    if (sample < 0 || sample >= spp)
        return fail(PBX_E_BADARG, "sample %lld outside segments of %d samples per pixel", (long long)sample, spp);
    if (spp > 1 && bpp == 8) return fail(PBX_E_BADARG, "samples_per_pixel %d on 64-bit samples", spp);
    return PBX_OK;
}

// Predictor = 3 (the floating-point predictor) is defined on IEEE samples only.
int tiff_fp_predictor_check(const pbx_tiff_segments* s, int32_t pixel_type) {
    if (s->predictor == 3 && pixel_type != PBX_FLOAT && pixel_type != PBX_DOUBLE)
        return fail(PBX_E_BADARG, "bad predictor 3 (the floating-point predictor) on a plane of integer samples");
    return PBX_OK;
}

// Host plan of one plane's strips or tiles: one stream per segment (its own row count: the last
// strip holds only the rows left), one ZChunk to place it, and for Predictor = 2 its rows for
// k_tiff_unpred.  No byte of segment data is decoded here.
// With `band` (pbx_band_write_tiff) s->data / s->offsets hold segment rows [sr0, sr1) only, and
// nothing is copied or rewritten in scratch: a stored segment is read where it was uploaded
// (ZC_INPUT, no stream, no scratch), and with Predictor = 2 every segment goes into P.uplace for
// k_tiff_unpred_place instead of P.unpred and P.chunks.  Segment numbers in messages count from
// the first segment handed over.
// With spp > 1 (chunky samples) a segment row holds spp samples per pixel, and registration and
// band writes are planned alike: a stored segment is read where it was uploaded, and every
// segment, whatever the predictor, goes into P.split for k_tiff_split_place with `dst` as its
// entry in the launch's TSplitDst table.
// Compression 50000 is one zstd frame per segment (zstd_frame_check, then ZS_ZSTD), under any
// predictor.  Predictor = 3 (bpp 4 or 8, spp 1) is planned as spp > 1 is, registration and band
// writes alike: a stored segment is read where it was uploaded, no TUnpred and no ZChunk, every
// segment a TPlace in P.fplace for k_tiff_fpunpred_place, its destination ZPlane `plane`.
int tiff_plan(int32_t size_x, int32_t size_y, int bpp, bool big_endian, const pbx_tiff_segments* s,
              uint64_t in_base, uint32_t plane, ZarrPlan& P, uint64_t* dlen_sum, bool band, int64_t sr0,
              int64_t sr1, int spp, uint32_t split_dst) {
    if (!s->tiled && s->seg_w != size_x)
        return fail(PBX_E_BADARG, "strip width %d != plane width %d", s->seg_w, size_x);
    if (s->predictor == 2 && bpp == 8) return fail(PBX_E_BADARG, "predictor 2 on floating-point samples");
    const bool fp = s->predictor == 3;
    if (fp && bpp != 4 && bpp != 8)
        return fail(PBX_E_BADARG, "bad predictor 3 (the floating-point predictor) on %d-byte samples", bpp);
    if (fp && spp != 1)
        return fail(PBX_E_BADARG, "bad predictor 3 (the floating-point predictor) on chunky segments of %d samples "
                                  "per pixel", spp);
    if (fp) {  // the call's destination: the rest of it comes from ZPlane `plane` at the launch
        P.fdst.push_back(TPlaceDst{nullptr, 0, 0, 0, 0, 0, (uint32_t)bpp, big_endian ? 1u : 0u});
        P.fdst_plane.push_back(plane);
    }
    const int64_t gx = s->tiled ? ((int64_t)size_x + s->seg_w - 1) / s->seg_w : 1;
    const int64_t gy = ((int64_t)size_y + s->seg_h - 1) / s->seg_h;
    if (sr1 < 0) sr1 = gy;
    const int64_t n = gx * (sr1 - sr0);
    const uint64_t total = s->offsets[n];
    for (int64_t i = 0; i < n; i++) {
        const uint64_t o = s->offsets[i], len = s->offsets[i + 1] - o;
        if (s->offsets[i + 1] < o || s->offsets[i + 1] > total)
            return fail(PBX_E_BADARG, "segment %lld: bad offsets", (long long)i);
        if (len == 0) return fail(PBX_E_BADARG, "segment %lld is empty", (long long)i);
        const int32_t x0 = (int32_t)((i % gx) * s->seg_w), y0 = (int32_t)((sr0 + i / gx) * s->seg_h);
        const int32_t rows = s->tiled ? s->seg_h : std::min(s->seg_h, size_y - y0);
        const uint64_t dlen = (uint64_t)s->seg_w * (uint64_t)rows * (uint64_t)bpp * (uint64_t)spp;
        if (dlen > 0x7fffffffull || len > 0x7fffffffull || rows > (65535 << 4))
            return fail(PBX_E_BADARG, "segment %lld too large", (long long)i);
        const uint64_t ob = o + in_base;
        const bool in_place = (band || spp > 1 || fp) && s->compression == PBX_TIFF_NONE;  // read from the upload buffer
        const uint64_t dst = in_place ? ob : P.scratch;
        uint32_t kind = ZS_COPY;
        if (s->compression == PBX_TIFF_NONE) {
            if (len != dlen)
                return fail(PBX_E_BADARG, "uncompressed segment %lld: %llu bytes, not %llu", (long long)i,
                            (unsigned long long)len, (unsigned long long)dlen);
        } else if (s->compression == PBX_TIFF_LZW) {
            // libtiff's test for the pre-6.0 bit order (LSB first, which begins 00 01 for Clear)
            if (len >= 2 && s->data[o] == 0 && (s->data[o + 1] & 1))
                return fail(PBX_E_BADARG, "segment %lld: old-style (pre-6.0, LSB-first) LZW", (long long)i);
            kind = ZS_LZW;
        } else if (s->compression == PBX_TIFF_ZSTD) {
            // one frame that decodes to the segment (a content size, if the frame has one, is dlen)
            if (int rc = zstd_frame_check(s->data + o, len, dlen, (long long)i, "segment")) return rc;
            kind = ZS_ZSTD;
        } else {
            kind = ZS_ZLIB;
        }
        if (!in_place) P.kind[kind].push_back(ZStream{ob, dst, (uint32_t)len, (uint32_t)dlen, kind, 0});
        if (dlen_sum) *dlen_sum += dlen;
        if (!in_place) P.scratch += (dlen + 255) & ~255ull;
        if (spp > 1) {
            P.split.push_back(TPlace{dst, (uint32_t)s->seg_w * (uint32_t)bpp * (uint32_t)spp, (uint32_t)rows, x0, y0,
                                     in_place ? 1u : 0u, split_dst});
            P.split_rows = std::max(P.split_rows, (uint32_t)rows);
            continue;
        }
        if (fp) {
            P.fplace.push_back(TPlace{dst, (uint32_t)s->seg_w * (uint32_t)bpp, (uint32_t)rows, x0, y0,
                                      in_place ? 1u : 0u, (uint32_t)P.fdst.size() - 1});
            P.fplace_rows = std::max(P.fplace_rows, (uint32_t)rows);
            continue;
        }
        if (band && s->predictor == 2) {
            P.uplace.push_back(TPlace{dst, (uint32_t)s->seg_w * (uint32_t)bpp, (uint32_t)rows, x0, y0,
                                      in_place ? 1u : 0u, 0});
            P.uplace_rows = std::max(P.uplace_rows, (uint32_t)rows);
            P.uplace_big_endian = big_endian;
            continue;
        }
        ZChunk c{};
        c.src = dst;
        c.nbytes = c.blocksize = (uint32_t)dlen;
        c.typesize = 1;
        c.flags = in_place ? ZC_INPUT : 0u;
        c.x0 = x0;
        c.y0 = y0;
        c.plane = plane;
        P.chunks.push_back(c);
        if (s->predictor == 2) {
            P.unpred.push_back(TUnpred{dst, (uint32_t)s->seg_w * (uint32_t)bpp, (uint32_t)rows, (uint32_t)bpp,
                                       big_endian ? 1u : 0u});
            P.unpred_rows = std::max(P.unpred_rows, (uint32_t)rows);
        }
    }
    return PBX_OK;
}

// ------------------------------------------------------- bit-packed samples and PackBits
static_assert(sizeof(pbx_tiff_packed) == 16, "pbx_tiff_packed is part of the C-ABI (ctypes mirror PbxTiffPacked)");
int tiff_packed_check(const pbx_tiff_segments* s, const pbx_tiff_packed* k, int32_t pixel_type) {
    if (int rc = tiff_segments_check_as(s, true)) return rc;
    if (k->bits < 1 || k->bits > 16) return fail(PBX_E_BADARG, "bad bits %d (1 .. 16)", k->bits);
    const bool integer = pixel_type >= PBX_INT8 && pixel_type <= PBX_UINT16;
    if (!integer || bpp_of(pixel_type) != (k->bits > 8 ? 2 : 1))
        return fail(PBX_E_BADARG, "%d-bit samples on a plane of pixel type %d (1 .. 8 bits take an 8-bit integer "
                                  "plane, 9 .. 16 a 16-bit one)", k->bits, pixel_type);
    if (k->fill_order != 1 && k->fill_order != 2) return fail(PBX_E_BADARG, "bad fill_order %d (1 or 2)", k->fill_order);
    if (k->fill_order == 2 && k->bits == 16)
        return fail(PBX_E_BADARG, "fill_order 2 on 16-bit samples (their bytes are in the file's order, not a bit "
                                  "stream's)");
    return PBX_OK;
}

// Host plan of the segment rows [sr0, sr1) (sr1 < 0: all) of bit-packed samples: tiff_plan's
// geometry with rows of ceil(seg_w * spp * bits / 8) bytes, so a decoder's dlen is rows times
// that.  Registration and band writes are planned alike, as chunky segments are: a stored segment
// is read where it was uploaded (its length must be its rows' padded bytes), a compressed one gets
// a stream (ZS_LZW, ZS_ZLIB, ZS_ZSTD or ZS_PACKBITS) into scratch, and every segment a TUnpack for
// k_tiff_unpack_place with `dst` as its entry in the launch's TSplitDst table.
int tiff_packed_plan(int32_t size_x, int32_t size_y, const pbx_tiff_segments* s, const pbx_tiff_packed* k,
                     uint64_t in_base, ZarrPlan& P, int64_t sr0, int64_t sr1, int spp, uint32_t dst,
                     uint64_t* dlen_sum) {
    if (!s->tiled && s->seg_w != size_x)
        return fail(PBX_E_BADARG, "strip width %d != plane width %d", s->seg_w, size_x);
    const int64_t gx = s->tiled ? ((int64_t)size_x + s->seg_w - 1) / s->seg_w : 1;
    const int64_t gy = ((int64_t)size_y + s->seg_h - 1) / s->seg_h;
    if (sr1 < 0) sr1 = gy;
    const int64_t n = gx * (sr1 - sr0);
    const uint64_t total = s->offsets[n];
    const uint64_t rb = tiff_packed_row_bytes(s->seg_w, spp, k->bits);
    for (int64_t i = 0; i < n; i++) {
        const uint64_t o = s->offsets[i], len = s->offsets[i + 1] - o;
        if (s->offsets[i + 1] < o || s->offsets[i + 1] > total)
            return fail(PBX_E_BADARG, "segment %lld: bad offsets", (long long)i);
        if (len == 0) return fail(PBX_E_BADARG, "segment %lld is empty", (long long)i);
        const int32_t x0 = (int32_t)((i % gx) * s->seg_w), y0 = (int32_t)((sr0 + i / gx) * s->seg_h);
        const int32_t rows = s->tiled ? s->seg_h : std::min(s->seg_h, size_y - y0);
        const uint64_t dlen = rb * (uint64_t)rows;
        if (rb > 0x7fffffffull || dlen > 0x7fffffffull || len > 0x7fffffffull || rows > (65535 << 4))
            return fail(PBX_E_BADARG, "segment %lld too large", (long long)i);
        const uint64_t ob = o + in_base;
        const bool in_place = s->compression == PBX_TIFF_NONE;  // read from the upload buffer
        if (in_place) {
            if (len != dlen)
                return fail(PBX_E_BADARG, "uncompressed segment %lld: %llu bytes, not %llu (%d rows of %llu bytes: "
                                          "%d samples of %d bits, padded to a byte)", (long long)i,
                            (unsigned long long)len, (unsigned long long)dlen, rows, (unsigned long long)rb,
                            s->seg_w * spp, k->bits);
        } else {
            uint32_t kind = ZS_ZLIB;
            if (s->compression == PBX_TIFF_LZW) {
                // libtiff's test for the pre-6.0 bit order (LSB first, which begins 00 01 for Clear)
                if (len >= 2 && s->data[o] == 0 && (s->data[o + 1] & 1))
                    return fail(PBX_E_BADARG, "segment %lld: old-style (pre-6.0, LSB-first) LZW", (long long)i);
                kind = ZS_LZW;
            } else if (s->compression == PBX_TIFF_ZSTD) {
                if (int rc = zstd_frame_check(s->data + o, len, dlen, (long long)i, "segment")) return rc;
                kind = ZS_ZSTD;
            } else if (s->compression == PBX_TIFF_PACKBITS) {
                kind = ZS_PACKBITS;
            }
            P.kind[kind].push_back(ZStream{ob, P.scratch, (uint32_t)len, (uint32_t)dlen, kind, 0});
        }
        P.unpack.push_back(TUnpack{in_place ? ob : P.scratch, (uint32_t)rb, (uint32_t)rows, x0, y0, in_place ? 1u : 0u, dst,
                                   (uint32_t)s->seg_w, (uint32_t)k->bits, (uint32_t)k->fill_order, 0});
        P.unpack_rows = std::max(P.unpack_rows, (uint32_t)rows);
        if (!in_place) P.scratch += (dlen + 255) & ~255ull;
        if (dlen_sum) *dlen_sum += dlen;
    }
    return PBX_OK;
}

// ------------------------------------------------------- JPEG-compressed TIFF segments
// Compression = 7 (TIFF Technical Note 2): every strip or tile is a JPEG stream of its own, the
// tables usually once per IFD in tag 347 (JPEGTables: SOI, DQT / DHT segments, EOI) and the
// segments abbreviated.  The host reads marker segments only -- never a byte of entropy-coded
// data, restart markers included -- and every length is checked against the bytes it lies in.
static_assert(sizeof(pbx_tiff_jpeg) == 24, "pbx_tiff_jpeg is part of the C-ABI (ctypes mirror PbxTiffJpeg)");

namespace {

// The quantisers and Huffman codes in force: tag 347's, then overridden by the segment's own.
struct JpegTables {
    bool qset[4] = {false, false, false, false};
    uint16_t q[4][64];  // in zigzag order, as stored
    bool hset[2][4] = {{false, false, false, false}, {false, false, false, false}};  // [DC / AC][Th]
    uint8_t bits[2][4][17];
    uint8_t vals[2][4][256];
};

// A segment's header up to the scan's entropy-coded data.
struct JpegHeader {
    uint32_t width = 0, height = 0, ncomp = 0;
    uint32_t h[3] = {0, 0, 0}, v[3] = {0, 0, 0}, tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    uint32_t restart = 0;
    uint64_t data = 0;  // offset of the entropy-coded data in the segment
};

// DQT payload p[0 .. len)
int jpeg_dqt(const uint8_t* p, uint64_t len, JpegTables& T, const char* what) {
    uint64_t q = 0;
    while (q < len) {
        const uint32_t pq = p[q] >> 4, tq = p[q] & 15;
        if (pq > 1 || tq > 3) return fail(PBX_E_BADARG, "%s: bad DQT (Pq %u, Tq %u)", what, pq, tq);
        if (pq == 1) return fail(PBX_E_BADARG, "%s: 16-bit quantiser (DQT with Pq = 1) is not supported", what);
        if (q + 65 > len) return fail(PBX_E_BADARG, "%s: truncated DQT", what);
        for (int k = 0; k < 64; k++) T.q[tq][k] = p[q + 1 + k];
        T.qset[tq] = true;
        q += 65;
    }
    return PBX_OK;
}

// DHT payload p[0 .. len): counts per length, then the symbols; the Kraft sum of every table
int jpeg_dht(const uint8_t* p, uint64_t len, JpegTables& T, const char* what) {
    uint64_t q = 0;
    while (q < len) {
        const uint32_t tc = p[q] >> 4, th = p[q] & 15;
        if (tc > 1 || th > 3) return fail(PBX_E_BADARG, "%s: bad DHT (Tc %u, Th %u)", what, tc, th);
        if (q + 17 > len) return fail(PBX_E_BADARG, "%s: truncated DHT", what);
        uint32_t n = 0, kraft = 0;
        T.bits[tc][th][0] = 0;
        for (int l = 1; l <= 16; l++) {
            T.bits[tc][th][l] = p[q + l];
            n += p[q + l];
            kraft += (uint32_t)p[q + l] << (16 - l);
        }
        if (n > 256 || kraft > 65536)
            return fail(PBX_E_BADARG, "%s: over-subscribed Huffman table (%s %u: %u codes, Kraft sum %u / 65536)", what,
                        tc ? "AC" : "DC", th, n, kraft);
        if (q + 17 + n > len) return fail(PBX_E_BADARG, "%s: truncated DHT", what);
        memset(T.vals[tc][th], 0, 256);
        memcpy(T.vals[tc][th], p + q + 17, n);
        T.hset[tc][th] = true;
        q += 17 + n;
    }
    return PBX_OK;
}

// The marker at f[q ..] (fill bytes before it skipped): its code, and for one with a length its
// payload [*pay, *pay + *plen); q moves past it.  400 if it or its payload leaves f[0 .. len).
int jpeg_next_marker(const uint8_t* f, uint64_t len, uint64_t& q, uint32_t* code, uint64_t* pay, uint64_t* plen,
                     const char* what) {
    if (q >= len || f[q] != 0xFF) return fail(PBX_E_BADARG, "%s: truncated header (no marker at byte %llu)", what, (unsigned long long)q);
    while (q < len && f[q] == 0xFF) q++;
    if (q >= len) return fail(PBX_E_BADARG, "%s: truncated header", what);
    *code = f[q++];
    *pay = q;
    *plen = 0;
    if (*code == 0xD8 || *code == 0xD9 || *code == 0x01 || (*code >= 0xD0 && *code <= 0xD7)) return PBX_OK;
    if (*code == 0) return fail(PBX_E_BADARG, "%s: FF 00 where a marker should stand", what);
    if (q + 2 > len) return fail(PBX_E_BADARG, "%s: truncated header", what);
    const uint32_t L = (uint32_t)f[q] << 8 | f[q + 1];
    if (L < 2 || q + L > len) return fail(PBX_E_BADARG, "%s: truncated header (marker FF %02X of %u bytes)", what, *code, L);
    *pay = q + 2;
    *plen = L - 2;
    q += L;
    return PBX_OK;
}

// Tag 347: SOI, table segments, EOI.
int jpeg_parse_tables(const uint8_t* f, uint64_t len, JpegTables& T) {
    const char* what = "JPEGTables";
    if (len < 2 || f[0] != 0xFF || f[1] != 0xD8) return fail(PBX_E_BADARG, "%s does not start with SOI", what);
    uint64_t q = 2;
    for (;;) {
        uint32_t code;
        uint64_t pay, plen;
        if (int rc = jpeg_next_marker(f, len, q, &code, &pay, &plen, what)) return rc;
        if (code == 0xD9) return PBX_OK;
        if (code == 0xDB) { if (int rc = jpeg_dqt(f + pay, plen, T, what)) return rc; }
        else if (code == 0xC4) { if (int rc = jpeg_dht(f + pay, plen, T, what)) return rc; }
        else if (code == 0xDA || (code >= 0xC0 && code <= 0xCF && code != 0xC8))
            return fail(PBX_E_BADARG, "%s: marker FF %02X in a tables-only stream", what, code);
    }
}

// A segment's marker segments up to and including the SOS header.  T (may be null) takes its
// DQT / DHT; *own says whether it has any (with T null they are stepped over, length-checked
// like every marker segment, and left for a second walk that has somewhere to put them).
int jpeg_parse_header(const uint8_t* f, uint64_t len, JpegTables* T, bool* own, JpegHeader& H, const char* what) {
    if (len < 2 || f[0] != 0xFF || f[1] != 0xD8) return fail(PBX_E_BADARG, "%s does not start with SOI (Compression 7)", what);
    uint64_t q = 2;
    bool sof = false;
    uint32_t cid[3] = {0, 0, 0};
    for (;;) {
        uint32_t code;
        uint64_t pay, plen;
        if (int rc = jpeg_next_marker(f, len, q, &code, &pay, &plen, what)) return rc;
        const uint8_t* p = f + pay;
        if (code == 0xDB || code == 0xC4) {
            *own = true;
            if (T)
                if (int rc = code == 0xDB ? jpeg_dqt(p, plen, *T, what) : jpeg_dht(p, plen, *T, what)) return rc;
            continue;
        }
        if (code == 0xDD) {
            if (plen != 2) return fail(PBX_E_BADARG, "%s: bad DRI", what);
            H.restart = (uint32_t)p[0] << 8 | p[1];
            continue;
        }
        if (code == 0xCC) return fail(PBX_E_BADARG, "%s: arithmetic coding (DAC) is not supported", what);
        if (code >= 0xC1 && code <= 0xCF && code != 0xC8) {
            static const char* names[16] = {"", "SOF1 (extended sequential)", "SOF2 (progressive)", "SOF3 (lossless)", "",
                                            "SOF5 (differential)", "SOF6 (differential progressive)", "SOF7 (differential lossless)",
                                            "", "SOF9 (arithmetic coding)", "SOF10 (progressive, arithmetic coding)",
                                            "SOF11 (lossless, arithmetic coding)", "", "SOF13 (arithmetic coding)",
                                            "SOF14 (arithmetic coding)", "SOF15 (arithmetic coding)"};
            return fail(PBX_E_BADARG, "%s: %s is not supported (baseline SOF0 only)", what, names[code & 15]);
        }
        if (code == 0xC0) {
            if (sof) return fail(PBX_E_BADARG, "%s: two SOF markers", what);
            if (plen < 6) return fail(PBX_E_BADARG, "%s: truncated SOF", what);
            if (p[0] != 8) return fail(PBX_E_BADARG, "%s: sample precision %u (8 only)", what, p[0]);
            H.height = (uint32_t)p[1] << 8 | p[2];
            H.width = (uint32_t)p[3] << 8 | p[4];
            H.ncomp = p[5];
            if (H.ncomp == 4) return fail(PBX_E_BADARG, "%s: 4 components (CMYK / YCCK) are not supported", what);
            if (H.ncomp != 1 && H.ncomp != 3) return fail(PBX_E_BADARG, "%s: %u components (1 or 3)", what, H.ncomp);
            if (plen != 6 + 3ull * H.ncomp) return fail(PBX_E_BADARG, "%s: truncated SOF", what);
            for (uint32_t c = 0; c < H.ncomp; c++) {
                cid[c] = p[6 + 3 * c];
                H.h[c] = p[7 + 3 * c] >> 4;
                H.v[c] = p[7 + 3 * c] & 15;
                H.tq[c] = p[8 + 3 * c];
                if (H.tq[c] > 3) return fail(PBX_E_BADARG, "%s: component %u names quantiser %u", what, c, H.tq[c]);
            }
            sof = true;
            continue;
        }
        if (code == 0xDA) {
            if (!sof) return fail(PBX_E_BADARG, "%s: SOS before SOF", what);
            if (plen < 1) return fail(PBX_E_BADARG, "%s: truncated SOS", what);
            const uint32_t ns = p[0];
            if (ns != H.ncomp)
                return fail(PBX_E_BADARG, "%s: more than one scan (the first holds %u of %u components)", what, ns, H.ncomp);
            if (plen != 4 + 2ull * ns) return fail(PBX_E_BADARG, "%s: truncated SOS", what);
            for (uint32_t c = 0; c < ns; c++) {
                if (p[1 + 2 * c] != cid[c]) return fail(PBX_E_BADARG, "%s: the scan's components are not the frame's, in order", what);
                H.td[c] = p[2 + 2 * c] >> 4;
                H.ta[c] = p[2 + 2 * c] & 15;
                if (H.td[c] > 3 || H.ta[c] > 3) return fail(PBX_E_BADARG, "%s: component %u names Huffman tables %u / %u", what, c, H.td[c], H.ta[c]);
            }
            if (p[1 + 2 * ns] != 0 || p[2 + 2 * ns] != 63 || p[3 + 2 * ns] != 0)
                return fail(PBX_E_BADARG, "%s: a scan of coefficients %u .. %u, Ah/Al 0x%02x (sequential: 0 .. 63, 0)", what,
                            p[1 + 2 * ns], p[2 + 2 * ns], p[3 + 2 * ns]);
            H.data = q;
            return PBX_OK;
        }
        if (code == 0xD9) return fail(PBX_E_BADARG, "%s: EOI before any scan", what);
        if (code == 0xD8 || code == 0x01 || (code >= 0xD0 && code <= 0xD7))
            return fail(PBX_E_BADARG, "%s: marker FF %02X in the header", what, code);
        // APPn, COM and anything else with a length: skipped
    }
}

// The decoder's form of one canonical code (JHuff, pbx_decode_types.h).
void jpeg_build_huff(const uint8_t* bits, const uint8_t* vals, JHuff& h) {
    memset(&h, 0, sizeof h);
    uint32_t code = 0, p = 0;
    for (int l = 1; l <= 16; l++) {
        h.maxcode[l] = -1;
        h.valoff[l] = (int32_t)p - (int32_t)code;
        for (uint32_t i = 0; i < bits[l]; i++, p++, code++)
            if (l <= 9)
                for (uint32_t k = 0; k < (1u << (9 - l)); k++) h.lut[(code << (9 - l)) + k] = (uint16_t)(l << 8 | vals[p]);
        if (bits[l]) h.maxcode[l] = (int32_t)code - 1;
        code <<= 1;
    }
    memcpy(h.val, vals, 256);
}

}  // namespace

// pbx_tiff_segments / pbx_tiff_jpeg fields of a JPEG layer that can be checked without the plane.
int tiff_jpeg_check(const pbx_tiff_segments* s, const pbx_tiff_jpeg* j, int32_t pixel_type, int32_t spp) {
    if (!s->data || !s->offsets || !j) return fail(PBX_E_BADARG, "null argument");
    if (s->seg_w < 1 || s->seg_h < 1) return fail(PBX_E_BADARG, "bad segment shape %d x %d", s->seg_w, s->seg_h);
    if (s->tiled && ((s->seg_w | s->seg_h) & 15))
        return fail(PBX_E_BADARG, "tile %d x %d: TileWidth and TileLength must be multiples of 16 (TIFF 6.0 section 15)",
                    s->seg_w, s->seg_h);
    if (s->compression != PBX_TIFF_JPEG) return fail(PBX_E_BADARG, "bad compression %d (the JPEG calls take 7)", s->compression);
    if (s->predictor != 1) return fail(PBX_E_BADARG, "bad predictor %d on JPEG segments (1 only)", s->predictor);
    if (s->flags) return fail(PBX_E_BADARG, "bad flags 0x%x", (unsigned)s->flags);
    if (j->reserved || (j->ycbcr != 0 && j->ycbcr != 1)) return fail(PBX_E_BADARG, "bad pbx_tiff_jpeg (ycbcr %d, reserved %d)", j->ycbcr, j->reserved);
    if (!j->tables && j->tables_len) return fail(PBX_E_BADARG, "null argument");
    if (pixel_type != PBX_UINT8) return fail(PBX_E_BADARG, "JPEG segments on a plane that is not uint8");
    if (spp != 1 && spp != 3) return fail(PBX_E_BADARG, "JPEG segments of %d samples per pixel (1 or 3)", spp);
    if (j->ycbcr && spp != 3) return fail(PBX_E_BADARG, "YCbCr (PhotometricInterpretation 6) with %d samples per pixel", spp);
    return PBX_OK;
}

// Host plan of the JPEG segment rows [sr0, sr1) (sr1 < 0: all) of a uint8 plane: tiff_plan's
// geometry, one JStream and one TJpegSeg per segment, table sets shared between the segments (and
// layers) whose resolved tables are the same bytes.  Every refusal is made here, before anything
// is uploaded.  Scratch holds one byte per decoded sample of every component, rows and columns
// padded to whole MCUs (pitches to 16, planes to 256 bytes).
int tiff_jpeg_plan(int32_t size_x, int32_t size_y, const pbx_tiff_segments* s, const pbx_tiff_jpeg* j, uint64_t in_base,
                   ZarrPlan& P, int64_t sr0, int64_t sr1, int spp, uint32_t dst, uint64_t* dlen_sum) {
    if (!s->tiled && s->seg_w != size_x)
        return fail(PBX_E_BADARG, "strip width %d != plane width %d", s->seg_w, size_x);
    JpegTables base;
    if (j->tables && j->tables_len)
        if (int rc = jpeg_parse_tables(j->tables, j->tables_len, base)) return rc;
    std::vector<std::pair<uint64_t, uint32_t>> known;  // (tables named, set) of this layer's abbreviated segments
    const int64_t gx = s->tiled ? ((int64_t)size_x + s->seg_w - 1) / s->seg_w : 1;
    const int64_t gy = ((int64_t)size_y + s->seg_h - 1) / s->seg_h;
    if (sr1 < 0) sr1 = gy;
    const int64_t n = gx * (sr1 - sr0);
    const uint64_t total = s->offsets[n];
    for (int64_t i = 0; i < n; i++) {
        const uint64_t o = s->offsets[i], len = s->offsets[i + 1] - o;
        if (s->offsets[i + 1] < o || s->offsets[i + 1] > total)
            return fail(PBX_E_BADARG, "segment %lld: bad offsets", (long long)i);
        if (len == 0) return fail(PBX_E_BADARG, "segment %lld is empty", (long long)i);
        if (len > 0x7fffffffull) return fail(PBX_E_BADARG, "segment %lld too large", (long long)i);
        const int32_t x0 = (int32_t)((i % gx) * s->seg_w), y0 = (int32_t)((sr0 + i / gx) * s->seg_h);
        const int32_t rows = s->tiled ? s->seg_h : std::min(s->seg_h, size_y - y0);
        char what[48];
        snprintf(what, sizeof what, "segment %lld", (long long)i);
        // An abbreviated segment (no DQT / DHT of its own: the normal case under tag 347) that
        // names the tables an earlier one of this layer named has that one's set: nothing is
        // copied, built or compared for it.
        JpegHeader H;
        bool own = false;
        if (int rc = jpeg_parse_header(s->data + o, len, nullptr, &own, H, what)) return rc;
        JpegTables mine;
        if (own) {
            mine = base;
            H = JpegHeader();
            if (int rc = jpeg_parse_header(s->data + o, len, &mine, &own, H, what)) return rc;
        }
        const JpegTables& T = own ? mine : base;
        if ((int64_t)H.width != s->seg_w || (int64_t)H.height != rows)
            return fail(PBX_E_BADARG, "%s: SOF size %u x %u != segment size %d x %d", what, H.width, H.height, s->seg_w, rows);
        if ((int)H.ncomp != spp)
            return fail(PBX_E_BADARG, "%s: a stream of %u components in segments of %d samples per pixel", what, H.ncomp, spp);
        uint32_t mode = JM_COPY;
        if (H.ncomp == 1) {
            if (H.h[0] != 1 || H.v[0] != 1)
                return fail(PBX_E_BADARG, "%s: sampling factors %ux%u on a one-component stream (1x1)", what, H.h[0], H.v[0]);
        } else {
            const bool sub = H.h[0] != 1 || H.v[0] != 1;
            if (H.h[1] != 1 || H.v[1] != 1 || H.h[2] != 1 || H.v[2] != 1 ||
                !((H.h[0] == 1 && H.v[0] == 1) || (H.h[0] == 2 && H.v[0] == 1) || (H.h[0] == 2 && H.v[0] == 2)))
                return fail(PBX_E_BADARG, "%s: sampling factors %ux%u, %ux%u, %ux%u (luma 1x1, 2x1 or 2x2 with chroma 1x1)", what,
                            H.h[0], H.v[0], H.h[1], H.v[1], H.h[2], H.v[2]);
            if (sub && !j->ycbcr)
                return fail(PBX_E_BADARG, "%s: subsampling %ux%u without PhotometricInterpretation 6 (YCbCr)", what, H.h[0], H.v[0]);
            mode = !j->ycbcr ? JM_COPY : H.h[0] == 1 ? JM_YCC : H.v[0] == 1 ? JM_YCC_H2V1 : JM_YCC_H2V2;
        }
        uint64_t names = H.ncomp;  // which tables the frame and the scan name
        for (uint32_t c = 0; c < H.ncomp; c++) names = names << 6 | H.tq[c] << 4 | H.td[c] << 2 | H.ta[c];
        uint32_t tabset = ~0u;
        if (!own)
            for (const auto& kn : known)
                if (kn.first == names) tabset = kn.second;
        JTabSet ts;
        if (tabset == ~0u) memset(&ts, 0, sizeof ts);
        for (uint32_t c = 0; c < H.ncomp && tabset == ~0u; c++) {
            if (!T.qset[H.tq[c]]) return fail(PBX_E_BADARG, "%s: missing quantiser %u (component %u)", what, H.tq[c], c);
            if (!T.hset[0][H.td[c]]) return fail(PBX_E_BADARG, "%s: missing Huffman table DC %u (component %u)", what, H.td[c], c);
            if (!T.hset[1][H.ta[c]]) return fail(PBX_E_BADARG, "%s: missing Huffman table AC %u (component %u)", what, H.ta[c], c);
            static const uint8_t nat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
            for (int k = 0; k < 64; k++) ts.q[c][nat[k]] = T.q[H.tq[c]][k];
            jpeg_build_huff(T.bits[0][H.td[c]], T.vals[0][H.td[c]], ts.h[2 * c]);
            jpeg_build_huff(T.bits[1][H.ta[c]], T.vals[1][H.ta[c]], ts.h[2 * c + 1]);
        }
        if (tabset == ~0u) {
            tabset = 0;
            while (tabset < P.jtabs.size() && memcmp(&P.jtabs[tabset], &ts, sizeof ts)) tabset++;
            if (tabset == P.jtabs.size()) P.jtabs.push_back(ts);
            if (!own) known.emplace_back(names, tabset);
        }
        const uint32_t hs = H.ncomp == 3 ? H.h[0] : 1, vs = H.ncomp == 3 ? H.v[0] : 1;
        const uint32_t mcux = (H.width + 8 * hs - 1) / (8 * hs), mcuy = (H.height + 8 * vs - 1) / (8 * vs);
        const uint32_t pitch0 = (mcux * hs * 8 + 15) & ~15u, pitchc = (mcux * 8 + 15) & ~15u;
        const uint64_t size0 = ((uint64_t)pitch0 * mcuy * vs * 8 + 255) & ~255ull;
        const uint64_t sizec = H.ncomp == 3 ? ((uint64_t)pitchc * mcuy * 8 + 255) & ~255ull : 0;
        if (size0 + 2 * sizec > 0x7fffffffull) return fail(PBX_E_BADARG, "segment %lld too large", (long long)i);
        const uint64_t dstoff = P.scratch;
        P.scratch += size0 + 2 * sizec;
        P.jstreams.push_back(JStream{o + in_base + H.data, dstoff, (uint32_t)(len - H.data), tabset, H.ncomp, hs, vs, mcux,
                                     mcuy, H.restart, pitch0, pitchc, (uint32_t)size0, (uint32_t)(size0 + sizec)});
        P.jsegs.push_back(TJpegSeg{dstoff, (uint32_t)size0, (uint32_t)(size0 + sizec), pitch0, pitchc, H.width, H.height, x0,
                                   y0, mode, H.ncomp, dst, 0});
        P.jseg_rows = std::max(P.jseg_rows, H.height);
        if (dlen_sum) *dlen_sum += (uint64_t)H.width * H.height * H.ncomp;
    }
    return PBX_OK;
}

// ------------------------------------------------------- JPEG 2000 TIFF segments
// Compression 33003 / 33004 / 33005 / 34712: every strip or tile is one raw JPEG 2000 codestream
// (SOC SIZ COD QCD ... SOT SOD packets EOC) of one tile.  The host reads marker segments only --
// never a packet header, never a code-block byte -- and every length is checked against the bytes
// it lies in.  Accepted: the reversible path (5/3 wavelet, QCD style 0: no quantisation) and the
// irreversible one (9/7 wavelet, QCD style 1 or 2: scalar quantisation, derived or expounded), one
// layer, one precinct per resolution, code-block style 0; everything else is refused by name.
// With PBX_TIFF_F_J2K_PACKETS (`packets` below) also 1 .. 64 quality layers, any precinct sizes and
// SOP / EPH markers: tiff_j2k_plan writes the stream's packets down as a list (T.800 B.12).
// With PBX_TIFF_F_J2K_SUBSAMPLED (`subsampled` below) also three components whose second and third
// share the sampling factors 2 x 1, 1 x 2 or 2 x 2 (the first 1 x 1, no colour transform).
namespace {

struct J2kHeader {
    uint32_t w = 0, h = 0, ncomp = 0, prec = 0;
    uint32_t prog = 0, mct = 0, levels = 0, xcb = 0, ycb = 0, guard = 0;
    uint32_t layers = 1, scod = 0;
    uint32_t xr = 1, yr = 1;  // XRsiz, YRsiz of components 1 and 2 (component 0: 1 x 1)
    bool precincts = false;
    uint8_t pp[33];     // PPx | PPy << 4 per resolution
    uint8_t exps[97];   // per sub-band, QCD order
    bool irrev = false; // the 9/7 path
    float step[97];     // irrev: the sub-band's quantisation step (T.800 E.1.1)
    uint64_t data = 0, end = 0;  // the packets
};

int j2k_parse_header(const uint8_t* f, uint64_t len, J2kHeader& H, const char* what, bool packets, bool subsampled) {
    static const uint8_t jp2[12] = {0, 0, 0, 12, 'j', 'P', ' ', ' ', 13, 10, 0x87, 10};
    if (len >= 12 && !memcmp(f, jp2, 12)) return fail(PBX_E_BADARG, "%s: jp2 box, not a codestream", what);
    if (len < 2 || f[0] != 0xFF || f[1] != 0x4F) return fail(PBX_E_BADARG, "%s does not start with SOC (JPEG 2000 codestream)", what);
    uint64_t q = 2, sot = 0;
    bool siz = false, cod = false, qcd = false, tile = false;
    uint32_t nexp = 0, qstyle = 0, psot = 0, trans = 1, nq = 0;
    uint8_t qraw[2 * 97];  // the QCD's entries as they stand: what they mean waits for COD
    for (;;) {
        if (q + 2 > len) return fail(PBX_E_BADARG, "%s: truncated header", what);
        if (f[q] != 0xFF) return fail(PBX_E_BADARG, "%s: truncated header (no marker at byte %llu)", what, (unsigned long long)q);
        const uint32_t code = f[q + 1];
        if (code == 0x93) {  // SOD
            if (!tile) return fail(PBX_E_BADARG, "%s: SOD before SOT", what);
            H.data = q + 2;
            break;
        }
        if (code == 0xD9 || code == 0x4F || code == 0x91 || code == 0x92 || (code >= 0x30 && code <= 0x3F))
            return fail(PBX_E_BADARG, "%s: marker FF %02X in the header", what, code);
        if (q + 4 > len) return fail(PBX_E_BADARG, "%s: truncated header", what);
        const uint32_t L = (uint32_t)f[q + 2] << 8 | f[q + 3];
        if (L < 2 || q + 2 + L > len) return fail(PBX_E_BADARG, "%s: truncated header (marker FF %02X of %u bytes)", what, code, L);
        const uint8_t* p = f + q + 4;
        const uint32_t plen = L - 2;
        auto be32 = [&](uint32_t at) { return (uint32_t)p[at] << 24 | (uint32_t)p[at + 1] << 16 | (uint32_t)p[at + 2] << 8 | p[at + 3]; };
        if (!siz && code != 0x51) return fail(PBX_E_BADARG, "%s: marker FF %02X before SIZ", what, code);
        if (code == 0x51) {
            if (siz) return fail(PBX_E_BADARG, "%s: two SIZ markers", what);
            if (plen < 36) return fail(PBX_E_BADARG, "%s: truncated SIZ", what);
            const uint32_t xs = be32(2), ys = be32(6), xo = be32(10), yo = be32(14), xt = be32(18), yt = be32(22),
                           xto = be32(26), yto = be32(30), nc = (uint32_t)p[34] << 8 | p[35];
            if (plen != 36 + 3ull * nc) return fail(PBX_E_BADARG, "%s: truncated SIZ", what);
            if (xo || yo || xto || yto)
                return fail(PBX_E_BADARG, "%s: non-zero image or tile offsets (%u, %u; %u, %u)", what, xo, yo, xto, yto);
            if (!xs || !ys || !xt || !yt) return fail(PBX_E_BADARG, "%s: bad SIZ (%u x %u, tiles %u x %u)", what, xs, ys, xt, yt);
            if (xt < xs || yt < ys) return fail(PBX_E_BADARG, "%s: more than one tile (%u x %u in tiles of %u x %u)", what, xs, ys, xt, yt);
            if (nc != 1 && nc != 3) return fail(PBX_E_BADARG, "%s: %u components (1 or 3)", what, nc);
            for (uint32_t c = 0; c < nc; c++) {
                const uint32_t ssiz = p[36 + 3 * c], xr = p[37 + 3 * c], yr = p[38 + 3 * c];
                if ((xr != 1 || yr != 1) && !subsampled)
                    return fail(PBX_E_BADARG, "%s: subsampled components (component %u: %u x %u)", what, c, xr, yr);
                if (xr != 1 || yr != 1) {
                    if (nc == 1) return fail(PBX_E_BADARG, "%s: subsampling on a stream of one component (%u x %u)", what, xr, yr);
                    if (c == 0) return fail(PBX_E_BADARG, "%s: subsampled first component (%u x %u)", what, xr, yr);
                    if (xr > 2 || yr > 2 || !xr || !yr)
                        return fail(PBX_E_BADARG, "%s: sampling factors %u x %u on component %u (2 x 1, 1 x 2 or 2 x 2)", what, xr, yr, c);
                }
                if (c == 2 && (xr != H.xr || yr != H.yr))
                    return fail(PBX_E_BADARG, "%s: chroma components of different sampling factors (%u x %u and %u x %u)", what,
                                H.xr, H.yr, xr, yr);
                if (c == 1) { H.xr = xr; H.yr = yr; }
                if (ssiz & 0x80) return fail(PBX_E_BADARG, "%s: signed components", what);
                if (c && ssiz + 1 != H.prec) return fail(PBX_E_BADARG, "%s: components of different precisions", what);
                H.prec = ssiz + 1;
            }
            if (H.prec != 8 && H.prec != 16) return fail(PBX_E_BADARG, "%s: precision %u (8 or 16)", what, H.prec);
            if (nc == 3 && H.prec != 8) return fail(PBX_E_BADARG, "%s: three components at precision 16", what);
            H.w = xs; H.h = ys; H.ncomp = nc;
            siz = true;
        } else if (code == 0x52) {
            if (tile) return fail(PBX_E_BADARG, "%s: COD in a tile-part header", what);
            if (cod) return fail(PBX_E_BADARG, "%s: two COD markers", what);
            if (plen < 10) return fail(PBX_E_BADARG, "%s: truncated COD", what);
            const uint32_t scod = p[0], layers = (uint32_t)p[2] << 8 | p[3];
            if ((scod & 6) && !packets) return fail(PBX_E_BADARG, "%s: SOP or EPH markers (Scod 0x%02x)", what, scod);
            if (scod & ~7u) return fail(PBX_E_BADARG, "%s: bad Scod 0x%02x", what, scod);
            H.prog = p[1];
            if (H.prog > 4) return fail(PBX_E_BADARG, "%s: bad progression order %u", what, H.prog);
            if (!packets && layers != 1) return fail(PBX_E_BADARG, "%s: %u quality layers (1)", what, layers);
            if (layers < 1 || layers > 64) return fail(PBX_E_BADARG, "%s: %u quality layers (1 .. 64)", what, layers);
            H.layers = layers;
            H.scod = scod;
            H.mct = p[4];
            if (H.mct > 1) return fail(PBX_E_BADARG, "%s: bad multiple-component transform %u", what, H.mct);
            H.levels = p[5];
            if (H.levels > 32) return fail(PBX_E_BADARG, "%s: %u decomposition levels (0 .. 32)", what, H.levels);
            H.xcb = p[6] + 2u; H.ycb = p[7] + 2u;
            if (p[6] > 8 || p[7] > 8 || H.xcb + H.ycb > 12)
                return fail(PBX_E_BADARG, "%s: bad code-block size 2^%u x 2^%u", what, H.xcb, H.ycb);
            if (p[8])
                return fail(PBX_E_BADARG, "%s: code-block style 0x%02x (bypass, reset, termall, vertically causal, predictable "
                            "termination and segmentation symbols are not supported)", what, p[8]);
            if (p[9] > 1) return fail(PBX_E_BADARG, "%s: bad wavelet transformation %u", what, p[9]);
            trans = p[9];
            H.precincts = scod & 1;
            if (plen != 10 + (H.precincts ? H.levels + 1 : 0)) return fail(PBX_E_BADARG, "%s: truncated COD", what);
            for (uint32_t r = 0; r <= H.levels; r++) H.pp[r] = H.precincts ? p[10 + r] : 0xFF;
            cod = true;
        } else if (code == 0x5C) {
            if (tile) return fail(PBX_E_BADARG, "%s: QCD in a tile-part header", what);
            if (qcd) return fail(PBX_E_BADARG, "%s: two QCD markers", what);
            if (plen < 1) return fail(PBX_E_BADARG, "%s: truncated QCD", what);
            qstyle = p[0] & 31;
            H.guard = p[0] >> 5;
            if (qstyle > 2) return fail(PBX_E_BADARG, "%s: bad quantisation style %u", what, qstyle);
            nq = plen - 1;
            if (nq > (qstyle ? 2u * 97u : 97u)) return fail(PBX_E_BADARG, "%s: QCD of %u sub-bands", what, qstyle ? nq / 2 : nq);
            memcpy(qraw, p + 1, nq);
            qcd = true;
        } else if (code == 0x90) {
            if (tile) return fail(PBX_E_BADARG, "%s: more than one tile-part", what);
            if (plen != 8) return fail(PBX_E_BADARG, "%s: truncated SOT", what);
            if (p[0] || p[1]) return fail(PBX_E_BADARG, "%s: more than one tile (tile index %u)", what, (uint32_t)p[0] << 8 | p[1]);
            psot = be32(2);
            if (p[6] != 0 || p[7] > 1) return fail(PBX_E_BADARG, "%s: more than one tile-part (%u of %u)", what, p[6], p[7]);
            sot = q;
            tile = true;
        } else if (code == 0x53 || code == 0x5D || code == 0x5E || code == 0x5F || code == 0x60 || code == 0x61 || code == 0x63) {
            static const char* nm[17] = {"", "", "", "COC", "", "", "", "", "", "", "", "", "", "QCC", "RGN", "POC", ""};
            const char* name = code == 0x60 ? "PPM" : code == 0x61 ? "PPT" : code == 0x63 ? "CRG" : nm[code & 15];
            return fail(PBX_E_BADARG, "%s: %s markers are not supported", what, name);
        } else if (code == 0x64 || code == 0x55 || code == 0x57 || code == 0x58) {
            // COM, TLM, PLM, PLT: skipped
        } else {
            return fail(PBX_E_BADARG, "%s: marker FF %02X in the header", what, code);
        }
        q += 2 + L;
    }
    if (!cod) return fail(PBX_E_BADARG, "%s: no COD marker", what);
    if (!qcd) return fail(PBX_E_BADARG, "%s: no QCD marker", what);
    H.irrev = trans == 0;
    if (H.irrev && qstyle == 0)
        return fail(PBX_E_BADARG, "%s: irreversible wavelet (9/7) with quantisation style 0 (no quantisation)", what);
    if (!H.irrev && qstyle)
        return fail(PBX_E_BADARG, "%s: quantisation style %u (scalar quantisation) with the reversible wavelet (5/3)", what, qstyle);
    const uint32_t nb = 3 * H.levels + 1;
    if (qstyle == 0) {
        nexp = nq;
        for (uint32_t k = 0; k < nexp && k < nb; k++) H.exps[k] = qraw[k] >> 3;
    } else if (qstyle == 2) {
        if (nq & 1) return fail(PBX_E_BADARG, "%s: QCD of %u bytes in 16-bit entries (style 2)", what, nq);
        nexp = nq / 2;
    } else {
        if (nq != 2) return fail(PBX_E_BADARG, "%s: QCD of %u bytes for the one entry of style 1", what, nq);
        nexp = nb;
    }
    if (nexp != nb)
        return fail(PBX_E_BADARG, "%s: QCD of %u sub-bands for %u decomposition levels", what, nexp, H.levels);
    if (H.mct && H.ncomp != 3) return fail(PBX_E_BADARG, "%s: multiple-component transform on %u component(s)", what, H.ncomp);
    if (H.mct && (H.xr != 1 || H.yr != 1))
        return fail(PBX_E_BADARG, "%s: subsampled components (%u x %u) with the multiple-component transform", what, H.xr, H.yr);
    if (H.irrev) {
        // T.800 E.1.1: step = 2^(R_b - eps_b) (1 + mu_b / 2^11), R_b the precision plus the band's
        // gain (0 LL, 1 HL and LH, 2 HH); style 1 derives every band from the LL entry (E-5):
        // eps_b = eps_0 - (levels - n_b), mu_b = mu_0, n_b the decompositions at band b
        for (uint32_t b = 0; b < nb; b++) {
            const uint32_t e = qstyle == 2 ? (uint32_t)qraw[2 * b] << 8 | qraw[2 * b + 1] : (uint32_t)qraw[0] << 8 | qraw[1];
            int32_t eps = (int32_t)(e >> 11);
            const uint32_t mu = e & 2047u;
            if (qstyle == 1) {
                const uint32_t nbd = b ? H.levels - ((b + 2) / 3 - 1) : H.levels;
                eps -= (int32_t)(H.levels - nbd);
                if (eps < 0) return fail(PBX_E_BADARG, "%s: quantisation style 1 derives exponent %d for sub-band %u", what, eps, b);
            }
            const uint32_t gain = b ? ((b - 1) % 3 == 2 ? 2u : 1u) : 0u;
            H.exps[b] = (uint8_t)eps;
            H.step[b] = ldexpf(1.0f + (float)mu / 2048.0f, (int)(H.prec + gain) - eps);
            if (H.guard + H.exps[b] > 31)  // (the half bit below bit-plane 0 takes one of the 31)
                return fail(PBX_E_BADARG, "%s: %u magnitude bit-planes on a 9/7 sub-band (at most 30)", what, H.guard + H.exps[b] - 1);
        }
    }
    for (uint32_t k = 0; k < nexp; k++)
        if (H.guard + H.exps[k] > 32)
            return fail(PBX_E_BADARG, "%s: %u magnitude bit-planes (at most 31)", what, H.guard + H.exps[k] - 1);
    for (uint32_t r = 0; r <= H.levels; r++) {
        const uint32_t ppx = H.pp[r] & 15, ppy = H.pp[r] >> 4, sh = H.levels - r;
        if (r && (!ppx || !ppy)) return fail(PBX_E_BADARG, "%s: precinct exponent 0 at resolution %u", what, r);
        const uint64_t rw = ((uint64_t)H.w + (1ull << sh) - 1) >> sh, rh = ((uint64_t)H.h + (1ull << sh) - 1) >> sh;
        if (!packets && (rw > (1ull << ppx) || rh > (1ull << ppy)))
            return fail(PBX_E_BADARG, "%s: more than one precinct in resolution %u", what, r);
    }
    H.end = len;
    if (psot) {
        // (a tile-part that says it is longer than its segment ends with the segment: what the
        // packets then miss is the device's to find)
        if (sot + psot < H.data) return fail(PBX_E_BADARG, "%s: tile-part length %u ends inside its header", what, psot);
        H.end = std::min<uint64_t>(sot + psot, len);
        if (H.end + 2 <= len && f[H.end] == 0xFF && f[H.end + 1] == 0x90)
            return fail(PBX_E_BADARG, "%s: more than one tile-part", what);
    } else if (len >= H.data + 2 && f[len - 2] == 0xFF && f[len - 1] == 0xD9) {
        H.end = len - 2;
    }
    return PBX_OK;
}

}  // namespace

// pbx_tiff_segments fields of a JPEG 2000 layer that can be checked without the plane.
int tiff_j2k_check(const pbx_tiff_segments* s, int32_t pixel_type, int32_t spp) {
    if (!s->data || !s->offsets) return fail(PBX_E_BADARG, "null argument");
    if (s->seg_w < 1 || s->seg_h < 1) return fail(PBX_E_BADARG, "bad segment shape %d x %d", s->seg_w, s->seg_h);
    if (s->tiled && ((s->seg_w | s->seg_h) & 15))
        return fail(PBX_E_BADARG, "tile %d x %d: TileWidth and TileLength must be multiples of 16 (TIFF 6.0 section 15)",
                    s->seg_w, s->seg_h);
    if (s->compression != PBX_TIFF_J2K) return fail(PBX_E_BADARG, "bad compression %d (the JPEG 2000 calls take 34712)", s->compression);
    if (s->predictor != 1) return fail(PBX_E_BADARG, "bad predictor %d on JPEG 2000 segments (1 only)", s->predictor);
    if (s->flags & ~(PBX_TIFF_F_J2K_PACKETS | PBX_TIFF_F_J2K_SUBSAMPLED | PBX_TIFF_F_J2K_YCBCR))
        return fail(PBX_E_BADARG, "bad flags 0x%x", (unsigned)s->flags);
    if (pixel_type != PBX_UINT8 && pixel_type != PBX_UINT16)
        return fail(PBX_E_BADARG, "JPEG 2000 segments on a plane that is neither uint8 nor uint16");
    if (spp != 1 && spp != 3) return fail(PBX_E_BADARG, "JPEG 2000 segments of %d samples per pixel (1 or 3)", spp);
    if ((s->flags & PBX_TIFF_F_J2K_YCBCR) && (spp != 3 || pixel_type != PBX_UINT8))
        return fail(PBX_E_BADARG, "YCbCr conversion (PBX_TIFF_F_J2K_YCBCR) on JPEG 2000 segments of %d sample(s) per pixel of %d bits "
                    "(3 of 8)", spp, 8 * bpp_of(pixel_type));
    return PBX_OK;
}

// Host plan of the JPEG 2000 segment rows [sr0, sr1) (sr1 < 0: all) of a uint8 / uint16 plane:
// tiff_plan's geometry; per segment a J2Stream and a TJ2Seg, per component two int32 planes in
// scratch (8 bytes a sample, each plane rounded up to 256 bytes) and a J2Comp, per sub-band
// (T.800 B.5) a J2Band, per code block (the band's grid anchored at 0, the last column and row
// clipped) a J2Block that says where its coefficients go, and per layer and precinct a J2Packet,
// in the order the stream's progression puts them, with the precinct's window into each band's
// grid and the window's two tag trees.  Everything follows from SIZ, COD and QCD.
int tiff_j2k_plan(int32_t size_x, int32_t size_y, int bpp, const pbx_tiff_segments* s, uint64_t in_base, ZarrPlan& P,
                  int64_t sr0, int64_t sr1, int spp, uint32_t dst, uint64_t* packets) {
    if (!s->tiled && s->seg_w != size_x)
        return fail(PBX_E_BADARG, "strip width %d != plane width %d", s->seg_w, size_x);
    const int64_t gx = s->tiled ? ((int64_t)size_x + s->seg_w - 1) / s->seg_w : 1;
    const int64_t gy = ((int64_t)size_y + s->seg_h - 1) / s->seg_h;
    if (sr1 < 0) sr1 = gy;
    const int64_t n = gx * (sr1 - sr0);
    const uint64_t total = s->offsets[n];
    for (int64_t i = 0; i < n; i++) {
        const uint64_t o = s->offsets[i], len = s->offsets[i + 1] - o;
        if (s->offsets[i + 1] < o || s->offsets[i + 1] > total)
            return fail(PBX_E_BADARG, "segment %lld: bad offsets", (long long)i);
        if (len == 0) return fail(PBX_E_BADARG, "segment %lld is empty", (long long)i);
        if (len > 0x7fffffffull) return fail(PBX_E_BADARG, "segment %lld too large", (long long)i);
        const int32_t x0 = (int32_t)((i % gx) * s->seg_w), y0 = (int32_t)((sr0 + i / gx) * s->seg_h);
        const int32_t rows = s->tiled ? s->seg_h : std::min(s->seg_h, size_y - y0);
        char what[48];
        snprintf(what, sizeof what, "segment %lld", (long long)i);
        J2kHeader H;
        if (int rc = j2k_parse_header(s->data + o, len, H, what, s->flags & PBX_TIFF_F_J2K_PACKETS,
                                      s->flags & PBX_TIFF_F_J2K_SUBSAMPLED))
            return rc;
        if ((int64_t)H.w != s->seg_w || (int64_t)H.h != rows)
            return fail(PBX_E_BADARG, "%s: SIZ size %u x %u != segment size %d x %d", what, H.w, H.h, s->seg_w, rows);
        if ((int)H.ncomp != spp)
            return fail(PBX_E_BADARG, "%s: a stream of %u components in segments of %d samples per pixel", what, H.ncomp, spp);
        if ((int)H.prec != 8 * bpp)
            return fail(PBX_E_BADARG, "%s: precision %u on a plane of %d-bit samples", what, H.prec, 8 * bpp);
        const bool ycc = s->flags & PBX_TIFF_F_J2K_YCBCR;
        if (ycc && H.mct)
            return fail(PBX_E_BADARG, "%s: YCbCr conversion (PBX_TIFF_F_J2K_YCBCR) on a stream with the multiple-component transform", what);
        if ((uint64_t)H.w * H.h * 4 + 255 > 0x7fffffffull) return fail(PBX_E_BADARG, "segment %lld too large", (long long)i);
        const uint32_t NL = H.levels, stream = (uint32_t)P.j2streams.size();
        auto res = [&](uint32_t v, uint32_t r) { return (uint32_t)(((uint64_t)v + (1ull << (NL - r)) - 1) >> (NL - r)); };
        // component c's own size: ceil(W / XRsiz) x ceil(H / YRsiz) (no offsets), 1 x 1 for component 0
        auto cwid = [&](uint32_t c) { return c ? (H.w + H.xr - 1) / H.xr : H.w; };
        auto chei = [&](uint32_t c) { return c ? (H.h + H.yr - 1) / H.yr : H.h; };
        TJ2Seg seg{{0, 0, 0}, H.w, H.h, x0, y0, H.ncomp,
                   H.mct | (H.irrev ? J2_SEG_IRREV : 0u) | (ycc ? J2_SEG_YCC : 0u) | (H.xr == 2 ? J2_SEG_XS2 : 0u) |
                       (H.yr == 2 ? J2_SEG_YS2 : 0u),
                   H.prec, dst};
        const uint32_t band0 = (uint32_t)P.j2bands.size(), blk0 = (uint32_t)P.j2blocks.size();
        struct Cell {  // a sub-band's code-block size and grid
            uint32_t xcb, ycb, nbx, nby;
        };
        std::vector<Cell> cells;
        for (uint32_t c = 0; c < H.ncomp; c++) {
            const uint32_t W = cwid(c), Hc = chei(c);
            const uint64_t plane = ((uint64_t)W * Hc * 4 + 255) & ~255ull;
            const uint64_t a = P.scratch;
            P.scratch += 2 * plane;
            seg.src[c] = a;
            P.j2comps.push_back(J2Comp{a, a + plane, W, Hc, NL, H.irrev ? 1u : 0u});
            P.j2irrev += H.irrev ? 1 : 0;
            for (uint32_t b = 0; b < 3 * NL + 1; b++) {
                const uint32_t r = b ? (b + 2) / 3 : 0, orient = b ? (b - 1) % 3 + 1 : 0;
                const uint32_t cw = res(W, r), ch = res(Hc, r);
                const uint32_t lw = r ? res(W, r - 1) : 0, lh = r ? res(Hc, r - 1) : 0;
                const uint32_t bx0 = orient & 1 ? lw : 0, by0 = orient & 2 ? lh : 0;
                const uint32_t bw = !r ? cw : orient & 1 ? cw - lw : lw, bh = !r ? ch : orient & 2 ? ch - lh : lh;
                const uint32_t ppx = H.pp[r] & 15, ppy = H.pp[r] >> 4;
                // (B.7: a code block is clipped to the precinct's part of the band)
                const uint32_t xcb = std::min(H.xcb, ppx - (r ? 1 : 0)), ycb = std::min(H.ycb, ppy - (r ? 1 : 0));
                const uint32_t nbx = bw && bh ? (bw + (1u << xcb) - 1) >> xcb : 0, nby = bw && bh ? (bh + (1u << ycb) - 1) >> ycb : 0;
                const uint32_t gexp = H.guard + H.exps[b];
                const float hstep = H.irrev ? 0.5f * H.step[b] : 0.0f;
                if (P.j2blocks.size() + (uint64_t)nbx * nby > 0x3ffffffull)
                    return fail(PBX_E_BADARG, "segment %lld: too many code blocks", (long long)i);
                P.j2bands.push_back(J2Band{(uint32_t)P.j2blocks.size(), nbx, nby, gexp ? gexp - 1 : 0, hstep});
                cells.push_back(Cell{xcb, ycb, nbx, nby});
                for (uint32_t by = 0; by < nby; by++)
                    for (uint32_t bx = 0; bx < nbx; bx++) {
                        const uint32_t ox = bx << xcb, oy = by << ycb;
                        const uint32_t w = std::min(1u << xcb, bw - ox), h = std::min(1u << ycb, bh - oy);
                        P.j2blocks.push_back(J2Block{a + 4 * ((uint64_t)(by0 + oy) * W + bx0 + ox), W, (uint16_t)w, (uint16_t)h,
                                                     stream, (uint8_t)orient, (uint8_t)(gexp ? gexp - 1 : 0), (uint16_t)(H.irrev ? 1 : 0), hstep, 0});
                        P.j2coef = std::max(P.j2coef, w * h);
                        P.j2flag = std::max(P.j2flag, (w + 2) * (h + 2));
                    }
            }
        }
        // The precincts (B.6) of every component and resolution, each with its windows into the
        // resolution's bands and their tag trees, and the key the progression order sorts it by.
        // With no offsets the position loops of B.12.1.3 - 5, which step and test with
        // XRsiz 2^(PPx + NL - r) and YRsiz 2^(PPy + NL - r), visit a precinct when they reach its
        // origin on the reference grid: precinct (px, py) of a component subsampled XRsiz x YRsiz
        // lies at (px XRsiz 2^(PPx + NL - r), py YRsiz 2^(PPy + NL - r)), inside the tile because
        // px 2^PPx < ceil(W / (XRsiz 2^(NL - r))) means px 2^PPx XRsiz 2^(NL - r) < W.
        struct Prec {
            uint64_t yo, xo;  // its origin on the reference grid
            uint32_t c, r;
            J2Packet pk;
        };
        std::vector<Prec> precs;
        const uint32_t nbands = 3 * NL + 1;
        for (uint32_t c = 0; c < H.ncomp; c++)
            for (uint32_t r = 0; r <= NL; r++) {
                const uint32_t ppx = H.pp[r] & 15, ppy = H.pp[r] >> 4;
                const uint64_t npx = ((uint64_t)res(cwid(c), r) + (1ull << ppx) - 1) >> ppx;
                const uint64_t npy = ((uint64_t)res(chei(c), r) + (1ull << ppy) - 1) >> ppy;
                const uint64_t xr = c ? H.xr : 1, yr = c ? H.yr : 1;
                if (precs.size() + npx * npy > 0xfffffull)
                    return fail(PBX_E_BADARG, "segment %lld: too many packets", (long long)i);
                const uint32_t fb = r ? 3 * r - 2 : 0, nb = r ? 3 : 1;
                for (uint64_t py = 0; py < npy; py++)
                    for (uint64_t px = 0; px < npx; px++) {
                        Prec q{(py << (ppy + NL - r)) * yr, (px << (ppx + NL - r)) * xr, c, r, J2Packet{band0 + c * nbands + fb, 0, (uint16_t)nb, {}}};
                        for (uint32_t k = 0; k < nb; k++) {
                            const Cell& g = cells[c * nbands + fb + k];
                            // the precinct's part of the band holds 2^(pb - cb) cells a side
                            const uint32_t sx = ppx - (r ? 1 : 0) - g.xcb, sy = ppy - (r ? 1 : 0) - g.ycb;
                            const uint64_t x0 = px << sx, y0 = py << sy;
                            J2Window W{(uint32_t)P.j2nodes, 0, 0, 0, 0, 0, 0};
                            if (x0 < g.nbx && y0 < g.nby) {
                                W.x0 = (uint32_t)x0;
                                W.y0 = (uint32_t)y0;
                                W.nx = (uint16_t)std::min<uint64_t>(1ull << sx, g.nbx - x0);
                                W.ny = (uint16_t)std::min<uint64_t>(1ull << sy, g.nby - y0);
                                uint32_t wl = W.nx, hl = W.ny;
                                for (;;) {
                                    W.nodes += wl * hl;
                                    W.tlevels++;
                                    if (wl == 1 && hl == 1) break;
                                    wl = (wl + 1) / 2;
                                    hl = (hl + 1) / 2;
                                }
                            }
                            P.j2nodes += 2ull * W.nodes;
                            if (P.j2nodes > 0x3fffffffull)
                                return fail(PBX_E_BADARG, "segment %lld: too many code blocks", (long long)i);
                            q.pk.win[k] = W;
                        }
                        precs.push_back(q);
                    }
            }
        // (a stable sort from component, resolution, raster order: what the keys leave open)
        auto order = [&](auto key) {
            std::stable_sort(precs.begin(), precs.end(), [&](const Prec& a, const Prec& b) { return key(a) < key(b); });
        };
        if (H.prog <= 1) order([](const Prec& q) { return std::make_tuple(q.r, q.c); });                // LRCP, RLCP
        else if (H.prog == 2) order([](const Prec& q) { return std::make_tuple(q.r, q.yo, q.xo, q.c); });  // RPCL
        else if (H.prog == 3) order([](const Prec& q) { return std::make_tuple(q.yo, q.xo, q.c, q.r); });  // PCRL
        else order([](const Prec& q) { return std::make_tuple(q.c, q.yo, q.xo, q.r); });                // CPRL
        const uint64_t npk = (uint64_t)precs.size() * H.layers;
        if (P.j2packets.size() + npk > 0xfffffull) return fail(PBX_E_BADARG, "segment %lld: too many packets", (long long)i);
        const uint32_t pk0 = (uint32_t)P.j2packets.size();
        auto emit = [&](size_t k0, size_t k1, uint32_t l) {
            for (size_t k = k0; k < k1; k++) {
                P.j2packets.push_back(precs[k].pk);
                P.j2packets.back().layer = (uint16_t)l;
            }
        };
        if (H.prog == 0) {  // the layers outermost
            for (uint32_t l = 0; l < H.layers; l++) emit(0, precs.size(), l);
        } else if (H.prog == 1) {  // inside the resolution
            for (size_t k0 = 0, k1; k0 < precs.size(); k0 = k1) {
                for (k1 = k0; k1 < precs.size() && precs[k1].r == precs[k0].r;) k1++;
                for (uint32_t l = 0; l < H.layers; l++) emit(k0, k1, l);
            }
        } else {  // innermost
            for (size_t k = 0; k < precs.size(); k++)
                for (uint32_t l = 0; l < H.layers; l++) emit(k, k + 1, l);
        }
        // a stream of several layers: a contribution a block and layer at most, and a gather area
        // of the stream's length for the blocks whose bytes lie in more than one packet
        const uint32_t nblk = (uint32_t)P.j2blocks.size() - blk0, slen = (uint32_t)(H.end - H.data);
        const uint64_t ncon = H.layers > 1 ? (uint64_t)nblk * H.layers : 0;
        if (P.j2cons + ncon > 0x3ffffffull) return fail(PBX_E_BADARG, "segment %lld: too many block contributions", (long long)i);
        uint64_t gather = 0;
        if (ncon) {
            gather = P.scratch;
            P.scratch += ((uint64_t)slen + 255) & ~255ull;
        }
        P.j2streams.push_back(J2Stream{o + in_base + H.data, gather, slen, band0, H.ncomp, NL, pk0, (uint32_t)npk, blk0, nblk,
                                       (uint32_t)P.j2cons, (uint32_t)ncon, H.layers,
                                       (H.irrev ? J2S_IRREV : 0u) | (H.scod & 2 ? J2S_SOP : 0u) | (H.scod & 4 ? J2S_EPH : 0u)});
        P.j2cons += ncon;
        P.j2segs.push_back(seg);
        P.j2seg_rows = std::max(P.j2seg_rows, H.h);
        if (packets) *packets += npk;
    }
    return PBX_OK;
}

// ------------------------------------------------------------------ one codec, one launch
int tiff_codec_check(const TiffCodec& c, int32_t pixel_type, int32_t spp, int64_t sample, uint64_t plane_label) {
    if (c.packed) {
        if (int rc = tiff_packed_check(c.s, c.packed, pixel_type)) return rc;
        return tiff_samples_check(spp, sample, bpp_of(pixel_type));
    }
    if (int rc = c.j2k    ? tiff_j2k_check(c.s, pixel_type, spp)
                 : c.jpeg ? tiff_jpeg_check(c.s, c.jpeg, pixel_type, spp)
                          : tiff_segments_check(c.s))
        return rc;
    if (c.s->predictor == 2 && (pixel_type == PBX_FLOAT || pixel_type == PBX_DOUBLE))
        return fail(PBX_E_BADARG, "plane %llu: predictor 2 on floating-point samples", (unsigned long long)plane_label);
    if (int rc = tiff_fp_predictor_check(c.s, pixel_type)) return rc;
    return tiff_samples_check(spp, sample, bpp_of(pixel_type));
}

int tiff_codec_plan(const TiffCodec& c, int32_t size_x, int32_t size_y, int bpp, bool big_endian, uint64_t in_base,
                    uint32_t plane, ZarrPlan& P, bool band, int64_t sr0, int64_t sr1, int spp, uint32_t dst) {
    if (c.packed) return tiff_packed_plan(size_x, size_y, c.s, c.packed, in_base, P, sr0, sr1, spp, dst);
    if (c.j2k) return tiff_j2k_plan(size_x, size_y, bpp, c.s, in_base, P, sr0, sr1, spp, dst);
    if (c.jpeg) return tiff_jpeg_plan(size_x, size_y, c.s, c.jpeg, in_base, P, sr0, sr1, spp, dst);
    return tiff_plan(size_x, size_y, bpp, big_endian, c.s, in_base, plane, P, nullptr, band, sr0, sr1, spp, dst);
}

SourceGrid source_grid(const pbx_tiff_segments* s, int32_t size_x, int32_t size_y, int32_t y0, int32_t rows) {
    const int64_t gx = s->tiled ? ((int64_t)size_x + s->seg_w - 1) / s->seg_w : 1;
    const int64_t r0 = y0 / s->seg_h, r1 = ((int64_t)y0 + (rows < 0 ? size_y : rows) + s->seg_h - 1) / s->seg_h;
    return SourceGrid{gx, r0, r1, s->offsets[gx * (r1 - r0)]};
}

SourceGrid source_grid(const pbx_zarr_chunks* z, int32_t size_x, int32_t size_y, int32_t y0, int32_t rows) {
    const int64_t gx = ((int64_t)size_x + z->chunk_x - 1) / z->chunk_x;
    const int64_t r0 = y0 / z->chunk_y, r1 = ((int64_t)y0 + (rows < 0 ? size_y : rows) + z->chunk_y - 1) / z->chunk_y;
    return SourceGrid{gx, r0, r1, z->offsets[gx * (r1 - r0)]};
}

LaunchLayout::LaunchLayout(const ZarrPlan& P, uint32_t crc_split) : j2segs(P.j2segs) {
    for (uint32_t k = 0; k < ZS_NKINDS; k++) {
        counts[k] = (uint32_t)P.kind[k].size();
        streams.insert(streams.end(), P.kind[k].begin(), P.kind[k].end());
    }
    for (uint32_t k = 0; k < ZK_NPOLY; k++) {
        ck_first[k] = (uint32_t)checks.size();
        for (const ZCheck& c : P.checks[k]) if (c.len < crc_split) checks.push_back(c);
        ck_wave[k] = (uint32_t)checks.size() - ck_first[k];
        for (const ZCheck& c : P.checks[k]) if (c.len >= crc_split) checks.push_back(c);
        ck_n[k] = (uint32_t)checks.size() - ck_first[k];
    }
    j2chroma = (uint32_t)(j2segs.end() - std::stable_partition(j2segs.begin(), j2segs.end(), [](const TJ2Seg& u) {
                              return !(u.rct & J2_SEG_CHROMA);
                          }));
    j2meta = (sizeof(J2Code) + sizeof(J2Walk)) * P.j2blocks.size() + sizeof(J2Contrib) * P.j2cons + 4 * P.j2nodes;
    nstreams = (uint32_t)streams.size();
    nchecks = (uint32_t)checks.size();
    njpeg = (uint32_t)P.jstreams.size();
    nj2 = (uint32_t)P.j2streams.size();
    err_streams = 0;
    err_checks = err_streams + nstreams;
    err_jpeg = err_checks + nchecks;
    err_j2k = err_jpeg + njpeg;
    nerr = err_j2k + nj2;
}

int launch_errors(const LaunchLayout& L, const uint32_t* err) {
    for (uint32_t s = 0; s < L.nstreams; s++)
        if (const uint32_t code = err[L.err_streams + s]) {
            static const char* names[ZS_NKINDS] = {"lz4", "zlib", "stored", "blosclz", "zstd", "gzip", "lzw", "packbits"};
            uint32_t k = 0, first = 0;
            while (s >= first + L.counts[k]) first += L.counts[k++];
            return fail(PBX_E_BADARG, "corrupt chunk stream %u (%s, decoder code %u)", s, names[k], code);
        }
    for (uint32_t s = 0; s < L.nchecks; s++)
        if (err[L.err_checks + s]) {
            const ZCheck& c = L.checks[s];
            return fail(PBX_E_BADARG, "chunk checksum mismatch: the %s of %u bytes is not 0x%08x",
                        c.poly == ZK_CRC32C ? "crc32c" : "gzip CRC-32", c.len, c.expect);
        }
    for (uint32_t s = 0; s < L.njpeg; s++)
        if (const uint32_t code = err[L.err_jpeg + s]) {
            static const char* why[6] = {"", "entropy data ends before the last MCU", "a code that is in no table",
                                         "a run that passes coefficient 63", "a DC size > 11 or an AC size > 10",
                                         "a restart marker missing, out of sequence or misplaced"};
            return fail(PBX_E_BADARG, "corrupt segment stream %u (jpeg, decoder code %u: %s)", s, code,
                        code < 6 ? why[code] : "?");
        }
    for (uint32_t s = 0; s < L.nj2; s++)
        if (const uint32_t code = err[L.err_j2k + s])
            return fail(PBX_E_BADARG, "corrupt segment stream %u (j2k, decoder code %u)", s, code);
    return PBX_OK;
}

}  // namespace pbx

// ------------------------------------------------------------------ test hooks (include/pbx.h)
using namespace pbx;

// pbx_test_tiff_j2k_decode's inverse wavelet of one component, in place in its plane A (pitch c.w):
// level by level every row and then every column of the resolution is de-interleaved into a line
// of Line samples (the low-pass half to the even places), lifted by lift(line) and written back.
template <class Line, class Sample, class Lift>
static void j2k_host_idwt(Sample* A, const J2Comp& c, Lift lift) {
    std::vector<Line> line;
    for (uint32_t r = 1; r <= c.levels; r++) {
        const uint32_t sh = c.levels - r;
        const uint32_t cw = (uint32_t)((c.w + (1ull << sh) - 1) >> sh), ch = (uint32_t)((c.h + (1ull << sh) - 1) >> sh);
        const uint32_t lw = (cw + 1) / 2, lh = (ch + 1) / 2;
        for (uint32_t y = 0; y < ch; y++) {
            line.assign(cw, 0);
            for (uint32_t x = 0; x < cw; x++) line[x < lw ? 2 * x : 2 * (x - lw) + 1] = A[(uint64_t)y * c.w + x];
            lift(line);
            for (uint32_t x = 0; x < cw; x++) A[(uint64_t)y * c.w + x] = (Sample)line[x];
        }
        for (uint32_t x = 0; x < cw; x++) {
            line.assign(ch, 0);
            for (uint32_t y = 0; y < ch; y++) line[y < lh ? 2 * y : 2 * (y - lh) + 1] = A[(uint64_t)y * c.w + x];
            lift(line);
            for (uint32_t y = 0; y < ch; y++) A[(uint64_t)y * c.w + x] = (Sample)line[y];
        }
    }
}

extern "C" {

const char* pbx_last_error(void) { return last_error().c_str(); }

int pbx_test_zarr_plan(const pbx_zarr_chunks* z, int32_t size_x, int32_t size_y, int32_t bpp, int32_t depth,
                       const int32_t* slices, int32_t nslices, int32_t y0, int32_t rows, uint64_t out[4]) {
    if (!z || !slices || !out || nslices < 1) return fail(PBX_E_BADARG, "null argument");
    if (int rc = zarr_chunks_check(z)) return rc;
    if (size_x <= 0 || size_y <= 0) return fail(PBX_E_BADARG, "bad plane size");
    if (bpp != 1 && bpp != 2 && bpp != 4 && bpp != 8) return fail(PBX_E_BADARG, "bad sample size %d", bpp);
    if (rows < 0 || y0 < 0 || (int64_t)y0 + rows > size_y) return fail(PBX_E_BADARG, "rows outside the plane");
    std::vector<ZarrWant> want;
    for (int32_t k = 0; k < nslices; k++) {
        if (int rc = zarr_slice_check(depth, slices[k])) return rc;
        want.push_back(ZarrWant{(uint32_t)slices[k], (uint32_t)k});
    }
    const int64_t gy = ((int64_t)size_y + z->chunk_y - 1) / z->chunk_y;
    const int64_t cy0 = rows ? y0 / z->chunk_y : 0, cy1 = rows ? ((int64_t)y0 + rows + z->chunk_y - 1) / z->chunk_y : gy;
    ZarrPlan P;
    if (int rc = zarr_plan(size_x, z, bpp, 0, cy0, cy1, depth, want, rows ? y0 : 0,
                           rows ? (int64_t)y0 + rows : gy * z->chunk_y, P))
        return rc;
    out[0] = out[1] = 0;
    for (const auto& v : P.kind) {
        out[0] += v.size();
        for (const ZStream& t : v) out[1] += t.dlen;
    }
    out[2] = P.skipped;
    out[3] = P.scratch;
    return PBX_OK;
}

int pbx_test_tiff_j2k_plan(const pbx_tiff_segments* s, int32_t size_x, int32_t size_y, int32_t pixel_type,
                           int32_t samples_per_pixel, int32_t y0, int32_t rows, uint64_t out[4]) {
    if (!s || !out) return fail(PBX_E_BADARG, "null argument");
    if (int rc = tiff_j2k_check(s, pixel_type, samples_per_pixel)) return rc;
    if (size_x <= 0 || size_y <= 0) return fail(PBX_E_BADARG, "bad plane size");
    if (rows < 0 || y0 < 0 || (int64_t)y0 + rows > size_y)
        return fail(PBX_E_BADARG, "rows %d+%d outside the plane (%d rows)", y0, rows, size_y);
    ZarrPlan P;
    uint64_t packets = 0;
    const bool band = rows > 0;
    if (int rc = tiff_j2k_plan(size_x, size_y, bpp_of(pixel_type), s, 0, P, band ? y0 / s->seg_h : 0,
                               band ? ((int64_t)y0 + rows + s->seg_h - 1) / s->seg_h : -1, samples_per_pixel, 0, &packets))
        return rc;
    out[0] = P.j2streams.size();
    out[1] = P.j2blocks.size();
    out[2] = packets;
    out[3] = P.scratch;
    return PBX_OK;
}

// Test hook: the whole decode on the CPU, no context and no device call: the planner's tables,
// then the device's own serial code (tiff_j2k_dev.h: j2k_packets per stream, j2k_block per code
// block, each block's state in heap blocks of exactly the sizes k_tiff_j2k_blocks has in LDS),
// the inverse 5/3 lifting, the inverse RCT, level shift and clamp; for an irreversible stream the
// same float32 functions the kernels call (tiff_j2k_dev.h: dequantisation, the 9/7 lifting, the
// ICT and the rounding), in the kernels' order, so that the two agree bit for bit.  Subsampled
// components are replicated and YCbCr ones converted by tiff_j2k_dev.h's j2k_chroma_at and
// j2k_ycc_rgb, k_tiff_j2k_place_chroma's too.  out: samples_per_pixel planes
// of size_x * size_y samples, uint8 or host-order uint16, no pitch.
int pbx_test_tiff_j2k_decode(const pbx_tiff_segments* s, int32_t size_x, int32_t size_y, int32_t pixel_type,
                             int32_t samples_per_pixel, void* out, uint64_t out_bytes) {
    if (!s || !out) return fail(PBX_E_BADARG, "null argument");
    if (int rc = tiff_j2k_check(s, pixel_type, samples_per_pixel)) return rc;
    if (size_x <= 0 || size_y <= 0) return fail(PBX_E_BADARG, "bad plane size");
    const int bpp = bpp_of(pixel_type);
    if (out_bytes != (uint64_t)size_x * size_y * bpp * samples_per_pixel) return fail(PBX_E_BADARG, "bad output size");
    ZarrPlan P;
    if (int rc = tiff_j2k_plan(size_x, size_y, bpp, s, 0, P, 0, -1, samples_per_pixel, 0)) return rc;
    static const uint32_t mq[J2_MQ_STATES] = {PBX_MQ_TABLE};
    std::vector<J2Code> code(P.j2blocks.size(), J2Code{0, 0, 0, 0});
    std::vector<J2Walk> walk(P.j2blocks.size(), J2Walk{0, 0});
    std::vector<J2Contrib> con(P.j2cons, J2Contrib{0, 0, 0, 0});
    std::vector<uint32_t> tt(P.j2nodes, 0);
    for (size_t i = 0; i < P.j2streams.size(); i++)
        if (const uint32_t e = j2k_packets(P.j2streams[i], P.j2packets.data(), P.j2bands.data(), s->data, tt.data(),
                                           code.data(), walk.data(), con.data()))
            return fail(PBX_E_BADARG, "corrupt segment stream %u (j2k, decoder code %u)", (unsigned)i, e);
    std::vector<int32_t> scr(P.scratch / 4, 0);
    // k_tiff_j2k_gather: each stream's gather area a heap block of exactly its planned size
    std::vector<std::vector<uint8_t>> gat(P.j2streams.size());
    for (size_t i = 0; i < P.j2streams.size(); i++)
        if (P.j2streams[i].ncon) gat[i].assign(P.j2streams[i].len, 0);
    for (const J2Contrib& G : con) {
        if (!G.len || G.block >= P.j2blocks.size()) continue;
        const uint32_t si = P.j2blocks[G.block].stream;
        const J2Stream& S = P.j2streams[si];
        uint32_t from, to;
        if (!j2k_gather_span(S, code[G.block], G, &from, &to)) continue;
        memcpy(gat[si].data() + to, s->data + S.src_off + from, G.len);
    }
    for (size_t i = 0; i < P.j2blocks.size(); i++) {
        const J2Block& B = P.j2blocks[i];
        const J2Code& C = code[i];
        const J2Stream& S = P.j2streams[B.stream];
        const uint32_t w = B.w, h = B.h, planes = B.mb - C.zbp;
        if (w * h > P.j2coef || (w + 2) * (h + 2) > P.j2flag) return fail(PBX_E_INTERNAL, "j2k plan: block %zu outgrows the launch", i);
        std::vector<int32_t> mag(w * h, 0);
        std::vector<uint8_t> flg((w + 2) * (h + 2), 0), ctx(19, 0);
        ctx[0] = 4 << 1; ctx[17] = 3 << 1; ctx[18] = 46 << 1;
        const uint8_t* run = j2k_code_bytes(S, C, s->data + S.src_off, gat[B.stream].data());
        if (C.passes && C.zbp < B.mb && planes <= (B.irrev ? 30u : 31u) && C.passes <= 3 * planes - 2 && run) {
            // the block's bytes in a heap block of their own: a read past them is caught
            const std::vector<uint8_t> bytes(run, run + C.len);
            if (B.irrev) j2k_block<true>(mag.data(), flg.data(), ctx.data(), mq, bytes.data(), C.len, w, h, B.orient, planes, C.passes);
            else j2k_block<false>(mag.data(), flg.data(), ctx.data(), mq, bytes.data(), C.len, w, h, B.orient, planes, C.passes);
        }
        for (uint32_t y = 0; y < h; y++)
            for (uint32_t x = 0; x < w; x++) {
                const bool neg = flg[(y + 1) * (w + 2) + x + 1] & J2F_NEG;
                int32_t& to = scr[B.dst / 4 + (uint64_t)y * B.pitch + x];
                if (B.irrev) {  // float planes where the reversible path has int32 ones
                    const float v = j2f_dequant(mag[y * w + x], neg, B.hstep);
                    memcpy(&to, &v, 4);
                } else {
                    to = neg ? -mag[y * w + x] : mag[y * w + x];
                }
            }
    }
    // T.800 F.3: one dimension in place, low-pass samples at the even places
    auto sr = [](std::vector<int64_t>& x) {
        const int64_t n = (int64_t)x.size();
        if (n < 2) return;
        auto at = [&](int64_t i) { return x[i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i]; };
        for (int64_t i = 0; i < n; i += 2) x[i] -= (at(i - 1) + at(i + 1) + 2) >> 2;
        for (int64_t i = 1; i < n; i += 2) x[i] += (at(i - 1) + at(i + 1)) >> 1;
    };
    for (const J2Comp& c : P.j2comps) {
        int32_t* A = scr.data() + c.a / 4;
        if (c.irrev) {  // the inverse 9/7 in float32, tiff_j2k_dev.h's arithmetic: k_tiff_j2k_idwt97's
            std::vector<float> F((uint64_t)c.w * c.h);
            memcpy(F.data(), A, F.size() * 4);
            j2k_host_idwt<float>(F.data(), c, [](std::vector<float>& x) { j2f_sr97(x.data(), (int64_t)x.size(), 1); });
            memcpy(A, F.data(), F.size() * 4);
        } else {
            j2k_host_idwt<int64_t>(A, c, sr);
        }
    }
    for (const TJ2Seg& u : P.j2segs)
        for (uint32_t y = 0; y < u.rows && (int64_t)u.y0 + y < size_y; y++)
            for (uint32_t x = 0; x < u.w && (int64_t)u.x0 + x < size_x; x++) {
                if (u.rct & J2_SEG_IRREV) {  // inverse ICT, level shift, round half to even, clamp
                    float fv[3] = {0, 0, 0};
                    for (uint32_t c = 0; c < u.ncomp; c++) memcpy(&fv[c], &scr[u.src[c] / 4 + j2k_chroma_at(c, x, y, u.w, u.rct)], 4);
                    if (u.ncomp == 3 && (u.rct & 1)) j2f_ict(fv);
                    uint32_t tv[3] = {0, 0, 0};
                    for (uint32_t c = 0; c < u.ncomp; c++) tv[c] = j2f_sample(fv[c], u.prec);
                    if (u.ncomp == 3 && (u.rct & J2_SEG_YCC)) j2k_ycc_rgb(tv);
                    for (uint32_t c = 0; c < u.ncomp; c++) {
                        const uint32_t t = tv[c];
                        const uint64_t at = (uint64_t)c * size_x * size_y + (uint64_t)(u.y0 + y) * size_x + u.x0 + x;
                        if (bpp == 1) ((uint8_t*)out)[at] = (uint8_t)t; else ((uint16_t*)out)[at] = (uint16_t)t;
                    }
                    continue;
                }
                int64_t v[3] = {0, 0, 0};
                for (uint32_t c = 0; c < u.ncomp; c++) v[c] = scr[u.src[c] / 4 + j2k_chroma_at(c, x, y, u.w, u.rct)];
                if (u.ncomp == 3 && (u.rct & 1)) {
                    const int64_t g = v[0] - ((v[1] + v[2]) >> 2), rr = v[2] + g, bb = v[1] + g;
                    v[0] = rr; v[1] = g; v[2] = bb;
                }
                uint32_t tv[3] = {0, 0, 0};
                for (uint32_t c = 0; c < u.ncomp; c++) {
                    const int64_t hi = (1ll << u.prec) - 1;
                    tv[c] = (uint32_t)std::min(hi, std::max<int64_t>(0, v[c] + (1ll << (u.prec - 1))));
                }
                if (u.ncomp == 3 && (u.rct & J2_SEG_YCC)) j2k_ycc_rgb(tv);
                for (uint32_t c = 0; c < u.ncomp; c++) {
                    const uint32_t t = tv[c];
                    const uint64_t at = (uint64_t)c * size_x * size_y + (uint64_t)(u.y0 + y) * size_x + u.x0 + x;
                    if (bpp == 1) ((uint8_t*)out)[at] = (uint8_t)t; else ((uint16_t*)out)[at] = (uint16_t)t;
                }
            }
    return PBX_OK;
}

int pbx_test_tiff_jpeg_plan(const pbx_tiff_segments* s, const pbx_tiff_jpeg* jpeg, int32_t size_x, int32_t size_y,
                            int32_t samples_per_pixel, int32_t y0, int32_t rows, uint64_t out[6]) {
    if (!s || !jpeg || !out) return fail(PBX_E_BADARG, "null argument");
    if (int rc = tiff_jpeg_check(s, jpeg, PBX_UINT8, samples_per_pixel)) return rc;
    if (size_x <= 0 || size_y <= 0) return fail(PBX_E_BADARG, "bad plane size");
    if (rows < 0 || y0 < 0 || (int64_t)y0 + rows > size_y)
        return fail(PBX_E_BADARG, "rows %d+%d outside the plane (%d rows)", y0, rows, size_y);
    ZarrPlan P;
    uint64_t sum = 0;
    const bool band = rows > 0;
    if (int rc = tiff_jpeg_plan(size_x, size_y, s, jpeg, 0, P, band ? y0 / s->seg_h : 0,
                                band ? ((int64_t)y0 + rows + s->seg_h - 1) / s->seg_h : -1, samples_per_pixel, 0, &sum))
        return rc;
    out[0] = P.jstreams.size();
    out[1] = sum;
    out[2] = P.scratch;
    out[3] = P.jtabs.size();
    out[4] = P.jsegs.empty() ? 0 : P.jsegs[0].mode;
    out[5] = 0;
    for (const JStream& t : P.jstreams) out[5] += t.csize;
    return PBX_OK;
}

int pbx_test_tiff_packed_plan(const pbx_tiff_segments* s, const pbx_tiff_packed* k, int32_t size_x, int32_t size_y,
                              int32_t pixel_type, int32_t y0, int32_t rows, uint64_t out[6]) {
    if (!s || !k || !out) return fail(PBX_E_BADARG, "null argument");
    if (int rc = tiff_codec_check(TiffCodec{s, nullptr, false, k}, pixel_type, k->samples_per_pixel, k->sample, 0))
        return rc;
    if (size_x <= 0 || size_y <= 0) return fail(PBX_E_BADARG, "bad plane size");
    if (rows < 0 || y0 < 0 || (int64_t)y0 + rows > size_y)
        return fail(PBX_E_BADARG, "rows %d+%d outside the plane (%d rows)", y0, rows, size_y);
    ZarrPlan P;
    uint64_t sum = 0;
    const bool band = rows > 0;
    if (int rc = tiff_packed_plan(size_x, size_y, s, k, 0, P, band ? y0 / s->seg_h : 0,
                                  band ? ((int64_t)y0 + rows + s->seg_h - 1) / s->seg_h : -1, k->samples_per_pixel, 0,
                                  &sum))
        return rc;
    out[0] = 0;
    for (const auto& kd : P.kind) out[0] += kd.size();
    out[1] = sum;
    out[2] = P.scratch;
    out[3] = P.unpack.size();
    out[4] = P.unpack.empty() ? 0 : P.unpack[0].row_bytes;
    out[5] = 0;
    for (const TUnpack& u : P.unpack) out[5] += u.rows;
    return PBX_OK;
}

// The three tiff_plan hooks: rows == 0 plans the whole plane as a registration does, rows > 0 the
// covering segment rows as a band write does; min_rows is the fewest rows the hook takes.
static int tiff_plan_hook(const pbx_tiff_segments* s, int32_t size_x, int32_t size_y, int32_t bpp,
                          int32_t samples_per_pixel, int32_t y0, int32_t rows, int32_t min_rows, uint64_t out[4]) {
    if (!s || !out) return fail(PBX_E_BADARG, "null argument");
    if (int rc = tiff_segments_check(s)) return rc;
    if (size_x <= 0 || size_y <= 0) return fail(PBX_E_BADARG, "bad plane size");
    if (bpp != 1 && bpp != 2 && bpp != 4 && bpp != 8) return fail(PBX_E_BADARG, "bad sample size %d", bpp);
    if (int rc = tiff_samples_check(samples_per_pixel, 0, bpp)) return rc;
    if (rows < min_rows || y0 < 0 || (int64_t)y0 + rows > size_y)
        return fail(PBX_E_BADARG, "rows %d+%d outside the plane (%d rows)", y0, rows, size_y);
    ZarrPlan P;
    uint64_t sum = 0;
    const bool band = rows > 0;
    if (int rc = tiff_plan(size_x, size_y, bpp, true, s, 0, 0, P, &sum, band, band ? y0 / s->seg_h : 0,
                           band ? ((int64_t)y0 + rows + s->seg_h - 1) / s->seg_h : -1, samples_per_pixel, 0))
        return rc;
    out[0] = 0;
    for (const auto& k : P.kind) out[0] += k.size();
    out[1] = sum;
    out[2] = P.scratch;
    out[3] = samples_per_pixel > 1 ? P.split.size()
             : s->predictor == 3   ? P.fplace.size()
                                   : (band ? P.uplace.empty() : P.unpred.empty()) ? 0 : 1;
    return PBX_OK;
}

int pbx_test_tiff_plan(const pbx_tiff_segments* s, int32_t size_x, int32_t size_y, int32_t bpp, uint64_t out[4]) {
    return tiff_plan_hook(s, size_x, size_y, bpp, 1, 0, 0, 0, out);
}

int pbx_test_tiff_plan_samples(const pbx_tiff_segments* s, int32_t size_x, int32_t size_y, int32_t bpp,
                               int32_t samples_per_pixel, int32_t y0, int32_t rows, uint64_t out[4]) {
    return tiff_plan_hook(s, size_x, size_y, bpp, samples_per_pixel, y0, rows, 0, out);
}

// (a band has at least one row: rows < 1 is refused where the other two take 0 for the whole plane)
int pbx_test_tiff_band_plan(const pbx_tiff_segments* s, int32_t size_x, int32_t size_y, int32_t bpp, int32_t y0,
                            int32_t rows, uint64_t out[4]) {
    return tiff_plan_hook(s, size_x, size_y, bpp, 1, y0, rows, 1, out);
}

}  // extern "C"
