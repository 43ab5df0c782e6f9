// source_plan.h — what runtime.cpp calls of source_plan.cpp: the host-side parsers and planners
// of the source formats (Zarr chunks, TIFF segments, JPEG and JPEG 2000 streams) and the
// thread's last error.  Plain C++: no HIP header, no context, no device call.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pbx.h"
#include "pbx_decode_types.h"

namespace pbx {

// Sets the calling thread's last error (pbx_last_error) and returns `code`.
int fail(int code, const char* fmt, ...);
// The calling thread's last error, to save and restore around calls that may overwrite it.
std::string& last_error();

inline int bpp_of(int32_t pt) {
    constexpr int kBpp[PBX_NPIXEL_TYPES] = {1, 1, 2, 2, 4, 4, 4, 8};
    return (pt >= 0 && pt < PBX_NPIXEL_TYPES) ? kBpp[pt] : 0;
}

// Host plan of one plane's chunks: metadata only (blosc headers, block starts and split
// sizes); every byte of chunk data is decoded on the GPU.  Frame layout: oracle/zarr_oracle.c.
struct ZarrPlan {
    std::vector<ZStream> kind[ZS_NKINDS];  // streams by decoder (enum ZS_*)
    std::vector<ZChunk> chunks;
    std::vector<ZCheck> checks[ZK_NPOLY];  // by polynomial: CRC-32 of decoded gzip chunks (scratch),
                                           // CRC-32C of crc32c chunks' uploaded bytes (input)
    uint64_t scratch = 0;
    uint64_t skipped = 0;  // blosc blocks left undecoded (deep chunks only)
    std::vector<TUnpred> unpred;  // TIFF segments whose rows are horizontally differenced
    uint32_t unpred_rows = 0;     // the tallest of them
    // pbx_band_write_tiff with Predictor = 2: the segments k_tiff_unpred_place un-predicts and
    // places into the launch's one destination (then no `unpred` and no `chunks`)
    std::vector<TPlace> uplace;
    uint32_t uplace_rows = 0;     // the tallest of them
    bool uplace_big_endian = false;
    // chunky TIFF segments of 2 .. 4 samples per pixel: every segment, whatever its predictor, for
    // k_tiff_split_place (then no `unpred`, no `uplace` and no `chunks`); TPlace::pad names the
    // segment's entry in the launch's TSplitDst table
    std::vector<TPlace> split;
    uint32_t split_rows = 0;      // the tallest of them
    // TIFF segments stored with Predictor = 3 (float / double planes): every segment, registration
    // and band writes alike, for k_tiff_fpunpred_place (then no `unpred`, no `uplace` and no
    // `chunks`); TPlace::pad names the segment's entry in `fdst`, one per tiff_plan call, whose
    // destination fields zarr_decode_place takes from the launch's ZPlane fdst_plane[entry]
    std::vector<TPlace> fplace;
    uint32_t fplace_rows = 0;     // the tallest of them
    std::vector<TPlaceDst> fdst;
    std::vector<uint32_t> fdst_plane;
    // TIFF segments of bit-packed samples (tiff_packed_plan): every segment, registration and band
    // writes alike, for k_tiff_unpack_place (then no `unpred`, no `uplace`, no `chunks`);
    // TUnpack::dst names the segment's entry in the launch's TSplitDst table
    std::vector<TUnpack> unpack;
    uint32_t unpack_rows = 0;     // the tallest of them
    // JPEG-compressed TIFF segments (tiff_jpeg_plan): one JStream and one TJpegSeg per segment
    // (then no `kind`, no `chunks`), the distinct table sets of the launch, and the tallest
    // segment; TJpegSeg::dst names the segment's entry in the launch's TSplitDst table
    std::vector<JStream> jstreams;
    std::vector<TJpegSeg> jsegs;
    std::vector<JTabSet> jtabs;
    uint32_t jseg_rows = 0;
    // JPEG 2000 TIFF segments (tiff_j2k_plan): one J2Stream and one TJ2Seg per segment, a J2Comp
    // per component of it, a J2Band per sub-band of those and a J2Block per code block, a
    // J2Packet per layer and precinct; the tag-tree nodes of the launch, the largest block's LDS needs, and the tallest segment
    std::vector<J2Stream> j2streams;
    std::vector<J2Packet> j2packets;   // every stream's packet list, in stream order
    std::vector<J2Band> j2bands;
    std::vector<J2Block> j2blocks;
    std::vector<J2Comp> j2comps;
    std::vector<TJ2Seg> j2segs;
    uint64_t j2nodes = 0;
    uint64_t j2cons = 0;               // entries of the J2Contrib table (streams of several layers)
    uint32_t j2coef = 0, j2flag = 0, j2seg_rows = 0, j2irrev = 0;  // j2irrev: irreversible (9/7) j2comps
};

// A plane cut out of a layer of chunks that hold `depth` planes each: its slice of every chunk
// and its index in the launch's ZPlane table.
struct ZarrWant {
    uint32_t slice, plane;
};

// The checks and planners: each is described where it is defined (source_plan.cpp).  All return
// PBX_OK or fail(); the planners append to P.
int zarr_chunks_check(const pbx_zarr_chunks* z);
int zarr_slice_check(int32_t depth, int64_t slice);
int zarr_plan(int32_t size_x, const pbx_zarr_chunks* z, int bpp, uint64_t in_base, int64_t cy0, int64_t cy1,
              int32_t depth, const std::vector<ZarrWant>& want, int64_t y_lo, int64_t y_hi, ZarrPlan& P);

int tiff_segments_check(const pbx_tiff_segments* s);
int tiff_samples_check(int32_t spp, int64_t sample, int bpp);
int tiff_fp_predictor_check(const pbx_tiff_segments* s, int32_t pixel_type);
int tiff_plan(int32_t size_x, int32_t size_y, int bpp, bool big_endian, const pbx_tiff_segments* s,
              uint64_t in_base, uint32_t plane, ZarrPlan& P, uint64_t* dlen_sum, bool band = false,
              int64_t sr0 = 0, int64_t sr1 = -1, int spp = 1, uint32_t split_dst = 0);

int tiff_jpeg_check(const pbx_tiff_segments* s, const pbx_tiff_jpeg* j, int32_t pixel_type, int32_t spp);
int tiff_jpeg_plan(int32_t size_x, int32_t size_y, const pbx_tiff_segments* s, const pbx_tiff_jpeg* j, uint64_t in_base,
                   ZarrPlan& P, int64_t sr0, int64_t sr1, int spp, uint32_t dst, uint64_t* dlen_sum = nullptr);

int tiff_j2k_check(const pbx_tiff_segments* s, int32_t pixel_type, int32_t spp);
int tiff_j2k_plan(int32_t size_x, int32_t size_y, int bpp, const pbx_tiff_segments* s, uint64_t in_base, ZarrPlan& P,
                  int64_t sr0, int64_t sr1, int spp, uint32_t dst, uint64_t* packets = nullptr);

// Bit-packed samples (pbx_*_tiff_packed): the fields of `k` that can be checked with the plane's
// pixel type alone, and tiff_segments_check's with PackBits among the compressions.
int tiff_packed_check(const pbx_tiff_segments* s, const pbx_tiff_packed* k, int32_t pixel_type);
// Padded bytes of a segment row: ceil(seg_w * spp * bits / 8).
inline uint64_t tiff_packed_row_bytes(int32_t seg_w, int32_t spp, int32_t bits) {
    return ((uint64_t)seg_w * (uint64_t)spp * (uint64_t)bits + 7) >> 3;
}
int tiff_packed_plan(int32_t size_x, int32_t size_y, const pbx_tiff_segments* s, const pbx_tiff_packed* k,
                     uint64_t in_base, ZarrPlan& P, int64_t sr0, int64_t sr1, int spp, uint32_t dst,
                     uint64_t* dlen_sum = nullptr);

// How a pbx_tiff_segments is compressed, as the entry point that took it says: its streams are
// JPEG 2000 codestreams (j2k), JPEG streams with the tables of `jpeg`, rows of bit-packed samples
// as `packed` describes them (under s->compression, PackBits included), or else what
// s->compression names.
struct TiffCodec {
    const pbx_tiff_segments* s;
    const pbx_tiff_jpeg* jpeg;
    bool j2k;
    const pbx_tiff_packed* packed = nullptr;
};
// The codec's own check (tiff_j2k_check, tiff_jpeg_check, tiff_packed_check or tiff_segments_check), then what holds
// for all: no Predictor = 2 on float / double, tiff_fp_predictor_check, tiff_samples_check.
// `plane_label` is the number messages call the plane by.
int tiff_codec_check(const TiffCodec& c, int32_t pixel_type, int32_t spp, int64_t sample, uint64_t plane_label);
// tiff_j2k_plan, tiff_jpeg_plan or tiff_plan of segment rows [sr0, sr1) (sr1 < 0: all) with the
// arguments each takes; `dst` is the layer's entry in the launch's TSplitDst table.
int tiff_codec_plan(const TiffCodec& c, int32_t size_x, int32_t size_y, int bpp, bool big_endian, uint64_t in_base,
                    uint32_t plane, ZarrPlan& P, bool band, int64_t sr0, int64_t sr1, int spp, uint32_t dst);

// The segments (chunks) that cover rows [y0, y0 + rows) (rows < 0: every row) of a plane of
// size_x x size_y: gx across, rows [r0, r1) of the grid, and the bytes those gx * (r1 - r0) streams
// take in `data`, which holds them alone (offsets[gx * (r1 - r0)]).
struct SourceGrid {
    int64_t gx, r0, r1;
    uint64_t used;
};
SourceGrid source_grid(const pbx_tiff_segments* s, int32_t size_x, int32_t size_y, int32_t y0 = 0, int32_t rows = -1);
SourceGrid source_grid(const pbx_zarr_chunks* z, int32_t size_x, int32_t size_y, int32_t y0 = 0, int32_t rows = -1);

// What one decode launch uploads of a finished plan and where its decoders report: the tables
// that are not the plan's own vectors, and the layout of err[].
struct LaunchLayout {
    uint32_t counts[ZS_NKINDS];  // streams by kind
    std::vector<ZStream> streams;  // P.kind[0], P.kind[1], ... one after another
    // checks by polynomial, and within one the ranges shorter than the CRC split length (a wave
    // each) before the others (a workgroup each): polynomial k has ck_n[k] checks from
    // ck_first[k], the first ck_wave[k] of them short
    std::vector<ZCheck> checks;
    uint32_t ck_first[ZK_NPOLY], ck_wave[ZK_NPOLY], ck_n[ZK_NPOLY];
    std::vector<TJ2Seg> j2segs;  // P.j2segs, those with J2_SEG_CHROMA after the others (stable)
    uint32_t j2chroma;           // how many those are
    uint64_t j2meta;             // bytes of the J2Code, J2Walk and J2Contrib tables and the tag-tree nodes
    // err[]: a dword per stream, per check (in `checks` order), per JPEG stream and per JPEG 2000 stream
    uint32_t nstreams, nchecks, njpeg, nj2;
    uint32_t err_streams, err_checks, err_jpeg, err_j2k, nerr;
    LaunchLayout(const ZarrPlan& P, uint32_t crc_split);
};
// The first non-zero entry of a launch's err[] (nerr dwords) as the 400 it stands for, or PBX_OK.
int launch_errors(const LaunchLayout& L, const uint32_t* err);

}  // namespace pbx
