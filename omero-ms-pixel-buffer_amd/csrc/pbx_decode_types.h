// pbx_decode_types.h — the tables of the source decoders: plain structs the host planners fill
// (source_plan.cpp), the runtime uploads as they are and the kernels read (kernels_zarr.hip,
// kernels_zstd.hip, kernels_tiff_src.hip, kernels_tiff_packed.hip, kernels_tiff_jpeg.hip, kernels_tiff_j2k.hip), with the
// decoders' stream kinds and error codes.  Plain C++ (no HIP headers): the launchers that take
// these tables are declared in pbx_kernels.h.
#pragma once
#include <stdint.h>

#include "pbx_common.h"

namespace pbx {

// NGFF/Zarr chunk decode (kernels_zarr.hip).  One wave per stream.
// ZS_GZIP: a raw deflate body followed by the 8 trailer bytes of its RFC 1952 member (the host
// has parsed the header); k_zarr_inflate2 takes no zlib header and no Adler-32 for it and
// requires the deflate data to end exactly 8 bytes before the stream's end.
// ZS_LZW: a TIFF 6.0 LZW strip or tile (kernels_tiff_src.hip).
// ZS_PACKBITS: a TIFF 6.0 PackBits strip or tile (kernels_tiff_packed.hip).
enum : uint32_t { ZS_LZ4 = 0, ZS_ZLIB = 1, ZS_COPY = 2, ZS_BLOSCLZ = 3, ZS_ZSTD = 4, ZS_GZIP = 5, ZS_LZW = 6,
                  ZS_PACKBITS = 7, ZS_NKINDS = 8 };
struct ZStream {
    uint64_t src_off;  // compressed bytes in the uploaded chunk buffer
    uint64_t dst_off;  // decoded bytes in the scratch buffer
    uint32_t csize, dlen, kind, pad;
};
enum : uint32_t { ZC_MISSING = 1u, ZC_INPUT = 2u, ZC_BITSHUF = 4u };
struct ZChunk {
    uint64_t src;                         // decoded chunk: scratch offset (or input offset if ZC_INPUT)
    uint32_t nbytes, blocksize, typesize; // blosc geometry (typesize 1 = not byte-shuffled;
                                          // with ZC_BITSHUF the bit-shuffle element size)
    uint32_t flags;                       // ZC_*
    int32_t x0, y0;                       // chunk origin in the plane
    uint32_t plane;                       // index into the ZPlane table of the launch
    uint32_t e0;                          // first element of the plane's slice in the decoded chunk
                                          // (slice * chunk_y * chunk_x; 0 for one plane per chunk)
};
static_assert(sizeof(ZChunk) == 40, "ZChunk is uploaded as is");
struct ZPlane {                           // a destination plane of one decode launch
    uint8_t* dev;                         // row 0 of the plane (a band: its virtual base)
    int64_t pitch;
    int32_t sx, sy, cw, chh;              // plane and chunk shape
    uint32_t bpp, pad;
    uint64_t fill;                        // fill bytes in stored order (missing chunks)
    int32_t y_lo, y_hi;                   // plane rows k_zarr_place may write: [y_lo, y_hi)
};

// Checksums of byte ranges (k_zarr_crc): the v3 crc32c codec over the uploaded chunk bytes, the
// gzip trailer's CRC-32 over the decoded chunk.  Ranges have any byte alignment and length.
enum : uint32_t { ZK_INPUT = 0, ZK_SCRATCH = 1 };             // ZCheck::buf
enum : uint32_t { ZK_CRC32 = 0, ZK_CRC32C = 1, ZK_NPOLY = 2 };  // ZCheck::poly
constexpr uint32_t ZK_ERR_MISMATCH = 40;  // err[] code of a range whose checksum differs
struct ZCheck {
    uint64_t off;      // first byte, in the buffer `buf` names
    uint32_t len;      // bytes
    uint32_t expect;   // the checksum the range must have (standard: init and final xor ~0)
    uint32_t buf, poly;
};
static_assert(sizeof(ZCheck) == 24, "ZCheck is uploaded as is");

// TIFF segments (kernels_tiff_src.hip).  k_tiff_lzw: one wave per ZS_LZW stream, err[] as the
// Zarr decoders'.  k_tiff_unpred: the inverse of Predictor = 2 in place on decoded segments in
// scratch: `rows` rows of row_bytes bytes (a multiple of bpp = 1, 2 or 4) from `off`; max_rows =
// the tallest segment of the launch.
struct TUnpred {
    uint64_t off;
    uint32_t row_bytes, rows, bpp, big_endian;
};
static_assert(sizeof(TUnpred) == 24, "TUnpred is uploaded as is");

// k_tiff_unpred_place (pbx_band_write_tiff, Predictor = 2): the inverse of the predictor and the
// placement in one pass.  Rows [y_lo, y_hi) of the destination that a segment holds are read at
// the segment's own pitch (from scratch, or from the upload buffer for a stored segment),
// summed in registers and stored into the pitched plane; its other rows are not touched.
struct TPlace {
    uint64_t src;        // the segment's decoded bytes: scratch offset (input offset with from_input)
    uint32_t row_bytes;  // seg_w * bpp, the segment's own pitch
    uint32_t rows;       // rows it holds (a short last strip: the rows left)
    int32_t x0, y0;      // its origin in the plane
    uint32_t from_input;
    uint32_t pad;        // k_tiff_split_place: the segment's entry in the launch's TSplitDst table
                         // (k_tiff_fpunpred_place: in its TPlaceDst table)
};
static_assert(sizeof(TPlace) == 32, "TPlace is uploaded as is");
struct TPlaceDst {       // passed by value
    uint8_t* dev;        // row 0 of the plane (a band: its virtual base), 256-byte aligned
    int64_t pitch;       // a multiple of 256
    int32_t sx, sy;      // plane size in samples
    int32_t y_lo, y_hi;  // plane rows that may be written
    uint32_t bpp;        // 1, 2 or 4 (k_tiff_fpunpred_place: 4 or 8)
    uint32_t big_endian;
};
static_assert(sizeof(TPlaceDst) == 40, "TPlaceDst is uploaded as is (k_tiff_fpunpred_place)");

// k_tiff_split_place (SamplesPerPixel 2 .. 4, PlanarConfiguration 1): a segment row holds spp
// interleaved samples per pixel (TPlace::row_bytes = seg_w * bpp * spp).  The kernel undoes
// Predictor = 2 with a stride of spp samples and stores component s of every pixel into plane
// dev[s]; a null dev[s] is a component nobody wants (a band write stores one).  One table entry
// per layer (TPlace::pad), so one launch serves every layer of a registration.
struct TSplitDst {
    uint8_t* dev[4];     // row 0 of component s's plane (a band: its virtual base), 256-byte aligned
    int64_t pitch;       // of every plane of the entry, a multiple of 256
    int32_t sx, sy;      // plane size in pixels
    int32_t y_lo, y_hi;  // plane rows that may be written
    uint32_t bpp;        // bytes per sample: 1, 2 or 4
    uint32_t big_endian;
    uint32_t spp;        // 2, 3 or 4
    uint32_t predictor;  // 1 or 2
};
static_assert(sizeof(TSplitDst) == 72, "TSplitDst is uploaded as is");

// k_tiff_unpack_place (kernels_tiff_packed.hip; pbx_planes_register_tiff_packed and
// pbx_band_write_tiff_packed): a segment whose rows are bit streams of `bits`-wide samples, MSB
// first, every row padded to a whole byte: row_bytes = ceil(seg_w * spp * bits / 8).  Sample i of
// a row is component i % spp of pixel i / spp and goes, unscaled, as uint8 (bits <= 8) or uint16
// into plane dev[i % spp] of entry `dst` of the launch's TSplitDst table (bpp 1 or 2 to match;
// spp 1 .. 4; predictor unused), clipped as k_tiff_split_place clips.  Also k_tiff_packbits: one
// wave per ZS_PACKBITS stream, err[] 0, or 1 the stream ends before dlen bytes are out, 3 a run
// past dlen.
struct TUnpack {
    uint64_t src;        // the segment's decoded bytes: scratch offset (input offset with from_input)
    uint32_t row_bytes;  // the segment's own pitch
    uint32_t rows;       // rows it holds (a short last strip: the rows left)
    int32_t x0, y0;      // its origin in the plane
    uint32_t from_input;
    uint32_t dst;        // its entry in the launch's TSplitDst table
    uint32_t seg_w;      // pixels of a row (a tile's padded width)
    uint32_t bits;       // 1 .. 16
    uint32_t fill_order; // 1, or 2: the bits of every source byte are reversed first
    uint32_t pad;
};
static_assert(sizeof(TUnpack) == 48, "TUnpack is uploaded as is");

// JPEG-compressed TIFF segments (kernels_tiff_jpeg.hip; Compression = 7, baseline streams of
// 8-bit samples).  The host parses the marker segments; the tables reach the device resolved per
// component of the scan, one JTabSet per distinct set of a launch.
// JHuff, a canonical Huffman code as the decoder reads it: lut[the next 9 bits] = length << 8 |
// symbol for codes of at most 9 bits (0: a longer code, or none), and for longer ones libjpeg's
// walk: the code of l bits is in the table if it is <= maxcode[l] (-1: no code of that length),
// and its symbol is val[code + valoff[l]].
struct JHuff {
    uint16_t lut[512];
    int32_t maxcode[18];  // [1 .. 16]
    int32_t valoff[18];   // [1 .. 16]: index of the first symbol of that length - its code
    uint8_t val[256];
};
static_assert(sizeof(JHuff) == 1424, "JHuff is uploaded as is");
struct JTabSet {
    uint16_t q[3][64];    // component c's quantiser, de-zigzagged (row-major)
    JHuff h[6];           // component c's DC table at 2 c, its AC table at 2 c + 1
};
static_assert(sizeof(JTabSet) == 8928, "JTabSet is uploaded as is");
// One stream (a strip or tile).  Its decoded planes lie in scratch from dst_off: component 0 with
// mcuy * vs * 8 rows of pitch0 bytes, then (ncomp == 3) components 1 and 2 at offc1 / offc2 with
// mcuy * 8 rows of pitchc bytes.  Pitches are multiples of 16, the offsets of 256.
struct JStream {
    uint64_t src_off;     // the entropy-coded data (after the SOS header) in the upload buffer
    uint64_t dst_off;
    uint32_t csize;       // bytes from src_off to the segment's end
    uint32_t tabset;      // index into the launch's JTabSet table
    uint32_t ncomp;       // 1 or 3
    uint32_t hs, vs;      // component 0's sampling factors: 1x1, 2x1 or 2x2 (the others: 1x1)
    uint32_t mcux, mcuy;  // the MCU grid
    uint32_t restart;     // restart interval in MCUs, 0 = none
    uint32_t pitch0, pitchc, offc1, offc2;
};
static_assert(sizeof(JStream) == 64, "JStream is uploaded as is");

// k_tiff_jpeg_place: a decoded segment (JStream's planes) upsampled, converted, split and placed
// into the planes of entry `dst` of the launch's TSplitDst table (bpp 1; spp 1 or 3; a null dev[s]
// is a component nobody wants), clipped as k_tiff_split_place clips.
enum : uint32_t { JM_COPY = 0, JM_YCC = 1, JM_YCC_H2V1 = 2, JM_YCC_H2V2 = 3 };
struct TJpegSeg {
    uint64_t src;         // JStream::dst_off
    uint32_t offc1, offc2, pitch0, pitchc;
    uint32_t w, rows;     // the segment's own size in pixels (the SOF's)
    int32_t x0, y0;       // its origin in the plane
    uint32_t mode;        // JM_*: components as they are (gray, or RGB stored as such), or YCbCr
                          // -> RGB with component 0 at 1x1, 2x1 (h2v1) or 2x2 (h2v2)
    uint32_t ncomp;       // 1 or 3
    uint32_t dst, pad;
};
static_assert(sizeof(TJpegSeg) == 56, "TJpegSeg is uploaded as is");

// JPEG 2000 TIFF segments (kernels_tiff_j2k.hip; Compression 33003 / 33004 / 33005 / 34712: one
// codestream of one tile per segment, reversible 5/3 or irreversible 9/7).  The host reads SIZ,
// COD and QCD and lays out everything below from them (tiff_j2k_plan); packet headers and
// code-block bytes are read on the device only.
// A component's int32 coefficients live in a plane A of w x h dwords (pitch w) with every
// resolution's low-pass band top left: resolution r covers [0, rh_r) x [0, rw_r), rw_r =
// ceil(w / 2^(levels - r)), its HL band right of resolution r - 1, LH below, HH diagonal.  A
// second plane B of the same size takes the inverse wavelet's horizontal pass.
// An irreversible (9/7) stream's planes hold float32 where a reversible one's hold int32: tier 1
// stores each coefficient dequantised (J2Block::hstep), the wavelet and the placement read floats.
struct J2Band {            // one sub-band of one component of one stream
    uint32_t blk0;         // its first code block in the launch's J2Block / J2Code tables
    uint32_t nbx, nby;     // the code-block grid, raster order (0 x 0: an empty band)
    uint32_t mb;           // magnitude bit-planes: guard bits + exponent - 1 (0 .. 31)
    float hstep;           // 9/7: half the quantisation step (its blocks carry it too), else 0
};
static_assert(sizeof(J2Band) == 20, "J2Band is uploaded as is");
// One packet (T.800 B.9) of a stream's packet list: the host runs the progression order's loops
// (B.12.1.1 - 5) over layers, resolutions, components and precincts and writes the packets down in
// the order the stream holds them; tier 2 walks the list.  A precinct's part of a sub-band is a
// window into the band's code-block grid, with a pair of tag trees of its own that all the layers'
// packets of that precinct share.
struct J2Window {
    uint32_t tt;           // its inclusion tag tree in the launch's node table (dwords); the
                           // zero-bit-plane tree follows it
    uint32_t nodes;        // nodes of one tree
    uint32_t tlevels;      // levels of one tree
    uint32_t x0, y0;       // its first code block in the band's grid
    uint16_t nx, ny;       // its code blocks (0 x 0: the precinct misses the band)
};
static_assert(sizeof(J2Window) == 24, "J2Window is uploaded as is");
struct J2Packet {
    uint32_t band;         // the first J2Band of its resolution
    uint16_t layer;
    uint16_t nbands;       // 1 (resolution 0) or 3
    J2Window win[3];
};
static_assert(sizeof(J2Packet) == 80, "J2Packet is uploaded as is");
struct J2Stream {
    uint64_t src_off;      // the packets (after SOD) in the upload buffer
    uint64_t gather;       // scratch offset of its gather area (layers > 1): `len` bytes
    uint32_t len;          // the packets' bytes
    uint32_t band0;        // component c's band b (QCD order) is J2Band band0 + c * (3 levels + 1) + b
    uint32_t ncomp, levels;
    uint32_t pk0, npk;     // its packets in the launch's J2Packet table, in stream order
    uint32_t blk0, nblk;   // its code blocks in the launch's J2Block / J2Code / J2Walk tables
    uint32_t con0, ncon;   // its room in the launch's J2Contrib table: nblk * layers, 0 with one layer
    uint32_t layers;       // 1 .. 64
    uint32_t mode;         // J2S_*
};
static_assert(sizeof(J2Stream) == 64, "J2Stream is uploaded as is");
// J2Stream::mode: the irreversible 9/7 path (float planes); Scod bit 1: a packet may start with an
// SOP marker segment; Scod bit 2: every packet header ends with an EPH marker
enum : uint32_t { J2S_IRREV = 1, J2S_SOP = 2, J2S_EPH = 4 };
struct J2Block {
    uint64_t dst;          // scratch offset of its first coefficient in the component's plane A
    uint32_t pitch;        // of that plane, in dwords
    uint16_t w, h;         // clipped to the band
    uint32_t stream;
    uint8_t orient, mb;    // 0 LL, 1 HL, 2 LH, 3 HH
    uint16_t irrev;        // 1: magnitudes keep the half bit below and are stored as float * hstep
    float hstep;           // half the band's quantisation step (0 on the reversible path)
    uint32_t pad;
};
static_assert(sizeof(J2Block) == 32, "J2Block is uploaded as is");
struct J2Code {            // written by k_tiff_j2k_packets (zero: the block is never included)
    uint32_t off, len;     // its bytes: one run of len bytes at off & ~J2C_GATHERED from
                           // J2Stream::src_off, or with J2C_GATHERED from J2Stream::gather in scratch;
                           // checked against J2Stream::len
    uint32_t passes, zbp;  // zbp <= mb and passes <= 3 (mb - zbp) - 2, summed over the layers
};
constexpr uint32_t J2C_GATHERED = 0x80000000u;  // (a stream has fewer than 2^31 bytes)
struct J2Walk {            // tier 2's state of one block between a packet's header and its data, and
                           // from layer to layer
    uint32_t lblock;       // Lblock - 3 | its contributions of at least one byte so far << 8
    uint32_t pend;         // the length its header gave in this packet + 1, 0: not in this packet
};
// A block's bytes in one packet, for k_tiff_j2k_gather: recorded for every block of a stream of
// several layers, then cleared (len 0) where the block has no other, which is read where it lies.
struct J2Contrib {
    uint32_t block;        // in the launch's tables
    uint32_t off, len;     // from J2Stream::src_off
    uint32_t at;           // where they go in the block's run: its bytes before this packet
};
static_assert(sizeof(J2Contrib) == 16, "J2Contrib is a device table");
struct J2Comp {            // one component of one stream, for the inverse wavelet
    uint64_t a, b;         // its planes in scratch
    uint32_t w, h, levels; // its own size: ceil(W / XRsiz) x ceil(H / YRsiz) of a subsampled one
    uint32_t irrev;        // 1: float planes, k_tiff_j2k_idwt97's; 0: int32 planes, k_tiff_j2k_idwt's
};
static_assert(sizeof(J2Comp) == 32, "J2Comp is uploaded as is");
struct TJ2Seg {            // one stream, for the placement
    uint64_t src[3];       // its components' planes A (1 and 2 of a subsampled stream: pitch ceil(w / 2)
                           // with J2_SEG_XS2, ceil(rows / 2) rows with J2_SEG_YS2)
    uint32_t w, rows;      // the segment's own size in pixels (the SIZ's)
    int32_t x0, y0;        // its origin in the plane
    uint32_t ncomp;        // 1 or 3
    uint32_t rct;          // bit 0: inverse colour transform (RCT, or ICT on float planes);
                           // bit 1 (J2_SEG_IRREV): float planes of an irreversible stream;
                           // J2_SEG_YCC: YCbCr -> RGB after the clamp; J2_SEG_XS2 / J2_SEG_YS2:
                           // components 1 and 2 at half width / half height.  Any of the last
                           // three: k_tiff_j2k_place_chroma's segment, not k_tiff_j2k_place's
    uint32_t prec;         // 8 or 16
    uint32_t dst;          // its entry in the launch's TSplitDst table
};
static_assert(sizeof(TJ2Seg) == 56, "TJ2Seg is uploaded as is");
// err[]: 0, or 1 a packet header or packet data runs past the stream's end, 2 a malformed packet
// header (a length of more than 32 bits), 3 zero bit-planes above Mb or more passes than the
// bit-planes allow.
enum : uint32_t { J2E_END = 1, J2E_HEADER = 2, J2E_PLANES = 3 };
constexpr uint32_t J2_SEG_IRREV = 2, J2_SEG_YCC = 4, J2_SEG_XS2 = 0x100, J2_SEG_YS2 = 0x200;
constexpr uint32_t J2_SEG_CHROMA = J2_SEG_YCC | J2_SEG_XS2 | J2_SEG_YS2;

}  // namespace pbx
