// pbx_kernels.h — host-side launchers of the gfx950 kernels: the tile pipeline (kernels_io.hip,
// kernels_deflate.hip, kernels_deflate_strategy.hip, kernels_tiff_predictor.hip) and the source
// decoders (kernels_zarr.hip, kernels_zstd.hip, kernels_tiff_src.hip, kernels_tiff_jpeg.hip,
// kernels_tiff_j2k.hip).  The tables the decoders take are plain structs the host planners fill
// (source_plan.cpp); they live in pbx_decode_types.h, which needs no HIP.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbx_common.h"
#include "pbx_decode_types.h"

namespace pbx {

// Synthetic plane (G_FAKE / G_NOISE) written little-endian into a pitched HBM plane.
// rows [y0, y0 + rows) of a synthetic plane, row y0 at `out`
hipError_t launch_gen_plane(hipStream_t st, uint8_t* out, int64_t pitch, int32_t sx, int32_t y0,
                            int32_t rows, int32_t pixel_type, int32_t kind, uint64_t seed,
                            int32_t plane_no, int32_t z, int32_t c, int32_t t);

// K1: raw / uncompressed-TIFF tiles (getTileDirect + big-endian; TIFF header in front).
// Resolution pyramid level: dst (dx x dy) = 2x2 box mean of src (sx x sy), edge samples
// repeated for odd sizes; samples big-endian in memory when `be`.
hipError_t launch_downsample(hipStream_t st, const uint8_t* src, int64_t spitch, int32_t sx, int32_t sy,
                             uint8_t* dst, int64_t dpitch, int32_t dx, int32_t dy, int32_t pixel_type,
                             bool be);
// Rows [y0, y0 + rows) of level r + k (k = 1 .. 4; row y0 at `dst`) from level r (sx x sy) in one
// pass, bit for bit what k launch_downsample calls leave there.  Source row Y is in band
// Y / band_rows, whose first row is at d_bands[Y / band_rows - band0] (a device table); only rows
// [y0 << k, min((y0 + rows) << k, sy)) are read.  k = 1: k_reduce_band1 (k_downsample's loop over banded
// rows); k >= 2: the tiled k_reduce_band, except where it was measured slower than the chain of
// single levels -- those (type, k) go level by level through `scratch`, reduce_band_scratch_bytes()
// bytes of it (0: none needed, scratch may be null).
size_t reduce_band_scratch_bytes(int32_t sx, int32_t sy, int32_t y0, int32_t rows, int32_t k, int32_t pixel_type);
hipError_t launch_reduce_band(hipStream_t st, const uint8_t* const* d_bands, int32_t band0, int32_t band_rows,
                              int64_t spitch, int32_t sx, int32_t sy, uint8_t* dst, int64_t dpitch, int32_t y0,
                              int32_t rows, int32_t k, int32_t pixel_type, bool be, uint8_t* scratch);
// test hook (pbx_test_stall_batch): one wave spinning until *flag == 0 or limit_ticks of the
// 100 MHz constant clock
hipError_t launch_stall(hipStream_t st, const uint32_t* flag, uint64_t limit_ticks);
hipError_t launch_extract(hipStream_t st, const TileDesc* d_tiles, uint32_t ntiles,
                          uint32_t nblocks, uint8_t* out, bool unaligned);
// Tiled-TIFF headers (IFD + TileOffsets/TileByteCounts), one workgroup per response: after
// k_extract for uncompressed responses (in `fixed`), after k_frame for deflate ones (`zout`).
hipError_t launch_tiff_tiled(hipStream_t st, const TiledHdr* d_th, uint32_t nth, uint8_t* fixed,
                             const uint64_t* offs, uint8_t* zout);

// K1+K2: extract + byte swap + sign flip + PNG filter (or raw BE bytes for deflate-TIFF)
// into the per-tile byte streams the deflate kernels read.  One workgroup per band.
hipError_t launch_filter(hipStream_t st, const TileDesc* d_tiles, uint32_t ntiles,
                         uint32_t nblocks, uint8_t* stream);
uint32_t filter_band_rows();
// PNG tiles with a Sub/Up/Avg/Paeth/adaptive filter and rows of whole dwords (<= 2 KiB,
// 16-byte aligned source): the same streams from dword-wide filter arithmetic (k_filter2).
hipError_t launch_filter2(hipStream_t st, const TileDesc* d_tiles, uint32_t ntiles, uint32_t nblocks,
                          uint32_t max_rb, uint8_t* stream);
uint32_t filter2_band_rows();
// PNG-filtered tiles with rows of whole 16-byte chunks (<= filter3_max_rb()): one wave per run
// of filter3_run_rows() rows, no LDS (k_filter3); nwaves = the runs of every tile; filter =
// the batch's PNG filter (1..4, 5 = adaptive), which every tile's d.filter holds
hipError_t launch_filter3(hipStream_t st, const TileDesc* d_tiles, uint32_t ntiles, uint32_t nwaves,
                          uint32_t max_rb, uint32_t filter, uint8_t* stream);
uint32_t filter3_run_rows(uint32_t filter);  // rows per wave for the PNG filter 1..5
// The adaptive option's tile mode, before the filter kernels: TF_ANONE of every adaptive PNG
// tile of d_tiles[0, ntiles) (one workgroup per tile; other tiles are left alone); max_rb: the
// widest of their rows in bytes.
hipError_t launch_adaptive_mode(hipStream_t st, TileDesc* d_tiles, uint32_t ntiles, uint32_t max_rb);
uint32_t filter3_max_rb();
uint32_t filter2_max_rb();

// K1+K2 for filter-None PNG rows and deflate-TIFF rows from 16-byte-aligned source rows:
// one workgroup per band of ROWS_BAND rows, staged in LDS, aligned 16-byte stream words.
constexpr uint32_t ROWS_BAND = 16;
constexpr uint32_t ROWS_MAX_RB = 8192;  // widest row (bytes) k_rows takes (LDS band <= 132 KB)
hipError_t launch_rows(hipStream_t st, const TileDesc* d_tiles, uint32_t ntiles, uint32_t nblocks,
                       uint32_t max_rb, uint8_t* stream);
inline uint32_t rows_blocks_for(uint32_t h) { return (h + ROWS_BAND - 1) / ROWS_BAND; }

// TIFF Predictor = 2 (kernels_tiff_predictor.hip): the horizontally differenced stream of TF_PRED
// tiles.  k_tiff_pred3: 16-byte aligned source rows of whole 16-byte chunks (<= filter3_max_rb()),
// one wave per run of tiff_pred3_run_rows() rows, no LDS; nwaves = the runs of every tile
// (TileDesc::rows_per_blk = a tile's first wave; a tile with none is skipped).  k_tiff_pred:
// every other tile (any x, any width, padded tiled-TIFF sub-tiles), one workgroup per band of
// TIFF_PRED_BAND rows staged in LDS (TileDesc::blk_first = a tile's first workgroup; a tile
// with none is skipped); max_rb = the widest row of at most ROWS_MAX_RB bytes (wider rows use
// no LDS).  The sub-tiles of tiled responses are in both kernels' tile ranges.
constexpr uint32_t TIFF_PRED_BAND = 16;
uint32_t tiff_pred3_run_rows();
hipError_t launch_tiff_pred3(hipStream_t st, const TileDesc* d_tiles, uint32_t ntiles, uint32_t nwaves,
                             uint32_t max_rb, uint8_t* stream);
hipError_t launch_tiff_pred(hipStream_t st, const TileDesc* d_tiles, uint32_t ntiles, uint32_t nblocks,
                            uint32_t max_rb, uint8_t* stream);

// K3-K6: deflate of every tile's stream into its compacted container.
struct DeflateLaunch {
    const TileDesc* tiles;  // deflate tiles (seg_first / seg_count / out_off = stream offset)
    uint32_t ntiles, nseg;
    uint8_t* stream;        // filtered streams (16-byte aligned per tile, slack after); k_lz77
                            // writes those of TF_DIRECT tiles
    SegInfo* info;          // [nseg]
    uint32_t* hist;         // [nseg * HIST_WORDS]
    uint32_t* mrec;         // [nseg * MREC_WORDS]
    uint32_t* codes;        // [nblk * CODE_WORDS]
    BlkInfo* blk;           // [nblk] Huffman blocks
    uint32_t nblk;
    uint64_t* sizes;        // [ntiles] container bytes
    uint64_t* offs;         // [ntiles + 1] exclusive scan of sizes (offs[ntiles] = total)
    uint64_t* offs_host = nullptr;  // or a mapped pinned copy of offs, written by the scan
    uint8_t* out;           // compacted containers
    uint64_t* stamps;       // [nseg * 32] phase clocks (diagnostics) or nullptr
    uint32_t* seg_tile;     // [nseg] tile of every segment (k_seg_map)
    uint32_t cus = 256;     // compute units of the device (persistent grids)
    uint32_t uniform_nseg = 0;  // every tile has this many segments (tile = seg / it), or 0
    uint32_t uniform_rcp = 0;   // recip32(uniform_nseg)
    bool row_filtered = false;  // some tile's stream is PNG-row-filtered (k_lz77's VALU walk form)
    int32_t strategy = 0;       // deflate strategy of the batch (deflate_seg.h STRAT_*): the k_lz77 instantiation
};
// k_lz77, k_huff, k_seg_sizes + k_scan_offsets, k_encode, k_frame.
// ev[0..3] (and ev2[0..3] if given) are recorded after k_lz77, k_huff, k_scan_offsets, k_encode;
// with fine = false only ev[3] (the serving path's spans need no more).
hipError_t launch_deflate(hipStream_t st, const DeflateLaunch& a, hipEvent_t* ev = nullptr,
                          hipEvent_t* ev2 = nullptr, bool fine = true);
size_t deflate_lds_bytes(int kernel);  // 0 k_lz77, 1 k_huff, 2 k_encode
// k_huff alone (test hook): blk[].seg0 / .nseg and info[].sl / .last must be set.
hipError_t launch_huffman(hipStream_t st, uint32_t nblk, BlkInfo* blk, SegInfo* info,
                          const uint32_t* hist, uint32_t* codes);

// NGFF/Zarr chunk decode (kernels_zarr.hip, kernels_zstd.hip; tables: pbx_decode_types.h).
// Streams ordered by kind (ZS_LZ4| ZS_ZLIB | ZS_COPY | ZS_BLOSCLZ | ZS_ZSTD | ZS_GZIP | ZS_LZW | ZS_PACKBITS), counts[k] of
// kind k; err[i] = 0 or a decoder error code per stream.
// zstd_lit: zstd_scratch_bytes(counts[ZS_ZSTD]) bytes (a block's literals per zstd frame).
hipError_t launch_zarr_decode(hipStream_t st, const ZStream* d_streams, const uint32_t* counts,
                              const uint8_t* src, uint8_t* scratch, uint8_t* zstd_lit, uint32_t* err);
size_t zstd_scratch_bytes(uint32_t nstreams);
hipError_t launch_zarr_zstd(hipStream_t st, const ZStream* d_streams, uint32_t n, const uint8_t* src,
                            uint8_t* scratch, uint8_t* litbuf, uint32_t* err);
// The checks d_checks[0 .. n) must all have polynomial `poly` and be ordered short ranges first:
// the first n_wave get one wave each, the rest a workgroup each (zarr_crc_split() bytes is where
// the host draws the line).  err[i] = 0 or ZK_ERR_MISMATCH.
uint32_t zarr_crc_split();
hipError_t launch_zarr_crc(hipStream_t st, const ZCheck* d_checks, uint32_t n_wave, uint32_t n, uint32_t poly,
                           const uint8_t* input, const uint8_t* scratch, uint32_t* err);
hipError_t launch_zarr_place(hipStream_t st, const ZChunk* d_chunks, uint32_t nchunks,
                             const ZPlane* d_planes, int32_t max_chunk_y, const uint8_t* scratch,
                             const uint8_t* input);

// TIFF segments (kernels_tiff_src.hip); what each kernel does is said at its table
// (pbx_decode_types.h: TUnpred, TPlace, TPlaceDst, TSplitDst).
hipError_t launch_tiff_lzw(hipStream_t st, const ZStream* d_streams, uint32_t n, const uint8_t* src,
                           uint8_t* scratch, uint32_t* err);
hipError_t launch_tiff_unpred(hipStream_t st, const TUnpred* d_segs, uint32_t n, uint32_t max_rows,
                              uint8_t* scratch);
hipError_t launch_tiff_unpred_place(hipStream_t st, const TPlace* d_segs, uint32_t n, uint32_t max_rows,
                                    const TPlaceDst& dst, const uint8_t* scratch, const uint8_t* input);
// k_tiff_fpunpred_place (Predictor = 3 on float / double samples): TPlace::row_bytes = seg_w * bpp
// bytes hold bpp byte planes of seg_w bytes, most significant first, differenced byte by byte
// over the whole row.  The kernel undoes the differences, interleaves the planes into samples in
// the destination's byte order and stores them, clipped as k_tiff_unpred_place clips.  d_dst is a
// device table with one entry per layer of a registration (one for a band write), named by
// TPlace::pad.
hipError_t launch_tiff_fpunpred_place(hipStream_t st, const TPlace* d_segs, uint32_t n, uint32_t max_rows,
                                      const TPlaceDst* d_dst, const uint8_t* scratch, const uint8_t* input);
hipError_t launch_tiff_split_place(hipStream_t st, const TPlace* d_segs, uint32_t n, uint32_t max_rows,
                                   const TSplitDst* d_dst, const uint8_t* scratch, const uint8_t* input);

// Bit-packed samples and PackBits streams (kernels_tiff_packed.hip; TUnpack).  k_tiff_packbits:
// one wave per ZS_PACKBITS stream, launched by launch_zarr_decode.  k_tiff_unpack_place: d_dst is
// the launch's TSplitDst table, TUnpack::dst a segment's entry in it.
hipError_t launch_tiff_packbits(hipStream_t st, const ZStream* d_streams, uint32_t n, const uint8_t* src,
                                uint8_t* scratch, uint32_t* err);
hipError_t launch_tiff_unpack_place(hipStream_t st, const TUnpack* d_segs, uint32_t n, uint32_t max_rows,
                                    const TSplitDst* d_dst, const uint8_t* scratch, const uint8_t* input);

// JPEG-compressed TIFF segments (kernels_tiff_jpeg.hip; JStream, JTabSet, TJpegSeg).
// err[]: 0, or 1 entropy data ends before the last MCU, 2 a code that is in no table, 3 a run that
// passes coefficient 63, 4 a DC size > 11 or an AC size > 10, 5 a restart marker that is missing,
// out of sequence or misplaced.
hipError_t launch_tiff_jpeg_decode(hipStream_t st, const JStream* d_streams, uint32_t n, const JTabSet* d_tabs,
                                   const uint8_t* src, uint8_t* scratch, uint32_t* err);
hipError_t launch_tiff_jpeg_place(hipStream_t st, const TJpegSeg* d_segs, uint32_t n, uint32_t max_rows,
                                  const TSplitDst* d_dst, const uint8_t* scratch);

// JPEG 2000 TIFF segments (kernels_tiff_j2k.hip; J2Stream, J2Packet, J2Band, J2Block, J2Comp,
// TJ2Seg).  k_tiff_j2k_packets (one workgroup per stream), k_tiff_j2k_gather (one wave per entry
// of the contribution table, n_con of them: 0 when every stream has one layer), k_tiff_j2k_blocks (one wave per code block;
// max_coef / max_flag: the most magnitudes / flag bytes a block of the launch needs in LDS),
// k_tiff_j2k_idwt / k_tiff_j2k_idwt97 (one workgroup per component; n_irrev of the n_comps
// components are irreversible, and a kernel none of them needs is not launched).  `meta` holds
// the J2Code table (n_blocks entries), the J2Contrib table (n_con), the J2Walk table (n_blocks) and
// after them the tag-tree nodes, all zero.
hipError_t launch_tiff_j2k_decode(hipStream_t st, const J2Stream* d_streams, uint32_t n_streams,
                                  const J2Packet* d_packets, const J2Band* d_bands, const J2Block* d_blocks,
                                  uint32_t n_blocks, uint32_t n_con, const J2Comp* d_comps, uint32_t n_comps,
                                  uint32_t n_irrev, uint32_t max_coef, uint32_t max_flag, uint8_t* meta,
                                  const uint8_t* src, uint8_t* scratch, uint32_t* err);
// d_segs: the n - n_chroma segments of k_tiff_j2k_place, then the n_chroma ones with J2_SEG_CHROMA
// bits (subsampled or YCbCr components) of k_tiff_j2k_place_chroma
hipError_t launch_tiff_j2k_place(hipStream_t st, const TJ2Seg* d_segs, uint32_t n, uint32_t n_chroma, uint32_t max_rows,
                                 const TSplitDst* d_dst, const uint8_t* scratch);

}  // namespace pbx
