"""pbx — Python host side of the MI355X /tile pipeline, mirroring the reference's interface.

The reference (glencoesoftware/omero-ms-pixel-buffer, Java) exposes the hot path as
``TileRequestHandler(pixelsService, tileCtx).getTile(client) -> byte[] | null``
(src/main/java/com/glencoesoftware/omero/ms/pixelbuffer/TileRequestHandler.java:74-139),
with the request parsed into a ``TileCtx`` (TileCtx.java:30-92) and replies built by
``PixelBufferVerticle.getTile`` (PixelBufferVerticle.java:90-147).  This module keeps the
same names, argument meanings and error behaviour:

* ``TileCtx.from_params`` raises ``ValueError`` for unparsable numbers (Java
  ``NumberFormatException`` -> HTTP 400, PixelBufferMicroserviceVerticle.java:344-348);
* ``TileRequestHandler.get_tile`` returns ``None`` for every failure the reference maps
  to ``null`` (unknown image, bad region, unsupported type/format: 404), and opens planes
  the GPU does not hold yet from a ``PixelSource`` (getPixels + getPixelBuffer);
* ``handle_get_tile`` reproduces the event-bus consumer: status, body and the
  ``filename`` header.

All compute runs in ``lib/libpbx.so`` (hand-written HIP kernels for gfx950) through the
plain C-ABI in include/pbx.h.  There is no CPU fallback: loading fails loudly if the
library is missing, and ``PixelsService`` raises if no HIP device is present.
"""
from __future__ import annotations

import ctypes
import json
import os
import time
from typing import Dict, Iterable, List, Mapping, Optional, Sequence, Tuple

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PBX_LIB") or os.path.join(os.path.dirname(_PKG_DIR), "lib", "libpbx.so")

# enum pbx_status — the HTTP status the reference ends with; E_NOT_RESIDENT (never sent to a
# client) = the context does not hold the plane: load it and retry (TileRequestHandler below)
OK, E_BADARG, E_NOTFOUND, E_INTERNAL, E_PENDING = 0, 400, 404, 500, 504
E_EXISTS, E_NOT_RESIDENT, E_NO_SPACE = 409, 460, 507
# plane states (pbx_plane_lookup); band states of sparse planes (pbx_plane_band_info)
PS_FILLING, PS_READY, PS_EVICTED = 0, 1, 2
BS_ABSENT, BS_LOADING, BS_READY = 0, 1, 2
# enum pbx_pixel_type (OMERO PixelType names)
PIXEL_TYPES = ["int8", "uint8", "int16", "uint16", "int32", "uint32", "float", "double"]
INT8, UINT8, INT16, UINT16, INT32, UINT32, FLOAT, DOUBLE = range(8)
BYTES_PER_PIXEL = [1, 1, 2, 2, 4, 4, 4, 8]
# enum pbx_format
FMT_RAW, FMT_PNG, FMT_TIF, FMT_UNKNOWN = range(4)
# enum pbx_source / byte order / png filter
SRC_HOST, SRC_GEN_FAKE, SRC_GEN_NOISE = range(3)
BIG_ENDIAN, LITTLE_ENDIAN = 0, 1
FILTER_NONE, FILTER_SUB, FILTER_UP, FILTER_AVG, FILTER_PAETH, FILTER_ADAPTIVE = range(6)
# enum pbx_deflate_strategy: match search in every segment (the reference's Deflater default),
# in none (zlib's Z_HUFFMAN_ONLY), or per segment where a sample of it says matches pay
DEFLATE_DEFAULT, DEFLATE_HUFFMAN_ONLY, DEFLATE_AUTO = range(3)
# enum pbx_tiff_predictor (tag 317's values): deflated TIFF samples as they are (the reference's
# TiffWriter), or every row horizontally differenced (integer pixel types only)
TIFF_PREDICTOR_NONE, TIFF_PREDICTOR_HORIZONTAL = 1, 2


class PbxConfig(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("png_filter", ctypes.c_int32),
                ("tiff_deflate", ctypes.c_int32), ("segment_bytes", ctypes.c_int32),
                ("max_batch_bytes", ctypes.c_uint64), ("coalesce", ctypes.c_int32),
                ("stage_rows", ctypes.c_int32), ("tiff_tile", ctypes.c_int32),
                ("request_timeout_us", ctypes.c_int32)]


class PbxPlaneDesc(ctypes.Structure):
    _fields_ = [("image_id", ctypes.c_int64), ("z", ctypes.c_int32), ("c", ctypes.c_int32),
                ("t", ctypes.c_int32), ("resolution", ctypes.c_int32),
                ("pixel_type", ctypes.c_int32), ("size_x", ctypes.c_int32),
                ("size_y", ctypes.c_int32), ("byte_order", ctypes.c_int32),
                ("source", ctypes.c_int32), ("host_data", ctypes.c_void_p),
                ("host_bytes", ctypes.c_uint64), ("seed", ctypes.c_uint64),
                ("plane_no", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class PbxImageDesc(ctypes.Structure):
    _fields_ = [("image_id", ctypes.c_int64), ("pixel_type", ctypes.c_int32),
                ("size_x", ctypes.c_int32), ("size_y", ctypes.c_int32), ("size_z", ctypes.c_int32),
                ("size_c", ctypes.c_int32), ("size_t_", ctypes.c_int32), ("levels", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class PbxResidencyStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in
                ("budget", "resident_bytes", "planes", "evicted_planes", "evictions", "evicted_bytes",
                 "bands", "band_evictions")]


class PbxZarrChunks(ctypes.Structure):
    _fields_ = [("chunk_x", ctypes.c_int32), ("chunk_y", ctypes.c_int32),
                ("codec", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("data", ctypes.c_void_p), ("offsets", ctypes.c_void_p),
                ("fill_bits", ctypes.c_uint64)]


class PbxTiffSegments(ctypes.Structure):
    _fields_ = [("seg_w", ctypes.c_int32), ("seg_h", ctypes.c_int32), ("tiled", ctypes.c_int32),
                ("compression", ctypes.c_int32), ("predictor", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("data", ctypes.c_void_p), ("offsets", ctypes.c_void_p)]


class PbxTiffJpeg(ctypes.Structure):
    _fields_ = [("tables", ctypes.c_void_p), ("tables_len", ctypes.c_uint64), ("ycbcr", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class PbxTiffPacked(ctypes.Structure):
    _fields_ = [("bits", ctypes.c_int32), ("fill_order", ctypes.c_int32),
                ("samples_per_pixel", ctypes.c_int32), ("sample", ctypes.c_int32)]


def _fill_tiff_packed(k: "PbxTiffPacked", packed: Mapping, samples_per_pixel: int = 1, sample: int = 0) -> None:
    """pbx_tiff_packed from a spec's `packed` dict (bits[, fill_order]) and its samples_per_pixel / sample."""
    k.bits, k.fill_order = packed["bits"], packed.get("fill_order", 1)
    k.samples_per_pixel, k.sample = samples_per_pixel, sample


def _fill_tiff_jpeg(j: "PbxTiffJpeg", jpeg: Mapping) -> object:
    """pbx_tiff_jpeg from a spec's `jpeg` dict (tables = tag 347's bytes or None, ycbcr); returns
    the buffer the struct points into, to be kept alive over the call."""
    tables = jpeg.get("tables")
    buf = ctypes.create_string_buffer(bytes(tables), len(tables)) if tables else None
    j.tables = ctypes.addressof(buf) if buf is not None else None
    j.tables_len = len(tables) if tables else 0
    j.ycbcr, j.reserved = 1 if jpeg.get("ycbcr") else 0, 0
    return buf


def _fill_plane_desc(d: "PbxPlaneDesc", spec: Mapping) -> None:
    """pbx_plane_desc from a plane spec (image_id, z, c, t, pixel_type, size_x, size_y[, level,
    big_endian]); it points at nothing."""
    d.image_id, d.z, d.c, d.t = spec["image_id"], spec["z"], spec["c"], spec["t"]
    d.resolution = spec.get("level", 0)
    d.pixel_type, d.size_x, d.size_y = spec["pixel_type"], spec["size_x"], spec["size_y"]
    d.byte_order = BIG_ENDIAN if spec.get("big_endian", True) else LITTLE_ENDIAN


def _fill_tiff_segments(s: "PbxTiffSegments", spec: Mapping) -> list:
    """pbx_tiff_segments from a spec (seg_w, seg_h, tiled, compression, segments[, predictor,
    flags]); returns the arrays the struct points into, to be kept alive over the call."""
    seg = spec["segments"]
    data, offsets = seg if isinstance(seg, tuple) else pack_chunks(seg)
    s.seg_w, s.seg_h, s.tiled = spec["seg_w"], spec["seg_h"], 1 if spec["tiled"] else 0
    s.compression, s.predictor, s.flags = spec["compression"], spec.get("predictor", 1), spec.get("flags", 0)
    s.data, s.offsets = data.ctypes.data, offsets.ctypes.data
    return [offsets, data]


def _fill_zarr_chunks(zc: "PbxZarrChunks", spec: Mapping) -> list:
    """pbx_zarr_chunks from a spec (chunk_x, chunk_y, codec, chunks[, fill_bits, crc32c]); returns
    the arrays the struct points into, to be kept alive over the call."""
    if spec["codec"] not in ZARR_CODECS:
        raise PbxError(400, "unsupported Zarr compressor %r" % (spec["codec"],))
    chunks = spec["chunks"]
    data, offsets = chunks if isinstance(chunks, tuple) else pack_chunks(chunks)
    zc.chunk_x, zc.chunk_y, zc.codec = spec["chunk_x"], spec["chunk_y"], ZARR_CODECS[spec["codec"]]
    zc.flags = ZARR_F_CRC32C if spec.get("crc32c") else 0
    zc.data, zc.offsets, zc.fill_bits = data.ctypes.data, offsets.ctypes.data, spec.get("fill_bits", 0)
    return [offsets, data]


class PbxZarrSlice(ctypes.Structure):
    _fields_ = [("layer", ctypes.c_uint32), ("slice", ctypes.c_uint32)]


# enum pbx_zarr_codec, keyed by the Zarr v2 compressor id / the v3 bytes-to-bytes codec name;
# pbx_zarr_chunks.flags (ZARR_F_CRC32C: every chunk ends in the v3 crc32c codec's checksum)
ZARR_RAW, ZARR_BLOSC, ZARR_ZLIB, ZARR_ZSTD, ZARR_GZIP = 0, 1, 2, 3, 4
ZARR_F_CRC32C = 1
ZARR_CODECS = {None: ZARR_RAW, "blosc": ZARR_BLOSC, "zlib": ZARR_ZLIB, "zstd": ZARR_ZSTD,
               "gzip": ZARR_GZIP}
_ZARR_DTYPES = {"i1": INT8, "u1": UINT8, "i2": INT16, "u2": UINT16, "i4": INT32, "u4": UINT32,
                "f4": FLOAT, "f8": DOUBLE}


class PbxTileReq(ctypes.Structure):
    _fields_ = [("image_id", ctypes.c_int64), ("z", ctypes.c_int32), ("c", ctypes.c_int32),
                ("t", ctypes.c_int32), ("resolution", ctypes.c_int32), ("x", ctypes.c_int32),
                ("y", ctypes.c_int32), ("w", ctypes.c_int32), ("h", ctypes.c_int32),
                ("format", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class PbxResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("format", ctypes.c_int32), ("w", ctypes.c_int32),
                ("h", ctypes.c_int32), ("data", ctypes.POINTER(ctypes.c_uint8)),
                ("len", ctypes.c_uint64), ("owner", ctypes.c_void_p)]


class PbxBatchStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in
                ("tiles", "ok_tiles", "png_tiles", "raw_tiles", "tif_tiles", "in_bytes",
                 "stream_bytes", "out_bytes", "deflate_out_bytes", "segments")] + \
               [(n, ctypes.c_double) for n in
                ("ms_extract", "ms_filter", "ms_deflate", "ms_assemble", "ms_total",
                  "ms_lz77", "ms_huff", "ms_encode")] + \
               [(n, ctypes.c_uint64) for n in ("blocks", "direct_tiles", "direct_bytes")]


class PbxSpans(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in
                ("get_tile_direct_ms", "write_image_ms", "create_metadata_ms", "batch_ms", "d2h_ms")] + \
               [("batch_tiles", ctypes.c_uint64)]


# Every symbol include/pbx.h declares (tests check the library exports all of them).
EXPORTS = [
    "pbx_config_default", "pbx_init", "pbx_shutdown", "pbx_last_error", "pbx_abi_version",
    "pbx_device_count", "pbx_plane_register", "pbx_plane_release", "pbx_plane_read_be",
    "pbx_get_tile", "pbx_get_tiles", "pbx_results_release", "pbx_batch_plan",
    "pbx_batch_launch", "pbx_batch_sync", "pbx_batch_fetch", "pbx_batch_destroy",
    "pbx_batch_stats_get", "pbx_tile_filename", "pbx_content_type", "pbx_format_from_string",
    "pbx_pixel_type_from_string", "pbx_bytes_per_pixel", "pbx_device_synchronize",
    "pbx_abi_sizes", "pbx_shard_of", "pbx_test_huffman", "pbx_ctx_stats_get",
    "pbx_test_batch_lz77", "pbx_submit", "pbx_wait", "pbx_plane_build_pyramid",
    "pbx_plane_register_zarr", "pbx_planes_register_zarr", "pbx_release_cached",
    "pbx_set_kernel_streams", "pbx_image_declare", "pbx_image_release", "pbx_plane_create",
    "pbx_plane_write_rows", "pbx_plane_commit", "pbx_plane_lookup", "pbx_set_residency_budget",
    "pbx_residency_stats_get", "pbx_test_fail_batch", "pbx_node_init", "pbx_node_shutdown",
    "pbx_node_size", "pbx_node_context", "pbx_node_route", "pbx_node_get_tile",
    "pbx_plane_create_sparse", "pbx_band_write", "pbx_plane_band_info", "pbx_result_spans",
    "pbx_test_stall_batch", "pbx_band_abort", "pbx_test_fail_band_write",
    "pbx_set_deflate_strategy", "pbx_get_deflate_strategy", "pbx_batch_lz_modes",
    "pbx_set_tiff_predictor", "pbx_get_tiff_predictor", "pbx_batch_pred_tiles",
    "pbx_band_write_zarr", "pbx_planes_register_zarr_deep", "pbx_band_write_zarr_deep",
    "pbx_test_zarr_plan", "pbx_planes_register_tiff", "pbx_test_tiff_plan",
    "pbx_band_write_tiff", "pbx_test_tiff_band_plan", "pbx_planes_register_tiff_samples",
    "pbx_band_write_tiff_sample", "pbx_test_tiff_plan_samples", "pbx_planes_register_tiff_jpeg",
    "pbx_band_write_tiff_jpeg", "pbx_test_tiff_jpeg_plan", "pbx_planes_register_tiff_j2k",
    "pbx_band_write_tiff_j2k", "pbx_test_tiff_j2k_plan", "pbx_test_tiff_j2k_decode",
    "pbx_planes_register_tiff_packed", "pbx_band_write_tiff_packed", "pbx_test_tiff_packed_plan",
    "pbx_band_write_tiff_group", "pbx_band_write_zarr_group", "pbx_test_band_group_admit",
    "pbx_band_write_reduced", "pbx_test_reduce_plan",
]

_lib = None


def lib() -> ctypes.CDLL:
    """Load lib/libpbx.so (build it with `make -C omero-ms-pixel-buffer_amd`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"pbx: native library missing at {LIB_PATH}; run "
                           "`python -c 'import __graft_entry__ as g; g.build()'`")
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
    L.pbx_last_error.restype = ctypes.c_char_p
    L.pbx_content_type.restype = ctypes.c_char_p
    L.pbx_content_type.argtypes = [ctypes.c_char_p]
    L.pbx_format_from_string.argtypes = [ctypes.c_char_p]
    L.pbx_pixel_type_from_string.argtypes = [ctypes.c_char_p]
    L.pbx_bytes_per_pixel.argtypes = [i32]
    L.pbx_config_default.argtypes = [ctypes.POINTER(PbxConfig)]
    L.pbx_init.argtypes = [ctypes.POINTER(PbxConfig), ctypes.POINTER(vp)]
    L.pbx_shutdown.argtypes = [vp]
    L.pbx_shutdown.restype = None
    L.pbx_device_synchronize.argtypes = [vp]
    L.pbx_set_kernel_streams.argtypes = [vp, i32, i32]
    L.pbx_release_cached.argtypes = [vp]
    L.pbx_set_deflate_strategy.argtypes = [vp, i32]
    L.pbx_get_deflate_strategy.argtypes = [vp, ctypes.POINTER(i32)]
    L.pbx_set_tiff_predictor.argtypes = [vp, i32]
    L.pbx_get_tiff_predictor.argtypes = [vp, ctypes.POINTER(i32)]
    L.pbx_batch_pred_tiles.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    L.pbx_batch_lz_modes.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.pbx_plane_register.argtypes = [vp, ctypes.POINTER(PbxPlaneDesc), ctypes.POINTER(u64)]
    L.pbx_plane_release.argtypes = [vp, u64]
    L.pbx_image_declare.argtypes = [vp, ctypes.POINTER(PbxImageDesc)]
    L.pbx_image_release.argtypes = [vp, ctypes.c_int64]
    L.pbx_plane_create.argtypes = [vp, ctypes.POINTER(PbxPlaneDesc), i32, i32, ctypes.POINTER(u64)]
    L.pbx_plane_write_rows.argtypes = [vp, u64, i32, i32, vp, u64]
    L.pbx_plane_commit.argtypes = [vp, u64]
    L.pbx_plane_lookup.argtypes = [vp, ctypes.c_int64, i32, i32, i32, i32, ctypes.POINTER(u64),
                                   ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.pbx_set_residency_budget.argtypes = [vp, u64]
    L.pbx_residency_stats_get.argtypes = [vp, ctypes.POINTER(PbxResidencyStats)]
    L.pbx_plane_read_be.argtypes = [vp, u64, vp, u64]
    L.pbx_plane_build_pyramid.argtypes = [vp, u64, i32, ctypes.POINTER(u64),
                                          ctypes.POINTER(ctypes.c_double)]
    L.pbx_plane_register_zarr.argtypes = [vp, ctypes.POINTER(PbxPlaneDesc),
                                          ctypes.POINTER(PbxZarrChunks), ctypes.POINTER(u64),
                                          ctypes.POINTER(ctypes.c_double)]
    L.pbx_planes_register_zarr.argtypes = [vp, u64, ctypes.POINTER(PbxPlaneDesc),
                                           ctypes.POINTER(PbxZarrChunks), ctypes.POINTER(u64),
                                           ctypes.POINTER(ctypes.c_double)]
    L.pbx_get_tile.argtypes = [vp, ctypes.POINTER(PbxTileReq), ctypes.POINTER(PbxResult)]
    L.pbx_test_batch_lz77.argtypes = [vp, vp, vp, vp, u64]
    L.pbx_ctx_stats_get.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.pbx_get_tiles.argtypes = [vp, ctypes.POINTER(PbxTileReq), u64, ctypes.POINTER(PbxResult)]
    L.pbx_submit.argtypes = [vp, ctypes.POINTER(PbxTileReq), u64, ctypes.POINTER(PbxResult),
                             ctypes.POINTER(vp)]
    L.pbx_wait.argtypes = [vp, vp, ctypes.c_int64]
    L.pbx_results_release.argtypes = [vp, ctypes.POINTER(PbxResult), u64]
    L.pbx_results_release.restype = None
    L.pbx_batch_plan.argtypes = [vp, ctypes.POINTER(PbxTileReq), u64, ctypes.POINTER(vp)]
    L.pbx_batch_launch.argtypes = [vp, vp]
    L.pbx_batch_sync.argtypes = [vp, vp]
    L.pbx_batch_fetch.argtypes = [vp, vp, ctypes.POINTER(PbxResult)]
    L.pbx_batch_destroy.argtypes = [vp, vp]
    L.pbx_batch_destroy.restype = None
    L.pbx_batch_stats_get.argtypes = [vp, vp, ctypes.POINTER(PbxBatchStats)]
    L.pbx_tile_filename.argtypes = [ctypes.POINTER(PbxTileReq), i32, i32, ctypes.c_char_p,
                                    ctypes.c_char_p, u64]
    L.pbx_abi_sizes.argtypes = [ctypes.POINTER(u64), ctypes.c_int]
    L.pbx_shard_of.argtypes = [ctypes.POINTER(PbxTileReq), i32, i32, i32]
    L.pbx_test_huffman.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 2 + [ctypes.c_uint32] + \
        [ctypes.c_void_p] * 2
    L.pbx_test_fail_batch.argtypes = [vp, u64]
    L.pbx_test_stall_batch.argtypes = [vp, u64]
    L.pbx_test_fail_band_write.argtypes = [vp, u64]
    L.pbx_plane_create_sparse.argtypes = [vp, ctypes.POINTER(PbxPlaneDesc), i32, i32, i32, ctypes.POINTER(u64)]
    L.pbx_band_write.argtypes = [vp, u64, i32, i32, vp, u64]
    L.pbx_band_write_zarr.argtypes = [vp, u64, i32, i32, ctypes.POINTER(PbxZarrChunks),
                                      ctypes.POINTER(ctypes.c_double)]
    L.pbx_planes_register_zarr_deep.argtypes = [vp, u64, ctypes.POINTER(PbxPlaneDesc),
                                                ctypes.POINTER(PbxZarrSlice), u64,
                                                ctypes.POINTER(PbxZarrChunks), ctypes.POINTER(i32),
                                                ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_double)]
    L.pbx_band_write_zarr_deep.argtypes = [vp, u64, i32, i32, ctypes.POINTER(PbxZarrChunks), i32, i32,
                                           ctypes.POINTER(ctypes.c_double)]
    L.pbx_test_zarr_plan.argtypes = [ctypes.POINTER(PbxZarrChunks), i32, i32, i32, i32,
                                     ctypes.POINTER(i32), i32, i32, i32, ctypes.POINTER(u64)]
    L.pbx_planes_register_tiff.argtypes = [vp, u64, ctypes.POINTER(PbxPlaneDesc),
                                           ctypes.POINTER(PbxTiffSegments), ctypes.POINTER(u64),
                                           ctypes.POINTER(ctypes.c_double)]
    L.pbx_test_tiff_plan.argtypes = [ctypes.POINTER(PbxTiffSegments), i32, i32, i32, ctypes.POINTER(u64)]
    L.pbx_band_write_tiff.argtypes = [vp, u64, i32, i32, ctypes.POINTER(PbxTiffSegments),
                                      ctypes.POINTER(ctypes.c_double)]
    L.pbx_test_tiff_band_plan.argtypes = [ctypes.POINTER(PbxTiffSegments), i32, i32, i32, i32, i32,
                                          ctypes.POINTER(u64)]
    L.pbx_planes_register_tiff_samples.argtypes = [vp, u64, ctypes.POINTER(PbxPlaneDesc),
                                                   ctypes.POINTER(PbxZarrSlice), u64,
                                                   ctypes.POINTER(PbxTiffSegments), ctypes.POINTER(i32),
                                                   ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_double)]
    L.pbx_band_write_tiff_sample.argtypes = [vp, u64, i32, i32, ctypes.POINTER(PbxTiffSegments), i32, i32,
                                             ctypes.POINTER(ctypes.c_double)]
    L.pbx_test_tiff_plan_samples.argtypes = [ctypes.POINTER(PbxTiffSegments), i32, i32, i32, i32, i32, i32,
                                             ctypes.POINTER(u64)]
    L.pbx_planes_register_tiff_jpeg.argtypes = [vp, u64, ctypes.POINTER(PbxPlaneDesc),
                                                ctypes.POINTER(PbxZarrSlice), u64,
                                                ctypes.POINTER(PbxTiffSegments), ctypes.POINTER(i32),
                                                ctypes.POINTER(PbxTiffJpeg), ctypes.POINTER(u64),
                                                ctypes.POINTER(ctypes.c_double)]
    L.pbx_band_write_tiff_jpeg.argtypes = [vp, u64, i32, i32, ctypes.POINTER(PbxTiffSegments), i32, i32,
                                           ctypes.POINTER(PbxTiffJpeg), ctypes.POINTER(ctypes.c_double)]
    L.pbx_test_tiff_jpeg_plan.argtypes = [ctypes.POINTER(PbxTiffSegments), ctypes.POINTER(PbxTiffJpeg), i32, i32,
                                          i32, i32, i32, ctypes.POINTER(u64)]
    L.pbx_planes_register_tiff_j2k.argtypes = [vp, u64, ctypes.POINTER(PbxPlaneDesc),
                                               ctypes.POINTER(PbxZarrSlice), u64,
                                               ctypes.POINTER(PbxTiffSegments), ctypes.POINTER(i32),
                                               ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_double)]
    L.pbx_band_write_tiff_j2k.argtypes = [vp, u64, i32, i32, ctypes.POINTER(PbxTiffSegments), i32, i32,
                                          ctypes.POINTER(ctypes.c_double)]
    L.pbx_test_tiff_j2k_plan.argtypes = [ctypes.POINTER(PbxTiffSegments), i32, i32, i32, i32, i32, i32,
                                         ctypes.POINTER(u64)]
    L.pbx_test_tiff_j2k_decode.argtypes = [ctypes.POINTER(PbxTiffSegments), i32, i32, i32, i32, vp, u64]
    L.pbx_planes_register_tiff_packed.argtypes = [vp, u64, ctypes.POINTER(PbxPlaneDesc),
                                                  ctypes.POINTER(PbxZarrSlice), u64,
                                                  ctypes.POINTER(PbxTiffSegments), ctypes.POINTER(PbxTiffPacked),
                                                  ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_double)]
    L.pbx_band_write_tiff_packed.argtypes = [vp, u64, i32, i32, ctypes.POINTER(PbxTiffSegments),
                                             ctypes.POINTER(PbxTiffPacked), ctypes.POINTER(ctypes.c_double)]
    L.pbx_test_tiff_packed_plan.argtypes = [ctypes.POINTER(PbxTiffSegments), ctypes.POINTER(PbxTiffPacked), i32, i32,
                                            i32, i32, i32, ctypes.POINTER(u64)]
    L.pbx_band_write_tiff_group.argtypes = [vp, ctypes.POINTER(u64), i32, i32, i32, i32,
                                            ctypes.POINTER(PbxTiffSegments), ctypes.POINTER(PbxTiffJpeg), i32,
                                            ctypes.POINTER(PbxTiffPacked), ctypes.POINTER(i32),
                                            ctypes.POINTER(ctypes.c_double)]
    L.pbx_band_write_zarr_group.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(i32), i32, i32, i32, i32,
                                            ctypes.POINTER(PbxZarrChunks), i32, ctypes.POINTER(i32),
                                            ctypes.POINTER(ctypes.c_double)]
    L.pbx_test_band_group_admit.argtypes = [ctypes.POINTER(i32), i32, i32, i32, ctypes.POINTER(i32)]
    L.pbx_band_write_reduced.argtypes = [vp, u64, i32, i32, u64, i32]
    L.pbx_test_reduce_plan.argtypes = [i32, i32, i32, i32, i32, i32, ctypes.POINTER(i32)]
    L.pbx_band_abort.argtypes = [vp, u64, i32]
    L.pbx_plane_band_info.argtypes = [vp, u64, ctypes.POINTER(i32), ctypes.POINTER(i32), vp]
    L.pbx_node_init.argtypes = [ctypes.POINTER(PbxConfig), i32, ctypes.POINTER(i32), i32, ctypes.POINTER(vp)]
    L.pbx_node_shutdown.argtypes = [vp]
    L.pbx_node_shutdown.restype = None
    L.pbx_node_size.argtypes = [vp]
    L.pbx_node_context.argtypes = [vp, i32]
    L.pbx_node_context.restype = vp
    L.pbx_node_route.argtypes = [vp, ctypes.POINTER(PbxTileReq), ctypes.POINTER(i32)]
    L.pbx_node_get_tile.argtypes = [vp, ctypes.POINTER(PbxTileReq), ctypes.POINTER(PbxResult),
                                    ctypes.POINTER(i32)]
    L.pbx_result_spans.argtypes = [ctypes.POINTER(PbxResult), ctypes.POINTER(PbxSpans)]
    _lib = L
    return L


class PbxError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"pbx status {status}: {msg}")
        self.status = status


def _check(status: int) -> None:
    if status != OK:
        raise PbxError(status, lib().pbx_last_error().decode(errors="replace"))


def device_count() -> int:
    return lib().pbx_device_count()


# ------------------------------------------------------------------------- TileCtx

def _parse_int(v: str, bits: int) -> int:
    """Java Integer.parseInt / Long.parseLong: optional sign, ASCII digits, in range."""
    if v is None:
        raise ValueError("null")  # parseInt(null) -> NumberFormatException
    s = v[1:] if v[:1] in ("+", "-") else v
    if not s or not s.isascii() or not s.isdigit():
        raise ValueError(f'For input string: "{v}"')
    n = int(v)
    if not -(1 << (bits - 1)) <= n < (1 << (bits - 1)):
        raise ValueError(f'For input string: "{v}"')
    return n


RESOLUTION_NONE = -1  # PBX_RESOLUTION_NONE: TileCtx.resolution == null


def _req_resolution(r: Optional[int]) -> int:
    """TileCtx.resolution -> pbx_tile_req.resolution (OMERO numbering, include/pbx.h): null ->
    PBX_RESOLUTION_NONE; a given negative level (setResolutionLevel throws -> 404) -> -2."""
    if r is None:
        return RESOLUTION_NONE
    return r if r >= 0 else -2


class TileCtx:
    """TileCtx.java:30-92 — the request context and the event-bus JSON payload."""

    def __init__(self, image_id: int, z: int, c: int, t: int, x: int = 0, y: int = 0,
                 w: int = 0, h: int = 0, resolution: Optional[int] = None,
                 format: Optional[str] = None, omero_session_key: Optional[str] = None):
        self.imageId = image_id
        self.z, self.c, self.t = z, c, t
        self.region = {"x": x, "y": y, "width": w, "height": h}
        self.resolution = resolution
        self.format = format
        self.omeroSessionKey = omero_session_key

    @classmethod
    def from_params(cls, params: Mapping[str, str], omero_session_key: Optional[str] = None):
        """TileCtx(MultiMap, String) (TileCtx.java:67-90); ValueError == NumberFormatException."""
        opt = lambda k: _parse_int(params[k], 32) if params.get(k) is not None else None
        return cls(_parse_int(params.get("imageId"), 64), _parse_int(params.get("z"), 32),
                   _parse_int(params.get("c"), 32), _parse_int(params.get("t"), 32),
                   opt("x") or 0, opt("y") or 0, opt("w") or 0, opt("h") or 0,
                   opt("resolution"), params.get("format"), omero_session_key)

    def to_json(self) -> str:
        return json.dumps({"omeroSessionKey": self.omeroSessionKey, "imageId": self.imageId,
                           "z": self.z, "c": self.c, "t": self.t,
                           "resolution": self.resolution, "region": self.region,
                           "format": self.format})

    @classmethod
    def from_json(cls, body: str) -> "TileCtx":
        d = json.loads(body)
        r = d.get("region") or {}
        for k in ("imageId", "z", "c", "t"):
            if not isinstance(d.get(k), int):
                raise ValueError(f"bad {k}")
        return cls(d["imageId"], d["z"], d["c"], d["t"], r.get("x", 0), r.get("y", 0),
                   r.get("width", 0), r.get("height", 0), d.get("resolution"),
                   d.get("format"), d.get("omeroSessionKey"))

    @property
    def x(self): return self.region["x"]

    @property
    def y(self): return self.region["y"]

    @property
    def w(self): return self.region["width"]

    @property
    def h(self): return self.region["height"]

    def to_req(self) -> PbxTileReq:
        return PbxTileReq(self.imageId, self.z, self.c, self.t,
                          _req_resolution(self.resolution),
                          self.x, self.y, self.w, self.h,
                          lib().pbx_format_from_string(
                              self.format.encode() if self.format is not None else None), 0)


def tile_filename(ctx: TileCtx) -> str:
    """PixelBufferVerticle.java:118-126 (uses the region after w/h defaulting)."""
    buf = ctypes.create_string_buffer(512)
    req = ctx.to_req()
    lib().pbx_tile_filename(ctypes.byref(req), ctx.w, ctx.h,
                            ctx.format.encode() if ctx.format is not None else None, buf, 512)
    return buf.value.decode()


def shard_of(ctx: TileCtx, world: int, tile_w: int = 512, tile_h: int = 512) -> int:
    """Rank that serves this request when requests are sharded over `world` GPUs."""
    req = ctx.to_req()
    r = lib().pbx_shard_of(ctypes.byref(req), tile_w, tile_h, world)
    if r < 0:
        _check(E_BADARG)
    return r


def band_rows(n_rows: int, world: int, rank: int) -> Tuple[int, int]:
    """Whole-slide split: contiguous tile-row band [lo, hi) of a rank."""
    return (n_rows * rank) // world, (n_rows * (rank + 1)) // world


def content_type(fmt: Optional[str]) -> str:
    """PixelBufferMicroserviceVerticle.java:373-379."""
    return lib().pbx_content_type(fmt.encode() if fmt is not None else None).decode()


# --------------------------------------------------------------------- PixelsService

def zarr_array_meta(array_dir: str) -> dict:
    """The .zarray of a Zarr v2 array directory, checked for what the GPU decode supports."""
    import json
    with open(os.path.join(array_dir, ".zarray")) as f:
        meta = json.load(f)
    if meta.get("zarr_format") != 2 or meta.get("order", "C") != "C" or meta.get("filters"):
        raise PbxError(400, "only Zarr v2 C-order arrays without filters are supported")
    if meta["dtype"][1:] not in _ZARR_DTYPES:
        raise PbxError(400, "unsupported dtype %s" % meta["dtype"])
    if len(meta["shape"]) < 2 or len(meta["shape"]) > 5 or len(meta["chunks"]) != len(meta["shape"]) or \
            any(not isinstance(cs, int) or cs < 1 for cs in meta["chunks"]):
        raise PbxError(400, "need shape [..., y, x] and chunks of the same rank")
    return meta


_ZARR3_DTYPES = {"int8": "i1", "uint8": "u1", "int16": "i2", "uint16": "u2", "int32": "i4",
                 "uint32": "u4", "float32": "f4", "float64": "f8"}
_CRC32C_TABLE: List[int] = []


def crc32c(data: bytes, crc: int = 0) -> int:
    """CRC-32C (Castagnoli, reflected 0x82F63B78) of data, table driven: what the Zarr v3 crc32c
    codec appends, little-endian.  Used on the host for shard indexes only; chunk checksums are
    checked on the GPU."""
    if not _CRC32C_TABLE:
        for n in range(256):
            c = n
            for _ in range(8):
                c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
            _CRC32C_TABLE.append(c)
    t, c = _CRC32C_TABLE, crc ^ 0xFFFFFFFF
    for b in data:
        c = t[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def _v3_codec(c) -> Tuple[str, dict]:
    if not isinstance(c, dict) or not isinstance(c.get("name"), str):
        raise PbxError(400, "bad codec entry %r" % (c,))
    return c["name"], c.get("configuration") or {}


def _v3_chunk_codecs(codecs, itemsize: int, what: str) -> Tuple[str, Optional[str], bool]:
    """(byte order '<' / '>' / '|', compressor name or None, crc32c?) of a v3 chunk pipeline:
    bytes, then at most one of blosc / gzip / zstd, then optionally crc32c."""
    if not isinstance(codecs, list) or not codecs:
        raise PbxError(400, "%s: no codecs" % what)
    name, cfg = _v3_codec(codecs[0])
    if name != "bytes":
        raise PbxError(400, "%s: codec %r where \"bytes\" must come first" % (what, name))
    endian = cfg.get("endian")
    if endian not in ("little", "big") and not (endian is None and itemsize == 1):
        raise PbxError(400, "%s: bytes codec endian %r" % (what, endian))
    order = "|" if itemsize == 1 else "<" if endian == "little" else ">"
    rest = [_v3_codec(c)[0] for c in codecs[1:]]
    crc = bool(rest) and rest[-1] == "crc32c"
    if crc:
        rest = rest[:-1]
    if len(rest) > 1 or (rest and rest[0] not in ("blosc", "gzip", "zstd")):
        raise PbxError(400, "%s: unsupported codecs %r (bytes, then one of blosc / gzip / zstd, then "
                            "crc32c)" % (what, [_v3_codec(c)[0] for c in codecs]))
    return order, (rest[0] if rest else None), crc


def _v3_fill_bits(fv, dt: str) -> int:
    """A v3 fill_value (a number, "NaN", "Infinity", "-Infinity" or a "0x..." bit pattern) as
    the sample's bit pattern."""
    import numpy as np
    native = np.dtype("=" + dt)
    if isinstance(fv, str):
        if fv[:2] in ("0x", "0X"):
            try:
                bits = int(fv, 16)
            except ValueError:
                raise PbxError(400, "fill_value %r" % (fv,))
            if bits >> (8 * native.itemsize):
                raise PbxError(400, "fill_value %r wider than the data type" % (fv,))
            return bits
        if fv not in ("NaN", "Infinity", "-Infinity") or native.kind != "f":
            raise PbxError(400, "fill_value %r" % (fv,))
        fv = float({"NaN": "nan", "Infinity": "inf", "-Infinity": "-inf"}[fv])
    elif isinstance(fv, bool) or not isinstance(fv, (int, float)):
        raise PbxError(400, "fill_value %r" % (fv,))
    try:
        if native.kind != "f" and (fv != int(fv) or not np.iinfo(native).min <= fv <= np.iinfo(native).max):
            raise ValueError
        return int(np.array([fv], dtype=native).view("u%d" % native.itemsize)[0])
    except (ValueError, OverflowError):
        raise PbxError(400, "fill_value %r outside %s" % (fv, native.name))


def zarr3_array_meta(array_dir: str) -> dict:
    """The zarr.json of a Zarr v3 array directory (NGFF 0.5), checked for what the GPU decode
    supports and brought to the keys the v2 code works on: shape, chunks (of a sharded array: the
    INNER chunk shape, which is the chunk grid the C-ABI sees), dtype (v2 spelling, byte order
    from the bytes codec), compressor ({"id": "blosc" / "gzip" / "zstd"} or None), plus
    zarr_format = 3, fill_bits, crc32c (the chunks end in the crc32c codec's checksum),
    key_encoding (prefix, separator) and shard (None, or the shard shape, the index location and
    whether the index carries a crc32c).  Anything else answers PbxError(400)."""
    with open(os.path.join(array_dir, "zarr.json")) as f:
        doc = json.load(f)
    if not isinstance(doc, dict) or doc.get("zarr_format") != 3 or doc.get("node_type") != "array":
        raise PbxError(400, "zarr.json is not a Zarr v3 array")
    dt = _ZARR3_DTYPES.get(doc.get("data_type")) if isinstance(doc.get("data_type"), str) else None
    if dt is None:
        raise PbxError(400, "unsupported data_type %r" % (doc.get("data_type"),))
    itemsize = int(dt[1:])
    shape = doc.get("shape")
    grid = doc.get("chunk_grid") or {}
    if grid.get("name") != "regular":
        raise PbxError(400, "unsupported chunk_grid %r" % (grid.get("name"),))
    outer = (grid.get("configuration") or {}).get("chunk_shape")
    ok_shape = lambda v: isinstance(v, list) and all(isinstance(n, int) and not isinstance(n, bool) for n in v)
    if not ok_shape(shape) or not ok_shape(outer) or not 2 <= len(shape) <= 5 or len(outer) != len(shape) or \
            any(n < 1 for n in outer) or any(n < 0 for n in shape):
        raise PbxError(400, "need shape [..., y, x] and a chunk_shape of the same rank")
    enc = doc.get("chunk_key_encoding") or {}
    ecfg = enc.get("configuration") or {}
    if enc.get("name") == "default":
        key = ("c", ecfg.get("separator", "/"))
    elif enc.get("name") == "v2":
        key = ("", ecfg.get("separator", "."))
    else:
        raise PbxError(400, "unsupported chunk_key_encoding %r" % (enc.get("name"),))
    if key[1] not in ("/", "."):
        raise PbxError(400, "chunk key separator %r" % (key[1],))
    if doc.get("storage_transformers"):
        raise PbxError(400, "storage_transformers are not supported")
    codecs = doc.get("codecs")
    shard, chunks = None, outer
    if isinstance(codecs, list) and any(isinstance(c, dict) and c.get("name") == "sharding_indexed" for c in codecs):
        if len(codecs) != 1:
            raise PbxError(400, "sharding_indexed must be the array's only codec")
        cfg = _v3_codec(codecs[0])[1]
        chunks = cfg.get("chunk_shape")
        if not ok_shape(chunks) or len(chunks) != len(outer) or any(n < 1 for n in chunks) or \
                any(o % n for o, n in zip(outer, chunks)):
            raise PbxError(400, "inner chunk_shape %r does not divide the shard shape %r" % (chunks, outer))
        loc = cfg.get("index_location", "end")
        if loc not in ("end", "start"):
            raise PbxError(400, "index_location %r" % (loc,))
        iorder, icomp, icrc = _v3_chunk_codecs(cfg.get("index_codecs"), 8, "index_codecs")
        if iorder != "<" or icomp is not None:
            raise PbxError(400, "index_codecs must be little-endian bytes, optionally crc32c")
        shard = dict(shape=list(outer), index_location=loc, index_crc32c=icrc)
        codecs = cfg.get("codecs")
    order, comp, crc = _v3_chunk_codecs(codecs, itemsize, "codecs")
    if "fill_value" not in doc:
        raise PbxError(400, "no fill_value")
    return dict(zarr_format=3, shape=list(shape), chunks=list(chunks), dtype=order + dt,
                compressor=None if comp is None else {"id": comp}, fill_bits=_v3_fill_bits(doc["fill_value"], dt),
                fill_value=doc["fill_value"], crc32c=crc, key_encoding=key, shard=shard,
                attributes=doc.get("attributes") or {})


def _array_meta(array_dir: str) -> dict:
    """The array's metadata: .zarray (v2) when the directory has one, else zarr.json (v3)."""
    if not os.path.exists(os.path.join(array_dir, ".zarray")) and \
            os.path.exists(os.path.join(array_dir, "zarr.json")):
        return zarr3_array_meta(array_dir)
    return zarr_array_meta(array_dir)


def _chunk_key(meta: dict, idx: Sequence[int]) -> str:
    """The store key of the chunk (of a sharded array: the shard) with grid indices idx."""
    if meta.get("zarr_format") == 3:
        prefix, sep = meta["key_encoding"]
        return sep.join(([prefix] if prefix else []) + [str(v) for v in idx])
    return meta.get("dimension_separator", ".").join(str(v) for v in idx)


def _shard_index(data: bytes, n: int, location: str, has_crc: bool, path: str) -> List[Optional[Tuple[int, int]]]:
    """The (offset, nbytes) of the n inner chunks of a shard file (None = missing), C order over
    the shard's inner-chunk grid: n pairs of uint64 LE at the end or the start of the file,
    followed by their crc32c when the index codecs say so.  Every range must lie inside the file
    and outside the index."""
    size = 16 * n + (4 if has_crc else 0)
    if len(data) < size:
        raise PbxError(400, "shard %s: %d bytes, shorter than its index" % (path, len(data)))
    lo = 0 if location == "start" else len(data) - size
    raw = data[lo:lo + size]
    if has_crc and crc32c(raw[:-4]) != int.from_bytes(raw[-4:], "little"):
        raise PbxError(400, "shard %s: index checksum mismatch" % path)
    out: List[Optional[Tuple[int, int]]] = []
    none = (1 << 64) - 1
    for k in range(n):
        off = int.from_bytes(raw[16 * k:16 * k + 8], "little")
        nb = int.from_bytes(raw[16 * k + 8:16 * k + 16], "little")
        if off == none and nb == none:
            out.append(None)
            continue
        if off + nb > len(data) or (off < lo + size and lo < off + nb):
            raise PbxError(400, "shard %s: inner chunk %d (%d + %d) outside the file or inside its index"
                           % (path, k, off, nb))
        out.append((off, nb))
    return out


def _read_chunk(array_dir: str, meta: dict, idx: Sequence[int], shards: dict) -> Optional[bytes]:
    """The bytes of the chunk with grid indices idx (None = absent).  For a sharded array idx
    counts inner chunks; `shards` keeps every shard file opened by this call (its bytes and
    parsed index), so each is read once."""
    sh = meta.get("shard")
    if not sh:
        return _read_chunk_file(os.path.join(array_dir, _chunk_key(meta, idx)))
    per = [o // c for o, c in zip(sh["shape"], meta["chunks"])]
    sidx = tuple(v // p for v, p in zip(idx, per))
    ent = shards.get(sidx)
    if ent is None:
        path = os.path.join(array_dir, _chunk_key(meta, sidx))
        data = _read_chunk_file(path)
        n = 1
        for p_ in per:
            n *= p_
        ent = shards[sidx] = (data, None if data is None else
                              _shard_index(data, n, sh["index_location"], sh["index_crc32c"], path))
    data, index = ent
    if data is None:
        return None
    k = 0
    for v, p_ in zip(idx, per):
        k = k * p_ + v % p_
    if index[k] is None:
        return None
    return data[index[k][0]:index[k][0] + index[k][1]]


def _lead_axes(ndim: int, axes: Optional[Sequence[str]]) -> List[str]:
    """Names of the leading (non-y/x) axes of an array: the NGFF multiscales "axes" when given
    (0.4: time, then channel, then space), else t, c, z with missing ones dropped from the left."""
    if axes is not None:
        names = [a["name"] if isinstance(a, dict) else a for a in axes]
        if len(names) != ndim or [n.lower() for n in names[-2:]] != ["y", "x"]:
            raise PbxError(400, "axes %r do not end in y, x" % (names,))
        lead = [n.lower() for n in names[:-2]]
        if any(n not in ("t", "c", "z") for n in lead) or len(set(lead)) != len(lead):
            raise PbxError(400, "unsupported axes %r" % (names,))
        return lead
    return ["t", "c", "z"][3 - (ndim - 2):]


def _read_chunk_file(path: str) -> Optional[bytes]:
    """A chunk file's bytes, or None when the file is absent (the chunk reads as fill_value)."""
    try:
        with open(path, "rb") as f:
            return f.read()
    except FileNotFoundError:
        return None


def _zarr_chunk_rows(array_dir: str, z: int, c: int, t: int, meta: Optional[dict],
                     axes: Optional[Sequence], y0: Optional[int] = None, rows: int = 0,
                     cache: Optional[dict] = None) -> dict:
    """What zarr_plane_spec and zarr_band_spec share: the array's geometry, codec, byte order
    and fill, and the chunk files (full width, C order) of the chunk rows covering plane rows
    [y0, y0 + rows) of plane (z, c, t), or of every chunk row (y0 None).  Chunks that hold
    more than one plane (a leading chunk extent above 1) add chunk_planes, the plane's slice of
    every chunk, and layer = what names the chunk files (planes of one layer share them); with
    `cache` (a dict the caller keeps for one registration) a layer's files are read once."""
    import numpy as np
    meta = meta or _array_meta(array_dir)
    shape, chunk, dt = meta["shape"], meta["chunks"], meta["dtype"]
    comp = meta.get("compressor")
    names = _lead_axes(len(shape), axes)
    want = {"t": t, "c": c, "z": z}
    lead = [want[n] for n in names]
    if any(want[n] for n in ("t", "c", "z") if n not in names):
        raise PbxError(404, "plane (z=%d, c=%d, t=%d) outside the array" % (z, c, t))
    for v, n in zip(lead, shape[:-2]):
        if not 0 <= v < n:
            raise PbxError(404, "plane (z=%d, c=%d, t=%d) outside the array" % (z, c, t))
    sy, sx, cy, cx = shape[-2], shape[-1], chunk[-2], chunk[-1]
    if y0 is None:
        y0, rows = 0, sy
    elif rows < 0 or y0 < 0 or y0 + rows > sy:
        raise PbxError(400, "rows %d+%d outside the array (%d rows)" % (y0, rows, sy))
    depth, slc = 1, 0
    for v, e in zip(lead, chunk[:-2]):
        depth, slc = depth * e, slc * e + v % e
    clead = [v // e for v, e in zip(lead, chunk[:-2])]
    layer = (array_dir, tuple(clead), y0, rows)
    chunks = cache.get(layer) if cache is not None else None
    if chunks is None:
        chunks, shards = [], {}  # (shard files of a sharded v3 array: each opened once)
        for j in range(y0 // cy, -(-(y0 + rows) // cy)):
            for i in range(-(-sx // cx)):
                chunks.append(_read_chunk(array_dir, meta, clead + [j, i], shards))
        if cache is not None:
            cache[layer] = chunks
    deep = dict(chunk_planes=depth, slice=slc, layer=layer) if depth > 1 else {}
    if "fill_bits" in meta:  # v3: worked out with the metadata
        fill_bits = meta["fill_bits"]
    else:
        native = np.dtype(dt).newbyteorder("=")
        fill_bits = int(np.array([meta.get("fill_value") or 0], dtype=native).view("u%d" % native.itemsize)[0])
    if meta.get("crc32c"):
        deep["crc32c"] = True
    return dict(pixel_type=_ZARR_DTYPES[dt[1:]], size_x=sx, size_y=sy, chunk_x=cx, chunk_y=cy,
                codec=None if comp is None else comp.get("id"), chunks=chunks,
                big_endian=dt[0] != "<", fill_bits=fill_bits, **deep)


def zarr_plane_spec(array_dir: str, image_id: int, z: int, c: int, t: int, level: int = 0,
                    meta: Optional[dict] = None, axes: Optional[Sequence] = None,
                    cache: Optional[dict] = None) -> dict:
    """register_zarr_planes() arguments for plane (z, c, t) of an NGFF array directory (axes:
    the multiscales "axes" of the image, else NGFF order t, c, z, y, x with fewer leading axes
    dropped from the left): chunk files named by dimension_separator "." or "/", absent
    files = fill_value.  `level` is the stored pyramid level (0 = full resolution).  For
    chunks that hold several planes the spec also has chunk_planes, slice and layer; `cache`
    (one dict for all the specs of a registration) has the planes of a layer share its files."""
    return dict(_zarr_chunk_rows(array_dir, z, c, t, meta, axes, cache=cache), image_id=image_id, z=z,
                c=c, t=t, level=level)


def zarr_band_spec(array_dir: str, z: int, c: int, t: int, y0: int, rows: int,
                   meta: Optional[dict] = None, axes: Optional[Sequence] = None) -> dict:
    """band_write_zarr() arguments for rows [y0, y0 + rows) of plane (z, c, t) of an NGFF array
    directory: only the files of the chunk rows that cover them are read (paths, axes and
    absent files as in zarr_plane_spec).  rows == 0 reads no file: the array's geometry, codec
    and byte order alone.  Chunks that hold several planes add chunk_planes and slice."""
    return dict(_zarr_chunk_rows(array_dir, z, c, t, meta, axes, y0, rows), y0=y0, rows=rows)


def pack_chunks(chunks: Sequence[Optional[bytes]]):
    """Chunk files of one plane as the C-ABI takes them: (uint8 data, uint64 offsets[n+1]),
    the files concatenated in C order over the chunk grid (None / b"" = missing chunk)."""
    import numpy as np
    lens = np.array([len(b) if b else 0 for b in chunks], dtype=np.uint64)
    offsets = np.zeros(len(chunks) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    data = np.frombuffer(b"".join(b for b in chunks if b) or b"\0", dtype=np.uint8)
    return data, offsets


# ----------------------------------------------------------------- TIFF / OME-TIFF files
# The reference's pixels service falls back from NGFF to the Bio-Formats pixel buffers over the
# original files (config.yaml:18), which for most installations are TIFF and OME-TIFF.  This is a
# dependency-free reader of the container (classic TIFF and BigTIFF, II and MM); every byte of
# pixel data is decoded on the GPU (pbx_planes_register_tiff).

TIFF_NONE, TIFF_LZW, TIFF_DEFLATE = 1, 5, 8  # enum pbx_tiff_compression
TIFF_ZSTD = 50000
TIFF_JPEG = 7  # through the pbx_*_tiff_jpeg calls only
TIFF_PACKBITS = 32773  # through the pbx_*_tiff_packed calls only
TIFF_F_J2K_PACKETS = 1  # pbx_tiff_segments.flags: JPEG 2000 layers, precincts, SOP / EPH (the pbx_*_tiff_j2k calls only)
TIFF_F_J2K_SUBSAMPLED = 4  # components 1 and 2 at half width and / or half height (the same calls only)
TIFF_F_J2K_YCBCR = 8  # YCbCr components outside the codestream: converted to RGB (the same calls only)
TIFF_J2K = 34712  # through the pbx_*_tiff_j2k calls only; what every Compression value below hands over as
_TIFF_J2K_COMPRESSIONS = (33003, 33004, 33005, 34712)  # Bio-Formats' TiffCompression: JPEG-2000 / Lossy, Aperio's two
_TIFF_TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 13: 4,
                   16: 8, 17: 8, 18: 8}
_TIFF_INT_FMT = {1: "B", 3: "H", 4: "I", 13: "I", 16: "Q", 18: "Q", 6: "b", 8: "h", 9: "i", 17: "q"}
_TIFF_TAGS = {256: "width", 257: "length", 258: "bits", 259: "compression", 262: "photometric",
              266: "fillorder", 270: "description", 273: "strip_offsets", 274: "orientation", 277: "spp",
              278: "rows_per_strip", 279: "strip_counts", 284: "planar", 317: "predictor", 322: "tile_w",
              323: "tile_h", 324: "tile_offsets", 325: "tile_counts", 330: "subifd_offsets",
              338: "extrasamples", 339: "sampleformat", 347: "jpeg_tables", 530: "ycbcr_subsampling"}
_TIFF_MAX_IFDS = 1 << 16
_TIFF_PIXEL_TYPES = {(1, 8): UINT8, (2, 8): INT8, (1, 16): UINT16, (2, 16): INT16, (1, 32): UINT32,
                     (2, 32): INT32, (3, 32): FLOAT, (3, 64): DOUBLE}


def tiff_ifds(path: str) -> List[dict]:
    """The IFD chain of a classic TIFF or BigTIFF file (II or MM), SubIFDs (tag 330) included,
    without any pixel data.  One dict per main IFD: width, length, bits (BitsPerSample),
    sampleformat, spp (SamplesPerPixel), bits_count / sampleformat_count (how many values those
    two tags hold; 1 if absent), planar (PlanarConfiguration, default 1), photometric (None if
    absent), extrasamples (a list), jpeg_tables (tag 347's bytes or None), ycbcr_subsampling (tag
    530's two values or None), compression, predictor, fillorder, orientation, tiled,
    seg_w x seg_h (TileWidth x TileLength, or ImageWidth x RowsPerStrip capped at the length),
    offsets / counts of the segments, description (ImageDescription or None), byteorder ("<" or
    ">"), bigtiff, subifds (such dicts).  Every offset and count is checked against the file
    size and IFD loops are refused: PbxError 400."""
    import struct
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        def read(off: int, n: int, what: str) -> bytes:
            if off < 0 or n < 0 or off + n > size:
                raise PbxError(400, "%s: %s at offset %d (%d bytes) lies past the end of the file (%d bytes)"
                               % (path, what, off, n, size))
            f.seek(off)
            return f.read(n)

        head = read(0, 8, "header")
        if head[:2] not in (b"II", b"MM"):
            raise PbxError(400, "%s: not a TIFF file" % path)
        bo = "<" if head[:2] == b"II" else ">"
        magic = struct.unpack(bo + "H", head[2:4])[0]
        if magic == 42:
            big, first = False, struct.unpack(bo + "I", head[4:8])[0]
        elif magic == 43:
            h2 = read(0, 16, "BigTIFF header")
            osz, zero, first = struct.unpack(bo + "HHQ", h2[4:16])
            if osz != 8 or zero != 0:
                raise PbxError(400, "%s: bad BigTIFF header" % path)
            big = True
        else:
            raise PbxError(400, "%s: not a TIFF file (magic %d)" % (path, magic))
        cnt_fmt, cnt_sz, ent_sz, inline, off_fmt = ("Q", 8, 20, 8, "Q") if big else ("H", 2, 12, 4, "I")
        seen: set = set()

        def ifd_at(off: int):
            if off in seen:
                raise PbxError(400, "%s: IFD loop at offset %d" % (path, off))
            if len(seen) >= _TIFF_MAX_IFDS:
                raise PbxError(400, "%s: more than %d IFDs" % (path, _TIFF_MAX_IFDS))
            seen.add(off)
            n = struct.unpack(bo + cnt_fmt, read(off, cnt_sz, "IFD"))[0]
            if n > 4096:
                raise PbxError(400, "%s: IFD at offset %d with %d entries" % (path, off, n))
            body = read(off + cnt_sz, n * ent_sz + inline, "IFD entries")
            d: dict = {}
            for k in range(n):
                e = body[k * ent_sz:(k + 1) * ent_sz]
                tag, typ = struct.unpack(bo + "HH", e[:4])
                count = struct.unpack(bo + off_fmt, e[4:4 + inline])[0]
                name = _TIFF_TAGS.get(tag)
                if name is None:
                    continue
                tsz = _TIFF_TYPE_SIZE.get(typ)
                if tag == 347 and typ in (1, 7):  # JPEGTables: UNDEFINED (or BYTE) bytes, kept as they are
                    d[name] = e[4 + inline:4 + inline + count] if count <= inline else \
                        read(struct.unpack(bo + off_fmt, e[4 + inline:])[0], count, "the value of tag 347")
                    continue
                if tsz is None or (typ != 2 and typ not in _TIFF_INT_FMT):
                    raise PbxError(400, "%s: tag %d has field type %d" % (path, tag, typ))
                nbytes = tsz * count
                raw = e[4 + inline:4 + inline + nbytes] if nbytes <= inline else \
                    read(struct.unpack(bo + off_fmt, e[4 + inline:])[0], nbytes, "the value of tag %d" % tag)
                if typ == 2:
                    d[name] = raw.split(b"\0", 1)[0].decode("utf-8", errors="replace")
                else:
                    d[name] = list(struct.unpack(bo + _TIFF_INT_FMT[typ] * count, raw))
            nxt = struct.unpack(bo + off_fmt, body[n * ent_sz:])[0]
            return d, nxt

        def finish(d: dict) -> dict:
            def one(name, default=None):
                v = d.get(name)
                if v is None:
                    if default is None:
                        raise PbxError(400, "%s: an IFD lacks the %s tag" % (path, name))
                    return default
                if isinstance(v, list):
                    if not v:
                        raise PbxError(400, "%s: empty %s tag" % (path, name))
                    if any(x != v[0] for x in v):  # BitsPerSample / SampleFormat per sample
                        raise PbxError(400, "%s: samples differ in %s: %r" % (path, name, v))
                    return v[0]
                return v
            out = dict(width=one("width"), length=one("length"), bits=one("bits", 1),
                       sampleformat=one("sampleformat", 1), spp=one("spp", 1),
                       compression=one("compression", 1), predictor=one("predictor", 1),
                       fillorder=one("fillorder", 1), orientation=one("orientation", 1),
                       description=d.get("description"), byteorder=bo, bigtiff=big,
                       planar=one("planar", 1),
                       photometric=one("photometric") if "photometric" in d else None,
                       extrasamples=list(d.get("extrasamples", [])),
                       jpeg_tables=d.get("jpeg_tables"),
                       ycbcr_subsampling=list(d["ycbcr_subsampling"]) if "ycbcr_subsampling" in d else None,
                       bits_count=len(d["bits"]) if "bits" in d else 1,
                       sampleformat_count=len(d["sampleformat"]) if "sampleformat" in d else 1)
            if out["width"] < 1 or out["length"] < 1:
                raise PbxError(400, "%s: image of %d x %d" % (path, out["width"], out["length"]))
            if "tile_offsets" in d:
                out.update(tiled=True, seg_w=one("tile_w"), seg_h=one("tile_h"),
                           offsets=d["tile_offsets"], counts=d.get("tile_counts"))
            else:
                out.update(tiled=False, seg_w=out["width"],
                           seg_h=min(one("rows_per_strip", 0xFFFFFFFF), out["length"]),
                           offsets=d.get("strip_offsets"), counts=d.get("strip_counts"))
            if out["seg_w"] < 1 or out["seg_h"] < 1:
                raise PbxError(400, "%s: segments of %d x %d" % (path, out["seg_w"], out["seg_h"]))
            if out["offsets"] is None or out["counts"] is None or len(out["offsets"]) != len(out["counts"]):
                raise PbxError(400, "%s: an IFD lacks segment offsets or byte counts" % path)
            for o, c in zip(out["offsets"], out["counts"]):
                if o + c > size:
                    raise PbxError(400, "%s: a segment at offset %d (%d bytes) lies past the end of the file "
                                   "(%d bytes)" % (path, o, c, size))
            out["subifds"] = []
            for so in d.get("subifd_offsets", []):
                sd, _ = ifd_at(so)
                out["subifds"].append(finish(sd))
            return out

        ifds, off = [], first
        if off == 0:
            raise PbxError(400, "%s: no IFD" % path)
        while off:
            d, off = ifd_at(off)
            ifds.append(finish(d))
        return ifds


_JPEG_SOF_NAMES = {0xC1: "SOF1 (extended sequential)", 0xC2: "SOF2 (progressive)", 0xC3: "SOF3 (lossless)",
                   0xC5: "SOF5 (differential)", 0xC6: "SOF6 (differential progressive)",
                   0xC7: "SOF7 (differential lossless)", 0xC9: "SOF9 (arithmetic coding)",
                   0xCA: "SOF10 (progressive, arithmetic coding)", 0xCB: "SOF11 (lossless, arithmetic coding)",
                   0xCD: "SOF13 (arithmetic coding)", 0xCE: "SOF14 (arithmetic coding)",
                   0xCF: "SOF15 (arithmetic coding)"}


def jpeg_header(data: bytes, what: str) -> dict:
    """The marker segments of a JPEG stream up to its first SOS header (no entropy-coded byte is
    read): precision, height, width, components = [(id, h, v, tq)], scan_components, dqt = [(pq,
    tq)], dht = [(tc, th)], restart (DRI, 0 if none), sof (the SOFn code), data = the offset
    after the SOS header.  A tables-only stream (tag 347) ends at EOI: sof and data are None.
    PbxError 400 with `what` for a stream that does not start with SOI or is cut short."""
    n = len(data)
    if n < 2 or data[0] != 0xFF or data[1] != 0xD8:
        raise PbxError(400, "%s does not start with SOI" % what)
    out = dict(precision=None, height=None, width=None, components=[], scan_components=None, dqt=[], dht=[],
               restart=0, sof=None, data=None)
    q = 2
    while True:
        if q >= n or data[q] != 0xFF:
            raise PbxError(400, "%s: truncated header (no marker at byte %d)" % (what, q))
        while q < n and data[q] == 0xFF:
            q += 1
        if q >= n:
            raise PbxError(400, "%s: truncated header" % what)
        code = data[q]
        q += 1
        if code == 0xD9:
            return out
        if code in (0xD8, 0x01, 0x00) or 0xD0 <= code <= 0xD7:
            raise PbxError(400, "%s: marker FF %02X in the header" % (what, code))
        if q + 2 > n:
            raise PbxError(400, "%s: truncated header" % what)
        L = data[q] << 8 | data[q + 1]
        if L < 2 or q + L > n:
            raise PbxError(400, "%s: truncated header (marker FF %02X of %d bytes)" % (what, code, L))
        p = data[q + 2:q + L]
        q += L
        if code == 0xDB:
            k = 0
            while k < len(p):
                out["dqt"].append((p[k] >> 4, p[k] & 15))
                k += 65 + 64 * (p[k] >> 4)
        elif code == 0xC4:
            k = 0
            while k + 17 <= len(p):
                out["dht"].append((p[k] >> 4, p[k] & 15))
                k += 17 + sum(p[k + 1:k + 17])
        elif code == 0xDD and len(p) == 2:
            out["restart"] = p[0] << 8 | p[1]
        elif 0xC0 <= code <= 0xCF and code not in (0xC4, 0xC8, 0xCC):
            if len(p) >= 6 and p[5] == 4:
                raise PbxError(400, "%s: 4 components (CMYK / YCCK) are not supported" % what)
            if len(p) < 6 or len(p) != 6 + 3 * p[5]:
                raise PbxError(400, "%s: truncated SOF" % what)
            out.update(sof=code, precision=p[0], height=p[1] << 8 | p[2], width=p[3] << 8 | p[4],
                       components=[(p[6 + 3 * c], p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15, p[8 + 3 * c])
                                   for c in range(p[5])])
        elif code == 0xCC:
            out["sof"] = out["sof"] or 0xCC
        elif code == 0xDA:
            if not p or len(p) != 4 + 2 * p[0]:
                raise PbxError(400, "%s: truncated SOS" % what)
            out["scan_components"] = p[0]
            out["data"] = q
            return out


def _tiff_jpeg_first_segment(path: str, ifd: dict, spp: int) -> None:
    """What the IFD and the first segment's header show of a Compression-7 file this library cannot
    load: PbxError 400 with the reason (the C-ABI checks every segment again)."""
    what = "%s: Compression 7: " % path
    if ifd.get("jpeg_tables") is not None:
        jpeg_header(bytes(ifd["jpeg_tables"]), what + "JPEGTables")
    if not ifd["offsets"]:
        return
    with open(path, "rb") as f:
        f.seek(ifd["offsets"][0])
        data = f.read(ifd["counts"][0])  # the whole segment: APPn data may push the SOS anywhere in it
    h = jpeg_header(data, what + "segment 0")
    if h["sof"] is None:
        raise PbxError(400, what + "segment 0: no SOF before the scan")
    if h["sof"] != 0xC0:
        raise PbxError(400, what + "segment 0: %s is not supported (baseline SOF0 only)"
                       % ("arithmetic coding (DAC)" if h["sof"] == 0xCC else _JPEG_SOF_NAMES[h["sof"]]))
    if h["precision"] != 8:
        raise PbxError(400, what + "segment 0: sample precision %d (8 only)" % h["precision"])
    comps = h["components"]
    if len(comps) == 4:
        raise PbxError(400, what + "segment 0: 4 components (CMYK / YCCK) are not supported")
    if len(comps) != spp:
        raise PbxError(400, what + "segment 0: a stream of %d components in segments of %d samples per pixel"
                       % (len(comps), spp))
    if any(pq for pq, _ in h["dqt"]):
        raise PbxError(400, what + "segment 0: 16-bit quantiser (DQT with Pq = 1) is not supported")
    rows = ifd["seg_h"] if ifd["tiled"] else min(ifd["seg_h"], ifd["length"])
    if (h["width"], h["height"]) != (ifd["seg_w"], rows):
        raise PbxError(400, what + "segment 0: SOF size %d x %d != segment size %d x %d"
                       % (h["width"], h["height"], ifd["seg_w"], rows))
    samp = [(c[1], c[2]) for c in comps]
    if len(comps) == 1 and samp[0] != (1, 1):
        raise PbxError(400, what + "segment 0: sampling factors %dx%d on a one-component stream (1x1)" % samp[0])
    if len(comps) == 3:
        if samp[1:] != [(1, 1), (1, 1)] or samp[0] not in ((1, 1), (2, 1), (2, 2)):
            raise PbxError(400, what + "segment 0: sampling factors %s (luma 1x1, 2x1 or 2x2 with chroma 1x1)"
                           % ", ".join("%dx%d" % s for s in samp))
        if samp[0] != (1, 1) and ifd.get("photometric") != 6:
            raise PbxError(400, what + "segment 0: subsampling %dx%d without PhotometricInterpretation 6 (YCbCr)"
                           % samp[0])
    if h["scan_components"] is not None and h["scan_components"] != len(comps):
        raise PbxError(400, what + "segment 0: more than one scan (the first holds %d of %d components)"
                       % (h["scan_components"], len(comps)))


_J2K_UNSUPPORTED_MARKERS = {0x53: "COC", 0x5D: "QCC", 0x5E: "RGN", 0x5F: "POC", 0x60: "PPM", 0x61: "PPT", 0x63: "CRG"}


def j2k_header(data: bytes, what: str) -> dict:
    """The marker segments of a raw JPEG 2000 codestream up to SOD (no packet byte is read): width,
    height, offsets (XOsiz, YOsiz, XTOsiz, YTOsiz), tile (XTsiz, YTsiz), components = [(precision,
    signed, XRsiz, YRsiz)], scod, progression, layers, mct, levels, xcb, ycb (the code block's
    exponents), style, transformation (1: the reversible 5/3, 0: the irreversible 9/7), precincts =
    [(PPx, PPy)] per resolution (15, 15 if none are declared), qstyle, guard, qcd (the QCD's entries
    as bytes), exponents and mantissas (per entry: style 0 has 8-bit entries and no mantissas,
    styles 1 and 2 have 16-bit entries, style 1 only the LL band's; j2k_steps derives the rest), markers
    (the codes met, in order), tile_index, tile_part, tile_parts, psot, sot and data (the offset
    after SOD).  PbxError 400 with `what` for a JP2 file, a stream that does not start with SOC,
    or a header cut short."""
    import struct
    n = len(data)
    if data[:12] == b"\x00\x00\x00\x0cjP  \r\n\x87\n":
        raise PbxError(400, "%s: jp2 box, not a codestream" % what)
    if n < 2 or data[0] != 0xFF or data[1] != 0x4F:
        raise PbxError(400, "%s does not start with SOC (JPEG 2000 codestream)" % what)
    out = dict(markers=[], components=[], exponents=[], precincts=None, data=None, sot=None)
    q = 2
    while True:
        if q + 2 > n:
            raise PbxError(400, "%s: truncated header" % what)
        if data[q] != 0xFF:
            raise PbxError(400, "%s: truncated header (no marker at byte %d)" % (what, q))
        code = data[q + 1]
        if code == 0x93:
            out["data"] = q + 2
            return out
        if code in (0xD9, 0x4F, 0x91, 0x92) or 0x30 <= code <= 0x3F:
            raise PbxError(400, "%s: marker FF %02X in the header" % (what, code))
        if q + 4 > n:
            raise PbxError(400, "%s: truncated header" % what)
        L = data[q + 2] << 8 | data[q + 3]
        if L < 2 or q + 2 + L > n:
            raise PbxError(400, "%s: truncated header (marker FF %02X of %d bytes)" % (what, code, L))
        p = data[q + 4:q + 2 + L]
        out["markers"].append(code)
        if code == 0x51:
            if len(p) < 36 or len(p) != 36 + 3 * (p[34] << 8 | p[35]):
                raise PbxError(400, "%s: truncated SIZ" % what)
            xs, ys, xo, yo, xt, yt, xto, yto = struct.unpack(">8I", p[2:34])
            out.update(width=xs, height=ys, offsets=(xo, yo, xto, yto), tile=(xt, yt),
                       components=[((p[36 + 3 * c] & 127) + 1, p[36 + 3 * c] >> 7, p[37 + 3 * c], p[38 + 3 * c])
                                   for c in range(p[34] << 8 | p[35])])
        elif code == 0x52:
            if len(p) < 10 or len(p) != 10 + ((p[5] + 1) if p[0] & 1 else 0):
                raise PbxError(400, "%s: truncated COD" % what)
            out.update(scod=p[0], progression=p[1], layers=p[2] << 8 | p[3], mct=p[4], levels=p[5], xcb=p[6] + 2,
                       ycb=p[7] + 2, style=p[8], transformation=p[9],
                       precincts=[(b & 15, b >> 4) for b in p[10:]] if p[0] & 1 else [(15, 15)] * (p[5] + 1))
        elif code == 0x5C:
            if len(p) < 1:
                raise PbxError(400, "%s: truncated QCD" % what)
            out.update(qstyle=p[0] & 31, guard=p[0] >> 5, qcd=bytes(p[1:]))
            if out["qstyle"] in (1, 2):
                ent = [p[k] << 8 | p[k + 1] for k in range(1, len(p) - 1, 2)]
                out.update(exponents=[e >> 11 for e in ent], mantissas=[e & 2047 for e in ent])
            else:
                out.update(exponents=[b >> 3 for b in p[1:]], mantissas=[])
        elif code == 0x90:
            if len(p) != 8:
                raise PbxError(400, "%s: truncated SOT" % what)
            if out["sot"] is not None:
                raise PbxError(400, "%s: more than one tile-part" % what)
            out.update(sot=q, tile_index=p[0] << 8 | p[1], psot=struct.unpack(">I", p[2:6])[0], tile_part=p[6],
                       tile_parts=p[7])
        q += 2 + L


def j2k_steps(h: dict) -> list:
    """Per sub-band (QCD order) of an irreversible header (j2k_header's dict, its QCD length already
    checked) the pair (exponent, quantisation step): T.800 E.1.1, step = 2^(P + gain - exponent) *
    (1 + mantissa / 2048), the gain 0 for LL, 1 for HL and LH, 2 for HH; style 1 derives every band
    from the LL entry, its exponent lowered by the levels the band lies above the deepest."""
    prec, levels = h["components"][0][0], h["levels"]
    out = []
    for b in range(3 * levels + 1):
        if h["qstyle"] == 2:
            eps, mu = h["exponents"][b], h["mantissas"][b]
        else:
            eps, mu = h["exponents"][0] - ((b + 2) // 3 - 1 if b else 0), h["mantissas"][0]
        gain = 0 if b == 0 else 2 if (b - 1) % 3 == 2 else 1
        out.append((eps, 2.0 ** (prec + gain - eps) * (1 + mu / 2048.0)))
    return out


def _tiff_j2k_first_segment(path: str, ifd: dict, spp: int, bits: int, packets: bool = False,
                            chroma: bool = False, ycbcr: bool = False) -> bool:
    """What the first segment's header shows of a JPEG 2000 IFD this library cannot load: PbxError
    400 with the reason, in the C-ABI's words (which checks every segment again).  `packets`: the
    caller hands the segments over with TIFF_F_J2K_PACKETS, which takes 1 .. 64 quality layers, any
    precinct sizes and SOP / EPH markers.  `chroma`: with TIFF_F_J2K_SUBSAMPLED where the stream
    needs it, which takes three components whose second and third are 2 x 1, 1 x 2 or 2 x 2; the
    answer is whether it does.  `ycbcr`: with TIFF_F_J2K_YCBCR."""
    if not ifd["offsets"]:
        return False
    with open(path, "rb") as f:
        f.seek(ifd["offsets"][0])
        data = f.read(ifd["counts"][0])
    what = "%s: Compression %d: segment 0" % (path, ifd["compression"])
    h = j2k_header(data, what)

    def no(why):
        raise PbxError(400, "%s: %s" % (what, why))
    if not h["markers"] or h["markers"][0] != 0x51:
        no("marker FF %02X before SIZ" % h["markers"][0] if h["markers"] else "truncated header")
    for code in h["markers"]:
        if code in _J2K_UNSUPPORTED_MARKERS:
            no("%s markers are not supported" % _J2K_UNSUPPORTED_MARKERS[code])
        if code not in (0x51, 0x52, 0x5C, 0x90, 0x64, 0x55, 0x57, 0x58):
            no("marker FF %02X in the header" % code)
    if any(h["offsets"]):
        no("non-zero image or tile offsets (%d, %d; %d, %d)" % h["offsets"])
    if h["tile"][0] < h["width"] or h["tile"][1] < h["height"]:
        no("more than one tile (%d x %d in tiles of %d x %d)" % (h["width"], h["height"], h["tile"][0], h["tile"][1]))
    comps = h["components"]
    if len(comps) not in (1, 3):
        no("%d components (1 or 3)" % len(comps))
    for c, (prec, signed, xr, yr) in enumerate(comps):
        if (xr, yr) != (1, 1) and not chroma:
            no("subsampled components (component %d: %d x %d)" % (c, xr, yr))
        if (xr, yr) != (1, 1):
            if len(comps) == 1:
                no("subsampling on a stream of one component (%d x %d)" % (xr, yr))
            if c == 0:
                no("subsampled first component (%d x %d)" % (xr, yr))
            if (xr, yr) not in ((2, 1), (1, 2), (2, 2)):
                no("sampling factors %d x %d on component %d (2 x 1, 1 x 2 or 2 x 2)" % (xr, yr, c))
        if c == 2 and (xr, yr) != comps[1][2:]:
            no("chroma components of different sampling factors (%d x %d and %d x %d)" % (comps[1][2:] + (xr, yr)))
        if signed:
            no("signed components")
        if prec != comps[0][0]:
            no("components of different precisions")
    prec = comps[0][0]
    if prec not in (8, 16):
        no("precision %d (8 or 16)" % prec)
    if len(comps) == 3 and prec != 8:
        no("three components at precision 16")
    if "levels" not in h:
        no("no COD marker")
    if h["scod"] & 6 and not packets:
        no("SOP or EPH markers (Scod 0x%02x)" % h["scod"])
    if h["progression"] > 4:
        no("bad progression order %d" % h["progression"])
    if h["layers"] != 1 and not packets:
        no("%d quality layers (1)" % h["layers"])
    if not 1 <= h["layers"] <= 64:
        no("%d quality layers (1 .. 64)" % h["layers"])
    if h["levels"] > 32:
        no("%d decomposition levels (0 .. 32)" % h["levels"])
    if not (2 <= h["xcb"] <= 10 and 2 <= h["ycb"] <= 10 and h["xcb"] + h["ycb"] <= 12):
        no("bad code-block size 2^%d x 2^%d" % (h["xcb"], h["ycb"]))
    if h["style"]:
        no("code-block style 0x%02x (bypass, reset, termall, vertically causal, predictable termination and "
           "segmentation symbols are not supported)" % h["style"])
    if h["transformation"] > 1:
        no("bad wavelet transformation %d" % h["transformation"])
    if "qstyle" not in h:
        no("no QCD marker")
    if h["qstyle"] > 2:
        no("bad quantisation style %d" % h["qstyle"])
    irrev = h["transformation"] == 0
    if irrev and h["qstyle"] == 0:
        no("irreversible wavelet (9/7) with quantisation style 0 (no quantisation)")
    if not irrev and h["qstyle"]:
        no("quantisation style %d (scalar quantisation) with the reversible wavelet (5/3)" % h["qstyle"])
    nq = len(h["qcd"])
    if h["qstyle"] == 2 and nq & 1:
        no("QCD of %d bytes in 16-bit entries (style 2)" % nq)
    if h["qstyle"] == 1 and nq != 2:
        no("QCD of %d bytes for the one entry of style 1" % nq)
    nexp = 3 * h["levels"] + 1 if h["qstyle"] == 1 else len(h["exponents"])
    if nexp != 3 * h["levels"] + 1:
        no("QCD of %d sub-bands for %d decomposition levels" % (nexp, h["levels"]))
    if h["mct"] > 1 or (h["mct"] and len(comps) != 3):
        no("multiple-component transform on %d component(s)" % len(comps))
    sub = len(comps) == 3 and comps[1][2:] != (1, 1)
    if h["mct"] and sub:
        no("subsampled components (%d x %d) with the multiple-component transform" % comps[1][2:])
    if irrev:
        for b, (eps, _) in enumerate(j2k_steps(h)):
            if eps < 0:
                no("quantisation style 1 derives exponent %d for sub-band %d" % (eps, b))
            if h["guard"] + eps > 31:
                no("%d magnitude bit-planes on a 9/7 sub-band (at most 30)" % (h["guard"] + eps - 1))
    for eps in ([] if irrev else h["exponents"]):
        if h["guard"] + eps > 32:
            no("%d magnitude bit-planes (at most 31)" % (h["guard"] + eps - 1))
    for r, (ppx, ppy) in enumerate(h["precincts"]):
        sh = h["levels"] - r
        if r and (ppx == 0 or ppy == 0):
            no("precinct exponent 0 at resolution %d" % r)
        if not packets and (-(-h["width"] >> sh) > 1 << ppx or -(-h["height"] >> sh) > 1 << ppy):
            no("more than one precinct in resolution %d" % r)
    if h["tile_index"]:
        no("more than one tile (tile index %d)" % h["tile_index"])
    if h["tile_part"] or h["tile_parts"] > 1:
        no("more than one tile-part (%d of %d)" % (h["tile_part"], h["tile_parts"]))
    if h["psot"]:
        end = h["sot"] + h["psot"]
        if end < h["data"]:
            no("tile-part length %d ends inside its header" % h["psot"])
        if data[end:end + 2] == b"\xff\x90":
            no("more than one tile-part")
    rows = ifd["seg_h"] if ifd["tiled"] else min(ifd["seg_h"], ifd["length"])
    if (h["width"], h["height"]) != (ifd["seg_w"], rows):
        no("SIZ size %d x %d != segment size %d x %d" % (h["width"], h["height"], ifd["seg_w"], rows))
    if len(comps) != spp:
        no("a stream of %d components in segments of %d samples per pixel" % (len(comps), spp))
    if prec != bits:
        no("precision %d on a plane of %d-bit samples" % (prec, bits))
    if ycbcr and h["mct"]:
        no("YCbCr conversion (PBX_TIFF_F_J2K_YCBCR) on a stream with the multiple-component transform")
    return sub


def _tiff_needs_packed(ifd: dict) -> bool:
    """Whether an IFD is what the pbx_*_tiff_packed calls exist for: samples that are not whole
    bytes, PackBits segments, or FillOrder 2."""
    return ifd["bits"] not in (8, 16, 32, 64) or ifd["compression"] == TIFF_PACKBITS or ifd["fillorder"] == 2


def _tiff_packed_pixel_type(path: str, ifd: dict) -> int:
    """_tiff_pixel_type for an IFD that goes through the pbx_*_tiff_packed calls (SamplesPerPixel
    and PlanarConfiguration are checked already): bits 1 .. 7 give UINT8 and 9 .. 15 UINT16,
    unscaled, as Bio-Formats unpacks them; 8 and 16 their usual types."""
    bits, sf, spp = ifd["bits"], ifd["sampleformat"], ifd["spp"]
    if ifd["compression"] not in (1, 5, 8, 32946, TIFF_ZSTD, TIFF_PACKBITS):
        raise PbxError(400, "%s: Compression %d with %d-bit samples or FillOrder %d (1 none, 5 LZW, 8 / 32946 deflate, "
                       "50000 zstd, 32773 PackBits)" % (path, ifd["compression"], bits, ifd["fillorder"]))
    if not 1 <= bits <= 16:
        raise PbxError(400, "%s: BitsPerSample %d with Compression %d / FillOrder %d (PackBits and FillOrder 2 are "
                       "supported on samples of 1 to 16 bits)" % (path, bits, ifd["compression"], ifd["fillorder"]))
    if bits in (8, 16):
        pt = _TIFF_PIXEL_TYPES.get((sf, bits))
        if pt is None:
            raise PbxError(400, "%s: SampleFormat %d with %d bits is none of the pixel types" % (path, sf, bits))
    else:
        if sf != 1:
            raise PbxError(400, "%s: SampleFormat %d with BitsPerSample %d (packed samples are unsigned integers: "
                           "SampleFormat 1 or none)" % (path, sf, bits))
        pt = UINT8 if bits < 8 else UINT16
        if ifd.get("photometric") == 0:
            raise PbxError(400, "%s: PhotometricInterpretation 0 (WhiteIsZero) on %d-bit packed samples is not "
                           "supported (the samples would have to be inverted)" % (path, bits))
    if ifd.get("photometric") == 3:
        raise PbxError(400, "%s: PhotometricInterpretation 3 (palette colour) is not supported" % path)
    if spp == 1 and ifd.get("photometric") not in (None, 0, 1):
        raise PbxError(400, "%s: PhotometricInterpretation %d with one %d-bit sample per pixel (0 or 1)"
                       % (path, ifd["photometric"], bits))
    if ifd["predictor"] != 1:
        raise PbxError(400, "%s: Predictor %d with %s (the predictor is defined on whole-byte samples, and the packed "
                       "path takes 1 only)" % (path, ifd["predictor"], "BitsPerSample %d" % bits if bits not in (8, 16)
                                               else "Compression 32773" if ifd["compression"] == TIFF_PACKBITS
                                               else "FillOrder 2"))
    if ifd["fillorder"] not in (1, 2):
        raise PbxError(400, "%s: FillOrder %d (1 or 2)" % (path, ifd["fillorder"]))
    if ifd["fillorder"] == 2 and bits == 16:
        raise PbxError(400, "%s: FillOrder 2 with 16-bit samples" % path)
    if ifd["orientation"] != 1:
        raise PbxError(400, "%s: Orientation %d (only 1, top left, is supported)" % (path, ifd["orientation"]))
    return pt


def _tiff_pixel_type(path: str, ifd: dict, j2k_packets: bool = False, j2k_chroma: bool = False,
                     aperio_ycbcr: bool = False, j2k_flags: Optional[list] = None, packed: bool = False) -> int:
    """The pixel type of an IFD this library can load, else PbxError 400 with the reason.
    SamplesPerPixel 1 to 4: every sample is a channel of that type, ExtraSamples included.
    For a Compression-7 IFD, and for a JPEG 2000 one (Compression 33003 / 33004 / 33005 / 34712),
    the first segment is read and its header checked too, by every caller (a band spec of no
    rows included: its refusals are tiff_plane_spec's).  j2k_packets, j2k_chroma, aperio_ycbcr: as
    tiff_plane_spec's; j2k_flags, a list, receives the TIFF_F_J2K_* flags a JPEG 2000 IFD's
    segments are to be handed over with.  packed: as tiff_plane_spec's; an IFD of 1- to 7-bit
    samples is then UINT8 and one of 9- to 15-bit samples UINT16."""
    spp = ifd["spp"]
    # a three-sample chunky JPEG 2000 IFD: YCbCr components outside the codestream
    j2k_rgb = ifd["compression"] in _TIFF_J2K_COMPRESSIONS and spp == 3 and ifd.get("planar", 1) == 1
    ycbcr = j2k_rgb and ((j2k_chroma and ifd.get("photometric") == 6) or (aperio_ycbcr and ifd["compression"] == 33003))
    if spp < 1 or spp > 4:
        raise PbxError(400, "%s: SamplesPerPixel %d (1 to 4 are supported)" % (path, spp))
    if spp > 1 and ifd.get("bits_count", 1) != spp:  # TIFF 6.0: one BitsPerSample value per sample
        raise PbxError(400, "%s: SamplesPerPixel %d with %d BitsPerSample value(s)"
                       % (path, spp, ifd.get("bits_count", 1)))
    jpeg = ifd["compression"] == TIFF_JPEG
    if spp > 1 and ifd.get("photometric") not in (None, 1, 2) and not (jpeg and ifd["photometric"] == 6 and spp == 3) \
            and not (ycbcr and ifd["photometric"] == 6 and j2k_chroma):
        raise PbxError(400, "%s: PhotometricInterpretation %d with SamplesPerPixel %d (1 BlackIsZero or 2 RGB, 6 YCbCr "
                       "with 3 samples under Compression 7; palette and CMYK are not supported)"
                       % (path, ifd["photometric"], spp))
    if ifd.get("planar", 1) not in (1, 2):
        raise PbxError(400, "%s: PlanarConfiguration %d (1 chunky or 2 planar)" % (path, ifd["planar"]))
    if packed and _tiff_needs_packed(ifd):  # (every other IFD is checked as it always was)
        return _tiff_packed_pixel_type(path, ifd)
    if ifd["bits"] not in (8, 16, 32, 64):
        raise PbxError(400, "%s: BitsPerSample %d (8, 16, 32 or 64)" % (path, ifd["bits"]))
    if spp > 1 and ifd["bits"] == 64:
        raise PbxError(400, "%s: SamplesPerPixel %d with 64-bit samples" % (path, spp))
    pt = _TIFF_PIXEL_TYPES.get((ifd["sampleformat"], ifd["bits"]))
    if pt is None:
        raise PbxError(400, "%s: SampleFormat %d with %d bits is none of the pixel types"
                       % (path, ifd["sampleformat"], ifd["bits"]))
    if jpeg and pt != UINT8:
        raise PbxError(400, "%s: Compression %d (1 none, 5 LZW, 7 JPEG on 8-bit samples, 8 / 32946 deflate, 50000 zstd)"
                       % (path, ifd["compression"]))
    j2k = ifd["compression"] in _TIFF_J2K_COMPRESSIONS
    if ifd["compression"] not in (1, 5, 8, 32946, TIFF_ZSTD) and not jpeg and not j2k:  # (the text older callers match)
        raise PbxError(400, "%s: Compression %d (1 none, 5 LZW, 8 / 32946 deflate, 50000 zstd)"
                       % (path, ifd["compression"]))
    if j2k:
        planar = spp > 1 and ifd.get("planar", 1) == 2
        if pt not in (UINT8, UINT16):
            raise PbxError(400, "%s: Compression %d (JPEG 2000) on samples that are neither uint8 nor uint16"
                           % (path, ifd["compression"]))
        if ifd["predictor"] != 1:
            raise PbxError(400, "%s: Predictor %d with Compression %d (JPEG 2000 segments take 1 only)"
                           % (path, ifd["predictor"], ifd["compression"]))
        if ifd.get("photometric") not in (None, 0, 1, 2) and not (ycbcr and ifd["photometric"] == 6 and j2k_chroma):
            raise PbxError(400, "%s: PhotometricInterpretation %d with Compression %d (JPEG 2000: 0, 1 or 2)"
                           % (path, ifd["photometric"], ifd["compression"]))
        if spp not in (1, 3) and not planar:
            raise PbxError(400, "%s: Compression %d (JPEG 2000) with SamplesPerPixel %d (1, or 3 chunky)"
                           % (path, ifd["compression"], spp))
        sub = _tiff_j2k_first_segment(path, ifd, 1 if planar else spp, ifd["bits"], j2k_packets,
                                      bool(j2k_chroma and j2k_rgb), bool(ycbcr))
        if j2k_flags is not None:
            j2k_flags.append((TIFF_F_J2K_PACKETS if j2k_packets else 0) | (TIFF_F_J2K_SUBSAMPLED if sub else 0) |
                             (TIFF_F_J2K_YCBCR if ycbcr else 0))
    if jpeg:
        planar = spp > 1 and ifd.get("planar", 1) == 2
        if ifd["predictor"] != 1:
            raise PbxError(400, "%s: Predictor %d with Compression 7 (JPEG segments take 1 only)" % (path, ifd["predictor"]))
        if spp not in (1, 3) and not planar:
            raise PbxError(400, "%s: Compression 7 with SamplesPerPixel %d (1, or 3 chunky; 4 components, CMYK / YCCK, "
                           "are not supported)" % (path, spp))
        if ifd.get("photometric") == 6 and planar:
            raise PbxError(400, "%s: PhotometricInterpretation 6 (YCbCr) with PlanarConfiguration 2 under Compression 7"
                           % path)
        if ifd.get("photometric") == 6 and spp != 3:
            raise PbxError(400, "%s: PhotometricInterpretation 6 (YCbCr) with SamplesPerPixel %d" % (path, spp))
        _tiff_jpeg_first_segment(path, ifd, 1 if planar else spp)
    if ifd["predictor"] not in (1, 2, 3):
        raise PbxError(400, "%s: Predictor %d (1, 2, or 3 on floating-point samples)" % (path, ifd["predictor"]))
    if ifd["predictor"] == 3 and pt not in (FLOAT, DOUBLE):
        raise PbxError(400, "%s: Predictor 3 (the floating-point predictor) on integer samples" % path)
    if ifd["predictor"] == 3 and spp > 1 and ifd.get("planar", 1) != 2:
        raise PbxError(400, "%s: Predictor 3 (the floating-point predictor) on chunky segments of %d samples per "
                       "pixel is not supported" % (path, spp))
    if ifd["predictor"] == 2 and pt in (FLOAT, DOUBLE):
        raise PbxError(400, "%s: Predictor 2 on floating-point samples" % path)
    if ifd["fillorder"] != 1:
        raise PbxError(400, "%s: FillOrder %d (only 1 is supported)" % (path, ifd["fillorder"]))
    if ifd["orientation"] != 1:
        raise PbxError(400, "%s: Orientation %d (only 1, top left, is supported)" % (path, ifd["orientation"]))
    return pt


def tiff_plane_spec(path: str, ifd: dict, image_id: int, z: int, c: int, t: int, level: int = 0,
                    sample: int = 0, j2k_packets: bool = False, j2k_chroma: bool = False,
                    aperio_ycbcr: bool = False, packed: bool = False) -> dict:
    """register_tiff_planes() arguments for the plane that is sample `sample` of one IFD (a
    tiff_ifds() dict, main or SubIFD): its segments are read from the file as they are, nothing
    is decoded here.  A chunky IFD (PlanarConfiguration 1) of S samples per pixel gives
    samples_per_pixel = S and all its segments, each holding all S samples; a planar one
    (PlanarConfiguration 2) an ordinary single-sample spec (samples_per_pixel = 1, sample = 0)
    of the segments of its group `sample`.  PbxError 400 names what is not supported.
    j2k_packets (JPEG 2000 IFDs only): take streams with several quality layers, several precincts
    in a resolution and SOP / EPH markers; the spec then carries flags = TIFF_F_J2K_PACKETS.
    Without it such a file is refused by name, as it always was.
    j2k_chroma (three-sample chunky JPEG 2000 IFDs only): take streams whose second and third
    components are stored at half width and / or half height (2 x 1, 1 x 2 or 2 x 2; replicated on
    the GPU), and PhotometricInterpretation 6: the components are then converted from YCbCr to RGB.
    The spec's flags carry TIFF_F_J2K_SUBSAMPLED and / or TIFF_F_J2K_YCBCR where the IFD needs them
    and only then.  Without it both are refused by name, as they always were.
    aperio_ycbcr: treat Compression 33003 with three chunky samples as YCbCr whatever the
    photometric tag says (OpenSlide's rule; off by default because the IFD does not say so).
    packed: take BitsPerSample 1 to 7 (a UINT8 plane) and 9 to 15 (UINT16; SampleFormat 1 or
    none), Compression 32773 (PackBits) and FillOrder 2: samples are unpacked MSB-first on the
    GPU, unscaled, as Bio-Formats hands them to the reference.  The spec of such an IFD then
    carries packed = dict(bits, fill_order) and goes through the pbx_*_tiff_packed calls; every
    other IFD's is what it always was.  Still refused by name: palette colour, WhiteIsZero on
    packed samples, Predictor 2 on this path, samples of different widths, signed samples below 8
    bits.  Without the keyword all of these IFDs are refused with the texts they always were."""
    return dict(_tiff_segment_rows(path, ifd, 0, None, sample, j2k_packets, j2k_chroma, aperio_ycbcr, packed),
                image_id=image_id, z=z, c=c, t=t, level=level)


def _tiff_segment_rows(path: str, ifd: dict, sr0: int, sr1: Optional[int], sample: int = 0,
                       j2k_packets: bool = False, j2k_chroma: bool = False, aperio_ycbcr: bool = False,
                       packed: bool = False) -> dict:
    """What tiff_plane_spec and tiff_band_spec share: the IFD's pixel type, geometry and byte
    order, and segments = (data, offsets) of its segment rows [sr0, sr1) (sr1 None: to the last;
    sr1 == sr0: none, segments is None and the file is not opened), each full width, read from
    the file as they are.  A planar IFD holds spp groups of gx * gy segments, one per sample:
    the rows are those of group `sample`."""
    import numpy as np
    j2k_flags: list = []
    pt = _tiff_pixel_type(path, ifd, j2k_packets, j2k_chroma, aperio_ycbcr, j2k_flags, packed)
    spp = ifd["spp"]
    if not 0 <= sample < spp:
        raise PbxError(400, "%s: sample %d outside SamplesPerPixel %d" % (path, sample, spp))
    planar = spp > 1 and ifd.get("planar", 1) == 2
    gx = -(-ifd["width"] // ifd["seg_w"]) if ifd["tiled"] else 1
    gy = -(-ifd["length"] // ifd["seg_h"])
    if planar and len(ifd["offsets"]) != spp * gx * gy:
        raise PbxError(400, "%s: %d segments for %d planar samples on a grid of %d x %d"
                       % (path, len(ifd["offsets"]), spp, gx, gy))
    if not planar and len(ifd["offsets"]) != gx * gy:
        raise PbxError(400, "%s: %d segments for a grid of %d x %d" % (path, len(ifd["offsets"]), gx, gy))
    base = sample * gx * gy if planar else 0
    k0, k1 = base + sr0 * gx, base + (gy if sr1 is None else sr1) * gx
    segments = None
    if k1 > k0:
        offsets = np.zeros(k1 - k0 + 1, dtype=np.uint64)
        np.cumsum(np.array(ifd["counts"][k0:k1], dtype=np.uint64), out=offsets[1:])
        data = np.empty(max(int(offsets[-1]), 1), dtype=np.uint8)
        with open(path, "rb") as f:
            for k, (o, n) in enumerate(zip(ifd["offsets"][k0:k1], ifd["counts"][k0:k1])):
                f.seek(o)
                if f.readinto(memoryview(data)[int(offsets[k]):int(offsets[k]) + n]) != n:
                    raise PbxError(400, "%s: segment %d is truncated" % (path, k0 + k))
        segments = (data, offsets)
    extra = {}
    if ifd["compression"] == TIFF_JPEG:  # -> the pbx_*_tiff_jpeg calls
        tables = ifd.get("jpeg_tables")
        extra["jpeg"] = dict(tables=bytes(tables) if tables is not None else None,
                             ycbcr=ifd.get("photometric") == 6 and not planar)
    if ifd["compression"] in _TIFF_J2K_COMPRESSIONS:  # -> the pbx_*_tiff_j2k calls
        extra["j2k"] = True
        if j2k_flags and j2k_flags[0]:
            extra["flags"] = j2k_flags[0]
    if packed and _tiff_needs_packed(ifd):  # -> the pbx_*_tiff_packed calls
        extra["packed"] = dict(bits=ifd["bits"], fill_order=ifd["fillorder"])
    return dict(extra, samples_per_pixel=1 if planar else spp, sample=0 if planar else sample, pixel_type=pt, size_x=ifd["width"], size_y=ifd["length"],
                big_endian=ifd["byteorder"] == ">", seg_w=ifd["seg_w"], seg_h=ifd["seg_h"],
                tiled=ifd["tiled"],
                compression=TIFF_DEFLATE if ifd["compression"] == 32946 else
                TIFF_J2K if ifd["compression"] in _TIFF_J2K_COMPRESSIONS else ifd["compression"],
                predictor=ifd["predictor"], segments=segments)


def tiff_band_spec(path: str, ifd: dict, y0: int, rows: int, sample: int = 0, j2k_packets: bool = False,
                   j2k_chroma: bool = False, aperio_ycbcr: bool = False, packed: bool = False) -> dict:
    """band_write_tiff() arguments for rows [y0, y0 + rows) of the plane that is sample `sample`
    of one IFD (a tiff_ifds() dict, main or SubIFD; samples_per_pixel and sample as
    tiff_plane_spec, and of a planar IFD only that sample's segments are read): pixel_type, size_x, size_y, big_endian (the file's byte order),
    seg_w, seg_h, tiled, compression, predictor and segments = (data, offsets) of the segment
    rows y0 // seg_h .. ceil((y0 + rows) / seg_h) - 1 only, each full width; exactly those byte
    ranges of the file are read.  rows == 0 reads nothing (segments is None): the geometry and
    byte order alone (of a Compression-7 IFD also segment 0, whose header decides whether the file
    can be loaded at all).  PbxError 400 as tiff_plane_spec, and for rows outside the plane.
    j2k_packets, j2k_chroma, aperio_ycbcr, packed: as tiff_plane_spec's (a packed IFD's spec
    carries `packed`, band_write_tiff's keyword of that name)."""
    if rows < 0 or y0 < 0 or y0 + rows > ifd["length"]:
        raise PbxError(400, "%s: rows %d+%d outside the image (%d rows)" % (path, y0, rows, ifd["length"]))
    sr0 = y0 // ifd["seg_h"]
    sr1 = -(-(y0 + rows) // ifd["seg_h"]) if rows else sr0
    return dict(_tiff_segment_rows(path, ifd, sr0, sr1, sample, j2k_packets, j2k_chroma, aperio_ycbcr, packed),
                y0=y0, rows=rows)


def _ome_layout(path: str, xml: str, samples: int = 1) -> Optional[dict]:
    """SizeZ/C/T, DimensionOrder and Type of the first Image of an OME-XML ImageDescription (None
    if the description is not OME-XML).  400 for what register_tiff_image cannot follow.  With
    `samples` = S samples per pixel in every IFD, the IFDs run over SizeC / S channel groups in
    DimensionOrder: planes[k] is the (z, c0, t) of IFD k's first sample, c0 a multiple of S."""
    if "<OME" not in xml[:4096]:
        return None
    import xml.etree.ElementTree as ET
    try:
        root = ET.fromstring(xml)
    except ET.ParseError as e:
        raise PbxError(400, "%s: OME-XML does not parse: %s" % (path, e))

    def local(el):
        return el.tag.rsplit("}", 1)[-1]
    images = [el for el in root if local(el) == "Image"]
    if len(images) != 1:
        raise PbxError(400, "%s: OME-XML with %d Image elements (only one is supported)" % (path, len(images)))
    px = [el for el in images[0] if local(el) == "Pixels"]
    if len(px) != 1:
        raise PbxError(400, "%s: OME-XML Image without Pixels" % path)
    a = px[0].attrib
    try:
        sz, sc, st = int(a["SizeZ"]), int(a["SizeC"]), int(a["SizeT"])
        order, typ = a["DimensionOrder"], a["Type"]
        sxy = (int(a["SizeX"]), int(a["SizeY"]))
    except (KeyError, ValueError) as e:
        raise PbxError(400, "%s: OME-XML Pixels attribute %s" % (path, e))
    if len(order) != 5 or order[:2] != "XY" or sorted(order[2:]) != ["C", "T", "Z"]:
        raise PbxError(400, "%s: OME-XML DimensionOrder %r" % (path, order))
    if typ not in PIXEL_TYPES:
        raise PbxError(400, "%s: OME-XML pixel Type %r" % (path, typ))
    if min(sz, sc, st) < 1:
        raise PbxError(400, "%s: OME-XML SizeZ/C/T %d/%d/%d" % (path, sz, sc, st))
    for ch in (el for el in px[0] if local(el) == "Channel"):
        try:
            cs = int(ch.attrib.get("SamplesPerPixel", 1))
        except ValueError as e:
            raise PbxError(400, "%s: OME-XML Channel attribute %s" % (path, e))
        if cs != samples:
            raise PbxError(400, "%s: OME-XML Channel with SamplesPerPixel %d, the first IFD has %d"
                           % (path, cs, samples))
    if sc % samples:
        raise PbxError(400, "%s: OME-XML SizeC %d is no multiple of the IFDs' SamplesPerPixel %d"
                       % (path, sc, samples))
    ext = {"Z": sz, "C": sc // samples, "T": st}
    planes = []
    for k in range(sz * (sc // samples) * st):
        idx, r = {}, k
        for ax in order[2:]:
            idx[ax] = r % ext[ax]
            r //= ext[ax]
        planes.append((idx["Z"], idx["C"] * samples, idx["T"]))
    at = {p: k for k, p in enumerate(planes)}
    for td in (el for el in px[0] if local(el) == "TiffData"):
        for u in (el for el in td if local(el) == "UUID"):
            fn = u.attrib.get("FileName")
            if fn is not None and os.path.basename(fn) != os.path.basename(path):
                raise PbxError(400, "%s: OME-XML TiffData names another file, %r (multi-file OME-TIFF is not "
                               "supported)" % (path, fn))
        ta = td.attrib
        try:
            first = (int(ta.get("FirstZ", 0)), int(ta.get("FirstC", 0)), int(ta.get("FirstT", 0)))
            ifd0 = int(ta.get("IFD", 0))
        except ValueError as e:
            raise PbxError(400, "%s: OME-XML TiffData attribute %s" % (path, e))
        if at.get(first) != ifd0:  # only the DimensionOrder's own layout: IFD k is plane k
            raise PbxError(400, "%s: OME-XML TiffData puts plane z=%d c=%d t=%d in IFD %d, not in "
                           "DimensionOrder %s" % ((path,) + first + (ifd0, order)))
    return dict(size_z=sz, size_c=sc, size_t=st, planes=planes, pixel_type=PIXEL_TYPES.index(typ), size_xy=sxy)


def tiff_image_layout(path: str, j2k_packets: bool = False, j2k_chroma: bool = False, aperio_ycbcr: bool = False,
                      packed: bool = False) -> dict:
    """What register_tiff_image and TiffSource make of a file: ifds (tiff_ifds), planes = the
    (z, c, t) of main IFD k's first sample, samples = S (SamplesPerPixel, the same in every IFD),
    size_z / size_c / size_t, pixel_type, levels (1 + SubIFDs per main IFD).  Every sample is a
    channel, ExtraSamples included: channel c lies in the IFD of (z, c - c % S, t) as sample
    c % S.  OME-TIFF: the first Image's SizeZ/C/T and DimensionOrder, IFD k = channel group k in
    that order.  Any other multi-page TIFF: page k is t = k and size_c = S (Bio-Formats'
    BaseTiffReader puts the pages of a plain TIFF on the time axis).  j2k_packets, j2k_chroma,
    aperio_ycbcr: as tiff_plane_spec's, for the header checks of JPEG 2000 IFDs; packed: as
    tiff_plane_spec's."""
    ifds = tiff_ifds(path)
    pt = _tiff_pixel_type(path, ifds[0], j2k_packets, j2k_chroma, aperio_ycbcr, packed=packed)
    S = ifds[0]["spp"]
    ome = _ome_layout(path, ifds[0]["description"], S) if ifds[0]["description"] else None
    if ome is not None:
        n = len(ome["planes"])
        if len(ifds) < n:
            raise PbxError(400, "%s: OME-XML names %d planes, the file has %d IFDs" % (path, n, len(ifds)))
        if ome["pixel_type"] != pt or ome["size_xy"] != (ifds[0]["width"], ifds[0]["length"]):
            raise PbxError(400, "%s: OME-XML Pixels disagree with the first IFD on type or size" % path)
        out = dict(ome, ifds=ifds[:n])
    else:
        out = dict(size_z=1, size_c=S, size_t=len(ifds), planes=[(0, 0, k) for k in range(len(ifds))],
                   pixel_type=pt, ifds=ifds)
    out["samples"] = S
    first = out["ifds"][0]
    for k, d in enumerate(out["ifds"]):
        if (d["width"], d["length"]) != (first["width"], first["length"]) or _tiff_pixel_type(path, d, j2k_packets, j2k_chroma, aperio_ycbcr, packed=packed) != pt:
            raise PbxError(400, "%s: IFD %d differs from the first in size or pixel type" % (path, k))
        for sd in [d] + d["subifds"]:
            if sd["spp"] != S:
                raise PbxError(400, "%s: IFD %d has SamplesPerPixel %d, the first has %d" % (path, k, sd["spp"], S))
        if len(d["subifds"]) != len(first["subifds"]):
            raise PbxError(400, "%s: IFD %d has %d SubIFDs, the first has %d" % (path, k, len(d["subifds"]),
                                                                                len(first["subifds"])))
    out["levels"] = 1 + len(first["subifds"])
    return out


def ngff_multiscales(image_dir: str):
    """(multiscales[0], image directory) of an NGFF image: .zattrs (NGFF 0.1-0.4), or without
    one the "ome" attributes of a Zarr v3 group's zarr.json (NGFF 0.5).  A bioformats2raw
    container root (attribute "bioformats2raw.layout") resolves to series 0."""
    if not os.path.exists(os.path.join(image_dir, ".zattrs")) and \
            os.path.exists(os.path.join(image_dir, "zarr.json")):
        # NGFF 0.5: a Zarr v3 group whose attributes["ome"] holds what .zattrs held
        with open(os.path.join(image_dir, "zarr.json")) as f:
            doc = json.load(f)
        if not isinstance(doc, dict) or doc.get("zarr_format") != 3 or doc.get("node_type") != "group":
            raise PbxError(400, "%s/zarr.json is not a Zarr v3 group" % image_dir)
        attrs = (doc.get("attributes") or {}).get("ome")
        if not isinstance(attrs, dict):
            raise PbxError(400, "no \"ome\" attributes in %s/zarr.json" % image_dir)
        where = "zarr.json"
    else:
        with open(os.path.join(image_dir, ".zattrs")) as f:
            attrs = json.load(f)
        where = ".zattrs"
    if "multiscales" not in attrs and "bioformats2raw.layout" in attrs:
        return ngff_multiscales(os.path.join(image_dir, "0"))
    ms = attrs.get("multiscales")
    if not ms or not ms[0].get("datasets"):
        raise PbxError(400, "no multiscales datasets in %s/%s" % (image_dir, where))
    return ms[0], image_dir


def make_config(device: Optional[int] = None, png_filter: int = FILTER_NONE,
                tiff_deflate: bool = False, coalesce: bool = True, stage_rows: bool = False,
                tiff_tile: Optional[int] = None, request_timeout_us: Optional[int] = None,
                deflate_strategy: Optional[int] = None, tiff_predictor: Optional[int] = None) -> PbxConfig:
    """``deflate_strategy`` and ``tiff_predictor`` are not fields of pbx_config (the struct keeps
    its size): they are checked here and applied by ``PixelsService`` with their setters right
    after init."""
    if deflate_strategy is not None and deflate_strategy not in (DEFLATE_DEFAULT, DEFLATE_HUFFMAN_ONLY,
                                                                  DEFLATE_AUTO):
        raise PbxError(E_BADARG, "deflate strategy %r out of range" % (deflate_strategy,))
    if tiff_predictor is not None and tiff_predictor not in (TIFF_PREDICTOR_NONE, TIFF_PREDICTOR_HORIZONTAL):
        raise PbxError(E_BADARG, "TIFF predictor %r out of range" % (tiff_predictor,))
    cfg = PbxConfig()
    _check(lib().pbx_config_default(ctypes.byref(cfg)))
    cfg.device = -1 if device is None else device
    cfg.png_filter = png_filter
    cfg.tiff_deflate = 1 if tiff_deflate else 0
    cfg.coalesce = 1 if coalesce else 0
    cfg.stage_rows = 1 if stage_rows else 0
    if tiff_tile is not None:  # else $PBX_TIFF_TILE or 0 (one strip, the reference's)
        cfg.tiff_tile = int(tiff_tile)
    if request_timeout_us is not None:  # else $PBX_REQUEST_TIMEOUT_US or 15 s (the event-bus send timeout)
        cfg.request_timeout_us = int(request_timeout_us)
    return cfg


class PixelsService:
    """Plane registry on one MI355X (the PixelsService / getPixels stand-in).

    Planes live in HBM.  ``register_plane`` takes a numpy array (any byte order) or a
    synthetic generator ("fake" = Bio-Formats FakeReader style, "noise" = G_NOISE).
    """

    def __init__(self, device: Optional[int] = None, png_filter: int = FILTER_NONE,
                 tiff_deflate: bool = False, coalesce: bool = True, stage_rows: bool = False,
                 tiff_tile: Optional[int] = None, sparse_band_rows: int = 0,
                 request_timeout_us: Optional[int] = None, deflate_strategy: Optional[int] = None,
                 tiff_predictor: Optional[int] = None, fill_siblings: bool = False, reduce_step: int = 2,
                 _handle=None):
        """deflate_strategy: DEFLATE_DEFAULT / DEFLATE_HUFFMAN_ONLY / DEFLATE_AUTO (None: the
        library's initial value, $PBX_DEFLATE_STRATEGY or DEFAULT).
        tiff_predictor: TIFF_PREDICTOR_NONE / TIFF_PREDICTOR_HORIZONTAL for deflated TIFF
        responses of integer pixel types (None: $PBX_TIFF_PREDICTOR or NONE).
        sparse_band_rows > 0: planes the handler opens on demand are sparse planes of bands
        of that many rows (region-proportional residency); 0: whole planes (or the handler's
        row band).
        fill_siblings: load_bands fills the bands of the planes that share the primary's segments
        or chunks (the other channels of chunky TIFF samples, of Zarr chunks that hold several
        channels) from the primary's one decode (band_write_*_group).  Off by default: a cold
        request then creates and fills its own plane alone.
        reduce_step (1 .. 4): a band of a derived level (DerivedLevels) is made from the level that
        many levels above it, or from the last stored level if that is nearer; the levels in
        between are not made for it.  A larger step reads more base rows per band (2^step rows
        per row) and caches fewer intermediate bands."""
        import threading
        if not 1 <= int(reduce_step) <= 4:
            raise ValueError("reduce_step %r outside 1 .. 4" % (reduce_step,))
        self.reduce_step = int(reduce_step)
        self.sparse_band_rows = int(sparse_band_rows)
        self.fill_siblings = bool(fill_siblings)
        self._load_lock = threading.Lock()  # one loader per plane key / band
        self._loading: Dict[tuple, list] = {}  # key -> [lock, users]; removed with its last user
        self._owned = _handle is None
        if _handle is not None:  # a context owned by a PixelsNode
            self._h = ctypes.c_void_p(_handle)
            return
        L = lib()
        cfg = make_config(device, png_filter, tiff_deflate, coalesce, stage_rows, tiff_tile,
                          request_timeout_us, deflate_strategy, tiff_predictor)
        h = ctypes.c_void_p()
        _check(L.pbx_init(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        if deflate_strategy is not None:
            self.set_deflate_strategy(deflate_strategy)
        if tiff_predictor is not None:
            self.set_tiff_predictor(tiff_predictor)

    def close(self) -> None:
        if self._h and self._owned:
            lib().pbx_shutdown(self._h)
        self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def register_plane(self, image_id: int, z: int, c: int, t: int, pixel_type: int,
                       size_x: int, size_y: int, data=None, generator: Optional[str] = None,
                       seed: int = 0, plane_no: int = 0, level: int = 0,
                       big_endian: Optional[bool] = None) -> int:
        """``level`` is the STORED pyramid level (0 = full resolution, the NGFF dataset
        index); requests name levels in OMERO's numbering (TileCtx.resolution, levels-1 =
        full resolution)."""
        d = PbxPlaneDesc()
        d.image_id, d.z, d.c, d.t, d.resolution = image_id, z, c, t, level
        d.pixel_type, d.size_x, d.size_y = pixel_type, size_x, size_y
        keep = None
        if generator is not None:
            d.source = {"fake": SRC_GEN_FAKE, "noise": SRC_GEN_NOISE}[generator]
            d.seed, d.plane_no = seed, plane_no
        else:
            import numpy as np
            a = np.ascontiguousarray(data)
            if big_endian is None:
                big_endian = a.dtype.byteorder == ">" or (
                    a.dtype.byteorder == "=" and os.sys.byteorder == "big")
            keep = a.view(np.uint8).reshape(-1)
            d.source = SRC_HOST
            d.byte_order = BIG_ENDIAN if big_endian else LITTLE_ENDIAN
            d.host_data = keep.ctypes.data
            d.host_bytes = keep.nbytes
        pid = ctypes.c_uint64()
        _check(lib().pbx_plane_register(self._h, ctypes.byref(d), ctypes.byref(pid)))
        del keep
        return pid.value

    def register_zarr_plane(self, image_id: int, z: int, c: int, t: int, pixel_type: int,
                            size_x: int, size_y: int, chunk_x: int, chunk_y: int,
                            codec: Optional[str], chunks: Sequence[Optional[bytes]],
                            big_endian: bool = True, fill_bits: int = 0, level: int = 0,
                            timing: bool = False, crc32c: bool = False):
        """Register a plane from its Zarr chunks (C order over the chunk grid; None or
        b"" = missing chunk -> fill; or pack_chunks()' (data, offsets) pair), decoded on the GPU
        (pbx_plane_register_zarr).  codec is the .zarray compressor id or the v3 codec name: None,
        "blosc", "zlib", "zstd" or "gzip"; crc32c: every chunk ends in the v3 crc32c codec's
        checksum (checked on the GPU).  Returns the plane id (and the
        decode / placement kernels' device ms with timing=True)."""
        if codec not in ZARR_CODECS:
            raise PbxError(400, "unsupported Zarr compressor %r" % (codec,))
        data, offsets = chunks if isinstance(chunks, tuple) else pack_chunks(chunks)
        d = PbxPlaneDesc()
        d.image_id, d.z, d.c, d.t, d.resolution = image_id, z, c, t, level
        d.pixel_type, d.size_x, d.size_y = pixel_type, size_x, size_y
        d.byte_order = BIG_ENDIAN if big_endian else LITTLE_ENDIAN
        zc = PbxZarrChunks()
        zc.chunk_x, zc.chunk_y, zc.codec = chunk_x, chunk_y, ZARR_CODECS[codec]
        zc.flags = ZARR_F_CRC32C if crc32c else 0
        zc.data, zc.offsets, zc.fill_bits = data.ctypes.data, offsets.ctypes.data, fill_bits
        pid = ctypes.c_uint64()
        ms = (ctypes.c_double * 2)()
        _check(lib().pbx_plane_register_zarr(self._h, ctypes.byref(d), ctypes.byref(zc),
                                             ctypes.byref(pid), ms))
        return (pid.value, (ms[0], ms[1])) if timing else pid.value

    def register_zarr_planes(self, planes: Sequence[dict], timing: bool = False):
        """Several Zarr planes decoded by one set of GPU launches (pbx_planes_register_zarr):
        each dict holds register_zarr_plane's arguments (image_id, z, c, t, pixel_type,
        size_x, size_y, chunk_x, chunk_y, codec, chunks[, big_endian, fill_bits,
        level, crc32c]).  All are registered or none.  Returns the plane ids (and the kernels'
        device ms with timing=True).  If some dict has chunk_planes > 1 (chunks that hold
        several planes, with its slice; zarr_plane_spec), the planes go through
        register_zarr_planes_deep, those with an equal "layer" sharing one set of chunks."""
        import numpy as np
        if any(p.get("chunk_planes", 1) > 1 for p in planes):
            layers, index, refs = [], {}, []
            for k, p in enumerate(planes):
                key = p.get("layer", ("plane", k))  # no layer named: chunks of its own
                if key not in index:
                    index[key] = len(layers)
                    layers.append(dict(chunk_x=p["chunk_x"], chunk_y=p["chunk_y"], codec=p["codec"],
                                       chunks=p["chunks"], fill_bits=p.get("fill_bits", 0),
                                       chunk_planes=p.get("chunk_planes", 1), crc32c=p.get("crc32c", False)))
                refs.append((index[key], p.get("slice", 0)))
            return self.register_zarr_planes_deep(planes, refs, layers, timing)
        n = len(planes)
        descs = (PbxPlaneDesc * n)()
        zcs = (PbxZarrChunks * n)()
        keep = []
        for k, p in enumerate(planes):
            keep += _fill_zarr_chunks(zcs[k], p)
            _fill_plane_desc(descs[k], p)
        ids = (ctypes.c_uint64 * n)()
        ms = (ctypes.c_double * 2)()
        _check(lib().pbx_planes_register_zarr(self._h, n, descs, zcs, ids, ms))
        del keep
        return (list(ids), (ms[0], ms[1])) if timing else list(ids)

    def register_zarr_planes_deep(self, planes: Sequence[dict], refs: Sequence[Tuple[int, int]],
                                  layers: Sequence[dict], timing: bool = False):
        """pbx_planes_register_zarr_deep: planes[k] (image_id, z, c, t, pixel_type, size_x, size_y
        [, big_endian, level]) is slice refs[k][1] of every chunk of layers[refs[k][0]]; a layer
        is a dict of chunk_x, chunk_y, codec, chunks (as register_zarr_plane), chunk_planes
        [, fill_bits, crc32c].  Every chunk is uploaded and decoded once.  Returns as
        register_zarr_planes."""
        n, nl = len(planes), len(layers)
        descs = (PbxPlaneDesc * n)()
        rf = (PbxZarrSlice * n)()
        zcs = (PbxZarrChunks * max(nl, 1))()
        depths = (ctypes.c_int32 * max(nl, 1))()
        keep = []
        for k, p in enumerate(planes):
            _fill_plane_desc(descs[k], p)
            if not (0 <= refs[k][0] < 2 ** 32 and 0 <= refs[k][1] < 2 ** 32):
                raise PbxError(400, "plane %d: bad layer or slice %r" % (k, tuple(refs[k])))
            rf[k].layer, rf[k].slice = refs[k]
        for k, l in enumerate(layers):
            keep += _fill_zarr_chunks(zcs[k], l)
            depths[k] = l.get("chunk_planes", 1)
        ids = (ctypes.c_uint64 * n)()
        ms = (ctypes.c_double * 2)()
        _check(lib().pbx_planes_register_zarr_deep(self._h, n, descs, rf, nl, zcs, depths, ids, ms))
        del keep
        return (list(ids), (ms[0], ms[1])) if timing else list(ids)

    def register_zarr_array(self, array_dir: str, image_id: int, z: int, c: int, t: int,
                            level: int = 0) -> int:
        """One (t, c, z) plane of an NGFF multiscale dataset (a Zarr v2 array directory, or a v3
        one: zarr.json and no .zarray, chunks or shards, zarr3_array_meta; with
        shape [..., y, x], NGFF order t, c, z, y, x) — what ZarrPixelBuffer reads through
        JZarr (omero-zarr-pixel-buffer 0.6.1, build.gradle:57).  Chunks of the plane are read
        from disk here and decoded on the GPU."""
        sp = zarr_plane_spec(array_dir, image_id, z, c, t, level)
        return self.register_zarr_planes([sp])[0]

    @staticmethod
    def _array_planes(meta: dict, axes) -> List[Tuple[int, int, int]]:
        names = _lead_axes(len(meta["shape"]), axes)
        ext = {"t": 1, "c": 1, "z": 1}
        ext.update(dict(zip(names, meta["shape"][:-2])))
        return [(z, c, t) for t in range(ext["t"]) for c in range(ext["c"]) for z in range(ext["z"])]

    def register_zarr_array_planes(self, array_dir: str, image_id: int,
                                   planes: Optional[Sequence[Tuple[int, int, int]]] = None,
                                   level: int = 0, axes=None) -> Dict[Tuple[int, int, int], int]:
        """Every (z, c, t) plane of an NGFF array (or the given ones) decoded by ONE set of GPU
        launches (pbx_planes_register_zarr).  Returns {(z, c, t): plane id}."""
        meta = _array_meta(array_dir)
        if planes is None:
            planes = self._array_planes(meta, axes)
        cache: dict = {}  # planes of one deep chunk share its files: read once, decoded once
        specs = [zarr_plane_spec(array_dir, image_id, z, c, t, level, meta, axes, cache) for z, c, t in planes]
        ids = self.register_zarr_planes(specs)
        return dict(zip([tuple(p) for p in planes], ids))

    def register_ngff_image(self, image_dir: str, image_id: int,
                            planes: Optional[Sequence[Tuple[int, int, int]]] = None
                            ) -> Dict[int, Dict[Tuple[int, int, int], int]]:
        """A whole NGFF multiscale image -- what ZarrPixelsService opens for an image
        (omero-zarr-pixel-buffer 0.6.1, build.gradle:57; PixelBufferVerticle.java:29,56) -- in
        ONE set of GPU launches: "multiscales"[0] (.zattrs, or the "ome" attributes of an NGFF 0.5
        group's zarr.json; ngff_multiscales) lists the datasets from full
        resolution down; dataset k becomes stored level k of every (z, c, t) plane (or of the
        given ones).  A bioformats2raw container (root .zattrs with "bioformats2raw.layout")
        is opened at its series 0.  Requests then select levels with OMERO's numbering:
        TileCtx.resolution = levels - 1 - k (TileRequestHandler.java:89-91).  All levels are
        registered, or none.  Returns {level: {(z, c, t): plane id}}."""
        ms, root = ngff_multiscales(image_dir)
        axes = ms.get("axes")
        specs, keys, cache = [], [], {}
        for k, ds in enumerate(ms["datasets"]):
            adir = os.path.join(root, ds["path"])
            meta = _array_meta(adir)
            for z, c, t in (planes if planes is not None else self._array_planes(meta, axes)):
                specs.append(zarr_plane_spec(adir, image_id, z, c, t, k, meta, axes, cache))
                keys.append((k, (z, c, t)))
        ids = self.register_zarr_planes(specs)
        out: Dict[int, Dict[Tuple[int, int, int], int]] = {}
        for (k, p), pid in zip(keys, ids):
            out.setdefault(k, {})[p] = pid
        return out

    def register_tiff_planes(self, planes: Sequence[dict], timing: bool = False):
        """Planes from TIFF strips or tiles, decoded by one set of GPU launches
        (pbx_planes_register_tiff): each dict (tiff_plane_spec) holds image_id, z, c, t,
        pixel_type, size_x, size_y, seg_w, seg_h, tiled, compression (1 none, 5 LZW, 8 deflate, 50000 zstd),
        predictor (1, 2, or 3 on FLOAT / DOUBLE planes), segments (a sequence of bytes in C order over the grid, or
        pack_chunks()' (data, offsets) pair) [, big_endian = the FILE's byte order, level,
        samples_per_pixel, sample].  Specs with samples_per_pixel > 1 (chunky segments of that many
        interleaved samples per pixel) that carry the SAME segments object are the samples of one
        layer, uploaded and decoded once (pbx_planes_register_tiff_samples).  Specs that carry
        jpeg = dict(tables = tag 347's bytes or None, ycbcr) are JPEG segments (compression 7, UINT8
        planes, samples_per_pixel 1 or 3) and go through pbx_planes_register_tiff_jpeg; a call
        that mixes them with others (a file whose pages or levels differ in compression) is two
        registrations, the others first, undone if the JPEG one fails.  Specs that carry j2k = True
        are JPEG 2000 segments (compression TIFF_J2K, UINT8 or UINT16 planes, samples_per_pixel 1
        or 3) and go through pbx_planes_register_tiff_j2k, a registration of their own after
        those, in the same way.  Specs that carry packed = dict(bits[, fill_order]) hold rows of
        bit-packed samples (bits 1 .. 16, padded to a byte per row; compression may also be
        TIFF_PACKBITS) and go through pbx_planes_register_tiff_packed, a registration of their
        own after those, in the same way.  All are
        registered or none.  Returns the plane ids (and the kernels' device ms with timing=True)."""
        jp = [3 if p.get("packed") is not None else 2 if p.get("j2k") else 1 if p.get("jpeg") is not None else 0
              for p in planes]
        if len(set(jp)) > 1:
            ids = [0] * len(planes)
            done: List[int] = []
            t0 = t1 = 0.0
            try:
                for codec in sorted(set(jp)):
                    mine = [k for k, j in enumerate(jp) if j == codec]
                    got, t = self.register_tiff_planes([planes[k] for k in mine], timing=True)
                    done += got
                    t0, t1 = t0 + t[0], t1 + t[1]
                    for k, pid in zip(mine, got):
                        ids[k] = pid
            except BaseException:
                for pid in done:
                    self.release_plane(pid)
                raise
            return (ids, (t0, t1)) if timing else ids
        if any(jp) or any(p.get("samples_per_pixel", 1) != 1 for p in planes):
            return self._register_tiff_samples(planes, timing)
        n = len(planes)
        descs = (PbxPlaneDesc * n)()
        sgs = (PbxTiffSegments * n)()
        keep = []
        for k, p in enumerate(planes):
            keep += _fill_tiff_segments(sgs[k], p)
            _fill_plane_desc(descs[k], p)
        ids = (ctypes.c_uint64 * n)()
        ms = (ctypes.c_double * 2)()
        _check(lib().pbx_planes_register_tiff(self._h, n, descs, sgs, ids, ms))
        del keep
        return (list(ids), (ms[0], ms[1])) if timing else list(ids)

    def register_tiff_planes_packed(self, planes: Sequence[dict], timing: bool = False):
        """pbx_planes_register_tiff_packed: register_tiff_planes for specs that all carry packed =
        dict(bits[, fill_order]) (tiff_plane_spec with packed=True on an IFD of 1- to 15-bit
        samples, PackBits segments or FillOrder 2).  predictor must be 1; pixel_type UINT8 / INT8
        for bits <= 8, UINT16 / INT16 above."""
        for k, p in enumerate(planes):
            if p.get("packed") is None:
                raise PbxError(400, "plane %d: no `packed` in its spec" % k)
        return self._register_tiff_samples(planes, timing)

    def _register_tiff_samples(self, planes: Sequence[dict], timing: bool):
        n = len(planes)
        descs = (PbxPlaneDesc * n)()
        rf = (PbxZarrSlice * n)()
        layer_of: Dict[int, int] = {}
        layers: List[dict] = []
        for k, p in enumerate(planes):
            spp, sample = p.get("samples_per_pixel", 1), p.get("sample", 0)
            l = layer_of.get(id(p["segments"])) if spp > 1 else None
            if l is None:
                l = len(layers)
                layers.append(p)
                if spp > 1:
                    layer_of[id(p["segments"])] = l
            elif any(layers[l].get(f) != p.get(f) for f in ("samples_per_pixel", "seg_w", "seg_h", "tiled",
                                                             "compression", "predictor", "jpeg", "j2k", "flags",
                                                             "packed")):
                raise PbxError(400, "plane %d: shares its segments with plane %d but not their layout"
                               % (k, planes.index(layers[l])))
            if not (0 <= sample < 2 ** 32):
                raise PbxError(400, "plane %d: bad sample %r" % (k, sample))
            _fill_plane_desc(descs[k], p)
            rf[k].layer, rf[k].slice = l, sample
        nl = len(layers)
        sgs = (PbxTiffSegments * nl)()
        spps = (ctypes.c_int32 * nl)()
        keep = []
        for l, p in enumerate(layers):
            keep += _fill_tiff_segments(sgs[l], p)
            spps[l] = p.get("samples_per_pixel", 1)
        ids = (ctypes.c_uint64 * n)()
        ms = (ctypes.c_double * 2)()
        if layers[0].get("packed") is not None:  # (all of them: register_tiff_planes)
            pks = (PbxTiffPacked * nl)()
            for l, p in enumerate(layers):
                _fill_tiff_packed(pks[l], p["packed"], spps[l])
            _check(lib().pbx_planes_register_tiff_packed(self._h, n, descs, rf, nl, sgs, pks, ids, ms))
        elif layers[0].get("j2k"):  # (all of them)
            _check(lib().pbx_planes_register_tiff_j2k(self._h, n, descs, rf, nl, sgs, spps, ids, ms))
        elif layers[0].get("jpeg") is not None:  # (all of them)
            jps = (PbxTiffJpeg * nl)()
            for l, p in enumerate(layers):
                keep.append(_fill_tiff_jpeg(jps[l], p["jpeg"]))
            _check(lib().pbx_planes_register_tiff_jpeg(self._h, n, descs, rf, nl, sgs, spps, jps, ids, ms))
        else:
            _check(lib().pbx_planes_register_tiff_samples(self._h, n, descs, rf, nl, sgs, spps, ids, ms))
        del keep
        return (list(ids), (ms[0], ms[1])) if timing else list(ids)

    def register_tiff_image(self, path: str, image_id: int, j2k_packets: bool = True, j2k_chroma: bool = True,
                            aperio_ycbcr: bool = False,
                            packed: bool = True) -> Dict[int, Dict[Tuple[int, int, int], int]]:
        """A whole TIFF / OME-TIFF file -- what the ordinary PixelsService opens through
        Bio-Formats for an image without an NGFF fileset (config.yaml:18) -- in ONE set of GPU
        launches: every plane of every level (tiff_image_layout: OME-XML axes, or page k = t;
        each main IFD's SubIFDs are stored levels 1, 2, ... of its plane).  An IFD of S samples
        per pixel gives the S channels c .. c + S - 1: a chunky one is one layer, read and
        decoded once and split into its S planes on the GPU; a planar one S single-sample
        planes.  All are registered, or none.  Returns {level: {(z, c, t): plane id}}, as
        register_ngff_image.  j2k_packets (default on here, where whole files are served): JPEG
        2000 IFDs are read with tiff_plane_spec's keyword of that name.  j2k_chroma (default on
        here too) and aperio_ycbcr (off: the IFD does not say so): likewise.  packed (default on
        here too): bit-packed samples, PackBits and FillOrder 2 are read with tiff_plane_spec's
        keyword of that name."""
        lay = tiff_image_layout(path, j2k_packets, j2k_chroma, aperio_ycbcr, **({"packed": True} if packed else {}))

        def plane_spec(d, *a, **kw):  # (the keywords only where they mean something)
            if d["compression"] in _TIFF_J2K_COMPRESSIONS:
                kw.update({k: True for k, v in (("j2k_packets", j2k_packets), ("j2k_chroma", j2k_chroma),
                                                ("aperio_ycbcr", aperio_ycbcr)) if v})
            if packed and _tiff_needs_packed(d):
                kw["packed"] = True
            return tiff_plane_spec(path, d, *a, **kw)
        specs, keys = [], []
        for (z, c, t), ifd in zip(lay["planes"], lay["ifds"]):
            for k, d in enumerate([ifd] + ifd["subifds"]):
                first = plane_spec(d, image_id, z, c, t, k)
                for s in range(lay["samples"]):
                    if s == 0:
                        specs.append(first)
                    elif first["samples_per_pixel"] > 1:  # chunky: the same segments object, one layer
                        specs.append(dict(first, c=c + s, sample=s))
                    else:  # planar: the sample's own segments
                        specs.append(plane_spec(d, image_id, z, c + s, t, k, sample=s))
                    keys.append((k, (z, c + s, t)))
        ids = self.register_tiff_planes(specs)
        out: Dict[int, Dict[Tuple[int, int, int], int]] = {}
        for (k, p), pid in zip(keys, ids):
            out.setdefault(k, {})[p] = pid
        return out

    def release_plane(self, plane_id: int) -> None:
        _check(lib().pbx_plane_release(self._h, plane_id))

    # ---------------------------------------------------------------- plane residency
    def declare_image(self, pixels: "Pixels") -> None:
        """pbx_image_declare: the Pixels row (getPixels, TileRequestHandler.java:220-241) and
        the PixelBuffer's resolution level count, so that z/c/t/resolution outside the image
        answer the reference's 404 without loading anything."""
        d = PbxImageDesc(pixels.image_id, pixels.pixel_type, pixels.size_x, pixels.size_y,
                         pixels.size_z, pixels.size_c, pixels.size_t, pixels.levels, 0)
        _check(lib().pbx_image_declare(self._h, ctypes.byref(d)))

    def release_image(self, image_id: int) -> None:
        _check(lib().pbx_image_release(self._h, image_id))

    def create_plane(self, image_id: int, z: int, c: int, t: int, pixel_type: int, size_x: int,
                     size_y: int, level: int = 0, band: Optional[Tuple[int, int]] = None,
                     big_endian: bool = True, generator: Optional[str] = None, seed: int = 0,
                     plane_no: int = 0) -> int:
        """pbx_plane_create: allocate a plane, or only the row band (y0, rows) of it.  Host
        planes are filled with write_rows() and published by commit_plane(); generator
        planes are generated on the GPU and ready at once."""
        d = PbxPlaneDesc()
        d.image_id, d.z, d.c, d.t, d.resolution = image_id, z, c, t, level
        d.pixel_type, d.size_x, d.size_y = pixel_type, size_x, size_y
        d.byte_order = BIG_ENDIAN if big_endian else LITTLE_ENDIAN
        if generator is not None:
            d.source = {"fake": SRC_GEN_FAKE, "noise": SRC_GEN_NOISE}[generator]
            d.seed, d.plane_no = seed, plane_no
        y0, rows = band if band is not None else (0, 0)
        pid = ctypes.c_uint64()
        _check(lib().pbx_plane_create(self._h, ctypes.byref(d), y0, rows, ctypes.byref(pid)))
        return pid.value

    def write_rows(self, plane_id: int, y0: int, data) -> None:
        """pbx_plane_write_rows: packed rows (bytes or an array of rows x size_x samples, in
        the byte order given to create_plane) starting at plane row y0."""
        import numpy as np
        a = np.ascontiguousarray(data) if not isinstance(data, (bytes, bytearray, memoryview)) else \
            np.frombuffer(data, np.uint8)
        buf = a.view(np.uint8).reshape(-1)
        rows = a.shape[0] if a.ndim >= 2 else None
        if rows is None:
            raise ValueError("write_rows: pass a 2-D array of rows (or use write_rows_bytes)")
        _check(lib().pbx_plane_write_rows(self._h, plane_id, y0, rows, buf.ctypes.data, buf.nbytes))

    def write_rows_bytes(self, plane_id: int, y0: int, rows: int, data: bytes) -> None:
        buf = ctypes.create_string_buffer(bytes(data), len(data)) if not isinstance(data, bytes) else data
        _check(lib().pbx_plane_write_rows(self._h, plane_id, y0, rows, buf, len(data)))

    def commit_plane(self, plane_id: int) -> None:
        _check(lib().pbx_plane_commit(self._h, plane_id))

    def lookup_plane(self, image_id: int, z: int, c: int, t: int, level: int = 0):
        """(plane id, state, band_y0, band_rows) of the plane registered under a key, or None."""
        pid, st, y0, n = ctypes.c_uint64(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        r = lib().pbx_plane_lookup(self._h, image_id, z, c, t, level, ctypes.byref(pid),
                                   ctypes.byref(st), ctypes.byref(y0), ctypes.byref(n))
        if r == E_NOTFOUND:
            return None
        _check(r)
        return pid.value, st.value, y0.value, n.value

    def set_residency_budget(self, nbytes: int) -> None:
        """pbx_set_residency_budget: HBM for planes (0 = none); idle planes are evicted LRU."""
        _check(lib().pbx_set_residency_budget(self._h, nbytes))

    def residency_stats(self) -> Dict[str, int]:
        s = PbxResidencyStats()
        _check(lib().pbx_residency_stats_get(self._h, ctypes.byref(s)))
        return {n: getattr(s, n) for n, _ in PbxResidencyStats._fields_}

    # ------------------------------------------------------------- sparse (banded) planes
    def create_sparse_plane(self, image_id: int, z: int, c: int, t: int, pixel_type: int, size_x: int,
                            size_y: int, band_rows: int, level: int = 0,
                            own: Optional[Tuple[int, int]] = None, big_endian: bool = True,
                            generator: Optional[str] = None, seed: int = 0, plane_no: int = 0) -> int:
        """pbx_plane_create_sparse: a plane held as bands of `band_rows` rows, each loaded on
        demand (band_write) and evicted on its own; `own` = (y0, rows) limits the rows this
        context may hold (another context owns the rest)."""
        d = PbxPlaneDesc()
        d.image_id, d.z, d.c, d.t, d.resolution = image_id, z, c, t, level
        d.pixel_type, d.size_x, d.size_y = pixel_type, size_x, size_y
        d.byte_order = BIG_ENDIAN if big_endian else LITTLE_ENDIAN
        if generator is not None:
            d.source = {"fake": SRC_GEN_FAKE, "noise": SRC_GEN_NOISE}[generator]
            d.seed, d.plane_no = seed, plane_no
        y0, rows = own if own is not None else (0, 0)
        pid = ctypes.c_uint64()
        _check(lib().pbx_plane_create_sparse(self._h, ctypes.byref(d), band_rows, y0, rows, ctypes.byref(pid)))
        return pid.value

    def band_write(self, plane_id: int, y0: int, rows: int, data: Optional[bytes]) -> None:
        """pbx_band_write: rows [y0, y0 + rows) of one band (packed, the plane's byte order);
        data None generates them (generator planes)."""
        if data is None:
            _check(lib().pbx_band_write(self._h, plane_id, y0, rows, None, 0))
        else:
            _check(lib().pbx_band_write(self._h, plane_id, y0, rows, data, len(data)))

    def band_write_reduced(self, plane_id: int, y0: int, rows: int, src_plane_id: int, k: int) -> None:
        """pbx_band_write_reduced: rows [y0, y0 + rows) of one band of the sparse plane
        `plane_id` (stored level r + k), made on the GPU from the resident rows
        [y0 << k, min((y0 + rows) << k, size_y)) of plane `src_plane_id` (level r, the same image,
        z, c, t, pixel type and byte order): k = 1 .. 4 levels of 2x2 means in one kernel, bit for
        bit build_pyramid's.  E_NOT_RESIDENT: a source band that holds one of those rows is not
        resident (nothing was written or allocated); load it and call again."""
        _check(lib().pbx_band_write_reduced(self._h, plane_id, y0, rows, src_plane_id, k))

    def band_write_zarr(self, plane_id: int, y0: int, rows: int, chunk_x: int, chunk_y: int,
                        codec: Optional[str], chunks: Sequence[Optional[bytes]], fill_bits: int = 0,
                        timing: bool = False, chunk_planes: int = 1, slice: int = 0, crc32c: bool = False):
        """pbx_band_write_zarr: rows [y0, y0 + rows) of one band, decoded on the GPU from the
        Zarr chunk rows y0 // chunk_y .. ceil((y0 + rows) / chunk_y) - 1 that cover them (each
        full width, C order; None or b"" = missing chunk -> fill; or pack_chunks()' (data,
        offsets) pair).  codec and crc32c as register_zarr_plane.  With timing=True returns the decode /
        placement kernels' device ms.  chunk_planes > 1: the chunks hold that many planes and
        the rows are those of slice `slice` of each (pbx_band_write_zarr_deep)."""
        zc = PbxZarrChunks()
        kept = _fill_zarr_chunks(zc, dict(chunk_x=chunk_x, chunk_y=chunk_y, codec=codec, chunks=chunks,
                                          fill_bits=fill_bits, crc32c=crc32c))
        ms = (ctypes.c_double * 2)()
        if chunk_planes == 1 and slice == 0:
            _check(lib().pbx_band_write_zarr(self._h, plane_id, y0, rows, ctypes.byref(zc), ms))
        else:
            _check(lib().pbx_band_write_zarr_deep(self._h, plane_id, y0, rows, ctypes.byref(zc),
                                                  chunk_planes, slice, ms))
        del kept
        return (ms[0], ms[1]) if timing else None

    def band_write_tiff(self, plane_id: int, y0: int, rows: int, seg_w: int, seg_h: int, tiled: bool,
                        compression: int, predictor: int, segments, timing: bool = False,
                        samples_per_pixel: int = 1, sample: int = 0, jpeg: Optional[Mapping] = None,
                        j2k: bool = False, flags: int = 0, packed: Optional[Mapping] = None):
        """pbx_band_write_tiff: rows [y0, y0 + rows) of one band, decoded on the GPU from the TIFF
        segment rows y0 // seg_h .. ceil((y0 + rows) / seg_h) - 1 that cover them (strips, or
        rows of tiles at full width, C order: a sequence of bytes, or pack_chunks()' (data,
        offsets) pair, as tiff_band_spec returns).  compression and predictor as
        register_tiff_planes; the sparse plane must have been created in the file's byte order.
        With samples_per_pixel > 1 the segments are chunky and hold that many interleaved samples
        per pixel, of which only `sample` is written (pbx_band_write_tiff_sample).
        flags: a spec's `flags` (TIFF_F_J2K_PACKETS on JPEG 2000 segments).
        packed: a spec's `packed` dict (bits[, fill_order]): band_write_tiff_packed.
        With timing=True returns the decoders' and the placement's device ms."""
        if packed is not None:
            return self.band_write_tiff_packed(plane_id, y0, rows, seg_w, seg_h, tiled, compression, segments,
                                               packed["bits"], packed.get("fill_order", 1), samples_per_pixel,
                                               sample, predictor=predictor, flags=flags, timing=timing)
        s = PbxTiffSegments()
        kept = _fill_tiff_segments(s, dict(seg_w=seg_w, seg_h=seg_h, tiled=tiled, compression=compression,
                                           predictor=predictor, flags=flags, segments=segments))
        ms = (ctypes.c_double * 2)()
        if j2k:  # JPEG 2000 segments (compression TIFF_J2K): a spec's `j2k`
            _check(lib().pbx_band_write_tiff_j2k(self._h, plane_id, y0, rows, ctypes.byref(s), samples_per_pixel,
                                                 sample, ms))
        elif jpeg is not None:  # JPEG segments (compression 7): a spec's `jpeg` dict, tables and ycbcr
            j = PbxTiffJpeg()
            keep = _fill_tiff_jpeg(j, jpeg)
            _check(lib().pbx_band_write_tiff_jpeg(self._h, plane_id, y0, rows, ctypes.byref(s), samples_per_pixel,
                                                  sample, ctypes.byref(j), ms))
            del keep
        elif samples_per_pixel == 1 and sample == 0:
            _check(lib().pbx_band_write_tiff(self._h, plane_id, y0, rows, ctypes.byref(s), ms))
        else:
            _check(lib().pbx_band_write_tiff_sample(self._h, plane_id, y0, rows, ctypes.byref(s),
                                                    samples_per_pixel, sample, ms))
        del kept
        return [ms[0], ms[1]] if timing else None

    def band_write_tiff_packed(self, plane_id: int, y0: int, rows: int, seg_w: int, seg_h: int, tiled: bool,
                               compression: int, segments, bits: int, fill_order: int = 1,
                               samples_per_pixel: int = 1, sample: int = 0, predictor: int = 1, flags: int = 0,
                               timing: bool = False):
        """pbx_band_write_tiff_packed: band_write_tiff for segment rows of bit-packed samples
        (bits 1 .. 16, MSB first, every row padded to a byte; fill_order 2: the bits of every
        byte reversed) under compression 1, 5, 8, 50000 or TIFF_PACKBITS.  Of samples_per_pixel
        chunky samples only `sample` is written.  With timing=True returns the decoders' and the
        placement's device ms."""
        s = PbxTiffSegments()
        kept = _fill_tiff_segments(s, dict(seg_w=seg_w, seg_h=seg_h, tiled=tiled, compression=compression,
                                           predictor=predictor, flags=flags, segments=segments))
        k = PbxTiffPacked()
        _fill_tiff_packed(k, dict(bits=bits, fill_order=fill_order), samples_per_pixel, sample)
        ms = (ctypes.c_double * 2)()
        _check(lib().pbx_band_write_tiff_packed(self._h, plane_id, y0, rows, ctypes.byref(s), ctypes.byref(k), ms))
        del kept
        return [ms[0], ms[1]] if timing else None

    @staticmethod
    def _group_args(plane_ids: Sequence[int], primary: int):
        """What the group calls refuse before they reach the library (the library refuses the
        same with the same status): returns the ids as a C array."""
        ids = [int(p) for p in plane_ids]
        n = len(ids)
        if not 1 <= n <= 4:
            raise PbxError(E_BADARG, "group of %d planes outside 1 .. 4" % n)
        if not 0 <= primary < n:
            raise PbxError(E_BADARG, "primary %d outside the group of %d" % (primary, n))
        if not ids[primary]:
            raise PbxError(E_BADARG, "primary %d names plane id 0 (nobody wants that member)" % primary)
        for i in range(n):
            if ids[i] and ids[i] in ids[:i]:
                raise PbxError(E_BADARG, "plane %d is members %d and %d of the group" % (ids[i], ids.index(ids[i]), i))
        return (ctypes.c_uint64 * n)(*ids)

    def _group_result(self, status: int, st, ms):
        """(statuses, kernel_ms) of a group call, or its PbxError carrying `statuses`."""
        if status != OK:
            e = PbxError(status, lib().pbx_last_error().decode(errors="replace"))
            e.statuses = list(st)
            raise e
        return list(st), [ms[0], ms[1]]

    def band_write_tiff_group(self, plane_ids: Sequence[int], primary: int, y0: int, rows: int, seg_w: int,
                              seg_h: int, tiled: bool, compression: int, predictor: int, segments,
                              jpeg: Optional[Mapping] = None, j2k: bool = False, flags: int = 0,
                              packed: Optional[Mapping] = None):
        """pbx_band_write_tiff_group: band_write_tiff of rows [y0, y0 + rows) into the bands of
        all the planes of chunky segments at once, from ONE upload and decode.  plane_ids[s] is
        the sparse plane of sample s (len(plane_ids) = the segments' samples per pixel, 0 = nobody
        wants that sample); plane_ids[primary] is the plane the caller needs, the others are
        filled if they can be.  The other arguments are band_write_tiff's.  Returns (statuses,
        kernel_ms): per member OK (written), 409 / 500 / 507 (kept out), -1 (id 0); raises what
        band_write_tiff of the primary alone would have raised (the PbxError's `statuses`
        attribute then holds the members')."""
        ids = self._group_args(plane_ids, primary)
        n = len(ids)
        s = PbxTiffSegments()
        kept = _fill_tiff_segments(s, dict(seg_w=seg_w, seg_h=seg_h, tiled=tiled, compression=compression,
                                           predictor=predictor, flags=flags, segments=segments))
        j = k = None
        if jpeg is not None:
            j = PbxTiffJpeg()
            kept.append(_fill_tiff_jpeg(j, jpeg))
        if packed is not None:
            k = PbxTiffPacked()
            _fill_tiff_packed(k, packed, n, 0)
        st, ms = (ctypes.c_int32 * n)(), (ctypes.c_double * 2)()
        status = lib().pbx_band_write_tiff_group(self._h, ids, n, primary, y0, rows, ctypes.byref(s),
                                                 ctypes.byref(j) if j is not None else None, 1 if j2k else 0,
                                                 ctypes.byref(k) if k is not None else None, st, ms)
        del kept
        return self._group_result(status, st, ms)

    def band_write_zarr_group(self, plane_ids: Sequence[int], slices: Sequence[int], primary: int, y0: int,
                              rows: int, chunk_x: int, chunk_y: int, codec: Optional[str],
                              chunks: Sequence[Optional[bytes]], fill_bits: int = 0, chunk_planes: int = 1,
                              crc32c: bool = False):
        """pbx_band_write_zarr_group: band_write_zarr of rows [y0, y0 + rows) into the bands of up
        to four planes that the same chunks hold, from ONE upload and decode: plane_ids[i]
        receives slice slices[i] (distinct, in [0, chunk_planes)).  primary, the result and the
        error as band_write_tiff_group; the other arguments are band_write_zarr's."""
        ids = self._group_args(plane_ids, primary)
        n = len(ids)
        sl = [int(v) for v in slices]
        if len(sl) != n:
            raise PbxError(E_BADARG, "%d slices for a group of %d planes" % (len(sl), n))
        for i in range(n):
            if sl[i] in sl[:i]:
                raise PbxError(E_BADARG, "slice %d is members %d and %d of the group" % (sl[i], sl.index(sl[i]), i))
        zc = PbxZarrChunks()
        kept = _fill_zarr_chunks(zc, dict(chunk_x=chunk_x, chunk_y=chunk_y, codec=codec, chunks=chunks,
                                          fill_bits=fill_bits, crc32c=crc32c))
        st, ms = (ctypes.c_int32 * n)(), (ctypes.c_double * 2)()
        status = lib().pbx_band_write_zarr_group(self._h, ids, (ctypes.c_int32 * n)(*sl), n, primary, y0, rows,
                                                 ctypes.byref(zc), chunk_planes, st, ms)
        del kept
        return self._group_result(status, st, ms)

    def band_abort(self, plane_id: int, y0: int) -> None:
        """pbx_band_abort: give back the band holding row y0 when its load is abandoned."""
        _check(lib().pbx_band_abort(self._h, plane_id, y0))

    def band_info(self, plane_id: int) -> Tuple[int, List[int]]:
        """(band_rows, [state of band k]) of a sparse plane (BS_ABSENT / BS_LOADING / BS_READY)."""
        br, nb = ctypes.c_int32(), ctypes.c_int32()
        _check(lib().pbx_plane_band_info(self._h, plane_id, ctypes.byref(br), ctypes.byref(nb), None))
        st = (ctypes.c_uint8 * max(nb.value, 1))()
        _check(lib().pbx_plane_band_info(self._h, plane_id, ctypes.byref(br), ctypes.byref(nb), st))
        return br.value, list(st)[:nb.value]

    def test_fail_batch(self, ahead: int) -> None:
        """Fault injection: the `ahead`-th batch launched from now on fails (500s); 0 = off."""
        _check(lib().pbx_test_fail_batch(self._h, ahead))

    def test_fail_band_write(self, ahead: int) -> None:
        """Upload failure injection: the `ahead`-th band write from now on fails; 0 = off."""
        _check(lib().pbx_test_fail_band_write(self._h, ahead))

    def test_stall_batch(self, ahead: int) -> None:
        """Stall injection: the `ahead`-th batch launched from now on does not complete until
        test_stall_batch(0) releases it (its callers get 500 at their deadline)."""
        _check(lib().pbx_test_stall_batch(self._h, ahead))

    # ------------------------------------------------------------- opening planes on demand
    def _exclusive(self, key):
        """Context manager: one loader per key (plane, or (plane, band)); the lock entry goes
        with its last user."""
        import contextlib
        import threading

        @contextlib.contextmanager
        def cm():
            with self._load_lock:
                ent = self._loading.get(key)
                if ent is None:
                    ent = self._loading[key] = [threading.Lock(), 0]
                ent[1] += 1
            try:
                with ent[0]:
                    yield
            finally:
                with self._load_lock:
                    ent[1] -= 1
                    if ent[1] == 0:
                        del self._loading[key]
        return cm()

    def load_plane(self, source: "PixelSource", pixels: "Pixels", z: int, c: int, t: int,
                   level: int = 0, band: Optional[Tuple[int, int]] = None,
                   band_bytes: int = 64 << 20, timeout_s: float = 60.0) -> int:
        """Open a plane this context does not hold, as getPixelBuffer + getTileDirect would
        (TileRequestHandler.java:86,107-109,201-211): declare the image, create the plane (or
        only `band` = (y0, rows) of it), stream its rows from `source` in bands of about
        `band_bytes`, commit.  If another caller is loading the same key, wait for it."""
        self.declare_image(pixels)
        key = (pixels.image_id, z, c, t, level)
        if _derived_from(source, pixels, level, 1) is not None:
            # a level the source does not store: the last stored level whole, then every derived
            # level at once (build_pyramid), under the stored level's lock
            if band is not None:
                raise PbxError(E_BADARG, "derived levels are not sharded by rows")
            found = self.lookup_plane(*key)
            if found is not None and found[1] == PS_READY:
                return found[0]
            last = source.stored_levels(pixels) - 1
            base = self.load_plane(source, pixels, z, c, t, last, None, band_bytes, timeout_s)
            with self._exclusive(key[:4] + (last,)):
                found = self.lookup_plane(*key)
                if found is not None and found[1] == PS_READY:
                    return found[0]
                try:
                    return self.build_pyramid(base, pixels.levels - 1 - last)[level - last - 1]
                except PbxError as e:
                    if e.status != E_EXISTS:
                        raise
                    found = self.lookup_plane(*key)  # another context user built them
                    if found is None:  # levels partly built, or released in between
                        raise PbxError(E_INTERNAL, "level %d of Image:%d z=%d c=%d t=%d: some derived level is "
                                       "registered, this one is not" % (level, pixels.image_id, z, c, t))
                    return found[0]
        with self._exclusive(key):
            found = self.lookup_plane(*key)
            if found is not None and found[1] == PS_READY:
                return found[0]
            segments = getattr(source, "plane_segments", None)
            sp = segments(pixels, z, c, t, level) if segments is not None and band is None else None
            if sp is not None:  # a TIFF plane: its strips or tiles, decoded on the GPU
                try:
                    return self.register_tiff_planes([sp])[0]
                except PbxError as e:
                    if e.status != E_EXISTS:
                        raise
                    found = self.lookup_plane(*key)  # another context user registered it
                    return found[0] if found is not None else 0
            sx, sy = source.level_size(pixels, level)
            y0, rows = band if band is not None else (0, sy)
            try:
                pid = self.create_plane(pixels.image_id, z, c, t, pixels.pixel_type, sx, sy, level,
                                        band=(y0, rows), big_endian=True)
            except PbxError as e:
                if e.status != E_EXISTS:
                    raise
                deadline = time.monotonic() + timeout_s  # another context user loads it
                while time.monotonic() < deadline:
                    found = self.lookup_plane(*key)
                    if found is None or found[1] != PS_FILLING:
                        return found[0] if found is not None else 0
                    time.sleep(0.001)
                raise
            step = max(1, band_bytes // max(1, sx * BYTES_PER_PIXEL[pixels.pixel_type]))
            try:
                for r in range(y0, y0 + rows, step):
                    n = min(step, y0 + rows - r)
                    self.write_rows_bytes(pid, r, n, source.read_rows(pixels, z, c, t, level, r, n))
                self.commit_plane(pid)
            except BaseException:
                self.release_plane(pid)
                raise
            return pid

    def _sparse_plane(self, source: "PixelSource", pixels: "Pixels", z: int, c: int, t: int, level: int,
                      sx: int, sy: int, own: Optional[Tuple[int, int]], big_endian: Optional[bool] = None) -> int:
        """The sparse plane of the key, created if absent or evicted (bands of
        self.sparse_band_rows rows, in the source's byte order: `big_endian`, or asked of the
        source), under the key's lock."""
        key = (pixels.image_id, z, c, t, level)
        with self._exclusive(key):
            found = self.lookup_plane(*key)
            if found is not None and found[1] != PS_EVICTED:
                return found[0]
            if big_endian is None:
                band_chunks = getattr(source, "band_chunks", None)
                band_segments = getattr(source, "band_segments", None)
                # chunks stay in the array's byte order (no rows: nothing is read for this)
                sp = band_chunks(pixels, z, c, t, level, 0, 0) if band_chunks is not None else None
                if sp is None and band_segments is not None:  # segments stay in the file's byte order
                    sp = band_segments(pixels, z, c, t, level, 0, 0)
                big_endian = sp["big_endian"] if sp is not None else True
            try:
                return self.create_sparse_plane(pixels.image_id, z, c, t, pixels.pixel_type, sx, sy,
                                                self.sparse_band_rows, level, own=own, big_endian=big_endian)
            except PbxError as e:
                if e.status != E_EXISTS:
                    raise
                return self.lookup_plane(*key)[0]

    def _sibling_group(self, source: "PixelSource", pixels: "Pixels", z: int, c: int, t: int, level: int,
                       sx: int, sy: int, own: Optional[Tuple[int, int]], pid: int, B: int) -> Optional[dict]:
        """fill_siblings: the planes that share the segments or chunks of plane `pid` = (z, c, t),
        looked up or created like it, as the arguments of the group calls -- ids (and slices)
        and primary -- or None when the source's spec has no shared siblings (single-sample and
        planar TIFF, one plane per Zarr chunk, rows only).  Siblings that are not sparse planes
        of the primary's bands and owned rows are left out.  Each key's lock is taken on its own,
        never inside another."""
        band_chunks = getattr(source, "band_chunks", None)
        band_segments = getattr(source, "band_segments", None)
        sp = band_chunks(pixels, z, c, t, level, 0, 0) if band_chunks is not None else None
        tsp = band_segments(pixels, z, c, t, level, 0, 0) if sp is None and band_segments is not None else None
        chans: Dict[int, int] = {}  # member (TIFF: sample, Zarr: slice) -> channel
        if tsp is not None and tsp.get("samples_per_pixel", 1) > 1:
            # chunky samples: channel c - sample + s is sample s
            chans = {s: c - tsp.get("sample", 0) + s for s in range(tsp["samples_per_pixel"])}
            mine, big = tsp.get("sample", 0), tsp["big_endian"]
        elif sp is not None and sp.get("chunk_planes", 1) > 1 and sp.get("layer") is not None:
            # the neighbours along the channel axis whose chunks are the primary's (at most 3)
            for step in (-1, 1):
                cc = c + step
                while 0 <= cc < pixels.size_c and len(chans) < 3:
                    try:
                        o = band_chunks(pixels, z, cc, t, level, 0, 0)
                    except PbxError:
                        break
                    if (o is None or o.get("chunk_planes") != sp["chunk_planes"] or
                            (o.get("layer") or ())[:2] != sp["layer"][:2]):
                        break
                    chans[o["slice"]] = cc
                    cc += step
            mine, big = sp["slice"], sp["big_endian"]
            chans[mine] = c
        else:
            return None
        held = self.lookup_plane(pixels.image_id, z, c, t, level)
        ids = {mine: pid}
        for m, cc in chans.items():
            if m == mine or not 0 <= cc < pixels.size_c:
                continue
            try:
                q = self._sparse_plane(source, pixels, z, cc, t, level, sx, sy, own, big)
                if self.band_info(q)[0] != B or self.lookup_plane(pixels.image_id, z, cc, t, level)[2:] != held[2:]:
                    continue
            except (PbxError, TypeError):  # not a sparse plane, or released meanwhile
                continue
            ids[m] = q
        if len(ids) < 2:
            return None
        if tsp is not None:
            return dict(ids=[ids.get(s, 0) for s in range(len(chans))], primary=mine)
        order = [mine] + sorted(m for m in ids if m != mine)
        return dict(ids=[ids[m] for m in order], slices=order, primary=0)

    def load_bands(self, source: "PixelSource", pixels: "Pixels", z: int, c: int, t: int, level: int,
                   y: int, h: int, own: Optional[Tuple[int, int]] = None,
                   timeout_s: float = 60.0, siblings: Optional[bool] = None) -> int:
        """Region-proportional loading (TileRequestHandler.java:102-109 reads only the region):
        the sparse plane of the key (created if absent, bands of self.sparse_band_rows rows) gets
        the bands that rows [y, y + h) cover, each read from `source` once; bands another
        caller is loading are waited for.  A source with chunk-level access
        (PixelSource.band_chunks) hands over the Zarr chunk rows covering each band, which are
        decoded on the GPU (band_write_zarr); one with segment-level access
        (PixelSource.band_segments) the TIFF strips or tile rows (band_write_tiff); any other
        source is read with read_rows.  siblings (None: the service's fill_siblings): the planes
        that share those segments or chunks -- the other samples of chunky TIFF segments, the
        other channels of Zarr chunks that hold several -- are looked up or created too and
        every absent band of this plane is loaded by one group call that fills theirs from the
        same decode, if they can be (band_write_tiff_group / band_write_zarr_group).  Returns
        the plane id.
        A level the source does not store (DerivedLevels) is made from the level reduce_step above
        it (_load_derived_bands)."""
        self.declare_image(pixels)
        key = (pixels.image_id, z, c, t, level)
        sx, sy = source.level_size(pixels, level)
        derived = _derived_from(source, pixels, level, self.reduce_step)
        if derived is not None:
            if own is not None:
                raise PbxError(E_BADARG, "derived levels are not sharded by rows")
            return self._load_derived_bands(source, pixels, z, c, t, level, y, h, timeout_s, *derived)
        band_chunks = getattr(source, "band_chunks", None)
        band_segments = getattr(source, "band_segments", None)
        pid = self._sparse_plane(source, pixels, z, c, t, level, sx, sy, own)
        B, states = self.band_info(pid)
        # every band the rows cover: the owned ones, and the guest bands past the owned rows that
        # a region starting in them covers (the reference's getTileDirect serves any region)
        y0, y1 = max(y, 0), min(y + h, sy)
        bands = [k for k in (range(y0 // B, (y1 + B - 1) // B) if y1 > y0 else ()) if states[k] != BS_READY]
        group = None
        if bands and (self.fill_siblings if siblings is None else siblings):
            group = self._sibling_group(source, pixels, z, c, t, level, sx, sy, own, pid, B)
        for k in bands:
            with self._exclusive(key + (k,)):
                deadline = time.monotonic() + timeout_s
                while True:
                    st = self.band_info(pid)[1][k]
                    if st == BS_READY:
                        break
                    if st == BS_ABSENT:
                        r0, r1 = k * B, min((k + 1) * B, sy)
                        try:
                            sp = (band_chunks(pixels, z, c, t, level, r0, r1 - r0)
                                  if band_chunks is not None else None)
                            tsp = (band_segments(pixels, z, c, t, level, r0, r1 - r0)
                                   if sp is None and band_segments is not None else None)
                            if tsp is not None and group is not None:
                                self.band_write_tiff_group(group["ids"], group["primary"], r0, r1 - r0,
                                                           tsp["seg_w"], tsp["seg_h"], tsp["tiled"],
                                                           tsp["compression"], tsp["predictor"], tsp["segments"],
                                                           jpeg=tsp.get("jpeg"), j2k=bool(tsp.get("j2k")),
                                                           flags=tsp.get("flags", 0), packed=tsp.get("packed"))
                            elif tsp is not None:
                                self.band_write_tiff(pid, r0, r1 - r0, tsp["seg_w"], tsp["seg_h"],
                                                     tsp["tiled"], tsp["compression"], tsp["predictor"],
                                                     tsp["segments"],
                                                     samples_per_pixel=tsp.get("samples_per_pixel", 1),
                                                     sample=tsp.get("sample", 0),
                                                     **({"jpeg": tsp["jpeg"]} if tsp.get("jpeg") is not None else {}),
                                                     **({"j2k": True} if tsp.get("j2k") else {}),
                                                     **({"flags": tsp["flags"]} if tsp.get("flags") else {}),
                                                     **({"packed": tsp["packed"]} if tsp.get("packed") is not None
                                                        else {}))
                            elif sp is not None and group is not None:
                                self.band_write_zarr_group(group["ids"], group["slices"], group["primary"], r0,
                                                           r1 - r0, sp["chunk_x"], sp["chunk_y"], sp["codec"],
                                                           sp["chunks"], sp["fill_bits"],
                                                           chunk_planes=sp["chunk_planes"],
                                                           crc32c=sp.get("crc32c", False))
                            elif sp is not None:
                                self.band_write_zarr(pid, r0, r1 - r0, sp["chunk_x"], sp["chunk_y"],
                                                     sp["codec"], sp["chunks"], sp["fill_bits"],
                                                     chunk_planes=sp.get("chunk_planes", 1),
                                                     slice=sp.get("slice", 0), crc32c=sp.get("crc32c", False))
                            else:
                                self.band_write(pid, r0, r1 - r0,
                                                source.read_rows(pixels, z, c, t, level, r0, r1 - r0))
                            break
                        except PbxError as e:
                            sts = getattr(e, "statuses", None)
                            if group is not None and sts is not None and sts[group["primary"]] == -1:
                                # refused before the primary was attempted (a sibling released,
                                # evicted or replaced meanwhile, or the piece's own fault): siblings
                                # are best effort, the single call decides
                                group = None
                                continue
                            if e.status != E_EXISTS:  # another binding loads it: wait
                                raise
                    if time.monotonic() > deadline:
                        raise PbxError(E_INTERNAL, "band %d of plane %d: timed out loading" % (k, pid))
                    time.sleep(0.001)
        return pid

    def _level_big_endian(self, source: "PixelSource", pixels: "Pixels", z: int, c: int, t: int, level: int) -> bool:
        """The byte order load_bands keeps a level's sparse plane in: the chunks' or segments' of
        a stored level, rows big-endian; a derived level has its last stored level's."""
        if _derived_from(source, pixels, level, 1) is not None:
            level = source.stored_levels(pixels) - 1
        sp = None
        for name in ("band_chunks", "band_segments"):
            f = getattr(source, name, None)
            sp = f(pixels, z, c, t, level, 0, 0) if sp is None and f is not None else sp
        return sp["big_endian"] if sp is not None else True

    def _load_derived_bands(self, source: "PixelSource", pixels: "Pixels", z: int, c: int, t: int, level: int,
                            y: int, h: int, timeout_s: float, src_level: int, k: int) -> int:
        """load_bands for a level the source does not store: every absent band [r0, r1) the rows
        cover gets the rows [r0 << k, min(r1 << k, size_y)) of `src_level` = level - k loaded
        (load_bands again: a derived source level becomes a sparse plane of its own, whose bands
        the neighbours reuse) and is then made from them on the GPU (band_write_reduced).  A
        source band evicted between the two is loaded again, LOAD_ATTEMPTS times at most.
        fill_siblings is ignored here, for the stored source level's bands too: what a derived
        request loads is its own channel's rows."""
        key = (pixels.image_id, z, c, t, level)
        sx, sy = source.level_size(pixels, level)
        ssy = source.level_size(pixels, src_level)[1]
        pid = self._sparse_plane(source, pixels, z, c, t, level, sx, sy, None,
                                 self._level_big_endian(source, pixels, z, c, t, level))
        B, states = self.band_info(pid)
        y0, y1 = max(y, 0), min(y + h, sy)
        for kb in (range(y0 // B, (y1 + B - 1) // B) if y1 > y0 else ()):
            if states[kb] == BS_READY:
                continue
            with self._exclusive(key + (kb,)):
                deadline, attempts = time.monotonic() + timeout_s, 0
                while True:
                    st = self.band_info(pid)[1][kb]
                    if st == BS_READY:
                        break
                    if st == BS_ABSENT:
                        r0, r1 = kb * B, min((kb + 1) * B, sy)
                        if attempts >= TileRequestHandler.LOAD_ATTEMPTS:
                            raise PbxError(E_INTERNAL, "band %d of plane %d: its source rows could not be held "
                                           "resident (residency budget smaller than the working set)" % (kb, pid))
                        attempts += 1
                        s0, s1 = r0 << k, min(r1 << k, ssy)
                        src = self.load_bands(source, pixels, z, c, t, src_level, s0, s1 - s0,
                                              timeout_s=timeout_s, siblings=False)
                        try:
                            self.band_write_reduced(pid, r0, r1 - r0, src, k)
                            break
                        except PbxError as e:
                            if e.status == E_NOT_RESIDENT:  # a source band was evicted in between
                                continue
                            if e.status != E_EXISTS:  # another binding makes it: wait
                                raise
                    if time.monotonic() > deadline:
                        raise PbxError(E_INTERNAL, "band %d of plane %d: timed out loading" % (kb, pid))
                    time.sleep(0.001)
        return pid

    def build_pyramid(self, plane_id: int, levels: int, timing: bool = False):
        """Stored levels r+1 .. r+levels of a plane, built on the GPU (2x2 box means);
        returns their plane ids (and the kernels' device ms with timing=True).  With L
        stored levels, tiles of stored level k are TileCtx(..., resolution=L-1-k) (OMERO's
        numbering, include/pbx.h)."""
        ids = (ctypes.c_uint64 * max(levels, 1))()
        ms = ctypes.c_double(0.0)
        _check(lib().pbx_plane_build_pyramid(self._h, plane_id, levels, ids, ctypes.byref(ms)))
        return (list(ids)[:levels], ms.value) if timing else list(ids)[:levels]

    def read_plane_be(self, plane_id: int, nbytes: int) -> bytes:
        buf = ctypes.create_string_buffer(nbytes)
        _check(lib().pbx_plane_read_be(self._h, plane_id, buf, nbytes))
        return buf.raw

    def synchronize(self) -> None:
        _check(lib().pbx_device_synchronize(self._h))

    def set_deflate_strategy(self, strategy: int) -> None:
        """Deflate strategy of the batches planned from now on (pbx_set_deflate_strategy)."""
        _check(lib().pbx_set_deflate_strategy(self._h, strategy))

    @property
    def deflate_strategy(self) -> int:
        v = ctypes.c_int32()
        _check(lib().pbx_get_deflate_strategy(self._h, ctypes.byref(v)))
        return v.value

    def set_tiff_predictor(self, predictor: int) -> None:
        """TIFF predictor of the batches planned from now on (pbx_set_tiff_predictor)."""
        _check(lib().pbx_set_tiff_predictor(self._h, predictor))

    @property
    def tiff_predictor(self) -> int:
        v = ctypes.c_int32()
        _check(lib().pbx_get_tiff_predictor(self._h, ctypes.byref(v)))
        return v.value

    def set_kernel_streams(self, streams: int, stagger: int = 1) -> None:
        """Kernel streams for pipelined batches (pbx_set_kernel_streams); 1 = serial."""
        _check(lib().pbx_set_kernel_streams(self._h, streams, stagger))

    def release_cached(self) -> None:
        """Free cached batch buffers (device and pinned) no live batch uses."""
        _check(lib().pbx_release_cached(self._h))

    # One getTile (pbx_get_tile): safe to call from many threads at once; concurrent
    # calls are coalesced into batches by the library (ctypes releases the GIL).
    def get_tile(self, ctx: TileCtx, spans: Optional[dict] = None) -> Tuple[int, Optional[bytes]]:
        """(status, body).  ``spans``: a dict that receives the serving batch's stage timings
        (pbx_result_spans: get_tile_direct_ms, write_image_ms, create_metadata_ms, batch_ms,
        d2h_ms, batch_tiles) when the request has a body."""
        req = ctx.to_req()
        res = PbxResult()
        lib().pbx_get_tile(self._h, ctypes.byref(req), ctypes.byref(res))
        try:
            body = ctypes.string_at(res.data, res.len) if res.status == OK and res.len else (
                b"" if res.status == OK else None)
            ctx.region["width"], ctx.region["height"] = res.w, res.h
            if spans is not None and res.owner:
                sp = PbxSpans()
                if lib().pbx_result_spans(ctypes.byref(res), ctypes.byref(sp)) == OK:
                    spans.update({f: getattr(sp, f) for f, _ in PbxSpans._fields_})
        finally:
            lib().pbx_results_release(self._h, ctypes.byref(res), 1)
        return res.status, body

    def ctx_stats(self) -> Tuple[int, int]:
        """(batches launched, requests served) so far."""
        b, r = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().pbx_ctx_stats_get(self._h, ctypes.byref(b), ctypes.byref(r)))
        return b.value, r.value

    # Batched getTile: one set of GPU launches for many requests.
    def get_tiles(self, ctxs: Sequence[TileCtx]) -> List[Tuple[int, Optional[bytes]]]:
        n = len(ctxs)
        reqs = (PbxTileReq * max(n, 1))(*[c.to_req() for c in ctxs])
        res = (PbxResult * max(n, 1))()
        st = lib().pbx_get_tiles(self._h, reqs, n, res)
        out = []
        try:
            for i in range(n):
                r = res[i]
                body = ctypes.string_at(r.data, r.len) if r.status == OK and r.len else (
                    b"" if r.status == OK else None)
                ctxs[i].region["width"], ctxs[i].region["height"] = r.w, r.h
                out.append((r.status, body))
        finally:
            lib().pbx_results_release(self._h, res, n)
        if st != OK and not out:
            _check(st)
        return out


    # Batched async: submit returns at once, Ticket.wait() collects (pbx_submit / pbx_wait).
    def submit(self, ctxs: Sequence[TileCtx]) -> "Ticket":
        return Ticket(self, ctxs)


class PixelsNode:
    """N device contexts in ONE process (pbx_node_*): the reference runs all its worker
    verticles in one JVM (PixelBufferMicroserviceVerticle.java:117-118,224-233), so a node-wide
    drop-in holds one context per GPU and routes every getTile to the context holding its plane
    or row band, or (planes replicated on every GPU) to the pbx_shard_of owner among them.
    ``services[k]`` is context k as a PixelsService (register planes / bands there).  The same
    device may be listed several times (tests run two contexts on one GPU)."""

    def __init__(self, n: int, devices: Optional[Sequence[int]] = None, shard_tile: int = 512, **config):
        L = lib()
        cfg = make_config(**config)
        devs = (ctypes.c_int32 * n)(*devices) if devices is not None else None
        h = ctypes.c_void_p()
        _check(L.pbx_node_init(ctypes.byref(cfg), n, devs, shard_tile, ctypes.byref(h)))
        self._h = h
        self.services = [PixelsService(_handle=L.pbx_node_context(h, k)) for k in range(n)]
        if config.get("deflate_strategy") is not None:
            for s in self.services:
                s.set_deflate_strategy(config["deflate_strategy"])
        if config.get("tiff_predictor") is not None:
            for s in self.services:
                s.set_tiff_predictor(config["tiff_predictor"])

    def route(self, ctx: TileCtx) -> Tuple[int, int]:
        """(status the serving context would answer, its index); E_NOT_RESIDENT -> the index is
        the shard owner, where the binding should load the plane."""
        req = ctx.to_req()
        k = ctypes.c_int32()
        st = lib().pbx_node_route(self._h, ctypes.byref(req), ctypes.byref(k))
        if st == E_BADARG:
            _check(st)
        return st, k.value

    def get_tile(self, ctx: TileCtx) -> Tuple[int, Optional[bytes], int]:
        """(status, body, index of the context that served it)."""
        req = ctx.to_req()
        res = PbxResult()
        k = ctypes.c_int32(-1)
        lib().pbx_node_get_tile(self._h, ctypes.byref(req), ctypes.byref(res), ctypes.byref(k))
        try:
            body = ctypes.string_at(res.data, res.len) if res.status == OK and res.len else (
                b"" if res.status == OK else None)
            ctx.region["width"], ctx.region["height"] = res.w, res.h
        finally:
            lib().pbx_results_release(None, ctypes.byref(res), 1)
        return res.status, body, k.value

    def close(self) -> None:
        if self._h:
            for s_ in self.services:
                s_._h = None
            lib().pbx_node_shutdown(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Ticket:
    """A submitted batch of getTile requests (pbx_submit); wait() returns what get_tiles would."""

    def __init__(self, service: PixelsService, ctxs: Sequence[TileCtx]):
        self.service, self.ctxs, self.n = service, list(ctxs), len(ctxs)
        self._reqs = make_reqs(self.ctxs)
        self._res = (PbxResult * max(self.n, 1))()
        h = ctypes.c_void_p()
        _check(lib().pbx_submit(service._h, self._reqs, self.n, self._res, ctypes.byref(h)))
        self._t = h

    def wait(self, timeout_us: int = -1) -> Optional[List[Tuple[int, Optional[bytes]]]]:
        """Results, or None if the batch is still running after timeout_us (then call again)."""
        if self._t is None:
            raise RuntimeError("pbx: ticket already collected")
        st = lib().pbx_wait(self.service._h, self._t, timeout_us)
        if st == E_PENDING:
            return None
        self._t = None
        out = []
        try:
            for i in range(self.n):
                r = self._res[i]
                body = ctypes.string_at(r.data, r.len) if r.status == OK and r.len else (
                    b"" if r.status == OK else None)
                self.ctxs[i].region["width"], self.ctxs[i].region["height"] = r.w, r.h
                out.append((r.status, body))
        finally:
            lib().pbx_results_release(self.service._h, self._res, self.n)
        if st != OK and not out:
            _check(st)
        return out


def make_reqs(ctxs: Sequence[TileCtx]):
    """ctypes array of pbx_tile_req for a request list (reusable across batches)."""
    return (PbxTileReq * max(len(ctxs), 1))(*[c.to_req() for c in ctxs]) if ctxs else \
        (PbxTileReq * 1)()


class Batch:
    """Device-resident batch (plan once, launch many): outputs stay in HBM until fetch()."""

    def __init__(self, service: PixelsService, ctxs: Sequence[TileCtx] = (), reqs=None):
        """``ctxs``: TileCtx requests; or ``reqs``: a prebuilt ``make_reqs`` array."""
        self.service = service
        if reqs is None:
            self.n = len(ctxs)
            reqs = make_reqs(ctxs)
        else:
            self.n = len(reqs)
        self._reqs = reqs
        h = ctypes.c_void_p()
        _check(lib().pbx_batch_plan(service.handle, self._reqs, self.n, ctypes.byref(h)))
        self._h = h

    def launch(self) -> None:
        _check(lib().pbx_batch_launch(self.service.handle, self._h))

    def sync(self) -> None:
        _check(lib().pbx_batch_sync(self.service.handle, self._h))

    def stats(self) -> PbxBatchStats:
        s = PbxBatchStats()
        _check(lib().pbx_batch_stats_get(self.service.handle, self._h, ctypes.byref(s)))
        return s

    def fetch(self) -> List[Tuple[int, Optional[bytes]]]:
        res = (PbxResult * max(self.n, 1))()
        _check(lib().pbx_batch_fetch(self.service.handle, self._h, res))
        try:
            return [(res[i].status, ctypes.string_at(res[i].data, res[i].len)
                     if res[i].status == OK else None) for i in range(self.n)]
        finally:
            lib().pbx_results_release(self.service.handle, res, self.n)

    def lz77_records(self, nseg: int, hist_words: int, mrec_words: int):
        """Test hook: (hist, mrec) uint32 arrays of every segment from k_lz77."""
        import numpy as np
        h = np.zeros(nseg * hist_words, np.uint32)
        m = np.zeros(nseg * mrec_words, np.uint32)
        _check(lib().pbx_test_batch_lz77(self.service.handle, self._h, h.ctypes.data,
                                         m.ctypes.data, nseg))
        return h.reshape(nseg, hist_words), m.reshape(nseg, mrec_words)

    def pred_tiles(self) -> Tuple[int, int]:
        """(fast, general): the planned batch's tiles (sub-tiles, for tiled TIFF) that go to the
        fast and to the general predictor kernel (pbx_batch_pred_tiles)."""
        f, g = ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib().pbx_batch_pred_tiles(self.service.handle, self._h, ctypes.byref(f), ctypes.byref(g)))
        return f.value, g.value

    def lz_modes(self):
        """Per segment of the launched batch, in batch order: 0 = parsed for matches,
        1 = Huffman-only (pbx_batch_lz_modes), as a uint8 numpy array."""
        import numpy as np
        nseg = int(self.stats().segments)
        m = np.zeros(nseg, np.uint8)
        n1 = ctypes.c_uint64()
        _check(lib().pbx_batch_lz_modes(self.service.handle, self._h, m.ctypes.data, nseg, ctypes.byref(n1)))
        assert int(m.sum()) == n1.value
        return m

    def fetch_into_host(self) -> int:
        """D2H of every result into library-owned pinned memory, then release it; returns
        the response bytes (bench: end-to-end rate without Python-side copies)."""
        res = (PbxResult * max(self.n, 1))()
        _check(lib().pbx_batch_fetch(self.service.handle, self._h, res))
        n = sum(res[i].len for i in range(self.n))
        lib().pbx_results_release(self.service.handle, res, self.n)
        return n

    def close(self) -> None:
        if self._h:
            lib().pbx_batch_destroy(self.service.handle, self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ----------------------------------------------------------------- plane sources

class Pixels:
    """The Pixels row getPixels returns (TileRequestHandler.java:220-241: pixelsType, sizeX..T)
    plus the PixelBuffer's getResolutionLevels()."""

    def __init__(self, image_id: int, pixel_type: int, size_x: int, size_y: int, size_z: int = 1,
                 size_c: int = 1, size_t: int = 1, levels: int = 1):
        self.image_id, self.pixel_type = image_id, pixel_type
        self.size_x, self.size_y = size_x, size_y
        self.size_z, self.size_c, self.size_t, self.levels = size_z, size_c, size_t, levels


class PixelSource:
    """Where a plane comes from when this context does not hold it: the reference's
    getPixels (TileRequestHandler.java:220-241) and getPixelBuffer(pixels) (:201-211) +
    PixelBuffer.getTileDirect (:107-109).  Subclass per storage (ROMIO files, Zarr, ...)."""

    def get_pixels(self, image_id: int) -> Optional[Pixels]:
        """The image's Pixels, or None if it does not exist (-> 404, :130-132)."""
        raise NotImplementedError

    def level_size(self, pixels: Pixels, level: int) -> Tuple[int, int]:
        """(size_x, size_y) of STORED level `level` (0 = full resolution)."""
        if level == 0:
            return pixels.size_x, pixels.size_y
        raise NotImplementedError

    def read_rows(self, pixels: Pixels, z: int, c: int, t: int, level: int, y0: int,
                  rows: int) -> bytes:
        """getTileDirect(z, c, t, 0, y0, sizeX, rows) at that level: packed big-endian rows."""
        raise NotImplementedError

    def band_chunks(self, pixels: Pixels, z: int, c: int, t: int, level: int, y0: int,
                    rows: int) -> Optional[dict]:
        """Optional, for storage that is Zarr: the chunk rows covering rows [y0, y0 + rows) of
        the plane at that level, as zarr_band_spec returns them (chunk_x, chunk_y, codec,
        chunks, fill_bits, big_endian = the array's byte order, and chunk_planes / slice for
        chunks that hold several planes); load_bands then has them
        decoded on the GPU instead of calling read_rows.  rows == 0 asks for the byte order and
        geometry only and must read no chunk.  None (the default): no chunk-level access."""
        return None

    def plane_segments(self, pixels: Pixels, z: int, c: int, t: int, level: int) -> Optional[dict]:
        """Optional, for storage that is TIFF: the whole plane at that level as tiff_plane_spec
        returns it; load_plane then registers it from its strips or tiles, decoded on the GPU
        (register_tiff_planes), instead of calling read_rows.  None (the default): rows only."""
        return None

    def band_segments(self, pixels: Pixels, z: int, c: int, t: int, level: int, y0: int,
                      rows: int) -> Optional[dict]:
        """Optional, for storage that is TIFF: the strips or tile rows covering rows
        [y0, y0 + rows) of the plane at that level, as tiff_band_spec returns them (seg_w,
        seg_h, tiled, compression, predictor, segments, big_endian = the file's byte order);
        load_bands then has them decoded on the GPU (band_write_tiff) instead of calling
        read_rows.  rows == 0 asks for the byte order and geometry only and must read no
        segment.  None (the default): no segment-level access."""
        return None


class NgffSource(PixelSource):
    """NGFF multiscale images on disk, {image_id: image directory} -- what ZarrPixelsService
    opens per image (config.yaml:18): dataset k of .zattrs "multiscales"[0] is stored level k.
    Planes are loaded band by band from the chunk files covering the requested rows
    (band_chunks -> zarr_band_spec), so it needs a service with sparse_band_rows."""

    def __init__(self, images: Mapping[int, str]):
        import threading
        self.images = dict(images)
        self._opened: Dict[int, tuple] = {}
        self._lock = threading.Lock()

    def _open(self, image_id: int):
        """(axes, [(array directory, .zarray)] per dataset) of an image, read once."""
        with self._lock:
            ent = self._opened.get(image_id)
            if ent is None:
                ms, root = ngff_multiscales(self.images[image_id])
                dirs = [os.path.join(root, ds["path"]) for ds in ms["datasets"]]
                ent = self._opened[image_id] = (ms.get("axes"), [(d, _array_meta(d)) for d in dirs])
            return ent

    def get_pixels(self, image_id: int) -> Optional[Pixels]:
        if image_id not in self.images:
            return None
        axes, levels = self._open(image_id)
        meta = levels[0][1]
        ext = {"t": 1, "c": 1, "z": 1}
        ext.update(zip(_lead_axes(len(meta["shape"]), axes), meta["shape"][:-2]))
        return Pixels(image_id, _ZARR_DTYPES[meta["dtype"][1:]], meta["shape"][-1], meta["shape"][-2],
                      ext["z"], ext["c"], ext["t"], levels=len(levels))

    def level_size(self, pixels: Pixels, level: int) -> Tuple[int, int]:
        shape = self._open(pixels.image_id)[1][level][1]["shape"]
        return shape[-1], shape[-2]

    def band_chunks(self, pixels: Pixels, z: int, c: int, t: int, level: int, y0: int,
                    rows: int) -> Optional[dict]:
        axes, levels = self._open(pixels.image_id)
        adir, meta = levels[level]
        return zarr_band_spec(adir, z, c, t, y0, rows, meta, axes)

    def read_rows(self, pixels: Pixels, z: int, c: int, t: int, level: int, y0: int,
                  rows: int) -> bytes:
        raise PbxError(E_BADARG, "NgffSource hands over Zarr chunks, not rows: serve it from a "
                       "PixelsService with sparse_band_rows (whole planes: register_ngff_image)")


class TiffSource(PixelSource):
    """TIFF / OME-TIFF files on disk, {image_id: path} -- the original files the ordinary OMERO
    PixelsService opens through Bio-Formats when an image has no NGFF fileset (config.yaml:18).
    On a service without sparse_band_rows a plane the context does not hold is registered whole
    from its IFD's strips or tiles (plane_segments -> PixelsService.load_plane ->
    register_tiff_planes); with sparse_band_rows only the bands a request's rows cover are
    loaded, each from the strips or tile rows that cover it (band_segments -> load_bands ->
    band_write_tiff).  Either way every byte of pixel data is decoded on the GPU."""

    def __init__(self, images: Mapping[int, str], j2k_packets: bool = True, j2k_chroma: bool = True,
                 aperio_ycbcr: bool = False, packed: bool = True):
        import threading
        self.images = dict(images)
        self.packed = packed  # bit-packed samples, PackBits, FillOrder 2: tiff_plane_spec's keyword of this name
        self.j2k_packets = j2k_packets  # JPEG 2000 IFDs: tiff_plane_spec's keywords of these names
        self.j2k_chroma = j2k_chroma
        self.aperio_ycbcr = aperio_ycbcr
        self._opened: Dict[int, dict] = {}
        self._lock = threading.Lock()

    def _open(self, image_id: int) -> dict:
        with self._lock:
            lay = self._opened.get(image_id)
            if lay is None:
                lay = self._opened[image_id] = tiff_image_layout(self.images[image_id], self.j2k_packets, self.j2k_chroma,
                                                                  self.aperio_ycbcr,
                                                                  **({"packed": True} if self.packed else {}))
            return lay

    def get_pixels(self, image_id: int) -> Optional[Pixels]:
        if image_id not in self.images:
            return None
        lay = self._open(image_id)
        return Pixels(image_id, lay["pixel_type"], lay["ifds"][0]["width"], lay["ifds"][0]["length"],
                      lay["size_z"], lay["size_c"], lay["size_t"], levels=lay["levels"])

    def _ifd(self, pixels: Pixels, z: int, c: int, t: int, level: int) -> Tuple[dict, int]:
        """(the IFD that holds channel c, c's sample in it): channel c of a file with S samples
        per pixel is sample c % S of the IFD of (z, c - c % S, t)."""
        lay = self._open(pixels.image_id)
        sample = c % lay["samples"]
        ifd = lay["ifds"][lay["planes"].index((z, c - sample, t))]
        return (ifd if level == 0 else ifd["subifds"][level - 1]), sample

    def level_size(self, pixels: Pixels, level: int) -> Tuple[int, int]:
        d = self._ifd(pixels, 0, 0, 0, level)[0]
        return d["width"], d["length"]

    def _j2k_kw(self, ifd: dict) -> dict:
        """(the keywords only for a JPEG 2000 IFD, `packed` only for an IFD that needs it: every
        other file is the call it always was)"""
        if ifd["compression"] not in _TIFF_J2K_COMPRESSIONS:
            return {"packed": True} if self.packed and _tiff_needs_packed(ifd) else {}
        return {k: True for k in ("j2k_packets", "j2k_chroma", "aperio_ycbcr") if getattr(self, k)}

    def plane_segments(self, pixels: Pixels, z: int, c: int, t: int, level: int) -> Optional[dict]:
        ifd, sample = self._ifd(pixels, z, c, t, level)
        return tiff_plane_spec(self.images[pixels.image_id], ifd, pixels.image_id, z, c, t, level, sample=sample,
                               **self._j2k_kw(ifd))

    def band_segments(self, pixels: Pixels, z: int, c: int, t: int, level: int, y0: int,
                      rows: int) -> Optional[dict]:
        ifd, sample = self._ifd(pixels, z, c, t, level)
        path = self.images[pixels.image_id]
        # (sample 0 -- every single-sample file -- is the call it always was)
        kw = self._j2k_kw(ifd)
        return tiff_band_spec(path, ifd, y0, rows, **kw) if sample == 0 else tiff_band_spec(path, ifd, y0, rows, sample=sample, **kw)

    def read_rows(self, pixels: Pixels, z: int, c: int, t: int, level: int, y0: int,
                  rows: int) -> bytes:
        raise PbxError(E_BADARG, "TiffSource hands over TIFF segments, not rows: whole planes go "
                       "through plane_segments and bands of a sparse plane through band_segments, "
                       "so serve it without a whole-row band")


def _derived_from(source, pixels: "Pixels", level: int, step: int) -> Optional[Tuple[int, int]]:
    """source.derived_from(pixels, level, step) of a source that has derived levels, or None: the
    source stores every level it declares, or stores this one."""
    f = getattr(source, "derived_from", None)
    return f(pixels, level, step) if f is not None else None


class DerivedLevels(PixelSource):
    """Lower resolution levels for a source that stores none, or too few: `inner`'s L stored levels
    are served as they are, and E more are declared after them, each the 2x2 mean of the one
    before (size (n + 1) // 2 per axis, the last column / row repeated when n is odd) -- what
    OMERO's pyramid generation gives an image too large to serve whole.  levels: E; None: halve
    until both sides of the smallest level are <= max_side (3192 is believed to be the default of
    omero.pixeldata.max_plane_width / _height; it has not been checked against a server).
    Nothing of a derived level is stored or read: a PixelsService makes its bands on the GPU from
    the resident bands of the level reduce_step above it (load_bands -> band_write_reduced), or,
    without sparse_band_rows, builds all E levels from the whole last stored level (load_plane ->
    build_pyramid).  Derived levels are not sharded by rows (a handler with band=: 400)."""

    def __init__(self, inner: PixelSource, levels: Optional[int] = None, max_side: int = 3192):
        if levels is not None and levels < 0:
            raise ValueError("levels %r" % (levels,))
        if max_side < 1:
            raise ValueError("max_side %r" % (max_side,))
        self.inner, self.levels, self.max_side = inner, levels, max_side
        self._counts: Dict[int, Tuple[int, int]] = {}  # image -> (stored levels, all levels)

    def get_pixels(self, image_id: int) -> Optional[Pixels]:
        import copy
        p = self.inner.get_pixels(image_id)
        if p is None:
            return None
        extra = self.levels
        if extra is None:
            extra, (sx, sy) = 0, self.inner.level_size(p, p.levels - 1)
            while max(sx, sy) > self.max_side:
                sx, sy, extra = (sx + 1) // 2, (sy + 1) // 2, extra + 1
        q = copy.copy(p)
        q.stored_levels, q.levels = p.levels, p.levels + extra
        self._counts[image_id] = (p.levels, q.levels)
        return q

    def resolution_is_derived(self, image_id: int, resolution: int) -> bool:
        """Whether `resolution` (OMERO numbering, 0 = the smallest level) names a derived level of
        the image; its level counts are looked up once (get_pixels) and remembered."""
        if image_id not in self._counts and self.get_pixels(image_id) is None:
            return False
        stored, levels = self._counts[image_id]
        return stored <= levels - 1 - resolution < levels

    def stored_levels(self, pixels: Pixels) -> int:
        """L: the levels `inner` stores (levels L .. pixels.levels - 1 are derived)."""
        n = getattr(pixels, "stored_levels", None)
        return n if n is not None else self.inner.get_pixels(pixels.image_id).levels

    def derived_from(self, pixels: Pixels, level: int, step: int) -> Optional[Tuple[int, int]]:
        """(source_level, k) of a derived level: it is made from source_level = max(L - 1,
        level - step), k = level - source_level levels above it.  None: a stored level, or no
        level of the image."""
        last = self.stored_levels(pixels) - 1
        if level <= last or level >= pixels.levels:
            return None
        src = max(last, level - step)
        return src, level - src

    def level_size(self, pixels: Pixels, level: int) -> Tuple[int, int]:
        last = self.stored_levels(pixels) - 1
        sx, sy = self.inner.level_size(pixels, min(level, last))
        for _ in range(level - last):
            sx, sy = (sx + 1) // 2, (sy + 1) // 2
        return sx, sy

    def _stored(self, name: str, pixels: Pixels, level: int, *args):
        f = getattr(self.inner, name, None)
        return f(pixels, *args) if f is not None and level < self.stored_levels(pixels) else None

    def read_rows(self, pixels: Pixels, z: int, c: int, t: int, level: int, y0: int, rows: int) -> bytes:
        if level >= self.stored_levels(pixels):
            raise PbxError(E_BADARG, "level %d is derived: its rows are made on the GPU, not read" % level)
        return self.inner.read_rows(pixels, z, c, t, level, y0, rows)

    def band_chunks(self, pixels: Pixels, z: int, c: int, t: int, level: int, y0: int, rows: int) -> Optional[dict]:
        return self._stored("band_chunks", pixels, level, z, c, t, level, y0, rows)

    def plane_segments(self, pixels: Pixels, z: int, c: int, t: int, level: int) -> Optional[dict]:
        return self._stored("plane_segments", pixels, level, z, c, t, level)

    def band_segments(self, pixels: Pixels, z: int, c: int, t: int, level: int, y0: int, rows: int) -> Optional[dict]:
        return self._stored("band_segments", pixels, level, z, c, t, level, y0, rows)


# ----------------------------------------------------------------- TileRequestHandler

class TileRequestHandler:
    """TileRequestHandler.java:53-243 — ``get_tile()`` returns bytes, or None (-> 404).

    With a ``source`` (PixelSource), a plane the context does not hold (status
    E_NOT_RESIDENT) is opened as the reference opens it per request — getPixels (:84; None ->
    404), getPixelBuffer + getTileDirect (:86,107-109) — loaded into HBM, and the request
    retried.  The service's policy decides what is loaded: the whole plane, or (with
    ``sparse_band_rows``) only the bands the request's rows cover (region-proportional, as
    getTileDirect reads only the region).  ``band`` = (y0, rows) limits what this context
    holds (a rank's share of a whole slide); requests outside it are answered None here
    (another rank serves them).  Between a load and the retry another loader may evict what
    was loaded (a residency budget smaller than the working set): the load is retried, and a
    tile that still cannot be held is a 500, never the reference's 404.  Without a source the
    context is a closed registry: not resident -> None (404)."""

    LOAD_ATTEMPTS = 4
    NO_SPACE_WAIT_S = 30.0

    def _never_fits(self, pixels: "Pixels", level: int) -> bool:
        """The plane (or one band of it) is larger than the whole residency budget."""
        budget = self.pixels_service.residency_stats()["budget"]
        if not budget:
            return False
        sx, sy = self.source.level_size(pixels, level)
        rows = self.pixels_service.sparse_band_rows or sy
        pitch = (sx * BYTES_PER_PIXEL[pixels.pixel_type] + 255) // 256 * 256
        return pitch * min(rows, sy) + 256 > budget

    def __init__(self, pixels_service: PixelsService, tile_ctx: TileCtx,
                 source: Optional[PixelSource] = None, band: Optional[Tuple[int, int]] = None,
                 tracer=None):
        """``tracer``: optional ``tracer(name, ms, tags)`` called with the reference's span
        names (TileRequestHandler.java:81 get_tile, :104 get_tile_direct, :147 create_metadata,
        :180 write_image; :84 get_pixels and getTileDirect reads of a cold plane as
        get_pixels / load_region): the device stages are those of the batch that served the
        request (pbx_result_spans), get_tile is this call's wall time."""
        self.pixels_service = pixels_service
        self.tile_ctx = tile_ctx
        self.source = source
        self.band = band
        self.tracer = tracer

    def _span(self, name: str, ms: float, **tags) -> None:
        if self.tracer is not None:
            self.tracer(name, ms, tags)

    def _serve(self):
        """One pbx_get_tile with the batch's stage spans."""
        sp = {} if self.tracer is not None else None
        status, body = self.pixels_service.get_tile(self.tile_ctx, sp)
        if sp:
            tags = {"batch_tiles": sp["batch_tiles"]}
            self._span("get_tile_direct", sp["get_tile_direct_ms"], **tags)
            self._span("create_metadata", sp["create_metadata_ms"], **tags)
            self._span("write_image", sp["write_image_ms"], **tags)
            self._span("d2h", sp["d2h_ms"], **tags)
        return status, body

    @staticmethod
    def _answer(status: int, body: Optional[bytes]) -> Optional[bytes]:
        """The tile, None for every status the reference answers null (-> 404), and an
        exception (-> 500, PixelBufferVerticle.java:141-146) for a device failure."""
        if status == E_INTERNAL:
            raise PbxError(E_INTERNAL, "tile batch failed on the device: " +
                           lib().pbx_last_error().decode(errors="replace"))
        return body if status == OK else None

    def get_tile(self, client=None) -> Optional[bytes]:
        t0 = time.perf_counter()
        try:
            return self._get_tile()
        finally:
            self._span("get_tile", (time.perf_counter() - t0) * 1e3)

    def _get_tile(self) -> Optional[bytes]:
        svc, tc = self.pixels_service, self.tile_ctx
        if self.band is not None and tc.resolution is not None:
            # a rank's share of the rows is a share of stored levels only, resident or not (the
            # source remembers an image's level counts: no metadata lookup on a resident hit)
            derived = getattr(self.source, "resolution_is_derived", None)
            if derived is not None and derived(tc.imageId, tc.resolution):
                raise PbxError(E_BADARG, "derived levels are not sharded by rows")
        status, body = self._serve()
        if status != E_NOT_RESIDENT or self.source is None:
            return self._answer(status, body)
        t1 = time.perf_counter()
        pixels = self.source.get_pixels(tc.imageId)
        self._span("get_pixels", (time.perf_counter() - t1) * 1e3)
        if pixels is None:
            return None  # :130-132 "Cannot find Image"
        level = 0
        if tc.resolution is not None:
            level = pixels.levels - 1 - tc.resolution  # OMERO numbering -> stored level (include/pbx.h)
        if not (0 <= level < pixels.levels and 0 <= tc.z < pixels.size_z and
                0 <= tc.c < pixels.size_c and 0 <= tc.t < pixels.size_t):
            svc.declare_image(pixels)  # the retry answers the reference's 404
            return self._answer(*svc.get_tile(tc))
        y, h = tc.y, (tc.h or pixels.size_y)  # :92-97 defaulting from the full-resolution size
        if self.band is not None and not (self.band[0] <= y < self.band[0] + self.band[1] and (
                svc.sparse_band_rows or y + h <= self.band[0] + self.band[1])):
            return None  # rows of another context's band (a sparse plane serves every region
            #              that starts in its rows, a whole-row band only those inside it)
        attempts, deadline = 0, time.monotonic() + self.NO_SPACE_WAIT_S
        while attempts < self.LOAD_ATTEMPTS:
            t1 = time.perf_counter()
            try:
                if svc.sparse_band_rows:
                    svc.load_bands(self.source, pixels, tc.z, tc.c, tc.t, level, y, h, own=self.band)
                else:
                    svc.load_plane(self.source, pixels, tc.z, tc.c, tc.t, level, self.band)
            except PbxError as e:
                # the budget is held by planes other requests are reading or have just loaded
                # (the library keeps a fresh plane until its first read): wait for them, unless
                # the plane could never fit
                if e.status != E_NO_SPACE or time.monotonic() > deadline or self._never_fits(pixels, level):
                    raise
                time.sleep(0.002)
                continue
            attempts += 1
            self._span("load_region", (time.perf_counter() - t1) * 1e3)
            status, body = self._serve()
            if status != E_NOT_RESIDENT:
                return self._answer(status, body)
        raise PbxError(E_INTERNAL, "Image:%d z=%d c=%d t=%d: the plane could not be held resident "
                       "(residency budget smaller than the working set)" % (tc.imageId, tc.z, tc.c, tc.t))

    getTile = get_tile


def handle_get_tile(service: PixelsService, body: str, source: Optional[PixelSource] = None, tracer=None):
    """PixelBufferVerticle.getTile (PixelBufferVerticle.java:90-147) over the JSON body.

    Returns (status, payload bytes or message, headers).  400 for an undecodable TileCtx,
    404 when the handler returns null, 500 for any other failure.  ``tracer``: as
    TileRequestHandler's, plus the consumer's own span "handle_get_tile" (:101-104).
    """
    t0 = time.perf_counter()
    try:
        return _handle_get_tile(service, body, source, tracer)
    finally:
        if tracer is not None:
            tracer("handle_get_tile", (time.perf_counter() - t0) * 1e3, {})


def _handle_get_tile(service, body, source, tracer):
    try:
        ctx = TileCtx.from_json(body)
    except Exception:
        return 400, b"Illegal tile context", {}
    try:
        tile = TileRequestHandler(service, ctx, source, tracer=tracer).get_tile()
    except PbxError as e:
        return (400 if e.status == E_BADARG else 500), b"Exception while retrieving tile", {}
    if tile is None:
        return 404, f"Cannot find Image:{ctx.imageId}".encode(), {}
    return 200, tile, {"filename": tile_filename(ctx),
                       "Content-Type": content_type(ctx.format),
                       "Content-Length": str(len(tile))}
