/*
 * pbx.h — C-ABI of the MI355X-native /tile pipeline (drop-in for the
 * omero-ms-pixel-buffer tile hot path).
 *
 * Plain C: no exceptions, no torch/HIP types, plain pointers and sizes.  Every
 * entry point is thread-safe.  Each declaration cites the reference interface
 * it replaces; paths are relative to
 * /root/reference/src/main/java/com/glencoesoftware/omero/ms/pixelbuffer/.
 *
 * Mapping to the reference:
 *   TileCtx (TileCtx.java:30-92)                  -> pbx_tile_req
 *   TileRequestHandler.getTile (TileRequestHandler.java:80-139)
 *                                                 -> pbx_get_tile / pbx_get_tiles
 *   PixelBuffer.getTileDirect (:107-109)          -> kernel K1 (extract + big-endian)
 *   writeImage("png"|"tif") (:176-199)            -> kernels K2..K7 (filter/deflate/frame)
 *   PixelsService.getPixelBuffer (:201-211)       -> planes registered with pbx_plane_register
 *   getPixels (Ice HQL, :220-241)                 -> the plane registry's image records
 *   reply "filename" header (PixelBufferVerticle.java:116-126)  -> pbx_tile_filename
 *   Content-Type (PixelBufferMicroserviceVerticle.java:373-379)  -> pbx_content_type
 */
#ifndef PBX_H
#define PBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBX_ABI_VERSION 9

/* Status codes are the HTTP status the reference's event-bus consumer ends with:
 * getTile() == null -> message.fail(404) (PixelBufferVerticle.java:111-114);
 * IllegalArgumentException -> 400 (:137-140); any other exception -> 500 (:141-146).
 *
 * PBX_E_NOT_RESIDENT is never sent to a client.  It means "this context does not hold the
 * plane the request needs": the image is unknown here, its (z, c, t, level) plane was never
 * loaded or was evicted, or the region lies outside the row band this context owns.  The
 * reference would open the plane on demand (getPixels + getPixelBuffer,
 * TileRequestHandler.java:84-86,201-241); the binding does the same — look the image up,
 * load the plane with pbx_image_declare / pbx_plane_create / pbx_plane_write_rows /
 * pbx_plane_commit and retry.  A context answers 404 only for what the
 * reference itself answers 404. */
enum pbx_status {
    PBX_OK = 0,
    PBX_E_BADARG = 400,
    PBX_E_NOTFOUND = 404,
    PBX_E_EXISTS = 409,      /* registration: the (image, z, c, t, level) key is taken (loaded
                                or being loaded by another caller) */
    PBX_E_NOT_RESIDENT = 460,/* tile status: load the plane, then retry (see above) */
    PBX_E_INTERNAL = 500,
    PBX_E_PENDING = 504,     /* pbx_wait: the batch is still running (not a tile status) */
    PBX_E_NO_SPACE = 507     /* registration: the plane does not fit the HBM residency budget
                                even after evicting every idle plane */
};

/* OMERO pixel types (ome.xml.model.enums.PixelType; TileRequestHandler.java:100-101,164-165). */
enum pbx_pixel_type {
    PBX_INT8 = 0, PBX_UINT8, PBX_INT16, PBX_UINT16, PBX_INT32, PBX_UINT32, PBX_FLOAT, PBX_DOUBLE,
    PBX_NPIXEL_TYPES
};

/* TileCtx.format (TileCtx.java:89): null -> raw bytes (:128), "png"/"tif" -> writeImage
 * (:122-123), anything else -> null -> 404 (:125-126). */
enum pbx_format { PBX_FMT_RAW = 0, PBX_FMT_PNG = 1, PBX_FMT_TIF = 2, PBX_FMT_UNKNOWN = 3 };

/* Byte order of the samples of a registered plane as handed to pbx_plane_register. */
enum pbx_byte_order { PBX_BIG_ENDIAN = 0, PBX_LITTLE_ENDIAN = 1 };

/* Plane sources: host bytes (copied to HBM) or an on-device synthetic generator
 * (Bio-Formats FakeReader-style G_FAKE, counter-hash G_NOISE). */
enum pbx_source { PBX_SRC_HOST = 0, PBX_SRC_GEN_FAKE = 1, PBX_SRC_GEN_NOISE = 2 };

/* PNG scanline filter used by the encoder.  NONE is what the reference's APNGWriter
 * writes (filter byte 0 on every row); the others decode to identical pixels.  ADAPTIVE: per
 * tile, NONE on every row when the tile's middle row says filtering does not pay, else per row
 * the filter with the smallest sum of |byte - prediction|. */
enum pbx_png_filter {
    PBX_FILTER_NONE = 0, PBX_FILTER_SUB = 1, PBX_FILTER_UP = 2, PBX_FILTER_AVG = 3,
    PBX_FILTER_PAETH = 4, PBX_FILTER_ADAPTIVE = 5
};

typedef struct pbx_config {
    int32_t device;          /* HIP device ordinal; -1 = $PBX_DEVICE, else $LOCAL_RANK, else 0 */
    int32_t png_filter;      /* enum pbx_png_filter; default NONE (reference) */
    int32_t tiff_deflate;    /* 0 = uncompressed TIFF (reference default); 1 = Compression=8 */
    int32_t segment_bytes;   /* deflate segment size (bytes of filtered stream); 0 = default */
    uint64_t max_batch_bytes;/* device scratch budget per batch; 0 = default */
    int32_t coalesce;        /* 1 (default) = concurrent pbx_get_tile calls are coalesced into
                                batches (one per GPU-busy interval); 0 = one batch per call */
    int32_t stage_rows;      /* 0 (default) = the deflate kernels read filter-None rows straight
                                from the plane; 1 = stage them in a stream buffer first (k_rows) */
    int32_t tiff_tile;       /* 0 (reference) = TIFF as one strip; T = tiled TIFF (TIFF 6.0 s.15)
                                of T x T tiles, edge tiles zero-padded; T a multiple of 16 in
                                [16, 4096]; with tiff_deflate every tile is its own zlib stream */
    int32_t request_timeout_us; /* deadline of one pbx_get_tile / pbx_node_get_tile call: past it
                                the call answers PBX_E_INTERNAL (500), as the reference's
                                event-bus send timeout does (PixelBufferMicroserviceVerticle.java:
                                148-151 default 15 s, :356-366 timeout -> 500); the late batch's
                                results are released when it completes.  0 = $PBX_REQUEST_TIMEOUT_US,
                                else 15,000,000; < 0 = no deadline */
} pbx_config;

typedef struct pbx_ctx pbx_ctx;

/* Lifecycle (PixelBufferMicroserviceVerticle.start/deploy :114-233, stop :298-308). */
int pbx_config_default(pbx_config* cfg);
int pbx_init(const pbx_config* cfg, pbx_ctx** out);
void pbx_shutdown(pbx_ctx* ctx);
/* Last error message of the calling thread (never NULL). */
const char* pbx_last_error(void);
int pbx_abi_version(void);
int pbx_device_count(void);

/* A plane (z,c,t,resolution) of an image.  Registering a resolution-0 plane creates or
 * checks the image record (the `Pixels` row getPixels returns, TileRequestHandler.java:220-241):
 * size_x/size_y/pixel_type are the image's. */
typedef struct pbx_plane_desc {
    int64_t image_id;
    int32_t z, c, t;
    int32_t resolution;      /* STORED pyramid level: 0 = full resolution, k = k-th downsampled
                                level (the NGFF multiscales dataset index).  Requests use
                                OMERO's numbering instead: see pbx_tile_req.resolution. */
    int32_t pixel_type;      /* enum pbx_pixel_type */
    int32_t size_x, size_y;
    int32_t byte_order;      /* enum pbx_byte_order of host_data (ignored for generators) */
    int32_t source;          /* enum pbx_source */
    const void* host_data;   /* PBX_SRC_HOST: size_y rows of size_x samples, row-major */
    uint64_t host_bytes;
    uint64_t seed;           /* generators */
    int32_t plane_no;        /* generators: FakeReader plane number / noise plane index */
    int32_t reserved;
} pbx_plane_desc;

int pbx_plane_register(pbx_ctx* ctx, const pbx_plane_desc* desc, uint64_t* plane_id);
/* Frees the plane.  Batches planned before the call keep reading it: the HBM is returned
 * when the last of them is destroyed (pbx_batch_destroy), never under a running kernel. */
int pbx_plane_release(pbx_ctx* ctx, uint64_t plane_id);

/* ---- Plane residency: planes opened on demand, in row bands, under an HBM budget ----
 *
 * The reference opens an image's PixelBuffer per request (getPixels :220-241, then
 * getPixelBuffer :201-211 and getTileDirect :107-109).  Here the bytes of a plane are loaded
 * into HBM once and then serve every tile of it; a request for a plane this context does not
 * hold answers PBX_E_NOT_RESIDENT and the binding loads it.
 *
 * pbx_image_declare records the Pixels row getPixels returns (:84; pixelsType, sizeX/Y/Z/C/T)
 * and the PixelBuffer's getResolutionLevels().  With it a request for a z/c/t outside the
 * image, or a resolution outside its levels, is the reference's 404 without loading anything;
 * without it (planes registered directly) the image is described by its registered planes. */
typedef struct pbx_image_desc {
    int64_t image_id;
    int32_t pixel_type;          /* enum pbx_pixel_type (Pixels.pixelsType) */
    int32_t size_x, size_y;      /* full resolution (Pixels.sizeX / sizeY) */
    int32_t size_z, size_c, size_t_;
    int32_t levels;              /* PixelBuffer.getResolutionLevels(); >= 1 */
    int32_t reserved;
} pbx_image_desc;
/* Idempotent; 400 if it contradicts an earlier declaration or a registered plane. */
int pbx_image_declare(pbx_ctx* ctx, const pbx_image_desc* desc);
/* Releases every plane of the image and forgets its record (requests then answer
 * NOT_RESIDENT).  404 if the image is unknown. */
int pbx_image_release(pbx_ctx* ctx, int64_t image_id);

/* Allocates a plane — or only its rows [band_y0, band_y0 + band_rows) when band_rows > 0 (a
 * rank's tile-row band of a whole slide) — under the key desc->(image_id, z,
 * c, t, resolution).  desc->size_x / size_y are the plane's (the level's) full size; requests
 * for rows outside the band answer PBX_E_NOT_RESIDENT (another context owns them).
 * desc->source: PBX_SRC_HOST -> the plane is empty and not served until pbx_plane_commit;
 * its rows arrive by pbx_plane_write_rows in desc->byte_order.  Generators -> the band is
 * generated on the GPU and the plane is ready at once.  409 if the key is loaded or being
 * loaded; 507 if it does not fit the residency budget (pbx_set_residency_budget). */
int pbx_plane_create(pbx_ctx* ctx, const pbx_plane_desc* desc, int32_t band_y0, int32_t band_rows,
                     uint64_t* plane_id);
/* Rows [y0, y0 + rows) of a created plane (inside its band): `rows` rows of size_x samples,
 * packed (size_x * bpp bytes each), as PixelBuffer.getTileDirect(z, c, t, 0, y0, sizeX, rows)
 * returns them.  Copied through pooled pinned staging to HBM; the caller's buffer is free
 * again when the call returns.  Any number of calls, in any order, of any band size. */
int pbx_plane_write_rows(pbx_ctx* ctx, uint64_t plane_id, int32_t y0, int32_t rows, const void* data,
                         uint64_t bytes);
/* Publishes a created plane: from now on its tiles are served.  400 if a row of the band was
 * never written. */
int pbx_plane_commit(pbx_ctx* ctx, uint64_t plane_id);
/* The plane registered under a key (STORED level): its id and state (0 loading, 1 ready,
 * 2 evicted) and resident band; 404 if the key is not registered.  Lets a binding that got
 * NOT_RESIDENT tell "load it" from "another caller is loading it". */
int pbx_plane_lookup(pbx_ctx* ctx, int64_t image_id, int32_t z, int32_t c, int32_t t, int32_t level,
                     uint64_t* plane_id, int32_t* state, int32_t* band_y0, int32_t* band_rows);

/* Sparse planes: region-proportional residency.  The reference reads only the requested region
 * per request (new byte[w*h*bpp] then getTileDirect(z, c, t, x, y, w, h), TileRequestHandler.java:
 * 102-109); a whole-slide plane is far larger than one request.  A sparse plane is registered
 * under its key at once (READY) but holds its rows as bands of `band_rows` rows (band k = rows
 * [k*band_rows, (k+1)*band_rows)), each loaded on demand, pinned by the batches that read it and
 * evicted on its own, least recently used first, under the residency budget.  A request whose
 * rows cover a band that is not resident answers PBX_E_NOT_RESIDENT; the binding loads the
 * covering bands (rows y .. y+h-1, by pbx_band_write) and retries.  A region straddling bands is
 * served bit-exact (its rows are gathered into a per-batch bridge buffer on the GPU).
 * own_y0 / own_rows (0/0 = the whole plane): the rows this context may hold; own_y0 a multiple of
 * band_rows; rows outside answer PBX_E_NOT_RESIDENT (another context owns them).  Generator
 * sources generate each band on the GPU when it is written with data == NULL. */
int pbx_plane_create_sparse(pbx_ctx* ctx, const pbx_plane_desc* desc, int32_t band_rows, int32_t own_y0,
                            int32_t own_rows, uint64_t* plane_id);
/* Rows [y0, y0 + rows) of ONE band (packed, desc->byte_order), as getTileDirect(z, c, t, 0, y0,
 * sizeX, rows) returns them; the first write of an absent band allocates it (507 if it cannot be
 * made to fit), the write that completes it makes it resident.  409 if the band is resident (or
 * another caller is allocating it).  data == NULL: generate the rows (generator planes).  A
 * failed write fails the band's whole load (every writer of it: load it again). */
int pbx_band_write(pbx_ctx* ctx, uint64_t plane_id, int32_t y0, int32_t rows, const void* data,
                   uint64_t bytes);
/* A loader that gives up on the band holding row y0 part-way (a failed piece, a Java exception
 * between pieces): the band goes back to absent and its HBM is returned (at once, or by the last
 * write still in flight); a resident or absent band is left as it is.  A write that fails does
 * the same by itself, and a band left loading with no write for 10 s is started over by the
 * next writer (or evicted).  400 for a plane that is not sparse. */
int pbx_band_abort(pbx_ctx* ctx, uint64_t plane_id, int32_t y0);
/* band_rows and the number of bands of a sparse plane; states (may be NULL, nbands entries):
 * 0 absent (never loaded, or evicted), 1 loading, 2 resident.  A band whose load failed, or that
 * has been loading without a write for 10 s (a loader that went away), reads as 0 and its HBM is
 * returned.  400 for a plane that is not sparse. */
int pbx_plane_band_info(pbx_ctx* ctx, uint64_t plane_id, int32_t* band_rows, int32_t* nbands, uint8_t* states);

/* HBM residency budget for planes (bytes; 0 = none, the default, or $PBX_HBM_BUDGET_MB).  A
 * registration that would exceed it first evicts idle planes, least recently used first (a
 * plane is idle when no planned batch reads it).  With or without a budget, a plane
 * allocation that fails for lack of device memory evicts idle planes and retries.  An evicted
 * plane's requests answer PBX_E_NOT_RESIDENT until it is registered again. */
int pbx_set_residency_budget(pbx_ctx* ctx, uint64_t bytes);
typedef struct pbx_residency_stats {
    uint64_t budget;             /* 0 = none */
    uint64_t resident_bytes;     /* HBM held by planes and bands (incl. released ones still read) */
    uint64_t planes;             /* registered (non-sparse) planes resident in HBM */
    uint64_t evicted_planes;     /* registered keys whose plane was evicted */
    uint64_t evictions, evicted_bytes;  /* totals since pbx_init (planes and bands) */
    uint64_t bands;              /* resident bands of sparse planes */
    uint64_t band_evictions;     /* bands evicted since pbx_init */
} pbx_residency_stats;
int pbx_residency_stats_get(pbx_ctx* ctx, pbx_residency_stats* out);
/* Resolution pyramid on the GPU (the lower levels
 * PixelBuffer.setResolutionLevel selects, TileRequestHandler.java:89-91): registers `levels`
 * planes of the same (image, z, c, t) at resolutions r+1 .. r+levels (r = the plane's), each
 * the 2x2 box mean of the one above (sizes rounded up; the last column / row repeated for odd
 * sizes; integers (sum + 2) >> 2 on the exact sum, arithmetic for signed types; float/double
 * ((a + b) + (c + d)) * 0.25), in the plane's byte order.  ids[k] = the plane id of level
 * r+1+k (ids may be NULL).  Tiles of a level are served with pbx_tile_req.resolution.
 * kernel_ms (may be NULL): device time of the downsampling kernels (HIP events). */
int pbx_plane_build_pyramid(pbx_ctx* ctx, uint64_t plane_id, int32_t levels, uint64_t* ids,
                            double* kernel_ms);
/* NGFF / Zarr planes: the reference's pixels service is ZarrPixelsService
 * (PixelBufferVerticle.java:29,56; beanRefContext.xml:51; config.yaml:18), which reads Zarr
 * chunks through omero-zarr-pixel-buffer 0.6.1 / JZarr (build.gradle:57) on every
 * getTileDirect.  Here the chunks of one (z, c, t, resolution) plane are uploaded once and
 * decoded on the GPU (one wave per compressed stream) straight into a resident HBM plane,
 * which then serves tiles like any registered plane.  Codec = the .zarray "compressor":
 * null, blosc (c-blosc 1.x frames: blosclz / lz4 / lz4hc / zlib / zstd, byte shuffle, bit
 * shuffle or none, split or not), zlib.  snappy and blosc2 frames -> 400.
 *
 * Zarr v3 (NGFF 0.5) codec pipelines come down to the same call: after "bytes", at most one of
 * blosc (the same c-blosc 1 frames), gzip or zstd, then optionally crc32c; the inner chunks of a
 * "sharding_indexed" shard are cut out by the host and handed over as the chunk grid.
 *   ZSTD  a present chunk is exactly ONE zstd frame (RFC 8878) that decodes to the whole chunk
 *         (numcodecs' v2 "zstd" compressor writes the same).  The host checks the magic, walks
 *         the block headers to the frame's end and answers 400 for a skippable frame, a
 *         dictionary id, a content size other than the chunk's bytes, a truncated frame or bytes
 *         after it.  A frame without a content size is accepted: the decoder's length check and
 *         the optional XXH64 content checksum decide on the device.
 *   GZIP  a present chunk is exactly ONE RFC 1952 member.  The host parses the header (CM = 8;
 *         FEXTRA, FNAME, FCOMMENT and FHCRC are skipped; a reserved FLG bit is 400) and the
 *         trailer: ISIZE must be the chunk's bytes.  The device inflates the body, requires it to
 *         end exactly 8 bytes before the chunk's end (a second member or trailing bytes are 400)
 *         and compares the CRC-32 of the decoded bytes with the trailer's (k_zarr_crc).
 * Both are taken whole for chunks that hold several planes, as zlib is. */
enum pbx_zarr_codec { PBX_ZARR_RAW = 0, PBX_ZARR_BLOSC = 1, PBX_ZARR_ZLIB = 2, PBX_ZARR_ZSTD = 3,
                      PBX_ZARR_GZIP = 4 };
/* pbx_zarr_chunks.flags.  CRC32C: the v3 "crc32c" codec as the last codec of a chunk -- the last
 * 4 bytes of every present chunk are the little-endian CRC-32C (Castagnoli) of the bytes before
 * them.  The planner cuts them off (a present chunk shorter than 4 bytes is 400) and hands the
 * codec the rest; the device checks every chunk's uploaded bytes (k_zarr_crc) and a mismatch is
 * 400 like a decoder error.  Valid with every codec, RAW included.  Any other bit is 400. */
#define PBX_ZARR_F_CRC32C 1

typedef struct pbx_zarr_chunks {
    int32_t chunk_x, chunk_y;   /* .zarray "chunks" (the x and y extents; edge chunks are full) */
    int32_t codec;              /* enum pbx_zarr_codec */
    int32_t flags;              /* PBX_ZARR_F_*; 0 = none */
    const uint8_t* data;        /* the chunk files concatenated, C order over the chunk grid */
    const uint64_t* offsets;    /* gx*gy + 1 entries (gx = ceil(size_x/chunk_x), ...); chunk
                                   i = cy*gx + cx is data[offsets[i] .. offsets[i+1]); an empty
                                   range is a missing chunk (every sample = fill) */
    uint64_t fill_bits;         /* .zarray fill_value as the sample's bit pattern */
} pbx_zarr_chunks;

/* desc: image/z/c/t/resolution/pixel_type/size as pbx_plane_register; byte_order = the
 * .zarray dtype's ('<' little, '>' / '|' big); source/host_data are ignored.
 * kernel_ms (may be NULL): [0] device ms of the decode kernels and the checksum kernel
 * (k_zarr_crc: crc32c chunks, gzip trailers), [1] of the placement kernel.
 * A malformed or unsupported chunk fails the whole plane with 400 (nothing registered).
 * A stream the device refuses is named "corrupt chunk stream N (codec, decoder code C)".  For
 * zlib / gzip (k_zarr_inflate2, k_zarr_inflate; the verdicts are zlib's) C is: 10 RFC 1950
 * header, 11 stored NLEN, 12 stored run past the input or the chunk, 13 block type 3, 14 HLIT >
 * 286 or HDIST > 30, 15 / 19 / 20 the code-length / literal-length / distance code lengths are
 * not a valid set (over-subscribed, or incomplete: only a literal/length or distance set whose
 * longest code is one bit may be incomplete; 19 also when symbol 256 has no code), 16 unassigned
 * code-length code (unreachable since 15 demands a complete code; the guard stays), 17 repeat of
 * nothing, 18 repeat past the count, 21 unassigned literal/length code, 22 literal past the
 * chunk, 23 length symbol 286 / 287, 24 unassigned or invalid distance code, 25 distance before
 * the start or match past the chunk, 26 input overrun, 27 chunk not filled, 28 trailer cut,
 * 29 Adler-32, 31 bytes after a gzip member's trailer. */
int pbx_plane_register_zarr(pbx_ctx* ctx, const pbx_plane_desc* desc, const pbx_zarr_chunks* chunks,
                            uint64_t* plane_id, double* kernel_ms);
/* n planes (e.g. every (z, c, t) plane of an NGFF resolution level) decoded by ONE set of
 * launches: descs[k] / chunks[k] as above, plane_ids[k] receives plane k's id.  More planes
 * per call = more compressed streams in flight (one wave each), which is what hides the
 * serial decode latency.  All planes are registered, or none (400/500). */
int pbx_planes_register_zarr(pbx_ctx* ctx, uint64_t n, const pbx_plane_desc* descs,
                             const pbx_zarr_chunks* chunks, uint64_t* plane_ids, double* kernel_ms);
/* Rows [y0, y0 + rows) of ONE band of a sparse plane, decoded on the GPU from the Zarr chunk
 * rows that cover them: pbx_band_write for a plane stored as NGFF/Zarr, so a cold tile costs
 * the chunks of its bands and not the plane's (ZarrPixelsService reads only the chunks the region
 * covers, TileRequestHandler.java:102-109).  `chunks` is as for pbx_plane_register_zarr (chunk
 * shape, codec, blosc forms, fill_bits) except that data / offsets hold only chunk rows
 * cy0 = y0 / chunk_y up to (not including) cy1 = ceil((y0 + rows) / chunk_y), each full width
 * (gx chunks) in C order: (cy1 - cy0) * gx + 1 offsets; an empty range is a missing chunk (fill).
 * Rows of those chunks outside [y0, y0 + rows) are decoded but not written, so band_rows need not
 * be a multiple of chunk_y and a band may be written in pieces at any rows.  The bytes land in
 * the plane's stored byte order: create the sparse plane with source PBX_SRC_HOST and the
 * .zarray dtype's byte order.  Band states, statuses (400 rows outside one band or a plane that
 * is not sparse, 409 resident band, 507 no room) and failure handling are pbx_band_write's, and
 * pieces written by either call may be mixed in one band.  Malformed input the host can see (null
 * pointers, codec, chunk shape, offsets, blosc headers) is 400 and leaves the band as it was; a
 * stream a decoder rejects on the device is 400 and fails the band's load like a failed upload.
 * Upload, decode and placement run on the upload stream: tile batches do not wait behind them.
 * kernel_ms (may be NULL): [0] device ms of the decode kernels, [1] of the placement kernel. */
int pbx_band_write_zarr(pbx_ctx* ctx, uint64_t plane_id, int32_t y0, int32_t rows,
                        const pbx_zarr_chunks* chunks, double* kernel_ms);

/* Chunks that hold more than one plane (.zarray "chunks" with a leading t / c / z extent
 * above 1: bioformats2raw --chunk_depth, dask volumes such as [1, 1, 16, 256, 256]).  A LAYER
 * is the gy * gx chunk files that share one set of leading chunk indices, as a pbx_zarr_chunks
 * (C order, data / offsets / missing chunks as above); every chunk of it decodes to
 * chunk_planes * chunk_y * chunk_x samples in C order, slice-major (edge chunks along the
 * leading axes are full, as in x and y; blosc nbytes = that product * bytes per sample, which
 * must be <= 2^31 - 1).  A plane's SLICE is its index inside the chunk: the C-order flattening
 * of (index mod chunk extent) over the leading axes -- chunks [1, 2, 4, cy, cx] give
 * slice = (c % 2) * 4 + z % 4. */
typedef struct pbx_zarr_slice { uint32_t layer, slice; } pbx_zarr_slice;
/* pbx_planes_register_zarr for deep chunks: plane k (descs[k]) is slice refs[k].slice of every
 * chunk of layers[refs[k].layer], whose chunks hold chunk_planes[layer] planes.  Every chunk
 * is uploaded and decoded ONCE, however many planes are cut from it.  Keys, statuses and
 * all-or-none are pbx_planes_register_zarr's; 400 also for a slice >= chunk_planes,
 * chunk_planes < 1, a layer that no plane names, and planes of one layer that disagree on
 * size, pixel type or byte order.  blosc blocks (compressed independently) that hold no byte
 * of a wanted slice are not decoded.  With every chunk_planes == 1 this is
 * pbx_planes_register_zarr of chunks[k] = layers[refs[k].layer]. */
int pbx_planes_register_zarr_deep(pbx_ctx* ctx, uint64_t n, const pbx_plane_desc* descs,
                                  const pbx_zarr_slice* refs, uint64_t n_layers,
                                  const pbx_zarr_chunks* layers, const int32_t* chunk_planes,
                                  uint64_t* plane_ids, double* kernel_ms);
/* pbx_band_write_zarr from chunks that hold chunk_planes planes: the rows come from slice
 * `slice` of the covering chunk rows.  Every rule of pbx_band_write_zarr holds; only the blosc
 * blocks that hold a byte of the slice's wanted rows are decoded (zlib, gzip, zstd and raw chunks and
 * memcpyed frames are taken whole).  400 for chunk_planes < 1 or slice outside
 * [0, chunk_planes).  chunk_planes == 1 is pbx_band_write_zarr. */
int pbx_band_write_zarr_deep(pbx_ctx* ctx, uint64_t plane_id, int32_t y0, int32_t rows,
                             const pbx_zarr_chunks* chunks, int32_t chunk_planes, int32_t slice,
                             double* kernel_ms);
/* TIFF / OME-TIFF planes.  For an image without an NGFF fileset the reference's
 * ZarrPixelsService (config.yaml:18) falls back to the ordinary OMERO PixelsService: Bio-Formats
 * pixel buffers over the original files, whose getTileDirect decompresses strips or tiles on the
 * CPU for every request (TileRequestHandler.java:201-211 getPixelBuffer, :107-109).  Here the
 * caller reads the file's IFD and hands over the plane's segments as they lie in the file; they
 * are decoded ONCE on the GPU into a resident plane, which then serves tiles like any other:
 *   NONE     segments copied (k_zarr_copy);
 *   LZW      TIFF 6.0 section 13 (MSB-first codes, "early change"), k_tiff_lzw, one wave a segment;
 *   DEFLATE  zlib streams (compression 8, and 32946 which the caller maps to 8), k_zarr_inflate2,
 *            Adler-32 checked;
 *   ZSTD     one Zstandard frame a segment (compression 50000: libtiff >= 4.0.10, tifffile, GDAL),
 *            k_zarr_zstd; the frame's header and block headers are checked on the host first (no
 *            dictionary id, no skippable frame, nothing after the frame, a content size -- if the
 *            frame carries one -- equal to the segment's decoded bytes), its content checksum and
 *            decoded length on the device;
 * then Predictor = 2 (horizontal differencing over whole samples in the file's byte order) is
 * undone per segment row (k_tiff_unpred) and k_zarr_place puts the segments into the plane.
 * Predictor = 3, the floating-point predictor (Adobe TIFF Technical Note 3), is accepted on float
 * and double planes of one sample per pixel, behind every compression: a segment row is stored
 * as byte planes (most significant bytes first in II and MM files alike) differenced byte by byte
 * over the whole row, and k_tiff_fpunpred_place undoes the differences, interleaves the planes
 * into samples in the file's byte order and places them, at registration and in band writes
 * alike (no k_tiff_unpred, no k_zarr_place; stored segments are read where they were uploaded).
 * pbx_band_write_tiff loads a sparse plane band by band from the segment rows a band covers.
 * Files with 2 .. 4 samples per pixel (RGB, RGBA) give one plane per sample: chunky segments
 * (PlanarConfiguration 1) through pbx_planes_register_tiff_samples / pbx_band_write_tiff_sample,
 * which split them on the GPU (k_tiff_split_place); planar ones (PlanarConfiguration 2) are
 * single-sample segments already and go through the calls below.
 * Bit-packed samples (BitsPerSample 1 .. 7 and 9 .. 15: masks, 4-bit gray, 10- / 12- / 14-bit
 * camera data), PackBits segments (Compression 32773) and FillOrder 2 go through the
 * pbx_*_tiff_packed calls further down and through no other: the calls here keep answering 400 for
 * compression 32773, and take whole-byte samples only.
 * Not supported (400 by the caller or here): SamplesPerPixel > 4, Predictor 3 on integer or
 * chunky multi-sample (RGB float) data, half-precision samples, pre-6.0 (LSB-first)
 * LZW streams, CCITT / Group 4 / LZMA / LERC / WebP / JPEG XR and other compressions, CMYK /
 * palette colour, WhiteIsZero inversion, Predictor 2 on bit-packed samples, samples that differ
 * in width.  JPEG 2000, lossless (the reversible 5/3 path) and
 * lossy (the irreversible 9/7 path, "JPEG-2000 Lossy", Aperio's 33003 / 33005), goes through the
 * pbx_*_tiff_j2k calls further down and through no other; Aperio's habit of YCbCr components
 * outside the codestream is undone only where the caller says so (PBX_TIFF_F_J2K_YCBCR; without it
 * components are stored as decoded).
 * JPEG (Compression 7, baseline, 8-bit, gray / RGB /
 * YCbCr) goes through the pbx_*_tiff_jpeg calls further down and through no other: old-style JPEG
 * (Compression 6), progressive, lossless, arithmetic-coded and 12-bit streams, YCbCr under any
 * other compression, and the Aperio habit of YCbCr data under PhotometricInterpretation 2 (stored
 * as it is, libtiff's rule) are not supported.
 * The JNI shim does not wrap these calls (as the deep Zarr calls). */
enum pbx_tiff_compression { PBX_TIFF_JPEG = 7 /* through the pbx_*_tiff_jpeg calls only */,
                            PBX_TIFF_J2K = 34712 /* through the pbx_*_tiff_j2k calls only */,
                            PBX_TIFF_PACKBITS = 32773 /* through the pbx_*_tiff_packed calls only */,
                            PBX_TIFF_NONE = 1, PBX_TIFF_LZW = 5, PBX_TIFF_DEFLATE = 8, PBX_TIFF_ZSTD = 50000 };
/* pbx_tiff_segments.flags.  J2K_PACKETS: the full packet structure of a JPEG 2000 codestream --
 * 1 .. 64 quality layers, any precinct sizes, SOP and EPH markers (see the JPEG 2000 calls below).
 * Taken by pbx_planes_register_tiff_j2k, pbx_band_write_tiff_j2k and the two pbx_test_tiff_j2k_*
 * hooks and by no other call; without it those four refuse such streams by name, as they always
 * have. */
#define PBX_TIFF_F_J2K_PACKETS 1
/* J2K_SUBSAMPLED: three components of precision 8 whose second and third are stored at half width
 * and / or half height (XRsiz x YRsiz 2 x 1, 1 x 2 or 2 x 2, the same for both; the first 1 x 1;
 * no multiple-component transform).  J2K_YCBCR: the three components are Y, Cb and Cr with no
 * colour transform declared in the codestream (Aperio's 33003, PhotometricInterpretation 6) and are
 * converted to RGB.  Both are taken by the same four calls and by no other; bit 2 (value 2) is not
 * assigned.  See the JPEG 2000 calls below. */
#define PBX_TIFF_F_J2K_SUBSAMPLED 4
#define PBX_TIFF_F_J2K_YCBCR 8
typedef struct pbx_tiff_segments {
    int32_t seg_w, seg_h;       /* tiles: TileWidth x TileLength (edge tiles are full, padded);
                                   strips: ImageWidth x RowsPerStrip (the last strip holds only
                                   the rows left) */
    int32_t tiled;              /* 0 strips, else tiles */
    int32_t compression;        /* enum pbx_tiff_compression */
    int32_t predictor;          /* 1 none, 2 horizontal differencing (integer samples only),
                                   3 floating-point (float / double planes, one sample a pixel) */
    int32_t flags;              /* PBX_TIFF_F_*; 0 = none */
    const uint8_t* data;        /* the segments' bytes, concatenated in C order over the grid */
    const uint64_t* offsets;    /* gx * gy + 1 offsets into data (as pbx_zarr_chunks); a strip
                                   image has gx = 1 */
} pbx_tiff_segments;            /* 40 bytes */
/* n planes from their TIFF segments in ONE set of launches, as pbx_planes_register_zarr: keys,
 * statuses, pinned staging and all-or-none are the same.  descs[k].byte_order is the FILE's byte
 * order (II little, MM big): the plane keeps it, nothing is swapped at load time.
 * 400 on the host for: null pointers, offsets that decrease, an empty segment (TIFF has no missing
 * chunk), seg_w / seg_h < 1, tiles whose width or length is not a multiple of 16 (TIFF 6.0
 * section 15), a strip width != size_x, a compression outside {1, 5, 8, 50000}, a predictor
 * outside {1, 2, 3}, predictor 2 on float / double, predictor 3 on anything but a float / double
 * plane of one sample per pixel ("bad predictor 3 ..."), a zstd segment that is not exactly one
 * frame decoding to the segment's bytes, flags != 0, an uncompressed segment whose length is not
 * its rows' bytes, an old-style LZW stream (first byte 0 and bit 0 of the second set: libtiff's
 * test).  A stream the device rejects (bad LZW code, fewer bytes than the segment holds, bad
 * deflate data or Adler-32, corrupt zstd data or content checksum) is 400 and nothing is registered.  A missing LZW EOI is accepted, as
 * libtiff accepts it.  kernel_ms (may be NULL): [0] decoders + un-predictor, [1] placement. */
int pbx_planes_register_tiff(pbx_ctx* ctx, uint64_t n, const pbx_plane_desc* descs,
                             const pbx_tiff_segments* segs, uint64_t* plane_ids, double* kernel_ms);
/* Rows [y0, y0 + rows) of ONE band of a sparse plane, decoded on the GPU from the TIFF strips or
 * tile rows that cover them: pbx_band_write_zarr for a plane stored as TIFF, so a cold tile of a
 * whole slide costs the segments of its bands and not the plane's (the Bio-Formats buffers decode
 * only the strips or tiles a region touches, TileRequestHandler.java:102-109).  `segs` is as for
 * pbx_planes_register_tiff except that data / offsets hold only segment rows sr0 = y0 / seg_h up
 * to (not including) sr1 = ceil((y0 + rows) / seg_h), each full width (gx segments; gx = 1 for
 * strips) in C order: (sr1 - sr0) * gx + 1 offsets.  A strip's row count follows the plane: the
 * last strip holds size_y - its first row.  Rows of those segments outside [y0, y0 + rows) are
 * decoded (LZW and deflate are serial) but neither un-predicted nor written, so band_rows need
 * not be a multiple of seg_h, a band may be written in pieces at any rows, and a segment row that
 * straddles two bands is decoded once for each.  The bytes land in the plane's stored byte order:
 * create the sparse plane with source PBX_SRC_HOST and the FILE's byte order; predictor sums use
 * that order, as at registration.  Stored segments are read where they were uploaded (no copy, no
 * scratch); with Predictor = 2 one kernel (k_tiff_unpred_place) undoes the differencing on the way
 * from the decoded segment into the band.  Band states, statuses (400 rows outside one band or a
 * plane that is not sparse, 409 resident band, 507 no room) and failure handling are
 * pbx_band_write's, and pieces written by any of the three band calls may be mixed in one band.
 * Every host-side refusal of pbx_planes_register_tiff applies to the covered segments (segment
 * numbers count from the first one handed over): 400, and the band is left as it was.  A stream
 * the device rejects is 400 and fails the band's load like a failed upload.  Upload, decode and
 * placement run on the upload stream.  kernel_ms (may be NULL): [0] device ms of the decoders
 * (about 0 for stored segments, which launch none), [1] of the placement. */
int pbx_band_write_tiff(pbx_ctx* ctx, uint64_t plane_id, int32_t y0, int32_t rows,
                        const pbx_tiff_segments* segs, double* kernel_ms);
/* Chunky multi-sample segments (SamplesPerPixel S = 2 .. 4, PlanarConfiguration 1: RGB, RGBA and
 * the like), one plane per sample, modelled on the deep-Zarr pair.  Plane k (descs[k]) is sample
 * refs[k].slice of layers[refs[k].layer], whose segments hold samples_per_pixel[layer]
 * interleaved samples per pixel: a segment row is seg_w * S samples and an uncompressed segment
 * seg_w * rows * bpp * S bytes.  Each layer is uploaded and decoded ONCE; k_tiff_split_place then
 * undoes Predictor = 2 with a stride of S samples (every sample is differenced against the same
 * component of the pixel before, TIFF 6.0 section 14) and scatters the components into their
 * planes in one pass.  Keys, all-or-none registration, statuses, staging and every segment
 * refusal are pbx_planes_register_tiff's, and with every samples_per_pixel == 1 the call is that
 * call.  400 also for: samples_per_pixel outside 1 .. 4, a sample >= S, S > 1 on 64-bit samples
 * (double), a layer no plane names, two planes naming the same sample of a layer, planes of one
 * layer that disagree on size, type or byte order.  Not every sample of a layer need be named:
 * the others are decoded (they are interleaved) but stored nowhere. */
int pbx_planes_register_tiff_samples(pbx_ctx* ctx, uint64_t n, const pbx_plane_desc* descs,
                                     const pbx_zarr_slice* refs, uint64_t n_layers,
                                     const pbx_tiff_segments* layers, const int32_t* samples_per_pixel,
                                     uint64_t* plane_ids, double* kernel_ms);
/* pbx_band_write_tiff for chunky segments of samples_per_pixel samples per pixel: the covering
 * segment rows are decoded for this call and only sample `sample` is written, into the band of
 * `plane_id` (one plane per call, as pbx_band_write_zarr_deep: a cold region of all S channels
 * decodes its segments S times through this call, once through pbx_band_write_tiff_group).
 * Stored segments are read where they were uploaded.  With samples_per_pixel == 1 (sample 0) this
 * is pbx_band_write_tiff.  400 as that call and as pbx_planes_register_tiff_samples. */
int pbx_band_write_tiff_sample(pbx_ctx* ctx, uint64_t plane_id, int32_t y0, int32_t rows,
                               const pbx_tiff_segments* segs, int32_t samples_per_pixel, int32_t sample,
                               double* kernel_ms);
/* JPEG-compressed segments (Compression = 7, TIFF Technical Note 2; DESIGN.md §10b "JPEG
 * segments"): every strip or tile is a baseline sequential Huffman JPEG stream (SOF0, 8-bit, one
 * scan of all components) of exactly the segment's size -- TileWidth x TileLength, or ImageWidth
 * x the strip's own row count -- with its tables in the IFD's JPEGTables (tag 347: SOI, DQT / DHT,
 * EOI) and / or in the stream itself, whose own override.  The host reads marker segments only;
 * entropy decoding (restart intervals, FF 00 stuffing, fill bytes), dequantisation and the
 * accurate integer IDCT run in k_tiff_jpeg_decode, one wave per segment, and k_tiff_jpeg_place
 * upsamples ("fancy" triangle filter), converts and places.  The arithmetic is libjpeg's, so the
 * planes equal libjpeg-turbo's (libtiff, PIL; by assumption javax.imageio and so Bio-Formats) byte
 * for byte as long as no IDCT output leaves [-512, 511] before the clamp.
 * Components: 1 (samples_per_pixel 1), or 3 (samples_per_pixel 3, chunky) which are converted
 * YCbCr -> RGB if and only if ycbcr is set (PhotometricInterpretation 6; libtiff's rule) and are
 * otherwise stored as they are; sampling 1x1, and under ycbcr also 2x1 or 2x2 luma over 1x1 chroma
 * (taken from the SOF, not from tag 530).  Planar files hand over each sample's segments as
 * one-sample segments. */
typedef struct pbx_tiff_jpeg {
    const uint8_t* tables;   /* tag 347's bytes, or NULL */
    uint64_t tables_len;
    int32_t ycbcr;           /* 1: PhotometricInterpretation 6, convert to RGB */
    int32_t reserved;        /* 0 */
} pbx_tiff_jpeg;             /* 24 bytes */
/* pbx_planes_register_tiff_samples for JPEG layers, jpeg[l] going with layers[l].  In these calls
 * compression must be 7, predictor 1 and every plane PBX_UINT8 (the other TIFF calls keep
 * answering "bad compression 7").  Keys, all-or-none, staging, statuses and kernel_ms ([0] decode,
 * [1] placement) are shared with that call.  400 on the host, before anything is uploaded, names:
 * a segment or tables stream that does not start with SOI or whose header is cut short, SOF1 /
 * SOF2 / SOF3 and arithmetic coding, precision != 8, 4 components, sampling factors outside the
 * three above, subsampling without ycbcr, ycbcr with samples_per_pixel != 3, more than one scan,
 * SOF size != segment size, a missing quantiser or Huffman table, an over-subscribed Huffman
 * table, a 16-bit quantiser.  400 from the device (nothing registered): entropy data that ends
 * before the last MCU, a code in no table, a run past coefficient 63, a DC size > 11 or an AC
 * size > 10, a restart marker missing, out of sequence or misplaced. */
int pbx_planes_register_tiff_jpeg(pbx_ctx* ctx, uint64_t n, const pbx_plane_desc* descs,
                                  const pbx_zarr_slice* refs, uint64_t n_layers,
                                  const pbx_tiff_segments* layers, const int32_t* samples_per_pixel,
                                  const pbx_tiff_jpeg* jpeg, uint64_t* plane_ids, double* kernel_ms);
/* pbx_band_write_tiff_sample for JPEG segments: the covering segment rows are decoded for this
 * call and sample `sample` alone is stored.  A device refusal fails the band's load as a bad LZW
 * stream does. */
int pbx_band_write_tiff_jpeg(pbx_ctx* ctx, uint64_t plane_id, int32_t y0, int32_t rows,
                             const pbx_tiff_segments* segs, int32_t samples_per_pixel, int32_t sample,
                             const pbx_tiff_jpeg* jpeg, double* kernel_ms);
/* JPEG 2000 segments (TIFF Compression 33003, 33004, 33005 and 34712, which all hand over as
 * compression = PBX_TIFF_J2K; DESIGN.md section 10b "JPEG 2000 segments"): every strip or tile is
 * one raw codestream (FF4F FF51 ...) of one tile of exactly the segment's size -- TileWidth x
 * TileLength, or ImageWidth x the strip's own row count.  Two paths, chosen per segment by its COD
 * (layers of one registration may mix them).  The reversible one: the 5/3 wavelet, QCD style 0 (no
 * quantisation), optionally the reversible colour transform; the planes equal the encoder's input
 * bit for bit.  The irreversible one: the 9/7 wavelet with QCD style 1 or 2 (scalar quantisation,
 * the steps derived from the LL band's or given per sub-band), optionally the irreversible colour
 * transform; T.800's arithmetic in float32 -- midpoint reconstruction of what the coded passes
 * leave open, step = 2^(P + gain - exponent) (1 + mantissa / 2048), the lifting constants of
 * F.3.8, "+ 2^(P-1)", round half to even, clamp -- so a plane equals the rounding of the exact
 * (float64) values except where those lie within 1/64 (8 bits) or 1/8 (16 bits) of a half, and
 * there differs by at most 1.  OpenJPEG's output is within 1 of it at 8 bits and within 3 at 16
 * (its decoder's own high-band constant).  The host reads SIZ, COD and QCD only; packet headers
 * (k_tiff_j2k_packets), the MQ and bit-plane decoder (k_tiff_j2k_blocks, one wave per code block),
 * the inverse wavelet (k_tiff_j2k_idwt, k_tiff_j2k_idwt97) and the colour transform, level shift
 * and placement (k_tiff_j2k_place) run on the device.
 * Components: 1 (samples_per_pixel 1) of precision 8 on a PBX_UINT8 plane or 16 on a PBX_UINT16
 * plane, or 3 (samples_per_pixel 3, chunky) of precision 8, stored as they are or through the
 * inverse RCT (5/3) or ICT (9/7) as the COD says.  0 .. 32 levels, any code-block size, all five progression orders,
 * one layer, one precinct per resolution, code-block style 0; COM, TLM, PLM and PLT are skipped.
 * With flags = PBX_TIFF_F_J2K_PACKETS also: 1 .. 64 quality layers, any declared precinct sizes
 * (precincts smaller than the code block clip it, T.800 B.7; exponent 0 at resolution 0 only), and
 * Scod bits 1 and 2 -- an SOP marker segment may stand before a packet (its Nsop is not verified),
 * an EPH marker must follow every packet header.  The host then writes down the stream's packets in
 * the order its progression gives (T.800 B.12); tier 2 walks that list, and a block whose bytes lie
 * in several packets has them copied into one run first (k_tiff_j2k_gather).  Without the flag
 * those streams are refused by name: "N quality layers (1)", "more than one precinct in resolution
 * R", "SOP or EPH markers".  With it: "N quality layers (1 .. 64)", "too many packets", "too many
 * block contributions"; a missing EPH is device code 2.
 * With PBX_TIFF_F_J2K_SUBSAMPLED (alone or with the other flags, on both paths) also streams of
 * three components of precision 8 whose components 1 and 2 share the sampling factors 2 x 1, 1 x 2
 * or 2 x 2 while component 0 is 1 x 1 and the multiple-component transform is 0.  Component c then
 * measures ceil(W / XRsiz) x ceil(H / YRsiz); its resolutions, sub-bands, code blocks, precincts,
 * scratch planes and inverse wavelet have that size, and the packet list's position loops (T.800
 * B.12.1.3 - 5) step by XRsiz 2^(PPx + NL - r) and YRsiz 2^(PPy + NL - r).  Upsampling is
 * replication: plane sample (x, y) of component c is component sample (x / XRsiz, y / YRsiz), as
 * OpenJPEG, Pillow and OpenSlide do for JPEG 2000 -- T.800 places a component sample on the
 * reference grid at multiples of XRsiz and YRsiz and defines no chroma siting; libjpeg's triangle
 * filter ("fancy upsampling", which the JPEG calls above use) is not used here.  Without the flag
 * such streams are refused as ever: "subsampled components (component C: X x Y)".  With it, by
 * name: "subsampling on a stream of one component", "subsampled first component", "sampling
 * factors X x Y on component C (2 x 1, 1 x 2 or 2 x 2)", "chroma components of different sampling
 * factors", "subsampled components (X x Y) with the multiple-component transform".
 * With PBX_TIFF_F_J2K_YCBCR the three components are converted to RGB after level shift, rounding
 * and clamp to uint8, by libjpeg's jdcolor.c 16-bit fixed point (the arithmetic of the JPEG calls'
 * ycbcr), with or without subsampling, on both paths; only the samples a call names are stored.
 * It needs samples_per_pixel 3 on a PBX_UINT8 plane and streams without the multiple-component
 * transform: "YCbCr conversion (PBX_TIFF_F_J2K_YCBCR) on ..." otherwise.  Segments with either
 * flag's property are placed by k_tiff_j2k_place_chroma.
 * Refused either way: more than one tile or
 * tile-part, code-block style bits, COC / QCC / POC / RGN / PPM / PPT / CRG, offsets, sampling
 * factors other than the three above, a subsampled first component, signed components, the JP2
 * wrapper.
 * pbx_planes_register_tiff_samples for such layers: compression must be PBX_TIFF_J2K and
 * predictor 1 (the other TIFF calls keep answering "bad compression 34712").  Keys, all-or-none,
 * staging, statuses and kernel_ms ([0] decode through the inverse wavelet, [1] placement) are
 * shared with that call.  400 on the host, before anything is uploaded, names: a jp2 box instead
 * of a codestream, a header cut short, the irreversible wavelet with quantisation style 0 and
 * quantisation style 1 or 2 with the reversible one, a QCD whose length does not fit its style and
 * the levels, more than 30 magnitude bit-planes on a 9/7 sub-band (31 on a 5/3 one), a style-1
 * exponent that goes negative, more than one layer, tile or tile-part, non-zero offsets, subsampled or signed components, a
 * precision other than 8 or 16, three components at precision 16, 2 or more than 3 components, a
 * SIZ size that is not the segment's, any code-block style bit, SOP or EPH markers, COC / QCC /
 * POC / RGN / PPM / PPT / CRG markers, more than one precinct in a resolution.  400 from the
 * device (nothing registered): "corrupt segment stream N (j2k, decoder code C)", C = 1 a packet
 * header or packet data past the stream's end, 2 a malformed packet header, 3 zero bit-planes
 * above the band's magnitude bit-planes or more passes than the bit-planes allow. */
int pbx_planes_register_tiff_j2k(pbx_ctx* ctx, uint64_t n, const pbx_plane_desc* descs,
                                 const pbx_zarr_slice* refs, uint64_t n_layers,
                                 const pbx_tiff_segments* layers, const int32_t* samples_per_pixel,
                                 uint64_t* plane_ids, double* kernel_ms);
/* pbx_band_write_tiff_sample for JPEG 2000 segments: the covering segment rows are decoded for
 * this call and sample `sample` alone is stored.  A device refusal fails the band's load as a bad
 * LZW stream does. */
int pbx_band_write_tiff_j2k(pbx_ctx* ctx, uint64_t plane_id, int32_t y0, int32_t rows,
                            const pbx_tiff_segments* segs, int32_t samples_per_pixel, int32_t sample,
                            double* kernel_ms);
/* Bit-packed samples, PackBits and FillOrder 2 (DESIGN.md §10b "packed samples and PackBits").
 * A segment row is a bit stream of seg_w * S samples of `bits` bits each (1 .. 16), most
 * significant bit first in II and MM files alike, padded to a whole byte: ceil(seg_w * S * bits
 * / 8) bytes a row, and an uncompressed segment is its rows times that.  With fill_order 2 the
 * bits of every byte are reversed first (TIFF 6.0 FillOrder).  Values are stored unscaled, as
 * Bio-Formats hands them to the reference: bits 1 .. 8 on an 8-bit integer plane, 9 .. 16 on a
 * 16-bit one, in the plane's byte order (descs[k].byte_order; 16-bit samples are whole bytes in
 * the file's order and keep it, so give the file's as in the other TIFF calls).  Sample i of a
 * row is component i % S of pixel i / S and goes to that component's plane
 * (k_tiff_unpack_place: one pass from the segment into up to four planes, tile padding and rows
 * outside the band clipped).  Compression is 1, 5, 8, 50000 as in pbx_planes_register_tiff, or
 * PBX_TIFF_PACKBITS (TIFF 6.0 section 9; k_tiff_packbits, one wave a segment: runs may cross
 * rows, bytes after the segment's last row are not read).  With bits 8 or 16 the placement is a
 * plain one: that is how PackBits files of ordinary samples are loaded. */
typedef struct pbx_tiff_packed {
    int32_t bits;               /* BitsPerSample, 1 .. 16 */
    int32_t fill_order;         /* 1 (MSB first), 2 (the bits of every byte reversed) */
    int32_t samples_per_pixel;  /* S, 1 .. 4: chunky samples of a segment row */
    int32_t sample;             /* pbx_band_write_tiff_packed: the sample the plane is, 0 .. S - 1;
                                   a registration takes it from refs[k].slice instead */
} pbx_tiff_packed;              /* 16 bytes */
/* pbx_planes_register_tiff_samples for such layers, packed[l] going with layers[l]: plane k is
 * sample refs[k].slice of layer refs[k].layer.  Keys, all-or-none registration, statuses, staging
 * and kernel_ms ([0] decoders, [1] placement) are that call's, stored segments are read where
 * they were uploaded.  400 on the host names: bits outside 1 .. 16, bits that do not fit the
 * plane's pixel type, fill_order outside {1, 2}, fill_order 2 with bits 16, a predictor other than
 * 1 (libtiff defines the predictor on whole-byte samples only), flags != 0, samples_per_pixel
 * outside 1 .. 4, a sample >= S, a compression outside {1, 5, 8, 50000, 32773}, and every other
 * refusal of pbx_planes_register_tiff (segment shape, tile size, strip width, offsets, empty
 * segments, an uncompressed segment that is not its rows' padded bytes, old-style LZW, zstd
 * framing).  400 from the device, nothing registered: "corrupt chunk stream N (packbits, decoder
 * code C)", C = 1 the stream ends before the segment's bytes are out, 3 a run that would write
 * past them; the other decoders' as before. */
int pbx_planes_register_tiff_packed(pbx_ctx* ctx, uint64_t n, const pbx_plane_desc* descs,
                                    const pbx_zarr_slice* refs, uint64_t n_layers,
                                    const pbx_tiff_segments* layers, const pbx_tiff_packed* packed,
                                    uint64_t* plane_ids, double* kernel_ms);
/* pbx_band_write_tiff_sample for such segments: the covering segment rows are decoded for this
 * call and sample packed->sample alone is stored.  Band states, statuses and failure handling are
 * pbx_band_write's, and pieces written by any band call may be mixed in one band. */
int pbx_band_write_tiff_packed(pbx_ctx* ctx, uint64_t plane_id, int32_t y0, int32_t rows,
                               const pbx_tiff_segments* segs, const pbx_tiff_packed* packed,
                               double* kernel_ms);
/* Band writes that span planes: ONE upload, decode and placement fills the bands of up to four
 * sparse planes that share the segments (the samples of chunky TIFF segments) or the chunks (the
 * slices of Zarr chunks that hold several planes), so that a cold RGB region costs one decode and
 * not three (DESIGN.md §10b "A band load that spans planes").
 * pbx_band_write_tiff_group: n is the segments' samples per pixel, 1 .. 4 (packed segments:
 * packed->samples_per_pixel, packed->sample is ignored); plane_ids[s] is the plane of sample s, 0 =
 * nobody wants that sample.  jpeg: NULL unless Compression 7; j2k non-zero: JPEG 2000 segments;
 * packed: NULL unless the rows are bit-packed / PackBits / FillOrder 2 -- the codec is chosen as the
 * four single calls choose it.
 * pbx_band_write_zarr_group: plane_ids[i] receives slice slices[i] of the covering chunk rows, n is
 * 1 .. 4, the slices are distinct and lie in [0, chunk_planes).
 * Both: plane_ids[primary] (a wanted id) is the plane the caller needs; the others are siblings,
 * filled if they can be.  All members are admitted in one critical section by pbx_band_write's
 * rule.  If the primary is kept out, no sibling is joined, nothing is uploaded or decoded and its
 * status is returned; a sibling that is kept out (resident: 409, being allocated or reset by
 * another caller: 409, reset as stale and the piece not at the band's first row: 500), or whose
 * band does not fit the residency budget (507, allocated after the primary's), is dropped and the
 * rest is written.  A failure of the one fill (an upload error, a stream a decoder rejects: 400)
 * fails the load of every band the call joined; each is reset by its last writer.  The return
 * value is what the corresponding single call on plane_ids[primary] would have returned, so a
 * binding's handling of 400 / 404 / 409 / 500 / 507 does not change.  statuses[i] (may be NULL):
 * PBX_OK (written), the status that kept member i out (409, 500, 507), the failure's status for
 * a member the failed call had joined, -1 for an id of 0 or a sibling never attempted.  kernel_ms
 * as in the single calls.  With n == 1 the calls are the single calls.
 * 400 before anything is joined: null arguments, n outside 1 .. 4 or (packed) not the segments'
 * samples per pixel, primary out of range or naming an id of 0, the same id (or slice) twice, a
 * plane that is not sparse, members that disagree on size, pixel type, byte order or band_rows or
 * whose rows do not lie in one band, and every refusal of the single calls.  404: an unknown id.
 * Pieces written by any band call may be mixed in one band; a loader that wants a sibling's band
 * completed uses the group call for every piece of it, and a sibling left partly written goes
 * stale like any abandoned load. */
int pbx_band_write_tiff_group(pbx_ctx* ctx, const uint64_t* plane_ids, int32_t n, int32_t primary,
                              int32_t y0, int32_t rows, const pbx_tiff_segments* segs,
                              const pbx_tiff_jpeg* jpeg, int32_t j2k, const pbx_tiff_packed* packed,
                              int32_t* statuses, double* kernel_ms);
int pbx_band_write_zarr_group(pbx_ctx* ctx, const uint64_t* plane_ids, const int32_t* slices, int32_t n,
                              int32_t primary, int32_t y0, int32_t rows, const pbx_zarr_chunks* z,
                              int32_t chunk_planes, int32_t* statuses, double* kernel_ms);
/* A band of a derived resolution level (DESIGN.md §10b "Derived levels"): rows [y0, y0 + rows) of
 * one band of the sparse plane plane_id, stored level r + k, are made on the GPU from the resident
 * rows of src_plane_id, stored level r, bit for bit what pbx_plane_build_pyramid would have put
 * there: k (1 .. 4) applications of its rule -- each level has size ((n + 1) / 2) per axis and a
 * sample is the mean of (2x, 2y), (min(2x + 1, n_x - 1), 2y), (2x, min(2y + 1, n_y - 1)) and the
 * diagonal of the level above, the clamp taken at every level -- in one kernel, no level in between
 * written to memory.  So the piece reads source rows [y0 << k, min((y0 + rows) << k, size_y)) and
 * no others.  The contract is pbx_band_write's: any piece inside one band, the first write
 * allocates (residency budget, eviction), the last one publishes; pieces written by any band call
 * may be mixed in one band.
 * The source is another plane of the same image, z, c, t, pixel type and byte order, of stored
 * level r = the destination's - k, whose size reduces to the destination's by the rule above: a
 * sparse plane (its band_rows need not be the destination's) or a whole dense READY plane.  Every
 * source band that holds a needed row must be resident; they are pinned from the check until the
 * kernel has finished and stamped as a batch that read them stamps them (least recently used
 * order; no longer "fresh").
 * 400: k outside 1 .. 4, src_plane_id == plane_id, a source of another image / z / c / t / pixel
 * type / byte order / level or of a size that does not reduce to the destination's, a dense source
 * that is a row band or still loading, a destination that is not a sparse plane, rows outside the
 * plane or leaving their band.  404: an unknown id.  PBX_E_NOT_RESIDENT: a needed source band (or
 * an evicted dense source) is not resident -- the destination band stays as it was, nothing is
 * allocated, and pbx_last_error names the first missing source rows; the binding loads them and
 * calls again.  409 / 500 / 507: exactly as pbx_band_write (pbx_test_fail_band_write counts this
 * call too). */
int pbx_band_write_reduced(pbx_ctx* ctx, uint64_t plane_id, int32_t y0, int32_t rows,
                           uint64_t src_plane_id, int32_t k);
/* Copy a registered plane back to the host, samples in big-endian order (test hook). */
int pbx_plane_read_be(pbx_ctx* ctx, uint64_t plane_id, void* out, uint64_t bytes);

/* TileCtx.resolution == null (TileCtx.java:86-88): the pixel buffer's default level. */
#define PBX_RESOLUTION_NONE (-1)

/* TileCtx (TileCtx.java:36-54, parsed at :67-90). */
typedef struct pbx_tile_req {
    int64_t image_id;
    int32_t z, c, t;
    int32_t resolution;      /* OMERO PixelBuffer.setResolutionLevel numbering
                                (TileRequestHandler.java:89-91): with L stored levels,
                                L-1 = full resolution, 0 = the smallest level; stored level
                                = L-1-resolution.  PBX_RESOLUTION_NONE = not given (full
                                resolution).  Outside [0, L), or any other negative value:
                                setResolutionLevel throws -> getTile null -> 404.  A binding
                                maps a given negative Integer to a value < -1. */
    int32_t x, y, w, h;      /* w/h == 0 -> plane size (TileRequestHandler.java:92-97) */
    int32_t format;          /* enum pbx_format */
    int32_t reserved;
} pbx_tile_req;

/* One response: status plus the exact-length body (TileRequestHandler.java:188-193). */
typedef struct pbx_result {
    int32_t status;          /* enum pbx_status */
    int32_t format;
    int32_t w, h;            /* region after the w/h defaulting (used by the filename header) */
    const uint8_t* data;     /* library-owned; valid until pbx_results_release */
    uint64_t len;
    void* owner;             /* internal */
} pbx_result;

/* Synchronous single tile: TileRequestHandler.getTile (TileRequestHandler.java:80-139).
 * Called from many threads at once (the Vert.x worker pool, PixelBufferVerticle.java:109-110),
 * requests are coalesced: all requests that arrive while the GPU is busy become one batch. */
int pbx_get_tile(pbx_ctx* ctx, const pbx_tile_req* req, pbx_result* out);
/* Synchronous batch: n independent getTile calls executed as one set of GPU launches. */
int pbx_get_tiles(pbx_ctx* ctx, const pbx_tile_req* reqs, uint64_t n, pbx_result* out);
/* Results go back to the context that produced them (ctx may be NULL). */
void pbx_results_release(pbx_ctx* ctx, pbx_result* results, uint64_t n);

/* Stage timings under the reference's tracing span names (TileRequestHandler.java:81
 * "get_tile", :104 "get_tile_direct", :147 "create_metadata", :180 "write_image").  A request is
 * served inside a batch, so the stages are the batch's (HIP events on its kernel stream; the
 * caller times its own get_tile span around pbx_get_tile):
 *   get_tile_direct_ms  the region gather from HBM (raw/TIFF extract kernel); 0 for a PNG-only
 *                       batch, whose gather is fused into the filter/deflate kernels
 *   write_image_ms      PNG row filters + deflate (LZ77, Huffman, encode) of the whole batch
 *   create_metadata_ms  container framing: IHDR/IDAT/IEND or the TIFF IFD, chunk CRCs
 *   batch_ms            the batch's device time, first to last kernel
 *   d2h_ms              host wall time from queuing the batch's device->host copy to its end
 *   batch_tiles         requests in the batch
 * Returns PBX_E_BADARG for a result without a body (error statuses, released results). */
typedef struct pbx_spans {
    double get_tile_direct_ms, write_image_ms, create_metadata_ms, batch_ms, d2h_ms;
    uint64_t batch_tiles;
} pbx_spans;
int pbx_result_spans(const pbx_result* r, pbx_spans* out);

/* Batched async: pbx_submit plans and launches n independent getTile
 * requests and returns at once; pbx_wait blocks until the batch has finished (timeout_us < 0:
 * no limit; 0: poll), fills out[0..n) (the array given to pbx_submit) exactly like
 * pbx_get_tiles and frees the ticket.  On PBX_E_PENDING the ticket stays valid: call again.
 * Batches run in submission order on the context's stream; results are released with
 * pbx_results_release. */
typedef struct pbx_ticket pbx_ticket;
int pbx_submit(pbx_ctx* ctx, const pbx_tile_req* reqs, uint64_t n, pbx_result* out,
               pbx_ticket** ticket);
int pbx_wait(pbx_ctx* ctx, pbx_ticket* ticket, int64_t timeout_us);

/* Device-resident batches: plan once, launch asynchronously on the context's stream,
 * outputs stay in HBM until pbx_batch_fetch.  Used by callers that pipeline requests
 * (and by bench.py, whose timed region is plan+launch+sync of one batch). */
typedef struct pbx_batch pbx_batch;
int pbx_batch_plan(pbx_ctx* ctx, const pbx_tile_req* reqs, uint64_t n, pbx_batch** out);
int pbx_batch_launch(pbx_ctx* ctx, pbx_batch* b);
int pbx_batch_sync(pbx_ctx* ctx, pbx_batch* b);
int pbx_batch_fetch(pbx_ctx* ctx, pbx_batch* b, pbx_result* out);
void pbx_batch_destroy(pbx_ctx* ctx, pbx_batch* b);

typedef struct pbx_batch_stats {
    uint64_t tiles, ok_tiles, png_tiles, raw_tiles, tif_tiles;
    uint64_t in_bytes;       /* w*h*bpp summed over OK tiles */
    uint64_t stream_bytes;   /* bytes fed to deflate (PNG filtered streams, deflate-TIFF) */
    uint64_t out_bytes;      /* total response bytes */
    uint64_t deflate_out_bytes; /* compressed payload bytes (zlib streams) */
    uint64_t segments;
    /* HIP events of the last launch: extract (raw/TIFF), filter (PNG rows), deflate (LZ77 ..
     * encode, all segments), assemble (container framing), total; then the deflate parts */
    double ms_extract, ms_filter, ms_deflate, ms_assemble, ms_total;
    double ms_lz77, ms_huff, ms_encode;
    uint64_t blocks;         /* deflate blocks (segments sharing one Huffman code) */
    /* adaptive-filter PNG tiles in the None mode read by k_lz77 straight from the plane (no
     * filter pass), and their bytes as in_bytes + stream_bytes count them */
    uint64_t direct_tiles, direct_bytes;
} pbx_batch_stats;
int pbx_batch_stats_get(pbx_ctx* ctx, pbx_batch* b, pbx_batch_stats* out);

/* Reply metadata. */
/* "image%d_z%d_c%d_t%d_x%d_y%d_w%d_h%d.%s" (PixelBufferVerticle.java:118-126), ext "bin" when
 * format is raw.  format_str is the caller's original TileCtx.format (may be NULL). */
int pbx_tile_filename(const pbx_tile_req* req, int32_t w, int32_t h, const char* format_str,
                      char* out, uint64_t cap);
/* PixelBufferMicroserviceVerticle.java:373-379. */
const char* pbx_content_type(const char* format_str);
/* TileCtx.format string -> enum pbx_format (null -> RAW). */
int pbx_format_from_string(const char* format_str);
int pbx_pixel_type_from_string(const char* name);
int pbx_bytes_per_pixel(int32_t pixel_type);

/* Batches launched and requests served so far by this context (coalescing check). */
int pbx_ctx_stats_get(pbx_ctx* ctx, uint64_t* batches, uint64_t* requests);

/* Free the context's cached (currently unused) device and pinned batch buffers; buffers
 * of batches still alive stay (torch.cuda.empty_cache analogue). */
int pbx_release_cached(pbx_ctx* ctx);

/* Synchronise the context's device (bench/test hook). */
int pbx_device_synchronize(pbx_ctx* ctx);

/* Pipelined batches (pbx_batch_launch, pbx_submit) with deflate work alternate over
 * `streams` kernel streams (1..4; default 3, or $PBX_KSTREAMS), each starting behind the
 * previous batch's stage `stagger` (1 = after its k_lz77 (default), 2 k_huff, 3 the
 * offsets scan, 4 k_encode; 0 = no wait), so one batch's latency-bound phases overlap
 * the next batch's kernels.  streams = 1: every batch in launch order on one stream
 * (per-kernel timings then have no overlap).  Synchronous calls (pbx_get_tile(s)) and
 * batches without deflate work always use the one stream.  No reference counterpart
 * (the reference runs one request per worker thread). */
int pbx_set_kernel_streams(pbx_ctx* ctx, int32_t streams, int32_t stagger);

/* Deflate strategy of every deflate tile (PNG under any filter setting, deflate-TIFF, tiled
 * deflate-TIFF).  The reference writes PNG through java.util.zip.Deflater with the default
 * level and strategy (TileRequestHandler.java:176-199), which searches for matches: DEFAULT
 * does, and stays the default.
 *   DEFAULT       every 16 KiB segment of a tile's stream is parsed for matches (runs, the
 *                 previous sample, the row above), then Huffman coded.
 *   HUFFMAN_ONLY  no match search at all: literals and a Huffman code, zlib's Z_HUFFMAN_ONLY.
 *                 The same bytes as DEFAULT (+-0.1 %) on noisy or photon-counting data with the
 *                 LZ77 kernel at 0.3 (Poisson counts) to 0.85 (uniform noise) of its time; up to
 *                 100x the bytes on ramps, backgrounds and saturated areas.
 *   AUTO          per segment: parsed unless fewer than 2 % of a sample of its positions
 *                 (one in 32) start a paying match, then Huffman-only.  Never more than
 *                 DEFAULT's bytes + 0.1 % on the measured tile kinds.
 * Every strategy's output is a valid zlib stream of the same pixels.  The initial value is
 * $PBX_DEFLATE_STRATEGY (0 / 1 / 2; any other value: pbx_init answers 400), else DEFAULT.  A
 * batch takes the strategy when it is planned (pbx_batch_plan, pbx_submit, pbx_get_tile(s),
 * the coalescer's batches); a later set does not change a planned batch.  Thread-safe. */
enum pbx_deflate_strategy { PBX_DEFLATE_DEFAULT = 0, PBX_DEFLATE_HUFFMAN_ONLY = 1, PBX_DEFLATE_AUTO = 2 };
int pbx_set_deflate_strategy(pbx_ctx* ctx, int32_t strategy);   /* 400 outside 0..2 */
int pbx_get_deflate_strategy(pbx_ctx* ctx, int32_t* strategy);
/* What a launched batch's LZ77 stage did with each segment.  modes (may be NULL): nseg bytes,
 * 0 = parsed, 1 = Huffman-only, segments in batch order; huffman_only (may be NULL): their
 * count.  400 if nseg != the batch's segment count or the batch has not been launched. */
int pbx_batch_lz_modes(pbx_ctx* ctx, pbx_batch* b, uint8_t* modes, uint64_t nseg, uint64_t* huffman_only);

/* TIFF Predictor (TIFF 6.0 section 14, tag 317) of deflated TIFF responses: format=tif under
 * cfg.tiff_deflate, strips and tiled (cfg.tiff_tile).  The reference's TiffWriter writes no
 * predictor (TileRequestHandler.java:176-199): NONE does not either, and stays the default.
 *   NONE        the big-endian samples are deflated as they are; no tag 317 in the IFD.
 *   HORIZONTAL  every row (of every T x T sub-tile, for tiled TIFF) keeps its first sample and
 *               stores sample i > 0 as (s[i] - s[i-1]) mod 2^bits, subtracted on the sample
 *               value and written big-endian; the zero padding of an edge sub-tile is
 *               differenced like data.  The IFD carries Predictor = 2 (one more entry: a strip
 *               response's data still starts at byte 160, a tiled response's offset arrays at
 *               176).  Smaller on spatially correlated samples (0.9 on photon counts of a smooth
 *               scene, 0.5 on ramps with zlib level 6), about 6 % larger on independent ones.
 * Only integer pixel types (int8 ... uint32) are differenced: the operation is not defined for
 * IEEE samples (Predictor = 3 is not implemented), so float and double responses are the same
 * bytes under both settings.  Uncompressed TIFF, raw and PNG responses never change.  The values
 * are tag 317's.  The initial value is $PBX_TIFF_PREDICTOR (1 / 2; any other value: pbx_init
 * answers 400), else NONE.  A batch takes the setting when it is planned (pbx_batch_plan,
 * pbx_submit, pbx_get_tile(s), the coalescer's batches); a later set does not change a planned
 * batch.  Thread-safe. */
enum pbx_tiff_predictor { PBX_TIFF_PREDICTOR_NONE = 1, PBX_TIFF_PREDICTOR_HORIZONTAL = 2 };
int pbx_set_tiff_predictor(pbx_ctx* ctx, int32_t predictor);   /* 400 outside {1, 2} */
int pbx_get_tiff_predictor(pbx_ctx* ctx, int32_t* predictor);
/* How many tiles of a planned batch (sub-tiles, for tiled TIFF) take each of the two predictor
 * kernels: fast (16-byte aligned source rows of whole 16-byte chunks up to 2 KiB, no padding;
 * $PBX_TIFF_PRED_FAST=0 sends these to the general kernel too) and general (the rest).  Either
 * pointer may be NULL.  Both are 0 with the predictor off. */
int pbx_batch_pred_tiles(pbx_ctx* ctx, pbx_batch* b, uint32_t* fast, uint32_t* general);

/* sizeof of the ABI structs, for bindings to check their layouts: pbx_config,
 * pbx_plane_desc, pbx_tile_req, pbx_result, pbx_batch_stats, pbx_image_desc,
 * pbx_residency_stats, pbx_spans (in that order).  Returns the number of structs (8). */
int pbx_abi_sizes(uint64_t* sizes, int n);

/* ---- A node: N device contexts in ONE process ----
 * The reference deploys its worker verticles in one JVM (PixelBufferMicroserviceVerticle.java:
 * 117-118,224-233: worker_pool_size threads calling TileRequestHandler.getTile).  A node-wide
 * drop-in therefore holds one context per GPU in that process and routes each request to the
 * context that holds its plane, or its row band (a whole slide split into tile-row bands over
 * the GPUs); where several hold it (planes replicated on every GPU) the
 * pbx_shard_of owner among them serves it.  devices: n HIP ordinals (NULL = 0 .. n-1; one
 * device may appear several times); shard_tile: the tile cell of the shard hash (0 = 512). */
typedef struct pbx_node pbx_node;
int pbx_node_init(const pbx_config* cfg, int32_t n, const int32_t* devices, int32_t shard_tile,
                  pbx_node** out);
void pbx_node_shutdown(pbx_node* node);
int32_t pbx_node_size(pbx_node* node);
/* Context k of the node (register planes / bands there; NULL if out of range). */
pbx_ctx* pbx_node_context(pbx_node* node, int32_t k);
/* The context that serves `req`: *index = a context that holds the plane (the status it would
 * answer is returned: PBX_OK, or the reference's 404 ...), else PBX_E_NOT_RESIDENT with *index =
 * the context the binding should load into: the one whose sparse plane owns the rows (bands not
 * loaded yet), else the pbx_shard_of owner. */
int pbx_node_route(pbx_node* node, const pbx_tile_req* req, int32_t* index);
/* pbx_get_tile on the routed context (served_by may be NULL); results are released with
 * pbx_results_release (any context of the node, or NULL). */
int pbx_node_get_tile(pbx_node* node, const pbx_tile_req* req, pbx_result* out, int32_t* served_by);

/* Fault injection (test hook): the `ahead`-th batch launched by this context from
 * now on (1 = the next) completes with a device failure: each of its requests answers 500
 * (PBX_E_INTERNAL, PixelBufferVerticle.java:141-146) unless it already had its own 4xx; the
 * context keeps serving.  0 disables.  $PBX_FAIL_BATCH=k does the same for the k-th launch
 * since pbx_init. */
int pbx_test_fail_batch(pbx_ctx* ctx, uint64_t ahead);
/* Stall injection (test hook): the `ahead`-th batch launched by this context from now on (1 =
 * the next) never completes until pbx_test_stall_batch(ctx, 0) releases it (a one-wave kernel
 * ahead of its kernels spins on a host flag; it also ends by itself after 30 s).  Later batches
 * queue behind it on the device, as behind a wedged one.  Callers of pbx_get_tile get 500 at
 * their deadline (pbx_config.request_timeout_us).  0 releases the stall and disarms. */
int pbx_test_stall_batch(pbx_ctx* ctx, uint64_t ahead);
/* Upload failure injection (test hook): the `ahead`-th pbx_band_write, pbx_band_write_zarr,
 * pbx_band_write_tiff or pbx_band_write_reduced from now on fails after joining its band's load, as a failed
 * host-to-device copy would.  A group call (pbx_band_write_tiff_group / _zarr_group) counts as
 * one write and fails every band it joined.  0 disables. */
int pbx_test_fail_band_write(pbx_ctx* ctx, uint64_t ahead);
/* Test hook, no context and no device: the admission decision of a band write that spans planes
 * (pbx_band_write_tiff_group / _zarr_group; csrc/band_state.h) on band descriptions given as plain
 * integers.  bands: n x 6 values, per member {state (0 absent, 1 loading, 2 resident), the band's
 * HBM is there, writers in flight, failed, stale_reset, idle past the stale limit}; first_row: the
 * piece starts at the band's first row.  out[i]: 1 = join and allocate, 2 = join as one more
 * writer, 409, 500, or -1 for a sibling that is never attempted because the primary is kept out.
 * 400: null arguments, n outside 1 .. 4, primary outside the group, a state outside 0 .. 2 or
 * negative writers. */
int pbx_test_band_group_admit(const int32_t* bands, int32_t n, int32_t primary, int32_t first_row,
                              int32_t* out);
/* Test hook, no context and no device: the source rows and bands of pbx_band_write_reduced
 * (csrc/reduce_plan.h).  Rows [y0, y0 + rows) of a level k below a level of src_size_y rows, held
 * in bands of dst_band_rows rows, from source bands of src_band_rows rows (a dense source:
 * src_band_rows = src_size_y).  out[0 .. 5): the first source row, the row after the last, the
 * first and the last source band, the destination level's rows.  400: k outside 1 .. 4, a size or
 * band height that is not positive, rows outside the destination level or leaving their band. */
int pbx_test_reduce_plan(int32_t k, int32_t src_size_y, int32_t src_band_rows, int32_t dst_band_rows,
                         int32_t y0, int32_t rows, int32_t* out);

/* Request sharding across GPUs (one process per GPU, no collectives): the rank that
 * owns a request, by hash of (image, z, c, t, tile column, tile row) for tile_w x tile_h
 * tiles.  Identical in every process. */
int pbx_shard_of(const pbx_tile_req* req, int32_t tile_w, int32_t tile_h, int32_t world);

/* Test hook: the Huffman stage of the deflate pipeline (k_huff) alone, on given symbol
 * histograms.  hist: nseg x 320 counts (288 literal/length, 32 distance); sl_last: nseg x 2
 * (segment bytes, final-segment flag).  Out: codes nseg x 480 (288 literal/length and 32
 * distance codes as bit-reversed code | length << 16, then 160 words of block header bits)
 * and info nseg x 4 (block type, header bits, data bits, output bytes).  Used by tests/ to
 * compare the GPU stage with the CPU emulator on adversarial histograms. */
int pbx_test_huffman(pbx_ctx* ctx, const uint32_t* hist, const uint32_t* sl_last, uint32_t nseg,
                     uint32_t* codes, uint32_t* info);

/* Test hook: the LZ77 stage's per-segment outputs of a launched batch (k_lz77: 320
 * histogram words and the match records per segment, segments in batch order), compared by
 * tests/ with the CPU emulator.  nseg must equal the batch's segment count. */
int pbx_test_batch_lz77(pbx_ctx* ctx, pbx_batch* b, uint32_t* hist, uint32_t* mrec, uint64_t nseg);

/* Test hook: the host planner of the Zarr decode alone (no context, no device call).  Plans
 * slices[0 .. nslices) of `chunks` (a layer of chunk_planes-deep chunks) for a plane of
 * size_x x size_y samples of bpp bytes: rows == 0 plans the whole plane (registration: every
 * chunk row, offsets as pbx_planes_register_zarr_deep), else rows [y0, y0 + rows) (offsets of
 * the covering chunk rows, as pbx_band_write_zarr_deep).  out: streams planned, the sum of
 * their decoded lengths, blosc blocks skipped, scratch bytes.  400 as the real calls. */
int pbx_test_zarr_plan(const pbx_zarr_chunks* chunks, int32_t size_x, int32_t size_y, int32_t bpp,
                       int32_t chunk_planes, const int32_t* slices, int32_t nslices, int32_t y0,
                       int32_t rows, uint64_t out[4]);

/* Test hook: the host planner of pbx_planes_register_tiff alone (no context, no device call) for
 * a plane of size_x x size_y samples of bpp bytes.  out: streams planned, the sum of their decoded
 * lengths (every segment's own rows: a short last strip counts its rows, an edge tile is full),
 * scratch bytes, 1 if the un-predictor launch is needed.  With Predictor = 3 (bpp 4 or 8 only)
 * out[3] is instead the number of segments handed to k_tiff_fpunpred_place, and stored segments
 * plan no stream and no scratch.  400 as the real call. */
int pbx_test_tiff_plan(const pbx_tiff_segments* segs, int32_t size_x, int32_t size_y, int32_t bpp,
                       uint64_t out[4]);

/* Test hook: the host planner of pbx_band_write_tiff alone (no context, no device call) for rows
 * [y0, y0 + rows) of a plane of size_x x size_y samples of bpp bytes; segs holds the covering
 * segment rows only.  out: streams handed to a decoder (LZW and deflate; stored segments count
 * 0), the sum of the decoded lengths of every covered segment, scratch bytes, 1 if the fused
 * un-predict-and-place kernel is launched (with Predictor = 3: the number of segments handed to
 * k_tiff_fpunpred_place).  400 as the real call, and for rows < 1 or rows
 * outside the plane. */
int pbx_test_tiff_band_plan(const pbx_tiff_segments* segs, int32_t size_x, int32_t size_y, int32_t bpp,
                            int32_t y0, int32_t rows, uint64_t out[4]);

/* Test hook: the host planner of pbx_planes_register_tiff_samples (rows == 0: the whole plane) or
 * pbx_band_write_tiff_sample (rows >= 1: rows [y0, y0 + rows), segs holding the covering segment
 * rows only) alone, no context and no device call, for a plane of size_x x size_y pixels of bpp
 * bytes a sample and segments of samples_per_pixel samples per pixel.  out: streams handed to a
 * decoder (stored multi-sample segments count 0: they are read where they were uploaded), the sum
 * of the decoded lengths of every segment planned (samples_per_pixel times the single-sample
 * figure), scratch bytes, and the number of segments handed to k_tiff_split_place (for
 * samples_per_pixel == 1: out[3] of pbx_test_tiff_plan / pbx_test_tiff_band_plan, Predictor = 3
 * included).  400 as the real calls. */
int pbx_test_tiff_plan_samples(const pbx_tiff_segments* segs, int32_t size_x, int32_t size_y, int32_t bpp,
                               int32_t samples_per_pixel, int32_t y0, int32_t rows, uint64_t out[4]);

/* Test hook: the header parser and planner of pbx_planes_register_tiff_jpeg (rows == 0: the whole
 * plane) or pbx_band_write_tiff_jpeg (rows >= 1, segs holding the covering segment rows only)
 * alone, no context and no device call.  Returns the status (the message through
 * pbx_last_error).  out: streams, decoded samples (every component of every segment at full
 * resolution), scratch bytes, distinct table sets, the first segment's placement mode (0 stored
 * as it is, 1 YCbCr 1x1, 2 h2v1, 3 h2v2), and the bytes of entropy-coded data (each stream from
 * the end of its SOS header to the end of its segment). */
int pbx_test_tiff_jpeg_plan(const pbx_tiff_segments* segs, const pbx_tiff_jpeg* jpeg, int32_t size_x, int32_t size_y,
                            int32_t samples_per_pixel, int32_t y0, int32_t rows, uint64_t out[6]);

/* Test hook: the header parser and planner of pbx_planes_register_tiff_j2k (rows == 0: the whole
 * plane) or pbx_band_write_tiff_j2k (rows >= 1, segs holding the covering segment rows only)
 * alone, no context and no device call.  Returns the status (the message through
 * pbx_last_error).  out: streams, code blocks, packets, scratch bytes. */
int pbx_test_tiff_j2k_plan(const pbx_tiff_segments* segs, int32_t size_x, int32_t size_y, int32_t pixel_type,
                           int32_t samples_per_pixel, int32_t y0, int32_t rows, uint64_t out[4]);

/* Test hook: the whole plane decoded on the CPU by the planner's tables and the device's own
 * serial code (packet headers, MQ and bit-plane decoder), no context and no device call.  out:
 * samples_per_pixel planes of size_x * size_y samples (uint8, or uint16 in host order), no
 * pitch; out_bytes must be exactly that. */
int pbx_test_tiff_j2k_decode(const pbx_tiff_segments* segs, int32_t size_x, int32_t size_y, int32_t pixel_type,
                             int32_t samples_per_pixel, void* out, uint64_t out_bytes);

/* Test hook: the host planner of pbx_planes_register_tiff_packed (rows == 0: the whole plane) or
 * pbx_band_write_tiff_packed (rows >= 1: rows [y0, y0 + rows), segs holding the covering segment
 * rows only) alone, no context and no device call.  400 as the real call.  out: streams handed to
 * a decoder (stored segments are read where they lie: none), the decoded bytes of every segment
 * (rows times padded row bytes), scratch bytes, segments handed to k_tiff_unpack_place, the padded
 * row bytes of a segment, and the rows the segments hold in all. */
int pbx_test_tiff_packed_plan(const pbx_tiff_segments* segs, const pbx_tiff_packed* packed, int32_t size_x,
                              int32_t size_y, int32_t pixel_type, int32_t y0, int32_t rows, uint64_t out[6]);

#ifdef __cplusplus
}
#endif
#endif /* PBX_H */
