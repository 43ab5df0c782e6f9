"""Zarr chunk rows on demand (pbx_band_write_zarr) next to whole-plane registration
(pbx_plane_register_zarr), on bench.py's Zarr plane: 16384^2 uint16 G_NOISE in 512^2 blosc-lz4
chunks (1,024 chunks, 32 per chunk row).  Prints, as means of three runs after a warm-up,
  band:   one 512-row band (one chunk row): wall ms including the upload, kernel ms decode + place
  plane:  the whole plane: the same three figures
  tile:   a cold 512^2 PNG tile through TileRequestHandler, from a source that hands over chunk
          rows (sparse bands of 512 rows) and by registering the whole plane first.
$PBX_LIB selects the library."""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _zarr  # noqa: E402
import pbx  # noqa: E402

SIDE, CHUNK, REPS = 16384, 512, 3
GX = SIDE // CHUNK


class ChunkRows(pbx.PixelSource):
    """The plane's chunk files held in memory, handed over by chunk row."""

    def __init__(self, image_id, chunks):
        self.image_id, self.chunks = image_id, chunks

    def get_pixels(self, image_id):
        return pbx.Pixels(image_id, pbx.UINT16, SIDE, SIDE) if image_id == self.image_id else None

    def band_chunks(self, pixels, z, c, t, level, y0, rows):
        rows_of = self.chunks[(y0 // CHUNK) * GX:-(-(y0 + rows) // CHUNK) * GX]
        return dict(chunk_x=CHUNK, chunk_y=CHUNK, codec="blosc", chunks=rows_of, fill_bits=0, big_endian=True)


def mean(v):
    return sum(v) / len(v)


def main():
    with pbx.PixelsService(device=0) as svc:
        pid = svc.register_plane(20, 0, 0, 0, pbx.UINT16, SIDE, SIDE, generator="noise")
        plane = np.frombuffer(svc.read_plane_be(pid, SIDE * SIDE * 2), ">u2").reshape(SIDE, SIDE)
        svc.release_plane(pid)
    with ThreadPoolExecutor(16) as ex:
        chunks = list(ex.map(lambda c: _zarr.blosc_encode(c.tobytes(), 2), _zarr.chunk_grid(plane, CHUNK, CHUNK)))
    cbytes = sum(len(c) for c in chunks)
    print("plane %d^2 uint16, %d blosc-lz4 chunks of %d^2, %.1f MB compressed, %.1f MB per chunk row"
          % (SIDE, len(chunks), CHUNK, cbytes / 1e6, cbytes / 1e6 / GX), flush=True)

    with pbx.PixelsService(device=0) as svc:
        sp = svc.create_sparse_plane(30, 0, 0, 0, pbx.UINT16, SIDE, SIDE, CHUNK)
        wall, dec, plc = [], [], []
        for r in range(REPS + 1):  # a cold band each time; the first warms the pools up
            packed = pbx.pack_chunks(chunks[r * GX:(r + 1) * GX])
            t0 = time.perf_counter()
            md, mp = svc.band_write_zarr(sp, r * CHUNK, CHUNK, CHUNK, CHUNK, "blosc", packed, timing=True)
            t1 = time.perf_counter()
            if r:
                wall.append(1e3 * (t1 - t0)), dec.append(md), plc.append(mp)
        st, body = svc.get_tile(pbx.TileCtx(30, 0, 0, 0, 1000, CHUNK, 512, 512))
        assert st == pbx.OK and body == plane[CHUNK:2 * CHUNK, 1000:1512].tobytes()
        svc.release_plane(sp)
        print("band  (512 rows, %d chunks): wall %.2f ms incl. upload, decode %.3f ms, place %.3f ms"
              % (GX, mean(wall), mean(dec), mean(plc)), flush=True)

        packed = pbx.pack_chunks(chunks)
        wall, dec, plc = [], [], []
        for r in range(REPS + 1):
            t0 = time.perf_counter()
            pid, (md, mp) = svc.register_zarr_plane(31, 0, 0, 0, pbx.UINT16, SIDE, SIDE, CHUNK, CHUNK, "blosc",
                                                    packed, timing=True)
            t1 = time.perf_counter()
            if r:
                wall.append(1e3 * (t1 - t0)), dec.append(md), plc.append(mp)
            svc.release_plane(pid)
        print("plane (%d rows, %d chunks): wall %.2f ms incl. upload, decode %.3f ms, place %.3f ms"
              % (SIDE, len(chunks), mean(wall), mean(dec), mean(plc)), flush=True)

    want = None
    for way in ("bands", "plane"):
        ms = []
        with pbx.PixelsService(device=0, sparse_band_rows=CHUNK if way == "bands" else 0) as svc:
            for r in range(REPS + 1):
                iid = 40 + r
                tc = pbx.TileCtx(iid, 0, 0, 0, 4096, 8192 + 100, 512, 512, format="png")  # 2 bands
                t0 = time.perf_counter()
                if way == "bands":
                    body = pbx.TileRequestHandler(svc, tc, ChunkRows(iid, chunks)).get_tile()
                else:
                    pid = svc.register_zarr_plane(iid, 0, 0, 0, pbx.UINT16, SIDE, SIDE, CHUNK, CHUNK, "blosc", chunks)
                    body = pbx.TileRequestHandler(svc, tc).get_tile()
                t1 = time.perf_counter()
                want = want or body
                assert body == want
                if r:
                    ms.append(1e3 * (t1 - t0))
                if way == "plane":
                    svc.release_plane(pid)
        print("tile  (cold 512^2 PNG over two bands) via %s: %.1f ms (%s)"
              % ("chunk rows on demand" if way == "bands" else "whole-plane registration",
                 mean(ms), " ".join("%.1f" % x for x in ms)), flush=True)


if __name__ == "__main__":
    main()
