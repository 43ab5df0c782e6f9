"""The cold lowest-resolution tile of a flat 100000 x 100000 uint16 source, by reduce_step.

A viewer's first request: resolution 0 of an image that stores one level.  DerivedLevels declares
the levels down to 3125 x 3125 (five of them); the tile's bands are made on the GPU from the base
rows they depend on, through intermediate derived levels every reduce_step levels.  For
reduce_step 1, 2 and 4, each in a fresh service: the wall time of the cold tile, the base rows and
bytes read from the source, the bytes resident afterwards (base bands + intermediate bands + the
level's own) and the time of a second tile in the same bands.  The source hands out generated rows
(one random row block repeated: reading costs a copy, as from a page cache), so the times are the
loader's and the GPU's, not a disk's.

  python scripts/derived_cold_tile.py [tile side, default 256]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))
import pbx  # noqa: E402

SIDE, B = 100000, 64


class Generated(pbx.PixelSource):
    def __init__(self):
        self.block = np.random.default_rng(1).integers(0, 65536, (B, SIDE), dtype=np.uint16).astype(">u2").tobytes()
        self.rows = self.reads = 0

    def get_pixels(self, image_id):
        return pbx.Pixels(image_id, pbx.UINT16, SIDE, SIDE)

    def read_rows(self, pixels, z, c, t, level, y0, rows):
        self.rows, self.reads = self.rows + rows, self.reads + 1
        return self.block[:rows * SIDE * 2]


def main():
    side = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    for step in (1, 2, 4):
        flat = Generated()
        src = pbx.DerivedLevels(flat)
        px = src.get_pixels(1)
        with pbx.PixelsService(sparse_band_rows=B, reduce_step=step) as svc:
            tc = pbx.TileCtx(1, 0, 0, 0, 1024, 1024, side, side, resolution=0, format="png")
            t0 = time.perf_counter()
            body = pbx.TileRequestHandler(svc, tc, src).get_tile()
            t1 = time.perf_counter()
            tc2 = pbx.TileCtx(1, 0, 0, 0, 1024 + side, 1024, side, side, resolution=0, format="png")
            body2 = pbx.TileRequestHandler(svc, tc2, src).get_tile()
            t2 = time.perf_counter()
            st = svc.residency_stats()
            held = [lv for lv in range(px.levels) if svc.lookup_plane(1, 0, 0, 0, lv) is not None]
            print("reduce_step %d: levels %d (smallest %s), cold %dx%d tile %.1f ms (%d bytes), base rows read %d in %d "
                  "reads = %.1f MB, resident %.1f MB in %d bands, levels held %s, next tile in the same bands %.2f ms (%d bytes)"
                  % (step, px.levels, src.level_size(px, px.levels - 1), side, side, (t1 - t0) * 1e3, len(body), flat.rows,
                     flat.reads, flat.rows * SIDE * 2 / 1e6, st["resident_bytes"] / 1e6, st["bands"], held,
                     (t2 - t1) * 1e3, len(body2)), flush=True)


if __name__ == "__main__":
    main()
