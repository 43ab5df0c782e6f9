"""The floating-point un-predictor (Predictor = 3, k_tiff_fpunpred_place) next to the placement
that exists without it: one cold 512-row band of a 32768-wide float32 plane in 256^2 tiles (two
tile rows, 256 tiles, 64 MiB decoded), for deflate / zstd / stored segments, and the same band
in stored strips of 16 rows (rows of 32768 samples: the kernel's wide form, 1,024 samples a wave
step, where the tiles' rows of 256 samples take its narrow one).

Per case, after a warm-up of both, REPS repeats that alternate two pbx_band_write_tiff calls on
cold bands of two sparse planes:
  p3:        the tiles written with Predictor 3: kernel_ms[0] (decoders; about 0 for stored
             segments), kernel_ms[1] (k_tiff_fpunpred_place), wall ms including the upload
  baseline:  the same pixels written with Predictor 1: kernel_ms[0], kernel_ms[1] (k_zarr_place)
and prints the medians with their min .. max, and the bytes uploaded.  The tiles cycle through
eight distinct ones (Poisson counts / 4, as dim fluorescence after flat-fielding).  $PBX_LIB
selects the library."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _tiff_fp as F  # noqa: E402
import pbx  # noqa: E402

W, ROWS, TILE, REPS, DISTINCT = 32768, 512, 256, 20, 8
GX, GY = W // TILE, ROWS // TILE
RPS = 16
CASES = [("deflate", pbx.TIFF_DEFLATE, True), ("zstd", pbx.TIFF_ZSTD, True), ("stored", pbx.TIFF_NONE, True),
         ("strips", pbx.TIFF_NONE, False)]  # (name, compression, tiled)


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def main():
    rng = np.random.default_rng(0)
    tiles = [(rng.poisson(300, (TILE, TILE)) * 0.25).astype("<f4") for _ in range(DISTINCT)]
    order = [(3 * j + 5 * i) % DISTINCT for j in range(GY) for i in range(GX)]
    band = np.block([[tiles[order[j * GX + i]] for i in range(GX)] for j in range(GY)])
    want = band[100:164, 5000:5512].astype(">f4").tobytes()
    print("band of %d rows of a %d-wide float32 plane, %d tiles of %d^2 (%d distinct), %.1f MiB decoded; "
          "%d repeats a case, median (min .. max)" % (ROWS, W, GX * GY, TILE, DISTINCT, band.nbytes / 2**20, REPS))
    print("%-8s %-4s %10s | %-24s %-24s %-24s" % ("segments", "pred", "upload MB", "decode ms (kernel_ms[0])",
                                                  "place ms (kernel_ms[1])", "wall ms"), flush=True)
    with pbx.PixelsService(device=0) as svc:
        image = 60
        for cname, comp, tiled in CASES:
            packed, plane, t = {}, {}, {1: ([], [], []), 3: ([], [], [])}
            geo = (TILE, TILE, True) if tiled else (W, RPS, False)
            for pred in (3, 1):
                if tiled:
                    enc = [F.compress(F.segments_of(x, (TILE, TILE), None, pred)[0], comp) for x in tiles]
                    packed[pred] = pbx.pack_chunks([enc[k] for k in order])
                else:
                    packed[pred] = pbx.pack_chunks(F.segments_of(band, None, RPS, pred))
                image += 1
                plane[pred] = (image, svc.create_sparse_plane(image, 0, 0, 0, pbx.FLOAT, W, ROWS * (REPS + 1), ROWS,
                                                              big_endian=False))
            for r in range(REPS + 1):  # a cold band each time; the first round warms both up
                for pred in (3, 1):
                    t0 = time.perf_counter()
                    md, mp = svc.band_write_tiff(plane[pred][1], r * ROWS, ROWS, *geo, comp, pred, packed[pred],
                                                 timing=True)
                    t1 = time.perf_counter()
                    if r == 0:
                        st, body = svc.get_tile(pbx.TileCtx(plane[pred][0], 0, 0, 0, 5000, 100, 512, 64))
                        assert st == pbx.OK and body == want, (cname, pred)
                    else:
                        t[pred][0].append(md), t[pred][1].append(mp), t[pred][2].append(1e3 * (t1 - t0))
            for pred in (3, 1):
                svc.release_plane(plane[pred][1])
                print("%-8s %-4d %10.2f | %-24s %-24s %-24s" % (cname, pred, packed[pred][0].nbytes / 1e6,
                                                             spread(t[pred][0]), spread(t[pred][1]),
                                                             spread(t[pred][2])), flush=True)


if __name__ == "__main__":
    main()
