"""TIFF tile rows on demand (pbx_band_write_tiff) next to whole-plane registration of the same
segments (pbx_planes_register_tiff): one cold 512-row band of a 32768-wide uint16 plane in 256^2
tiles (two tile rows, 256 tiles, 32 MiB decoded), for stored / LZW / deflate segments with
Predictor 1 and 2.

Per case, after a warm-up of both calls, REPS repeats that alternate
  band:      band_write_tiff of a cold band: kernel_ms[0] (decoders), kernel_ms[1] (placement:
             k_zarr_place, or k_tiff_unpred_place with Predictor 2), wall ms including the upload
  baseline:  register_tiff_planes of the same segments as a 32768 x 512 plane of their own:
             kernel_ms[0] (decoders, the copy of stored segments, k_tiff_unpred) + kernel_ms[1]
and prints the medians with their min .. max, and the bytes uploaded.  The tiles cycle through
eight distinct ones (Poisson counts, as dim fluorescence), so that the pure-Python LZW encoder of
tests/_tiff_src.py has 1 MiB to encode and not 32.  $PBX_LIB selects the library."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _tiff_src as T  # noqa: E402
import pbx  # noqa: E402

W, ROWS, TILE, REPS, DISTINCT = 32768, 512, 256, 20, 8
GX, GY = W // TILE, ROWS // TILE
COMPS = [("stored", pbx.TIFF_NONE), ("lzw", pbx.TIFF_LZW), ("deflate", pbx.TIFF_DEFLATE)]


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def main():
    rng = np.random.default_rng(0)
    tiles = [rng.poisson(300, (TILE, TILE)).astype("<u2") for _ in range(DISTINCT)]
    order = [(3 * j + 5 * i) % DISTINCT for j in range(GY) for i in range(GX)]
    band = np.block([[tiles[order[j * GX + i]] for i in range(GX)] for j in range(GY)])
    want = band[100:164, 5000:5512].astype(">u2").tobytes()
    print("band of %d rows of a %d-wide uint16 plane, %d tiles of %d^2 (%d distinct), %.1f MiB decoded; "
          "%d repeats a case, median (min .. max)" % (ROWS, W, GX * GY, TILE, DISTINCT, band.nbytes / 2**20, REPS))
    print("%-8s %-4s %10s | %-24s %-24s %-24s %-24s | %-24s" % (
        "segments", "pred", "upload MB", "band decode ms", "band place ms", "band kernels ms", "band wall ms",
        "baseline kernels ms"), flush=True)
    with pbx.PixelsService(device=0) as svc:
        image = 50
        for cname, comp in COMPS:
            for pred in (1, 2):
                enc = [T.compress((T.predict2(t) if pred == 2 else t).tobytes(), comp) for t in tiles]
                packed = pbx.pack_chunks([enc[k] for k in order])
                geo = dict(seg_w=TILE, seg_h=TILE, tiled=True, compression=comp, predictor=pred)
                image += 2
                sparse = svc.create_sparse_plane(image, 0, 0, 0, pbx.UINT16, W, ROWS * (REPS + 1), ROWS,
                                                 big_endian=False)
                whole = dict(geo, image_id=image + 1, z=0, c=0, t=0, pixel_type=pbx.UINT16, size_x=W, size_y=ROWS,
                             big_endian=False, segments=packed)
                dec, plc, wall, base = [], [], [], []
                for r in range(REPS + 1):  # a cold band each time; the first round warms both calls up
                    t0 = time.perf_counter()
                    md, mp = svc.band_write_tiff(sparse, r * ROWS, ROWS, segments=packed, timing=True, **geo)
                    t1 = time.perf_counter()
                    (pid,), (bd, bp) = svc.register_tiff_planes([whole], timing=True)
                    if r == 0:
                        for iid in (image, image + 1):
                            st, body = svc.get_tile(pbx.TileCtx(iid, 0, 0, 0, 5000, 100, 512, 64))
                            assert st == pbx.OK and body == want, (cname, pred, iid)
                    else:
                        dec.append(md), plc.append(mp), wall.append(1e3 * (t1 - t0)), base.append(bd + bp)
                    svc.release_plane(pid)
                svc.release_plane(sparse)
                print("%-8s %-4d %10.2f | %-24s %-24s %-24s %-24s | %-24s" % (
                    cname, pred, packed[0].nbytes / 1e6, spread(dec), spread(plc),
                    spread([a + b for a, b in zip(dec, plc)]), spread(wall), spread(base)), flush=True)


if __name__ == "__main__":
    main()
