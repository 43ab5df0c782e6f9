"""JPEG-compressed RGB TIFF tiles (k_tiff_jpeg_decode + k_tiff_jpeg_place) next to the same
pixels as chunky deflate RGB tiles through the existing _samples calls (k_zarr_inflate2 +
k_tiff_split_place): one cold 512-row band of a 32768-wide uint8 RGB image in 256^2 tiles (two
tile rows, 256 tiles, 48 MiB decoded), JPEG quality 85 as 4:2:0 and as 4:4:4.

Per case, after a warm-up of every call, REPS repeats that alternate
  jpeg reg:   register_tiff_planes of the three samples of the one JPEG layer: ONE decode,
              kernel_ms[0] (k_tiff_jpeg_decode) and kernel_ms[1] (k_tiff_jpeg_place)
  jpeg band:  band_write_tiff(jpeg=..., sample=c) of a cold band of each channel's sparse plane,
              c = 0, 1, 2: THREE decodes; wall ms of the three calls with uploads
  base reg / base band: the same two through the deflate tiles
and prints medians with their min .. max, then per case the decode ratio against deflate, the
placement kernels' time per byte stored, and what the S-fold decode of cold bands costs: the
kernels of the three one-sample band writes over those of the one registration.  The tiles cycle
through four distinct ones (Poisson counts, every component its own).  What is compared with the
baseline is time, not pixels: JPEG is lossy, and each path is checked against its own decode.
$PBX_LIB selects the library."""
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _tiff_jpeg as J  # noqa: E402
import pbx  # noqa: E402

W, ROWS, TILE, S, REPS, DISTINCT = 32768, 512, 256, 3, 20, 4
GX, GY = W // TILE, ROWS // TILE
MIB = float(1 << 20)


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def main():
    rng = np.random.default_rng(0)
    tiles = [np.stack([rng.poisson(40 + 25 * s, (TILE, TILE)) for s in range(S)], axis=2).astype(np.uint8)
             for _ in range(DISTINCT)]
    order = [(3 * j + 5 * i) % DISTINCT for j in range(GY) for i in range(GX)]
    x0, y0 = 5000, 100
    k = order[(y0 // TILE) * GX + x0 // TILE]
    cut = (slice(y0 % TILE, y0 % TILE + 64), slice(x0 % TILE, x0 % TILE + 100))
    plane_b = W * ROWS
    print("band of %d rows of a %d-wide uint8 RGB image, %d tiles of %d^2 (%d distinct), %.0f MiB decoded; "
          "%d repeats a case, median (min .. max), ms" % (ROWS, W, GX * GY, TILE, DISTINCT, S * plane_b / MIB, REPS))
    print("%-6s %9s %9s | %-23s %-23s | %-23s %-23s %-23s | %-23s %-23s | %-23s %-23s %-23s" % (
        "jpeg", "jpeg MB", "defl MB", "jpeg reg decode", "jpeg reg place", "jpeg band decode x3", "jpeg band place x3",
        "jpeg band wall x3", "base reg decode", "base reg split", "base band decode x3", "base band split x3",
        "base band wall x3"), flush=True)
    notes = []
    zenc = [zlib.compress(t.tobytes(), 6) for t in tiles]
    zpacked = pbx.pack_chunks([zenc[i] for i in order])
    zgeo = dict(seg_w=TILE, seg_h=TILE, tiled=True, compression=pbx.TIFF_DEFLATE, predictor=1)
    with pbx.PixelsService(device=0) as svc:
        image = 90
        for name, sub in (("4:2:0", 2), ("4:4:4", 0)):
            enc = [J.pil_jpeg(t, quality=85, subsampling=sub) for t in tiles]
            tabs = J.split_tables(enc[0])[0]
            assert all(J.split_tables(e)[0] == tabs for e in enc)
            packed = pbx.pack_chunks([J.split_tables(enc[i])[1] for i in order])
            want = J.pil_decode(enc[k])[cut]
            jgeo = dict(seg_w=TILE, seg_h=TILE, tiled=True, compression=pbx.TIFF_JPEG, predictor=1)
            jp = dict(tables=tabs, ycbcr=True)
            image += 4
            jreg = [dict(jgeo, image_id=image, z=0, c=s, t=0, pixel_type=pbx.UINT8, size_x=W, size_y=ROWS, big_endian=False,
                         segments=packed, samples_per_pixel=S, sample=s, jpeg=jp) for s in range(S)]
            breg = [dict(zgeo, image_id=image + 1, z=0, c=s, t=0, pixel_type=pbx.UINT8, size_x=W, size_y=ROWS,
                         big_endian=False, segments=zpacked, samples_per_pixel=S, sample=s) for s in range(S)]
            jsp = [svc.create_sparse_plane(image + 2, 0, s, 0, pbx.UINT8, W, ROWS * (REPS + 1), ROWS, big_endian=False)
                   for s in range(S)]
            bsp = [svc.create_sparse_plane(image + 3, 0, s, 0, pbx.UINT8, W, ROWS * (REPS + 1), ROWS, big_endian=False)
                   for s in range(S)]
            jd, jpl, jbd, jbp, jbw, bd, bp, bbd, bbp, bbw = ([] for _ in range(10))
            for r in range(REPS + 1):  # cold bands each time; the first round warms every call up
                ids, (a, b) = svc.register_tiff_planes(jreg, timing=True)
                t0 = time.perf_counter()
                band = [svc.band_write_tiff(jsp[s], r * ROWS, ROWS, segments=packed, timing=True, samples_per_pixel=S,
                                            sample=s, jpeg=jp, **jgeo) for s in range(S)]
                t1 = time.perf_counter()
                ids1, (c, d) = svc.register_tiff_planes(breg, timing=True)
                t2 = time.perf_counter()
                band1 = [svc.band_write_tiff(bsp[s], r * ROWS, ROWS, segments=zpacked, timing=True, samples_per_pixel=S,
                                             sample=s, **zgeo) for s in range(S)]
                t3 = time.perf_counter()
                if r == 0:
                    for iid, ref in ((image, want), (image + 2, want), (image + 1, tiles[k][cut]), (image + 3, tiles[k][cut])):
                        for s in range(S):
                            st, body = svc.get_tile(pbx.TileCtx(iid, 0, s, 0, x0, y0, 100, 64))
                            assert st == pbx.OK and body == ref[:, :, s].tobytes(), (name, iid, s)
                else:
                    jd.append(a), jpl.append(b), bd.append(c), bp.append(d)
                    jbd.append(sum(m[0] for m in band)), jbp.append(sum(m[1] for m in band)), jbw.append(1e3 * (t1 - t0))
                    bbd.append(sum(m[0] for m in band1)), bbp.append(sum(m[1] for m in band1)), bbw.append(1e3 * (t3 - t2))
                for pid in ids + ids1:
                    svc.release_plane(pid)
            for pid in jsp + bsp:
                svc.release_plane(pid)
            print("%-6s %9.2f %9.2f | %-23s %-23s | %-23s %-23s %-23s | %-23s %-23s | %-23s %-23s %-23s" % (
                name, packed[0].nbytes / 1e6, zpacked[0].nbytes / 1e6, spread(jd), spread(jpl), spread(jbd), spread(jbp),
                spread(jbw), spread(bd), spread(bp), spread(bbd), spread(bbp), spread(bbw)), flush=True)
            med = statistics.median
            notes.append("%-6s | jpeg decode / deflate decode %5.2f x | ps per byte stored: k_tiff_jpeg_place %6.2f (3 planes), "
                         "%6.2f (1 plane); k_tiff_split_place %6.2f, %6.2f | 3 one-sample band writes / 1 registration, "
                         "kernels: jpeg %5.2f x, deflate %5.2f x" % (
                             name, med(jd) / med(bd), 1e9 * med(jpl) / (3 * plane_b), 1e9 * med(jbp) / (3 * plane_b),
                             1e9 * med(bp) / (3 * plane_b), 1e9 * med(bbp) / (3 * plane_b),
                             (med(jbd) + med(jbp)) / (med(jd) + med(jpl)), (med(bbd) + med(bbp)) / (med(bd) + med(bp))))
    print("\nratios of medians")
    for n in notes:
        print(n)


if __name__ == "__main__":
    main()
