"""Chunky RGB TIFF tiles split into three planes (k_tiff_split_place) next to the same pixels
stored as three single-sample IFDs and loaded through the single-sample calls: one cold 512-row
band of a 32768-wide uint8 RGB image in 256^2 tiles (two tile rows, 256 tiles, 48 MiB decoded), for
stored / LZW / deflate segments with Predictor 1 and 2.

Per case, after a warm-up of every call, REPS repeats that alternate
  rgb reg:    register_tiff_planes of the three samples of the one chunky layer: ONE decode,
              kernel_ms[0] (decoders; stored segments launch none) and kernel_ms[1]
              (k_tiff_split_place: 48 MiB read, 3 x 16 MiB written)
  rgb band:   band_write_tiff(samples_per_pixel=3, sample=c) of a cold band of each channel's sparse
              plane, c = 0, 1, 2: THREE decodes, kernel_ms[1] of each = k_tiff_split_place storing
              one component (48 MiB read, 16 MiB written); wall ms of the three calls with uploads
  base reg:   register_tiff_planes of the three single-sample planes in one call: decoders, the
              copy of stored segments and k_tiff_unpred in kernel_ms[0], k_zarr_place in [1]
  base band:  band_write_tiff of a cold band of each of the three single-sample planes:
              kernel_ms[1] = k_zarr_place (Predictor 1) or k_tiff_unpred_place (Predictor 2),
              16 MiB read and 16 MiB written each
and prints medians with their min .. max, then per case the placement kernels' time per byte
moved (read + written), and what the S-fold decode of cold RGB bands costs: the kernels of the
three one-sample band writes over those of the one registration that decodes once.  The tiles
cycle through four distinct ones (Poisson counts, every component its own), so that the
pure-Python LZW encoder of tests/_tiff_src.py has 1.5 MiB to encode a case.  $PBX_LIB selects the
library."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _tiff_rgb as R  # noqa: E402
import _tiff_src as T  # noqa: E402
import pbx  # noqa: E402

W, ROWS, TILE, S, REPS, DISTINCT = 32768, 512, 256, 3, 20, 4
GX, GY = W // TILE, ROWS // TILE
COMPS = [("stored", pbx.TIFF_NONE), ("lzw", pbx.TIFF_LZW), ("deflate", pbx.TIFF_DEFLATE)]
MIB = float(1 << 20)


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def main():
    rng = np.random.default_rng(0)
    tiles = [np.stack([rng.poisson(40 + 25 * s, (TILE, TILE)) for s in range(S)], axis=2).astype(np.uint8)
             for _ in range(DISTINCT)]
    order = [(3 * j + 5 * i) % DISTINCT for j in range(GY) for i in range(GX)]
    x0, y0 = 5000, 100
    tx, ty = x0 // TILE, y0 // TILE  # (the checked region lies inside one tile)
    piece = tiles[order[ty * GX + tx]][y0 % TILE:y0 % TILE + 64, x0 % TILE:x0 % TILE + 100]
    plane_b = W * ROWS
    print("band of %d rows of a %d-wide uint8 RGB image, %d tiles of %d^2 (%d distinct), %.0f MiB decoded; "
          "%d repeats a case, median (min .. max), ms" % (ROWS, W, GX * GY, TILE, DISTINCT, S * plane_b / MIB, REPS))
    print("%-8s %-4s %9s | %-23s %-23s | %-23s %-23s %-23s | %-23s %-23s | %-23s %-23s" % (
        "segments", "pred", "upload MB", "rgb reg decode", "rgb reg split", "rgb band decode x3", "rgb band split x3",
        "rgb band wall x3", "base reg decode", "base reg place", "base band decode x3", "base band place x3"), flush=True)
    notes = []
    with pbx.PixelsService(device=0) as svc:
        image = 70
        for cname, comp in COMPS:
            for pred in (1, 2):
                enc = [T.compress(R.chunky_segments(t, (TILE, TILE), None, pred)[0], comp) for t in tiles]
                packed = pbx.pack_chunks([enc[k] for k in order])
                enc1 = [[T.compress(T.segments_of(np.ascontiguousarray(t[:, :, s]), (TILE, TILE), None, pred)[0], comp)
                         for t in tiles] for s in range(S)]
                packed1 = [pbx.pack_chunks([enc1[s][k] for k in order]) for s in range(S)]
                geo = dict(seg_w=TILE, seg_h=TILE, tiled=True, compression=comp, predictor=pred)
                image += 4
                rgb_reg = [dict(geo, image_id=image, z=0, c=s, t=0, pixel_type=pbx.UINT8, size_x=W, size_y=ROWS,
                                segments=packed, samples_per_pixel=S, sample=s) for s in range(S)]
                base_reg = [dict(geo, image_id=image + 1, z=0, c=s, t=0, pixel_type=pbx.UINT8, size_x=W, size_y=ROWS,
                                 segments=packed1[s]) for s in range(S)]
                rgb_sp = [svc.create_sparse_plane(image + 2, 0, s, 0, pbx.UINT8, W, ROWS * (REPS + 1), ROWS)
                          for s in range(S)]
                base_sp = [svc.create_sparse_plane(image + 3, 0, s, 0, pbx.UINT8, W, ROWS * (REPS + 1), ROWS)
                           for s in range(S)]
                rd, rs, bd, bs, bw, sd, sp_, sbd, sbp = ([] for _ in range(9))
                for r in range(REPS + 1):  # cold bands each time; the first round warms every call up
                    ids, (a, b) = svc.register_tiff_planes(rgb_reg, timing=True)
                    t0 = time.perf_counter()
                    band = [svc.band_write_tiff(rgb_sp[s], r * ROWS, ROWS, segments=packed, timing=True,
                                                samples_per_pixel=S, sample=s, **geo) for s in range(S)]
                    t1 = time.perf_counter()
                    ids1, (c, d) = svc.register_tiff_planes(base_reg, timing=True)
                    band1 = [svc.band_write_tiff(base_sp[s], r * ROWS, ROWS, segments=packed1[s], timing=True, **geo)
                             for s in range(S)]
                    if r == 0:
                        for iid in range(image, image + 4):
                            for s in range(S):
                                st, body = svc.get_tile(pbx.TileCtx(iid, 0, s, 0, x0, y0, 100, 64))
                                assert st == pbx.OK and body == piece[:, :, s].tobytes(), (cname, pred, iid, s)
                    else:
                        rd.append(a), rs.append(b), sd.append(c), sp_.append(d)
                        bd.append(sum(m[0] for m in band)), bs.append(sum(m[1] for m in band))
                        bw.append(1e3 * (t1 - t0))
                        sbd.append(sum(m[0] for m in band1)), sbp.append(sum(m[1] for m in band1))
                    for pid in ids + ids1:
                        svc.release_plane(pid)
                for pid in rgb_sp + base_sp:
                    svc.release_plane(pid)
                print("%-8s %-4d %9.2f | %-23s %-23s | %-23s %-23s %-23s | %-23s %-23s | %-23s %-23s" % (
                    cname, pred, packed[0].nbytes / 1e6, spread(rd), spread(rs), spread(bd), spread(bs), spread(bw),
                    spread(sd), spread(sp_), spread(sbd), spread(sbp)), flush=True)
                med = statistics.median
                # ps per byte read + written: the split kernel moves 3 + 3 planes at registration and
                # 3 + 1 per one-sample band write; the single-sample placement 1 + 1 per plane
                notes.append("%-8s %-4d | split, 3 planes out %6.2f   split, 1 plane out %6.2f   single-sample %-19s %6.2f"
                             "   | 3 one-sample band writes / 1 registration, kernels: %5.2f x" % (
                                 cname, pred, 1e9 * med(rs) / (6 * plane_b), 1e9 * med(bs) / (3 * 4 * plane_b),
                                 "k_tiff_unpred_place" if pred == 2 else "k_zarr_place",
                                 1e9 * med(sbp) / (3 * 2 * plane_b),
                                 (med(bd) + med(bs)) / (med(rd) + med(rs))))
    print("\nplacement kernels, ps per byte read + written (medians); the cost of decoding three times")
    for n in notes:
        print(n)


if __name__ == "__main__":
    main()
