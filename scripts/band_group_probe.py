"""A cold RGB band filled for all three channels from ONE decode (pbx_band_write_tiff_group) next to
the three one-sample band writes that were the only way before: one cold 512-row band of a
32768-wide uint8 RGB image in 256^2 tiles (two tile rows, 256 tiles, 48 MiB decoded), as
scripts/tiff_rgb_probe.py, for stored / LZW / deflate segments with Predictor 1 and 2, JPEG 4:2:0
and lossless JPEG 2000 (5 levels, 64^2 code blocks, the reversible colour transform).

Per case, after a warm-up of every call, REPS repeats that alternate, each on cold bands,
  band x3:   band_write_tiff(samples_per_pixel=3, sample=c), c = 0, 1, 2: three uploads, three decodes
  group 3:   band_write_tiff_group of the three planes: one upload, one decode, three planes placed
  group 1:   band_write_tiff_group with one wanted plane (ids [p, 0, 0]), next to
  single:    band_write_tiff of sample 0 alone, which it should cost
and prints medians with their min .. max: the decoders' and the placement's device ms, the wall ms
of the calls and the bytes uploaded; then the ratios band x3 / group 3 and group 1 / single.
Last, the cold-tile time of the three channels of one region through TileRequestHandler over a
TiffSource on a deflate file of the same tiles, with fill_siblings off and on.  The tiles cycle
through four distinct ones (Poisson counts, every component its own).  $PBX_LIB selects the
library."""
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _tiff_j2k as J2  # noqa: E402
import _tiff_jpeg as J  # noqa: E402
import _tiff_rgb as R  # noqa: E402
import _tiff_src as T  # noqa: E402
import pbx  # noqa: E402

W, ROWS, TILE, S, REPS, DISTINCT = 32768, 512, 256, 3, 20, 4
GX, GY = W // TILE, ROWS // TILE
MIB = float(1 << 20)
med = statistics.median


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (med(v), min(v), max(v))


def cases(tiles, order):
    """(name, the band's packed segments, band_write_tiff keywords, the decoded tiles)."""
    for cname, comp in (("stored", pbx.TIFF_NONE), ("lzw", pbx.TIFF_LZW), ("deflate", pbx.TIFF_DEFLATE)):
        for pred in (1, 2):
            enc = [T.compress(R.chunky_segments(t, (TILE, TILE), None, pred)[0], comp) for t in tiles]
            yield "%s p%d" % (cname, pred), pbx.pack_chunks([enc[k] for k in order]), dict(compression=comp, predictor=pred), tiles
    enc = [J.pil_jpeg(t, quality=85, subsampling=2) for t in tiles]
    tabs = J.split_tables(enc[0])[0]
    assert all(J.split_tables(e)[0] == tabs for e in enc)
    yield ("jpeg 4:2:0", pbx.pack_chunks([J.split_tables(enc[k])[1] for k in order]),
           dict(compression=pbx.TIFF_JPEG, predictor=1, jpeg=dict(tables=tabs, ycbcr=True)), [J.pil_decode(e) for e in enc])
    enc = [J2.encode(t, num_resolutions=6, codeblock_size=(64, 64), mct=1) for t in tiles]
    yield "j2k rct", pbx.pack_chunks([enc[k] for k in order]), dict(compression=pbx.TIFF_J2K, predictor=1, j2k=True), tiles


def handler_times(tiles, order):
    """Cold-tile ms of c = 0, 1, 2 of one 512 x 256 region, fill_siblings off and on."""
    a = np.concatenate([np.concatenate([tiles[order[j * GX + i]] for i in range(GX)], axis=1) for j in range(GY)], axis=0)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "rgb.tif")
        R.write_tiff(path, [R.page_of(a, compression=pbx.TIFF_DEFLATE, predictor=2, tile=(TILE, TILE))])
        out = {}
        src = pbx.TiffSource({7: path})
        src.get_pixels(7)  # the file's layout is read once, outside the timing
        for on in (False, True):
            times = []
            for r in range(REPS + 1):  # (a service of its own each time: every tile is cold)
                with pbx.PixelsService(device=0, sparse_band_rows=ROWS, fill_siblings=on) as svc:
                    t0 = time.perf_counter()
                    bodies = [pbx.TileRequestHandler(svc, pbx.TileCtx(7, 0, c, 0, 5000, 100, 512, 256), src).get_tile()
                              for c in range(S)]
                    t1 = time.perf_counter()
                    assert [b == a[100:356, 5000:5512, c].tobytes() for c, b in enumerate(bodies)] == [True] * S
                    if r:
                        times.append(1e3 * (t1 - t0))
            out[on] = times
    return out


def main():
    rng = np.random.default_rng(0)
    tiles = [np.stack([rng.poisson(40 + 25 * s, (TILE, TILE)) for s in range(S)], axis=2).astype(np.uint8)
             for _ in range(DISTINCT)]
    order = [(3 * j + 5 * i) % DISTINCT for j in range(GY) for i in range(GX)]
    x0, y0 = 5000, 100
    k = order[(y0 // TILE) * GX + x0 // TILE]
    cut = (slice(y0 % TILE, y0 % TILE + 64), slice(x0 % TILE, x0 % TILE + 100))
    print("band of %d rows of a %d-wide uint8 RGB image, %d tiles of %d^2 (%d distinct), %.0f MiB decoded; "
          "%d repeats a case, median (min .. max), ms" % (ROWS, W, GX * GY, TILE, DISTINCT, S * W * ROWS / MIB, REPS))
    print("%-11s %9s | %-23s %-23s %-26s | %-23s %-23s %-26s | %-23s %-23s | %-23s %-23s" % (
        "segments", "upload MB", "band x3 decode", "band x3 place", "band x3 wall", "group 3 decode", "group 3 place",
        "group 3 wall", "group 1 decode+place", "group 1 wall", "single decode+place", "single wall"), flush=True)
    notes = []
    geo = dict(seg_w=TILE, seg_h=TILE, tiled=True)
    with pbx.PixelsService(device=0) as svc:
        image = 110
        for name, packed, kw, decoded in cases(tiles, order):
            image += 4
            rows = ROWS * (REPS + 1)
            sp = [[svc.create_sparse_plane(image + g, 0, s, 0, pbx.UINT8, W, rows, ROWS, big_endian=False) for s in range(S)]
                  for g in range(4)]
            gkw = dict(kw)
            comp, pred = gkw.pop("compression"), gkw.pop("predictor")
            xd, xp, xw, gd, gp, gw, od, ow, sd, sw = ([] for _ in range(10))
            for r in range(REPS + 1):  # cold bands each time; the first round warms every call up
                y = r * ROWS
                t0 = time.perf_counter()
                x3 = [svc.band_write_tiff(sp[0][s], y, ROWS, segments=packed, timing=True, samples_per_pixel=S, sample=s,
                                          **geo, **kw) for s in range(S)]
                t1 = time.perf_counter()
                _, g3 = svc.band_write_tiff_group(sp[1], 0, y, ROWS, TILE, TILE, True, comp, pred, packed, **gkw)
                t2 = time.perf_counter()
                _, g1 = svc.band_write_tiff_group([sp[2][0], 0, 0], 0, y, ROWS, TILE, TILE, True, comp, pred, packed, **gkw)
                t3 = time.perf_counter()
                s1 = svc.band_write_tiff(sp[3][0], y, ROWS, segments=packed, timing=True, samples_per_pixel=S, sample=0,
                                         **geo, **kw)
                t4 = time.perf_counter()
                if r == 0:
                    for g, chans in ((0, range(S)), (1, range(S)), (2, (0,)), (3, (0,))):
                        for s in chans:
                            st, body = svc.get_tile(pbx.TileCtx(image + g, 0, s, 0, x0, y0, 100, 64))
                            assert st == pbx.OK and body == decoded[k][cut][:, :, s].tobytes(), (name, g, s)
                else:
                    xd.append(sum(m[0] for m in x3)), xp.append(sum(m[1] for m in x3)), xw.append(1e3 * (t1 - t0))
                    gd.append(g3[0]), gp.append(g3[1]), gw.append(1e3 * (t2 - t1))
                    od.append(g1[0] + g1[1]), ow.append(1e3 * (t3 - t2))
                    sd.append(s1[0] + s1[1]), sw.append(1e3 * (t4 - t3))
            for planes in sp:
                for pid in planes:
                    svc.release_plane(pid)
            mb = packed[0].nbytes / 1e6
            print("%-11s %9.2f | %-23s %-23s %-26s | %-23s %-23s %-26s | %-23s %-23s | %-23s %-23s" % (
                name, mb, spread(xd), spread(xp), spread(xw), spread(gd), spread(gp), spread(gw), spread(od), spread(ow),
                spread(sd), spread(sw)), flush=True)
            notes.append("%-11s | uploaded MB: band x3 %7.2f, group 3 %7.2f | band x3 / group 3: decode %5.2f x  kernels %5.2f x  "
                         "wall %5.2f x | group 3 / single: kernels %5.2f x  wall %5.2f x | group 1 / single: kernels %5.2f x  wall %5.2f x" % (
                             name, 3 * mb, mb, med(xd) / max(med(gd), 1e-9), (med(xd) + med(xp)) / (med(gd) + med(gp)),
                             med(xw) / med(gw), (med(gd) + med(gp)) / med(sd), med(gw) / med(sw), med(od) / med(sd),
                             med(ow) / med(sw)))
    print("\nuploads and ratios of medians")
    for n in notes:
        print(n)
    ht = handler_times(tiles, order)
    print("\ncold 512 x 256 tile of c = 0, 1, 2 through TileRequestHandler (deflate, Predictor 2, bands of %d rows), wall ms of "
          "the three requests:" % ROWS)
    print("fill_siblings off %s   on %s   off / on %.2f x" % (spread(ht[False]), spread(ht[True]), med(ht[False]) / med(ht[True])))


if __name__ == "__main__":
    main()
