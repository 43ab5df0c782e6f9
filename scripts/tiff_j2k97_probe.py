"""Lossy JPEG 2000 TIFF tiles (9/7: k_tiff_j2k_blocks with the dequantising store,
k_tiff_j2k_idwt97, k_tiff_j2k_place's float branch) next to the same pixels as lossless 5/3 tiles
(k_tiff_j2k_idwt, the integer placement), in scripts/tiff_j2k_probe.py's layout: one cold 512-row
band of a 32768-wide image in 256^2 tiles (two tile rows, 256 tiles), five levels, 64^2 code blocks.

Two cases: uint16 gray Poisson counts, and uint8 RGB through the colour transform (ICT against
RCT; a band write of sample 0).  Per case, after a warm-up of both, REPS repeats that alternate a
cold 9/7 band write and a cold 5/3 band write, and print medians with their min .. max: uploaded
MB, kernel_ms[0] (decode: packet headers, code blocks and inverse wavelet together), kernel_ms[1]
(placement) and the wall time of the call with its upload.  The 9/7 streams are PIL's at full
quality, so tier 1 has about as many passes to decode as on the lossless side, and the difference
is what the float wavelet and the dequantising store cost.  The 9/7 pixels are checked against
the CPU hook, the 5/3 ones against the tiles.  $PBX_LIB selects the library."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _tiff_j2k as J  # noqa: E402
import _tiff_j2k97 as M  # noqa: E402
import pbx  # noqa: E402

W, ROWS, TILE, REPS, DISTINCT = 32768, 512, 256, 20, 4
GX, GY = W // TILE, ROWS // TILE


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def main():
    rng = np.random.default_rng(0)
    order = [(3 * j + 5 * i) % DISTINCT for j in range(GY) for i in range(GX)]
    x0, y0 = 5000, 100
    k = order[(y0 // TILE) * GX + x0 // TILE]
    cut = (slice(y0 % TILE, y0 % TILE + 64), slice(x0 % TILE, x0 % TILE + 100))
    print("band of %d rows of a %d-wide image, %d tiles of %d^2 (%d distinct), 5 levels, 64^2 code blocks; %d repeats a "
          "case, median (min .. max), ms" % (ROWS, W, GX * GY, TILE, DISTINCT, REPS))
    print("%-10s %8s %8s | %-26s %-23s %-26s | %-26s %-23s %-26s" % (
        "case", "9/7 MB", "5/3 MB", "9/7 decode", "9/7 place", "9/7 wall", "5/3 decode", "5/3 place", "5/3 wall"), flush=True)
    with pbx.PixelsService(device=0) as svc:
        image = 190
        for name, dtype, S in (("u16 gray", np.uint16, 1), ("u8 rgb ct", np.uint8, 3)):
            if S == 1:
                tiles = [rng.poisson(300, (TILE, TILE)).astype(dtype) for _ in range(DISTINCT)]
            else:
                tiles = [np.stack([rng.poisson(40 + 25 * s, (TILE, TILE)) for s in range(S)], axis=2).astype(dtype)
                         for _ in range(DISTINCT)]
            o = dict(num_resolutions=6, codeblock_size=(64, 64), mct=1 if S == 3 else 0)
            lossy = [M.encode(t, **o) for t in tiles]
            exact = [J.encode(t, **o) for t in tiles]
            passes = []
            for e in (lossy[k], exact[k]):
                hd = M.parse(e)
                passes.append(sum(v[2] for comp in J.packets(e, hd, J.geometry(hd)[0]) for band in comp for v in band.values()))
            pg = M.page_of(tiles[k], tile=(TILE, TILE), **o)
            rc, msg, hook = M.hook_page(pg)
            assert rc == 0, msg
            packed = pbx.pack_chunks([lossy[i] for i in order])
            zpacked = pbx.pack_chunks([exact[i] for i in order])
            pt = pbx.UINT8 if dtype == np.uint8 else pbx.UINT16
            geo = dict(seg_w=TILE, seg_h=TILE, tiled=True, predictor=1, samples_per_pixel=S, sample=0,
                       compression=pbx.TIFF_J2K, timing=True, j2k=True)
            image += 2
            jp = svc.create_sparse_plane(image, 0, 0, 0, pt, W, ROWS * (REPS + 1), ROWS, big_endian=False)
            zp = svc.create_sparse_plane(image + 1, 0, 0, 0, pt, W, ROWS * (REPS + 1), ROWS, big_endian=False)
            wants = [hook[cut] if S == 1 else hook[cut][:, :, 0], tiles[k][cut] if S == 1 else tiles[k][cut][:, :, 0]]
            jd, jl, jw, zd, zl, zw = ([] for _ in range(6))
            for r in range(REPS + 1):  # a cold band each time; the first round warms both calls up
                t0 = time.perf_counter()
                a = svc.band_write_tiff(jp, r * ROWS, ROWS, segments=packed, **geo)
                t1 = time.perf_counter()
                b = svc.band_write_tiff(zp, r * ROWS, ROWS, segments=zpacked, **geo)
                t2 = time.perf_counter()
                if r == 0:
                    for iid, want in zip((image, image + 1), wants):
                        st, body = svc.get_tile(pbx.TileCtx(iid, 0, 0, 0, x0, y0, 100, 64))
                        assert st == pbx.OK and body == J.be_bytes(want), (name, iid)
                else:
                    jd.append(a[0]), jl.append(a[1]), jw.append(1e3 * (t1 - t0))
                    zd.append(b[0]), zl.append(b[1]), zw.append(1e3 * (t2 - t1))
            for pid in (jp, zp):
                svc.release_plane(pid)
            print("%-10s %8.2f %8.2f | %-26s %-23s %-26s | %-26s %-23s %-26s" % (
                name, packed[0].nbytes / 1e6, zpacked[0].nbytes / 1e6, spread(jd), spread(jl), spread(jw), spread(zd),
                spread(zl), spread(zw)), flush=True)
            print("%-10s   coding passes of tile %d: 9/7 %d, 5/3 %d; 9/7 decode / 5/3 decode %.2f x" % (
                name, k, passes[0], passes[1], statistics.median(jd) / statistics.median(zd)), flush=True)


if __name__ == "__main__":
    main()
