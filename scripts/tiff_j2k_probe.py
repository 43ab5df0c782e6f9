"""Lossless JPEG 2000 TIFF tiles (k_tiff_j2k_packets + _blocks + _idwt, k_tiff_j2k_place) next to
the same pixels as deflate (zlib 6) tiles through the existing calls: one cold 512-row band of a
32768-wide image in 256^2 tiles (two tile rows, 256 tiles), five levels, 64^2 code blocks.

Two cases: uint16 gray Poisson counts, and uint8 RGB through the reversible colour transform (a
band write of sample 0: every component is decoded, one is stored; the deflate tiles are chunky
RGB, split the same way).  Per case, after a warm-up of both calls, REPS repeats that alternate a
cold JPEG 2000 band write and a cold deflate band write, and print medians with their min .. max:
uploaded MB, kernel_ms[0] (decode: packet headers, code blocks and inverse wavelet together; the
three are not timed apart here), kernel_ms[1] (placement) and the wall time of the call with its
upload.  The pixels of both paths are checked against the tiles.  $PBX_LIB selects the library."""
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _tiff_j2k as J  # noqa: E402
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
    print("%-10s %8s %8s | %-26s %-23s %-26s | %-23s %-23s %-23s" % (
        "case", "j2k MB", "defl MB", "j2k decode", "j2k place", "j2k wall", "defl decode", "defl place", "defl wall"), flush=True)
    with pbx.PixelsService(device=0) as svc:
        image = 90
        for name, dtype, S in (("u16 gray", np.uint16, 1), ("u8 rgb rct", np.uint8, 3)):
            if S == 1:
                tiles = [rng.poisson(300, (TILE, TILE)).astype(dtype) for _ in range(DISTINCT)]
            else:
                tiles = [np.stack([rng.poisson(40 + 25 * s, (TILE, TILE)) for s in range(S)], axis=2).astype(dtype)
                         for _ in range(DISTINCT)]
            enc = [J.encode(t, num_resolutions=6, codeblock_size=(64, 64), mct=1 if S == 3 else 0) for t in tiles]
            assert all(np.array_equal(J.pil_decode(e), t) for e, t in zip(enc, tiles))
            packed = pbx.pack_chunks([enc[i] for i in order])
            zenc = [zlib.compress(t.astype(t.dtype.newbyteorder("<")).tobytes(), 6) for t in tiles]
            zpacked = pbx.pack_chunks([zenc[i] for i in order])
            pt = pbx.UINT8 if dtype == np.uint8 else pbx.UINT16
            geo = dict(seg_w=TILE, seg_h=TILE, tiled=True, predictor=1, samples_per_pixel=S, sample=0)
            image += 2
            jp = svc.create_sparse_plane(image, 0, 0, 0, pt, W, ROWS * (REPS + 1), ROWS, big_endian=False)
            zp = svc.create_sparse_plane(image + 1, 0, 0, 0, pt, W, ROWS * (REPS + 1), ROWS, big_endian=False)
            want = tiles[k][cut] if S == 1 else tiles[k][cut][:, :, 0]
            jd, jl, jw, zd, zl, zw = ([] for _ in range(6))
            for r in range(REPS + 1):  # a cold band each time; the first round warms both calls up
                t0 = time.perf_counter()
                a = svc.band_write_tiff(jp, r * ROWS, ROWS, compression=pbx.TIFF_J2K, segments=packed, timing=True, j2k=True, **geo)
                t1 = time.perf_counter()
                b = svc.band_write_tiff(zp, r * ROWS, ROWS, compression=pbx.TIFF_DEFLATE, segments=zpacked, timing=True, **geo)
                t2 = time.perf_counter()
                if r == 0:
                    for iid in (image, image + 1):
                        st, body = svc.get_tile(pbx.TileCtx(iid, 0, 0, 0, x0, y0, 100, 64))
                        assert st == pbx.OK and body == J.be_bytes(want), (name, iid)
                else:
                    jd.append(a[0]), jl.append(a[1]), jw.append(1e3 * (t1 - t0))
                    zd.append(b[0]), zl.append(b[1]), zw.append(1e3 * (t2 - t1))
            for pid in (jp, zp):
                svc.release_plane(pid)
            print("%-10s %8.2f %8.2f | %-26s %-23s %-26s | %-23s %-23s %-23s" % (
                name, packed[0].nbytes / 1e6, zpacked[0].nbytes / 1e6, spread(jd), spread(jl), spread(jw), spread(zd),
                spread(zl), spread(zw)), flush=True)
            print("%-10s   j2k decode / deflate decode %.1f x" % (name, statistics.median(jd) / statistics.median(zd)), flush=True)


if __name__ == "__main__":
    main()
