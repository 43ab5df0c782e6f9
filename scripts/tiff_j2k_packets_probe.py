"""What the JPEG 2000 packet structure costs (PBX_TIFF_F_J2K_PACKETS; k_tiff_j2k_packets walking a
longer packet list, k_tiff_j2k_gather, k_tiff_j2k_blocks reading gathered runs): scripts/
tiff_j2k_probe.py's uint16 gray band -- one cold 512-row band of a 32768-wide image in 256^2 tiles,
five levels, 64^2 code blocks -- encoded twice by PIL: with 3 quality layers and 128^2 precincts,
and as the single-layer stream of that probe.  Both are handed over with the flag set.

    python scripts/tiff_j2k_packets_probe.py [layered | single | both | all]

Per case, after a warm-up, REPS cold band writes (the cases alternating with `both`): uploaded MB,
packets and code blocks a tile, kernel_ms[0] (decode: tier 2, gather, tier 1 and the inverse
wavelet together), kernel_ms[1] (placement) and the wall time, medians with min .. max.  The
kernels are told apart by one rocprofv3 --kernel-trace --stats pass per case, each in a run of its
own.  $PBX_LIB selects the library."""
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _tiff_j2k as J  # noqa: E402
import pbx  # noqa: E402

W, ROWS, TILE, REPS, DISTINCT = 32768, 512, 256, 20, 4
GX, GY = W // TILE, ROWS // TILE
LAYERS = dict(quality_mode="rates", quality_layers=[20, 5, 0])
CASES = {"layered": dict(LAYERS, precinct_size=(128, 128)), "single": {},
         # the two halves of `layered` apart (with `all`): the gather without the precincts' smaller
         # code blocks, and those blocks without a gather
         "layers": LAYERS, "precincts": dict(precinct_size=(128, 128))}


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def plan(stream):
    data, offs = pbx.pack_chunks([stream])
    s = pbx.PbxTiffSegments()
    s.seg_w, s.seg_h, s.tiled, s.compression, s.predictor, s.flags = TILE, TILE, 1, pbx.TIFF_J2K, 1, pbx.TIFF_F_J2K_PACKETS
    s.data, s.offsets = data.ctypes.data, offs.ctypes.data
    out = (ctypes.c_uint64 * 4)()
    assert pbx.lib().pbx_test_tiff_j2k_plan(ctypes.byref(s), TILE, TILE, pbx.UINT16, 1, 0, 0, out) == 0
    return list(out)


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    names = list(CASES) if which == "all" else ["layered", "single"] if which == "both" else [which]
    rng = np.random.default_rng(0)
    order = [(3 * j + 5 * i) % DISTINCT for j in range(GY) for i in range(GX)]
    x0, y0 = 5000, 100
    k = order[(y0 // TILE) * GX + x0 // TILE]
    cut = (slice(y0 % TILE, y0 % TILE + 64), slice(x0 % TILE, x0 % TILE + 100))
    tiles = [rng.poisson(300, (TILE, TILE)).astype(np.uint16) for _ in range(DISTINCT)]
    print("band of %d rows of a %d-wide image, %d tiles of %d^2 (%d distinct), uint16 gray, 5 levels, 64^2 code blocks; %d "
          "repeats a case, median (min .. max), ms" % (ROWS, W, GX * GY, TILE, DISTINCT, REPS))
    packed = {}
    for name in names:
        enc = [J.encode(t, num_resolutions=6, codeblock_size=(64, 64), **CASES[name]) for t in tiles]
        assert all(np.array_equal(J.pil_decode(e), t) for e, t in zip(enc, tiles))
        packed[name] = pbx.pack_chunks([enc[i] for i in order])
        p = plan(enc[0])
        print("%-8s %.2f MB uploaded; tile 0: %d code blocks, %d packets, %d bytes of scratch" % (
            name, packed[name][0].nbytes / 1e6, p[1], p[2], p[3]), flush=True)
    geo = dict(seg_w=TILE, seg_h=TILE, tiled=True, predictor=1, compression=pbx.TIFF_J2K, j2k=True, flags=pbx.TIFF_F_J2K_PACKETS)
    with pbx.PixelsService(device=0) as svc:
        planes = {n: svc.create_sparse_plane(92 + i, 0, 0, 0, pbx.UINT16, W, ROWS * (REPS + 1), ROWS, big_endian=False)
                  for i, n in enumerate(names)}
        ms = {n: ([], [], []) for n in names}
        for r in range(REPS + 1):  # a cold band each time; the first round warms the call up
            for i, n in enumerate(names):
                t0 = time.perf_counter()
                a = svc.band_write_tiff(planes[n], r * ROWS, ROWS, segments=packed[n], timing=True, **geo)
                t1 = time.perf_counter()
                if r == 0:
                    st, body = svc.get_tile(pbx.TileCtx(92 + i, 0, 0, 0, x0, y0, 100, 64))
                    assert st == pbx.OK and body == J.be_bytes(tiles[k][cut]), n
                else:
                    ms[n][0].append(a[0]), ms[n][1].append(a[1]), ms[n][2].append(1e3 * (t1 - t0))
        for pid in planes.values():
            svc.release_plane(pid)
    print("%-8s | %-26s %-23s %-26s" % ("case", "decode", "place", "wall"))
    for n in names:
        print("%-8s | %-26s %-23s %-26s" % (n, spread(ms[n][0]), spread(ms[n][1]), spread(ms[n][2])), flush=True)
    if "layered" in names and "single" in names:
        print("layered decode / single decode %.3f x" % (statistics.median(ms["layered"][0]) / statistics.median(ms["single"][0])))


if __name__ == "__main__":
    main()
