"""What subsampled chroma and the YCbCr conversion cost: scripts/tiff_j2k_probe.py's RGB band (one
cold 512-row band of a 32768-wide uint8 image in 256^2 tiles, five levels, 64^2 code blocks, 5/3)
from the same pixels as 4:4:4 (three 1 x 1 components stored as they are: k_tiff_j2k_place), as
4:4:4 with the YCbCr conversion and as 4:2:2 with it (k_tiff_j2k_place_chroma; the chroma dropped
to every second column and merged by tests/_tiff_j2k_chroma.py).

    python scripts/tiff_j2k_chroma_probe.py            the three cases alternating, REPS repeats:
                                                       medians with min .. max of uploaded MB,
                                                       kernel_ms[0] (decode), kernel_ms[1]
                                                       (placement) and the call's wall time
    python scripts/tiff_j2k_chroma_probe.py 422        one case alone (444, 444ycc or 422), for a
                                                       kernel-trace pass in a run of its own

The pixels of every case are checked against the tiles.  $PBX_LIB selects the library."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _tiff_j2k as J  # noqa: E402
import _tiff_j2k_chroma as C  # noqa: E402
import pbx  # noqa: E402
from _tiff_jpeg import ycc_to_rgb  # noqa: E402

W, ROWS, TILE, REPS, DISTINCT = 32768, 512, 256, 20, 4
GX, GY = W // TILE, ROWS // TILE
OPTS = dict(num_resolutions=6, codeblock_size=(64, 64))


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def main():
    only = sys.argv[1] if len(sys.argv) > 1 else None
    rng = np.random.default_rng(0)
    order = [(3 * j + 5 * i) % DISTINCT for j in range(GY) for i in range(GX)]
    x0, y0 = 5000, 100
    k = order[(y0 // TILE) * GX + x0 // TILE]
    cut = (slice(y0 % TILE, y0 % TILE + 64), slice(x0 % TILE, x0 % TILE + 100))
    tiles = [np.stack([rng.poisson(40 + 25 * s, (TILE, TILE)) for s in range(3)], axis=2).astype(np.uint8) for _ in range(DISTINCT)]
    cases = {}
    full = [J.encode(t, mct=0, **OPTS) for t in tiles]
    cases["444"] = (full, 0, [t[:, :, 0] for t in tiles])
    cases["444ycc"] = (full, pbx.TIFF_F_J2K_YCBCR, [ycc_to_rgb(t[:, :, 0], t[:, :, 1], t[:, :, 2])[:, :, 0] for t in tiles])
    half = [C.encode(t[:, :, 0], C.sub(t[:, :, 1], 2, 1), C.sub(t[:, :, 2], 2, 1), 2, 1, **OPTS)[0] for t in tiles]
    cases["422"] = (half, pbx.TIFF_F_J2K_SUBSAMPLED | pbx.TIFF_F_J2K_YCBCR,
                    [C.planes(t[:, :, 0], C.sub(t[:, :, 1], 2, 1), C.sub(t[:, :, 2], 2, 1), 2, 1, True)[:, :, 0] for t in tiles])
    names = [only] if only else list(cases)
    print("band of %d rows of a %d-wide uint8 image, 3 components, %d tiles of %d^2 (%d distinct), 5 levels, 64^2 code blocks, "
          "5/3; sample 0 stored; %d repeats a case, median (min .. max), ms" % (ROWS, W, GX * GY, TILE, DISTINCT, REPS))
    print("%-8s %8s | %-28s %-23s %-28s" % ("case", "MB", "decode", "place", "wall"), flush=True)
    geo = dict(seg_w=TILE, seg_h=TILE, tiled=True, predictor=1, samples_per_pixel=3, sample=0, compression=pbx.TIFF_J2K, j2k=True)
    with pbx.PixelsService(device=0) as svc:
        packed = {n: pbx.pack_chunks([cases[n][0][i] for i in order]) for n in names}
        planes = {n: svc.create_sparse_plane(100 + i, 0, 0, 0, pbx.UINT8, W, ROWS * (REPS + 1), ROWS, big_endian=False)
                  for i, n in enumerate(names)}
        dec, plc, wall = ({n: [] for n in names} for _ in range(3))
        for r in range(REPS + 1):  # a cold band each time; the first round warms the calls up
            for i, n in enumerate(names):
                t0 = time.perf_counter()
                a = svc.band_write_tiff(planes[n], r * ROWS, ROWS, segments=packed[n], timing=True, flags=cases[n][1], **geo)
                t1 = time.perf_counter()
                if r == 0:
                    st, body = svc.get_tile(pbx.TileCtx(100 + i, 0, 0, 0, x0, y0, 100, 64))
                    assert st == pbx.OK and body == cases[n][2][k][cut].tobytes(), n
                else:
                    dec[n].append(a[0]), plc[n].append(a[1]), wall[n].append(1e3 * (t1 - t0))
        for n in names:
            svc.release_plane(planes[n])
            print("%-8s %8.2f | %-28s %-23s %-28s" % (n, packed[n][0].nbytes / 1e6, spread(dec[n]), spread(plc[n]), spread(wall[n])),
                  flush=True)
    if not only:
        print("4:2:2 decode / 4:4:4 decode %.3f; coefficients 2/3" % (statistics.median(dec["422"]) / statistics.median(dec["444"])))


if __name__ == "__main__":
    main()
