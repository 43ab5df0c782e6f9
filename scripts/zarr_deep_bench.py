"""What Zarr chunks that hold several planes cost, and the one-plane-per-chunk
placement A/B.  $PBX_LIB selects the library and $PBX_PKG the directory that holds the pbx
package (an older commit's, for a library without the newer symbols).

  python scripts/zarr_deep_bench.py depth1 [--cache FILE]
      bench.py's Zarr plane (16384^2 uint16 G_NOISE, 512^2 blosc-lz4 chunks) registered with
      pbx_plane_register_zarr: decode and place ms of three registrations after a warm-up.
      Run it with the parent commit's library and this one alternating (--cache keeps the
      encoded chunks between the processes).
  python scripts/zarr_deep_bench.py deep
      The same 16 planes of 4096^2 uint16 G_NOISE registered from one-plane chunks (512^2) and
      from chunks of 16 planes (16 x 512 x 512), blosc lz4 shuffle: decode GB/s, place GB/s
      (2 x plane bytes / place time), streams in flight; then one 512-row band of slice 5
      written with pbx_band_write_zarr_deep: streams decoded, decode and place ms, wall ms.
      PBX_ZARR_NO_BLOCK_SKIP=1 decodes every block of the covering chunks (the A/B of the skip).
"""
import ctypes
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ.get("PBX_PKG") or os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))
import _zarr  # noqa: E402
import pbx  # noqa: E402

REPS = 3


def noise_planes(svc, n, side):
    out = []
    for k in range(n):
        pid = svc.register_plane(20, 0, 0, k, pbx.UINT16, side, side, generator="noise", plane_no=k)
        out.append(np.frombuffer(svc.read_plane_be(pid, side * side * 2), ">u2").reshape(side, side))
        svc.release_plane(pid)
    return out


def encode(blocks):
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda b: _zarr.blosc_encode(b.tobytes(), 2), blocks))


def planned(packed, cx, cy, sx, sy, depth, slices, y0=0, rows=0):
    """pbx_test_zarr_plan: [streams, sum of dlen, blocks skipped, scratch bytes]."""
    data, offsets = packed
    zc = pbx.PbxZarrChunks()
    zc.chunk_x, zc.chunk_y, zc.codec = cx, cy, pbx.ZARR_BLOSC
    zc.data, zc.offsets = data.ctypes.data, offsets.ctypes.data
    sl = (ctypes.c_int32 * len(slices))(*slices)
    out = (ctypes.c_uint64 * 4)()
    assert pbx.lib().pbx_test_zarr_plan(ctypes.byref(zc), sx, sy, 2, depth, sl, len(slices), y0, rows, out) == 0
    return list(out)


def depth1(cache):
    side, chunk = 16384, 512
    with pbx.PixelsService(device=0) as svc:
        if cache and os.path.exists(cache):
            z = np.load(cache)
            packed = (z["data"], z["offsets"])
        else:
            plane = noise_planes(svc, 1, side)[0]
            packed = pbx.pack_chunks(encode(_zarr.chunk_grid(plane, chunk, chunk)))
            if cache:
                np.savez(cache, data=packed[0], offsets=packed[1])
        dec, plc = [], []
        for r in range(REPS + 1):
            pid, (md, mp) = svc.register_zarr_plane(21, 0, 0, 0, pbx.UINT16, side, side, chunk, chunk, "blosc",
                                                    packed, timing=True)
            if r:
                dec.append(md), plc.append(mp)
            svc.release_plane(pid)
    print("depth1 %s: place ms %.4f (%s), decode ms %.3f (%s)"
          % (os.environ.get("PBX_LIB", "tree"), sum(plc) / REPS, " ".join("%.4f" % v for v in plc),
             sum(dec) / REPS, " ".join("%.3f" % v for v in dec)), flush=True)


def deep():
    side, chunk, depth, slc = 4096, 512, 16, 5
    g = side // chunk
    raw = depth * side * side * 2
    with pbx.PixelsService(device=0, sparse_band_rows=chunk) as svc:
        planes = noise_planes(svc, depth, side)
        vol = np.stack(planes).astype(">u2")  # (stacking alone gives the native byte order)
        flat = [pbx.pack_chunks(encode(_zarr.chunk_grid(p, chunk, chunk))) for p in planes]
        cubes = [np.ascontiguousarray(vol[:, j * chunk:(j + 1) * chunk, i * chunk:(i + 1) * chunk])
                 for j in range(g) for i in range(g)]
        files = encode(cubes)
        layer = pbx.pack_chunks(files)
        descs = [dict(image_id=30, z=k, c=0, t=0, pixel_type=pbx.UINT16, size_x=side, size_y=side) for k in range(depth)]
        ways = {
            "one plane per chunk": (
                lambda: svc.register_zarr_planes([dict(d, chunk_x=chunk, chunk_y=chunk, codec="blosc", chunks=flat[k])
                                                  for k, d in enumerate(descs)], timing=True),
                sum(planned(f, chunk, chunk, side, side, 1, [0])[0] for f in flat), sum(len(f[0]) for f in flat)),
            "16 planes per chunk": (
                lambda: svc.register_zarr_planes_deep(descs, [(0, k) for k in range(depth)],
                                                      [dict(chunk_x=chunk, chunk_y=chunk, codec="blosc", chunks=layer,
                                                            chunk_planes=depth)], timing=True),
                planned(layer, chunk, chunk, side, side, depth, list(range(depth)))[0], len(layer[0])),
        }
        for name, (call, streams, cbytes) in ways.items():
            dec, plc, wall = [], [], []
            for r in range(REPS + 1):
                t0 = time.perf_counter()
                ids, (md, mp) = call()
                t1 = time.perf_counter()
                if r:
                    dec.append(md), plc.append(mp), wall.append(1e3 * (t1 - t0))
                if r == REPS:
                    for k in (0, slc, depth - 1):
                        assert svc.read_plane_be(ids[k], side * side * 2) == planes[k].tobytes(), (name, k)
                for pid in ids:
                    svc.release_plane(pid)
            md, mp = sum(dec) / REPS, sum(plc) / REPS
            print("%s: %.0f MB compressed, %d streams in flight, decode %.3f ms = %.1f GB/s decoded, place %.3f ms = "
                  "%.0f GB/s, wall %.1f ms incl. upload" % (name, cbytes / 1e6, streams, md, raw / md / 1e6, mp,
                                                            2 * raw / mp / 1e6, sum(wall) / REPS), flush=True)
        # one cold band (rows 512..1023 = chunk row 1) of slice 5
        row = pbx.pack_chunks(files[g:2 * g])
        plan = planned(row, chunk, chunk, side, side, depth, [slc], chunk, chunk)
        dec, plc, wall = [], [], []
        for r in range(REPS + 1):
            sp = svc.create_sparse_plane(40 + r, slc, 0, 0, pbx.UINT16, side, side, chunk)
            t0 = time.perf_counter()
            md, mp = svc.band_write_zarr(sp, chunk, chunk, chunk, chunk, "blosc", row, timing=True,
                                         chunk_planes=depth, slice=slc)
            t1 = time.perf_counter()
            if r:
                dec.append(md), plc.append(mp), wall.append(1e3 * (t1 - t0))
            st, body = svc.get_tile(pbx.TileCtx(40 + r, slc, 0, 0, 1000, chunk + 7, 512, 300))
            assert st == pbx.OK and body == planes[slc][chunk + 7:chunk + 307, 1000:1512].tobytes()
            svc.release_plane(sp)
        print("band of slice %d (%d rows, %d chunks of %d planes)%s: %d streams decoded (%d blocks skipped, %.1f MB "
              "decoded), decode %.3f ms, place %.3f ms, wall %.2f ms incl. upload of %.0f MB"
              % (slc, chunk, g, depth, " without the block skip" if os.environ.get("PBX_ZARR_NO_BLOCK_SKIP") else "",
                 plan[0], plan[2], plan[1] / 1e6, sum(dec) / REPS, sum(plc) / REPS, sum(wall) / REPS,
                 len(row[0]) / 1e6), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "depth1":
        depth1(sys.argv[3] if len(sys.argv) > 3 and sys.argv[2] == "--cache" else None)
    elif len(sys.argv) > 1 and sys.argv[1] == "deep":
        deep()
    else:
        sys.exit(__doc__)
