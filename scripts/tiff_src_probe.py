"""What loading a plane from TIFF segments costs on the device: kernel_ms[0]
(decoders + k_tiff_unpred) and kernel_ms[1] (k_zarr_place) of one plane registered with
register_tiff_planes, the wall time of the call (upload included), and for comparison the same
tiles decoded by libtiff through PIL on 1 and 16 threads.

  python scripts/tiff_src_probe.py [side] [--out FILE.json]
      A side^2 (default 16384) uint16 plane stored as 512^2 tiles x {LZW, deflate} x predictor
      {1, 2}; the data is uniform noise (G_NOISE's statistics) and a smooth scene with photon
      noise (a 4096^2 scene repeated over the plane; every tile is its own stream).  LZW tiles
      are written by libtiff (through PIL), deflate tiles by zlib level 6.
"""
import io
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ.get("PBX_PKG") or os.path.join(ROOT, "omero-ms-pixel-buffer_amd"))
import _tiff_src as T  # noqa: E402
import pbx  # noqa: E402

TILE, REPS, THREADS = 512, 3, 16


def planes(side):
    rng = np.random.default_rng(0)
    yield "noise", rng.integers(0, 65536, (side, side), dtype=np.uint16)
    n = min(side, 4096)
    y, x = np.mgrid[0:n, 0:n]
    base = 400 + 300 * np.sin(x / 97.0) * np.cos(y / 61.0) + 0.05 * x
    scene = rng.poisson(base).astype(np.uint16)
    yield "poisson scene", np.tile(scene, (side // n, side // n))


def encode_tile(args):
    """(segment bytes, a one-strip TIFF holding it for PIL) of one tile."""
    from PIL import Image, TiffImagePlugin
    t, comp, pred = args
    if comp == pbx.TIFF_LZW:
        TiffImagePlugin.STRIP_SIZE = 1 << 24  # one strip
        b = io.BytesIO()
        Image.fromarray(t).save(b, format="TIFF", compression="tiff_lzw", tiffinfo={317: pred})
        blob = b.getvalue()
    else:
        seg = zlib.compress((T.predict2(t) if pred == 2 else t).tobytes(), 6)
        blob = T.write_tiff(None, [dict(width=TILE, length=TILE, bits=16, sampleformat=1, compression=8,
                                       predictor=pred, rows_per_strip=TILE, segments=[seg])])
    return blob


def strip_of(blob):
    import struct
    # the one strip of a little-endian classic TIFF: tags 273 / 279 of its first IFD
    ifd = struct.unpack("<I", blob[4:8])[0]
    n = struct.unpack("<H", blob[ifd:ifd + 2])[0]
    tags = {}
    for k in range(n):
        tag, typ, cnt, val = struct.unpack("<HHII", blob[ifd + 2 + 12 * k:ifd + 14 + 12 * k])
        tags[tag] = (cnt, val)
    assert tags[273][0] == 1 and tags[279][0] == 1, "one strip expected"
    return blob[tags[273][1]:tags[273][1] + tags[279][1]]


def pil_decode(blob):
    from PIL import Image
    im = Image.open(io.BytesIO(blob))
    im.load()
    return im.size[0]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    side = int(args[0]) if args else 16384
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    assert side % TILE == 0
    results = []
    image = 1
    with pbx.PixelsService() as svc, ThreadPoolExecutor(THREADS) as pool:
        for dname, a in planes(side):
            tiles = [np.ascontiguousarray(a[y:y + TILE, x:x + TILE]) for y in range(0, side, TILE)
                     for x in range(0, side, TILE)]
            want = a.astype(">u2").tobytes()
            for cname, comp in (("lzw", pbx.TIFF_LZW), ("deflate", pbx.TIFF_DEFLATE)):
                for pred in (1, 2):
                    blobs = list(pool.map(encode_tile, [(t, comp, pred) for t in tiles]))
                    segs = pbx.pack_chunks([strip_of(b) for b in blobs])
                    spec = dict(z=0, c=0, t=0, pixel_type=pbx.UINT16, size_x=side, size_y=side, seg_w=TILE,
                                seg_h=TILE, tiled=True, compression=comp, predictor=pred, big_endian=False,
                                segments=segs)
                    runs = []
                    for rep in range(REPS + 1):  # the first is the warm-up
                        image += 1
                        svc.synchronize()
                        t0 = time.perf_counter()
                        (pid,), ms = svc.register_tiff_planes([dict(spec, image_id=image)], timing=True)
                        svc.synchronize()
                        wall = (time.perf_counter() - t0) * 1e3
                        if rep == 0:
                            assert svc.read_plane_be(pid, len(want)) == want, "decoded plane differs"
                        else:
                            runs.append((ms[0], ms[1], wall))
                        svc.release_plane(pid)
                    cpu = {}
                    for nt in (1, THREADS):
                        with ThreadPoolExecutor(nt) as p2:
                            t0 = time.perf_counter()
                            list(p2.map(pil_decode, blobs))
                            cpu[nt] = (time.perf_counter() - t0) * 1e3
                    runs.sort(key=lambda r: r[0])
                    dec, place, wall = runs[len(runs) // 2]
                    gb = a.nbytes / 1e9
                    r = dict(data=dname, compression=cname, predictor=pred, side=side, tiles=len(tiles),
                             compressed_bytes=int(segs[1][-1]), decoded_bytes=a.nbytes,
                             decode_ms=dec, place_ms=place, wall_ms=wall,
                             decode_gbs=gb / (dec / 1e3), place_gbs=gb / (place / 1e3),
                             decode_ms_all=[x[0] for x in runs], wall_ms_all=[x[2] for x in runs],
                             libtiff_1_thread_ms=cpu[1], libtiff_16_threads_ms=cpu[THREADS])
                    results.append(r)
                    print("%-13s %-7s p%d  ratio %.2f  decode %8.2f ms (%6.1f GB/s)  place %6.2f ms (%6.1f GB/s)  "
                          "wall %8.1f ms | libtiff 1 thread %8.0f ms, 16 threads %7.0f ms"
                          % (dname, cname, pred, a.nbytes / r["compressed_bytes"], dec, r["decode_gbs"], place,
                             r["place_gbs"], wall, cpu[1], cpu[THREADS]), flush=True)
    if out:
        with open(out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
