"""Generate tests/golden/tiff/: TIFF / OME-TIFF files written by tifffile 2021.7.2 + imagecodecs
2021.8.26 (and one by PIL / libtiff), with the planes they hold as big-endian samples in .npy.
That imagecodecs has no LZW encoder, so every LZW file is the tifffile-written uncompressed
file recompressed by libtiff's tiffcp (same layout, predictor and byte order options).

Run with the interpreter that has those writers:
    /opt/conda/bin/python3.9 tests/golden/tiff/make_tiff_golden.py

Images are 150 x 100, so that 64 x 64 tiles have padded edges and strips of 32 rows a short last
one.  The whole cross product of {strips, tiles} x {none, LZW, deflate} x predictor {1, 2} x
{II, MM} x pixel type would be some 3 MiB; the files below cover every pair of those axes with
each pixel type instead and stay under 1 MiB together.  Variants of one pixel type hold the same
image, so one .npy per type serves them all.  The PIL-written 700 x 500 ramp has no .npy: it is
(x mod 100 + y // 4) mod 256, which the tests compute.  manifest.json lists every file."""
import json
import os
import subprocess
import tempfile

import numpy as np
import tifffile

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, TILE, RPS = 150, 100, (64, 64), 32
DTYPES = {"uint8": "u1", "int16": "i2", "uint16": "u2", "uint32": "u4", "float": "f4"}


def scene(kind, w=W, h=H, seed=0):
    """A smooth scene with photon-like noise (compressible, but every match length occurs)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 1.5 + np.sin(x / 17.0) * np.cos(y / 11.0) + 0.004 * x
    img = rng.poisson(np.maximum(base, 1)).astype(np.int64)
    if kind == "u1":
        return (img & 0xFF).astype(np.uint8)
    if kind == "i2":
        return (img * 1237 - 9000).astype(np.int16)
    if kind == "u2":
        return (img * 3011).astype(np.uint16)
    if kind == "u4":
        return (img * 170000001).astype(np.uint32)
    return (img * 0.25).astype(np.float32)


TIFFCP = os.path.join(os.path.dirname(os.sys.executable), "tiffcp")


def lzw_copy(fname, a, opts, layout, pred, bo, tile=TILE):
    """tifffile writes the file uncompressed; tiffcp (libtiff) rewrites it LZW-compressed."""
    opts = {k: v for k, v in opts.items() if k not in ("compression", "predictor")}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, fname)
        tifffile.imwrite(src, a, **opts)
        cmd = [TIFFCP, "-c", "lzw:%d" % pred, "-B" if bo == ">" else "-L"]
        cmd += ["-t", "-w", str(tile[0]), "-l", str(tile[1])] if layout == "tiles" else ["-s", "-r", str(RPS)]
        if opts.get("bigtiff"):
            cmd.append("-8")
        subprocess.check_call(cmd + [src, os.path.join(HERE, fname)])


def main():
    files = []
    planes = {}
    for name, k in DTYPES.items():
        planes[name] = scene(k)
        np.save(os.path.join(HERE, "plane_%s.npy" % name), planes[name].astype(">" + k))

    def write(fname, a, npy, layout, comp, pred, bo, **kw):
        opts = dict(byteorder=bo, photometric="minisblack", metadata=None)
        if comp != "none":
            opts["compression"] = {"lzw": "lzw", "deflate": "adobe_deflate"}[comp]
        if pred == 2:
            opts["predictor"] = True
        if layout == "tiles":
            opts["tile"] = TILE
        else:
            opts["rowsperstrip"] = RPS
        opts.update(kw)
        if comp == "lzw":
            lzw_copy(fname, a, opts, layout, pred, bo)
        else:
            tifffile.imwrite(os.path.join(HERE, fname), a, **opts)
        files.append(dict(file=fname, planes={"0": {"0,0,0": npy}}, layout=layout, compression=comp,
                          predictor=pred, byteorder=bo, width=int(a.shape[-1]), length=int(a.shape[-2]),
                          bigtiff=bool(kw.get("bigtiff", False))))

    # compressed: layout x predictor x byte order pairwise, for every integer type and codec
    combos = [("strips", 1, "<"), ("tiles", 2, ">"), ("strips", 2, ">"), ("tiles", 1, "<"),
              ("strips", 2, "<"), ("tiles", 2, "<")]
    for name in ("uint8", "int16", "uint16", "uint32"):
        for comp in ("lzw", "deflate"):
            for n, (layout, pred, bo) in enumerate(combos):
                if n >= 4 and (name, comp) != ("uint16", "lzw"):
                    continue
                fname = "%s_%s_%s_p%d_%s.tif" % (name, layout, comp, pred, "II" if bo == "<" else "MM")
                write(fname, planes[name], "plane_%s.npy" % name, layout, comp, pred, bo)
    # uncompressed
    # (predictor 1 only: tifffile applies a predictor only together with a compression)
    for name, layout, pred, bo in (("uint8", "strips", 1, "<"), ("uint8", "tiles", 1, ">"),
                                   ("uint16", "tiles", 1, "<"), ("int16", "strips", 1, ">")):
        fname = "%s_%s_none_p%d_%s.tif" % (name, layout, pred, "II" if bo == "<" else "MM")
        write(fname, planes[name], "plane_%s.npy" % name, layout, "none", pred, bo)
    # float32: predictor 1 only
    write("float_strips_lzw_p1_II.tif", planes["float"], "plane_float.npy", "strips", "lzw", 1, "<")
    write("float_tiles_deflate_p1_MM.tif", planes["float"], "plane_float.npy", "tiles", "deflate", 1, ">")
    # BigTIFF
    write("uint16_tiles_lzw_p2_II_big.tif", planes["uint16"], "plane_uint16.npy", "tiles", "lzw", 2, "<",
          bigtiff=True)

    # OME-TIFF, Z = 2, C = 3, T = 2, stored in DimensionOrder XYCTZ (IFD k: c fastest, then t, then z)
    rng = np.random.default_rng(5)
    ome = np.stack([scene("u1", 70, 50, seed=10 + k) for k in range(12)]).reshape(2, 2, 3, 50, 70)  # Z T C Y X
    ome_planes = {}
    for z in range(2):
        for t in range(2):
            for c in range(3):
                fn = "ome_z%d_c%d_t%d.npy" % (z, c, t)
                np.save(os.path.join(HERE, fn), ome[z, t, c])
                ome_planes["%d,%d,%d" % (z, c, t)] = fn
    lzw_copy("ome_zct_lzw.ome.tif", ome, dict(tile=(32, 32), photometric="minisblack",
                                              metadata={"axes": "ZTCYX"}, ome=True), "tiles", 1, "<", (32, 32))
    files.append(dict(file="ome_zct_lzw.ome.tif", planes={"0": ome_planes}, layout="tiles", compression="lzw",
                      predictor=1, byteorder="<", width=70, length=50, bigtiff=False,
                      ome=dict(size_z=2, size_c=3, size_t=2, order="XYCTZ")))

    # a pyramid: two SubIFD levels under the one main IFD
    full = planes["uint16"]
    lv1 = full[::2, ::2].copy()
    lv2 = full[::4, ::4].copy()
    np.save(os.path.join(HERE, "pyramid_l1.npy"), lv1.astype(">u2"))
    np.save(os.path.join(HERE, "pyramid_l2.npy"), lv2.astype(">u2"))
    # (deflate: tiffcp does not carry SubIFDs over)
    with tifffile.TiffWriter(os.path.join(HERE, "pyramid_uint16_deflate.tif")) as tw:
        o = dict(tile=(32, 32), compression="adobe_deflate", predictor=True, photometric="minisblack", metadata=None)
        tw.write(full, subifds=2, **o)
        tw.write(lv1, subfiletype=1, **o)
        tw.write(lv2, subfiletype=1, **o)
    files.append(dict(file="pyramid_uint16_deflate.tif", layout="tiles", compression="deflate", predictor=2,
                      byteorder="<", width=W, length=H, bigtiff=False,
                      planes={"0": {"0,0,0": "plane_uint16.npy"}, "1": {"0,0,0": "pyramid_l1.npy"},
                              "2": {"0,0,0": "pyramid_l2.npy"}}))

    # a second writer's LZW streams: PIL / libtiff, a ramp that compresses to long strings
    from PIL import Image
    ramp = ((np.arange(700)[None, :] % 100 + np.arange(500)[:, None] // 4) & 0xFF).astype(np.uint8)
    Image.fromarray(ramp).save(os.path.join(HERE, "ramp_pil_lzw.tif"), compression="tiff_lzw")
    files.append(dict(file="ramp_pil_lzw.tif", planes={"0": {"0,0,0": None}}, layout="strips",
                      compression="lzw", predictor=1, byteorder="<", width=700, length=500, bigtiff=False,
                      ramp=True))

    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump({"files": files}, f, indent=1, sort_keys=True)
    total = 0
    for fn in sorted(os.listdir(HERE)):
        n = os.path.getsize(os.path.join(HERE, fn))
        total += n
        assert n <= 64 * 1024 or fn.endswith(".py"), (fn, n)
    print("%d files, %d bytes" % (len(os.listdir(HERE)), total))
    assert total < 1 << 20


if __name__ == "__main__":
    main()
