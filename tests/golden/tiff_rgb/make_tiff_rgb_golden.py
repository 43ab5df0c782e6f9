"""Generate tests/golden/tiff_rgb/: RGB / RGBA TIFF and OME-TIFF files written by tifffile
2021.7.2 + imagecodecs (LZW ones recompressed by libtiff's tiffcp, as tests/golden/tiff does, and
one written by PIL / libtiff), with the images they hold as big-endian (rows, width, samples)
arrays in .npy.  Sample s of an image is channel c0 + s of the planes the library makes of it.

Run with the interpreter that has those writers:
    /opt/conda/bin/python3.9 tests/golden/tiff_rgb/make_tiff_rgb_golden.py

Images are 150 x 100, tiles 64 x 64 (padded edges), strips of 32 rows (a short last one).
Variants of one pixel type hold the same image.  manifest.json lists every file: its layout and
"planes" = {level: {"z,c,t": [npy, sample]}}."""
import json
import os
import subprocess
import tempfile

import numpy as np
import tifffile

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, TILE, RPS = 150, 100, (64, 64), 32
TIFFCP = os.path.join(os.path.dirname(os.sys.executable), "tiffcp")


def scene(dtype, samples, w=W, h=H, seed=0):
    """A smooth colour scene with photon-like noise, every component its own."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = np.zeros((h, w, samples), dtype)
    for s in range(samples):
        base = 2.0 + np.sin(x / (13.0 + 3 * s)) * np.cos(y / (9.0 + 2 * s)) + 0.004 * (s + 1) * x
        img = rng.poisson(np.maximum(base, 1)).astype(np.int64)
        out[:, :, s] = (img * (3011 if out.dtype.itemsize == 2 else 23) + 7 * s) & (0xFFFF if out.dtype.itemsize == 2 else 0xFF)
    return out


def main():
    files = []
    images = {"rgb8": scene(np.uint8, 3, seed=1), "rgb16": scene(np.uint16, 3, seed=2),
              "rgba8": scene(np.uint8, 4, seed=3)}
    for name, a in images.items():
        np.save(os.path.join(HERE, name + ".npy"), a.astype(a.dtype.newbyteorder(">")))

    def planes_of(npy, samples, z=0, t=0):
        return {"%d,%d,%d" % (z, c, t): [npy, c] for c in range(samples)}

    def write(fname, name, layout, comp, pred, bo, planar=1, **kw):
        a = images[name]
        s = a.shape[2]
        opts = dict(byteorder=bo, photometric="rgb", metadata=None,
                    planarconfig="separate" if planar == 2 else "contig")
        if s == 4:
            opts["extrasamples"] = ["unassalpha"]
        if comp == "deflate":
            opts["compression"] = "adobe_deflate"
        if pred == 2 and comp == "deflate":
            opts["predictor"] = True
        if layout == "tiles":
            opts["tile"] = TILE
        else:
            opts["rowsperstrip"] = RPS
        opts.update(kw)
        data = np.moveaxis(a, 2, 0) if planar == 2 else a
        dst = os.path.join(HERE, fname)
        if comp == "lzw":  # imagecodecs has no LZW encoder: tiffcp recompresses the stored file
            with tempfile.TemporaryDirectory() as tmp:
                src = os.path.join(tmp, fname)
                tifffile.imwrite(src, data, **opts)
                cmd = [TIFFCP, "-c", "lzw:%d" % pred, "-B" if bo == ">" else "-L",
                       "-p", "separate" if planar == 2 else "contig"]
                cmd += ["-t", "-w", str(TILE[0]), "-l", str(TILE[1])] if layout == "tiles" else ["-s", "-r", str(RPS)]
                subprocess.check_call(cmd + [src, dst])
        else:
            tifffile.imwrite(dst, data, **opts)
        files.append(dict(file=fname, planes={"0": planes_of(name + ".npy", s)}, layout=layout, compression=comp,
                          predictor=pred, byteorder=bo, planar=planar, samples=s, width=W, length=H))

    write("rgb8_strips_lzw_p2_II.tif", "rgb8", "strips", "lzw", 2, "<")
    write("rgb8_tiles_deflate_p2_MM.tif", "rgb8", "tiles", "deflate", 2, ">")
    write("rgb8_tiles_none_p1_II.tif", "rgb8", "tiles", "none", 1, "<")
    write("rgb16_tiles_lzw_p2_MM.tif", "rgb16", "tiles", "lzw", 2, ">")
    write("rgb16_strips_deflate_p1_II.tif", "rgb16", "strips", "deflate", 1, "<")
    write("rgba8_strips_deflate_p2_II.tif", "rgba8", "strips", "deflate", 2, "<")
    write("rgba8_strips_lzw_p1_MM.tif", "rgba8", "strips", "lzw", 1, ">")
    # PlanarConfiguration = 2: one group of segments per sample
    write("rgb8_planar_tiles_deflate_p2_II.tif", "rgb8", "tiles", "deflate", 2, "<", planar=2)
    write("rgb8_planar_strips_lzw_p2_MM.tif", "rgb8", "strips", "lzw", 2, ">", planar=2)
    # (16-bit planar LZW as strips only: tiffcp re-tiles separate planes byte by byte, which is
    # wrong for 16-bit samples; strips of the same size are copied as they are)
    write("rgb16_planar_strips_lzw_p2_MM.tif", "rgb16", "strips", "lzw", 2, ">", planar=2)
    write("rgb16_planar_tiles_deflate_p1_II.tif", "rgb16", "tiles", "deflate", 1, "<", planar=2)

    # PIL / libtiff: RGB, LZW with Predictor = 2, libtiff's own strip size
    from PIL import Image
    Image.fromarray(images["rgb8"]).save(os.path.join(HERE, "rgb8_pil_lzw_p2.tif"), compression="tiff_lzw",
                                         tiffinfo={317: 2})
    files.append(dict(file="rgb8_pil_lzw_p2.tif", planes={"0": planes_of("rgb8.npy", 3)}, layout="strips",
                      compression="lzw", predictor=2, byteorder="<", planar=1, samples=3, width=W, length=H))

    # RGB OME-TIFF, Z = 2: one IFD per Z with three samples, <Channel SamplesPerPixel="3">, SizeC = 3
    ome = np.stack([scene(np.uint8, 3, 70, 50, seed=20 + z) for z in range(2)])  # Z Y X S
    np.save(os.path.join(HERE, "ome_rgb_z2.npy"), ome)
    tifffile.imwrite(os.path.join(HERE, "ome_rgb_z2.ome.tif"), ome, tile=(32, 32), photometric="rgb",
                     compression="adobe_deflate", predictor=True, metadata={"axes": "ZYXS"}, ome=True)
    files.append(dict(file="ome_rgb_z2.ome.tif", layout="tiles", compression="deflate", predictor=2, byteorder="<",
                      planar=1, samples=3, width=70, length=50, ome=dict(size_z=2, size_c=3, size_t=1),
                      planes={"0": {"%d,%d,0" % (z, c): ["ome_rgb_z2.npy", [z, c]] for z in range(2) for c in range(3)}}))

    # an RGB pyramid: two SubIFD levels under the one main IFD
    full = images["rgb8"]
    lv1, lv2 = full[::2, ::2].copy(), full[::4, ::4].copy()
    np.save(os.path.join(HERE, "pyramid_rgb_l1.npy"), lv1)
    np.save(os.path.join(HERE, "pyramid_rgb_l2.npy"), lv2)
    with tifffile.TiffWriter(os.path.join(HERE, "pyramid_rgb8_deflate.tif")) as tw:
        o = dict(tile=(32, 32), compression="adobe_deflate", predictor=True, photometric="rgb", metadata=None)
        tw.write(full, subifds=2, **o)
        tw.write(lv1, subfiletype=1, **o)
        tw.write(lv2, subfiletype=1, **o)
    files.append(dict(file="pyramid_rgb8_deflate.tif", layout="tiles", compression="deflate", predictor=2,
                      byteorder="<", planar=1, samples=3, width=W, length=H,
                      planes={"0": planes_of("rgb8.npy", 3), "1": planes_of("pyramid_rgb_l1.npy", 3),
                              "2": planes_of("pyramid_rgb_l2.npy", 3)}))

    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump({"files": files}, f, indent=1, sort_keys=True)
    total = 0
    for fn in sorted(os.listdir(HERE)):
        n = os.path.getsize(os.path.join(HERE, fn))
        total += n
        assert n <= 128 * 1024 or fn.endswith(".py"), (fn, n)
    print("%d files, %d bytes" % (len(os.listdir(HERE)), total))
    assert total < 1 << 20


if __name__ == "__main__":
    main()
