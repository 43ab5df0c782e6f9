"""Generate tests/golden/tiff_fp/: float TIFF files stored with Predictor = 3 (the floating-point
predictor, Adobe TIFF Technical Note 3) and Zstandard TIFF files (Compression = 50000), written by
tifffile 2021.7.2 + imagecodecs 2021.8.26 and by libtiff's tiffcp, with the planes they hold as
big-endian samples in .npy.  imagecodecs has no LZW encoder, so every LZW file is the
tifffile-written uncompressed file recompressed by tiffcp -c lzw:3 (libtiff applies Predictor 3
itself) -- in II files only: this libtiff swaps the samples of an MM file before it splits them
into byte planes, so its MM Predictor 3 files hold the planes in reverse and neither tifffile nor
the Technical Note's rule reads them back.  The MM LZW files are therefore written by the tests'
own writer (tests/_tiff_src.py and tests/_tiff_fp.py, writer "helper") and read back here with
tifffile, which pins them.  tifffile writes zstd frames that carry their content size, tiffcp (libtiff) frames
without one: both shapes are here.

Run with the interpreter that has those writers:
    /opt/conda/bin/python3.9 tests/golden/tiff_fp/make_tiff_fp_golden.py

The images are the 150 x 100 scene of tests/golden/tiff/make_tiff_golden.py (64 x 64 tiles have
padded edges, strips of 32 rows a short last one) as float32 and as float64.  The float64 plane
would be 120,000 bytes as .npy, over the 64 KiB a fixture may have: it is the float32 plane
divided by 3 in float64 (every mantissa byte in use), which the tests compute from
plane_float.npy (manifest: "derive": "f8_div3").  manifest.json lists every file."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import tifffile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tiff"))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_tiff_golden import RPS, TILE, scene  # noqa: E402

TIFFCP = os.path.join(os.path.dirname(sys.executable), "tiffcp")
W, H = 150, 100


def tiffcp(fname, a, codec, layout, bo, bigtiff=False):
    """tifffile writes the file uncompressed; tiffcp (libtiff) recompresses it (codec as tiffcp's
    -c takes it: lzw:3, zstd, zstd:2 ...)."""
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, fname)
        tifffile.imwrite(src, a, photometric="minisblack", metadata=None, byteorder=bo)
        cmd = [TIFFCP, "-c", codec, "-B" if bo == ">" else "-L"]
        cmd += ["-t", "-w", str(TILE[0]), "-l", str(TILE[1])] if layout == "tiles" else ["-s", "-r", str(RPS)]
        if bigtiff:
            cmd.append("-8")
        subprocess.check_call(cmd + [src, os.path.join(HERE, fname)])


def main():
    files = []
    f4 = scene("f4")
    f8 = f4.astype(np.float64) / 3
    u2 = scene("u2")
    np.save(os.path.join(HERE, "plane_float.npy"), f4.astype(">f4"))
    np.save(os.path.join(HERE, "plane_uint16.npy"), u2.astype(">u2"))
    planes = {"float": (f4, dict(npy="plane_float.npy")),
              "double": (f8, dict(npy="plane_float.npy", derive="f8_div3")),
              "uint16": (u2, dict(npy="plane_uint16.npy"))}

    def entry(fname, ref, layout, comp, pred, bo, writer, **more):
        files.append(dict(dict(file=fname, planes={"0": {"0,0,0": ref}}, layout=layout, compression=comp,
                               predictor=pred, byteorder=bo, width=W, length=H, bigtiff=False, writer=writer),
                          **more))

    def write(name, layout, comp, pred, bo, writer="tifffile", suffix="", **kw):
        a, ref = planes[name]
        fname = "%s_%s_%s_p%d_%s%s.tif" % (name, layout, comp, pred, "II" if bo == "<" else "MM",
                                            suffix if writer == "tifffile" else "_" + writer)
        if writer == "tiffcp":
            tiffcp(fname, a, "%s:%d" % (comp, pred) if pred != 1 else comp, layout, bo, **kw)
        elif writer == "helper":
            import _tiff_fp
            import _tiff_src
            geo = dict(tile=TILE) if layout == "tiles" else dict(rows_per_strip=RPS)
            _tiff_src.write_tiff(os.path.join(HERE, fname), [_tiff_fp.page_of(a.astype(bo + a.dtype.str[1:]), 5, pred, **geo)],
                                 byteorder=bo)
            back = tifffile.imread(os.path.join(HERE, fname))
            assert back.dtype.itemsize == a.dtype.itemsize and back.tobytes() == a.tobytes(), fname
        else:
            opts = dict(byteorder=bo, photometric="minisblack", metadata=None,
                        compression={"deflate": "adobe_deflate", "zstd": "zstd"}[comp])
            if pred != 1:
                opts["predictor"] = True
            if layout == "tiles":
                opts["tile"] = TILE
            else:
                opts["rowsperstrip"] = RPS
            opts.update(kw)
            tifffile.imwrite(os.path.join(HERE, fname), a, **opts)
        entry(fname, ref, layout, comp, pred, bo, writer, bigtiff=bool(kw.get("bigtiff", False)))

    # Predictor 3: {strips, tiles} x {deflate, zstd, LZW} x {II, MM} pairwise, float32 and float64
    combos = [("strips", "deflate", "<"), ("tiles", "deflate", ">"), ("strips", "zstd", ">"),
              ("tiles", "zstd", "<"), ("strips", "lzw", "<"), ("tiles", "lzw", ">")]
    for name, flip in (("float", False), ("double", True)):
        for layout, comp, bo in combos:
            if flip:
                bo = "<" if bo == ">" else ">"
            write(name, layout, comp, 3, bo, writer="tifffile" if comp != "lzw" else "tiffcp" if bo == "<" else "helper")
    # libtiff's own zstd frames (no content size, a window descriptor) behind Predictor 3
    write("float", "tiles", "zstd", 3, "<", writer="tiffcp")
    # uint16 zstd with Predictor 1 and 2: tifffile's frames and libtiff's
    for layout, pred, bo in (("strips", 1, "<"), ("tiles", 2, ">")):
        write("uint16", layout, "zstd", pred, bo)
    for layout, pred, bo in (("tiles", 1, ">"), ("strips", 2, "<")):
        write("uint16", layout, "zstd", pred, bo, writer="tiffcp")
    # BigTIFF
    write("float", "strips", "zstd", 3, "<", suffix="_big", bigtiff=True)

    # a pyramid: two SubIFD levels under the one main IFD, zstd + Predictor 3
    lv1, lv2 = f4[::2, ::2].copy(), f4[::4, ::4].copy()
    np.save(os.path.join(HERE, "pyramid_l1.npy"), lv1.astype(">f4"))
    np.save(os.path.join(HERE, "pyramid_l2.npy"), lv2.astype(">f4"))
    with tifffile.TiffWriter(os.path.join(HERE, "pyramid_float_zstd_p3.tif")) as tw:
        o = dict(tile=(32, 32), compression="zstd", predictor=True, photometric="minisblack", metadata=None)
        tw.write(f4, subifds=2, **o)
        tw.write(lv1, subfiletype=1, **o)
        tw.write(lv2, subfiletype=1, **o)
    files.append(dict(file="pyramid_float_zstd_p3.tif", layout="tiles", compression="zstd", predictor=3,
                      byteorder="<", width=W, length=H, bigtiff=False, writer="tifffile",
                      planes={"0": {"0,0,0": dict(npy="plane_float.npy")}, "1": {"0,0,0": dict(npy="pyramid_l1.npy")},
                              "2": {"0,0,0": dict(npy="pyramid_l2.npy")}}))

    # planar (PlanarConfiguration 2), two float32 samples: every sample is a channel
    second = (f4[::-1] * 1.5).astype(np.float32)
    np.save(os.path.join(HERE, "planar_s1.npy"), second.astype(">f4"))
    tifffile.imwrite(os.path.join(HERE, "planar2_float_zstd_p3.tif"), np.stack([f4, second]), planarconfig="separate",
                     photometric="minisblack", compression="zstd", predictor=True, tile=TILE, metadata=None)
    files.append(dict(file="planar2_float_zstd_p3.tif", layout="tiles", compression="zstd", predictor=3,
                      byteorder="<", width=W, length=H, bigtiff=False, writer="tifffile", samples=2,
                      planes={"0": {"0,0,0": dict(npy="plane_float.npy"), "0,1,0": dict(npy="planar_s1.npy")}}))

    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump({"files": files}, f, indent=1, sort_keys=True)
    total = 0
    for fn in sorted(os.listdir(HERE)):
        if fn == "__pycache__":
            continue
        n = os.path.getsize(os.path.join(HERE, fn))
        total += n
        assert n <= 64 * 1024, (fn, n)
    print("%d files, %d bytes" % (len(os.listdir(HERE)), total))
    assert total < 1 << 20


if __name__ == "__main__":
    main()
