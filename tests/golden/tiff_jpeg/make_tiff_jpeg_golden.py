"""Generate tests/golden/tiff_jpeg/: JPEG-compressed (Compression 7) TIFF / OME-TIFF files, the
segments encoded by PIL (libjpeg-turbo) and wrapped by tests/_tiff_jpeg.py's container writer, plus
one file from PIL's own TIFF writer.  Every .npy holds the pixels PIL (libtiff + libjpeg-turbo)
decodes from the file itself; a SubIFD level, which PIL does not open, is decoded from a one-page
file of the same segments.  One file is written by tifffile + imagecodecs, through the interpreter
that has them (CONDA_PY), and judged by PIL like the rest: imagecodecs links IJG libjpeg 9, which
upsamples differently, so it writes but does not judge.

    python tests/golden/tiff_jpeg/make_tiff_jpeg_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _tiff_jpeg as J  # noqa: E402

W, H = 100, 70
CONDA_PY = "/opt/conda/bin/python3.9"
OME =('<?xml version="1.0"?><OME xmlns="http://www.openmicroscopy.org/Schemas/OME/2016-06"><Image ID="Image:0">'
       '<Pixels ID="Pixels:0" DimensionOrder="XYCZT" Type="uint8" SizeX="%d" SizeY="%d" SizeZ="2" SizeC="3" SizeT="1">'
       '<Channel ID="Channel:0:0" SamplesPerPixel="3"/><TiffData/></Pixels></Image></OME>')


def scene(w=W, h=H, seed=0, samples=3):
    """Smooth structure plus noise and a few hard edges: every quantiser band gets something."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for s in range(samples):
        a = 128 + 90 * np.sin(x / (5.0 + s) + seed) * np.cos(y / (7.0 - s)) + rng.normal(0, 12, (h, w))
        a[h // 3:h // 3 + 6, w // 4:w // 2] = 250 - 100 * s
        a[:, w - 3:] = 5 + 40 * s
        out.append(np.clip(a, 0, 255).astype(np.uint8))
    return np.stack(out, axis=-1) if samples > 1 else out[0]


def pil_pages(path):
    im = Image.open(path)
    out = []
    for k in range(getattr(im, "n_frames", 1)):
        im.seek(k)
        out.append(np.asarray(im).copy())
    return out


def main():
    files = []

    def add(fname, pages, bo="<", big=False, levels=None, ome=None, **info):
        """pages: page_of() dicts (one plane each, or Z planes for `ome`); levels: {level: page}
        of the SubIFDs of page 0, decoded from one-page files of their own."""
        path = os.path.join(HERE, fname)
        J.write_tiff(path, pages, bo, big)
        planes = {}
        npy = fname.split(".")[0] + ".npy"
        got = pil_pages(path)
        arr = np.stack(got) if len(got) > 1 else got[0]
        np.save(os.path.join(HERE, npy), arr)
        s = pages[0]["spp"]
        planes["0"] = {}
        for k in range(len(got)):
            for c in range(s):
                key = ("%d,%d,0" % (k, c)) if ome else ("0,%d,%d" % (c, k))
                planes["0"][key] = [npy, ([k] if len(got) > 1 else []) + ([c] if s > 1 else [])]
        for level, pg in (levels or {}).items():
            with tempfile.TemporaryDirectory() as td:
                J.write_tiff(os.path.join(td, "l.tif"), [dict(pg, subifds=[])], bo, big)
                a = pil_pages(os.path.join(td, "l.tif"))[0]
            n2 = fname.split(".")[0] + "_l%d.npy" % level
            np.save(os.path.join(HERE, n2), a)
            planes[str(level)] = {"0,%d,0" % c: [n2, [c] if s > 1 else []] for c in range(s)}
        files.append(dict(file=fname, planes=planes, byteorder=bo, bigtiff=big, samples=s, width=pages[0]["width"],
                          length=pages[0]["length"], tiled=pages[0]["tile"] is not None, **info))

    rgb, gray = scene(seed=1), scene(seed=2, samples=1)
    add("ycbcr444_strips16.tif", [J.page_of(rgb, rows_per_strip=16, subsampling=0, quality=85)], ycbcr=True, sampling=[1, 1])
    add("ycbcr422_tiles16.tif", [J.page_of(rgb, tile=(16, 16), subsampling=1, quality=75)], ycbcr=True, sampling=[2, 1])
    add("ycbcr420_tiles32_MM.tif", [J.page_of(rgb, tile=(32, 32), subsampling=2, quality=75)], bo=">", ycbcr=True,
        sampling=[2, 2])
    add("ycbcr420_strips8_big.tif", [J.page_of(rgb, rows_per_strip=8, subsampling=2, quality=90)], big=True, ycbcr=True,
        sampling=[2, 2])
    add("gray_tiles16_MM.tif", [J.page_of(gray, tile=(16, 16), quality=80)], bo=">", ycbcr=False, sampling=[1, 1])
    add("gray_strips_restart.tif", [J.page_of(gray, rows_per_strip=24, quality=75, restart_blocks=3)], ycbcr=False,
        sampling=[1, 1], restart=3)
    add("rgb_planar_strips16.tif", [J.page_of(rgb, rows_per_strip=16, planar=2, photometric=2, quality=85)], ycbcr=False,
        sampling=[1, 1], planar=2)
    add("ycbcr420_restart_tiles32.tif", [J.page_of(rgb, tile=(32, 32), subsampling=2, quality=75, restart_blocks=2)],
        ycbcr=True, sampling=[2, 2], restart=2)
    add("ycbcr422_no_tables_tag.tif", [J.page_of(rgb, rows_per_strip=32, subsampling=1, quality=60, tables="segment")],
        ycbcr=True, sampling=[2, 1], tables="segment")
    lv1, lv2 = np.ascontiguousarray(rgb[::2, ::2]), np.ascontiguousarray(rgb[::4, ::4])
    o = dict(tile=(16, 16), subsampling=2, quality=80)
    p1, p2 = J.page_of(lv1, **o), J.page_of(lv2, **o)
    add("pyramid_ycbcr420.tif", [J.page_of(rgb, subifds=[p1, p2], **o)], levels={1: p1, 2: p2}, ycbcr=True, sampling=[2, 2])
    zs = [scene(70, 50, seed=20 + z) for z in range(2)]
    add("ome_rgb_z2.ome.tif", [J.page_of(zs[0], tile=(32, 32), subsampling=0, quality=85, description=OME % (70, 50)),
                               J.page_of(zs[1], tile=(32, 32), subsampling=0, quality=85)],
        ome=dict(size_z=2, size_c=3, size_t=1), ycbcr=True, sampling=[1, 1])
    # PIL's own TIFF writer (libtiff): JPEG-compressed RGB, the tables in tag 347
    name = "pil_rgb_jpeg.tif"
    Image.fromarray(rgb).save(os.path.join(HERE, name), compression="jpeg", quality=80)
    np.save(os.path.join(HERE, "pil_rgb_jpeg.npy"), pil_pages(os.path.join(HERE, name))[0])
    files.append(dict(file=name, planes={"0": {"0,%d,0" % c: ["pil_rgb_jpeg.npy", [c]] for c in range(3)}}, byteorder="<",
                      bigtiff=False, samples=3, width=W, length=H, tiled=False, pil=True))

    # tifffile + imagecodecs (libjpeg 9): tiled YCbCr 4:2:0, every tile a whole stream with its own
    # tables, no tag 347.  Written by the interpreter that has them; judged, like the rest, by PIL.
    name = "tifffile_ycbcr420_tiles32.tif"
    src = os.path.join(HERE, "_rgb.npy")
    np.save(src, rgb)
    try:
        subprocess.check_call([CONDA_PY, "-c",
                               "import sys, numpy, tifffile\n"
                               "tifffile.imwrite(sys.argv[2], numpy.load(sys.argv[1]), tile=(32, 32), compression='jpeg',"
                               " photometric='rgb', metadata=None)\n", src, os.path.join(HERE, name)])
    finally:
        os.remove(src)
    np.save(os.path.join(HERE, "tifffile_ycbcr420_tiles32.npy"), pil_pages(os.path.join(HERE, name))[0])
    files.append(dict(file=name, planes={"0": {"0,%d,0" % c: ["tifffile_ycbcr420_tiles32.npy", [c]] for c in range(3)}},
                      byteorder="<", bigtiff=False, samples=3, width=W, length=H, tiled=True, ycbcr=True, sampling=[2, 2],
                      tables="segment"))

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
