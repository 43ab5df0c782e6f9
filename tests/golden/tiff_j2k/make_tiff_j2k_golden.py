"""Generate tests/golden/tiff_j2k/: TIFF / OME-TIFF files whose strips and tiles are lossless
JPEG 2000 codestreams (Compression 33003, 33004, 33005 and 34712), the segments encoded by PIL
(OpenJPEG, no_jp2=True, irreversible=False) and wrapped by tests/_tiff_j2k.py's container writer.
Every .npy holds the pixels the file was encoded from -- the reversible path returns exactly those
-- and the manifest the SHA-256 of each plane's big-endian bytes.

    python tests/golden/tiff_j2k/make_tiff_j2k_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _tiff_j2k as J  # noqa: E402

W, H = 100, 70
OME = ('<?xml version="1.0"?><OME xmlns="http://www.openmicroscopy.org/Schemas/OME/2016-06"><Image ID="Image:0">'
       '<Pixels ID="Pixels:0" DimensionOrder="XYCZT" Type="uint16" SizeX="%d" SizeY="%d" SizeZ="2" SizeC="1" SizeT="1">'
       '<Channel ID="Channel:0:0" SamplesPerPixel="1"/><TiffData/></Pixels></Image></OME>')


def scene(w=W, h=H, seed=0, samples=1, dtype=np.uint8):
    """Smooth structure, noise and hard edges; for uint16 the whole range."""
    rng = np.random.default_rng(seed)
    top = np.iinfo(dtype).max
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for s in range(samples):
        a = 0.5 + 0.35 * np.sin(x / (5.0 + s) + seed) * np.cos(y / (7.0 - s)) + rng.normal(0, 0.05, (h, w))
        a[h // 3:h // 3 + 6, w // 4:w // 2] = 1.0 - 0.3 * s
        a[:, w - 3:] = 0.0
        out.append(np.clip(a * top, 0, top).astype(dtype))
    return np.stack(out, axis=-1) if samples > 1 else out[0]


def digest(a):
    return hashlib.sha256(J.be_bytes(np.ascontiguousarray(a))).hexdigest()


def main():
    files = []

    def add(fname, pages, bo="<", big=False, ome=False, **info):
        """pages: page_of() dicts, one plane (or RGB triple) each; SubIFDs are stored levels."""
        J.write_tiff(os.path.join(HERE, fname), pages, bo, big)
        stem = fname.split(".")[0]
        s = pages[0]["spp"]
        arr = np.stack([p["array"] for p in pages]) if len(pages) > 1 else pages[0]["array"]
        np.save(os.path.join(HERE, stem + ".npy"), arr)
        planes = {"0": {}}
        for k, p in enumerate(pages):
            for c in range(s):
                key = ("%d,%d,0" % (k, c)) if ome else ("0,%d,%d" % (c, k))
                a = p["array"][:, :, c] if s > 1 else p["array"]
                planes["0"][key] = [stem + ".npy", ([k] if len(pages) > 1 else []) + ([c] if s > 1 else []), digest(a)]
        for level, sub in enumerate(pages[0]["subifds"], 1):
            np.save(os.path.join(HERE, "%s_l%d.npy" % (stem, level)), sub["array"])
            planes[str(level)] = {"0,%d,0" % c: ["%s_l%d.npy" % (stem, level), [c] if s > 1 else [],
                                                  digest(sub["array"][:, :, c] if s > 1 else sub["array"])]
                                  for c in range(s)}
        files.append(dict(file=fname, planes=planes, byteorder=bo, bigtiff=big, samples=s, width=pages[0]["width"],
                          length=pages[0]["length"], tiled=pages[0]["tile"] is not None, bits=pages[0]["bits"],
                          compression=pages[0]["compression"], **info))

    g8, g16, rgb = scene(seed=1), scene(seed=2, dtype=np.uint16), scene(seed=3, samples=3)
    add("gray8_strips16.tif", [J.page_of(g8, 33003, rows_per_strip=16, num_resolutions=3)])
    add("gray16_tiles32_MM.tif", [J.page_of(g16, 34712, tile=(32, 32), num_resolutions=4, codeblock_size=(16, 16))], bo=">")
    add("rgb_rct_tiles16.tif", [J.page_of(rgb, 33005, tile=(16, 16), mct=1, num_resolutions=3, progression="RPCL")], mct=1)
    add("rgb_stored_strips24_big.tif", [J.page_of(rgb, 33004, rows_per_strip=24, mct=0, num_resolutions=4,
                                                  progression="CPRL", codeblock_size=(4, 4))], big=True, mct=0)
    add("rgb_planar_tiles16.tif", [J.page_of(rgb, 33003, tile=(16, 16), planar=True, num_resolutions=2)], planar=2)
    lv1, lv2 = np.ascontiguousarray(g16[::2, ::2]), np.ascontiguousarray(g16[::4, ::4])
    o = dict(tile=(32, 32), num_resolutions=5, progression="PCRL")
    add("pyramid_gray16.tif", [J.page_of(g16, 34712, subifds=[J.page_of(lv1, 34712, **o), J.page_of(lv2, 34712, **o)], **o)])
    zs = [scene(70, 50, seed=20 + z, dtype=np.uint16) for z in range(2)]
    add("ome_gray16_z2.ome.tif", [J.page_of(zs[0], 33003, tile=(32, 32), description=OME % (70, 50), precinct_size=(64, 64),
                                            codeblock_size=(32, 32), num_resolutions=2),
                                  J.page_of(zs[1], 33003, tile=(32, 32), num_resolutions=2)], ome=True)
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
