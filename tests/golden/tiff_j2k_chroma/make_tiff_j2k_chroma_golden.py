"""Generate tests/golden/tiff_j2k_chroma/: TIFF files whose JPEG 2000 segments carry subsampled
chroma and / or YCbCr components outside the codestream (PBX_TIFF_F_J2K_SUBSAMPLED,
PBX_TIFF_F_J2K_YCBCR).  PIL's OpenJPEG encoder cannot subsample: every segment is merged at tier 2
from three single-component PIL streams by tests/_tiff_j2k_chroma.py, and the pages are wrapped by
tests/_tiff_j2k.py's container writer.

    ycc422_tiles32_33003.tif     4:2:2 (2 x 1), 5/3, tiles of 32 x 32, Compression 33003 and
                                 PhotometricInterpretation 2: Aperio's habit, read as YCbCr only
                                 with aperio_ycbcr
    ycc420_strips16_photo6.tif   4:2:0 (2 x 2), 9/7, strips of 16 rows, PhotometricInterpretation 6
    ycc422_strips8_w37_MM.tif    4:2:2 (2 x 1), 5/3, strips of 8 rows of the odd width 37 (23 rows: the
                                 last strip has 7), 16 x 16 precincts, RPCL, big-endian, Photometric 6

Every .npy holds the three components as the library stores them WITHOUT the conversion (Y, and
Cb, Cr replicated): of a reversible file the encoder's input exactly, of the irreversible one the
float64 model rounded half to even, with the mask (packed bits) of the samples whose real value
lies within 1/64 of a half-integer.  The manifest keeps the SHA-256 of each plane's bytes, the
share of samples inside that window (chosen by seed to be no higher than 0.0361, the highest of
the 8-bit files of tests/golden/tiff_j2k97/) and, where the subsampled sizes are even, the largest
difference between Pillow's RGB and ycc_to_rgb of these planes.

    python tests/golden/tiff_j2k_chroma/make_tiff_j2k_chroma_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _tiff_j2k as J  # noqa: E402
import _tiff_j2k97 as J97  # noqa: E402
import _tiff_j2k_chroma as C  # noqa: E402
from _tiff_jpeg import ycc_to_rgb  # noqa: E402

SHARE = 0.0361


def digest(a):
    return hashlib.sha256(J.be_bytes(np.ascontiguousarray(a))).hexdigest()


def main():
    files = []

    def add(fname, page, bo="<", **info):
        J.write_tiff(os.path.join(HERE, fname), [page], bo)
        stem = fname.split(".")[0]
        lossy = J.parse(page["segments"][0])["transform"] == 0
        inside = 0.0
        if lossy:
            model = C.page_model(page)
            want, mask = J97.rint(model, 8), J97.in_window(model, J97.WINDOW8)
            inside = float(mask.mean())
            assert inside <= SHARE, (fname, inside)
            np.save(os.path.join(HERE, stem + "_mask.npy"), np.packbits(mask))
        else:
            want = C.page_planes(page, False)
        np.save(os.path.join(HERE, stem + ".npy"), want)
        xs, ys = page["factors"]
        pil = None
        if all(J.parse(s)["w"] % xs == 0 and J.parse(s)["h"] % ys == 0 for s in page["segments"]):
            got = J97.assemble(page, J.pil_decode).astype(np.int64)
            pil = int(np.abs(got - ycc_to_rgb(want[:, :, 0], want[:, :, 1], want[:, :, 2]).astype(np.int64)).max())
        files.append(dict(file=fname, width=page["width"], length=page["length"], bits=8, samples=3, factors=[xs, ys],
                          compression=page["compression"], photometric=page["photometric"], tiled=page["tile"] is not None,
                          byteorder=bo, lossy=lossy, inside=round(inside, 4), pil=pil,
                          planes={"0": {"0,%d,0" % c: [stem + ".npy", [c], digest(want[:, :, c])] for c in range(3)}}, **info))

    add("ycc422_tiles32_33003.tif",
        C.page_of(C.ycc_smooth(100, 70, 1), 2, 1, 33003, tile=(32, 32), photometric=2, num_resolutions=4, progression="LRCP"),
        aperio=True)
    for seed in range(2, 40):  # the first seed whose model keeps the share
        pg = C.page_of(C.ycc_smooth(72, 40, seed), 2, 2, 33005, rows_per_strip=16, photometric=6, irreversible=True,
                       num_resolutions=3, progression="RLCP")
        if J97.in_window(C.page_model(pg), J97.WINDOW8).mean() <= SHARE:
            break
    add("ycc420_strips16_photo6.tif", pg, seed=seed)
    add("ycc422_strips8_w37_MM.tif",
        C.page_of(C.ycc_smooth(37, 23, 3), 2, 1, 34712, rows_per_strip=8, photometric=6, num_resolutions=3, progression="RPCL",
                  precinct_size=(16, 16), codeblock_size=(8, 8)), ">")
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(dict(files=files), f, indent=1, sort_keys=True)
        f.write("\n")
    total = 0
    for fn in sorted(os.listdir(HERE)):
        n = os.path.getsize(os.path.join(HERE, fn))
        total += n
        assert n <= 34268 or fn.endswith(".py"), (fn, n)  # the largest file of tests/golden/tiff_j2k/
    print("%d files, %d bytes" % (len(os.listdir(HERE)), total), [(f["file"], f["inside"], f["pil"]) for f in files])


if __name__ == "__main__":
    main()
