"""Generate tests/golden/tiff_j2k_packets/: TIFF files whose JPEG 2000 segments use the packet
structure behind PBX_TIFF_F_J2K_PACKETS -- several quality layers, several precincts in a
resolution, SOP and EPH markers.  The segments are encoded by PIL (OpenJPEG, reversible, rates
8 / 3 / lossless), the markers inserted by tests/_tiff_j2k_packets.py (PIL reads the rewritten
streams to the same pixels: checked here), the pages wrapped by tests/_tiff_j2k.py's container
writer.  Every .npy holds the pixels the file was encoded from -- the reversible path returns
exactly those -- and the manifest the SHA-256 of each plane's big-endian bytes, in
tests/golden/tiff_j2k/'s format.

    python tests/golden/tiff_j2k_packets/make_tiff_j2k_packets_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _tiff_j2k as J  # noqa: E402
import _tiff_j2k_packets as K  # noqa: E402


def digest(a):
    return hashlib.sha256(J.be_bytes(np.ascontiguousarray(a))).hexdigest()


def layered(markers=False, **opts):
    def enc(arr, **kw):
        s = K.encode_layers(arr, **dict(kw, **opts))
        if markers:
            s = K.insert_sop_eph(s, True, True)
        assert np.array_equal(J.pil_decode(s), arr)
        return s
    return enc


def main():
    files = []

    def add(fname, page, bo="<"):
        J.write_tiff(os.path.join(HERE, fname), [page], bo)
        stem = fname.split(".")[0]
        a, s = page["array"], page["spp"]
        np.save(os.path.join(HERE, stem + ".npy"), a)
        planes = {"0,%d,0" % c: [stem + ".npy", [c] if s > 1 else [], digest(a[:, :, c] if s > 1 else a)] for c in range(s)}
        h = K.parse(page["segments"][0])
        files.append(dict(file=fname, width=page["width"], length=page["length"], bits=page["bits"], samples=s,
                          compression=page["compression"], tiled=page["tile"] is not None, byteorder=bo, bigtiff=False,
                          layers=h["layers"], scod=h["scod"], progression=K.PROGRESSIONS[h["prog"]], planes={"0": planes}))

    add("gray16_tiles32_layers3.tif",
        J97_page(K.smooth(100, 70, 1, np.uint16), layered(num_resolutions=4, progression="RPCL"), 33005, tile=(32, 32)))
    add("gray8_strips16_layers3_sop_eph_MM.tif",
        J97_page(K.smooth(100, 70, 2, np.uint8), layered(True, num_resolutions=3, progression="PCRL"), 34712, rows_per_strip=16), ">")
    add("rgb_rct_tiles32_layers2.tif",
        J97_page(K.smooth(48, 40, 3, np.uint8, samples=3),
                 layered(rates=(6, 0), precinct=(32, 32), cb=(16, 16), mct=1, num_resolutions=3, progression="CPRL"), 33003,
                 tile=(32, 32)))
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(dict(files=files), f, indent=1, sort_keys=True)
        f.write("\n")


def J97_page(arr, encoder, compression, **kw):
    import _tiff_j2k97 as J97
    return J97.page_of(arr, compression, encoder=encoder, **kw)


if __name__ == "__main__":
    main()
