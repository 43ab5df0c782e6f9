"""Generate tests/golden/tiff_j2k97/: TIFF files whose strips and tiles are lossy JPEG 2000
codestreams (9/7 wavelet, scalar quantisation; Compression 33003, 33004, 33005 and 34712), the
segments encoded by PIL (OpenJPEG, no_jp2=True, irreversible=True) and wrapped by
tests/_tiff_j2k.py's container writer.  The lossy path has no original to return: every .npy
holds rint(model), tests/_tiff_j2k97.py's float64 model rounded half to even and clamped, every
_mask.npy (bits, np.packbits) the pixels whose model value lies within the window of its precision
of a half-integer, and the manifest the SHA-256 of each plane's big-endian bytes, the share of
pixels inside the window and D, the largest |PIL - rint(model)| of the file.  A machine without
the model's minutes checks against these.

    python tests/golden/tiff_j2k97/make_tiff_j2k97_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _tiff_j2k as J  # noqa: E402
import _tiff_j2k97 as M  # noqa: E402

W, H = 72, 50


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

    def add(fname, page, bo="<", big=False, **info):
        """page: one page_of() dict (a plane or an RGB triple); its SubIFDs are stored levels."""
        J.write_tiff(os.path.join(HERE, fname), [page], bo, big)
        stem = fname.split(".")[0]
        s, prec = page["spp"], page["bits"]
        planes, D, share = {}, 0, []
        for level, pg in enumerate([page] + page["subifds"]):
            model = M.assemble(pg)
            want, mask = M.rint(model, prec), M.in_window(model, M.window(prec))
            pil = M.assemble(pg, J.pil_decode)
            ok, inside, _ = M.close(pil, model, M.window(prec), prec)
            assert ok or prec == 16, fname  # (OpenJPEG's own constant: DESIGN 10b)
            D = max(D, int(np.abs(pil.astype(np.int64) - want.astype(np.int64)).max()))
            share.append(round(inside, 4))
            npy = stem + (".npy" if level == 0 else "_l%d.npy" % level)
            np.save(os.path.join(HERE, npy), want)
            np.save(os.path.join(HERE, npy.replace(".npy", "_mask.npy")), np.packbits(mask))
            planes[str(level)] = {"0,%d,0" % c: [npy, [c] if s > 1 else [], digest(want[:, :, c] if s > 1 else want)]
                                  for c in range(s)}
        files.append(dict(file=fname, planes=planes, byteorder=bo, bigtiff=big, samples=s, width=page["width"],
                          length=page["length"], tiled=page["tile"] is not None, bits=prec,
                          compression=page["compression"], D=D, inside=share, **info))

    g8, g16, rgb = scene(seed=1), scene(seed=2, dtype=np.uint16), scene(seed=3, samples=3)
    add("gray8_strips16.tif", M.page_of(g8, 33003, rows_per_strip=16, num_resolutions=3))
    add("gray16_tiles32_MM.tif", M.page_of(g16, 34712, tile=(32, 32), num_resolutions=4, codeblock_size=(16, 16)), bo=">")
    add("rgb_ict_tiles16.tif", M.page_of(rgb, 33005, tile=(16, 16), mct=1, num_resolutions=3, progression="RPCL"), mct=1)
    add("rgb_stored_strips24_big.tif", M.page_of(rgb, 33004, rows_per_strip=24, mct=0, num_resolutions=4, progression="CPRL",
                                                 codeblock_size=(4, 4), quality_mode="dB", quality_layers=[38]),
        big=True, mct=0)
    add("rgb_planar_tiles16.tif", M.page_of(rgb, 33003, tile=(16, 16), planar=True, num_resolutions=2), planar=2)
    add("gray8_style1_tiles32.tif", M.page_of(g8, 33005, tile=(32, 32), num_resolutions=4,
                                              encoder=lambda a, **kw: M.to_style1(M.encode(a, **kw))), qstyle=1)
    lv1 = np.ascontiguousarray(g16[::2, ::2])
    o = dict(tile=(32, 32), num_resolutions=5, progression="PCRL")
    add("pyramid_mixed_gray16.tif", M.page_of(g16, 34712, subifds=[J.page_of(lv1, 34712, **o)], **o), mixed=True)
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump({"files": files}, f, indent=1, sort_keys=True)
    total = 0
    for fn in sorted(os.listdir(HERE)):
        n = os.path.getsize(os.path.join(HERE, fn))
        total += n
        assert n <= 34268 or fn.endswith(".py"), (fn, n)  # the largest file of tests/golden/tiff_j2k/
    print("%d files, %d bytes" % (len(os.listdir(HERE)), total))


if __name__ == "__main__":
    main()
