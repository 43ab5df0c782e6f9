"""JPEG 2000 TIFF segments with quality layers, precincts and SOP / EPH markers on the GPU
(PBX_TIFF_F_J2K_PACKETS): k_tiff_j2k_packets walking the host's packet list, k_tiff_j2k_gather
copying a block's bytes out of several packets into one run, and k_tiff_j2k_blocks reading that run.

The yardstick is the CPU hook (pbx_test_tiff_j2k_decode), which runs the very functions the kernels
run (tiff_j2k_dev.h) and is held to PIL, to tests/_tiff_j2k_packets.py's model and to the encoder's
input by tests/test_tiff_j2k_packets_host.py; reversible streams are held to the input here too."""
import hashlib
import itertools
import json
import os

import numpy as np
import pytest

import _tiff_j2k as J
import _tiff_j2k97 as J97
import _tiff_j2k_packets as K
import pbx
from test_gpu_tiff_j2k import ptype, rows_of, specs_of

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiff_j2k_packets")
with open(os.path.join(GOLD, "manifest.json")) as _f:
    FILES = json.load(_f)["files"]
_ids = itertools.count(8_900_000)  # disjoint from the other test files (shared service)
FLAG = pbx.TIFF_F_J2K_PACKETS


def page(a, encoder, compression=33005, **kw):
    return J97.page_of(a, compression, encoder=encoder, **kw)


def layered(**opts):
    return lambda a, **kw: K.encode_layers(a, **dict(kw, **opts))


def hook(pg, flags=FLAG):
    rc, msg, want = K.hook_page(pg, flags)
    assert rc == 0, msg
    return want


def flagged(pg, image, flags=FLAG, **kw):
    return [dict(sp, flags=flags) if flags else sp for sp in specs_of(pg, image, **kw)]


def check_pages(svc, pages, what=""):
    """Every page a layer of ONE registration; every plane byte for byte the CPU hook's, and for a
    reversible page the array it was encoded from."""
    specs, wants = [], []
    for pg in pages:
        sp = flagged(pg, next(_ids), pg.get("flags", FLAG))
        a = hook(pg, pg.get("flags", FLAG))
        if not pg.get("lossy"):
            assert np.array_equal(a, pg["array"]), what
        specs += sp
        wants += [a[:, :, c] if a.ndim == 3 else a for c in range(len(sp))]
    ids = svc.register_tiff_planes(specs)
    try:
        for k, (pid, want) in enumerate(zip(ids, wants)):
            got = np.frombuffer(svc.read_plane_be(pid, want.nbytes), want.dtype.newbyteorder(">")).reshape(want.shape)
            assert np.array_equal(got, want), (what, k, specs[k]["size_x"], specs[k]["size_y"], specs[k]["c"],
                                               np.argwhere(got != want)[:4].tolist())
    finally:
        for pid in ids:
            svc.release_plane(pid)


def check_bands(svc, pg, B, what=""):
    """The page band by band (B rows a band) through pbx_band_write_tiff_j2k."""
    want = hook(pg)
    h, w = want.shape[:2]
    sp0 = flagged(pg, 0)[0]
    data, offsets = sp0["segments"]
    gx, seg_h = (-(-w // sp0["seg_w"]) if sp0["tiled"] else 1), sp0["seg_h"]
    rows = min(B, h)
    image = next(_ids)
    pid = svc.create_sparse_plane(image, 0, 0, 0, ptype(want), w, h, rows, big_endian=False)
    try:
        for r0 in range(0, h, rows):
            n = min(rows, h - r0)
            k0, k1 = (r0 // seg_h) * gx, -(-(r0 + n) // seg_h) * gx
            piece = (data[int(offsets[k0]):int(offsets[k1])].copy(), offsets[k0:k1 + 1] - offsets[k0])
            svc.band_write_tiff(pid, r0, n, sp0["seg_w"], seg_h, sp0["tiled"], pbx.TIFF_J2K, 1, piece, j2k=True, flags=FLAG)
            got = np.frombuffer(rows_of(svc, image, r0, n, w), want.dtype.newbyteorder(">")).reshape(n, w)
            assert np.array_equal(got, want[r0:r0 + n]), (what, B, r0)
        assert set(svc.band_info(pid)[1]) == {pbx.BS_READY}
    finally:
        svc.release_plane(pid)


# ------------------------------------------------------------------------------ 40 x 24
W0, H0 = 40, 24
LAYOUTS = [dict(rows_per_strip=8), dict(rows_per_strip=16), dict(tile=(16, 16))]


def pages_40x24(prog, markers=False):
    a = K.smooth(W0, H0, 5, np.uint16)
    enc = layered(num_resolutions=4, progression=prog)
    if markers:
        plain = enc
        enc = lambda x, **kw: K.insert_sop_eph(plain(x, **kw), True, True)
    return [page(a, enc, **lay) for lay in LAYOUTS]


@pytest.mark.parametrize("prog", K.PROGRESSIONS)
def test_layers_and_precincts_in_strips_and_tiles(service, prog):
    """3 layers x 16 x 16 precincts x 8 x 8 blocks x 3 levels, in strips of 8 and 16 rows and tiles
    of 16 x 16: whole (one registration of the three), and band by band."""
    pages = pages_40x24(prog)
    h = K.parse(pages[1]["segments"][0])
    assert (h["layers"], h["levels"], h["prog"], h["pp"][-1]) == (3, 3, K.PROGRESSIONS.index(prog), (4, 4))
    assert K.facts(pages[1]["segments"][0])["several"]
    check_pages(service, pages, prog)
    for pg in pages:
        for B in (16, 40, 100):
            check_bands(service, pg, B, prog)


def test_sop_and_eph(service):
    pages = pages_40x24("RPCL", markers=True)
    assert K.parse(pages[0]["segments"][0])["scod"] == 7
    check_pages(service, pages, "SOP + EPH")
    check_bands(service, pages[2], 16, "SOP + EPH")


# ------------------------------------------------------------------------------ RGB
def test_one_sample_of_three_between_sentinels(service):
    """RGB 48 x 32 through the RCT, 2 layers, 32 x 32 precincts over 16 x 16 blocks: rows 9 .. 22
    of one sample by pbx_band_write_tiff_j2k, the rows around them and the sibling planes as they were."""
    S, h, w = 3, 32, 48
    a = K.smooth(w, h, 23, np.uint8, samples=3)
    pg = page(a, layered(rates=(6, 0), precinct=(32, 32), cb=(16, 16), mct=1, num_resolutions=3), tile=(32, 32))
    hd = K.parse(pg["segments"][0])
    assert hd["layers"] == 2 and hd["mct"] == 1 and hd["pp"][-1] == (5, 5)
    want = hook(pg)
    assert np.array_equal(want, a)
    sp0 = flagged(pg, 0)[0]
    for target in range(S):
        image = next(_ids)
        pids = [service.create_sparse_plane(image, 0, c, 0, pbx.UINT8, w, h, h, big_endian=False) for c in range(S)]
        try:
            for c in range(S):
                if c != target:
                    service.band_write(pids[c], 0, h, bytes([0x30 + c]) * (h * w))
            service.band_write(pids[target], 0, 9, b"\xA5" * (9 * w))
            service.band_write(pids[target], 23, 9, b"\x5A" * (9 * w))
            service.band_write_tiff(pids[target], 9, 14, 32, 32, True, pbx.TIFF_J2K, 1, sp0["segments"], samples_per_pixel=S,
                                    sample=target, j2k=True, flags=FLAG)
            assert service.band_info(pids[target])[1] == [pbx.BS_READY]
            got = rows_of(service, image, 0, h, w, c=target)
            assert got[:9 * w] == b"\xA5" * (9 * w) and got[23 * w:] == b"\x5A" * (9 * w)
            assert got[9 * w:23 * w] == want[9:23, :, target].tobytes()
            for c in range(S):
                if c != target:
                    assert rows_of(service, image, 0, h, w, c=c) == bytes([0x30 + c]) * (h * w)
        finally:
            for pid in pids:
                service.release_plane(pid)


# ------------------------------------------------------------------------------ the gather
def test_gather_at_the_waves_edges(service):
    """One 64 x 64 tile of noise, a single 64 x 64 block, 8 layers cut by K.wave_edges: a pass
    without bytes, then contributions of 1, 63, 64, 65 and 129 bytes and one of thousands (a lane
    per byte, stride 64: a partial wave, exactly one, one and a byte, two and a byte, many), a layer
    that leaves the block out.  And four such blocks (128 x 128, one level) in the same launch."""
    recut = lambda a, **kw: K.relayer(K.encode_plain(a, **kw), 8, K.wave_edges)
    pages = [page(K.noise(64, 64, 64), recut, tile=(64, 64), num_resolutions=1, codeblock_size=(64, 64)),
             page(K.noise(128, 128, 128), recut, tile=(128, 128), num_resolutions=2, codeblock_size=(64, 64), progression="CPRL")]
    for pg, nblocks in zip(pages, (1, 4)):
        f = K.facts(pg["segments"][0])
        L = f["lengths"]
        assert len(L) == 7 * nblocks and 0 in L and 1 in L and any(60 <= n <= 68 for n in L) and any(n > 128 for n in L), L
        assert {63, 64, 65, 129} <= set(L) and f["lblock_grows"]
    check_pages(service, pages, "gather")


def test_strip_sweep(service):
    """Widths 1 .. 20 x heights 1 .. 12, gray uint8, 2 layers, 8 x 8 precincts over 4 x 4 blocks,
    levels and progressions rotating: precincts of one sample, bands a precinct misses, resolutions
    of one row.  Five widths a registration."""
    for w0 in range(1, 21, 5):
        pages = []
        for w in range(w0, w0 + 5):
            for h in range(1, 13):
                a = K.smooth(w, h, 100 * w + h, np.uint8) if (w + h) % 3 else K.noise(w, h, 100 * w + h)
                pages.append(page(a, layered(rates=(4, 0), precinct=(8, 8), cb=(4, 4), num_resolutions=1 + (w + 2 * h) % 4,
                                             progression=K.PROGRESSIONS[(w + h) % 5]), rows_per_strip=8))
        check_pages(service, pages, "w %d .. %d" % (w0, w0 + 4))


# ------------------------------------------------------------------------------ irreversible
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["u8", "u16"])
def test_irreversible_layers(service, dtype):
    a = K.smooth(W0, H0, 21, dtype)
    enc = lambda x, **kw: J97.encode(x, **dict(kw, quality_mode="dB", quality_layers=[30, 40, 50], precinct_size=(16, 16),
                                              codeblock_size=(8, 8)))
    pages = [dict(page(a, enc, num_resolutions=4, **lay), lossy=True) for lay in LAYOUTS[1:]]
    hd = K.parse(pages[0]["segments"][0])
    assert hd["transform"] == 0 and hd["layers"] == 3 and hd["scod"] & 1 and K.facts(pages[0]["segments"][0])["several"]
    check_pages(service, pages, "9/7")
    check_bands(service, pages[1], 16, "9/7")


def test_simple_and_layered_layers_in_one_registration(service):
    """A flag-clear one-layer stream, a layered 5/3 stream and a layered 9/7 stream as three layers
    (pbx_tiff_segments) of one registration: gathered and ungathered blocks, int32 and float planes."""
    a = K.smooth(W0, H0, 31, np.uint16)
    lossy = lambda x, **kw: J97.encode(x, **dict(kw, quality_mode="dB", quality_layers=[30, 45], precinct_size=(16, 16),
                                                codeblock_size=(8, 8)))
    pages = [dict(J.page_of(a, tile=(16, 16), num_resolutions=3), flags=0),
             page(a, layered(num_resolutions=4, progression="PCRL"), tile=(16, 16)),
             dict(page(a, lossy, num_resolutions=4, rows_per_strip=16), lossy=True),
             dict(J.page_of(K.noise(W0, H0, 32), rows_per_strip=8, num_resolutions=2), flags=0)]
    assert K.parse(pages[0]["segments"][0])["layers"] == 1 and K.parse(pages[2]["segments"][0])["layers"] == 2
    check_pages(service, pages, "mixed")


# ------------------------------------------------------------------------------ refusals
def refused(service, a, stream, code):
    """400 with the code, nothing registered; the band as it was."""
    h, w = a.shape
    image = next(_ids)
    spec = dict(image_id=image, z=0, c=0, t=0, pixel_type=ptype(a), size_x=w, size_y=h, big_endian=False, seg_w=w, seg_h=h,
                tiled=False, compression=pbx.TIFF_J2K, predictor=1, j2k=True, flags=FLAG, segments=pbx.pack_chunks([stream]))
    with pytest.raises(pbx.PbxError, match=r"corrupt segment stream 0 \(j2k, decoder code %d\)" % code) as e:
        service.register_tiff_planes([spec])
    assert e.value.status == 400
    assert service.lookup_plane(image, 0, 0, 0) is None
    pid = service.create_sparse_plane(image, 0, 0, 0, ptype(a), w, h, h, big_endian=False)
    try:
        with pytest.raises(pbx.PbxError, match=r"corrupt segment stream 0 \(j2k, decoder code %d\)" % code) as e:
            service.band_write_tiff(pid, 0, h, w, h, False, pbx.TIFF_J2K, 1, spec["segments"], j2k=True, flags=FLAG)
        assert e.value.status == 400
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT]
    finally:
        service.release_plane(pid)


def test_device_refusals(service):
    a, s = K.device_case()
    hdr_cut, data_cut = K.layer2_cuts(s)
    refused(service, a, s[:hdr_cut], 1)   # cut inside a layer-2 packet header
    refused(service, a, s[:data_cut], 1)  # cut inside gathered data
    refused(service, a, K.passes_overflow_in_the_sum(s), 3)
    n = len(K.walk(s)[3])
    refused(service, a, K.insert_sop_eph(s, False, True, skip_eph_of=n // 2), 2)


def test_flipped_bits(service):
    """The first 8 of the 200 seeded flips tests/test_tiff_j2k_packets_host.py classifies: the GPU
    answers each as the CPU hook does, refusal code or bytes."""
    a, s = K.flip_case()
    h, w = a.shape
    for bad in K.flipped(s, 200, 11)[:8]:
        rc, msg, want = K.cpu_decode(*K.one(bad, a), np.uint16, 1)
        if rc:
            refused(service, a, bad, int(msg[-2]))
            continue
        image = next(_ids)
        spec = dict(image_id=image, z=0, c=0, t=0, pixel_type=pbx.UINT16, size_x=w, size_y=h, big_endian=False, seg_w=w,
                    seg_h=h, tiled=False, compression=pbx.TIFF_J2K, predictor=1, j2k=True, flags=FLAG,
                    segments=pbx.pack_chunks([bad]))
        (pid,) = service.register_tiff_planes([spec])
        try:
            got = np.frombuffer(service.read_plane_be(pid, want[0].nbytes), np.dtype(">u2")).reshape(h, w)
            assert np.array_equal(got, want[0])
        finally:
            service.release_plane(pid)


def test_without_the_flag_nothing_changes(service):
    a, s = K.device_case()
    image = next(_ids)
    spec = dict(image_id=image, z=0, c=0, t=0, pixel_type=pbx.UINT16, size_x=W0, size_y=H0, big_endian=False, seg_w=W0,
                seg_h=H0, tiled=False, compression=pbx.TIFF_J2K, predictor=1, j2k=True, segments=pbx.pack_chunks([s]))
    with pytest.raises(pbx.PbxError, match=r"segment 0: 3 quality layers \(1\)"):
        service.register_tiff_planes([spec])
    with pytest.raises(pbx.PbxError, match="bad flags 0x2"):
        service.register_tiff_planes([dict(spec, flags=2)])
    with pytest.raises(pbx.PbxError, match="bad flags 0x1"):  # the flag is the JPEG 2000 calls' alone
        service.register_tiff_planes([dict(spec, j2k=False, compression=8, flags=1)])
    assert service.lookup_plane(image, 0, 0, 0) is None


# ------------------------------------------------------------------------------ files
def expected(entry, key):
    npy, index, digest = entry["planes"]["0"][key]
    a = np.load(os.path.join(GOLD, npy))
    a = np.ascontiguousarray(a[:, :, index[0]] if index else a)
    assert hashlib.sha256(J.be_bytes(a)).hexdigest() == digest, (entry["file"], key)
    return a


@pytest.mark.parametrize("entry", FILES, ids=[f["file"] for f in FILES])
def test_fixture_registered_whole(service, entry):
    """register_tiff_image takes layered, multi-precinct files by default."""
    assert entry["layers"] > 1 and entry["scod"] & 1
    ids = service.register_tiff_image(os.path.join(GOLD, entry["file"]), next(_ids))
    try:
        assert sorted("%d,%d,%d" % p for p in ids[0]) == sorted(entry["planes"]["0"])
        for (z, c, t), pid in ids[0].items():
            want = expected(entry, "%d,%d,%d" % (z, c, t))
            got = np.frombuffer(service.read_plane_be(pid, want.nbytes), want.dtype.newbyteorder(">")).reshape(want.shape)
            assert np.array_equal(got, want), (entry["file"], c)
    finally:
        for pid in ids[0].values():
            service.release_plane(pid)
    with pytest.raises(pbx.PbxError, match="quality layers \\(1\\)|SOP or EPH markers"):
        service.register_tiff_image(os.path.join(GOLD, entry["file"]), next(_ids), j2k_packets=False)


def test_tiff_source_serves_a_png_tile(oracle):
    entry = next(e for e in FILES if e["file"].startswith("gray16_tiles32"))
    path = os.path.join(GOLD, entry["file"])
    want = expected(entry, "0,0,0")
    with pbx.PixelsService(sparse_band_rows=16) as svc:
        src = pbx.TiffSource({74: path})
        png = pbx.TileRequestHandler(svc, pbx.TileCtx(74, 0, 0, 0, 8, 20, 40, 10, format="png"), src).get_tile()
        r, px, _ = oracle.png_decode(png)
        assert r == 0
        assert np.array_equal(np.frombuffer(px, np.dtype(">u2")).reshape(10, 40), want[20:30, 8:48])
        # rows 20 .. 29 lie in band 1 of 16 rows alone
        states = svc.band_info(svc.lookup_plane(74, 0, 0, 0)[0])[1]
        assert [s == pbx.BS_READY for s in states] == [False, True, False, False, False], states
