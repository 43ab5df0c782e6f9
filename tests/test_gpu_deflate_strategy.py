"""The deflate strategies on the GPU (pbx_set_deflate_strategy: DEFAULT / HUFFMAN_ONLY / AUTO,
k_lz77's three instantiations) against the CPU emulator (csrc/emu.cpp
pbxemu_deflate_strategy / pbxemu_lz77_strategy): per segment the symbol histogram, the match
records and the mode (pbx_batch_lz_modes), end to end the zlib payload byte for byte, the
decoded pixels and the chunk CRCs -- through every source path of k_lz77's fill (direct plane
rows, staged rows, row-filtered streams, deflate-TIFF, tiled deflate-TIFF, unaligned columns,
the sparse planes' bridge buffer), at the smallest shapes, in a batch of more than 256 Huffman
blocks, and with the strategy captured when a batch is planned."""
import itertools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import _emu
import _emu_strategy as ES
import pbx

pytestmark = pytest.mark.gpu

_ids = itertools.count(9_300_000)
STRATS = [pbx.DEFLATE_DEFAULT, pbx.DEFLATE_HUFFMAN_ONLY, pbx.DEFLATE_AUTO]
PT = {1: pbx.UINT8, 2: pbx.UINT16}


@pytest.fixture(scope="module")
def svc():
    """This module's own context: the tests set its strategy (the session's shared service
    keeps the default)."""
    s = pbx.PixelsService()
    yield s
    s.close()


def _records(m, nw, wv):
    n = int(m[wv])
    return [(int(m[nw + wv * 256 + j]) & 0xFFFF, (int(m[nw + wv * 256 + j]) >> 16) + 3,
             int(m[nw + nw * 256 + wv * 256 + j]) + 1) for j in range(n)]


def _png_chunks_ok(body):
    o = 8
    while o < len(body):  # every chunk: length, type, data, CRC-32 of type + data
        n = int.from_bytes(body[o:o + 4], "big")
        assert zlib.crc32(body[o + 4:o + 8 + n]) == int.from_bytes(body[o + 8 + n:o + 12 + n], "big"), body[o + 4:o + 8]
        o += 12 + n
    assert o == len(body) and body[-8:-4] == b"IEND"


def _check_png(oracle, body, stream, rowlen, strategy, pixels_be, tag):
    z = ES.deflate(stream, rowlen, strategy)
    assert body[99:99 + len(z)] == z, tag
    assert len(body) == 99 + len(z) + 16, tag  # IDAT CRC and IEND follow the zlib stream
    assert zlib.decompress(z) == stream, tag
    r, px, _ = oracle.png_decode(body)
    assert r == 0 and px == pixels_be, tag
    _png_chunks_ok(body)


def _modes_each(service, ctxs):
    """The segment modes of every request, each planned and launched as a batch of its own (a
    batch orders its segments by the kernel group of their tiles, not by request)."""
    out = []
    for c in ctxs:
        b = pbx.Batch(service, [c])
        b.launch()
        b.sync()
        out.append(b.lz_modes().tolist())
        b.close()
    return out


def _register(service, a, little_endian):
    """a: 2-D uint8 / uint16 pixels; returns (image id, pixel type, big-endian pixel bytes)."""
    iid = next(_ids)
    h, w = a.shape
    pt = PT[a.dtype.itemsize]
    be = a.astype(a.dtype.newbyteorder(">"))
    data = a.astype(a.dtype.newbyteorder("<")) if little_endian else be
    service.register_plane(iid, 0, 0, 0, pt, w, h, data=data, big_endian=not little_endian)
    return iid, pt, be


@pytest.fixture(scope="module")
def stage_cases():
    """(name, pixels, little-endian plane): test_gpu_lz77.py's shapes (96 x 700 big-endian
    planes, 80 x 512 little-endian 16-bit ones: the headline's byte-swapping fast fill), a mixed
    tile whose top rows are noise and bottom rows constant (Huffman-only and parsed segments in
    one Huffman block under AUTO), and the pair either side of AUTO's threshold."""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:96, 0:700]
    out = [("noise16", rng.integers(0, 4096, (96, 700)).astype(np.uint16), False),
           ("runs8", ((xx // 37) % 3 * 50 + (yy // 11) % 2).astype(np.uint8), False),
           ("period3", (xx % 3 * 7 + (rng.random((96, 700)) < 0.05)).astype(np.uint8), False)]
    rows = np.tile(rng.integers(0, 65536, (1, 700)), (96, 1)).astype(np.uint16)
    rows[::7] = rng.integers(0, 65536, (14, 700))
    out.append(("rowrep16", rows, False))
    out.append(("noise512", rng.integers(0, 4096, (80, 512)).astype(np.uint16), True))
    rep = np.repeat(rng.integers(0, 65536, (10, 512)), 8, axis=0).astype(np.uint16)
    rep[5::13] = rng.integers(0, 65536, (len(rep[5::13]), 512))
    out.append(("rowrep512", rep, True))
    out.append(("zeros512", np.zeros((80, 512), np.uint16), True))
    mixed = rng.integers(0, 4096, (80, 512)).astype(np.uint16)
    mixed[44:] = 0x0123
    out.append(("mixed512", mixed, True))
    for want, a, _ in ES.threshold_pair():
        out.append(("threshold%d" % want, a, False))
    return out


@pytest.mark.parametrize("strategy", STRATS)
@pytest.mark.parametrize("case", range(10))
def test_stage_parity_and_end_to_end(svc, oracle, stage_cases, case, strategy):
    name, a, le = stage_cases[case]
    h, w = a.shape
    bpp = a.dtype.itemsize
    iid, pt, be = _register(svc, a, le)
    svc.set_deflate_strategy(strategy)
    b = pbx.Batch(svc, [pbx.TileCtx(iid, 0, 0, 0, 0, 0, w, h, format="png")])
    b.launch()
    b.sync()
    nseg = b.stats().segments
    L = _emu.lib()
    gh, gm = b.lz77_records(nseg, L.pbxemu_hist_words(), L.pbxemu_mrec_words())
    gmodes = b.lz_modes()
    (st, body), = b.fetch()
    b.close()
    svc.release_image(iid)
    stream = ES.png_stream(a)
    rowlen = 1 + w * bpp
    eh, em, emodes = ES.lz77(stream, rowlen, strategy)
    assert gh.shape == eh.shape and gmodes.tolist() == emodes.tolist(), (name, gmodes, emodes)
    nw = L.pbxemu_threads() // 64
    for k in range(nseg):
        for wv in range(nw):
            g, e = _records(gm[k], nw, wv), _records(em[k], nw, wv)
            assert g == e, (name, strategy, k, wv, [x for x in g if x not in e][:4], [x for x in e if x not in g][:4])
        assert (gh[k] == eh[k]).all(), (name, strategy, k, np.nonzero(gh[k] != eh[k])[0][:8])
    if strategy == pbx.DEFLATE_AUTO:
        if name == "mixed512":  # both kinds of segment in the tile's one Huffman block
            assert 0 < int(gmodes.sum()) < nseg and L.pbxemu_nblocks(len(stream)) == 1
        if name.startswith("threshold"):
            assert gmodes.tolist() == [1 if name == "threshold10" else 0]
    assert st == pbx.OK
    _check_png(oracle, body, stream, rowlen, strategy, be.tobytes(), (name, strategy))


def _mixed_plane(rng, h, w, dtype=np.uint16):
    """Blocks of 24 rows: noise, a constant, a ramp, noise with a zero right half."""
    a = rng.integers(0, 4096 if dtype == np.uint16 else 256, (h, w)).astype(dtype)
    for r0 in range(0, h, 24):
        k = (r0 // 24) % 4
        if k == 1:
            a[r0:r0 + 24] = 77
        elif k == 2:
            a[r0:r0 + 24] = np.arange(w).astype(dtype)
        elif k == 3:
            a[r0:r0 + 24, w // 2:] = 0
    return a


@pytest.mark.parametrize("strategy", STRATS)
def test_staged_rows_and_unaligned_columns(oracle, strategy):
    """stage_rows=True (k_rows writes the stream k_lz77 loads), and on the default service a
    region whose first column is not 16-byte aligned (the staged row kernel, not the direct
    fill)."""
    rng = np.random.default_rng(21)
    a = _mixed_plane(rng, 120, 600)
    for staged in (True, False):
        with pbx.PixelsService(stage_rows=staged, deflate_strategy=strategy) as s:
            assert s.deflate_strategy == strategy
            iid, pt, be = _register(s, a, True)
            regs = [(0, 0, 512, 100), (0, 10, 600, 110)] if staged else [(3, 1, 509, 99), (5, 30, 64, 70), (1, 0, 599, 120)]
            res = s.get_tiles([pbx.TileCtx(iid, 0, 0, 0, x, y, w, h, format="png") for x, y, w, h in regs])
            for (x, y, w, h), (st, body) in zip(regs, res):
                assert st == pbx.OK
                sub = a[y:y + h, x:x + w]
                _check_png(oracle, body, ES.png_stream(sub), 1 + 2 * w, strategy,
                           sub.astype(">u2").tobytes(), (staged, x, y, w, h, strategy))


@pytest.mark.parametrize("strategy", STRATS)
@pytest.mark.parametrize("filt", [1, 4, 5])
def test_row_filtered_streams(oracle, filt, strategy):
    """png_filter Sub / Paeth / adaptive: k_lz77 loads the filtered stream from the arena and
    AUTO's sample sees those bytes (the emulator runs on the oracle's filtered scanlines)."""
    rng = np.random.default_rng(30 + filt)
    planes = [_mixed_plane(rng, 96, 512), rng.poisson(40.0, (96, 300)).astype(np.uint16),
              _mixed_plane(rng, 96, 333, np.uint8)]
    with pbx.PixelsService(png_filter=filt, deflate_strategy=strategy) as s:
        ctxs, want = [], []
        for a in planes:
            iid, pt, be = _register(s, a, a.dtype.itemsize == 2)
            h, w = a.shape
            for y0, hh in ((0, 96), (20, 50)):
                ctxs.append(pbx.TileCtx(iid, 0, 0, 0, 0, y0, w, hh, format="png"))
                tile_be = np.frombuffer(be[y0:y0 + hh].tobytes(), np.uint8)
                stream = oracle.png_filter_stream(tile_be, pt, w, hh, filt).tobytes()
                want.append((stream, 1 + w * a.dtype.itemsize, tile_be.tobytes()))
        res = s.get_tiles(ctxs)
        gmodes = _modes_each(s, ctxs)
        for i, ((st, body), (stream, rowlen, px)) in enumerate(zip(res, want)):
            assert st == pbx.OK
            _check_png(oracle, body, stream, rowlen, strategy, px, (filt, strategy, i))
            assert gmodes[i] == ES.lz77(stream, rowlen, strategy)[2].tolist(), (filt, strategy, i)


@pytest.mark.parametrize("strategy", STRATS)
def test_deflate_tiff_every_pixel_type(oracle, strategy):
    """Deflate-TIFF strips (the tile's big-endian rows, no filter byte) of all 8 pixel types,
    from the noise and the ramp generator's pixels."""
    sx, sy = 300, 90
    with pbx.PixelsService(tiff_deflate=True, deflate_strategy=strategy) as s:
        ctxs, want = [], []
        for pt, kind in itertools.product(range(8), (1, 2)):
            iid = next(_ids)
            plane = oracle.gen_region(kind, pt, 0, 0, sx, sy, big_endian=True)
            s.register_plane(iid, 0, 0, 0, pt, sx, sy, data=plane, big_endian=True)
            x, y, w, h = (16, 3, 256, 80) if kind == 1 else (0, 0, sx, sy)
            ctxs.append(pbx.TileCtx(iid, 0, 0, 0, x, y, w, h, format="tif"))
            bpp = oracle.BPP[pt]
            want.append((oracle.extract_be(plane, True, pt, sx * bpp, x, y, w, h).tobytes(), w * bpp))
        res = s.get_tiles(ctxs)
        for i, ((st, body), (tile, rowlen)) in enumerate(zip(res, want)):
            assert st == pbx.OK
            z = ES.deflate(tile, rowlen, strategy)
            assert body[160:] == z, (strategy, i)
            r, px, meta = oracle.tiff_decode(body, len(tile))
            assert r == 0 and meta["compression"] == 8 and px == tile, (strategy, i)


def _tile_table(body):
    """(TileOffsets, TileByteCounts) of a big-endian tiled TIFF."""
    ifd = int.from_bytes(body[4:8], "big")
    tags = {}
    for k in range(int.from_bytes(body[ifd:ifd + 2], "big")):
        e = body[ifd + 2 + 12 * k: ifd + 14 + 12 * k]
        tags[int.from_bytes(e[0:2], "big")] = (int.from_bytes(e[4:8], "big"), int.from_bytes(e[8:12], "big"))
    n, o = tags[324]
    c = tags[325][1]
    if n == 1:
        return [o], [c]
    return ([int.from_bytes(body[o + 4 * k: o + 4 * k + 4], "big") for k in range(n)],
            [int.from_bytes(body[c + 4 * k: c + 4 * k + 4], "big") for k in range(n)])


@pytest.mark.parametrize("strategy", STRATS)
def test_tiled_deflate_tiff(oracle, strategy):
    """tiff_tile = 64 on a 100 x 70 region: four sub-tiles, the edge ones zero-padded; each is
    the emulator's stream of its padded rows, and the oracle's TIFF decoder gives the region."""
    T = 64
    rng = np.random.default_rng(41)
    a = _mixed_plane(rng, 100, 140)
    with pbx.PixelsService(tiff_tile=T, tiff_deflate=True, deflate_strategy=strategy) as s:
        iid, pt, be = _register(s, a, True)
        x, y, w, h = 8, 20, 100, 70
        (st, body), = s.get_tiles([pbx.TileCtx(iid, 0, 0, 0, x, y, w, h, format="tif")])
        assert st == pbx.OK
        sub = a[y:y + h, x:x + w]
        r, px, meta = oracle.tiff_decode(body, w * h * 2)
        assert r == 0 and meta["compression"] == 8 and px == sub.astype(">u2").tobytes()
        offs, cnts = _tile_table(body)
        assert len(offs) == 4
        for k, (o, c) in enumerate(zip(offs, cnts)):
            ty, tx = divmod(k, 2)
            pad = np.zeros((T, T), np.uint16)
            part = sub[ty * T:(ty + 1) * T, tx * T:(tx + 1) * T]
            pad[:part.shape[0], :part.shape[1]] = part
            assert body[o:o + c] == ES.deflate(pad.astype(">u2").tobytes(), T * 2, strategy), (strategy, k)


@pytest.mark.parametrize("strategy", STRATS)
def test_sparse_plane_region_across_two_bands(oracle, strategy):
    """A region straddling two bands of a sparse plane is gathered into the batch's bridge
    buffer: k_lz77 fills from there."""
    sx, sy, B = 512, 128, 64
    rng = np.random.default_rng(51)
    a = _mixed_plane(rng, sy, sx)
    with pbx.PixelsService(deflate_strategy=strategy) as s:
        iid = next(_ids)
        pid = s.create_sparse_plane(iid, 0, 0, 0, pbx.UINT16, sx, sy, B, big_endian=True)
        for k in range(2):
            s.band_write(pid, k * B, B, a[k * B:(k + 1) * B].astype(">u2").tobytes())
        regs = [(0, 40, 512, 60), (7, 30, 300, 70)]
        res = s.get_tiles([pbx.TileCtx(iid, 0, 0, 0, x, y, w, h, format="png") for x, y, w, h in regs])
        for (x, y, w, h), (st, body) in zip(regs, res):
            assert st == pbx.OK
            sub = a[y:y + h, x:x + w]
            _check_png(oracle, body, ES.png_stream(sub), 1 + 2 * w, strategy, sub.astype(">u2").tobytes(),
                       (strategy, x, y, w, h))


@pytest.mark.parametrize("strategy", STRATS)
def test_smallest_shapes(svc, oracle, strategy):
    """Streams shorter than a sample (no sampled chunk: parsed), of one chunk, and a tile
    whose last segment ends in a partial chunk."""
    rng = np.random.default_rng(61)
    svc.set_deflate_strategy(strategy)
    ctxs, want, iids = [], [], []
    for bpp in (1, 2):
        dt = np.uint8 if bpp == 1 else np.uint16
        a = _mixed_plane(rng, 40, 1000, dt)
        a[:8] = 5  # runs in the small tiles' rows
        iid, pt, be = _register(svc, a, bpp == 2)
        iids.append(iid)
        # (1000, 2): one short segment; (1000, 33) of 16-bit samples: 66,033 bytes, four segments of
        # 13,216 and a last one of 13,169 bytes = 411 chunks and 17 bytes
        for w, h in ((1, 1), (2, 1), (3, 2), (33, 1), (16 // bpp, 5), (1000, 2), (1000, 33)):
            ctxs.append(pbx.TileCtx(iid, 0, 0, 0, 0, 0, w, h, format="png"))
            sub = a[:h, :w]
            want.append((ES.png_stream(sub), 1 + w * bpp, sub.astype(sub.dtype.newbyteorder(">")).tobytes()))
    assert (len(want[-1][0]) % 13216) % 32 == 17
    res = svc.get_tiles(ctxs)
    gmodes = _modes_each(svc, ctxs)
    for i, ((st, body), (stream, rowlen, px)) in enumerate(zip(res, want)):
        assert st == pbx.OK
        _check_png(oracle, body, stream, rowlen, strategy, px, (strategy, i, len(stream)))
        assert gmodes[i] == ES.lz77(stream, rowlen, strategy)[2].tolist(), (strategy, i)
    for iid in iids:
        svc.release_image(iid)


def test_auto_batch_of_320_tiles(svc, oracle):
    """More Huffman blocks than the small-batch k_huff takes (its batch form), tiles of mixed
    kinds and heights under AUTO: every payload equals the emulator's."""
    rng = np.random.default_rng(71)
    svc.set_deflate_strategy(pbx.DEFLATE_AUTO)
    ctxs, want, iids = [], [], []
    for w, bpp in ((300, 2), (256, 2), (700, 1), (100, 1)):
        hs = [int(rng.integers(3, 60)) for _ in range(80)]
        a = _mixed_plane(rng, sum(hs), w, np.uint8 if bpp == 1 else np.uint16)
        iid, pt, be = _register(svc, a, bpp == 2)
        iids.append(iid)
        y = 0
        for h in hs:
            ctxs.append(pbx.TileCtx(iid, 0, 0, 0, 0, y, w, h, format="png"))
            sub = a[y:y + h]
            want.append((ES.png_stream(sub), 1 + w * bpp, sub.astype(sub.dtype.newbyteorder(">")).tobytes()))
            y += h
    assert len(ctxs) == 320
    b = pbx.Batch(svc, ctxs)
    b.launch()
    b.sync()
    assert b.stats().blocks > 256
    gmodes = b.lz_modes()
    res = b.fetch()
    b.close()
    assert 0 < int(gmodes.sum()) < len(gmodes)  # both kinds of segment in the batch
    emodes = []
    for i, ((st, body), (stream, rowlen, px)) in enumerate(zip(res, want)):
        assert st == pbx.OK
        _check_png(oracle, body, stream, rowlen, pbx.DEFLATE_AUTO, px, i)
        emodes += ES.lz77(stream, rowlen, pbx.DEFLATE_AUTO)[2].tolist()
    assert gmodes.tolist() == emodes
    for iid in iids:
        svc.release_image(iid)


def test_strategy_is_captured_when_the_batch_is_planned(svc, oracle):
    rng = np.random.default_rng(81)
    a = rng.poisson(3.0, (128, 512)).astype(np.uint8)  # DEFAULT keeps matches AUTO's sample declines
    stream, rowlen = ES.png_stream(a), 513
    z_def, z_auto = ES.deflate(stream, rowlen, pbx.DEFLATE_DEFAULT), ES.deflate(stream, rowlen, pbx.DEFLATE_AUTO)
    assert z_def != z_auto
    iid, pt, be = _register(svc, a, False)
    tc = [pbx.TileCtx(iid, 0, 0, 0, 0, 0, 512, 128, format="png")]
    svc.set_deflate_strategy(pbx.DEFLATE_AUTO)
    b = pbx.Batch(svc, tc)                      # planned under AUTO
    svc.set_deflate_strategy(pbx.DEFLATE_DEFAULT)
    assert svc.deflate_strategy == pbx.DEFLATE_DEFAULT
    b.launch()
    b.sync()
    (st, body), = b.fetch()
    modes = b.lz_modes()
    b.close()
    assert st == pbx.OK and body[99:99 + len(z_auto)] == z_auto and modes.all()
    # a DEFAULT batch on the same context afterwards: a fresh context's bytes
    (st, again), = svc.get_tiles(tc)
    with pbx.PixelsService() as fresh:
        assert fresh.deflate_strategy == pbx.DEFLATE_DEFAULT
        fresh.register_plane(iid, 0, 0, 0, pt, 512, 128, data=a, big_endian=True)
        (st2, ref), = fresh.get_tiles(tc)
    assert st == st2 == pbx.OK and again == ref and again[99:99 + len(z_def)] == z_def
    # out of range: 400, the value stays
    for bad in (-1, 3, 99):
        with pytest.raises(pbx.PbxError) as e:
            svc.set_deflate_strategy(bad)
        assert e.value.status == pbx.E_BADARG
    assert svc.deflate_strategy == pbx.DEFLATE_DEFAULT
    # lz_modes before the launch, or with a wrong segment count: 400
    b2 = pbx.Batch(svc, tc)
    with pytest.raises(pbx.PbxError) as e:
        pbx._check(pbx.lib().pbx_batch_lz_modes(svc.handle, b2._h, None, 5, None))
    assert e.value.status == pbx.E_BADARG
    b2.launch()
    b2.sync()
    with pytest.raises(pbx.PbxError) as e:
        pbx._check(pbx.lib().pbx_batch_lz_modes(svc.handle, b2._h, None, 10 ** 6, None))
    assert e.value.status == pbx.E_BADARG
    assert not b2.lz_modes().any()
    b2.close()
    svc.release_image(iid)


def test_environment_sets_the_initial_strategy():
    """$PBX_DEFLATE_STRATEGY in a fresh child process (one at a time)."""
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(pbx.__file__)))
    code = ("import sys; sys.path.insert(0, %r); import pbx\n"
            "with pbx.PixelsService() as s: print('strategy', s.deflate_strategy)\n" % pkg)
    env = dict(os.environ, PBX_DEFLATE_STRATEGY="2")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "strategy 2" in out.stdout, (out.stdout, out.stderr)
