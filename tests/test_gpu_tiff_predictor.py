"""TIFF Predictor = 2 on the GPU (pbx_set_tiff_predictor; k_tiff_pred3 and k_tiff_pred,
csrc/kernels_tiff_predictor.hip) against the numpy restatement of tests/_tiff_pred.py.

The oracle's TIFF decoder ignores tag 317, so the tests read StripOffsets / TileOffsets
themselves, inflate every strip or sub-tile with zlib and compare the inflated bytes, whole,
with the restated stream of the oracle's tile; the inverse of those bytes must be the tile.
Planes are host uploads of full-range seeded values (tests/_values.py): low bytes borrow.
pbx_batch_pred_tiles shows which of the two kernels a shape reached."""
import ctypes
import hashlib
import itertools
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import _emu
import _tiff_pred as TP
import _values as V
import pbx

pytestmark = pytest.mark.gpu

_ids = itertools.count(9_700_000)
BPP = TP.BPP
INT_TYPES = list(range(6))
HORIZONTAL = pbx.TIFF_PREDICTOR_HORIZONTAL


@pytest.fixture(scope="module")
def on():
    s = pbx.PixelsService(tiff_deflate=True, tiff_predictor=HORIZONTAL)
    yield s
    s.close()


@pytest.fixture(scope="module")
def off():
    s = pbx.PixelsService(tiff_deflate=True)
    yield s
    s.close()


@pytest.fixture(scope="module")
def run_rows():
    L = _emu.lib()
    L.pbxemu_tiff_pred_run_rows.restype = ctypes.c_uint32
    return int(L.pbxemu_tiff_pred_run_rows())


def _register(svc, plane, pt, big_endian):
    iid = next(_ids)
    sy, sx = plane.shape
    svc.register_plane(iid, 0, 0, 0, pt, sx, sy, data=plane if big_endian else V.le(plane), big_endian=big_endian)
    return iid


def _tile(oracle, plane, pt, big_endian, reg):
    """The oracle's big-endian tile of the plane as it was uploaded."""
    sy, sx = plane.shape
    data = plane if big_endian else V.le(plane)
    return oracle.extract_be(data, big_endian, pt, sx * BPP[pt], *reg).tobytes()


def _tif(iid, reg):
    return pbx.TileCtx(iid, 0, 0, 0, *reg, format="tif")


def _routing(svc, ctxs):
    b = pbx.Batch(svc, ctxs)
    try:
        return b.pred_tiles()
    finally:
        b.close()


def _check_strip(body, tile, w, h, bpp, tag):
    parts, tags, order = TP.pieces(body)
    assert order == sorted(order) and len(order) == 12, tag
    assert tags[TP.TAG_PREDICTOR] == (3, 1, 2), tag
    assert (tags[256][2], tags[257][2], tags[258][2], tags[273][2]) == (w, h, 8 * bpp, 160), tag
    assert tags[279][2] == len(body) - 160 and len(parts) == 1, tag
    got = parts[0]
    assert len(got) == len(tile), tag
    want = TP.forward(tile, w, h, bpp)
    if got != want:
        bad = next(i for i in range(len(got)) if got[i] != want[i])
        raise AssertionError((tag, "first differing stream byte", bad, "row", bad // (w * bpp), "col", bad % (w * bpp)))
    assert TP.inverse(got, w, h, bpp) == tile, tag


def _fast_ok(reg, bpp):
    x, _, w, _ = reg
    return (x * bpp) % 16 == 0 and (w * bpp) % 16 == 0 and w * bpp <= 2048


# ------------------------------------------------------------------ types, byte orders and x

@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("pt", INT_TYPES)
def test_types_byte_orders_and_x(on, oracle, pt, big_endian):
    """Aligned rows at x = 0 and at x > 0 (a first sample differenced against the plane's x - 1
    would show there), unaligned x, and rows that are no whole chunks at x = 0 and x > 0."""
    bpp = BPP[pt]
    plane = V.random_bits(pt, 200, 24, 11)
    iid = _register(on, plane, pt, big_endian)
    regs = [(0, 1, 64, 10), (16, 2, 64, 11), (32, 0, 128, 9), (3, 1, 64, 10), (0, 0, 61, 10), (5, 3, 61, 9)]
    ctxs = [_tif(iid, r) for r in regs]
    nfast = sum(_fast_ok(r, bpp) for r in regs)
    assert nfast == 3 and _routing(on, ctxs) == (nfast, len(regs) - nfast)
    for r, (st, body) in zip(regs, on.get_tiles(ctxs)):
        assert st == pbx.OK
        _check_strip(body, _tile(oracle, plane, pt, big_endian, r), r[2], r[3], bpp, (pt, big_endian, r))
    on.release_image(iid)


# ----------------------------------------------------------------------------------- widths

@pytest.mark.parametrize("pt,big_endian", [(pbx.UINT8, True), (pbx.INT16, False), (pbx.UINT16, True),
                                           (pbx.UINT32, False), (pbx.INT32, True)])
def test_row_widths(on, oracle, run_rows, pt, big_endian):
    """1, 2, 3 samples; rows of 15, 16, 17 bytes; 1024 bytes (64 chunks), 1040 (65: lane 63's
    tail carried into lane 0), 2048, and 2064 (past the fast kernel) -- at x = 0 and x = 16."""
    bpp = BPP[pt]
    rbs = [bpp, 2 * bpp, 3 * bpp, 16, 1024, 1040, 2048, 2064] + ([15, 17] if bpp == 1 else [16 - bpp, 16 + bpp])
    h = run_rows + 1
    plane = V.random_bits(pt, 2064 // bpp + 24, h + 2, 12)
    iid = _register(on, plane, pt, big_endian)
    regs = [(x, 1, rb // bpp, h) for rb in rbs for x in (0, 16)]
    ctxs = [_tif(iid, r) for r in regs]
    nfast = sum(_fast_ok(r, bpp) for r in regs)
    assert nfast == 8 and _routing(on, ctxs) == (nfast, len(regs) - nfast)
    for r, (st, body) in zip(regs, on.get_tiles(ctxs)):
        assert st == pbx.OK
        _check_strip(body, _tile(oracle, plane, pt, big_endian, r), r[2], r[3], bpp, (pt, big_endian, r))
    on.release_image(iid)


def test_rows_of_large_and_oversized_bands(on, oracle):
    """Rows of 6,002 and 8,192 bytes: the general kernel's LDS band over 64 KiB (up to its
    widest).  Rows over 8 KiB do not fit it: the kernel's plane-reading branch."""
    pt, bpp = pbx.UINT16, 2
    plane = V.random_bits(pt, 4200, 19, 13)
    iid = _register(on, plane, pt, False)
    regs = [(1, 0, 3001, 17), (3, 2, 4096, 16), (0, 0, 4104, 17), (3, 1, 4197, 18)]
    ctxs = [_tif(iid, r) for r in regs]
    assert _routing(on, ctxs) == (0, 4)
    for r, (st, body) in zip(regs, on.get_tiles(ctxs)):
        assert st == pbx.OK
        _check_strip(body, _tile(oracle, plane, pt, False, r), r[2], r[3], bpp, r)
    on.release_image(iid)


# ---------------------------------------------------------------------------------- heights

@pytest.mark.parametrize("pt,big_endian", [(pbx.UINT8, True), (pbx.UINT16, False), (pbx.INT32, True)])
def test_heights_around_a_run_and_a_band(on, oracle, run_rows, pt, big_endian):
    """One row; the fast kernel's run length - 1, exact, + 1 and several runs (one and two
    chunk groups); the general kernel's band of 16 rows - 1, exact, + 1."""
    bpp = BPP[pt]
    hs = sorted({1, run_rows - 1, run_rows, run_rows + 1, 3 * run_rows + 2, 15, 16, 17, 33})
    plane = V.random_bits(pt, 1040 // bpp + 8, max(hs) + 1, 14)
    iid = _register(on, plane, pt, big_endian)
    regs = [(x, 1, w, h) for h in hs for x, w in ((0, 64 // bpp), (0, 1040 // bpp), (1, 72 // bpp + 1))]
    ctxs = [_tif(iid, r) for r in regs]
    assert _routing(on, ctxs) == (2 * len(hs), len(hs))
    for r, (st, body) in zip(regs, on.get_tiles(ctxs)):
        assert st == pbx.OK
        _check_strip(body, _tile(oracle, plane, pt, big_endian, r), r[2], r[3], bpp, (pt, r))
    on.release_image(iid)


# ---------------------------------------------------------------------------- kernel routing

_ALIGNED = [(pbx.UINT8, [(0, 0, 16, 3), (16, 1, 1040, 9), (32, 0, 2048, 17)]),
            (pbx.INT16, [(0, 0, 8, 1), (8, 1, 520, 9), (16, 2, 1024, 8)]),
            (pbx.UINT32, [(0, 0, 4, 7), (4, 1, 260, 10), (8, 0, 512, 16)])]


def _aligned_digest(svc, big_endian):
    """sha256 of every response of the aligned shapes (the fast kernel's, unless it is switched
    off), and the batch routing."""
    out, routing = [], [0, 0]
    for pt, regs in _ALIGNED:
        plane = V.random_bits(pt, 2100, 20, 15)
        iid = _register(svc, plane, pt, big_endian)
        ctxs = [_tif(iid, r) for r in regs]
        f, g = _routing(svc, ctxs)
        routing[0] += f
        routing[1] += g
        for st, body in svc.get_tiles(ctxs):
            assert st == pbx.OK
            out.append(hashlib.sha256(body).hexdigest())
        svc.release_image(iid)
    return routing, out


_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import pbx, test_gpu_tiff_predictor as T
with pbx.PixelsService(tiff_deflate=True) as s:
    print("predictor", s.tiff_predictor)
    for be in (True, False):
        routing, digests = T._aligned_digest(s, be)
        print("routing", routing[0], routing[1])
        print("digests", " ".join(digests))
"""


def test_fast_switched_off_gives_identical_responses(on, oracle):
    """$PBX_TIFF_PRED_FAST=0 (and $PBX_TIFF_PREDICTOR=2 as the initial value) in one fresh child
    process: every aligned shape through the general kernel, byte-identical responses."""
    here = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(pbx.__file__)))
    env = dict(os.environ, PBX_TIFF_PRED_FAST="0", PBX_TIFF_PREDICTOR="2")
    out = subprocess.run([sys.executable, "-c", _CHILD % (pkg, here)], env=env, capture_output=True, text=True,
                         timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    assert lines[0] == "predictor 2"
    for k, be in enumerate((True, False)):
        routing, digests = _aligned_digest(on, be)
        assert routing == [9, 0]
        assert lines[1 + 2 * k] == "routing 0 9"
        assert lines[2 + 2 * k].split()[1:] == digests, be
    # and the shapes themselves are right (the digests alone only say both kernels agree)
    pt, regs = _ALIGNED[0]
    plane = V.random_bits(pt, 2100, 20, 15)
    iid = _register(on, plane, pt, True)
    for r, (st, body) in zip(regs, on.get_tiles([_tif(iid, r) for r in regs])):
        _check_strip(body, _tile(oracle, plane, pt, True, r), r[2], r[3], 1, r)
    on.release_image(iid)


# ------------------------------------------------------------------------------- tiled TIFF

def _check_tiled(body, tile, w, h, bpp, T, tag):
    parts, tags, order = TP.pieces(body)
    ntx, nty = -(-w // T), -(-h // T)
    n = ntx * nty
    assert order == sorted(order) and len(order) == 13 and tags[TP.TAG_PREDICTOR] == (3, 1, 2), tag
    assert (tags[256][2], tags[257][2], tags[322][2], tags[323][2]) == (w, h, T, T), tag
    data = 176 if n == 1 else (176 + 8 * n + 15) // 16 * 16
    if n > 1:
        assert tags[324] == (4, n, 176) and tags[325] == (4, n, 176 + 4 * n), tag
    offs = TP._array(body, tags[324])
    cnts = TP._array(body, tags[325])
    assert offs[0] == data and offs[-1] + cnts[-1] == len(body), tag
    assert all(offs[k] + cnts[k] == offs[k + 1] for k in range(n - 1)), tag
    assert not any(body[176 + 8 * n:data]) if n > 1 else True, tag
    want = TP.forward_subtiles(tile, w, h, bpp, T)
    assert len(parts) == n == len(want), tag
    for k in range(n):
        assert parts[k] == want[k], (tag, "sub-tile", k)
        assert TP.inverse(parts[k], T, T, bpp) == TP.pad_subtile(tile, w, h, bpp, T, k % ntx, k // ntx), (tag, k)


@pytest.mark.parametrize("T", [16, 64])
def test_tiled_tiff_ragged_edges(oracle, T):
    """Regions of several sub-tiles with ragged right and bottom edges (unaligned and aligned x:
    the unpadded sub-tiles of the aligned ones take the fast kernel), one exact sub-tile, and
    float responses byte-identical to a predictor-off context's."""
    with pbx.PixelsService(tiff_deflate=True, tiff_tile=T, tiff_predictor=HORIZONTAL) as s, \
            pbx.PixelsService(tiff_deflate=True, tiff_tile=T) as ref:
        for pt, big_endian in ((pbx.UINT8, True), (pbx.UINT16, False), (pbx.INT32, True)):
            bpp = BPP[pt]
            plane = V.random_bits(pt, 3 * T + 40, 2 * T + 30, 16)
            iid = _register(s, plane, pt, big_endian)
            regs = [(5, 3, 2 * T + 8, 2 * T + 5), (16, 1, 2 * T + T // 2, T + 3), (32, 2, T, T), (7, 0, T - 1, 1)]
            ctxs = [_tif(iid, r) for r in regs]
            # aligned regions: (2 x 1 whole sub-tiles of 3 x 2) and the exact one take the fast kernel
            assert _routing(s, ctxs) == (3, 9 + 6 + 1 + 1 - 3), (T, pt)
            for r, (st, body) in zip(regs, s.get_tiles(ctxs)):
                assert st == pbx.OK
                _check_tiled(body, _tile(oracle, plane, pt, big_endian, r), r[2], r[3], bpp, T, (T, pt, r))
            s.release_image(iid)
        for pt in (pbx.FLOAT, pbx.DOUBLE):
            plane = V.random_bits(pt, 2 * T + 9, T + 7, 17)
            reg = (1, 2, 2 * T + 3, T + 4)
            got = []
            for svc in (s, ref):
                iid = _register(svc, plane, pt, True)
                assert _routing(svc, [_tif(iid, reg)]) == (0, 0)
                (st, body), = svc.get_tiles([_tif(iid, reg)])
                assert st == pbx.OK
                got.append(body)
                svc.release_image(iid)
            assert got[0] == got[1] and TP.TAG_PREDICTOR not in TP.ifd(got[0])[0], (T, pt)


# -------------------------------------------------------- what the setting leaves untouched

def test_float_and_double_strips_are_untouched(on, off, oracle):
    for pt, big_endian in itertools.product((pbx.FLOAT, pbx.DOUBLE), (True, False)):
        plane = V.random_bits(pt, 80, 20, 18)
        regs = [(0, 0, 64, 16), (3, 1, 61, 9)]
        got = []
        for svc in (on, off):
            iid = _register(svc, plane, pt, big_endian)
            ctxs = [_tif(iid, r) for r in regs]
            assert _routing(svc, ctxs) == (0, 0)
            got.append(svc.get_tiles(ctxs))
            svc.release_image(iid)
        assert got[0] == got[1] and all(st == pbx.OK for st, _ in got[0])
        for r, (st, body) in zip(regs, got[0]):
            parts, tags, order = TP.pieces(body)
            assert TP.TAG_PREDICTOR not in tags and len(order) == 11
            assert parts[0] == _tile(oracle, plane, pt, big_endian, r)


def test_predictor_without_tiff_deflate_is_the_reference_tiff(oracle):
    with pbx.PixelsService(tiff_predictor=HORIZONTAL) as s:
        assert s.tiff_predictor == HORIZONTAL
        for pt in (pbx.UINT8, pbx.INT16, pbx.UINT32):
            plane = V.random_bits(pt, 80, 20, 19)
            iid = _register(s, plane, pt, False)
            for reg in ((0, 0, 64, 16), (3, 1, 61, 9)):
                assert _routing(s, [_tif(iid, reg)]) == (0, 0)
                (st, body), = s.get_tiles([_tif(iid, reg)])
                tile = _tile(oracle, plane, pt, False, reg)
                rst, ref = oracle.tiff_encode(np.frombuffer(tile, np.uint8), pt, reg[2], reg[3])
                assert st == pbx.OK and rst == 0 and body == ref
            s.release_image(iid)


def test_mixed_batch(on, off, oracle):
    """PNG, raw, float TIFF and predictor TIFF (both kernels) in one batch: the first three are
    a predictor-off context's bytes."""
    p16, pf = V.random_bits(pbx.UINT16, 300, 40, 20), V.random_bits(pbx.FLOAT, 100, 20, 21)
    reqs = [("png", 0, (0, 0, 256, 32)), ("png", 0, (3, 1, 100, 7)), (None, 0, (5, 2, 77, 9)), ("tif", 1, (0, 0, 64, 16)),
            ("tif", 0, (8, 1, 256, 33)), ("tif", 0, (3, 2, 99, 17)), (None, 1, (0, 0, 100, 20)), ("tif", 0, (0, 0, 8, 1))]
    got = []
    for svc in (on, off):
        ids = [_register(svc, p16, pbx.UINT16, False), _register(svc, pf, pbx.FLOAT, True)]
        ctxs = [pbx.TileCtx(ids[k], 0, 0, 0, *r, format=f) for f, k, r in reqs]
        if svc is on:
            assert _routing(svc, ctxs) == (2, 1)
        got.append(svc.get_tiles(ctxs))
        for i in ids:
            svc.release_image(i)
    for k, (f, which, r) in enumerate(reqs):
        assert got[0][k][0] == got[1][k][0] == pbx.OK
        if f == "tif" and which == 0:
            assert got[0][k][1] != got[1][k][1]
            _check_strip(got[0][k][1], _tile(oracle, p16, pbx.UINT16, False, r), r[2], r[3], 2, r)
        else:
            assert got[0][k][1] == got[1][k][1], (k, f)


# ---------------------------------------------------------------------------- serving paths

def test_serving_paths(oracle):
    """A lone pbx_get_tile (the single-request framing), pbx_submit / pbx_wait, a sparse-plane
    region that straddles two bands (the bridge buffer), and 32 concurrent callers."""
    pt, bpp = pbx.UINT16, 2
    plane = V.random_bits(pt, 520, 128, 22)
    regs = [(0, 0, 512, 64), (8, 40, 256, 60), (7, 30, 300, 70), (0, 60, 8, 9), (513, 3, 7, 125)]
    with pbx.PixelsService(tiff_deflate=True, tiff_predictor=HORIZONTAL) as s:
        iid = _register(s, plane, pt, False)
        for r in regs:  # one request at a time
            st, body = s.get_tile(_tif(iid, r))
            assert st == pbx.OK
            _check_strip(body, _tile(oracle, plane, pt, False, r), r[2], r[3], bpp, ("lone", r))
        res = s.submit([_tif(iid, r) for r in regs]).wait()
        for r, (st, body) in zip(regs, res):
            assert st == pbx.OK
            _check_strip(body, _tile(oracle, plane, pt, False, r), r[2], r[3], bpp, ("submit", r))
        # sparse plane of two bands of 64 rows, big-endian: regions 2 and 3 of `regs` straddle them
        sid = next(_ids)
        pid = s.create_sparse_plane(sid, 0, 0, 0, pt, 520, 128, 64, big_endian=True)
        for k in range(2):
            s.band_write(pid, 64 * k, 64, plane[64 * k:64 * (k + 1)].tobytes())
        ctxs = [_tif(sid, r) for r in regs]
        assert _routing(s, ctxs) == (3, 2)
        for r, (st, body) in zip(regs, s.get_tiles(ctxs)):
            assert st == pbx.OK
            _check_strip(body, _tile(oracle, plane, pt, True, r), r[2], r[3], bpp, ("sparse", r))
        # 32 callers at once (the coalescer's batches)
        out = [None] * 32

        def call(k):
            out[k] = s.get_tile(_tif(iid, regs[k % len(regs)]))
        ts = [threading.Thread(target=call, args=(k,)) for k in range(32)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for k in range(32):
            r = regs[k % len(regs)]
            assert out[k][0] == pbx.OK
            _check_strip(out[k][1], _tile(oracle, plane, pt, False, r), r[2], r[3], bpp, ("caller", k))


# ----------------------------------------------------------------------------- setter timing

def test_setting_is_captured_when_the_batch_is_planned(oracle):
    pt = pbx.UINT16
    plane = V.random_bits(pt, 64, 16, 23)
    reg = (0, 0, 64, 16)
    with pbx.PixelsService(tiff_deflate=True) as s, pbx.PixelsService(tiff_deflate=True) as fresh:
        assert s.tiff_predictor == pbx.TIFF_PREDICTOR_NONE
        iid = _register(s, plane, pt, True)
        tile = _tile(oracle, plane, pt, True, reg)
        (st, plain), = s.get_tiles([_tif(iid, reg)])
        fid = _register(fresh, plane, pt, True)
        assert plain == fresh.get_tiles([_tif(fid, reg)])[0][1]
        s.set_tiff_predictor(HORIZONTAL)
        b_on = pbx.Batch(s, [_tif(iid, reg)])      # planned with the predictor
        s.set_tiff_predictor(pbx.TIFF_PREDICTOR_NONE)
        b_off = pbx.Batch(s, [_tif(iid, reg)])     # planned without
        s.set_tiff_predictor(HORIZONTAL)
        assert s.tiff_predictor == HORIZONTAL
        assert b_on.pred_tiles() == (1, 0) and b_off.pred_tiles() == (0, 0)
        for b in (b_on, b_off):
            b.launch()
            b.sync()
        (st1, body_on), = b_on.fetch()
        (st2, body_off), = b_off.fetch()
        b_on.close()
        b_off.close()
        assert st1 == st2 == pbx.OK and body_off == plain
        _check_strip(body_on, tile, 64, 16, 2, "planned on")
        for bad in (0, 3, -1):  # out of range: 400, the value stays
            with pytest.raises(pbx.PbxError) as e:
                s.set_tiff_predictor(bad)
            assert e.value.status == pbx.E_BADARG
        assert s.tiff_predictor == HORIZONTAL


# --------------------------------------------------------------------------- bytes on the GPU

@pytest.mark.parametrize("kind", ["fake", "scene"])
def test_64_tiles_are_exact_and_smaller(on, off, oracle, kind):
    """64 tiles of 512 x 512 uint16 through the fast kernel: every tile exact, and fewer bytes in
    total than with the predictor off (tests/test_tiff_predictor.py established the inequality
    on the CPU first)."""
    pt, n = pbx.UINT16, 4096
    scene = TP.smooth_scene(n, n, 7).astype(">u2") if kind == "scene" else None
    regs = [(512 * i, 512 * j, 512, 512) for j in range(8) for i in range(8)]
    total = []
    for svc in (on, off):
        iid = next(_ids)
        if kind == "fake":
            svc.register_plane(iid, 0, 0, 0, pt, n, n, generator="fake")
        else:
            svc.register_plane(iid, 0, 0, 0, pt, n, n, data=scene, big_endian=True)
        ctxs = [_tif(iid, r) for r in regs]
        if svc is on:
            assert _routing(svc, ctxs) == (64, 0)
        res = svc.get_tiles(ctxs)
        svc.release_image(iid)
        assert all(st == pbx.OK for st, _ in res)
        total.append(sum(len(body) for _, body in res))
        if svc is on:
            for r, (_, body) in zip(regs, res):
                tile = (oracle.gen_region(1, pt, *r).tobytes() if kind == "fake"
                        else V.cut(scene, *r))
                _check_strip(body, tile, 512, 512, 2, (kind, r))
    print(kind, "predictor", total[0], "plain", total[1], "ratio %.3f" % (total[0] / total[1]))
    assert total[0] < total[1]
