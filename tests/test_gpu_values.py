"""GPU: the I/O kernels (csrc/kernels_io.hip) on full-range sample values (tests/_values.py).

The generators of the other GPU tests give small positive numbers or a ramp; here the planes
hold uniform random bits, every type's extremes, every Paeth triple and rows whose filter sums
tie.  References: the numpy restatement of the PNG stream written from the PNG specification
(_numpy_ref.png_stream) and the CPU oracle's stream; numpy slicing of the big-endian plane;
_numpy_ref.downsample (pinned to exact integer arithmetic by tests/test_values.py, which also
asserts that the planes and tiles requested here hold what they claim).

Which filter kernel takes a PNG tile is decided by its shape alone (runtime.cpp, the
filt2_ok / filt3_ok lines of the plan); rb = row bytes, x = the tile's first byte in its row:

  kernel                 takes
  k_filter3, G = 1       x % 16 == 0, rb % 16 == 0, 16 <= rb <= 2048, and the widest such row
                         of the batch <= 1024 B
  k_filter3, G = 2       the same, the widest such row of the batch > 1024 B (G is per batch:
                         the two are kept in separate get_tiles calls)
  k_filter2              x % 16 == 0, rb % 4 == 0, rb % 16 != 0, 16 <= rb <= 2048
  k_filter, from LDS     everything else while 17 * (round16(rb) + 16) + 256 <= 64 KiB
                         (rb <= 3,823)
  k_filter, from plane   everything else above that

k_adaptive_mode (the adaptive option's tile mode) stages its two rows in LDS unless the widest
adaptive row of the batch is above 16,368 B; then every tile of the batch is read from the
plane.

That the tests bite was shown with three one-line changes of kernels_io.hip, each built and
run once on an MI355X (272 cases here; the whole file takes 30 s, the slowest case 0.4 s):

  change                                    fails here                          older tests
  ds_mean4: (s + 2) / 4 for >> 2            test_pyramid_full_range, the 12     test_resolution_pyramid
                                            cases of int8 / int16 / int32       for int8 only (noise cast
                                                                                to int8 is negative)
  ds_mean4: the sum in 32 bits              test_pyramid_full_range, the 8      none
                                            cases of int32 / uint32
  filt_pred: Paeth's pb <= pc into <        test_adaptive_ties, both cases      none
                                            (only since the tie tiles hold
                                            the five-valued alphabet: two
                                            values never reach pb == pc < pa)

No kernel bug was found: every case passed on the unchanged kernels, floats included (-0,
denormals and their round-to-even ties, overflow of a + b come out as the header's rule says).
"""
import io
import itertools
import zlib

import numpy as np
import pytest

import pbx
import _numpy_ref as R
import _values as V

pytestmark = pytest.mark.gpu

_ids = itertools.count(500000)

FILTERS = [pbx.FILTER_SUB, pbx.FILTER_UP, pbx.FILTER_AVG, pbx.FILTER_PAETH, pbx.FILTER_ADAPTIVE]


def _register(svc, plane, pt, big_endian=True):
    """Register a plane of _values (big-endian samples) in either host byte order."""
    iid = next(_ids)
    sy, sx = plane.shape
    pid = svc.register_plane(iid, 0, 0, 0, pt, sx, sy, data=plane if big_endian else V.le(plane),
                             big_endian=big_endian)
    return iid, pid


def _idat(body):
    """The bytes the IDAT chunks of a PNG inflate to (zlib, an inflate of its own)."""
    assert body[:8] == b"\x89PNG\r\n\x1a\n"
    pos, data = 8, b""
    while pos < len(body):
        n = int.from_bytes(body[pos:pos + 4], "big")
        kind = body[pos + 4:pos + 8]
        if kind == b"IDAT":
            data += body[pos + 8:pos + 8 + n]
        assert zlib.crc32(body[pos + 4:pos + 8 + n]) == int.from_bytes(body[pos + 8 + n:pos + 12 + n], "big")
        pos += 12 + n
    return zlib.decompress(data)


def _png_tiles(svc, iid, tiles):
    res = svc.get_tiles([pbx.TileCtx(iid, 0, 0, 0, *t, format="png") for t in tiles])
    assert [st for st, _ in res] == [pbx.OK] * len(tiles)
    return [body for _, body in res]


# ------------------------------------------------- a. filters on random bits and extremes

FILTER_PLANE_RB, FILTER_PLANE_H = 3872, 50


def filter_regions(bpp):
    """Two batches of (x, y, rb, h) in bytes / rows: every path at its smallest and largest
    row; heights 13, 25, 49 end k_filter3's runs of 12 and 24 rows inside the tile."""
    odd = 17 if bpp == 1 else 18
    g1 = [(0, 0, 16, 13), (16, 1, 16, 49), (0, 1, 1024, 25), (32, 0, 1024, 49),   # k_filter3, G = 1
          (0, 0, 20, 13), (16, 1, 2044, 25), (0, 0, 2044, 49),                     # k_filter2
          (0, 0, odd, 13), (0, 2, 2052, 25), (2, 1, 1024, 25), (6, 0, 16, 49),     # k_filter, LDS
          (0, 0, 3856, 17), (2, 1, 3840, 33)]                                      # k_filter, plane
    g2 = [(0, 0, 1040, 13), (0, 1, 2048, 25), (16, 0, 2048, 49), (0, 3, 16, 25)]   # k_filter3, G = 2
    return [[(x // bpp, y, rb // bpp, h) for (x, y, rb, h) in g] for g in (g1, g2)]


def _filter_planes(pt):
    sx = FILTER_PLANE_RB // V.BPP[pt]
    return [V.random_bits(pt, sx, FILTER_PLANE_H, 5), V.extremes(pt, sx, FILTER_PLANE_H)]


@pytest.mark.parametrize("big_endian", [True, False])
@pytest.mark.parametrize("pt", V.PNG_TYPES)
@pytest.mark.parametrize("filt", FILTERS)
def test_filters_full_range(oracle, filt, pt, big_endian):
    """Sub, Up, Avg, Paeth and the adaptive choice on uniform random bits and on the type's
    extremes, on every filter kernel at its smallest and largest row: the inflated IDAT equals
    the restatement from the PNG specification and the oracle's stream."""
    with pbx.PixelsService(png_filter=filt) as svc:
        for plane in _filter_planes(pt):
            iid, _ = _register(svc, plane, pt, big_endian)
            for tiles in filter_regions(V.BPP[pt]):
                for (x, y, w, h), body in zip(tiles, _png_tiles(svc, iid, tiles)):
                    tile = V.cut(plane, x, y, w, h)
                    got = _idat(body)
                    assert got == R.png_stream(tile, pt, w, h, filt), (x, y, w, h)
                    assert got == oracle.png_filter_stream(np.frombuffer(tile, np.uint8), pt, w, h,
                                                           filt).tobytes(), (x, y, w, h)


@pytest.mark.parametrize("filt", FILTERS)
def test_filters_decode_under_pil(filt):
    """One tile per filter and type decodes under PIL to the tile's pixels (signed samples
    offset by half the range, as the PNG holds them)."""
    pytest.importorskip("PIL")
    from PIL import Image
    with pbx.PixelsService(png_filter=filt) as svc:
        for pt in V.PNG_TYPES:
            plane = _filter_planes(pt)[0]
            iid, _ = _register(svc, plane, pt)
            tiles = [filter_regions(V.BPP[pt])[0][k] for k in (2, 5, 9)]
            for (x, y, w, h), body in zip(tiles, _png_tiles(svc, iid, tiles)):
                im = np.array(Image.open(io.BytesIO(body)))
                bits = 8 * V.BPP[pt]
                want = plane[y:y + h, x:x + w].astype(np.int64)
                if pt in (V.INT8, V.INT16):
                    want = want + (1 << (bits - 1))
                assert im.shape == (h, w) and (im.astype(np.int64) == want).all(), (pt, x, y, w, h)


# ------------------------------------------------------ b. every Paeth triple on the device

def _paeth_id(c):
    return "%s-s%d-a%d" % (c[0], c[1], c[2])


def _run_paeth_case(oracle, filt, run, shift, lo, hi):
    pt = V.PAETH_RUNS[run]["pt"]
    plane, tiles = V.paeth_case(run, shift, lo, hi)
    with pbx.PixelsService(png_filter=filt) as svc:
        iid, pid = _register(svc, plane, pt)
        bodies = _png_tiles(svc, iid, tiles)
    for (x, y, w, h), body in zip(tiles, bodies):
        tile = np.frombuffer(V.cut(plane, x, y, w, h), np.uint8)
        assert _idat(body) == oracle.png_filter_stream(tile, pt, w, h, filt).tobytes(), (run, y)


@pytest.mark.parametrize("case", V.paeth_cases(), ids=_paeth_id)
def test_paeth_every_triple(oracle, case):
    """Filter Paeth on planes that hold every (left, up, up-left) byte triple: over the slices
    of a run all 2^24, on each implementation -- k_filter3's packed forms with one and two
    chunks per lane and 8- and 16-bit samples (the sign flip included), k_filter2's packed-f16
    paeth4, k_filter's integer filt_byte on an unaligned region -- and, for the two packed
    implementations, in every byte lane of a dword (four shifts).  tests/test_values.py
    asserts the coverage; the oracle's stream is pinned to the PNG specification there."""
    _run_paeth_case(oracle, pbx.FILTER_PAETH, *case)


@pytest.mark.parametrize("case", [c for c in V.paeth_cases() if c[1] == 0], ids=_paeth_id)
def test_paeth_every_triple_adaptive(oracle, case):
    """The same planes under the adaptive option: no tile of them is in the None mode, so the
    five sums (Paeth's among them) are taken on every row, and all five filters are chosen."""
    _run_paeth_case(oracle, pbx.FILTER_ADAPTIVE, *case)


# -------------------------------------------------------------------------------- c. ties

@pytest.mark.parametrize("unstaged", [False, True], ids=["staged", "unstaged"])
def test_adaptive_ties(oracle, unstaged):
    """Rows whose smallest sum is shared take the lowest filter, and q0 == q1 takes None, on
    k_filter3, k_filter2 and both paths of k_filter; the tile mode read from LDS (staged) and,
    in a batch with a 16,400-byte row, from the plane (unstaged; k_filter3 then with two chunks
    per lane).  The tiles over five neighbouring values hang on the order of Paeth's own
    comparisons in the sums (k_filter's and k_adaptive_mode's filt_pred, which no fixed filter
    runs).  Every IDAT equals both references; None-mode tiles hold filter byte 0 only."""
    planes = V.tie_planes(unstaged)
    with pbx.PixelsService(png_filter=pbx.FILTER_ADAPTIVE) as svc:
        ctxs, meta = [], []
        for p in planes:
            iid, _ = _register(svc, p["plane"], p["pt"])
            for t in p["tiles"]:
                ctxs.append(pbx.TileCtx(iid, 0, 0, 0, *t, format="png"))
                meta.append((p, t))
        res = svc.get_tiles(ctxs)
    modes = [0, 0]
    for (p, (x, y, w, h)), (st, body) in zip(meta, res):
        assert st == pbx.OK
        tile = V.cut(p["plane"], x, y, w, h)
        want = R.png_rows(tile, p["pt"], w, h, 5)
        got = _idat(body)
        assert got == want["stream"].tobytes(), (p["name"], x, y, w, h)
        assert got == oracle.png_filter_stream(np.frombuffer(tile, np.uint8), p["pt"], w, h, 5).tobytes()
        modes[want["tile_none"]] += 1
        if want["tile_none"]:
            assert not np.frombuffer(got, np.uint8).reshape(h, -1)[:, 0].any(), (p["name"], x, y, w, h)
    assert min(modes) > 0


# ----------------------------------------------------------------------------- d. pyramid

def _pyramid_planes(pt, kind):
    shapes = V.pyramid_shapes(pt)
    if kind == "extremes":
        return [V.extremes(pt, w, h, start=k) for k, (w, h) in enumerate(shapes)] + \
               [V.extremes(pt, *V.extremes_full_shape(pt))]
    return [V.random_bits(pt, w, h, 20 + k) for k, (w, h) in enumerate(shapes)] + \
           [V.random_bits(pt, 301, 97, 11)]


@pytest.mark.parametrize("kind", ["extremes", "random_bits"])
@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("pt", range(8))
def test_pyramid_full_range(pt, big_endian, kind):
    """build_pyramid down to 1 x 1 on the extremes and on random bits: 1-wide and 1-high planes
    and widths around k_downsample's vector groups, both host byte orders.  Integers are
    bit-exact (the signed floor (s + 2) >> 2 on negative sums, sums beyond 32 bits); floats are
    bit-exact against ((a + b) + (c + d)) * 0.25 in the sample's precision -- -0, denormals and
    their round-to-even ties, overflow of a + b -- except that where the reference is NaN
    (tests/test_values.py: on the extremes exactly the listed cells, on random bits under 5 %
    at level 1) any NaN will do."""
    dt = R.DTYPES_BE[pt]
    planes = _pyramid_planes(pt, kind)
    nan1 = tot1 = 0
    with pbx.PixelsService() as svc:
        for plane in planes:
            sy, sx = plane.shape
            _, pid = _register(svc, plane, pt, big_endian)
            nlev = V.levels_to_1x1(sx, sy)
            ids = svc.build_pyramid(pid, nlev) if nlev else []
            want = plane
            for k, lid in enumerate(ids, start=1):
                with np.errstate(all="ignore"):
                    want = R.downsample(want).astype(dt)
                h, w = want.shape
                got = V.from_bytes(svc.read_plane_be(lid, w * h * V.BPP[pt]), pt, w, h)
                if pt >= V.FLOAT:
                    nan = np.isnan(want)
                    assert np.isnan(got[nan]).all(), (sx, sy, k)
                    if k == 1:
                        nan1, tot1 = nan1 + int(nan.sum()), tot1 + nan.size
                    ut = ">u%d" % V.BPP[pt]
                    bad = (got.view(ut) != want.view(ut)) & ~nan
                    assert not bad.any(), (sx, sy, k, got[bad][:4], want[bad][:4])
                else:
                    assert got.tobytes() == want.tobytes(), (sx, sy, k)
            assert want.shape == (1, 1)
            for lid in ids + [pid]:
                svc.release_plane(lid)
    if pt >= V.FLOAT and kind == "random_bits":
        assert nan1 <= 0.05 * tot1


def test_pyramid_grid_stride(oracle):
    """A level of more than 65,536 x 256 vector groups (k_downsample's grid is capped at 65,536
    blocks; the rest is its grid-stride loop): a generated uint8 noise plane of 32,768 x 16,392,
    2,048 groups x 8,196 rows = 16,785,408.  Level 1 equals the restatement on bands of 64
    output rows: the first, one in the middle, the one before group 16,777,216 (row 8,192) and
    the last (rows 8,132..8,195, the second trip of the loop)."""
    sx, sy = 32768, 16392
    iid = next(_ids)
    with pbx.PixelsService() as svc:
        pid = svc.register_plane(iid, 0, 0, 0, pbx.UINT8, sx, sy, generator="noise", seed=3)
        ids = []
        try:
            ids = svc.build_pyramid(pid, 1)
            assert (sx // 2 // 8) * (sy // 2) > 65536 * 256
            bands = [0, 4096, 8128, sy // 2 - 64]
            res = svc.get_tiles([pbx.TileCtx(iid, 0, 0, 0, 0, y, sx // 2, 64, resolution=0) for y in bands])
            for y, (st, body) in zip(bands, res):
                assert st == pbx.OK
                src = oracle.gen_region(2, pbx.UINT8, 0, 2 * y, sx, 128, seed=3).reshape(128, sx)
                assert body == R.downsample(src).tobytes(), y
        finally:
            for lid in ids + [pid]:
                svc.release_plane(lid)


# ------------------------------------------------------------------- e. byte swap and flip

RAW_REGIONS = [(0, 0, 0, 0), (0, 0, 64, 48), (5, 3, 17, 9), (300, 96, 1, 1), (1, 0, 300, 1),
               (0, 1, 1, 96), (64, 32, 128, 64), (13, 7, 257, 31)]  # test_raw_all_types' list


@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("pt", range(8))
def test_swap_and_flip_random_bits(oracle, pt, big_endian):
    """Every byte of a sample busy: raw and uncompressed TIFF are the bytes numpy slices from
    the big-endian plane (NaN payloads included), deflate TIFF and tiled TIFF decode to them,
    and filter-None PNG (direct reader and staged rows) inflates to the numpy stream."""
    sx, sy = 301, 97
    plane = V.random_bits(pt, sx, sy, 40)
    full = [(x, y, w or sx, h or sy) for (x, y, w, h) in RAW_REGIONS]
    tiles = [V.cut(plane, *r) for r in full]
    for kw in (dict(), dict(tiff_deflate=True), dict(tiff_tile=64), dict(tiff_tile=64, tiff_deflate=True),
               dict(stage_rows=True)):
        with pbx.PixelsService(**kw) as svc:
            iid, _ = _register(svc, plane, pt, big_endian)
            if not kw:
                res = svc.get_tiles([pbx.TileCtx(iid, 0, 0, 0, *r) for r in RAW_REGIONS])
                assert [st for st, _ in res] == [pbx.OK] * len(full)
                assert [body for _, body in res] == tiles
            if "stage_rows" not in kw:
                res = svc.get_tiles([pbx.TileCtx(iid, 0, 0, 0, *r, format="tif") for r in RAW_REGIONS])
                for (x, y, w, h), tile, (st, body) in zip(full, tiles, res):
                    assert st == pbx.OK
                    r, px, meta = oracle.tiff_decode(body, len(tile))
                    assert r == 0 and px == tile, (kw, x, y, w, h)
                    assert meta["compression"] == (8 if kw.get("tiff_deflate") else 1)
                    if not kw:
                        assert body[160:] == tile and body == oracle.tiff_encode(np.frombuffer(tile, np.uint8), pt, w, h)[1]
            if pt in V.PNG_TYPES and ("stage_rows" in kw or not kw):
                bodies = _png_tiles(svc, iid, RAW_REGIONS)
                for (x, y, w, h), tile, body in zip(full, tiles, bodies):
                    assert _idat(body) == R.png_stream(tile, pt, w, h, 0), (kw, x, y, w, h)
