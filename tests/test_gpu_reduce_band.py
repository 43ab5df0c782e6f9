"""GPU: bands of derived resolution levels (pbx_band_write_reduced, k_reduce_band) and the
sources that serve them (pbx.DerivedLevels).

A band of stored level r + k of a sparse plane is made from the resident bands of level r in one
kernel; it must be bit for bit what pbx_plane_build_pyramid makes.  Two references, which must
agree with each other as well: tests/_numpy_ref.downsample applied k times (the rule restated in
numpy), and the same base registered as a dense plane and run through build_pyramid(levels=k).
Destination bands are read back as raw whole-band tiles through get_tile, so the bands go through
the serving path as a request's do.

Floats: bit-exact except where the reference is NaN (any NaN will do), as
test_gpu_values.test_pyramid_full_range compares them.  The planes of odd multiples of the smallest
denormal tell a kernel whose level arithmetic was contracted into FMAs from one that rounds every
level: test_denormal_plane_separates_fma_from_exact shows on the CPU that the two evaluations
differ on exactly these planes.
"""
import functools
import itertools

import numpy as np
import pytest

import pbx
import _numpy_ref as R
import _tiff_src as T
import _values as V

gpu = pytest.mark.gpu

_ids = itertools.count(7300000, 10)


# ------------------------------------------------------------------------------ helpers

def chain(plane, k):
    """The level k below `plane` by the numpy restatement, big-endian samples."""
    out = plane
    for _ in range(k):
        with np.errstate(all="ignore"):
            out = R.downsample(out).astype(plane.dtype)
    return out


def stored(plane, big_endian):
    """The bytes of rows of `plane` in the byte order of a plane created with `big_endian`."""
    return plane if big_endian else V.le(plane)


def same(got, want, pt, what):
    """Bit-exact; floats: NaN wherever the reference is NaN, bit-exact elsewhere."""
    assert got.shape == want.shape, what
    if pt >= V.FLOAT:
        nan = np.isnan(want)
        assert np.isnan(got[nan]).all(), what
        ut = ">u%d" % V.BPP[pt]
        bad = (got.view(ut) != want.view(ut)) & ~nan
        assert not bad.any(), (what, np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])
    else:
        assert got.tobytes() == want.tobytes(), what


def sparse_source(svc, iid, plane, pt, big_endian, band_rows, level=0, bands=None):
    """A sparse plane of `plane` at stored level `level`, the given bands (all) written."""
    sy, sx = plane.shape
    pid = svc.create_sparse_plane(iid, 0, 0, 0, pt, sx, sy, band_rows, level, big_endian=big_endian)
    rows = stored(plane, big_endian)
    for b in (range(-(-sy // band_rows)) if bands is None else bands):
        lo, hi = b * band_rows, min((b + 1) * band_rows, sy)
        svc.band_write(pid, lo, hi - lo, rows[lo:hi].tobytes())
    return pid


def reduce_level(svc, dst, src, k, dy, band_rows, split=False):
    """Every band of the destination, the odd ones in two pieces written out of order."""
    for b in range(-(-dy // band_rows)):
        lo, hi = b * band_rows, min((b + 1) * band_rows, dy)
        if split and b % 2 and hi - lo > 1:
            svc.band_write_reduced(dst, lo + 1, hi - lo - 1, src, k)
            svc.band_write_reduced(dst, lo, 1, src, k)
        else:
            svc.band_write_reduced(dst, lo, hi - lo, src, k)


def read_level(svc, iid, pt, dx, dy, band_rows, resolution=0):
    """The level as raw whole-band tiles through get_tile."""
    parts = []
    for lo in range(0, dy, band_rows):
        hi = min(lo + band_rows, dy)
        st, body = svc.get_tile(pbx.TileCtx(iid, 0, 0, 0, 0, lo, dx, hi - lo, resolution=resolution))
        assert st == pbx.OK, (st, lo, hi)
        parts.append(body)
    return V.from_bytes(b"".join(parts), pt, dx, dy)


def dense_pyramid(svc, plane, pt, big_endian, k):
    """Level k of the plane registered dense and run through build_pyramid(levels=k)."""
    iid = next(_ids)
    sy, sx = plane.shape
    pid = svc.register_plane(iid, 0, 0, 0, pt, sx, sy, data=stored(plane, big_endian), big_endian=big_endian)
    ids = svc.build_pyramid(pid, k)
    want = chain(plane, k)
    h, w = want.shape
    got = V.from_bytes(svc.read_plane_be(ids[-1], w * h * V.BPP[pt]), pt, w, h)
    for q in ids + [pid]:
        svc.release_plane(q)  # (the image's record goes with its last plane)
    return got


def reduced_through_bands(svc, plane, pt, big_endian, k, src_rows, dst_rows, split=False):
    """Level k of `plane` made band by band from a sparse source (src_rows > 0) or a dense one."""
    iid = next(_ids)
    sy, sx = plane.shape
    want = chain(plane, k)
    dy, dx = want.shape
    svc.declare_image(pbx.Pixels(iid, pt, sx, sy, levels=k + 1))
    if src_rows:
        src = sparse_source(svc, iid, plane, pt, big_endian, src_rows)
    else:
        src = svc.register_plane(iid, 0, 0, 0, pt, sx, sy, data=stored(plane, big_endian), big_endian=big_endian)
    dst = svc.create_sparse_plane(iid, 0, 0, 0, pt, dx, dy, dst_rows, k, big_endian=big_endian)
    reduce_level(svc, dst, src, k, dy, dst_rows, split)
    assert set(svc.band_info(dst)[1]) == {pbx.BS_READY}
    got = read_level(svc, iid, pt, dx, dy, dst_rows)
    svc.release_image(iid)
    return got


def sweep_shapes(pt, k):
    n = 8 // V.BPP[pt]
    return list(dict.fromkeys(V.pyramid_shapes(pt) + [(37, 29), (45, 21), (64, 48),
                                                      ((n << k) - 1, (1 << k) + 1), ((n << k) + 1, (1 << k) + 1)]))


@pytest.fixture(scope="module")
def svc():
    with pbx.PixelsService() as s:
        yield s


# ------------------------------------------------------------------------- parity sweep

@gpu
@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("pt", range(8))
def test_parity_sweep(svc, pt, big_endian, k):
    """Every pixel type, both stored byte orders, k = 1 .. 4: degenerate planes, widths around
    the 8-byte store groups, planes odd at every level, (2^k n +- 1) x (2^k + 1); source bands of
    5 rows against destination bands of 3 (pieces straddle source bands unevenly, odd bands
    written in two pieces, last row first), 8 against 4, and a dense source."""
    for i, (sx, sy) in enumerate(sweep_shapes(pt, k)):
        plane = V.random_bits(pt, sx, sy, 40 + i)
        want = chain(plane, k)
        same(dense_pyramid(svc, plane, pt, big_endian, k), want, pt, ("build_pyramid", sx, sy))
        same(reduced_through_bands(svc, plane, pt, big_endian, k, 5, 3, split=True), want, pt, ("5/3", sx, sy))
        same(reduced_through_bands(svc, plane, pt, big_endian, k, 8, 4), want, pt, ("8/4", sx, sy))
        if (sx, sy) in ((37, 29), (64, 48)):
            same(reduced_through_bands(svc, plane, pt, big_endian, k, 0, 4), want, pt, ("dense", sx, sy))


@gpu
@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("pt", [V.UINT8, V.UINT16, V.DOUBLE])
def test_more_than_one_tile_each_way(svc, pt, k):
    """Planes wider and taller than a workgroup's tile (a level-1 tile is 512 bytes x 64 rows):
    several tiles across and down, the last ones partial, a destination band of 80 rows."""
    sx, sy = 1024 // V.BPP[pt] * 2 + 2 * (1 << k) + 3, 3 * 64 + 37
    plane = V.random_bits(pt, sx, sy, 7 + k)
    same(reduced_through_bands(svc, plane, pt, True, k, 64, 80), chain(plane, k), pt, (sx, sy))


# -------------------------------------------------------------------- full-range values

def denormal_plane(pt, sx=181, sy=75, seed=5):
    """Odd multiples of the smallest denormal, both signs."""
    rng = np.random.default_rng([seed, pt])
    ut = ">u%d" % V.BPP[pt]
    mag = (rng.integers(0, 1 << 15, (sy, sx)).astype(np.uint64) * 2 + 1)
    sign = rng.integers(0, 2, (sy, sx)).astype(np.uint64) << np.uint64(8 * V.BPP[pt] - 1)
    return (mag | sign).astype(ut).view(R.DTYPES_BE[pt])


def _units(plane):
    """A denormal plane as signed integers, in units of the smallest denormal."""
    bits = 8 * V.BPP[V.FLOAT if plane.dtype.itemsize == 4 else V.DOUBLE]
    u = plane.view(">u%d" % (bits // 8)).astype(np.int64)
    mag = u & ((1 << (bits - 1)) - 1)
    return np.where(u >> (bits - 1), -mag, mag)


def _pad(a):
    if a.shape[1] % 2:
        a = np.concatenate([a, a[:, -1:]], axis=1)
    if a.shape[0] % 2:
        a = np.concatenate([a, a[-1:, :]], axis=0)
    return a


def _rhe(num, den):
    """num / den rounded to the nearest integer, ties to even (den 4 or 16, integer arrays)."""
    q, r = np.floor_divide(num, den), np.mod(num, den)
    up = (2 * r > den) | ((2 * r == den) & (q % 2 != 0))
    return q + up


def test_denormal_plane_separates_fma_from_exact():
    """CPU: on the denormal planes numpy's chain is the evaluation that rounds every level (sums of
    denormals are exact, each * 0.25 rounds to nearest even), and a contracted one -- the next
    level's a + b computed as fma(sum_a, 0.25, b), the product never rounded -- gives other
    samples at level 2.  So a kernel built with contraction fails test_full_range_values."""
    for pt in (V.FLOAT, V.DOUBLE):
        plane = denormal_plane(pt)
        a = _pad(_units(plane))
        p, q, r, s = a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2]
        sum1 = (p + q) + (r + s)           # exact: denormals add without rounding
        m1 = _rhe(sum1, 4)                 # the level rounds here
        assert (m1 == _units(chain(plane, 1))).all()
        a, S = _pad(m1), _pad(sum1)
        p, q, r, s = a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2]
        exact2 = _rhe((p + q) + (r + s), 4)
        assert (exact2 == _units(chain(plane, 2))).all()
        # contracted: a + b = fma(sum_a, 0.25, b) = round(sum_a / 4 + b), likewise c + d
        Sp, Sr = S[0::2, 0::2], S[1::2, 0::2]
        fma2 = _rhe(_rhe(Sp + 4 * q, 4) + _rhe(Sr + 4 * s, 4), 4)
        # (a tie at level 1 in `a` and an odd `b`: about one sum in eight is off by one unit, and
        # about a quarter of those move the level-2 sample; 874 samples here)
        assert (fma2 != exact2).sum() >= 8, (pt, int((fma2 != exact2).sum()))


@gpu
@pytest.mark.parametrize("big_endian", [True, False], ids=["be", "le"])
@pytest.mark.parametrize("pt", range(8))
def test_full_range_values(svc, pt, big_endian):
    """The extremes of every type in every 2x2 arrangement (signed floors on negative sums, sums
    beyond 32 bits, -0, denormal ties, overflow of a + b, infinities and NaN), k = 1 .. 4; for
    the float types also the planes of odd multiples of the smallest denormal."""
    planes = [V.extremes(pt, *V.extremes_full_shape(pt))]
    if pt >= V.FLOAT:
        planes.append(denormal_plane(pt))
    for plane in planes:
        for k in (1, 2, 3, 4):
            want = chain(plane, k)
            same(dense_pyramid(svc, plane, pt, big_endian, k), want, pt, ("build_pyramid", k))
            same(reduced_through_bands(svc, plane, pt, big_endian, k, 64, 64), want, pt, ("bands", k))


# ----------------------------------------------------------------------------- statuses

SX, SY, SB, DB = 1000, 64, 8, 4   # uint16: a source band is 8 * 2048 + 256 bytes, a destination band 4 * 1024 + 256
S_BAND, D_BAND = 8 * 2048 + 256, 4 * 1024 + 256


def _status(call):
    with pytest.raises(pbx.PbxError) as e:
        call()
    return e.value.status


def _pair(svc, bands=None, k=1, dims=(1, 1, 1), levels=None):
    """A uint16 source (the given bands written) and an empty destination k levels below."""
    iid = next(_ids)
    plane = V.random_bits(V.UINT16, SX, SY, 3)
    svc.declare_image(pbx.Pixels(iid, pbx.UINT16, SX, SY, *dims, levels=levels or k + 1))
    src = sparse_source(svc, iid, plane, pbx.UINT16, True, SB, bands=bands)
    dy, dx = chain(plane, k).shape
    dst = svc.create_sparse_plane(iid, 0, 0, 0, pbx.UINT16, dx, dy, DB, k)
    return iid, plane, src, dst


@gpu
def test_missing_source_band_is_not_resident():
    """Destination rows 4..7 at k = 1 need source rows 8..15 = source band 1."""
    with pbx.PixelsService() as svc:
        iid, plane, src, dst = _pair(svc, bands=[0, 2])
        before = svc.band_info(dst), svc.residency_stats()["resident_bytes"]
        assert _status(lambda: svc.band_write_reduced(dst, 4, 4, src, 1)) == pbx.E_NOT_RESIDENT
        msg = pbx.lib().pbx_last_error().decode()
        assert "source rows 8..16" in msg and "band 1" in msg, msg
        assert (svc.band_info(dst), svc.residency_stats()["resident_bytes"]) == before
        assert before[1] == 2 * S_BAND
        # a piece that needs no missing row is written (source rows 0..7: band 0)
        svc.band_write_reduced(dst, 0, 4, src, 1)
        assert svc.band_info(dst)[1][:2] == [pbx.BS_READY, pbx.BS_ABSENT]
        # a whole dense plane is a source too
        jid = next(_ids)
        svc.declare_image(pbx.Pixels(jid, pbx.UINT16, SX, SY, levels=2))
        dense = svc.register_plane(jid, 0, 0, 0, pbx.UINT16, SX, SY, data=plane)
        d3 = svc.create_sparse_plane(jid, 0, 0, 0, pbx.UINT16, 500, 32, DB, 1)
        svc.band_write_reduced(d3, 0, 4, dense, 1)
        assert read_level(svc, jid, pbx.UINT16, 500, 4, 4).tobytes() == chain(plane, 1)[:4].tobytes()


@gpu
def test_resident_destination_and_bad_arguments():
    with pbx.PixelsService() as svc:
        iid, plane, src, dst = _pair(svc, dims=(2, 2, 2), levels=3)
        red = lambda *a: _status(lambda: svc.band_write_reduced(*a))
        svc.band_write_reduced(dst, 0, 4, src, 1)
        assert red(dst, 0, 4, src, 1) == pbx.E_EXISTS            # resident
        assert red(dst, 1, 2, src, 1) == pbx.E_EXISTS
        for k in (0, 5, -1):
            assert red(dst, 4, 4, src, k) == pbx.E_BADARG
        assert red(dst, 4, 4, dst, 1) == pbx.E_BADARG            # its own source
        assert red(dst, 6, 4, src, 1) == pbx.E_BADARG            # rows leave the band
        assert "cross the end of band 1" in pbx.lib().pbx_last_error().decode()
        assert red(dst, 30, 4, src, 1) == pbx.E_BADARG           # rows leave the plane
        assert red(dst, 4, 0, src, 1) == pbx.E_BADARG
        assert red(src, 8, 8, dst, 1) == pbx.E_BADARG            # the wrong way round: level
        assert red(dst, 4, 4, src, 2) == pbx.E_BADARG            # level 1 is not 2 below level 0
        assert red(dst, 4, 4, 987654321, 1) == pbx.E_NOTFOUND
        assert red(987654321, 4, 4, src, 1) == pbx.E_NOTFOUND
        mk = lambda **kw: svc.create_sparse_plane(**{**dict(image_id=iid, z=0, c=0, t=0, pixel_type=pbx.UINT16,
                                                            size_x=500, size_y=32, band_rows=DB, level=1), **kw})
        assert red(mk(c=1), 4, 4, src, 1) == pbx.E_BADARG        # another channel
        assert red(mk(z=1), 4, 4, src, 1) == pbx.E_BADARG
        assert red(mk(t=1), 4, 4, src, 1) == pbx.E_BADARG
        assert red(mk(z=1, c=1, big_endian=False), 4, 4, src, 1) == pbx.E_BADARG
        lv2 = mk(level=2)
        assert red(lv2, 4, 4, src, 1) == pbx.E_BADARG            # level 2 from level 0 with k = 1
        assert red(lv2, 4, 4, src, 2) == pbx.E_BADARG            # 1000 x 64 is 250 x 16 two levels down, not 500 x 32
        other = next(_ids)
        svc.declare_image(pbx.Pixels(other, pbx.INT16, SX, SY, levels=2))
        assert red(svc.create_sparse_plane(other, 0, 0, 0, pbx.INT16, 500, 32, DB, 1), 4, 4, src, 1) == pbx.E_BADARG
        # mismatched type and byte order under the same key
        jid = next(_ids)
        svc.declare_image(pbx.Pixels(jid, pbx.UINT16, SX, SY, levels=2))
        s2 = sparse_source(svc, jid, plane, pbx.UINT16, True, SB)
        assert red(svc.create_sparse_plane(jid, 0, 0, 0, pbx.UINT16, 500, 32, DB, 1, big_endian=False), 4, 4, s2, 1) == pbx.E_BADARG
        assert "byte order" in pbx.lib().pbx_last_error().decode()
        # a size that does not reduce to the destination's
        kid = next(_ids)
        svc.declare_image(pbx.Pixels(kid, pbx.UINT16, SX, SY, levels=2))
        s3 = sparse_source(svc, kid, plane, pbx.UINT16, True, SB)
        assert red(svc.create_sparse_plane(kid, 0, 0, 0, pbx.UINT16, 501, 32, DB, 1), 4, 4, s3, 1) == pbx.E_BADARG
        # a dense source that is a row band; a dense destination
        lid = next(_ids)
        svc.declare_image(pbx.Pixels(lid, pbx.UINT16, SX, SY, levels=2))
        rb = svc.create_plane(lid, 0, 0, 0, pbx.UINT16, SX, SY, band=(0, 16))
        svc.write_rows_bytes(rb, 0, 16, plane[:16].tobytes())
        svc.commit_plane(rb)
        d4 = svc.create_sparse_plane(lid, 0, 0, 0, pbx.UINT16, 500, 32, DB, 1)
        assert red(d4, 0, 4, rb, 1) == pbx.E_BADARG
        assert "row band" in pbx.lib().pbx_last_error().decode()
        assert red(rb, 0, 4, d4, 1) == pbx.E_BADARG
        assert svc.band_info(d4)[1] == [pbx.BS_ABSENT] * 8


@gpu
def test_source_bands_are_evictable_after_the_call():
    """A budget of the source bands plus one destination band: the reduction fits; afterwards a
    source band written again (larger than what is free) must evict, and only the source bands the
    reduction read can go -- the destination band was just published and is still fresh."""
    with pbx.PixelsService() as svc:
        iid, plane, src, dst = _pair(svc, bands=[0, 1])
        svc.set_residency_budget(2 * S_BAND + D_BAND)
        svc.band_write_reduced(dst, 0, 4, src, 1)   # reads source band 0
        assert svc.residency_stats()["resident_bytes"] == 2 * S_BAND + D_BAND
        svc.band_write(src, 2 * SB, SB, plane[2 * SB:3 * SB].tobytes())
        states = svc.band_info(src)[1]
        assert states[2] == pbx.BS_READY and states[:2].count(pbx.BS_ABSENT) == 1
        assert states[0] == pbx.BS_ABSENT  # the band the reduction read: no longer fresh, so it went first
        assert svc.band_info(dst)[1][0] == pbx.BS_READY
        assert read_level(svc, iid, pbx.UINT16, 500, 4, 4).tobytes() == chain(plane, 1)[:4].tobytes()


@gpu
def test_injected_failure_leaves_nothing_behind():
    with pbx.PixelsService() as svc:
        iid, plane, src, dst = _pair(svc, bands=[0, 1])
        svc.set_residency_budget(2 * S_BAND + D_BAND)
        svc.test_fail_band_write(1)
        assert _status(lambda: svc.band_write_reduced(dst, 0, 4, src, 1)) == pbx.E_INTERNAL
        assert "injected" in pbx.lib().pbx_last_error().decode()
        assert svc.band_info(dst)[1] == [pbx.BS_ABSENT] * 8
        assert svc.residency_stats()["resident_bytes"] == 2 * S_BAND
        # the source band it pinned is unpinned (and no longer fresh): it can be evicted
        svc.band_write(src, 2 * SB, SB, plane[2 * SB:3 * SB].tobytes())
        assert svc.band_info(src)[1][:3] == [pbx.BS_ABSENT, pbx.BS_READY, pbx.BS_READY]
        assert _status(lambda: svc.band_write_reduced(dst, 0, 4, src, 1)) == pbx.E_NOT_RESIDENT
        svc.band_write_reduced(dst, 4, 4, src, 1)  # source band 1 is there
        got = svc.get_tile(pbx.TileCtx(iid, 0, 0, 0, 0, 4, 500, 4, resolution=0))
        assert got == (pbx.OK, chain(plane, 1)[4:8].tobytes())


# --------------------------------------------------------------------------- end to end

class FlatRows(pbx.PixelSource):
    """A flat image (one stored level) read by rows, counting what is read."""

    def __init__(self, image_id, plane, pt):
        self.plane, self.pt = plane, pt
        self.px = pbx.Pixels(image_id, pt, plane.shape[1], plane.shape[0])
        self.reads, self.rows, self.starts = 0, 0, []

    def get_pixels(self, image_id):
        return self.px if image_id == self.px.image_id else None

    def read_rows(self, pixels, z, c, t, level, y0, rows):
        assert level == 0
        self.reads, self.rows = self.reads + 1, self.rows + rows
        self.starts.append(y0)
        return self.plane[y0:y0 + rows].tobytes()


@functools.lru_cache(maxsize=None)
def e2e_levels():
    plane = V.random_bits(V.UINT16, 1000, 777, 99)
    return [chain(plane, k) for k in range(5)]


def e2e_tiles(w, h):
    """Regions of a w x h level in bands of 64 rows: a corner, bands straddled, the last rows
    and columns, the whole level if it is small."""
    t = [(0, 0, min(w, 64), min(h, 48)), (w - min(w, 33), h - min(h, 17), min(w, 33), min(h, 17))]
    if h > 64:
        t += [(3, 50, min(w - 3, 201), min(h - 50, 30)), (w // 2, 63, w - w // 2, 2)]
    if h > 200:
        t.append((1, 120, w - 2, 80))
    if w * h < 1 << 16:
        t.append((0, 0, w, h))
    return t


def tile_pixels(oracle, body, fmt, nbytes):
    if fmt is None:
        return body
    r, px, _ = oracle.png_decode(body) if fmt == "png" else oracle.tiff_decode(body, nbytes)
    assert r == 0
    return px


@gpu
@pytest.mark.parametrize("step", [1, 2, 4])
def test_flat_source_serves_every_resolution(oracle, step):
    levels = e2e_levels()
    iid = next(_ids)
    flat = FlatRows(iid, levels[0], pbx.UINT16)
    src = pbx.DerivedLevels(flat, levels=4)
    with pbx.PixelsService(sparse_band_rows=64, reduce_step=step) as svc:
        for res in range(5):  # OMERO numbering: 0 is the smallest level
            lv = levels[4 - res]
            h, w = lv.shape
            for (x, y, tw, th), fmt in zip(e2e_tiles(w, h), itertools.cycle([None, "png", "tif"])):
                tc = pbx.TileCtx(iid, 0, 0, 0, x, y, tw, th, resolution=res, format=fmt)
                body = pbx.TileRequestHandler(svc, tc, src).get_tile()
                assert body is not None, (res, x, y, tw, th, fmt)
                want = lv[y:y + th, x:x + tw].tobytes()
                assert tile_pixels(oracle, body, fmt, len(want)) == want, (res, x, y, tw, th, fmt)
        # outside a derived level, and a resolution the wrapper does not declare: the reference's 404
        assert pbx.TileRequestHandler(svc, pbx.TileCtx(iid, 0, 0, 0, 60, 0, 8, 8, resolution=0), src).get_tile() is None
        assert pbx.TileRequestHandler(svc, pbx.TileCtx(iid, 0, 0, 0, 0, 0, 8, 8, resolution=5), src).get_tile() is None
        # rows sharded over ranks: not for derived levels
        with pytest.raises(pbx.PbxError) as e:
            pbx.TileRequestHandler(svc, pbx.TileCtx(iid, 0, 0, 0, 0, 0, 8, 8, resolution=1), src, band=(0, 64)).get_tile()
        assert e.value.status == pbx.E_BADARG and "not sharded by rows" in str(e.value)


@gpu
def test_derived_tile_reads_only_its_base_rows(oracle):
    """A tile at derived level 2 (rows 70..79: destination band 1, rows 64..127) reads the base
    rows 256..511 -- four base bands -- and nothing else, whatever the step; a second tile in the
    same destination band reads nothing; both steps give the same bytes.  Without the wrapper the
    same request is the reference's 404."""
    levels = e2e_levels()
    bodies = []
    for step in (1, 2):
        iid = next(_ids)
        flat = FlatRows(iid, levels[0], pbx.UINT16)
        src = pbx.DerivedLevels(flat, levels=4)
        with pbx.PixelsService(sparse_band_rows=64, reduce_step=step) as svc:
            tc = pbx.TileCtx(iid, 0, 0, 0, 5, 70, 200, 10, resolution=2)
            body = pbx.TileRequestHandler(svc, tc, src).get_tile()
            assert body == levels[2][70:80, 5:205].tobytes()
            assert sorted(flat.starts) == [256, 320, 384, 448] and flat.rows == 256
            tc2 = pbx.TileCtx(iid, 0, 0, 0, 0, 100, 250, 27, resolution=2, format="png")
            png = pbx.TileRequestHandler(svc, tc2, src).get_tile()
            assert tile_pixels(oracle, png, "png", 0) == levels[2][100:127].tobytes()
            assert flat.reads == 4
            made = {lv: svc.lookup_plane(iid, 0, 0, 0, lv) is not None for lv in range(5)}
            assert made == {0: True, 1: step == 1, 2: True, 3: False, 4: False}
            bodies.append((body, png))
    assert bodies[0] == bodies[1]
    iid = next(_ids)
    bare = FlatRows(iid, levels[0], pbx.UINT16)
    with pbx.PixelsService(sparse_band_rows=64) as svc:
        tc = pbx.TileCtx(iid, 0, 0, 0, 5, 70, 200, 10, resolution=2)
        assert pbx.TileRequestHandler(svc, tc, bare).get_tile() is None
        assert bare.reads == 0


@gpu
def test_whole_planes_build_the_pyramid():
    """Without sparse_band_rows a derived level is built with every other one from the whole last
    stored level (build_pyramid), once."""
    levels = e2e_levels()
    iid = next(_ids)
    flat = FlatRows(iid, levels[0], pbx.UINT16)
    src = pbx.DerivedLevels(flat, levels=4)
    with pbx.PixelsService() as svc:
        for res, (x, y, w, h) in ((0, (3, 5, 50, 40)), (3, (100, 200, 300, 150)), (1, (0, 0, 125, 98)), (4, (10, 700, 900, 77))):
            body = pbx.TileRequestHandler(svc, pbx.TileCtx(iid, 0, 0, 0, x, y, w, h, resolution=res), src).get_tile()
            assert body == levels[4 - res][y:y + h, x:x + w].tobytes(), res
        assert flat.rows == 777
        assert svc.residency_stats()["planes"] == 5


@gpu
def test_tiff_source(tmp_path):
    """A flat deflate-tiled uint8 TIFF through TiffSource wrapped in DerivedLevels: the base bands
    are decoded from the file's tile rows on the GPU, the derived bands made from them."""
    a = V.random_bits(V.UINT8, 500, 300, 17)
    path = tmp_path / "flat.tif"
    T.write_tiff(str(path), [T.page_of(np.ascontiguousarray(a).view(np.uint8), compression=8, tile=(128, 64))])
    iid = next(_ids)
    src = pbx.DerivedLevels(pbx.TiffSource({iid: str(path)}), levels=3)
    px = src.get_pixels(iid)
    assert (px.levels, src.stored_levels(px), src.level_size(px, 3)) == (4, 1, (63, 38))
    with pbx.PixelsService(sparse_band_rows=32) as svc:
        for res, (x, y, w, h) in ((0, (0, 0, 63, 38)), (1, (7, 20, 100, 40)), (2, (0, 90, 250, 60)), (3, (16, 32, 256, 64))):
            body = pbx.TileRequestHandler(svc, pbx.TileCtx(iid, 0, 0, 0, x, y, w, h, resolution=res), src).get_tile()
            assert body == chain(a, 3 - res)[y:y + h, x:x + w].tobytes(), res
