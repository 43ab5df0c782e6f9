"""CPU: the source rows and bands of a reduced band write (csrc/reduce_plan.h) through the test
hook pbx_test_reduce_plan, against a restatement in Python, and the Python side of derived levels
(pbx.DerivedLevels) that needs no device.

The rule (include/pbx.h, pbx_band_write_reduced): a level has (n + 1) // 2 rows of the level above,
row y of it reads rows 2y and min(2y + 1, n - 1), the clamp taken at every level; so rows
[y0, y0 + rows) of the level k below a level of n rows read rows [y0 << k, min((y0 + rows) << k, n))
of it, which lie in the bands first // B .. (last - 1) // B.  The restatement below gets the rows
by walking the dependencies level by level instead of from that closed form.
"""
import ctypes
import itertools

import numpy as np
import pytest

import pbx

KS = [1, 2, 3, 4]
SRC_BAND_ROWS = [5, 8, 64]
DST_BAND_ROWS = [3, 4, 64]
HEIGHTS = [1, 7, 29, 777]


def plan(k, sy, sb, db, y0, rows):
    out = (ctypes.c_int32 * 5)(*([-7] * 5))
    st = pbx.lib().pbx_test_reduce_plan(k, sy, sb, db, y0, rows, out)
    return st, list(out)


def sizes(n, k):
    """Rows of the levels 0 .. k below a level of n rows."""
    s = [n]
    for _ in range(k):
        s.append((s[-1] + 1) // 2)
    return s


def needed_rows(n, k, y0, rows):
    """The rows of level 0 that rows [y0, y0 + rows) of level k depend on, found level by level."""
    s = sizes(n, k)
    need = set(range(y0, y0 + rows))
    for j in range(k, 0, -1):
        need = {r for y in need for r in (2 * y, min(2 * y + 1, s[j - 1] - 1))}
    return need


def pieces(dy, db):
    """Pieces of a destination level of dy rows in bands of db rows: every whole band, and in
    every band its first row alone, its last row alone and a middle part."""
    out = []
    for lo in range(0, dy, db):
        hi = min(lo + db, dy)
        out += [(lo, hi - lo), (lo, 1), (hi - 1, 1)]
        if hi - lo > 2:
            out.append((lo + 1, hi - lo - 2))
    return list(dict.fromkeys(out))


@pytest.mark.parametrize("k", KS)
def test_source_rows_and_bands(k):
    n = 0
    for sy, sb, db in itertools.product(HEIGHTS, SRC_BAND_ROWS, DST_BAND_ROWS):
        dy = sizes(sy, k)[-1]
        for y0, rows in pieces(dy, db):
            st, (s0, s1, b0, b1, got_dy) = plan(k, sy, sb, db, y0, rows)
            assert st == pbx.OK, (k, sy, sb, db, y0, rows)
            assert got_dy == dy
            # exactly the closed form ...
            assert (s0, s1) == (y0 << k, min((y0 + rows) << k, sy)), (k, sy, y0, rows)
            # ... which is the hull of what the level-by-level walk needs (and the walk leaves no gap)
            need = needed_rows(sy, k, y0, rows)
            assert (min(need), max(need) + 1) == (s0, s1), (k, sy, y0, rows)
            assert need == set(range(s0, s1)), (k, sy, y0, rows)
            # the bands are the ones that hold those rows
            assert {r // sb for r in range(s0, s1)} == set(range(b0, b1 + 1)), (k, sy, sb, y0, rows)
            n += 1
    assert n > 100


def test_dense_source_is_one_band():
    for k, sy in itertools.product(KS, HEIGHTS):
        dy = sizes(sy, k)[-1]
        st, (s0, s1, b0, b1, _) = plan(k, sy, sy, 64, 0, min(dy, 64))
        assert st == pbx.OK and (b0, b1) == (0, 0) and s0 == 0


@pytest.mark.parametrize("k", [0, 5, -1])
def test_refuses_k_outside_1_to_4(k):
    st, out = plan(k, 777, 8, 4, 0, 1)
    assert st == pbx.E_BADARG and out == [-7] * 5
    assert b"outside 1 .. 4" in pbx.lib().pbx_last_error()


def test_refuses_rows_crossing_a_band_or_leaving_the_plane():
    for k, sy, db in itertools.product(KS, HEIGHTS, DST_BAND_ROWS):
        dy = sizes(sy, k)[-1]
        if dy > db:
            assert plan(k, sy, 8, db, db - 1, 2)[0] == pbx.E_BADARG  # rows db-1 and db: two bands
            assert b"cross" in pbx.lib().pbx_last_error()
        assert plan(k, sy, 8, db, dy - 1, 2)[0] == pbx.E_BADARG  # one row past the plane (or band)
        assert plan(k, sy, 8, db, dy, 1)[0] == pbx.E_BADARG
        assert plan(k, sy, 8, db, 0, 0)[0] == pbx.E_BADARG
        assert plan(k, sy, 8, db, -1, 1)[0] == pbx.E_BADARG
    assert plan(1, 0, 8, 4, 0, 1)[0] == pbx.E_BADARG
    assert plan(1, 7, 0, 4, 0, 1)[0] == pbx.E_BADARG
    assert plan(1, 7, 8, 0, 0, 1)[0] == pbx.E_BADARG
    assert pbx.lib().pbx_test_reduce_plan(1, 7, 8, 4, 0, 1, None) == pbx.E_BADARG


def test_abi_is_where_it_was():
    L = pbx.lib()
    assert L.pbx_abi_version() == 9
    assert L.pbx_abi_sizes((ctypes.c_uint64 * 8)(), 8) == 8
    for name in ("pbx_band_write_reduced", "pbx_test_reduce_plan"):
        assert name in pbx.EXPORTS and getattr(L, name)


# ------------------------------------------------------------------ DerivedLevels, no device

class Flat(pbx.PixelSource):
    def __init__(self, sx, sy, levels=1):
        self.sx, self.sy, self.levels = sx, sy, levels

    def get_pixels(self, image_id):
        return pbx.Pixels(image_id, pbx.UINT16, self.sx, self.sy, levels=self.levels) if image_id == 1 else None

    def level_size(self, pixels, level):
        sx, sy = self.sx, self.sy
        for _ in range(level):
            sx, sy = sx // 2, sy // 2  # a stored pyramid that rounds down: not the derived rule
        return sx, sy

    def read_rows(self, pixels, z, c, t, level, y0, rows):
        return b"rows %d %d %d" % (level, y0, rows)

    def band_chunks(self, pixels, z, c, t, level, y0, rows):
        return {"level": level}


def test_derived_levels_sizes_and_delegation():
    src = pbx.DerivedLevels(Flat(1001, 777, levels=2), levels=3)
    assert src.get_pixels(2) is None
    px = src.get_pixels(1)
    assert (px.levels, px.size_x, px.size_y, px.pixel_type) == (5, 1001, 777, pbx.UINT16)
    assert src.stored_levels(px) == 2
    assert [src.level_size(px, k) for k in range(5)] == [(1001, 777), (500, 388), (250, 194), (125, 97), (63, 49)]
    # stored levels go to the inner source untouched, derived ones have nothing to read
    assert src.read_rows(px, 0, 0, 0, 1, 4, 5) == b"rows 1 4 5"
    assert src.band_chunks(px, 0, 0, 0, 1, 0, 0) == {"level": 1}
    assert src.band_chunks(px, 0, 0, 0, 2, 0, 0) is None
    assert src.band_segments(px, 0, 0, 0, 0, 0, 0) is None and src.plane_segments(px, 0, 0, 0, 3) is None
    with pytest.raises(pbx.PbxError) as e:
        src.read_rows(px, 0, 0, 0, 2, 0, 1)
    assert e.value.status == pbx.E_BADARG
    # source_level = max(L - 1, level - step)
    assert [src.derived_from(px, lv, 2) for lv in range(5)] == [None, None, (1, 1), (1, 2), (2, 2)]
    assert [src.derived_from(px, lv, 1) for lv in range(2, 5)] == [(1, 1), (2, 1), (3, 1)]
    assert [src.derived_from(px, lv, 4) for lv in range(2, 5)] == [(1, 1), (1, 2), (1, 3)]
    # OMERO numbering: resolution 0 is the smallest level, 4 the full size
    assert [src.resolution_is_derived(1, r) for r in range(-1, 6)] == [False, True, True, True, False, False, False]
    assert not src.resolution_is_derived(2, 0)


@pytest.mark.parametrize("size,max_side,extra", [((100000, 100000), 3192, 5), ((3192, 3192), 3192, 0),
                                                 ((3193, 10), 3192, 1), ((10, 6385), 3192, 2),
                                                 ((1000, 777), 100, 4)])
def test_derived_levels_halve_until_max_side(size, max_side, extra):
    src = pbx.DerivedLevels(Flat(*size), max_side=max_side)
    px = src.get_pixels(1)
    assert px.levels == 1 + extra
    assert max(src.level_size(px, px.levels - 1)) <= max_side
    if extra:
        assert max(src.level_size(px, px.levels - 2)) > max_side


def test_reduce_step_is_1_to_4():
    for bad in (0, 5, -1):
        with pytest.raises(ValueError):
            pbx.PixelsService(reduce_step=bad)
    with pytest.raises(ValueError):
        pbx.DerivedLevels(Flat(10, 10), levels=-1)
    assert np.iinfo(np.int32).max >> 4 > 100000  # (y0 + rows) << k stays far inside 32 bits
