"""The admission decision of a band write that spans planes (csrc/band_state.h behind
pbx_test_band_group_admit), the exports of the two group calls, and the refusals the Python
methods make before they reach the library.  No device: the hook takes band descriptions as plain
integers and the refusals need no context.

The rule, restated here from include/pbx.h (pbx_band_write and the group calls):
  resident                                      -> 409
  loading, no writers, failed or idle too long  -> reset, then as absent (an idle one sets stale_reset)
  absent, stale_reset, piece not at first row   -> 500
  absent                                        -> join and allocate
  loading, HBM missing or failed                -> 409 (being allocated or reset by another caller)
  loading                                       -> join
and of a group: every member by that rule, unless the primary is kept out: then nobody joins."""
import ctypes
import itertools

import pytest

import pbx

ABSENT, LOADING, READY = 0, 1, 2
ALLOC, JOIN, SKIPPED = 1, 2, -1

# the six band conditions of the sweep: (state, hbm there, writers, failed, idle past the stale limit)
CONDITIONS = {
    "absent": (ABSENT, 0, 0, 0, 0),
    "loading": (LOADING, 1, 1, 0, 0),
    "loading without HBM": (LOADING, 0, 1, 0, 0),
    "failed, no writers": (LOADING, 1, 0, 1, 0),
    "stale, no writers": (LOADING, 1, 0, 0, 1),
    "resident": (READY, 1, 0, 0, 0),
}


def describe(cond, stale_reset):
    state, hbm, writers, failed, idle = CONDITIONS[cond]
    return [state, hbm, writers, failed, stale_reset, idle]


def rule(band, first_row):
    state, hbm, writers, failed, stale_reset, idle = band
    if state == READY:
        return 409
    if state == LOADING and writers == 0 and (failed or idle):
        if not failed:
            stale_reset = 1
        state = ABSENT
    if state == ABSENT:
        return 500 if stale_reset and not first_row else ALLOC
    if not hbm or failed:
        return 409
    return JOIN


def group_rule(bands, primary, first_row):
    own = rule(bands[primary], first_row)
    if own not in (ALLOC, JOIN):
        return [own if i == primary else SKIPPED for i in range(len(bands))]
    return [rule(b, first_row) for b in bands]


def admit(bands, primary, first_row):
    n = len(bands)
    flat = (ctypes.c_int32 * (6 * n))(*[v for b in bands for v in b])
    out = (ctypes.c_int32 * n)()
    rc = pbx.lib().pbx_test_band_group_admit(flat, n, primary, first_row, out)
    assert rc == 0, pbx.lib().pbx_last_error()
    return list(out)


MEMBERS = [describe(c, s) for c in CONDITIONS for s in (0, 1)]


def test_symbols_are_exported():
    L = pbx.lib()
    for name in ("pbx_band_write_tiff_group", "pbx_band_write_zarr_group", "pbx_test_band_group_admit"):
        assert name in pbx.EXPORTS and hasattr(L, name), name


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_admission_sweep(n):
    """Exhaustive: every combination of the six conditions x stale_reset per member, every primary,
    both values of the first-row flag (12^n x n x 2 groups; 165,888 for n = 4)."""
    checked = 0
    for bands in itertools.product(MEMBERS, repeat=n):
        for primary in range(n):
            for first_row in (0, 1):
                got = admit(bands, primary, first_row)
                assert got == group_rule(bands, primary, first_row), (bands, primary, first_row, got)
                checked += 1
    assert checked == 12 ** n * n * 2


def test_a_group_of_one_is_the_single_rule():
    for band in MEMBERS:
        for first_row in (0, 1):
            assert admit([band], 0, first_row) == [rule(band, first_row)]
    # the single rule's outcomes, case by case
    assert admit([describe("absent", 0)], 0, 0) == [ALLOC]
    assert admit([describe("absent", 1)], 0, 0) == [500]
    assert admit([describe("absent", 1)], 0, 1) == [ALLOC]
    assert admit([describe("loading", 0)], 0, 0) == [JOIN]
    assert admit([describe("loading without HBM", 0)], 0, 1) == [409]
    assert admit([describe("failed, no writers", 0)], 0, 0) == [ALLOC]
    assert admit([describe("failed, no writers", 1)], 0, 0) == [500]
    assert admit([describe("stale, no writers", 0)], 0, 0) == [500]
    assert admit([describe("stale, no writers", 0)], 0, 1) == [ALLOC]
    assert admit([describe("resident", 0)], 0, 1) == [409]
    # a failed load that still has a writer is not reset by this caller
    assert admit([[LOADING, 1, 1, 1, 0, 0]], 0, 1) == [409]
    # an idle load that still has a writer is joined
    assert admit([[LOADING, 1, 1, 0, 0, 1]], 0, 0) == [JOIN]


def test_primary_kept_out_means_nobody_joins():
    free = describe("absent", 0)
    for cond, stale_reset, first_row, status in (("resident", 0, 1, 409), ("loading without HBM", 0, 1, 409),
                                                 ("absent", 1, 0, 500), ("stale, no writers", 0, 0, 500)):
        for n in (2, 3, 4):
            for primary in range(n):
                bands = [free] * n
                bands[primary] = describe(cond, stale_reset)
                got = admit(bands, primary, first_row)
                assert got[primary] == status and all(g == SKIPPED for i, g in enumerate(got) if i != primary), got
    # and a sibling that is kept out keeps nobody else out
    assert admit([free, describe("resident", 0), describe("loading", 0), describe("absent", 1)], 0, 0) == [ALLOC, 409, JOIN, 500]


def test_hook_refusals():
    L = pbx.lib()
    one = (ctypes.c_int32 * 6)(*describe("absent", 0))
    out = (ctypes.c_int32 * 4)()
    for args, msg in (((None, 1, 0, 0, out), b"null argument"), ((one, 1, 0, 0, None), b"null argument"),
                      ((one, 0, 0, 0, out), b"group of 0 planes outside 1 .. 4"),
                      ((one, 5, 0, 0, out), b"group of 5 planes outside 1 .. 4"),
                      ((one, 1, 1, 0, out), b"primary 1 outside the group of 1"),
                      ((one, 1, -1, 0, out), b"primary -1 outside the group of 1"),
                      (((ctypes.c_int32 * 6)(3, 0, 0, 0, 0, 0), 1, 0, 0, out), b"bad band description 0"),
                      (((ctypes.c_int32 * 6)(1, 1, -1, 0, 0, 0), 1, 0, 0, out), b"bad band description 0")):
        assert L.pbx_test_band_group_admit(*args) == 400
        assert L.pbx_last_error() == msg


def test_python_refusals_need_no_device():
    """The service methods refuse a malformed group before they touch the library: on a service
    object that has no context at all."""
    svc = pbx.PixelsService(_handle=0)
    segs = [b"\0" * 16]
    tiff = (0, 4, 4, 4, False, pbx.TIFF_NONE, 1, segs)
    zarr = (0, 4, 4, 4, None, [b"\0" * 16])
    for ids, primary, msg in (([], 0, "group of 0 planes outside 1 .. 4"),
                              ([1, 2, 3, 4, 5], 0, "group of 5 planes outside 1 .. 4"),
                              ([1, 2], 2, "primary 2 outside the group of 2"),
                              ([1, 2], -1, "primary -1 outside the group of 2"),
                              ([1, 0, 3], 1, "primary 1 names plane id 0"),
                              ([7, 0, 7], 0, "plane 7 is members 0 and 2 of the group")):
        with pytest.raises(pbx.PbxError, match=msg) as e:
            svc.band_write_tiff_group(ids, primary, *tiff)
        assert e.value.status == 400
        with pytest.raises(pbx.PbxError, match=msg) as e:
            svc.band_write_zarr_group(ids, list(range(len(ids))), primary, *zarr, chunk_planes=8)
        assert e.value.status == 400
    with pytest.raises(pbx.PbxError, match="1 slices for a group of 2 planes") as e:
        svc.band_write_zarr_group([1, 2], [0], 0, *zarr, chunk_planes=2)
    assert e.value.status == 400
    with pytest.raises(pbx.PbxError, match="slice 1 is members 0 and 1 of the group") as e:
        svc.band_write_zarr_group([1, 2], [1, 1], 0, *zarr, chunk_planes=2)
    assert e.value.status == 400
    # the default is off, and load_bands takes the keyword
    assert svc.fill_siblings is False and pbx.PixelsService(_handle=0, fill_siblings=True).fill_siblings is True
    import inspect
    assert inspect.signature(pbx.PixelsService.load_bands).parameters["siblings"].default is None
