"""k_tiff_jpeg_decode and k_tiff_jpeg_place on hand-built scans that no encoder writes
(tests/_tiff_jpeg_cases.py; test_tiff_jpeg_frames_host.py holds the same streams equal to PIL and
their coverage to a checklist): a marker code, and a stuffed FF, at each of the 64 lanes of a refill
round, fill bytes, streams that end on a round or without EOI, 1,665-bit blocks, three table sets
under ids in no default order, every code length, size and extreme bit pattern, every batch shape,
and rows wider than the placement kernel's step of 1024 pixels.  The cases of a group are the
layers of one registration: one decode and one placement launch.  Every comparison is byte-exact
against the model; every refusal is a 400 that names the decoder code both models predicted."""
import itertools

import numpy as np
import pytest

import _tiff_jpeg as J
import _tiff_jpeg_cases as C
import _tiff_jpeg_frames as F
import pbx

pytestmark = pytest.mark.gpu

_ids = itertools.count(11_300_000)  # disjoint from the other test files (shared service)


def specs_of(page, image, samples=None):
    """register_tiff_planes specs of a chunky page: one per sample."""
    h, w, s, tile = page["length"], page["width"], page["spp"], page["tile"]
    tabs = next((bytes(t[2]) for t in page["extra"] if t[0] == 347), None)
    base = dict(image_id=image, z=0, t=0, pixel_type=pbx.UINT8, size_x=w, size_y=h, big_endian=False,
                seg_w=tile[0] if tile else w, seg_h=tile[1] if tile else min(page["rows_per_strip"], h),
                tiled=tile is not None, compression=pbx.TIFF_JPEG, predictor=1,
                jpeg=dict(tables=tabs, ycbcr=page["photometric"] == 6))
    packed = pbx.pack_chunks(page["segments"])
    return [dict(base, c=c, samples_per_pixel=s, sample=c, segments=packed) for c in (samples or range(s))]


def check_layers(svc, layers):
    """layers = [(name, page, expected (h, w) or (h, w, S))]: ONE registration, every plane equal."""
    specs, wants, names = [], [], []
    for name, page, want in layers:
        sp = specs_of(page, next(_ids))
        specs += sp
        wants += [want[:, :, c] if want.ndim == 3 else want for c in range(len(sp))]
        names += [name] * len(sp)
    ids = svc.register_tiff_planes(specs)
    try:
        for k, (pid, want) in enumerate(zip(ids, wants)):
            got = np.frombuffer(svc.read_plane_be(pid, want.size), np.uint8).reshape(want.shape)
            assert np.array_equal(got, want), (names[k], specs[k]["c"], np.argwhere(got != want)[:4].tolist())
    finally:
        for pid in ids:
            svc.release_plane(pid)


def expected(case):
    name, w, h, stream, kind = case
    return J.decode(stream, ycbcr=kind != "rgb", exempt=F.padding_blocks(stream) if name in C.EXEMPT else None)


def page_of(case):
    name, w, h, stream, kind = case
    return J.stream_page(w, h, stream, photometric=2 if kind == "rgb" else None)


def rows_of(svc, image, y0, rows, w, c=0):
    st, body = svc.get_tile(pbx.TileCtx(image, 0, c, 0, 0, y0, w, rows))
    assert st == pbx.OK, st
    return body


def band_write_whole(svc, case):
    """The case's last sample written as one band into a sparse plane."""
    name, w, h, stream, kind = case
    pg = page_of(case)
    S = pg["spp"]
    want = expected(case).reshape(h, w, -1)[:, :, S - 1]
    image = next(_ids)
    sp = specs_of(pg, image)[0]
    pid = svc.create_sparse_plane(image, 0, 0, 0, pbx.UINT8, w, h, h, big_endian=False)
    try:
        svc.band_write_tiff(pid, 0, h, w, h, False, 7, 1, sp["segments"], jpeg=sp["jpeg"], samples_per_pixel=S, sample=S - 1)
        assert svc.band_info(pid)[1] == [pbx.BS_READY]
        assert rows_of(svc, image, 0, h, w) == want.tobytes(), name
    finally:
        svc.release_plane(pid)


# ------------------------------------------------------------------------------ well-formed
@pytest.mark.parametrize("group", list(C.cases()))
def test_group_of_hand_built_streams(service, group):
    cases = C.cases()[group]
    layers = [(c[0], page_of(c), expected(c)) for c in cases]
    if group == "tables":  # the same streams abbreviated, their tables in tag 347
        for c in cases:
            tabs, rest = J.split_tables(c[3])
            pg = dict(page_of(c), segments=[rest], extra=[(347, 1, list(tabs))])
            layers.append((c[0] + " (tag 347)", pg, expected(c)))
    check_layers(service, layers)
    band_write_whole(service, cases[-1])


# ------------------------------------------------------------------------------ wide rows
def test_rows_wider_than_the_placement_step(service):
    """1045 = 1024 + a whole group + a partial group of 5, and 2080 (three steps), 1 .. 3 rows, in
    all four placement modes; 1040-wide tiles whose second column is clipped to 5 pixels."""
    check_layers(service, [(name, pg, J.decode_page(pg)) for name, pg in C.wide_pages()])


def test_band_write_of_one_sample_of_a_wide_row(service):
    """Rows 1 .. 2 of the 1045 x 3 4:2:0 strip, sample 1: the sentinel row above and the sibling
    planes stay as they were."""
    w, h, S, target = C.WIDE, 3, 3, 1
    pg = dict(C.wide_pages())["wide_420_%dx3" % w]
    want = J.decode_page(pg)
    sp = specs_of(pg, 0)[0]
    image = next(_ids)
    pids = [service.create_sparse_plane(image, 0, c, 0, pbx.UINT8, w, h, h, big_endian=False) for c in range(S)]
    try:
        for c in range(S):
            if c != target:
                service.band_write(pids[c], 0, h, bytes([0x30 + c]) * (h * w))
        service.band_write(pids[target], 0, 1, b"\xA5" * w)
        service.band_write_tiff(pids[target], 1, 2, w, h, False, 7, 1, sp["segments"], samples_per_pixel=S, sample=target,
                                jpeg=sp["jpeg"])
        assert service.band_info(pids[target])[1] == [pbx.BS_READY]
        got = rows_of(service, image, 0, h, w, c=target)
        assert got[:w] == b"\xA5" * w
        assert got[w:] == want[1:3, :, target].tobytes()
        for c in range(S):
            if c != target:
                assert rows_of(service, image, 0, h, w, c=c) == bytes([0x30 + c]) * (h * w)
    finally:
        for pid in pids:
            service.release_plane(pid)


# ------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("name", list(C.malformed()))
def test_malformed_stream_is_refused_with_its_decoder_code(service, name):
    """The code is the one the model and the schedule model end in (host test); the reason each
    case gives for it stands in _tiff_jpeg_cases.malformed().  A 400 that names it, nothing
    registered, and a band write leaves its band absent."""
    w, h, stream, kind, code, why = C.malformed()[name]
    pg = J.stream_page(w, h, stream)
    image = next(_ids)
    specs = specs_of(pg, image)
    with pytest.raises(pbx.PbxError, match=r"corrupt segment stream 0 \(jpeg, decoder code %d" % code) as e:
        service.register_tiff_planes(specs)
    assert e.value.status == 400
    assert all(service.lookup_plane(image, 0, c, 0) is None for c in range(pg["spp"]))
    pid = service.create_sparse_plane(image, 0, 0, 0, pbx.UINT8, w, h, h, big_endian=False)
    try:
        with pytest.raises(pbx.PbxError, match=r"corrupt segment stream 0 \(jpeg, decoder code %d" % code) as e:
            service.band_write_tiff(pid, 0, h, w, h, False, 7, 1, specs[0]["segments"], jpeg=specs[0]["jpeg"],
                                    samples_per_pixel=pg["spp"], sample=0)
        assert e.value.status == 400
        assert service.band_info(pid)[1] == [pbx.BS_ABSENT]
    finally:
        service.release_plane(pid)
