"""k_zarr_inflate2 (and k_zarr_inflate, the single-wave decoder behind PBX_INFLATE_1WAVE) on
hand-built deflate streams that take the paths zlib's own encoder never writes
(tests/_deflate_cases.py; test_deflate_frames_host.py checks the same streams against zlib and
their coverage against a checklist).  The streams are the chunks of a one-row uint8 plane under
the Zarr "zlib" codec: streams of equal decoded length share one registration, so many of them,
at unaligned source offsets, decode in one launch.  Every comparison is byte-exact; every
refusal is a 400 that names the decoder code the cases file predicted from the source."""
import itertools

import pytest

import _deflate_cases as C
import _deflate_frames as F
import pbx

pytestmark = pytest.mark.gpu

_ids = itertools.count(9_500_000)  # disjoint from the other test files (shared service)


def decode_frames(service, frames, length, codec="zlib"):
    """The streams as the chunks of a 1 x (n * length) uint8 plane; the plane's bytes."""
    iid = next(_ids)
    pid = service.register_zarr_plane(iid, 0, 0, 0, pbx.UINT8, length * len(frames), 1, length, 1, codec, frames,
                                      big_endian=False)
    try:
        return service.read_plane_be(pid, length * len(frames))
    finally:
        service.release_plane(pid)


def decode_all(service):
    """name -> the bytes the kernel decoded (or the error of the case's registration): one
    registration per distinct decoded length."""
    out, groups = {}, {}
    for name, b in C.cases().items():
        groups.setdefault(len(b.content), []).append(name)
    for length, names in groups.items():
        try:
            got = decode_frames(service, [C.cases()[n].frame for n in names], length)
            for k, n in enumerate(names):
                out[n] = got[k * length:(k + 1) * length]
        except pbx.PbxError as e:
            for n in names:
                out[n] = e
    return out


_decoded = {}


def decoded(service, one_wave):
    """The launcher reads PBX_INFLATE_1WAVE at every launch; the caller has set or cleared it."""
    if one_wave not in _decoded:
        _decoded[one_wave] = decode_all(service)
    return _decoded[one_wave]


@pytest.fixture(params=["two_wave", "one_wave"])
def one_wave(request, monkeypatch):
    if request.param == "one_wave":
        monkeypatch.setenv("PBX_INFLATE_1WAVE", "1")
    else:
        monkeypatch.delenv("PBX_INFLATE_1WAVE", raising=False)
    return request.param == "one_wave"


def assert_decoded(service, one_wave, name):
    got, want = decoded(service, one_wave)[name], C.cases()[name].content
    assert not isinstance(got, Exception), got
    if got != want:
        first = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError("%s: first wrong byte at %d of %d" % (name, first, len(want)))


@pytest.mark.parametrize("name", C.small_cases())
def test_stream(service, one_wave, name):
    assert_decoded(service, one_wave, name)


@pytest.mark.parametrize("dist", F.RING_DISTS)
def test_ring_boundary_distance_at_every_start_phase(service, one_wave, dist):
    """The consumer's ring / HBM split at ZP_RINGB - 64 = 16320 (the single-wave decoder's ring is
    the whole window, ZR_INF): a match of 258 at this distance that begins at each position 0..63
    of a 64-byte step (all 8 x 64 streams decode in one launch)."""
    for phase in range(64):
        assert_decoded(service, one_wave, "ring_dist_%d_phase_%02d" % (dist, phase))


# ------------------------------------------------------------------ the other front ends
def test_gzip_members_and_bytes_after_the_trailer(service):
    members, trailing = C.gzip_cases()
    n = len(members[0].content)
    assert decode_frames(service, [b.frame for b in members], n, "gzip") == b"".join(b.content for b in members)
    iid = next(_ids)
    with pytest.raises(pbx.PbxError) as ei:
        service.register_zarr_plane(iid, 0, 0, 0, pbx.UINT8, 2 * n, 1, n, 1, "gzip", [members[1].frame, trailing],
                                    big_endian=False)
    assert ei.value.status == 400 and "stream 1 (gzip, decoder code 31)" in str(ei.value), str(ei.value)
    assert service.lookup_plane(iid, 0, 0, 0) is None


def test_blosc_zlib_splits_of_hand_built_streams(service, one_wave):
    chunk, raw = C.blosc_case()
    n = len(raw) // 2
    iid = next(_ids)
    pid = service.register_zarr_plane(iid, 0, 0, 0, pbx.UINT16, n, 1, n, 1, "blosc", [chunk], big_endian=False)
    try:
        import numpy as np
        assert service.read_plane_be(pid, len(raw)) == np.frombuffer(raw, "<u2").astype(">u2").tobytes()
    finally:
        service.release_plane(pid)


def test_tiff_deflate_strips_of_hand_built_streams(service, one_wave):
    """Compression 8: one stream per strip; two planes of one strip each in one call."""
    names = ("hlit_286_hdist_30_hclen_19_and_every_repeat_form", "widest_token_48_bits_at_every_bit_phase")
    specs = []
    for n in names:
        b = C.cases()[n]
        specs.append(dict(image_id=next(_ids), z=0, c=0, t=0, pixel_type=pbx.UINT8, size_x=len(b.content), size_y=1,
                          seg_w=len(b.content), seg_h=1, tiled=False, compression=8, predictor=1,
                          big_endian=False, segments=[b.frame]))
    ids = service.register_tiff_planes(specs)
    try:
        for n, pid in zip(names, ids):
            want = C.cases()[n].content
            assert service.read_plane_be(pid, len(want)) == want, n
    finally:
        for pid in ids:
            service.release_plane(pid)


# ---------------------------------------------------------------------------- refusals
GOOD = "hlit_286_hdist_30_hclen_19_and_every_repeat_form"


def refused(service, frames, size, what):
    iid = next(_ids)
    with pytest.raises(pbx.PbxError) as ei:
        service.register_zarr_plane(iid, 0, 0, 0, pbx.UINT8, size * len(frames), 1, size, 1, "zlib", frames,
                                    big_endian=False)
    assert ei.value.status == 400 and what in str(ei.value), str(ei.value)
    assert service.lookup_plane(iid, 0, 0, 0) is None


def check_refusal(service, name):
    frame, size, code, guard = C.malformed()[name]
    good = C.cases()[GOOD]
    refused(service, [frame], size, "(zlib, decoder code %d)" % code)
    assert decode_frames(service, [good.frame], len(good.content)) == good.content


@pytest.mark.parametrize("name", [n for n, v in C.malformed().items() if v[2] not in C.ONE_WAVE_SKIPS])
def test_malformed_stream_is_refused_with_its_decoder_code(service, one_wave, name):
    """The guard that stops each case is named in _deflate_cases.py.  A 400 that carries the code,
    nothing registered, and a good stream in a later registration decodes intact."""
    check_refusal(service, name)


TRAILER_CASES = [n for n, v in C.malformed().items() if v[2] in C.ONE_WAVE_SKIPS]


@pytest.mark.parametrize("name", TRAILER_CASES)
def test_cut_or_wrong_trailer_is_refused_by_the_two_wave_decoder(service, monkeypatch, name):
    monkeypatch.delenv("PBX_INFLATE_1WAVE", raising=False)
    check_refusal(service, name)


@pytest.mark.parametrize("name", TRAILER_CASES)
def test_single_wave_decoder_reads_no_trailer(service, monkeypatch, name):
    """k_zarr_inflate checks no Adler-32: the known difference of the A/B path, and the only thing
    that shows from outside which kernel ran.  With PBX_INFLATE_1WAVE set the streams the two-wave
    decoder refuses with 28 / 29 register and decode to their content."""
    import zlib
    monkeypatch.setenv("PBX_INFLATE_1WAVE", "1")
    frame, size, code, guard = C.malformed()[name]
    assert decode_frames(service, [frame], size) == zlib.decompressobj(-15).decompress(frame[2:])


@pytest.mark.parametrize("name", list(C.truncated()))
def test_stream_cut_inside_a_huffman_block_is_refused(service, one_wave, name):
    """The code depends on the bytes that follow the stream in the upload buffer: only the refusal."""
    frame, size = C.truncated()[name]
    good = C.cases()[GOOD]
    refused(service, [frame], size, "(zlib, decoder code ")
    assert decode_frames(service, [good.frame], len(good.content)) == good.content


def test_malformed_stream_beside_good_ones_registers_nothing(service, one_wave):
    """The refused stream between two good ones of its length: the whole registration fails."""
    frame, size, code, guard = C.malformed()["distance_past_the_start_in_mid_batch"]
    ok = F.build([F.fixed(list(C.rnd(size, 1)))]).frame
    refused(service, [ok, frame, ok], size, "stream 1 (zlib, decoder code %d)" % code)
    assert decode_frames(service, [ok, ok, ok], size) == C.rnd(size, 1) * 3
