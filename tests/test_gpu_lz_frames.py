"""k_zarr_lz4 and k_zarr_blosclz on hand-built streams that take the paths liblz4's and c-blosc's
encoders never write (tests/_lz_cases.py; test_lz_frames_host.py checks the same streams against
the oracle and the libraries, and their coverage against a checklist).  The streams are the blocks
of one c-blosc frame, the single chunk of a one-row uint8 plane: streams of equal decoded length
share a registration, so many of them, at unaligned source offsets, decode in one launch.  Every
comparison is byte-exact; every refusal is a 400 that names the decoder code the cases file
predicted from the source."""
import ctypes
import itertools

import numpy as np
import pytest

import _lz_cases as C
import _lz_frames as F
import pbx

pytestmark = pytest.mark.gpu

_ids = itertools.count(10_300_000)  # disjoint from the other test files (shared service)
CODEC = {"lz4": F.LZ4, "blosclz": F.BLOSCLZ}


def frame_of(cases, codec, **kw):
    """One frame of the cases (equal lengths), the streams at unaligned offsets."""
    cases = list(cases)
    gaps = [(3 * k + 1) % 7 for k in range(len(cases))]
    return F.blosc_frame([c.stream for c in cases], len(cases[0].content), codec, gaps=gaps, **kw)


def decode_frame(service, frame, nbytes, pixel_type=pbx.UINT8, bpp=1):
    """The frame as the only chunk of a 1 x n plane; the plane's bytes."""
    pid = service.register_zarr_plane(next(_ids), 0, 0, 0, pixel_type, nbytes // bpp, 1, nbytes // bpp, 1, "blosc",
                                      [frame], big_endian=False)
    try:
        return service.read_plane_be(pid, nbytes)
    finally:
        service.release_plane(pid)


def decode_group(service, cases, codec):
    """name -> the bytes the kernel decoded for it (or the registration's error)."""
    names = list(cases)
    n = len(cases[names[0]].content)
    try:
        got = decode_frame(service, frame_of(cases.values(), codec), n * len(names))
    except pbx.PbxError as e:
        return {k: e for k in names}
    return {k: got[i * n:(i + 1) * n] for i, k in enumerate(names)}


_decoded = {}


def decoded(service, kind):
    """One registration per distinct decoded length of the named cases."""
    if kind not in _decoded:
        out, groups = {}, {}
        for name, c in (C.lz4_cases() if kind == "lz4" else C.blz_cases()).items():
            groups.setdefault(len(c.content), {})[name] = c
        for group in groups.values():
            out.update(decode_group(service, group, CODEC[kind]))
        _decoded[kind] = out
    return _decoded[kind]


def assert_same(name, got, want):
    assert not isinstance(got, Exception), got
    if got != want:
        first = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError("%s: first wrong byte at %d of %d" % (name, first, len(want)))


@pytest.mark.parametrize("name", C.lz4_small_names())
def test_lz4_stream(service, name):
    assert_same(name, decoded(service, "lz4")[name], C.lz4_cases()[name].content)


def test_lz4_window_reload_at_the_loop_top_in_every_phase(service):
    """0..83 literals before a fixed body: the reload at the loop top, with a batch pending whose
    literals lie behind ip in the old window, at every ip - base from 941 to 1004."""
    for k in C.PREFIXES:
        name = "top_reload_prefix_%02d" % k
        assert_same(name, decoded(service, "lz4")[name], C.lz4_cases()[name].content)


@pytest.mark.parametrize("path", C.LZ4_PATHS)
@pytest.mark.parametrize("off", F.LZ4_RING_OFFS)
def test_lz4_ring_boundary_offset_at_every_start_phase(service, off, path):
    """The ring / HBM split of seq_batch (off > 4032, a match of 8 in a batch) and of
    OutRing::match (off > 4096, a match of 300): the match begins at each of 64 consecutive
    positions, across a 64-byte step and a 256-byte flush boundary (64 streams, one launch)."""
    cases = C.lz4_phases(off, path)
    got = decode_group(service, cases, F.LZ4)
    for name, c in cases.items():
        assert_same(name, got[name], c.content)


@pytest.mark.parametrize("name", list(C.blz_cases()))
def test_blosclz_stream(service, name):
    assert_same(name, decoded(service, "blosclz")[name], C.blz_cases()[name].content)


@pytest.mark.parametrize("dist", F.BLZ_RING_DISTS)
def test_blosclz_ring_boundary_distance_at_every_start_phase(service, dist):
    cases = C.blz_phases(dist)
    got = decode_group(service, cases, F.BLOSCLZ)
    for name, c in cases.items():
        assert_same(name, got[name], c.content)


@pytest.mark.parametrize("kind", ["lz4", "blosclz"])
def test_byte_shuffled_frame_of_hand_built_splits(service, oracle, kind):
    """typesize 2 with the byte-shuffle bit: k_zarr_place unshuffles what the decoders wrote.
    Expected: the oracle's decode of the same frame."""
    cases = {k: c for k, c in (C.lz4_cases() if kind == "lz4" else C.blz_cases()).items() if len(c.content) == C.A}
    frame = frame_of(cases.values(), CODEC[kind], typesize=2, shuffle=True)
    n = C.A * len(cases)
    out = ctypes.create_string_buffer(n)
    assert oracle.lib().pbxo_zarr_decode_chunk(1, frame, ctypes.c_size_t(len(frame)), out, ctypes.c_size_t(n)) == 0
    want = np.frombuffer(out.raw, "<u2").astype(">u2").tobytes()
    assert decode_frame(service, frame, n, pbx.UINT16, 2) == want


# ---------------------------------------------------------------------------- refusals
GOOD = {"lz4": "literal_lengths_0_1_14_15_16_269_270_525", "blosclz": "match_lengths_3_8_9_263_264"}


def good_case(kind):
    return (C.lz4_cases() if kind == "lz4" else C.blz_cases())[GOOD[kind]]


def refused(service, kind, streams, size, what):
    iid = next(_ids)
    frame = F.blosc_frame(streams, size, CODEC[kind], gaps=[(5 * k + 2) % 7 for k in range(len(streams))])
    with pytest.raises(pbx.PbxError) as ei:
        service.register_zarr_plane(iid, 0, 0, 0, pbx.UINT8, size * len(streams), 1, size * len(streams), 1, "blosc",
                                    [frame], big_endian=False)
    assert ei.value.status == 400 and what in str(ei.value), str(ei.value)
    assert service.lookup_plane(iid, 0, 0, 0) is None


def check_refusal(service, kind, stream, size, code):
    good = good_case(kind)
    refused(service, kind, [stream], size, "(%s, decoder code %d)" % (kind, code))
    assert decode_frame(service, frame_of([good], CODEC[kind]), len(good.content)) == good.content


@pytest.mark.parametrize("name", list(C.lz4_malformed()))
def test_lz4_malformed_stream_is_refused_with_its_decoder_code(service, name):
    """The guard that stops each case, and the path the stream takes to it, are named in
    _lz_cases.py.  A 400 that carries the code, nothing registered, and a good stream in a later
    registration decodes intact."""
    stream, size, code, guard, path = C.lz4_malformed()[name]
    check_refusal(service, "lz4", stream, size, code)


@pytest.mark.parametrize("name", list(C.blz_malformed()))
def test_blosclz_malformed_stream_is_refused_with_its_decoder_code(service, name):
    stream, size, code, guard = C.blz_malformed()[name]
    check_refusal(service, "blosclz", stream, size, code)


@pytest.mark.parametrize("kind,name", [("lz4", "offset_one_beyond_the_start_mid_batch"),
                                       ("blosclz", "distance_one_beyond_the_start")])
def test_malformed_stream_between_good_ones_registers_nothing(service, kind, name):
    """The refused stream between two good ones of its length: the message names stream 1 and the
    whole registration fails."""
    v = (C.lz4_malformed() if kind == "lz4" else C.blz_malformed())[name]
    good = good_case(kind)
    assert len(good.content) == v[1]
    refused(service, kind, [good.stream, v[0], good.stream], v[1], "stream 1 (%s, decoder code %d)" % (kind, v[2]))
    got = decode_frame(service, F.blosc_frame([good.stream] * 3, v[1], CODEC[kind]), 3 * v[1])
    assert got == good.content * 3
