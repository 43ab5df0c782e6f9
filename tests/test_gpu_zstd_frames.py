"""k_zarr_zstd on hand-built frames that take every format path of RFC 8878 the kernel has
(tests/_zstd_cases.py; test_zstd_frames_host.py checks the same frames against libzstd and their
coverage against a checklist).  The frames are the chunks of a one-row uint8 plane under the
Zarr "zstd" codec, the shortest route to the kernel: frames of equal decoded length share one
registration, so many of them, at unaligned source offsets, decode in one launch.  Every
comparison is byte-exact; every refusal is a 400 that names the decoder code the kernel set."""
import itertools

import numpy as np
import pytest

import _tiff_fp
import _zarr
import _zstd_cases as C
import _zstd_frames as F
import pbx

pytestmark = pytest.mark.gpu

_ids = itertools.count(9_900_000)  # disjoint from the other test files (shared service)


def decode_frames(service, frames, length):
    """The frames as the chunks of a 1 x (n * length) uint8 plane; the plane's bytes."""
    iid = next(_ids)
    pid = service.register_zarr_plane(iid, 0, 0, 0, pbx.UINT8, length * len(frames), 1, length, 1, "zstd", frames,
                                      big_endian=False)
    try:
        return service.read_plane_be(pid, length * len(frames))
    finally:
        service.release_plane(pid)


_decoded = None


def decoded(service):
    """name -> the bytes the kernel decoded (or the error of the case's registration): one
    registration per distinct decoded length, made once."""
    global _decoded
    if _decoded is None:
        _decoded = {}
        groups = {}
        for name, b in C.cases().items():
            groups.setdefault(len(b.content), []).append(name)
        for length, names in groups.items():
            try:
                out = decode_frames(service, [C.cases()[n].frame for n in names], length)
                for k, n in enumerate(names):
                    _decoded[n] = out[k * length:(k + 1) * length]
            except pbx.PbxError as e:
                for n in names:
                    _decoded[n] = e
    return _decoded


def assert_decoded(service, name):
    got, want = decoded(service)[name], C.cases()[name].content
    assert not isinstance(got, Exception), got
    if got != want:
        first = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError("%s: first wrong byte at %d of %d" % (name, first, len(want)))


@pytest.mark.parametrize("name", [n for n in C.cases() if not n.startswith("ring_offset_")])
def test_frame(service, name):
    assert_decoded(service, name)


@pytest.mark.parametrize("off", F.RING_OFFSETS)
def test_ring_boundary_offset_at_every_start_phase(service, off):
    """seq_batch's ring / HBM split at RING - 64 = 4032: a match of this offset that begins at each
    position 0..63 of a 64-byte step (all 6 x 64 frames decode in one launch)."""
    for phase in range(64):
        assert_decoded(service, "ring_offset_%d_phase_%02d" % (off, phase))


# ----------------------------------------------------------- the other two front ends
def test_blosc_zstd_splits_of_hand_built_frames(service):
    chunk, raw = C.blosc_case()
    plane = np.frombuffer(raw, "<u2").reshape(1, -1)
    iid = next(_ids)
    pid = service.register_zarr_plane(iid, 0, 0, 0, pbx.UINT16, plane.shape[1], 1, plane.shape[1], 1, "blosc",
                                      [chunk], big_endian=False)
    try:
        assert service.read_plane_be(pid, plane.nbytes) == plane.astype(">u2").tobytes()
    finally:
        service.release_plane(pid)


def test_tiff_zstd_strips_of_hand_built_frames(service):
    """Compression 50000: one frame per strip; two planes of one strip each in one call."""
    names = ("modes_predefined_rle_fse_and_repeat_of_each", "huf_fse_weights_exit_after_state2")
    specs = []
    for n in names:
        b = C.cases()[n]
        specs.append(dict(image_id=next(_ids), z=0, c=0, t=0, pixel_type=pbx.UINT8, size_x=len(b.content), size_y=1,
                          seg_w=len(b.content), seg_h=1, tiled=False, compression=_tiff_fp.ZSTD, predictor=1,
                          big_endian=False, segments=[b.frame]))
    ids = service.register_tiff_planes(specs)
    try:
        for n, pid in zip(names, ids):
            want = C.cases()[n].content
            assert service.read_plane_be(pid, len(want)) == want, n
    finally:
        for pid in ids:
            service.release_plane(pid)


# ------------------------------------- content checksums of libzstd's own encoder (xxh64_wave)
CHECKSUM_LENGTHS = list(range(1, 71)) + [255, 256, 257, 1023, 1024, 1025, 1055, 1056, 1057]


def periodic(n, seed):
    return (C.rnd(5, seed) * (n // 5 + 1))[:n]


def test_checksummed_frames_of_every_tail_length(service):
    """xxh64_wave's 1 KiB rounds, 32-byte stripes, 8-byte, 4-byte and single-byte tails: noise (a raw
    block), a period of 5 (a compressed block) and a constant (an RLE block) of every length."""
    for n in CHECKSUM_LENGTHS:
        datas = [C.rnd(n, 3000 + n), periodic(n, 4000 + n), bytes([n & 255]) * n]
        frames = [_zarr.zstd_frame(d, 3, checksum=True) for d in datas]
        assert all(f[4] & 4 for f in frames)
        assert decode_frames(service, frames, n) == b"".join(datas), n


def test_checksummed_frames_at_every_destination_alignment(service):
    """The Zarr codec's destinations are 256-byte aligned; the blocks of a blosc chunk are not: five
    blocks of n bytes land at k * n, so gld64 sees every alignment mod 4 when n is odd or 2 mod 4.
    (c-blosc stores a block whose frame is not smaller than the block: lengths from 33 up.)"""
    for n in [x for x in CHECKSUM_LENGTHS if x >= 33]:
        raw = b"".join(periodic(n, 5000 + n + k) for k in range(5))
        chunk = _zarr.blosc_encode(raw, 1, clevel=3, shuffle=False, codec="zstd", blocksize=n, zstd_checksum=True)
        starts = [int.from_bytes(chunk[16 + 4 * k:20 + 4 * k], "little") for k in range(5)]
        sizes = [int.from_bytes(chunk[s:s + 4], "little") for s in starts]
        assert not chunk[2] & 2 and all(s < n for s in sizes), (n, sizes)  # five zstd frames, none stored
        assert all(chunk[s + 8] & 4 for s in starts)                     # ... with content checksums
        iid = next(_ids)
        pid = service.register_zarr_plane(iid, 0, 0, 0, pbx.UINT8, 5 * n, 1, 5 * n, 1, "blosc", [chunk],
                                          big_endian=False)
        try:
            assert service.read_plane_be(pid, 5 * n) == raw, n
        finally:
            service.release_plane(pid)


def test_flipped_content_byte_fails_the_checksum_at_every_tail_length(service):
    """One bit of a raw block's data: only the content checksum can notice (decoder code 37)."""
    good = C.cases()["hdr_fcs1_single_segment"]
    for n in (1, 3, 4, 7, 8, 31, 32, 33, 36, 40, 63, 64, 65, 1023, 1024, 1025, 1056, 1057):
        data = C.rnd(n, 6000 + n)
        frame = bytearray(_zarr.zstd_frame(data, 3, checksum=True))
        assert len(frame) >= n + 4 + 3  # a raw block: the content lies just before the checksum
        frame[-5 - (n // 2)] ^= 0x20
        with pytest.raises(pbx.PbxError) as ei:
            decode_frames(service, [bytes(frame)], n)
        assert ei.value.status == 400 and "zstd, decoder code 37)" in str(ei.value), (n, str(ei.value))
    assert decode_frames(service, [good.frame], len(good.content)) == good.content


# ---------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("name", list(C.malformed()))
def test_malformed_frame_is_refused_with_its_decoder_code(service, name):
    """The guard that stops each case is named in _zstd_cases.py.  A 400 that carries the code,
    nothing registered, and a good frame in a later registration decodes intact."""
    frame, size, code = C.malformed()[name]
    good = C.cases()["rep_all_four_cases_and_ll0_shift"]
    iid = next(_ids)
    with pytest.raises(pbx.PbxError) as ei:
        service.register_zarr_plane(iid, 0, 0, 0, pbx.UINT8, size, 1, size, 1, "zstd", [frame], big_endian=False)
    assert ei.value.status == 400
    assert "zstd, decoder code %d)" % code in str(ei.value), str(ei.value)
    assert service.lookup_plane(iid, 0, 0, 0) is None
    assert decode_frames(service, [good.frame], len(good.content)) == good.content


def test_malformed_frame_beside_good_ones_registers_nothing(service):
    """The refused frame between two good ones of its length: the whole registration fails."""
    frame, size, code = C.malformed()[C.OFFSET0]
    ok = F.build([("raw", C.rnd(size, 1))]).frame
    iid = next(_ids)
    with pytest.raises(pbx.PbxError) as ei:
        service.register_zarr_plane(iid, 0, 0, 0, pbx.UINT8, 3 * size, 1, size, 1, "zstd", [ok, frame, ok],
                                    big_endian=False)
    assert ei.value.status == 400 and "stream 1 (zstd, decoder code %d)" % code in str(ei.value)
    assert service.lookup_plane(iid, 0, 0, 0) is None
    assert decode_frames(service, [ok, ok, ok], size) == C.rnd(size, 1) * 3
