"""The hand-built zstd frames (tests/_zstd_frames.py, tests/_zstd_cases.py) on the CPU: every
well-formed one decodes under the system libzstd to exactly the writer's expected bytes, the
censuses cover the whole checklist of format paths, and libzstd's verdict on each malformed frame
is pinned.  The reference here is libzstd, never the kernel; test_gpu_zstd_frames.py then gives
the same frames to k_zarr_zstd."""
import ctypes

import pytest

import _tiff_fp
import _zarr
import _zstd_cases as C
import _zstd_frames as F


def libzstd_verdict(frame, dlen):
    """The decoded bytes, or libzstd's error name."""
    L = _zarr._libzstd()
    L.ZSTD_decompress.restype = ctypes.c_size_t
    L.ZSTD_decompress.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    L.ZSTD_getErrorName.restype = ctypes.c_char_p
    L.ZSTD_getErrorName.argtypes = [ctypes.c_size_t]
    out = ctypes.create_string_buffer(max(dlen, 1))
    n = L.ZSTD_decompress(out, dlen, bytes(frame), len(frame))
    if L.ZSTD_isError(n):
        return L.ZSTD_getErrorName(n).decode()
    return out.raw[:n]


def test_xxh64_matches_libzstd_content_checksums():
    for n in list(range(0, 71)) + [255, 256, 257, 1023, 1024, 1025, 1055, 1056, 1057, 5000]:
        data = C.rnd(n, 7000 + n)
        frame = _zarr.zstd_frame(data, 3, checksum=True)
        assert int.from_bytes(frame[-4:], "little") == F.xxh64(data) & 0xFFFFFFFF, n


def test_fse_encoder_is_the_inverse_of_the_decoding_table():
    """Decode the states back, as RFC 8878 4.1.1 describes, for each predefined table."""
    for kind, nsym in (("LL", 36), ("OF", 29), ("ML", 53)):
        tab = F.fse_table(*F.DEFS[kind])
        syms = [int(s) for s in C.rnd(500, nsym)[:] if s < nsym] + list(range(nsym))
        st = F.fse_states(tab, syms)
        for i, s in enumerate(syms):
            sym, nb, base = tab.entries[st[i]]
            assert sym == s and (i + 1 == len(syms) or base <= st[i + 1] < base + (1 << nb))


@pytest.mark.parametrize("name", [n for n in C.cases() if not n.startswith("ring_offset_")])
def test_well_formed_frame_decodes_under_libzstd_to_the_expected_bytes(name):
    b = C.cases()[name]
    assert _tiff_fp.zstd_decode(b.frame, len(b.content)) == b.content


@pytest.mark.parametrize("off", F.RING_OFFSETS)
def test_ring_boundary_frames_decode_under_libzstd(off):
    for phase in range(64):
        b = C.cases()["ring_offset_%d_phase_%02d" % (off, phase)]
        assert len(b.content) == C.RING_PRE + C.RING_LITS + 370
        assert _tiff_fp.zstd_decode(b.frame, len(b.content)) == b.content, phase


def test_censuses_cover_the_whole_checklist():
    """A condition, not a measurement: every path of the checklist is taken by some case."""
    seen = set().union(*(b.census for b in C.cases().values()))
    missing = [item for item in C.CHECKLIST if item not in seen]
    assert not missing, missing
    assert len(set(C.CHECKLIST)) == len(C.CHECKLIST)


def test_sequence_bit_counts_of_the_wide_cases():
    """The writer knows T, the bits a sequence reads: 56 is the last single read, 57 the first split."""
    cs = C.cases()
    assert "T:56" in cs["T56_read64_limit"].census and "T:57" not in cs["T56_read64_limit"].census
    assert "max_T:57" in cs["T57_first_split_read"].census
    assert "max_T:64" in cs["T64_split_read"].census
    assert "max_T:73" in cs["T73_fse_tables_at_accuracy_logs_9_8_9"].census


# RFC 8878 calls each of these corrupt and k_zarr_zstd refuses them, but the system libzstd
# (1.4.x) decodes them: it forces an offset of 0 to 1, does not look at the two reserved bits of
# the Symbol_Compression_Modes byte and does not ask that the sequence bitstream be used up.
# The offset-0 frame is asserted to *decode*, so that the reason the project differs from its
# reference stays on record; the other two may be refused by a later libzstd, and where they are
# decoded the bytes must be the ones the frame describes.
LIBZSTD_LENIENT = {C.OFFSET0, "bits_left_over_in_the_sequence_stream", "reserved_mode_bits"}


@pytest.mark.parametrize("name", list(C.malformed()))
def test_libzstd_verdict_on_malformed_frame(name):
    frame, dlen, code = C.malformed()[name]
    assert 6 <= code <= 37
    got = libzstd_verdict(frame, dlen)
    if name == C.OFFSET0:
        pre = C.rnd(8, 90)
        assert got == pre + pre[-1:] * 4  # the match of 4 at "offset 0" copied from offset 1
    elif name in LIBZSTD_LENIENT:
        # a later libzstd may refuse; this one decodes what the frame says without the defect
        good = F.build([("raw", C.rnd(8, 90)), F.Comp(C.rnd(2, 93), [(2, F.O(4), 10)])])
        assert isinstance(got, str) or got == good.content
    else:
        assert isinstance(got, str), "libzstd decoded %d bytes" % len(got)


def test_oracle_zstd_path_agrees(oracle):
    """The oracle's own zstd path (libzstd behind its blosc reader) on hand-built frames as the
    splits of a blosc chunk: the chunk test_gpu_zstd_frames.py registers."""
    chunk, raw = C.blosc_case()
    L = oracle.lib()
    out = ctypes.create_string_buffer(len(raw))
    rc = L.pbxo_zarr_decode_chunk(1, chunk, ctypes.c_size_t(len(chunk)), out, ctypes.c_size_t(len(raw)))
    assert rc == 0 and out.raw == raw
