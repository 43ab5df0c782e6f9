"""The hand-built LZ4 and BloscLZ streams (tests/_lz_frames.py, tests/_lz_cases.py) on the CPU: every
well-formed one decodes to exactly the writer's bytes under the Python reference, under the oracle
(pbxo_lz4_decode / pbxo_blosclz_decode: the arbiter) and, where it obeys the encoder-side rules,
under the library (LZ4_decompress_safe of the system liblz4; c-blosc 1.21's frame decoder for
BloscLZ); every frame decodes under the oracle's and c-blosc's frame decoders; the censuses of the
schedule model cover the checklist line by line; the oracle refuses every malformed stream.  The
reference is never the kernel; test_gpu_lz_frames.py then gives the same streams to k_zarr_lz4 and
k_zarr_blosclz."""
import ctypes
import os
import re

import pytest

import _lz_cases as C
import _lz_frames as F
import _zarr

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "omero-ms-pixel-buffer_amd", "csrc")


def oracle_stream(oracle, codec, stream, olen):
    fn = oracle.lib().pbxo_lz4_decode if codec == F.LZ4 else oracle.lib().pbxo_blosclz_decode
    out = ctypes.create_string_buffer(olen + 1)
    rc = fn(bytes(stream), ctypes.c_size_t(len(stream)), out, ctypes.c_size_t(olen))
    return rc, out.raw[:olen]


def oracle_frame(oracle, frame, nbytes):
    out = ctypes.create_string_buffer(nbytes)
    rc = oracle.lib().pbxo_zarr_decode_chunk(1, frame, ctypes.c_size_t(len(frame)), out, ctypes.c_size_t(nbytes))
    return rc, out.raw


_lz4 = None


def liblz4_decode(stream, olen):
    """LZ4_decompress_safe: the bytes, or its negative return value."""
    global _lz4
    if _lz4 is None:
        _lz4 = ctypes.CDLL("liblz4.so.1")
        _lz4.LZ4_decompress_safe.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    out = ctypes.create_string_buffer(olen)
    n = _lz4.LZ4_decompress_safe(bytes(stream), out, len(stream), olen)
    return out.raw if n == olen else n


def need_cblosc():
    if _zarr.cblosc() is None:
        pytest.skip("c-blosc 1.21 library not in this image")


def test_kernel_constants_are_the_sources():
    text = "".join(open(os.path.join(CSRC, f)).read() for f in ("kernels_zarr.hip", "zarr_dev.h"))
    for name, value in C.KERNEL_CONSTANTS.items():
        assert re.findall(r"constexpr uint32_t %s = (\d+);" % name, text) == [str(value)], name
    # the constants the kernels spell as literals, where the model reads them
    for snippet in ("if (ip + 64 + 20 > win.base + ZWIN)", "ml + 4 <= 256 && lln <= 256 &&",
                    "ls + lln + 24 <= win.base + ZWIN", "mt && s_off > RING - 64", "if (off > ZR) {",
                    "k < len; k += 1024", "s_waitcnt(0xF78);  // vmcnt(8)", "while (upto - f >= 256u)",
                    "if (q - base > ZWIN - 64) load(q);", "while (p < 64 && cnt < cap)",
                    "if (ip < ilen && (ip < win.base || ip + 84 > win.base + ZWIN)) win.load(ip);"):
        assert snippet in text, snippet
    assert (F.TOP_MARGIN, F.JOIN_MAX, F.JOIN_TAIL, F.BATCH_SPLIT, F.MATCH_SPLIT, F.FAR_CHUNK, F.VMCNT, F.CAND) == \
        (84, 256, 24, F.ZR_LZ4 - 64, F.ZR_LZ4, 1024, 8, 64)


# ------------------------------------------------------------------------------------- LZ4
def check_lz4(oracle, name, c):
    n = len(c.content)
    assert 0 < len(c.stream) < n
    assert F.lz4_decode(c.stream, n) == c.content
    assert oracle_stream(oracle, F.LZ4, c.stream, n) == (0, c.content)
    got = liblz4_decode(c.stream, n)
    if name in C.LZ4_ORACLE_ONLY:
        assert isinstance(got, int) and got < 0, "liblz4 decodes an oracle-only case"
    else:
        assert got == c.content, "liblz4: %r" % (got if isinstance(got, int) else "other bytes")


@pytest.mark.parametrize("name", C.lz4_small_names())
def test_lz4_stream_decodes_under_the_reference_the_oracle_and_liblz4(oracle, name):
    check_lz4(oracle, name, C.lz4_cases()[name])


def test_lz4_prefix_sweep_decodes(oracle):
    for k in C.PREFIXES:
        name = "top_reload_prefix_%02d" % k
        check_lz4(oracle, name, C.lz4_cases()[name])


@pytest.mark.parametrize("path", C.LZ4_PATHS)
@pytest.mark.parametrize("off", F.LZ4_RING_OFFS)
def test_lz4_ring_boundary_streams_decode(oracle, off, path):
    for name, c in C.lz4_phases(off, path).items():
        assert len(c.content) == C.lz4_phase_length(off)
        check_lz4(oracle, name, c)


def test_the_oracle_only_list_is_exactly_what_liblz4_refuses():
    """Only end-rule violators; every other case passed the library above."""
    refused = {n for n, c in C.lz4_cases().items() if isinstance(liblz4_decode(c.stream, len(c.content)), int)}
    assert refused == set(C.LZ4_ORACLE_ONLY)
    assert all("final_sequence" in n for n in C.LZ4_ORACLE_ONLY)


def test_lz4_censuses_cover_the_whole_checklist():
    seen = set().union(*(c.census for c in C.lz4_cases().values()))
    missing = [item for item in C.LZ4_CHECKLIST if item not in seen]
    assert not missing, missing
    assert len(set(C.LZ4_CHECKLIST)) == len(C.LZ4_CHECKLIST)
    causes = sum((c.counts for c in C.lz4_cases().values()), F.Counter())
    assert all(causes["batch_exec:" + k] > 0 for k in C.LZ4_CAUSES), causes
    assert all(causes[k] > 0 for k in ("round", "fast", "join", "perseq", "reload", "flush", "batch:ring",
                                       "batch:same_step", "outring:ring", "outring:hbm")), causes


def test_lz4_phase_censuses_cover_every_distance_path_and_phase():
    seen = set()
    for off in F.LZ4_RING_OFFS:
        for path in C.LZ4_PATHS:
            for c in C.lz4_phases(off, path).values():
                seen |= c.census
                assert c.counts["batch:hbm" if path == "batch" else "outring:hbm"] == \
                    (off > (F.BATCH_SPLIT if path == "batch" else F.MATCH_SPLIT))
    missing = [item for item in C.LZ4_PHASE_CHECKLIST if item not in seen]
    assert not missing, missing


def test_every_hbm_source_of_the_model_lies_behind_the_vmcnt_wait():
    """The model refuses (asserts) a source that is not flushed; here: at least VMCNT vector-memory
    operations follow the store that flushed it, in every case, and the tightest case has 11."""
    gaps = []
    groups = [C.lz4_cases(), C.blz_cases()] + [C.lz4_phases(o, p) for o in F.LZ4_RING_OFFS for p in C.LZ4_PATHS] + \
        [C.blz_phases(d) for d in F.BLZ_RING_DISTS]
    for g in groups:
        for c in g.values():
            gaps += [int(i.rsplit(":", 1)[1]) for i in c.census if i.startswith("hbm:min_vm_ops")]
    assert gaps and min(gaps) == 11 and min(gaps) >= F.VMCNT
    c = C.lz4_cases()["far_match_of_1024_at_4097_eleven_stores_after_its_source"]
    assert "hbm:min_vm_ops_since_source_flush:11" in c.census


def test_the_prefix_sweep_meets_every_phase_of_the_top_reload():
    seen = set()
    for k in C.PREFIXES:
        seen |= {i for i in C.lz4_cases()["top_reload_prefix_%02d" % k].census if i.startswith("top_reload:")}
    assert seen >= {"top_reload:%d:pending" % v for v in range(F.ZWIN - F.TOP_MARGIN + 1, F.ZWIN - F.TOP_MARGIN + 65)}


@pytest.mark.parametrize("name", list(C.lz4_malformed()))
def test_lz4_malformed_stream(oracle, name):
    stream, n, code, guard, path = C.lz4_malformed()[name]
    assert 0 < len(stream) < n
    got, census, counts = F.lz4_schedule(stream, n)
    assert got == code, "the model ends with code %d" % got
    if name in C.LZ4_MALFORMED_PATHS:
        key, value = C.LZ4_MALFORMED_PATHS[name]
        assert counts[key] == value, counts
    with pytest.raises(F.Malformed):
        F.lz4_decode(stream, n)
    assert oracle_stream(oracle, F.LZ4, stream, n)[0] != 0
    assert isinstance(liblz4_decode(stream, n), int)


def test_lz4_malformed_cases_name_every_code():
    assert {v[2] for v in C.lz4_malformed().values()} == set(range(1, 8))


# --------------------------------------------------------------------------------- BloscLZ
def check_blz(oracle, c):
    n = len(c.content)
    assert 0 < len(c.stream) < n
    assert F.blosclz_decode(c.stream, n) == c.content
    assert oracle_stream(oracle, F.BLOSCLZ, c.stream, n) == (0, c.content)


@pytest.mark.parametrize("name", list(C.blz_cases()))
def test_blosclz_stream_decodes_under_the_reference_the_oracle_and_cblosc(oracle, name):
    c = C.blz_cases()[name]
    check_blz(oracle, c)
    need_cblosc()
    n = len(c.content)
    assert _zarr.cblosc_decode(F.blosc_frame([c.stream], n, F.BLOSCLZ), n) == c.content


@pytest.mark.parametrize("dist", F.BLZ_RING_DISTS)
def test_blosclz_ring_boundary_streams_decode(oracle, dist):
    cases = C.blz_phases(dist)
    for c in cases.values():
        check_blz(oracle, c)
    need_cblosc()
    frame, content = frame_of(cases, F.BLOSCLZ)
    assert _zarr.cblosc_decode(frame, len(content)) == content


def test_blosclz_censuses_cover_the_whole_checklist():
    seen = set().union(*(c.census for c in C.blz_cases().values()))
    missing = [item for item in C.BLZ_CHECKLIST if item not in seen]
    assert not missing, missing
    seen = set().union(*(c.census for d in F.BLZ_RING_DISTS for c in C.blz_phases(d).values()))
    missing = [item for item in C.BLZ_PHASE_CHECKLIST if item not in seen]
    assert not missing, missing
    for d in F.BLZ_RING_DISTS:
        assert all(c.counts["match:hbm"] == (d > F.MATCH_SPLIT) for c in C.blz_phases(d).values())


@pytest.mark.parametrize("name", list(C.blz_malformed()))
def test_blosclz_malformed_stream(oracle, name):
    stream, n, code, guard = C.blz_malformed()[name]
    assert 0 < len(stream) < n
    assert F.blosclz_schedule(stream, n)[0] == code
    with pytest.raises(F.Malformed):
        F.blosclz_decode(stream, n)
    assert oracle_stream(oracle, F.BLOSCLZ, stream, n)[0] != 0
    need_cblosc()
    out = ctypes.create_string_buffer(n)
    assert _zarr.cblosc().blosc_decompress_ctx(F.blosc_frame([stream], n, F.BLOSCLZ), out, n, 1) != n


def test_blosclz_malformed_cases_name_every_reachable_code():
    """1 (an empty split) is refused by the planner and 6 lies behind the guard of 5: _lz_cases.py."""
    assert {v[2] for v in C.blz_malformed().values()} == {2, 3, 4, 5, 7, 8}


# ---------------------------------------------------------------------------------- frames
def frame_of(cases, codec, **kw):
    """One frame of all the cases (equal lengths), streams at unaligned offsets; its content."""
    cases = list(cases.values())
    n = len(cases[0].content)
    gaps = [(3 * k + 1) % 7 for k in range(len(cases))]
    return F.blosc_frame([c.stream for c in cases], n, codec, gaps=gaps, **kw), b"".join(c.content for c in cases)


def by_length(cases):
    out = {}
    for name, c in cases.items():
        out.setdefault(len(c.content), {})[name] = c
    return out


@pytest.mark.parametrize("codec", [F.LZ4, F.BLOSCLZ], ids=["lz4", "blosclz"])
def test_frames_decode_under_the_oracle_and_cblosc(oracle, codec):
    cases = C.lz4_cases() if codec == F.LZ4 else C.blz_cases()
    groups = by_length(cases)
    assert set(groups) == (set(C.A_LENGTHS) | {C.B} if codec == F.LZ4 else {C.A, C.B})
    for n, group in groups.items():
        frame, content = frame_of(group, codec)
        assert oracle_frame(oracle, frame, len(content)) == (0, content)
        if _zarr.cblosc() is not None:  # (c-blosc decodes LZ4 with liblz4: without the oracle-only cases)
            frame, content = frame_of({k: c for k, c in group.items() if k not in C.LZ4_ORACLE_ONLY}, codec)
            assert _zarr.cblosc_decode(frame, len(content)) == content


def test_shuffled_frames_decode_under_the_oracle_and_cblosc(oracle):
    """typesize 2 with the byte-shuffle bit: the streams' bytes are the shuffled block."""
    for codec, cases in ((F.LZ4, C.lz4_cases()), (F.BLOSCLZ, C.blz_cases())):
        frame, content = frame_of(by_length(cases)[C.A], codec, typesize=2, shuffle=True)
        rc, out = oracle_frame(oracle, frame, len(content))
        assert rc == 0 and out != content and sorted(out[:C.A]) == sorted(content[:C.A])
        if _zarr.cblosc() is not None and codec == F.BLOSCLZ:
            assert _zarr.cblosc_decode(frame, len(content)) == out
