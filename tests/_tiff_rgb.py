"""What the multi-sample (RGB, RGBA, ...) TIFF tests add to tests/_tiff_src.py: the forward
horizontal predictor with a stride of S samples (TIFF 6.0 section 14: a sample is differenced
against the same component of the pixel before), segment builders for chunky
(PlanarConfiguration 1) and planar (PlanarConfiguration 2) strips and tiles, and a page writer
that emits S BitsPerSample / SampleFormat values and tags 262 / 284 / 338.  Arrays are
(rows, width, S) in the file's byte order.  Independent of the library under test; pinned by
tests/test_tiff_rgb_host.py against libtiff (through PIL)."""
import numpy as np

import _tiff_src as T
from _tiff_src import compress, lzw_encode  # noqa: F401  (re-exported for the tests)


def predict2s(a):
    """Forward Predictor = 2 of a (rows, width, S) integer array: every sample minus the same
    component of the pixel to its left, modulo 2^bits.  Same dtype (byte order kept)."""
    a = np.ascontiguousarray(a)
    native = a.astype(a.dtype.newbyteorder("="))
    u = native.view(np.dtype("u%d" % native.dtype.itemsize))
    d = u.copy()
    d[:, 1:, :] = u[:, 1:, :] - u[:, :-1, :]
    return d.view(native.dtype).astype(a.dtype)


def _pieces(a, tile, rows_per_strip):
    """The (rows, width, S) pieces of a: tiles (edge tiles zero-padded) or strips."""
    h, w, s = a.shape
    if tile:
        tw, th = tile
        for y in range(0, h, th):
            for x in range(0, w, tw):
                t = np.zeros((th, tw, s), a.dtype)
                p = a[y:y + th, x:x + tw]
                t[:p.shape[0], :p.shape[1]] = p
                yield t
    else:
        rps = rows_per_strip or h
        for y in range(0, h, rps):
            yield a[y:y + rps]


def chunky_segments(a, tile=None, rows_per_strip=None, predictor=1):
    """Uncompressed PlanarConfiguration = 1 segments of a (rows, width, S) array: every pixel's
    S samples side by side."""
    a = np.ascontiguousarray(a)
    return [(predict2s(p) if predictor == 2 else np.ascontiguousarray(p)).tobytes()
            for p in _pieces(a, tile, rows_per_strip)]


def planar_segments(a, tile=None, rows_per_strip=None, predictor=1):
    """Uncompressed PlanarConfiguration = 2 segments: S groups, one per sample, each the
    single-sample segments of that component (tests/_tiff_src.segments_of)."""
    a = np.ascontiguousarray(a)
    segs = []
    for s in range(a.shape[2]):
        segs += T.segments_of(np.ascontiguousarray(a[:, :, s]), tile, rows_per_strip, predictor)
    return segs


def page_of(a, compression=1, predictor=1, tile=None, rows_per_strip=None, planar=1, photometric=None,
            extrasamples=None, description=None, subifds=(), extra=(), **lzw_knobs):
    """A page dict for write_tiff from a (rows, width, S) array (its dtype's byte order must be
    the file's).  photometric defaults to 2 (RGB) for S >= 3 and 1 otherwise; samples past the
    photometric's own (3 for RGB, 1 for grey) are declared ExtraSamples = 0 (unspecified) unless
    `extrasamples` (a list) says otherwise."""
    a = np.ascontiguousarray(a)
    h, w, s = a.shape
    build = planar_segments if planar == 2 else chunky_segments
    segs = [compress(x, compression, **lzw_knobs) for x in build(a, tile, rows_per_strip, predictor)]
    if photometric is None:
        photometric = 2 if s >= 3 else 1
    if extrasamples is None:
        extrasamples = [0] * (s - (3 if photometric == 2 else 1))
    return dict(width=w, length=h, bits=a.dtype.itemsize * 8, sampleformat=T._SF[a.dtype.kind], spp=s,
                compression=compression, predictor=predictor, tile=tile, rows_per_strip=rows_per_strip or h,
                segments=segs, planar=planar, photometric=photometric, extrasamples=list(extrasamples),
                description=description, subifds=[_finish(p) for p in subifds], extra=list(extra))


def _finish(page):
    """The page as tests/_tiff_src.write_tiff takes it: that writer emits one BitsPerSample, one
    SampleFormat and Photometric = 1, so those three tags are replaced through `extra` (a tag
    written twice would be malformed: _write drops the base writer's entry of every such pair)."""
    if page.get("_finished"):
        return page
    s = page["spp"]
    extra = [(258, 3, [page["bits"]] * s), (339, 3, [page["sampleformat"]] * s), (262, 3, [page["photometric"]]),
             (284, 3, [page["planar"]])]
    if page["extrasamples"]:
        extra.append((338, 3, list(page["extrasamples"])))
    own = {t[0] for t in page["extra"]}  # a test's own entry for one of these tags stands
    return dict(page, extra=list(page["extra"]) + [t for t in extra if t[0] not in own], _finished=True)


def write_tiff(path, pages, byteorder="<", bigtiff=False):
    """tests/_tiff_src.write_tiff for pages of page_of(): S BitsPerSample / SampleFormat values,
    PhotometricInterpretation, PlanarConfiguration and ExtraSamples.  Returns the file's bytes."""
    return _write(path, [_finish(p) for p in pages], byteorder, bigtiff)


def _write(path, pages, byteorder, bigtiff):
    # _tiff_src.write_tiff writes tags 258, 262 and 339 itself; pages that carry their own in
    # `extra` get them instead.  The IFD is rebuilt from that writer's bytes: entries are sorted
    # by tag and the FIRST of two equal tags is the base writer's, which is dropped.
    import struct
    raw = bytearray(T.write_tiff(None, pages, byteorder, bigtiff))
    bo = byteorder
    cnt_fmt, cnt_sz, ent_sz, off_fmt, off_sz = ("Q", 8, 20, "Q", 8) if bigtiff else ("H", 2, 12, "I", 4)

    def fix(at):
        """Drop the first of every pair of equal tags of the IFD at `at` (in place: the IFD
        shrinks, the next-IFD pointer moves up, the bytes left over are never referenced).
        Returns the offset of the next IFD."""
        n = struct.unpack_from(bo + cnt_fmt, raw, at)[0]
        ents = [bytes(raw[at + cnt_sz + k * ent_sz:at + cnt_sz + (k + 1) * ent_sz]) for k in range(n)]
        nxt = bytes(raw[at + cnt_sz + n * ent_sz:at + cnt_sz + n * ent_sz + off_sz])
        tags = [struct.unpack(bo + "H", e[:2])[0] for e in ents]
        keep = [e for k, e in enumerate(ents) if not (k + 1 < n and tags[k + 1] == tags[k])]
        for e in keep:
            if struct.unpack(bo + "H", e[:2])[0] == 330:  # SubIFDs: fix them too
                cnt = struct.unpack(bo + off_fmt, e[4:4 + off_sz])[0]
                styp = struct.unpack(bo + "H", e[2:4])[0]
                ssz = 8 if styp == 18 else 4
                field = e[4 + off_sz:]
                data = field[:ssz * cnt] if ssz * cnt <= off_sz else \
                    bytes(raw[struct.unpack(bo + off_fmt, field)[0]:struct.unpack(bo + off_fmt, field)[0] + ssz * cnt])
                for so in struct.unpack(bo + ("Q" if ssz == 8 else "I") * cnt, data):
                    fix(so)
        struct.pack_into(bo + cnt_fmt, raw, at, len(keep))
        p = at + cnt_sz
        for e in keep:
            raw[p:p + ent_sz] = e
            p += ent_sz
        raw[p:p + off_sz] = nxt
        return struct.unpack(bo + off_fmt, nxt)[0]

    off = struct.unpack_from(bo + off_fmt, raw, 8 if bigtiff else 4)[0]
    while off:
        off = fix(off)
    if path is not None:
        with open(path, "wb") as f:
            f.write(raw)
    return bytes(raw)
