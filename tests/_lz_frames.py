"""Byte-exact writers for LZ4 blocks and BloscLZ streams (pure Python; no library encoder), plain
reference decoders that restate the oracle's (oracle/zarr_oracle.c: pbxo_lz4_decode,
pbxo_blosclz_decode), the c-blosc 1.x frame that carries one stream per block, and a MODEL of the
schedule k_zarr_lz4 / k_zarr_blosclz (csrc/kernels_zarr.hip, csrc/zarr_dev.h) take over a stream:
rounds, batch executions by cause, window reloads, ring / HBM match sources, flushes.  The model is
read off the kernel source and shares no code with the reference decoders: it never produces a
byte.  A writer executes its own sequences and so knows the content.
tests/test_lz_frames_host.py checks all of it against the oracle, liblz4 and c-blosc."""
from collections import Counter, namedtuple

# the kernels' constants (test_lz_frames_host.py compares them with the sources)
ZWIN = 1024       # input window, bytes
ZR_LZ4 = 4096     # output ring, bytes
CAND = 64         # candidate starts of a round = batch entries = lanes
TOP_MARGIN = 84   # the loop top reloads the window when ip + 84 passes its end
JOIN_MAX = 256    # a serial sequence joins the batch when literals and match are <= 256 each
JOIN_TAIL = 24    # ... and ls + lln + 24 stays inside the window
FAR_CHUNK = 1024  # OutRing::match reads HBM 1 KiB a round trip
BATCH_SPLIT = ZR_LZ4 - 64   # seq_batch: off > 4032 reads HBM
MATCH_SPLIT = ZR_LZ4        # OutRing::match: off > 4096 reads HBM
VMCNT = 8         # the far paths wait for all but the last 8 vector-memory operations

LZ4_RING_OFFS = (4031, 4032, 4033, 4095, 4096, 4097, 65535)
BLZ_RING_DISTS = (4095, 4096, 4097)
BLZ_MAX_NEAR = 8191          # 13-bit distances: 1 .. 8191; 8192 and up take the far form
BLZ_FAR_BASE = 8192


class Malformed(Exception):
    pass


# ------------------------------------------------------------------------------ LZ4 writer
Seq = namedtuple("Seq", "lit off ml ll_ext ml_ext")
Fill = namedtuple("Fill", "lit off")


def S(lit=b"", off=None, ml=None, ll_ext=None, ml_ext=None):
    """One LZ4 sequence: literals, then (off, ml) or nothing (the final sequence).  ll_ext / ml_ext:
    the extension bytes to write instead of the canonical ones."""
    return Seq(bytes(lit), off, ml, ll_ext, ml_ext)


def ext_bytes(n):
    """The canonical 255-terminated extension of n >= 0."""
    return [255] * (n // 255) + [n % 255]


def lz4_seq_bytes(s):
    ll = len(s.lit)
    lext = s.ll_ext if s.ll_ext is not None else (ext_bytes(ll - 15) if ll >= 15 else [])
    if s.off is None:
        return bytes([min(ll, 15) << 4] + list(lext)) + s.lit
    m = s.ml - 4
    assert m >= 0
    mext = s.ml_ext if s.ml_ext is not None else (ext_bytes(m - 15) if m >= 15 else [])
    return bytes([min(ll, 15) << 4 | min(m, 15)] + list(lext)) + s.lit + bytes([s.off & 255, s.off >> 8]) + bytes(mext)


def _copy(out, dist, length):
    assert 1 <= dist <= len(out), "distance %d at %d" % (dist, len(out))
    if dist >= length:
        out += out[len(out) - dist:len(out) - dist + length]
    else:
        seg = bytes(out[len(out) - dist:])
        out += (seg * (length // dist + 1))[:length]


def lz4_build(seqs, length=None):
    """(stream, content) of a list of S(...) and at most one Fill(lit, off): a sequence whose match
    is as long as it takes for the content to be `length` bytes."""
    seqs = list(seqs)
    fills = [i for i, s in enumerate(seqs) if isinstance(s, Fill)]
    if fills:
        i, = fills
        rest = sum(len(s.lit) + (s.ml or 0) for k, s in enumerate(seqs) if k != i)
        need = length - rest - len(seqs[i].lit)
        assert need >= 4, "no room for the fill match (%d)" % need
        seqs[i] = S(seqs[i].lit, seqs[i].off, need)
    out, stream = bytearray(), bytearray()
    for s in seqs:
        stream += lz4_seq_bytes(s)
        out += s.lit
        if s.off is not None:
            _copy(out, s.off, s.ml)
    assert length is None or len(out) == length, (len(out), length)
    return bytes(stream), bytes(out)


# -------------------------------------------------------------------------- BloscLZ writer
BL = namedtuple("BL", "lit level")
BM = namedtuple("BM", "len dist ext")
BFill = namedtuple("BFill", "dist")


def L(lit, level=0):
    """A literal run of 1..32 bytes; `level` goes into the top three bits of the control byte
    (read as the compression level in a stream's first byte, which the decoders mask off)."""
    assert 1 <= len(lit) <= 32
    return BL(bytes(lit), level)


def M(length, dist, ext=None):
    """A match of >= 3 bytes; ext: the length-extension bytes instead of the canonical ones."""
    return BM(length, dist, ext)


def blz_op_bytes(o, first=False):
    if isinstance(o, BL):
        assert first or o.level == 0
        return bytes([o.level << 5 | (len(o.lit) - 1)]) + o.lit
    assert not first, "a stream begins with a literal run"
    assert o.len >= 3 and 1 <= o.dist <= BLZ_FAR_BASE + 65535
    far = o.dist > BLZ_MAX_NEAR  # 8192 = (31 << 8 | 255) + 1 is the far marker: far form, field 0
    d = 31 << 8 | 255 if far else o.dist - 1
    n = o.len - 2
    out = [min(n, 7) << 5 | d >> 8]
    if n >= 7:
        out += o.ext if o.ext is not None else ext_bytes(n - 7)
    out.append(d & 255)
    if far:
        out += [(o.dist - BLZ_FAR_BASE) >> 8, (o.dist - BLZ_FAR_BASE) & 255]
    return bytes(out)


def blz_build(ops, length=None):
    """(stream, content) of a list of L(...) / M(...) and at most one BFill(dist)."""
    ops = list(ops)
    fills = [i for i, o in enumerate(ops) if isinstance(o, BFill)]
    if fills:
        i, = fills
        rest = sum(len(o.lit) if isinstance(o, BL) else o.len for k, o in enumerate(ops) if k != i)
        assert length - rest >= 3, "no room for the fill match"
        ops[i] = M(length - rest, ops[i].dist)
    out, stream = bytearray(), bytearray()
    for k, o in enumerate(ops):
        stream += blz_op_bytes(o, k == 0)
        if isinstance(o, BL):
            out += o.lit
        else:
            _copy(out, o.dist, o.len)
    assert length is None or len(out) == length, (len(out), length)
    return bytes(stream), bytes(out)


# ---------------------------------------------------------------------- reference decoders
def lz4_decode(stream, olen):
    """pbxo_lz4_decode in Python: the bytes, or Malformed."""
    d, n, ip, out = bytes(stream), len(stream), 0, bytearray()
    while True:
        if ip >= n:
            raise Malformed("input ends where a token should be")
        tok = d[ip]
        ip += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                if ip >= n:
                    raise Malformed("literal extension cut")
                b = d[ip]
                ip += 1
                ll += b
                if b != 255:
                    break
        if ip + ll > n or len(out) + ll > olen:
            raise Malformed("literals past the input or the output")
        out += d[ip:ip + ll]
        ip += ll
        if ip == n:
            break
        if ip + 2 > n:
            raise Malformed("offset cut")
        off = d[ip] | d[ip + 1] << 8
        ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                if ip >= n:
                    raise Malformed("match extension cut")
                b = d[ip]
                ip += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        if off == 0 or off > len(out) or len(out) + ml > olen:
            raise Malformed("match outside the output")
        for _ in range(ml):
            out.append(out[-off])
    if len(out) != olen:
        raise Malformed("output short")
    return bytes(out)


def blosclz_decode(stream, olen):
    """pbxo_blosclz_decode in Python: the bytes, or Malformed."""
    d, n, out = bytes(stream), len(stream), bytearray()
    if n == 0:
        raise Malformed("empty")
    ctrl, ip = d[0] & 31, 1
    while True:
        if ctrl >= 32:
            ln, ofs = (ctrl >> 5) - 1, (ctrl & 31) << 8
            if ln == 6:
                while True:
                    if ip + 1 >= n:
                        raise Malformed("length extension cut")
                    code = d[ip]
                    ip += 1
                    ln += code
                    if code != 255:
                        break
            elif ip + 1 >= n:
                raise Malformed("distance byte cut")
            code = d[ip]
            ip += 1
            ln += 3
            dist = ofs + code + 1
            if code == 255 and ofs == 31 << 8:
                if ip + 1 >= n:
                    raise Malformed("far distance cut")
                dist = (d[ip] << 8 | d[ip + 1]) + BLZ_FAR_BASE
                ip += 2
            if len(out) + ln > olen or dist > len(out):
                raise Malformed("match outside the output")
            if ip >= n:
                break  # parsed, not copied
            ctrl = d[ip]
            ip += 1
            for _ in range(ln):
                out.append(out[-dist])
        else:
            k = ctrl + 1
            if len(out) + k > olen or ip + k > n:
                raise Malformed("literals past the input or the output")
            out += d[ip:ip + k]
            ip += k
            if ip >= n:
                break
            ctrl = d[ip]
            ip += 1
    if len(out) != olen:
        raise Malformed("output short")
    return bytes(out)


# ------------------------------------------------------------------------------- container
LZ4, BLOSCLZ = 1, 0  # c-blosc codec numbers (flags bits 5..7)


def blosc_frame(streams, length, codec, gaps=None, typesize=1, shuffle=False, check=True):
    """A c-blosc 1.x frame of len(streams) blocks of `length` bytes, one stream each (flags: don't
    split); gaps[k] bytes of filler lie before block k's size field, so block starts, and with
    them the streams, sit at chosen unaligned offsets.  A stream as long as its block would read as
    stored and a longer one is refused by the frame rule: every stream is strictly shorter."""
    n = len(streams)
    gaps = gaps or [0] * n
    flags = codec << 5 | 0x10 | (1 if shuffle else 0)
    body, starts = bytearray(), []
    for s, g in zip(streams, gaps):
        assert not check or 0 < len(s) < length, "stream of %d bytes for %d" % (len(s), length)
        body += b"\xee" * g
        starts.append(16 + 4 * n + len(body))
        body += len(s).to_bytes(4, "little") + s
    cbytes = 16 + 4 * n + len(body)
    return bytes([2, 1, flags, typesize]) + (n * length).to_bytes(4, "little") + length.to_bytes(4, "little") + \
        cbytes.to_bytes(4, "little") + b"".join(x.to_bytes(4, "little") for x in starts) + bytes(body)


# ---------------------------------------------------- the model: OutRing and the VM queue
class _Ring:
    """OutRing's bookkeeping: op, flushed, one flush store per completed 256-byte run, and the
    order of vector-memory operations (flush stores, HBM loads), from which the far paths'
    vmcnt(8) argument is checked: an HBM source must lie under `flushed`, and at least VMCNT
    operations must have been issued after the store that flushed its last byte."""

    def __init__(self, olen, cen, cnt):
        self.op, self.flushed, self.olen, self.vm = 0, 0, olen, 0
        self.store_no, self.cen, self.cnt, self.min_gap = {}, cen, cnt, None

    def flush(self, upto):
        while upto - self.flushed >= 256:
            self.store_no[self.flushed >> 8] = self.vm
            self.vm += 1
            self.flushed += 256
            self.cnt["flush"] += 1

    def hbm_load(self, last_byte):
        """One HBM load whose needed bytes end at `last_byte` (inclusive)."""
        assert last_byte < self.flushed, "HBM source %d not flushed (%d)" % (last_byte, self.flushed)
        gap = self.vm - self.store_no[last_byte >> 8] - 1
        self.min_gap = gap if self.min_gap is None else min(self.min_gap, gap)
        self.vm += 1

    def match(self, off, length, tag):
        """OutRing::match; False where it refuses."""
        if off == 0 or off > self.op or length > self.olen - self.op:
            return False
        cen, op = self.cen, self.op
        if off < 64:
            cen.add("%s:period:%d" % (tag, off))
            if length > 64:
                cen.add("%s:period:%d:len>64" % (tag, off))
        if off > MATCH_SPLIT:
            src = "hbm"
            chunks = 0
            for k in range(0, length, FAR_CHUNK):
                n = min(length - k, FAR_CHUNK)
                self.hbm_load(op + k - off + n - 1)
                self.flush(op + k + n)
                chunks += 1
            self.cnt[tag + ":hbm"] += 1
            if chunks > 1:
                cen.add("%s:far:chunks>1" % tag)
            if length > 1024:
                cen.add("%s:len>1024:far" % tag)
        else:
            src = "ring"
            for k in range(0, length, 64):
                self.flush(op + k + min(length - k, 64))
            self.cnt[tag + ":ring"] += 1
            if length > 1024:
                cen.add("%s:len>1024:near" % tag)
        cen.add("%s:off:%d:src:%s" % (tag, off, src))
        cen.add("%s:off:%d:phase:%d" % (tag, off, op & 63))
        cen.add("%s:off:%d:flushphase:%d" % (tag, off, op & 255))
        self.op += length
        return True

    def literals(self, n):
        for c in range(0, n, 64):
            self.flush(self.op + c + min(n - c, 64))
        self.op += n


def _gap_item(ring, cen):
    if ring.min_gap is not None:
        cen.add("hbm:min_vm_ops_since_source_flush:%d" % ring.min_gap)


# ------------------------------------------------------------- the model: k_zarr_lz4
def lz4_schedule(stream, olen):
    """(code, census, counts): the decoder code k_zarr_lz4 ends with, the set of paths taken and
    how often.  A transliteration of the kernel's loop (window base, ip, the pending batch, op,
    flushed) that copies nothing."""
    d, ilen = bytes(stream) + bytes(4096), len(stream)
    cen, cnt = set(), Counter()
    o = _Ring(olen, cen, cnt)
    batch = []  # (ll, ml, off): the pending batch
    w = dict(base=0)
    ip, bad = 0, 0
    seen_lane = None  # the lane at which the last fast round's walk stopped on this ip

    def reload(q, why):
        w["base"] = q
        cnt["reload"] += 1
        cen.add("reload:" + why)

    def exec_batch(cause):
        if not batch:
            return True
        cnt["batch_exec:" + cause] += 1
        cen.add("batch_exec:%s:of:%d" % (cause, len(batch)))
        op0, T = o.op, sum(ll + ml for ll, ml, _ in batch)
        ok = T <= olen - op0
        st = 0
        for ll, ml, off in batch:
            if off == 0 or off > op0 + st + ll:
                ok = False
            st += ll + ml
        if not ok:
            del batch[:]
            return False
        # byte p of the batch: its sequence, whether a literal, and a match byte's source
        owner, st = [], 0
        starts = []
        for j, (ll, ml, off) in enumerate(batch):
            starts.append(st)
            owner += [j] * (ll + ml)
            st += ll + ml
        kinds = [set() for _ in batch]
        for cb in range(0, T, 64):
            n = min(64, T - cb)
            pend, ptr, far_last = [False] * 64, [0] * 64, None
            for k in range(n):
                p = cb + k
                j = owner[p]
                ll, ml, off = batch[j]
                r = p - starts[j]
                if r < ll:
                    continue
                rm = r - ll
                if off < 64 and rm in (0, 63, 64, 65, 127, 128, 255):
                    cen.add("batch:period:%d:rm:%d" % (off, rm))
                rep = rm % off if off < 64 else rm
                src = starts[j] + ll + rep - off  # from op0
                if off > BATCH_SPLIT:
                    kinds[j].add("hbm")
                    far_last = max(far_last or 0, op0 + src)
                elif src >= cb:
                    kinds[j].add("same_step")
                    pend[k], ptr[k] = True, src - cb
                    assert ptr[k] < k
                    if off < ml:
                        cen.add("batch:same_step:overlapping")
                else:
                    kinds[j].add("ring")
                    assert op0 + src >= op0 + cb + 64 - ZR_LZ4
            if far_last is not None:
                o.hbm_load(far_last)
            iters = 0
            while any(pend):  # pointer jumping
                iters += 1
                np_, nq = [pend[ptr[k]] for k in range(64)], [ptr[ptr[k]] for k in range(64)]
                for k in range(64):
                    if pend[k] and np_[k]:
                        ptr[k] = nq[k]
                    else:
                        pend[k] = False
            if iters:
                cen.add("batch:jump_iterations:%d" % iters)
            o.flush(op0 + (T if T - cb < 64 else cb + 64))
        for j, (ll, ml, off) in enumerate(batch):
            at = op0 + starts[j] + ll
            for kd in kinds[j]:
                cnt["batch:" + kd] += 1
                cen.add("batch:off:%d:src:%s" % (off, kd))
            if off <= 64:
                cen.add("batch:off:%d:len:%d" % (off, ml))
            if off in LZ4_RING_OFFS:
                cen.add("batch:off:%d:phase:%d" % (off, (starts[j] + ll) & 63))
                cen.add("batch:off:%d:flushphase:%d" % (off, at & 255))
        o.op = op0 + T
        del batch[:]
        return True

    while True:
        if ip >= ilen:
            bad = 1
            break
        base = w["base"]
        if ip + TOP_MARGIN > base + ZWIN:
            if batch:
                cen.add("top_reload:%d:pending" % (ip - base))
            if not exec_batch("reload_top"):
                bad = 6
                break
            reload(ip, "top")
        # the 64 candidates and the walk
        def cand(k):
            q = ip + k
            tok = d[q]
            ll, ml0 = tok >> 4, tok & 15
            ok = ll < 15 and ml0 < 15 and q + 3 + ll <= ilen and q + 1 + ll != ilen
            return ok, k + 3 + ll, ll, ml0 + 4, d[q + 1 + ll] | d[q + 2 + ll] << 8
        p, got, cap = 0, [], CAND - len(batch)
        stop = None
        while p < 64 and len(got) < cap:
            ok, nx, ll, ml, off = cand(p)
            if not ok:
                stop = p
                break
            got.append((ll, ml, off))
            p = nx
        if got:
            cnt["round"] += 1
            cnt["fast"] += len(got)
            for ll, ml, off in got:
                cen.add("ll:%d/ext0" % ll)
                cen.add("ml:%d/ext0" % ml)
            if p >= 64:
                cen.add("round:full:%d" % len(got))
            elif stop is not None:
                cen.add("walk_stop:long_successor")
            elif cand(p)[0]:
                cen.add("walk_stop:cap_cuts_the_walk")
            batch += got
            ip += p
            seen_lane = stop
            if len(batch) == CAND:
                cen.add("batch_full:fast")
                if not exec_batch("full"):
                    bad = 6
                    break
            continue
        # the serial parse
        cen.add("serial_at:" + ("first" if seen_lane is None else "last" if seen_lane == 63 else "middle"))
        seen_lane = None
        cnt["serial"] += 1
        state = dict(bad=0)

        def sbyte(q, field):
            if q - w["base"] > ZWIN - 1:
                if batch:
                    cen.add("sbyte_reload:%s:pending" % field)
                if not exec_batch("reload_sbyte"):
                    state["bad"] = 6
                reload(q, "sbyte:" + field)
            return d[q]
        t0 = sbyte(ip, "token")
        if state["bad"]:
            bad = 6
            break
        k, lln, nlext = 1, t0 >> 4, 0
        if lln == 15:
            while True:
                if ip + k >= ilen:
                    bad = 2
                    break
                b = sbyte(ip + k, "llext")
                k += 1
                nlext += 1
                lln += b
                if b != 255:
                    break
            if bad or state["bad"]:
                bad = bad or 6
                break
        ls = ip + k
        if lln > ilen - ls or lln > olen - o.op:
            bad = 3
            break
        final = ls + lln == ilen
        ml, off2, nmext = t0 & 15, 0, 0
        joined = False
        if not final:
            if ilen - (ls + lln) < 2:
                bad = 4
                break
            k += lln
            off2 = sbyte(ip + k, "off_lo") | sbyte(ip + k + 1, "off_hi") << 8
            k += 2
            if ml == 15:
                while True:
                    if ip + k >= ilen:
                        bad = 5
                        break
                    b = sbyte(ip + k, "mlext")
                    k += 1
                    nmext += 1
                    ml += b
                    if b != 255:
                        break
                if bad:
                    break
            if state["bad"]:
                bad = state["bad"]
                break
            cen.add("ll:%d/ext%d" % (lln, nlext))
            cen.add("ml:%d/ext%d" % (ml + 4, nmext))
            base = w["base"]
            fits = (ml + 4 <= JOIN_MAX, lln <= JOIN_MAX, ls >= base and ls + lln + JOIN_TAIL <= base + ZWIN)
            if all(fits):
                batch.append((lln, ml + 4, off2))
                cnt["join"] += 1
                cen.add("join:ll:%d" % lln)
                cen.add("join:ml:%d" % (ml + 4))
                ip += k
                if len(batch) == CAND:
                    cen.add("batch_full:join")
                    if not exec_batch("full"):
                        bad = 6
                        break
                joined = True
            elif fits == (True, False, True):
                cen.add("perseq:only_because:ll:%d" % lln)
            elif fits == (False, True, True):
                cen.add("perseq:only_because:ml:%d" % (ml + 4))
            elif fits[:2] == (True, True):
                cen.add("perseq:only_because:window")
        elif state["bad"]:
            bad = state["bad"]
            break
        if joined:
            continue
        if not exec_batch("before_copy"):
            bad = 6
            break
        if lln > olen - o.op:  # (the guard after the batch: see the kernel)
            bad = 3
            break
        cnt["perseq"] += 1
        for c in range(0, lln, 64):
            if (ls + c - w["base"]) % (1 << 32) > ZWIN - 64:
                reload(ls + c, "literals" if c == 0 else "literals_mid_run")
        o.literals(lln)
        if final:
            cen.add("end:final_ll:%s" % (lln if lln < 5 else ">=5"))
            if lln > 64:
                cen.add("end:final_ll:>64")
            if cnt["perseq"] == 1 and not cnt["fast"] and not cnt["join"]:
                cen.add("end:single_literal_sequence")
            ip = ilen
            break
        ip += k
        if not o.match(off2, ml + 4, "outring"):
            bad = 6
            break
        if ip < ilen and (ip < w["base"] or ip + TOP_MARGIN > w["base"] + ZWIN):
            reload(ip, "after_perseq")
    if not bad and o.op != olen:
        bad = 7
    if not bad:
        cen.add("end:olen_mod_256:%d" % (olen & 255))
    _gap_item(o, cen)
    return bad, frozenset(cen), cnt


# ---------------------------------------------------------- the model: k_zarr_blosclz
def blosclz_schedule(stream, olen):
    """(code, census, counts) of k_zarr_blosclz's serial parse."""
    d, ilen = bytes(stream) + bytes(4096), len(stream)
    cen, cnt = set(), Counter()
    o = _Ring(olen, cen, cnt)
    w = dict(base=0)

    def byte(q, field):
        if q - w["base"] > ZWIN - 1:
            w["base"] = q
            cnt["reload"] += 1
            cen.add("reload:" + field)
        return d[q]
    ip, bad = 0, 1 if ilen == 0 else 0
    ctrl = 0
    if not bad:
        cen.add("level:%d" % (d[0] >> 5))
        ctrl = byte(0, "ctrl") & 31
        ip = 1
    prev_lit = None
    while not bad:
        if ctrl >= 32:
            ln, ofs, next_ = (ctrl >> 5) - 1, (ctrl & 31) << 8, 0
            if ln == 6:
                while True:
                    if ip + 1 >= ilen:
                        bad = 2
                        break
                    code = byte(ip, "lenext")
                    ip += 1
                    next_ += 1
                    ln += code
                    if code != 255:
                        break
                if bad:
                    break
            elif ip + 1 >= ilen:
                bad = 3
                break
            code = byte(ip, "dist")
            ip += 1
            ln += 3
            dist, form = ofs + code + 1, 13
            if code == 255 and ofs == 31 << 8:
                if ip + 1 >= ilen:
                    bad = 4
                    break
                dist, form = (byte(ip, "far_hi") << 8 | byte(ip + 1, "far_lo")) + BLZ_FAR_BASE, 16
                ip += 2
            if ln > olen - o.op or dist > o.op:
                bad = 5
                break
            if ip >= ilen:
                cen.add("end:match_parsed_not_copied")
                break
            ctrl = byte(ip, "ctrl")
            ip += 1
            cen.add("match:len:%d/ext%d" % (ln, next_))
            cen.add("dist:%d:form:%d" % (dist, form))
            if not o.match(dist, ln, "match"):
                bad = 6
                break
            prev_lit = None
        else:
            nl = ctrl + 1
            if nl > olen - o.op or ip + nl > ilen:
                bad = 7
                break
            if (ip - w["base"]) % (1 << 32) > ZWIN - 64:
                w["base"] = ip
                cnt["reload"] += 1
                cen.add("reload:literals")
            cen.add("lit:%d" % nl)
            if prev_lit is not None:
                cen.add("lit:%d>lit:%d" % (prev_lit, nl))
            prev_lit = nl
            o.literals(nl)
            ip += nl
            if ip >= ilen:
                cen.add("end:literals")
                break
            ctrl = byte(ip, "ctrl")
            ip += 1
    if not bad and o.op != olen:
        bad = 8
    _gap_item(o, cen)
    return bad, frozenset(cen), cnt
