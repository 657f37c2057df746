"""Record framing and offset order (TSX_VALIDATE_FRAMES): helpers shared by the emulated and the device tests.  `N` is a
tsxform._native.Native (emulated or real).  The yardstick of every expected status and every field of tsx_records_info is
reference_walk_frames(): a plain serial walk in Python over the semantics of include/tsxform.h, on top of records_cases.reference_walk
and oracle.crc32c.  Statuses come from records_cases.expected_statuses."""
import random

import numpy as np

import tsxform
from oracle import oracle as _o
from tests import records_cases as rc

nat = tsxform._native
VR = rc.VR
VF = getattr(nat, "VALIDATE_FRAMES", 0x400)
RECORDS, OFFSETS = 5, 6
I64_MAX = (1 << 63) - 1


# ---- the reference ------------------------------------------------------------------------------------------------------------
def read_varint(s, q, lim, width=5):
    """ByteUtils.readVarint (width 5) / readVarlong (width 10) at s[q], inside [q, lim): (value, next position), or None when it is
    malformed or leaves the range.  Excess bits of the last permitted byte are dropped, as Java's int / long arithmetic drops them."""
    bits = 32 if width == 5 else 64
    val = 0
    for i in range(width):
        if q >= lim:
            return None
        b = s[q]; q += 1
        val |= (b & 0x7F) << (7 * i)
        if not b & 0x80:
            val &= (1 << bits) - 1
            v = (val >> 1) ^ -(val & 1)
            return v, q
    return None


def _sized(s, q, e, least):
    r = read_varint(s, q, e)
    if r is None or r[0] < least:
        return None
    n, q = r
    if n > 0:
        if n > e - q:
            return None
        q += n
    return q


def walk_records(s, q, end, count, last_delta):
    """Exactly `count` records in s[q:end]: 0, or the reason of the first failing field of the lowest-numbered failing record."""
    prev = -1
    for _ in range(count):
        r = read_varint(s, q, end)                                      # length
        if r is None or r[0] < 0 or r[0] > end - r[1]:
            return RECORDS
        b = r[1]; e = b + r[0]
        if b >= e:                                                      # attributes
            return RECORDS
        r = read_varint(s, b + 1, e, 10)                                # timestampDelta
        if r is None:
            return RECORDS
        r = read_varint(s, r[1], e)                                     # offsetDelta
        if r is None:
            return RECORDS
        d, p = r
        if d < 0 or d > last_delta or d <= prev:
            return OFFSETS
        prev = d
        p = _sized(s, p, e, -1)                                         # key
        if p is None:
            return RECORDS
        p = _sized(s, p, e, -1)                                         # value
        if p is None:
            return RECORDS
        r = read_varint(s, p, e)                                        # headers
        if r is None or r[0] < 0:
            return RECORDS
        nh, p = r
        for _h in range(nh):
            p = _sized(s, p, e, 0)
            if p is None:
                return RECORDS
            p = _sized(s, p, e, -1)
            if p is None:
                return RECORDS
        if p != e:
            return RECORDS
        q = e
    return 0 if q == end else RECORDS


def frames_check(s, p, end, have_prev, prev_last):
    """The checks behind a batch's CRC: (reason, last offset, records read)."""
    base = int.from_bytes(s[p:p + 8], "big", signed=True)
    lod = int.from_bytes(s[p + 23:p + 27], "big", signed=True)
    count = int.from_bytes(s[p + 57:p + 61], "big", signed=True)
    if base < 0 or lod < 0 or base + lod > I64_MAX or (have_prev and base <= prev_last):
        return OFFSETS, 0, 0
    if count < 0:
        return RECORDS, 0, 0
    if s[p + 22] & 7:
        return 0, base + lod, 0
    return walk_records(s, p + 61, end, count, lod), base + lod, count


def reference_walk_frames(stream):
    """(batches, compressed_batches, records, first_bad_pos, reason) of TSX_VALIDATE_RECORDS | TSX_VALIDATE_FRAMES; NONE, 0 when clean."""
    s = bytes(stream)
    nb0, nc0, bad0, why0 = rc.reference_walk(s)                         # checks 1-4: nb0 batches pass them, then bad0 / why0
    p, nb, nc, nr = 0, 0, 0, 0
    have, last = False, 0
    for _ in range(nb0):
        end = p + 12 + int.from_bytes(s[p + 8:p + 12], "big")
        why, l, n = frames_check(s, p, end, have, last)
        if why:
            return nb, nc, nr, p, why
        have, last = True, l
        nb += 1; nc += 1 if s[p + 22] & 7 else 0; nr += n
        p = end
    return nb, nc, nr, bad0, why0


# ---- a builder ----------------------------------------------------------------------------------------------------------------
def varint(v, pad_to=0):
    """Zigzag varint of v; pad_to: a longer (non-canonical) encoding of that many bytes."""
    z = ((v << 1) ^ (v >> 63)) & 0xFFFFFFFFFFFFFFFF
    out = bytearray()
    while True:
        b = z & 0x7F; z >>= 7
        if z or len(out) + 1 < pad_to:
            out.append(b | 0x80)
        else:
            out.append(b); break
    return bytes(out)


def record(delta, key=b"key", value=b"value", headers=(), ts=0, attributes=0, **raw):
    """One record.  key / value None: null (-1).  headers: (key, value) pairs, or bytes taken as they are.  raw: the ENCODING of a field in
    place of the honest one - length, klen, vlen, hcount (ts and delta: bytes in place of the number) - and tail: bytes behind the fields."""
    body = bytes([attributes]) + (ts if isinstance(ts, bytes) else varint(ts)) + (delta if isinstance(delta, bytes) else varint(delta))
    body += raw.get("klen", varint(-1 if key is None else len(key))) + (key or b"")
    body += raw.get("vlen", varint(-1 if value is None else len(value))) + (value or b"")
    body += raw.get("hcount", varint(len(headers)))
    for h in headers:
        body += h if isinstance(h, bytes) else varint(len(h[0])) + h[0] + varint(-1 if h[1] is None else len(h[1])) + (h[1] or b"")
    body += raw.get("tail", b"")
    return raw.get("length", varint(len(body))) + body


def seal(batch):
    """`batch` with its batchLength left alone and its CRC recomputed."""
    b = bytearray(batch)
    b[17:21] = _o.crc32c(bytes(b[21:])).to_bytes(4, "big")
    return bytes(b)


def batch(base, records, attributes=0, lod=None, count=None, region=None):
    """A sealed v2 batch of `records` (encoded records).  lod / count default to what the records say; region: the bytes behind the header
    in place of the records (a compressed payload)."""
    payload = b"".join(records) if region is None else region
    n = len(records)
    lod = max(n - 1, 0) if lod is None else lod
    count = n if count is None else count
    body = (attributes.to_bytes(2, "big") + (lod & 0xFFFFFFFF).to_bytes(4, "big") + (0).to_bytes(8, "big") * 2 + (0xFFFFFFFFFFFFFFFF).to_bytes(8, "big") +
            (0xFFFF).to_bytes(2, "big") + (0xFFFFFFFF).to_bytes(4, "big") + (count & 0xFFFFFFFF).to_bytes(4, "big") + payload)
    return seal((base & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "big") + (9 + len(body)).to_bytes(4, "big") + (0).to_bytes(4, "big") + b"\x02" + bytes(4) + body)


class Batch:
    """A batch of the built stream taken apart: its header fields and its records as keyword sets of record(), to change and put together
    again.  slack: bytes behind the last record."""

    def __init__(self, base, recs, attributes=0, region=None):
        self.base, self.recs, self.attributes, self.region = base, [dict(r) for r in recs], attributes, region
        self.lod = self.count = None
        self.slack = b""
        self.base_damage = None                                         # baseOffset written behind the seal (it lies outside the CRC)

    def copy(self):
        c = Batch(self.base, self.recs, self.attributes, self.region)
        c.lod, c.count, c.slack, c.base_damage = self.lod, self.count, self.slack, self.base_damage
        return c

    def last(self):
        return self.base + (max(len(self.recs) - 1, 0) if self.lod is None else self.lod)

    def bytes(self):
        recs = [record(**r) for r in self.recs]
        region = self.region if self.region is not None else (b"".join(recs) + self.slack if self.slack else None)
        b = batch(self.base, recs, self.attributes, self.lod, self.count, region)
        if self.base_damage is not None:
            b = (self.base_damage & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "big") + b[8:]
        return b


_built = {}


def built_batches():
    """The batches of the built stream: 14 of them, 70 KB in all, offsets with gaps of 100 between the batches; keys, values and headers
    of every kind (null key, null value, empty value, header with a null value, a value of 9 KB that spans three 4099-byte chunks); batch 4
    is compressed (a garbage payload behind a sane header), batch 7 a control batch, batch 9 empty (compaction's leftover, lastOffsetDelta
    kept)."""
    if "b" not in _built:
        rnd = random.Random(20241)
        out = []
        for i in range(14):
            base = 1000 + 100 * i
            if i == 4:
                out.append(Batch(base, [], attributes=2, region=bytes(rnd.randrange(256) for _ in range(3000))))
                out[-1].lod, out[-1].count = 30, 31
                continue
            if i == 9:
                out.append(Batch(base, []))
                out[-1].lod = 17
                continue
            recs = []
            for d in range(12 + i):
                r = {"delta": d, "ts": rnd.randrange(-5, 100000), "key": bytes(rnd.randrange(256) for _ in range(rnd.randrange(0, 20))),
                     "value": bytes(rnd.randrange(97, 123) for _ in range(rnd.choice((0, 5, 130, 300, 700)))), "headers": ()}
                if d % 5 == 1:
                    r["key"] = None
                if d % 7 == 2:
                    r["value"] = None
                if d % 4 == 3:
                    r["headers"] = ((b"h" * rnd.randrange(0, 9), b"v" * rnd.randrange(0, 200)), (b"null", None))
                if i == 5 and d == 6:
                    r["value"] = bytes(rnd.randrange(256) for _ in range(9000))
                recs.append(r)
            out.append(Batch(base, recs, attributes=0x20 if i == 7 else 0))
        _built["b"] = out
    return [b.copy() for b in _built["b"]]


def stream_of(batches):
    """(stream, [start of every batch])"""
    parts = [b.bytes() for b in batches]
    starts, at = [], 0
    for p in parts:
        starts.append(at); at += len(p)
    return b"".join(parts), starts


# ---- damage -------------------------------------------------------------------------------------------------------------------
def _rec(field, value, i=3):
    def f(b, prev):
        b.recs[i][field] = value
    return f


def _set(**kw):
    def f(b, prev):
        for k, v in kw.items():
            setattr(b, k, v(b, prev) if callable(v) else v)
    return f


def _length(delta=None, enc=None, i=3):
    def f(b, prev):
        n = len(record(**dict(b.recs[i], length=b"")))                  # the body
        b.recs[i]["length"] = enc(n) if enc else varint(n + delta)
    return f


def _cut_off_length(b, prev):
    b.slack = b"\x80"; b.count = len(b.recs) + 1


def _two(b, prev):                                                      # an offsets failure of the batch AND a framing failure in it
    b.base_damage = prev.last(); b.recs[2]["klen"] = varint(-2)


def _rec3_and_rec7(b, prev):
    b.recs[3]["delta"] = varint(2); b.recs[7]["vlen"] = varint(-2)


# (name, mutation of a Batch given its predecessor, the reason the reference must find at that batch - 0: the stream stays clean)
DAMAGE = [
    ("count+1", _set(count=lambda b, p: len(b.recs) + 1), RECORDS), ("count-1", _set(count=lambda b, p: len(b.recs) - 1), RECORDS),
    ("count0", _set(count=0), RECORDS), ("count<0", _set(count=-1), RECORDS),
    ("lod<last", _set(lod=lambda b, p: len(b.recs) - 2), OFFSETS), ("lod<0", _set(lod=-1), OFFSETS),
    ("length+1", _length(1), RECORDS), ("length-1", _length(-1), RECORDS), ("length>batch", _length(1 << 20), RECORDS),
    ("length<0", _length(enc=lambda n: varint(-3)), RECORDS), ("length5bytes", _length(enc=lambda n: varint(n, 5)), 0),
    ("length6bytes", _length(enc=lambda n: varint(n, 6)), RECORDS), ("length cut off", _cut_off_length, RECORDS),
    ("klen>record", _rec("klen", varint(10000)), RECORDS), ("klen-2", _rec("klen", varint(-2)), RECORDS), ("vlen-2", _rec("vlen", varint(-2)), RECORDS),
    ("nulls", lambda b, p: b.recs[3].update(key=None, value=None), 0), ("hcount-1", _rec("hcount", varint(-1)), RECORDS),
    ("hkey-1", lambda b, p: b.recs[3].update(headers=(varint(-1) + varint(1) + b"x",)), RECORDS), ("slack", _rec("tail", b"\x00"), RECORDS),
    ("ts11bytes", _rec("ts", b"\x80" * 10 + b"\x00"), RECORDS),
    ("delta repeated", _rec("delta", varint(2)), OFFSETS), ("delta decreasing", _rec("delta", varint(1)), OFFSETS),
    ("delta>lod", lambda b, p: b.recs[-1].update(delta=varint(len(b.recs))), OFFSETS), ("delta<0", _rec("delta", varint(-1), 0), OFFSETS),
    ("base top bit", _set(base_damage=lambda b, p: b.base | 1 << 63), OFFSETS),
    ("base=prev last", _set(base_damage=lambda b, p: p.last()), OFFSETS), ("base=prev last-1", _set(base_damage=lambda b, p: p.last() - 1), OFFSETS),
    ("base low bit", _set(base_damage=lambda b, p: b.base ^ 1), 0),
    ("offsets and framing", _two, OFFSETS), ("record 3 offsets, record 7 framing", _rec3_and_rec7, OFFSETS),
]
TARGETS = {"inside": 6, "first": 0, "last": 13}                         # batches of the built stream with records; "seam" is "inside" cut at its first byte


def damaged(name_fn, target):
    """The built stream with one batch changed: (stream, the batch's position, the reason expected there).  The stream's first batch has
    no predecessor: the two cases that need one move the SECOND batch's baseOffset onto / in front of the first batch's last offset there
    (the same check, seen from the only side the first batch has) - the reason is then found at the second batch."""
    name, fn, why = name_fn
    bs = built_batches()
    j = TARGETS[target]
    if j == 0 and ("prev last" in name or name == "offsets and framing"):
        j = 1
    fn(bs[j], bs[j - 1] if j else None)
    s, starts = stream_of(bs)
    return s, starts[j], why, starts[j]


def sizes_for(stream, size, seam=None, empties=(1,)):
    """Chunks of `size` bytes, one more boundary at stream position `seam`, empty chunks put in."""
    cuts = sorted(set(list(range(0, len(stream), size)) + ([seam] if seam else [])) | {len(stream)})
    sizes = [b - a for a, b in zip(cuts, cuts[1:])] or [0]
    for i in sorted(empties):
        sizes.insert(min(i, len(sizes)), 0)
    return sizes


def special_streams():
    """[(name, stream, (first_bad_pos, reason) the reference must find - NONE, 0: clean)] - batches that must pass, precedence, speculation."""
    out = []
    bs = built_batches()
    s, st = stream_of(bs)
    out.append(("compressed, control and empty batches pass", s, (rc.NONE, 0)))
    bs[4].base_damage = bs[3].last()
    out.append(("a compressed batch's baseOffset is checked", stream_of(bs)[0], (st[4], OFFSETS)))
    bs = built_batches(); bs[9].lod = 99; bs[13] = Batch(5000, []); bs[13].lod = 0x7FFFFFFF
    out.append(("an empty batch with any lastOffsetDelta", stream_of(bs)[0], (rc.NONE, 0)))
    bs = built_batches(); bs[5].count = len(bs[5].recs) - 1
    s, st = stream_of(bs)
    out.append(("framing in front of crc", rc.flip(s, st[8] + 30), (st[5], RECORDS)))
    out.append(("crc in front of framing", rc.flip(s, st[2] + 30), (st[2], rc.CRC)))
    return out


def nested_stream():
    """A record value that holds a whole CRC-valid batch with bad framing (its count says one record more) which begins exactly on chunk
    1's first byte (CUT-byte chunks): the walker of chunk 1 takes it for its entry and fails it; the chain never arrives there."""
    inner = Batch(77, [{"delta": d} for d in range(5)]); inner.count = 6
    inner = inner.bytes()
    first = batch(10, [record(d, value=b"f" * 50) for d in range(9)])
    pad = rc.CUT - len(first) - 61 - 40
    while True:
        outer = batch(30, [record(0, value=b"a" * 30), record(1, key=b"k" * 9, value=b"\x11" * pad + inner + b"\x22" * 300), record(2)])
        at = (first + outer).index(inner)
        if at == rc.CUT:
            break
        pad += rc.CUT - at
    rest = [batch(40 + 10 * i, [record(d, value=bytes([65 + i]) * (100 + 10 * i)) for d in range(10)], attributes=0) for i in range(5)]
    s = first + outer + b"".join(rest)
    assert s[rc.CUT:rc.CUT + len(inner)] == inner and reference_walk_frames(inner)[3:] == (0, RECORDS)
    return s


# ---- fuzz ---------------------------------------------------------------------------------------------------------------------
FUZZ_SEED, FUZZ_N = 771, 300


def fuzz_cases(segment, n=FUZZ_N, seed=FUZZ_SEED):
    """n single-byte mutations of the valid segment, every second one resealed (the CRC of the batch that held the byte recomputed), each
    with a cut size of its own.  A value byte says nothing about framing, and values are 95 % of the segment: three positions of four are
    drawn from a batch header (one) or from the first 6 bytes of a record - length, attributes, timestampDelta, offsetDelta, keyLength -
    (two), the fourth anywhere.  -> [(stream, cut size, resealed)]"""
    rnd = random.Random(seed)
    bat = rc.batches_of(segment)
    recs = []
    for p, l in bat:
        q = p + 61
        for _ in range(int.from_bytes(segment[p + 57:p + 61], "big")):
            n_, b = read_varint(segment, q, p + l)
            recs.append(q); q = b + n_
    out = []
    for i in range(n):
        k = rnd.randrange(4)
        at = rnd.randrange(len(segment)) if k == 0 else rnd.choice(bat)[0] + rnd.randrange(61) if k == 1 else rnd.choice(recs) + rnd.randrange(6)
        s = bytearray(segment)
        s[at] ^= 1 << rnd.randrange(8)
        reseal = i % 2 == 1
        if reseal:
            p, l = [(p, l) for p, l in bat if p <= at < p + l][0]
            s[p + 17:p + 21] = _o.crc32c(bytes(s[p + 21:p + l])).to_bytes(4, "big")
        out.append((bytes(s), rnd.choice((rc.CUT, 65536, rnd.randrange(1500, 40000))), reseal))
    return out


# ---- running ------------------------------------------------------------------------------------------------------------------
def info(N, ctx):
    r = N.ctx_records(ctx)
    return int(r.batches), int(r.compressed_batches), int(r.records), int(r.first_bad_pos), int(r.first_bad_reason)


def check(N, flags, stream, sizes, mem="host", ctx=None, want=None, **cfg):
    """The batch with TSX_VALIDATE_RECORDS | TSX_VALIDATE_FRAMES: statuses, dst_len and tsx_records_info as reference_walk_frames says; the
    delivered chunks' bytes are those of `want` (default: of the run without either flag).  -> (outputs, info, repaired_chunks)"""
    ref = reference_walk_frames(stream)
    if want is None:
        want, d0 = rc.run(N, flags, stream, sizes, mem, ctx, **cfg)
        assert (d0["status"] == 0).all(), (mem, cfg, list(d0["status"]))
    outs, d = rc.run(N, flags | VR | VF, stream, sizes, mem, ctx, **cfg)
    exp = rc.expected_statuses(sizes, ref[3])
    assert [int(x) for x in d["status"]] == exp, (mem, cfg, ref, [int(x) for x in d["status"]])
    for i, e in enumerate(exp):
        assert (outs[i] == want[i] and int(d["dst_len"][i]) == len(want[i])) if e == 0 else (outs[i] == b"" and d["dst_len"][i] == 0), (mem, cfg, i)
    got = rep = None
    if ctx is not None:
        got = info(N, ctx)
        rep = int(N.ctx_records(ctx).repaired_chunks)
        assert got == ref, (mem, cfg, got, ref)
    return outs, got, rep


def damage_matrix(N, ctx, size, flags):
    """Every damage on every target at one cut size, with TSX_VALIDATE_RECORDS alone (today's verdict: clean) and with the new flag.
    -> the number of streams run."""
    n = 0
    for case in DAMAGE:
        for target in ("inside", "seam", "first", "last"):
            s, pos, why, at = damaged(case, "inside" if target == "seam" else target)
            ref = reference_walk_frames(s)
            assert ref[3:] == ((pos, why) if why else (rc.NONE, 0)), (case[0], target, ref, pos, why)
            assert rc.reference_walk(s)[2:] == (rc.NONE, 0), case[0]
            sizes = sizes_for(s, size, seam=at if target == "seam" else None)
            if target == "seam":
                assert at in np.cumsum([0] + sizes)
            elif target == "inside":
                assert at % size
            want, d0 = rc.run(N, flags | VR, s, sizes, "host", ctx)     # today's behaviour: this damage is not seen
            assert (d0["status"] == 0).all() and rc.info(N, ctx)[:4] == rc.reference_walk(s), (case[0], target)
            assert int(N.ctx_records(ctx).records) == 0
            check(N, flags, s, sizes, "host", ctx, want=want)
            n += 1
    return n
