"""Record-batch validation (TSX_VALIDATE_RECORDS): helpers shared by the emulated and the device tests.  `N` is a tsxform._native.Native
(emulated or real).  The yardstick of every expected status and every field of tsx_records_info is reference_walk(): a plain serial walk
over the stream in Python, with the CRC of oracle.crc32c."""
import numpy as np

import tsxform
from oracle import oracle as _o
from tests import parity_cases as pc
from tsxform import synth

nat = tsxform._native
VR = getattr(nat, "VALIDATE_RECORDS", 0x100)
E_RECORDS = getattr(nat, "E_RECORDS", -11)
NONE = 0xFFFFFFFFFFFFFFFF
TRUNCATED, LENGTH, MAGIC, CRC = 1, 2, 3, 4
MEMS = ("zero_copy", "host", "device", "packed", "packed_zc")
CUT = 4099                                                              # odd: chunk boundaries meet every alignment, a batch spans up to 9 chunks


def make_batch(base_offset, payload, attributes=0):
    """One v2 record batch around `payload` (the bytes behind the 61-byte header; their framing is not the validator's business)."""
    payload = bytes(payload)
    body = (attributes.to_bytes(2, "big") + (0).to_bytes(4, "big") + (0).to_bytes(8, "big") * 2 + (0xFFFFFFFFFFFFFFFF).to_bytes(8, "big") +
            (0xFFFF).to_bytes(2, "big") + (0xFFFFFFFF).to_bytes(4, "big") + (1 if payload else 0).to_bytes(4, "big") + payload)
    assert len(body) == 40 + len(payload)
    return (base_offset.to_bytes(8, "big") + (9 + len(body)).to_bytes(4, "big") + (0).to_bytes(4, "big") + b"\x02" +
            _o.crc32c(body).to_bytes(4, "big") + body)


_segments = {}


def valid_segment(n=300000):
    """synth's "B" content of n bytes, cut at the end of its last complete batch: a stream that begins and ends on a batch boundary.
    n = 300000: 19 batches of 3.6 - 34 KiB, 290455 bytes."""
    if n not in _segments:
        c = synth.gen_chunk("B", 7, 1, 2, n)
        p, l = synth.record_batches_of(c)[-1]
        s = c[:p + l].tobytes()
        _segments[n] = s
    return _segments[n]


def batches_of(stream):
    """[(start, length)] of a VALID stream."""
    out, p = [], 0
    while p < len(stream):
        l = 12 + int.from_bytes(stream[p + 8:p + 12], "big")
        out.append((p, l)); p += l
    assert p == len(stream)
    return out


def reference_walk(stream):
    """(batches, compressed_batches, first_bad_pos, reason): DefaultRecordBatch.ensureValid() batch after batch; NONE, 0 for a clean stream."""
    stream = bytes(stream)
    n, p, nb, nc = len(stream), 0, 0, 0
    while p < n:
        if n - p < 61:
            return nb, nc, p, TRUNCATED
        l = int.from_bytes(stream[p + 8:p + 12], "big", signed=True)
        if l < 49:
            return nb, nc, p, LENGTH
        if p + 12 + l > n:
            return nb, nc, p, TRUNCATED
        if stream[p + 16] != 2:
            return nb, nc, p, MAGIC
        if _o.crc32c(stream[p + 21:p + 12 + l]) != int.from_bytes(stream[p + 17:p + 21], "big"):
            return nb, nc, p, CRC
        nb += 1; nc += 1 if stream[p + 22] & 7 else 0
        p += 12 + l
    return nb, nc, NONE, 0


def cut(stream, size, empties=()):
    """Chunk sizes of `stream` in pieces of `size` bytes; empties: indices at which a zero-length chunk is put in."""
    sizes = [min(size, len(stream) - a) for a in range(0, len(stream), size)] or [0]
    for i in sorted(empties):
        sizes.insert(i, 0)
    return sizes


def expected_statuses(sizes, bad_pos):
    """TSX_E_RECORDS from the chunk that holds stream position bad_pos on, 0 in front of it."""
    if bad_pos == NONE:
        return [0] * len(sizes)
    at, j = 0, None
    for i, s in enumerate(sizes):
        if s and at <= bad_pos < at + s:
            j = i
        at += s
    assert j is not None, (bad_pos, at)
    return [0 if i < j else E_RECORDS for i in range(len(sizes))]


def run(N, flags, stream, sizes, mem="host", ctx=None, level=3, **cfg):
    """One transform batch whose chunks are `stream` cut into `sizes`, in slot layout with garbage in the gaps between the source slots
    (mem: gcm_verify_cases.run_transform's kinds).  -> (outputs by dst_len, descs)."""
    stream = np.frombuffer(bytes(stream), np.uint8)
    assert sum(sizes) == stream.size
    soff, doff, caps, st, dt = pc.layout(sizes, flags, N)
    src = np.full(max(st, 16), 0xA5, np.uint8)
    src[5::7] = 2                                                       # (a gap that looks like a magic byte here and there)
    at = 0
    for s, o_ in zip(sizes, soff):
        src[o_:o_ + s] = stream[at:at + s]; at += s
    slot = (N.transformed_bound(max(sizes + [0]), flags) + 63) // 64 * 64
    dst = np.full(max(dt, len(sizes) * slot, 16) + 64, 0xEE, np.uint8)
    d = pc.make_descs(sizes, soff, doff, caps)
    p = nat.Native.make_params(flags, synth.KEY, synth.AAD, zstd_level=level)
    registered = mem in ("zero_copy", "packed_zc")
    if mem == "packed_zc":
        cfg = dict(cfg, zero_copy_packed=1)
    with N.configured(**cfg):
        if mem == "device":
            ds, dd = N.device_malloc(src.size), N.device_malloc(dst.size)
            try:
                N.h2d(ds, src); N.h2d(dd, dst)
                N.transform_batch(p, d, ds, dd, dst.size, nat.MEM_DEVICE, ctx=ctx, src_size=src.size)
                N.d2h(dst, dd)
            finally:
                N.device_free(ds); N.device_free(dd)
        else:
            if registered:
                N.host_register(dst)
            try:
                N.transform_batch(p, d, src, dst, dst.size, nat.MEM_HOST_PACKED if mem.startswith("packed") else nat.MEM_HOST, ctx=ctx)
            finally:
                if registered:
                    N.host_unregister(dst)
    return [dst[int(d["dst_off"][i]):int(d["dst_off"][i]) + int(d["dst_len"][i])].tobytes() for i in range(len(sizes))], d


def info(N, ctx):
    r = N.ctx_records(ctx)
    return int(r.batches), int(r.compressed_batches), int(r.first_bad_pos), int(r.first_bad_reason), int(r.repaired_chunks)


def check(N, flags, stream, sizes, mem="host", ctx=None, want=None, repaired=None, **cfg):
    """The batch with the flag: statuses, dst_len and tsx_records_info as reference_walk says; the delivered chunks' bytes are those of
    `want` (default: of the run without the flag).  repaired: what repaired_chunks must be (None: not looked at).  -> (outputs, info)."""
    ref = reference_walk(stream)
    if want is None:
        want, d0 = run(N, flags, stream, sizes, mem, ctx, **cfg)
        assert (d0["status"] == 0).all(), (mem, cfg, list(d0["status"]))
        if ctx is not None:
            assert info(N, ctx) == (0, 0, NONE, 0, 0)                   # a batch without the flag has nothing to say
    outs, d = run(N, flags | VR, stream, sizes, mem, ctx, **cfg)
    exp = expected_statuses(sizes, ref[2])
    assert [int(x) for x in d["status"]] == exp, (mem, cfg, ref, [int(x) for x in d["status"]])
    for i, e in enumerate(exp):
        assert (outs[i] == want[i] and int(d["dst_len"][i]) == len(want[i])) if e == 0 else (outs[i] == b"" and d["dst_len"][i] == 0), (mem, cfg, i)
    got = None
    if ctx is not None:
        got = info(N, ctx)
        assert got[:4] == ref, (mem, cfg, got, ref)
        if repaired is not None:
            assert got[4] == repaired, (mem, cfg, got)
    return outs, got


def long_batch(stream, sizes_of=CUT, min_len=3 * CUT, first_chunk=2):
    """(start, length, chunk) of the first batch of a valid stream that is at least min_len long and begins in chunk >= first_chunk."""
    for p, l in batches_of(stream):
        if l >= min_len and p // sizes_of >= first_chunk:
            return p, l, p // sizes_of
    raise AssertionError("no such batch")


def flip(stream, at):
    b = bytearray(stream); b[at] ^= 1
    return bytes(b)


def damage_cases(stream):
    """[(name, damaged stream)]: one byte of one batch at a time, hostile lengths, and the stream's ends.  `fails` of a case says whether the
    reference walk must find something (a byte of baseOffset or partitionLeaderEpoch is outside the CRC)."""
    p, l, j = long_batch(stream)
    cases = [("len%d" % k, flip(stream, p + 8 + k), True) for k in range(4)]
    cases += [("magic", flip(stream, p + 16), True)] + [("crc%d" % k, flip(stream, p + 17 + k), True) for k in range(4)]
    cases += [("attributes", flip(stream, p + 21), True), ("last", flip(stream, p + l - 1), True), ("body+2chunks", flip(stream, p + 61 + 2 * CUT), True)]
    cases += [("baseOffset", flip(stream, p + 3), False), ("leaderEpoch", flip(stream, p + 13), False)]
    for name, v in (("len7FFFFFFF", 0x7FFFFFFF), ("len80000000", 0x80000000), ("len48", 48)):
        b = bytearray(stream); b[p + 8:p + 12] = v.to_bytes(4, "big")
        cases.append((name, bytes(b), True))
    cases += [("cut1", stream[:-1], True), ("cut61", stream[:-61], True), ("garbage1", stream + b"\x5A", True), ("garbage60", stream + b"\x5A" * 60, True),
              ("zeros4096", stream + bytes(4096), True)]
    return cases, (p, l, j)


def nested_stream():
    """A record value that holds a complete CRC-valid batch which begins exactly on chunk 1's first byte (CUT-byte chunks): the walker of
    chunk 1 takes it for its entry, the chain arrives elsewhere.  The outer batch ends inside chunk 1, five more batches follow."""
    first = make_batch(0, bytes(range(256)) * 3 + b"x" * 171)           # 1000 bytes
    assert len(first) == 1000
    inner = make_batch(77, b"inner" * 90, attributes=1)
    pad = CUT - (len(first) + 61)
    outer = make_batch(1, b"\x11" * pad + inner + b"\x22" * 300)
    rest = b"".join(make_batch(2 + i, bytes([i]) * (1500 + 100 * i), attributes=i & 1) for i in range(5))
    s = first + outer + rest
    assert s[CUT:CUT + len(inner)] == inner and len(first) + len(outer) < 2 * CUT
    return s


def gpu_stream():
    """About 8 MiB of B content as ONE valid stream, generated once: (stream, the batch that crosses the 4 MiB boundary)."""
    if "gpu" not in _segments:
        s = valid_segment(8 << 20)
        cross = [(p, l) for p, l in batches_of(s) if p < (4 << 20) < p + l]
        _segments["gpu"] = (s, cross[0])
    return _segments["gpu"]
