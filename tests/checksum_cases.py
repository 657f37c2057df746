"""Zstandard content checksum (TSX_ZSTD_CHECKSUM): helpers shared by the emulated and the device tests.  The reference is the real libzstd
the oracle has loaded, opened through ctypes from the path orc_zstd_path() reports and driven the way oracle/zstd_ref.c drives it, plus
ZSTD_c_checksumFlag = 1.  `N` is a tsxform._native.Native (emulated or real); `o` is the oracle module."""
import ctypes as C

import numpy as np
import pytest

import tsxform
from tests import parity_cases as pc
from tests import zstd_inspect as zi
from tsxform import synth

nat = tsxform._native
CK = nat.COMPRESS | getattr(nat, "ZSTD_CHECKSUM", 8)
SIZES = [0, 1, 3, 4, 7, 8, 15, 16, 31, 32, 33, 63, 64, 65, 255, 256, 1000, 131071, 131072, 131073, 200000, 300007]
_Z = None


def need157(o):
    if not o.zstd_version().startswith("1.5.7"):
        pytest.skip("libzstd 1.5.7 not available")


def libzstd(o):
    global _Z
    if _Z is None:
        Z = C.CDLL(o.lib().orc_zstd_path().decode())
        Z.ZSTD_createCCtx.restype = C.c_void_p
        Z.ZSTD_freeCCtx.argtypes = [C.c_void_p]
        Z.ZSTD_CCtx_setParameter.restype = C.c_size_t; Z.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
        Z.ZSTD_CCtx_setPledgedSrcSize.restype = C.c_size_t; Z.ZSTD_CCtx_setPledgedSrcSize.argtypes = [C.c_void_p, C.c_ulonglong]
        Z.ZSTD_compress2.restype = C.c_size_t; Z.ZSTD_compress2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        Z.ZSTD_compressBound.restype = C.c_size_t; Z.ZSTD_compressBound.argtypes = [C.c_size_t]
        Z.ZSTD_decompress.restype = C.c_size_t; Z.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        Z.ZSTD_isError.restype = C.c_uint; Z.ZSTD_isError.argtypes = [C.c_size_t]
        Z.ZSTD_getErrorName.restype = C.c_char_p; Z.ZSTD_getErrorName.argtypes = [C.c_size_t]
        _Z = Z
    return _Z


def frame(o, data, level=3, checksum=True):
    """libzstd's frame of `data`: ZSTD_createCCtx, level, content size flag, [checksum flag,] pledged size, ZSTD_compress2."""
    Z = libzstd(o)
    a = np.ascontiguousarray(np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data)
    cap = Z.ZSTD_compressBound(a.size)
    dst = np.zeros(max(cap, 1), np.uint8)
    c = Z.ZSTD_createCCtx()
    try:
        for prm, v in ((100, level), (200, 1), (201, 1 if checksum else 0)):
            assert not Z.ZSTD_isError(Z.ZSTD_CCtx_setParameter(c, prm, v))
        assert not Z.ZSTD_isError(Z.ZSTD_CCtx_setPledgedSrcSize(c, a.size))
        r = Z.ZSTD_compress2(c, dst.ctypes.data, cap, a.ctypes.data, a.size)
        assert not Z.ZSTD_isError(r), Z.ZSTD_getErrorName(r)
    finally:
        Z.ZSTD_freeCCtx(c)
    return dst[:r].tobytes()


def libzstd_rejects(o, blob, size):
    """ZSTD_decompress's verdict on a (damaged) frame: the error's name, or None when it decodes."""
    Z = libzstd(o)
    src = np.frombuffer(blob, np.uint8)
    dst = np.zeros(max(size, 1), np.uint8)
    r = Z.ZSTD_decompress(dst.ctypes.data, size, src.ctypes.data, src.size)
    return Z.ZSTD_getErrorName(r).decode() if Z.ZSTD_isError(r) else None


def contents(n):
    """The three contents of the byte-identity matrix at size n: Kafka-like, incompressible (raw blocks), zeros (RLE blocks)."""
    return {"K": synth.gen_chunk("K", 21, 0, 0, n), "R": synth.gen_chunk("R", 21, 0, 1, n), "zero": np.zeros(n, np.uint8)}


def run_transform(N, flags, chunks, level=3, profile=nat.ZSTD_PROFILE_1_5_7, mem=None, dst_caps=None, guard=0, ctx=None):
    """parity_cases.run_transform with a level and `guard` bytes of 0xEE behind every slot (the output buffer starts as 0xEE everywhere).
    -> (outputs, descs, bytes of each guard)."""
    sizes = [int(c.size) for c in chunks]
    soff, doff, caps, st, dt = pc.layout(sizes, flags, N, slack=guard)
    caps = [c - guard for c in caps]
    if dst_caps:
        caps = [c if o_ is None else o_ for c, o_ in zip(caps, dst_caps)]
    src = np.zeros(max(st, 16), np.uint8)
    for c, o_ in zip(chunks, soff):
        src[o_:o_ + c.size] = c
    dst = np.full(max(dt, 16), 0xEE, np.uint8)
    d = pc.make_descs(sizes, soff, doff, caps)
    p = nat.Native.make_params(flags, synth.KEY, synth.AAD, zstd_level=level, zstd_profile=profile)
    if mem == "device":
        ds, dd = N.device_malloc(src.size), N.device_malloc(dst.size)
        N.h2d(ds, src); N.h2d(dd, dst)
        N.transform_batch(p, d, ds, dd, dst.size, nat.MEM_DEVICE, ctx=ctx)
        N.d2h(dst, dd)
        N.device_free(ds); N.device_free(dd)
    elif mem == "packed":
        N.transform_batch(p, d, src, dst, dst.size, nat.MEM_HOST_PACKED, ctx=ctx)
        return [dst[int(d["dst_off"][i]):int(d["dst_off"][i]) + int(d["dst_len"][i])].tobytes() for i in range(len(sizes))], d, []
    else:
        N.transform_batch(p, d, src, dst, dst.size, ctx=ctx)
    outs = [dst[doff[i]:doff[i] + int(d["dst_len"][i])].tobytes() for i in range(len(sizes))]
    guards = [dst[doff[i] + caps[i]:doff[i] + caps[i] + guard].tobytes() for i in range(len(sizes))]
    return outs, d, guards


def transform_rc(N, flags, n=1000):
    """tsx_transform_batch's return code for one small chunk (no exception)."""
    x = synth.gen_chunk("K", 3, 0, 0, n)
    soff, doff, caps, st, dt = pc.layout([n], flags, N)
    src = np.zeros(st, np.uint8); src[:n] = x
    dst = np.zeros(dt, np.uint8)
    d = pc.make_descs([n], soff, doff, caps)
    p = nat.Native.make_params(flags, synth.KEY, synth.AAD)
    return N.lib.tsx_transform_batch(None, C.byref(p), d.ctypes.data, 1, src.ctypes.data, src.size, dst.ctypes.data, dst.size, nat.MEM_HOST)


def decode_both_forms(N, flags, blobs, sizes):
    """The same batch through the block form (the default for small batches) and the chunk form (dec_block_chunks = 0).
    -> {"block": (outs, descs, chunks the block form kept), "chunk": (outs, descs, -1)}"""
    res = {}
    ctx = N.ctx_create(0, 0, 0)
    try:
        outs, d = pc.run_detransform(N, flags, blobs, sizes, ctx=ctx)
        res["block"] = (outs, d, pc.blockmode_chunks(N, ctx, len(blobs)))
        with N.configured(dec_block_chunks=0):
            outs, d = pc.run_detransform(N, flags, blobs, sizes, ctx=ctx)
            res["chunk"] = (outs, d, pc.blockmode_chunks(N, ctx, len(blobs)))
    finally:
        N.ctx_destroy(ctx)
    assert res["block"][2] >= 0 and res["chunk"][2] == -1
    return res


def raw_sections(blob):
    """(raw block bodies, raw literals sections of compressed blocks) of a frame, each a list of (offset, length) in the frame, length > 0.
    The blocks come from tests/zstd_inspect.py; a block's body starts three bytes behind its header."""
    hdr, blocks, _ = zi.parse_frame(blob, decode=False)
    p = hdr["header_size"]
    raw_blocks, raw_lits = [], []
    for b in blocks:
        body = p + 3
        if b.btype == "raw":
            if b.size:
                raw_blocks.append((body, b.size))
            p = body + b.size
        elif b.btype == "rle":
            p = body + 1
        else:
            if b.lit_type == "raw" and b.lit_regen:
                hl = {0: 1, 2: 1, 1: 2, 3: 3}[(blob[body] >> 2) & 3]
                raw_lits.append((body + hl, b.lit_regen))
            p = body + b.size
    assert p + (4 if hdr["checksum"] else 0) == len(blob)
    return raw_blocks, raw_lits


def flip(blob, at, mask=0x40):
    x = bytearray(blob); x[at] ^= mask
    return bytes(x)


def rawlit_input(n):
    """Incompressible bytes, then the same bytes again: a compressed block whose literals section is raw (half of n random literals, one
    long match).  n <= 256 KiB."""
    R = synth.gen_chunk("R", 33, 0, 0, (n + 1) // 2)
    return np.concatenate([R, R])[:n]


def damage_cases(o, level=3):
    """-> (cases, controls).  cases: (name, damaged checksummed frame, content size), each one rejected by libzstd itself (asserted
    here, so an input that is accidentally no damage is noticed).  controls: (name, checksum-free frame of the same input with the same
    body damage, content size, the bytes libzstd restores from it) - libzstd accepts those."""
    rawblk = synth.gen_chunk("R", 33, 0, 1, 1000)                       # incompressible: one raw block
    rawlit = rawlit_input(6000)
    cases, controls = [], []
    f = frame(o, rawblk, level)
    for k in range(4):
        cases.append(("checksum byte %d" % k, flip(f, len(f) - 4 + k, 1 << (2 * k)), rawblk.size))
    for name, x, pick in (("raw block body", rawblk, 0), ("raw literals", rawlit, 1)):
        f, g = frame(o, x, level), frame(o, x, level, checksum=False)
        assert f[5:-4] == g[5:] and f[4] == g[4] | 4
        secs = raw_sections(f)[pick]
        assert secs and raw_sections(g)[pick] == secs, "%s: the input no longer produces such a section" % name
        at = secs[0][0] + min(20, secs[0][1] - 1)
        cases.append((name, flip(f, at), x.size))
        want = bytearray(x.tobytes())
        ctl = flip(g, at)
        back = o.zstd_decompress_chunk(ctl, x.size)
        assert back != x.tobytes() and len(back) == len(want)
        controls.append((name, ctl, x.size, back))
    for name, blob, size in cases:
        err = libzstd_rejects(o, blob, size)
        assert err is not None, "%s: libzstd decodes the damaged frame" % name
    return cases, controls


def device_xxh64(N, data, offsets):
    """XXH64 of `data` placed at each of `offsets` bytes past a 256-byte aligned device address, by the library's one-wave hash (test hook
    tsx_debug_xxh64).  -> list of 64-bit values."""
    f = N.lib.tsx_debug_xxh64
    f.restype = C.c_int; f.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_ulonglong)]
    a = np.ascontiguousarray(data, dtype=np.uint8)
    res = []
    for off in offsets:
        host = np.zeros(off + a.size + 64, np.uint8); host[off:off + a.size] = a
        dev = N.device_malloc(host.size)
        try:
            N.h2d(dev, host)
            out = C.c_ulonglong(0)
            assert f(dev + off, a.size, C.byref(out)) == 0
            res.append(out.value)
        finally:
            N.device_free(dev)
    return res
