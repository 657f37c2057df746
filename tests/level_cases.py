"""Level-aware batch helpers (Zstandard levels 1 - 3): the same slot layout as tests/parity_cases.py, with
tsx_batch_params.zstd_level set.  `N` is a tsxform._native.Native (emulated or real); `o` is the oracle module."""
import numpy as np

import tsxform
from tests import parity_cases as pc
from tsxform import synth

nat = tsxform._native


def run_transform(N, flags, chunks, level, mem=None, profile=nat.ZSTD_PROFILE_1_5_7, ctx=None, key=synth.KEY, aad=synth.AAD):
    """Returns (list of transformed bytes, descs)."""
    sizes = [int(c.size) for c in chunks]
    soff, doff, caps, st, dt = pc.layout(sizes, flags, N)
    src = np.zeros(max(st, 16), np.uint8)
    for c, o_ in zip(chunks, soff):
        src[o_:o_ + c.size] = c
    dst = np.zeros(max(dt, 16), np.uint8)
    d = pc.make_descs(sizes, soff, doff, caps)
    p = nat.Native.make_params(flags, key, aad, zstd_level=level, zstd_profile=profile)
    if mem == "device":
        ds, dd = N.device_malloc(src.size), N.device_malloc(dst.size)
        N.h2d(ds, src)
        N.transform_batch(p, d, ds, dd, dst.size, nat.MEM_DEVICE, ctx=ctx)
        N.d2h(dst, dd)
        N.device_free(ds); N.device_free(dd)
    elif mem == "packed":
        N.transform_batch(p, d, src, dst, dst.size, nat.MEM_HOST_PACKED, ctx=ctx)
        return [dst[int(d["dst_off"][i]):int(d["dst_off"][i]) + int(d["dst_len"][i])].tobytes() for i in range(len(sizes))], d
    else:
        N.transform_batch(p, d, src, dst, dst.size, ctx=ctx)
    return [dst[doff[i]:doff[i] + d["dst_len"][i]].tobytes() for i in range(len(sizes))], d


def transform_status(N, flags, level, n=1000):
    """tsx_transform_batch's return code for one small chunk at `level` (no exception)."""
    x = synth.gen_chunk("K", 3, 0, 0, n)
    soff, doff, caps, st, dt = pc.layout([n], flags, N)
    src = np.zeros(st, np.uint8); src[:n] = x
    dst = np.zeros(dt, np.uint8)
    d = pc.make_descs([n], soff, doff, caps)
    p = nat.Native.make_params(flags, synth.KEY, synth.AAD, zstd_level=level)
    return N.lib.tsx_transform_batch(None, nat.C.byref(p), d.ctypes.data, 1, src.ctypes.data, src.size, dst.ctypes.data, dst.size, nat.MEM_HOST)


def oracle_flags(o, flags):
    return (o.COMPRESS if flags & nat.COMPRESS else 0) | (o.ENCRYPT if flags & nat.ENCRYPT else 0) | (o.CRC if flags & nat.CRC else 0)


def expected(o, flags, level, i, data, segment=0):
    """The oracle's transformed chunk i at `level`: libzstd frame (one-shot, content size), then GCM, as the chain does it."""
    raw = data.tobytes()
    body = o.zstd_compress_chunk(raw, level) if flags & nat.COMPRESS else raw
    if flags & nat.ENCRYPT:
        body = o.gcm_encrypt_chunk(synth.KEY, synth.iv_for(segment, i), synth.AAD, body)
    return body


def check_vs_oracle(N, o, flags, chunks, level, **kw):
    outs, d = run_transform(N, flags, chunks, level, **kw)
    for i, c in enumerate(chunks):
        assert d["status"][i] == 0, (i, c.size, d["status"][i])
        assert outs[i] == expected(o, flags, level, i, c), "chunk %d (n=%d) at level %d differs from the oracle" % (i, c.size, level)
        if flags & nat.CRC:
            assert int(d["crc32c"][i]) == o.crc32c(c.tobytes()), i
    return outs, d


def check_roundtrip(N, flags, chunks, outs):
    back, d2 = pc.run_detransform(N, flags, outs, [int(c.size) for c in chunks])
    for i, c in enumerate(chunks):
        assert d2["status"][i] == 0, (i, d2["status"][i])
        assert back[i] == c.tobytes(), "chunk %d round trip" % i
