"""A failed chunk inside a packed batch (TSX_MEM_HOST_PACKED + TSX_VERIFY), shared by the emulated and the device test.  A packed chunk's
final offset is decided behind the waves, on the host: in place when they wrote into the caller's buffer (zero-copy output), by the copies
otherwise.  Both ways must say the same about a chunk that is not TSX_OK: no bytes, no room, its successor starts where it would have."""
import ctypes

import numpy as np

import tsxform
from tests import parity_cases as pc
from tests import verify_cases as vc
from tsxform import synth

nat = tsxform._native
FIELDS = ("status", "dst_off", "dst_len", "dst_cap", "crc32c", "src_off", "src_len")


def chunks():
    return [synth.gen_chunk("K", 52, 0, 3, 20000), synth.gen_chunk("R", 33, 0, 1, 1000), synth.gen_chunk("K", 52, 0, 4, 9000), np.zeros(5000, np.uint8)]


def check_failed_chunk_in_packed_batch(N):
    """Flags x (pooled, explicit context) x (no damage, frame of chunk 0 / 1 / 3 damaged at byte 8) x (zero-copy, copies) -> combinations run."""
    batch = chunks()
    n = len(batch)
    sizes = [int(c.size) for c in batch]
    zc = N.lib.tsx_debug_last_zero_copy; zc.restype = ctypes.c_int; zc.argtypes = [ctypes.c_void_p]
    ctx = N.ctx_create(0, 0, 0)
    ran = 0
    try:
        for flags in (vc.VF, vc.VF | nat.ENCRYPT | nat.CRC):
            soff, doff, caps, st, _ = pc.layout(sizes, flags, N)
            src = np.zeros(st, np.uint8)
            for c, o_ in zip(batch, soff):
                src[o_:o_ + c.size] = c
            slot = (N.transformed_bound(max(sizes), flags) + 63) // 64 * 64
            p = nat.Native.make_params(flags, synth.KEY, synth.AAD)
            for pooled in (True, False):
                clean = None
                for damaged in (None, 0, 1, 3):
                    res = {}
                    for copies in (0, 1):
                        what = (flags, pooled, damaged, copies)
                        dst = np.full(n * slot + 64, 0xEE, np.uint8)
                        d = pc.make_descs(sizes, soff, doff, caps)
                        N.host_register(dst)
                        try:
                            with N.configured(zero_copy_packed=1, no_zero_copy_out=copies, verify_damage_frame_chunk=-1 if damaged is None else damaged,
                                              verify_damage_frame_off=8):
                                N.transform_batch(p, d, src, dst, dst.size, nat.MEM_HOST_PACKED, ctx=None if pooled else ctx)
                                if not pooled:
                                    assert zc(ctx) == 1 - copies, what
                        finally:
                            N.host_unregister(dst)
                        ran += 1
                        want = [vc.E_VERIFY if i == damaged else 0 for i in range(n)]
                        assert [int(x) for x in d["status"]] == want, (what, list(d["status"]))
                        at = 0
                        for i in range(n):                              # a failed chunk's dst_off is therefore its successor's
                            assert int(d["dst_off"][i]) == at, (what, i, list(d["dst_off"]), list(d["dst_len"]))
                            at += int(d["dst_len"][i])
                        if damaged is not None:
                            assert int(d["dst_len"][damaged]) == 0, what
                        outs = [dst[int(d["dst_off"][i]):int(d["dst_off"][i]) + int(d["dst_len"][i])].tobytes() for i in range(n)]
                        res[copies] = (outs, d.copy())
                        if damaged is None and copies == 0:
                            clean = outs
                            assert all(len(x) > 0 for x in clean), what
                        for i in range(n):
                            if i != damaged:
                                assert outs[i] == clean[i], (what, i)
                    for f in FIELDS:                                    # zero-copy against copies, field for field
                        assert (res[0][1][f] == res[1][1][f]).all(), (flags, pooled, damaged, f, list(res[0][1][f]), list(res[1][1][f]))
                    assert (res[0][1]["iv"] == res[1][1]["iv"]).all() and res[0][0] == res[1][0], (flags, pooled, damaged)
    finally:
        N.ctx_destroy(ctx)
    return ran
