"""Verify on upload (TSX_VERIFY) under the CPU emulator: the flag's validation, clean frames of every block kind pass (and stay the
bytes they were), and what the block form does not
judge is decoded in full; damage to the source or the frame: tests/test_emu_zstd_verify_damage.py.  Full-size chunks, the natural fallbacks and verification under load run on the device
(tests/test_zzzzzzzz_gpu_zstd_verify.py)."""
import ctypes
import time

import numpy as np
import pytest

import tsxform
from tests import checksum_cases as cc
from tests import gcm_verify_cases as gv
from tests import parity_cases as pc
from tests import verify_cases as vc
from tsxform import synth

nat = tsxform._native


@pytest.fixture()
def ctx(emu):
    h = emu.ctx_create(0, 0, 0)
    yield h
    emu.ctx_destroy(h)


# ---- 1. flag semantics -----------------------------------------------------------------------------------------------------
def test_the_flag_needs_compression_on_transform_and_is_ignored_on_detransform(emu, oracle):
    v = nat.VERIFY
    assert v == 0x20 and nat.E_VERIFY == -10
    for flags in (v, v | nat.CRC, v | nat.ENCRYPT, v | nat.ENCRYPT | nat.CRC):
        assert cc.transform_rc(emu, flags) == nat.E_INVAL, flags
    for flags in (vc.VF, vc.VF | nat.CRC, vc.VF | nat.ENCRYPT | nat.CRC, vc.VF | nat.ZSTD_CHECKSUM):
        assert cc.transform_rc(emu, flags) == 0, flags
    assert cc.transform_rc(emu, 0x40 | nat.COMPRESS) == nat.E_INVAL
    x = synth.gen_chunk("K", 9, 6, 0, 30000)
    outs, d, _ = cc.run_transform(emu, vc.VF, [x], 3)
    for flags in (vc.VF, vc.VF | nat.ZSTD_CHECKSUM, nat.COMPRESS):      # callers build one flags word for both directions
        back, d2 = pc.run_detransform(emu, flags, outs, [x.size])
        assert d2["status"][0] == 0 and back[0] == x.tobytes()
    assert "restore" in emu.strerror(nat.E_VERIFY)


# ---- 2. clean frames -------------------------------------------------------------------------------------------------------
# The whole size / content matrix in every run; the runs cover every level, both profiles, the checksum on and off and the three memory
# kinds (each value of each with at least two values of every other: the emulated compressor needs ~15 s per run of the matrix).
@pytest.mark.parametrize("level,profile,checksum,mem", [
    (3, nat.ZSTD_PROFILE_1_5_7, False, None), (3, nat.ZSTD_PROFILE_1_5_7, True, "device"), (1, nat.ZSTD_PROFILE_1_5_7, True, "packed"),
    (2, nat.ZSTD_PROFILE_1_5_7, False, "device"), (3, nat.ZSTD_PROFILE_1_5_6, True, None), (1, nat.ZSTD_PROFILE_1_5_6, False, "packed"),
    (2, nat.ZSTD_PROFILE_1_5_6, True, None)])
def test_clean_frames_pass_in_the_block_form_and_keep_their_bytes(emu, oracle, ctx, level, profile, checksum, mem):
    vc.check_clean(emu, oracle, ctx, vc.clean_chunks(), level, profile, checksum, mem)


def _small():
    return [synth.gen_chunk("K", 53, 0, 0, 131073), synth.gen_chunk("R", 53, 0, 1, 65791), np.zeros(140000, np.uint8), synth.gen_chunk("K", 53, 0, 2, 7),
            np.zeros(0, np.uint8)]


def test_clean_frames_on_the_other_paths_of_the_front_end(emu, oracle, ctx):
    """Stages as separate launches (verified before the GCM / copy launch), the copy path instead of zero-copy output, a call that
    travels as two members, and a workspace that holds three chunks at a time."""
    chunks = _small()
    enc = nat.COMPRESS | nat.ENCRYPT | nat.CRC | nat.ZSTD_CHECKSUM
    base, d0, _ = cc.run_transform(emu, enc, chunks, 3, ctx=ctx)
    for cfg in ({"stages_separate": 1}, {"no_zero_copy_out": 1}):
        with emu.configured(**cfg):
            vc.check_clean(emu, oracle, ctx, chunks, 3, nat.ZSTD_PROFILE_1_5_7, True, None)
            vc.check_clean(emu, oracle, ctx, chunks, 3, nat.ZSTD_PROFILE_1_5_7, False, "packed")
            outs, d, _ = cc.run_transform(emu, enc | nat.VERIFY, chunks, 3, ctx=ctx)
            assert (d["status"] == 0).all() and outs == base and vc.counts(emu, ctx) == (len(chunks), 0), cfg
    members = emu.lib.tsx_debug_last_members; members.restype = ctypes.c_int; members.argtypes = [ctypes.c_void_p]
    sixteen = [synth.gen_chunk("K" if i % 2 else "R", 53, 0, i, 2000 + 1001 * i) for i in range(16)]
    vc.check_clean(emu, oracle, ctx, sixteen, 3, nat.ZSTD_PROFILE_1_5_7, False, None)
    assert members(ctx) == 2
    with emu.configured(verify_slice_chunks=3):
        vc.check_clean(emu, oracle, ctx, sixteen[:8], 3, nat.ZSTD_PROFILE_1_5_7, True, None)
        vc.check_clean(emu, oracle, ctx, sixteen[:8], 3, nat.ZSTD_PROFILE_1_5_7, True, "device")


# ---- 5. phase two ----------------------------------------------------------------------------------------------------------
def test_forced_fallback_verifies_clean_chunks_in_full(emu, oracle, ctx):
    chunks = _small() + [synth.gen_chunk("B", 53, 0, 3, 70000)]
    with emu.configured(verify_force_fallback=1):
        for checksum in (False, True):
            vc.check_clean(emu, oracle, ctx, chunks, 3, nat.ZSTD_PROFILE_1_5_7, checksum, None, block_form=False)
        vc.check_clean(emu, oracle, ctx, chunks, 1, nat.ZSTD_PROFILE_1_5_6, True, "device", block_form=False)


def test_a_chunk_handed_back_and_restarted_verifies_clean(emu, oracle):
    """A guest wave that gives its chunk up, and a wave the hardware moved onto a reserved CU: another wave starts the chunk again, and
    the frame it finishes is the one that is verified."""
    for f, t in (("hipemu_cu_key_shift", [ctypes.c_int]), ("hipemu_force_yield_after", [ctypes.c_int]), ("hipemu_relocate_after", [ctypes.c_int])):
        getattr(emu.lib, f).argtypes = t; getattr(emu.lib, f).restype = None
    flags = vc.VF | nat.ZSTD_CHECKSUM | nat.ENCRYPT | nat.CRC
    sizes = [200000, 131072 + 5, 30001, 17]
    chunks = [synth.gen_chunk("K" if i % 3 else "B", 31, 1, i, s) for i, s in enumerate(sizes)]
    want, d0, _ = cc.run_transform(emu, flags & ~nat.VERIFY, chunks, 3)
    with emu.configured(fetch_quiet_ms=1):
        time.sleep(0.01)
        emu.service_quiesce(0)
        s0 = emu.service_stats(0)
        emu.lib.hipemu_cu_key_shift(3)
        try:
            for after in (4, 3):
                time.sleep(0.01)
                emu.lib.hipemu_force_yield_after(after)
                got, d, _ = cc.run_transform(emu, flags, chunks, 3)
                assert got == want and (d["status"] == 0).all(), after
        finally:
            emu.lib.hipemu_cu_key_shift(0); emu.lib.hipemu_force_yield_after(0)
        emu.service_quiesce(0)
        s1 = emu.service_stats(0)
        emu.lib.hipemu_cu_key_shift(1)
        try:
            emu.lib.hipemu_relocate_after(4)
            got, d, _ = cc.run_transform(emu, flags, chunks, 3)
            assert got == want and (d["status"] == 0).all()
        finally:
            emu.lib.hipemu_relocate_after(0); emu.lib.hipemu_cu_key_shift(0)
    assert s1["returned_chunks"] - s0["returned_chunks"] >= 1, (s0, s1)


# ---- 6. no memory ----------------------------------------------------------------------------------------------------------
def _armed(emu, k, run):
    """run() with the k-th allocation from here on failing once.  -> run()'s result, once that allocation has been reached."""
    emu.lib.hipemu_fail_alloc_at.argtypes = [ctypes.c_long]; emu.lib.hipemu_alloc_calls.restype = ctypes.c_long
    emu.lib.hipemu_fail_alloc_at(k)
    try:
        res = run()
        reached = emu.lib.hipemu_alloc_calls()
    finally:
        emu.lib.hipemu_fail_alloc_at(0)
    assert reached >= k, (k, reached)
    return res


@pytest.mark.parametrize("k,n,fallback", [(1, 30000, False), (2, 540000, False), (3, 680000, True)])
def test_no_memory_for_the_verifier_is_said_per_chunk(emu, k, n, fallback):
    """Each allocation of a verifying call fails once, on a context that has its own workspace: 1 = the context's pinned verdict words,
    2 = the device's workspace (no chunk of the piece has been examined: every one is TSX_E_NOMEM), 3 = the buffer a chunk is restored
    into in phase two (that chunk alone).  The verifier's workspace and its phase-two buffer belong to the device and outlive every test:
    for their allocation to be reached they must have to GROW, so the batch is larger, in chunks (the empty ones cost nothing) and in
    bytes (n incompressible ones: the emulated compressor is through them at once), than any verifying piece before it - 400000 bytes
    in 40 chunks (tests/verify_cases.py), and n is 140000 more each time.  In phase two the first chunk, larger than any before it, is the one that needs a new buffer.
    Host memory, in one piece: the caller allocates nothing between arming and the call."""
    chunks = [synth.gen_chunk("R", 57, 0, 1, n), synth.gen_chunk("K", 57, 0, 0, 30000)] + [np.zeros(0, np.uint8)] * (1 if k == 1 else 46)
    flags = nat.COMPRESS | nat.ENCRYPT
    one = {"no_pipeline": 1}
    cfg = dict(one, verify_force_fallback=1) if fallback else one
    h = emu.ctx_create(0, 0, 0)
    try:
        want, d0 = gv.run_transform(emu, flags, chunks, "host", ctx=h, **one)
        assert (d0["status"] == 0).all()
        outs, d = _armed(emu, k, lambda: gv.run_transform(emu, flags | nat.VERIFY, chunks, "host", ctx=h, **cfg))
        failed = [0] if fallback else range(len(chunks))
        assert [int(x) for x in d["status"]] == [nat.E_NOMEM if i in failed else 0 for i in range(len(chunks))]
        for i in range(len(chunks)):
            assert (outs[i] == b"" and d["dst_len"][i] == 0) if i in failed else outs[i] == want[i], i
        outs, d = gv.run_transform(emu, flags | nat.VERIFY, chunks, "host", ctx=h, **cfg)
        assert (d["status"] == 0).all() and outs == want
    finally:
        emu.ctx_destroy(h)
