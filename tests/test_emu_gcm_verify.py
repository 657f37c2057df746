"""Verify on upload, AES-GCM stage (TSX_VERIFY_GCM) under the CPU emulator: the flag's validation, clean batches pass and keep their
bytes on every path of the front end, and one damaged byte of the delivered IV || C || TAG - IV, ciphertext or tag - fails that chunk
alone, exactly when the flag is set.  Full-size chunks and the piece pipeline run on the device
(tests/test_zzzzzzzzzzz_gpu_gcm_verify.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import tsxform
from tests import checksum_cases as cc
from tests import gcm_verify_cases as gv
from tests import parity_cases as pc
from tsxform import synth

nat = tsxform._native
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def ctx(emu):
    h = emu.ctx_create(0, 0, 0)
    yield h
    emu.ctx_destroy(h)


def _zero_copy(N, ctx):
    f = N.lib.tsx_debug_last_zero_copy; f.restype = ctypes.c_int; f.argtypes = [ctypes.c_void_p]
    return f(ctx)


# ---- 1. the flag ------------------------------------------------------------------------------------------------------------
def test_the_flag_needs_encryption_on_transform_and_is_ignored_on_detransform(emu, oracle):
    g = nat.VERIFY_GCM
    assert g == 0x80 and gv.VG == g
    for flags in (g, g | nat.CRC, g | nat.COMPRESS, g | nat.COMPRESS | nat.CRC):
        assert cc.transform_rc(emu, flags) == nat.E_INVAL, flags
    for flags in (g | gv.ENC, g | gv.ENC | nat.CRC, g | gv.CE, g | gv.CE | nat.CRC, g | gv.CE | nat.ZSTD_CHECKSUM, g | gv.CE | nat.VERIFY,
                  g | gv.CE | nat.CRC | nat.ZSTD_CHECKSUM | nat.VERIFY):
        assert cc.transform_rc(emu, flags) == 0, flags
    for flags in (0x10 | gv.CE, 0x40 | gv.CE, 0x10 | gv.CE | g, 0x40 | gv.CE | g):
        assert cc.transform_rc(emu, flags) == nat.E_INVAL, flags
    x = synth.gen_chunk("K", 9, 6, 0, 30000)
    for flags in (gv.ENC, gv.CE):                                       # callers build one flags word for both directions
        outs, d = gv.run_transform(emu, flags | g, [x], "host")
        back, d2 = pc.run_detransform(emu, flags | g, outs, [x.size])
        assert d2["status"][0] == 0 and back[0] == x.tobytes(), flags


def test_the_constant_is_the_same_in_every_layer():
    h = open(os.path.join(ROOT, "include", "tsxform.h")).read()
    jn = open(os.path.join(ROOT, "java", "io", "aiven", "kafka", "tieredstorage", "gpu", "TsxNative.java")).read()
    c = int(re.search(r"#define\s+TSX_VERIFY_GCM\s+(0x[0-9A-Fa-f]+)u", h).group(1), 16)
    j = int(re.search(r"public static final int VERIFY_GCM = (0x[0-9A-Fa-f]+);", jn).group(1), 16)
    assert c == j == nat.VERIFY_GCM == 0x80
    assert re.search(r"#define\s+TSX_ABI_VERSION\s+4\b", h) and nat.ABI_VERSION == 4


# ---- 2. clean, encrypt only -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["zero_copy", "host", "device", "packed"])
def test_clean_encrypt_only_chunks_pass_and_are_openssl_s_bytes(emu, oracle, ctx, mem):
    chunks = gv.enc_chunks()
    flags = gv.ENC | nat.CRC
    want, d0 = gv.run_transform(emu, flags, chunks, mem, ctx=ctx)
    plain = emu.ctx_timing(ctx).gcm_launches
    assert (d0["status"] == 0).all()
    for i, c in enumerate(chunks):
        assert want[i] == pc.oracle_transform(oracle, flags, c, i), (mem, i)
    gv.check_clean(emu, flags, chunks, mem, ctx=ctx, want=want)
    assert emu.ctx_timing(ctx).gcm_launches > plain > 0
    assert _zero_copy(ctx=ctx, N=emu) == (1 if mem == "zero_copy" else 0)


# ---- 3. clean, compress + encrypt -------------------------------------------------------------------------------------------
def test_clean_compressed_chunks_pass_on_every_path_of_the_front_end(emu, oracle, ctx):
    chunks = gv.comp_chunks()
    flags = gv.CE | nat.CRC
    want, d0 = gv.run_transform(emu, flags, chunks, "zero_copy", ctx=ctx)
    assert (d0["status"] == 0).all() and _zero_copy(emu, ctx) == 1 and emu.ctx_timing(ctx).gcm_launches == 0     # (the waves encrypt their own frames)
    for i, c in enumerate(chunks):
        assert want[i] == pc.oracle_transform(oracle, flags, c, i), i
    gv.check_clean(emu, flags, chunks, "zero_copy", ctx=ctx, want=want)
    assert _zero_copy(emu, ctx) == 1 and emu.ctx_timing(ctx).gcm_launches > 0
    for mem, cfg in (("zero_copy", {"stages_separate": 1}), ("zero_copy", {"no_zero_copy_out": 1}), ("host", {}), ("device", {}), ("packed", {}), ("packed_zc", {}),
                     ("device", {"stages_separate": 1})):
        gv.check_clean(emu, flags, chunks, mem, ctx=ctx, want=want, **cfg)
    assert _zero_copy(emu, ctx) == 0
    gv.check_clean(emu, flags, chunks, "packed_zc", ctx=ctx, want=want)
    assert _zero_copy(emu, ctx) == 1
    # the Zstandard verifier in front, the content checksum inside the frame
    gv.check_clean(emu, flags | nat.VERIFY | nat.ZSTD_CHECKSUM, chunks, "zero_copy", ctx=ctx)
    gv.check_clean(emu, flags | nat.VERIFY | nat.ZSTD_CHECKSUM, chunks, "host", ctx=ctx, stages_separate=1)


def test_clean_compressed_chunks_pass_at_the_other_levels_and_as_two_members(emu, ctx):
    small = gv.comp_chunks()[1:]
    for level in (1, 2):
        gv.check_clean(emu, gv.CE, small, "zero_copy", level=level, ctx=ctx)
    members = emu.lib.tsx_debug_last_members; members.restype = ctypes.c_int; members.argtypes = [ctypes.c_void_p]
    sixteen = [synth.gen_chunk("K" if i % 2 else "R", 53, 0, i, 2000 + 1001 * i) for i in range(16)]
    gv.check_clean(emu, gv.CE | nat.CRC, sixteen, "zero_copy", ctx=ctx)
    assert members(ctx) == 2
    gv.check_clean(emu, gv.CE | nat.CRC, sixteen, "packed", ctx=ctx)


# ---- 4. damage --------------------------------------------------------------------------------------------------------------
def test_every_damaged_position_of_an_encrypt_only_chunk_fails_that_chunk_alone(emu, ctx):
    chunks = gv.damage_enc_chunks()
    base = gv.check_clean(emu, gv.ENC, chunks, "zero_copy", ctx=ctx)
    at = gv.targets(base)
    assert (1, 12 + 65535) in at and (1, 12 + 65536) in at and (0, 12 + 17) in at and (0, 12 + 17 + 15) in at and (2, 27) in at and len(at) == 20
    assert gv.check_damage(emu, gv.ENC, chunks, "zero_copy", at, ctx=ctx) == 20


def test_every_damaged_position_of_a_compressed_chunk_fails_that_chunk_alone(emu, ctx):
    chunks = gv.damage_comp_chunks()
    base = gv.check_clean(emu, gv.CE, chunks, "zero_copy", ctx=ctx)
    assert len(base[0]) - 28 > 65791 and len(base[1]) - 28 < 32        # raw blocks: the frame crosses the sub-block edge; a frame of one short block
    at = gv.targets(base)
    assert (0, 12 + 65535) in at and (0, 12 + 65536) in at
    assert gv.check_damage(emu, gv.CE, chunks, "zero_copy", at, ctx=ctx) == len(at)


@pytest.mark.parametrize("mem,cfg", [("zero_copy", {}), ("zero_copy", {"no_zero_copy_out": 1}), ("host", {}), ("device", {}), ("packed", {}), ("packed_zc", {}),
                                     ("zero_copy", {"stages_separate": 1}), ("device", {"stages_separate": 1})])
def test_tag_and_ciphertext_damage_on_every_path_of_the_front_end(emu, ctx, mem, cfg):
    for flags, chunks in ((gv.ENC | nat.CRC, gv.damage_enc_chunks()), (gv.CE | nat.CRC, gv.damage_comp_chunks())):
        base = gv.check_clean(emu, flags, chunks, mem, ctx=ctx, **cfg)
        at = gv.targets(base, full=False)
        assert gv.check_damage(emu, flags, chunks, mem, at, ctx=ctx, **cfg) == 2 * len(chunks)


def test_the_zstandard_verifier_runs_first_and_its_failures_are_skipped(emu, ctx):
    """Both flags, chunk 0's source damaged for the Zstandard verifier and chunk 1's tag for the GCM verifier: each fails its own chunk."""
    chunks = gv.damage_comp_chunks() + [synth.gen_chunk("K", 53, 0, 5, 3000)]
    flags = gv.CE | nat.VERIFY
    base = gv.check_clean(emu, flags, chunks, "zero_copy", ctx=ctx)
    for cfg in ({}, {"stages_separate": 1}):
        outs, d = gv.run_transform(emu, flags | gv.VG, chunks, "zero_copy", ctx=ctx, verify_damage_src_chunk=0, verify_damage_src_off=100,
                                   verify_damage_out_chunk=1, verify_damage_out_off=len(base[1]) - 1, **cfg)
        assert [int(x) for x in d["status"]] == [gv.E_VERIFY, gv.E_VERIFY, 0] and outs[2] == base[2] and list(d["dst_len"][:2]) == [0, 0], cfg
        # a hit on a chunk that has already failed changes nothing for the others
        outs, d = gv.run_transform(emu, flags | gv.VG, chunks, "zero_copy", ctx=ctx, verify_damage_src_chunk=0, verify_damage_src_off=100,
                                   verify_damage_out_chunk=0, verify_damage_out_off=20, **cfg)
        assert [int(x) for x in d["status"]] == [gv.E_VERIFY, 0, 0] and outs[1:] == base[1:], cfg


def test_an_offset_behind_the_chunk_and_a_chunk_that_failed_before_are_left_alone(emu, ctx):
    chunks = gv.damage_enc_chunks()
    base = gv.check_clean(emu, gv.ENC, chunks, "zero_copy", ctx=ctx)
    for j, off in ((0, len(base[0])), (2, 28), (-1, 0), (7, 0)):
        outs, d = gv.run_transform(emu, gv.ENC | gv.VG, chunks, "zero_copy", ctx=ctx, verify_damage_out_chunk=j, verify_damage_out_off=off)
        assert (d["status"] == 0).all() and outs == base, (j, off)
    # chunk 1's slot is too small: it is TSX_E_DST_TOO_SMALL with or without the flag, never examined, and the others verify
    sizes = [int(c.size) for c in chunks]
    soff, doff, caps, st, dt = pc.layout(sizes, gv.ENC, emu)
    src = np.zeros(st, np.uint8)
    for c, o_ in zip(chunks, soff):
        src[o_:o_ + c.size] = c
    dst = np.zeros(dt, np.uint8)
    d = pc.make_descs(sizes, soff, doff, caps); d["dst_cap"][1] = 100
    emu.transform_batch(nat.Native.make_params(gv.ENC | gv.VG, synth.KEY, synth.AAD), d, src, dst, dst.size, ctx=ctx)
    assert [int(x) for x in d["status"]] == [0, nat.E_DST_TOO_SMALL, 0] and d["dst_len"][1] == 0
    assert [dst[doff[i]:doff[i] + int(d["dst_len"][i])].tobytes() for i in (0, 2)] == [base[0], base[2]]


def test_no_memory_for_the_verifier_is_said_per_chunk(emu):
    """The one allocation of a compressing batch's GCM verifier - its pinned verdict words - fails: no chunk has been examined, so none is
    TSX_OK.  (An encrypt-only batch verifies in stream and allocates nothing.)"""
    emu.lib.hipemu_fail_alloc_at.argtypes = [ctypes.c_long]; emu.lib.hipemu_alloc_calls.restype = ctypes.c_long
    chunks = [synth.gen_chunk("K", 57, 0, 0, 30000), synth.gen_chunk("R", 57, 0, 1, 15000), np.zeros(0, np.uint8)]
    h = emu.ctx_create(0, 0, 0)
    try:
        want, d0 = gv.run_transform(emu, gv.CE, chunks, "host", ctx=h)  # (the context has its workspace: the verifier's words are the one allocation left)
        assert (d0["status"] == 0).all()
        emu.lib.hipemu_fail_alloc_at(1)
        try:
            outs, d = gv.run_transform(emu, gv.CE | gv.VG, chunks, "host", ctx=h)
            reached = emu.lib.hipemu_alloc_calls()
        finally:
            emu.lib.hipemu_fail_alloc_at(0)
        assert reached >= 1 and (d["status"] == nat.E_NOMEM).all() and (d["dst_len"] == 0).all() and outs == [b""] * 3
        gv.check_clean(emu, gv.CE, chunks, "host", ctx=h, want=want)
    finally:
        emu.ctx_destroy(h)


def test_the_key_schedule_does_not_stay_on_the_device(emu, ctx):
    residue = emu.lib.tsx_debug_key_residue; residue.restype = ctypes.c_int; residue.argtypes = [ctypes.c_void_p]
    chunks = gv.damage_comp_chunks()
    for flags, cfg in ((gv.CE, {}), (gv.CE, {"stages_separate": 1}), (gv.ENC, {})):
        gv.check_clean(emu, flags, chunks, "zero_copy", ctx=ctx, **cfg)
        assert residue(ctx) == 0, (flags, cfg)
        gv.run_transform(emu, flags | gv.VG, chunks, "zero_copy", ctx=ctx, verify_damage_out_chunk=0, verify_damage_out_off=40, **cfg)
        assert residue(ctx) == 0, (flags, cfg)
