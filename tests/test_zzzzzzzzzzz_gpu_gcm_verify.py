"""Verify on upload, AES-GCM stage (TSX_VERIFY_GCM) on the device: the emulator's clean and damage matrices on the product library
(tests/gcm_verify_cases.py), and what the emulator cannot afford - full-size chunks in registered host buffers, slot and packed layout
(the verifier reads the caller's buffer back over PCIe), and a batch that travels through the piece pipeline."""
import ctypes

import numpy as np
import pytest

import tsxform
from tests import checksum_cases as cc
from tests import gcm_verify_cases as gv
from tests import parity_cases as pc
from tsxform import synth

nat = tsxform._native
pytestmark = pytest.mark.gpu
PATHS = [("zero_copy", {}), ("zero_copy", {"no_zero_copy_out": 1}), ("host", {}), ("device", {}), ("packed", {}), ("packed_zc", {}),
         ("zero_copy", {"stages_separate": 1}), ("device", {"stages_separate": 1})]


@pytest.fixture()
def ctx(gpu):
    h = gpu.ctx_create(0, 0, 0)
    yield h
    gpu.ctx_destroy(h)


def _zero_copy(N, ctx):
    f = N.lib.tsx_debug_last_zero_copy; f.restype = ctypes.c_int; f.argtypes = [ctypes.c_void_p]
    return f(ctx)


def test_the_flag_needs_encryption(gpu):
    g = gv.VG
    for flags in (g, g | nat.CRC, g | nat.COMPRESS):
        assert cc.transform_rc(gpu, flags) == nat.E_INVAL, flags
    for flags in (g | gv.ENC, g | gv.CE | nat.CRC, g | gv.CE | nat.CRC | nat.ZSTD_CHECKSUM | nat.VERIFY):
        assert cc.transform_rc(gpu, flags) == 0, flags
    for flags in (0x10 | gv.CE, 0x40 | gv.CE):
        assert cc.transform_rc(gpu, flags) == nat.E_INVAL, flags


@pytest.mark.parametrize("mem", ["zero_copy", "host", "device", "packed"])
def test_clean_encrypt_only_chunks_pass_and_are_openssl_s_bytes(gpu, oracle, ctx, mem):
    chunks = gv.enc_chunks()
    flags = gv.ENC | nat.CRC
    want, d0 = gv.run_transform(gpu, flags, chunks, mem, ctx=ctx)
    plain = gpu.ctx_timing(ctx).gcm_launches
    assert (d0["status"] == 0).all()
    for i, c in enumerate(chunks):
        assert want[i] == pc.oracle_transform(oracle, flags, c, i), (mem, i)
    gv.check_clean(gpu, flags, chunks, mem, ctx=ctx, want=want)
    assert gpu.ctx_timing(ctx).gcm_launches > plain > 0
    assert _zero_copy(gpu, ctx) == (1 if mem == "zero_copy" else 0)


def test_clean_compressed_chunks_pass_on_every_path_of_the_front_end(gpu, oracle, ctx):
    chunks = gv.comp_chunks()
    flags = gv.CE | nat.CRC
    want, d0 = gv.run_transform(gpu, flags, chunks, "zero_copy", ctx=ctx)
    assert (d0["status"] == 0).all() and _zero_copy(gpu, ctx) == 1
    for i, c in enumerate(chunks):
        assert want[i] == pc.oracle_transform(oracle, flags, c, i), i
    for mem, cfg in PATHS:
        gv.check_clean(gpu, flags, chunks, mem, ctx=ctx, want=want, **cfg)
    gv.check_clean(gpu, flags, chunks, "zero_copy", ctx=None, want=want)                    # a pooled context
    gv.check_clean(gpu, flags | nat.VERIFY | nat.ZSTD_CHECKSUM, chunks, "zero_copy", ctx=ctx)
    for level in (1, 2):
        gv.check_clean(gpu, flags, chunks, "zero_copy", level=level, ctx=ctx)
    members = gpu.lib.tsx_debug_last_members; members.restype = ctypes.c_int; members.argtypes = [ctypes.c_void_p]
    sixteen = [synth.gen_chunk("K" if i % 2 else "R", 53, 0, i, 2000 + 1001 * i) for i in range(16)]
    gv.check_clean(gpu, flags, sixteen, "zero_copy", ctx=ctx)
    assert members(ctx) == 2


def test_every_damaged_position_fails_its_chunk_alone(gpu, ctx):
    for flags, chunks in ((gv.ENC, gv.damage_enc_chunks()), (gv.CE, gv.damage_comp_chunks())):
        base = gv.check_clean(gpu, flags, chunks, "zero_copy", ctx=ctx)
        at = gv.targets(base)
        assert (0 if flags == gv.CE else 1, 12 + 65536) in at
        assert gv.check_damage(gpu, flags, chunks, "zero_copy", at, ctx=ctx, base=base) == len(at)


@pytest.mark.parametrize("mem,cfg", PATHS)
def test_tag_and_ciphertext_damage_on_every_path_of_the_front_end(gpu, ctx, mem, cfg):
    for flags, chunks in ((gv.ENC | nat.CRC, gv.damage_enc_chunks()), (gv.CE | nat.CRC, gv.damage_comp_chunks())):
        base = gv.check_clean(gpu, flags, chunks, mem, ctx=ctx, **cfg)
        assert gv.check_damage(gpu, flags, chunks, mem, gv.targets(base, full=False), ctx=ctx, base=base, **cfg) == 2 * len(chunks)


def test_both_verifiers_and_the_key_schedule(gpu, ctx):
    residue = gpu.lib.tsx_debug_key_residue; residue.restype = ctypes.c_int; residue.argtypes = [ctypes.c_void_p]
    chunks = gv.damage_comp_chunks() + [synth.gen_chunk("K", 53, 0, 5, 3000)]
    flags = gv.CE | nat.VERIFY
    base = gv.check_clean(gpu, flags, chunks, "zero_copy", ctx=ctx)
    outs, d = gv.run_transform(gpu, flags | gv.VG, chunks, "zero_copy", ctx=ctx, verify_damage_src_chunk=0, verify_damage_src_off=100,
                               verify_damage_out_chunk=1, verify_damage_out_off=len(base[1]) - 1)
    assert [int(x) for x in d["status"]] == [gv.E_VERIFY, gv.E_VERIFY, 0] and outs[2] == base[2] and list(d["dst_len"][:2]) == [0, 0]
    assert residue(ctx) == 0


_BIG = None


def _big():
    """One K and one R chunk of 4 MiB, their clean outputs in both layouts (compress + encrypt + CRC), made once."""
    global _BIG
    if _BIG is None:
        _BIG = {"chunks": [synth.gen_chunk("K", 11, 0, 1, 4 << 20), synth.gen_chunk("R", 11, 0, 0, 4 << 20)]}
    return _BIG


@pytest.mark.parametrize("mem", ["zero_copy", "packed_zc"])
def test_full_size_chunks_in_registered_host_buffers(gpu, mem):
    """Pooled contexts, as the broker's upload threads use them: the waves write the caller's registered buffer, the verifier reads it back."""
    big = _big()
    chunks = big["chunks"]
    flags = gv.CE | nat.CRC
    clean, d = gv.run_transform(gpu, flags | gv.VG, chunks, mem)
    assert (d["status"] == 0).all() and big.setdefault("clean", clean) == clean          # both layouts: the same bytes
    back, d2 = pc.run_detransform(gpu, flags, clean, [int(c.size) for c in chunks])
    assert (d2["status"] == 0).all() and back == [c.tobytes() for c in chunks] and (d2["crc32c"] == d["crc32c"]).all()
    Lk, Lr = len(clean[0]) - 28, len(clean[1]) - 28
    assert Lk > (1 << 20) and Lr > (4 << 20)
    at = [(0, 12), (1, 12 + (Lr - 1) // 65536 * 65536 + 5), (0, 12 + Lk + 15)]    # first ciphertext byte; a byte of the last sub-block; the last tag byte
    assert gv.check_damage(gpu, flags, chunks, mem, at, base=clean, unflagged=False) == 3


@pytest.mark.parametrize("mem", ["zero_copy", "host"])
def test_a_batch_through_the_piece_pipeline(gpu, ctx, mem):
    chunks = [synth.gen_chunk("K" if i % 2 else "R", 67, 0, i, 65537) for i in range(64)]
    flags = gv.ENC | nat.CRC
    base = gv.check_clean(gpu, flags, chunks, mem, ctx=ctx)
    cut = gv.check_clean(gpu, flags, chunks, mem, ctx=ctx, want=base, sub_bytes=1 << 20)     # four pieces of 16 chunks
    assert cut == base
    assert gv.check_damage(gpu, flags, chunks, mem, [(63, 12 + 65537 + 15), (16, 12 + 65536)], ctx=ctx, base=base, sub_bytes=1 << 20) == 2
