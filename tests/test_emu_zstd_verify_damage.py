"""Verify on upload (TSX_VERIFY) under the CPU emulator, the failures: one flipped bit anywhere in the source chunk or in the frame
fails that chunk and only that chunk, in the block form and in phase two.  (Flag, clean frames: tests/test_emu_zstd_verify.py.)"""
import pytest

import tsxform
from tests import checksum_cases as cc
from tests import verify_cases as vc

nat = tsxform._native


@pytest.fixture()
def ctx(emu):
    h = emu.ctx_create(0, 0, 0)
    yield h
    emu.ctx_destroy(h)


# ---- 3. every output byte is compared ---------------------------------------------------------------------------------------
def test_one_flipped_source_bit_anywhere_fails_that_chunk_only(emu, oracle, ctx):
    for chunks, targets in vc.split_targets(vc.source_positions(oracle)):
        vc.check_source_damage(emu, ctx, vc.VF, targets, chunks=chunks)


def test_one_flipped_source_bit_anywhere_fails_that_chunk_only_in_phase_two(emu, oracle, ctx):
    for chunks, targets in vc.split_targets(vc.source_positions(oracle)):
        vc.check_source_damage(emu, ctx, vc.VF, targets, chunks=chunks, fallback=True)


def test_source_damage_in_an_encrypted_packed_batch_is_skipped_like_any_failure(emu, oracle, ctx):
    """Packed layout: the failed chunk takes no room, the chunks behind it follow the one before it."""
    flags = vc.VF | nat.ENCRYPT | nat.CRC
    chunks = vc.damage_batch()
    base, d0, _ = cc.run_transform(emu, flags, chunks, 3, mem="packed", ctx=ctx)
    with emu.configured(verify_damage_src_chunk=1, verify_damage_src_off=500):
        outs, d, _ = cc.run_transform(emu, flags, chunks, 3, mem="packed", ctx=ctx)
    assert list(d["status"]) == [0, nat.E_VERIFY, 0, 0] and d["dst_len"][1] == 0
    assert [outs[i] for i in (0, 2, 3)] == [base[i] for i in (0, 2, 3)]
    assert d["dst_off"][2] == d["dst_off"][1] == d["dst_len"][0]


# ---- 4. frame damage -------------------------------------------------------------------------------------------------------
def test_a_damaged_frame_fails_its_chunk(emu, oracle, ctx):
    assert vc.check_frame_damage(emu, ctx) == 2 * 5 + 3 * 4
