"""Zstandard content checksum on the device, where a wave's lanes run in lockstep and the hash's lane exchange is real: the checks of
tests/test_emu_zstd_checksum.py against the product library (byte identity with libzstd 1.5.7 + ZSTD_c_checksumFlag, the full chain,
slot capacity, both decoder forms on good and damaged frames, validation, members side by side), then what only the device can run -
full 4 MiB and 6 MiB chunks, and a 16-chunk fetch in the block form with one damaged chunk.  (Named to run after the other GPU files.)"""
import numpy as np
import pytest

import tsxform
from tests import checksum_cases as cc
from tests import parity_cases as pc
from tests import test_emu_zstd_checksum as E
from tsxform import synth

nat = tsxform._native
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("level", [1, 2, 3])
def test_checksummed_frames_are_byte_identical_to_libzstd_on_the_device(gpu, oracle, level):
    E.test_checksummed_frames_are_byte_identical_to_libzstd(gpu, oracle, level)


def test_the_wave_hash_at_odd_and_8_byte_offsets_on_the_device(gpu, oracle):
    E.test_the_wave_hash_at_odd_and_8_byte_offsets(gpu, oracle)


@pytest.mark.parametrize("mem", [None, "device", "packed"])
def test_full_chain_with_checksum_on_the_device(gpu, oracle, mem):
    E.test_full_chain_with_checksum_matches_libzstd_and_the_oracles_gcm(gpu, oracle, mem)


def test_staged_path_emits_the_same_bytes_on_the_device(gpu, oracle):
    E.test_staged_path_emits_the_same_bytes(gpu, oracle)


@pytest.mark.parametrize("mem", [None, "device"])
def test_a_slot_without_room_for_the_checksum_is_too_small_on_the_device(gpu, oracle, mem):
    E.test_a_slot_without_room_for_the_checksum_is_too_small(gpu, oracle, mem)


@pytest.mark.parametrize("level", [1, 3, 19])
def test_libzstds_checksummed_frames_decode_in_both_forms_on_the_device(gpu, oracle, level):
    E.test_libzstds_checksummed_frames_decode_in_both_forms(gpu, oracle, level)


def test_damaged_checksummed_frames_are_bad_frames_in_both_forms_on_the_device(gpu, oracle):
    E.test_damaged_checksummed_frames_are_bad_frames_in_both_forms(gpu, oracle)


def test_only_the_damaged_chunk_of_a_mixed_batch_fails_on_the_device(gpu, oracle):
    E.test_only_the_damaged_chunk_of_a_mixed_batch_fails(gpu, oracle)


def test_the_flag_is_validated_on_the_device(gpu, oracle):
    E.test_the_flag_needs_compression_on_transform_and_is_ignored_on_detransform(gpu, oracle)


def test_members_with_and_without_the_flag_share_the_queue_on_the_device(gpu, oracle):
    E.test_members_with_and_without_the_flag_share_the_queue(gpu, oracle)


# ---- full-size chunks ----------------------------------------------------------------------------------------------------
def _big_inputs():
    return {"K 4 MiB": synth.gen_chunk("K", 9, 1, 3), "B 4 MiB": synth.gen_chunk("B", 9, 1, 5, synth.CHUNK), "K 6 MiB": pc.big_chunk("K6")}


def test_full_size_chunks_with_checksum_and_back_through_both_forms(gpu, oracle):
    """One 4 MiB K chunk, one 4 MiB B chunk and one 6 MiB chunk at level 3 with the flag: byte for byte libzstd's frames (the last four
    bytes are the wave's hash of 131072 and 196608 stripes), restored by the block form and by the chunk form, CRC32C as before."""
    cc.need157(oracle)
    inputs = _big_inputs()
    vals = list(inputs.values())
    outs, d, _ = cc.run_transform(gpu, cc.CK | nat.CRC, vals, 3, mem="device")
    want = [cc.frame(oracle, v, 3) for v in vals]
    for i, name in enumerate(inputs):
        assert d["status"][i] == 0 and outs[i] == want[i], name
    res = cc.decode_both_forms(gpu, nat.COMPRESS | nat.CRC, outs, [int(v.size) for v in vals])
    for form, (back, d2, kept) in res.items():
        assert (d2["status"] == 0).all() and (d2["crc32c"] == d["crc32c"]).all(), form
        for i, name in enumerate(inputs):
            assert back[i] == vals[i].tobytes(), (form, name)
    assert res["block"][2] == len(vals)


def test_a_16_chunk_fetch_in_the_block_form_with_one_damaged_chunk(gpu, oracle):
    """libzstd's checksummed level-3 frames of 16 chunks; chunk 5's frame has one byte flipped inside a raw literals section (libzstd
    itself rejects it): fifteen chunks come back exact from the block form, chunk 5 is TSX_E_BAD_FRAME with nothing restored."""
    cc.need157(oracle)
    inputs = [synth.gen_chunk("K", 51, 0, i, 150000 + 10007 * i) for i in range(16)]
    inputs[5] = cc.rawlit_input(200000)
    blobs = [cc.frame(oracle, x, 3) for x in inputs]
    secs = cc.raw_sections(blobs[5])[1]
    assert secs, "chunk 5 has no raw literals section"
    blobs[5] = cc.flip(blobs[5], secs[0][0] + secs[0][1] // 2)
    assert cc.libzstd_rejects(oracle, blobs[5], inputs[5].size) is not None
    ctx = gpu.ctx_create(0, 0, 0)
    try:
        outs, d = pc.run_detransform(gpu, nat.COMPRESS | nat.CRC, blobs, [int(x.size) for x in inputs], ctx=ctx)
        kept = pc.blockmode_chunks(gpu, ctx, 16)
    finally:
        gpu.ctx_destroy(ctx)
    assert kept == 15
    for i, x in enumerate(inputs):
        if i == 5:
            assert d["status"][i] == nat.E_BAD_FRAME and d["dst_len"][i] == 0
        else:
            assert d["status"][i] == 0 and outs[i] == x.tobytes() and int(d["crc32c"][i]) == oracle.crc32c(x.tobytes()), i
