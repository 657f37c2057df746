"""Record-batch validation (TSX_VALIDATE_RECORDS) on the device: the matrices of tests/test_emu_records.py on the product library, and two
4 MiB chunks of one valid stream in registered host buffers."""
import numpy as np
import pytest

import tsxform
from tests import parity_cases as pc
from tests import records_cases as rc
from tests import test_emu_records as emu_tests
from tsxform import synth

nat = tsxform._native
pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx(gpu):
    h = gpu.ctx_create(0, 0, 0)
    yield h
    gpu.ctx_destroy(h)


@pytest.fixture(scope="module")
def segment():
    return rc.valid_segment(300000)


def test_the_flag_goes_with_every_stage_combination_and_detransform_ignores_it(gpu):
    emu_tests.test_the_flag_goes_with_every_stage_combination_and_detransform_ignores_it(gpu)


def test_a_batch_without_chunks_or_without_bytes_is_a_clean_stream(gpu, ctx):
    emu_tests.test_a_batch_without_chunks_or_without_bytes_is_a_clean_stream(gpu, ctx)


@pytest.mark.parametrize("size,empties", [(rc.CUT, ()), (rc.CUT, (0, 40)), (65536, ()), (65536, (2, 3)), (1 << 20, ())])
def test_a_clean_segment_passes_in_every_cut_and_keeps_its_bytes(gpu, ctx, segment, size, empties):
    emu_tests.test_a_clean_segment_passes_in_every_cut_and_keeps_its_bytes(gpu, ctx, segment, size, empties)


@pytest.mark.parametrize("mem", rc.MEMS)
def test_a_clean_segment_passes_on_every_memory_kind(gpu, ctx, segment, mem):
    emu_tests.test_a_clean_segment_passes_on_every_memory_kind(gpu, ctx, segment, mem)


def test_a_clean_segment_passes_through_the_piece_pipeline_and_the_compressor(gpu, ctx, segment):
    emu_tests.test_a_clean_segment_passes_through_the_piece_pipeline_and_the_compressor(gpu, ctx, segment)


def test_a_header_split_at_every_byte_and_a_batch_that_ends_on_a_chunk_end(gpu, ctx):
    emu_tests.test_a_header_split_at_every_byte_and_a_batch_that_ends_on_a_chunk_end(gpu, ctx)


def test_one_damaged_byte_hostile_lengths_and_bad_stream_ends(gpu, ctx, segment):
    emu_tests.test_one_damaged_byte_hostile_lengths_and_bad_stream_ends(gpu, ctx, segment)


def test_damage_is_found_on_the_other_paths_too(gpu, ctx, segment):
    emu_tests.test_damage_is_found_on_the_other_paths_too(gpu, ctx, segment)


def test_a_chunk_that_carries_another_error_keeps_it(gpu, ctx, segment):
    emu_tests.test_a_chunk_that_carries_another_error_keeps_it(gpu, ctx, segment)


@pytest.mark.parametrize("mem,cfg", [("zero_copy", {}), ("host", {}), ("packed", {}), ("host", {"stages_separate": 1})])
def test_a_chunk_that_a_verifier_and_the_validator_fail_reports_the_verifier(gpu, ctx, segment, mem, cfg):
    emu_tests.test_a_chunk_that_a_verifier_and_the_validator_fail_reports_the_verifier(gpu, ctx, segment, mem, cfg)


def test_a_valid_batch_inside_a_record_value_is_not_counted(gpu, ctx):
    emu_tests.test_a_valid_batch_inside_a_record_value_is_not_counted(gpu, ctx)


def test_a_damaged_first_batch_of_a_chunk_is_reported_not_skipped(gpu, ctx, segment):
    emu_tests.test_a_damaged_first_batch_of_a_chunk_is_reported_not_skipped(gpu, ctx, segment)


def test_a_batch_longer_than_many_chunks_and_three_thousand_empty_batches(gpu, ctx):
    emu_tests.test_a_batch_longer_than_many_chunks_and_three_thousand_empty_batches(gpu, ctx)


def _two_chunks(N, ctx, flags, stream, packed, level=3):
    """`stream` as two chunks, the first of 4 MiB, source and destination in registered host buffers.  -> (outputs, descs)."""
    sizes = [4 << 20, len(stream) - (4 << 20)]
    soff, doff, caps, st, dt = pc.layout(sizes, flags, N)
    src = np.full(st, 0xA5, np.uint8)
    data = np.frombuffer(stream, np.uint8)
    src[soff[0]:soff[0] + sizes[0]] = data[:sizes[0]]; src[soff[1]:soff[1] + sizes[1]] = data[sizes[0]:]
    slot = (N.transformed_bound(max(sizes), flags) + 63) // 64 * 64
    dst = np.zeros(max(dt, 2 * slot) + 64, np.uint8)
    d = pc.make_descs(sizes, soff, doff, caps)
    p = nat.Native.make_params(flags, synth.KEY, synth.AAD, zstd_level=level)
    N.host_register(src); N.host_register(dst)
    try:
        N.transform_batch(p, d, src, dst, dst.size, nat.MEM_HOST_PACKED if packed else nat.MEM_HOST, ctx=ctx)
    finally:
        N.host_unregister(dst); N.host_unregister(src)
    return [dst[int(d["dst_off"][i]):int(d["dst_off"][i]) + int(d["dst_len"][i])].tobytes() for i in range(2)], d


@pytest.mark.parametrize("packed,flags,level", [(False, nat.ENCRYPT | nat.CRC, 3), (True, nat.COMPRESS | nat.ENCRYPT | nat.CRC, 1)])
def test_two_4_mib_chunks_of_one_stream_in_registered_buffers(gpu, ctx, packed, flags, level):
    stream, (p, l) = rc.gpu_stream()
    assert len(stream) > (7 << 20) and p < (4 << 20) < p + l
    ref = rc.reference_walk(stream)
    assert ref[2:] == (rc.NONE, 0) and ref[0] > 300
    want, d0 = _two_chunks(gpu, ctx, flags, stream, packed, level)
    assert (d0["status"] == 0).all()
    outs, d = _two_chunks(gpu, ctx, flags | rc.VR, stream, packed, level)
    assert (d["status"] == 0).all() and outs == want and list(d["dst_off"]) == list(d0["dst_off"])
    assert rc.info(gpu, ctx) == ref + (0,)
    print("records: %.3f ms for %d bytes in 2 chunks" % (gpu.ctx_records(ctx).ms, len(stream)))
    bad = rc.flip(stream, p + 18)                                       # a crc byte of the batch that crosses the chunk boundary
    refb = rc.reference_walk(bad)
    assert refb[2:] == (p, rc.CRC)
    outs, d = _two_chunks(gpu, ctx, flags | rc.VR, bad, packed, level)
    assert list(d["status"]) == [rc.E_RECORDS, rc.E_RECORDS] and list(d["dst_len"]) == [0, 0] and outs == [b"", b""]
    assert rc.info(gpu, ctx)[:4] == refb
