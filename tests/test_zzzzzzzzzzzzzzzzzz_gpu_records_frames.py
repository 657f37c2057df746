"""Record framing and offset order (TSX_VALIDATE_FRAMES) on the device: the matrices of tests/test_emu_records_frames.py on the product
library (a CRC-only chain for the matrices), one compressing and encrypting run of the 290 KB segment in registered buffers, and two 4 MiB
chunks of one valid stream, clean and with one sealed `length` damage in the last batch."""
import pytest

import tsxform
from tests import records_cases as rc
from tests import records_frames_cases as fc
from tests import test_emu_records_frames as emu_tests
from tests import test_zzzzzzzzzzzz_gpu_records as gpu_records

nat = tsxform._native
pytestmark = pytest.mark.gpu
CE = nat.COMPRESS | nat.ENCRYPT


@pytest.fixture()
def ctx(gpu):
    h = gpu.ctx_create(0, 0, 0)
    yield h
    gpu.ctx_destroy(h)


@pytest.fixture(scope="module")
def segment():
    s = rc.valid_segment(300000)
    assert fc.reference_walk_frames(s) == (19, 0, 630, rc.NONE, 0)
    return s


def test_the_flag_modifies_validate_records_and_the_streamed_form_refuses_it(gpu, segment):
    emu_tests.test_the_flag_modifies_validate_records_and_the_streamed_form_refuses_it(gpu, segment)


@pytest.mark.parametrize("mem", rc.MEMS)
def test_a_clean_segment_passes_on_every_memory_kind_and_every_record_is_read(gpu, ctx, segment, mem):
    emu_tests.test_a_clean_segment_passes_on_every_memory_kind_and_every_record_is_read(gpu, ctx, segment, mem)


def test_a_clean_segment_passes_behind_every_chain(gpu, ctx, segment):
    emu_tests.test_a_clean_segment_passes_behind_every_chain(gpu, ctx, segment)


@pytest.mark.parametrize("mem", ["zero_copy", "packed_zc"])
def test_the_whole_segment_compressed_and_encrypted_in_registered_buffers(gpu, ctx, segment, mem):
    sizes = rc.cut(segment, 65536, (2,))
    want, d0 = rc.run(gpu, CE | nat.CRC | rc.VR, segment, sizes, mem, ctx)
    assert (d0["status"] == 0).all() and int(gpu.ctx_records(ctx).records) == 0
    outs, got, rep = fc.check(gpu, CE | nat.CRC, segment, sizes, mem, ctx, want=want)
    assert got == (19, 0, 630, rc.NONE, 0) and rep == 0


def test_the_built_stream_and_its_special_batches(gpu, ctx):
    emu_tests.test_the_built_stream_and_its_special_batches(gpu, ctx)


@pytest.mark.parametrize("size", [rc.CUT, 65536])
def test_the_damage_matrix(gpu, ctx, size):
    emu_tests.test_the_damage_matrix(gpu, ctx, size)


def test_a_badly_framed_batch_inside_a_record_value_is_not_judged(gpu, ctx):
    emu_tests.test_a_badly_framed_batch_inside_a_record_value_is_not_judged(gpu, ctx)


def test_a_damaged_first_batch_of_a_chunk_is_repaired_with_the_uncut_result(gpu, ctx, segment):
    emu_tests.test_a_damaged_first_batch_of_a_chunk_is_repaired_with_the_uncut_result(gpu, ctx, segment)


def test_the_seam_between_two_walkers_is_checked_by_the_resolver(gpu, ctx):
    emu_tests.test_the_seam_between_two_walkers_is_checked_by_the_resolver(gpu, ctx)


def test_seeded_fuzz_against_the_reference(gpu, ctx, segment):
    emu_tests.test_seeded_fuzz_against_the_reference(gpu, ctx, segment)


def test_two_4_mib_chunks_of_one_stream_clean_and_with_a_sealed_length_damage(gpu, ctx):
    stream, (p, l) = rc.gpu_stream()
    assert len(stream) > (7 << 20) and p < (4 << 20) < p + l
    ref = fc.reference_walk_frames(stream)
    assert ref[3:] == (rc.NONE, 0) and ref[0] > 300 and ref[2] > 10000
    flags = nat.ENCRYPT | nat.CRC
    want, d0 = gpu_records._two_chunks(gpu, ctx, flags | rc.VR, stream, False)
    assert (d0["status"] == 0).all()
    outs, d = gpu_records._two_chunks(gpu, ctx, flags | rc.VR | fc.VF, stream, False)
    assert (d["status"] == 0).all() and outs == want and fc.info(gpu, ctx) == ref
    print("records with frames: %.3f ms for %d bytes, %d records in 2 chunks" % (gpu.ctx_records(ctx).ms, len(stream), ref[2]))
    # the last batch of the stream (it begins in the second chunk): its first record one byte shorter than it is, sealed
    p, l = rc.batches_of(stream)[-1]
    assert p > (4 << 20)
    b = bytearray(stream[p:p + l])
    n, q = fc.read_varint(bytes(b), 61, l)
    assert q == 63
    b[61:63] = fc.varint(n - 1)
    bad = stream[:p] + fc.seal(bytes(b))
    refb = fc.reference_walk_frames(bad)
    assert refb[3:] == (p, fc.RECORDS) and refb[0] == ref[0] - 1 and rc.reference_walk(bad)[2:] == (rc.NONE, 0)
    outs, d = gpu_records._two_chunks(gpu, ctx, flags | rc.VR | fc.VF, bad, False)
    assert list(d["status"]) == [0, rc.E_RECORDS] and outs[0] == want[0] and outs[1] == b"" and fc.info(gpu, ctx) == refb
