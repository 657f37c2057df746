"""Record-batch validation of a segment streamed in several calls (tsx_transform_batch_stream) on the device: the matrices of
tests/test_emu_records_stream.py on the product library, and one 8 MiB stream as two calls of one chunk each in registered host buffers -
the smallest shape in which a 4 MiB chunk, zero-copy output and a batch open across two calls meet."""
import numpy as np
import pytest

import tsxform
from tests import parity_cases as pc
from tests import records_cases as rc
from tests import records_stream_cases as rs
from tests import test_emu_records_stream as emu_tests
from tsxform import synth

nat = tsxform._native
pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctxs(gpu):
    hs = [gpu.ctx_create(0, 0, 0) for _ in range(3)]
    yield hs
    for h in hs:
        gpu.ctx_destroy(h)


@pytest.fixture(scope="module")
def segment():
    return rc.valid_segment(300000)


def test_the_rules_of_the_entry_point_and_a_refused_call_leaves_the_state_as_it_was(gpu, ctxs):
    emu_tests.test_the_rules_of_the_entry_point_and_a_refused_call_leaves_the_state_as_it_was(gpu, ctxs)


@pytest.mark.parametrize("mem", rc.MEMS)
def test_one_call_with_the_declared_length_of_its_bytes_equals_the_flag_path(gpu, ctxs, segment, mem):
    emu_tests.test_one_call_with_the_declared_length_of_its_bytes_equals_the_flag_path(gpu, ctxs, segment, mem)


@pytest.mark.parametrize("variant", emu_tests.VARIANTS)
def test_the_call_boundary_at_every_byte_of_a_header_and_around_the_ends(gpu, ctxs, variant):
    emu_tests.test_the_call_boundary_at_every_byte_of_a_header_and_around_the_ends(gpu, ctxs, variant)


def test_a_length_beyond_the_declared_end_and_a_stream_that_ends_inside_a_header(gpu, ctxs):
    emu_tests.test_a_length_beyond_the_declared_end_and_a_stream_that_ends_inside_a_header(gpu, ctxs)


@pytest.mark.parametrize("per", [1, 3, 16])
def test_the_segment_in_calls_of_a_few_chunks_on_a_different_context_per_call(gpu, ctxs, segment, per):
    emu_tests.test_the_segment_in_calls_of_a_few_chunks_on_a_different_context_per_call(gpu, ctxs, segment, per)


@pytest.mark.parametrize("per", [1, 5])
def test_damage_in_calls_of_a_few_chunks_and_every_later_call_is_refused_per_chunk(gpu, ctxs, segment, per):
    emu_tests.test_damage_in_calls_of_a_few_chunks_and_every_later_call_is_refused_per_chunk(gpu, ctxs, segment, per)


def test_a_batch_of_ten_chunks_open_across_five_calls(gpu, ctxs):
    emu_tests.test_a_batch_of_ten_chunks_open_across_five_calls(gpu, ctxs)


def test_a_valid_batch_inside_a_record_value_on_the_first_byte_of_a_call_is_not_counted(gpu, ctxs):
    emu_tests.test_a_valid_batch_inside_a_record_value_on_the_first_byte_of_a_call_is_not_counted(gpu, ctxs)


def test_a_compressing_chain_with_both_verifiers_in_two_calls(gpu, ctxs, segment):
    emu_tests.test_a_compressing_chain_with_both_verifiers_in_two_calls(gpu, ctxs, segment)


def _two_calls(N, ctx, flags, stream, packed, level, declared=None, calls=2):
    """`stream` as two calls of one chunk each, the first of 4 MiB; source and destination of each call in registered host buffers;
    declared: the stream is begun with that length (None: no state, no flag); calls=1: the first call only.  -> ([(output, descs)] per call, state)."""
    state = N.records_begin(declared) if declared is not None else None
    out, at = [], 0
    for size in (4 << 20, len(stream) - (4 << 20))[:calls]:
        soff, doff, caps, st, dt = pc.layout([size], flags, N)
        src = np.full(st, 0xA5, np.uint8)
        src[soff[0]:soff[0] + size] = np.frombuffer(stream, np.uint8)[at:at + size]
        slot = (N.transformed_bound(size, flags) + 63) // 64 * 64
        dst = np.zeros(max(dt, slot) + 64, np.uint8)
        d = pc.make_descs([size], soff, doff, caps)
        d["iv"][0] = np.frombuffer(synth.iv_for(0, len(out)), np.uint8)
        p = nat.Native.make_params(flags, synth.KEY, synth.AAD, zstd_level=level)
        N.host_register(src); N.host_register(dst)
        try:
            N.transform_batch(p, d, src, dst, dst.size, nat.MEM_HOST_PACKED if packed else nat.MEM_HOST, ctx=ctx, state=state)
        finally:
            N.host_unregister(dst); N.host_unregister(src)
        out.append((dst[int(d["dst_off"][0]):int(d["dst_off"][0]) + int(d["dst_len"][0])].tobytes(), d))
        at += size
    return out, state


@pytest.mark.parametrize("packed,flags,level", [(False, nat.ENCRYPT | nat.CRC, 3), (True, nat.COMPRESS | nat.ENCRYPT | nat.CRC, 1)])
def test_an_8_mib_stream_as_two_calls_of_one_chunk_in_registered_buffers(gpu, ctxs, packed, flags, level):
    stream, (p, l) = rc.gpu_stream()
    assert len(stream) > (7 << 20) and p < (4 << 20) < p + l              # that batch is open across the two calls
    ref = rc.reference_walk(stream)
    assert ref[2:] == (rc.NONE, 0) and ref[0] > 300
    want, _ = _two_calls(gpu, ctxs[0], flags, stream, packed, level)
    assert all(d["status"][0] == 0 for _, d in want)
    runs, st = _two_calls(gpu, ctxs[0], flags | rc.VR, stream, packed, level, declared=len(stream))
    assert [int(d["status"][0]) for _, d in runs] == [0, 0] and [o for o, _ in runs] == [o for o, _ in want]
    assert rs.result(gpu, st) == (True, ref)
    print("records, streamed: %.3f ms for the second call of %d bytes" % (gpu.records_result(st)[1].ms, len(stream) - (4 << 20)))
    bad = rc.flip(stream, p + 18)                                       # a crc byte of the batch that is open across the calls
    refb = rc.reference_walk(bad)
    assert refb[2:] == (p, rc.CRC)
    runs, st = _two_calls(gpu, ctxs[1], flags | rc.VR, bad, packed, level, declared=len(bad))
    assert [int(d["status"][0]) for _, d in runs] == [0, rc.E_RECORDS] and int(runs[1][1]["dst_len"][0]) == 0 and runs[1][0] == b""
    wantb, _ = _two_calls(gpu, ctxs[2], flags, bad, packed, level, calls=1)         # call 0 had been delivered before the verdict could fall
    assert runs[0][0] == wantb[0][0] and wantb[0][0] != want[0][0]
    assert rs.result(gpu, st) == (True, refb)
