"""Verify on upload (TSX_VERIFY) on the device: the emulator's checks against the product library (clean frames at levels 1-3, flipped
source bits, damaged frames), then what only the device can run - full-size chunks, the two natural ways into phase two (a chunk above
16 MiB, a frame of more than 264 blocks), and verifying uploads from four threads next to a fetching one.  (Named to run after the other
GPU files.)"""
import multiprocessing as mp
import threading
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

import tsxform
from tests import checksum_cases as cc
from tests import parity_cases as pc
from tests import verify_cases as vc
from tests import zstd_inspect as zi
from tsxform import synth

nat = tsxform._native
pytestmark = pytest.mark.gpu
MiB = 1 << 20


@pytest.fixture()
def ctx(gpu):
    h = gpu.ctx_create(0, 0, 0)
    yield h
    gpu.ctx_destroy(h)


def _gen_b(c):
    return synth.gen_chunk("B", 61, 0, c, 4 * MiB)


_B = None


def b_chunks():
    """Eight 4 MiB chunks of Kafka v2 record batches (seconds each on one core: generated side by side, once)."""
    global _B
    if _B is None:
        with ProcessPoolExecutor(8, mp_context=mp.get_context("spawn")) as ex:
            _B = list(ex.map(_gen_b, range(8)))
    return _B


# ---- the emulator's checks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level,profile,checksum,mem", [
    (3, nat.ZSTD_PROFILE_1_5_7, False, None), (3, nat.ZSTD_PROFILE_1_5_7, True, "device"), (1, nat.ZSTD_PROFILE_1_5_7, True, "packed"),
    (2, nat.ZSTD_PROFILE_1_5_7, False, "device"), (3, nat.ZSTD_PROFILE_1_5_6, True, None), (1, nat.ZSTD_PROFILE_1_5_6, False, "packed"),
    (2, nat.ZSTD_PROFILE_1_5_6, True, None)])
def test_clean_frames_pass_in_the_block_form_on_the_device(gpu, oracle, ctx, level, profile, checksum, mem):
    vc.check_clean(gpu, oracle, ctx, vc.clean_chunks(), level, profile, checksum, mem)


def test_the_flag_is_validated_on_the_device(gpu, oracle):
    for flags in (nat.VERIFY, nat.VERIFY | nat.CRC, nat.VERIFY | nat.ENCRYPT):
        assert cc.transform_rc(gpu, flags) == nat.E_INVAL, flags
    assert cc.transform_rc(gpu, vc.VF | nat.ENCRYPT | nat.CRC) == 0


@pytest.mark.parametrize("fallback", [False, True])
def test_six_flipped_source_bits_each_fail_their_chunk_on_the_device(gpu, oracle, ctx, fallback):
    K = vc.damage_targets()[0]
    sp = vc.sequence_positions(oracle, K)
    targets = [(0, 0), (0, K.size - 1), (0, 131072), (0, sp["match"]), (0, sp["literal"]), (0, sp["run_last"])]
    vc.check_source_damage(gpu, ctx, vc.VF | nat.ENCRYPT | nat.CRC, targets, fallback=fallback)


def test_a_damaged_frame_fails_its_chunk_on_the_device(gpu, oracle, ctx):
    assert vc.check_frame_damage(gpu, ctx) == 2 * 5 + 3 * 4


# ---- full-size chunks ------------------------------------------------------------------------------------------------------
def test_full_size_chunks_verify_clean_and_are_libzstds_bytes(gpu, oracle, ctx):
    """16 x 4 MiB K, 8 x 4 MiB B and one 6 MiB chunk in one device-memory batch: every chunk judged by the block form, TSX_OK, and the
    frames byte for byte libzstd 1.5.7's; the verifier's launches and time are in tsx_timing."""
    cc.need157(oracle)
    chunks = [synth.gen_chunk("K", 9, 1, i) for i in range(16)] + b_chunks() + [pc.big_chunk("K6")]
    outs, d, _ = cc.run_transform(gpu, vc.VF | nat.ZSTD_CHECKSUM | nat.CRC, chunks, 3, mem="device", ctx=ctx)
    assert (d["status"] == 0).all(), list(d["status"])
    assert vc.counts(gpu, ctx) == (len(chunks), 0)
    t = gpu.ctx_timing(ctx)
    print("verifier: %.2f ms, %d launches, for %d chunks (%d MiB); compression %.1f ms" % (t.unzstd_ms, t.unzstd_launches, len(chunks),
                                                                                          sum(int(c.size) for c in chunks) // MiB, t.zstd_ms))
    assert t.unzstd_launches > 0 and t.unzstd_ms > 0
    for i, c in enumerate(chunks):
        assert outs[i] == cc.frame(oracle, c, 3), i


def test_a_chunk_above_16_MiB_is_verified_in_phase_two(gpu, oracle, ctx):
    x = np.concatenate([synth.gen_chunk("K", 12, 0, c) for c in range(5)])[:17 * MiB]
    outs, d, _ = cc.run_transform(gpu, vc.VF, [x], 3, mem="device", ctx=ctx)
    assert d["status"][0] == 0 and vc.counts(gpu, ctx) == (0, 1)
    assert oracle.zstd_decompress_chunk(outs[0], x.size) == x.tobytes()
    with gpu.configured(verify_damage_src_chunk=0, verify_damage_src_off=16 * MiB + 12345):
        outs, d, _ = cc.run_transform(gpu, vc.VF, [x], 3, mem="device", ctx=ctx)
    assert d["status"][0] == nat.E_VERIFY and d["dst_len"][0] == 0 and vc.counts(gpu, ctx) == (0, 1)


def test_a_frame_of_more_than_264_blocks_is_verified_in_phase_two(gpu, oracle, ctx):
    """8 MiB of record batches under profile 1.5.7: the pre-splitter cuts its 64 full blocks into more than the block form takes."""
    cc.need157(oracle)
    B = b_chunks()
    x = np.concatenate([B[0], B[1]])
    want = oracle.zstd_compress_chunk(x.tobytes())
    assert len(zi.parse_frame(want, decode=False)[1]) > 264
    outs, d, _ = cc.run_transform(gpu, vc.VF, [x, B[2]], 3, mem="device", ctx=ctx)
    assert (d["status"] == 0).all() and outs[0] == want
    assert vc.counts(gpu, ctx) == (1, 1)


# ---- under load ------------------------------------------------------------------------------------------------------------
def test_verifying_uploads_from_four_threads_next_to_a_fetching_one(gpu, oracle):
    """Four threads x 2 batches x 64 chunks of 1 MiB with verification on (pooled contexts: one verifier workspace between them) while a
    fifth thread fetches single chunks: every chunk TSX_OK, the frames the ones a batch without the flag writes (libzstd's, where it is
    there to ask), every fetch returns its chunk, and nothing is left in flight."""
    flags = nat.COMPRESS | nat.ENCRYPT | nat.CRC
    chunks = [synth.gen_chunk("K" if i % 2 else "R", 71, 0, i, MiB) for i in range(8)]
    chunks = [chunks[i % 8] if i % 8 else synth.gen_chunk("K", 71, 1, i, MiB) for i in range(64)]
    want, d0, _ = cc.run_transform(gpu, flags, chunks, 3)
    assert (d0["status"] == 0).all()
    if oracle.zstd_version().startswith("1.5.7"):
        for i in (0, 1, 8, 63):
            assert want[i] == oracle.gcm_encrypt_chunk(synth.KEY, synth.iv_for(0, i), synth.AAD, oracle.zstd_compress_chunk(chunks[i].tobytes()))
    errors, stop, fetched = [], threading.Event(), [0]

    def uploader(t):
        try:
            for _ in range(2):
                outs, d, _ = cc.run_transform(gpu, flags | nat.VERIFY, chunks, 3)
                assert (d["status"] == 0).all(), list(d["status"])
                assert outs == want
        except Exception as e:                                          # noqa: BLE001 (reported below)
            errors.append((t, repr(e)))

    def fetcher():
        try:
            while not stop.is_set():
                i = fetched[0] % 64
                back, d = pc.run_detransform(gpu, flags, [want[i]], [MiB])
                assert d["status"][0] == 0 and back[0] == chunks[i].tobytes(), i
                fetched[0] += 1
        except Exception as e:                                          # noqa: BLE001
            errors.append(("fetch", repr(e)))
    ts = [threading.Thread(target=uploader, args=(t,)) for t in range(4)]
    ft = threading.Thread(target=fetcher)
    ft.start()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    stop.set()
    ft.join()
    assert not errors, errors
    assert fetched[0] >= 1
    gpu.service_quiesce(0)
    assert gpu.pool_stats(0)["in_use"] == 0
    outs, d, _ = cc.run_transform(gpu, flags | nat.VERIFY, chunks[:4], 3)
    assert (d["status"] == 0).all() and outs == want[:4]
