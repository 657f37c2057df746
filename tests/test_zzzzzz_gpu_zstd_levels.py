"""Zstandard levels 1 and 2 on the device: full-size chunks byte for byte libzstd 1.5.7's at the same level, the full chain against the
oracle, a 256-chunk B segment at level 1, levels side by side from 16 threads, level 1 next to a fetch that makes guest waves hand
their chunks back, and a differential fuzz of 464 inputs per level - past the window, collision-rich, accelerated - with the 1.5.6 profile
over a part of them.  (The logic, with fewer inputs, runs on the CPU emulator: tests/test_emu_zstd_levels.py - which does not run a
wave's lanes in lockstep: a lane that reads a table word another lane of its wave has just written is tested here alone.)"""
import functools
import threading
import time

import numpy as np
import pytest

import tsxform
from tests import fuzz_cases as fc
from tests import level_cases as lc
from tests import parity_cases as pc
from tests import zstd_inspect as zi
from tsxform import synth

nat = tsxform._native
pytestmark = pytest.mark.gpu
MiB = 1 << 20
CHUNK = 4 * MiB


def _need157(oracle):
    if not oracle.zstd_version().startswith("1.5.7"):
        pytest.skip("libzstd 1.5.7 not available")


@functools.lru_cache(maxsize=1)
def _chunks():
    K = synth.gen_chunk("K", 5, 0, 1, CHUNK); B = synth.gen_chunk("B", 5, 0, 1, CHUNK); R = synth.gen_chunk("R", 5, 0, 1, CHUNK)
    mixed = np.concatenate([K[:MiB], R[:MiB], B[:MiB], np.zeros(MiB // 2, np.uint8), K[MiB:MiB + MiB // 2]])
    big6 = np.concatenate([synth.gen_chunk("K", 6, 0, 0, CHUNK), B[:2 * MiB]])
    big10 = np.concatenate([synth.gen_chunk("B", 7, 0, 0, CHUNK), synth.gen_chunk("K", 7, 0, 1, CHUNK), R[:2 * MiB]])
    return [K, B, R, mixed, big6, big10]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("level", [1, 2])
def test_full_size_chunks_are_libzstds_bytes(gpu, oracle, level):
    _need157(oracle)
    chunks = _chunks()
    outs, d = lc.run_transform(gpu, nat.COMPRESS, chunks, level)
    for i, c in enumerate(chunks):
        assert d["status"][i] == 0
        assert outs[i] == oracle.zstd_compress_chunk(c.tobytes(), level), "chunk %d (%d bytes) at level %d" % (i, c.size, level)
    flags = nat.COMPRESS | nat.ENCRYPT | nat.CRC
    for mem in (None, "device", "packed"):
        outs, d = lc.check_vs_oracle(gpu, oracle, flags, chunks[:4], level, mem=mem)
    lc.check_roundtrip(gpu, flags, chunks[:4], outs)


@pytest.mark.timeout(900)
def test_256_chunk_B_segment_at_level_1(gpu, oracle):
    """A 1 GiB segment of content B in 4 MiB chunks, one batch at level 1 through the full chain, every chunk checked.  (16 distinct chunks,
    each 16 times at different places and IVs: generating B on the host costs ~2 s per chunk.)"""
    _need157(oracle)
    import torch
    dev = torch.device("cuda", 0)
    n = 256
    distinct = [synth.gen_chunk("B", 77, 0, i, CHUNK) for i in range(16)]
    chunks = [distinct[(i * 5) % 16] for i in range(n)]
    flags = nat.COMPRESS | nat.ENCRYPT | nat.CRC
    src = torch.from_numpy(np.concatenate(chunks)).to(dev)
    slot = (gpu.transformed_bound(CHUNK, flags) + 63) // 64 * 64
    dst = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    d = np.zeros(n, nat.DESC_DTYPE); d["src_off"] = np.arange(n, dtype=np.uint64) * CHUNK; d["src_len"] = CHUNK
    d["dst_off"] = np.arange(n, dtype=np.uint64) * slot; d["dst_cap"] = slot
    for i in range(n):
        d["iv"][i] = np.frombuffer(synth.iv_for(0, i), np.uint8)
    p = nat.Native.make_params(flags, synth.KEY, synth.AAD, zstd_level=1)
    gpu.transform_batch(p, d, src.data_ptr(), dst.data_ptr(), dst.numel(), nat.MEM_DEVICE)
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    total = 0
    for i in range(n):
        assert d["status"][i] == 0, i
        got = host[i * slot:i * slot + int(d["dst_len"][i])].tobytes()
        assert got == lc.expected(oracle, flags, 1, i, chunks[i]), "chunk %d" % i
        assert int(d["crc32c"][i]) == oracle.crc32c(chunks[i].tobytes())
        total += len(got)
    print("B x 256 at level 1: transformed / original = %.4f" % (total / (n * CHUNK)))


@pytest.mark.timeout(600)
def test_levels_1_2_3_concurrently_from_16_threads(gpu, oracle):
    """Context-less calls from 16 threads, levels 1, 2, 3 interleaved: one device queue, every frame its own level's."""
    _need157(oracle)
    chunks = [synth.gen_chunk("K" if i % 2 else "B", 55, 0, i, s) for i, s in enumerate([CHUNK, 1500000, 200000, 70000])]
    flags = nat.COMPRESS | nat.ENCRYPT | nat.CRC
    exp = {lv: [lc.expected(oracle, flags, lv, i, c) for i, c in enumerate(chunks)] for lv in (1, 2, 3)}
    errors = []

    def worker(t):
        lv = 1 + t % 3
        try:
            for _ in range(3):
                outs, d = lc.run_transform(gpu, flags, chunks, lv)
                assert (d["status"] == 0).all() and outs == exp[lv], (t, lv)
        except Exception as e:                                          # noqa: BLE001 (reported below)
            errors.append(repr(e))
    th = [threading.Thread(target=worker, args=(t,)) for t in range(16)]
    [x.start() for x in th]
    [x.join() for x in th]
    assert not errors, errors


@pytest.mark.timeout(600)
def test_level_1_next_to_a_fetch_while_guest_waves_run_it(gpu, oracle):
    """Uploads at level 1 fill the chip (guest waves on the reserved CUs too); fetches arrive and the guests hand their level-1 chunks back.
    Every frame of every batch is still libzstd's level-1 frame, and every fetch returns its chunk."""
    _need157(oracle)
    import torch
    dev = torch.device("cuda", 0)
    flags = nat.COMPRESS | nat.ENCRYPT | nat.CRC
    n, T = 512, 4
    base = [synth.gen_chunk("K", 88, 0, i, CHUNK) for i in range(8)]
    exp = [lc.expected(oracle, flags, 1, i, base[i % 8]) for i in range(8)]
    src = torch.from_numpy(np.concatenate([base[i % 8] for i in range(n)])).to(dev)
    slot = (gpu.transformed_bound(CHUNK, flags) + 63) // 64 * 64
    d = np.zeros(n, nat.DESC_DTYPE); d["src_off"] = np.arange(n, dtype=np.uint64) * CHUNK; d["src_len"] = CHUNK
    d["dst_off"] = np.arange(n, dtype=np.uint64) * slot; d["dst_cap"] = slot
    for i in range(n):
        d["iv"][i] = np.frombuffer(synth.iv_for(0, i % 8), np.uint8)
    p = nat.Native.make_params(flags, synth.KEY, synth.AAD, zstd_level=1)
    ctxs = [gpu.ctx_create(0, n, CHUNK) for _ in range(T)]
    dsts = [torch.empty(n * slot, dtype=torch.uint8, device=dev) for _ in range(T)]
    ds = [d.copy() for _ in range(T)]
    fr = np.frombuffer(exp[0], np.uint8).copy(); back = np.zeros(CHUNK, np.uint8)
    fctx = gpu.ctx_create(0, 4, CHUNK)

    def fetch():
        e = np.zeros(1, nat.DESC_DTYPE); e["src_len"] = fr.size; e["dst_cap"] = CHUNK
        gpu.detransform_batch(p, e, fr, back, back.size, nat.MEM_HOST, ctx=fctx)
        assert e["status"][0] == 0 and back.tobytes() == base[0].tobytes()

    fetch()
    old_quiet = gpu.debug_config("fetch_quiet_ms", 400)
    time.sleep(0.7)
    sv0 = gpu.service_stats(0)
    stop = [False]
    errors, rounds = [], [0] * T

    def loader(t):
        try:
            while not stop[0]:
                gpu.transform_batch(p, ds[t], src.data_ptr(), dsts[t].data_ptr(), dsts[t].numel(), nat.MEM_DEVICE, ctx=ctxs[t])
                h = dsts[t].cpu().numpy()
                for i in range(0, n, 37):
                    assert ds[t]["status"][i] == 0 and h[i * slot:i * slot + int(ds[t]["dst_len"][i])].tobytes() == exp[i % 8], (t, i)
                rounds[t] += 1
        except Exception as e:                                          # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=loader, args=(t,)) for t in range(T)]
    [x.start() for x in th]
    try:
        time.sleep(1.5)
        t_end = time.perf_counter() + 5.0
        while time.perf_counter() < t_end:
            fetch()
            time.sleep(0.05)
    finally:
        stop[0] = True
        [x.join() for x in th]
        gpu.debug_config("fetch_quiet_ms", old_quiet)
    sv1 = gpu.service_stats(0)
    assert not errors, errors
    assert min(rounds) >= 1, rounds
    print("level 1 under fetches: %d rounds, %d chunks handed back" % (sum(rounds), sv1["returned_chunks"] - sv0["returned_chunks"]))


# ---- differential fuzz ---------------------------------------------------------------------------------------------------
FUZZ_SEED = {1: 20261101, 2: 20261102}
FUZZ_KINDS = (("small", 256), ("straddle", 96), ("big", 32), ("collision", 32), ("accel", 32))
TAIL_DELTAS = (-16, -9, -8, -7, -3, -1, 0, 1, 2, 3, 6, 7, 8, 9, 10, 16)       # the last block: 1 .. 7 bytes (raw), 8 and a few more, or none


@functools.lru_cache(maxsize=2)
def _fuzz_cases(level):
    """[(kind, input)] for `level` - built once, shared (unchanged) by the tests below."""
    rng = np.random.default_rng(FUZZ_SEED[level])
    cases = [(kind, fc.level_case(rng, level, kind)) for kind, n in FUZZ_KINDS for _ in range(n)]
    W = fc.LEVEL_WINDOW[level]
    cases += [("tail", fc.gen_case(rng, W + fc.BLOCK * (1 + i % 2) + dlt)) for i, dlt in enumerate(TAIL_DELTAS)]
    return cases


@functools.lru_cache(maxsize=2)
def _fuzz_frames(level):
    """libzstd's frames of _fuzz_cases(level)."""
    from oracle import oracle as o
    return [o.zstd_compress_chunk(x.tobytes(), level) for _, x in _fuzz_cases(level)]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("level", [1, 2])
def test_differential_fuzz_vs_libzstd_at_levels_1_and_2(gpu, oracle, level):
    """Per level 256 structured inputs of 0 - 420 KB (both band edges among them), 96 whose far match straddles the low edge of the window
    (512 KiB / 1 MiB), 32 structured ones longer than the window, 32 collision-rich, 32 with accelerated steps and 16 that end within 16
    bytes of a block boundary: every frame is libzstd 1.5.7's at that level and the device decoder restores the input; the first 64 also
    go through the full chain in the three memory kinds."""
    _need157(oracle)
    cases, frames = _fuzz_cases(level), _fuzz_frames(level)
    assert len(cases) == 464
    for lo in range(0, len(cases), 128):
        part = [x for _, x in cases[lo:lo + 128]]
        outs, d = lc.run_transform(gpu, nat.COMPRESS, part, level, mem="device")
        back, d2 = pc.run_detransform(gpu, nat.COMPRESS, outs, [int(x.size) for x in part])
        for i, x in enumerate(part):
            what = "level %d seed %d case %d (%s, %d bytes)" % (level, FUZZ_SEED[level], lo + i, cases[lo + i][0], x.size)
            assert d["status"][i] == 0, what
            assert outs[i] == frames[lo + i], what + ": frame differs from libzstd"
            assert d2["status"][i] == 0 and back[i] == x.tobytes(), what + ": the device decoder does not restore the input"
    flags = nat.COMPRESS | nat.ENCRYPT | nat.CRC
    first = [x for _, x in cases[:64]]
    for mem in (None, "device", "packed"):
        lc.check_vs_oracle(gpu, oracle, flags, first, level, mem=mem)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("level", [1, 2])
def test_profile_1_5_6_at_levels_1_and_2_on_the_device(gpu, oracle, level):
    """48 of the fuzz inputs (every kind) through ZSTD_PROFILE_1_5_6, the same parse without 1.5.7's pre-splitter: libzstd decodes every
    frame back to the input, and where the pre-splitter cut nothing (every block of libzstd 1.5.7's frame but the last regenerates 128 KiB)
    the frame is libzstd 1.5.7's, byte for byte.  Inputs of both sorts occur."""
    _need157(oracle)
    cases, frames = _fuzz_cases(level), _fuzz_frames(level)
    pick = list(range(0, 256, 16)) + list(range(256, 352, 8)) + list(range(352, 448, 6)) + list(range(448, 464, 4))
    assert len(pick) == 48
    chunks = [cases[i][1] for i in pick]
    outs, d = lc.run_transform(gpu, nat.COMPRESS, chunks, level, mem="device", profile=nat.ZSTD_PROFILE_1_5_6)
    uncut = cut = 0
    for k, i in enumerate(pick):
        what = "level %d seed %d case %d (%s, %d bytes)" % (level, FUZZ_SEED[level], i, cases[i][0], chunks[k].size)
        raw = chunks[k].tobytes()
        assert d["status"][k] == 0, what
        assert oracle.zstd_decompress_chunk(outs[k], len(raw)) == raw, what + ": libzstd does not decode the 1.5.6 frame to the input"
        sizes = zi.block_sizes(frames[i])
        if all(s == fc.BLOCK for s in sizes[:-1]):
            uncut += 1
            assert outs[k] == frames[i], what + ": nothing for the pre-splitter to cut, yet the 1.5.6 frame is not libzstd 1.5.7's"
        else:
            cut += 1
    print("level %d, profile 1.5.6: %d inputs pinned to libzstd 1.5.7's bytes, %d where its pre-splitter cuts" % (level, uncut, cut))
    assert uncut >= 1 and cut >= 1, (uncut, cut)
