"""Zstandard levels 1 and 2 on the device: full-size chunks byte for byte libzstd 1.5.7's at the same level, the full chain against the
oracle, a 256-chunk B segment at level 1, levels side by side from 16 threads, and level 1 next to a fetch that makes guest waves hand
their chunks back.  (The logic, with small inputs, runs on the CPU emulator: tests/test_emu_zstd_levels.py.)"""
import functools
import threading
import time

import numpy as np
import pytest

import tsxform
from tests import level_cases as lc
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
