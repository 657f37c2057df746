"""Zstandard levels 1 and 2 (strategy fast, and dfast for level 2 in (128 KiB, 256 KiB]) under the CPU emulator: the parameters are
libzstd's own, the frames are the real libzstd 1.5.7's bytes at the same level, levels share the compressor service and its workspaces,
and the front end refuses every other level.  Full-size chunks run on the device (tests/test_zzzzzz_gpu_zstd_levels.py)."""
import ctypes
import os
import subprocess
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
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tiered-storage-for-apache-kafka_amd", "csrc")
KiB = 1024


def _need157(oracle):
    if not oracle.zstd_version().startswith("1.5.7"):
        pytest.skip("libzstd 1.5.7 not available")


# ---- parameters ----------------------------------------------------------------------------------------------------
_PROBE = r"""
#include <hip/hip_runtime.h>
#include "zstd_common.h"
extern "C" void probe(int level, unsigned long long n, unsigned* out) {
    const zs_level_params c = zs_level_cparams(level, n);
    out[0] = c.windowLog; out[1] = c.chainLog; out[2] = c.hashLog; out[3] = c.searchLog; out[4] = c.minMatch; out[5] = c.targetLength; out[6] = c.strategy;
}
"""

SIZES = [0, 1, 7, 1000, 16384, 16385, 131072, 131073, 262144, 262145, 4 << 20, 64 << 20]


def test_cparams_equal_the_librarys_getCParams(oracle, tmp_path):
    """zs_level_cparams (csrc/zstd_common.h, host + device) against ZSTD_getCParams(level, srcSize, 0) of the parity library itself."""
    _need157(oracle)
    src = tmp_path / "probe.cpp"; src.write_text(_PROBE)
    so = tmp_path / "probe.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "tests", "emu"), "-I", CSRC, str(src), "-o", str(so)])
    P = ctypes.CDLL(str(so))
    P.probe.argtypes = [ctypes.c_int, ctypes.c_ulonglong, ctypes.POINTER(ctypes.c_uint * 7)]
    Z = ctypes.CDLL(oracle.lib().orc_zstd_path().decode())

    class CP(ctypes.Structure):
        _fields_ = [(n, ctypes.c_uint) for n in ("windowLog", "chainLog", "hashLog", "searchLog", "minMatch", "targetLength")] + [("strategy", ctypes.c_int)]
    Z.ZSTD_getCParams.restype = CP
    Z.ZSTD_getCParams.argtypes = [ctypes.c_int, ctypes.c_ulonglong, ctypes.c_size_t]
    for level in (1, 2, 3):
        for n in SIZES:
            want = Z.ZSTD_getCParams(level, n, 0)
            got = (ctypes.c_uint * 7)()
            P.probe(level, n, ctypes.byref(got))
            assert list(got) == [getattr(want, f) for f, _ in CP._fields_], (level, n, list(got))
    # level 2 in (128 KiB, 256 KiB] is dfast (the existing double-fast parse with level 2's parameters)
    for n in (131073, 200000, 262144):
        got = (ctypes.c_uint * 7)(); P.probe(2, n, ctypes.byref(got))
        assert list(got) == [18, 14, 14, 1, 5, 0, 2]


# ---- frames ----------------------------------------------------------------------------------------------------------
def _cases():
    rng = np.random.default_rng(11)
    K = synth.gen_chunk("K", 5, 0, 0, 300000); R = synth.gen_chunk("R", 5, 0, 0, 120000)
    return {
        "golden15": np.frombuffer(bytes.fromhex("000000030000000A01000A0000001E"), np.uint8),
        "empty": K[:0], "one": K[:1], "K7": K[:7], "K8": K[:8], "K63": K[:63], "K64": K[:64], "K255": K[:255], "K256": K[:256],
        "K1000": K[:1000], "K4096": K[:4096], "K70000": K[:70000],
        "R50000": R[:50000], "zeros": np.zeros(150000, np.uint8), "period7": np.tile(np.frombuffer(b"abcdefg", np.uint8), 12000),
        "mixKR": np.concatenate([K[:60000], R[:60000], K[60000:120000], np.zeros(20000, np.uint8)]),
        "lowent": rng.integers(0, 4, 100000, dtype=np.uint8),
        "skewed": np.minimum(rng.geometric(0.3, 100000), 255).astype(np.uint8),
        "ramp": (np.arange(100000) % 256).astype(np.uint8),
        "farmatch": np.concatenate([R[:20000], K[:50000], R[:20000], K[20000:30000], R[5000:15000]]),
        "jumps": np.concatenate([R[:3000], np.zeros(40000, np.uint8), R[:3000], R[100000:120000], np.tile(R[:999], 30)]),
    }


@pytest.mark.parametrize("level", [1, 2])
def test_levels_1_and_2_are_byte_identical_to_libzstd(emu, oracle, level):
    _need157(oracle)
    cases = _cases()
    names = list(cases)
    outs, d = lc.run_transform(emu, nat.COMPRESS, [cases[n] for n in names], level)
    for i, n in enumerate(names):
        assert d["status"][i] == 0, n
        assert outs[i] == oracle.zstd_compress_chunk(cases[n].tobytes(), level), "%s: level %d frame differs from libzstd" % (n, level)


@pytest.mark.parametrize("level", [1, 2])
def test_sizes_around_the_parameter_bands(emu, oracle, level):
    """16 KiB, 128 KiB and 256 KiB change minMatch and the table sizes; level 2 in (128 KiB, 256 KiB] is dfast."""
    _need157(oracle)
    K = synth.gen_chunk("K", 7, 0, 3, 262150)
    sizes = [16383, 16384, 16385, 131071, 131072, 131073, 200000, 262143, 262144, 262145]
    chunks = [K[:s] for s in sizes]
    outs, d = lc.run_transform(emu, nat.COMPRESS, chunks, level)
    for i, s in enumerate(sizes):
        assert d["status"][i] == 0 and outs[i] == oracle.zstd_compress_chunk(chunks[i].tobytes(), level), (level, s)


def test_fast_pre_splitter_cuts_where_libzstd_does(emu, oracle):
    """libzstd 1.5.7 gives strategy fast its own pre-block splitter (ZSTD_splitBlock_fromBorders: the first, last and middle 512 bytes of a
    128 KiB block) - not the dfast one (split_block_1_5_7).  A B span long enough that full blocks after the first are split."""
    _need157(oracle)
    B = synth.gen_chunk("B", 5, 0, 1, 4 << 20)
    spans = [B[:400000]]                                               # libzstd: 128, 96, 32, 128 KiB ... blocks at levels 1 and 2
    for level in (1, 2):
        outs, d = lc.run_transform(emu, nat.COMPRESS, spans, level)
        assert d["status"][0] == 0
        assert outs[0] == oracle.zstd_compress_chunk(spans[0].tobytes(), level), level
        cut = [b.regen for b in zi.parse_frame(outs[0], decode=True)[1]]
        assert cut[:4] == [131072, 98304, 32768, 131072], (level, cut)


@pytest.mark.parametrize("level", [1, 2])
def test_profile_1_5_6_has_no_pre_splitter(emu, oracle, level):
    """Profile 1.5.6 is the same code without 1.5.7's pre-splitter (an unverified stand-in, as at level 3): one 128 KiB block per 128 KiB of
    input, frames libzstd decodes back to the input."""
    x = synth.gen_chunk("B", 5, 0, 1, 300000)
    outs, d = lc.run_transform(emu, nat.COMPRESS, [x], level, profile=nat.ZSTD_PROFILE_1_5_6)
    assert d["status"][0] == 0
    blocks = zi.parse_frame(outs[0], decode=True)[1]
    assert [b.regen for b in blocks] == [131072, 131072, 300000 - 262144]
    assert oracle.zstd_decompress_chunk(outs[0]) == x.tobytes()


def test_differential_fuzz_levels_1_and_2(emu, oracle):
    """220 generated inputs (synthetic kinds, random, runs, repeats, at small sizes), alternating levels, against libzstd."""
    _need157(oracle)
    rng = np.random.default_rng(20261016)
    chunks = []
    for i in range(220):
        kind = i % 6
        n = int(rng.integers(0, 6000)) if i % 11 else int(rng.integers(6000, 40000))
        if kind == 0:
            x = synth.gen_chunk("K", 100 + i, 0, 0, n)
        elif kind == 1:
            x = synth.gen_chunk("B", 100 + i, 0, 0, n)
        elif kind == 2:
            x = rng.integers(0, int(rng.integers(1, 256)) + 1, n, dtype=np.uint8) if n else np.zeros(0, np.uint8)
        elif kind == 3:
            x = np.repeat(rng.integers(0, 256, max(n // 13, 1), dtype=np.uint8), 13)[:n]
        elif kind == 4:
            unit = rng.integers(0, 256, int(rng.integers(1, 300)), dtype=np.uint8)
            x = np.tile(unit, n // unit.size + 1)[:n].copy()
            if n:
                x[rng.integers(0, n, max(n // 200, 1))] ^= 0x5A
        else:
            x = synth.gen_chunk("R", 100 + i, 0, 0, n)
        chunks.append(np.ascontiguousarray(x, dtype=np.uint8))
    for level in (1, 2):
        part = chunks[level - 1::2]
        outs, d = lc.run_transform(emu, nat.COMPRESS, part, level)
        for i, x in enumerate(part):
            assert d["status"][i] == 0 and outs[i] == oracle.zstd_compress_chunk(x.tobytes(), level), (level, i, x.size)


# ---- past the window, shared buckets, acceleration (tests/fuzz_cases.py; the same generators at full count on the device) ----
def _frames_equal_libzstds_and_decode(emu, oracle, chunks, level, what):
    outs, d = lc.run_transform(emu, nat.COMPRESS, chunks, level)
    for i, x in enumerate(chunks):
        assert d["status"][i] == 0, (what, level, i, x.size)
        assert outs[i] == oracle.zstd_compress_chunk(x.tobytes(), level), "%s case %d (%d bytes): level %d frame differs from libzstd" % (what, i, x.size, level)
    lc.check_roundtrip(emu, nat.COMPRESS, chunks, outs)


@pytest.mark.parametrize("level", [1, 2])
def test_matches_that_straddle_the_windows_low_edge(emu, oracle, level):
    """16 inputs longer than the level's window (512 KiB / 1 MiB) in which a copy's partner crosses the lowest valid index of a block:
    prefixStartIndex, the candidate test against it, the backward count's limit.  First the guard, from libzstd's frames alone: at least
    half of the inputs make libzstd emit an offset within 4096 of the window size (seeds 20261018 / 20261019: 12 of 16 at either level,
    7 and 6 within 64) - else the generator has stopped reaching the edge and the comparison below proves little."""
    _need157(oracle)
    W = fc.LEVEL_WINDOW[level]
    rng = np.random.default_rng(20261017 + level)
    chunks = [fc.straddle_case(rng, W) for _ in range(16)]
    near = [fc.offsets_near_window(oracle.zstd_compress_chunk(x.tobytes(), level), W) for x in chunks]
    reached = sum(1 for n in near if n)
    print("level %d: %d of %d straddle inputs have a libzstd offset in (W - 4096, W]" % (level, reached, len(chunks)))
    assert 2 * reached >= len(chunks), near
    _frames_equal_libzstds_and_decode(emu, oracle, chunks, level, "straddle")


@pytest.mark.parametrize("level", [1, 2])
def test_structured_inputs_longer_than_the_window(emu, oracle, level):
    """gen_case beyond the window: ZSTD_window_enforceMaxDist in the chunk loop, repcodes a slide invalidates at a block's start."""
    _need157(oracle)
    rng = np.random.default_rng(20261027 + level)
    chunks = [fc.level_case(rng, level, "big") for _ in range(4)]
    assert all(x.size >= fc.LEVEL_WINDOW[level] for x in chunks)
    _frames_equal_libzstds_and_decode(emu, oracle, chunks, level, "big")


@pytest.mark.parametrize("level", [1, 2])
def test_shared_buckets_and_accelerated_steps_over_several_blocks(emu, oracle, level):
    """6 collision-rich inputs (lanes of one wave step in one bucket: the earlier lane's position is the candidate, the last lane's the
    write) and 6 with incompressible stretches that push the step to 2, 3, 4, 5 ... before a match on either position of a pair (the
    write of the following position that libzstd makes for steps up to 4), 300 - 420 KB each: three blocks and more."""
    _need157(oracle)
    rng = np.random.default_rng(20261037 + level)
    chunks = [fc.level_case(rng, level, "collision") for _ in range(6)] + [fc.level_case(rng, level, "accel") for _ in range(6)]
    assert all(x.size > 2 * fc.BLOCK for x in chunks)
    _frames_equal_libzstds_and_decode(emu, oracle, chunks, level, "collision/accel")


def test_level_2_is_dfast_between_128_and_256_KiB(emu, oracle):
    """The double-fast parser with level 2's own parameters (windowLog 18, both tables 2^14, minMatch 5): structured inputs over the band,
    its first and its last size included."""
    _need157(oracle)
    rng = np.random.default_rng(20261047)
    sizes = [131073, 262144] + [int(rng.integers(131074, 262144)) for _ in range(6)]
    chunks = [fc.gen_case(rng, s) for s in sizes]
    _frames_equal_libzstds_and_decode(emu, oracle, chunks, 2, "dfast band")


# ---- service: levels side by side, hand-back ------------------------------------------------------------------------------
def test_levels_submitted_concurrently_keep_their_own_bytes(emu, oracle):
    """Members of levels 1, 2 and 3 from several threads share the one device queue; each frame is its own level's."""
    _need157(oracle)
    chunks = [synth.gen_chunk("K" if i % 2 else "B", 41, 0, i, 20000 + 9000 * i) for i in range(3)]
    exp = {lv: [oracle.zstd_compress_chunk(c.tobytes(), lv) for c in chunks] for lv in (1, 2, 3)}
    errors = []

    def worker(lv):
        try:
            for _ in range(1):
                outs, d = lc.run_transform(emu, nat.COMPRESS, chunks, lv)
                assert (d["status"] == 0).all() and outs == exp[lv], lv
        except Exception as e:                                          # noqa: BLE001 (reported below)
            errors.append((lv, repr(e)))
    ts = [threading.Thread(target=worker, args=(lv,)) for lv in (1, 2, 3, 1, 2, 3)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert exp[1] != exp[3] and exp[2] != exp[3]


def test_level_1_chunks_handed_back_restart_on_workspaces_level_3_used(emu, oracle):
    """A guest wave hands a level-1 chunk back mid-chunk; another wave starts it again from its first byte in the chunk's workspace, which a
    level-3 chunk used just before (its tables sized and tagged for dfast): the frames stay libzstd's level-1 bytes."""
    _need157(oracle)
    for f, t in (("hipemu_cu_key_shift", [ctypes.c_int]), ("hipemu_force_yield_after", [ctypes.c_int]), ("hipemu_relocate_after", [ctypes.c_int])):
        getattr(emu.lib, f).argtypes = t; getattr(emu.lib, f).restype = None
    flags = nat.COMPRESS | nat.ENCRYPT | nat.CRC
    sizes = [200000, 131072 + 5, 30001, 17]
    chunks = [synth.gen_chunk("K" if i % 3 else "B", 31, 1, i, s) for i, s in enumerate(sizes)]
    with emu.configured(fetch_quiet_ms=1):
        time.sleep(0.01)
        ref1, d1 = lc.check_vs_oracle(emu, oracle, flags, chunks, 1)
        emu.service_quiesce(0)
        s0 = emu.service_stats(0)
        emu.lib.hipemu_cu_key_shift(3)
        try:
            for after in (4, 3):
                time.sleep(0.01)
                lc.run_transform(emu, flags, chunks, 3)                 # the workspaces: level 3's tables last
                emu.lib.hipemu_force_yield_after(after)
                got, d = lc.run_transform(emu, flags, chunks, 1)
                assert got == ref1 and (d["status"] == 0).all() and (d["crc32c"] == d1["crc32c"]).all(), after
        finally:
            emu.lib.hipemu_cu_key_shift(0); emu.lib.hipemu_force_yield_after(0)
        emu.service_quiesce(0)
        s1 = emu.service_stats(0)
        emu.lib.hipemu_cu_key_shift(1)
        try:
            emu.lib.hipemu_relocate_after(4)
            got, d = lc.run_transform(emu, flags, chunks, 1)
            assert got == ref1 and (d["status"] == 0).all()
        finally:
            emu.lib.hipemu_relocate_after(0); emu.lib.hipemu_cu_key_shift(0)
    assert s1["returned_chunks"] - s0["returned_chunks"] >= 2, (s0, s1)


# ---- front end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", [None, "packed", "device"])
def test_full_chain_at_level_1_matches_the_oracle_and_round_trips(emu, oracle, mem):
    _need157(oracle)
    chunks = [synth.gen_chunk("K", 9, 2, 0, 150000), synth.gen_chunk("B", 9, 2, 1, 65537), synth.gen_chunk("K", 9, 2, 2, 17)]
    for flags in (nat.COMPRESS | nat.ENCRYPT | nat.CRC, nat.COMPRESS | nat.CRC, nat.COMPRESS):
        outs, d = lc.check_vs_oracle(emu, oracle, flags, chunks, 1, mem=mem)
        lc.check_roundtrip(emu, flags, chunks, outs)


def test_other_levels_are_refused_and_0_is_3(emu, oracle):
    flags = nat.COMPRESS | nat.ENCRYPT | nat.CRC
    for level in (-1, 4, 19, 22):
        assert lc.transform_status(emu, flags, level) == nat.E_UNSUPPORTED, level
        assert lc.transform_status(emu, nat.COMPRESS, level) == nat.E_UNSUPPORTED, level
    for level in (0, 1, 2, 3):
        assert lc.transform_status(emu, flags, level) == 0, level
    assert lc.transform_status(emu, nat.ENCRYPT | nat.CRC, 7) == 0     # (the level only matters when the batch compresses)
    x = [synth.gen_chunk("K", 9, 3, 0, 90000)]
    a, _ = lc.run_transform(emu, flags, x, 0)
    b, _ = lc.run_transform(emu, flags, x, 3)
    assert a == b
    a, _ = lc.run_transform(emu, nat.COMPRESS, x, 0)
    assert a[0] == oracle.zstd_compress_chunk(x[0].tobytes())
