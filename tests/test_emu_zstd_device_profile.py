"""TSX_ZSTD_PROFILE_DEVICE under the CPU emulator: standard frames from the lane-parallel parse (csrc/zstd_enc_devparse.h).  The frames are
no library's bytes, so every chunk is judged by tests/device_profile_cases.py's "passes" - libzstd, the inspector and both device decoder
forms restore it, offsets and blocks keep the format's limits - and by the digests of tests/golden/device_profile_frames.json, which the
device has to reproduce (tests/test_zzzzzzzzzzzzzz_gpu_device_profile.py).  The emulator runs a wave's lanes as fibers, one after the
other between two rendezvous: a frame that depends on lane order shows up as a digest the device does not share."""
import ctypes
import functools
import threading
import time

import numpy as np
import pytest

import tsxform
from tests import device_profile_cases as dc
from tests import level_cases as lc
from tests import parity_cases as pc
from tests import zstd_inspect as zi
from tsxform import synth

nat = tsxform._native
FULL = nat.COMPRESS | nat.ENCRYPT | nat.CRC
MiB = 1 << 20
# a dozen cases for the chains: one and several blocks, a raw block, an RLE-like one, the smallest sizes
SOME = ["K_0", "K_1", "B_7", "K_8", "twin_65", "period3_2049", "K_131071", "B_131073", "zeros_131079", "R_131072", "twin_262145", "K_262145"]


@functools.lru_cache(maxsize=1)
def _cases():
    names = dc.names()
    return names, [dc.case(n) for n in names]


@functools.lru_cache(maxsize=1)
def _batch(emu):
    names, chunks = _cases()
    return dc.run(emu, nat.COMPRESS, chunks)


def _some():
    return [dc.case(n) for n in SOME]


# ---- every size, every content --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", dc.KINDS + ["far"])
def test_every_chunk_passes(emu, oracle, kind):
    names, chunks = _cases()
    frames, d = _batch(emu)
    pick = [i for i, n in enumerate(names) if n.rsplit("_", 1)[0] == kind]
    assert len(pick) == (1 if kind == "far" else len(dc.SIZES))
    dc.check_pass(emu, oracle, [chunks[i] for i in pick], [frames[i] for i in pick], d[pick], [names[i] for i in pick])


def test_repeats_beyond_the_window_are_not_used(emu, oracle):
    """2.5 MiB with period 2 MiB + 3: the only repeats lie 3 bytes beyond the 2 MiB window.  Nothing else in the chunk matches, so every
    block comes out raw - and a parse that took them would have failed the offset check of test_every_chunk_passes."""
    names, chunks = _cases()
    frames, d = _batch(emu)
    i = names.index(dc.FAR)
    hdr, blocks, _ = zi.parse_frame(frames[i], decode="sizes")
    assert not hdr["single_segment"] and hdr["window_log"] == 21
    assert [b.btype for b in blocks] == ["raw"] * len(blocks) and len(blocks) == 20


def test_frames_are_the_golden_files(emu):
    names, chunks = _cases()
    frames, d = _batch(emu)
    want = dc.golden()
    assert set(names) <= set(want) and set(want) - set(names) == set(dc.BIG)
    differ = [n for n, f in zip(names, frames) if dc.digest(f) != {k: want[n][k] for k in ("size", "sha256")}]
    assert not differ, "frames differ from tests/golden/device_profile_frames.json (tests/golden/make_device_profile_frames.py): %s" % differ[:8]


def test_a_parse_that_finds_nothing_does_not_pass(emu, oracle):
    """Every validity check holds for a parse without a single match.  So: the 1 MiB K and B frames lie nearer to libzstd 1.5.7's level-1
    frame than to the raw size, and R comes out within the bound as raw blocks."""
    if not oracle.zstd_version().startswith("1.5.7"):
        pytest.skip("libzstd 1.5.7 not available")
    names, chunks = _cases()
    frames, d = _batch(emu)
    for kind in ("K", "B"):
        i = names.index("%s_%d" % (kind, MiB + 13))
        n = int(chunks[i].size)
        level1 = len(oracle.zstd_compress_chunk(chunks[i].tobytes(), 1))
        print("%s: %d bytes -> %d (libzstd level 1: %d, cap %d)" % (kind, n, len(frames[i]), level1, (level1 + n) // 2))
        assert 2 * len(frames[i]) <= level1 + n, (kind, len(frames[i]), level1, n)
    i = names.index("R_%d" % (MiB + 13))
    assert len(frames[i]) <= oracle.zstd_compress_bound(int(chunks[i].size))
    assert all(b.btype == "raw" for b in zi.parse_frame(frames[i], decode="sizes")[1])


# ---- chains, memory kinds ---------------------------------------------------------------------------------------------------
def _frames_of(oracle, outs, flags):
    return [oracle.gcm_decrypt_chunk(synth.KEY, synth.AAD, o_) if flags & nat.ENCRYPT else o_ for o_ in outs]


def test_full_chain_carries_the_same_frames(emu, oracle):
    """ENCRYPT | CRC around the compressor: the oracle's GCM opens every chunk, and what it finds is the frame of the COMPRESS-only batch."""
    names, _ = _cases()
    plain, _ = _batch(emu)
    chunks = _some()
    outs, d = dc.run(emu, FULL, chunks)
    assert (d["status"] == 0).all()
    for i, (n, c) in enumerate(zip(SOME, chunks)):
        assert int(d["crc32c"][i]) == oracle.crc32c(c.tobytes()), n
        assert oracle.gcm_decrypt_chunk(synth.KEY, synth.AAD, outs[i]) == plain[names.index(n)], n
    lc.check_roundtrip(emu, FULL, chunks, outs)


@pytest.mark.parametrize("flags", [nat.COMPRESS | nat.ZSTD_CHECKSUM, FULL | nat.ZSTD_CHECKSUM])
def test_content_checksum_on_request(emu, oracle, flags):
    names, _ = _cases()
    plain, _ = _batch(emu)
    chunks = _some()
    outs, d = dc.run(emu, flags, chunks)
    frames = _frames_of(oracle, outs, flags)
    for i, (n, c) in enumerate(zip(SOME, chunks)):
        assert d["status"][i] == 0, n
        assert zi.parse_frame(frames[i], decode=False)[0]["checksum"], n
        assert len(frames[i]) == len(plain[names.index(n)]) + 4, n
        dc.check_frame(oracle, frames[i], c, n)                         # (libzstd verifies the checksum it finds)
    dc.check_decoders(emu, chunks, outs, flags & ~nat.ZSTD_CHECKSUM)


@pytest.mark.parametrize("flags", [nat.COMPRESS | nat.VERIFY, FULL | nat.ZSTD_CHECKSUM | nat.VERIFY | nat.VERIFY_GCM])
def test_verify_on_upload_accepts_every_chunk(emu, oracle, flags):
    chunks = _some()
    outs, d = dc.run(emu, flags, chunks)
    assert (d["status"] == 0).all(), d["status"]
    frames = _frames_of(oracle, outs, flags)
    for n, c, f in zip(SOME, chunks, frames):
        assert oracle.zstd_decompress_chunk(f) == c.tobytes(), n


@pytest.mark.parametrize("mem", [None, "device", "packed"])
def test_memory_kinds(emu, oracle, mem):
    names, _ = _cases()
    plain, _ = _batch(emu)
    chunks = _some()
    for flags in (nat.COMPRESS, FULL):
        outs, d = dc.run(emu, flags, chunks, mem=mem)
        assert (d["status"] == 0).all(), (mem, flags)
        assert _frames_of(oracle, outs, flags) == [plain[names.index(n)] for n in SOME], (mem, flags)
        lc.check_roundtrip(emu, flags, chunks, outs)


def test_explicit_context(emu, oracle):
    names, _ = _cases()
    plain, _ = _batch(emu)
    chunks = _some()
    ctx = emu.ctx_create()
    try:
        outs, d = dc.run(emu, nat.COMPRESS, chunks, ctx=ctx)
    finally:
        emu.ctx_destroy(ctx)
    assert (d["status"] == 0).all() and outs == [plain[names.index(n)] for n in SOME]


# ---- determinism ---------------------------------------------------------------------------------------------------------------
def test_the_same_batch_twice_and_a_chunk_alone_or_among_sixteen(emu):
    names, _ = _cases()
    plain, _ = _batch(emu)
    chunks = _some()
    want = [plain[names.index(n)] for n in SOME]
    a, da = dc.run(emu, nat.COMPRESS, chunks)
    b, db = dc.run(emu, nat.COMPRESS, chunks)
    assert a == b == want and (da["status"] == 0).all() and (db["status"] == 0).all()
    x = dc.case("K_262145")
    alone, _ = dc.run(emu, nat.COMPRESS, [x])
    sixteen = [dc.case("B_131079") if i % 2 else dc.case("twin_262145") for i in range(16)]
    sixteen[11] = x
    among, d = dc.run(emu, nat.COMPRESS, sixteen)
    assert (d["status"] == 0).all()
    assert alone[0] == among[11] == plain[names.index("K_262145")]
    assert among[1] == among[3] and among[0] == among[2]


def test_a_chunk_handed_back_and_started_again_gives_the_same_frame(emu, oracle):
    """A guest wave hands a chunk back between two blocks; whoever takes it starts from its first byte in the chunk's workspace, whose
    tables the wave before left half filled (and, before that, an exact level-3 parse had sized and tagged for itself)."""
    for f, t in (("hipemu_cu_key_shift", [ctypes.c_int]), ("hipemu_force_yield_after", [ctypes.c_int]), ("hipemu_relocate_after", [ctypes.c_int])):
        getattr(emu.lib, f).argtypes = t; getattr(emu.lib, f).restype = None
    names, _ = _cases()
    plain, _ = _batch(emu)
    pick = ["K_262145", "B_131079", "twin_262145", "K_8"]
    chunks = [dc.case(n) for n in pick]
    with emu.configured(fetch_quiet_ms=1):
        time.sleep(0.01)
        ref, d1 = dc.run(emu, FULL, chunks)
        assert [oracle.gcm_decrypt_chunk(synth.KEY, synth.AAD, o_) for o_ in ref] == [plain[names.index(n)] for n in pick]
        emu.service_quiesce(0)
        s0 = emu.service_stats(0)
        emu.lib.hipemu_cu_key_shift(3)
        try:
            for after in (4, 3):
                time.sleep(0.01)
                lc.run_transform(emu, FULL, chunks, 3)                  # the workspaces: level 3's tables last
                emu.lib.hipemu_force_yield_after(after)
                got, d = dc.run(emu, FULL, chunks)
                assert got == ref and (d["status"] == 0).all() and (d["crc32c"] == d1["crc32c"]).all(), after
        finally:
            emu.lib.hipemu_cu_key_shift(0); emu.lib.hipemu_force_yield_after(0)
        emu.service_quiesce(0)
        s1 = emu.service_stats(0)
        emu.lib.hipemu_cu_key_shift(1)
        try:
            emu.lib.hipemu_relocate_after(4)
            got, d = dc.run(emu, FULL, chunks)
            assert got == ref and (d["status"] == 0).all()
        finally:
            emu.lib.hipemu_relocate_after(0); emu.lib.hipemu_cu_key_shift(0)
    assert s1["returned_chunks"] - s0["returned_chunks"] >= 2, (s0, s1)


# ---- one service for every profile and level ---------------------------------------------------------------------------------
def test_profile_next_to_exact_levels_3_and_1(emu, oracle):
    if not oracle.zstd_version().startswith("1.5.7"):
        pytest.skip("libzstd 1.5.7 not available")
    chunks = [synth.gen_chunk("K" if i % 2 else "B", 43, 0, i, 20000 + 9000 * i) for i in range(3)]
    exact = {lv: [oracle.zstd_compress_chunk(c.tobytes(), lv) for c in chunks] for lv in (1, 3)}
    mine, d0 = dc.run(emu, nat.COMPRESS, chunks)
    assert (d0["status"] == 0).all()
    errors = []

    def worker(what):
        try:
            if what == "device":
                outs, d = dc.run(emu, nat.COMPRESS, chunks)
                assert (d["status"] == 0).all() and outs == mine, what
            else:
                outs, d = lc.run_transform(emu, nat.COMPRESS, chunks, what)
                assert (d["status"] == 0).all() and outs == exact[what], what
        except Exception as e:                                          # noqa: BLE001 (reported below)
            errors.append((what, repr(e)))
    ts = [threading.Thread(target=worker, args=(w,)) for w in ("device", 3, 1, "device", 3, 1)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for c, f in zip(chunks, mine):
        assert oracle.zstd_decompress_chunk(f) == c.tobytes()
    assert mine != exact[3] and mine != exact[1]


# ---- front end ------------------------------------------------------------------------------------------------------------------
def _status(emu, flags, level, profile, n=1000):
    x = synth.gen_chunk("K", 3, 0, 0, n)
    soff, doff, caps, st, dt = pc.layout([n], flags, emu)
    src = np.zeros(st, np.uint8); src[:n] = x
    dst = np.zeros(dt, np.uint8)
    d = pc.make_descs([n], soff, doff, caps)
    p = nat.Native.make_params(flags, synth.KEY, synth.AAD, zstd_level=level, zstd_profile=profile)
    return emu.lib.tsx_transform_batch(None, nat.C.byref(p), d.ctypes.data, 1, src.ctypes.data, src.size, dst.ctypes.data, dst.size, nat.MEM_HOST)


def test_levels_and_unknown_profiles_are_refused(emu):
    for flags in (nat.COMPRESS, FULL):
        assert _status(emu, flags, 0, dc.DEVICE) == 0
        for level in (1, 2, 3, -1):
            assert _status(emu, flags, level, dc.DEVICE) == nat.E_UNSUPPORTED, level
        assert _status(emu, flags, 0, 3) == nat.E_UNSUPPORTED
        assert _status(emu, flags, 3, nat.ZSTD_PROFILE_1_5_7) == 0
    assert _status(emu, nat.ENCRYPT | nat.CRC, 2, dc.DEVICE) == 0      # (level and profile only matter when the batch compresses)


def test_detransform_ignores_the_profile(emu):
    """One parameter block serves both directions: a fetch with the profile set (and, as before, with a level) succeeds."""
    chunks = _some()
    outs, d = dc.run(emu, FULL, chunks)
    sizes = [len(b) for b in outs]
    soff, st = [], 0
    for s in sizes:
        soff.append(st); st += (s + 15) // 16 * 16 + 16
    doff, dt = [], 0
    for c in chunks:
        doff.append(dt); dt += (int(c.size) + 15) // 16 * 16 + 16
    src = np.zeros(max(st, 16), np.uint8)
    for b, o_ in zip(outs, soff):
        src[o_:o_ + len(b)] = np.frombuffer(b, np.uint8)
    dst = np.zeros(max(dt, 16), np.uint8)
    d2 = pc.make_descs(sizes, soff, doff, [int(c.size) for c in chunks])
    p = nat.Native.make_params(FULL, synth.KEY, synth.AAD, zstd_level=0, zstd_profile=dc.DEVICE)
    emu.detransform_batch(p, d2, src, dst, dst.size)
    for i, c in enumerate(chunks):
        assert d2["status"][i] == 0 and dst[doff[i]:doff[i] + int(d2["dst_len"][i])].tobytes() == c.tobytes(), SOME[i]
