"""TSX_ZSTD_PROFILE_DEVICE under the CPU emulator, second family (tests/device_profile_cases.py): 96 seeded structured inputs, two copies
exactly D bytes apart for D either side of the 2 MiB window, inputs aimed at the frame loop between blocks of different types (a block
that is parsed and then emitted raw must leave nothing in the repeat-offset history), and a 6 MiB chunk.  Every frame is judged as in
tests/test_emu_zstd_device_profile.py - libzstd, the inspector and both device decoder forms restore it, the format's limits hold - and by
its digest in tests/golden/device_profile_fuzz_frames.json, which the device has to reproduce
(tests/test_zzzzzzzzzzzzzzz_gpu_device_profile_fuzz.py).  A census over the set says what it reaches, so it cannot go vacuous unnoticed."""
import ctypes
import functools
import time

import pytest

import tsxform
from tests import device_profile_cases as dc
from tests import level_cases as lc
from tsxform import synth

nat = tsxform._native
FULL = nat.COMPRESS | nat.ENCRYPT | nat.CRC
FAMILIES = {"fuzz": dc.FUZZ, "edge": dc.EDGE, "aimed": dc.AIMED, "big": dc.BIG_EMU}
HANDED_BACK = ["rep_over_raw", "edge_2097152_noise", "fuzz_064", "fuzz_080"]     # (the two fuzz cases: collision and accel, 300 - 420 KB)


@functools.lru_cache(maxsize=1)
def _cases():
    names = dc.fuzz_names(device_only=False)
    return names, [dc.fuzz_case(n) for n in names]


@functools.lru_cache(maxsize=1)
def _batch(emu):
    names, chunks = _cases()
    frames, d = dc.run(emu, nat.COMPRESS, chunks)
    assert (d["status"] == 0).all(), [(n, int(s)) for n, s in zip(names, d["status"]) if s]
    return frames, d


@functools.lru_cache(maxsize=1)
def _census(emu):
    return dc.census(_batch(emu)[0])


def _frame(emu, name):
    return _batch(emu)[0][_cases()[0].index(name)]


# ---- every chunk passes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_frame_keeps_the_format(emu, oracle, family):
    names, chunks = _cases()
    frames, d = _batch(emu)
    for n in FAMILIES[family]:
        i = names.index(n)
        dc.check_frame(oracle, frames[i], chunks[i], dc.label(n))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_both_decoder_forms_restore_the_chunks(emu, family):
    """Every edge, aimed and big case, and every fourth fuzz case (all kinds among them)."""
    names, chunks = _cases()
    frames, d = _batch(emu)
    pick = [names.index(n) for k, n in enumerate(FAMILIES[family]) if family != "fuzz" or k % 4 == 0]
    assert len(pick) == (24 if family == "fuzz" else len(FAMILIES[family]))
    dc.check_decoders(emu, [chunks[i] for i in pick], [frames[i] for i in pick])


def test_frames_are_the_golden_files(emu):
    names, chunks = _cases()
    frames, d = _batch(emu)
    want = dc.fuzz_golden()["frames"]
    assert set(want) - set(names) == set(dc.BIG_DEVICE) and set(names) <= set(want)
    differ = [n for n, f, c in zip(names, frames, chunks) if dict(dc.digest(f), chunk=int(c.size)) != want[n]]
    assert not differ, "frames differ from tests/golden/device_profile_fuzz_frames.json (tests/golden/make_device_profile_frames.py): %s" % differ[:8]


# ---- the window's edge ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.EDGE)
def test_window_edge(emu, name):
    """Two copies of 6000 noise bytes exactly D apart.  D <= 2 MiB: the candidate at distance D is inside the window and is taken.  D beyond:
    it is not, nothing else is like the second copy, so the second copy is literals and no offset comes near the window's size."""
    D, begin, end = dc.edge_second_copy(name)
    blocks, seqs = dc.sequences(_frame(emu, name))
    at_d = sum(1 for s in seqs if s[4] == D)
    over = [s for s in seqs if s[4] > dc.WINDOW - 4096]
    in_copy = [s for s in seqs if s[0] < end and s[0] + s[2] > begin]
    print("%s: %d sequences, %d with offset D, %d above 2^21 - 4096, %d matches in the second copy" % (name, len(seqs), at_d, len(over), len(in_copy)))
    if D <= dc.WINDOW:
        assert at_d >= 1, name
        assert all(s[4] == D for s in over), over[:4]
    else:
        assert not over, over[:4]
        assert not in_copy, in_copy[:4]


# ---- what the set reaches ------------------------------------------------------------------------------------------------------
def test_census_of_the_set(emu):
    c = _census(emu)
    print(c)
    assert c["frames"] == len(_cases()[0])
    assert c["blocks"]["raw"] >= 1 and c["blocks"]["rle"] >= 1 and c["blocks"]["compressed"] >= 1, c["blocks"]
    assert c["raw_to_compressed"] >= 1, c
    assert c["raw_or_rle_to_compressed_first_ll_gt_0"] >= 1, c
    assert c["max_lit_length"] >= 65536, c
    assert c["offsets_at_window"] >= 1, c


def test_aimed_inputs_reach_what_they_aim_at(emu):
    def types(name):
        return [b.btype for b in dc.sequences(_frame(emu, name))[0]]
    assert types("raw_then_K") == ["raw", "compressed", "compressed"]
    assert types("K_then_short_run") == ["compressed", "rle"]
    assert dc.census([_frame(emu, "ll_70000")])["max_lit_length"] >= 70000
    blocks, seqs = dc.sequences(_frame(emu, "matches_in_raw"))
    assert [b.btype for b in blocks] == ["raw", "compressed"]
    assert blocks[1].seqs[0][0] == 0, "block 1 starts with a match: %s" % (blocks[1].seqs[0],)
    assert seqs[0][4] == dc.BLOCK - 40 * dc.SLICE, seqs[0]


@pytest.mark.parametrize("name", ["rep_over_raw", "rep_over_raw_twin"])
def test_a_raw_block_leaves_nothing_in_the_repeat_history(emu, name):
    """Block 1 is parsed (one match at REP_RAW_DIST) and emitted raw: no decoder ever sees that sequence.  Block 2's first sequence copies
    from REP_RAW_DIST - it must say so - or, in the twin, from the offset of block 0's last sequence, which IS repeat offset 1."""
    blocks, seqs = dc.sequences(_frame(emu, name))
    assert [b.btype for b in blocks] == ["compressed", "raw", "compressed"]
    assert [s for s in seqs if s[5] == 0][-1][4] == dc.REP_TWIN_DIST, "block 0's last offset"
    ll, ml, ob = blocks[2].seqs[0]
    assert ll > 0 and ml >= 200, (ll, ml, ob)
    assert ob == (1 if name.endswith("twin") else dc.REP_RAW_DIST + 3), (ll, ml, ob)


# ---- handed back between two blocks ----------------------------------------------------------------------------------------------
def test_chunks_handed_back_and_started_again_give_the_same_frames(emu, oracle):
    """As test_a_chunk_handed_back_and_started_again_gives_the_same_frame: a guest wave gives its chunk back between two blocks, with the
    tables and the repeat history of the blocks it had parsed in the workspace, and whoever takes it starts from the first byte."""
    for f in ("hipemu_cu_key_shift", "hipemu_force_yield_after"):
        getattr(emu.lib, f).argtypes = [ctypes.c_int]; getattr(emu.lib, f).restype = None
    chunks = [dc.fuzz_case(n) for n in HANDED_BACK]
    want = [_frame(emu, n) for n in HANDED_BACK]
    assert all(len(dc.sequences(f)[0]) >= 3 for f in want)
    with emu.configured(fetch_quiet_ms=1):
        time.sleep(0.01)
        ref, d1 = dc.run(emu, FULL, chunks)
        assert [oracle.gcm_decrypt_chunk(synth.KEY, synth.AAD, o_) for o_ in ref] == want
        emu.service_quiesce(0)
        s0 = emu.service_stats(0)
        emu.lib.hipemu_cu_key_shift(3)
        try:
            for after in (2, 3, 4):
                time.sleep(0.01)
                lc.run_transform(emu, FULL, chunks, 3)                  # the workspaces: level 3's tables last
                emu.lib.hipemu_force_yield_after(after)
                got, d = dc.run(emu, FULL, chunks)
                assert got == ref and (d["status"] == 0).all() and (d["crc32c"] == d1["crc32c"]).all(), after
        finally:
            emu.lib.hipemu_cu_key_shift(0); emu.lib.hipemu_force_yield_after(0)
        emu.service_quiesce(0)
        s1 = emu.service_stats(0)
    assert s1["returned_chunks"] - s0["returned_chunks"] >= 2, (s0, s1)
