"""The repeat-offset history both decoder forms resolve through one function (csrc/zstd_dec_dev.h, dec_rep_offsets): cases shared by
the emulated and the device tests.  The input is one 380 KB "B" chunk compressed by the real libzstd (through the oracle) at level 3,
the common case, and at level 19, whose optimal parser uses every entry of the history: the frame is first counted with
tests/zstd_inspect.py and must itself exercise what the tests are about - every history index, users of the history at the start of
a later block (where the fold reads what the previous block left behind), groups past the first 64 sequences of a block - before
either form decodes a byte of it.  `N` is a tsxform._native.Native (emulated or real); `o` is the oracle module."""
import tsxform
from tests import checksum_cases as cc
from tests import zstd_inspect as zi
from tsxform import synth

nat = tsxform._native
LEVELS = (3, 19)
_CASE = None
_COUNTS = None


def case(o):
    """-> (the source chunk, {level: libzstd's frame of it}); built once."""
    global _CASE
    if _CASE is None:
        x = synth.gen_chunk("B", 9, 1, 3, 380000)
        _CASE = (x, {lv: o.zstd_compress_chunk(x, lv) for lv in LEVELS})
    return _CASE


def census(blob):
    """What a frame asks of the repeat-offset pass, counted on its sequences (literal length, match length, offset code):
    idx[i]     sequences that use history entry i = code - 1 (+ 1 when the literal length is 0); i = 3 is "rep0 - 1"
    at_start   users of the history among the first three sequences of a block that is not the frame's first
    low_lanes  users in lanes 0-2 of a group of 64 that is not its block's first
    symbolic3  index-3 users in front of their block's first new offset: "rep0 - 1" of an entry the block form does not know yet
    big_blocks compressed blocks with more than 64 sequences"""
    blocks = zi.parse_frame(blob, decode="sizes")[1]
    c = {"blocks": sum(b.btype == "compressed" for b in blocks), "sequences": sum(b.nbseq for b in blocks), "idx": [0, 0, 0, 0],
         "at_start": 0, "low_lanes": 0, "symbolic3": 0, "big_blocks": sum(b.nbseq > 64 for b in blocks)}
    for bi, b in enumerate(blocks):
        seen_new = False
        for i, (ll, ml, ob) in enumerate(b.seqs):
            if ob > 3:
                seen_new = True
                continue
            idx = ob - 1 + (1 if ll == 0 else 0)
            c["idx"][idx] += 1
            c["at_start"] += bi > 0 and i < 3
            c["low_lanes"] += i >= 64 and i % 64 < 3
            c["symbolic3"] += idx == 3 and not seen_new
    return c


def check_the_input_exercises_the_history(o):
    """Conditions on libzstd's frames, not on the code under test."""
    global _COUNTS
    if _COUNTS is None:
        _COUNTS = {lv: census(case(o)[1][lv]) for lv in LEVELS}
    counts = _COUNTS
    for lv in LEVELS:
        print("level %d: %s" % (lv, counts[lv]))
    print("index-3 users on a history entry still symbolic in the block form (level 19): %d" % counts[19]["symbolic3"])
    c = counts[19]
    assert min(c["idx"]) >= 10, c
    assert c["at_start"] >= 5, c
    assert c["big_blocks"] >= 3, c
    return counts


def check_both_forms_restore_the_chunk(N, o):
    x, blobs = case(o)
    frames = [blobs[lv] for lv in LEVELS]
    res = cc.decode_both_forms(N, nat.COMPRESS, frames, [int(x.size)] * len(frames))
    wrong = {}                                                          # form -> (statuses, levels whose bytes differ): both forms are reported
    for form, (outs, d, kept) in res.items():
        status, differ = [int(v) for v in d["status"]], [lv for lv, out in zip(LEVELS, outs) if out != x.tobytes()]
        if differ or status != [0] * len(frames):
            wrong[form] = (status, differ)
    assert not wrong, wrong
    assert res["block"][2] == len(frames), "a frame left the block form"
    assert list(res["block"][1]["status"]) == list(res["chunk"][1]["status"]) and res["block"][0] == res["chunk"][0]


def check_both_forms_agree_on_damage(N, o):
    """One byte flipped at a third and at half of the level-19 frame: whatever that does to it, it does the same in both forms."""
    x, blobs = case(o)
    f = blobs[19]
    damaged = [cc.flip(f, len(f) // 3), cc.flip(f, len(f) // 2)]
    res = cc.decode_both_forms(N, nat.COMPRESS, damaged, [int(x.size)] * len(damaged))
    assert list(res["block"][1]["status"]) == list(res["chunk"][1]["status"]), (list(res["block"][1]["status"]), list(res["chunk"][1]["status"]))
