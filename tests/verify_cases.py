"""Verify on upload (TSX_VERIFY): helpers shared by the emulated and the device tests.  `N` is a tsxform._native.Native (emulated or
real); `o` is the oracle module.  Positions inside sequences come from the oracle's restatement of the level-3 parser
(oracle.zstd_l3_sequences), positions inside frames from tests/zstd_inspect.py."""
import ctypes as C

import numpy as np

import tsxform
from tests import checksum_cases as cc
from tests import zstd_inspect as zi
from tsxform import synth

nat = tsxform._native
VERIFY = getattr(nat, "VERIFY", 0x20)
E_VERIFY = getattr(nat, "E_VERIFY", -10)
VF = nat.COMPRESS | VERIFY
SIZES = [0, 1, 7, 8, 9, 255, 256, 65791, 131071, 131072, 131073, 262149, 300000]


def counts(N, ctx):
    """(chunks the block form judged, chunks decoded in full) of ctx's last verifying batch (test hook tsx_debug_verify_counts)."""
    f = N.lib.tsx_debug_verify_counts
    f.restype = C.c_int; f.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    a, b = C.c_uint32(), C.c_uint32()
    assert f(ctx, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


_CLEAN = None


def clean_chunks():
    """The clean matrix: every size as K (Kafka-like), R (incompressible: raw blocks) and zeros (RLE blocks), and B at 400000."""
    global _CLEAN
    if _CLEAN is None:
        chunks = []
        for n in SIZES:
            chunks += [synth.gen_chunk("K", 51, 0, 0, n), synth.gen_chunk("R", 51, 0, 1, n), np.zeros(n, np.uint8)]
        chunks.append(synth.gen_chunk("B", 51, 0, 2, 400000))
        _CLEAN = chunks
    return _CLEAN


def libzstd_frames(o, chunks, level, checksum):
    """libzstd 1.5.7's frames of the chunks, or None where that library is not the one the oracle has loaded."""
    if not o.zstd_version().startswith("1.5.7"):
        return None
    return [cc.frame(o, c, level, checksum=checksum) for c in chunks]


def check_clean(N, o, ctx, chunks, level, profile, checksum, mem, block_form=True):
    """The batch with and without TSX_VERIFY: every chunk TSX_OK, the same bytes (libzstd's, under profile 1.5.7 where libzstd 1.5.7
    is there to ask), and every chunk verified the expected way."""
    flags = nat.COMPRESS | (nat.ZSTD_CHECKSUM if checksum else 0)
    what = (level, profile, checksum, mem)
    want = libzstd_frames(o, chunks, level, checksum) if profile == nat.ZSTD_PROFILE_1_5_7 else None
    if want is None:                                                    # no libzstd to ask (or not its profile): the run without the flag is the reference
        want, d0, _ = cc.run_transform(N, flags, chunks, level, profile=profile, mem=mem, ctx=ctx)
        assert (d0["status"] == 0).all(), what
    outs, d, _ = cc.run_transform(N, flags | VERIFY, chunks, level, profile=profile, mem=mem, ctx=ctx)
    assert (d["status"] == 0).all(), (what, list(d["status"]))
    assert outs == want and [int(x) for x in d["dst_len"]] == [len(w) for w in want], what
    assert counts(N, ctx) == ((len(chunks), 0) if block_form else (0, len(chunks))), (what, counts(N, ctx))
    t = N.ctx_timing(ctx)
    assert t.unzstd_launches > 0
    return outs


def sequence_positions(o, data):
    """Positions of `data` by the role they play in its level-3 frame: {"match": one byte inside a match, "literal": one inside a
    literal run in front of a match, "run_first" / "run_last": the first and last byte of the chunk's last literal run - the literals
    behind its last block's last sequence where there are any ("tail": True), else the last sequence's that has some}."""
    pos, res = 0, {}
    for seqs, lit, bsize in o.zstd_l3_sequences(np.ascontiguousarray(data).tobytes(), 1):
        end = pos + lit + sum(ml for _, ml, _ in seqs)
        for ll, ml, _ in seqs:
            if ll >= 3:
                res["literal"] = pos + ll // 2
            if ll:
                res["run_first"], res["run_last"], res["tail"] = pos, pos + ll - 1, False
            if ml >= 3:
                res["match"] = pos + ll + ml // 2
            pos += ll + ml
        if end > pos:
            res["run_first"], res["run_last"], res["tail"] = pos, end - 1, True
        pos = end
    assert pos == data.size and set(res) == {"match", "literal", "run_first", "run_last", "tail"}, res
    return res


def damage_targets():
    """(K chunk of 300000 bytes, zeros chunk of 140000 bytes): chunks 0 and 2 of the damage batches."""
    return synth.gen_chunk("K", 52, 0, 0, 300000), np.zeros(140000, np.uint8)


def damage_batch():
    """Chunk 1: Kafka-like bytes that end in 24 incompressible ones - literals behind the block's last sequence, which the 300000-byte
    chunk's blocks happen not to have (they end in matches).  Chunk 3: one raw block."""
    K, Z = damage_targets()
    tail = np.concatenate([synth.gen_chunk("K", 52, 0, 1, 3000), synth.gen_chunk("R", 52, 0, 3, 24)])
    return [K, tail, Z, synth.gen_chunk("R", 52, 0, 2, 5000)]


def source_positions(o, full=True):
    """[(chunk of damage_batch(), offset)]: the first two bytes, the last, the three around the first block boundary, the first and
    last byte of the last literal run, a byte inside a match and one inside a literal run, seeded random positions; the same edges of
    the zeros chunk (RLE blocks); both ends of the literals behind the small chunk's last sequence, and a byte of the raw block."""
    batch = damage_batch()
    K, Z = batch[0], batch[2]
    sp, st = sequence_positions(o, K), sequence_positions(o, batch[1])
    assert st["tail"] and st["run_last"] == batch[1].size - 1
    at = [0, 1, K.size - 1, 131071, 131072, 131073, sp["run_first"], sp["run_last"], sp["match"], sp["literal"]]
    if full:
        rng = np.random.RandomState(20261018)
        at += [int(x) for x in rng.randint(0, K.size, 12)]
    res = [(0, p) for p in at]
    zat = [0, 1, Z.size - 1, 131071, 131072, 131073] if full else [0, Z.size - 1, 131072]
    return res + [(2, p) for p in zat] + [(1, st["run_first"]), (1, st["run_last"]), (3, 2500)]


def split_targets(targets):
    """-> [(chunks, targets renumbered)]: the positions of the 300000-byte chunk in a batch with one bystander, the others in a batch
    without that chunk (the emulated compressor needs seconds for it, every run)."""
    batch = damage_batch()
    return [([batch[0], batch[3]], [(0, p) for j, p in targets if j == 0]), (batch[1:], [(j - 1, p) for j, p in targets if j != 0])]


def check_source_damage(N, ctx, flags, targets, level=3, fallback=False, chunks=None):
    """Every (chunk, offset) of `targets`: that chunk alone is TSX_E_VERIFY with dst_len 0, the others are TSX_OK with the bytes of the
    undamaged run."""
    chunks = damage_batch() if chunks is None else chunks
    base, d0, _ = cc.run_transform(N, flags, chunks, level, ctx=ctx)
    assert (d0["status"] == 0).all()
    for j, off in targets:
        with N.configured(verify_damage_src_chunk=j, verify_damage_src_off=off, verify_force_fallback=1 if fallback else 0):
            outs, d, _ = cc.run_transform(N, flags, chunks, level, ctx=ctx)
        want = [E_VERIFY if i == j else 0 for i in range(len(chunks))]
        assert list(d["status"]) == want, (j, off, list(d["status"]))
        assert d["dst_len"][j] == 0 and counts(N, ctx) == ((0, len(chunks)) if fallback else (len(chunks), 0)), (j, off)
        for i in range(len(chunks)):
            if i != j:
                assert outs[i] == base[i], (j, off, i)
    # the source is as it was afterwards (device copy and all): the next clean run passes
    outs, d, _ = cc.run_transform(N, flags, chunks, level, ctx=ctx)
    assert (d["status"] == 0).all() and outs == base


def frame_damage_cases(N, ctx, level=3):
    """-> (chunks, [(name, flags, chunk, offset in its frame)]).  Positions are read off the frames the library itself writes (they are
    libzstd's: check_clean): a byte of a raw block, a byte of a raw literals section, the bytes of a block header, and each of the four
    checksum bytes of an otherwise intact frame."""
    rawblk = synth.gen_chunk("R", 33, 0, 1, 1000)                       # incompressible: one raw block
    rawlit = cc.rawlit_input(6000)                                      # a compressed block whose literals are raw
    K = synth.gen_chunk("K", 52, 0, 3, 150000)
    chunks = [rawblk, rawlit, K]
    plain, d, _ = cc.run_transform(N, nat.COMPRESS, chunks, level, ctx=ctx)
    ck, d2, _ = cc.run_transform(N, cc.CK, chunks, level, ctx=ctx)
    assert (d["status"] == 0).all() and (d2["status"] == 0).all()
    cases = []
    for flags, frames in ((VF, plain), (VF | nat.ZSTD_CHECKSUM, ck)):
        secs = cc.raw_sections(frames[0])[0]
        assert secs, "the incompressible input no longer gives a raw block"
        cases.append(("raw block byte", flags, 0, secs[0][0] + min(20, secs[0][1] - 1)))
        secs = cc.raw_sections(frames[1])[1]
        assert secs, "the repeated input no longer gives raw literals"
        cases.append(("raw literals byte", flags, 1, secs[0][0] + min(20, secs[0][1] - 1)))
        hs = zi.parse_frame(frames[2], decode=False)[0]["header_size"]
        for k in range(3):
            cases.append(("block header byte %d" % k, flags, 2, hs + k))
    for i, f in enumerate(ck):
        for k in range(4):
            cases.append(("checksum byte %d" % k, VF | nat.ZSTD_CHECKSUM, i, len(f) - 4 + k))
    return chunks, cases


def check_frame_damage(N, ctx, level=3, pick=None):
    chunks, cases = frame_damage_cases(N, ctx, level)
    base = {}
    for name, flags, j, off in cases if pick is None else [cases[i] for i in pick]:
        if flags not in base:
            base[flags] = cc.run_transform(N, flags, chunks, level, ctx=ctx)[0]
        with N.configured(verify_damage_frame_chunk=j, verify_damage_frame_off=off):
            outs, d, _ = cc.run_transform(N, flags, chunks, level, ctx=ctx)
        assert list(d["status"]) == [E_VERIFY if i == j else 0 for i in range(len(chunks))], (name, j, off, list(d["status"]))
        assert d["dst_len"][j] == 0, name
        for i in range(len(chunks)):
            if i != j:
                assert outs[i] == base[flags][i], (name, i)
    return len(cases)
