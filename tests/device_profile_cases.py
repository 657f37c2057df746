"""TSX_ZSTD_PROFILE_DEVICE: the case list, and what "a chunk passes" means.  The profile's frames are standard Zstandard and no library's
bytes, so nothing here compares frames with libzstd's: a frame is judged by who can read it (real libzstd, tests/zstd_inspect.py, both
device decoder forms), by the format limits its parse must keep (offsets, block sizes, ZSTD_compressBound), and by its digest in
tests/golden/device_profile_frames.json (emulator and device agree lane for lane).  `N` is a tsxform._native.Native (emulated or real),
`o` the oracle module."""
import hashlib
import json
import os

import numpy as np

import tsxform
from tests import level_cases as lc
from tests import parity_cases as pc
from tests import zstd_inspect as zi
from tsxform import synth

nat = tsxform._native
DEVICE = nat.ZSTD_PROFILE_DEVICE
KiB, MiB = 1 << 10, 1 << 20
BLOCK = 128 * KiB
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_profile_frames.json")

SIZES = [0, 1, 7, 8, 63, 64, 65, 127, 128, 2047, 2048, 2049, BLOCK - 1, BLOCK, BLOCK + 1, BLOCK + 7, 2 * BLOCK + 1, MiB + 13]
KINDS = ["K", "B", "R", "zeros", "period3", "twin"]
FAR = "far_2560KiB"                  # 2.5 MiB with period 2 MiB + 3: every repeat lies beyond the 2 MiB window
BIG = ["K_4MiB", "B_4MiB"]           # golden digests and the device only


def window_log(n):
    """zs_level3_cparams(n).windowLog (csrc/zstd_common.h): the window the profile's frames declare."""
    w = 14 if n <= 16 * KiB else 17 if n <= 128 * KiB else 18 if n <= 256 * KiB else 21
    src_log = max((n - 1).bit_length(), 6) if n >= 64 else 6
    return max(min(w, src_log), 10)


_BASES = {}


def _base(kind):
    if kind not in _BASES:
        n = MiB + 13
        if kind in ("K", "B", "R"):
            x = synth.gen_chunk(kind, 77, 0, 0, n)
        elif kind == "zeros":
            x = np.zeros(n, np.uint8)
        elif kind == "period3":
            x = np.tile(np.frombuffer(b"xyz", np.uint8), n // 3 + 1)[:n]
        else:                                                          # twin slices: every 2 KiB equals the 2 KiB before it
            x = np.tile(np.random.default_rng(20261020).integers(0, 256, 2048, dtype=np.uint8), n // 2048 + 1)[:n]
        x = np.ascontiguousarray(x, dtype=np.uint8); x.setflags(write=False)
        _BASES[kind] = x
    return _BASES[kind]


def case(name):
    if name == FAR:
        unit = np.random.default_rng(20261021).integers(0, 256, 2 * MiB + 3, dtype=np.uint8)
        return np.ascontiguousarray(np.tile(unit, 2)[:2 * MiB + 512 * KiB])
    if name in BIG:
        return synth.gen_chunk(name[0], 78, 0, 0, 4 * MiB)
    kind, n = name.rsplit("_", 1)
    return _base(kind)[:int(n)]


def names(upto=MiB + 13, far=True):
    """The case list in its fixed order: every content at every size (<= upto), then the far-period case."""
    out = ["%s_%d" % (k, s) for k in KINDS for s in SIZES if s <= upto]
    return out + ([FAR] if far else [])


def golden():
    with open(GOLDEN) as f:
        return json.load(f)["frames"]


def digest(frame):
    return {"size": len(frame), "sha256": hashlib.sha256(frame).hexdigest()}


def run(N, flags, chunks, **kw):
    """tests/level_cases.run_transform with the profile set (zstd_level 0: the profile has no levels)."""
    return lc.run_transform(N, flags, chunks, 0, profile=DEVICE, **kw)


def resolved_offsets(blocks):
    """(position, offset, block number) of every sequence, the repeat-offset history followed as a decoder does."""
    rep, pos, out = [1, 4, 8], 0, []
    for bi, b in enumerate(blocks):
        start = pos
        for ll, ml, ob in b.seqs:
            pos += ll
            if ob > 3:
                off = ob - 3; rep = [off, rep[0], rep[1]]
            else:
                idx = ob - 1 + (1 if ll == 0 else 0)
                if idx == 0:
                    off = rep[0]
                elif idx == 1:
                    off = rep[1]; rep = [off, rep[0], rep[2]]
                elif idx == 2:
                    off = rep[2]; rep = [off, rep[0], rep[1]]
                else:
                    off = rep[0] - 1; rep = [off, rep[0], rep[1]]
            out.append((pos, off, bi))
            pos += ml
        pos = start + b.regen
    return out


def check_frame(o, frame, x, what=""):
    """Everything about one frame that needs no device: libzstd and the inspector restore the chunk, the format limits hold."""
    raw = x.tobytes()
    n = len(raw)
    assert len(frame) <= o.zstd_compress_bound(n), (what, n, len(frame))
    assert o.zstd_decompress_chunk(frame) == raw, "%s: libzstd does not restore the chunk" % what
    hdr, blocks, back = zi.parse_frame(frame, decode=True)
    assert back == raw, "%s: the inspector does not restore the chunk" % what
    assert hdr["frame_size"] == len(frame) - (4 if hdr["checksum"] else 0), what
    assert hdr.get("content_size") == n, (what, hdr)
    wlog = window_log(n)
    assert hdr["single_segment"] == ((1 << wlog) >= n), (what, hdr)
    if not hdr["single_segment"]:
        assert hdr["window_log"] == wlog and hdr["window_mantissa"] == 0, (what, hdr)
    assert all(b.regen <= BLOCK for b in blocks), what
    assert [b.regen for b in blocks[:-1]] == [BLOCK] * (len(blocks) - 1), "%s: blocks are cut at fixed 128 KiB" % what
    for pos, off, bi in resolved_offsets(blocks):
        assert 0 < off <= min(pos, 1 << wlog), "%s: offset %d at position %d (block %d, window 2^%d)" % (what, off, pos, bi, wlog)
    assert all(ml >= 4 for b in blocks for _, ml, _ in b.seqs), what
    return blocks


def check_decoders(N, chunks, frames, flags=None):
    """Both device decoder forms restore every chunk (the block form is the default for small batches; dec_block_chunks = 0 is the chunk form)."""
    flags = nat.COMPRESS if flags is None else flags
    sizes = [int(c.size) for c in chunks]
    for form in ("block", "chunk"):
        with N.configured(**({"dec_block_chunks": 0} if form == "chunk" else {})):
            back, d2 = pc.run_detransform(N, flags, frames, sizes)
        for i, c in enumerate(chunks):
            assert d2["status"][i] == 0, (form, i, sizes[i], int(d2["status"][i]))
            assert back[i] == c.tobytes(), "%s form: chunk %d (%d bytes)" % (form, i, sizes[i])


def check_pass(N, o, chunks, frames, d, labels=None):
    """The issue's "a chunk passes", for a COMPRESS-only batch."""
    for i, c in enumerate(chunks):
        what = labels[i] if labels else "chunk %d" % i
        assert d["status"][i] == 0, (what, int(d["status"][i]))
        check_frame(o, frames[i], c, what)
    check_decoders(N, chunks, frames)


def repeat_share(blocks):
    """(sequences that use a repeat code, all sequences) of a parsed frame."""
    seqs = [s for b in blocks for s in b.seqs]
    return sum(1 for _, _, ob in seqs if ob <= 3), len(seqs)


# ---- the second family: seeded fuzz, the window's edge, aimed block sequences, chunks over 4 MiB --------------------------------------
# The cases above are homogeneous contents at many sizes.  These are not: 96 structured random inputs (tests/fuzz_cases.py), a pair of
# copies exactly D bytes apart for D either side of the 2 MiB window, inputs aimed at what the frame loop does between blocks of
# different types, and two chunks over 4 MiB.  Digests and census: tests/golden/device_profile_fuzz_frames.json.
FUZZ_GOLDEN = os.path.join(os.path.dirname(GOLDEN), "device_profile_fuzz_frames.json")
WINDOW = 1 << 21
FUZZ_SEED = 20261022
FUZZ_KINDS = ["small"] * 64 + ["collision"] * 16 + ["accel"] * 16
FUZZ = ["fuzz_%03d" % i for i in range(len(FUZZ_KINDS))]
EDGE_D = [WINDOW - 1, WINDOW, WINDOW + 1, WINDOW + 2048]
EDGE = ["edge_%d_%s" % (D, f) for D in EDGE_D for f in ("zeros", "noise")]
EDGE_LEAD, EDGE_U, EDGE_TAIL = 100, 6000, 3000
AIMED = ["rep_over_raw", "rep_over_raw_twin", "raw_then_K", "ll_70000", "K_then_short_run", "matches_in_raw"]
BIG_EMU = ["mixed6"]                 # emulator, golden digests and the device
BIG_DEVICE = ["mixed10"]             # golden digests and the device only
SLICE = BLOCK // 64
REP_RAW_DIST = SLICE + 8             # rep_over_raw: the offset of the one match in the block that comes out raw
REP_TWIN_DIST = 2 * SLICE + 8        # ... and of block 0's last sequence


def label(name):
    return "%s (%s)" % (name, FUZZ_KINDS[int(name[5:])]) if name in FUZZ else name


def _noise(*key):
    """Incompressible bytes from a generator of their own: no state shared between cases."""
    def draw(n):
        return rng.integers(0, 256, n, dtype=np.uint8)
    rng = np.random.default_rng([20261023] + [int(k) for k in key])
    return draw


_FUZZ = {}


def _fuzz_inputs():
    """All 96 at once: one generator, one order (64 small, 16 collision, 16 accel)."""
    if not _FUZZ:
        from tests import fuzz_cases as fz
        rng = np.random.default_rng(FUZZ_SEED)
        for name, kind in zip(FUZZ, FUZZ_KINDS):
            x = np.ascontiguousarray(fz.level_case(rng, 3, kind), dtype=np.uint8); x.setflags(write=False)
            _FUZZ[name] = x
    return _FUZZ


def edge_case(D, filler, key=0):
    """100 noise | U (6000 noise bytes) | filler | U | 3000 noise, the two U exactly D bytes apart: the only source of the second U lies
    at distance D, so for D = 2 MiB the candidate AT the window's edge decides the parse, and for D = 2 MiB + 1 the one just beyond it."""
    draw = _noise(1, D, filler == "noise", key)
    U = draw(EDGE_U)
    U[0] |= 1                                                       # (a run of zeros in front of it does not reach into U)
    fill = draw(D - EDGE_U) if filler == "noise" else np.zeros(D - EDGE_U, np.uint8)
    return np.concatenate([draw(EDGE_LEAD), U, fill, U, draw(EDGE_TAIL)])


def edge_second_copy(name):
    """(D, first byte, end) of the second U in an edge case."""
    D = int(name.split("_")[1])
    return D, EDGE_LEAD + D, EDGE_LEAD + D + EDGE_U


def _k(lo, hi):
    return _base("K")[lo:hi]


def _plant(x, at, src, n):
    x[at:at + n] = x[src:src + n]


def _rep_over_raw(dist2):
    """Block 0 compresses and its last sequence has offset REP_TWIN_DIST; block 1 is noise with ONE match (24 bytes at REP_RAW_DIST), so it is
    parsed, leaves that offset in the parse's history and comes out raw; block 2 is 10 noise bytes, 200 bytes copied from `dist2` back, then K.
    A decoder never saw block 1's sequence: with dist2 = REP_RAW_DIST block 2's first sequence must carry its offset, with dist2 =
    REP_TWIN_DIST it is the repeat code.  Every copy lies 8 bytes into a slice and its source at a slice's first byte, where the parse visits
    every position."""
    draw = _noise(2)
    b0 = np.concatenate([_k(0, BLOCK - 3 * SLICE), draw(3 * SLICE)])
    _plant(b0, BLOCK - SLICE + 8, BLOCK - SLICE + 8 - REP_TWIN_DIST, 24)
    b1 = draw(BLOCK)
    _plant(b1, BLOCK - SLICE + 8, BLOCK - SLICE + 8 - REP_RAW_DIST, 24)
    x = np.concatenate([b0, b1, draw(10), np.zeros(200, np.uint8), _k(BLOCK, BLOCK + 40000)])
    _plant(x, 2 * BLOCK + 10, 2 * BLOCK + 10 - dist2, 200)
    return x


def _aimed(name):
    draw = _noise(3, AIMED.index(name))
    if name == "rep_over_raw":
        return _rep_over_raw(REP_RAW_DIST)
    if name == "rep_over_raw_twin":
        return _rep_over_raw(REP_TWIN_DIST)
    if name == "raw_then_K":                                        # a compressed block whose every table is new, after a raw one
        return np.concatenate([draw(BLOCK), _k(0, 200000)])
    if name == "ll_70000":                                          # a literal length of 70 002: beyond the last literal-length code's base (65 536)
        return np.concatenate([_k(0, BLOCK), draw(70000), _k(0, 3000), draw(70001), _k(100, 900)])
    if name == "K_then_short_run":                                  # (a full block of one byte has 64 sequences and compresses: RLE takes a short last block)
        return np.concatenate([_k(0, BLOCK), np.full(100, 0x5A, np.uint8)])
    if name == "matches_in_raw":                                    # the frame's first block: a few matches, raw all the same; block 1 starts with a match
        x = np.concatenate([draw(BLOCK), np.zeros(300, np.uint8), _k(0, 50000)])
        for s in (9, 20, 31, 50):
            _plant(x, s * SLICE + 8, (s - 2) * SLICE, 32)
        _plant(x, BLOCK, 40 * SLICE, 300)
        return x
    raise ValueError(name)


def fuzz_names(big=True, device_only=True):
    """The second family in its fixed order."""
    return FUZZ + EDGE + AIMED + ((BIG_EMU + (BIG_DEVICE if device_only else [])) if big else [])


def fuzz_case(name):
    if name in FUZZ:
        return _fuzz_inputs()[name]
    if name in EDGE:
        _, D, filler = name.split("_")
        return edge_case(int(D), filler)
    if name in AIMED:
        return np.ascontiguousarray(_aimed(name))
    if name in BIG_EMU + BIG_DEVICE:
        return pc.big_chunk(name)
    raise ValueError(name)


def fuzz_golden():
    with open(FUZZ_GOLDEN) as f:
        return json.load(f)


def sequences(frame):
    """(blocks, [(position, literal length, match length, offBase, resolved offset, block number)]) without decoding literals or output."""
    blocks = zi.parse_frame(frame, decode="sizes")[1]
    flat = [(ll, ml, ob) for b in blocks for ll, ml, ob in b.seqs]
    return blocks, [(pos, ll, ml, ob, off, bi) for (pos, off, bi), (ll, ml, ob) in zip(resolved_offsets(blocks), flat)]


def census(frames):
    """What a set of frames reaches, so that a test can say the set has not gone vacuous: block types, transitions from a raw or RLE block
    to a compressed one (and those whose compressed block starts with literals), the largest literal length, offsets at and near the 2 MiB
    window's edge, and the share of sequences that use the repeat code."""
    c = {"frames": 0, "blocks": {"raw": 0, "rle": 0, "compressed": 0}, "raw_to_compressed": 0, "rle_to_compressed": 0,
         "raw_or_rle_to_compressed_first_ll_gt_0": 0, "max_lit_length": 0, "offsets_at_window": 0, "offsets_near_window": 0,
         "max_offset": 0, "sequences": 0, "repeat_code_sequences": 0}
    for f in frames:
        blocks, seqs = sequences(f)
        c["frames"] += 1
        for i, b in enumerate(blocks):
            c["blocks"][b.btype] += 1
            if i and b.btype == "compressed" and blocks[i - 1].btype != "compressed":
                c["%s_to_compressed" % blocks[i - 1].btype] += 1
                if b.seqs and b.seqs[0][0] > 0:
                    c["raw_or_rle_to_compressed_first_ll_gt_0"] += 1
        for pos, ll, ml, ob, off, bi in seqs:
            c["max_lit_length"] = max(c["max_lit_length"], ll)
            c["max_offset"] = max(c["max_offset"], off)
            c["offsets_at_window"] += off == WINDOW
            c["offsets_near_window"] += WINDOW - 4096 < off <= WINDOW
            c["repeat_code_sequences"] += ob <= 3
        c["sequences"] += len(seqs)
    return c
