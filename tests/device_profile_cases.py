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
