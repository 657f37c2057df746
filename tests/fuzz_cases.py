"""Structured random inputs for differential tests of the Zstd kernels against the real libzstd (shared by
tools/fuzz_emu.py, the emulator tests and the GPU tests)."""
import numpy as np

from tsxform import synth


def gen_case(rng, total=None):
    """A byte string built from segments of different statistical character, with cross references at all distances."""
    if total is None:
        total = int(rng.choice([rng.integers(0, 300), rng.integers(300, 20000), rng.integers(20000, 140000), rng.integers(126000, 136000),
                                rng.integers(140000, 420000), rng.integers(255000, 270000)]))
    parts, made = [], 0
    pool = []
    while made < total:
        kind = rng.integers(0, 9)
        n = int(min(total - made, rng.choice([rng.integers(1, 40), rng.integers(40, 2000), rng.integers(2000, 60000)])))
        if kind == 0:
            seg = rng.integers(0, 256, n, dtype=np.uint8)
        elif kind == 1:
            seg = rng.integers(0, int(rng.integers(2, 20)), n, dtype=np.uint8)
        elif kind == 2:
            seg = np.full(n, rng.integers(0, 256), np.uint8)
        elif kind == 3:
            p = rng.integers(0, 256, int(rng.integers(1, 70)), dtype=np.uint8)
            seg = np.tile(p, n // p.size + 1)[:n]
        elif kind == 4:
            seg = synth.gen_chunk("K", int(rng.integers(0, 1 << 30)), 0, 0, n)
        elif kind == 5 and pool:                                   # verbatim copy of an earlier part (match at its distance)
            src = pool[int(rng.integers(0, len(pool)))]
            o = int(rng.integers(0, max(1, src.size - 1)))
            seg = src[o:o + n].copy()
            n = seg.size
        elif kind == 6 and pool:                                   # earlier part with sparse byte edits (repcode-rich)
            src = pool[int(rng.integers(0, len(pool)))]
            o = int(rng.integers(0, max(1, src.size - 1)))
            seg = src[o:o + n].copy()
            n = seg.size
            if n:
                k = int(rng.integers(1, 2 + n // int(rng.integers(4, 200))))
                seg[rng.integers(0, n, k)] = rng.integers(0, 256, k, dtype=np.uint8)
        elif kind == 7:
            seg = np.minimum(rng.geometric(float(rng.uniform(0.05, 0.6)), n), 255).astype(np.uint8)
        else:
            seg = (np.arange(n) * int(rng.integers(1, 5)) % 256).astype(np.uint8)
        if n == 0:
            continue
        parts.append(seg); pool.append(seg); made += n
    return np.concatenate(parts)[:total] if parts else np.zeros(0, np.uint8)


# ---- levels 1 and 2 (strategy fast): inputs for the window's edge, shared buckets within one wave step, and step acceleration ----
LEVEL_WINDOW = {1: 1 << 19, 2: 1 << 20, 3: 1 << 21}          # window size for sources above 256 KiB
BLOCK = 131072


def _long_match_filler(rng, n):
    """n bytes the fast parser covers with a few long matches, so a small hash table (16 K entries at level 1) still holds what came before
    them: zeros, a short tiled unit or a long one.  (Incompressible bytes would keep the table too - the accelerated search inserts few of
    them - but a search that arrives at A with a step of hundreds finds nothing there.)"""
    kind = int(rng.integers(0, 3))
    if kind == 0 or n == 0:
        return np.zeros(n, np.uint8)
    unit = rng.integers(0, 256, int(rng.integers(1, 301) if kind == 1 else rng.integers(300, 5001)), dtype=np.uint8)
    return np.tile(unit, n // unit.size + 1)[:n]


def fast_block_ends(x):
    """Where libzstd 1.5.7 ends the blocks of x at levels 1 and 2 once its first block has compressed: the pre-splitter of strategy fast
    compares byte histograms of a 128 KiB block's first and last 512 bytes and, when they differ, cuts at 32, 64 or 96 KiB by the middle's.
    A model to aim inputs with (the blocks after a cut are no longer aligned to 128 KiB); tests judge by libzstd's own frames."""
    ends, pos, n = [], 0, int(x.size)
    while n - pos >= BLOCK:
        size = BLOCK
        if pos:
            b, e, m = (np.bincount(x[pos + o:pos + o + 512], minlength=256).astype(np.int64) for o in (0, BLOCK - 512, BLOCK // 2 - 256))
            if np.abs(b - e).sum() * 16 >= 512 * 14:
                dB, dE = int(np.abs(b - m).sum()), int(np.abs(e - m).sum())
                size = 65536 if abs(dB - dE) * 3 < 512 else 32768 if dB > dE else 98304
        pos += size; ends.append(pos)
    if pos < n:
        ends.append(n)
    return ends


def straddle_case(rng, W):
    """lead | A | mid | A | tail with the second A ending a block (at E) so that its partner crosses the low edge of that block's window
    (valid candidates are the positions >= E - W): the partner of its first x bytes lies just below the edge, the rest just inside, at
    distance W - t.  A parser that is off by one at the edge, or counts backwards past it, emits another frame than libzstd.  (A match
    found a position late is extended backwards to the edge all the same; where only minMatch bytes lie inside, there is no later one.)
    A itself, at a block's border, makes the pre-splitter cut, and the blocks after a cut end elsewhere: E moves up in steps of 32 KiB
    (the lead grows) to the first place where fast_block_ends() expects a block to end."""
    A = rng.integers(0, 256, int(rng.integers(64, 6001)), dtype=np.uint8)
    t = int(rng.integers(9, 64)) if rng.integers(0, 2) else int(rng.integers(64, 4000))
    x = int(rng.integers(0, min(A.size, 2000)))
    if rng.integers(0, 3) == 0:                                    # a short A with just minMatch bytes inside (7 / 6 at levels 1 / 2 past 256 KiB):
        A = A[:int(rng.integers(64, 136))]                         # the one candidate AT the edge, every position up to it visited
        x = A.size - {1 << 19: 7, 1 << 20: 6}.get(W, 5)
    E = W + BLOCK * int(rng.integers(1, 3))
    lead = _long_match_filler(rng, E - W - x + 3 * 32768) if rng.integers(0, 3) else gen_case(rng, E - W - x + 3 * 32768)
    mid = _long_match_filler(rng, W - t - A.size)
    tail = gen_case(rng, int(rng.integers(0, 150001)))
    for j in (0, 1, 2, 3):
        case = np.concatenate([lead[:E - W - x + j * 32768], A, mid, A, tail])
        if E + j * 32768 in fast_block_ends(case):
            return case
    return np.concatenate([lead[:E - W - x], A, mid, A, tail])


def _texture(rng, n):
    kind = int(rng.integers(0, 3))
    if kind == 0:                                                  # an alphabet of 1 - 3 symbols
        syms = rng.integers(0, 256, int(rng.integers(1, 4)), dtype=np.uint8)
        return syms[rng.integers(0, syms.size, n)]
    if kind == 1:                                                  # a period of 1 - 8 bytes, one byte edited every 60 - 130
        unit = rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8)
        x = np.tile(unit, n // unit.size + 1)[:n]
        at = np.cumsum(rng.integers(60, 131, n // 60 + 1))
    else:                                                          # runs of one byte, broken at random distances below 64
        x = np.full(n, rng.integers(0, 256), np.uint8)
        at = np.cumsum(rng.integers(1, 64, n + 1))
    at = at[at < n]
    x[at] = rng.integers(0, 256, at.size, dtype=np.uint8)
    return x


def collision_case(rng, n):
    """Low-entropy textures over n bytes (at least three blocks): many of the up to 62 positions of one wave step fall into one bucket."""
    parts, made = [], 0
    while made < n:
        m = int(min(n - made, rng.integers(30000, 150001)))
        seg = _texture(rng, m)
        if rng.integers(0, 4) == 0:                                # two textures interleaved, in pieces of 1 - 399 bytes
            other = _texture(rng, m)
            pieces = rng.integers(1, 400, m // 100 + 2)
            take = np.repeat(np.arange(pieces.size) & 1, pieces)[:m].astype(bool)
            seg = np.where(take, other, seg)
        parts.append(seg); made += m
    return np.concatenate(parts)


def accel_case(rng, n):
    """Incompressible stretches of 100 - 20000 bytes (the search step grows by one every 128 bytes without a match: 2, 3, 4, 5 ... 150), each
    followed by a copy of earlier bytes - mostly the start of a recent stretch, where every position was inserted - that begins at an even
    offset of its stretch in some cases and an odd one in others, so the first match falls on either position of a pair.
    For a match on the second position, libzstd also inserts the first position of the next pair while the step is at most 4 (stretches of
    under 384 bytes; that position lies 3 bytes into the copy at step 4), and only a later search for those very bytes tells: half of the
    copies repeat the one before them from 3 bytes further on."""
    out = np.empty(n, np.uint8)
    starts, made, src = [], 0, None
    while made < n:
        L = int(rng.choice([rng.integers(100, 400), rng.integers(256, 384), rng.integers(400, 3000), rng.integers(256, 384),
                            rng.integers(3000, 20001) if rng.integers(0, 2) else rng.integers(100, 3000)]))
        L = min((L & ~1) | int(rng.integers(0, 2)), n - made)
        out[made:made + L] = rng.integers(0, 256, L, dtype=np.uint8)
        starts.append(made); made += L
        if made >= n:
            break
        if src is not None and rng.integers(0, 2):
            src += 3
        else:
            src = starts[int(rng.integers(max(0, len(starts) - 4), len(starts)))] if rng.integers(0, 2) else starts[int(rng.integers(0, len(starts)))]
            src += int(rng.choice([0, rng.integers(0, 9), rng.integers(0, 64)]))
        m = int(min(rng.integers(8, 1500), n - made, made - src))
        out[made:made + m] = out[src:src + m]
        made += m
    return out


def level_case(rng, level, kind):
    """One input of `kind` sized for `level`'s window (tools/fuzz_*.py --level, the device fuzz)."""
    W = LEVEL_WINDOW[level]
    if kind == "small":
        return gen_case(rng)
    if kind == "straddle":
        return straddle_case(rng, W)
    if kind == "big":
        return gen_case(rng, W + int(rng.integers(0, 300001)))
    if kind == "collision":
        return collision_case(rng, int(rng.integers(300000, 420001)))
    if kind == "accel":
        return accel_case(rng, int(rng.integers(300000, 420001)))
    raise ValueError(kind)


def offsets_near_window(frame, W, within=4096):
    """How many explicit offsets of `frame` (libzstd's own, say) lie in (W - within, W]: does an input reach the window's low edge at all?"""
    from tests import zstd_inspect as zi
    return sum(1 for b in zi.parse_frame(frame, decode=True)[1] for _, _, ob in b.seqs if ob > 3 and W - within < ob - 3 <= W)



# Full-size chunks on which the sliding of the 2 MiB window decides the output: repcodes / match candidates that lie between
# 2 MiB - blockSize and 2 MiB behind the block, one of them exactly AT the lowest valid index (found by tools/fuzz_gpu.py; a
# restatement that slides the window to the block's end, or excludes the bound itself, differs from libzstd 1.5.7 on every one).
WINDOW_EDGE_SEEDS = (1009, 1045, 1071, 1093, 1096, 1113)


def window_edge_case(seed):
    return gen_case(np.random.default_rng(seed), 4194304 - (seed % 3) * 40000)


def window_edge_cases():
    return [window_edge_case(s) for s in WINDOW_EDGE_SEEDS]


def header_cases():
    """tests/golden/fuzz_regress/hdr_*.bin, by name: the smallest inputs whose level-3 frames carry the literal-section headers no other case
    of the differential tests produces.  No RNG: incompressible bytes come from SHA-256 in counter mode.
      hdr_lit_raw_31 / 32 / 33   n noise bytes, then nine copies: n raw literals and one match - the 1-byte header ends at 31
      hdr_lit_raw_4095 / 4096    the same with one copy: the 2-byte header ends at 4095
      hdr_lit_rle_70             RLE literals in a compressed block.  Every literal of the block must be the same byte, and a frame's first bytes
                                 are literals of whatever they are, so it takes a SECOND block, i.e. a first one of 128 KiB: 200-byte noise
                                 segments, each closed by an 8-byte marker (a match every 208 bytes keeps the parser visiting every position);
                                 then seventy times one byte 0xA5 and 32 bytes from the middle of a segment - seventy equal literals between
                                 seventy matches.  133 382 bytes: no shorter input has a second block."""
    import hashlib
    noise = np.frombuffer(b"".join(hashlib.sha256(b"tsx header cases %d" % i).digest() for i in range(4200)), np.uint8)
    c = {}
    for n in (31, 32, 33):
        c["hdr_lit_raw_%d" % n] = np.tile(noise[:n], 10)
    for n in (4095, 4096):
        c["hdr_lit_raw_%d" % n] = np.concatenate([noise[:n], noise[:n]])
    marker = np.frombuffer(b"~marker~", np.uint8)
    segs = [noise[200 * j:200 * j + 200] for j in range(640)]
    parts = [np.concatenate([np.concatenate([s, marker]) for s in segs])[:BLOCK]]
    for j in range(5, 355, 5):
        parts += [np.array([0xA5], np.uint8), segs[j][60:92]]
    c["hdr_lit_rle_70"] = np.concatenate(parts)
    return c
