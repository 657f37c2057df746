"""Every frame feature libzstd emits, and libzstd's verdict on damaged frames: cases shared by the emulated and the device tests of the two
decoder forms (csrc/zstd_dec.hip, csrc/zstd_dec_blocks.hip; both parse through csrc/zstd_dec_dev.h).

The vocabulary is a table of (content, advanced parameters) whose frames - made by the real libzstd 1.5.7 the oracle has loaded - together
hold every block type, literals mode, Huffman tree description, sequence table mode, sequence count format and inheritance pattern of
RFC 8878 that the library can be made to emit.  `census` counts them with tests/zstd_inspect.py and `check_vocabulary_is_covered` asserts
the counts before a byte is decoded: conditions on libzstd's frames, not on the code under test.

The damaged corpus flips bits inside every kind of region of about ten such frames (`regions`), truncates them and inserts bytes at region
boundaries.  Each damaged frame carries libzstd's own verdict - the bytes ZSTD_decompress returned, or its error name - and
`check_verdicts` holds both forms to it.  `N` is a tsxform._native.Native (emulated or real); `o` is the oracle module."""
import collections

import numpy as np

import tsxform
from tests import checksum_cases as cc
from tests import zstd_inspect as zi
from tsxform import synth

nat = tsxform._native
LEVEL, WINDOW_LOG, TARGET_CBLOCK, CHECKSUM, LITERAL_MODE, MAX_BLOCK = 100, 101, 130, 201, 1002, 1015      # ZSTD_cParameter numbers of 1.5.7
REJECT = (nat.E_BAD_FRAME, nat.E_BAD_SIZE, nat.E_DST_TOO_SMALL)
STRICT = "huffman stream not fully consumed"                              # the one place where the decoder is stricter than libzstd 1.5.7
ZB_MAX_BLOCKS = 264                                                      # csrc/zstd_dec_blocks.h: frames of more blocks go to the chunk form


def libzstd_frame(o, data, params):
    """libzstd's frame of `data`: pledged size, content size flag, then every (parameter, value) of `params` in order, ZSTD_compress2."""
    Z = cc.libzstd(o)
    a = np.ascontiguousarray(np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data)
    cap = Z.ZSTD_compressBound(a.size)
    dst = np.zeros(max(cap, 1), np.uint8)
    c = Z.ZSTD_createCCtx()
    try:
        assert not Z.ZSTD_isError(Z.ZSTD_CCtx_setPledgedSrcSize(c, a.size))
        assert not Z.ZSTD_isError(Z.ZSTD_CCtx_setParameter(c, 200, 1))
        for prm, v in params:
            r = Z.ZSTD_CCtx_setParameter(c, prm, v)
            assert not Z.ZSTD_isError(r), (prm, v, Z.ZSTD_getErrorName(r))
        r = Z.ZSTD_compress2(c, dst.ctypes.data, cap, a.ctypes.data, a.size)
        assert not Z.ZSTD_isError(r), Z.ZSTD_getErrorName(r)
    finally:
        Z.ZSTD_freeCCtx(c)
    return dst[:r].tobytes()


def libzstd_verdict(o, blob, size):
    """ZSTD_decompress of a frame into exactly `size` bytes: the bytes it returned, or (a str) the name of its error."""
    Z = cc.libzstd(o)
    src = np.frombuffer(blob, np.uint8) if blob else np.zeros(1, np.uint8)
    dst = np.zeros(max(size, 1), np.uint8)
    r = Z.ZSTD_decompress(dst.ctypes.data, size, src.ctypes.data, len(blob))
    return Z.ZSTD_getErrorName(r).decode() if Z.ZSTD_isError(r) else dst[:r].tobytes()


# ---- content (fixed seeds, numpy only) ---------------------------------------------------------------------------------------------
def K(n): return synth.gen_chunk("K", 9, 1, 3, n)
def B(n): return synth.gen_chunk("B", 9, 1, 3, n)


def const_seq(n, ll, ml, lit=97, seed=5):
    """A 64 KiB random pool, then `ll` copies of one byte + `ml` bytes from a random place of the pool, over and over: every sequence has
    the same literal length and match length (RLE-mode tables), every literal is the same byte (RLE literals)."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, 65536).astype(np.uint8)
    reps = (max(n - pool.size, 0) + ll + ml - 1) // (ll + ml)
    at = rng.integers(0, 65536 - ml, reps)
    body = np.empty((reps, ll + ml), np.uint8)
    body[:, :ll] = lit
    body[:, ll:] = pool[at[:, None] + np.arange(ml)[None, :]]
    return np.concatenate([pool, body.reshape(-1)])[:n]


def words(n, nw, seed=5):
    """`nw` random 4-byte words, then a random sequence of them: tens of thousands of minimum-length matches in a block."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 256, (nw, 4)).astype(np.uint8)
    idx = rng.integers(0, nw, (n - nw * 4) // 4)
    return np.concatenate([w.reshape(-1), w[idx].reshape(-1)])


def low(k, n, seed=7):
    return np.random.default_rng(seed).integers(0, k, n).astype(np.uint8)


def skewlow(n, k=12, seed=7):
    """Bytes 0..k-1, each half as likely as the one before: a Huffman tree of few symbols, described by direct weights."""
    p = np.array([2.0 ** -i for i in range(1, k + 1)]); p /= p.sum()
    return np.random.default_rng(seed).choice(k, n, p=p).astype(np.uint8)


def zeros_K_const(nz, nk, nc):
    return np.concatenate([np.zeros(nz, np.uint8), K(nk), np.full(nc, 9, np.uint8)])


def sparse(n, per, k=64, ml=30, seed=3):
    """Uniform bytes 0..k-1 with `ml` bytes copied from a random earlier place every `per` bytes: few sequences between long literals."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, k, n).astype(np.uint8)
    for p in range(per, n - ml, per):
        q = int(rng.integers(0, p - ml))
        x[p:p + ml] = x[q:q + ml]
    return x


def periodic(n, period=600, seed=3):
    """One random period over and over; every 20 to 60 bytes a byte changes for good.  Behind the first period every sequence is one
    literal and a match at the same distance: the repeat-offset code alone, an RLE-mode offset table."""
    rng = np.random.default_rng(seed)
    x = np.tile(rng.integers(0, 256, period).astype(np.uint8), n // period + 1)[:n].copy()
    pos = np.cumsum(rng.integers(20, 60, n // 20))
    for p in pos[(pos > period) & (pos < n)]:
        x[p::period] ^= np.uint8(rng.integers(1, 256))
    return x


# ---- the vocabulary ------------------------------------------------------------------------------------------------------------------
# (name, content, parameters).  Sizes are the smallest tried at which the features named on the right survived in libzstd 1.5.7's frames;
# the census below, not this table, is what the tests rely on.  A sub-block of a split block (target size) says Repeat for all three
# tables whatever the first sub-block's modes were: that is where Repeats of RLE and of predefined tables come from.
def _table():
    return [
        ("K level -5", K(60000), [(LEVEL, -5)]),                                          # raw literals with sequences
        ("K window 10", K(60000), [(LEVEL, 3), (WINDOW_LOG, 10)]),                        # Window_Descriptor, 1 KiB blocks, 1-byte counts, predefined LL / ML
        ("B window 10 long", B(272000), [(LEVEL, 3), (WINDOW_LOG, 10)]),                  # more than 264 blocks: the chunk form's; raw blocks between
        ("K level 19 window 14", K(120000), [(LEVEL, 19), (WINDOW_LOG, 14)]),             # Repeats of all three tables, treeless
        ("sparse target 1340", sparse(131072, 1000), [(LEVEL, 3), (TARGET_CBLOCK, 1340)]),    # 71 blocks in a row inherit tree and tables; treeless-1
        ("sparse level 5 window 13 target 1340", sparse(60000, 1000), [(LEVEL, 5), (WINDOW_LOG, 13), (TARGET_CBLOCK, 1340)]),    # Repeat of predefined
        ("periodic target 1340", periodic(262144), [(LEVEL, 3), (TARGET_CBLOCK, 1340)]),  # RLE-mode OF, Repeat of RLE
        ("B level 19 block 1340", B(100000), [(LEVEL, 19), (MAX_BLOCK, 1340)]),           # everything mixed, 1-stream compressed
        ("const_seq level 19", const_seq(200000, 1, 8), [(LEVEL, 19)]),                   # RLE literals, RLE-mode LL and ML
        ("words level 19", words(262144, 4096), [(LEVEL, 19)]),                           # 3-byte sequence count
        ("low3", low(3, 40000), [(LEVEL, 3)]),                                            # direct Huffman weights
        ("low6 block 1340", low(6, 40000), [(LEVEL, 3), (MAX_BLOCK, 1340)]),              # treeless on a direct tree
        ("skewlow 5000", skewlow(5000), [(LEVEL, 3)]),
        ("low4 300", low(4, 300), [(LEVEL, 19)]),                                         # 0 sequences, one-block frames
        ("skewlow 150", skewlow(150), [(LEVEL, 19)]),
        ("low20 block 1340", low(20, 100000), [(LEVEL, 3), (MAX_BLOCK, 1340)]),           # zero-sequence blocks, RLE-mode ML, predefined + treeless
        ("zeros K const", zeros_K_const(140000, 30000, 140000), [(LEVEL, 3)]),            # RLE blocks, predefined tables
        ("K checksum", K(60000), [(LEVEL, 3), (CHECKSUM, 1)]),                            # a content checksum behind the last block
    ]


_VOCAB = None


def vocabulary(o):
    """-> [(name, source bytes, libzstd's frame)], built once."""
    global _VOCAB
    if _VOCAB is None:
        cc.need157(o)
        _VOCAB = [(name, x.tobytes(), libzstd_frame(o, x, params)) for name, x, params in _table()]
    return _VOCAB


MODES = ("predefined", "rle", "compressed", "repeat")
FEATURES = (["block raw", "block rle", "block compressed"]
            + ["literals raw", "literals rle", "literals compressed-1", "literals compressed-4", "literals treeless-1", "literals treeless-4"]
            + ["tree fse", "tree direct"] + ["%s %s" % (t, m) for t in ("ll", "of", "ml") for m in MODES]
            + ["repeat of rle", "repeat of predefined", "count 0", "count 1 byte", "count 2 bytes", "count 3 bytes",
               "window descriptor", "checksum"])


def census(blob):
    """What one frame contains, counted per block (FEATURES), plus "blocks" and "inherit run": the longest run of consecutive blocks
    that take both the Huffman tree (treeless literals) and all three sequence tables (Repeat) from earlier blocks.  The source of a
    Repeat is found the way zb_index_kernel finds it: the last earlier block with sequences whose mode for that table is no Repeat."""
    hdr, blocks, _ = zi.parse_frame(blob, decode=False)
    c = collections.Counter({"blocks": len(blocks), "window descriptor": int(not hdr["single_segment"]), "checksum": int(hdr["checksum"])})
    src = [None, None, None]
    run = 0
    for b in blocks:
        c["block " + b.btype] += 1
        inherits = False
        if b.btype == "compressed":
            c["literals " + (b.lit_type if b.lit_streams == 0 else "%s-%d" % (b.lit_type, b.lit_streams))] += 1
            if b.huf_header:
                c["tree " + b.huf_header] += 1
            c["count " + ("0" if b.nbseq == 0 else "1 byte" if b.nbseq < 128 else "2 bytes" if b.nbseq < 0x7F00 else "3 bytes")] += 1
            for k, (t, m) in enumerate(zip(("ll", "of", "ml"), b.modes)):
                c["%s %s" % (t, m)] += 1
                if m != "repeat":
                    src[k] = m
                elif src[k] in ("rle", "predefined"):
                    c["repeat of " + src[k]] += 1
            inherits = b.lit_type == "treeless" and b.modes == ("repeat",) * 3
        run = run + 1 if inherits else 0
        c["inherit run"] = max(c["inherit run"], run)
    return c


def check_vocabulary_is_covered(o):
    """Conditions on libzstd's frames alone.  -> the summed counts."""
    total = collections.Counter()
    sizes = []
    for name, x, blob in vocabulary(o):
        c = census(blob)
        sizes.append(c["blocks"])
        print("%-32s %7d -> %6d bytes, %3d blocks: %s" % (name, len(x), len(blob), c["blocks"], {k: v for k, v in sorted(c.items()) if v and k != "blocks"}))
        run = c.pop("inherit run")
        total.update(c)
        total["inherit run"] = max(total["inherit run"], run)
    print("vocabulary: %s" % {k: total[k] for k in FEATURES + ["inherit run"]})
    missing = [k for k in FEATURES if total[k] == 0]
    assert not missing, "no frame of the table holds: %s" % missing
    assert total["inherit run"] >= 30, total["inherit run"]
    assert min(sizes) <= 200 and max(sizes) > ZB_MAX_BLOCKS, sizes
    return total


def decode_batches(N, blobs, sizes, batch=128):
    """Both forms over `blobs`, at most `batch` frames a call.  -> {"block": (outs, statuses, kept), "chunk": ...}; kept is a list of
    flags, one per frame: the block form decoded it itself."""
    res = {"block": ([], [], []), "chunk": ([], [], [])}
    for lo in range(0, len(blobs), batch):
        part = cc.decode_both_forms(N, nat.COMPRESS, blobs[lo:lo + batch], sizes[lo:lo + batch])
        n = len(blobs[lo:lo + batch])
        for form, (outs, d, kept) in part.items():
            res[form][0].extend(outs); res[form][1].extend(int(s) for s in d["status"])
        res["block"][2].append((n, part["block"][2]))
    return res


_RESULTS = {}                                                            # (id(N), frame, size) -> {form: (status, CRC32C of the output)}


def _remember(N, o, blobs, sizes, res):
    for i, (f, n) in enumerate(zip(blobs, sizes)):
        _RESULTS[(id(N), f, n)] = {form: (res[form][1][i], o.crc32c(res[form][0][i])) for form in ("block", "chunk")}


def check_both_forms_restore(N, o, extra=()):
    """Every frame of the vocabulary (and of `extra`: (name, source, frame)) through both forms, one frame a batch so that
    tsx_debug_blockmode_chunks speaks about that frame."""
    cases = vocabulary(o) + list(extra)
    for name, x, blob in cases:
        assert o.zstd_decompress_chunk(blob, len(x)) == x, name
    wrong, left = {}, []
    for name, x, blob in cases:
        res = decode_batches(N, [blob], [len(x)])
        _remember(N, o, [blob], [len(x)], res)
        nblocks = len(zi.parse_frame(blob, decode=False)[1])
        for form in ("block", "chunk"):
            if res[form][1][0] != 0 or res[form][0][0] != x:
                wrong[(name, form)] = (res[form][1][0], len(res[form][0][0]))
        kept = res["block"][2][0][1]
        if kept != (1 if nblocks <= ZB_MAX_BLOCKS else 0):
            left.append((name, nblocks, kept))
    assert not wrong, wrong
    assert not left, "frames of at most %d blocks the block form did not keep (or larger ones it kept): %s" % (ZB_MAX_BLOCKS, left)
    return len(cases)


# ---- regions of a frame ------------------------------------------------------------------------------------------------------------
KINDS = ("frame header", "block header", "raw block", "RLE block", "literals header", "Huffman tree", "Huffman jump table", "Huffman streams",
         "raw/RLE literals", "sequences header", "table descriptions", "sequence bitstream", "checksum")


def regions(blob):
    """[(lo, hi, kind)], lo < hi, back to back over the whole frame; the kinds are KINDS."""
    hdr, blocks, _ = zi.parse_frame(blob, decode=False)
    p = hdr["header_size"]
    R = [(0, p, "frame header")]
    for b in blocks:
        R.append((p, p + 3, "block header"))
        body = p + 3
        if b.btype != "compressed":
            p = body + (b.size if b.btype == "raw" else 1)
            R.append((body, p, "raw block" if b.btype == "raw" else "RLE block"))
            continue
        R.append((body, body + b.lit_hl, "literals header"))
        q = body + b.lit_hl
        if b.lit_type in ("raw", "rle"):
            R.append((q, body + b.seq_at, "raw/RLE literals"))
        else:
            jump = 6 if b.lit_streams == 4 else 0
            R.append((q, q + b.huf_tree_size, "Huffman tree")); q += b.huf_tree_size
            R.append((q, q + jump, "Huffman jump table")); q += jump
            R.append((q, body + b.seq_at, "Huffman streams"))
        R.append((body + b.seq_at, body + b.seq_tables_at, "sequences header"))
        R.append((body + b.seq_tables_at, body + b.seq_stream_at, "table descriptions"))
        R.append((body + b.seq_stream_at, body + b.size, "sequence bitstream"))
        p = body + b.size
    if hdr["checksum"]:
        R.append((p, p + 4, "checksum")); p += 4
    assert p == len(blob)
    R = [r for r in R if r[1] > r[0]]
    assert all(a[1] == b[0] for a, b in zip(R, R[1:])) and R[0][0] == 0 and R[-1][1] == len(blob)
    return R


# ---- the damaged corpus ------------------------------------------------------------------------------------------------------------
def _bases():
    mixed = np.concatenate([np.zeros(4000, np.uint8), synth.gen_chunk("R", 9, 1, 4, 4000), K(12000), np.full(4000, 9, np.uint8)])
    return [
        (K(40000), [(LEVEL, 3)]),
        (K(40000), [(LEVEL, 19)]),
        (B(60000), [(LEVEL, 3)]),
        (B(60000), [(LEVEL, 19), (TARGET_CBLOCK, 1340)]),
        (K(40000), [(LEVEL, 3), (WINDOW_LOG, 10)]),
        (K(20000), [(LEVEL, -3)]),
        (skewlow(5000), [(LEVEL, 3), (MAX_BLOCK, 1340)]),
        (const_seq(90000, 1, 8), [(LEVEL, 19)]),
        (B(60000), [(LEVEL, 19), (MAX_BLOCK, 4096)]),
        (low(20, 20000), [(LEVEL, 3), (MAX_BLOCK, 1340)]),
        (mixed, [(LEVEL, 3), (MAX_BLOCK, 1340), (CHECKSUM, 1)]),
    ]


# flips per base frame and kind, once with one bit and once with two: more where libzstd accepts most damage (payload bytes), so that
# both verdicts keep at least a quarter of the corpus
FLIPS = collections.defaultdict(lambda: 2, {"Huffman streams": 6, "raw block": 5, "raw/RLE literals": 5, "sequence bitstream": 4})
Damaged = collections.namedtuple("Damaged", "blob size base kind how verdict")
_DAMAGED = None


def damaged(o):
    """-> [Damaged]: the deterministic plan described at the top, each frame with libzstd's verdict.  Built once."""
    global _DAMAGED
    if _DAMAGED is not None:
        return _DAMAGED
    cc.need157(o)
    out = []
    for bi, (x, params) in enumerate(_bases()):
        f = libzstd_frame(o, x, params)
        assert libzstd_verdict(o, f, x.size) == x.tobytes()
        R = regions(f)
        rng = np.random.default_rng(1000 + bi)
        for kind in KINDS:
            span = [r for r in R if r[2] == kind]
            if not span:
                continue
            at = np.concatenate([np.arange(lo, hi) for lo, hi, _ in span])
            for bits in (1, 2):
                for _ in range(FLIPS[kind]):
                    g = bytearray(f)
                    for _ in range(bits):
                        g[int(at[int(rng.integers(0, at.size))])] ^= 1 << int(rng.integers(0, 8))
                    out.append((bytes(g), x.size, bi, kind, "%d-bit flip" % bits))
        edges = [lo for lo, _, _ in R[1:]]
        for k in range(4):
            e = edges[int(rng.integers(0, len(edges)))]
            out.append((f[:e], x.size, bi, R[[r[0] for r in R].index(e)][2], "truncation"))
            e = edges[int(rng.integers(0, len(edges)))]
            ins = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
            out.append((f[:e] + ins + f[e:], x.size, bi, R[[r[0] for r in R].index(e)][2], "insertion"))
    _DAMAGED = [Damaged(blob, int(size), bi, kind, how, libzstd_verdict(o, blob, int(size))) for blob, size, bi, kind, how in out]
    return _DAMAGED


_STRICT = {}


def inspector_is_strict(blob):
    """True when tests/zstd_inspect.py, which follows RFC 8878 to the letter, refuses the frame for a Huffman stream that is not consumed
    exactly - the one check libzstd 1.5.7's fast Huffman loops leave out."""
    if blob not in _STRICT:
        try:
            zi.parse_frame(blob, decode=True)
            _STRICT[blob] = False
        except ValueError as e:
            _STRICT[blob] = STRICT in str(e)
        except Exception:                                               # noqa: BLE001 - a damaged frame may break the inspector anywhere
            _STRICT[blob] = False
    return _STRICT[blob]


def check_the_corpus_is_balanced(o):
    """Conditions on libzstd (and the inspector) alone."""
    D = damaged(o)
    accepted = sum(isinstance(d.verdict, bytes) for d in D)
    per_kind = collections.Counter(d.kind for d in D)
    print("damaged corpus: %d frames, libzstd accepts %d and rejects %d; per kind %s" % (len(D), accepted, len(D) - accepted, dict(per_kind)))
    assert 500 <= len(D) <= 700, len(D)
    assert 4 * accepted >= len(D) and 4 * (len(D) - accepted) >= len(D)
    assert all(per_kind[k] > 0 for k in KINDS), per_kind
    streams = [d for d in D if d.kind == "Huffman streams" and "flip" in d.how and isinstance(d.verdict, bytes)]
    strict = sum(inspector_is_strict(d.blob) for d in D if isinstance(d.verdict, bytes) and d.kind == "Huffman streams")
    print("libzstd accepts %d frames with a flip in a Huffman stream; RFC 8878 refuses %d of them" % (len(streams), strict))
    assert 2 * strict <= len(streams), (strict, len(streams))
    return len(D), accepted


def apply_rules(blob, size, verdict, status, out, strict=None):
    """Rules 1, 2 and 4 for one frame and one form.  -> (class, None) or (class, what is wrong).  The classes: "both reject",
    "both accept", "only we reject" (allowed for unconsumed Huffman streams alone), "only we accept"."""
    if isinstance(verdict, str):
        if status == 0:
            return "only we accept", "libzstd: %s, status 0 with %d bytes" % (verdict, len(out))
        return "both reject", None if status in REJECT else "status %d" % status
    if status == 0:
        return "both accept", None if out == verdict else "status 0, bytes differ from libzstd's (%d / %d)" % (len(out), len(verdict))
    if strict is None:
        strict = inspector_is_strict(blob)
    if strict and status == nat.E_BAD_FRAME:
        return "only we reject", None
    return "only we reject", "libzstd decodes it, status %d, %s" % (status, "Huffman stream not consumed" if strict else "no unconsumed Huffman stream")


def check_against_libzstd(o, blobs, sizes, statuses, outs):
    """Rules 1, 2 and 4 for frames from anywhere (the older damage tests)."""
    classes, wrong = collections.Counter(), []
    for i, (f, n) in enumerate(zip(blobs, sizes)):
        cls, err = apply_rules(f, n, libzstd_verdict(o, f, n), int(statuses[i]), outs[i])
        classes[cls] += 1
        if err:
            wrong.append((i, err))
    print("against libzstd: %s" % dict(classes))
    assert not wrong, wrong
    return classes


def check_verdicts(N, o, subset=None):
    """Both forms over the damaged corpus (or damaged(o)[i] for i in subset), held to libzstd's verdicts:
    1. libzstd rejects: both forms reject, with a status of REJECT;
    2. libzstd restores bytes and we report status 0: the same bytes, in both forms;
    3. both forms report the same status for every frame;
    4. libzstd restores bytes and we reject: only with E_BAD_FRAME and only where tests/zstd_inspect.py refuses the frame for a Huffman
       stream that is not consumed exactly - and every such frame is rejected.  At most half of the libzstd-accepted frames with a flip
       inside a Huffman stream may end here.
    -> the class counts."""
    D = damaged(o)
    idx = list(range(len(D))) if subset is None else list(subset)
    part = [D[i] for i in idx]
    res = decode_batches(N, [d.blob for d in part], [d.size for d in part])
    _remember(N, o, [d.blob for d in part], [d.size for d in part], res)
    classes, rule4, wrong = collections.Counter(), collections.Counter(), []
    for k, d in enumerate(part):
        sb, sc = res["block"][1][k], res["chunk"][1][k]
        if sb != sc:                                                    # rule 3
            wrong.append((idx[k], d.kind, d.how, "the forms disagree: block %d, chunk %d" % (sb, sc)))
        strict = inspector_is_strict(d.blob) if isinstance(d.verdict, bytes) else None
        for form in ("block", "chunk"):
            status, out = res[form][1][k], res[form][0][k]
            cls, err = apply_rules(d.blob, d.size, d.verdict, status, out, strict)
            if not err and strict and status == 0:                     # the strictness is kept: what RFC 8878 refuses here is not decoded
                err = "a Huffman stream is not consumed exactly, yet status 0"
            if err:
                wrong.append((idx[k], d.kind, d.how, form, err))
            if form == "chunk":
                classes[cls] += 1
                if cls == "only we reject":
                    rule4[d.kind] += 1
    streams = sum(isinstance(d.verdict, bytes) and d.kind == "Huffman streams" and "flip" in d.how for d in part)
    print("verdicts over %d damaged frames: %s" % (len(part), {c: classes[c] for c in ("both accept", "both reject", "only we reject", "only we accept")}))
    print("only we reject (a Huffman stream not consumed exactly), per kind: %s; libzstd-accepted flips in Huffman streams: %d" % (dict(rule4), streams))
    assert not wrong, wrong[:20]
    assert 2 * sum(rule4.values()) <= streams, (dict(rule4), streams)
    return classes


def remembered(N, blob, size):
    """{form: (status, CRC32C of the output)} of a frame an earlier check of this process decoded on N; None otherwise."""
    return _RESULTS.get((id(N), blob, size))


def write_corpus(path, frames):
    """[(frame, declared size)] as the file tests/emu/asan_frames.cpp reads: u32 count, then u32 size, u32 length and the bytes of each."""
    with open(path, "wb") as f:
        f.write(np.uint32(len(frames)).tobytes())
        for blob, size in frames:
            f.write(np.array([size, len(blob)], np.uint32).tobytes()); f.write(blob)
