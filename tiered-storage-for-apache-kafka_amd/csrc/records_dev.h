// Record-batch validation (TSX_VALIDATE_RECORDS): what one wave does with the STREAM of a batch - its chunks, concatenated in descriptor
// order - gfx950.  The stream is Kafka's log format v2: a sequence of record batches (DefaultRecordBatch.java: baseOffset @0, batchLength
// @8, partitionLeaderEpoch @12, magic @16, crc @17, attributes @21 ..., all big-endian; the CRC32C covers [21, 12 + batchLength)).
// Internal: not part of the C ABI.
//
// Every length in the stream is untrusted input.  The only way to a byte of the source is rec_seek(): it takes a position BELOW the
// call's end and yields the chunk that holds it, and every caller establishes `position < avail` (or `end <= avail`) before it asks - a
// damaged length yields a verdict, never an address.
//
// A call holds a PART of a stream (tsx_transform_batch_stream; tsx_transform_batch: all of it).  Positions here are the VIEW's: position 0
// is the first header byte carried in from the call before (chunk 0 of the view: tsx_rec_head.in.hdr, pinned memory), or the call's first
// byte when nothing is carried.  Two lengths are kept apart: `total`, the stream's declared end, decides truncation; `avail`, the call's
// end, decides what can be read.  avail <= total.
#pragma once
#include "crc_dev.h"

#define TSX_REC_HEADER 61u              /* RECORD_BATCH_OVERHEAD: the smallest batch (no records) */
#define TSX_REC_MIN_LEN 49              /* ... as its batchLength field says it (everything behind the first 12 bytes) */
#define TSX_REC_SCAN_TILE 4096u         /* bytes of a chunk a walker without an entry examines per staging step */
#define TSX_REC_SCAN_TRIES 8u           /* candidates a walker puts to the CRC before it gives up (the resolver then walks its chunk itself) */
#define TSX_REC_SCAN_MAX_LEN (1u << 20) /* ... and the longest batch it puts to the CRC, unless its own chunk is longer: a candidate is a guess, and a guess
                                           with a length of a GiB is a second of one wave's CRC (measured: 1.5 s per 1 GiB segment before this bound) */

struct tsx_rec_view {                   // the call's part of the stream, as the descriptors lay it out
    const uint8_t* src;                 // the batch's source buffer (device addressable)
    const uint8_t* carry;               // chunk 0: the carried header bytes (the view's second base: off[] names offsets in src only)
    const uint64_t* pos;                // pos[k]: position of chunk k's first byte, pos[n] = avail
    const uint64_t* off;                // off[k]: chunk k's offset in src, k >= 1
    uint32_t n;                         // chunks of the view: the call's + 1
    uint64_t total, avail;
};

struct tsx_rec_cursor { uint64_t lo, hi; const uint8_t* p; uint32_t ci; };     // chunk ci holds stream positions [lo, hi) at p

__device__ static inline void rec_cursor_reset(tsx_rec_cursor& c) { c.lo = 0; c.hi = 0; c.p = nullptr; c.ci = 0; }

// q < v.avail.  Afterwards c.lo <= q < c.hi.  The next chunk first (a walk moves forward), else the last k with pos[k] <= q by bisection:
// it is not empty, because pos[k + 1] > q.
__device__ static inline void rec_seek(const tsx_rec_view& v, tsx_rec_cursor& c, uint64_t q) {
    if (q >= c.lo && q < c.hi) return;
    uint32_t k = c.ci + 1;
    if (!(c.hi != 0 && k < v.n && v.pos[k] <= q && q < v.pos[k + 1])) {
        uint32_t a = 0, b = v.n - 1;                                    // invariant: pos[a] <= q, answer in [a, b]
        while (a < b) {
            const uint32_t m = a + (b - a + 1) / 2;
            if (v.pos[m] <= q) a = m; else b = m - 1;
        }
        k = a;
    }
    c.ci = k; c.lo = v.pos[k]; c.hi = v.pos[k + 1]; c.p = k ? v.src + v.off[k] : v.carry;
}

__device__ static inline uint8_t rec_byte(const tsx_rec_view& v, tsx_rec_cursor& c, uint64_t q) {
    rec_seek(v, c, q);
    return c.p[q - c.lo];
}

__device__ static inline uint32_t rec_be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// The CRC32C register (java.util.zip.CRC32C without the final inversion) behind positions [a, b), a <= b <= v.avail, b - a < 2^32, for a
// run that stood at `reg` in front of a - 0xFFFFFFFF where the checksum begins; by one wave, every lane calls and gets the result.  For A
// followed by B the register is the register of A moved over |B| xor the run over B: a batch open across calls continues where it stood.  cur: the wave's own (uniform) cursor - it stays where the span ended, so that a walk asks the tables (pinned memory: a read
// crosses PCIe) once per chunk it enters and not once per batch.  The span is taken apart where it crosses from one chunk to the next; of
// each part the bytes up to the first 16-byte aligned ADDRESS go to lane 63, the whole aligned pieces to the lanes in stripes of 64-byte
// lines (crc32c_wave's way: slicing-by-4 over the tables in ldsTab), the rest to lane 62.  Every run starts from remainder 0 and is moved
// to the span's end with crc_pow_bytes; so is `reg`, over the whole span.
__device__ static inline uint32_t rec_crc_reg(const tsx_crc_tables* __restrict__ tab, const tsx_rec_view& v, tsx_rec_cursor& cur, uint64_t a, uint64_t b,
                                              const uint32_t* ldsTab, uint32_t lane, uint32_t reg) {
    #define REC_CRC_W(x) { s ^= (x); s = ldsTab[3 * 256 + (s & 0xFF)] ^ ldsTab[2 * 256 + ((s >> 8) & 0xFF)] ^ ldsTab[256 + ((s >> 16) & 0xFF)] ^ ldsTab[s >> 24]; }
    #define REC_CRC_B(x) { s ^= (x); for (int k_ = 0; k_ < 8; k_++) s = crc_mulx(s); }
    uint32_t acc = 0;
    for (uint64_t q = a; q < b;) {                                      // (uniform)
        rec_seek(v, cur, q);
        const uint64_t e = b < cur.hi ? b : cur.hi;
        const uint8_t* const p = cur.p + (q - cur.lo);
        const uint32_t L = (uint32_t)(e - q);
        uint32_t head = (16u - (uint32_t)((uintptr_t)p & 15u)) & 15u;
        if (head > L) head = L;
        const uint32_t nq = (L - head) >> 4, tail = (L - head) & 15u;
        const uint32_t per = (((nq + 63) >> 6) + 3) & ~3u;
        const uint32_t p0 = min(lane * per, nq), p1 = min(p0 + per, nq);
        const uint4* in = reinterpret_cast<const uint4*>(p + head);
        uint32_t s = 0, i = p0;
        for (; i + 4 <= p1; i += 4) {
            const uint4 w0 = in[i], w1 = in[i + 1], w2 = in[i + 2], w3 = in[i + 3];
            REC_CRC_W(w0.x) REC_CRC_W(w0.y) REC_CRC_W(w0.z) REC_CRC_W(w0.w)
            REC_CRC_W(w1.x) REC_CRC_W(w1.y) REC_CRC_W(w1.z) REC_CRC_W(w1.w)
            REC_CRC_W(w2.x) REC_CRC_W(w2.y) REC_CRC_W(w2.z) REC_CRC_W(w2.w)
            REC_CRC_W(w3.x) REC_CRC_W(w3.y) REC_CRC_W(w3.z) REC_CRC_W(w3.w)
        }
        for (; i < p1; i++) {
            const uint4 w = in[i];
            REC_CRC_W(w.x) REC_CRC_W(w.y) REC_CRC_W(w.z) REC_CRC_W(w.w)
        }
        if (p1 > p0) acc ^= crc_mulmod(s, crc_pow_bytes(tab, (b - e) + tail + ((uint64_t)(nq - p1) << 4)));
        if (lane == 63 && head) {
            s = 0;
            for (uint32_t k = 0; k < head; k++) REC_CRC_B(p[k])
            acc ^= crc_mulmod(s, crc_pow_bytes(tab, (b - q) - head));
        }
        if (lane == 62 && tail) {
            const uint8_t* t = p + head + ((size_t)nq << 4);
            s = 0;
            for (uint32_t k = 0; k < tail; k++) REC_CRC_B(t[k])
            acc ^= crc_mulmod(s, crc_pow_bytes(tab, b - e));
        }
        q = e;
    }
    #undef REC_CRC_W
    #undef REC_CRC_B
    for (int o = 32; o; o >>= 1) acc ^= __shfl_xor(acc, o);
    return acc ^ crc_mulmod(reg, crc_pow_bytes(tab, b - a));
}
// ... and the checksum of a span that holds all of its bytes
__device__ static inline uint32_t rec_crc(const tsx_crc_tables* __restrict__ tab, const tsx_rec_view& v, tsx_rec_cursor& cur, uint64_t a, uint64_t b,
                                          const uint32_t* ldsTab, uint32_t lane) {
    return ~rec_crc_reg(tab, v, cur, a, b, ldsTab, lane, 0xFFFFFFFFu);
}

// FRAMES (TSX_VALIDATE_FRAMES): the tile also stages the records of the batch under examination, and is 640 bytes longer - with them the
// LDS of both frames kernels is a whole number of 1280-byte allocation granules (walker 7, resolver 11).
#define TSX_REC_FRAMES_MORE 640u
template <bool FRAMES> struct tsx_rec_lds_t {
    uint32_t tab[4 * 256];                                              // slicing tables 0..3 of tsx_crc_tables
    uint8_t hdr[64];                                                    // the header of the batch under examination
    uint8_t tile[TSX_REC_SCAN_TILE + 64 + (FRAMES ? TSX_REC_FRAMES_MORE : 0u)];   // a walker without an entry: the bytes it looks for one in
};
typedef tsx_rec_lds_t<false> tsx_rec_lds;

template <class LDS>
__device__ static inline void rec_lds_init(const tsx_crc_tables* __restrict__ tab, LDS* L, uint32_t lane) {
    const uint4* g = reinterpret_cast<const uint4*>(&tab->slice[0][0]);
    uint4* l = reinterpret_cast<uint4*>(L->tab);
    for (uint32_t i = lane; i < 4 * 256 / 4; i += 64) l[i] = g[i];
    __syncthreads();
}

// ---- TSX_VALIDATE_FRAMES: the records of one batch --------------------------------------------------------------------------------------
// A reader of the record region: a staged tile in LDS (stream positions [tb, tb + cnt)), and rec_byte() for whatever lies outside it - a
// varint behind a key or value longer than the tile.  Every caller establishes `q < lim <= end <= avail` before it asks.
struct tsx_rec_reader { tsx_rec_cursor cur; const uint8_t* tile; uint64_t tb; uint32_t cnt; };

__device__ static inline uint32_t rec_rd(const tsx_rec_view& v, tsx_rec_reader& r, uint64_t q) {
    const uint64_t d = q - r.tb;                                        // (q < tb wraps: not in the tile)
    return d < r.cnt ? r.tile[d] : rec_byte(v, r.cur, q);
}

// ByteUtils.readVarint: zigzag, at most 5 bytes, a continuation bit on the 5th is malformed, the 5th byte's excess bits fall off the int.
// false: malformed, or it would leave [q, lim).  q moves behind it.
__device__ static inline bool rec_varint(const tsx_rec_view& v, tsx_rec_reader& r, uint64_t& q, uint64_t lim, int32_t* out) {
    uint32_t val = 0;
    for (uint32_t i = 0; i < 5; i++) {
        if (q >= lim) return false;
        const uint32_t b = rec_rd(v, r, q++);
        val |= (b & 0x7Fu) << (7 * i);
        if (!(b & 0x80u)) { *out = (int32_t)(val >> 1) ^ -(int32_t)(val & 1u); return true; }
    }
    return false;
}
// ByteUtils.readVarlong: at most 10 bytes; its value (a timestamp delta) is not looked at
__device__ static inline bool rec_varlong_skip(const tsx_rec_view& v, tsx_rec_reader& r, uint64_t& q, uint64_t lim) {
    for (uint32_t i = 0; i < 10; i++) {
        if (q >= lim) return false;
        if (!(rec_rd(v, r, q++) & 0x80u)) return true;
    }
    return false;
}
// a length varint >= min_len and, when positive, that many bytes inside [q, lim)
__device__ static inline bool rec_sized(const tsx_rec_view& v, tsx_rec_reader& r, uint64_t& q, uint64_t lim, int32_t min_len) {
    int32_t n;
    if (!rec_varint(v, r, q, lim, &n) || n < min_len) return false;
    if (n > 0) { if ((uint64_t)n > lim - q) return false; q += (uint64_t)n; }
    return true;
}

// One record's fields behind its length, body [b, e), e <= end: DefaultRecord.readFrom's order.  Returns the reason of the first field
// that fails (0: none).  *delta, *have: the record's offsetDelta, once it has been read (its order against the record in front is the
// caller's to check, and outranks what this returns when it fails: the offsetDelta stands in front of the key).
__device__ static inline uint32_t rec_record_fields(const tsx_rec_view& v, tsx_rec_reader& r, uint64_t b, uint64_t e, int32_t last_delta, int32_t* delta, bool* have) {
    uint64_t q = b;
    if (q >= e) return TSX_REC_RECORDS;                                 // attributes
    q++;
    if (!rec_varlong_skip(v, r, q, e)) return TSX_REC_RECORDS;          // timestampDelta
    int32_t d;
    if (!rec_varint(v, r, q, e, &d)) return TSX_REC_RECORDS;            // offsetDelta
    *delta = d; *have = true;
    if (d < 0 || d > last_delta) return TSX_REC_OFFSETS;
    if (!rec_sized(v, r, q, e, -1)) return TSX_REC_RECORDS;             // key
    if (!rec_sized(v, r, q, e, -1)) return TSX_REC_RECORDS;             // value
    int32_t nh;
    if (!rec_varint(v, r, q, e, &nh) || nh < 0) return TSX_REC_RECORDS; // headers: every one takes two bytes or more, the body bounds the loop
    for (int32_t h = 0; h < nh; h++)
        if (!rec_sized(v, r, q, e, 0) || !rec_sized(v, r, q, e, -1)) return TSX_REC_RECORDS;
    return q == e ? 0u : TSX_REC_RECORDS;
}

// The records of one uncompressed batch whose CRC has passed: exactly `count` (>= 0) records in [from, end), end <= avail; the whole wave
// calls and gets the reason (0, TSX_REC_RECORDS, TSX_REC_OFFSETS) of the lowest-numbered record that fails.  Trip by trip: the region from
// the next record on is staged into the tile (coalesced), every lane follows the chain of length varints through it - the same LDS words
// for all, one dependent hop per record, up to 64 records that BEGIN in the tile - and keeps the bounds of record `lane`; then each lane
// reads its record's fields.  A record that reaches beyond the tile is read through rec_byte() where it must be (its varints), and its key
// and value are stepped over by arithmetic.
template <class LDS>
__device__ static inline uint32_t rec_frames_records(const tsx_rec_view& v, uint64_t from, uint64_t end, int32_t count, int32_t last_delta, LDS* L, uint32_t lane) {
    tsx_rec_reader r;
    rec_cursor_reset(r.cur); r.tile = L->tile; r.tb = 0; r.cnt = 0;
    uint64_t q = from;
    int32_t prev = -1;
    for (uint32_t done = 0; done < (uint32_t)count;) {                  // (uniform)
        const uint64_t left = end - q;
        const uint32_t cnt = left < sizeof L->tile ? (uint32_t)left : (uint32_t)sizeof L->tile;
        __syncthreads();                                                // (the last trip's readers of the tile are done)
        for (uint32_t i = lane; i < cnt; i += 64) L->tile[i] = rec_byte(v, r.cur, q + i);
        __syncthreads();
        r.tb = q; r.cnt = cnt;
        const uint32_t want = (uint32_t)count - done < 64u ? (uint32_t)count - done : 64u;
        uint32_t m = 0;
        bool chain_bad = false;
        uint64_t s = q, my_b = 0, my_e = 0;
        while (m < want) {
            if (s >= end) { chain_bad = true; break; }                  // more records counted than the batch holds
            if (s - q >= cnt) break;                                    // the next record begins behind the tile (m >= 1: s == q is inside it)
            uint64_t t = s;
            int32_t len;
            if (!rec_varint(v, r, t, end, &len) || len < 0 || (uint64_t)len > end - t) { chain_bad = true; break; }
            if (m == lane) { my_b = t; my_e = t + (uint64_t)len; }
            s = t + (uint64_t)len; m++;
        }
        uint32_t why = 0;
        int32_t d = 0;
        bool have = false;
        if (lane < m) why = rec_record_fields(v, r, my_b, my_e, last_delta, &d, &have);
        int32_t pd = __shfl_up(d, 1);
        uint32_t ph = __shfl_up((uint32_t)have, 1);
        if (lane == 0) { pd = prev; ph = 1; }
        if (lane < m && have && ph && d <= pd) why = TSX_REC_OFFSETS;   // (a record in front without a delta has failed, and decides)
        uint32_t key = why ? lane << 3 | why : 0xFFFFFFFFu;
        if (chain_bad && lane == m) key = m << 3 | TSX_REC_RECORDS;     // (m < 64)
        for (int o = 32; o; o >>= 1) { const uint32_t x = __shfl_xor(key, o); key = x < key ? x : key; }
        if (key != 0xFFFFFFFFu) return key & 7u;
        prev = __shfl(d, (int)m - 1);
        done += m; q = s;
    }
    return q == end ? 0u : TSX_REC_RECORDS;                             // a count too small leaves bytes over
}

__device__ static inline int64_t rec_be64s(const uint8_t* p) { return (int64_t)((uint64_t)rec_be32(p) << 32 | rec_be32(p + 4)); }

// The checks of TSX_VALIDATE_FRAMES on a batch at `pos` whose CRC has passed and whose header is in L->hdr; the whole wave calls.  have_prev,
// prev_last: baseOffset + lastOffsetDelta of the valid batch in front, when the caller knows it.  Returns the reason (0: valid) and the
// header's baseOffset, last offset and recordsCount.
template <class LDS>
__device__ static inline uint32_t rec_frames_batch(const tsx_rec_view& v, uint64_t pos, uint64_t end, bool comp, bool have_prev, int64_t prev_last,
                                                   LDS* L, uint32_t lane, int64_t* base_out, int64_t* last_out, int32_t* count_out) {
    const int64_t base = rec_be64s(L->hdr);
    const int32_t last_delta = (int32_t)rec_be32(L->hdr + 23), count = (int32_t)rec_be32(L->hdr + 57);
    *base_out = base; *count_out = count; *last_out = 0;
    if (base < 0 || last_delta < 0 || base > INT64_MAX - (int64_t)last_delta || (have_prev && base <= prev_last)) return TSX_REC_OFFSETS;
    *last_out = base + (int64_t)last_delta;
    if (count < 0) return TSX_REC_RECORDS;
    if (comp) return 0;                                                 // a compressed batch's records cannot be read
    return rec_frames_records(v, pos + TSX_REC_HEADER, end, count, last_delta, L, lane);
}

// The serial walk from `start` (a batch boundary, start <= stop <= avail) over every batch that begins below `stop`; the whole wave
// calls.  For each batch, in DefaultRecordBatch.ensureValid()'s order: at least a header left, batchLength >= 49 (signed), the batch
// inside the stream - both against `total` - magic 2, CRC.  w->exit is where the first batch at or behind `stop` begins.  A batch whose 61
// header bytes, or whose end, lie behind the call's end cannot be judged here: the walk ends at it (TSX_REC_WALK_PENDING, w->exit) and the
// resolver carries it into the next call.  The next header's bytes are asked for before the CRC of this batch runs: the load's latency
// passes under it - when the call holds all 61 of them.
// FRAMES (TSX_VALIDATE_FRAMES): a batch whose CRC has passed is then examined by rec_frames_batch, and counts only if that passes too.  f:
// the walk's further results; have_prev, prev_last: the last offset of the valid batch in front of `start`, when the caller knows it (the
// resolver does; a walker does not, and leaves the seam to the resolver: f->has_first, f->first_base).
template <bool FRAMES, class LDS>
__device__ static inline void rec_walk(const tsx_crc_tables* __restrict__ tab, const tsx_rec_view& v, uint64_t start, uint64_t stop,
                                       LDS* L, uint32_t lane, tsx_rec_walk* w, tsx_rec_walk_frames* f = nullptr, bool have_prev = false, int64_t prev_last = 0) {
    tsx_rec_cursor cur, ccur;                                           // the lanes' own (header bytes) and the wave's (CRC spans)
    rec_cursor_reset(cur); rec_cursor_reset(ccur);
    w->found = TSX_REC_WALK_FOUND; w->entry = start; w->batches = 0; w->compressed = 0; w->bad_reason = 0; w->bad_pos = 0;
    if (FRAMES) { f->records = 0; f->first_base = 0; f->last = 0; f->has_first = 0; f->pad_ = 0; }
    uint64_t pos = start;
    bool have = false;
    uint8_t nb = 0;
    while (pos < stop) {
        uint32_t why = 0;
        if (v.total - pos < TSX_REC_HEADER) why = TSX_REC_TRUNCATED;
        else if (v.avail - pos < TSX_REC_HEADER) { w->found |= TSX_REC_WALK_PENDING; break; }
        else {
            if (!have && lane < TSX_REC_HEADER) nb = rec_byte(v, cur, pos + lane);
            __syncthreads();                                            // (the last batch's readers of hdr are done)
            if (lane < TSX_REC_HEADER) L->hdr[lane] = nb;
            __syncthreads();
            have = false;
            const int32_t len = (int32_t)rec_be32(L->hdr + 8);
            const uint64_t left = v.total - pos - 12;
            if (len < TSX_REC_MIN_LEN) why = TSX_REC_LENGTH;
            else if ((uint64_t)len > left) why = TSX_REC_TRUNCATED;
            else if (L->hdr[16] != 2) why = TSX_REC_MAGIC;
            else {
                const uint32_t want = rec_be32(L->hdr + 17);
                const uint32_t comp = (L->hdr[22] & 7u) != 0;
                const uint64_t end = pos + 12 + (uint64_t)len;
                if (end > v.avail) { w->found |= TSX_REC_WALK_PENDING; break; }
                if (end < stop && v.avail - end >= TSX_REC_HEADER) { if (lane < TSX_REC_HEADER) nb = rec_byte(v, cur, end + lane); have = true; }
                if (rec_crc(tab, v, ccur, pos + 21, end, L->tab, lane) != want) why = TSX_REC_CRC;
                else if (FRAMES) {
                    int64_t base, last;
                    int32_t count;
                    why = rec_frames_batch(v, pos, end, comp != 0, have_prev, prev_last, L, lane, &base, &last, &count);
                    if (!f->has_first) { f->has_first = 1; f->first_base = base; }
                    if (!why) {
                        w->batches++; w->compressed += comp; pos = end;
                        if (!comp) f->records += (uint32_t)count;
                        have_prev = true; prev_last = last; f->last = last;
                    }
                }
                else { w->batches++; w->compressed += comp; pos = end; }
            }
        }
        if (why) { w->bad_reason = why; w->bad_pos = pos; break; }
    }
    w->exit = pos;
}

// A walker that does not know where its chunk's first batch begins: from stream positions [lo, hi) the first one that looks like a header
// (magic 2, a length that is at least a header's, ends inside the call - a candidate whose end lies behind it cannot be confirmed and is
// skipped - and is no longer than TSX_REC_SCAN_MAX_LEN or the chunk, attribute bits 7..15 zero) AND whose CRC confirms.  Returns false when there is none among the first TSX_REC_SCAN_TRIES that look like
// one: a chunk wholly inside a batch, a batch longer than the bound, or a hostile chunk - the resolver walks such a chunk itself.
template <class LDS>
__device__ static inline bool rec_find_entry(const tsx_crc_tables* __restrict__ tab, const tsx_rec_view& v, uint64_t lo, uint64_t hi,
                                             LDS* L, uint32_t lane, uint64_t* entry) {
    tsx_rec_cursor cur, ccur;
    rec_cursor_reset(cur); rec_cursor_reset(ccur);
    uint32_t tries = 0;
    const uint64_t max_len = hi - lo > TSX_REC_SCAN_MAX_LEN ? hi - lo : TSX_REC_SCAN_MAX_LEN;
    for (uint64_t base = lo; base < hi; base += TSX_REC_SCAN_TILE) {
        const uint64_t avail = v.avail - base;
        const uint32_t cnt = avail < TSX_REC_SCAN_TILE + 64 ? (uint32_t)avail : TSX_REC_SCAN_TILE + 64;
        const uint32_t lim = hi - base < TSX_REC_SCAN_TILE ? (uint32_t)(hi - base) : TSX_REC_SCAN_TILE;
        __syncthreads();
        for (uint32_t i = lane; i < cnt; i += 64) L->tile[i] = rec_byte(v, cur, base + i);
        __syncthreads();
        for (uint32_t from = 0; from < lim;) {
            uint32_t best = 0xFFFFFFFFu;
            for (uint32_t i = (from & ~63u) + lane; i < lim && i + TSX_REC_HEADER <= cnt; i += 64) {
                if (i < from) continue;
                const uint8_t* h = L->tile + i;
                if (h[16] != 2 || h[21] != 0 || (h[22] & 0x80)) continue;
                const int32_t len = (int32_t)rec_be32(h + 8);
                if (len < TSX_REC_MIN_LEN || (uint64_t)len > v.avail - (base + i) - 12 || (uint64_t)len > max_len) continue;
                best = i;
                break;
            }
            for (int o = 32; o; o >>= 1) { const uint32_t x = __shfl_xor(best, o); best = x < best ? x : best; }
            if (best == 0xFFFFFFFFu) break;
            const uint64_t p = base + best;
            const uint64_t end = p + 12 + (uint64_t)rec_be32(L->tile + best + 8);
            if (rec_crc(tab, v, ccur, p + 21, end, L->tab, lane) == rec_be32(L->tile + best + 17)) { *entry = p; return true; }
            if (++tries >= TSX_REC_SCAN_TRIES) return false;
            from = best + 1;
        }
    }
    return false;
}
