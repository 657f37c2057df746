// Record-batch validation (TSX_VALIDATE_RECORDS) - gfx950.
//
// The chunks of a transform batch, concatenated in descriptor order, are ONE stream of Kafka v2 record batches; every batch of it is
// checked the way DefaultRecordBatch.ensureValid() plus a walk over the log would (records_dev.h), and the first invalid one decides
// (include/tsxform.h).  The walk `pos += 12 + batchLength` is a chain of dependent loads, one per batch - millions for a segment of
// small batches - so it is not made once, but once per chunk, side by side:
//   records_walk_kernel     one wave per chunk.  Walker k owns the batches that BEGIN in chunk k and follows them to their end, wherever
//                           that lies.  Walker 0 enters at position 0; walker k > 0 does not know its entry and takes the first position
//                           of its chunk that looks like a header and whose CRC confirms (rec_find_entry).
//   records_resolve_kernel  one wave per call.  Chains the walkers from position 0: walker k's result counts only if the chain arrives
//                           exactly at its entry; otherwise the resolver walks that chunk's batches itself, from the true position, with
//                           the same device function (repaired_chunks).  A CRC-valid batch inside a record value, a damaged first batch the
//                           scan skipped, a hostile chunk: speculation loses and the result is still the serial walk's.
// A call may hold a PART of a stream (tsx_transform_batch_stream; records_dev.h has the view).  The resolver then first closes the batch
// that was open on entry - its CRC register continued over the call's bytes - chains the walkers from that batch's end instead of 0, and
// at the call's end writes what the next call needs into the block's head: the raw bytes of a header that has not all arrived, or the open
// batch's fields and register.  A whole stream in one call is the case in which nothing comes in and nothing goes out.
// TSX_VALIDATE_FRAMES: both kernel bodies are templates on `bool FRAMES`.  records_walk_kernel / records_resolve_kernel are the <false>
// instances - what they always were.  records_walk_frames_kernel / records_resolve_frames_kernel, the <true> ones, examine every batch
// that has passed its CRC further (records_dev.h: rec_frames_batch - offsets, count, the framing of the records); a walker does not know
// the batch in front of its first one, so its result (tsx_rec_walk_frames) carries that batch's baseOffset and its own last offset, and
// the resolver checks the seam when it accepts the result.  One call only: the streamed form refuses the flag.
#include <string.h>

#include "records_dev.h"

size_t tsx_records_block_bytes(uint32_t n, bool frames) {
    n++;                                                                // (the view's chunks)
    return sizeof(tsx_rec_head) + ((size_t)n + 1) * 8 + (size_t)n * 8 + (size_t)n * (frames ? sizeof(tsx_rec_walk_frames) : sizeof(tsx_rec_walk)) +
           (((size_t)n * 4 + 63) & ~(size_t)63);
}
static_assert(sizeof(tsx_rec_head) == 64 + 2 * 112 && sizeof(tsx_rec_carry) == 112 && sizeof(tsx_rec_walk) == 40, "every part of the block begins 8-byte aligned");
static_assert(sizeof(tsx_rec_walk_frames) == 72, "... with TSX_VALIDATE_FRAMES too");

tsx_rec_block tsx_records_block_at(void* base, uint32_t n, bool frames) {
    tsx_rec_block b;
    n++;
    b.head = (tsx_rec_head*)base;
    b.pos = (uint64_t*)(b.head + 1);
    b.off = b.pos + n + 1;
    b.walks = frames ? nullptr : (tsx_rec_walk*)(b.off + n);
    b.fwalks = frames ? (tsx_rec_walk_frames*)(b.off + n) : nullptr;
    b.verdicts = frames ? (int32_t*)(b.fwalks + n) : (int32_t*)(b.walks + n);
    return b;
}

void tsx_records_block_fill(void* h_base, const tsx_chunk_desc* descs, uint32_t n, uint32_t hdr_n, bool frames) {
    const tsx_rec_block b = tsx_records_block_at(h_base, n, frames);
    memset(b.head, 0, sizeof *b.head);
    uint64_t at = hdr_n;
    b.pos[0] = 0; b.off[0] = 0;
    for (uint32_t i = 0; i < n; i++) { b.pos[i + 1] = at; b.off[i + 1] = descs[i].src_off; at += descs[i].src_len; }
    b.pos[n + 1] = at;
    for (uint32_t i = 0; i <= n; i++) {
        b.verdicts[i] = TSX_E_NOMEM;
        if (frames) memset(&b.fwalks[i], 0, sizeof b.fwalks[i]); else memset(&b.walks[i], 0, sizeof b.walks[i]);
    }
}

// what a kernel of either kind says "walker's result" to, and the 40 bytes both kinds have
template <bool FRAMES> struct rec_walk_of { typedef tsx_rec_walk type; };
template <> struct rec_walk_of<true> { typedef tsx_rec_walk_frames type; };
__device__ static inline tsx_rec_walk* rec_walk_base(tsx_rec_walk* w) { return w; }
__device__ static inline tsx_rec_walk* rec_walk_base(tsx_rec_walk_frames* w) { return &w->w; }
__device__ static inline tsx_rec_walk_frames* rec_walk_more(tsx_rec_walk*) { return nullptr; }
__device__ static inline tsx_rec_walk_frames* rec_walk_more(tsx_rec_walk_frames* w) { return w; }

template <bool FRAMES>
__device__ static __forceinline__ void records_walk_body(const tsx_crc_tables* __restrict__ tab, const uint8_t* __restrict__ src, const uint64_t* __restrict__ pos,
                                                         const uint64_t* __restrict__ off, uint32_t n, typename rec_walk_of<FRAMES>::type* __restrict__ walks,
                                                         const uint8_t* __restrict__ carry, uint64_t total, uint64_t start) {
    __shared__ tsx_rec_lds_t<FRAMES> L;
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    tsx_rec_view v; v.src = src; v.carry = carry; v.pos = pos; v.off = off; v.n = n; v.total = total; v.avail = pos[n];
    const uint64_t lo = pos[k], hi = pos[k + 1];
    typename rec_walk_of<FRAMES>::type wk;
    tsx_rec_walk& w = *rec_walk_base(&wk);
    w.entry = 0; w.exit = 0; w.bad_pos = 0; w.found = 0; w.batches = 0; w.compressed = 0; w.bad_reason = 0;
    if (FRAMES) { tsx_rec_walk_frames* f = rec_walk_more(&wk); f->records = 0; f->first_base = 0; f->last = 0; f->has_first = 0; f->pad_ = 0; }
    // `start` is the one position known to be a batch boundary (0, or the end of the batch that was open on entry): the walker of the chunk
    // that holds it enters there, the walkers behind it guess, and a chunk in front of it lies inside the open batch - nothing begins there
    if (hi > lo && hi > start) {                                        // (uniform)
        rec_lds_init(tab, &L, lane);
        uint64_t entry = start;
        if (lo <= start || rec_find_entry(tab, v, lo, hi, &L, lane, &entry)) rec_walk<FRAMES>(tab, v, entry, hi, &L, lane, &w, rec_walk_more(&wk));
    }
    if (lane == 0) walks[k] = wk;
}

__global__ __launch_bounds__(64) void records_walk_kernel(const tsx_crc_tables* __restrict__ tab, const uint8_t* __restrict__ src, const uint64_t* __restrict__ pos,
                                                          const uint64_t* __restrict__ off, uint32_t n, tsx_rec_walk* __restrict__ walks,
                                                          const uint8_t* __restrict__ carry, uint64_t total, uint64_t start) {
    records_walk_body<false>(tab, src, pos, off, n, walks, carry, total, start);
}
// TSX_VALIDATE_FRAMES: the same walk, and behind each batch's CRC its offsets, its count and its records (records_dev.h: rec_frames_batch)
__global__ __launch_bounds__(64) void records_walk_frames_kernel(const tsx_crc_tables* __restrict__ tab, const uint8_t* __restrict__ src, const uint64_t* __restrict__ pos,
                                                                 const uint64_t* __restrict__ off, uint32_t n, tsx_rec_walk_frames* __restrict__ walks,
                                                                 const uint8_t* __restrict__ carry, uint64_t total, uint64_t start) {
    records_walk_body<true>(tab, src, pos, off, n, walks, carry, total, start);
}

template <bool FRAMES>
__device__ static __forceinline__ void records_resolve_body(const tsx_crc_tables* __restrict__ tab, const uint8_t* __restrict__ src, const uint64_t* __restrict__ pos,
                                                            const uint64_t* __restrict__ off, uint32_t n, const typename rec_walk_of<FRAMES>::type* __restrict__ walks,
                                                            int32_t* __restrict__ verdicts, tsx_rec_head* __restrict__ head, uint64_t total, uint64_t start) {
    typedef typename rec_walk_of<FRAMES>::type walk_t;
    __shared__ tsx_rec_lds_t<FRAMES> L;
    const uint32_t lane = threadIdx.x;
    tsx_rec_view v; v.src = src; v.carry = head->in.hdr; v.pos = pos; v.off = off; v.n = n; v.total = total; v.avail = pos[n];
    rec_lds_init(tab, &L, lane);
    uint64_t at = start, batches = 0, compressed = 0, bad_pos = ~0ull;
    uint32_t reason = 0, repaired = 0, bad_open = 0;
    bool pending = false;
    // TSX_VALIDATE_FRAMES: the records read, and the last offset of the chain's last valid batch (the first batch of a stream has none in front)
    uint64_t records = 0;
    int64_t last = 0;
    bool have_last = false;
    tsx_rec_cursor cur, ccur;                                           // the lanes' own (header bytes) and the wave's (CRC spans)
    rec_cursor_reset(cur); rec_cursor_reset(ccur);
    // ---- the batch that was open on entry: its register runs on over the call's bytes up to its end; a tail longer than the whole call
    // only advances the register, and every chunk passes ----
    const uint32_t in_open = head->in.open, in_want = head->in.want, in_comp = head->in.comp;
    uint32_t open_reg = head->in.reg;
    if (in_open) {                                                      // (uniform)
        open_reg = rec_crc_reg(tab, v, ccur, 0, start < v.avail ? start : v.avail, L.tab, lane, open_reg);
        if (start > v.avail) pending = true;
        else if (~open_reg != in_want) { reason = TSX_REC_CRC; bad_pos = 0; bad_open = 1; }
        else { batches++; compressed += in_comp; }
    }
    // the walkers' results and the chunks' ends come out of pinned memory 64 chunks at a time, one load per lane: one trip over PCIe per
    // group, not one per chunk
    __shared__ walk_t sw[64];
    __shared__ uint64_t shi[64];
    for (uint32_t k0 = 0; k0 < n && !reason && !pending; k0 += 64) {    // (uniform)
        __syncthreads();
        if (k0 + lane < n) { sw[lane] = walks[k0 + lane]; shi[lane] = pos[k0 + lane + 1]; }
        __syncthreads();
        for (uint32_t k = k0; k < n && k < k0 + 64 && !reason && !pending; k++) {
            const uint64_t hi = shi[k - k0];
            if (at >= hi) continue;                                     // an empty chunk, or one that lies inside a batch: no batch begins here
            walk_t wk = sw[k - k0];                                     // (pos[k] <= at: the chunk in front was walked up to its end)
            tsx_rec_walk& w = *rec_walk_base(&wk);
            if (!w.found || w.entry != at) { rec_walk<FRAMES>(tab, v, at, hi, &L, lane, &w, rec_walk_more(&wk), have_last, last); repaired++; }
            else if (FRAMES) {
                // the seam: the walker did not know the batch in front of its first one.  Its place is that of the batch's own offsets
                // check: behind the CRC (has_first says it passed), in front of the count and the records - whatever else the walker
                // found in or behind that batch does not count
                tsx_rec_walk_frames* f = rec_walk_more(&wk);
                if (f->has_first && have_last && f->first_base <= last) {
                    w.batches = 0; w.compressed = 0; f->records = 0; w.bad_reason = TSX_REC_OFFSETS; w.bad_pos = w.entry; w.exit = w.entry;
                    w.found = TSX_REC_WALK_FOUND;
                }
            }
            if (FRAMES) { tsx_rec_walk_frames* f = rec_walk_more(&wk); records += f->records; if (w.batches) { have_last = true; last = f->last; } }
            batches += w.batches; compressed += w.compressed;
            if (w.bad_reason) { reason = w.bad_reason; bad_pos = w.bad_pos; }
            pending = (w.found & TSX_REC_WALK_PENDING) != 0;
            at = w.exit;
        }
    }
    // ---- what the next call needs: the batch at `at` has not all arrived (its walk has judged what it could) ----
    tsx_rec_carry out;
    out.open_pos = 0; out.open_end = 0; out.open = 0; out.want = 0; out.reg = 0; out.comp = 0; out.hdr_n = 0;
    if (!reason && pending) {                                           // (uniform)
        if (in_open && start > v.avail) { out.open = 1; out.open_end = start; out.want = in_want; out.reg = open_reg; out.comp = in_comp; }
        else if (v.avail - at < TSX_REC_HEADER) {
            out.hdr_n = (uint32_t)(v.avail - at);
            if (lane < out.hdr_n) head->out.hdr[lane] = rec_byte(v, cur, at + lane);
        } else {
            uint8_t nb = 0;
            if (lane < TSX_REC_HEADER) nb = rec_byte(v, cur, at + lane);
            __syncthreads();
            if (lane < TSX_REC_HEADER) L.hdr[lane] = nb;
            __syncthreads();
            out.open = 1; out.open_pos = at; out.open_end = at + 12 + (uint64_t)rec_be32(L.hdr + 8);
            out.want = rec_be32(L.hdr + 17); out.comp = (L.hdr[22] & 7u) != 0;
            out.reg = rec_crc_reg(tab, v, ccur, at + 21, v.avail, L.tab, lane, 0xFFFFFFFFu);
        }
    }
    // the chunk that holds the first invalid batch's first byte - or the call's first byte, when the batch began in a call before - and
    // every chunk behind it are not delivered
    uint32_t bad_chunk = n;
    if (reason) {                                                       // (uniform; the verdict needed a byte of this call at or behind that position)
        const uint64_t first = pos[1];
        rec_seek(v, cur, bad_pos > first ? bad_pos : first);
        bad_chunk = cur.ci;
    }
    for (uint32_t i = lane; i < n; i += 64) verdicts[i] = i >= bad_chunk ? TSX_E_RECORDS : TSX_OK;
    if (lane == 0) {
        if (FRAMES) head->records = records;
        head->batches = batches; head->compressed = compressed; head->first_bad_pos = bad_pos; head->first_bad_reason = reason; head->repaired = repaired; head->bad_open = bad_open;
        head->out.open_pos = out.open_pos; head->out.open_end = out.open_end; head->out.open = out.open; head->out.want = out.want; head->out.reg = out.reg;
        head->out.comp = out.comp; head->out.hdr_n = out.hdr_n;
    }
    __threadfence_system();                                             // (every lane: the verdicts and the result before the word that says so)
    if (lane == 0) head->done = 1;
}

__global__ __launch_bounds__(64) void records_resolve_kernel(const tsx_crc_tables* __restrict__ tab, const uint8_t* __restrict__ src, const uint64_t* __restrict__ pos,
                                                             const uint64_t* __restrict__ off, uint32_t n, const tsx_rec_walk* __restrict__ walks,
                                                             int32_t* __restrict__ verdicts, tsx_rec_head* __restrict__ head, uint64_t total, uint64_t start) {
    records_resolve_body<false>(tab, src, pos, off, n, walks, verdicts, head, total, start);
}
// TSX_VALIDATE_FRAMES: the same chain, the order of offsets across every seam, and repairs that examine the records too
__global__ __launch_bounds__(64) void records_resolve_frames_kernel(const tsx_crc_tables* __restrict__ tab, const uint8_t* __restrict__ src, const uint64_t* __restrict__ pos,
                                                                    const uint64_t* __restrict__ off, uint32_t n, const tsx_rec_walk_frames* __restrict__ walks,
                                                                    int32_t* __restrict__ verdicts, tsx_rec_head* __restrict__ head, uint64_t total, uint64_t start) {
    records_resolve_body<true>(tab, src, pos, off, n, walks, verdicts, head, total, start);
}

void tsx_launch_records(hipStream_t st, const tsx_crc_tables* d_tab, const uint8_t* src, void* hd_base, uint32_t n, uint64_t total, uint64_t start, bool frames) {
    const tsx_rec_block b = tsx_records_block_at(hd_base, n, frames);
    const uint32_t nv = n + 1;
    if (frames) {
        hipLaunchKernelGGL(records_walk_frames_kernel, dim3(nv), dim3(64), 0, st, d_tab, src, (const uint64_t*)b.pos, (const uint64_t*)b.off, nv, b.fwalks, (const uint8_t*)b.head->in.hdr, total, start);
        hipLaunchKernelGGL(records_resolve_frames_kernel, dim3(1), dim3(64), 0, st, d_tab, src, (const uint64_t*)b.pos, (const uint64_t*)b.off, nv, (const tsx_rec_walk_frames*)b.fwalks, b.verdicts, b.head, total, start);
        return;
    }
    hipLaunchKernelGGL(records_walk_kernel, dim3(nv), dim3(64), 0, st, d_tab, src, (const uint64_t*)b.pos, (const uint64_t*)b.off, nv, b.walks, (const uint8_t*)b.head->in.hdr, total, start);
    hipLaunchKernelGGL(records_resolve_kernel, dim3(1), dim3(64), 0, st, d_tab, src, (const uint64_t*)b.pos, (const uint64_t*)b.off, nv, (const tsx_rec_walk*)b.walks, b.verdicts, b.head, total, start);
}
