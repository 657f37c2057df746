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
#include <string.h>

#include "records_dev.h"

size_t tsx_records_block_bytes(uint32_t n) {
    return sizeof(tsx_rec_head) + ((size_t)n + 1) * 8 + (size_t)n * 8 + (size_t)n * sizeof(tsx_rec_walk) + (((size_t)n * 4 + 63) & ~(size_t)63);
}
static_assert(sizeof(tsx_rec_head) == 64 && sizeof(tsx_rec_walk) == 40, "every part of the block begins 8-byte aligned");

tsx_rec_block tsx_records_block_at(void* base, uint32_t n) {
    tsx_rec_block b;
    b.head = (tsx_rec_head*)base;
    b.pos = (uint64_t*)(b.head + 1);
    b.off = b.pos + n + 1;
    b.walks = (tsx_rec_walk*)(b.off + n);
    b.verdicts = (int32_t*)(b.walks + n);
    return b;
}

void tsx_records_block_fill(void* h_base, const tsx_chunk_desc* descs, uint32_t n) {
    const tsx_rec_block b = tsx_records_block_at(h_base, n);
    memset(b.head, 0, sizeof *b.head);
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; i++) {
        b.pos[i] = at; b.off[i] = descs[i].src_off; at += descs[i].src_len;
        b.verdicts[i] = TSX_E_NOMEM;
        memset(&b.walks[i], 0, sizeof b.walks[i]);
    }
    b.pos[n] = at;
}

__global__ __launch_bounds__(64) void records_walk_kernel(const tsx_crc_tables* __restrict__ tab, const uint8_t* __restrict__ src, const uint64_t* __restrict__ pos,
                                                          const uint64_t* __restrict__ off, uint32_t n, tsx_rec_walk* __restrict__ walks) {
    __shared__ tsx_rec_lds L;
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    tsx_rec_view v; v.src = src; v.pos = pos; v.off = off; v.n = n; v.total = pos[n];
    const uint64_t lo = pos[k], hi = pos[k + 1];
    tsx_rec_walk w; w.entry = 0; w.exit = 0; w.bad_pos = 0; w.found = 0; w.batches = 0; w.compressed = 0; w.bad_reason = 0;
    if (hi > lo) {                                                      // (uniform)
        rec_lds_init(tab, &L, lane);
        uint64_t entry = lo;
        if (lo == 0 || rec_find_entry(tab, v, lo, hi, &L, lane, &entry)) rec_walk(tab, v, entry, hi, &L, lane, &w);
    }
    if (lane == 0) walks[k] = w;
}

__global__ __launch_bounds__(64) void records_resolve_kernel(const tsx_crc_tables* __restrict__ tab, const uint8_t* __restrict__ src, const uint64_t* __restrict__ pos,
                                                             const uint64_t* __restrict__ off, uint32_t n, const tsx_rec_walk* __restrict__ walks,
                                                             int32_t* __restrict__ verdicts, tsx_rec_head* __restrict__ head) {
    __shared__ tsx_rec_lds L;
    const uint32_t lane = threadIdx.x;
    tsx_rec_view v; v.src = src; v.pos = pos; v.off = off; v.n = n; v.total = pos[n];
    rec_lds_init(tab, &L, lane);
    uint64_t at = 0, batches = 0, compressed = 0, bad_pos = ~0ull;
    uint32_t reason = 0, repaired = 0, bad_chunk = n;
    // the walkers' results and the chunks' ends come out of pinned memory 64 chunks at a time, one load per lane: one trip over PCIe per
    // group, not one per chunk
    __shared__ tsx_rec_walk sw[64];
    __shared__ uint64_t shi[64];
    for (uint32_t k0 = 0; k0 < n && !reason; k0 += 64) {                // (uniform)
        __syncthreads();
        if (k0 + lane < n) { sw[lane] = walks[k0 + lane]; shi[lane] = pos[k0 + lane + 1]; }
        __syncthreads();
        for (uint32_t k = k0; k < n && k < k0 + 64 && !reason; k++) {
            const uint64_t hi = shi[k - k0];
            if (at >= hi) continue;                                     // an empty chunk, or one that lies inside a batch: no batch begins here
            tsx_rec_walk w = sw[k - k0];                                // (pos[k] <= at: the chunk in front was walked up to its end)
            if (!w.found || w.entry != at) { rec_walk(tab, v, at, hi, &L, lane, &w); repaired++; }
            batches += w.batches; compressed += w.compressed;
            if (w.bad_reason) { reason = w.bad_reason; bad_pos = w.bad_pos; bad_chunk = k; }
            at = w.exit;
        }
    }
    // the first invalid batch begins in chunk bad_chunk: that chunk and every chunk behind it are not delivered
    for (uint32_t i = lane; i < n; i += 64) verdicts[i] = i >= bad_chunk ? TSX_E_RECORDS : TSX_OK;
    if (lane == 0) { head->batches = batches; head->compressed = compressed; head->first_bad_pos = bad_pos; head->first_bad_reason = reason; head->repaired = repaired; }
    __threadfence_system();                                             // (every lane: the verdicts and the result before the word that says so)
    if (lane == 0) head->done = 1;
}

void tsx_launch_records(hipStream_t st, const tsx_crc_tables* d_tab, const uint8_t* src, void* hd_base, uint32_t n) {
    const tsx_rec_block b = tsx_records_block_at(hd_base, n);
    hipLaunchKernelGGL(records_walk_kernel, dim3(n), dim3(64), 0, st, d_tab, src, (const uint64_t*)b.pos, (const uint64_t*)b.off, n, b.walks);
    hipLaunchKernelGGL(records_resolve_kernel, dim3(1), dim3(64), 0, st, d_tab, src, (const uint64_t*)b.pos, (const uint64_t*)b.off, n, (const tsx_rec_walk*)b.walks, b.verdicts, b.head);
}
