// Zstandard frame decoder — gfx950, one workgroup of three 64-lane wavefronts per chunk.
//
// Replaces zstd-jni's  Zstd.decompressedSize(chunk) / Zstd.decompress(chunk, size)
//   core/src/main/java/io/aiven/kafka/tieredstorage/transform/DecompressionChunkEnumeration.java:39-46
// and accepts any single Zstandard frame (RFC 8878) with a known content size and no dictionary — not only
// the frames our own compressor writes: raw / RLE / compressed blocks, raw / RLE / Huffman (1 or 4 streams,
// treeless) literals, predefined / RLE / FSE / repeat sequence tables, repeat offsets.
// Errors are per chunk: TSX_E_BAD_SIZE when the frame declares no usable content size (the reference throws
// "Invalid decompressed size"), TSX_E_DST_TOO_SMALL, TSX_E_BAD_FRAME for anything malformed.  A content
// checksum, when present, is verified against the restored bytes by the execution wave once the frame is complete
// (zstd-jni: "Restored data doesn't match checksum"); a mismatch is TSX_E_BAD_FRAME like any other damage.
//
// A block goes through three stages, each a serial chain that keeps only a few lanes busy, so the chunk's three waves run one
// stage each, one block apart, and meet at one workgroup barrier per block.  In iteration `it` of the loop:
//   wave 1  dec_stage_literals, block it      its header and literals section: the 1 or 4 Huffman streams on lanes 0-3, through
//           per-stream LDS windows and an 11-bit table that yields up to three symbols per read
//           -> the block's descriptor and literal buffer, rings of three (the execution wave reads them two iterations later)
//   wave 0  dec_stage_sequences, block it - 1 the LL / ML / OF state machines in lanes 0-2 (one table read, two DPP adds per
//           sequence), then every lane extracts its own sequence's extra bits; repeat offsets resolved in order
//           -> the block's (literal length, match length, offset) arrays and sequence count, rings of two
//   wave 2  dec_stage_execute, block it - 2   64 sequences per step, positions by prefix sums, copies in dependency rounds
//           -> the output
// Every loop is bounded by sizes read from the frame; every index into LDS or the workspace is checked against them.
// The frame parsing of every stage and the repeat-offset history are in zstd_dec_dev.h (dec_*), shared with the block-parallel form
// (zstd_dec_blocks.hip); this file keeps what is its own: the three-wave pipeline, the tables and Huffman tree carried across
// blocks, in-order execution, and the error codes.
#include "zstd_dec_dev.h"
static DecLapOut g_dprof_out;                                         // 8 u64 per chunk: phase laps of the decoder (a TSX_PROF2 build)
#ifdef TSX_PROF2
extern "C" void tsx_debug_set_dprof(void* dev_ptr) { g_dprof_out.buf = (unsigned long long*)dev_ptr; }
#endif

// What the three waves know about their chunk once its frame header is read; none of it changes.  The decoder needs no hash tables: the
// literal buffers and the sequence arrays (three arrays of ZS_DSEQ_CAP dwords: literal lengths, match lengths, offsets) borrow the
// compressor's workspace regions.
struct DecChunk {
    const uint8_t* __restrict__ src; uint32_t srcSize;                 // the frame
    uint8_t* __restrict__ out; uint64_t contentSize; bool hasChecksum;
    uint8_t* ws;                                                       // the chunk's workspace: three literal buffers, two sets of sequence arrays (the slots below)
};
// The rings.  A slot is rewritten when the last stage that reads it is done with block k: descriptors and literals are read by
// the execution wave two iterations after they were written (three slots), sequences one iteration after (two).
__device__ __forceinline__ static uint8_t* dec_lit_slot(const DecChunk& c, uint32_t k) { const uint32_t s = k % 3; return c.ws + (s == 0 ? ZS_WS_LIT : s == 1 ? ZS_WS_HASHLONG : ZS_WS_HASHLONG + (192u << 10)); }   // literal slot of block k
__device__ __forceinline__ static BlkDesc* dec_desc_slot(DecLds& L, uint32_t k) { return &L.desc[k % 3]; }               // descriptor slot of block k
__device__ __forceinline__ static uint32_t* dec_seq_slot(const DecChunk& c, uint32_t k) { return (uint32_t*)(c.ws + (k & 1 ? ZS_WS_STBITS : ZS_WS_SEQS)); }   // sequence slot of block k,
__device__ __forceinline__ static uint32_t* dec_nseq_slot(DecLds& L, uint32_t k) { return &L.nseq[k & 1]; }                                 // and of its sequence count

// ---- stage 1 (wave 1): block k's header and literals section -> its descriptor and literal slots ----
// p: the block header's position, moved behind the block; prodDone: this was the frame's last block, and the frame ends behind it.
__device__ __forceinline__ static int32_t dec_stage_literals(DecLds& L, const DecChunk& c, uint32_t k, uint32_t& p, bool& prodDone, uint32_t lane) {
    uint8_t* const lit = dec_lit_slot(c, k);
    const DecBlockHdr bh = dec_block_header(c.src, c.srcSize, p);
    if (!bh.ok) return DERR_FRAME;
    p = bh.next;
    BlkDesc bd; bd.off = bh.off; bd.bsize = bh.bsize; bd.btype = bh.btype; bd.last = bh.last; bd.litInPlace = 0; bd.litOff = 0; bd.litSize = 0; bd.q = 0;
    if (bh.btype == 2) {
        const uint8_t* const blk = c.src + bh.off;
        const DecLit h = dec_lit_header(blk, bh.bsize);
        if (!h.section) return DERR_FRAME;
        if (h.ltype == 0) { bd.litInPlace = 1; bd.litOff = h.hl; }
        else if (h.ltype == 1) { const uint8_t b = blk[h.hl]; for (uint32_t i = lane; i < h.litSize; i += LANES) lit[i] = b; }
        else {
            uint32_t t = h.hl;
            if (h.ltype == 2) {
                const uint32_t used = dec_huf_tree(L, blk + h.hl, h.csize, lane);
                if (!used) return DERR_FRAME;
                t += used;
            } else if (!L.hufValid) return DERR_FRAME;                 // treeless: the tree of the latest block that carried one is still in LDS
            if (!dec_huf_streams(L, blk + t, h.section - t, h.streams, h.litSize, lit, lane)) return DERR_FRAME;
        }
        bd.litSize = h.litSize; bd.q = h.section;
    }
    if (bh.last) {
        if (!dec_frame_end(p, c.srcSize, c.hasChecksum)) return DERR_FRAME;
        prodDone = true;
    }
    if (lane == 0) *dec_desc_slot(L, k) = bd;
    return TSX_OK;
}

// ---- stage 2 (wave 0): the sequences of block k -> (literal length, match length, offset) arrays in its sequence slot ----
// rep0..2: the repeat-offset history, carried across the blocks of the frame (wave-uniform); fseDone: block k was the last one.
__device__ __forceinline__ static int32_t dec_stage_sequences(DecLds& L, const DecChunk& c, uint32_t k, uint32_t& rep0, uint32_t& rep1, uint32_t& rep2, bool& fseDone,
                                                              uint32_t lane, DecLaps& laps) {
    const BlkDesc* const bdp = dec_desc_slot(L, k);
    const uint32_t bsize = DUNI(bdp->bsize), btype = DUNI(bdp->btype), boff = DUNI(bdp->off);
    if (DUNI(bdp->last)) fseDone = true;
    if (btype != 2) return TSX_OK;
    uint32_t* const sLL = dec_seq_slot(c, k); uint32_t* const sML = sLL + ZS_DSEQ_CAP; uint32_t* const sOF = sML + ZS_DSEQ_CAP;
    const uint8_t* const blk = c.src + boff;
    const DecSeqHdr sh = dec_seq_header(blk, bsize, DUNI(bdp->q));
    if (!sh.ok) return DERR_FRAME;
    const uint32_t nbSeq = DUNI(sh.nbSeq);                              // loaded through the vector path: pin it (and every loop bound derived from it) to SGPRs
    if (nbSeq) {
        // the three sequence tables (literal lengths, offsets, match lengths); a Repeat keeps the previous block's table
        const uint32_t modes = DUNI(sh.modes);
        uint32_t t = DUNI(sh.t);
        for (int i = 0; i < 3; i++) {
            const uint32_t mode = (modes >> (6 - 2 * i)) & 3;
            int* const validp = i == 0 ? &L.llValid : i == 1 ? &L.ofValid : &L.mlValid;
            if (mode == 3) {
                WAVE_SYNC();
                if (!*validp) return DERR_FRAME;
                continue;
            }
            const int32_t used = dec_seq_table(L, i, mode, blk + t, bsize - t, lane);
            if (used < 0) return DERR_FRAME;
            if (lane == 0) *validp = 1;
            t += (uint32_t)used;
        }
        if (t >= bsize) return DERR_FRAME;
        __threadfence_block();
        WAVE_SYNC();
        laps.lap(1);                                                    // 1: sequence tables
        // the sequences, 64 at a time (one per lane): passes 1 and 2 in dec_seq_group, pass 3 in dec_rep_offsets
        DecSeqStream stream = {blk + t, DUNI(bsize - t), 0, 0, 0};
        TSX_SETPRIO(3);                                                 // the sequence stage is the chunk's critical path: its chain goes first
        for (uint32_t g = 0; g < nbSeq; g += LANES) {
            const uint32_t cnt = DUNI(nbSeq - g < LANES ? nbSeq - g : LANES);
            uint32_t ll, ml, offBase;
            if (!dec_seq_group(L, stream, g, cnt, nbSeq, lane, ll, ml, offBase)) return DERR_FRAME;
            const bool valid = lane < cnt;
            const uint32_t off = dec_rep_offsets(offBase, ll, valid, cnt, rep0, rep1, rep2, [](uint32_t v) { return v - 1; });
            if (valid) { sLL[g + lane] = ll; sML[g + lane] = ml; sOF[g + lane] = off; }
            laps.lap(2);                                                // 2: FSE sequence decode
        }
        TSX_SETPRIO(0);
        if (stream.B != 0) return DERR_FRAME;                           // BIT_endOfDStream: every bit of the stream was used
    }
    if (lane == 0) *dec_nseq_slot(L, k) = nbSeq;
    return TSX_OK;
}

// One group of up to 64 sequences (this lane's: ll, ml, off) whose literals start at lit and whose output starts at out + opos;
// myOut = where this lane's sequence starts.  Positions come from prefix sums, so literal runs and every match whose source lies
// before the group's first output byte are copied by their own lane, all at once; only matches that read bytes produced inside
// the same group (short offsets) are replayed in order.  Short runs are copied by their own lane (all lanes at once), long ones
// (> ZS_LONG_RUN bytes) by the whole wave.  A match is ready when its source bytes are final: before the group's first output
// byte, or - after the fence that follows each round - inside literal runs and matches already copied.  Each round copies every
// pending match whose source touches no earlier pending match's destination; a match that overlaps its own destination
// (offset < length) is replayed by the whole wave, in 64-byte steps or as a periodic pattern.
__device__ __forceinline__ static void dec_exec_group(uint8_t* __restrict__ out, const uint8_t* __restrict__ lit, uint32_t opos, uint32_t myOut,
                                                      uint32_t ll, uint32_t ml, uint32_t off, bool valid, uint32_t lane) {
    const uint32_t mOut = myOut + ll, s0 = mOut - off;
    exec_copies(out + myOut, lit, ll, valid && ll, lane);
    unsigned long long pend = __ballot(valid && ml);
    bool first = true;
    do {
        const bool mineP = (pend >> lane) & 1;
        bool blocked = mineP && off < ml;
        if (first) blocked = mineP && s0 + ml > opos;                          // round 0: only sources before the group
        else
            for (unsigned long long m = pend; m; m &= m - 1) {
                const int j = __ffsll((long long)m) - 1;
                const uint32_t dj = __builtin_amdgcn_readlane(mOut, j), ej = dj + __builtin_amdgcn_readlane(ml, j);
                if ((uint32_t)j < lane && s0 < ej && s0 + ml > dj) blocked = true;
            }
        const unsigned long long ready = __ballot(mineP && !blocked);
        if (ready || first) {
            exec_copies(out + mOut, out + s0, ml, (ready >> lane) & 1, lane);
            pend &= ~ready;
            first = false;
        } else {                                                                // the first pending match overlaps itself
            const int i = __ffsll((long long)pend) - 1;
            pend &= pend - 1;
            const uint32_t dpos = __builtin_amdgcn_readlane(mOut, i), o_ = __builtin_amdgcn_readlane(off, i), m_ = __builtin_amdgcn_readlane(ml, i);
            const uint32_t from = dpos - o_;
            if (o_ >= LANES) {
                for (uint32_t k = 0; k < m_; k += LANES) {
                    if (k) __threadfence_block();                               // a 64-byte step may read bytes written by the previous step
                    if (k + lane < m_) out[dpos + k + lane] = out[from + k + lane];
                }
            } else {
                for (uint32_t k = lane; k < m_; k += LANES) out[dpos + k] = out[from + (k % o_)];   // periodic pattern
            }
        }
        __threadfence_block();
    } while (pend);
}

// ---- stage 3 (wave 2): block k into the output (its literals were decoded two iterations ago, its sequences one) ----
// opos: the bytes restored so far; frameDone: block k was the last one.
__device__ __forceinline__ static int32_t dec_stage_execute(DecLds& L, const DecChunk& c, uint32_t k, uint32_t& opos, bool& frameDone, uint32_t lane) {
    const BlkDesc* const bdp = dec_desc_slot(L, k);
    const uint32_t bsize = DUNI(bdp->bsize), btype = DUNI(bdp->btype), boff = DUNI(bdp->off);
    uint8_t* __restrict__ const out = c.out;
    frameDone = DUNI(bdp->last) != 0;
    if (btype == 0) {                                                   // raw
        if (opos + (uint64_t)bsize > c.contentSize) return DERR_FRAME;
        for (uint32_t i = lane; i < bsize; i += LANES) out[opos + i] = c.src[boff + i];
        opos += bsize;
        __threadfence_block();
        return TSX_OK;
    }
    if (btype == 1) {                                                   // RLE
        if (opos + (uint64_t)bsize > c.contentSize) return DERR_FRAME;
        const uint8_t b = c.src[boff];
        for (uint32_t i = lane; i < bsize; i += LANES) out[opos + i] = b;
        opos += bsize;
        __threadfence_block();
        return TSX_OK;
    }
    const uint32_t litSize = DUNI(bdp->litSize), nbSeq = DUNI(*dec_nseq_slot(L, k));
    const uint8_t* const litPtr = DUNI(bdp->litInPlace) ? c.src + boff + DUNI(bdp->litOff) : dec_lit_slot(c, k);
    const uint32_t* const sLL = dec_seq_slot(c, k); const uint32_t* const sML = sLL + ZS_DSEQ_CAP; const uint32_t* const sOF = sML + ZS_DSEQ_CAP;
    uint32_t lp = 0;
    for (uint32_t g = 0; g < nbSeq; g += LANES) {
        const uint32_t cnt = nbSeq - g < LANES ? nbSeq - g : LANES;
        const bool valid = lane < cnt;
        const uint32_t ll = valid ? sLL[g + lane] : 0, ml = valid ? sML[g + lane] : 0, off = valid ? sOF[g + lane] : 0;
        uint32_t litIncl = ll, totIncl = ll + ml;
        dec_incl_scan2(litIncl, totIncl, lane);
        const uint32_t groupLit = (uint32_t)__builtin_amdgcn_readlane(litIncl, LANES - 1), groupTot = (uint32_t)__builtin_amdgcn_readlane(totIncl, LANES - 1);
        if (lp + groupLit > litSize || (uint64_t)opos + groupTot > c.contentSize) return DERR_FRAME;
        const uint32_t myLit = lp + litIncl - ll, myOut = opos + totIncl - (ll + ml);
        if (__any(valid && ml && (off == 0 || off > myOut + ll))) return DERR_FRAME;
        dec_exec_group(out, litPtr + myLit, opos, myOut, ll, ml, off, valid, lane);
        lp += groupLit; opos += groupTot;
    }
    const uint32_t tail = litSize - lp;                                 // the literals behind the last sequence
    if ((uint64_t)opos + tail > c.contentSize) return DERR_FRAME;
    for (uint32_t i = lane; i < tail; i += LANES) out[opos + i] = litPtr[lp + i];
    opos += tail;
    __threadfence_block();
    return TSX_OK;
}

// ---- the kernel: frame header, the pipeline, the frame's end -------------------------------------------------------------------
__device__ __forceinline__ static void zstd_decompress_body(DecLds& L, const uint8_t* __restrict__ frames, int from_mid, uint64_t mid_stride,
                                                            tsx_chunk_desc* __restrict__ descs, uint8_t* __restrict__ dst_base,
                                                            int32_t* __restrict__ status, uint8_t* __restrict__ work,
                                                            const uint32_t* __restrict__ skip, uint32_t skip_stride, DecLapOut dprof) {
    const uint32_t lane = threadIdx.x & (LANES - 1), role = DUNI(threadIdx.x >> 6), chunk = blockIdx.x;   // wave 0: sequences, wave 1: literals, wave 2: execution
    if (status[chunk] != TSX_OK) return;
    if (skip && skip[(size_t)chunk * skip_stride] == 1) return;       // decoded by the block-parallel form (zstd_dec_blocks.hip)
    const tsx_chunk_desc d = descs[chunk];
    const uint8_t* const src = from_mid ? frames + (uint64_t)chunk * mid_stride : frames + d.src_off;
    const uint32_t srcSize = from_mid ? d.src_len - 28 : d.src_len;
    DecLaps laps;
    const DecFrame fh = dec_frame_header(src, srcSize);
    const DecChunk c = {src, srcSize, dst_base + d.dst_off, fh.contentSize, fh.hasChecksum, work + (size_t)chunk * ZS_WS_BYTES};
    // each wave's own state, in its registers: the literal wave's read position, the sequence wave's repeat-offset history, the
    // execution wave's output position - and whether it has seen the frame's last block (a descriptor slot may already be
    // rewritten by another wave when the barrier opens, so each wave answers that from what it consumed itself)
    uint32_t p = fh.p, rep0 = 1, rep1 = 4, rep2 = 8, opos = 0;
    bool prodDone = false, fseDone = false, frameDone = false;
    int32_t err = fh.status != TSX_OK ? fh.status : fh.contentSize > d.dst_cap ? TSX_E_DST_TOO_SMALL : TSX_OK;
    if (err == TSX_OK) {
        if (role == 0 && lane == 0) { L.hufValid = 0; L.llValid = 0; L.ofValid = 0; L.mlValid = 0; L.err = TSX_OK; }
        if (role == 0) dec_code_tables(L, lane);
        __syncthreads();
        // Iteration `it`: block it's literals, block it - 1's sequences, block it - 2's execution, side by side; one workgroup barrier
        // per iteration.  An error of any wave is posted in L.err and ends all three behind the barrier.
        for (uint32_t it = 0;; it++) {
            int32_t myErr = TSX_OK;
            if (role == 1) {
                if (!prodDone) { myErr = dec_stage_literals(L, c, it, p, prodDone, lane); laps.lap(0); }                               // 0: block header + literals section
            } else if (role == 2) {
                if (it >= 2) { myErr = dec_stage_execute(L, c, it - 2, opos, frameDone, lane); laps.lap(3); }                          // 3: execution
            } else if (it >= 1 && !fseDone) myErr = dec_stage_sequences(L, c, it - 1, rep0, rep1, rep2, fseDone, lane, laps);          // 1, 2: tables, sequences
            if (myErr != TSX_OK && lane == 0) L.err = myErr;
            laps.lap(4);                                                // 4: this wave's work outside the named phases
            __threadfence_block();
            __syncthreads();
            laps.lap(5);                                                // 5: waiting for the other waves
            err = (int32_t)DUNI(L.err);
            if (err != TSX_OK) break;
            if (role == 0 ? fseDone : role == 1 ? prodDone : frameDone) break;     // a wave that has nothing left to do leaves; the barrier counts live waves
        }
        if (role == 2 && err == TSX_OK && opos != c.contentSize) err = DERR_FRAME;
        if (role == 2 && err == TSX_OK && c.hasChecksum) {              // (the literal wave has found the four bytes at the frame's end: dec_frame_end)
            __threadfence_block();
            if (!dec_checksum_ok(c.out, opos, dec_checksum_at(c.src, c.srcSize - 4), lane)) err = DERR_FRAME;
        }
    }
    if (lane == 0) {                                                    // laps: wave 1 -> 0 (literals), 6 (wait); wave 2 -> 3 (execution), 5 (wait); wave 0 -> 1, 2, 4, 7 (wait)
        if (role == 1) { laps.put(dprof, chunk, 0, 0, 4); laps.put(dprof, chunk, 6, 5); }
        else if (role == 2) { laps.put(dprof, chunk, 3, 3, 4); laps.put(dprof, chunk, 5, 5); }
        else { laps.put(dprof, chunk, 1, 1); laps.put(dprof, chunk, 2, 2); laps.put(dprof, chunk, 4, 4); laps.put(dprof, chunk, 7, 5); }
    }
    if (role == 2 && lane == 0) {
        if (err != TSX_OK) { status[chunk] = err; descs[chunk].dst_len = 0; }
        else descs[chunk].dst_len = opos;
    }
}

// Two builds of the same body.  The batch decoder is shaped for residency: 6 waves per SIMD (80 VGPRs; the compiler reports 0 bytes of
// scratch for it as well).  The one that runs BEHIND the block-parallel form of a fetch (skip list: it only decodes what that form handed
// back) must not touch scratch at all, whatever a later change does to the other: a queue's first scratch-using dispatch makes the
// runtime (re)size that queue's scratch, and while the compressor service's long-lived kernel holds its own (large) scratch that request
// waits for the kernel to end - measured: the first fetch after uploads began took 18.6 s, every later one 4 ms.  No fetch-path kernel
// uses scratch (tests/test_boundary.py checks the compiler's resource report).
#define ZD_KERNEL_PARAMS const uint8_t* __restrict__ frames, int from_mid, uint64_t mid_stride, tsx_chunk_desc* __restrict__ descs, uint8_t* __restrict__ dst_base, \
                         int32_t* __restrict__ status, uint8_t* __restrict__ work, const uint32_t* __restrict__ skip, uint32_t skip_stride, DecLapOut dprof
__global__ __launch_bounds__(3 * LANES) __attribute__((amdgpu_waves_per_eu(6, 6))) void zstd_decompress_kernel(ZD_KERNEL_PARAMS) {
    __shared__ DecLds L;
    zstd_decompress_body(L, frames, from_mid, mid_stride, descs, dst_base, status, work, skip, skip_stride, dprof);
}
__global__ __launch_bounds__(3 * LANES) void zstd_decompress_fallback_kernel(ZD_KERNEL_PARAMS) {
    __shared__ DecLds L;
    zstd_decompress_body(L, frames, from_mid, mid_stride, descs, dst_base, status, work, skip, skip_stride, dprof);
}

uint32_t tsx_launch_zstd_decompress(hipStream_t st, const uint8_t* frames, int from_mid, uint64_t mid_stride,
                                    tsx_chunk_desc* d_descs, uint32_t n, uint8_t* dst, int32_t* d_status, void* d_work,
                                    const uint32_t* skip, uint32_t skip_stride, bool no_scratch) {
    if (!n) return 0;
    const auto kernel = skip || no_scratch ? zstd_decompress_fallback_kernel : zstd_decompress_kernel;
    hipLaunchKernelGGL(kernel, dim3(n), dim3(3 * LANES), 0, st, frames, from_mid, mid_stride, d_descs, dst, d_status, (uint8_t*)d_work, skip, skip_stride, g_dprof_out);
    return 1;
}

// test hook: XXH64 (seed 0) of len bytes at a device address of any alignment, by one wave as the decoders run it -> *out
__global__ __launch_bounds__(LANES) void xxh64_probe_kernel(const uint8_t* p, uint32_t len, unsigned long long* out) {
    const unsigned long long h = xxh64_wave(p, len, threadIdx.x);
    if (threadIdx.x == 0) *out = h;
}
extern "C" int tsx_debug_xxh64(const void* dev_ptr, uint32_t len, unsigned long long* out) {
    unsigned long long* d = nullptr;
    if (!out || (len && !dev_ptr) || hipMalloc((void**)&d, sizeof *d) != hipSuccess) return TSX_E_INVAL;
    hipLaunchKernelGGL(xxh64_probe_kernel, dim3(1), dim3(LANES), 0, (hipStream_t)0, (const uint8_t*)dev_ptr, len, d);
    const hipError_t e = hipMemcpy(out, d, sizeof *d, hipMemcpyDeviceToHost);
    hipFree(d);
    return e == hipSuccess ? TSX_OK : TSX_E_DEVICE;
}
