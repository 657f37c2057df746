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
// A block goes through three stages, each a serial chain that keeps only a few lanes busy, so the chunk's three
// waves run them one block apart and meet at one workgroup barrier per block:
//   wave 1  block headers + literals: the 1 or 4 Huffman streams on lanes 0-3, through per-stream LDS windows and an
//           11-bit table that yields up to three symbols per read                          -> literal buffer k % 3
//   wave 0  sequence stream: the LL / ML / OF state machines in lanes 0-2 (one table read, two DPP adds per sequence),
//           then every lane extracts its own sequence's extra bits; repeat offsets resolved in order -> arrays k & 1
//   wave 2  execution: 64 sequences per step, positions by prefix sums, copies in dependency rounds  -> the output
// Every loop is bounded by sizes read from the frame; every index into LDS or the workspace is checked against them.
// The frame parsing of every stage is in zstd_dec_dev.h (dec_*), shared with the block-parallel form (zstd_dec_blocks.hip); this
// file keeps what is its own: the three-wave pipeline, the tables and Huffman tree carried across blocks, the concrete repeat
// offsets (pass 3), in-order execution, and the error codes.
#include "zstd_dec_dev.h"
#ifdef TSX_PROF2
static unsigned long long* g_dprof_out = nullptr;                     // 8 u64 per chunk: phase laps of the decoder
extern "C" void tsx_debug_set_dprof(void* dev_ptr) { g_dprof_out = (unsigned long long*)dev_ptr; }
#define DLT(k) do { const unsigned long long n_ = (unsigned long long)clock64(); dlt_[k] += n_ - dlast_; dlast_ = n_; } while (0)
#else
#define DLT(k) do {} while (0)
#endif

// ---- the kernel -------------------------------------------------------------------------------------------
#define FAIL(code) do { err = (code); goto done; } while (0)                 /* both waves, before the block loop */
#define RFAIL(code) do { myErr = (code); goto block_end; } while (0)        /* one wave, inside its role */

__device__ __forceinline__ static void zstd_decompress_body(DecLds& L, const uint8_t* __restrict__ frames, int from_mid, uint64_t mid_stride,
                                                            tsx_chunk_desc* __restrict__ descs, uint8_t* __restrict__ dst_base,
                                                            int32_t* __restrict__ status, uint8_t* __restrict__ work,
                                                            const uint32_t* __restrict__ skip, uint32_t skip_stride
#ifdef TSX_PROF2
                                                            , unsigned long long* __restrict__ dprof
#endif
                                                            ) {
    const uint32_t lane = threadIdx.x & (LANES - 1), role = DUNI(threadIdx.x >> 6), chunk = blockIdx.x;   // wave 0: sequence streams, wave 1: literals, wave 2: execution
    if (status[chunk] != TSX_OK) return;
    if (skip && skip[(size_t)chunk * skip_stride] == 1) return;       // decoded by the block-parallel form (zstd_dec_blocks.hip)
    const tsx_chunk_desc d = descs[chunk];
    const uint8_t* __restrict__ src = from_mid ? frames + (uint64_t)chunk * mid_stride : frames + d.src_off;
    const uint32_t srcSize = from_mid ? d.src_len - 28 : d.src_len;
    uint8_t* __restrict__ out = dst_base + d.dst_off;
    uint8_t* const ws = work + (size_t)chunk * ZS_WS_BYTES;
    // literals of block k -> litBuf[k % 3], its sequences -> seqBuf[k & 1] (three arrays of ZS_DSEQ_CAP dwords); the decoder needs no hash tables
    uint8_t* const litBuf[3] = {ws + ZS_WS_LIT, ws + ZS_WS_HASHLONG, ws + ZS_WS_HASHLONG + (192u << 10)};
    uint8_t* const seqBuf[2] = {ws + ZS_WS_SEQS, ws + ZS_WS_STBITS};
    int32_t err = TSX_OK;
#ifdef TSX_PROF2
    unsigned long long dlt_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dlast_ = (unsigned long long)clock64();
#endif
    uint32_t opos = 0;
    uint32_t rep0 = 1, rep1 = 4, rep2 = 8;                           // repeat-offset history, carried across the blocks of the frame (wave-uniform)
    uint64_t contentSize = 0;
    uint32_t p = 0;
    bool hasChecksum = false, prodDone = false, fseDone = false, frameDone = false;
    {   const DecFrame fh = dec_frame_header(src, srcSize);
        if (fh.status != TSX_OK) FAIL(fh.status);
        if (fh.contentSize > d.dst_cap) FAIL(TSX_E_DST_TOO_SMALL);
        p = fh.p; contentSize = fh.contentSize; hasChecksum = fh.hasChecksum;
    }
    if (role == 0 && lane == 0) { L.hufValid = 0; L.llValid = 0; L.ofValid = 0; L.mlValid = 0; L.zeroEntry = 0; L.err = TSX_OK; }
    if (role == 0 && lane < 36) { L.cLLbase[lane] = dLLbase[lane]; L.cLLbits[lane] = dLLbits[lane]; }
    if (role == 0 && lane < 53) { L.cMLbase[lane] = dMLbase[lane]; L.cMLbits[lane] = dMLbits[lane]; }
    __syncthreads();
    // ---- blocks: wave 1 (literals) works one block ahead of wave 0 (sequences + execution) ----
    // Iteration `it`: wave 1 parses block it's header and literals section (Huffman streams -> litBuf[it & 1]) and publishes
    // L.desc[it & 1]; wave 0 decodes and executes the sequences of block it - 1.  One workgroup barrier per iteration; an error
    // of either wave is posted in L.err and ends both after the barrier.  Neither phase of a block waits for the other's
    // memory latency any more: the serial chains of the two phases run side by side.
    for (uint32_t it = 0;; it++) {
        int32_t myErr = TSX_OK;
        // Was block it - 1 the frame's last one?  Each wave answers from its own registers (a descriptor slot may already be
        // rewritten by the other wave when the barrier opens): wave 1 finished producing, wave 0 consumed a block marked last.
        {
            if (role == 1) {
                if (!prodDone) {
                    uint8_t* const lit = litBuf[it % 3];
                    const DecBlockHdr bh = dec_block_header(src, srcSize, p);
                    if (!bh.ok) RFAIL(DERR_FRAME);
                    p = bh.next;
                    BlkDesc bd; bd.off = bh.off; bd.bsize = bh.bsize; bd.btype = bh.btype; bd.last = bh.last; bd.litInPlace = 0; bd.litOff = 0; bd.litSize = 0; bd.q = 0;
                    if (bh.btype == 2) {
                        const uint8_t* const blk = src + bh.off;
                        const DecLit h = dec_lit_header(blk, bh.bsize);
                        if (!h.section) RFAIL(DERR_FRAME);
                        if (h.ltype == 0) { bd.litInPlace = 1; bd.litOff = h.hl; }
                        else if (h.ltype == 1) { const uint8_t b = blk[h.hl]; for (uint32_t i = lane; i < h.litSize; i += LANES) lit[i] = b; }
                        else {
                            uint32_t t = h.hl;
                            if (h.ltype == 2) {
                                if (lane == 0) L.scalH[0] = huf_readTable(L, blk + h.hl, h.csize);
                                WAVE_SYNC();
                                const uint32_t used = L.scalH[0];
                                WAVE_SYNC();
                                if (!used) RFAIL(DERR_FRAME);
                                huf_buildX_wave(L, lane);
                                WAVE_SYNC();
                                t += used;
                            } else if (!L.hufValid) RFAIL(DERR_FRAME);
                            if (!dec_huf_streams(L, blk + t, h.section - t, h.streams, h.litSize, lit, lane)) RFAIL(DERR_FRAME);
                        }
                        bd.litSize = h.litSize; bd.q = h.section;
                    }
                    if (bh.last) {
                        if (!dec_frame_end(p, srcSize, hasChecksum)) RFAIL(DERR_FRAME);
                        prodDone = true;
                    }
                    if (lane == 0) L.desc[it % 3] = bd;
                    DLT(0);                                             // 0: block header + literals section
                }
            } else if (role == 2) {
                if (it >= 2) {
                    // ---- wave 2: execute block it - 2 (its literals were decoded two iterations ago, its sequences one) ----
                    const BlkDesc* const bdp = &L.desc[(it - 2) % 3];
                    const uint32_t bsize = DUNI(bdp->bsize), btype = DUNI(bdp->btype), boff = DUNI(bdp->off);
                    frameDone = DUNI(bdp->last) != 0;
                    if (btype == 0) {                                   // raw
                        if (opos + (uint64_t)bsize > contentSize) RFAIL(DERR_FRAME);
                        for (uint32_t i = lane; i < bsize; i += LANES) out[opos + i] = src[boff + i];
                        opos += bsize;
                        __threadfence_block();
                    } else if (btype == 1) {                            // RLE
                        if (opos + (uint64_t)bsize > contentSize) RFAIL(DERR_FRAME);
                        const uint8_t b = src[boff];
                        for (uint32_t i = lane; i < bsize; i += LANES) out[opos + i] = b;
                        opos += bsize;
                        __threadfence_block();
                    } else {
                        const uint32_t litSize = DUNI(bdp->litSize), nbSeq = DUNI(L.nseq[(it - 2) & 1]);
                        const uint8_t* const litPtr = DUNI(bdp->litInPlace) ? src + boff + DUNI(bdp->litOff) : litBuf[(it - 2) % 3];
                        const uint32_t* const sLL = (const uint32_t*)seqBuf[(it - 2) & 1]; const uint32_t* const sML = sLL + ZS_DSEQ_CAP; const uint32_t* const sOF = sML + ZS_DSEQ_CAP;
                        uint32_t lp = 0;
                        for (uint32_t g = 0; g < nbSeq; g += LANES) {
                            const uint32_t cnt = nbSeq - g < LANES ? nbSeq - g : LANES;
                            const bool valid = lane < cnt;
                            const uint32_t ll = valid ? sLL[g + lane] : 0, ml = valid ? sML[g + lane] : 0, off = valid ? sOF[g + lane] : 0;
                            // Execution.  Positions come from prefix sums, so literal runs and every match whose source lies before the
                            // group's first output byte are copied by their own lane, all at once; only matches that read bytes produced
                            // inside the same group (short offsets) are replayed in order with wave-wide copies.
                            uint32_t litIncl = ll, totIncl = ll + ml;
                            for (int o = 1; o < LANES; o <<= 1) {
                                const uint32_t a = __shfl_up(litIncl, o), t = __shfl_up(totIncl, o);
                                if (lane >= (uint32_t)o) { litIncl += a; totIncl += t; }
                            }
                            const uint32_t groupLit = (uint32_t)__builtin_amdgcn_readlane(litIncl, LANES - 1), groupTot = (uint32_t)__builtin_amdgcn_readlane(totIncl, LANES - 1);
                            if (lp + groupLit > litSize || (uint64_t)opos + groupTot > contentSize) RFAIL(DERR_FRAME);
                            const uint32_t myLit = lp + litIncl - ll, myOut = opos + totIncl - (ll + ml), mOut = myOut + ll;
                            if (__any(valid && ml && (off == 0 || off > mOut))) RFAIL(DERR_FRAME);
                            // Short runs are copied by their own lane (all lanes at once), long ones (> ZS_LONG_RUN bytes) by the whole wave.
                            // A match is ready when its source bytes are final: before the group's first output byte, or - after the
                            // fence that follows each round - inside literal runs and matches already copied.  Each round copies every
                            // pending match whose source touches no earlier pending match's destination; a match that overlaps its own
                            // destination (offset < length) is replayed by the whole wave, in 64-byte steps or as a periodic pattern.
                            const uint32_t s0 = mOut - off;
                            exec_copies(out + myOut, litPtr + myLit, ll, valid && ll, lane);
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
                            lp += groupLit; opos += groupTot;
                        }
                        const uint32_t tail = litSize - lp;
                        if ((uint64_t)opos + tail > contentSize) RFAIL(DERR_FRAME);
                        for (uint32_t k = lane; k < tail; k += LANES) out[opos + k] = litPtr[lp + k];
                        opos += tail;
                        __threadfence_block();
                    }
                    DLT(3);                                             // 3: execution
                }
            } else if (it >= 1 && !fseDone) {
                // ---- wave 0: the sequences of block it - 1 -> (literal length, match length, offset) arrays in seqBuf[(it - 1) & 1] ----
                const BlkDesc* const bdp = &L.desc[(it - 1) % 3];
                const uint32_t bsize = DUNI(bdp->bsize), btype = DUNI(bdp->btype), boff = DUNI(bdp->off);
                if (DUNI(bdp->last)) fseDone = true;
                if (btype == 2) {
                    uint32_t* const sLL = (uint32_t*)seqBuf[(it - 1) & 1]; uint32_t* const sML = sLL + ZS_DSEQ_CAP; uint32_t* const sOF = sML + ZS_DSEQ_CAP;
                    const uint8_t* const blk = src + boff;
                    const DecSeqHdr sh = dec_seq_header(blk, bsize, DUNI(bdp->q));
                    if (!sh.ok) RFAIL(DERR_FRAME);
                    const uint32_t nbSeq = DUNI(sh.nbSeq);                      // loaded through the vector path: pin it (and every loop bound derived from it) to SGPRs
                    if (nbSeq) {
                        // the three sequence tables (literal lengths, offsets, match lengths); a Repeat keeps the previous block's table
                        const uint32_t modes = DUNI(sh.modes);
                        uint32_t t = DUNI(sh.t);
                        for (int k = 0; k < 3; k++) {
                            const uint32_t mode = (modes >> (6 - 2 * k)) & 3;
                            int* const validp = k == 0 ? &L.llValid : k == 1 ? &L.ofValid : &L.mlValid;
                            if (mode == 3) {
                                WAVE_SYNC();
                                if (!*validp) RFAIL(DERR_FRAME);
                                continue;
                            }
                            const int32_t used = dec_seq_table(L, k, mode, blk + t, bsize - t, lane);
                            if (used < 0) RFAIL(DERR_FRAME);
                            if (lane == 0) *validp = 1;
                            t += (uint32_t)used;
                        }
                        if (t >= bsize) RFAIL(DERR_FRAME);
                        __threadfence_block();
                        WAVE_SYNC();
                        DLT(1);                                                 // 1: sequence tables
                        // ---- decode the sequences, 64 at a time (one per lane): passes 1 and 2 in dec_seq_group, pass 3 below ----
                        DecSeqStream stream = {blk + t, DUNI(bsize - t), 0, 0, 0};
                        TSX_SETPRIO(3);                                         // the sequence stage is the chunk's critical path: its chain goes first
                        for (uint32_t g = 0; g < nbSeq; g += LANES) {
                            const uint32_t cnt = DUNI(nbSeq - g < LANES ? nbSeq - g : LANES);
                            uint32_t ll, ml, offBase;
                            if (!dec_seq_group(L, stream, g, cnt, nbSeq, lane, ll, ml, offBase)) RFAIL(DERR_FRAME);
                            const bool valid = lane < cnt;
                            // pass 3: repeat offsets.  A sequence with a new offset (code > 3) knows it already and only pushes it onto the
                            // history; the scalar loop visits just the sequences that USE the history (codes 1..3), in order, first
                            // folding in the new offsets pushed since the previous visit (only the last three matter).  Code c names
                            // history entry idx = c - 1 (+ 1 when the literal length is 0; idx 3 = rep0 - 1); idx >= 2 pushes the whole
                            // history down, idx 1 swaps the first two, idx 0 leaves it alone.  All on wave-uniform values, no branches.
                            uint32_t off = offBase - 3;
                            {
                                const unsigned long long ll0 = __ballot(valid && ll == 0);
                                unsigned long long users = __ballot(valid && offBase <= 3);
                                uint32_t r0 = DUNI(rep0), r1 = DUNI(rep1), r2 = DUNI(rep2);
                                uint32_t prev = 0;                                                  // first sequence not folded in yet
                                for (;;) {
                                    const uint32_t j = users ? (uint32_t)__ffsll((long long)users) - 1 : cnt;      // next user, or the group's end
                                    const uint32_t gap = j - prev;                                  // new offsets pushed by sequences [prev, j)
                                    const uint32_t a1 = __builtin_amdgcn_readlane(offBase, (int)(j >= 1 ? j - 1 : 0)) - 3;
                                    const uint32_t a2 = __builtin_amdgcn_readlane(offBase, (int)(j >= 2 ? j - 2 : 0)) - 3;
                                    const uint32_t a3 = __builtin_amdgcn_readlane(offBase, (int)(j >= 3 ? j - 3 : 0)) - 3;
                                    const uint32_t n2 = gap >= 3 ? a3 : gap == 2 ? r0 : gap == 1 ? r1 : r2;
                                    const uint32_t n1 = gap >= 2 ? a2 : gap == 1 ? r0 : r1;
                                    const uint32_t n0 = gap >= 1 ? a1 : r0;
                                    r0 = n0; r1 = n1; r2 = n2;
                                    if (!users) break;
                                    users &= users - 1;
                                    const uint32_t ob = __builtin_amdgcn_readlane(offBase, (int)j);
                                    const uint32_t idx = ob - 1 + (uint32_t)((ll0 >> j) & 1);       // 0..3
                                    const uint32_t c01 = idx == 0 ? r0 : r1, c23 = idx == 2 ? r2 : r0 - 1;
                                    const uint32_t o_ = idx < 2 ? c01 : c23;
                                    r2 = idx >= 2 ? r1 : r2;
                                    r1 = idx >= 1 ? r0 : r1;
                                    r0 = o_;
                                    off = tsx_writelane(o_, j, off);
                                    prev = j + 1;
                                }
                                rep0 = r0; rep1 = r1; rep2 = r2;
                            }
                            if (valid) { sLL[g + lane] = ll; sML[g + lane] = ml; sOF[g + lane] = off; }
                            DLT(2);                                                 // 2: FSE sequence decode
                        }
                        TSX_SETPRIO(0);
                        if (stream.B != 0) RFAIL(DERR_FRAME);                      // BIT_endOfDStream: every bit of the stream was used
                    }
                    if (lane == 0) L.nseq[(it - 1) & 1] = nbSeq;
                }
            }
        }
block_end:
        if (myErr != TSX_OK && lane == 0) L.err = myErr;
        DLT(4);                                                         // 4: this wave's work outside the named phases
        __threadfence_block();
        __syncthreads();
        DLT(5);                                                         // 5: waiting for the other wave
        const int32_t posted = (int32_t)DUNI(L.err);
        if (posted != TSX_OK) { err = posted; break; }
        if (role == 0 ? fseDone : role == 1 ? prodDone : frameDone) break;     // a wave that has nothing left to do leaves; the barrier counts live waves
    }
    if (role == 2 && err == TSX_OK && opos != contentSize) err = DERR_FRAME;
    if (role == 2 && err == TSX_OK && hasChecksum) {                    // (the literal wave has found the four bytes at the frame's end: dec_frame_end)
        __threadfence_block();
        if (!dec_checksum_ok(out, opos, dec_checksum_at(src, srcSize - 4), lane)) err = DERR_FRAME;
    }
done:
#ifdef TSX_PROF2
    if (lane == 0 && dprof) {                                           // laps: wave 1 -> 0 (literals), 6 (wait); wave 2 -> 3 (execution), 5 (wait); wave 0 -> 1, 2, 4, 7 (wait)
        unsigned long long* const dp = dprof + (size_t)chunk * 8;
        if (role == 1) { dp[0] = dlt_[0] + dlt_[4]; dp[6] = dlt_[5]; }
        else if (role == 2) { dp[3] = dlt_[3] + dlt_[4]; dp[5] = dlt_[5]; }
        else { dp[1] = dlt_[1]; dp[2] = dlt_[2]; dp[4] = dlt_[4]; dp[7] = dlt_[5]; }
    }
#endif
    if (role == 2 && lane == 0) {
        if (err != TSX_OK) { status[chunk] = err; descs[chunk].dst_len = 0; }
        else descs[chunk].dst_len = opos;
    }
}

#ifdef TSX_PROF2
#define ZD_PROF_PARAM , unsigned long long* __restrict__ dprof
#define ZD_PROF_ARG , dprof
#else
#define ZD_PROF_PARAM
#define ZD_PROF_ARG
#endif
// Two builds of the same body.  The batch decoder is shaped for residency: 6 waves per SIMD (80 VGPRs, a few spilled to scratch).  The one
// that runs BEHIND the block-parallel form of a fetch (skip list: it only decodes what that form handed back) must not touch scratch at
// all: a queue's first scratch-using dispatch makes the runtime (re)size that queue's scratch, and while the compressor service's
// long-lived kernel holds its own (large) scratch that request waits for the kernel to end - measured: the first fetch after uploads
// began took 18.6 s, every later one 4 ms (gpurun r05a).  No fetch-path kernel uses scratch (tests/test_boundary.py checks the code object).
__global__ __launch_bounds__(3 * LANES) __attribute__((amdgpu_waves_per_eu(6, 6))) void zstd_decompress_kernel(const uint8_t* __restrict__ frames, int from_mid, uint64_t mid_stride,
                                                                tsx_chunk_desc* __restrict__ descs, uint8_t* __restrict__ dst_base,
                                                                int32_t* __restrict__ status, uint8_t* __restrict__ work,
                                                                const uint32_t* __restrict__ skip, uint32_t skip_stride ZD_PROF_PARAM) {
    __shared__ DecLds L;
    zstd_decompress_body(L, frames, from_mid, mid_stride, descs, dst_base, status, work, skip, skip_stride ZD_PROF_ARG);
}
__global__ __launch_bounds__(3 * LANES) void zstd_decompress_fallback_kernel(const uint8_t* __restrict__ frames, int from_mid, uint64_t mid_stride,
                                                                tsx_chunk_desc* __restrict__ descs, uint8_t* __restrict__ dst_base,
                                                                int32_t* __restrict__ status, uint8_t* __restrict__ work,
                                                                const uint32_t* __restrict__ skip, uint32_t skip_stride ZD_PROF_PARAM) {
    __shared__ DecLds L;
    zstd_decompress_body(L, frames, from_mid, mid_stride, descs, dst_base, status, work, skip, skip_stride ZD_PROF_ARG);
}

uint32_t tsx_launch_zstd_decompress(hipStream_t st, const tsx_zstd_consts* /*d_zc*/, const uint8_t* frames, int from_mid, uint64_t mid_stride,
                                    tsx_chunk_desc* d_descs, uint32_t n, uint8_t* dst, int32_t* d_status, void* d_work,
                                    const uint32_t* skip, uint32_t skip_stride, bool no_scratch) {
    if (!n) return 0;
    if (skip || no_scratch) hipLaunchKernelGGL(zstd_decompress_fallback_kernel, dim3(n), dim3(3 * LANES), 0, st, frames, from_mid, mid_stride, d_descs, dst, d_status, (uint8_t*)d_work, skip, skip_stride
#ifdef TSX_PROF2
                       , g_dprof_out
#endif
                       );
    else hipLaunchKernelGGL(zstd_decompress_kernel, dim3(n), dim3(3 * LANES), 0, st, frames, from_mid, mid_stride, d_descs, dst, d_status, (uint8_t*)d_work, skip, skip_stride
#ifdef TSX_PROF2
                       , g_dprof_out
#endif
                       );
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
