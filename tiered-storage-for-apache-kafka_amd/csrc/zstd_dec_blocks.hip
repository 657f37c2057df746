// Zstandard frame decoder, block-parallel form — gfx950.  For SMALL batches (a fetch: one chunk, or the few chunks of a prefetch
// window - DefaultChunkManager.java:50-70, ChunkCache.java:159-184), where zstd_dec.hip's one-workgroup-per-chunk pipeline is all
// latency: a 4 MiB chunk is 32 blocks one after the other, 25-50 ms however idle the chip is.  Here the unit of work is the BLOCK:
//
//   zb_index_kernel    one wave per chunk.  Frame header; lane 0 walks the block headers (a chain of <= 264 three-byte reads); then
//                      one lane per block parses the literals-section and sequences-section headers - sizes, table modes, where
//                      each table description and the bit stream start - and lane 0 assigns every block its place in the literal
//                      and sequence arenas and notes which earlier block holds the Huffman tree (treeless literals) and the FSE
//                      tables (Repeat mode) in force.
//   zb_decode_kernel   one workgroup (two waves) per block, all blocks of all chunks at once.  Wave 1 decodes the literals, wave 0
//                      the sequences - through the same stage helpers as zstd_dec.hip (zstd_dec_dev.h: 11-bit multi-symbol Huffman
//                      table, the three FSE state machines in lanes 0-2, field extraction on all lanes) - but a block that inherits a tree or a table rebuilds
//                      it from the earlier block's bytes, and repeat offsets are resolved SYMBOLICALLY: a block does not know the
//                      history it starts from, so an offset that comes out of the history is recorded as "incoming entry i minus d"
//                      and the block's outgoing history is a function of the incoming one.
//   zb_scatter_kernel  one workgroup (8 waves) per block.  Chains the block summaries up to its own block (output position = sum of the
//                      regenerated sizes before it, incoming history = composition of the outgoing ones: O(1) per block), shares the
//                      block's groups of 64 sequences out over its waves and writes ONE WORD PER OUTPUT BYTE: the byte itself for a
//                      literal, the position it copies from for a match byte.
//   zb_jump_kernel     <= log3(size) + 1 passes of pointer jumping (two jumps each, in place: three hops guaranteed) over those words: "where I copy from" becomes "where that copies from"
//                      until every word is a literal - the execution stage without any order between sequences, blocks or
//                      workgroups (in-order execution is ONE dependency chain through the whole chunk: see the comment there).
//   zb_emit_kernel     words -> bytes.  A frame with a content checksum is verified here: the emit workgroups of its chunk count themselves
//                      when their bytes are out, and the last one hashes the chunk on one wave (xxh64_dev.h) - no launch of its own, nothing
//                      at all for a frame without a checksum.
//
// This form is a fast path, not a second authority: anything it does not like (more than 264 blocks, a chunk above 16 MiB, a
// malformed frame, an offset out of range, a copy chain that does not end in a literal, restored bytes that do not match the frame's checksum) clears the chunk's `mode` word and zstd_decompress_kernel - which
// is launched behind it with that word as its skip list - decodes the chunk and reports the error code.  Bytes are either final
// and correct or rewritten by the fallback.  Both forms parse frame bytes through the same helpers (zstd_dec_dev.h, dec_*), so
// they read every frame alike; this file adds only the limits of its own (ZB_MAX_BLOCKS, ZB_MAX_CHUNK, raw / RLE blocks of at most
// Block_Maximum_Size, offsets below 2^31, the per-block regenerated sizes), each of which hands the chunk back.
#include "zstd_dec_dev.h"
#include "zstd_dec_blocks.h"
#ifdef ZB_DEBUG
#include <stdio.h>
#endif

#define ZB_SYM 0x80000000u                      /* a history-relative offset: ZB_SYM | entry << 28 | decrement */
#define ZB_SYM_ENTRY(v) (((v) >> 28) & 7u)
#define ZB_SYM_DEC(v) ((v) & 0x0FFFFFFFu)

#ifdef HIPEMU
#define ZB_LOAD_AGENT(p) (*(volatile const uint32_t*)(p))
#define ZB_STORE_AGENT(p, v) do { *(volatile uint32_t*)(p) = (v); } while (0)
#else
#define ZB_LOAD_AGENT(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define ZB_STORE_AGENT(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#endif

__device__ static inline uint32_t zb_sym_dec(uint32_t v) { return (v & ZB_SYM) ? v + 1 : v - 1; }     // "rep0 - 1" on either kind of value
__device__ static inline uint32_t zb_subst(uint32_t v, uint32_t h0, uint32_t h1, uint32_t h2) {        // a recorded offset given the incoming history
    if (!(v & ZB_SYM)) return v;
    const uint32_t e = ZB_SYM_ENTRY(v), r = e == 0 ? h0 : e == 1 ? h1 : h2;
    return r - ZB_SYM_DEC(v);                                           // 0 or wrapped when the frame is corrupt: caught where it is used
}

// A chunk's arena: literals | literal lengths | match lengths | offsets (seq_cap words each) | one word per output byte (the decoder
// only: zb_arena_stride and zb_verify_stride differ by that array)
__host__ __device__ static inline size_t zb_arena_words_at(uint32_t lit_cap, uint32_t seq_cap) { return (size_t)lit_cap + 12u * (size_t)seq_cap; }
struct ZbArena { uint8_t* lit; uint32_t* seq; uint32_t* words; };
__device__ static inline ZbArena zb_arena(uint8_t* arenas, uint32_t chunk, uint64_t astride, uint32_t lit_cap, uint32_t seq_cap) {
    uint8_t* const base = arenas + (size_t)chunk * astride;
    return ZbArena{base, (uint32_t*)(base + lit_cap), (uint32_t*)(base + zb_arena_words_at(lit_cap, seq_cap))};
}

// ---------------------------------------------------------------------------------------------------
// index: one wave per chunk
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LANES) void zb_index_kernel(const uint8_t* __restrict__ frames, int from_mid, uint64_t mid_stride,
                                                         const tsx_chunk_desc* __restrict__ descs, const int32_t* __restrict__ status,
                                                         uint8_t* __restrict__ hdrs, uint32_t lit_cap, uint32_t seq_cap) {
    __shared__ uint32_t sOff[ZB_MAX_BLOCKS], sSize[ZB_MAX_BLOCKS];
    __shared__ uint8_t sType[ZB_MAX_BLOCKS];
    __shared__ uint32_t sN, sBad;
    const uint32_t lane = threadIdx.x, chunk = blockIdx.x;
    ZbChunk* const C = (ZbChunk*)(hdrs + (size_t)chunk * ZB_CHUNK_HDR_BYTES);
    if (lane < 32) C->live[lane] = 0;
    if (lane == 0) { C->emitDone = 0; C->hasCksum = 0; }
    if (lane == 0) C->mode = 0;                                       // "not taken" until the last line of this kernel says otherwise (no memset launch: nothing
                                                                      // else of the header is read before this kernel has written it)
    if (status[chunk] != TSX_OK) return;                              // nothing to decode, nothing to fall back to
    const tsx_chunk_desc d = descs[chunk];
    const uint8_t* __restrict__ src = from_mid ? frames + (uint64_t)chunk * mid_stride : frames + d.src_off;
    const uint32_t srcSize = from_mid ? (d.src_len >= 28 ? d.src_len - 28 : 0) : d.src_len;
    if (lane == 0) {
        // every early return below leaves mode = 0: the chunk-serial kernel decodes the chunk (and owns the error codes)
        uint32_t n = 0, bad = 1;
        do {
            if (d.dst_cap > ZB_MAX_CHUNK) break;
            const DecFrame fh = dec_frame_header(src, srcSize);
            if (fh.status != TSX_OK || fh.contentSize > d.dst_cap) break;
            C->contentSize = (uint32_t)fh.contentSize;
            uint32_t p = fh.p;
            bool closed = false;
            while (n < ZB_MAX_BLOCKS) {                                 // the chain of block headers
                const DecBlockHdr bh = dec_block_header(src, srcSize, p);
                if (!bh.ok) break;
                if (bh.btype != 2 && bh.bsize > ZS_BLOCK_MAX) break;   // a raw / RLE block regenerates Block_Size bytes: <= Block_Maximum_Size
                sOff[n] = bh.off; sSize[n] = bh.bsize; sType[n] = (uint8_t)(bh.btype | (bh.last << 2));
                n++; p = bh.next;
                if (bh.last) { closed = dec_frame_end(p, srcSize, fh.hasChecksum); break; }
            }
            if (closed && fh.hasChecksum) {
                if (fh.contentSize == 0) break;                         // no byte, no emit wave to check it: the chunk-serial kernel does
                C->cksum = dec_checksum_at(src, p); C->hasCksum = 1;
            }
            if (closed) bad = 0;
        } while (0);
        sN = n; sBad = bad;
    }
    __syncthreads();
    const uint32_t n = sN;
    if (sBad) return;
    // ---- one lane per block: the section headers ----
    for (uint32_t b = lane; b < n; b += LANES) {
        ZbBlock B;
        B.off = sOff[b]; B.bsize = sSize[b]; B.btype = sType[b] & 3; B.last = sType[b] >> 2; B.ltype = 0; B.modes = 0;
        B.litSize = 0; B.q = 0; B.nbSeq = 0; B.litAt = 0; B.seqAt = 0; B.hufSrc = 0xFFFF; B.tblSrc[0] = B.tblSrc[1] = B.tblSrc[2] = 0xFFFF;
        B.tOff[0] = B.tOff[1] = B.tOff[2] = 0; B.streamOff = 0; B.regen = B.btype == 2 ? 0 : B.bsize; B.endHist[0] = B.endHist[1] = B.endHist[2] = 0; B.ok = 0;
        bool bad = false;
        if (B.btype == 2) {
            const uint8_t* const blk = src + B.off;
            const DecLit h = dec_lit_header(blk, B.bsize);
            const DecSeqHdr sh = h.section ? dec_seq_header(blk, B.bsize, h.section) : DecSeqHdr{0, 0, 0, 0};
            if (!sh.ok) bad = true;
            else {
                B.ltype = (uint8_t)h.ltype; B.litSize = h.litSize; B.q = h.section; B.nbSeq = sh.nbSeq; B.modes = (uint8_t)sh.modes;
                if (sh.nbSeq) {
                    // where each table description defined here starts, and the bit stream behind them (the tables themselves are
                    // built by the decode kernel).  Unrolled: B stays in registers - a dynamic index into B.tOff would put the whole
                    // struct into scratch, and no kernel on the fetch path may use scratch: see zstd_dec.hip, zstd_decompress_fallback_kernel
                    uint32_t t = sh.t;
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        if (bad) continue;
                        const uint32_t mode = (sh.modes >> (6 - 2 * k)) & 3;
                        const uint32_t maxSymK = k == 0 ? 35 : k == 1 ? 31 : 52, maxLogK = k == 0 ? 9 : k == 1 ? 8 : 9;
                        B.tOff[k] = t;
                        if (mode == 1) { if (t >= B.bsize) bad = true; t++; }
                        else if (mode == 2) {
                            if (t >= B.bsize) { bad = true; continue; }
                            const uint32_t used = fse_skipNCount(maxSymK, blk + t, B.bsize - t, maxLogK);
                            if (!used) bad = true;
                            t += used;
                        }
                    }
                    if (!bad && t >= B.bsize) bad = true;
                    B.streamOff = t;
                }
            }
        }
        if (bad) sBad = 1;                                             // (any lane: same value)
        C->blk[b] = B;
    }
    __threadfence_block();
    __syncthreads();
    if (sBad) return;
    // ---- lane 0: arenas, inheritance ----
    if (lane == 0) {
        uint32_t litAt = 0, seqAt = 0, huf = 0xFFFF, tb[3] = {0xFFFF, 0xFFFF, 0xFFFF};
        bool bad = false;
        for (uint32_t b = 0; b < n && !bad; b++) {
            ZbBlock* const B = &C->blk[b];
            if (B->btype != 2) continue;
            if (B->ltype == 2) huf = b;
            if (B->ltype == 3) { if (huf == 0xFFFF) bad = true; B->hufSrc = (uint16_t)huf; }
            if (B->ltype != 0) { B->litAt = litAt; litAt += (B->litSize + 64 + 15) & ~15u; }
            if (litAt > lit_cap) bad = true;
            if (B->nbSeq) {
                for (int k = 0; k < 3; k++) {
                    const uint32_t mode = (B->modes >> (6 - 2 * k)) & 3;
                    if (mode != 3) tb[k] = b; else if (tb[k] == 0xFFFF) bad = true;
                    B->tblSrc[k] = (uint16_t)tb[k];
                }
                B->seqAt = seqAt; seqAt += (B->nbSeq + 63) & ~63u;
                if (seqAt > seq_cap) bad = true;
            }
        }
        if (!bad) { C->nblocks = n; __threadfence(); C->mode = 1; }
    }
}

// ---------------------------------------------------------------------------------------------------
// decode: one workgroup (wave 0 sequences, wave 1 literals) per block
// ---------------------------------------------------------------------------------------------------
#define ZB_FAIL() do { if (lane == 0) ZB_STORE_AGENT(&C->mode, 0u); return; } while (0)
static DecLapOut g_zbprof_out;                                        // 8 u64 per (chunk, block): phase laps of zb_decode_kernel (tools/zb_phase_laps.py)
#ifdef TSX_PROF2
extern "C" void tsx_debug_set_zbprof(void* dev_ptr) { g_zbprof_out.buf = (unsigned long long*)dev_ptr; }
#endif

__global__ __launch_bounds__(2 * LANES) void zb_decode_kernel(const uint8_t* __restrict__ frames, int from_mid, uint64_t mid_stride,
                                                              const tsx_chunk_desc* __restrict__ descs, uint8_t* __restrict__ hdrs, uint8_t* __restrict__ arenas,
                                                              uint64_t astride, uint32_t lit_cap, uint32_t seq_cap, DecLapOut zbprof) {
    __shared__ DecLds L;
    const uint32_t lane = threadIdx.x & (LANES - 1), role = DUNI(threadIdx.x >> 6), b = blockIdx.x, chunk = blockIdx.y;
    DecLaps laps;
    const size_t lapRow = (size_t)chunk * ZB_MAX_BLOCKS + b;
    ZbChunk* const C = (ZbChunk*)(hdrs + (size_t)chunk * ZB_CHUNK_HDR_BYTES);
    if (DUNI(C->mode) != 1 || b >= DUNI(C->nblocks)) return;
    ZbBlock* const B = &C->blk[b];
    if (DUNI(B->btype) != 2) return;
    const tsx_chunk_desc d = descs[chunk];
    const uint8_t* __restrict__ src = from_mid ? frames + (uint64_t)chunk * mid_stride : frames + d.src_off;
    const ZbArena A = zb_arena(arenas, chunk, astride, lit_cap, seq_cap);
    const uint8_t* const blk = src + DUNI(B->off);
    const uint32_t bsize = DUNI(B->bsize);
    if (role == 1) {
        // ---- literals ----
        const DecLit h = dec_lit_header(blk, bsize);                      // (validated by the index kernel)
        if (h.ltype == 0) return;                                       // raw literals are read in place
        uint8_t* const lit = A.lit + DUNI(B->litAt);
        if (h.ltype == 1) { const uint8_t v = blk[h.hl]; for (uint32_t i = lane; i < h.litSize; i += LANES) lit[i] = v; return; }
        uint32_t t = h.hl;
        const uint8_t* tree = blk + h.hl; uint32_t treeAvail = h.csize;
        if (h.ltype == 3) {                                             // treeless: the tree of the latest block that carried one
            const ZbBlock* const S = &C->blk[DUNI(B->hufSrc)];
            const uint8_t* const sblk = src + DUNI(S->off);
            const DecLit sh = dec_lit_header(sblk, DUNI(S->bsize));
            if (sh.ltype != 2 || !sh.section) ZB_FAIL();
            tree = sblk + sh.hl; treeAvail = sh.csize;
        }
        const uint32_t used = dec_huf_tree(L, tree, treeAvail, lane);
        if (!used) ZB_FAIL();
        laps.lap(6);
        if (h.ltype == 2) t += used;
        if (t > h.hl + h.csize) ZB_FAIL();
        if (!dec_huf_streams(L, blk + t, h.hl + h.csize - t, h.streams, h.litSize, lit, lane)) ZB_FAIL();
        laps.lap(7);
        if (lane == 0) { laps.put(zbprof, lapRow, 6, 6); laps.put(zbprof, lapRow, 7, 7); }
        return;
    }
    // ---- sequences ----
    const uint32_t nbSeq = DUNI(B->nbSeq), litSize = DUNI(B->litSize);
    if (nbSeq == 0) { if (lane == 0) { B->regen = litSize; B->endHist[0] = ZB_SYM; B->endHist[1] = ZB_SYM | (1u << 28); B->endHist[2] = ZB_SYM | (2u << 28); B->ok = 1; } return; }
    dec_code_tables(L, lane);
    WAVE_SYNC();
    for (int k = 0; k < 3; k++) {
        const ZbBlock* const S = &C->blk[DUNI(B->tblSrc[k])];           // this block itself unless the table is a Repeat
        const uint32_t mode = (DUNI(S->modes) >> (6 - 2 * k)) & 3, to = DUNI(S->tOff[k]), sb = DUNI(S->bsize);
        if (mode == 3 || to > sb) ZB_FAIL();
        if (dec_seq_table(L, k, mode, src + DUNI(S->off) + to, sb - to, lane) < 0) ZB_FAIL();
    }
    laps.lap(0);
    uint32_t* const sLL = A.seq + DUNI(B->seqAt); uint32_t* const sML = sLL + seq_cap; uint32_t* const sOF = sML + seq_cap;
    const uint32_t t = DUNI(B->streamOff);
    DecSeqStream stream = {blk + t, bsize - t, 0, 0, 0};                // n >= 1 (index kernel)
    uint32_t r0 = ZB_SYM, r1 = ZB_SYM | (1u << 28), r2 = ZB_SYM | (2u << 28);      // the history this block starts from, whatever it is
    uint32_t sumLL = 0, sumML = 0;
    for (uint32_t g = 0; g < nbSeq; g += LANES) {
        const uint32_t cnt = DUNI(nbSeq - g < LANES ? nbSeq - g : LANES);
        uint32_t ll, ml, offBase;
        if (!dec_seq_group(L, stream, g, cnt, nbSeq, lane, ll, ml, offBase)) ZB_FAIL();
        const bool valid = lane < cnt;
        laps.lap(1);
        if (__any(valid && offBase > 3 && offBase - 3 >= ZB_SYM)) ZB_FAIL();     // an offset of 2 GiB or more: not in a frame this form takes
        // pass 3: repeat offsets, on values that are either offsets or references into the incoming history
        const uint32_t off = dec_rep_offsets(offBase, ll, valid, cnt, r0, r1, r2, [](uint32_t v) { return zb_sym_dec(v); });
        laps.lap(4);
        if (valid) { sLL[g + lane] = ll; sML[g + lane] = ml; sOF[g + lane] = off; }
        uint32_t a = ll, m = ml;
        for (int o = 32; o; o >>= 1) { a += __shfl_xor(a, o); m += __shfl_xor(m, o); }
        sumLL += DUNI(a); sumML += DUNI(m);
        if (sumLL > litSize || litSize + sumML > ZS_BLOCK_MAX) ZB_FAIL();   // a block regenerates at most Block_Maximum_Size bytes
        laps.lap(5);
    }
    if (lane == 0) for (int k = 0; k < 6; k++) laps.put(zbprof, lapRow, k, k);
    if (stream.B != 0) ZB_FAIL();                                       // every bit of the stream was used
    if (lane == 0) { B->regen = litSize + sumML; B->endHist[0] = r0; B->endHist[1] = r1; B->endHist[2] = r2; B->ok = 1; }
}

// ---------------------------------------------------------------------------------------------------
// execution by pointer jumping: scatter -> ceil(log3(size)) + 1 jump passes -> emit
//
// Executing sequences in order is a dependency chain through the whole chunk: in log-like content every record copies its field
// names from the record before it (offset ~ one record), so byte p of record r is a copy of a copy ... of record 0 - the first
// sequences of a block read the last bytes of the block before it, and 32 blocks "side by side" still run one after the other
// (measured: 24 ms per chunk with cross-block waits against 33 ms for the chunk-serial kernel).  What breaks the chain is not
// order but TRANSITIVITY: give every output byte a word - the byte itself when it is a literal, else the position it copies
// from (p - offset, always < p) - and replace "where I copy from" by "where THAT copies from" until every word is a literal:
// pointer jumping, two jumps per pass = three hops guaranteed (zb_jump_kernel): ceil(log3(chain depth)) + 1 <= ceil(log3(size)) + 1
// passes, all bytes of all blocks at once, no ordering between workgroups at all (a word read while another thread replaces it
// holds either ancestor - both are valid - so the update is done in place).
// ---------------------------------------------------------------------------------------------------
#define ZB_LIT 0x80000000u                      /* src word: ZB_LIT | byte (resolved), else the chunk position this byte copies from */

// ---- the block walk: what zb_scatter_kernel and zb_verify_kernel share ----
// One workgroup of ZB_SC_WAVES waves per block.  Every wave walks the block summaries (positions, incoming repeat-offset history:
// O(1) per block, wave-uniform), the waves share out the block's groups of 64 sequences: a first sweep leaves every group's literal
// and output byte counts in LDS, their prefix sums place the groups, and then every group is walked on its own - every output byte
// goes to the kernel's functor once.  (One wave per block took 0.9 ms of a single chunk's 2.7 ms: ~85 groups one after the other, each
// behind its own loads - profiles/r03_dec_single_chunk_kernel_stats.txt.)  Both helpers are entered and left by whole workgroups.
#define ZB_SC_WAVES 8u
#define ZB_SC_GROUPS ((ZS_BLOCK_MAX / 3u + LANES - 1) / LANES + 1)      /* a sequence regenerates >= 3 bytes, a block <= 128 KiB */
struct ZbWalkLds {
    uint32_t regen[ZB_MAX_BLOCKS];                                      // regenerated size of every block
    uint32_t hist[3][ZB_MAX_BLOCKS];                                    // outgoing history of every block (symbolic in its incoming one)
    uint8_t flag[ZB_MAX_BLOCKS];                                        // 1 compressed, 2 decoded fine, 4 has sequences
    uint32_t lit[ZB_SC_GROUPS + 1], tot[ZB_SC_GROUPS + 1];              // per group of 64 sequences: literal / output bytes, then their exclusive prefixes
    uint32_t gStart[ZB_SC_WAVES][LANES + 1], gLL[ZB_SC_WAVES][LANES], gLit[ZB_SC_WAVES][LANES], gSrc[ZB_SC_WAVES][LANES];   // the group a wave is walking
};
struct ZbWalk {
    uint32_t h0, h1, h2, start, regen, total;                           // the history block b starts from, its first output position and size, the sum over all blocks
    bool ok;                                                            // every compressed block was decoded and the sum stays within ZB_MAX_CHUNK
};
// block summaries into LDS, barrier, the walk to block b (wave-uniform; every wave for itself; every workgroup of the chunk sees the same sums)
__device__ __forceinline__ static ZbWalk zb_walk_to(ZbWalkLds& L, const ZbChunk* C, uint32_t nb, uint32_t b, uint32_t tid) {
    for (uint32_t i = tid; i < nb; i += ZB_SC_WAVES * LANES) {
        const ZbBlock* const S = &C->blk[i];
        L.regen[i] = S->regen;
        L.hist[0][i] = S->endHist[0]; L.hist[1][i] = S->endHist[1]; L.hist[2][i] = S->endHist[2];
        L.flag[i] = (uint8_t)((S->btype == 2 ? 1 : 0) | (S->ok ? 2 : 0) | (S->nbSeq ? 4 : 0));
    }
    __threadfence_block();
    __syncthreads();
    ZbWalk w = {1, 4, 8, 0, 0, 0, true};
    for (uint32_t i = 0; i < nb; i++) {                                 // O(1) per block
        const uint32_t rg = DUNI(L.regen[i]), fl = DUNI(L.flag[i]);
        if (i == b) { w.start = w.total; w.regen = rg; }
        if (fl & 1) {
            if (!(fl & 2)) w.ok = false;
            if (i < b && (fl & 4)) {
                const uint32_t e0 = DUNI(L.hist[0][i]), e1 = DUNI(L.hist[1][i]), e2 = DUNI(L.hist[2][i]);
                const uint32_t n0 = zb_subst(e0, w.h0, w.h1, w.h2), n1 = zb_subst(e1, w.h0, w.h1, w.h2), n2 = zb_subst(e2, w.h0, w.h1, w.h2);
                w.h0 = n0; w.h1 = n1; w.h2 = n2;
            }
        }
        w.total += rg;
        if (w.total > ZB_MAX_CHUNK) { w.ok = false; break; }
    }
    return w;
}
// A compressed block: f(p, isLiteral, v) once for every output position p of [w.start, w.start + w.regen) - v is the byte when it is
// a literal, else the chunk position it copies from (< p).  ZB_WALK_SUMS: the sequences' sums do not fit the block (the decode kernel
// has checked them: cannot happen) - workgroup-uniform, returned before any byte.  ZB_WALK_REACH: a match of one of this wave's groups
// starts before the chunk does - wave-uniform; the wave has left its other groups out and done its share of the trailing literals.
enum : uint32_t { ZB_WALK_OK, ZB_WALK_SUMS, ZB_WALK_REACH };
template <class F>
__device__ __forceinline__ static uint32_t zb_walk_block(ZbWalkLds& L, const ZbBlock* B, const uint8_t* __restrict__ src, const ZbArena& A, uint32_t seq_cap,
                                                         const ZbWalk& w, uint32_t tid, F f) {
    const uint32_t lane = tid & (LANES - 1), wv = DUNI(tid >> 6), boff = DUNI(B->off);
    const uint32_t litSize = DUNI(B->litSize), nbSeq = DUNI(B->nbSeq);
    const uint8_t* litPtr = A.lit + DUNI(B->litAt);
    if (DUNI(B->ltype) == 0) { const DecLit h = dec_lit_header(src + boff, DUNI(B->bsize)); litPtr = src + boff + h.hl; }
    const uint32_t* const sLL = A.seq + DUNI(B->seqAt); const uint32_t* const sML = sLL + seq_cap; const uint32_t* const sOF = sML + seq_cap;
    const uint32_t ngroups = (nbSeq + LANES - 1) / LANES;
    if (ngroups > ZB_SC_GROUPS) return ZB_WALK_SUMS;                    // (the decode kernel bounds the match lengths' sum)
    // sweep 1: the groups' byte counts
    for (uint32_t gi = wv; gi < ngroups; gi += ZB_SC_WAVES) {
        const uint32_t q = gi * LANES + lane;
        uint32_t a = q < nbSeq ? sLL[q] : 0, t = q < nbSeq ? a + sML[q] : 0;
        for (int o = 32; o; o >>= 1) { a += __shfl_xor(a, o); t += __shfl_xor(t, o); }
        if (lane == 0) { L.lit[gi] = a; L.tot[gi] = t; }
    }
    __threadfence_block();
    __syncthreads();
    if (wv == 0) {                                                       // exclusive prefixes, 64 groups per step
        uint32_t cl = 0, ct = 0;
        for (uint32_t g0 = 0; g0 <= ngroups; g0 += LANES) {
            const uint32_t gi = g0 + lane;
            const uint32_t a = gi < ngroups ? L.lit[gi] : 0, t = gi < ngroups ? L.tot[gi] : 0;
            uint32_t ia = a, it = t;
            dec_incl_scan2(ia, it, lane);
            if (gi <= ngroups) { L.lit[gi] = cl + ia - a; L.tot[gi] = ct + it - t; }
            cl += (uint32_t)__builtin_amdgcn_readlane(ia, LANES - 1); ct += (uint32_t)__builtin_amdgcn_readlane(it, LANES - 1);
        }
    }
    __threadfence_block();
    __syncthreads();
    const uint32_t allLit = DUNI(L.lit[ngroups]), allTot = DUNI(L.tot[ngroups]);
    if (allLit > litSize || allTot + (litSize - allLit) != w.regen) return ZB_WALK_SUMS;
    // sweep 2: every group on its own
    uint32_t res = ZB_WALK_OK;
    for (uint32_t gi = wv; gi < ngroups; gi += ZB_SC_WAVES) {
        const uint32_t g = gi * LANES;
        const uint32_t cnt = nbSeq - g < LANES ? nbSeq - g : LANES;
        const uint32_t lp = DUNI(L.lit[gi]), opos = w.start + DUNI(L.tot[gi]), groupTot = DUNI(L.tot[gi + 1]) - DUNI(L.tot[gi]);
        const bool valid = lane < cnt;
        const uint32_t ll = valid ? sLL[g + lane] : 0, ml = valid ? sML[g + lane] : 0;
        uint32_t off = valid ? sOF[g + lane] : 0;
        if (off & ZB_SYM) off = zb_subst(off, w.h0, w.h1, w.h2);
        uint32_t litIncl = ll, totIncl = ll + ml;
        dec_incl_scan2(litIncl, totIncl, lane);
        const uint32_t myLit = lp + litIncl - ll, myOut = opos + totIncl - (ll + ml), mOut = myOut + ll;
        if (__any(valid && ml && (off == 0 || off > mOut))) { res = ZB_WALK_REACH; break; }
        // the group's ~1.5 KB of output, all lanes side by side: position -> its sequence by a binary search over the 64 start
        // positions (a lane walking its own run would serialise a 100 KB match on one lane)
        WAVE_SYNC();
        L.gStart[wv][lane] = valid ? myOut : opos + groupTot; L.gLL[wv][lane] = ll; L.gLit[wv][lane] = myLit; L.gSrc[wv][lane] = mOut - off;
        if (lane == 0) L.gStart[wv][LANES] = opos + groupTot;
        __threadfence_block();
        WAVE_SYNC();
        for (uint32_t p = opos + lane; p < opos + groupTot; p += LANES) {
            uint32_t i = 0;
            for (uint32_t s_ = 32; s_; s_ >>= 1) if (L.gStart[wv][i + s_] <= p) i += s_;     // the last sequence that starts at or before p
            const uint32_t rel = p - L.gStart[wv][i], l_ = L.gLL[wv][i]; const bool isLit = rel < l_;
            f(p, isLit, isLit ? (uint32_t)litPtr[L.gLit[wv][i] + rel] : L.gSrc[wv][i] + (rel - l_));
        }
    }
    // the literals behind the last sequence
    for (uint32_t k = tid; k < litSize - allLit; k += ZB_SC_WAVES * LANES) f(w.start + allTot + k, true, (uint32_t)litPtr[allLit + k]);
    return res;
}

// scatter: ONE WORD PER OUTPUT BYTE - the byte itself for a literal, the position it copies from for a match byte
__global__ __launch_bounds__(ZB_SC_WAVES * LANES) void zb_scatter_kernel(const uint8_t* __restrict__ frames, int from_mid, uint64_t mid_stride,
                                                                         tsx_chunk_desc* __restrict__ descs, uint8_t* __restrict__ hdrs, uint8_t* __restrict__ arenas,
                                                                         uint64_t astride, uint32_t lit_cap, uint32_t seq_cap) {
    __shared__ ZbWalkLds L;
    __shared__ uint32_t sFail;
    const uint32_t tid = threadIdx.x, lane = tid & (LANES - 1), b = blockIdx.x, chunk = blockIdx.y;
    ZbChunk* const C = (ZbChunk*)(hdrs + (size_t)chunk * ZB_CHUNK_HDR_BYTES);
    if (DUNI(ZB_LOAD_AGENT(&C->mode)) != 1) return;
    const uint32_t nb = DUNI(C->nblocks);
    if (b >= nb) return;
    const tsx_chunk_desc d = descs[chunk];
    const uint8_t* __restrict__ src = from_mid ? frames + (uint64_t)chunk * mid_stride : frames + d.src_off;
    const ZbArena A = zb_arena(arenas, chunk, astride, lit_cap, seq_cap);
    uint32_t* const words = A.words;
    if (tid == 0) sFail = 0;
    const ZbWalk w = zb_walk_to(L, C, nb, b, tid);
    const uint32_t contentSize = DUNI(C->contentSize);
    if (!w.ok || w.total != contentSize) { if (tid == 0) ZB_STORE_AGENT(&C->mode, 0u); return; }
    const ZbBlock* const B = &C->blk[b];
    const uint32_t btype = DUNI(B->btype), boff = DUNI(B->off);
    if (b == 0 && tid == 0) descs[chunk].dst_len = contentSize;
    if (btype == 0) { for (uint32_t i = tid; i < w.regen; i += ZB_SC_WAVES * LANES) words[w.start + i] = ZB_LIT | src[boff + i]; return; }
    if (btype == 1) { const uint32_t v = ZB_LIT | src[boff]; for (uint32_t i = tid; i < w.regen; i += ZB_SC_WAVES * LANES) words[w.start + i] = v; return; }
    const uint32_t res = zb_walk_block(L, B, src, A, seq_cap, w, tid, [words](uint32_t p, bool isLit, uint32_t v) { words[p] = isLit ? (ZB_LIT | v) : v; });
    if (res == ZB_WALK_SUMS) { if (tid == 0) ZB_STORE_AGENT(&C->mode, 0u); return; }
    if (res == ZB_WALK_REACH && lane == 0) sFail = 1;
    __threadfence_block();
    __syncthreads();
    if (tid == 0 && sFail) ZB_STORE_AGENT(&C->mode, 0u);                // the chunk-serial kernel behind this launch redoes the chunk
}

// ---------------------------------------------------------------------------------------------------
// verify on upload: a frame the compressor has just written, against the chunk it was written from
//
// When the expected output is known, nothing has to be executed: the frame restores orig[0, n) exactly if its content size is n and,
// for every output position p, a literal byte equals orig[p] and a match byte satisfies orig[p - offset] == orig[p] - by induction
// on p (the bytes before p are orig's, so the byte a match copies IS orig[p - offset]) that is byte equality of the restored chunk.
// No order between sequences, blocks or workgroups, no word per output byte, no jump passes, no emit: this kernel runs behind
// zb_index_kernel and zb_decode_kernel in place of zb_scatter_kernel, with that kernel's geometry and ITS WALK (zb_walk_to,
// zb_walk_block: a verdict is worth what its agreement with the reader's walk is, so there is one) - and where scatter stores
// words[p], it compares.
//
// descs[i] describes FRAME i to the two kernels in front (src_len = frame bytes + 28, read with from_mid = 1; dst_cap = the source
// chunk's length) and says where the source chunk is: src_base + dst_off.  status[i] != 0: chunk i is not verified.
// verdicts: ZB_VERDICT_WORDS words per chunk, zero before the launch, in memory the host reads (plain stores; every writer of a word
// stores the same value):
//   [ZB_V_FAIL]      the frame does not restore the chunk: a byte differs, an offset reaches before the chunk's first byte, the
//                    content size is not the chunk's length, or the content checksum is not the SOURCE chunk's
//   [ZB_V_NOT_TAKEN] the block form has no opinion (its own limits, or a frame it does not parse): the caller decodes the frame in full
//   [ZB_V_SEEN]      the workgroup of block 0 got past the prologue: without it (and without the other two) nothing looked at the chunk
// A frame of an EMPTY chunk with a content checksum is one the index kernel leaves to the chunk-serial form (no emit wave would check
// it); there is no byte to compare, so the first wave checks here that the frame regenerates nothing and carries the empty input's hash.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ZB_SC_WAVES * LANES) void zb_verify_kernel(const uint8_t* __restrict__ frames, uint64_t mid_stride,
                                                                        const tsx_chunk_desc* __restrict__ descs, const int32_t* __restrict__ status,
                                                                        const uint8_t* __restrict__ src_base, uint8_t* __restrict__ hdrs, uint8_t* __restrict__ arenas,
                                                                        uint64_t astride, uint32_t lit_cap, uint32_t seq_cap, uint32_t* __restrict__ verdicts) {
    __shared__ ZbWalkLds L;
    const uint32_t tid = threadIdx.x, lane = tid & (LANES - 1), wv = DUNI(tid >> 6), b = blockIdx.x, chunk = blockIdx.y;
    if (status[chunk] != TSX_OK) return;
    ZbChunk* const C = (ZbChunk*)(hdrs + (size_t)chunk * ZB_CHUNK_HDR_BYTES);
    uint32_t* const V = verdicts + (size_t)chunk * ZB_VERDICT_WORDS;
    const tsx_chunk_desc d = descs[chunk];
    const uint8_t* __restrict__ src = frames + (uint64_t)chunk * mid_stride;
    const uint8_t* __restrict__ orig = src_base + d.dst_off;
    const uint32_t origLen = d.dst_cap;
#define ZV_FAIL() do { if (lane == 0) V[ZB_V_FAIL] = 1; } while (0)
#define ZV_NOT_TAKEN() do { if (lane == 0) V[ZB_V_NOT_TAKEN] = 1; } while (0)
    if (DUNI(ZB_LOAD_AGENT(&C->mode)) != 1) {
        if (b != 0 || wv != 0) return;
        if (origLen != 0) { ZV_NOT_TAKEN(); return; }
        const uint32_t srcSize = d.src_len >= 28 ? d.src_len - 28 : 0;
        const DecFrame fh = dec_frame_header(src, srcSize);
        if (fh.status != TSX_OK) { ZV_NOT_TAKEN(); return; }
        if (fh.contentSize != 0) { ZV_FAIL(); return; }
        uint32_t p = fh.p;
        for (uint32_t k = 0; k < ZB_MAX_BLOCKS; k++) {
            const DecBlockHdr bh = dec_block_header(src, srcSize, p);
            if (!bh.ok || bh.btype == 2) break;                         // (a compressed block of nothing: not ours to judge)
            if (bh.bsize != 0) { ZV_FAIL(); return; }
            p = bh.next;
            if (!bh.last) continue;
            if (!dec_frame_end(p, srcSize, fh.hasChecksum)) break;
            if (fh.hasChecksum && !dec_checksum_ok(orig, 0, dec_checksum_at(src, p), lane)) { ZV_FAIL(); return; }
            if (lane == 0) V[ZB_V_SEEN] = 1;
            return;
        }
        ZV_NOT_TAKEN();
        return;
    }
    const uint32_t nb = DUNI(C->nblocks);
    if (b >= nb) return;
    const ZbWalk w = zb_walk_to(L, C, nb, b, tid);
    // A block the decode kernel did not finish, or blocks that do not add up to the frame's own content size: a frame this form does
    // not read - not taken.  A content size that is not the chunk's length: a mismatch
    if (!w.ok || w.total != DUNI(C->contentSize)) { if (b == 0 && wv == 0) ZV_NOT_TAKEN(); return; }
    if (w.total != origLen) { if (b == 0 && wv == 0) ZV_FAIL(); return; }
    if (b == 0 && tid == 0) V[ZB_V_SEEN] = 1;
    // every position below is < origLen: the block's bytes are [w.start, w.start + w.regen) of a sum that equals it
    const ZbBlock* const B = &C->blk[b];
    const uint32_t btype = DUNI(B->btype), boff = DUNI(B->off);
    bool diff = false;
    if (btype == 0) { for (uint32_t i = tid; i < w.regen; i += ZB_SC_WAVES * LANES) diff |= orig[w.start + i] != src[boff + i]; }
    else if (btype == 1) { const uint8_t v = src[boff]; for (uint32_t i = tid; i < w.regen; i += ZB_SC_WAVES * LANES) diff |= orig[w.start + i] != v; }
    else {
        const uint32_t res = zb_walk_block(L, B, src, zb_arena(arenas, chunk, astride, lit_cap, seq_cap), seq_cap, w, tid,
                                           [orig, &diff](uint32_t p, bool isLit, uint32_t v) { diff |= orig[p] != (isLit ? (uint8_t)v : orig[v]); });
        if (res == ZB_WALK_SUMS) { if (wv == 0) ZV_NOT_TAKEN(); return; }
        diff |= res == ZB_WALK_REACH;                                   // a match that starts before the chunk does: restores nothing
    }
    if (__any(diff)) ZV_FAIL();
    // Four wrong checksum bytes make a chunk unreadable to every reader: the last wave of the frame's last block (the short one) hashes the
    // SOURCE chunk when it is done comparing
    if (b + 1 == nb && wv == ZB_SC_WAVES - 1 && DUNI(C->hasCksum) && !dec_checksum_ok(orig, origLen, DUNI(C->cksum), lane)) ZV_FAIL();
#undef ZV_FAIL
#undef ZV_NOT_TAKEN
}

// one jump pass: every unresolved word takes its source's word, twice (four words per thread).  Chain depths are small in practice
// (log-like content: every word resolved after 7 jumps = 4 passes, its matches reach ~100 KB back, not to the previous record) while the
// launcher must queue the passes the WORST case needs (a 4 MiB chain at offset 1 or 2: three guaranteed hops per pass, 15 passes queued): a pass notes whether it left
// anything unresolved, and the passes behind one that did not return at their first instruction.
#ifdef HIPEMU
// Test harness only (tests/test_emu_zstd.py::test_jump_passes_cover_the_worst_store_order): the emulator runs a grid's threads one after
// the other, so an in-place pass sees every earlier thread's stores - the BEST order for pointer jumping.  With a snapshot every read of
// a pass sees the words as they were before it - the worst order the device can produce (three hops per pass) - and the pass bound of
// tsx_launch_zstd_decompress_blocks can be checked against it on the CPU.
static const uint8_t* g_zb_snap = nullptr;
#endif
__global__ __launch_bounds__(256) void zb_jump_kernel(uint8_t* __restrict__ hdrs, uint8_t* __restrict__ arenas, uint64_t astride, uint32_t lit_cap, uint32_t seq_cap,
                                                      uint32_t round) {
    const uint32_t chunk = blockIdx.y;
    ZbChunk* const C = (ZbChunk*)(hdrs + (size_t)chunk * ZB_CHUNK_HDR_BYTES);
    if (C->mode != 1) return;
    if (round > 0 && C->live[round - 1] == 0) return;
    const uint32_t n = C->contentSize, p = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (p >= n) return;
    uint32_t* const words = zb_arena(arenas, chunk, astride, lit_cap, seq_cap).words;
    const uint32_t* rd = words;                                         // what this pass reads (the array itself: the update is in place)
#ifdef HIPEMU
    if (g_zb_snap) rd = (const uint32_t*)(g_zb_snap + ((const uint8_t*)words - arenas));
#endif
    if (p + 4 <= n) {
        uint4 v = *reinterpret_cast<const uint4*>(rd + p);
        if ((v.x & v.y & v.z & v.w) & ZB_LIT) return;                   // all four resolved already
        // two jumps per pass: a word that is still a position after the first takes its source's word once more (a pass costs one
        // read and one write of the word array whatever it resolves)
        uint32_t a = (v.x & ZB_LIT) ? v.x : rd[v.x], b_ = (v.y & ZB_LIT) ? v.y : rd[v.y], c = (v.z & ZB_LIT) ? v.z : rd[v.z], d_ = (v.w & ZB_LIT) ? v.w : rd[v.w];
        if (!((a & b_ & c & d_) & ZB_LIT)) {
            a = (a & ZB_LIT) ? a : rd[a]; b_ = (b_ & ZB_LIT) ? b_ : rd[b_]; c = (c & ZB_LIT) ? c : rd[c]; d_ = (d_ & ZB_LIT) ? d_ : rd[d_];
        }
        v.x = a; v.y = b_; v.z = c; v.w = d_;
        *reinterpret_cast<uint4*>(words + p) = v;
        if (!((a & b_ & c & d_) & ZB_LIT) && round < 32) C->live[round] = 1;       // (every writer stores the same value)
    } else {
        for (uint32_t q = p; q < n; q++) {
            const uint32_t v = rd[q];
            if (!(v & ZB_LIT)) { uint32_t w = rd[v]; if (!(w & ZB_LIT)) w = rd[w]; words[q] = w; if (!(w & ZB_LIT) && round < 32) C->live[round] = 1; }
        }
    }
}

// words -> bytes; a word that is still a position after the last round means a corrupt chain: the chunk goes back to the fallback.
// So does a chunk whose bytes do not match its frame's content checksum.  The bytes exist only here, and nothing orders the emit
// workgroups of a chunk: every workgroup that has written bytes releases them (one device-scope fence behind its barrier) and counts
// itself in C->emitDone; the first wave of the workgroup that completes the count acquires the others' bytes and hashes the chunk on
// its own - milliseconds for 4 MiB, which a fetch of checksummed frames pays and any other fetch does not: it leaves
// before the barrier.
__global__ __launch_bounds__(256) void zb_emit_kernel(const tsx_chunk_desc* __restrict__ descs, uint8_t* __restrict__ dst_base, uint8_t* __restrict__ hdrs,
                                                      uint8_t* __restrict__ arenas, uint64_t astride, uint32_t lit_cap, uint32_t seq_cap) {
    const uint32_t chunk = blockIdx.y;
    ZbChunk* const C = (ZbChunk*)(hdrs + (size_t)chunk * ZB_CHUNK_HDR_BYTES);
    if (C->mode != 1) return;
    const uint32_t n = C->contentSize, p = (blockIdx.x * 256 + threadIdx.x) * 16, lane = threadIdx.x & (LANES - 1);
    if (p - lane * 16 >= n) return;                                     // whole waves leave: the lanes of a wave with bytes stay together for the hand-off below
    const uint32_t* const words = zb_arena(arenas, chunk, astride, lit_cap, seq_cap).words;
    uint8_t* const out = dst_base + descs[chunk].dst_off;                // slots are 16-byte aligned
    uint32_t all = ZB_LIT;
    if (p >= n) {}
    else if (p + 16 <= n) {
        uint32_t w[4];
        for (int k = 0; k < 4; k++) {
            const uint4 v = *reinterpret_cast<const uint4*>(words + p + 4 * k);
            all &= v.x & v.y & v.z & v.w;
            w[k] = (v.x & 0xFF) | (v.y & 0xFF) << 8 | (v.z & 0xFF) << 16 | (v.w & 0xFF) << 24;
        }
        *reinterpret_cast<uint4*>(out + p) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (uint32_t q = p; q < n; q++) { const uint32_t v = words[q]; all &= v; out[q] = (uint8_t)v; }
    }
    if (!(all & ZB_LIT)) ZB_STORE_AGENT(&C->mode, 0u);
    if (!DUNI(C->hasCksum)) return;
    __syncthreads();                                                    // (waves that have left are not waited for) the workgroup's bytes are written ...
    if (threadIdx.x >= LANES) return;
    __threadfence();                                                    // ... and released, with its verdict on their words, before its count: one fence per 4 KiB
    uint32_t last = 0;
    if (lane == 0) last = atomicAdd(&C->emitDone, 1u) + 1 == (n + 4095) / 4096 ? 1u : 0u;
    if (!DUNI(last)) return;
    __threadfence();                                                    // acquire: every counted workgroup's bytes
    if (DUNI(ZB_LOAD_AGENT(&C->mode)) != 1) return;                     // handed back already
    if (!dec_checksum_ok(out, n, DUNI(C->cksum), lane) && lane == 0) ZB_STORE_AGENT(&C->mode, 0u);
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
static inline uint32_t zb_lit_cap(uint32_t max_out) { return ((max_out + 80u * ZB_MAX_BLOCKS) + 255u) & ~255u; }
static inline uint32_t zb_seq_cap(uint32_t max_out) { return ((max_out / 3u + 64u * ZB_MAX_BLOCKS + 64u) + 63u) & ~63u; }
static inline size_t zb_align256(size_t v) { return (v + 255u) & ~(size_t)255u; }
static inline size_t zb_verify_stride(uint32_t max_out) { return zb_align256(zb_arena_words_at(zb_lit_cap(max_out), zb_seq_cap(max_out))); }
static inline size_t zb_arena_stride(uint32_t max_out) { return zb_align256(zb_arena_words_at(zb_lit_cap(max_out), zb_seq_cap(max_out)) + 4u * ((size_t)max_out + 64u)); }
// workspace of a batch: [n chunk headers][n arenas]
struct ZbWork { uint8_t* hdrs; uint8_t* arenas; uint64_t astride; uint32_t lit_cap, seq_cap; };
static inline ZbWork zb_work(void* work, uint32_t n, uint32_t max_out, size_t astride) {
    return ZbWork{(uint8_t*)work, (uint8_t*)work + (size_t)n * ZB_CHUNK_HDR_BYTES, (uint64_t)astride, zb_lit_cap(max_out), zb_seq_cap(max_out)};
}
size_t tsx_zstd_blockmode_bytes(uint32_t n, uint32_t max_out) { return (size_t)n * (ZB_CHUNK_HDR_BYTES + zb_arena_stride(max_out)); }
bool tsx_zstd_blockmode_takes(uint32_t max_out) { return max_out <= ZB_MAX_CHUNK; }
// the list zstd_decompress_kernel skips by: word i * stride == 1 <=> chunk i was decoded here
const uint32_t* tsx_zstd_blockmode_skip(const void* bwork, uint32_t* stride_words) {
    *stride_words = (uint32_t)(ZB_CHUNK_HDR_BYTES / 4);
    return (const uint32_t*)((const uint8_t*)bwork + offsetof(ZbChunk, mode));
}

// index + decode: the two launches in front of scatter and of verify (zbprof: where a TSX_PROF2 build leaves the phase laps, if anywhere)
static void zb_launch_index_decode(hipStream_t st, const uint8_t* frames, int from_mid, uint64_t mid_stride, const tsx_chunk_desc* d_descs,
                                   const int32_t* d_status, uint32_t n, const ZbWork& W, DecLapOut zbprof) {
    hipLaunchKernelGGL(zb_index_kernel, dim3(n), dim3(LANES), 0, st, frames, from_mid, mid_stride, d_descs, d_status, W.hdrs, W.lit_cap, W.seq_cap);
    hipLaunchKernelGGL(zb_decode_kernel, dim3(ZB_MAX_BLOCKS, n), dim3(2 * LANES), 0, st, frames, from_mid, mid_stride, d_descs, W.hdrs, W.arenas, W.astride, W.lit_cap, W.seq_cap, zbprof);
}

uint32_t tsx_launch_zstd_decompress_blocks(hipStream_t st, const uint8_t* frames, int from_mid, uint64_t mid_stride, tsx_chunk_desc* d_descs, uint32_t n,
                                           uint32_t max_out, uint8_t* dst, int32_t* d_status, void* bwork) {
    if (!n) return 0;
    const ZbWork W = zb_work(bwork, n, max_out, zb_arena_stride(max_out));
    zb_launch_index_decode(st, frames, from_mid, mid_stride, d_descs, d_status, n, W, g_zbprof_out);
    hipLaunchKernelGGL(zb_scatter_kernel, dim3(ZB_MAX_BLOCKS, n), dim3(ZB_SC_WAVES * LANES), 0, st, frames, from_mid, mid_stride, d_descs, W.hdrs, W.arenas, W.astride, W.lit_cap, W.seq_cap);
    // A copy chain is at most as long as the chunk.  A pass makes two jumps IN PLACE: the first reads its source's word, the second the
    // word of what that named - either may still hold its value from before the pass (another thread has not stored yet), so what a pass
    // guarantees is old[old[old[q]]]: three hops of the chain as it was, not four.  ceil(log3(max_out)) + 1 passes therefore resolve every
    // word whatever the order of the stores (14 + 1 for a 4 MiB run at offset 1; round 3 queued log4 + 1 = 13 and such chunks silently
    // took the chunk-serial kernel as well).  The passes behind one that resolved everything return at their first instruction.
    uint32_t rounds = 1;
    for (uint64_t reach = 1; reach < (uint64_t)max_out; reach *= 3) rounds++;
    static_assert(sizeof(((ZbChunk*)0)->live) / sizeof(((ZbChunk*)0)->live[0]) >= 18, "live[] covers the passes of a 16 MiB chunk");
    const uint32_t tiles = (max_out + 1023) / 1024;                     // 256 threads x 4 words
#ifdef HIPEMU
    // test harness: TSX_EMU_JUMP_SNAPSHOT=1 gives every pass the word array as it was before the pass (the worst store order),
    // TSX_EMU_JUMP_ROUNDS=k queues k passes instead of the bound above (to show what too few do)
    uint8_t* snap = getenv("TSX_EMU_JUMP_SNAPSHOT") ? (uint8_t*)malloc((size_t)n * W.astride) : nullptr;
    if (const char* e = getenv("TSX_EMU_JUMP_ROUNDS")) { const long v = atol(e); if (v >= 1 && v <= 31) rounds = (uint32_t)v; }
#endif
    for (uint32_t r = 0; r < rounds; r++) {
#ifdef HIPEMU
        if (snap) { memcpy(snap, W.arenas, (size_t)n * W.astride); g_zb_snap = snap; }
#endif
        hipLaunchKernelGGL(zb_jump_kernel, dim3(tiles, n), dim3(256), 0, st, W.hdrs, W.arenas, W.astride, W.lit_cap, W.seq_cap, r);
    }
#ifdef HIPEMU
    if (snap) { g_zb_snap = nullptr; free(snap); }                     // (snapshot mode is a single-threaded test: callers without it never touch the word)
#endif
    hipLaunchKernelGGL(zb_emit_kernel, dim3((max_out + 4095) / 4096, n), dim3(256), 0, st, (const tsx_chunk_desc*)d_descs, dst, W.hdrs, W.arenas, W.astride, W.lit_cap, W.seq_cap);
    return 4 + rounds;
}

// ---- verify on upload --------------------------------------------------------------------------------
// index, decode, verify: three launches.  The workspace is the decoder's without its largest part, the word per output byte.
// max_len: the longest source chunk of the launch (chunks above ZB_MAX_CHUNK are not taken; the arenas are sized for the others).
static inline uint32_t zb_verify_max(uint32_t max_len) { return max_len < ZB_MAX_CHUNK ? max_len : ZB_MAX_CHUNK; }
size_t tsx_zstd_verify_bytes(uint32_t n, uint32_t max_len) { return (size_t)n * (ZB_CHUNK_HDR_BYTES + zb_verify_stride(zb_verify_max(max_len))); }
uint32_t tsx_launch_zstd_verify_blocks(hipStream_t st, const uint8_t* frames, uint64_t mid_stride, const tsx_chunk_desc* d_descs, const int32_t* d_status,
                                       uint32_t n, uint32_t max_len, const uint8_t* src_base, void* work, uint32_t* verdicts) {
    if (!n) return 0;
    const ZbWork W = zb_work(work, n, zb_verify_max(max_len), zb_verify_stride(zb_verify_max(max_len)));
    zb_launch_index_decode(st, frames, 1, mid_stride, d_descs, d_status, n, W, DecLapOut{});
    hipLaunchKernelGGL(zb_verify_kernel, dim3(ZB_MAX_BLOCKS, n), dim3(ZB_SC_WAVES * LANES), 0, st, frames, mid_stride, d_descs, d_status, src_base, W.hdrs, W.arenas,
                       W.astride, W.lit_cap, W.seq_cap, verdicts);
    return 3;
}
