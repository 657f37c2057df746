// Device-side pieces shared by the two frame-decoder kernels (zstd_dec.hip: one workgroup per chunk, blocks pipelined;
// zstd_dec_blocks.hip: one workgroup per block, for small batches).  Included by those two files only.  It holds:
//   format tables, bit readers, the LDS state of a decoding workgroup (DecLds), FSE / Huffman table builders;
//   every stage that parses frame bytes, once for both kernels:
//     dec_frame_header    magic, descriptor, window, dictionary ID, content size
//     dec_block_header    one block header; dec_frame_end: the checksum's place and the frame's end behind the last block;
//                         dec_checksum_ok: the restored bytes against that checksum (xxh64_dev.h)
//     dec_lit_header      literals-section header: raw / RLE / Huffman sizes and stream count
//     dec_huf_streams     the 1 or 4 Huffman streams through per-stream LDS windows
//     dec_seq_header      sequence count and table modes; dec_seq_table: one table from its description
//     dec_seq_group       the sequence bit stream for one group of 64 sequences: end mark, window refill, initial states,
//                         pass 1 (the state chain, seq_chain_step) and pass 2 (field extraction);
//     dec_rep_offsets     pass 3: the repeat-offset history over that group, on concrete offsets (chunk-serial form) or on
//                         references into a history not yet known (block form) - the one difference is a functor;
//   what both forms set up the same way: dec_code_tables (LL / ML code tables into LDS), dec_huf_tree (a Huffman tree
//   description -> the decoding table), dec_incl_scan2 (positions from lengths), DecLaps (the TSX_PROF2 lap timers);
//   the copy helpers of the chunk-serial form's execution stage.
// What the forms do differently stays in their own files: execution, the state the chunk-serial form carries across blocks,
// the block form's own limits, and what a failure means to each.
#pragma once
#include "zstd_common.h"
#include "xxh64_dev.h"

#define LANES 64
#define DERR_FRAME TSX_E_BAD_FRAME

__device__ static const uint32_t dLLbase[36] = {0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,18,20,22,24,28,32,40,48,64,128,256,512,1024,2048,4096,8192,16384,32768,65536};
__device__ static const uint8_t dLLbits[36] = {0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1,2,2,3,3,4,6,7,8,9,10,11,12,13,14,15,16};
__device__ static const uint32_t dMLbase[53] = {3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25,26,27,28,29,30,31,32,33,34,35,37,39,41,43,47,51,59,67,83,99,131,259,515,1027,2051,4099,8195,16387,32771,65539};
__device__ static const uint8_t dMLbits[53] = {0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1,2,2,3,3,4,4,5,7,8,9,10,11,12,13,14,15,16};
__device__ static const short dLLnorm[36] = {4,3,2,2,2,2,2,2,2,2,2,2,2,1,1,1,2,2,2,2,2,2,2,2,2,3,2,1,1,1,1,1,-1,-1,-1,-1};
__device__ static const short dOFnorm[29] = {1,1,1,1,1,1,2,2,2,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,-1,-1,-1,-1,-1};
__device__ static const short dMLnorm[53] = {1,4,3,2,2,2,2,2,2,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,1,-1,-1,-1,-1,-1,-1,-1};

__device__ static inline uint32_t dhb32(uint32_t v) { return 31u - (uint32_t)__clz((int)v); }
__device__ static inline uint64_t dld64(const uint8_t* p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }

#define ZS_DWIN 2048u
#define ZS_DPAD 16u
#define ZS_HWIN 256u
struct FseD { uint16_t base; uint8_t sym; uint8_t nb; };
// sequence decoding entry, one dword: next-state base (bits 0-8) | nbBits (9-13) | nbBits + the symbol's number of extra
// bits (14-20) | the symbol (21-26).  Bits 9-20 are laid out so that ONE add sums both counts over the three tables (no carry:
// 3 x 9 < 32, 3 x 40 < 128).  The symbol's base value comes from a small per-code table when the lanes decode the fields.
#define DUNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(x)))
// v_writelane_b32: a wave-uniform value lands in lane `lane` of a per-lane register (this clang has the intrinsic, not the builtin)
#ifdef HIPEMU
#define tsx_writelane(v, lane, old) __builtin_amdgcn_writelane((uint32_t)(v), (uint32_t)(lane), (uint32_t)(old))
#else
extern "C" __device__ uint32_t tsx_writelane(uint32_t v, uint32_t lane, uint32_t old) __asm("llvm.amdgcn.writelane.i32");
#endif
typedef uint32_t SeqD;
#define SEQD(base_, nb_, ebits_, sym_) ((uint32_t)(base_) | ((uint32_t)(nb_) << 9) | ((uint32_t)((nb_) + (ebits_)) << 14) | ((uint32_t)(sym_) << 21))
#define SEQD_BASE(e_) ((e_) & 0x1FFu)
#define SEQD_NB(e_) (((e_) >> 9) & 0x1Fu)
#define SEQD_TOT(e_) (((e_) >> 14) & 0x7Fu)
#define SEQD_EBITS(e_) (SEQD_TOT(e_) - SEQD_NB(e_))
#define SEQD_SYM(e_) (((e_) >> 21) & 0x3Fu)
#define SEQD_COUNTS(e_) (((e_) >> 9) & 0xFFFu)                        /* nbBits | (nbBits + extra bits) << 5 */
#ifdef HIPEMU
#define TSX_SCHED_BARRIER() do {} while (0)
#define TSX_SETPRIO(p_) do {} while (0)
#else
#define TSX_SCHED_BARRIER() __builtin_amdgcn_sched_barrier(0)
#define TSX_SETPRIO(p_) __builtin_amdgcn_s_setprio(p_)          /* issue priority of this wave among the SIMD's waves, 0..3 */
#endif
// row_shl:n - lane i reads lane i + n of its row of 16, 0 past the row's end
#define DPP_SHL(v_, n_) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v_), 0x100 + (n_), 0xF, 0xF, true))
// what the literal wave hands to the sequence wave for one block
struct BlkDesc { uint32_t off, bsize, btype, last, litInPlace, litOff, litSize, q; };
// Wave-level rendezvous: the lanes of ONE wave run in lockstep, so this is only a memory fence + a compiler barrier on the
// device (a workgroup barrier here would wait for the chunk's other wave, which is somewhere else entirely).
#ifdef HIPEMU
#define WAVE_SYNC() hipemu::wave_barrier()
#else
#define WAVE_SYNC() do { __threadfence_block(); __builtin_amdgcn_wave_barrier(); } while (0)
#endif
struct DecLds {
    // Literal Huffman table, indexed by the next 11 bits of a stream (Max_Number_of_Bits of a literals tree is 11, RFC 8878
    // 4.2.1): up to three whole symbols that those bits decode to | total bits << 24 | number of symbols << 28
    uint32_t hufX[2048];
    uint16_t hufRs[16], hufSymStart[16];   // canonical form: first table index / first entry of hufSorted of each weight
    uint8_t hufSorted[256];                // symbols by (weight, symbol)
    uint32_t hufLog; int hufValid;
    SeqD ll[512], of[256], ml[512];
    SeqD zeroEntry;              // the 'table' of the lanes that run no state machine
    alignas(8) uint16_t rec[LANES * 4];   // pass 1 -> pass 2: the three states of each of the group's 64 sequences
    uint8_t cellSym[512];        // table construction scratch: symbol of each cell
    uint32_t cLLbase[36], cMLbase[53]; uint8_t cLLbits[36], cMLbits[53];   // LDS copies of the length code tables
    FseD wt[64];                 // FSE table of the Huffman-weight stream (tableLog <= 6)
    uint32_t llLog, ofLog, mlLog; int llValid, ofValid, mlValid;
    uint8_t weights[256];
    uint32_t rankCount[16], rankStart[16];
    short norm[64];
    uint16_t symNext[64];
    uint32_t scal[16];
    uint32_t streamOff[5];
    // the literal wave's own scratch and windows (the two waves of a chunk run concurrently)
    short normH[16]; uint16_t symNextH[16]; uint8_t cellSymH[64]; uint32_t scalH[4];
    BlkDesc desc[3];             // block k in slot k % 3: written by the literal stage, read by the sequence and execution stages
    uint32_t nseq[2];            // sequence stage -> execution stage: number of sequences of block k in slot k & 1
    int32_t err;                 // first error of either wave
    alignas(16) uint8_t hwin[4 * (ZS_HWIN + 16)];   // one window per Huffman stream
    alignas(16) uint8_t swin[ZS_DPAD + ZS_DWIN + 32];   // the sequence bit stream's window behind ZS_DPAD zero bytes (seq_chain_step reads up to 7 bytes in front of the stream)
};

// ---- lap timers of a TSX_PROF2 build (tools/prof_small.py, tools/show_prof.py, tools/zb_phase_laps.py) -------------------
// A decoding kernel takes a DecLapOut by value and every wave keeps a DecLaps: lap(k) adds the clocks since the wave's previous
// lap to its bucket k, put() stores bucket a (+ bucket b) in word `slot` of the 8 u64 of `row`.  Both are empty in the product
// build: no kernel argument, no register, no instruction.
#ifdef TSX_PROF2
struct DecLapOut { unsigned long long* buf; };
struct DecLaps {
    unsigned long long t[8] = {0, 0, 0, 0, 0, 0, 0, 0}, last = (unsigned long long)clock64();
    __device__ __forceinline__ void lap(int k) { const unsigned long long n = (unsigned long long)clock64(); t[k] += n - last; last = n; }
    __device__ __forceinline__ void put(const DecLapOut& o, size_t row, int slot, int a, int b = -1) const { if (o.buf) o.buf[row * 8 + slot] = t[a] + (b >= 0 ? t[b] : 0); }
};
#else
struct DecLapOut {};
struct DecLaps {
    __device__ __forceinline__ void lap(int) {}
    __device__ __forceinline__ void put(const DecLapOut&, size_t, int, int, int = -1) const {}
};
#endif

// ---- backward bit reader (BIT_DStream) -----------------------------------------------------------------
struct BitR { const uint8_t* start; const uint8_t* ptr; uint64_t c; uint32_t consumed; bool bad; };
__device__ static void br_init(BitR& b, const uint8_t* src, uint32_t n) {
    b.start = src; b.bad = false; b.consumed = 0; b.c = 0; b.ptr = src;
    if (n == 0) { b.bad = true; return; }
    const uint8_t last = src[n - 1];
    if (last == 0) { b.bad = true; return; }
    if (n >= 8) {
        b.ptr = src + n - 8; b.c = dld64(b.ptr);
        b.consumed = 8 - dhb32(last);
    } else {
        uint64_t c = 0;
        for (uint32_t i = 0; i < n; i++) c |= (uint64_t)src[i] << (8 * i);
        b.c = c;
        b.consumed = 8 - dhb32(last) + (8 - n) * 8;
    }
}
__device__ static inline uint64_t br_look(const BitR& b, uint32_t nb) {          // nb >= 1
    return (b.c << (b.consumed & 63)) >> (64 - nb);
}
__device__ static inline uint64_t br_read(BitR& b, uint32_t nb) {
    if (!nb) return 0;
    const uint64_t v = br_look(b, nb);
    b.consumed += nb;
    return v;
}
// returns false once the stream is over-read
__device__ static inline bool br_reload(BitR& b) {
    if (b.consumed > 64) return false;
    if (b.ptr >= b.start + 8) { b.ptr -= b.consumed >> 3; b.consumed &= 7; b.c = dld64(b.ptr); return true; }
    if (b.ptr == b.start) return true;
    uint32_t nbBytes = b.consumed >> 3;
    if (b.ptr - nbBytes < b.start) nbBytes = (uint32_t)(b.ptr - b.start);
    b.ptr -= nbBytes; b.consumed -= nbBytes * 8;
    // fewer than 8 bytes may remain readable behind ptr only when the stream itself is shorter than 8 bytes
    b.c = dld64(b.ptr);
    return true;
}

// An 8-byte read from a window of a bit stream held in LDS: win[0 ..) = stream bytes [wbase ..), positions are offsets in the
// stream, so no pointer ever leaves the window array.
__device__ static inline uint64_t wld64(const uint8_t* win, uint32_t wbase, uint32_t pos) { return dld64(win + (pos - wbase)); }

// One step of the sequence chain (pass 1 of the sequence stage in zstd_dec.hip and zstd_dec_blocks.hip), on the vector unit.  Lanes 0, 1, 2
// run the LL, ML and OF state machines (that is the order in which a sequence's state-update bits sit in the stream, highest first); the
// other lanes carry state 0 through an all-zero entry.  One table read serves all three, two DPP adds give every machine the bits below
// its own field and lane 0 the sequence's bit total, and the 8 bytes that hold the update bits are read together with the entries from
// the cursor alone ([B - 56.., B)): only a sequence that reads more than 56 bits needs a second, dependent read.  win = the window
// behind its ZS_DPAD zero bytes: near the stream's start the 8 bytes begin up to 7 bytes in front of it, which costs no select.  The
// state goes to *rec for pass 2; an over-read shows as a negative cursor (collected in bad, checked once per group) and is clamped so that
// no load leaves the window.  The wave is alone on its SIMD, so a step costs its instruction count (~5 cycles each) plus one LDS latency:
// profiles/r03_zb_phase_laps.txt.
__device__ __forceinline__ void seq_chain_step(const SeqD* __restrict__ tbl, uint16_t* __restrict__ rec, const uint8_t* __restrict__ win, uint32_t wbase,
                                               uint32_t& st, uint32_t& B, uint32_t& bad) {
    const int32_t p8 = (int32_t)(B >> 3) - 7;                           // >= wbase when wbase != 0 (the window's margin), >= -7 else
    const uint32_t e_ = tbl[st];                                        // first: LDS answers in order, and this is the read the chain waits for
    uint64_t c8 = dld64(win + (p8 - (int32_t)wbase));
    *rec = (uint16_t)st;
    TSX_SCHED_BARRIER();                                                // both reads are in flight before anything waits
    const uint32_t pc = SEQD_COUNTS(e_);
    const uint32_t below = DPP_SHL(pc, 1) + DPP_SHL(pc, 2);             // the machines below this one
    // extra bits of the offset, match length, literal length, then the state updates: LL, ML, OF (ZSTD_decodeSequence order)
    const int32_t raw = (int32_t)(B - DUNI((pc + below) >> 5));
    bad |= (uint32_t)raw;
    const uint32_t lo = (uint32_t)(raw < 0 ? 0 : raw);
    int32_t sh = (int32_t)lo - 8 * p8;
    if (__builtin_expect(sh < 0, 0)) { c8 = wld64(win, wbase, lo >> 3); sh = (int32_t)(lo & 7); }       // rare
    st = SEQD_BASE(e_) + ((uint32_t)(c8 >> ((uint32_t)sh + (below & 31))) & ((1u << (pc & 31)) - 1));
    B = lo;
}

// ---- FSE table description + decoding table (lane 0) ---------------------------------------------------------
// returns bytes consumed, 0 on error
// (STORE = false walks the description without keeping the counts: how long it is, and whether it is well formed)
template <bool STORE>
__device__ static uint32_t fse_walkNCount(short* norm, uint32_t* maxSymPtr, uint32_t* tableLogPtr, const uint8_t* src, uint32_t n, uint32_t maxLogAllowed) {
    if (n < 1) return 0;
    // bounded forward bit reader over at most n bytes
    uint64_t bitpos = 0;
    // 4 bytes at the bit cursor: one unaligned load while they are all inside the description, byte by byte (zeros past its end) otherwise
    #define NC_PEEK(k) ({ uint32_t v_ = 0; const uint64_t b0_ = bitpos >> 3; \
                          if (b0_ + 4 <= n) __builtin_memcpy(&v_, src + b0_, 4); \
                          else for (int i_ = 0; i_ < 4; i_++) { const uint64_t b_ = b0_ + i_; v_ |= (uint32_t)(b_ < n ? src[b_] : 0) << (8 * i_); } \
                          (v_ >> (bitpos & 7)) & ((1u << (k)) - 1); })
    const uint32_t tableLog = NC_PEEK(4) + 5; bitpos += 4;
    if (tableLog > maxLogAllowed) return 0;
    int remaining = (1 << tableLog) + 1, threshold = 1 << tableLog, nbBits = (int)tableLog + 1;
    uint32_t sym = 0; const uint32_t maxSym = *maxSymPtr;
    bool prev0 = false;
    while (remaining > 1 && sym <= maxSym) {
        if (prev0) {
            for (;;) {
                const uint32_t r = NC_PEEK(2); bitpos += 2;
                for (uint32_t k = 0; k < r; k++) { if (sym > maxSym) return 0; if (STORE) norm[sym] = 0; sym++; }
                if (r != 3) break;
                if ((bitpos >> 3) > n + 4) return 0;
            }
            prev0 = false;
            continue;
        }
        const int mx = (2 * threshold - 1) - remaining;
        int count;
        const uint32_t lo = NC_PEEK(nbBits - 1);
        if ((int)lo < mx) { count = (int)lo; bitpos += nbBits - 1; }
        else { count = (int)NC_PEEK(nbBits); if (count >= threshold) count -= mx; bitpos += nbBits; }
        count--;
        remaining -= count < 0 ? -count : count;
        if (sym > maxSym) return 0;
        if (STORE) norm[sym] = (short)count;
        sym++;
        prev0 = count == 0;
        while (remaining < threshold) { nbBits--; threshold >>= 1; }
        if ((bitpos >> 3) > n + 4) return 0;
    }
    #undef NC_PEEK
    if (remaining != 1) return 0;
    const uint32_t used = (uint32_t)((bitpos + 7) >> 3);
    if (used > n) return 0;
    *maxSymPtr = sym - 1; *tableLogPtr = tableLog;
    return used;
}
__device__ static inline uint32_t fse_readNCount(short* norm, uint32_t* maxSymPtr, uint32_t* tableLogPtr, const uint8_t* src, uint32_t n, uint32_t maxLogAllowed) {
    return fse_walkNCount<true>(norm, maxSymPtr, tableLogPtr, src, n, maxLogAllowed);
}
__device__ static inline uint32_t fse_skipNCount(uint32_t maxSym, const uint8_t* src, uint32_t n, uint32_t maxLogAllowed) {
    uint32_t ms = maxSym, tl = 0;
    return fse_walkNCount<false>(nullptr, &ms, &tl, src, n, maxLogAllowed);
}

template <class E, class Fill>
__device__ static bool fse_buildDTable(E* dt, uint8_t* cellSym, const short* norm, uint32_t maxSym, uint32_t tableLog, uint16_t* symNext, Fill fill) {
    const uint32_t size = 1u << tableLog, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
    uint32_t high = size - 1;
    for (uint32_t s = 0; s <= maxSym; s++) {
        if (norm[s] == -1) { cellSym[high--] = (uint8_t)s; symNext[s] = 1; }
        else symNext[s] = (uint16_t)norm[s];
    }
    uint32_t pos = 0;
    for (uint32_t s = 0; s <= maxSym; s++)
        for (int i = 0; i < norm[s]; i++) {
            cellSym[pos] = (uint8_t)s;
            pos = (pos + step) & mask;
            while (pos > high) pos = (pos + step) & mask;
        }
    if (pos != 0) return false;
    for (uint32_t u = 0; u < size; u++) {
        const uint8_t s = cellSym[u];
        const uint32_t ns = symNext[s]++;
        const uint32_t nb = tableLog - dhb32(ns);
        E e; e.nb = (uint8_t)nb; e.base = (uint16_t)((ns << nb) - size);
        fill(e, s);
        dt[u] = e;
    }
    return true;
}
// kind 0 = literal lengths, 1 = offsets, 2 = match lengths: extra bits / base value of a code
__device__ static inline uint32_t seq_ebits(const DecLds& L, uint32_t sym, int kind) { return kind == 0 ? L.cLLbits[sym] : kind == 1 ? sym : L.cMLbits[sym]; }
// The same table (FSE_buildDTable: spread the symbols with the odd stride `step`, number each symbol's cells in ascending
// position) built by the whole wave instead of one lane walking 2 x 512 cells through dependent LDS accesses:
//  * the spread visits the cells in the order (i * step) & mask, i = 0, 1, ..., skipping the cells above `high` that the
//    low-probability symbols (count -1) own; so cell u is the r-th one filled, r = i(u) - #{low cells visited before},
//    i(u) = u * step^-1 mod size, and its symbol is the one whose run of the cumulative counts holds r;
//  * cells are numbered 64 at a time in ascending position: a cell's state number is its symbol's running count (kept in
//    lane `symbol`) plus its rank among the same-symbol lanes of the round.
// norm[] is in LDS (L.norm), maxSym < 64.  Returns false (wave-uniform) when the counts do not fill the table.
__device__ static bool fse_buildSeqTable_wave(SeqD* dt, DecLds& L, uint32_t maxSym, uint32_t tableLog, int kind, uint32_t lane) {
    const uint32_t size = 1u << tableLog, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
    uint16_t* const cum = (uint16_t*)L.cellSym;                           // [64] exclusive prefix of the positive counts
    uint16_t* const lowI = cum + 64;                                      // [<= 64] visit index of each low-probability cell
    uint8_t* const lowSym = L.cellSym + 256;                              // [<= 64] symbol of the k-th low-probability cell
    const int nv = lane <= maxSym ? (int)L.norm[lane] : 0;
    const uint32_t c = nv > 0 ? (uint32_t)nv : 0;
    const bool lowp = nv == -1;
    uint32_t incl = c;
    for (uint32_t o = 1; o < LANES; o <<= 1) { const uint32_t v = __shfl_up(incl, o); if (lane >= o) incl += v; }
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane(incl, LANES - 1);
    const unsigned long long lowMask = __ballot(lowp);
    const uint32_t nLow = (uint32_t)__popcll(lowMask);
    if (total + nLow != size) return false;
    uint32_t inv = step;                                                  // odd: step * step = 1 (mod 8); each Newton step doubles the bits
    for (int it = 0; it < 3; it++) inv *= 2u - step * inv;
    inv &= mask;
    WAVE_SYNC();                                                          // the scratch may still be read as the previous table's
    cum[lane] = (uint16_t)(incl - c);
    if (lowp) {
        const uint32_t k = (uint32_t)__popcll(lowMask & ((1ull << lane) - 1));   // low cells go to the top, in symbol order
        lowI[k] = (uint16_t)(((size - 1 - k) * inv) & mask); lowSym[k] = (uint8_t)lane;
    }
    WAVE_SYNC();
    uint32_t next = lowp ? 1u : c;                                        // symNext of symbol `lane`
    const uint32_t high = size - 1 - nLow;
    for (uint32_t base = 0; base < size; base += LANES) {
        const uint32_t u = base + lane;
        const bool active = u < size;
        uint32_t sym = 0;
        if (active) {
            if (u > high) sym = lowSym[size - 1 - u];
            else {
                const uint32_t i = (u * inv) & mask;
                uint32_t r = i;
                for (uint32_t k = 0; k < nLow; k++) r -= lowI[k] < i ? 1u : 0u;
                for (uint32_t b = 32; b; b >>= 1) if (cum[sym + b] <= r) sym += b;     // the last symbol whose run starts at or before r
            }
        }
        uint32_t ns = 1;
        unsigned long long rem = __ballot(active);
        while (rem) {
            const uint32_t cur = (uint32_t)__builtin_amdgcn_readlane(sym, __ffsll((long long)rem) - 1);     // v_readlane: no LDS round trip
            const unsigned long long m = __ballot(active && sym == cur);
            const uint32_t first = (uint32_t)__builtin_amdgcn_readlane(next, (int)cur);
            if (active && sym == cur) ns = first + (uint32_t)__popcll(m & ((1ull << lane) - 1));
            if (lane == cur) next += (uint32_t)__popcll(m);
            rem &= ~m;
        }
        if (active) {
            const uint32_t nb = tableLog - dhb32(ns);
            dt[u] = SEQD((ns << nb) - size, nb, seq_ebits(L, sym, kind), sym);
        }
    }
    WAVE_SYNC();
    return true;
}
// A Huffman tree description -> weights, canonical form (lane 0 alone: a serial parse).  Out of line on purpose: it is the one real
// call of the decoding kernels, and inlined into them it only lengthens the live ranges of their pipelines' registers.
__device__ __attribute__((noinline)) static uint32_t huf_readTable(DecLds& L, const uint8_t* src, uint32_t n) {
    if (n < 1) return 0;
    const uint32_t hb = src[0];
    uint32_t nw = 0, used;
    if (hb >= 128) {
        nw = hb - 127; used = 1 + (nw + 1) / 2;
        if (used > n) return 0;
        for (uint32_t i = 0; i < nw; i++) { const uint8_t b = src[1 + i / 2]; L.weights[i] = (i & 1) ? (b & 15) : (b >> 4); }
    } else {
        used = 1 + hb;
        if (hb < 2 || used > n) return 0;
        uint32_t maxSym = 12, tl;
        const uint32_t h = fse_readNCount(L.normH, &maxSym, &tl, src + 1, hb, 6);
        if (!h) return 0;
        if (!fse_buildDTable(L.wt, L.cellSymH, L.normH, maxSym, tl, L.symNextH, [](FseD& e, uint32_t sym) { e.sym = (uint8_t)sym; })) return 0;
        BitR b; br_init(b, src + 1 + h, hb - h);
        if (b.bad) return 0;
        uint32_t s1 = (uint32_t)br_read(b, tl), s2 = (uint32_t)br_read(b, tl);
        br_reload(b);
        for (;;) {
            if (nw > 253) return 0;
            { const FseD e = L.wt[s1]; L.weights[nw++] = e.sym; s1 = e.base + (uint32_t)br_read(b, e.nb); }
            if (!br_reload(b)) { L.weights[nw++] = L.wt[s2].sym; break; }
            if (nw > 253) return 0;
            { const FseD e = L.wt[s2]; L.weights[nw++] = e.sym; s2 = e.base + (uint32_t)br_read(b, e.nb); }
            if (!br_reload(b)) { L.weights[nw++] = L.wt[s1].sym; break; }
        }
    }
    // the last weight is implicit
    uint32_t total = 0;
    for (uint32_t i = 0; i < 16; i++) L.rankCount[i] = 0;
    for (uint32_t i = 0; i < nw; i++) { const uint32_t w = L.weights[i]; if (w > 12) return 0; L.rankCount[w]++; total += w ? (1u << (w - 1)) : 0; }
    if (total == 0) return 0;
    const uint32_t tableLog = dhb32(total) + 1;
    if (tableLog > 11) return 0;
    const uint32_t rest = (1u << tableLog) - total;
    if (rest & (rest - 1)) return 0;
    const uint32_t lastW = dhb32(rest) + 1;
    L.weights[nw++] = (uint8_t)lastW; L.rankCount[lastW]++;
    if (L.rankCount[1] < 2 || (L.rankCount[1] & 1)) return 0;
    // canonical layout: weight-1 symbols (the longest codes, tableLog bits) own the lowest table indices, one index each; a
    // symbol of weight w owns 1 << (w - 1) consecutive indices and is coded on tableLog + 1 - w bits
    uint32_t next = 0, cnt = 0;
    for (uint32_t w = 1; w <= tableLog; w++) {
        L.hufRs[w] = (uint16_t)next; next += L.rankCount[w] << (w - 1);
        L.hufSymStart[w] = (uint16_t)cnt; L.rankStart[w] = cnt; cnt += L.rankCount[w];
    }
    L.hufRs[tableLog + 1] = (uint16_t)next;
    for (uint32_t sy = 0; sy < nw; sy++) { const uint32_t w = L.weights[sy]; if (w) L.hufSorted[L.rankStart[w]++] = (uint8_t)sy; }
    L.hufLog = tableLog; L.hufValid = 1;
    return used;
}

// One symbol from the canonical form: idx = the next tableLog bits (zero-padded below the stream's first bit).  -> symbol | nbBits << 8
__device__ static inline uint32_t huf_decode1(const DecLds& L, uint32_t idx, uint32_t tableLog) {
    uint32_t w = 1;
    for (uint32_t ww = 2; ww <= tableLog; ww++) if (L.hufRs[ww] <= idx) w = ww;          // empty weights share their start with the next one
    const uint32_t sym = L.hufSorted[L.hufSymStart[w] + ((idx - L.hufRs[w]) >> (w - 1))];
    return sym | ((tableLog + 1 - w) << 8);
}
// The 11-bit multi-symbol table, built by the whole wave: entry x = the (up to three) symbols whose codes fit entirely in x.
__device__ static void huf_buildX_wave(DecLds& L, uint32_t lane) {
    const uint32_t tl = L.hufLog, mask = (1u << tl) - 1;
    for (uint32_t x = lane; x < 2048; x += LANES) {
        uint32_t pos = 0, ns = 0, syms = 0;
        for (uint32_t k = 0; k < 3 && pos < 11; k++) {
            const uint32_t rem = 11 - pos;
            const uint32_t idx = rem >= tl ? (x >> (rem - tl)) & mask : (x << (tl - rem)) & mask;
            const uint32_t e = huf_decode1(L, idx, tl);
            if ((e >> 8) > rem) break;                                 // this code runs past the 11 bits
            syms |= (e & 0xFF) << (8 * k); pos += e >> 8; ns++;
        }
        L.hufX[x] = syms | (pos << 24) | (ns << 28);
    }
}
// The Huffman tree description at tree / avail -> the decoding table (L.hufX, L.hufLog; L.hufValid set): lane 0 parses the
// description, the whole wave builds the table.  One wave, every lane with the same arguments.  Returns the bytes the
// description used, 0 (wave-uniform) when it is malformed.
__device__ __forceinline__ static uint32_t dec_huf_tree(DecLds& L, const uint8_t* __restrict__ tree, uint32_t avail, uint32_t lane) {
    if (lane == 0) L.scalH[0] = huf_readTable(L, tree, avail);
    WAVE_SYNC();
    const uint32_t used = DUNI(L.scalH[0]);
    WAVE_SYNC();
    if (!used) return 0;
    huf_buildX_wave(L, lane);
    WAVE_SYNC();
    return used;
}
// The literal-length and match-length code tables (base value and extra bits of every code) and the table of the lanes that
// run no state machine, staged in LDS by one wave for dec_seq_table and dec_seq_group; visible after the caller's barrier.
__device__ __forceinline__ static void dec_code_tables(DecLds& L, uint32_t lane) {
    if (lane == 0) L.zeroEntry = 0;
    if (lane < 36) { L.cLLbase[lane] = dLLbase[lane]; L.cLLbits[lane] = dLLbits[lane]; }
    if (lane < 53) { L.cMLbase[lane] = dMLbase[lane]; L.cMLbits[lane] = dMLbits[lane]; }
}

// ---- frame parsing, one helper per stage ----------------------------------------------------------------------------------
// Both kernels parse frames through these, so a frame means the same to both: the block-parallel form may only take a chunk that
// it decodes exactly as the chunk-serial form would.  The helpers report failure (a status, a false, an ok of 0); what a failure
// does - an error code of the chunk-serial form, the chunk handed back by the block form - is the caller's business.

// Frame header: magic, descriptor, window, dictionary ID, content size.  The checks run in this order, and the order decides
// the code: a frame that declares no content size is TSX_E_BAD_SIZE, whatever follows its dictionary ID.  (The dst_cap check
// is the caller's: TSX_E_DST_TOO_SMALL in the chunk-serial form, the chunk handed back in the block form.)
struct DecFrame { int32_t status; uint32_t p; uint64_t contentSize; bool hasChecksum; };   // p: the first block header
__device__ __forceinline__ static DecFrame dec_frame_header(const uint8_t* __restrict__ src, uint32_t srcSize) {
    DecFrame f; f.status = DERR_FRAME; f.p = 0; f.contentSize = 0; f.hasChecksum = false;
    if (srcSize < 6) return f;
    if (src[0] != 0x28 || src[1] != 0xB5 || src[2] != 0x2F || src[3] != 0xFD) return f;
    const uint32_t fhd = src[4];
    const uint32_t single = (fhd >> 5) & 1, dictFlag = fhd & 3, fcsFlag = fhd >> 6;
    f.hasChecksum = (fhd >> 2) & 1;
    if (fhd & 8) return f;                                              // reserved bit
    uint32_t p = 5;
    if (!single) { if (p >= srcSize) return f; if ((src[p] >> 3) > 21) return f; p++; }
    const uint32_t dl = dictFlag == 0 ? 0 : dictFlag == 1 ? 1 : dictFlag == 2 ? 2 : 4;
    if (p + dl > srcSize) return f;
    uint32_t dictId = 0; for (uint32_t i = 0; i < dl; i++) dictId |= (uint32_t)src[p + i] << (8 * i);
    if (dictId) return f;                                               // dictionaries are not supported (the reference uses none)
    p += dl;
    const uint32_t fl = fcsFlag == 0 ? single : fcsFlag == 1 ? 2 : fcsFlag == 2 ? 4 : 8;
    if (fl == 0) { f.status = TSX_E_BAD_SIZE; return f; }               // unknown content size: "Invalid decompressed size"
    if (p + fl > srcSize) return f;
    uint64_t contentSize = 0;
    for (uint32_t i = 0; i < fl; i++) contentSize |= (uint64_t)src[p + i] << (8 * i);
    if (fl == 2) contentSize += 256;
    f.status = TSX_OK; f.p = p + fl; f.contentSize = contentSize;
    return f;
}

// The block header at p.  ok = 0 on a reserved block type, a compressed block outside 2 .. Block_Maximum_Size bytes, or a body
// that runs past the frame.  next = the position behind the body (a raw block's bsize bytes, an RLE block's one byte).
struct DecBlockHdr { uint32_t ok, last, btype, bsize, off, next; };    // off: where the body starts
__device__ __forceinline__ static DecBlockHdr dec_block_header(const uint8_t* __restrict__ src, uint32_t srcSize, uint32_t p) {
    DecBlockHdr h; h.ok = 0; h.last = 0; h.btype = 0; h.bsize = 0; h.off = p; h.next = p;
    if (p + 3 > srcSize) return h;
    const uint32_t bh = (uint32_t)src[p] | ((uint32_t)src[p + 1] << 8) | ((uint32_t)src[p + 2] << 16);
    h.off = p + 3; h.last = bh & 1; h.btype = (bh >> 1) & 3; h.bsize = bh >> 3;
    if (h.btype == 3) return h;
    if (h.btype == 2 && (h.bsize > ZS_BLOCK_MAX || h.bsize < 2)) return h;
    const uint32_t body = h.btype == 1 ? 1 : h.bsize;
    if (h.off + body > srcSize) return h;
    h.next = h.off + body; h.ok = 1;
    return h;
}
// Behind the last block: the optional content checksum (four bytes, verified by dec_checksum_ok once the content is restored),
// then the frame's end.
__device__ __forceinline__ static bool dec_frame_end(uint32_t p, uint32_t srcSize, bool hasChecksum) {
    if (hasChecksum) { if (p + 4 > srcSize) return false; p += 4; }
    return p == srcSize;
}
// The four checksum bytes at p: the low 32 bits of XXH64 of the content, little endian.
__device__ __forceinline__ static uint32_t dec_checksum_at(const uint8_t* __restrict__ src, uint32_t p) {
    return (uint32_t)src[p] | ((uint32_t)src[p + 1] << 8) | ((uint32_t)src[p + 2] << 16) | ((uint32_t)src[p + 3] << 24);
}
// Do the restored bytes out[0, n) hash to `expected`?  One wave, every lane with the same arguments; the bytes are visible to it.
__device__ __forceinline__ static bool dec_checksum_ok(const uint8_t* out, uint32_t n, uint32_t expected, uint32_t lane) {
    return (uint32_t)xxh64_wave(out, n, lane) == expected;
}

// Literals-section header of a compressed block -> section size (0 = malformed).  hl = header bytes, csize = Huffman
// section bytes (tree description + streams) behind them.
struct DecLit { uint32_t ltype, hl, litSize, csize, streams, section; };
__device__ __forceinline__ static DecLit dec_lit_header(const uint8_t* __restrict__ blk, uint32_t bsize) {
    DecLit h; h.section = 0; h.csize = 0; h.streams = 1;
    const uint32_t b0 = blk[0], sf = (b0 >> 2) & 3;
    h.ltype = b0 & 3;
    if (h.ltype < 2) {
        if (sf == 0 || sf == 2) { h.litSize = b0 >> 3; h.hl = 1; }
        else if (sf == 1) { if (bsize < 2) return h; h.litSize = (b0 >> 4) + ((uint32_t)blk[1] << 4); h.hl = 2; }
        else { if (bsize < 3) return h; h.litSize = (b0 >> 4) + ((uint32_t)blk[1] << 4) + ((uint32_t)blk[2] << 12); h.hl = 3; }
        if (h.litSize > ZS_BLOCK_MAX) return h;
        const uint32_t sec = h.ltype == 0 ? h.hl + h.litSize : h.hl + 1;
        if (sec > bsize) return h;
        h.section = sec;
    } else {
        uint32_t bits;
        if (sf == 0) { h.hl = 3; bits = 10; h.streams = 1; }
        else if (sf == 1) { h.hl = 3; bits = 10; h.streams = 4; }
        else if (sf == 2) { h.hl = 4; bits = 14; h.streams = 4; }
        else { h.hl = 5; bits = 18; h.streams = 4; }
        if (h.hl > bsize) return h;
        uint64_t v = 0;
        for (uint32_t i = 0; i < h.hl; i++) v |= (uint64_t)blk[i] << (8 * i);
        h.litSize = (uint32_t)(v >> 4) & ((1u << bits) - 1);
        h.csize = (uint32_t)(v >> (4 + bits)) & ((1u << bits) - 1);
        if (h.litSize > ZS_BLOCK_MAX || h.hl + h.csize > bsize || h.litSize == 0) return h;
        h.section = h.hl + h.csize;
    }
    return h;
}

// The 1 or 4 Huffman streams of a literals section (tree built: L.hufX, L.hufLog), on lanes 0-3: pay / payload = the section's
// bytes behind the tree description.  Each stream decodes through its own LDS window of the stream, refilled by the whole wave
// whenever a lane gets close to its window's lower edge (a reload from global memory would be a dependent round trip every four
// symbols).  Returns false (wave-uniform) on a malformed stream.
__device__ __forceinline__ static bool dec_huf_streams(DecLds& L, const uint8_t* __restrict__ pay, uint32_t payload, uint32_t streams, uint32_t litSize,
                                                       uint8_t* __restrict__ lit, uint32_t lane) {
    uint32_t sOff[5], sCnt[4];
    if (streams == 1) { sOff[0] = 0; sOff[1] = payload; sOff[2] = sOff[3] = sOff[4] = payload; sCnt[0] = litSize; sCnt[1] = sCnt[2] = sCnt[3] = 0; }
    else {
        if (payload < 10) return false;
        const uint32_t s1 = pay[0] | (pay[1] << 8), s2 = pay[2] | (pay[3] << 8), s3 = pay[4] | (pay[5] << 8);
        if (6 + (uint64_t)s1 + s2 + s3 >= payload) return false;
        sOff[0] = 6; sOff[1] = 6 + s1; sOff[2] = sOff[1] + s2; sOff[3] = sOff[2] + s3; sOff[4] = payload;
        const uint32_t seg = (litSize + 3) / 4;
        if (3 * seg > litSize) return false;
        sCnt[0] = sCnt[1] = sCnt[2] = seg; sCnt[3] = litSize - 3 * seg;
    }
    bool ok = true;
    const bool mine = lane < streams;
    uint32_t o = 0; for (uint32_t k = 0; k < lane && k < 4; k++) o += mine ? sCnt[k] : 0;
    const uint32_t cnt = mine ? sCnt[lane] : 0, sn = mine ? sOff[lane + 1] - sOff[lane] : 0, sbeg = mine ? sOff[lane] : 0;
    uint8_t* const outp = lit + o;
    // Bh = bits of the stream not read yet (cursor from the top; the last byte carries the end mark).  A step decodes four
    // symbols (<= 44 bits) from ONE 8-byte window read at the cursor, no branches inside; the last symbols of a stream (fewer
    // than four left, or fewer than 44 bits) go one at a time, with the bits below the stream's first one read as zeros like
    // libzstd's container does.
    uint32_t hi = 0, Bh = 0; bool hdone = !mine;
    if (mine) {
        const uint32_t lastByte = sn ? pay[sbeg + sn - 1] : 0;
        if (lastByte == 0) { ok = false; hdone = true; }
        else Bh = 8 * (sn - 1) + dhb32(lastByte);
    }
    const uint32_t tableLog = L.hufLog, tmask = (1u << tableLog) - 1;
    for (;;) {
        const uint32_t myTop = hdone ? 0 : (Bh >> 3) + 8;                                  // bytes past the stream's end are zeros
        const uint32_t myWb = myTop > ZS_HWIN ? (myTop - ZS_HWIN + 15) & ~15u : 0;       // top - wb <= ZS_HWIN = one 16-byte piece per lane
        for (uint32_t s_ = 0; s_ < streams; s_++) {
            const uint32_t top = (uint32_t)__builtin_amdgcn_readlane(myTop, (int)s_), wb = (uint32_t)__builtin_amdgcn_readlane(myWb, (int)s_), beg = (uint32_t)__builtin_amdgcn_readlane(sbeg, (int)s_), n_ = (uint32_t)__builtin_amdgcn_readlane(sn, (int)s_);
            const uint32_t k = lane * 16;
            if (wb + k < top) {
                uint4 v;
                if (wb + k + 16 <= n_) __builtin_memcpy(&v, pay + beg + wb + k, 16);
                else { uint8_t tmp[16]; for (uint32_t j = 0; j < 16; j++) tmp[j] = wb + k + j < n_ ? pay[beg + wb + k + j] : 0; __builtin_memcpy(&v, tmp, 16); }
                *reinterpret_cast<uint4*>(&L.hwin[s_ * (ZS_HWIN + 16) + k]) = v;
            }
        }
        __threadfence_block();
        WAVE_SYNC();
        if (!hdone) {
            const uint8_t* const win = &L.hwin[lane * (ZS_HWIN + 16)];
            // five table reads per 8-byte window read: each yields the one to three symbols coded in the next 11 bits
            while (hi + 16 <= cnt && Bh >= 56 && ((Bh - 56) >> 3) >= myWb) {
                const uint32_t lo = Bh - 56;
                const uint64_t c = wld64(win, myWb, lo >> 3) >> (lo & 7);                 // bits [lo, lo + 56) of the stream
                uint32_t used = 0;
                #pragma unroll
                for (int k = 0; k < 5; k++) {
                    const uint32_t e = L.hufX[(uint32_t)(c >> (45 - used)) & 0x7FF];
                    const uint32_t sy = e & 0xFFFFFF;                                    // one byte of slack behind the symbols
                    __builtin_memcpy(outp + hi, &sy, 4);
                    hi += e >> 28; used += (e >> 24) & 15;
                }
                Bh -= used;
            }
            while (hi < cnt && (hi + 16 > cnt || Bh < 56)) {                               // the stream's tail, one symbol at a time
                const uint32_t need = Bh < tableLog ? Bh : tableLog, lo = Bh - need;
                if ((lo >> 3) < myWb) break;                                               // behind the window: refill first
                const uint32_t bits = (uint32_t)(wld64(win, myWb, lo >> 3) >> (lo & 7)) & ((1u << need) - 1);
                const uint32_t e = huf_decode1(L, (bits << (tableLog - need)) & tmask, tableLog);
                if ((e >> 8) > Bh) { ok = false; hdone = true; break; }                     // reads past the stream's first bit
                outp[hi++] = (uint8_t)e; Bh -= e >> 8;
            }
            if (!hdone && hi >= cnt) { if (Bh != 0) ok = false; hdone = true; }             // every bit used, none missing
        }
        WAVE_SYNC();
        if (__all(hdone)) break;
    }
    return !__any(!ok);
}

// Sequences-section header at q: the number of sequences and, when there are any, the Symbol_Compression_Modes byte.  ok = 0
// when it runs past the block, declares more sequences than a block can hold, sets the reserved mode bits, or - with no
// sequences - leaves bytes in the block.  t = the first table description.
struct DecSeqHdr { uint32_t ok, nbSeq, modes, t; };
__device__ __forceinline__ static DecSeqHdr dec_seq_header(const uint8_t* __restrict__ blk, uint32_t bsize, uint32_t q) {
    DecSeqHdr h; h.ok = 0; h.nbSeq = 0; h.modes = 0; h.t = 0;
    if (q >= bsize) return h;
    uint32_t nbSeq = blk[q];
    if (nbSeq < 128) q += 1;
    else if (nbSeq < 255) { if (q + 2 > bsize) return h; nbSeq = ((nbSeq - 128) << 8) + blk[q + 1]; q += 2; }
    else { if (q + 3 > bsize) return h; nbSeq = blk[q + 1] + ((uint32_t)blk[q + 2] << 8) + 0x7F00; q += 3; }
    h.nbSeq = nbSeq;
    if (nbSeq > ZS_BLOCK_MAX / 3 + 1) return h;                        // 128 KiB / minMatch 3 = 43691 at most in a valid block
    if (nbSeq == 0) { h.ok = q == bsize; return h; }
    if (q >= bsize) return h;
    h.modes = blk[q]; h.t = q + 1;
    h.ok = (h.modes & 3) == 0;
    return h;
}

// One of the three sequence tables (k: 0 literal lengths, 1 offsets, 2 match lengths) from its description: mode 0 predefined,
// 1 RLE, 2 FSE-compressed (a Repeat, mode 3, is the caller's).  Lane 0 parses the description (a short serial bit parse), the
// whole wave builds the table (fse_buildSeqTable_wave).  desc / avail: the description's bytes.  Returns the bytes it used, -1
// (wave-uniform) when the description is malformed.
__device__ __forceinline__ static int32_t dec_seq_table(DecLds& L, int k, uint32_t mode, const uint8_t* __restrict__ desc, uint32_t avail, uint32_t lane) {
    SeqD* const dt = k == 0 ? L.ll : k == 1 ? L.of : L.ml;
    uint32_t* const logp = k == 0 ? &L.llLog : k == 1 ? &L.ofLog : &L.mlLog;
    const uint32_t maxSymK = k == 0 ? 35 : k == 1 ? 31 : 52, maxLogK = k == 0 ? 9 : k == 1 ? 8 : 9;
    if (mode == 0) {
        const short* const dn = k == 0 ? dLLnorm : k == 1 ? dOFnorm : dMLnorm;
        const uint32_t dmax = k == 0 ? 35 : k == 1 ? 28 : 52, dlog = k == 1 ? 5 : 6;
        if (lane <= dmax) L.norm[lane] = dn[lane];
        if (lane == 0) *logp = dlog;
        __threadfence_block();
        WAVE_SYNC();
        return fse_buildSeqTable_wave(dt, L, dmax, dlog, k, lane) ? 0 : -1;
    }
    if (mode == 1) {                                                    // one symbol, no state bits
        if (avail < 1) return -1;
        const uint32_t sym = DUNI(desc[0]);
        if (sym > maxSymK) return -1;
        if (lane == 0) { dt[0] = SEQD(0, 0, seq_ebits(L, sym, k), sym); *logp = 0; }
        __threadfence_block();
        WAVE_SYNC();
        return 1;
    }
    if (avail < 1) return -1;
    if (lane == 0) {
        uint32_t ms = maxSymK, tl = 0;
        const uint32_t used = fse_readNCount(L.norm, &ms, &tl, desc, avail, maxLogK);
        L.scal[0] = used; L.scal[3] = ms; L.scal[4] = tl;
        if (used) *logp = tl;
    }
    __threadfence_block();
    WAVE_SYNC();
    const uint32_t used = DUNI(L.scal[0]), ms = DUNI(L.scal[3]), tl = DUNI(L.scal[4]);
    WAVE_SYNC();
    return used && fse_buildSeqTable_wave(dt, L, ms, tl, k, lane) ? (int32_t)used : -1;
}

// The sequence bit stream of a compressed block (bytes / n: behind the table descriptions, n >= 1) and where its decoding stands.
struct DecSeqStream { const uint8_t* bytes; uint32_t n, B, wbase, st; };   // B: bits not read yet (the cursor, from the top); st: this lane's state
// One group of up to 64 sequences, the first at index g of the block's nbSeq (cnt = min(64, nbSeq - g), wave-uniform): this
// lane's sequence g + lane -> its literal length, match length and offset code (offBase: 1..3 repeat, else offset + 3).  The
// tables are built (L.ll, L.of, L.ml and their logs, L.cLLbase / L.cMLbase, L.zeroEntry).  The first group also reads the end
// mark and the initial states.  The stream is one serial chain (read backwards; each FSE state transition says how many bits
// the next one reads), staged through an LDS window that the whole wave refills.  Only the part of a sequence that IS serial
// runs serially: pass 1 walks the three state machines (seq_chain_step) and leaves each sequence's states in L.rec; pass 2 lets
// every lane pull its sequence's extra bits out of the window - all 64 at once.  Returns false (wave-uniform) when the stream
// is malformed or shorter than its sequences need; whether every bit was used is the caller's check, after the last group.
__device__ __forceinline__ static bool dec_seq_group(DecLds& L, DecSeqStream& S, uint32_t g, uint32_t cnt, uint32_t nbSeq, uint32_t lane,
                                                     uint32_t& ll, uint32_t& ml, uint32_t& offBase) {
    const uint8_t* const win = L.swin + ZS_DPAD;
    if (g == 0) {                                                       // BIT_initDStream: the last byte carries the end mark
        const uint32_t lastByte = DUNI(S.bytes[S.n - 1]);
        if (lastByte == 0) return false;
        S.B = 8 * (S.n - 1) + dhb32(lastByte);
    }
    // 64 sequences read at most 64 * 89 bits = 712 bytes below the cursor; every read is an 8-byte load at byte (bit >> 3), so
    // the window holds [wbase, (B >> 3) + 8) with the bytes past the stream's end as zeros
    if (g == 0 || (S.wbase != 0 && (S.B >> 3) < S.wbase + 736)) {
        WAVE_SYNC();                                                    // everyone is done with the previous window
        const uint32_t top = (S.B >> 3) + 8;
        S.wbase = top > ZS_DWIN ? (top - ZS_DWIN) & ~15u : 0;
        for (uint32_t k = lane * 16; S.wbase + k < top; k += LANES * 16) {
            uint4 v;
            if (S.wbase + k + 16 <= S.n) __builtin_memcpy(&v, S.bytes + S.wbase + k, 16);
            else { uint8_t tmp[16]; for (uint32_t j = 0; j < 16; j++) tmp[j] = S.wbase + k + j < S.n ? S.bytes[S.wbase + k + j] : 0; __builtin_memcpy(&v, tmp, 16); }
            *reinterpret_cast<uint4*>(&L.swin[ZS_DPAD + k]) = v;
        }
        if (lane < ZS_DPAD / 4) reinterpret_cast<uint32_t*>(L.swin)[lane] = 0;      // the margin in front of the window
        __threadfence_block();
        WAVE_SYNC();
        if (g == 0) {                                                   // initial states: LL, OF, ML (ZSTD_initFseState order)
            const uint32_t llLog = DUNI(L.llLog), ofLog = DUNI(L.ofLog), mlLog = DUNI(L.mlLog);
            const uint32_t lo = S.B - (llLog + ofLog + mlLog);          // <= 26 bits
            if ((int32_t)lo < 0) return false;
            const uint32_t w = DUNI((uint32_t)(wld64(win, S.wbase, lo >> 3) >> (lo & 7)));
            const uint32_t sm = w & ((1u << mlLog) - 1), so = (w >> mlLog) & ((1u << ofLog) - 1), sl = (w >> (mlLog + ofLog)) & ((1u << llLog) - 1);
            S.st = lane == 0 ? sl : lane == 1 ? sm : lane == 2 ? so : 0;
            S.B = lo;
        }
    }
    // pass 1: the chain, on the vector unit (seq_chain_step).  An over-read shows as a negative cursor (collected in `bad`,
    // checked once per group).  The last sequence of a block reads no update bits: peeled off the loop.
    const SeqD* const tbl = lane == 0 ? L.ll : lane == 1 ? L.ml : lane == 2 ? L.of : &L.zeroEntry;   // lanes 3..63 carry state 0
    uint16_t* const recp = &L.rec[lane < 3 ? lane : 3];
    uint32_t bad = 0;
    const uint32_t Bgroup = S.B;
    const uint32_t upd = g + cnt < nbSeq ? cnt : cnt - 1;
    uint32_t j = 0;
    for (; j + 2 <= upd; j += 2) {                                      // two steps per trip: rec offsets become immediates, half the loop control
        seq_chain_step(tbl, recp + j * 4, win, S.wbase, S.st, S.B, bad);
        seq_chain_step(tbl, recp + j * 4 + 4, win, S.wbase, S.st, S.B, bad);
    }
    if (j < upd) seq_chain_step(tbl, recp + j * 4, win, S.wbase, S.st, S.B, bad);
    if (upd < cnt) {
        const uint32_t e_ = tbl[S.st];
        recp[upd * 4] = (uint16_t)S.st;
        const uint32_t eb = SEQD_EBITS(e_);
        const int32_t raw = (int32_t)(S.B - DUNI(eb + DPP_SHL(eb, 1) + DPP_SHL(eb, 2)));
        bad |= (uint32_t)raw;
        S.B = (uint32_t)(raw < 0 ? 0 : raw);
    }
    if (bad >> 31) return false;                                        // the stream is shorter than its sequences need
    __threadfence_block();
    WAVE_SYNC();
    // pass 2: every lane decodes the fields of its own sequence from the window; its cursor is the group's minus the bits of the
    // sequences before it (prefix sum)
    const bool valid = lane < cnt;
    ll = 0; ml = 0; offBase = 4;
    uint32_t el = 0, eo = 0, em = 0, mine = 0;
    if (valid) {
        uint64_t r; __builtin_memcpy(&r, &L.rec[lane * 4], 8);
        el = L.ll[(uint32_t)r & 0xFFFF]; em = L.ml[(uint32_t)(r >> 16) & 0xFFFF]; eo = L.of[(uint32_t)(r >> 32) & 0xFFFF];
        mine = SEQD_TOT(el) + SEQD_TOT(eo) + SEQD_TOT(em);
        if (g + lane + 1 == nbSeq) mine = SEQD_EBITS(el) + SEQD_EBITS(eo) + SEQD_EBITS(em);
    }
    uint32_t incl = mine;
    for (uint32_t o = 1; o < LANES; o <<= 1) { const uint32_t v = __shfl_up(incl, o); if (lane >= o) incl += v; }
    if (valid) {
        const uint32_t oc = SEQD_EBITS(eo), mbits = SEQD_EBITS(em), lbits = SEQD_EBITS(el);
        const uint32_t lbase = L.cLLbase[SEQD_SYM(el)], mbase = L.cMLbase[SEQD_SYM(em)];
        const uint32_t lo1 = Bgroup - (incl - mine) - oc;               // offset bits first (<= 31), then ML, then LL (<= 16 each)
        offBase = (1u << oc) + ((uint32_t)(wld64(win, S.wbase, lo1 >> 3) >> (lo1 & 7)) & ((1u << oc) - 1));
        const uint32_t lo2 = lo1 - mbits - lbits;
        const uint32_t w2 = (uint32_t)(wld64(win, S.wbase, lo2 >> 3) >> (lo2 & 7));
        ll = lbase + (w2 & ((1u << lbits) - 1));
        ml = mbase + ((w2 >> lbits) & ((1u << mbits) - 1));
    }
    return true;
}

// Pass 3 of the sequence stage: the repeat offsets of one group (offBase, ll, valid, cnt as dec_seq_group left them), given the
// history r0, r1, r2 the group starts from -> this lane's offset; the history is left as the next group finds it.  A sequence
// with a new offset (code > 3) knows it already and only pushes it onto the history; the scalar loop visits just the sequences
// that USE the history (codes 1..3), in order, first folding in the new offsets pushed since the previous visit (only the last
// three matter).  Code c names history entry idx = c - 1 (+ 1 when the literal length is 0; idx 3 = "rep0 - 1"); idx >= 2
// pushes the whole history down, idx 1 swaps the first two, idx 0 leaves it alone.  All on wave-uniform values, no branches.
// What an entry IS differs between the forms - a concrete offset, or a reference into a history the block does not know yet -
// and only "rep0 - 1" looks inside one: minus1(r0) is the caller's.
template <class Minus1>
__device__ __forceinline__ static uint32_t dec_rep_offsets(uint32_t offBase, uint32_t ll, bool valid, uint32_t cnt,
                                                           uint32_t& r0, uint32_t& r1, uint32_t& r2, Minus1 minus1) {
    uint32_t off = offBase - 3;
    const unsigned long long ll0 = __ballot(valid && ll == 0);
    unsigned long long users = __ballot(valid && offBase <= 3);
    r0 = DUNI(r0); r1 = DUNI(r1); r2 = DUNI(r2);                        // the history lives in SGPRs: the loop below is scalar
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
        const uint32_t c01 = idx == 0 ? r0 : r1, c23 = idx == 2 ? r2 : minus1(r0);
        const uint32_t o_ = idx < 2 ? c01 : c23;
        r2 = idx >= 2 ? r1 : r2;
        r1 = idx >= 1 ? r0 : r1;
        r0 = o_;
        off = tsx_writelane(o_, j, off);
        prev = j + 1;
    }
    return off;
}

// Inclusive scan of two values over the wave: positions from lengths (literal bytes and output bytes of a group's sequences).
__device__ __forceinline__ static void dec_incl_scan2(uint32_t& a, uint32_t& t, uint32_t lane) {
    for (int o = 1; o < LANES; o <<= 1) { const uint32_t x = __shfl_up(a, o), y = __shfl_up(t, o); if (lane >= (uint32_t)o) { a += x; t += y; } }
}

// Per-lane copy of a short, non-overlapping run (a literal run, or a match whose source is already final): up to four
// 8-byte loads are in flight before the first store, so a run of <= 32 bytes costs one memory round trip.
__device__ static __forceinline__ void copy_small(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t n) {
    uint32_t k = 0;
    while (n - k >= 32) {
        const uint64_t a = dld64(src + k), b = dld64(src + k + 8), c = dld64(src + k + 16), d = dld64(src + k + 24);
        __builtin_memcpy(dst + k, &a, 8); __builtin_memcpy(dst + k + 8, &b, 8); __builtin_memcpy(dst + k + 16, &c, 8); __builtin_memcpy(dst + k + 24, &d, 8);
        k += 32;
    }
    const uint32_t r = n - k;                                       // < 32
    uint64_t q0 = 0, q1 = 0, q2 = 0; uint32_t w = 0; uint16_t h = 0; uint8_t b1 = 0;
    const uint32_t nq = r >> 3;
    if (nq > 0) q0 = dld64(src + k);
    if (nq > 1) q1 = dld64(src + k + 8);
    if (nq > 2) q2 = dld64(src + k + 16);
    uint32_t t = k + 8 * nq;
    if (r & 4) { __builtin_memcpy(&w, src + t, 4); }
    if (r & 2) { __builtin_memcpy(&h, src + t + (r & 4), 2); }
    if (r & 1) { b1 = src[t + (r & 6)]; }
    if (nq > 0) __builtin_memcpy(dst + k, &q0, 8);
    if (nq > 1) __builtin_memcpy(dst + k + 8, &q1, 8);
    if (nq > 2) __builtin_memcpy(dst + k + 16, &q2, 8);
    if (r & 4) __builtin_memcpy(dst + t, &w, 4);
    if (r & 2) __builtin_memcpy(dst + t + (r & 4), &h, 2);
    if (r & 1) dst[t + (r & 6)] = b1;
}

// Non-overlapping copy by the whole wave (every lane calls it with the same arguments).
__device__ static __forceinline__ void copy_wave(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t n, uint32_t lane) {
    for (uint32_t k = lane * 8; k + 8 <= n; k += LANES * 8) { const uint64_t v = dld64(src + k); __builtin_memcpy(dst + k, &v, 8); }
    const uint32_t t = n & ~7u;
    if (lane < (n & 7)) dst[t + lane] = src[t + lane];
}
#define ZS_LONG_RUN 128u
#define ZS_DSEQ_CAP 43712u            /* >= 128 KiB / 3 sequences per block; 3 x 4 x cap bytes fit ZS_WS_SEQS and ZS_WS_STBITS.. */
static_assert(12u * ZS_DSEQ_CAP <= 16u * (ZS_MAX_SEQ + 64) && 12u * ZS_DSEQ_CAP <= 6u * ZS_WS_CODE_STRIDE + ZS_BLOCKOUT_CAP, "sequence arrays fit the workspace regions they borrow");
static_assert(ZS_WS_HASHLONG + (192u << 10) + ZS_BLOCK_MAX + 256 <= ZS_WS_SEQS, "literal buffers fit the hash-table region");
// One run per lane (mine = this lane has one): the short ones all at once, each by its own lane; the long ones one after the
// other, each by the whole wave (a single lane would spend one memory round trip per 32 bytes on them).
__device__ static __forceinline__ void exec_copies(uint8_t* dst, const uint8_t* src, uint32_t n, bool mine, uint32_t lane) {
    const bool big = mine && n > ZS_LONG_RUN;
    if (mine && !big) copy_small(dst, src, n);
    unsigned long long bigm = __ballot(big);
    const uint64_t d64 = (uint64_t)dst, s64 = (uint64_t)src;
    while (bigm) {
        const int i = __ffsll((long long)bigm) - 1;
        bigm &= bigm - 1;
        // readlane returns int: every half goes through uint32_t before it is widened (an OR-ed int sign-extends)
        const uint64_t d = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)(d64 >> 32), i) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)d64, i);
        const uint64_t s_ = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)(s64 >> 32), i) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)s64, i);
        copy_wave((uint8_t*)d, (const uint8_t*)s_, (uint32_t)__builtin_amdgcn_readlane(n, i), lane);
    }
}
