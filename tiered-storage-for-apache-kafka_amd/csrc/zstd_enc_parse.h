// Zstandard compressor, parse stage (included by zstd_enc.hip after zstd_enc_dev.h): the LDS source window (Win, ring*, win_append,
// win_ensure), the wave-wide byte counts, the hashes and tags of the table entries, and the two parsers of a block - match_block
// (double-fast, level 3) and fast_block (levels 1 and 2) - which leave sequences in the workspace and a summary in MfState.
// From EncLds the parsers are handed p.ring and p.scr (match_block) or p.ring (fast_block: unused, its window stays empty); while they
// run they may use only EncLds::p, which aliases everything of the entropy stage.  Their shared opening and closing lines stay written
// out twice: as force-inlined helpers they gave both hot loops another register allocation (profiles/enc_split_resource_usage.txt).
__device__ static inline uint32_t hash8(uint64_t u, uint32_t h) { return (uint32_t)((u * 0xCF1BBCDCB7A56463ULL) >> (64 - h)); }
__device__ static inline uint32_t hashS(uint64_t u, uint32_t h, uint32_t mls) {
    if (mls == 5) return (uint32_t)(((u << 24) * 889523592379ULL) >> (64 - h));
    return ((uint32_t)u * 2654435761U) >> (32 - h);                       // mls == 4
}

// ---- tagged table entries ------------------------------------------------------------------------------------
// libzstd's tables hold indices only, so every probe costs a read of the candidate's bytes - here a random HBM line per
// probe, nearly all of them for candidates that do not match.  The tables are private to the kernel, so an entry also
// carries, in the bits above the index, a tag hashed from exactly the bytes the serial code compares (8 for the long
// table, 4 for the short one): equal bytes imply equal tags, so a probe whose tag differs is rejected without touching
// the candidate and the parse is unchanged.  idxBits = bits of (chunk size + 2); 9 tag bits for a 4 MiB chunk.
__device__ static inline uint32_t tag8(uint64_t u, uint32_t hBitsL, uint32_t tagBits) {       // bits right below the long index
    return tagBits ? (uint32_t)(((u * 0xCF1BBCDCB7A56463ULL) << hBitsL) >> (64 - tagBits)) : 0u;
}
__device__ static inline uint32_t tag4(uint32_t u, uint32_t tagBits) { return tagBits ? (u * 0x85EBCA6Bu) >> (32 - tagBits) : 0u; }

// ---- the source window ------------------------------------------------------------------------------------
// Under 8 resident waves per CU every dependent global round trip costs a wave 800-2000 cycles (tools/ubench/lat.hip),
// and the serial parse needs the bytes around ip at every step: position hashing, repcode checks, match extension,
// complementary insertions.  So the parser keeps chunk bytes [lo, hi) (the last ~4 KiB and the next ~4 KiB) in an LDS
// ring, refilled 4 KiB at a time with coalesced 16-byte loads; only the hash tables and candidates older than the ring
// are read from global memory.  The ring aliases the entropy stage's scratch (EncLds) and is re-primed per block.
struct Win { uint32_t lo, hi; };      // wave-uniform

// The ring is ZS_RING bytes plus a 16-byte mirror of its first bytes, so an unaligned 8-byte read never has to wrap
// (gfx950 LDS reads need no alignment: one ds_read_b64 / ds_read_b32 each).
__device__ static inline uint64_t ring8(const uint32_t* ring, uint32_t p) {
    uint64_t v; __builtin_memcpy(&v, reinterpret_cast<const uint8_t*>(ring) + (p & (ZS_RING - 1)), 8); return v;
}
__device__ static inline uint32_t ring4(const uint32_t* ring, uint32_t p) {
    uint32_t v; __builtin_memcpy(&v, reinterpret_cast<const uint8_t*>(ring) + (p & (ZS_RING - 1)), 4); return v;
}
__device__ static inline uint32_t ring1(const uint32_t* ring, uint32_t p) { return reinterpret_cast<const uint8_t*>(ring)[p & (ZS_RING - 1)]; }

// Append chunk bytes [w.hi, w.hi + ZS_FILL) to the ring (16-byte pieces; pieces that start beyond the chunk are skipped
// by re-reading the last valid piece, so nothing outside the caller's buffer granule is touched).
template <class SP> __device__ __forceinline__ static void win_append(SP src, uint32_t lastPiece, uint32_t* ring, Win& w, uint32_t lane) {
    uint4 v[ZS_FILL / 1024];
    WAVE_MEM_SYNC();                                                  // (emulator) no lane may still be reading the slots replaced here
#pragma unroll
    for (uint32_t k = 0; k < ZS_FILL / 1024; k++) {
        uint32_t pp = w.hi + k * 1024 + lane * 16;
        if (pp > lastPiece) pp = lastPiece;
        v[k] = ld128a(src + pp);
    }
#pragma unroll
    for (uint32_t k = 0; k < ZS_FILL / 1024; k++)
        *reinterpret_cast<uint4*>(&ring[((w.hi + k * 1024 + lane * 16) >> 2) & ZS_RWM]) = v[k];
    if ((w.hi & (ZS_RING - 1)) == 0 && lane == 0) *reinterpret_cast<uint4*>(&ring[ZS_RING / 4]) = v[0];    // the mirror
    w.hi += ZS_FILL;
    if (w.hi - w.lo > ZS_RING) w.lo = w.hi - ZS_RING;
    WAVE_MEM_SYNC();
}
// make [ip, ip + ZS_SAFE) resident (or everything up to the end of the chunk)
template <class SP> __device__ __forceinline__ static void win_ensure(SP src, uint32_t srcCeil, uint32_t lastPiece, uint32_t* ring, Win& w,
                                                  uint32_t ip, uint32_t lane) {
    if (ip < w.lo || ip > w.hi + ZS_RING / 2) {                      // far jump: restart the ring behind ip
        WAVE_MEM_SYNC();
        const uint32_t base = ip > ZS_FILL ? (ip - ZS_FILL) & ~(ZS_FILL - 1) : 0;
        w.lo = w.hi = base;
    }
    while (ip + ZS_SAFE > w.hi && w.hi < srcCeil) win_append(src, lastPiece, ring, w, lane);
}

// number of equal bytes of src[a..] and src[b..] (b < a), not reading a-side bytes at or beyond iend: the continuation of a
// match beyond the 64 bytes the step's first comparison covers (rare; 64 lanes x 8 bytes per pass)
__device__ static uint32_t wave_count(const uint8_t* __restrict__ src, const uint32_t* ring, const Win w, uint32_t a, uint32_t b, uint32_t iend, uint32_t lane) {
    uint32_t total = 0;
    for (;;) {
        const uint32_t off = total + 8 * lane;
        uint32_t n = 8;
        if (a + total + 8 * LANES <= iend) {                         // every lane compares 8 whole bytes
            uint64_t x;
            if (a + total >= w.lo && a + total + 8 * LANES <= w.hi && b + total >= w.lo) x = ring8(ring, a + off) ^ ring8(ring, b + off);
            else { PCNT(21, 1); x = ld64(src + a + off) ^ ld64(src + b + off); }
            n = x ? (uint32_t)(__ffsll((long long)x) - 1) >> 3 : 8;
        } else {
            const uint32_t avail = (a + off < iend) ? iend - (a + off) : 0;
            if (avail >= 8) {
                uint64_t x = ld64(src + a + off) ^ ld64(src + b + off);
                n = x ? (uint32_t)(__ffsll((long long)x) - 1) >> 3 : 8;
            } else {
                n = 0;
                while (n < avail && src[a + off + n] == src[b + off + n]) n++;
            }
        }
        const unsigned long long m = __ballot(n < 8);
        if (m) {
            const int fl = __ffsll((long long)m) - 1;
            return total + 8 * (uint32_t)fl + __builtin_amdgcn_readlane(n, fl);
        }
        total += 8 * LANES;
    }
}

// backward extension: while (ip > anchor && match > low && src[ip-1] == src[match-1])
__device__ static uint32_t wave_count_back(const uint8_t* __restrict__ src, const uint32_t* ring, const Win w, uint32_t ip, uint32_t match, uint32_t anchor,
                                           uint32_t low, uint32_t lane) {
    uint32_t lim = ip - anchor;
    if (match - low < lim) lim = match - low;
    if (lim == 0) return 0;
    uint32_t done = 0;
    for (;;) {
        const uint32_t i = done + lane;
        bool ok = i < lim;
        const uint32_t j = ok ? i : done;
        if (ip <= w.hi && ip - done >= w.lo + LANES && match - done >= w.lo + LANES) ok = ok && ring1(ring, ip - 1 - j) == ring1(ring, match - 1 - j);
        else ok = ok && src[ip - 1 - i] == src[match - 1 - i];
        const unsigned long long m = __ballot(!ok);
        if (m) return done + (uint32_t)(__ffsll((long long)m) - 1);
        done += LANES;
    }
}

struct MfState { uint32_t nbSeq, litSize, lastLL, anchor; };

// The parser keeps the literals where they are: a sequence records where its literal run starts in the chunk and the
// entropy stage gathers them with all lanes (gather_literals) instead of copying on the serial critical path.

// ---------------------------------------------------------------------------------------------------
// double-fast match finder for one block (ZSTD_compressBlock_doubleFast_noDict_generic, speculative form).
// All "positions" are offsets within the chunk; table values are libzstd's indices = position + 2; rep[] is updated as the serial
// code does.  Everything that is the same for all lanes (ip, anchor, offsets, step...) is derived from ballots / readlanes so it
// lives in SGPRs and the control flow is scalar.  On log-like data 54 % of all sequences start at the FIRST position searched after
// the previous match and 69 % within two (tools/stats/parse_stats.c), and only a step's first event is ever used, hence:
//   * lane roles: lane 0 = the complementary insertion at curr + 2, lanes 1.. = consecutive positions from ip - 2 (lanes 1, 2 are
//     the complementary insertions at ip - 2 / ip - 1, lanes 3.. the K search positions, lane 3 + K the look-ahead for the "long
//     match at +1" rule, lane 63 fetches the bytes of the immediate-repcode check): the complementary insertions of the previous
//     match share the hash computation, the collision check and the store instructions of the next step;
//   * K starts at ZS_K0 (4) after a match and widens (ZS_K1 = 32, then 59) only while nothing is found;
//   * two lanes of a step that touch the same bucket are not patched up but avoided: a byte scoreboard in LDS (converging to the
//     lowest lane id per slot) finds the first lane with an earlier partner and the step is cut in front of it - before the table
//     loads are issued, so a cut costs no memory traffic; only the look-ahead lane is resolved exactly (one ballot);
//   * only the step's first (potential) event is verified: the wave compares the 64 bytes around that ONE candidate with the ring
//     (8 behind, 56 ahead: verification, forward and backward extension in one round trip, one byte per lane, one ballot); a
//     tag's false positive (1/512) is struck out and the next event of the same step taken.
// ---------------------------------------------------------------------------------------------------
#ifndef ZS_K0
#define ZS_K0 4u              /* search positions of the first step after a match */
#endif
#ifndef ZS_K1
#define ZS_K1 32u             /* ... of the second step; doubling from there */
#endif
#define ZS_KMAX 59u           /* lanes 3..61 search, 62 looks ahead, 63 serves the immediate repcode */
// the rare continuations (matches longer than the 64 bytes the first comparison covers) stay out of line
__device__ ZS_NOINLINE static uint32_t count_more(const uint8_t* __restrict__ src, const uint32_t* ring, const Win w, uint32_t a, uint32_t b, uint32_t iend, uint32_t lane) {
    return wave_count(src, ring, w, a, b, iend, lane);
}
__device__ ZS_NOINLINE static uint32_t count_more_back(const uint8_t* __restrict__ src, const uint32_t* ring, const Win w, uint32_t ip, uint32_t match, uint32_t anchor,
                                                       uint32_t low, uint32_t lane) {
    return wave_count_back(src, ring, w, ip, match, anchor, low, lane);
}

// bit i = lane i is valid and chunk byte pa + i - nb equals byte pb + i - nb (pb < pa).  Bytes come from the ring when the whole
// 64-byte span is resident, else from global memory (valid lanes only touch [0, srcSize)).
__device__ __forceinline__ static unsigned long long eq_mask(const gbytes_t src, const uint32_t* ring, const Win w, uint32_t pa, uint32_t pb,
                                                             uint32_t nb, bool valid, uint32_t lane) {
    const bool aR = pa >= w.lo + nb && pa + (64 - nb) <= w.hi;
    const bool bR = pb >= w.lo + nb && pb + (64 - nb) <= w.hi;
    const uint32_t ia = valid ? pa + lane - nb : pa, ib = valid ? pb + lane - nb : pb;
    uint32_t x, y;
    if (bR) y = ring1(ring, ib); else y = src[ib];
    if (aR) x = ring1(ring, ia); else x = src[ia];
    return __ballot(valid && x == y);
}
__device__ static inline uint32_t cto64(unsigned long long m) { return m == ~0ull ? 64u : (uint32_t)__ffsll((long long)~m) - 1; }

__device__ ZS_NOINLINE static void match_block(const uint8_t* __restrict__ src, const uint32_t srcSize_, const uint32_t blockStart,
                                                    const uint32_t blockSize_, uint32_t* __restrict__ hashLong, uint32_t* __restrict__ hashSmall,
                                                    const zs_cparams cp, const uint32_t dictLimitIn, uint32_t* rep, zs_seq* __restrict__ seqs,
                                                    MfState& ms, uint32_t* ring, uint8_t* scr, const uint32_t lane, const uint32_t sched) {
    // Speculation schedule (never changes the output, only what a search run costs): positions of the first step after a match, of the
    // second step; doubling from there.  sched = K0 | K1 << 8, 0 in a field = the compile-time default (4, 32).  Measured with 18-step
    // runs, three batches in flight / one at a time (profiles/r02_sweep_k_schedule.txt): (2,16) 17.6-17.9 GiB/s / 762 ms, (3,24) 18.5-18.6 /
    // 729-735, (4,32) 18.8 / 719, (4,48) 18.8 / 725, (6,32) 18.75 / 723: the dependent round trips a wider step saves are worth more than
    // the table lines it wastes, on a full chip too.  (Sweeps of 6 steps had said the opposite - their start-up transient dominates.)
    // Round 3 tried to bound a step by a PREDICTOR as well: a 256-byte recency filter over the 4-grams of the bytes already parsed says
    // for every search lane whether the tail of its 8-byte window has been seen lately (on log-like content the first event of a run sits
    // where the window turns from novel bytes into recurring ones).  On the exact parse it cuts the speculative reads from 15.8 to 5.3
    // per sequence at fewer steps (tools/stats/step_sim.c, profiles/r03_step_sim_K.txt) - and on the device it LOSES: 18.6-18.8 GiB/s
    // against 19.2-19.4 in flight, 9.6 against 10.3 one batch at a time (three alternating rounds, profiles/r03_gram_predictor_ab.txt),
    // like round 2's event-position predictor: ~16 instructions and two LDS round trips per step on the serial path cost more than the
    // table lines they save.  The code is in the history (commit "Parser: 4-gram recency predictor"), not in the kernel.
    const uint32_t kFirst = (UNI(sched) & 0xFF) ? (UNI(sched) & 0xFF) : ZS_K0, kSecond = ((UNI(sched) >> 8) & 0xFF) ? ((UNI(sched) >> 8) & 0xFF) : ZS_K1;
    const gbytes_t gsrc = (gbytes_t)uni_ptr(src);
    const gwords_t gL = (gwords_t)uni_ptr(hashLong), gS = (gwords_t)uni_ptr(hashSmall);
    ZS_GLOBAL zs_seq* const gseqs = (ZS_GLOBAL zs_seq*)uni_ptr(seqs);
    const uint32_t srcSize = UNI(srcSize_);
    uint32_t nbSeq = 0, litSize = 0;
    static_assert(sizeof(zs_seq) == 16, "zs_put_seq writes the four fields as one 16-byte store");
    const uint32_t iend = UNI(blockStart + blockSize_), blockSize = UNI(blockSize_), dictLimit = UNI(dictLimitIn), maxDist = 1u << UNI(cp.windowLog);
    const uint32_t plowIdx = (iend + 2 - dictLimit > maxDist) ? iend + 2 - maxDist : dictLimit;
    const uint32_t hBitsL = UNI(cp.hashLog), hBitsS = UNI(cp.chainLog), mls = UNI(cp.minMatch);
    const uint32_t srcCeil = (srcSize + ZS_FILL - 1) & ~(ZS_FILL - 1), lastPiece = (srcSize - 1) & ~15u;
    const uint32_t idxBits = 32u - (uint32_t)__clz((int)(srcSize + 2)), tagBits = 32u - idxBits, idxMask = (uint32_t)((1ull << idxBits) - 1);
    uint32_t ip = UNI(blockStart), anchor = ip;
    uint32_t off1 = UNI(rep[0]), off2 = UNI(rep[1]), sav1 = 0, sav2 = 0;
    if (ip + 2 == plowIdx) ip++;
    {   const uint32_t cur = ip + 2, windowLow = (cur - dictLimit > maxDist) ? cur - maxDist : dictLimit, maxRep = cur - windowLow;
        if (off2 > maxRep) { sav2 = off2; off2 = 0; }
        if (off1 > maxRep) { sav1 = off1; off1 = 0; }
    }
    Win w; w.lo = w.hi = 0;
#define STORE_SEQ(ll_, lp_, ob_, ml_) do { if (lane == 0) zs_put_seq(&gseqs[nbSeq], (ob_), (ll_), (ml_) - 3, (lp_)); \
                                           litSize += (ll_); nbSeq++; } while (0)
    if (blockSize >= 8) {
        const uint32_t ilimit = iend - 8;
        bool afterMatch = false;          // the immediate-repcode check (offset_2 at ip) of the match just stored is still due
        bool comp = false;                // ... and so are its complementary insertions (X = curr + 2, ip - 2, ip - 1)
        bool runStart = true;
        uint32_t X = 0, step = 1, nextStep = 0, width = kFirst;
        for (;;) {                                                    // one iteration per wave step
            if (runStart) { step = 1; nextStep = ip + 256; width = kFirst; runStart = false; }
            uint32_t K = 0;
            const bool tail = ip + step > ilimit;
            if (tail) {
                if (!(ip <= ilimit && (comp || afterMatch))) break;
            } else {
                if (step == 1) {
                    K = ilimit - ip;
                    const uint32_t K1 = nextStep > ip + 1 ? nextStep - ip : 1;
                    if (K1 < K) K = K1;
                } else {
                    uint32_t K1 = 1;
                    if (nextStep > ip + step) K1 = (nextStep - ip - 1) / step + 1;
                    K = (ilimit - step - ip) / step + 1;
                    if (K1 < K) K = K1;
                }
                if (width < K) K = width;
            }
            if (ip + ZS_SAFE > w.hi || ip < w.lo) win_ensure(gsrc, srcCeil, lastPiece, ring, w, ip, lane);
            // ---- positions, hashes, table entries ----
            const uint32_t pos = lane == 0 ? X : lane < 3 ? ip + lane - 3 : ip + (lane - 3) * step;
            const bool compL = comp && lane < 2, compS = comp && (lane == 0 || lane == 2);
            bool searching = lane >= 3 && lane < 3 + K;
            const bool lane3 = lane == 3;                             // ip itself: searched (K > 0) or only checked for the immediate repcode
            const bool mayUse = compL || compS || (lane >= 3 && lane <= 3 + K);
            const uint32_t spos = mayUse ? pos : ip;                  // an address every lane may read
            const bool posWin = ip + K * step + 8 <= w.hi && (!comp || (X >= w.lo && ip >= w.lo + 2));
            uint64_t d8;
            if (posWin) d8 = ring8(ring, spos); else { d8 = gld64(gsrc + spos); LOADED64(d8); }
            const uint32_t hl = hash8(d8, hBitsL), hs = hashS(d8, hBitsS, mls);
            const uint32_t tL = tag8(d8, hBitsL, tagBits), tS = tag4((uint32_t)d8, tagBits);
            const uint32_t eL = ((tL << 1) << (idxBits - 1)) | (pos + 2), eS = ((tS << 1) << (idxBits - 1)) | (pos + 2);
            // ---- repcode pre-check: with the bytes at pos + 1 - off1 in the ring the first repcode hit is known before any probe ----
            const bool r1Near = K > 0 && off1 > 0 && posWin && ip + 1 >= w.lo + off1;
            uint32_t r1 = 0;
            if (r1Near) {
                r1 = ring4(ring, searching ? pos + 1 - off1 : ip);
                const unsigned long long rb = __ballot(searching && r1 == (uint32_t)(d8 >> 8));
                if (rb) { const uint32_t fr = (uint32_t)__ffsll((long long)rb) - 1; K = fr - 2; searching = lane >= 3 && lane <= fr; }
            }
            // ---- two lanes, one bucket: find the first lane with an earlier partner and stop in front of it ----
            bool shadowL0 = false, shadowS0 = false;                  // lane 0's insertion is overwritten by lane 1's / lane 2's
            if (comp) {
                shadowL0 = __builtin_amdgcn_readlane(hl, 0) == __builtin_amdgcn_readlane(hl, 1);
                shadowS0 = __builtin_amdgcn_readlane(hs, 0) == __builtin_amdgcn_readlane(hs, 2);
            }
            bool flagLook = false;
            if (K > 0) {
                const bool partL = compL || (lane >= 3 && lane <= 3 + K), partS = compS || searching;
                const uint32_t sl = hl & (ZS_SCR - 1), ss = ZS_SCR + (hs & (ZS_SCR - 1));
                WAVE_MEM_SYNC();
                if (partL) scr[sl] = (uint8_t)lane;
                if (partS) scr[ss] = (uint8_t)lane;
                WAVE_MEM_SYNC();
                uint32_t rL = partL ? scr[sl] : lane, rS = partS ? scr[ss] : lane;
                while (__any(lane < rL || lane < rS)) {               // converge on the lowest lane id of every shared slot
                    WAVE_MEM_SYNC();
                    if (lane < rL) scr[sl] = (uint8_t)lane;
                    if (lane < rS) scr[ss] = (uint8_t)lane;
                    WAVE_MEM_SYNC();
                    rL = partL ? scr[sl] : lane; rS = partS ? scr[ss] : lane;
                }
                const unsigned long long fb = __ballot(lane >= 3 && (rL < lane || rS < lane));
                if (fb) {
                    const uint32_t t = (uint32_t)__ffsll((long long)fb) - 1;
                    if (t == 3) {
                        // ip itself shares a slot with a complementary insertion: make those first, then search
                        if (lane == 0) { if (!shadowL0) gL[hl] = eL; if (!shadowS0) gS[hs] = eS; }
                        if (lane == 1) gL[hl] = eL;
                        if (lane == 2) gS[hs] = eS;
                        comp = false;
                        PCNT(19, 1);
                        continue;
                    }
                    if (t <= 3 + K) {                                 // lanes 3 .. t - 1 search, lane t looks ahead
                        if (t < 3 + K) PCNT(19, 1);
                        K = t - 3; searching = searching && lane < t; flagLook = true;
                    }
                }
            }
            const uint32_t look = 3 + K;
            // ---- probes (K + 1 long, K short), the far bytes of the repcode checks ----
            const bool probeL = K > 0 && lane >= 3 && lane <= look, probeS = searching;
            const uint32_t hl3 = __builtin_amdgcn_readlane(hl, 3), hs3 = __builtin_amdgcn_readlane(hs, 3);
            uint32_t cL = 0, cS = 0;
            if (K > 0) {
                cL = gL[probeL ? hl : hl3];
                cS = gS[probeS ? hs : hs3];
            }
            const bool r2Near = afterMatch && posWin && ip >= w.lo + off2;
            const bool needFar = (K > 0 && off1 > 0 && !r1Near) || (afterMatch && !r2Near);
            uint32_t rfar = 0;
            if (needFar) {
                uint32_t fa = (searching && off1 > 0) ? pos + 1 - off1 : ip;
                if (lane == 63 && afterMatch) fa = ip - off2;
                rfar = gld32(gsrc + fa);
            }
            if (K > 0 && off1 > 0 && !r1Near) r1 = rfar;
            PCNT(12, 1); PCNT(15, K);
            // ---- the immediate repcode of the previous match (offset_2 at ip) ----
            if (afterMatch) {
                afterMatch = false;
                const uint32_t r2 = r2Near ? ring4(ring, ip - off2) : (uint32_t)__builtin_amdgcn_readlane(rfar, 63);
                const uint32_t d0 = __builtin_amdgcn_readlane((uint32_t)d8, 3);
                if (UNI(r2) == d0) {
                    const uint32_t a = ip + 4;
                    uint32_t n = cto64(eq_mask(gsrc, ring, w, a, a - off2, 0, a + lane < iend, lane));
                    if (n == 64) n += UNI(count_more(src, ring, w, a + 64, a + 64 - off2, iend, lane));
                    const uint32_t rlen = 4 + n;
                    const uint32_t t = off2; off2 = off1; off1 = t;
                    if (comp) {
                        if (lane == 0) { if (!shadowL0) gL[hl] = eL; if (!shadowS0) gS[hs] = eS; }
                        if (lane == 1) gL[hl] = eL;
                        if (lane == 2) gS[hs] = eS;
                        comp = false;
                    }
                    WAVE_MEM_SYNC();                                  // (emulator) the insertion at ip comes after the complementary ones
                    if (lane3) { gS[hs] = eS; gL[hl] = eL; }
                    STORE_SEQ(0, ip, 1, rlen);
                    ip += rlen; anchor = ip;
                    PCNT(13, 1);
                    afterMatch = ip <= ilimit && off2 > 0;
                    runStart = true;
                    continue;
                }
            }
            // ---- the look-ahead lane sees the insertion an earlier lane of this step makes into its bucket ----
            if (flagLook) {
                const uint32_t hk = __builtin_amdgcn_readlane(hl, look);
                const unsigned long long em = __ballot((compL || searching) && hl == hk && !(lane == 0 && shadowL0));
                if (em) {
                    const uint32_t e = 63u - (uint32_t)__clzll((long long)em); const uint32_t ee = __builtin_amdgcn_readlane(eL, e);
                    if (lane == look) cL = ee;
                }
            }
            // ---- events ----
            const uint32_t iL = cL & idxMask, iS = cS & idxMask;
            bool vL = probeL && iL >= plowIdx && ((cL ^ eL) & ~idxMask) == 0;        // in the window and same tag
            bool vS = probeS && iS >= plowIdx && ((cS ^ eS) & ~idxMask) == 0;
            const bool repOK = searching && off1 > 0 && r1 == (uint32_t)(d8 >> 8);
            int f = -1;
            uint32_t start = 0, mlen = 0, offBase = 0;
            bool isRep = false;
            for (;;) {
                const uint32_t ev = !searching ? 0u : repOK ? 1u : vL ? 2u : vS ? 3u : 0u;
                const unsigned long long bm = __ballot(ev != 0);
                if (!bm) { f = -1; break; }
                f = __ffsll((long long)bm) - 1;
                const uint32_t evf = __builtin_amdgcn_readlane(ev, f);
                const uint32_t posf = ip + ((uint32_t)f - 3) * step;
                if (evf == 1) {                                       // repcode at posf + 1
                    start = posf + 1;
                    const uint32_t a = start + 4;
                    uint32_t n = cto64(eq_mask(gsrc, ring, w, a, a - off1, 0, a + lane < iend, lane));
                    if (n == 64) n += UNI(count_more(src, ring, w, a + 64, a + 64 - off1, iend, lane));
                    mlen = 4 + n; offBase = 1; isRep = true;
                    break;
                }
                const uint32_t lowPos = plowIdx - 2;
                if (evf == 2) {                                       // long match at posf
                    uint32_t mpos = __builtin_amdgcn_readlane(iL, f) - 2;
                    uint32_t lim = posf - anchor; if (mpos - lowPos < lim) lim = mpos - lowPos;
                    const bool valid = lane < 8 ? (8 - lane) <= lim : posf + (lane - 8) < iend;
                    const unsigned long long m = eq_mask(gsrc, ring, w, posf, mpos, 8, valid, lane);
                    if (((m >> 8) & 0xFF) != 0xFF) { if (lane == (uint32_t)f) vL = false; PCNT(21, 1); continue; }     // a tag's false positive
                    uint32_t fwd = cto64(m >> 8);
                    if (fwd == 56) fwd += UNI(count_more(src, ring, w, posf + 56, mpos + 56, iend, lane));
                    uint32_t back = (uint32_t)__clz((int)~(((uint32_t)m & 0xFF) << 24));
                    if (back == 8 && lim > 8) back += UNI(count_more_back(src, ring, w, posf - 8, mpos - 8, anchor, lowPos, lane));
                    start = posf - back; mpos -= back; mlen = fwd + back;
                    offBase = start - mpos + 3;
                    break;
                }
                {                                                     // short match at posf; a strictly longer long match at +1 wins
                    uint32_t mpos = __builtin_amdgcn_readlane(iS, f) - 2;
                    uint32_t lim = posf - anchor; if (mpos - lowPos < lim) lim = mpos - lowPos;
                    const bool valid = lane < 8 ? (8 - lane) <= lim : posf + (lane - 8) < iend;
                    unsigned long long m = eq_mask(gsrc, ring, w, posf, mpos, 8, valid, lane);
                    if (((m >> 8) & 0xF) != 0xF) { if (lane == (uint32_t)f) vS = false; PCNT(21, 1); continue; }
                    uint32_t fwd = cto64(m >> 8);
                    if (fwd == 56) fwd += UNI(count_more(src, ring, w, posf + 56, mpos + 56, iend, lane));
                    uint32_t sp = posf;
                    if (__builtin_amdgcn_readlane((uint32_t)vL, f + 1)) {
                        const uint32_t p1 = posf + step, m1 = __builtin_amdgcn_readlane(iL, f + 1) - 2;
                        uint32_t lim1 = p1 - anchor; if (m1 - lowPos < lim1) lim1 = m1 - lowPos;
                        const bool valid1 = lane < 8 ? (8 - lane) <= lim1 : p1 + (lane - 8) < iend;
                        const unsigned long long mm = eq_mask(gsrc, ring, w, p1, m1, 8, valid1, lane);
                        if (((mm >> 8) & 0xFF) == 0xFF) {
                            uint32_t f1 = cto64(mm >> 8);
                            if (f1 == 56) f1 += UNI(count_more(src, ring, w, p1 + 56, m1 + 56, iend, lane));
                            if (f1 > fwd) { sp = p1; mpos = m1; fwd = f1; m = mm; lim = lim1; }
                        }
                    }
                    uint32_t back = (uint32_t)__clz((int)~(((uint32_t)m & 0xFF) << 24));
                    if (back == 8 && lim > 8) back += UNI(count_more_back(src, ring, w, sp - 8, mpos - 8, anchor, lowPos, lane));
                    start = sp - back; mpos -= back; mlen = fwd + back;
                    offBase = start - mpos + 3;
                    break;
                }
            }
            // ---- commit: the visited positions insert themselves, then the pending complementary insertions ----
            const uint32_t lastIns = f >= 0 ? (uint32_t)f : 2 + K;
            if (lane >= 3 && lane <= lastIns) { gL[hl] = eL; gS[hs] = eS; }
            if (comp) {
                if (lane == 0) { if (!shadowL0) gL[hl] = eL; if (!shadowS0) gS[hs] = eS; }
                if (lane == 1) gL[hl] = eL;
                if (lane == 2) gS[hs] = eS;
                comp = false;
            }
            if (f < 0) {
                if (tail) break;
                const bool inc = ip + K * step >= nextStep;
                ip += K * step;
                if (inc) { step++; nextStep += 256; }
                width = width < kSecond ? kSecond : (width * 2 > ZS_KMAX ? ZS_KMAX : width * 2);
                continue;
            }
            if (!isRep) {
                off2 = off1; off1 = offBase - 3;
                WAVE_MEM_SYNC();                                      // (emulator) ... after the insertions of the visited positions
                if (step < 4 && lane == (uint32_t)f + 1) gL[hl] = eL;              // hashLong[hl1] = ip1
            }
            STORE_SEQ(start - anchor, anchor, offBase, mlen);
            X = ip + ((uint32_t)f - 3) * step + 2;                    // curr + 2
            ip = UNI(start + mlen); anchor = ip;
            off1 = UNI(off1); off2 = UNI(off2);
            PCNT(13, 1);
            comp = ip <= ilimit;
            afterMatch = comp && off2 > 0;
            runStart = true;
        }
    }
    sav2 = (sav1 != 0 && off1 != 0) ? sav1 : sav2;
    rep[0] = off1 ? off1 : sav1;
    rep[1] = off2 ? off2 : sav2;
    ms.nbSeq = nbSeq; ms.lastLL = iend - anchor; ms.anchor = anchor;
    ms.litSize = litSize + ms.lastLL;
#undef STORE_SEQ
    PT(4);
}

// ---------------------------------------------------------------------------------------------------
// fast match finder for one block (strategy fast, levels 1 and 2: ZSTD_compressBlock_fast_noDict_generic of libzstd 1.5.x).
// The serial code visits positions in pairs (a, a + 1); the next pair starts `step` further on (2 after every match, + 1 each 128 bytes
// without one), and each pair is preceded by a repcode check at the first position of the pair after it.  For every position it reads
// the table entry, writes its own index there and compares 4 bytes with the candidate, so a table ends up holding the last position of
// each bucket.  Here one wave step takes up to 31 pairs (two lanes each) at once: every lane hashes its position, a lane whose bucket an
// earlier lane of the step shares takes that lane's position as its candidate instead of the table's (what the serial read would see),
// and of the events in serial order (repcode at the next pair, match at a, match at a + 1) the first one wins.  The writes the serial
// code made up to that event are committed, one lane per bucket (the last one).  Table values are libzstd's indices = position + 2.
// ---------------------------------------------------------------------------------------------------
__device__ static inline uint32_t hashF(uint64_t u, uint32_t h, uint32_t mls) {
    if (mls == 5) return (uint32_t)(((u << 24) * 889523592379ULL) >> (64 - h));
    if (mls == 6) return (uint32_t)(((u << 16) * 227718039650203ULL) >> (64 - h));
    if (mls == 7) return (uint32_t)(((u << 8) * 58295818150454627ULL) >> (64 - h));
    return ((uint32_t)u * 2654435761U) >> (32 - h);                       // mls == 4
}
#define ZS_FAST_PAIRS0 4u     /* pairs of the first wave step after a match (most matches follow within a few positions) */
#define ZS_FAST_PAIRS 31u     /* ... of every later step (lane 2 x 31 = 62 holds the first position of the pair after the last) */
__device__ ZS_NOINLINE static void fast_block(const uint8_t* __restrict__ src, const uint32_t blockStart, const uint32_t blockSize_,
                                              uint32_t* __restrict__ table, const zs_cparams cp, const uint32_t dictLimitIn, uint32_t* rep,
                                              zs_seq* __restrict__ seqs, MfState& ms, uint32_t* ring, const uint32_t lane) {
    const gbytes_t gsrc = (gbytes_t)uni_ptr(src);
    const gwords_t gT = (gwords_t)uni_ptr(table);
    ZS_GLOBAL zs_seq* const gseqs = (ZS_GLOBAL zs_seq*)uni_ptr(seqs);
    const uint32_t iend = UNI(blockStart + blockSize_), dictLimit = UNI(dictLimitIn), maxDist = 1u << UNI(cp.windowLog);
    const uint32_t plowIdx = (iend + 2 - dictLimit > maxDist) ? iend + 2 - maxDist : dictLimit;    // prefixStartIndex
    const uint32_t lowPos = plowIdx - 2;
    const uint32_t hlog = UNI(cp.hashLog), mls = UNI(cp.minMatch);
    uint32_t nbSeq = 0, litSize = 0;
    uint32_t ip = UNI(blockStart), anchor = ip;
    uint32_t off1 = UNI(rep[0]), off2 = UNI(rep[1]), sav1 = 0, sav2 = 0;
    if (ip + 2 == plowIdx) ip++;
    {   const uint32_t cur = ip + 2, windowLow = (cur - dictLimit > maxDist) ? cur - maxDist : dictLimit, maxRep = cur - windowLow;
        if (off2 > maxRep) { sav2 = off2; off2 = 0; }
        if (off1 > maxRep) { sav1 = off1; off1 = 0; }
    }
    Win w; w.lo = w.hi = 0;                                           // no LDS window: the count helpers read global memory
#define STORE_SEQ(ll_, lp_, ob_, ml_) do { if (lane == 0) zs_put_seq(&gseqs[nbSeq], (ob_), (ll_), (ml_) - 3, (lp_)); \
                                           litSize += (ll_); nbSeq++; } while (0)
    if (blockSize_ >= 8) {
        const uint32_t ilimit = iend - 8;
        const uint32_t jl = lane >> 1, role = lane & 1u;
        for (;;) {                                                    // _start: a match ended at ip (or the block begins)
            uint32_t a = ip, an = ip + 2, s = 2, ns = ip + 128;       // pair k: a_k, a_(k+1), step of iteration k, nextStep
            if (an + 1 >= ilimit) break;
            uint32_t np = ZS_FAST_PAIRS0;
            uint32_t evType = 0, evLane = 0;
            for (;;) {                                                // one wave step: pairs 0 .. np - 1 from (a, an, s, ns)
                uint32_t la = 0, lan = 0, ls = 0, lns = 0;            // this lane's pair: a_j, a_(j+1), step and nextStep of iteration j
                uint32_t ta = a, tan = an, tsv = s, tns = ns;
                for (uint32_t j = 0; j <= np; j++) {
                    if (j == jl) { la = ta; lan = tan; ls = tsv; lns = tns; }
                    const uint32_t nn = tan + tsv;                    // a_(j+2)
                    ta = tan; tan = nn;
                    if (nn >= tns) { tsv++; tns += 128; }
                }
                const uint32_t pos = la + role;
                const bool inPair = jl < np && lan + 1 < ilimit;      // iteration j runs (ip3 < ilimit)
                const bool hashed = jl <= np && pos <= ilimit;       // (+ the first position after the last pair: the write a match at a + 1 may add)
                const uint64_t d8 = gld64(gsrc + (hashed ? pos : ip));
                const uint32_t h = hashed ? hashF(d8, hlog, mls) : 0xFFFFFFFFu;
                // the serial read of this position comes after the writes of every earlier lane's position
                uint32_t cand = 0, later = 64;
                bool local = false;
                const uint32_t last = 2 * np;
                for (uint32_t i = 0; i <= last; i++) {
                    const uint32_t hi = __builtin_amdgcn_readlane(h, i), pi = __builtin_amdgcn_readlane(pos, i);
                    if (hi == h) {
                        if (i < lane) { cand = pi + 2; local = true; }
                        else if (i > lane && later == 64) later = i;
                    }
                }
                if (inPair && !local) cand = gT[h];
                bool mOK = false, rOK = false;
                if (inPair && cand >= plowIdx) mOK = gld32(gsrc + (cand - 2)) == (uint32_t)d8;
                if (inPair && role == 0 && off1 > 0 && lan >= off1) rOK = gld32(gsrc + lan) == gld32(gsrc + (lan - off1));
                const unsigned long long evm = __ballot(mOK || rOK);
                const unsigned long long validm = __ballot(inPair);
                uint32_t lastLane;                                    // writes of lanes 0 .. lastLane are committed
                if (evm) {
                    evLane = (uint32_t)__ffsll((long long)evm) - 1;
                    const uint32_t rf = __builtin_amdgcn_readlane((uint32_t)rOK, evLane);
                    evType = (evLane & 1u) ? 3u : rf ? 1u : 2u;       // 1 repcode at the next pair, 2 match at a, 3 match at a + 1
                    lastLane = (evLane | 1u);
                    if (evType == 3 && __builtin_amdgcn_readlane(ls, evLane) <= 4) lastLane++;
                } else {
                    lastLane = validm ? 63u - (uint32_t)__clzll((long long)validm) : 0u;
                }
                if (validm && lane <= lastLane && later > lastLane) gT[h] = pos + 2;
                if (evm) {
                    // ---- the event: sequence, table fill, immediate repcodes ----
                    const uint32_t pf = __builtin_amdgcn_readlane(pos, evLane);
                    const uint32_t cur0 = pf;                         // (the serial code's current0: the pair's a for a repcode)
                    uint32_t st, mpos, mlen, offBase;
                    if (evType == 1) {
                        st = __builtin_amdgcn_readlane(lan, evLane); mpos = st - off1;
                        const uint32_t b1 = src[st - 1] == src[mpos - 1];
                        st -= b1; mpos -= b1; mlen = 4 + b1; offBase = 1;
                    } else {
                        mpos = __builtin_amdgcn_readlane(cand, evLane) - 2;
                        off2 = off1; off1 = pf - mpos; offBase = off1 + 3;
                        const uint32_t back = UNI(count_more_back(src, ring, w, pf, mpos, anchor, lowPos, lane));
                        st = pf - back; mpos -= back; mlen = 4 + back;
                    }
                    mlen += UNI(count_more(src, ring, w, st + mlen, mpos + mlen, iend, lane));
                    STORE_SEQ(st - anchor, anchor, offBase, mlen);
                    ip = UNI(st + mlen); anchor = ip;
                    off1 = UNI(off1); off2 = UNI(off2);
                    if (ip <= ilimit) {
                        WAVE_MEM_SYNC();                              // (emulator) after the step's own writes
                        if (lane == 0) {
                            gT[hashF(gld64(gsrc + cur0 + 2), hlog, mls)] = cur0 + 4;
                            gT[hashF(gld64(gsrc + ip - 2), hlog, mls)] = ip;
                        }
                        while (off2 > 0 && ip <= ilimit && gld32(gsrc + ip) == gld32(gsrc + (ip - off2))) {
                            const uint32_t rl = 4 + UNI(count_more(src, ring, w, ip + 4, ip + 4 - off2, iend, lane));
                            const uint32_t t = off2; off2 = off1; off1 = t;
                            WAVE_MEM_SYNC();
                            if (lane == 0) gT[hashF(gld64(gsrc + ip), hlog, mls)] = ip + 2;
                            STORE_SEQ(0, ip, 1, rl);
                            ip += rl; anchor = ip;
                        }
                    }
                    WAVE_MEM_SYNC();
                    break;
                }
                if (!validm || __builtin_amdgcn_readlane((uint32_t)inPair, 2 * np - 2) == 0) { evType = 4; break; }    // the block's tail
                // no event: go on from pair np
                a = __builtin_amdgcn_readlane(la, 2 * np); an = __builtin_amdgcn_readlane(lan, 2 * np);
                s = __builtin_amdgcn_readlane(ls, 2 * np); ns = __builtin_amdgcn_readlane(lns, 2 * np);
                WAVE_MEM_SYNC();
                np = ZS_FAST_PAIRS;
            }
            if (evType == 4) break;
        }
    }
    sav2 = (sav1 != 0 && off1 != 0) ? sav1 : sav2;
    rep[0] = off1 ? off1 : sav1;
    rep[1] = off2 ? off2 : sav2;
    ms.nbSeq = nbSeq; ms.lastLL = iend - anchor; ms.anchor = anchor;
    ms.litSize = litSize + ms.lastLL;
#undef STORE_SEQ
}
