// Zstandard compressor, parse stage of TSX_ZSTD_PROFILE_DEVICE (included by zstd_enc.hip after zstd_enc_parse.h): device_block, a
// parse shaped for the wave instead of for libzstd's bytes.  It leaves what match_block and fast_block leave - zs_seq records in the
// chunk's sequence array, a summary in MfState, the repeat-offset history - and everything behind it (gather_literals, the entropy
// stages, the frame loop) is shared with them.  The frames are standard Zstandard; they are not any libzstd's bytes.
//
//  * Slices.  A block of n bytes is cut into 64 slices of max(ceil(n / 64), 64) bytes (2 KiB for a full block); lane j parses slice j
//    greedily.  A match starts in the lane's slice and ends at the slice's end at the latest; its source lies anywhere earlier in the
//    chunk, inside the window.  So the wave keeps 64 independent probe chains in flight where the exact parsers keep one.
//  * Tables.  Two, in the places of the exact parsers' tables and zeroed with them: blocks with an even number publish into hashLong's
//    place and blocks with an odd number into hashSmall's; every lane probes both.  The table of the other parity holds nothing but the
//    blocks before this one, so every candidate from it lies behind the reader.  An entry is (block number + 1) << 17 | (0x1FFFF -
//    position in the block), and lanes publish with an atomic max: a newer block beats an older one, and inside the block being parsed
//    the EARLIEST position of a bucket wins - the one that lies behind most of the lanes that will read it.
//  * Determinism.  The frame may depend on nothing but the chunk's bytes: not on lane timing, not on device against emulator (whose
//    lanes are fibers, not a lockstep wave).  One round is three phases with a rendezvous between them: (1) every searching lane reads
//    its source bytes and its two buckets; (2) every searching lane publishes its position - max is order independent; (3) every lane
//    reads its candidates' bytes (source only), or 32 more bytes of the match it is in, and stores a sequence into its OWN 512 slots of
//    the sequence array.  No lane reads a table word or a sequence slot that another lane writes in the same phase.  Table words are
//    read with agent-scope loads:
//    the atomics execute in L2 and leave the CU's vector L1 as it was.  (Workgroup scope would do for a table only this wave touches, and
//    compiles to sc0 loads and plain atomics - and was measured 2.5 times SLOWER on a lone segment: DESIGN.md 5.)
//  * Sequences.  After the last round the wave compacts the 64 lists in slice order (prefix sum of the counts; the destination never
//    lies behind the source, 64 sequences per step).  The literals behind a slice's last match go in front of the first sequence of the
//    next slice that has one - literal runs are contiguous in the source, so litPos + litLength stay valid - and the last slices' tail
//    becomes lastLL.
//  * Repeat offsets.  The parse searches none.  While compacting, a sequence with literals whose offset equals the previous sequence's
//    gets repeat code 1, every other one offset + 3: only code 1 is used and only with literals, so "repeat offset 1 is the previous
//    sequence's actual offset" holds throughout and needs no serial pass.  The block's first sequence compares with rep[0] as handed
//    in; rep[] goes back as a decoder would hold it after the block.
#define ZS_DP_LANE_SEQ (ZS_MAX_SEQ / LANES)     /* sequence slots of one lane: a 2 KiB slice holds 512 matches of 4 bytes */
#define ZS_DP_MIN_SLICE 64u                     /* small blocks use fewer lanes, not shorter slices */
#define ZS_DP_STEP_LOG 5u                       /* a miss advances by 1 + (misses since the last match >> 5) */
static_assert(ZS_DP_LANE_SEQ * 4u * LANES == ZS_BLOCK_MAX, "a lane's slots hold whatever a slice of a full block can produce");

__device__ static inline uint32_t dp_entry(uint32_t pos) { return (((pos >> 17) + 1u) << 17) | (0x1FFFFu - (pos & 0x1FFFFu)); }
__device__ static inline uint32_t dp_entry_pos(uint32_t e) { return (((e >> 17) - 1u) << 17) + (0x1FFFFu - (e & 0x1FFFFu)); }
#ifdef HIPEMU
#define DP_TABLE_LOAD(p) (*(p))
#define DP_TABLE_MAX(p, v) ((void)atomicMax((p), (v)))
#define DP_LOADED(a, b) do {} while (0)
__device__ static inline void dp_get_seq(const zs_seq* p, uint32_t& offBase, uint32_t& litLength, uint32_t& mlBase, uint32_t& litPos) {
    offBase = p->offBase; litLength = p->litLength; mlBase = p->mlBase; litPos = p->litPos;
}
#else
#define DP_TABLE_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define DP_TABLE_MAX(p, v) ((void)__hip_atomic_fetch_max((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
#define DP_LOADED(a, b) asm volatile("" : "+v"(a), "+v"(b))        /* both buckets have arrived before any lane publishes */
__device__ static inline void dp_get_seq(const ZS_GLOBAL zs_seq* p, uint32_t& offBase, uint32_t& litLength, uint32_t& mlBase, uint32_t& litPos) {
    const zs_u32x4 t = *reinterpret_cast<const ZS_GLOBAL zs_u32x4*>(p);                         // field order of zs_seq, as zs_put_seq
    offBase = t.x; litLength = t.y; mlBase = t.z; litPos = t.w;
}
#endif

__device__ ZS_NOINLINE static void device_block(const uint8_t* __restrict__ src, const uint32_t srcSize_, const uint32_t blockStart_, const uint32_t blockSize_,
                                                uint32_t* __restrict__ hashLong, uint32_t* __restrict__ hashSmall, const zs_cparams cp, uint32_t* rep,
                                                zs_seq* __restrict__ seqs, MfState& ms, const uint32_t lane) {
    const gbytes_t gsrc = (gbytes_t)uni_ptr(src);
    ZS_GLOBAL zs_seq* const gseqs = (ZS_GLOBAL zs_seq*)uni_ptr(seqs);
    const uint32_t srcSize = UNI(srcSize_), blockStart = UNI(blockStart_), blockSize = UNI(blockSize_), iend = blockStart + blockSize;
    const uint32_t maxDist = 1u << UNI(cp.windowLog), mls = UNI(cp.minMatch);
    const bool odd = ((blockStart >> 17) & 1u) != 0;                  // (blocks are cut at fixed 128 KiB: block number = start >> 17)
    const gwords_t gW = (gwords_t)uni_ptr(odd ? hashSmall : hashLong), gR = (gwords_t)uni_ptr(odd ? hashLong : hashSmall);
    const uint32_t hW = odd ? UNI(cp.chainLog) : UNI(cp.hashLog), hR = odd ? UNI(cp.hashLog) : UNI(cp.chainLog);
    const bool probeOld = blockStart != 0;
    const bool tableOK = blockStart < 0xFFFE0000u;                    // (block number + 1 fits the entry's 15 bits)
    uint32_t sliceLen = (blockSize + LANES - 1) / LANES;
    if (sliceLen < ZS_DP_MIN_SLICE) sliceLen = ZS_DP_MIN_SLICE;
    uint32_t sBeg = blockStart + lane * sliceLen;
    if (sBeg > iend) sBeg = iend;
    const uint32_t sEnd = iend - sBeg < sliceLen ? iend : sBeg + sliceLen;
    ZS_GLOBAL zs_seq* const mine = gseqs + lane * ZS_DP_LANE_SEQ;
    uint32_t pos = sBeg, anchor = sBeg, cnt = 0, matched = 0, miss = 0;
    uint32_t cand = 0, len = 0;                                       // a match being extended: pos is its start, cand its source, len its length so far
    bool ext = false;
#define DP_STORE_MATCH() do { zs_put_seq(mine + cnt, pos - cand, pos - anchor, len - 3, anchor); /* (offBase: the offset itself until the lists are compacted) */ \
                              cnt++; matched += len; pos += len; anchor = pos; miss = 0; ext = false; } while (0)

    for (;;) {
        const bool searching = !ext && tableOK && pos + 4 <= sEnd && pos + 8 <= srcSize && cnt < ZS_DP_LANE_SEQ;
        if (!__any(searching || ext)) break;
        VM_DRAIN();                                                   // the last round's publications have reached L2
        // ---- (1) source bytes, hashes, buckets ----
        uint64_t d8 = 0;
        uint32_t hw = 0, eW = 0, eR = 0;
        if (searching) {
            d8 = gld64(gsrc + pos);
            hw = hashF(d8, hW, mls);
            eW = DP_TABLE_LOAD(gW + hw);
            if (probeOld) eR = DP_TABLE_LOAD(gR + hashF(d8, hR, mls));
            DP_LOADED(eW, eR);
        }
        WAVE_MEM_SYNC();
        // ---- (2) publish ----
        if (searching) DP_TABLE_MAX(gW + hw, dp_entry(pos));
        WAVE_MEM_SYNC();
        // ---- (3) one round trip for every lane, whatever it is doing: a searching lane reads 8 bytes at both candidates and the 8 bytes in
        // front of itself and of them; a lane inside a match reads the next 32 bytes of both sides.  A match longer than the first
        // comparison is continued in the following rounds, so that no lane waits for another lane's long match.
        uint32_t a0 = pos, a1 = pos, a2 = pos, a3 = pos, a4 = pos, a5 = pos, a6 = pos, a7 = pos;   // (every address a lane may read: pos + 8 <= srcSize)
        bool okW = false, okR = false;
        uint32_t cW = pos, cR = pos;
        const uint32_t last8 = srcSize - 8;
        if (searching) {
            if (eW) cW = dp_entry_pos(eW);
            if (eR) cR = dp_entry_pos(eR);
            okW = cW < pos && pos - cW <= maxDist; okR = cR < pos && pos - cR <= maxDist;
            if (okW) a0 = cW;
            if (okR) a1 = cR;
            if (pos >= 8) a2 = pos - 8;
            if (okW && cW >= 8) a3 = cW - 8;
            if (okR && cR >= 8) a4 = cR - 8;
        } else if (ext) {
            const uint32_t p = pos + len, q = cand + len;             // (q < p; addresses past the chunk's last 8 bytes are clamped and their data not used)
            a0 = p < last8 ? p : last8; a1 = p + 8 < last8 ? p + 8 : last8; a2 = p + 16 < last8 ? p + 16 : last8; a3 = p + 24 < last8 ? p + 24 : last8;
            a4 = q < last8 ? q : last8; a5 = q + 8 < last8 ? q + 8 : last8; a6 = q + 16 < last8 ? q + 16 : last8; a7 = q + 24 < last8 ? q + 24 : last8;
        }
        uint64_t v0 = 0, v1 = 0, v2 = 0, v3 = 0, v4 = 0, v5 = 0, v6 = 0, v7 = 0;
        if (searching || ext) { v0 = gld64(gsrc + a0); v1 = gld64(gsrc + a1); v2 = gld64(gsrc + a2); v3 = gld64(gsrc + a3); v4 = gld64(gsrc + a4); }
        if (ext) { v5 = gld64(gsrc + a5); v6 = gld64(gsrc + a6); v7 = gld64(gsrc + a7); }
        if (searching) {
            const uint32_t lim = sEnd - pos;                          // the match ends with the slice
            const uint64_t xW = v0 ^ d8, xR = v1 ^ d8;
            uint32_t nW = okW ? (xW ? (uint32_t)(__ffsll((long long)xW) - 1) >> 3 : 8u) : 0u, nR = okR ? (xR ? (uint32_t)(__ffsll((long long)xR) - 1) >> 3 : 8u) : 0u;
            if (nW > lim) nW = lim;
            if (nR > lim) nR = lim;
            const bool useW = nW >= 4 && nW >= nR;                    // the longer one; the nearer table on a tie
            if (useW || nR >= 4) {
                cand = useW ? cW : cR; len = useW ? nW : nR;
                // backward: the bytes in front of both, as far as they are this lane's literals (at most 8)
                uint32_t nb = 0;
                if (pos >= 8 && cand >= 8) {
                    const uint64_t xb = v2 ^ (useW ? v3 : v4);
                    nb = xb ? (uint32_t)__clzll((long long)xb) >> 3 : 8u;
                    if (nb > pos - anchor) nb = pos - anchor;
                }
                const bool more = len == 8 && lim > 8;
                pos -= nb; cand -= nb; len += nb;
                if (more) ext = true; else DP_STORE_MATCH();
            } else {
                pos += 1 + (miss >> ZS_DP_STEP_LOG); miss++;
            }
        } else if (ext) {
            bool open = true;
#define DP_EXT_STEP(va_, vb_) do { if (open) { const uint32_t at = pos + len, rem = sEnd - at;                                             \
                if (rem == 0) open = false;                                                                                              \
                else if (at <= last8) { const uint64_t x = (va_) ^ (vb_); uint32_t n = x ? (uint32_t)(__ffsll((long long)x) - 1) >> 3 : 8u; \
                                        if (n > rem) n = rem; len += n; if (n < 8) open = false; }                                       \
                else { while (pos + len < sEnd && gsrc[pos + len] == gsrc[cand + len]) len++; open = false; } } } while (0)
            DP_EXT_STEP(v0, v4); DP_EXT_STEP(v1, v5); DP_EXT_STEP(v2, v6); DP_EXT_STEP(v3, v7);
#undef DP_EXT_STEP
            if (!open) DP_STORE_MATCH();
        }
    }
#undef DP_STORE_MATCH
    stage_sync();                                                     // every lane's list is visible to every lane

    // ---- the 64 lists become one ----
    const uint32_t tail = sEnd - anchor;                              // literals behind the slice's last match (an empty slice: all of it)
    const unsigned long long ne = __ballot(cnt != 0);
    const uint32_t T = wave_excl_scan(tail, lane), base = wave_excl_scan(cnt, lane);
    const uint32_t nbSeq = wave_sum(cnt), totalTail = wave_sum(tail), totalMatched = wave_sum(matched);
    const unsigned long long below = ne & ((1ull << lane) - 1);
    const uint32_t prev = below ? 63u - (uint32_t)__clzll((long long)below) : 0u;
    const uint32_t Tprev = __shfl(T, (int)prev);
    const uint32_t extra = below ? T - Tprev : T;                     // literals in front of this slice that no sequence has taken
    uint32_t r0 = UNI(rep[0]), r1 = UNI(rep[1]), r2 = UNI(rep[2]);
    uint32_t carry = r0;                                              // the previous sequence's offset
#define DP_PUSH(l_) do { r2 = r1; r1 = r0; r0 = (uint32_t)__builtin_amdgcn_readlane((int)raw, (int)(l_)); } while (0)
    for (unsigned long long todo = ne; todo; todo &= todo - 1) {
        const uint32_t j = (uint32_t)__ffsll((long long)todo) - 1;
        const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane((int)cnt, (int)j), dj = (uint32_t)__builtin_amdgcn_readlane((int)base, (int)j);
        const uint32_t xj = (uint32_t)__builtin_amdgcn_readlane((int)extra, (int)j);
        for (uint32_t k = 0; k < cj; k += LANES) {
            const uint32_t i = k + lane;
            const bool v = i < cj;
            uint32_t raw = 0, ll = 0, mlBase = 0, lp = 0;
            if (v) dp_get_seq(gseqs + j * ZS_DP_LANE_SEQ + i, raw, ll, mlBase, lp);
            WAVE_MEM_SYNC();                                          // (emulator) read by all lanes before the destination, which may overlap, is written
            uint32_t before = __shfl_up(raw, 1);
            if (lane == 0) before = carry;
            if (v && i == 0) { ll += xj; lp -= xj; }
            const uint32_t offBase = (ll > 0 && raw == before) ? 1u : raw + 3;
            if (v) zs_put_seq(gseqs + dj + i, offBase, ll, mlBase, lp);
            const uint32_t nv = cj - k < LANES ? cj - k : LANES;
            carry = (uint32_t)__builtin_amdgcn_readlane((int)raw, (int)(nv - 1));
            // the history a decoder holds: every sequence that carries an offset pushes it; at most the last three of this step count
            unsigned long long m = __ballot(v && offBase != 1u);
            if (m) {
                const uint32_t h1 = 63u - (uint32_t)__clzll((long long)m); m &= ~(1ull << h1);
                if (m) {
                    const uint32_t h2 = 63u - (uint32_t)__clzll((long long)m); m &= ~(1ull << h2);
                    if (m) DP_PUSH(63u - (uint32_t)__clzll((long long)m));
                    DP_PUSH(h2);
                }
                DP_PUSH(h1);
            }
        }
    }
#undef DP_PUSH
    rep[0] = r0; rep[1] = r1; rep[2] = r2;
    uint32_t lastLL = blockSize;
    if (ne) lastLL = totalTail - (uint32_t)__builtin_amdgcn_readlane((int)T, (int)(63u - (uint32_t)__clzll((long long)ne)));
    ms.nbSeq = UNI(nbSeq); ms.lastLL = UNI(lastLL); ms.anchor = iend - UNI(lastLL);
    ms.litSize = blockSize - UNI(totalMatched);
}
