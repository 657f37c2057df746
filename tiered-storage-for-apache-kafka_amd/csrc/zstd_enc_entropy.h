// Zstandard compressor, entropy stage of a block (included by zstd_enc.hip after zstd_enc_dev.h and zstd_enc_huf.h): the lane-0 bit
// writer and FSE coder, huf_writeCTable, wave_histogram, the wave bit packer, the literals section (compress_literals), the sequences
// section (compress_sequences), and the gathering of a parsed block's literals (gather_literals, copy_run).
// From EncLds: hufRepeat and scal (ZS_SCAL_*), and every member of the entropy struct.  While the literal stage runs, huf[] is live and
// ll is not, `of` and everything behind hist is work space; while the sequence stage runs, ll / of / ml are live and huf[] waits in the
// workspace.  The parse stage's p (and g, crcTab) must be dead: gather_literals is the first thing to run after a parse.
// ---- lane-0 serial pieces (FSE / Huffman table construction), work arrays in LDS ---------------------------
struct BitW { uint8_t* start; uint8_t* p; uint8_t* end; uint64_t acc; uint32_t n; bool overflow; };
__device__ static inline void bw_init(BitW& b, uint8_t* dst, uint8_t* end) { b.start = b.p = dst; b.end = end; b.acc = 0; b.n = 0; b.overflow = false; }
__device__ static inline void bw_add(BitW& b, uint64_t v, uint32_t nb) {
    if (!nb) return;
    b.acc |= (v & ((1ull << nb) - 1)) << b.n;
    b.n += nb;
    while (b.n >= 8) { if (b.p < b.end) *b.p++ = (uint8_t)b.acc; else b.overflow = true; b.acc >>= 8; b.n -= 8; }
}
__device__ static inline uint32_t bw_close(BitW& b) {
    bw_add(b, 1, 1);
    if (b.n) { if (b.p < b.end) *b.p++ = (uint8_t)b.acc; else b.overflow = true; b.n = 0; }
    return (uint32_t)(b.p - b.start);
}

__device__ static uint32_t fse_minTableLog(uint32_t srcSize, uint32_t maxSym) {
    uint32_t a = hb32(srcSize) + 1, b = hb32(maxSym) + 2;
    return a < b ? a : b;
}
__device__ static uint32_t fse_optimalTableLog(uint32_t maxTableLog, uint32_t srcSize, uint32_t maxSym, uint32_t minus) {
    uint32_t maxBitsSrc = hb32(srcSize - 1) - minus, tableLog = maxTableLog, minBits = fse_minTableLog(srcSize, maxSym);
    if (maxBitsSrc < tableLog) tableLog = maxBitsSrc;
    if (minBits > tableLog) tableLog = minBits;
    if (tableLog < 5) tableLog = 5;
    if (tableLog > 12) tableLog = 12;
    return tableLog;
}

__device__ ZS_NOINLINE static int fse_normalizeM2(short* norm, uint32_t tableLog, const uint32_t* cnt, uint32_t total, uint32_t maxSym, short lowProbCount) {
    const short NOT_YET = -2;
    uint32_t s, distributed = 0, toDist;
    const uint32_t lowThreshold = total >> tableLog;
    uint32_t lowOne = (uint32_t)(((uint64_t)total * 3) >> (tableLog + 1));
    for (s = 0; s <= maxSym; s++) {
        if (cnt[s] == 0) { norm[s] = 0; continue; }
        if (cnt[s] <= lowThreshold) { norm[s] = lowProbCount; distributed++; total -= cnt[s]; continue; }
        if (cnt[s] <= lowOne) { norm[s] = 1; distributed++; total -= cnt[s]; continue; }
        norm[s] = NOT_YET;
    }
    toDist = (1u << tableLog) - distributed;
    if (toDist == 0) return 0;
    if ((total / toDist) > lowOne) {
        lowOne = (uint32_t)(((uint64_t)total * 3) / (toDist * 2));
        for (s = 0; s <= maxSym; s++)
            if (norm[s] == NOT_YET && cnt[s] <= lowOne) { norm[s] = 1; distributed++; total -= cnt[s]; }
        toDist = (1u << tableLog) - distributed;
    }
    if (distributed == maxSym + 1) {
        uint32_t maxV = 0, maxC = 0;
        for (s = 0; s <= maxSym; s++) if (cnt[s] > maxC) { maxV = s; maxC = cnt[s]; }
        norm[maxV] += (short)toDist;
        return 0;
    }
    if (total == 0) {
        for (s = 0; toDist > 0; s = (s + 1) % (maxSym + 1)) if (norm[s] > 0) { toDist--; norm[s]++; }
        return 0;
    }
    {   const uint64_t vStepLog = 62 - tableLog, mid = (1ULL << (vStepLog - 1)) - 1;
        const uint64_t rStep = ((((uint64_t)1 << vStepLog) * toDist) + mid) / total;
        uint64_t tmpTotal = mid;
        for (s = 0; s <= maxSym; s++) {
            if (norm[s] == NOT_YET) {
                const uint64_t end = tmpTotal + (cnt[s] * rStep);
                const uint32_t weight = (uint32_t)(end >> vStepLog) - (uint32_t)(tmpTotal >> vStepLog);
                if (weight < 1) return -1;
                norm[s] = (short)weight;
                tmpTotal = end;
            }
        }
    }
    return 0;
}

__device__ ZS_NOINLINE static int fse_normalizeCount(short* norm, uint32_t tableLog, const uint32_t* cnt, uint32_t total, uint32_t maxSym, bool useLowProb) {
    const short lowProbCount = useLowProb ? -1 : 1;
    const uint64_t scale = 62 - tableLog, step = ((uint64_t)1 << 62) / total, vStep = 1ULL << (scale - 20);
    int still = 1 << tableLog;
    uint32_t s, largest = 0; short largestP = 0;
    const uint32_t lowThreshold = total >> tableLog;
    if (tableLog < fse_minTableLog(total, maxSym)) return -1;
    for (s = 0; s <= maxSym; s++) {
        if (cnt[s] == total) return 0;
        if (cnt[s] == 0) { norm[s] = 0; continue; }
        if (cnt[s] <= lowThreshold) { norm[s] = lowProbCount; still--; }
        else {
            short proba = (short)((cnt[s] * step) >> scale);
            if (proba < 8) { const uint64_t restToBeat = vStep * kRtb[proba]; proba += (cnt[s] * step) - ((uint64_t)proba << scale) > restToBeat; }
            if (proba > largestP) { largestP = proba; largest = s; }
            norm[s] = proba; still -= proba;
        }
    }
    if (-still >= (norm[largest] >> 1)) { if (fse_normalizeM2(norm, tableLog, cnt, total, maxSym, lowProbCount) < 0) return -1; }
    else norm[largest] += (short)still;
    return (int)tableLog;
}

__device__ ZS_NOINLINE static uint32_t fse_writeNCount(uint8_t* out0, const short* norm, uint32_t maxSym, uint32_t tableLog) {
    uint8_t* out = out0;
    int nbBits, remaining, threshold; const int tableSize = 1 << tableLog;
    uint32_t bitStream = 0; int bitCount = 0; uint32_t symbol = 0; const uint32_t alphabetSize = maxSym + 1; int previousIs0 = 0;
    bitStream += (tableLog - 5) << bitCount; bitCount += 4;
    remaining = tableSize + 1; threshold = tableSize; nbBits = (int)tableLog + 1;
    while (symbol < alphabetSize && remaining > 1) {
        if (previousIs0) {
            uint32_t start = symbol;
            while (symbol < alphabetSize && !norm[symbol]) symbol++;
            if (symbol == alphabetSize) break;
            while (symbol >= start + 24) { start += 24; bitStream += 0xFFFFU << bitCount; out[0] = (uint8_t)bitStream; out[1] = (uint8_t)(bitStream >> 8); out += 2; bitStream >>= 16; }
            while (symbol >= start + 3) { start += 3; bitStream += 3U << bitCount; bitCount += 2; }
            bitStream += (symbol - start) << bitCount; bitCount += 2;
            if (bitCount > 16) { out[0] = (uint8_t)bitStream; out[1] = (uint8_t)(bitStream >> 8); out += 2; bitStream >>= 16; bitCount -= 16; }
        }
        {   int c = norm[symbol++];
            const int mx = (2 * threshold - 1) - remaining;
            remaining -= c < 0 ? -c : c;
            c++;
            if (c >= threshold) c += mx;
            bitStream += (uint32_t)c << bitCount;
            bitCount += nbBits;
            bitCount -= (c < mx);
            previousIs0 = (c == 1);
            if (remaining < 1) return 0;
            while (remaining < threshold) { nbBits--; threshold >>= 1; }
        }
        if (bitCount > 16) { out[0] = (uint8_t)bitStream; out[1] = (uint8_t)(bitStream >> 8); out += 2; bitStream >>= 16; bitCount -= 16; }
    }
    if (remaining != 1) return 0;
    out[0] = (uint8_t)bitStream; out[1] = (uint8_t)(bitStream >> 8);
    out += (bitCount + 7) / 8;
    return (uint32_t)(out - out0);
}

__device__ ZS_NOINLINE static void fse_buildCTable(FseTable& ct, const short* norm, uint32_t maxSym, uint32_t tableLog, uint16_t* cumul, uint8_t* tableSymbol) {
    const uint32_t tableSize = 1u << tableLog, tableMask = tableSize - 1, step = (tableSize >> 1) + (tableSize >> 3) + 3;
    uint32_t highThreshold = tableSize - 1, u;
    ct.tableLog = tableLog;
    cumul[0] = 0;
    for (u = 1; u <= maxSym + 1; u++) {
        if (norm[u - 1] == -1) { cumul[u] = (uint16_t)(cumul[u - 1] + 1); tableSymbol[highThreshold--] = (uint8_t)(u - 1); }
        else cumul[u] = (uint16_t)(cumul[u - 1] + (uint32_t)norm[u - 1]);
    }
    cumul[maxSym + 1] = (uint16_t)(tableSize + 1);
    {   uint32_t position = 0;
        for (uint32_t symbol = 0; symbol <= maxSym; symbol++) {
            const int freq = norm[symbol];
            for (int n = 0; n < freq; n++) {
                tableSymbol[position] = (uint8_t)symbol;
                position = (position + step) & tableMask;
                while (position > highThreshold) position = (position + step) & tableMask;
            }
        }
    }
    for (u = 0; u < tableSize; u++) { const uint8_t s = tableSymbol[u]; ct.state[cumul[s]++] = (uint16_t)(tableSize + u); }
    {   uint32_t total = 0;
        for (uint32_t s = 0; s <= maxSym; s++) {
            const int nv = norm[s];
            if (nv == 0) { ct.dnb[s] = ((tableLog + 1) << 16) - (1u << tableLog); ct.dfs[s] = 0; }
            else if (nv == -1 || nv == 1) { ct.dnb[s] = (tableLog << 16) - (1u << tableLog); ct.dfs[s] = (int)(total - 1); total++; }
            else {
                const uint32_t maxBitsOut = tableLog - hb32((uint32_t)nv - 1), minStatePlus = (uint32_t)nv << maxBitsOut;
                ct.dnb[s] = (maxBitsOut << 16) - minStatePlus; ct.dfs[s] = (int)(total - (uint32_t)nv); total += (uint32_t)nv;
            }
        }
    }
}
__device__ static inline uint32_t fse_init2(const FseTable& ct, uint32_t symbol) {
    const uint32_t dnb = ct.dnb[symbol];
    const uint32_t nbBitsOut = (dnb + (1u << 15)) >> 16;
    const uint32_t value = (nbBitsOut << 16) - dnb;
    return ct.state[(value >> nbBitsOut) + ct.dfs[symbol]];
}
__device__ static inline void fse_encode(BitW& b, const FseTable& ct, uint32_t& value, uint32_t symbol) {
    const uint32_t nbBitsOut = (value + ct.dnb[symbol]) >> 16;
    bw_add(b, value, nbBitsOut);
    value = ct.state[(value >> nbBitsOut) + ct.dfs[symbol]];
}

// HUF_compressWeights + HUF_writeCTable; returns header size, 0xFFFFFFFF when the table cannot be described
__device__ ZS_NOINLINE static uint32_t huf_writeCTable(uint8_t* dst, const HufTable& ct, uint32_t maxSym, uint32_t huffLog, EncLds& L) {
    uint8_t* const hw = reinterpret_cast<uint8_t*>(L.hist2);            // 256 weights + one pad byte ...
    for (uint32_t n = 0; n < maxSym; n++) { const uint32_t nb = ct.nb[n]; hw[n] = nb ? (uint8_t)(huffLog + 1 - nb) : 0; }
    uint32_t hSize = 0;
    {   // HUF_compressWeights(dst + 1, hw, maxSym)
        uint8_t* op = dst + 1; const uint32_t wtSize = maxSym;
        uint32_t maxSV = ZS_HUF_TABLELOG_MAX; uint32_t* cnt = L.hist2 + 68;    // ... and behind them the 13 counters of the weights' histogram
        if (wtSize > 1) {
            for (int i = 0; i <= ZS_HUF_TABLELOG_MAX; i++) cnt[i] = 0;
            for (uint32_t i = 0; i < wtSize; i++) cnt[hw[i]]++;
            while (!cnt[maxSV]) maxSV--;
            uint32_t maxCount = 0;
            for (uint32_t i = 0; i <= maxSV; i++) if (cnt[i] > maxCount) maxCount = cnt[i];
            if (maxCount == wtSize) hSize = 1;
            else if (maxCount == 1) hSize = 0;
            else {
                const uint32_t tableLog = fse_optimalTableLog(6, wtSize, maxSV, 2);
                if (fse_normalizeCount(L.norm, tableLog, cnt, wtSize, maxSV, false) < 0) return 0xFFFFFFFFu;
                op += fse_writeNCount(op, L.norm, maxSV, tableLog);
                fse_buildCTable(L.of, L.norm, maxSV, tableLog, L.cumul, L.tableSymbol);     // L.of is free until the sequence stage
                // FSE_compress_usingCTable: two interleaved states, from the last weight to the first
                if (wtSize <= 2) hSize = 0;
                else {
                    BitW b; bw_init(b, op, op + 512);
                    const uint8_t* ip = hw + wtSize; uint32_t s1, s2;
                    if (wtSize & 1) { s1 = fse_init2(L.of, *--ip); s2 = fse_init2(L.of, *--ip); fse_encode(b, L.of, s1, *--ip); }
                    else { s2 = fse_init2(L.of, *--ip); s1 = fse_init2(L.of, *--ip); }
                    while (ip > hw) { fse_encode(b, L.of, s2, *--ip); if (ip > hw) fse_encode(b, L.of, s1, *--ip); }
                    bw_add(b, s2, tableLog); bw_add(b, s1, tableLog);
                    op += bw_close(b);
                    hSize = (uint32_t)(op - (dst + 1));
                }
            }
        }
    }
    if ((hSize > 1) & (hSize < maxSym / 2)) { dst[0] = (uint8_t)hSize; return hSize + 1; }
    if (maxSym > 128) return 0xFFFFFFFFu;
    dst[0] = (uint8_t)(128 + (maxSym - 1));
    hw[maxSym] = 0;
    for (uint32_t n = 0; n < maxSym; n += 2) dst[(n / 2) + 1] = (uint8_t)((hw[n] << 4) + hw[n + 1]);
    return ((maxSym + 1) / 2) + 1;
}

__device__ ZS_NOINLINE static void wave_histogram(uint32_t* hist, const uint8_t* __restrict__ p, uint32_t n, uint32_t lane) {
    for (uint32_t i = lane; i < 256; i += LANES) hist[i] = 0;
    __syncthreads();
    for (uint32_t i = lane; i < n; i += LANES) atomicAdd(&hist[p[i]], 1u);
    __syncthreads();
}

// ---- the wave bit packer -------------------------------------------------------------------------------------
// Both bit streams of a block (a Huffman stream, the FSE sequence stream) are written from the LAST item to the first, LSB-first, and
// closed by a 1 bit.  Every lane takes a contiguous run of the n items in emission order (reversed index r: item n - 1 - r), counts the
// bits of its run, a prefix sum gives it its first bit, and the lanes OR their 32-bit words into zeroed 4-byte aligned scratch; the last
// lane appends what the caller has for the stream's end and the end mark.  The callers keep what differs: which bits an item contributes.
struct WavePack { uint32_t r0, r1, startBit; uint32_t* tmp; uint64_t acc; uint32_t word, nacc; };
__device__ __forceinline__ static void wp_range(WavePack& p, uint32_t n, uint32_t lane) {
    const uint32_t per = (n + LANES - 1) / LANES;
    p.r0 = lane * per < n ? lane * per : n; p.r1 = p.r0 + per < n ? p.r0 + per : n;
}
// bits = this lane's bits: the items of its run and, in the last lane, whatever the caller puts behind the last item (the sequence stream's
// final states) - but NOT the end mark, which is counted here and written by wp_finish.  Returns the stream's length in bits.
__device__ __forceinline__ static uint32_t wp_scan(WavePack& p, uint32_t bits, uint32_t lane) {
    if (lane == LANES - 1) bits++;                                   // end mark
    p.startBit = wave_excl_scan(bits, lane);
    return __shfl(p.startBit + bits, LANES - 1);
}
__device__ __forceinline__ static void wp_begin(WavePack& p, uint32_t* __restrict__ tmp, uint32_t totalBits, uint32_t lane) {
    const uint32_t words = (totalBits + 31) / 32;
    for (uint32_t w = lane; w < words; w += LANES) tmp[w] = 0;
    stage_sync();
    p.tmp = tmp; p.acc = 0; p.word = p.startBit >> 5; p.nacc = p.startBit & 31;
}
__device__ __forceinline__ static void wp_put(WavePack& p, uint64_t v, uint32_t nb) {          // nb <= 32, v < 2^nb
    p.acc |= v << p.nacc;
    p.nacc += nb;
    if (p.nacc >= 32) { atomicOr(&p.tmp[p.word], (uint32_t)p.acc); p.acc >>= 32; p.nacc -= 32; p.word++; }
}
__device__ __forceinline__ static void wp_finish(WavePack& p, uint32_t lane) {
    if (lane == LANES - 1) wp_put(p, 1, 1);                          // end mark
    if (p.nacc) atomicOr(&p.tmp[p.word], (uint32_t)p.acc);
    stage_sync();
}

// One Huffman stream (HUF_compress1X_usingCTable) into tmp; returns the stream size in bytes.
__device__ ZS_NOINLINE static uint32_t wave_huf_encode(uint32_t* __restrict__ tmp, const uint8_t* __restrict__ src, uint32_t n, const HufTable& ct, uint32_t lane) {
    WavePack p;
    wp_range(p, n, lane);
    uint32_t bits = 0;
    for (uint32_t r = p.r0; r < p.r1; r++) bits += ct.nb[src[n - 1 - r]];
    const uint32_t total = wp_scan(p, bits, lane);
    wp_begin(p, tmp, total, lane);
    for (uint32_t r = p.r0; r < p.r1; r++) {
        const uint8_t s = src[n - 1 - r];
        wp_put(p, ct.val[s], ct.nb[s]);
    }
    wp_finish(p, lane);
    return (total + 7) / 8;
}

// HUF_compress1X / 4X_usingCTable + the compressibility check of HUF_compressCTable_internal.
// Writes at op (inside blockout); returns the total size from ostart, 0 if not compressible.
__device__ ZS_NOINLINE static uint32_t wave_huf_compress(uint8_t* ostart, uint8_t* op, const uint8_t* __restrict__ lit, uint32_t n, bool single, const HufTable& ct,
                                             uint32_t* tmp, uint32_t lane) {
    if (single) {
        const uint32_t c = wave_huf_encode(tmp, lit, n, ct, lane);
        wave_copy(op, (const uint8_t*)tmp, c, lane);
        op += c;
    } else {
        if (n < 12) return 0;
        const uint32_t seg = (n + 3) / 4;
        uint8_t* const jump = op;
        op += 6;
        for (int i = 0; i < 4; i++) {
            const uint32_t len = i < 3 ? seg : n - 3 * seg;
            const uint32_t c = wave_huf_encode(tmp, lit + (uint32_t)i * seg, len, ct, lane);
            if (c == 0 || c > 65535) return 0;
            if (i < 3 && lane == 0) put_le(jump + 2 * i, c, 2);
            wave_copy(op, (const uint8_t*)tmp, c, lane);
            op += c;
            __syncthreads();
        }
    }
    const uint32_t tot = (uint32_t)(op - ostart);
    if (tot >= n - 1) return 0;
    return tot;
}

// ---------------------------------------------------------------------------------------------------
// literals section (ZSTD_compressLiterals).  Returns its size; updates L.huf / L.hufRepeat ("next" side).
// cur = index of the confirmed (previous) Huffman state; the candidate state is written at cur ^ 1.
// ---------------------------------------------------------------------------------------------------
// Raw_Literals_Block (type 0: the n bytes follow) or RLE_Literals_Block (type 1: one byte follows); the header is 1, 2 or 3 bytes
__device__ static uint32_t write_plain_literals(uint8_t* dst, const uint8_t* lit, uint32_t n, uint32_t type, uint32_t lane) {
    const uint32_t fl = 1 + (n > 31) + (n > 4095);
    WAVE_MEM_SYNC();                // the fallback overwrites what a Huffman attempt left at dst: other lanes' earlier stores come first
    if (lane == 0) {
        put_le(dst, fl == 1 ? type + (n << 3) : type + ((fl == 2 ? 1u : 3u) << 2) + (n << 4), fl);
        if (type == 1) dst[fl] = lit[0];
    }
    if (type == 1) return fl + 1;
    wave_copy(dst + fl, lit, n, lane);
    return fl + n;
}
// "histogram, then the largest count": returns the largest count, *top (if asked for) receives the highest byte value that occurs
__device__ __forceinline__ static uint32_t wave_hist_max(uint32_t* hist, const uint8_t* __restrict__ p, uint32_t n, uint32_t lane, uint32_t* top = nullptr) {
    wave_histogram(hist, p, n, lane);
    uint32_t m = 0, t = 0;
    for (uint32_t i = lane; i < 256; i += LANES) { const uint32_t c = hist[i]; if (c > m) m = c; if (c) t = i; }
    if (top) *top = wave_max(t);
    return wave_max(m);
}

__device__ ZS_NOINLINE static uint32_t compress_literals(uint8_t* dst, const uint8_t* __restrict__ lit, uint32_t n, EncLds& L, int cur, bool suspectUncompressible,
                                             uint32_t* tmp, uint32_t lane) {
    const int nxt = cur ^ 1;
    const uint32_t lhSize = 3 + (n >= 1024) + (n >= 16384);
    bool single = n < 256;
    // "next" starts as a copy of "prev" (nothing to copy: we only switch `cur` when a new table is adopted)
    if (n < 64) return write_plain_literals(dst, lit, n, 0, lane);              // ZSTD_minLiteralsToCompress (dfast, no valid repeat)
    const int prevRepeat = L.hufRepeat[cur];
    const bool preferRepeat = n <= 1024;                                   // strategy < lazy && srcSize <= 1024
    uint8_t* const ostart = dst + lhSize;
    // ---- HUF_compress_internal ----
    uint32_t cLit = 0; bool usedOld = false, newTable = false, decided = false;
    if (suspectUncompressible && n >= 40960) {                             // sample the first and last 4 KiB
        uint32_t largestTotal = wave_hist_max(L.hist2, lit, 4096, lane);
        __syncthreads();
        largestTotal += wave_hist_max(L.hist2, lit + n - 4096, 4096, lane);
        if (largestTotal <= ((2 * 4096) >> 7) + 4) { cLit = 0; decided = true; }
    }
    uint32_t maxSym = 255, largest = 0;
    if (!decided) {
        PT(5);
        largest = wave_hist_max(L.hist, lit, n, lane, &maxSym);
        if (largest == n) { cLit = 1; decided = true; if (lane == 0) ostart[0] = lit[0]; }
        else if (largest <= (n >> 7) + 4) { cLit = 0; decided = true; }
    }
    if (!decided) {
        int repeat = prevRepeat;
        if (repeat == 1) {                                                 // HUF_validateCTable
            bool bad = L.huf[cur].maxSym < maxSym;
            for (uint32_t i = lane; i <= maxSym; i += LANES) bad |= (L.hist[i] != 0) & (L.huf[cur].nb[i] == 0);
            if (__any(bad)) repeat = 0;
        }
        if (preferRepeat && repeat != 0) {
            cLit = wave_huf_compress(ostart, ostart, lit, n, single, L.huf[cur], tmp, lane);
            usedOld = true;
        } else {
            // build the candidate table (lane 0), describe it, compare with reusing the old one
            PT(5);
            // the work arrays in what is dead right now (huf_buildCTable): `of` (free until the weights are FSE-coded, below), and everything
            // behind the counts in `hist` up to the end of `norm` (tail of `ml`, `hist2`, `tableSymbol`, `cumul`, `norm`)
            static_assert(sizeof(L.of) >= HUF_WORK_A_BYTES, "the first group of work arrays fits the OF table");
            static_assert(offsetof(EncLds, norm) + sizeof(((EncLds*)0)->norm) - (offsetof(EncLds, hist) + sizeof(((EncLds*)0)->hist)) >= HUF_WORK_B_BYTES && (offsetof(EncLds, hist) & 3) == 0,
                          "lcount[-1 .. 255] + par[512] fit behind the byte histogram");
            uint32_t huffLog = fse_optimalTableLog(ZS_LitHufLog, n, maxSym, 1);
            huffLog = UNI(huf_buildCTable(L.huf[nxt], L.hist, maxSym, huffLog, reinterpret_cast<uint8_t*>(&L.of), reinterpret_cast<uint8_t*>(L.hist) + sizeof(L.hist), &L.scal[ZS_SCAL_HUF_BC], lane));
            uint32_t oldBits = 0, newBits = 0;                             // (what reusing the old table / using the new one would cost: all lanes)
            if (repeat != 0) {
                for (uint32_t s_ = lane; s_ <= maxSym; s_ += LANES) { oldBits += L.huf[cur].nb[s_] * L.hist[s_]; newBits += L.huf[nxt].nb[s_] * L.hist[s_]; }
                oldBits = wave_sum(oldBits); newBits = wave_sum(newBits);
            }
            if (lane == 0) {
                const uint32_t hSize = huf_writeCTable(ostart, L.huf[nxt], maxSym, huffLog, L);
                uint32_t useOld = 0, fail = 0;
                if (hSize == 0xFFFFFFFFu) fail = 1;
                else {
                    if (repeat != 0) {
                        if ((oldBits >> 3) <= hSize + (newBits >> 3) || hSize + 12 >= n) useOld = 1;
                    }
                    if (!useOld && hSize + 12 >= n) fail = 1;
                }
                L.scal[ZS_SCAL_HUF_HSIZE] = hSize; L.scal[ZS_SCAL_HUF_USEOLD] = useOld; L.scal[ZS_SCAL_HUF_FAIL] = fail;
            }
            __syncthreads();
            const uint32_t hSize = L.scal[ZS_SCAL_HUF_HSIZE]; const bool useOld = L.scal[ZS_SCAL_HUF_USEOLD], fail = L.scal[ZS_SCAL_HUF_FAIL];
            __syncthreads();
            PT(6);
            if (fail) cLit = 0;
            else if (useOld) { cLit = wave_huf_compress(ostart, ostart, lit, n, single, L.huf[cur], tmp, lane); usedOld = true; }
            else { cLit = wave_huf_compress(ostart, ostart + hSize, lit, n, single, L.huf[nxt], tmp, lane); newTable = true; }
        }
    }
    // ---- back in ZSTD_compressLiterals ----
    PT(7);
    const uint32_t minGain = (n >> 6) + 2;
    if (cLit == 0 || cLit >= n - minGain) return write_plain_literals(dst, lit, n, 0, lane);
    if (cLit == 1) return write_plain_literals(dst, lit, n, 1, lane);          // n >= 64 here, so (srcSize >= 8) holds
    const uint32_t hType = (usedOld && !newTable) ? 3u : 2u;                // set_repeat : set_compressed
    if (newTable) L.scal[ZS_SCAL_NEWHUF] = 1;                                           // caller adopts huf[nxt] if the block is kept
    if (lane == 0) {                                                       // 3 / 4 / 5 bytes: type, size format, then 10 / 14 / 18 bits for each of the two sizes
        const uint32_t fmt = lhSize == 3 ? (uint32_t)!single : lhSize - 2, sizeBits = 10 + 4 * (lhSize - 3);
        put_le(dst, hType + (fmt << 2) + ((uint64_t)n << 4) + ((uint64_t)cLit << (4 + sizeBits)), lhSize);
    }
    return lhSize + cLit;
}

// ---------------------------------------------------------------------------------------------------
// sequences section (ZSTD_buildSequencesStatistics + ZSTD_encodeSequences).  Returns bytes written at op,
// 0xFFFFFFFF if the block must be emitted raw.
// ---------------------------------------------------------------------------------------------------
__device__ static int select_encoding(uint32_t mostFrequent, uint32_t nbSeq, uint32_t defaultNormLog, bool defaultAllowed, uint32_t mult) {
    if (mostFrequent == nbSeq) return (defaultAllowed && nbSeq <= 2) ? 0 : 1;           // set_basic : set_rle
    if (defaultAllowed) {
        const uint32_t dynMin = ((1u << defaultNormLog) * mult) >> 3;                    // mult = 10 - strategy (9 fast, 8 dfast)
        if (nbSeq < dynMin || mostFrequent < (nbSeq >> (defaultNormLog - 1))) return 0;   // set_basic
    }
    return 2;                                                                            // set_compressed
}

// lane 0: one of LL / OF / ML.  Returns description size (0xFFFFFFFF on failure); *type receives the mode.
__device__ ZS_NOINLINE static uint32_t build_seq_table(uint8_t* op, FseTable& ct, uint32_t FSELog, uint32_t* cnt, uint32_t maxSymStart, const uint8_t* codes, uint32_t nbSeq,
                                           const short* defaultNorm, uint32_t defaultNormLog, uint32_t defaultMax, bool isOffsets, EncLds& L, uint32_t* type) {
    uint32_t max = maxSymStart;
    while (!cnt[max]) max--;
    uint32_t mostFrequent = 0;
    for (uint32_t s = 0; s <= max; s++) if (cnt[s] > mostFrequent) mostFrequent = cnt[s];
    const bool defaultAllowed = isOffsets ? (max <= ZS_DefaultMaxOff) : true;
    const int t = select_encoding(mostFrequent, nbSeq, defaultNormLog, defaultAllowed, L.scal[ZS_SCAL_MULT]);
    *type = (uint32_t)t;
    if (t == 1) {                                                          // rle
        ct.tableLog = 0; ct.state[0] = 0; ct.state[1] = 0; ct.dnb[max] = 0; ct.dfs[max] = 0;
        *op = codes[0];
        return 1;
    }
    if (t == 0) {
        for (uint32_t s = 0; s <= defaultMax; s++) L.norm[s] = defaultNorm[s];
        fse_buildCTable(ct, L.norm, defaultMax, defaultNormLog, L.cumul, L.tableSymbol);
        return 0;
    }
    uint32_t nbSeq_1 = nbSeq;
    const uint32_t tableLog = fse_optimalTableLog(FSELog, nbSeq, max, 2);
    if (cnt[codes[nbSeq - 1]] > 1) { cnt[codes[nbSeq - 1]]--; nbSeq_1--; }
    if (fse_normalizeCount(L.norm, tableLog, cnt, nbSeq_1, max, nbSeq_1 >= 2048) < 0) return 0xFFFFFFFFu;
    const uint32_t sz = fse_writeNCount(op, L.norm, max, tableLog);
    fse_buildCTable(ct, L.norm, max, tableLog, L.cumul, L.tableSymbol);
    return sz;
}

__device__ ZS_NOINLINE static uint32_t compress_sequences(uint8_t* op0, uint8_t* oend, const zs_seq* __restrict__ seqs, uint32_t nbSeq, uint8_t* __restrict__ codes,
                                              EncLds& L, uint32_t* tmp, uint32_t tmpCap, uint32_t lane) {
    uint8_t* op = op0;
    uint8_t* const llC = codes; uint8_t* const ofC = codes + ZS_WS_CODE_STRIDE; uint8_t* const mlC = codes + 2 * ZS_WS_CODE_STRIDE;
    const uint32_t nbSeqBytes = nbSeq < 128 ? 1 : nbSeq < 0x7F00 ? 2 : 3;      // Number_of_Sequences: n / (n >> 8) + 0x80, n & 0xFF / 0xFF, n - 0x7F00 (LE)
    if (lane == 0) put_le(op, nbSeqBytes == 1 ? nbSeq : nbSeqBytes == 2 ? ((nbSeq >> 8) + 0x80) | ((nbSeq & 0xFF) << 8) : 0xFF | ((nbSeq - 0x7F00) << 8), nbSeqBytes);
    op += nbSeqBytes;
    if (nbSeq == 0) return (uint32_t)(op - op0);
    // codes + the three histograms (all lanes); cnt layout: [0..35] LL, [64..95] OF, [128..180] ML inside hist2
    uint32_t* const cLL = L.hist2; uint32_t* const cOF = L.hist2 + 64; uint32_t* const cML = L.hist2 + 128;
    for (uint32_t i = lane; i < 192; i += LANES) L.hist2[i] = 0;
    __syncthreads();
    for (uint32_t u = lane; u < nbSeq; u += LANES) {
        const zs_seq q = seqs[u];
        const uint32_t a = LLcode(q.litLength), b = hb32(q.offBase), c = MLcode(q.mlBase);
        llC[u] = (uint8_t)a; ofC[u] = (uint8_t)b; mlC[u] = (uint8_t)c;
        atomicAdd(&cLL[a], 1u); atomicAdd(&cOF[b], 1u); atomicAdd(&cML[c], 1u);
    }
    stage_sync();
    PT(8);
    if (lane == 0) {
        uint8_t* const seqHead = op; uint8_t* q = op + 1;
        // LL, OF, ML in the order of their descriptions; the first failure ends it
        const struct { FseTable* ct; uint32_t fseLog; uint32_t* cnt; uint32_t maxSym; const uint8_t* codes; const short* defNorm; uint32_t defLog, defMax; bool isOffsets; } tabs[3] = {
            {&L.ll, ZS_LLFSELog, cLL, ZS_MaxLL, llC, kLLdefaultNorm, 6, ZS_MaxLL, false},
            {&L.of, ZS_OffFSELog, cOF, ZS_MaxOff, ofC, kOFdefaultNorm, 5, ZS_DefaultMaxOff, true},
            {&L.ml, ZS_MLFSELog, cML, ZS_MaxML, mlC, kMLdefaultNorm, 6, ZS_MaxML, false}};
        uint32_t type[3] = {0, 0, 0}, lastCountSize = 0, fail = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (fail) continue;
            const uint32_t sz = build_seq_table(q, *tabs[k].ct, tabs[k].fseLog, tabs[k].cnt, tabs[k].maxSym, tabs[k].codes, nbSeq, tabs[k].defNorm, tabs[k].defLog,
                                                tabs[k].defMax, tabs[k].isOffsets, L, &type[k]);
            if (sz == 0xFFFFFFFFu) { fail = 1; continue; }
            if (type[k] == 2) lastCountSize = sz;
            q += sz;
        }
        // lane 0 hands over: where the bit stream starts, the count size rule, failure
        L.scal[ZS_SCAL_SEQ_QOFF] = fail ? 0xFFFFFFFFu : (uint32_t)(q - op0);
        L.scal[ZS_SCAL_SEQ_COUNTSIZE] = lastCountSize;
        if (!fail) *seqHead = (uint8_t)((type[0] << 6) + (type[1] << 4) + (type[2] << 2));
        PT(9);
    }
    stage_sync();
    const uint32_t qoff = L.scal[ZS_SCAL_SEQ_QOFF], lastCountSize = L.scal[ZS_SCAL_SEQ_COUNTSIZE];
    __syncthreads();
    if (qoff == 0xFFFFFFFFu) return 0xFFFFFFFFu;
    // ---- ZSTD_encodeSequences, wave-parallel ----
    // (A) the three FSE state machines are independent chains: lanes 0 / 1 / 2 walk LL / OF / ML from the last sequence to
    //     the first and record, per sequence, the bits each transition emits (value | nbBits << 12).
    uint16_t* const stb = (uint16_t*)(codes + 3 * ZS_WS_CODE_STRIDE);
    uint32_t finalState = 0, finalLog = 0;
    if (lane < 3) {
        const FseTable& ct = lane == 0 ? L.ll : lane == 1 ? L.of : L.ml;
        const uint8_t* __restrict__ cd = codes + lane * ZS_WS_CODE_STRIDE;
        uint16_t* __restrict__ o = stb + lane * ZS_WS_CODE_STRIDE;
        uint32_t st = fse_init2(ct, cd[nbSeq - 1]);
        o[nbSeq - 1] = 0;
        if (nbSeq >= 2) {                                           // codes are read 8 at a time, one group ahead of their use
            int32_t n = (int32_t)nbSeq - 2;
            uint32_t g = (uint32_t)n & ~7u;
            uint64_t cur = *reinterpret_cast<const uint64_t*>(cd + g);
            for (;;) {
                const uint64_t nxt = g >= 8 ? *reinterpret_cast<const uint64_t*>(cd + g - 8) : 0;
                const int top = n & 7;
                // the per-symbol constants do not depend on the state: fetch all eight before walking the dependent chain,
                // which then costs one LDS lookup (the next state) per symbol
                uint32_t dn[8]; int32_t df[8];
#pragma unroll
                for (int j = 0; j < 8; j++) { const uint32_t sym = (uint32_t)(cur >> (8 * j)) & 0xFF; dn[j] = ct.dnb[sym < 56 ? sym : 0]; df[j] = ct.dfs[sym < 56 ? sym : 0]; }
                uint32_t ob[4] = {0, 0, 0, 0};
#pragma unroll
                for (int j = 7; j >= 0; j--) {
                    if (j <= top) {
                        const uint32_t nb = (st + dn[j]) >> 16;
                        ob[j >> 1] |= ((st & ((1u << nb) - 1)) | (nb << 12)) << (16 * (j & 1));
                        st = ct.state[(st >> nb) + df[j]];
                    }
                }
                if (top == 7) *reinterpret_cast<uint4*>(o + g) = make_uint4(ob[0], ob[1], ob[2], ob[3]);
                else {
#pragma unroll
                    for (int j = 0; j < 8; j++) if (j <= top) o[g + j] = (uint16_t)(ob[j >> 1] >> (16 * (j & 1)));
                }
                if (g == 0) break;
                g -= 8; n = (int32_t)g + 7; cur = nxt;
            }
        }
        finalState = st & ((1u << ct.tableLog) - 1); finalLog = ct.tableLog;
    }
    stage_sync();
    PT(10);
    // (B) every lane packs a contiguous run of sequences (in emission order: last sequence first)
    const uint32_t fLL = __shfl(finalState, 0), fOF = __shfl(finalState, 1), fML = __shfl(finalState, 2);
    const uint32_t gLL = __shfl(finalLog, 0), gOF = __shfl(finalLog, 1), gML = __shfl(finalLog, 2);
    WavePack p;
    wp_range(p, nbSeq, lane);
    uint32_t bits = 0;
    for (uint32_t r = p.r0; r < p.r1; r++) {
        const uint32_t n = nbSeq - 1 - r;
        bits += (stb[n] >> 12) + (stb[ZS_WS_CODE_STRIDE + n] >> 12) + (stb[2 * ZS_WS_CODE_STRIDE + n] >> 12) + kLLbits[llC[n]] + kMLbits[mlC[n]] + ofC[n];
    }
    if (lane == LANES - 1) bits += gML + gOF + gLL;                 // final states
    const uint32_t totalBits = wp_scan(p, bits, lane);
    const uint32_t bitstreamSize = (totalBits + 7) / 8;
    uint8_t* const q = op0 + qoff;
    if (q + bitstreamSize > oend || bitstreamSize > tmpCap) return 0xFFFFFFFFu;       // does not fit: the block goes out raw
    wp_begin(p, tmp, totalBits, lane);
    for (uint32_t r = p.r0; r < p.r1; r++) {
        const uint32_t n = nbSeq - 1 - r;
        const zs_seq sq = seqs[n];
        const uint32_t lc = llC[n], oc = ofC[n], mc = mlC[n];
        const uint32_t sLL = stb[n], sOF = stb[ZS_WS_CODE_STRIDE + n], sML = stb[2 * ZS_WS_CODE_STRIDE + n];
        const uint32_t nOF = sOF >> 12, nML = sML >> 12, nLL = sLL >> 12;
        const uint32_t v1 = (sOF & 0xFFF) | ((sML & 0xFFF) << nOF) | ((sLL & 0xFFF) << (nOF + nML));
        wp_put(p, v1, nOF + nML + nLL);
        const uint32_t bl = kLLbits[lc], bm = kMLbits[mc];
        const uint64_t v2 = (uint64_t)(sq.litLength & ((1u << bl) - 1)) | ((uint64_t)(sq.mlBase & ((1u << bm) - 1)) << bl);
        wp_put(p, v2, bl + bm);
        wp_put(p, sq.offBase & (uint32_t)((1ull << oc) - 1), oc);
    }
    if (lane == LANES - 1) { wp_put(p, fML, gML); wp_put(p, fOF, gOF); wp_put(p, fLL, gLL); }
    wp_finish(p, lane);
    wave_copy(q, (const uint8_t*)tmp, bitstreamSize, lane);
    stage_sync();
    PT(10);
    if (lastCountSize && (lastCountSize + bitstreamSize) < 4) return 0xFFFFFFFFu;
    return qoff + bitstreamSize;
}

// Per-lane copy of a short run with up to 32 bytes of loads in flight before the first store (a byte loop would pay one
// memory round trip per byte).
__device__ static inline void copy_run(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t n) {
    uint32_t k = 0;
    while (n - k >= 32) {
        const uint64_t a = ld64(src + k), b = ld64(src + k + 8), c = ld64(src + k + 16), d = ld64(src + k + 24);
        __builtin_memcpy(dst + k, &a, 8); __builtin_memcpy(dst + k + 8, &b, 8); __builtin_memcpy(dst + k + 16, &c, 8); __builtin_memcpy(dst + k + 24, &d, 8);
        k += 32;
    }
    const uint32_t r = n - k, nq = r >> 3;
    uint64_t q0 = 0, q1 = 0, q2 = 0; uint32_t w = 0; uint16_t h = 0; uint8_t b1 = 0;
    if (nq > 0) q0 = ld64(src + k);
    if (nq > 1) q1 = ld64(src + k + 8);
    if (nq > 2) q2 = ld64(src + k + 16);
    const uint32_t t = k + 8 * nq;
    if (r & 4) __builtin_memcpy(&w, src + t, 4);
    if (r & 2) __builtin_memcpy(&h, src + t + (r & 4), 2);
    if (r & 1) b1 = src[t + (r & 6)];
    if (nq > 0) __builtin_memcpy(dst + k, &q0, 8);
    if (nq > 1) __builtin_memcpy(dst + k + 8, &q1, 8);
    if (nq > 2) __builtin_memcpy(dst + k + 16, &q2, 8);
    if (r & 4) __builtin_memcpy(dst + t, &w, 4);
    if (r & 2) __builtin_memcpy(dst + t + (r & 4), &h, 2);
    if (r & 1) dst[t + (r & 6)] = b1;
}

// Literals of a parsed block, gathered by all lanes: sequence u's run is src[litPos, litPos + litLength) and lands at the
// running sum of the earlier runs; the tail after the last match follows.
__device__ ZS_NOINLINE static void gather_literals(uint8_t* __restrict__ lit, const uint8_t* __restrict__ src, const zs_seq* __restrict__ seqs,
                                                   uint32_t nbSeq, uint32_t tailPos, uint32_t tailLen, uint32_t lane) {
    uint32_t base = 0;
    for (uint32_t g = 0; g < nbSeq; g += LANES) {
        const uint32_t u = g + lane;
        uint32_t ll = 0, lp = 0;
        if (u < nbSeq) { const zs_seq q = seqs[u]; ll = q.litLength; lp = q.litPos; }
        uint32_t incl = ll;
        for (int o = 1; o < LANES; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if (lane >= (uint32_t)o) incl += t; }
        const uint32_t dst = base + incl - ll;
        copy_run(lit + dst, src + lp, ll);
        base += __shfl(incl, LANES - 1);
    }
    for (uint32_t i = lane; i < tailLen; i += LANES) lit[base + i] = src[tailPos + i];
}
