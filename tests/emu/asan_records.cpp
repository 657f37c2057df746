// TEST HARNESS ONLY: the bounds of the record-batch validator (csrc/records.hip, TSX_VALIDATE_RECORDS) under AddressSanitizer.  ONE
// executable: the emulated sources compiled with -fsanitize=address + this driver (csrc/Makefile, emu-asan-records).  A valid segment of v2
// record batches and every damaged variant of it - one byte of one batch at a time, hostile lengths, bad stream ends, a header split at
// every byte - go through tsx_transform_batch as 4099-byte chunks.  The source is handed over as device memory in its own heap block that
// ends with the last chunk's last byte, and the gaps between the chunks' slots are poisoned: a kernel that reads one byte outside the
// chunks the descriptors name ends the program with a report.  Statuses and tsx_records_info are compared with a serial walk made here.
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tsxform.h"

typedef std::vector<uint8_t> Bytes;
static int g_failed = 0, g_runs = 0;
#define CHECK(c) do { if (!(c)) { printf("  FAIL line %d (%s): %s\n", __LINE__, g_case.c_str(), #c); g_failed++; } } while (0)
static std::string g_case;

static uint32_t crc32c(const uint8_t* p, size_t n) {
    static uint32_t tab[256];
    if (!tab[1]) for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u))); tab[i] = c; }
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) c = tab[(c ^ p[i]) & 0xFF] ^ (c >> 8);
    return ~c;
}
static void be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }
static uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
static uint32_t g_lcg = 12345;
static uint32_t lcg() { g_lcg = g_lcg * 1103515245u + 12345u; return g_lcg >> 8; }
static void appendBatch(Bytes& s, uint32_t total, uint32_t baseOffset, uint8_t attributes) {
    const size_t at = s.size();
    s.resize(at + total, 0);
    uint8_t* p = s.data() + at;
    be32(p + 4, baseOffset); be32(p + 8, total - 12); p[16] = 2; p[22] = attributes; be32(p + 57, total > 61 ? 1 : 0);
    for (uint32_t i = 61; i < total; i++) p[i] = (uint8_t)(lcg() % 7 ? "offset=key=value=ts=\n"[i % 21] : lcg());
    be32(p + 17, crc32c(p + 21, total - 21));
}

struct Walk { uint64_t batches, compressed, badPos; uint32_t reason; };
static Walk referenceWalk(const Bytes& s) {
    Walk w{0, 0, UINT64_MAX, 0};
    size_t p = 0;
    const size_t n = s.size();
    while (p < n) {
        uint32_t why = 0;
        const int32_t len = n - p >= 61 ? (int32_t)rd32(&s[p + 8]) : 0;
        if (n - p < 61) why = 1;
        else if (len < 49) why = 2;
        else if ((uint64_t)len > n - p - 12) why = 1;
        else if (s[p + 16] != 2) why = 3;
        else if (crc32c(&s[p + 21], (size_t)len - 9) != rd32(&s[p + 17])) why = 4;
        if (why) { w.badPos = p; w.reason = why; return w; }
        w.batches++; w.compressed += (s[p + 22] & 7) != 0;
        p += 12 + (size_t)len;
    }
    return w;
}

// `stream` cut into `sizes` through a transform with the flag; the expectations come from referenceWalk
static void runCase(tsx_ctx* ctx, const Bytes& stream, const std::vector<uint32_t>& sizes, uint32_t flags) {
    g_runs++;
    const uint32_t n = (uint32_t)sizes.size();
    std::vector<tsx_chunk_desc> d(n);
    size_t so = 0, dof = 0, srcEnd = 0;
    for (uint32_t i = 0; i < n; i++) {
        memset(&d[i], 0, sizeof d[i]);
        d[i].src_off = so; d[i].src_len = sizes[i]; d[i].dst_off = dof; d[i].dst_cap = (uint32_t)tsx_transformed_bound(sizes[i], flags);
        srcEnd = so + sizes[i];
        so += ((sizes[i] + 15) & ~(size_t)15) + 16; dof += ((d[i].dst_cap + 15) & ~(size_t)15) + 16;
    }
    uint8_t* src = (uint8_t*)aligned_alloc(16, (srcEnd + 15) & ~(size_t)15 ? (srcEnd + 15) & ~(size_t)15 : 16);
    memset(src, 0xA5, (srcEnd + 15) & ~(size_t)15);
    size_t at = 0;
    for (uint32_t i = 0; i < n; i++) { if (sizes[i]) memcpy(src + d[i].src_off, stream.data() + at, sizes[i]); at += sizes[i]; }
    CHECK(at == stream.size());
    for (uint32_t i = 0; i < n; i++) {                                  // everything between two chunks, and behind the last one, is out of bounds
        const size_t lo = d[i].src_off + sizes[i], hi = i + 1 < n ? d[i + 1].src_off : (srcEnd + 15) & ~(size_t)15;
        if (hi > lo) ASAN_POISON_MEMORY_REGION(src + lo, hi - lo);
    }
    Bytes dst(dof + 16);
    tsx_batch_params p; memset(&p, 0, sizeof p);
    p.flags = flags | TSX_VALIDATE_RECORDS; p.zstd_profile = TSX_ZSTD_PROFILE_1_5_7;
    const int rc = tsx_transform_batch(ctx, &p, d.data(), n, src, srcEnd, dst.data(), dst.size(), TSX_MEM_DEVICE);
    CHECK(rc == TSX_OK);
    const Walk w = referenceWalk(stream);
    uint32_t bad = n;
    at = 0;
    for (uint32_t i = 0; i < n; i++) { if (sizes[i] && w.badPos >= at && w.badPos < at + sizes[i]) bad = i; at += sizes[i]; }
    CHECK((w.reason != 0) == (bad < n));
    at = 0;
    for (uint32_t i = 0; i < n; i++) {
        CHECK(d[i].status == (i >= bad ? TSX_E_RECORDS : TSX_OK));
        if (i < bad) CHECK(d[i].dst_len == sizes[i] && (!sizes[i] || memcmp(dst.data() + d[i].dst_off, stream.data() + at, sizes[i]) == 0));
        else CHECK(d[i].dst_len == 0);
        at += sizes[i];
    }
    tsx_records_info info;
    CHECK(tsx_ctx_records(ctx, &info) == TSX_OK);
    CHECK(info.batches == w.batches && info.compressed_batches == w.compressed && info.first_bad_pos == w.badPos && info.first_bad_reason == w.reason);
    ASAN_UNPOISON_MEMORY_REGION(src, (srcEnd + 15) & ~(size_t)15);
    free(src);
}

static std::vector<uint32_t> cut(size_t total, uint32_t size) {
    std::vector<uint32_t> v;
    for (size_t a = 0; a < total; a += size) v.push_back((uint32_t)(total - a < size ? total - a : size));
    if (v.empty()) v.push_back(0);
    return v;
}

int main() {
    setenv("TSX_ALLOW_ANY_ARCH", "1", 1);                               // the emulator reports arch "emu"
    if (tsx_init(1, nullptr) < 1) { printf("tsx_init failed\n"); return 2; }
    tsx_ctx* ctx = nullptr;
    if (tsx_ctx_create(0, 0, 0, &ctx) != TSX_OK) { printf("tsx_ctx_create failed\n"); return 2; }
    const uint32_t CUT = 4099;
    Bytes seg;
    std::vector<size_t> starts;
    for (uint32_t i = 0; i < 19; i++) { starts.push_back(seg.size()); appendBatch(seg, 3600 + lcg() % 30000, i, (uint8_t)(i % 4 == 3)); }
    size_t p = 0, l = 0;                                                // a batch of at least three chunks that begins in chunk >= 2
    for (size_t i = 0; i < starts.size() && !l; i++) {
        const size_t len = (i + 1 < starts.size() ? starts[i + 1] : seg.size()) - starts[i];
        if (len >= 3 * CUT && starts[i] / CUT >= 2) { p = starts[i]; l = len; }
    }
    if (!l) { printf("no long batch\n"); return 2; }
    g_case = "clean";
    for (uint32_t size : {CUT, 65536u, (uint32_t)seg.size()}) runCase(ctx, seg, cut(seg.size(), size), TSX_CRC);
    {   // two zero-length chunks inserted
        std::vector<uint32_t> s = cut(seg.size(), CUT);
        s.insert(s.begin() + 9, 0); s.insert(s.begin(), 0);
        runCase(ctx, seg, s, 0);
    }
    // ---- one byte at a time ----
    const size_t one[] = {p + 8, p + 9, p + 10, p + 11, p + 16, p + 17, p + 18, p + 19, p + 20, p + 21, p + l - 1, p + 61 + 2 * CUT, p + 3, p + 13};
    for (size_t at : one) {
        g_case = "byte " + std::to_string(at - p);
        Bytes b = seg; b[at] ^= 1;
        runCase(ctx, b, cut(b.size(), CUT), TSX_CRC);
    }
    // ---- hostile lengths ----
    for (uint32_t v : {0x7FFFFFFFu, 0x80000000u, 48u, 0xFFFFFFFFu, 0u, (uint32_t)(seg.size() - p - 12 + 1)}) {
        g_case = "length " + std::to_string(v);
        Bytes b = seg; be32(&b[p + 8], v);
        runCase(ctx, b, cut(b.size(), CUT), TSX_CRC);
        Bytes first = seg; be32(&first[8], v);                          // ... and in the very first batch
        runCase(ctx, first, cut(first.size(), CUT), 0);
    }
    // ---- stream ends ----
    {
        g_case = "ends";
        Bytes b(seg.begin(), seg.end() - 1); runCase(ctx, b, cut(b.size(), CUT), TSX_CRC);
        b.assign(seg.begin(), seg.end() - 61); runCase(ctx, b, cut(b.size(), CUT), TSX_CRC);
        b = seg; b.push_back(0x5A); runCase(ctx, b, cut(b.size(), CUT), TSX_CRC);
        b = seg; b.insert(b.end(), 60, 0x5A); runCase(ctx, b, cut(b.size(), CUT), TSX_CRC);
        b = seg; b.insert(b.end(), 4096, 0); runCase(ctx, b, cut(b.size(), CUT), TSX_CRC);
        b.assign(seg.begin(), seg.begin() + 30); runCase(ctx, b, cut(b.size(), CUT), 0);      // a stream shorter than a header
    }
    // ---- a header split at every byte; the first batch of a chunk damaged; a batch inside a record value ----
    {
        Bytes two; appendBatch(two, 261, 0, 0); appendBatch(two, 361, 1, 4);
        for (uint32_t k = 0; k <= 60; k++) {
            g_case = "split " + std::to_string(k);
            runCase(ctx, two, {261 + k, 361 - k}, 0);
            Bytes b = two; b[261 + 60] ^= 1;
            runCase(ctx, b, {261 + k, 361 - k}, 0);
        }
        g_case = "first batch of a chunk";
        Bytes b = seg; b[starts[4] + 20] ^= 1;
        runCase(ctx, b, cut(b.size(), CUT), TSX_CRC);
        g_case = "nested";
        Bytes inner; appendBatch(inner, 511, 77, 1);
        Bytes s; appendBatch(s, 1000, 0, 0);
        const size_t outerAt = s.size();
        appendBatch(s, 61 + (CUT - 1061) + 511 + 300, 1, 0);
        memcpy(&s[CUT], inner.data(), inner.size());
        be32(&s[outerAt + 17], crc32c(&s[outerAt + 21], 61 + (CUT - 1061) + 511 + 300 - 21));
        for (uint32_t i = 0; i < 5; i++) appendBatch(s, 1500 + 100 * i, 2 + i, (uint8_t)(i & 1));
        runCase(ctx, s, cut(s.size(), CUT), TSX_CRC);
        tsx_records_info info;
        CHECK(tsx_ctx_records(ctx, &info) == TSX_OK && info.batches == 7 && info.repaired_chunks >= 1);
    }
    tsx_ctx_destroy(ctx);
    tsx_shutdown();
    printf("asan records: %d runs, %d failed\n", g_runs, g_failed);
    return g_failed ? 1 : 0;
}
