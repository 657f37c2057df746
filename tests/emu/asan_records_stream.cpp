// TEST HARNESS ONLY: the bounds of the record-batch validator on a stream given in SEVERAL calls (tsx_transform_batch_stream) under
// AddressSanitizer.  ONE executable: the emulated sources compiled with -fsanitize=address + this driver (csrc/Makefile,
// emu-asan-records-stream).  Every call's source is a heap block of its own that ends with the call's last byte, with the gaps between
// the chunks' slots poisoned, and the state lives in a heap block of exactly 192 bytes: a kernel that reads one byte behind the call's
// bytes - the look-ahead load of the next header, a speculating walker's candidate, the CRC of a batch that is still open - or a host
// that touches byte 192 of the state ends the program with a report.  The matrices are those of tests/test_emu_records_stream.py: the
// call boundary at every byte of a header and around the ends, and a damaged segment in calls of 1 and 5 chunks.  Statuses and the
// result are compared with a serial walk over the whole stream made here.
#include <sanitizer/asan_interface.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tsxform.h"

typedef std::vector<uint8_t> Bytes;
typedef std::vector<std::vector<uint32_t>> Calls;
static int g_failed = 0, g_runs = 0;
static std::string g_case;
#define CHECK(c) do { if (!(c)) { printf("  FAIL line %d (%s): %s\n", __LINE__, g_case.c_str(), #c); g_failed++; } } while (0)

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

// the serial walk, and d: the last byte the verdict needs
struct Walk { uint64_t batches, compressed, badPos, d; uint32_t reason; };
static Walk referenceWalk(const Bytes& s) {
    Walk w{0, 0, UINT64_MAX, UINT64_MAX, 0};
    size_t p = 0;
    const size_t n = s.size();
    while (p < n) {
        uint32_t why = 0;
        const int32_t len = n - p >= 61 ? (int32_t)rd32(&s[p + 8]) : 0;
        uint64_t d = p + 60;
        if (n - p < 61) { why = 1; d = p; }
        else if (len < 49) why = 2;
        else if ((uint64_t)len > n - p - 12) why = 1;
        else if (s[p + 16] != 2) why = 3;
        else if (crc32c(&s[p + 21], (size_t)len - 9) != rd32(&s[p + 17])) { why = 4; d = p + 12 + (uint64_t)len - 1; }
        if (why) { w.badPos = p; w.reason = why; w.d = d; return w; }
        w.batches++; w.compressed += (s[p + 22] & 7) != 0;
        p += 12 + (size_t)len;
    }
    return w;
}

// `stream` in calls.size() calls on one state; the expectations come from referenceWalk and the rule of include/tsxform.h
static void runCase(tsx_ctx* const* ctxs, const Bytes& stream, const Calls& calls, uint32_t flags) {
    g_runs++;
    const Walk w = referenceWalk(stream);
    tsx_records_state* const st = (tsx_records_state*)malloc(TSX_RECORDS_STATE_BYTES);       // exactly 192 bytes
    CHECK(tsx_records_begin(st, stream.size()) == TSX_OK);
    uint64_t base = 0;
    for (size_t k = 0; k < calls.size(); k++) {
        const std::vector<uint32_t>& sizes = calls[k];
        const uint32_t n = (uint32_t)sizes.size();
        std::vector<tsx_chunk_desc> d(n ? n : 1);
        size_t so = 0, dof = 0, srcEnd = 0, bytes = 0;
        for (uint32_t i = 0; i < n; i++) {
            memset(&d[i], 0, sizeof d[i]);
            d[i].src_off = so; d[i].src_len = sizes[i]; d[i].dst_off = dof; d[i].dst_cap = (uint32_t)tsx_transformed_bound(sizes[i], flags);
            if (sizes[i]) srcEnd = so + sizes[i];
            so += ((sizes[i] + 15) & ~(size_t)15) + 16; dof += ((d[i].dst_cap + 15) & ~(size_t)15) + 16;
            bytes += sizes[i];
        }
        for (uint32_t i = 0; i < n; i++) if (d[i].src_off > srcEnd) d[i].src_off = srcEnd & ~(size_t)15;     // (empty chunks behind the last byte)
        uint8_t* src = (uint8_t*)malloc(srcEnd ? srcEnd : 1);           // ends with the call's last byte
        memset(src, 0xA5, srcEnd ? srcEnd : 1);
        size_t at = 0;
        for (uint32_t i = 0; i < n; i++) { if (sizes[i]) memcpy(src + d[i].src_off, stream.data() + base + at, sizes[i]); at += sizes[i]; }
        size_t covered = 0;
        for (uint32_t i = 0; i < n; i++) {                              // everything between two chunks is out of bounds
            if (!sizes[i]) continue;
            if (d[i].src_off > covered) ASAN_POISON_MEMORY_REGION(src + covered, d[i].src_off - covered);
            covered = d[i].src_off + sizes[i];
        }
        if (!srcEnd) ASAN_POISON_MEMORY_REGION(src, 1);
        Bytes dst(dof + 16);
        tsx_batch_params p; memset(&p, 0, sizeof p);
        p.flags = flags | TSX_VALIDATE_RECORDS; p.zstd_profile = TSX_ZSTD_PROFILE_1_5_7;
        const int rc = tsx_transform_batch_stream(ctxs[k % 3], &p, d.data(), n, src, srcEnd, dst.data(), dst.size(), TSX_MEM_DEVICE, st);
        CHECK(rc == TSX_OK);
        // the rule
        uint32_t bad = n;                                               // first chunk that is not delivered
        if (w.reason && w.d < base) bad = 0;
        else if (w.reason && w.d < base + bytes) {
            const uint64_t want = w.badPos > base ? w.badPos : base;
            uint64_t q = base;
            for (uint32_t i = 0; i < n; i++) { if (sizes[i] && want >= q && want < q + sizes[i]) bad = i; q += sizes[i]; }
            CHECK(bad < n);
        }
        at = 0;
        for (uint32_t i = 0; i < n; i++) {
            CHECK(d[i].status == (i >= bad ? TSX_E_RECORDS : TSX_OK));
            if (i < bad) CHECK(d[i].dst_len == sizes[i] && (!sizes[i] || memcmp(dst.data() + d[i].dst_off, stream.data() + base + at, sizes[i]) == 0));
            else CHECK(d[i].dst_len == 0);
            at += sizes[i];
        }
        base += bytes;
        tsx_records_info info;
        CHECK(tsx_records_result(st, &info) == (base == stream.size() ? 1 : 0));
        ASAN_UNPOISON_MEMORY_REGION(src, srcEnd ? srcEnd : 1);
        free(src);
    }
    CHECK(base == stream.size());
    tsx_records_info info;
    CHECK(tsx_records_result(st, &info) == 1);
    CHECK(info.batches == w.batches && info.compressed_batches == w.compressed && info.first_bad_pos == w.badPos && info.first_bad_reason == w.reason);
    free(st);
}

static std::vector<uint32_t> cut(size_t total, uint32_t size) {
    std::vector<uint32_t> v;
    for (size_t a = 0; a < total; a += size) v.push_back((uint32_t)(total - a < size ? total - a : size));
    return v;
}
static Calls split(const std::vector<uint32_t>& sizes, size_t per) {
    Calls c;
    for (size_t a = 0; a < sizes.size(); a += per) c.push_back(std::vector<uint32_t>(sizes.begin() + (long)a, sizes.begin() + (long)(a + per < sizes.size() ? a + per : sizes.size())));
    return c;
}

int main() {
    setenv("TSX_ALLOW_ANY_ARCH", "1", 1);                               // the emulator reports arch "emu"
    if (tsx_init(1, nullptr) < 1) { printf("tsx_init failed\n"); return 2; }
    tsx_ctx* ctxs[3] = {nullptr, nullptr, nullptr};                     // [2] stays NULL: the pool
    for (int i = 0; i < 2; i++) if (tsx_ctx_create(0, 0, 0, &ctxs[i]) != TSX_OK) { printf("tsx_ctx_create failed\n"); return 2; }
    // ---- the boundary at every byte: three batches of 200, 61 and 300 bytes ----
    Bytes three; appendBatch(three, 200, 0, 0); appendBatch(three, 61, 1, 0); appendBatch(three, 300, 2, 2);
    const struct { const char* name; int at; } variants[] = {{"clean", -1}, {"length", 211}, {"magic", 216}, {"crc", 219}, {"last", 260}};
    for (const auto& var : variants) {
        Bytes v = three;
        if (var.at >= 0) v[(size_t)var.at] ^= 1;
        uint32_t k = 0;
        for (uint32_t q = 198; q <= 561; q++) {
            if (q > 263 && q < 559) continue;
            // chunks of 7 and 64 bytes at every cut, of 1 byte at every third
            for (uint32_t size : {1u, 7u, 64u}) {
                if (size == 1 && q % 3) continue;
                g_case = std::string(var.name) + " cut " + std::to_string(q) + " by " + std::to_string(size);
                runCase(ctxs, v, {cut(q, size), cut(v.size() - q, size)}, (k++ & 1) ? TSX_CRC : 0);
            }
        }
        for (uint32_t mid : {1u, 20u, 59u, 60u, 61u}) {
            g_case = std::string(var.name) + " middle " + std::to_string(mid);
            runCase(ctxs, v, {cut(203, 64), cut(mid, 7), cut(v.size() - 203 - mid, 64)}, 0);
            runCase(ctxs, v, {cut(203, 1), cut(mid, 1), cut(v.size() - 203 - mid, 7)}, TSX_CRC);
        }
        g_case = std::string(var.name) + " empty calls";
        std::vector<uint32_t> last = cut(v.size() - 230, 7); last.push_back(0);
        runCase(ctxs, v, {cut(230, 64), {}, {0, 0, 0}, last}, 0);
    }
    // ---- damage: a segment of 19 batches in calls of 1 and 5 chunks of 4099 bytes ----
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
    std::vector<std::pair<std::string, Bytes>> damaged;
    damaged.push_back({"clean", seg});
    for (size_t at : {p + 8, p + 9, p + 10, p + 11, p + 16, p + 17, p + 18, p + 19, p + 20, p + 21, p + l - 1, p + 61 + 2 * CUT, p + 3, p + 13}) {
        Bytes b = seg; b[at] ^= 1; damaged.push_back({"byte " + std::to_string(at - p), b});
    }
    for (uint32_t v : {0x7FFFFFFFu, 0x80000000u, 48u}) { Bytes b = seg; be32(&b[p + 8], v); damaged.push_back({"length " + std::to_string(v), b}); }
    { Bytes b(seg.begin(), seg.end() - 1); damaged.push_back({"cut1", b}); }
    { Bytes b(seg.begin(), seg.end() - 61); damaged.push_back({"cut61", b}); }
    { Bytes b = seg; b.push_back(0x5A); damaged.push_back({"garbage1", b}); }
    { Bytes b = seg; b.insert(b.end(), 60, 0x5A); damaged.push_back({"garbage60", b}); }
    { Bytes b = seg; b.insert(b.end(), 4096, 0); damaged.push_back({"zeros4096", b}); }
    for (const auto& c : damaged)
        for (size_t per : {1u, 5u}) {
            g_case = c.first + " in calls of " + std::to_string(per);
            runCase(ctxs, c.second, split(cut(c.second.size(), CUT), per), per == 1 ? TSX_CRC : 0);
        }
    for (int i = 0; i < 2; i++) tsx_ctx_destroy(ctxs[i]);
    tsx_shutdown();
    printf("asan records stream: %d runs, %d failed\n", g_runs, g_failed);
    return g_failed ? 1 : 0;
}
