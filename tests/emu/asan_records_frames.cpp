// TEST HARNESS ONLY: the bounds of the record walk (csrc/records_dev.h, TSX_VALIDATE_FRAMES) under AddressSanitizer.  ONE executable: the
// emulated sources compiled with -fsanitize=address + this driver (csrc/Makefile, emu-asan-records-frames).  A stream of well-framed v2
// record batches built here and every damaged variant of it - counts, lengths, inner fields, offset deltas, base offsets, each sealed
// with a valid CRC, on a batch inside a chunk, on a chunk's first byte, on the stream's first and last batch - go through
// tsx_transform_batch as 4099- and 65536-byte chunks.  The source is handed over as device memory in its own heap block that ends with the
// last chunk's last byte, and the gaps between the chunks' slots are poisoned: a kernel that follows a damaged length to one byte outside
// the chunks the descriptors name ends the program with a report.  Statuses and tsx_records_info are compared with a serial walk made here.
#include <sanitizer/asan_interface.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "tsxform.h"

typedef std::vector<uint8_t> Bytes;
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
static void be64(uint8_t* p, uint64_t v) { be32(p, (uint32_t)(v >> 32)); be32(p + 4, (uint32_t)v); }
static int64_t rd64(const uint8_t* p) { return (int64_t)((uint64_t)rd32(p) << 32 | rd32(p + 4)); }
static uint32_t g_lcg = 4711;
static uint32_t lcg() { g_lcg = g_lcg * 1103515245u + 12345u; return g_lcg >> 8; }

// ---- the builder ----
static Bytes varint(int64_t v, size_t padTo = 0) {
    uint64_t z = ((uint64_t)v << 1) ^ (uint64_t)(v >> 63);
    Bytes out;
    for (;;) {
        const uint8_t b = z & 0x7F; z >>= 7;
        if (z || out.size() + 1 < padTo) out.push_back(b | 0x80); else { out.push_back(b); break; }
    }
    return out;
}
static void add(Bytes& a, const Bytes& b) { a.insert(a.end(), b.begin(), b.end()); }
struct Rec {                                                            // raw*: the encoding of a field in place of the honest one
    int32_t delta = 0; Bytes key, value; bool nullKey = false, nullValue = false; Bytes headers; int32_t nHeaders = 0;
    bool hasLength = false, hasTs = false, hasDelta = false, hasKlen = false, hasVlen = false, hasHcount = false;
    Bytes rawLength, rawTs, rawDelta, rawKlen, rawVlen, rawHcount, tail;
    Bytes body() const {
        Bytes b{0};
        add(b, hasTs ? rawTs : varint(7)); add(b, hasDelta ? rawDelta : varint(delta));
        add(b, hasKlen ? rawKlen : varint(nullKey ? -1 : (int64_t)key.size())); if (!nullKey) add(b, key);
        add(b, hasVlen ? rawVlen : varint(nullValue ? -1 : (int64_t)value.size())); if (!nullValue) add(b, value);
        add(b, hasHcount ? rawHcount : varint(nHeaders)); add(b, headers); add(b, tail);
        return b;
    }
    Bytes bytes() const { const Bytes b = body(); Bytes r = hasLength ? rawLength : varint((int64_t)b.size()); add(r, b); return r; }
};
struct Batch {
    int64_t base = 0; std::vector<Rec> recs; uint16_t attributes = 0; bool hasRegion = false; Bytes region, slack;
    bool hasLod = false, hasCount = false, hasBaseDamage = false; int32_t lod = 0, count = 0; int64_t baseDamage = 0;
    int64_t last() const { return base + (hasLod ? lod : (recs.empty() ? 0 : (int32_t)recs.size() - 1)); }
    Bytes bytes() const {
        Bytes b(61, 0);
        if (hasRegion) add(b, region); else { for (const Rec& r : recs) add(b, r.bytes()); add(b, slack); }
        be64(&b[0], (uint64_t)base); be32(&b[8], (uint32_t)b.size() - 12); b[16] = 2; b[21] = (uint8_t)(attributes >> 8); b[22] = (uint8_t)attributes;
        be32(&b[23], (uint32_t)(hasLod ? lod : (recs.empty() ? 0 : (int32_t)recs.size() - 1)));
        memset(&b[43], 0xFF, 14);
        be32(&b[57], (uint32_t)(hasCount ? count : (int32_t)recs.size()));
        be32(&b[17], crc32c(&b[21], b.size() - 21));
        if (hasBaseDamage) be64(&b[0], (uint64_t)baseDamage);          // behind the seal: bytes 0..15 are outside the CRC
        return b;
    }
};
static Bytes filler(size_t n) { Bytes v(n); for (auto& x : v) x = (uint8_t)(lcg() % 7 ? "offset=key=value=ts=\n"[lcg() % 21] : lcg()); return v; }
static std::vector<Batch> builtBatches() {
    g_lcg = 4711;
    std::vector<Batch> out;
    for (int i = 0; i < 14; i++) {
        Batch b; b.base = 1000 + 100 * i;
        if (i == 4) { b.attributes = 2; b.hasRegion = true; b.region = filler(3000); b.hasLod = b.hasCount = true; b.lod = 30; b.count = 31; out.push_back(b); continue; }
        if (i == 9) { b.hasLod = true; b.lod = 17; out.push_back(b); continue; }
        if (i == 7) b.attributes = 0x20;
        for (int d = 0; d < 12 + i; d++) {
            static const size_t lens[5] = {0, 5, 130, 300, 700};
            Rec r; r.delta = d; r.key = filler(lcg() % 20); r.value = filler(lens[lcg() % 5]);
            if (d % 5 == 1) r.nullKey = true;
            if (d % 7 == 2) r.nullValue = true;
            if (d % 4 == 3) { r.nHeaders = 2; add(r.headers, varint(3)); add(r.headers, filler(3)); add(r.headers, varint(40)); add(r.headers, filler(40)); add(r.headers, varint(0)); add(r.headers, varint(-1)); }
            if (i == 5 && d == 6) r.value = filler(9000);             // a record over three 4099-byte chunks: longer than the walk's tile
            b.recs.push_back(r);
        }
        out.push_back(b);
    }
    return out;
}
static Bytes streamOf(const std::vector<Batch>& bs, std::vector<size_t>* starts = nullptr) {
    Bytes s;
    for (const Batch& b : bs) { if (starts) starts->push_back(s.size()); add(s, b.bytes()); }
    return s;
}

// ---- the reference: a serial walk ----
static bool readVarint(const Bytes& s, size_t& q, size_t lim, int width, int64_t* out) {
    uint64_t val = 0;
    for (int i = 0; i < width; i++) {
        if (q >= lim) return false;
        const uint8_t b = s[q++];
        if (7 * i < 64) val |= (uint64_t)(b & 0x7F) << (7 * i);
        if (!(b & 0x80)) {
            if (width == 5) { const uint32_t v = (uint32_t)val; *out = (int32_t)((v >> 1) ^ (0u - (v & 1u))); }
            else *out = (int64_t)((val >> 1) ^ (0ull - (val & 1ull)));
            return true;
        }
    }
    return false;
}
static bool sized(const Bytes& s, size_t& q, size_t e, int64_t least) {
    int64_t n;
    if (!readVarint(s, q, e, 5, &n) || n < least) return false;
    if (n > 0) { if ((uint64_t)n > e - q) return false; q += (size_t)n; }
    return true;
}
static uint32_t walkRecords(const Bytes& s, size_t q, size_t end, int32_t count, int32_t lod) {
    int64_t prev = -1;
    for (int32_t i = 0; i < count; i++) {
        int64_t len, d, nh;
        if (!readVarint(s, q, end, 5, &len) || len < 0 || (uint64_t)len > end - q) return 5;
        const size_t e = q + (size_t)len;
        size_t p = q;
        if (p >= e) return 5;
        p++;
        if (!readVarint(s, p, e, 10, &d)) return 5;
        if (!readVarint(s, p, e, 5, &d)) return 5;
        if (d < 0 || d > lod || d <= prev) return 6;
        prev = d;
        if (!sized(s, p, e, -1) || !sized(s, p, e, -1)) return 5;
        if (!readVarint(s, p, e, 5, &nh) || nh < 0) return 5;
        for (int64_t h = 0; h < nh; h++) if (!sized(s, p, e, 0) || !sized(s, p, e, -1)) return 5;
        if (p != e) return 5;
        q = e;
    }
    return q == end ? 0 : 5;
}
struct Walk { uint64_t batches, compressed, records, badPos; uint32_t reason; };
static Walk referenceWalk(const Bytes& s) {
    Walk w{0, 0, 0, UINT64_MAX, 0};
    size_t p = 0;
    const size_t n = s.size();
    bool have = false;
    int64_t last = 0;
    while (p < n) {
        uint32_t why = 0;
        const int32_t len = n - p >= 61 ? (int32_t)rd32(&s[p + 8]) : 0;
        if (n - p < 61) why = 1;
        else if (len < 49) why = 2;
        else if ((uint64_t)len > n - p - 12) why = 1;
        else if (s[p + 16] != 2) why = 3;
        else if (crc32c(&s[p + 21], (size_t)len - 9) != rd32(&s[p + 17])) why = 4;
        const size_t end = p + 12 + (size_t)len;
        int32_t count = 0;
        bool comp = false;
        if (!why) {
            const int64_t base = rd64(&s[p]);
            const int32_t lod = (int32_t)rd32(&s[p + 23]);
            count = (int32_t)rd32(&s[p + 57]); comp = (s[p + 22] & 7) != 0;
            if (base < 0 || lod < 0 || base > INT64_MAX - lod || (have && base <= last)) why = 6;
            else if (count < 0) why = 5;
            else if (!comp) why = walkRecords(s, p + 61, end, count, lod);
            if (!why) { have = true; last = base + lod; }
        }
        if (why) { w.badPos = p; w.reason = why; return w; }
        w.batches++; w.compressed += comp; if (!comp) w.records += (uint32_t)count;
        p = end;
    }
    return w;
}

// `stream` cut into `sizes` through a transform with both flags; the expectations come from referenceWalk
static void runCase(tsx_ctx* ctx, const Bytes& stream, const std::vector<uint32_t>& sizes, uint32_t flags, uint32_t wantReason, uint64_t wantPos) {
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
    const size_t srcAlloc = (srcEnd + 15) & ~(size_t)15;
    uint8_t* src = (uint8_t*)aligned_alloc(16, srcAlloc ? srcAlloc : 16);
    memset(src, 0xA5, srcAlloc);
    size_t at = 0;
    for (uint32_t i = 0; i < n; i++) { if (sizes[i]) memcpy(src + d[i].src_off, stream.data() + at, sizes[i]); at += sizes[i]; }
    CHECK(at == stream.size());
    for (uint32_t i = 0; i < n; i++) {                                  // everything between two chunks, and behind the last one, is out of bounds
        const size_t lo = d[i].src_off + sizes[i], hi = i + 1 < n ? d[i + 1].src_off : srcAlloc;
        if (hi > lo) ASAN_POISON_MEMORY_REGION(src + lo, hi - lo);
    }
    Bytes dst(dof + 16);
    tsx_batch_params p; memset(&p, 0, sizeof p);
    p.flags = flags | TSX_VALIDATE_RECORDS | TSX_VALIDATE_FRAMES; p.zstd_profile = TSX_ZSTD_PROFILE_1_5_7;
    const int rc = tsx_transform_batch(ctx, &p, d.data(), n, src, srcEnd, dst.data(), dst.size(), TSX_MEM_DEVICE);
    CHECK(rc == TSX_OK);
    const Walk w = referenceWalk(stream);
    CHECK(w.reason == wantReason && w.badPos == wantPos);               // (the reference itself against what the case was built to be)
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
    CHECK(info.batches == w.batches && info.compressed_batches == w.compressed && info.first_bad_pos == w.badPos && info.first_bad_reason == w.reason && info.records == w.records);
    ASAN_UNPOISON_MEMORY_REGION(src, srcAlloc);
    free(src);
}

// chunks of `size` bytes, one more boundary at `seam` (0: none), an empty chunk put in at index 1
static std::vector<uint32_t> cut(size_t total, uint32_t size, size_t seam = 0) {
    std::vector<size_t> cuts;
    for (size_t a = 0; a < total; a += size) cuts.push_back(a);
    cuts.push_back(total);
    if (seam && seam % size) { cuts.push_back(seam); std::sort(cuts.begin(), cuts.end()); }
    std::vector<uint32_t> v;
    for (size_t i = 0; i + 1 < cuts.size(); i++) v.push_back((uint32_t)(cuts[i + 1] - cuts[i]));
    if (v.empty()) v.push_back(0);
    v.insert(v.begin() + (v.size() > 1 ? 1 : 0), 0);
    return v;
}

struct Damage { const char* name; std::function<void(Batch&, const Batch*)> fn; uint32_t why; bool needsPrev; };
static void setRaw(Bytes& raw, bool& has, const Bytes& v) { raw = v; has = true; }

int main() {
    setenv("TSX_ALLOW_ANY_ARCH", "1", 1);                               // the emulator reports arch "emu"
    if (tsx_init(1, nullptr) < 1) { printf("tsx_init failed\n"); return 2; }
    tsx_ctx* ctx = nullptr;
    if (tsx_ctx_create(0, 0, 0, &ctx) != TSX_OK) { printf("tsx_ctx_create failed\n"); return 2; }
    auto length = [](int64_t plus, size_t padTo, bool absolute) {
        return [=](Batch& b, const Batch*) { Rec& r = b.recs[3]; const int64_t n = (int64_t)r.body().size(); setRaw(r.rawLength, r.hasLength, absolute ? varint(plus) : varint(n + plus, padTo)); };
    };
    const std::vector<Damage> damage = {
        {"count+1", [](Batch& b, const Batch*) { b.hasCount = true; b.count = (int32_t)b.recs.size() + 1; }, 5, false},
        {"count-1", [](Batch& b, const Batch*) { b.hasCount = true; b.count = (int32_t)b.recs.size() - 1; }, 5, false},
        {"count0", [](Batch& b, const Batch*) { b.hasCount = true; b.count = 0; }, 5, false},
        {"count<0", [](Batch& b, const Batch*) { b.hasCount = true; b.count = -1; }, 5, false},
        {"count max", [](Batch& b, const Batch*) { b.hasCount = true; b.count = 0x7FFFFFFF; }, 5, false},
        {"lod<last", [](Batch& b, const Batch*) { b.hasLod = true; b.lod = (int32_t)b.recs.size() - 2; }, 6, false},
        {"lod<0", [](Batch& b, const Batch*) { b.hasLod = true; b.lod = -1; }, 6, false},
        {"length+1", length(1, 0, false), 5, false}, {"length-1", length(-1, 0, false), 5, false}, {"length>batch", length(1 << 20, 0, false), 5, false},
        {"length max", length(0x7FFFFFFF, 0, true), 5, false}, {"length<0", length(-3, 0, true), 5, false}, {"length5bytes", length(0, 5, false), 0, false},
        {"length6bytes", length(0, 6, false), 5, false},
        {"length cut off", [](Batch& b, const Batch*) { b.slack = {0x80}; b.hasCount = true; b.count = (int32_t)b.recs.size() + 1; }, 5, false},
        {"klen>record", [](Batch& b, const Batch*) { setRaw(b.recs[3].rawKlen, b.recs[3].hasKlen, varint(10000)); }, 5, false},
        {"klen max", [](Batch& b, const Batch*) { setRaw(b.recs[3].rawKlen, b.recs[3].hasKlen, varint(0x7FFFFFFF)); }, 5, false},
        {"klen-2", [](Batch& b, const Batch*) { setRaw(b.recs[3].rawKlen, b.recs[3].hasKlen, varint(-2)); }, 5, false},
        {"vlen-2", [](Batch& b, const Batch*) { setRaw(b.recs[3].rawVlen, b.recs[3].hasVlen, varint(-2)); }, 5, false},
        {"vlen max", [](Batch& b, const Batch*) { setRaw(b.recs[3].rawVlen, b.recs[3].hasVlen, varint(0x7FFFFFFF)); }, 5, false},
        {"nulls", [](Batch& b, const Batch*) { b.recs[3].nullKey = b.recs[3].nullValue = true; }, 0, false},
        {"hcount-1", [](Batch& b, const Batch*) { setRaw(b.recs[3].rawHcount, b.recs[3].hasHcount, varint(-1)); }, 5, false},
        {"hcount max", [](Batch& b, const Batch*) { setRaw(b.recs[3].rawHcount, b.recs[3].hasHcount, varint(0x7FFFFFFF)); }, 5, false},
        {"hkey-1", [](Batch& b, const Batch*) { Rec& r = b.recs[3]; r.nHeaders = 1; r.headers = varint(-1); add(r.headers, varint(1)); r.headers.push_back('x'); }, 5, false},
        {"slack", [](Batch& b, const Batch*) { b.recs[3].tail = {0}; }, 5, false},
        {"ts11bytes", [](Batch& b, const Batch*) { Bytes t(10, 0x80); t.push_back(0); setRaw(b.recs[3].rawTs, b.recs[3].hasTs, t); }, 5, false},
        {"delta repeated", [](Batch& b, const Batch*) { setRaw(b.recs[3].rawDelta, b.recs[3].hasDelta, varint(2)); }, 6, false},
        {"delta decreasing", [](Batch& b, const Batch*) { setRaw(b.recs[3].rawDelta, b.recs[3].hasDelta, varint(1)); }, 6, false},
        {"delta>lod", [](Batch& b, const Batch*) { setRaw(b.recs.back().rawDelta, b.recs.back().hasDelta, varint((int64_t)b.recs.size())); }, 6, false},
        {"delta<0", [](Batch& b, const Batch*) { setRaw(b.recs[0].rawDelta, b.recs[0].hasDelta, varint(-1)); }, 6, false},
        {"base top bit", [](Batch& b, const Batch*) { b.hasBaseDamage = true; b.baseDamage = (int64_t)((uint64_t)b.base | 1ull << 63); }, 6, false},
        {"base=prev last", [](Batch& b, const Batch* p) { b.hasBaseDamage = true; b.baseDamage = p->last(); }, 6, true},
        {"base=prev last-1", [](Batch& b, const Batch* p) { b.hasBaseDamage = true; b.baseDamage = p->last() - 1; }, 6, true},
        {"base low bit", [](Batch& b, const Batch*) { b.hasBaseDamage = true; b.baseDamage = b.base ^ 1; }, 0, false},
        {"offsets and framing", [](Batch& b, const Batch* p) { b.hasBaseDamage = true; b.baseDamage = p->last(); setRaw(b.recs[2].rawKlen, b.recs[2].hasKlen, varint(-2)); }, 6, true},
        {"record 3 offsets, record 7 framing", [](Batch& b, const Batch*) { setRaw(b.recs[3].rawDelta, b.recs[3].hasDelta, varint(2)); setRaw(b.recs[7].rawVlen, b.recs[7].hasVlen, varint(-2)); }, 6, false},
    };
    {
        g_case = "clean";
        const Bytes s = streamOf(builtBatches());
        for (uint32_t size : {4099u, 65536u, (uint32_t)s.size()}) runCase(ctx, s, cut(s.size(), size), TSX_CRC, 0, UINT64_MAX);
    }
    for (const Damage& dm : damage) {
        for (int target = 0; target < 4; target++) {                   // inside a chunk, on a chunk's first byte, the stream's first batch, its last
            std::vector<Batch> bs = builtBatches();
            size_t j = target < 2 ? 6 : target == 2 ? 0 : 13;
            if (j == 0 && dm.needsPrev) j = 1;                          // (the first batch has no batch in front: the check is seen from the second)
            dm.fn(bs[j], j ? &bs[j - 1] : nullptr);
            std::vector<size_t> starts;
            const Bytes s = streamOf(bs, &starts);
            g_case = std::string(dm.name) + " target " + std::to_string(target);
            for (uint32_t size : {4099u, 65536u})
                runCase(ctx, s, cut(s.size(), size, target == 1 ? starts[j] : 0), target == 3 ? 0u : TSX_CRC, dm.why, dm.why ? starts[j] : UINT64_MAX);
        }
    }
    {   // batches that must pass or fail for their header alone; precedence against the CRC
        std::vector<Batch> bs = builtBatches();
        std::vector<size_t> st;
        Bytes s = streamOf(bs, &st);
        g_case = "compressed baseOffset";
        bs[4].hasBaseDamage = true; bs[4].baseDamage = bs[3].last();
        s = streamOf(bs);
        runCase(ctx, s, cut(s.size(), 4099), TSX_CRC, 6, st[4]);
        g_case = "framing in front of crc";
        bs = builtBatches(); bs[5].hasCount = true; bs[5].count = (int32_t)bs[5].recs.size() - 1;
        s = streamOf(bs); Bytes t = s; t[st[8] + 30] ^= 1;
        runCase(ctx, t, cut(t.size(), 4099), TSX_CRC, 5, st[5]);
        g_case = "crc in front of framing";
        t = s; t[st[2] + 30] ^= 1;
        runCase(ctx, t, cut(t.size(), 4099), TSX_CRC, 4, st[2]);
    }
    tsx_ctx_destroy(ctx);
    tsx_shutdown();
    printf("asan records frames: %d runs, %d failed\n", g_runs, g_failed);
    return g_failed ? 1 : 0;
}
