// TEST HARNESS ONLY: the level option of the C++ host layer (tsx::GpuTransformChunkEnumeration / GpuTransformFinisher, zstdLevel) over
// a libtsxform build given on the command line; frames checked with the oracle's libzstd at the same level.
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "tsxhost.hpp"

extern "C" size_t orc_zstd_compress_chunk(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, int level);   // oracle/zstd_ref.c

using namespace tsx;
static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { printf("  FAIL line %d: %s\n", __LINE__, #c); g_failed++; } } while (0)

static Bytes libzstd(const Bytes& b, int level) {
    Bytes out(b.size() + b.size() / 128 + 1024);
    const size_t r = orc_zstd_compress_chunk(b.data(), b.size(), out.data(), out.size(), level);
    if (r == (size_t)-1) throw std::runtime_error("oracle compress failed");
    out.resize(r);
    return out;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: host_levels <libtsxform path>\n"); return 2; }
    auto be = std::make_shared<Backend>(argv[1]);
    Bytes data(120000);
    {   // log-like text: words of a small vocabulary picked by an LCG
        static const char* words[] = {"offset=", "key=", "value=", "ts=", "partition ", "topic-a ", "topic-b ", "\n", "1700000", "abc", "xyz", "42 "};
        uint32_t x = 12345; size_t i = 0;
        while (i < data.size()) {
            x = x * 1103515245u + 12345u;
            const char* w = words[(x >> 16) % 12];
            for (size_t k = 0; w[k] && i < data.size(); k++) data[i++] = (uint8_t)w[k];
            if (((x >> 8) & 7) == 0 && i < data.size()) data[i++] = (uint8_t)('0' + ((x >> 20) % 10));
        }
    }
    const int chunk = 40000;
    for (int level : {0, 1, 2, 3}) {
        auto base = std::make_shared<BaseTransformChunkEnumeration>(std::make_shared<ByteArrayInputStream>(data), chunk);
        auto g = std::make_shared<GpuTransformChunkEnumeration>(be, base, true, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_1_5_7, false, level);
        CHECK(g->zstdLevel() == level);
        size_t off = 0, n = 0;
        while (g->hasMoreElements()) {
            const Bytes f = g->nextElement();
            const Bytes part(data.begin() + (long)off, data.begin() + (long)std::min(off + chunk, data.size()));
            CHECK(f == libzstd(part, level ? level : 3));
            off += part.size(); n++;
        }
        CHECK(n == 3);
        // the finisher transforms through the enumeration: its object is the level's frames back to back
        auto base2 = std::make_shared<BaseTransformChunkEnumeration>(std::make_shared<ByteArrayInputStream>(data), chunk);
        auto g2 = std::make_shared<GpuTransformChunkEnumeration>(be, base2, true, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_1_5_7, false, level);
        GpuTransformFinisher fin(g2, (int)data.size());
        CHECK(fin.zstdLevel() == level);
        Bytes object(1 << 20);
        object.resize(fin.fillPart(object.data(), object.size()));
        Bytes want;
        for (size_t o = 0; o < data.size(); o += chunk) {
            const Bytes f = libzstd(Bytes(data.begin() + (long)o, data.begin() + (long)std::min(o + chunk, data.size())), level ? level : 3);
            want.insert(want.end(), f.begin(), f.end());
        }
        CHECK(object == want);
        if (level == 1) CHECK(object != libzstd(Bytes(data.begin(), data.begin() + chunk), 3));
        printf("  level %d: %zu bytes\n", level, object.size());
    }
    for (int bad : {-1, 4, 19, 22}) {
        bool threw = false;
        try {
            auto base = std::make_shared<BaseTransformChunkEnumeration>(std::make_shared<ByteArrayInputStream>(data), chunk);
            GpuTransformChunkEnumeration g(be, base, true, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_1_5_7, false, bad);
        } catch (const std::invalid_argument&) { threw = true; }
        CHECK(threw);
    }
    printf("host levels: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
