// TEST HARNESS ONLY: the content checksum option of the C++ host layer (tsx::GpuTransformChunkEnumeration / GpuTransformFinisher,
// zstdChecksum) over a libtsxform build given on the command line.  Reference: the real libzstd the oracle has loaded, opened from the path
// orc_zstd_path() reports and driven as oracle/zstd_ref.c drives it, plus ZSTD_c_checksumFlag.
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "tsxhost.hpp"

extern "C" size_t orc_zstd_compress_chunk(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, int level);   // oracle/zstd_ref.c
extern "C" const char* orc_zstd_path(void);

using namespace tsx;
static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { printf("  FAIL line %d: %s\n", __LINE__, #c); g_failed++; } } while (0)

static Bytes libzstd(const Bytes& b, bool checksum) {
    Bytes out(b.size() + b.size() / 128 + 1024);
    if (!checksum) {
        const size_t r = orc_zstd_compress_chunk(b.data(), b.size(), out.data(), out.size(), 3);
        if (r == (size_t)-1) throw std::runtime_error("oracle compress failed");
        out.resize(r);
        return out;
    }
    static void* h = dlopen(orc_zstd_path(), RTLD_NOW);
    if (!h) throw std::runtime_error("no libzstd");
    auto create = (void* (*)(void))dlsym(h, "ZSTD_createCCtx");
    auto destroy = (size_t (*)(void*))dlsym(h, "ZSTD_freeCCtx");
    auto set = (size_t (*)(void*, int, int))dlsym(h, "ZSTD_CCtx_setParameter");
    auto pledge = (size_t (*)(void*, unsigned long long))dlsym(h, "ZSTD_CCtx_setPledgedSrcSize");
    auto compress2 = (size_t (*)(void*, void*, size_t, const void*, size_t))dlsym(h, "ZSTD_compress2");
    auto isError = (unsigned (*)(size_t))dlsym(h, "ZSTD_isError");
    void* c = create();
    pledge(c, b.size());
    set(c, 200 /* ZSTD_c_contentSizeFlag */, 1); set(c, 100 /* ZSTD_c_compressionLevel */, 3); set(c, 201 /* ZSTD_c_checksumFlag */, 1);
    const size_t r = compress2(c, out.data(), out.size(), b.data(), b.size());
    destroy(c);
    if (isError(r)) throw std::runtime_error("libzstd compress failed");
    out.resize(r);
    return out;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: host_checksum <libtsxform path>\n"); return 2; }
    auto be = std::make_shared<Backend>(argv[1]);
    Bytes data(120000);
    {   // log-like text: words of a small vocabulary picked by an LCG
        static const char* words[] = {"offset=", "key=", "value=", "ts=", "partition ", "topic-a ", "topic-b ", "\n", "1700000", "abc", "xyz", "42 "};
        uint32_t x = 4242; size_t i = 0;
        while (i < data.size()) {
            x = x * 1103515245u + 12345u;
            const char* w = words[(x >> 16) % 12];
            for (size_t k = 0; w[k] && i < data.size(); k++) data[i++] = (uint8_t)w[k];
            if (((x >> 8) & 7) == 0 && i < data.size()) data[i++] = (uint8_t)('0' + ((x >> 20) % 10));
        }
    }
    const int chunk = 40000;
    for (bool on : {false, true}) {
        auto base = std::make_shared<BaseTransformChunkEnumeration>(std::make_shared<ByteArrayInputStream>(data), chunk);
        auto g = std::make_shared<GpuTransformChunkEnumeration>(be, base, true, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_1_5_7, false, 0, on);
        CHECK(g->zstdChecksum() == on);
        size_t off = 0, n = 0;
        while (g->hasMoreElements()) {
            const Bytes f = g->nextElement();
            const Bytes part(data.begin() + (long)off, data.begin() + (long)std::min(off + chunk, data.size()));
            CHECK(f == libzstd(part, on));                             // off: today's bytes; on: bit 2 and libzstd's checksum
            CHECK(f.size() > 8 && ((f[4] >> 2) & 1) == (on ? 1 : 0));
            off += part.size(); n++;
        }
        CHECK(n == 3);
        // the finisher transforms through the enumeration: its object is the frames back to back
        auto base2 = std::make_shared<BaseTransformChunkEnumeration>(std::make_shared<ByteArrayInputStream>(data), chunk);
        auto g2 = std::make_shared<GpuTransformChunkEnumeration>(be, base2, true, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_1_5_7, true, 0, on);
        GpuTransformFinisher fin(g2, (int)data.size());
        CHECK(fin.zstdChecksum() == on);
        Bytes object(1 << 20);
        object.resize(fin.fillPart(object.data(), object.size()));
        Bytes want;
        std::vector<int> sizes;
        for (size_t o = 0; o < data.size(); o += chunk) {
            const Bytes f = libzstd(Bytes(data.begin() + (long)o, data.begin() + (long)std::min(o + chunk, data.size())), on);
            want.insert(want.end(), f.begin(), f.end());
            sizes.push_back((int)f.size());
        }
        CHECK(object == want);
        // the manifest's chunk index frame never carries a checksum, whatever the option says for the chunks
        const Bytes idx = base64Decode(serializeTransformedChunks(*be, sizes));
        CHECK(idx == libzstd(ChunkSizesBinaryCodec::encode(sizes), false));
        CHECK(idx.size() > 5 && (idx[4] & 4) == 0);
        CHECK(deserializeTransformedChunks(*be, base64Encode(idx)) == sizes);
        printf("  checksum %s: %zu bytes\n", on ? "on" : "off", object.size());
    }
    // refused when the chain does not compress; accepted with compression
    for (bool compress : {false, true}) {
        bool threw = false;
        try {
            auto base = std::make_shared<BaseTransformChunkEnumeration>(std::make_shared<ByteArrayInputStream>(data), chunk);
            GpuTransformChunkEnumeration g(be, base, compress, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_1_5_7, false, 0, true);
        } catch (const std::invalid_argument&) { threw = true; }
        CHECK(threw == !compress);
    }
    printf("host checksum: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
