// TEST HARNESS ONLY: the verify-on-upload option of the C++ host layer (tsx::GpuTransformChunkEnumeration / GpuTransformFinisher,
// zstdVerify) over a libtsxform build given on the command line.  That the option reaches the batch is shown by what only a verifying
// batch does: with the library's test switch verify_damage_src_chunk set, a chunk fails with TSX_E_VERIFY - and raises what any failed
// chunk raises - exactly when the option is on.
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "tsxhost.hpp"

using namespace tsx;
static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { printf("  FAIL line %d: %s\n", __LINE__, #c); g_failed++; } } while (0)

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: host_verify <libtsxform path>\n"); return 2; }
    auto be = std::make_shared<Backend>(argv[1]);
    void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);                   // (the library the backend has loaded: same handle)
    auto config = h ? (long long (*)(const char*, long long))dlsym(h, "tsx_debug_config") : nullptr;
    if (!config) { printf("no tsx_debug_config in %s\n", argv[1]); return 2; }
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
    auto enumeration = [&](bool on, bool readAhead) {
        auto base = std::make_shared<BaseTransformChunkEnumeration>(std::make_shared<ByteArrayInputStream>(data), chunk);
        return std::make_shared<GpuTransformChunkEnumeration>(be, base, true, std::nullopt, secureRandomIvSupplier(), 3, false, TSX_ZSTD_PROFILE_1_5_7, readAhead, 0, true, on);
    };
    Bytes objects[2];
    for (bool on : {false, true}) {
        auto g = enumeration(on, false);
        CHECK(g->zstdVerify() == on && g->zstdChecksum());
        std::vector<Bytes> frames;
        while (g->hasMoreElements()) frames.push_back(g->nextElement());
        CHECK(frames.size() == 3);
        GpuTransformFinisher fin(enumeration(on, true), (int)data.size());
        CHECK(fin.zstdVerify() == on);
        Bytes object(1 << 20);
        object.resize(fin.fillPart(object.data(), object.size()));
        Bytes want;
        for (const Bytes& f : frames) want.insert(want.end(), f.begin(), f.end());
        CHECK(object == want);                                         // clean chunks: the same frames, verified or not
        objects[on ? 1 : 0] = object;
        printf("  verify %s: %zu bytes\n", on ? "on" : "off", object.size());
    }
    CHECK(objects[0] == objects[1] && !objects[0].empty());
    // a chunk whose frame does not restore it: raised with the option, unnoticed without it (the switch only acts inside a verifying batch)
    config("verify_damage_src_chunk", 1); config("verify_damage_src_off", 777);
    for (bool on : {false, true}) {
        std::string what;
        try {
            auto g = enumeration(on, false);
            while (g->hasMoreElements()) g->nextElement();
        } catch (const std::runtime_error& e) { what = e.what(); }
        CHECK(on ? what == be->strerror(TSX_E_VERIFY) : what.empty());
        what.clear();
        try {
            GpuTransformFinisher fin(enumeration(on, false), (int)data.size());
            Bytes object(1 << 20);
            fin.fillPart(object.data(), object.size());
        } catch (const std::runtime_error& e) { what = e.what(); }
        CHECK(on ? what == be->strerror(TSX_E_VERIFY) : what.empty());
        printf("  damaged source, verify %s: %s\n", on ? "on" : "off", what.empty() ? "no error" : what.c_str());
    }
    config("verify_damage_src_chunk", -1);
    CHECK(be->strerror(TSX_E_VERIFY).find("does not restore") != std::string::npos);
    // refused when the chain does not compress; accepted with compression
    for (bool compress : {false, true}) {
        bool threw = false;
        try {
            auto base = std::make_shared<BaseTransformChunkEnumeration>(std::make_shared<ByteArrayInputStream>(data), chunk);
            GpuTransformChunkEnumeration g(be, base, compress, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_1_5_7, false, 0, false, true);
        } catch (const std::invalid_argument&) { threw = true; }
        CHECK(threw == !compress);
    }
    printf("host verify: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
