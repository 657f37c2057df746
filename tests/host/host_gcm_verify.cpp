// TEST HARNESS ONLY: the GCM verify-on-upload option of the C++ host layer (tsx::GpuTransformChunkEnumeration / GpuTransformFinisher,
// gcmVerify) over a libtsxform build given on the command line.  That the option reaches the batch is shown by what only a verifying
// batch does: with the library's test switch verify_damage_out_chunk set (one bit of a delivered chunk's tag), the chunk fails with
// TSX_E_VERIFY - and raises what any failed chunk raises - exactly when the option is on; without it the damaged chunk is handed on.
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "tsxhost.hpp"

using namespace tsx;
static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { printf("  FAIL line %d: %s\n", __LINE__, #c); g_failed++; } } while (0)

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: host_gcm_verify <libtsxform path>\n"); return 2; }
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
    DataKeyAndAAD keys;
    keys.dataKey.resize(32); keys.aad.resize(32);
    for (int i = 0; i < 32; i++) { keys.dataKey[i] = (uint8_t)(5 * i + 1); keys.aad[i] = (uint8_t)(99 + i); }
    const int chunk = 40000;
    uint8_t counter = 0;
    const IvSupplier fixedIvs = [&counter](uint8_t iv[12]) { for (int k = 0; k < 12; k++) iv[k] = (uint8_t)(counter + k); counter++; };
    for (bool compress : {false, true}) {
        auto enumeration = [&](bool on, bool readAhead) {
            counter = 0;                                                // the same IVs for every enumeration: the same bytes, option on or off
            auto base = std::make_shared<BaseTransformChunkEnumeration>(std::make_shared<ByteArrayInputStream>(data), chunk);
            return std::make_shared<GpuTransformChunkEnumeration>(be, base, compress, keys, fixedIvs, 3, false, TSX_ZSTD_PROFILE_1_5_7, readAhead, 0, false, false, on);
        };
        Bytes objects[2];
        for (bool on : {false, true}) {
            auto g = enumeration(on, false);
            CHECK(g->gcmVerify() == on && !g->zstdVerify());
            std::vector<Bytes> chunks;
            while (g->hasMoreElements()) chunks.push_back(g->nextElement());
            CHECK(chunks.size() == 3);
            GpuTransformFinisher fin(enumeration(on, false), (int)data.size(), true, nullptr, false);
            CHECK(fin.gcmVerify() == on);
            Bytes object(1 << 20);
            object.resize(fin.fillPart(object.data(), object.size()));
            Bytes want;
            for (const Bytes& f : chunks) want.insert(want.end(), f.begin(), f.end());
            CHECK(object == want);                                     // clean chunks: the same bytes, verified or not
            objects[on ? 1 : 0] = object;
            printf("  %s, gcm verify %s: %zu bytes\n", compress ? "compress + encrypt" : "encrypt", on ? "on" : "off", object.size());
        }
        CHECK(objects[0] == objects[1] && !objects[0].empty());
        // one bit of chunk 1's delivered IV || C || TAG: raised with the option, handed on without it (the hook acts either way)
        config("verify_damage_out_chunk", 1); config("verify_damage_out_off", 20);
        for (bool on : {false, true}) {
            std::string what;
            Bytes object;
            try {
                auto g = enumeration(on, false);
                while (g->hasMoreElements()) { const Bytes c = g->nextElement(); object.insert(object.end(), c.begin(), c.end()); }
            } catch (const std::runtime_error& e) { what = e.what(); }
            CHECK(on ? what == be->strerror(TSX_E_VERIFY) : what.empty());
            if (!on) CHECK(object.size() == objects[0].size() && object != objects[0]);
            what.clear();
            try {
                GpuTransformFinisher fin(enumeration(on, false), (int)data.size(), true, nullptr, false);
                Bytes part(1 << 20);
                fin.fillPart(part.data(), part.size());
            } catch (const std::runtime_error& e) { what = e.what(); }
            CHECK(on ? what == be->strerror(TSX_E_VERIFY) : what.empty());
            printf("  %s, damaged output, gcm verify %s: %s\n", compress ? "compress + encrypt" : "encrypt", on ? "on" : "off", what.empty() ? "no error" : what.c_str());
        }
        config("verify_damage_out_chunk", -1);
    }
    // refused when the chain does not encrypt; accepted with encryption
    for (bool encrypt : {false, true}) {
        bool threw = false;
        try {
            auto base = std::make_shared<BaseTransformChunkEnumeration>(std::make_shared<ByteArrayInputStream>(data), chunk);
            GpuTransformChunkEnumeration g(be, base, true, encrypt ? std::optional<DataKeyAndAAD>(keys) : std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_1_5_7, false, 0,
                                           false, false, true);
        } catch (const std::invalid_argument&) { threw = true; }
        CHECK(threw == !encrypt);
    }
    printf("host gcm verify: %d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
