// TEST HARNESS ONLY: the GCM verify-on-upload option of the C++ host layer (tsx::GpuTransformChunkEnumeration / GpuTransformFinisher,
// gcmVerify) over a libtsxform build given on the command line.  That the option reaches the batch is shown by what only a verifying
// batch does: with the library's test switch verify_damage_out_chunk set (one bit of a delivered chunk's tag), the chunk fails with
// TSX_E_VERIFY - and raises what any failed chunk raises - exactly when the option is on; without it the damaged chunk is handed on.
#include "host_check.hpp"

int main(int argc, char** argv) {
    auto be = host_backend(argc, argv, "host_gcm_verify");
    if (!be) return 2;
    auto config = host_debug_config(argv[1]);
    if (!config) return 2;
    const Bytes data = host_log_text(120000, 4242);
    const DataKeyAndAAD keys = host_keys();
    const int chunk = 40000;
    uint8_t counter = 0;
    const IvSupplier fixedIvs = host_counting_ivs(counter);
    for (bool compress : {false, true}) {
        auto enumeration = [&](bool on, bool readAhead) {
            counter = 0;
            return std::make_shared<GpuTransformChunkEnumeration>(be, host_chunks(data, chunk), compress, keys, fixedIvs, 3, false, TSX_ZSTD_PROFILE_1_5_7, readAhead, 0, false, false, on);
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
    for (bool encrypt : {false, true})
        CHECK(host_throws<std::invalid_argument>([&] {
            GpuTransformChunkEnumeration g(be, host_chunks(data, chunk), true, encrypt ? std::optional<DataKeyAndAAD>(keys) : std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_1_5_7, false, 0,
                                           false, false, true);
        }) == !encrypt);
    return host_done("host gcm verify");
}
