// TEST HARNESS ONLY: the verify-on-upload option of the C++ host layer (tsx::GpuTransformChunkEnumeration / GpuTransformFinisher,
// zstdVerify) over a libtsxform build given on the command line.  That the option reaches the batch is shown by what only a verifying
// batch does: with the library's test switch verify_damage_src_chunk set, a chunk fails with TSX_E_VERIFY - and raises what any failed
// chunk raises - exactly when the option is on.
#include "host_check.hpp"

int main(int argc, char** argv) {
    auto be = host_backend(argc, argv, "host_verify");
    if (!be) return 2;
    auto config = host_debug_config(argv[1]);
    if (!config) return 2;
    const Bytes data = host_log_text(120000, 4242);
    const int chunk = 40000;
    auto enumeration = [&](bool on, bool readAhead) {
        return std::make_shared<GpuTransformChunkEnumeration>(be, host_chunks(data, chunk), true, std::nullopt, secureRandomIvSupplier(), 3, false, TSX_ZSTD_PROFILE_1_5_7, readAhead, 0, true, on);
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
    for (bool compress : {false, true})
        CHECK(host_throws<std::invalid_argument>([&] { GpuTransformChunkEnumeration g(be, host_chunks(data, chunk), compress, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_1_5_7, false, 0, false, true); }) == !compress);
    return host_done("host verify");
}
