// TEST HARNESS ONLY: the level option of the C++ host layer (tsx::GpuTransformChunkEnumeration / GpuTransformFinisher, zstdLevel) over
// a libtsxform build given on the command line; frames checked with the oracle's libzstd at the same level.
#include "host_check.hpp"

static Bytes libzstd(const Bytes& b, int level) {
    Bytes out(b.size() + b.size() / 128 + 1024);
    const size_t r = orc_zstd_compress_chunk(b.data(), b.size(), out.data(), out.size(), level);
    if (r == (size_t)-1) throw std::runtime_error("oracle compress failed");
    out.resize(r);
    return out;
}

int main(int argc, char** argv) {
    auto be = host_backend(argc, argv, "host_levels");
    if (!be) return 2;
    const Bytes data = host_log_text(120000, 12345);
    const int chunk = 40000;
    for (int level : {0, 1, 2, 3}) {
        auto g = std::make_shared<GpuTransformChunkEnumeration>(be, host_chunks(data, chunk), true, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_1_5_7, false, level);
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
        auto g2 = std::make_shared<GpuTransformChunkEnumeration>(be, host_chunks(data, chunk), true, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_1_5_7, false, level);
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
    for (int bad : {-1, 4, 19, 22})
        CHECK(host_throws<std::invalid_argument>([&] { GpuTransformChunkEnumeration g(be, host_chunks(data, chunk), true, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_1_5_7, false, bad); }));
    return host_done("host levels");
}
