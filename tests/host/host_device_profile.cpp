// TEST HARNESS ONLY: TSX_ZSTD_PROFILE_DEVICE through the C++ host layer (tsx::GpuTransformChunkEnumeration / GpuTransformFinisher) over a
// libtsxform build given on the command line.  The profile's frames are no library's bytes: the enumeration's and the finisher's are
// compared with the synchronous path's (tsx_transform_batch through the Backend, one chunk per call), and the oracle's libzstd restores
// every chunk from its frame.  A level together with the profile, and an unknown profile, are refused at construction.
#include "host_check.hpp"

static Bytes libzstdRestores(const Bytes& frame, size_t n) {
    Bytes out(n + 16);
    const long long r = orc_zstd_decompress_chunk(frame.data(), frame.size(), out.data(), n);
    if (r < 0) throw std::runtime_error("oracle decompress failed");
    out.resize((size_t)r);
    return out;
}

// the synchronous path: one chunk, one tsx_transform_batch
static Bytes syncFrame(Backend& be, const Bytes& part) {
    std::vector<tsx_chunk_desc> d(1);
    memset(d.data(), 0, sizeof(tsx_chunk_desc));
    d[0].src_len = (uint32_t)part.size(); d[0].dst_cap = (uint32_t)be.transformedBound(part.size(), TSX_COMPRESS);
    Bytes src(((part.size() + 15) & ~(size_t)15) + 16), dst((((size_t)d[0].dst_cap + 15) & ~(size_t)15) + 16);
    memcpy(src.data(), part.data(), part.size());
    tsx_batch_params p; memset(&p, 0, sizeof p);
    p.flags = TSX_COMPRESS; p.zstd_profile = TSX_ZSTD_PROFILE_DEVICE;
    be.transformBatch(p, d, src.data(), src.size(), dst.data(), dst.size());
    if (d[0].status != TSX_OK) throw std::runtime_error("synchronous transform failed");
    dst.resize(d[0].dst_len);
    return dst;
}

int main(int argc, char** argv) {
    auto be = host_backend(argc, argv, "host_device_profile");
    if (!be) return 2;
    const Bytes data = host_log_text(300000, 4321);
    const int chunk = 140000;                                           // two blocks per chunk; 3 chunks, the last one short
    Bytes want;
    size_t level3 = 0;
    for (bool readAhead : {false, true}) {
        auto g = std::make_shared<GpuTransformChunkEnumeration>(be, host_chunks(data, chunk), true, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_DEVICE, readAhead, 0);
        CHECK(g->zstdProfile() == TSX_ZSTD_PROFILE_DEVICE && g->zstdLevel() == 0);
        size_t off = 0, n = 0;
        Bytes all;
        while (g->hasMoreElements()) {
            const Bytes f = g->nextElement();
            const Bytes part(data.begin() + (long)off, data.begin() + (long)std::min(off + chunk, data.size()));
            CHECK(f == syncFrame(*be, part));
            CHECK(libzstdRestores(f, part.size()) == part);
            if (!readAhead) { Bytes l3(part.size() + 1024); const size_t r = orc_zstd_compress_chunk(part.data(), part.size(), l3.data(), l3.size(), 3); CHECK(r != f.size() || memcmp(l3.data(), f.data(), r) != 0); level3 += r; }
            all.insert(all.end(), f.begin(), f.end());
            off += part.size(); n++;
        }
        CHECK(n == 3);
        if (!readAhead) want = all; else CHECK(all == want);
    }
    {   // the finisher transforms through the enumeration: its object is the profile's frames back to back; verify on upload accepts them
        auto g = std::make_shared<GpuTransformChunkEnumeration>(be, host_chunks(data, chunk), true, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_DEVICE, false, 0, false, true);
        GpuTransformFinisher fin(g, (int)data.size());
        CHECK(fin.zstdProfile() == TSX_ZSTD_PROFILE_DEVICE);
        Bytes object(1 << 20);
        object.resize(fin.fillPart(object.data(), object.size()));
        CHECK(object == want);
        printf("  device profile: %zu bytes (level 3: %zu, original %zu)\n", object.size(), level3, data.size());
    }
    {   // ... and so does the plain TransformFinisher over the enumeration
        auto g = std::make_shared<GpuTransformChunkEnumeration>(be, host_chunks(data, chunk), true, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_DEVICE, false, 0);
        TransformFinisher fin(g, (int)data.size());
        Bytes object;
        while (fin.hasMoreElements()) { const Bytes part = fin.nextElement(); object.insert(object.end(), part.begin(), part.end()); }
        CHECK(object == want);
    }
    for (int level : {1, 2, 3})
        CHECK(host_throws<std::invalid_argument>([&] { GpuTransformChunkEnumeration g(be, host_chunks(data, chunk), true, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_DEVICE, false, level); }));
    CHECK(host_throws<std::invalid_argument>([&] { GpuTransformChunkEnumeration g(be, host_chunks(data, chunk), true, std::nullopt, secureRandomIvSupplier(), 2, false, 3u, false, 0); }));
    return host_done("host device profile");
}
