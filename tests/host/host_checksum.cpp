// TEST HARNESS ONLY: the content checksum option of the C++ host layer (tsx::GpuTransformChunkEnumeration / GpuTransformFinisher,
// zstdChecksum) over a libtsxform build given on the command line.  Reference: the real libzstd the oracle has loaded, opened from the path
// orc_zstd_path() reports and driven as oracle/zstd_ref.c drives it, plus ZSTD_c_checksumFlag.
#include "host_check.hpp"

static Bytes libzstd(const Bytes& b, bool checksum) {
    Bytes out(b.size() + b.size() / 128 + 1024);
    const size_t r = checksum ? harness_libzstd_checksummed(b.data(), b.size(), out.data(), out.size(), 3) : orc_zstd_compress_chunk(b.data(), b.size(), out.data(), out.size(), 3);
    if (r == (size_t)-1) throw std::runtime_error(checksum ? "libzstd compress failed" : "oracle compress failed");
    out.resize(r);
    return out;
}

int main(int argc, char** argv) {
    auto be = host_backend(argc, argv, "host_checksum");
    if (!be) return 2;
    const Bytes data = host_log_text(120000, 4242);
    const int chunk = 40000;
    for (bool on : {false, true}) {
        auto g = std::make_shared<GpuTransformChunkEnumeration>(be, host_chunks(data, chunk), true, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_1_5_7, false, 0, on);
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
        auto g2 = std::make_shared<GpuTransformChunkEnumeration>(be, host_chunks(data, chunk), true, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_1_5_7, true, 0, on);
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
    for (bool compress : {false, true})
        CHECK(host_throws<std::invalid_argument>([&] { GpuTransformChunkEnumeration g(be, host_chunks(data, chunk), compress, std::nullopt, secureRandomIvSupplier(), 2, false, TSX_ZSTD_PROFILE_1_5_7, false, 0, true); }) == !compress);
    return host_done("host checksum");
}
