// TEST HARNESS ONLY: the record-batch validation option of the C++ host layer (tsx::GpuTransformChunkEnumeration / GpuTransformFinisher,
// recordsValidate) over a libtsxform build given on the command line.  A segment of hand-made v2 record batches through the plain, the
// encrypting and the compressing chain: clean, the object is the same with the option on or off; with one bit of a batch's crc field
// flipped, the option raises what any failed chunk raises (TSX_E_RECORDS' text) and without it the segment is handed on; a segment that
// does not fit one batch is refused with the option on, never validated in part.
#include "host_check.hpp"

int main(int argc, char** argv) {
    auto be = host_backend(argc, argv, "host_records");
    if (!be) return 2;
    Bytes data;
    std::vector<size_t> starts;
    const uint32_t lens[] = {900, 25000, 61, 47000, 3000, 33039};      // 109000 bytes: batch 3 runs from chunk 0 into chunk 2 (40000-byte chunks)
    for (uint32_t i = 0; i < 6; i++) {
        starts.push_back(data.size());
        data.resize(data.size() + lens[i]);
        harness_record_batch(data.data() + starts[i], lens[i], i, "partition topic-a offset=42 value=abc\n", 5);
    }
    CHECK(data.size() == 109000);
    const DataKeyAndAAD keys = host_keys();
    const int chunk = 40000;
    uint8_t counter = 0;
    const IvSupplier fixedIvs = host_counting_ivs(counter);
    const char* const names[3] = {"plain", "encrypt", "compress + encrypt"};
    for (int chain = 0; chain < 3; chain++) {
        auto enumeration = [&](const Bytes& segment, bool on, int batchChunks) {
            counter = 0;
            return std::make_shared<GpuTransformChunkEnumeration>(be, host_chunks(segment, chunk), chain == 2, chain ? std::optional<DataKeyAndAAD>(keys) : std::nullopt, fixedIvs, batchChunks, false,
                                                                  TSX_ZSTD_PROFILE_1_5_7, false, 0, false, false, false, on);
        };
        Bytes objects[2];
        for (bool on : {false, true}) {
            auto g = enumeration(data, on, 3);
            CHECK(g->recordsValidate() == on && !g->gcmVerify());
            Bytes want;
            int n = 0;
            while (g->hasMoreElements()) { const Bytes c = g->nextElement(); want.insert(want.end(), c.begin(), c.end()); n++; }
            CHECK(n == 3);
            GpuTransformFinisher fin(enumeration(data, on, 3), (int)data.size(), true, nullptr, false);
            CHECK(fin.recordsValidate() == on);
            Bytes object(1 << 20);
            object.resize(fin.fillPart(object.data(), object.size()));
            CHECK(object == want && (chain || object == data));
            objects[on ? 1 : 0] = object;
            printf("  %s, records validate %s: %zu bytes\n", names[chain], on ? "on" : "off", object.size());
        }
        CHECK(objects[0] == objects[1] && !objects[0].empty());
        Bytes bad = data;
        bad[starts[3] + 19] ^= 1;                                      // a crc byte of the batch that begins in chunk 0
        for (bool on : {false, true}) {
            std::string what;
            try {
                auto g = enumeration(bad, on, 3);
                while (g->hasMoreElements()) g->nextElement();
            } catch (const std::runtime_error& e) { what = e.what(); }
            CHECK(on ? what == be->strerror(TSX_E_RECORDS) : what.empty());
            what.clear();
            try {
                GpuTransformFinisher fin(enumeration(bad, on, 3), (int)bad.size(), true, nullptr, false);
                Bytes part(1 << 20);
                fin.fillPart(part.data(), part.size());
            } catch (const std::runtime_error& e) { what = e.what(); }
            CHECK(on ? what == be->strerror(TSX_E_RECORDS) : what.empty());
            printf("  %s, damaged source, records validate %s: %s\n", names[chain], on ? "on" : "off", what.empty() ? "no error" : what.c_str());
        }
        // three chunks, batches of two: refused with the option on (before anything is transformed), two batches without it
        for (bool on : {false, true}) {
            std::string what;
            int n = 0;
            try {
                auto g = enumeration(data, on, 2);
                while (g->hasMoreElements()) { g->nextElement(); n++; }
            } catch (const std::logic_error& e) { what = e.what(); }
            CHECK(on ? (n == 0 && what.find("the whole segment must fit one batch") != std::string::npos) : (n == 3 && what.empty()));
            what.clear();
            try {
                GpuTransformFinisher fin(enumeration(data, on, 2), (int)data.size(), true, nullptr, false);
                Bytes part(1 << 20);
                fin.fillPart(part.data(), part.size());
            } catch (const std::logic_error& e) { what = e.what(); }
            CHECK(on ? what.find("the whole segment must fit one batch") != std::string::npos : what.empty());
            if (chain == 0) printf("  segment of three chunks in batches of two, records validate %s: %s\n", on ? "on" : "off", what.empty() ? "no error" : "refused");
        }
    }
    return host_done("host records");
}
