// TEST HARNESS ONLY: streamed record-batch validation in the C++ host layer (tsx::GpuTransformChunkEnumeration / GpuTransformFinisher,
// recordsStreamBytes) over a libtsxform build given on the command line.  host_records.cpp's segment - 109000 bytes in 40000-byte chunks,
// three chunks - in batches of TWO chunks: accepted with streaming, where recordsValidate refuses; the object is
// the one made with the option off, for the plain, the encrypting and the compressing chain, through the enumeration and through the
// finisher with and without read-ahead.  With one bit of the crc field of the batch that crosses from the first batch of chunks into the
// second (the last one, [75961, 109000)) flipped, the first batch is handed on and the second raises TSX_E_RECORDS' text with the position
// and the reason; batch 3, which ends at byte 72961, fails the first; a declared length one byte too long raises the "ended at" error when the source
// is drained; both options together are refused.
#include "host_check.hpp"

int main(int argc, char** argv) {
    auto be = host_backend(argc, argv, "host_records_stream");
    if (!be) return 2;
    Bytes data;
    std::vector<size_t> starts;
    const uint32_t lens[] = {900, 25000, 61, 47000, 3000, 33039};      // 109000 bytes in 40000-byte chunks: batch 3 runs from chunk 0 into chunk 1, batch 5 from chunk 1 into chunk 2
    for (uint32_t i = 0; i < 6; i++) {
        starts.push_back(data.size());
        data.resize(data.size() + lens[i]);
        harness_record_batch(data.data() + starts[i], lens[i], i, "partition topic-a offset=42 value=abc\n", 5);
    }
    CHECK(data.size() == 109000 && starts[3] < 40000 && starts[3] + lens[3] < 80000 && starts[5] < 80000);
    const DataKeyAndAAD keys = host_keys();
    const int chunk = 40000;
    uint8_t counter = 0;
    const IvSupplier fixedIvs = host_counting_ivs(counter);
    const char* const names[3] = {"plain", "encrypt", "compress + encrypt"};
    for (int chain = 0; chain < 3; chain++) {
        auto enumeration = [&](const Bytes& segment, bool validate, int64_t streamBytes, bool readAhead = false) {
            counter = 0;
            return std::make_shared<GpuTransformChunkEnumeration>(be, host_chunks(segment, chunk), chain == 2, chain ? std::optional<DataKeyAndAAD>(keys) : std::nullopt, fixedIvs, 2, false,
                                                                  TSX_ZSTD_PROFILE_1_5_7, readAhead, 0, false, false, false, validate, streamBytes);
        };
        // ---- clean: the old option refuses batches of two, streaming takes them; the object is the one made with the option off ----
        CHECK(host_throws<std::logic_error>([&] { auto g = enumeration(data, true, -1); g->hasMoreElements(); }));
        Bytes want;
        {
            auto g = enumeration(data, false, -1);
            CHECK(g->recordsStreamBytes() == -1 && !g->recordsValidate());
            while (g->hasMoreElements()) { const Bytes c = g->nextElement(); want.insert(want.end(), c.begin(), c.end()); }
        }
        CHECK(!want.empty() && (chain || want == data));
        {
            auto g = enumeration(data, false, (int64_t)data.size());
            CHECK(g->recordsStreamBytes() == (int64_t)data.size() && !g->recordsValidate());
            Bytes got;
            int n = 0;
            while (g->hasMoreElements()) { const Bytes c = g->nextElement(); got.insert(got.end(), c.begin(), c.end()); n++; }
            CHECK(n == 3 && got == want);
        }
        for (bool readAhead : {false, true}) {
            GpuTransformFinisher fin(enumeration(data, false, (int64_t)data.size()), (int)data.size(), true, nullptr, readAhead);
            CHECK(fin.recordsStreamBytes() == (int64_t)data.size());
            Bytes object(1 << 20);
            object.resize(fin.fillPart(object.data(), object.size()));
            CHECK(object == want);
            printf("  %s, streamed in batches of two, finisher read-ahead %s: %zu bytes\n", names[chain], readAhead ? "on" : "off", object.size());
        }
        {
            auto g = enumeration(data, false, (int64_t)data.size(), true);       // the enumeration's own read-ahead
            Bytes got;
            while (g->hasMoreElements()) { const Bytes c = g->nextElement(); got.insert(got.end(), c.begin(), c.end()); }
            CHECK(got == want);
        }
        // ---- the crc field of a batch: batch 3 lies in the first two chunks - nothing is handed on; the last batch begins there and ends in
        // chunk 2 - chunks 0 and 1 are handed on, the verdict falls when the second batch is asked for ----
        for (int which : {3, 5}) {
        Bytes bad = data;
        bad[starts[which] + 19] ^= 1;
        const std::string text = be->strerror(TSX_E_RECORDS) + " (first invalid record batch at stream position " + std::to_string(starts[which]) + ", reason 4 crc)";
        const int handedOn = which == 3 ? 0 : 2;
        {
            std::string what;
            int n = 0;
            try {
                auto g = enumeration(bad, false, (int64_t)bad.size());
                while (g->hasMoreElements()) { g->nextElement(); n++; }
            } catch (const std::runtime_error& e) { what = e.what(); }
            CHECK(n == handedOn && what == text);
            what.clear();
            size_t got = 0;
            try {
                GpuTransformFinisher fin(enumeration(bad, false, (int64_t)bad.size()), (int)bad.size(), true, nullptr, false);
                Bytes part(1 << 20);
                got = fin.readSome(part.data(), part.size());               // the first batch
                fin.readSome(part.data(), part.size());                     // the second
            } catch (const std::runtime_error& e) { what = e.what(); }
            CHECK((got > 0) == (handedOn > 0) && what == text);
            printf("  %s, source damaged in batch %d, streamed: %s\n", names[chain], which, what.c_str());
        }
        }
        // ---- a declared length one byte too long: every chunk passes, the drain says that the stream is not complete ----
        {
            std::string what;
            int n = 0;
            try {
                auto g = enumeration(data, false, (int64_t)data.size() + 1);
                while (g->hasMoreElements()) { g->nextElement(); n++; }
            } catch (const std::logic_error& e) { what = e.what(); }
            CHECK(n == 3 && what.find("ended at 109000 bytes, 109001 were declared") != std::string::npos);
            what.clear();
            try {
                GpuTransformFinisher fin(enumeration(data, false, (int64_t)data.size() + 1), (int)data.size(), true, nullptr, true);
                Bytes part(1 << 20);
                fin.fillPart(part.data(), part.size());
            } catch (const std::logic_error& e) { what = e.what(); }
            CHECK(what.find("ended at 109000 bytes, 109001 were declared") != std::string::npos);
            if (chain == 0) printf("  declared one byte too long: %s\n", what.c_str());
        }
        // ---- both options together ----
        CHECK(host_throws<std::invalid_argument>([&] { enumeration(data, true, (int64_t)data.size()); }));
        CHECK(host_throws<std::invalid_argument>([&] { enumeration(data, false, -2); }));
    }
    return host_done("host records stream");
}
