// TEST HARNESS ONLY: the record-framing option of the C++ host layer (tsx::GpuTransformChunkEnumeration / GpuTransformFinisher,
// recordsFrames) over a libtsxform build given on the command line.  A segment of well-framed v2 record batches through the plain, the
// encrypting and the compressing chain: clean, the object is the same with the option on or off; with one batch's recordsCount raised by
// one and the batch sealed with a fresh CRC, the option raises what any failed chunk raises (TSX_E_RECORDS' text) and recordsValidate alone
// hands the segment on; the option without recordsValidate, or with the streamed form, is refused at construction.
#include "host_check.hpp"
#include "../records_frames_harness.h"

int main(int argc, char** argv) {
    auto be = host_backend(argc, argv, "host_records_frames");
    if (!be) return 2;
    Bytes data(200000);
    std::vector<size_t> starts;
    const uint32_t nrec[] = {3, 40, 1, 60, 20}, vlen[] = {200, 700, 5, 900, 800};
    size_t total = 0;
    for (uint32_t i = 0; i < 5; i++) { starts.push_back(total); total += frames_batch(data.data() + total, 100 * i, nrec[i], vlen[i], "partition topic-a offset=42 value=abc\n"); }
    starts.push_back(total);
    data.resize(total);
    const int chunk = 40000;
    CHECK(total > 80001 && total <= 120000 && starts[3] < 40000 && starts[4] > 80000);
    const DataKeyAndAAD keys = host_keys();
    uint8_t counter = 0;
    const IvSupplier fixedIvs = host_counting_ivs(counter);
    const char* const names[3] = {"plain", "encrypt", "compress + encrypt"};
    for (int chain = 0; chain < 3; chain++) {
        auto enumeration = [&](const Bytes& segment, bool validate, int64_t streamed, bool frames) {
            counter = 0;
            return std::make_shared<GpuTransformChunkEnumeration>(be, host_chunks(segment, chunk), chain == 2, chain ? std::optional<DataKeyAndAAD>(keys) : std::nullopt, fixedIvs, 3, false,
                                                                  TSX_ZSTD_PROFILE_1_5_7, false, 0, false, false, false, validate, streamed, frames);
        };
        Bytes objects[2];
        for (bool on : {false, true}) {
            auto g = enumeration(data, true, -1, on);
            CHECK(g->recordsValidate() && g->recordsFrames() == on);
            Bytes want;
            int n = 0;
            while (g->hasMoreElements()) { const Bytes c = g->nextElement(); want.insert(want.end(), c.begin(), c.end()); n++; }
            CHECK(n == 3);
            GpuTransformFinisher fin(enumeration(data, true, -1, on), (int)data.size(), true, nullptr, false);
            CHECK(fin.recordsFrames() == on);
            Bytes object(1 << 20);
            object.resize(fin.fillPart(object.data(), object.size()));
            CHECK(object == want && (chain || object == data));
            objects[on ? 1 : 0] = object;
            printf("  %s, records frames %s: %zu bytes\n", names[chain], on ? "on" : "off", object.size());
        }
        CHECK(objects[0] == objects[1] && !objects[0].empty());
        Bytes bad = data;
        harness_be32(bad.data() + starts[3] + 57, nrec[3] + 1);        // one record more than the batch holds ...
        frames_seal(bad.data() + starts[3], (uint32_t)(starts[4] - starts[3]));      // ... under a valid CRC
        for (bool on : {false, true}) {
            std::string what;
            try {
                auto g = enumeration(bad, true, -1, on);
                while (g->hasMoreElements()) g->nextElement();
            } catch (const std::runtime_error& e) { what = e.what(); }
            CHECK(on ? what == be->strerror(TSX_E_RECORDS) : what.empty());
            what.clear();
            try {
                GpuTransformFinisher fin(enumeration(bad, true, -1, on), (int)bad.size(), true, nullptr, false);
                Bytes part(1 << 20);
                fin.fillPart(part.data(), part.size());
            } catch (const std::runtime_error& e) { what = e.what(); }
            CHECK(on ? what == be->strerror(TSX_E_RECORDS) : what.empty());
            printf("  %s, sealed damage, records frames %s: %s\n", names[chain], on ? "on" : "off", what.empty() ? "no error" : what.c_str());
        }
        for (int streamed = 0; streamed <= 1; streamed++) {
            std::string what;
            try { enumeration(data, streamed != 0, streamed ? (int64_t)data.size() : -1, true); } catch (const std::invalid_argument& e) { what = e.what(); }
            CHECK(what.find("segment.records.validate.frames needs segment.records.validate") != std::string::npos);
            if (chain == 0) printf("  records frames %s: %s\n", streamed ? "with the streamed form" : "without records validate", what.empty() ? "no error" : "refused");
        }
    }
    return host_done("host records frames");
}
