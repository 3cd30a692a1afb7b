// lazy_records.cpp -- the lazy-build contract of the host's record image (gbwt_rs_amd/csrc/host_index.cpp: HostIndex::ensure_records)
// under AddressSanitizer + UBSan: a build that throws marks nothing, and every caller -- a later one, or two at the same time -- gets the
// same InvalidData.  The file is one whose record starts only the lazy decode rejects: its Elias-Fano words are well formed, but the last
// starts lie past the record bytes (an open that decodes the starts on the device and leaves the host's image for later accepts it).
// Built and run by tests/test_capi_cpu.py::test_lazy_records_under_sanitizers (CPU only).
// usage: lazy_records SCRATCH_FILE
#include "host_index.hpp"
#include <cstdio>
#include <thread>

using namespace gbwt_hip;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static bool rejected(const HostIndex &h) {
    try { h.ensure_records(); } catch (const InvalidData &) { return true; } catch (...) { return false; }
    return false;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    // 4.5 MB of record bytes (a load takes the lazy path from 4 MB) in 1 024 records; the last four start one byte past the data
    HostIndex w;
    w.sequences = 1; w.size = 1; w.alphabet_offset = 0; w.alphabet_size = 2;
    const uint64_t records = 1024, len = uint64_t(4608) << 10;
    w.data.assign(len, 0);
    for (uint64_t k = 0; k < records; k++) w.starts.push_back(k < records - 4 ? k * (len / records) : len + 1);
    w.starts.push_back(len);
    save_index_file(w, argv[1], false);
    bool eager_rejects = false;         // (the load that decodes the starts on the host at once rejects the file)
    try { load_index_file(argv[1]); } catch (const InvalidData &) { eager_rejects = true; }
    CHECK(eager_rejects);

    HostIndex h;
    load_index_file_into(argv[1], h, true, [](HostIndex &x) { x.starts_on_device = true; }, true);
    CHECK(h.lazy_records != nullptr);
    bool finished = true;
    try { h.finish(); } catch (...) { finished = false; }
    CHECK(finished);
    CHECK(!h.records_made());
    CHECK(rejected(h));
    CHECK(rejected(h));                 // the failed build marked nothing: the second caller builds again and fails the same way
    bool first = false, second = false;
    std::thread a([&] { first = rejected(h); }), b([&] { second = rejected(h); });
    a.join();
    b.join();
    CHECK(first && second);
    CHECK(!h.records_made());
    std::printf("%s\n", failures ? "FAILED" : "lazy records ok");
    return failures ? 1 : 0;
}
