// adopt_metadata (csrc/host_index.hpp) as a program of its own, built with ASan + UBSan by tests/test_merge_cpu.py: an assembled image
// -- two tags, three path names, two samples, one contig, a graph of three labelled nodes -- moved into the image index_from_records makes
// of a one-record stream; then the same without metadata and without a graph.  Four lines per case for the test to compare; "done" at the end.
#include <cinttypes>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "host_index.hpp"
#include "meta_images.hpp"

static void describe(const char *name, const HostIndex &h) {
    std::printf("%s.tags %s ; %s\n", name, tag_line(h.tags).c_str(), tag_line(h.gbz_tags).c_str());
    std::printf("%s.metadata %d flags %" PRIu64 " counts %" PRIu64 " %" PRIu64 " %" PRIu64 " generic %d paths", name, int(h.has_metadata), h.metadata_flags, h.sample_count,
                h.haplotype_count, h.contig_count, int(h.generic_phase_on_disk));
    for (const PathName &p : h.path_names) std::printf(" %u,%u,%u,%u", p.sample, p.contig, p.phase, p.fragment);
    std::printf(" samples %s contigs %s\n", joined(h.sample_names, '|').c_str(), joined(h.contig_names, '|').c_str());
    std::printf("%s.graph %d translation %d nodes %" PRIu64 " labels %s segments %zu %zu %" PRIu64 "\n", name, int(h.is_gbz), int(h.has_translation), h.graph_nodes,
                joined(h.sequences_labels, '|').c_str(), h.segment_names.size(), h.segment_starts.size(), h.mapping_len);
    std::printf("%s.records %" PRIu64 " sequences %" PRIu64 " alphabet %" PRIu64 " %" PRIu64 " bidirectional %d data %zu starts %zu\n", name, h.size, h.sequences, h.alphabet_offset,
                h.alphabet_size, int(h.bidirectional), h.data.size(), h.starts.size());
}

static HostIndex assembled(bool metadata, bool graph) {
    HostIndex m = with_metadata({"s1", "s2"}, {"chr"}, {{0, 0, 0, 0}, {1, 0, 1, 0}, {1, 0, 2, 7}});
    m.has_metadata = metadata; m.haplotype_count = 3; m.generic_phase_on_disk = false;
    m.tags = {{"source", "x"}, {"reference_samples", "s1"}};
    m.gbz_tags = {{"source", "y"}, {"k", "v"}};
    m.is_gbz = graph; m.graph_nodes = 3; m.sequences_labels = strings({"A", "CC", "GGG"});
    return m;
}

// the image of the endmarker's record of an index without sequences, and what it is once `m` has been adopted
static HostIndex fresh() {
    const uint8_t data[1] = {0};
    const uint64_t starts[1] = {0};
    return index_from_records(data, 1, starts, 1, 21, 28, 0, 0, true);
}
static HostIndex adopted(HostIndex &&m) {
    HostIndex h = fresh();
    adopt_metadata(h, std::move(m));
    return h;
}

int main() {
    describe("fresh", fresh());
    describe("all", adopted(assembled(true, true)));
    describe("no_metadata", adopted(assembled(false, true)));
    describe("no_graph", adopted(assembled(true, false)));
    std::printf("done\n");
    return 0;
}
