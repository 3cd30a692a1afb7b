// The host's part of a removal (csrc/remove_meta.hpp) as a program of its own, built with ASan + UBSan by tests/test_remove_cpu.py: the
// check of the path ids, name dropping and remapping, the haplotype count, the trimming of reference_samples, the labels of the nodes
// that are no longer visited, and the translation refusal.  One line per case for the test to compare; "done" at the end.
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

#include "meta_images.hpp"
#include "remove_meta.hpp"

static void print_metadata(const char *name, const HostIndex &m) {
    std::printf("%s_samples %s\n%s_contigs %s\n%s_paths", name, joined(m.sample_names).c_str(), name, joined(m.contig_names).c_str(), name);
    for (const PathName &p : m.path_names) std::printf(" %u,%u,%u,%u", p.sample, p.contig, p.phase, p.fragment);
    std::printf("\n%s_counts %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", name, m.sample_count, m.haplotype_count, m.contig_count, m.metadata_flags);
}

int main() {
    // the path ids
    std::string what;
    const uint64_t good[] = {4, 0, 2}, high[] = {1, 6, 9}, twice[] = {3, 1, 3};
    std::printf("ids_good %d\n", remove_check_ids(good, 3, 5, what) ? 1 : 0);
    const bool high_ok = remove_check_ids(high, 3, 6, what);
    std::printf("ids_high %d %s\n", high_ok ? 1 : 0, what.c_str());
    const bool twice_ok = remove_check_ids(twice, 3, 6, what);
    std::printf("ids_twice %d %s\n", twice_ok ? 1 : 0, what.c_str());
    std::printf("ids_none %d\n", remove_check_ids(nullptr, 0, 0, what) ? 1 : 0);

    // samples _gbwt_ref, s1, s2, s3; contigs chrA, chrB, chrC; s2 lives on path 3 alone, chrB on paths 2 and 3, chrC on path 5
    const HostIndex a = with_metadata({"_gbwt_ref", "s1", "s2", "s3"}, {"chrA", "chrB", "chrC"},
                                      {{0, 0, 0, 0}, {1, 0, 1, 0}, {1, 1, 2, 5}, {2, 1, 1, 0}, {3, 0, 1, 0}, {3, 2, 1, 0}});
    HostIndex m;
    MergeRefusal bad = remove_metadata(a, {0, 0, 1, 1, 0, 0}, m);           // paths 2 and 3 go: s2 and chrB with them
    if (bad) { std::printf("FAIL refused: %s\n", bad.what.c_str()); return 1; }
    print_metadata("some", m);
    HostIndex none;
    bad = remove_metadata(a, {0, 0, 0, 0, 0, 0}, none);
    if (bad) { std::printf("FAIL refused: %s\n", bad.what.c_str()); return 1; }
    print_metadata("nothing", none);
    HostIndex all;
    bad = remove_metadata(a, {1, 1, 1, 1, 1, 1}, all);
    if (bad) { std::printf("FAIL refused: %s\n", bad.what.c_str()); return 1; }
    print_metadata("all", all);

    HostIndex bare, o1, o2;
    bare.bidirectional = true; bare.sequences = 2;
    const MergeRefusal without = remove_metadata(bare, {1}, o1);
    std::printf("without %s%s\n", kind(without), o1.has_metadata ? " with metadata" : "");
    HostIndex partial = with_metadata({"s"}, {"c"}, {{0, 0, 0, 0}});
    partial.metadata_flags = 5;                                  // no sample names
    const MergeRefusal incomplete = remove_metadata(partial, {0}, o2);
    std::printf("incomplete %s %s\n", kind(incomplete), incomplete.what.c_str());

    // reference_samples: s2 is no longer a sample; "elsewhere" never was one and stays
    const TagList tags = {{"source", "x"}, {"reference_samples", "s1 s2 elsewhere"}, {"k", "v"}};
    std::printf("tags %s\n", tag_line(remove_tags(tags, a.sample_names, m.sample_names)).c_str());
    std::printf("tags_gone %s\n", tag_line(remove_tags({{"reference_samples", "s2"}, {"k", "v"}}, a.sample_names, m.sample_names)).c_str());
    std::printf("tags_plain %s\n", tag_line(remove_tags({{"source", "x"}}, a.sample_names, m.sample_names)).c_str());

    // graph: the input holds nodes 10 .. 13 (alphabet 20 .. 27); the result keeps 11 .. 13 (offset 21, size 28) and nobody visits 12: its
    // records are the one byte 0.  Records: endmarker, 22, 23, 24, 25, 26, 27.
    HostIndex g, r, out;
    g.is_gbz = true; g.alphabet_offset = 19; g.alphabet_size = 28; g.sequences_labels = strings({"ACG", "C", "T", "GG"});
    r.alphabet_offset = 21; r.alphabet_size = 28;
    const uint8_t bytes[] = {1, 0, 0, 0,  1, 0, 0, 0,  1, 0, 0, 0,  0,  0,  1, 0, 0, 0,  1, 0, 0, 0};
    r.data.assign(bytes, bytes + sizeof(bytes));
    r.starts = {0, 4, 8, 12, 13, 14, 18, 22};
    bad = remove_graph(g, r, out);
    std::printf("labels %" PRIu64 " %s%s\n", out.graph_nodes, joined(out.sequences_labels, '|').c_str(), bad ? " refused" : "");
    HostIndex empty, out2;
    empty.alphabet_offset = 0; empty.alphabet_size = 1; empty.data.assign(1, 0); empty.starts = {0, 1};
    bad = remove_graph(g, empty, out2);
    std::printf("labels_none %" PRIu64 " %zu%s\n", out2.graph_nodes, out2.sequences_labels.size(), bad ? " refused" : "");
    g.has_translation = true;
    const MergeRefusal translated = remove_graph(g, r, out);
    std::printf("translation %s %s\n", kind(translated), translated.what.find("translation") != std::string::npos ? "named" : "unnamed");
    std::printf("done\n");
    return 0;
}
