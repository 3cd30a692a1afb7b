// The host's part of a merge (csrc/merge_meta.hpp) as a program of its own, built with ASan + UBSan by tests/test_merge_cpu.py: name
// unions, remapping, the duplicate-path refusal, the haplotype count, the tag and reference_samples rules, the one-sided-metadata refusal
// and the union of the node labels.  One line per case for the test to compare; "done" at the end.
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

#include "meta_images.hpp"
#include "merge_meta.hpp"

int main() {
    // a: samples _gbwt_ref, s1; contigs chrA, chrB.  b: samples s2, s1, s3; contigs chrB, chrC, chrA.
    const HostIndex a = with_metadata({"_gbwt_ref", "s1"}, {"chrA", "chrB"}, {{0, 0, 0, 0}, {1, 0, 1, 0}, {1, 1, 2, 5}});
    const HostIndex b = with_metadata({"s2", "s1", "s3"}, {"chrB", "chrC", "chrA"}, {{0, 0, 1, 0}, {2, 1, 1, 0}, {1, 2, 2, 0}});
    HostIndex m;
    MergeRefusal bad = merge_metadata(a, b, m);
    if (bad) { std::printf("FAIL refused: %s\n", bad.what.c_str()); return 1; }
    std::printf("samples %s\ncontigs %s\npaths", joined(m.sample_names).c_str(), joined(m.contig_names).c_str());
    for (const PathName &p : m.path_names) std::printf(" %u,%u,%u,%u", p.sample, p.contig, p.phase, p.fragment);
    std::printf("\ncounts %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", m.sample_count, m.haplotype_count, m.contig_count, m.metadata_flags);

    // path 1 of b2 is (s1, chrA, 1, 0) after remapping: a's path 1
    const HostIndex b2 = with_metadata({"s2", "s1"}, {"chrC", "chrA"}, {{0, 0, 1, 0}, {1, 1, 1, 0}});
    HostIndex d;
    bad = merge_metadata(a, b2, d);
    std::printf("duplicate %s %s\n", kind(bad), bad.what.substr(0, 11).c_str());

    HostIndex bare;
    bare.bidirectional = true; bare.sequences = 2;
    HostIndex o1, o2, o3, o4;
    std::printf("one_sided %s %s\n", kind(merge_metadata(a, bare, o1)), kind(merge_metadata(bare, a, o2)));
    HostIndex partial = with_metadata({"s"}, {"c"}, {{0, 0, 0, 0}});
    partial.metadata_flags = 5;                                  // no sample names
    std::printf("incomplete %s\n", kind(merge_metadata(a, partial, o3)));
    const MergeRefusal neither = merge_metadata(bare, bare, o4);
    std::printf("neither %s%s\n", kind(neither), o4.has_metadata ? " with metadata" : "");

    const TagList ta = {{"source", "x"}, {"reference_samples", "r1 r2"}, {"k", "a"}}, tb = {{"k", "b"}, {"reference_samples", "r2 r3"}, {"only_b", "q"}};
    std::printf("tags %s\n", tag_line(merge_tags(ta, tb)).c_str());
    std::printf("rs_only_b %s\n", tag_line(merge_tags({{"source", "x"}}, {{"source", "y"}, {"reference_samples", "r9"}})).c_str());
    std::printf("rs_absent %s\n", tag_line(merge_tags({{"source", "x"}}, {{"source", "y"}})).c_str());

    // graphs: a holds nodes 11 .. 12 (alphabet 22 .. 25), b nodes 10 .. 13 with 11 unlabelled; the union is 10 .. 13
    HostIndex ga, gb;
    ga.is_gbz = gb.is_gbz = true;
    ga.alphabet_offset = 21; ga.alphabet_size = 26; ga.sequences_labels = strings({"", "T"});
    gb.alphabet_offset = 19; gb.alphabet_size = 28; gb.sequences_labels = strings({"ACG", "", "T", "GG"});
    HostIndex g;
    bad = merge_graph(ga, gb, 19, 28, g);
    std::string labels;
    for (size_t i = 0; i < g.sequences_labels.size(); i++) { if (i) labels += '|'; labels += g.sequences_labels.str(i); }
    std::printf("labels %" PRIu64 " %s%s\n", g.graph_nodes, labels.c_str(), bad ? " refused" : "");
    ga.sequences_labels = strings({"", "A"});
    bad = merge_graph(ga, gb, 19, 28, g);
    std::printf("conflict %s %s\n", kind(bad), bad.what.substr(0, 7).c_str());
    gb.has_translation = true;
    std::printf("translation %s\n", kind(merge_graph(ga, gb, 19, 28, g)));
    std::printf("done\n");
    return 0;
}
