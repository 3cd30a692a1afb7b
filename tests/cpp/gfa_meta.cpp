// The host's part of a construction from GFA (csrc/gfa_meta.hpp) as a program of its own, built with ASan + UBSan by
// tests/test_gfa_build_cpu.py: the name fields of a GFA file's P- and W-lines (argv[1]; the test passes tests/golden/example.gfa) go
// through the metadata assembly, and the result is printed for the test to compare:
//   counts <samples> <haplotypes> <contigs> <flags> <paths>
//   path <sample> <contig> <phase> <fragment>          (one per path, in path order; phase as it is held in memory)
//   samples <name> ...      contigs <name> ...
//   rs <value of RS:Z: of "H\tVN:Z:1.1\tRS:Z:a b">
//   star <fragment of a W-line whose start is "*">
//   duplicate <1-based line reported for two equal W names on lines 3 and 5>
//   hap <1-based line reported for a non-numeric haplotype on line 7, with a duplicate on line 9>
//   counts_host <lines> <segments> <links> <p_lines> <w_lines> <steps> <label_bytes>
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

#include "gfa_meta.hpp"

using namespace gbwt_hip;

// the path lines of a text, found the slow way: P-lines, then W-lines
static std::vector<GfaPathLine> path_lines(const std::string &text) {
    std::vector<GfaPathLine> p, w;
    uint64_t at = 0, line = 0;
    while (at < text.size()) {
        uint64_t end = text.find('\n', at);
        if (end == std::string::npos) end = text.size();
        if (end > at && (text[at] == 'P' || text[at] == 'W')) {
            GfaPathLine x;
            x.line = line; x.walk = text[at] == 'W';
            uint32_t k = 0;
            for (uint64_t i = at; i < end && k < (x.walk ? 6u : 2u); i++) if (text[i] == '\t') x.tab[k++] = i;
            (x.walk ? w : p).push_back(x);
        }
        at = end + 1; line++;
    }
    p.insert(p.end(), w.begin(), w.end());
    return p;
}

static GfaMetaRefusal assemble(const std::string &text, HostIndex &h, uint64_t stop = ~uint64_t(0)) {
    std::vector<GfaPathFields> fields;
    for (const GfaPathLine &p : path_lines(text)) fields.push_back(gfa_path_fields(text.data(), p));
    return assemble_gfa_metadata(fields, stop, h);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const GfaFile file(argv[1]);
    const std::string text(file.data(), file.size());
    HostIndex h;
    const GfaMetaRefusal bad = assemble(text, h);
    if (bad) { std::printf("FAIL refused line %" PRIu64 ": %s\n", bad.line, bad.what.c_str()); return 1; }
    std::printf("counts %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %zu\n", h.sample_count, h.haplotype_count, h.contig_count, h.metadata_flags, h.path_names.size());
    for (const PathName &p : h.path_names) std::printf("path %u %u %u %u\n", p.sample, p.contig, p.phase, p.fragment);
    std::printf("samples");
    for (size_t i = 0; i < h.sample_names.size(); i++) std::printf(" %s", h.sample_names.str(i).c_str());
    std::printf("\ncontigs");
    for (size_t i = 0; i < h.contig_names.size(); i++) std::printf(" %s", h.contig_names.str(i).c_str());
    std::printf("\ngeneric_on_disk %d\n", h.generic_phase_on_disk ? 1 : 0);

    std::string rs;
    std::printf("rs %s\n", gfa_reference_samples("H\tVN:Z:1.1\tRS:Z:a b", rs) ? rs.c_str() : "(none)");
    std::printf("rs_absent %d\n", gfa_reference_samples("H\tVN:Z:1.0", rs) ? 1 : 0);

    HostIndex star;
    const GfaMetaRefusal none = assemble("W\ts\t1\tc\t*\t5\t>1\nW\ts\t1\tc\t7\t9\t>1\n", star);
    std::printf("star %u %u refused %" PRIu64 "\n", star.path_names[0].fragment, star.path_names[1].fragment, none.line);

    HostIndex dup;
    const std::string twins = "H\n\nW\ts\t1\tc\t0\t5\t>1\nP\tc\t1+\t*\nW\ts\t1\tc\t*\t5\t>1\n";
    std::printf("duplicate %" PRIu64 "\n", assemble(twins, dup).line);
    std::printf("duplicate_behind_stop %" PRIu64 "\n", assemble(twins, dup, 4).line);     // the device has refused line 5 (0-based 4): not looked at

    HostIndex hap;
    const std::string both = "#\n#\n#\n#\nW\ts\t1\tc\t0\t5\t>1\n#\nW\ts\tx\tc\t0\t5\t>1\n#\nW\ts\t1\tc\t0\t5\t>1\n";
    std::printf("hap %" PRIu64 "\n", assemble(both, hap).line);

    const GfaCounts c = count_gfa_on_host(text.data(), text.size());
    std::printf("counts_host %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", c.lines, c.segments, c.links, c.p_lines, c.w_lines, c.steps, c.label_bytes);
    return 0;
}
