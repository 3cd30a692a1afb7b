// The host's side of the GFA text (csrc/gfa_host.cpp) as a program of its own, built with ASan + UBSan by tests/test_gfa_host_cpu.py and
// linked with gfa_host.cpp and host_index.cpp only: no GPU, no HIP.  It reads its work from the file GFA_HOST_JOB names, one item per line:
//   file <path>      load this GBZ through HostIndex
//   lines <name>     host_graph_lines of the loaded file into GFA_HOST_OUT/<name>; prints "lines.<name> <the text in hex>"
//   row <k> <v ...>  host_segment_path over the GBWT nodes v ... of the loaded file; prints "row.<k> <summed segment lengths> <segment>:<orientation> ..."
// "done" at the end.
#include <fcntl.h>

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "gfa_host.hpp"

using namespace gbwt_hip;

int main() {
    const char *job = std::getenv("GFA_HOST_JOB"), *out_dir = std::getenv("GFA_HOST_OUT");
    if (!job || !out_dir) { std::printf("FAIL no job\n"); return 1; }
    std::ifstream in(job);
    HostIndex h;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream fields(line);
        std::string what, name;
        fields >> what >> name;
        if (what == "file") {
            h = load_index_file(name);
        } else if (what == "lines") {
            const std::string path = std::string(out_dir) + "/" + name;
            uint64_t bytes = 0;
            {
                PositionalFile file;
                file.fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
                if (file.fd < 0) { std::printf("FAIL cannot create %s\n", path.c_str()); return 1; }
                bytes = host_graph_lines(h, h.has_translation && !h.segment_starts.empty(), file);     // (with the thread count the code picks)
                if (file.failed) { std::printf("FAIL short write\n"); return 1; }
            }
            std::ifstream written(path, std::ios::binary);
            const std::string text((std::istreambuf_iterator<char>(written)), std::istreambuf_iterator<char>());
            if (text.size() != bytes) { std::printf("FAIL %s: %zu bytes in the file, %" PRIu64 " returned\n", name.c_str(), text.size(), bytes); return 1; }
            std::printf("lines.%s ", name.c_str());
            for (unsigned char c : text) std::printf("%02x", c);
            std::printf("\n");
        } else if (what == "row") {
            std::vector<uint32_t> nodes;
            for (uint32_t v; fields >> v;) nodes.push_back(v);
            std::vector<std::pair<uint64_t, bool>> tokens{{99, true}};      // (cleared by the call)
            uint64_t seq_len = 99;
            host_segment_path(h, nodes.data(), nodes.size(), tokens, seq_len);
            std::printf("row.%s %" PRIu64, name.c_str(), seq_len);
            for (const auto &t : tokens) std::printf(" %" PRIu64 ":%d", t.first, int(t.second));
            std::printf("\n");
        }
    }
    std::printf("done\n");
    return 0;
}
