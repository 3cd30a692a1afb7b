// The reference's test of GBZ::reference_positions (src/gbz/tests.rs:521-567), restated against the C++ mirror of its interface
// (include/gbwt_hip.hpp): for every reference path of example.gbz the starting positions of all nodes are collected with start / forward /
// sequence, and reference_positions(interval) for interval 0 .. 9 must keep exactly those at or behind the offset of the position kept
// before + interval.  Usage: test_reference_positions <golden dir>.
// Without a HIP device the library has no fallback: the program then checks for GBWT_HIP_NO_DEVICE and says so.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gbwt_hip.hpp"

using namespace gbwt_hip;

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : "tests/golden";
    if (gbwt_hip_device_count() == 0) {
        try {
            GBZ graph(dir + "/example.gbz");
            REQUIRE(!"opened an index without a device");
        } catch (const Error &e) {
            REQUIRE(e.status == GBWT_HIP_NO_DEVICE);
            std::printf("no HIP device: GBWT_HIP_NO_DEVICE as documented (no CPU fallback)\n");
            return 0;
        }
    }
    GBZ graph(dir + "/example.gbz");
    const std::vector<size_t> ref_paths = graph.reference_paths(true);
    REQUIRE((ref_paths == std::vector<size_t>{0, 1}));

    // For each reference path, collect the starting positions of all nodes.
    std::vector<ReferencePath> node_starts;
    for (size_t id : ref_paths) {
        size_t path_offset = 0;
        ReferencePath truth{id, 0, {}};
        for (auto curr = graph.start(encode_path(id, Orientation::Forward)); curr; curr = graph.forward(*curr)) {
            truth.positions.emplace_back(path_offset, *curr);
            const auto label = graph.sequence(node_id(curr->node));
            REQUIRE(label.has_value());
            path_offset += label->size();
        }
        truth.len = path_offset;
        node_starts.push_back(truth);
    }
    REQUIRE(node_starts[0].len == 5 && node_starts[1].len == 4);

    // Check the indexed positions with various intervals.
    for (size_t interval = 0; interval < 10; interval++) {
        const std::vector<ReferencePath> paths = graph.reference_positions(interval);
        REQUIRE(paths.size() == node_starts.size());
        for (size_t i = 0; i < paths.size(); i++) {
            REQUIRE(paths[i].id == node_starts[i].id);
            REQUIRE(paths[i].len == node_starts[i].len);
            size_t next = 0;
            auto iter = paths[i].positions.begin();
            for (const auto &truth : node_starts[i].positions) {
                if (truth.first >= next) {
                    REQUIRE(iter != paths[i].positions.end());
                    REQUIRE(iter->first == truth.first);
                    REQUIRE(iter->second.node == truth.second.node && iter->second.offset == truth.second.offset);
                    ++iter;
                    next = truth.first + interval;
                }
            }
            REQUIRE(iter == paths[i].positions.end());
        }
    }
    std::printf("reference positions mirror: all checks passed\n");
    return 0;
}
