// The memo of a request family (csrc/request_key.hpp) as a program of its own, built with ASan + UBSan by tests/test_request_key_cpu.py.
// One line per case, "ok <case>" or "FAIL <case>"; "done" at the end.
#include <cstdio>

#include "request_key.hpp"

using gbwt_hip::RequestKey;

static void check(const char *name, bool ok) { std::printf("%s %s\n", ok ? "ok" : "FAIL", name); }

int main() {
    const char ab[] = "ABCD", abx[] = "ABCX";
    {
        RequestKey k;
        check("fresh_matches_nothing", !k.valid() && !k.matches({{ab, 4}}, {1}) && !k.matches({{ab, 4}}, {}));
        check("fresh_not_even_empty", !k.matches({{nullptr, 0}}, {}) && !k.matches({}, {}));
    }
    {
        RequestKey k;
        k.store({{nullptr, 0}}, {1, 7});
        check("empty_same_parameters", k.valid() && k.matches({{nullptr, 0}}, {1, 7}) && k.matches({{ab, 0}}, {1, 7}));
        check("empty_other_parameter", !k.matches({{nullptr, 0}}, {1, 8}) && !k.matches({{nullptr, 0}}, {1}) && !k.matches({{nullptr, 0}}, {1, 7, 0}));
        check("empty_not_bytes", !k.matches({{ab, 1}}, {1, 7}));
    }
    {
        RequestKey k;
        k.store({{ab, 4}}, {0, -1, 2});
        check("equal_bytes_match", k.matches({{ab, 4}}, {0, -1, 2}));
        check("one_parameter_differs", !k.matches({{ab, 4}}, {1, -1, 2}) && !k.matches({{ab, 4}}, {0, 255, 2}) && !k.matches({{ab, 4}}, {0, -1, 3}));
        check("prefix_shorter", !k.matches({{ab, 3}}, {0, -1, 2}));
        check("prefix_longer", !k.matches({{"ABCDE", 5}}, {0, -1, 2}));
        check("last_byte_differs", !k.matches({{abx, 4}}, {0, -1, 2}));
        check("null_with_length", !k.matches({{nullptr, 4}}, {0, -1, 2}));
        check("more_parts", !k.matches({{ab, 4}, {nullptr, 0}}, {0, -1, 2}));
    }
    {
        RequestKey k;
        k.store({{"AB", 2}, {"C", 1}}, {3});
        check("two_parts_match", k.matches({{"AB", 2}, {"C", 1}}, {3}));
        check("two_parts_other_split", !k.matches({{"A", 1}, {"BC", 2}}, {3}));
        check("two_parts_as_one", !k.matches({{"ABC", 3}}, {3}));
        check("second_part_differs", !k.matches({{"AB", 2}, {"D", 1}}, {3}));
        k.drop();
        check("dropped_matches_nothing", !k.valid() && !k.matches({{"AB", 2}, {"C", 1}}, {3}));
        k.store({{abx, 4}}, {});
        check("store_after_drop", k.valid() && k.matches({{abx, 4}}, {}) && !k.matches({{ab, 4}}, {}) && !k.matches({{"AB", 2}, {"C", 1}}, {3}));
        k.store({{ab, 2}}, {5});                 // a store replaces the request, it does not append to it
        check("store_replaces", k.matches({{"AB", 2}}, {5}) && !k.matches({{abx, 4}}, {}));
    }
    {
        RequestKey k;
        k.store({{nullptr, 0}, {nullptr, 0}}, {0, 0, 0});     // an edges request of no rows: ids and orientations
        check("null_parts_accepted", k.matches({{nullptr, 0}, {nullptr, 0}}, {0, 0, 0}) && !k.matches({{nullptr, 0}}, {0, 0, 0}));
    }
    std::printf("done\n");
    return 0;
}
