// extract_files.cpp -- csrc/extract_files.hpp on the host (tests/test_tags_cpu.py builds it with ASan + UBSan): the line of `base`.names as
// it is written and read back, every rule and message of the reader, the path predicate at the ends of u64, and the two checks the readers
// share with their exact messages.
#include <cstdio>
#include <string>
#include <vector>

#include "extract_files.hpp"

using namespace gbwt_hip;

static int failures = 0;
static void expect(bool ok, const char *name) {
    std::printf("%s %s\n", ok ? "ok" : "FAIL", name);
    if (!ok) failures++;
}

struct Parsed { FileCheck check; std::vector<uint64_t> ids, lens; };
static Parsed parse(const std::string &text) {
    Parsed p;
    p.check = parse_names(text, p.ids, p.lens);
    return p;
}
static bool refused(const std::string &text, const std::string &message) {
    const Parsed p = parse(text);
    return p.check.status == GBWT_HIP_INVALID_DATA && p.check.message == message;
}
static bool invalid_digit(const std::string &line) { return refused("1\tx\t2\n" + line + "\n", "invalid digit found in string: " + line); }

int main() {
    using V = std::vector<uint64_t>;
    // the writer: id, sample, contig, phase, fragment, bases, tab-separated, a newline; the reader takes the first and the last field
    std::string lines;
    append_names_line(lines, 7, "HG002", "chr1", 2, 0, 12345);
    expect(lines == "7\tHG002\tchr1\t2\t0\t12345\n", "writer_line_format");
    append_names_line(lines, 8, "a sample", "contig 1 of 2", 0, 3, 0);
    const Parsed written = parse(lines);
    expect(written.check.ok() && written.ids == V{7, 8} && written.lens == V{12345, 0}, "writer_line_parses_back_names_with_spaces");
    const Parsed two = parse("5\t4\n0\tanything\t5");
    expect(two.check.ok() && two.ids == V{5, 0} && two.lens == V{4, 5}, "two_fields_no_final_newline");
    const Parsed crlf = parse("3\ts\tc\t0\t0\t9\r\n4\t1\r\n");
    expect(crlf.check.ok() && crlf.ids == V{3, 4} && crlf.lens == V{9, 1}, "crlf_stripped");
    expect(refused("", "No path names found"), "empty_text");
    expect(refused("5 4\n", "Name line missing last field"), "line_without_tab");
    expect(refused("5\t4\n\n0\t5\n", "Name line missing last field"), "empty_line_in_the_middle");
    expect(refused("\n", "Name line missing last field"), "newline_alone");
    expect(invalid_digit("1x\ts\t5"), "non_digit_in_id");
    expect(invalid_digit("1\ts\t5 "), "non_digit_in_bases");
    expect(invalid_digit("\ts\t5"), "empty_id_field");
    expect(invalid_digit("12345678901234567890\t5") && invalid_digit("5\t12345678901234567890"), "twenty_digits");
    const Parsed nines = parse("9999999999999999999\t9999999999999999999\n");
    expect(nines.check.ok() && nines.ids == V{9999999999999999999ull} && nines.lens == V{9999999999999999999ull}, "nineteen_nines");
    V ids, lens;
    const std::string missing = "/nonexistent-directory/extract_files.names";
    const FileCheck unopened = read_names(missing, ids, lens);
    expect(unopened.status == GBWT_HIP_IO_ERROR && unopened.message == "cannot open " + missing && ids.empty(), "file_that_does_not_exist");
    // path p is sequence 2 p: with 12 sequences paths 0 .. 5 exist
    expect(!path_exists(12, 6), "path_exists_half_of_sequences");
    expect(!path_exists(12, uint64_t(1) << 63) && !path_exists(~uint64_t(0), uint64_t(1) << 63), "path_exists_2_63");
    expect(!path_exists(12, ~uint64_t(0)) && !path_exists(~uint64_t(0), ~uint64_t(0)), "path_exists_2_64_minus_1");
    expect(path_exists(12, 5) && path_exists(12, 0) && !path_exists(0, 0), "path_exists_last_id");
    const FileCheck lacking = check_paths_exist(12, {0, 6}, {4, 5});
    expect(lacking.status == GBWT_HIP_INVALID_DATA && lacking.message == "Invalid length for path 6: expected 5, got 0 (no such path)" && check_paths_exist(12, {0, 5}, {4, 5}).ok(),
           "no_such_path_message");
    // rows of a text with an endmarker behind every row: bases 4, 0 and 5
    const uint64_t rows[4] = {0, 5, 6, 12};
    const FileCheck mismatch = check_walked_lengths({2, 9, 3}, {4, 0, 6}, rows);
    expect(mismatch.status == GBWT_HIP_INVALID_DATA && mismatch.message == "Invalid length for path 3: expected 6, got 5", "length_mismatch_message");
    expect(check_walked_lengths({2, 9, 3}, {4, 0, 5}, rows).ok() && check_walked_lengths({}, {}, rows).ok(), "matching_lengths");
    expect(!endmarker_valid(-2) && endmarker_valid(-1) && endmarker_valid(0) && endmarker_valid(255) && !endmarker_valid(256), "endmarker_argument");
    std::printf("%s\n", failures == 0 ? "done" : "failed");
    return failures == 0 ? 0 : 1;
}
