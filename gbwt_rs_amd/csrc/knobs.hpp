// knobs.hpp -- the GBWT_HIP_* settings of an open and of a workspace, each read from the environment once.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <optional>

#include "device_index.hpp"
#include "extract_knobs.hpp"   // ExtractKnobs: the settings of a workspace, in plain C++ for extract_plan.hpp

// The GBWT_HIP_* settings of an open, read ONCE by gbwt_hip_open_file_flags / gbwt_hip_open_records_flags before the loader or any thread
// of the open starts, and kept on the handle: nothing else of an open looks at the environment (getenv is not safe against a concurrent
// setenv, and the early copy, the tail thread and the loader's jobs run next to the caller).  Unset = std::nullopt where it matters whether
// a setting is there at all, or where its default depends on the index.
struct OpenKnobs {
    bool seq_len = true;                               // GBWT_HIP_SEQ_LEN (0: no lengths, no samples)
    std::optional<uint32_t> sample_interval;           // GBWT_HIP_SAMPLE_INTERVAL (0: no samples; unset: by the size of the index, and coarse samples may be kept)
    std::optional<uint32_t> sample_coarse;             // GBWT_HIP_SAMPLE_COARSE (unset: nominal interval / 512)
    bool serial_samples = false;                       // GBWT_HIP_SERIAL_SAMPLES: a walk of every sequence instead of checkpoints
    bool two_pass = false;                             // GBWT_HIP_TWO_PASS_OPEN: lengths, then samples, by two walks of every sequence
    bool orientation_check = false;                    // GBWT_HIP_ORIENTATION_CHECK: fingerprints even where samples make them unnecessary
    std::optional<double> checkpoint_gap;              // GBWT_HIP_CHECKPOINT_GAP (unset: by the interval and the chains)
    std::optional<uint32_t> checkpoint_cap;            // GBWT_HIP_CHECKPOINT_CAP (unset: the interval)
    std::optional<uint32_t> chains;                    // GBWT_HIP_CHAINS (unset: CHAIN_MAX, and a handful of chained records are linked again without)
    uint32_t gather_limit = 1u << 21;                  // GBWT_HIP_GATHER_LIMIT: the counts of the packed blocks (0: none; tests lower it)
    uint32_t lookahead_hops = 15;                      // GBWT_HIP_LOOKAHEAD_HOPS
    bool walk_tables = true, deep_tables = true, compact_tables = true;   // GBWT_HIP_WALK_TABLES / _DEEP_TABLES / _COMPACT_TABLES (0 switches off)
    std::optional<uint64_t> table_bytes;               // GBWT_HIP_TABLE_BYTES (unset: by the device's memory)
    bool line_cache = true;                            // GBWT_HIP_LINE_CACHE (0: requests size their lines themselves)
    uint32_t locate_interval = 64;                     // GBWT_HIP_LOCATE_INTERVAL: expected records between two sampled ones of the locate index (1: every record, 0: none)
    bool trace = false;                                // GBWT_HIP_TRACE_OPEN set (any value): phase timings on stderr
    static OpenKnobs from_env() {
        OpenKnobs k;
        const auto on = [](const char *name) { const char *v = std::getenv(name); return !(v && std::atoi(v) == 0); };     // "0" switches off
        const auto forced = [](const char *name) { const char *v = std::getenv(name); return v && std::atoi(v) != 0; };  // anything but "0" switches on
        k.seq_len = on("GBWT_HIP_SEQ_LEN");
        if (const char *v = std::getenv("GBWT_HIP_SAMPLE_INTERVAL")) k.sample_interval = static_cast<uint32_t>(std::max(0, std::atoi(v)));
        if (const char *v = std::getenv("GBWT_HIP_SAMPLE_COARSE")) k.sample_coarse = static_cast<uint32_t>(std::max(1, std::atoi(v)));
        k.serial_samples = forced("GBWT_HIP_SERIAL_SAMPLES");
        k.two_pass = forced("GBWT_HIP_TWO_PASS_OPEN");
        k.orientation_check = forced("GBWT_HIP_ORIENTATION_CHECK");
        if (const char *v = std::getenv("GBWT_HIP_CHECKPOINT_GAP")) k.checkpoint_gap = std::max(2.0, std::atof(v));
        if (const char *v = std::getenv("GBWT_HIP_CHECKPOINT_CAP")) k.checkpoint_cap = static_cast<uint32_t>(std::max(1, std::atoi(v)));
        if (const char *v = std::getenv("GBWT_HIP_CHAINS")) k.chains = static_cast<uint32_t>(std::min<long>(gbwt_hip::CHAIN_MAX, std::max<long>(0, std::atol(v))));
        if (const char *v = std::getenv("GBWT_HIP_GATHER_LIMIT")) k.gather_limit = static_cast<uint32_t>(std::min<long>(1l << 21, std::max<long>(0, std::atol(v))));
        if (const char *v = std::getenv("GBWT_HIP_LOOKAHEAD_HOPS")) k.lookahead_hops = static_cast<uint32_t>(std::max(0, std::atoi(v)));
        k.walk_tables = on("GBWT_HIP_WALK_TABLES"); k.deep_tables = on("GBWT_HIP_DEEP_TABLES"); k.compact_tables = on("GBWT_HIP_COMPACT_TABLES");
        if (const char *v = std::getenv("GBWT_HIP_TABLE_BYTES")) k.table_bytes = std::strtoull(v, nullptr, 10);
        k.line_cache = on("GBWT_HIP_LINE_CACHE");
        if (const char *v = std::getenv("GBWT_HIP_LOCATE_INTERVAL")) k.locate_interval = static_cast<uint32_t>(std::min<long>(1l << 30, std::max<long>(0, std::atol(v))));
        k.trace = std::getenv("GBWT_HIP_TRACE_OPEN") != nullptr;
        return k;
    }
    // GBWT_HIP_LAZY_HOST_RECORDS, once per process: 0 = an open from a file makes the host's copy of the records in the loader's background
    static bool lazy_host_records() {
        static const bool lazy = [] { const char *e = std::getenv("GBWT_HIP_LAZY_HOST_RECORDS"); return !(e && e[0] == '0'); }();
        return lazy;
    }
};
