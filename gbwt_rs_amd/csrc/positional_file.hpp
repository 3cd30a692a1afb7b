// positional_file.hpp -- a file written at positions (plain C++): what the whole-file writers (batch_writer.hpp) and the host's graph
// lines (gfa_host.cpp) put their bytes into.
#pragma once

#include <fcntl.h>
#include <unistd.h>

#include <atomic>
#include <cstddef>
#include <cstdint>

namespace gbwt_hip {

// A file written at positions: every producer knows (or is told, in order) where its bytes go, so several threads write at once --
// one thread moved config 4's 4.5 GB to /dev/shm at 2.4 GB/s, most of it spent in the page cache's per-page work.
struct PositionalFile {
    int fd = -1;
    std::atomic<int> failed{0};
    ~PositionalFile() { if (fd >= 0) ::close(fd); }
    bool write_at(const char *data, size_t bytes, uint64_t at) {
        while (bytes != 0) {
            const ssize_t w = ::pwrite(fd, data, bytes, static_cast<off_t>(at));
            if (w <= 0) { failed = 1; return false; }
            data += w; bytes -= static_cast<size_t>(w); at += static_cast<uint64_t>(w);
        }
        return true;
    }
};

}  // namespace gbwt_hip
