// batch_writer.hpp -- the pipelined whole-file writer shared by gbwt_hip_write_gfa* (capi_lines.hip), gbwt_hip_write_sequences
// (capi_sequences.hip), gbwt_hip_write_tag_array (capi_tags.hip) and gbwt_hip_write_suffix_array (capi_suffix_array.hip): batches of device
// text, formatted into two device buffers in turn, leave for a file at known positions while the next batch is made.
#pragma once

#include <fcntl.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "capi_internal.hpp"
#include "positional_file.hpp"

namespace gbwt_hip {

// The writer's side of a whole-file write: one thread that first puts out what precedes the batches (`preamble`, host work: the H-, S- and
// L-lines of a GFA file; returns the bytes it wrote from offset 0 on, nothing when unset), then takes finished batches -- device text -- and
// moves them to the file in pieces of 32 MiB: the piece travels into one of a few pinned buffers (the copy of the next piece runs under
// whatever happens to this one) and a small pool of threads writes the buffers at their positions.  The caller formats the next batch into
// the other device text buffer meanwhile.
struct BatchWriter {
    static constexpr size_t PIECE = size_t(32) << 20;
    int WRITERS = 3, BUFFERS = 5;            // GBWT_HIP_GFA_WRITERS (1 .. 16); two more pinned buffers than writing threads
    struct Job { const char *text; uint64_t bytes; int slot; };
    struct Piece { int buffer; uint64_t bytes, at; };
    std::mutex m;
    std::condition_variable cv;
    std::deque<Job> jobs;
    std::deque<Piece> pieces;              // pinned buffers that hold a piece on its way to the file
    std::vector<char> buffer_busy;
    bool closing = false, no_more_pieces = false, slot_busy[2] = {false, false};
    gbwt_hip_status status = GBWT_HIP_OK;
    std::string message;
    std::thread worker;
    PositionalFile *file = nullptr;
    std::function<uint64_t()> preamble;
    const char *what = "gfa";              // (GBWT_HIP_TRACE_GFA lines and error messages)
    int device = 0;

    void fail_with(gbwt_hip_status st, const std::string &msg) {
        std::lock_guard<std::mutex> lock(m);
        if (status == GBWT_HIP_OK) { status = st; message = msg; }
        cv.notify_all();
    }
    void run() {
        if (const char *v = std::getenv("GBWT_HIP_GFA_WRITERS")) WRITERS = std::min(16, std::max(1, std::atoi(v)));
        BUFFERS = WRITERS + 2;
        std::vector<void *> pinned(BUFFERS, nullptr);
        buffer_busy.assign(BUFFERS, 0);
        hipStream_t stream = nullptr;
        const bool trace = std::getenv("GBWT_HIP_TRACE_GFA") != nullptr;       // phases of a whole-file write on stderr
        const auto t0 = std::chrono::steady_clock::now();
        const auto since = [&t0]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
        uint64_t batch_bytes = 0;
        std::vector<std::thread> pool;
        try {
            uint64_t cursor = preamble ? preamble() : 0;
            if (file->failed) throw std::runtime_error("short write");
            if (trace && preamble) std::fprintf(stderr, "[%s] preamble: %llu bytes generated and written in %.1f ms\n", what, static_cast<unsigned long long>(cursor), since());
            HIP_CHECK(hipSetDevice(device));
            HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
            for (int i = 0; i < BUFFERS; i++) HIP_CHECK(hipHostMalloc(&pinned[i], PIECE, hipHostMallocDefault));
            for (int t = 0; t < WRITERS; t++)
                pool.emplace_back([this, &pinned]() {
                    for (;;) {
                        Piece p;
                        {
                            std::unique_lock<std::mutex> lock(m);
                            cv.wait(lock, [&] { return !pieces.empty() || no_more_pieces; });
                            if (pieces.empty()) return;
                            p = pieces.front(); pieces.pop_front();
                        }
                        if (!file->write_at(static_cast<const char *>(pinned[p.buffer]), p.bytes, p.at)) fail_with(GBWT_HIP_IO_ERROR, "short write");
                        { std::lock_guard<std::mutex> lock(m); buffer_busy[p.buffer] = 0; }
                        cv.notify_all();
                    }
                });
            for (;;) {
                Job job;
                {
                    std::unique_lock<std::mutex> lock(m);
                    cv.wait(lock, [&] { return !jobs.empty() || closing || status != GBWT_HIP_OK; });
                    if (status != GBWT_HIP_OK || jobs.empty()) break;
                    job = jobs.front(); jobs.pop_front();
                }
                batch_bytes += job.bytes;
                for (uint64_t done = 0; done < job.bytes; done += PIECE) {
                    int b = -1;
                    {
                        std::unique_lock<std::mutex> lock(m);
                        cv.wait(lock, [&] { for (int i = 0; i < BUFFERS; i++) if (!buffer_busy[i]) return true; return status != GBWT_HIP_OK; });
                        if (status != GBWT_HIP_OK) break;
                        for (int i = 0; i < BUFFERS; i++) if (!buffer_busy[i]) { b = i; break; }
                        buffer_busy[b] = 1;
                    }
                    const uint64_t len = std::min<uint64_t>(PIECE, job.bytes - done);
                    HIP_CHECK(hipMemcpyAsync(pinned[b], job.text + done, len, hipMemcpyDeviceToHost, stream));
                    HIP_CHECK(hipStreamSynchronize(stream));
                    { std::lock_guard<std::mutex> lock(m); pieces.push_back(Piece{b, len, cursor + done}); }
                    cv.notify_all();
                }
                cursor += job.bytes;
                {   // the device text of this batch has left: the formatter may have the slot back
                    std::lock_guard<std::mutex> lock(m);
                    slot_busy[job.slot] = false;
                }
                cv.notify_all();
            }
        } catch (const HipError &e) {
            fail_with(GBWT_HIP_DEVICE_ERROR, std::string(e.what) + ": " + hipGetErrorString(e.err));
        } catch (const std::exception &e) {
            fail_with(GBWT_HIP_IO_ERROR, std::string(what) + " writer: " + e.what());
        }
        { std::lock_guard<std::mutex> lock(m); no_more_pieces = true; }
        cv.notify_all();
        for (auto &t : pool) t.join();
        if (trace) std::fprintf(stderr, "[%s] batches: %llu bytes; writer threads done at %.1f ms\n", what, static_cast<unsigned long long>(batch_bytes), since());
        for (int i = 0; i < BUFFERS; i++) if (pinned[i]) (void)hipHostFree(pinned[i]);
        if (stream) (void)hipStreamDestroy(stream);
        std::lock_guard<std::mutex> lock(m);
        closing = true; slot_busy[0] = slot_busy[1] = false;
        cv.notify_all();
    }
    void start() { worker = std::thread([this]() { run(); }); }
    // the formatter's side: wait until the device text buffer of `slot` has been read out; false when the writer has failed
    bool acquire(int slot) {
        std::unique_lock<std::mutex> lock(m);
        cv.wait(lock, [&] { return !slot_busy[slot] || status != GBWT_HIP_OK; });
        if (status != GBWT_HIP_OK) return false;
        slot_busy[slot] = true;
        return true;
    }
    void submit(const char *text, uint64_t bytes, int slot) {
        { std::lock_guard<std::mutex> lock(m); jobs.push_back(Job{text, bytes, slot}); }
        cv.notify_all();
    }
    gbwt_hip_status finish() {
        { std::lock_guard<std::mutex> lock(m); closing = true; }
        cv.notify_all();
        if (worker.joinable()) worker.join();
        return status;
    }
    ~BatchWriter() { (void)finish(); }
};

}  // namespace gbwt_hip
