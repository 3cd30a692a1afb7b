// request_key.hpp -- the memo of a request family (plain C++): which request the results still in the workspace answer.  The C idiom "size
// query, then the same call with a buffer" must not compute twice: a call that repeats the stored request only copies the results out.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <vector>

namespace gbwt_hip {

struct KeyPart { const void *data; size_t bytes; };   // one array of a request as the caller gave it (ids, states, orientations)

class RequestKey {
public:
    // The parameters and the length of every part are compared before any byte; a part of no bytes is never looked at (its pointer may be null)
    bool matches(std::initializer_list<KeyPart> parts, std::initializer_list<int64_t> params) const {
        if (!valid_ || params.size() != params_.size() || !std::equal(params.begin(), params.end(), params_.begin())) return false;
        if (parts.size() != sizes_.size() || !std::equal(parts.begin(), parts.end(), sizes_.begin(), [](const KeyPart &p, size_t b) { return p.bytes == b; })) return false;
        const uint8_t *at = bytes_.data();
        for (const KeyPart &p : parts) {
            if (p.bytes != 0 && (p.data == nullptr || std::memcmp(at, p.data, p.bytes) != 0)) return false;
            at += p.bytes;
        }
        return true;
    }
    void store(std::initializer_list<KeyPart> parts, std::initializer_list<int64_t> params) {
        drop();
        for (const KeyPart &p : parts) {
            sizes_.push_back(p.bytes);
            if (p.bytes != 0) bytes_.insert(bytes_.end(), static_cast<const uint8_t *>(p.data), static_cast<const uint8_t *>(p.data) + p.bytes);
        }
        params_.assign(params);
        valid_ = true;
    }
    void drop() { valid_ = false; bytes_.clear(); sizes_.clear(); params_.clear(); }
    bool valid() const { return valid_; }

private:
    bool valid_ = false;
    std::vector<uint8_t> bytes_;
    std::vector<size_t> sizes_;
    std::vector<int64_t> params_;
};

}  // namespace gbwt_hip
