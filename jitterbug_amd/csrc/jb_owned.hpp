// jb_owned.hpp — "this allocation has exactly one owner and is freed exactly once".  The C ABI handle (jb_api.hip) holds its device
// buffers, pinned host staging and event through this move-only owner: destroying the handle frees them, and the handle cannot be copied.
// A lazily created group is allocated into local owners and moved into the handle only once every allocation in it has succeeded, so a
// failure frees what the group had taken and leaves the handle as it was.  Written against a tiny API trait, like jb_device_guard.hpp,
// so that tests/host_harness.cpp can run it with a recording stub.
#pragma once

#include <cstddef>
#include <utility>

namespace jb {

template <typename P, typename Api>      // P: pointer (or handle) type; Api::alloc(P*, size_t n): 0 or the error code; Api::free(P)
class Owned {
    P p_ = P();
    size_t n_ = 0;
public:
    Owned() = default;
    Owned(Owned&& o) noexcept : p_(std::exchange(o.p_, P())), n_(std::exchange(o.n_, 0)) {}
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, P()); n_ = std::exchange(o.n_, 0); }
        return *this;
    }
    ~Owned() { reset(); }
    P get() const { return p_; }
    size_t size() const { return n_; }      // elements
    explicit operator bool() const { return p_ != P(); }
    auto alloc(size_t n) {                  // frees what it held, then takes n elements; on failure it holds nothing
        reset();
        const auto rc = Api::alloc(&p_, n);
        if (rc == 0) n_ = n; else p_ = P();
        return rc;
    }
    void reset() {
        if (p_ != P()) Api::free(p_);
        p_ = P(); n_ = 0;
    }
};

}  // namespace jb
