// gs_ws.h -- one walk over a caller-allocated workspace gives both its size and its pointers.  A layout function walks its segments
// in order with a GsWs and returns the typed pointers with the total: the `*_ws_bytes` export calls it with base == nullptr, the entry
// point with the caller's block, and checks ws_bytes against that same total.
#pragma once
#include <cstddef>

static inline size_t gs_align_up(size_t x, size_t a) { return (x + a - 1) & ~(size_t)(a - 1); }      // a: a power of two

class GsWs {
    char* base_;
    size_t align_, off_ = 0;
    void* advance(size_t n) { void* p = base_ ? base_ + off_ : nullptr; off_ += n; return p; }

public:
    GsWs(void* base, size_t align) : base_((char*)base), align_(align) {}
    // `count` items of T (nullptr while sizing); the next segment starts at the next multiple of the alignment
    template <typename T> T* take(size_t count) { return (T*)advance(gs_align_up(count * sizeof(T), align_)); }
    // the last segment of a layout whose size is not rounded up
    template <typename T> T* tail(size_t count) { return (T*)advance(count * sizeof(T)); }
    void pad(size_t bytes) { advance(bytes); }
    size_t bytes() const { return off_; }
};
