// ws_carve.hpp -- the one way a workspace is cut into regions.  A layout
// function takes its regions from a WsCarve in order; run on a null base it
// gives the sizes only, so the size a query reports and the pointers an entry
// point uses come from the same walk.
#pragma once
#include <cstddef>

namespace psvi {

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

struct WsCarve {
    char* base;  // nullptr: sizes only (every region nullptr)
    size_t off;
    explicit WsCarve(void* b) : base(static_cast<char*>(b)), off(0) {}
    // the next region, `count` elements of T rounded up to 256 bytes (count 0:
    // where an open-ended trailing region starts)
    template <class T>
    T* take(size_t count) {
        T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += align256(sizeof(T) * count);
        return r;
    }
    size_t bytes() const { return off; }
};

}  // namespace psvi
