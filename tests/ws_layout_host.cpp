// Host check of the workspace walker (csrc/gs_ws.h, included alone): see tests/test_ws_layout_cpu.py.
#include "gs_ws.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct Seg { size_t size, count; bool tail; };      // items of `size` bytes; tail: the last, unrounded segment
struct Got { char* p; size_t before, after; };

static Got take(GsWs& w, const Seg& s)
{
    Got g;
    g.before = w.bytes();
    switch (s.size) {
    case 1: g.p = (char*)(s.tail ? w.tail<char>(s.count) : w.take<char>(s.count)); break;
    case 4: g.p = (char*)(s.tail ? w.tail<int32_t>(s.count) : w.take<int32_t>(s.count)); break;
    case 8: g.p = (char*)(s.tail ? w.tail<uint64_t>(s.count) : w.take<uint64_t>(s.count)); break;
    default: g.p = (char*)(s.tail ? w.tail<long double>(s.count) : w.take<long double>(s.count)); break;   // 16 bytes
    }
    g.after = w.bytes();
    return g;
}

static int run(size_t align, const std::vector<Seg>& segs, size_t pad_after /* index of the segment a 256-byte pad follows */)
{
    // sizing walk
    GsWs size(nullptr, align);
    std::vector<size_t> offs;
    for (size_t i = 0; i < segs.size(); ++i) {
        const Got g = take(size, segs[i]);
        CHECK(g.p == nullptr);
        CHECK(g.before % align == 0);                                     // every segment starts aligned
        CHECK(g.after - g.before >= segs[i].size * segs[i].count);        // and holds its items
        CHECK(segs[i].tail ? g.after - g.before == segs[i].size * segs[i].count
                           : (g.after % align == 0 && g.after - g.before < segs[i].size * segs[i].count + align));
        offs.push_back(g.before);
        if (i == pad_after) {
            const size_t b = size.bytes();
            size.pad(256);
            CHECK(size.bytes() == b + 256);
        }
    }
    const size_t bytes = size.bytes();
    // carving walk over a block of exactly that size
    char* block = (char*)std::malloc(bytes ? bytes : 1);
    CHECK(block != nullptr);
    GsWs carve(block, align);
    size_t end = 0;
    for (size_t i = 0; i < segs.size(); ++i) {
        const Got g = take(carve, segs[i]);
        const size_t len = segs[i].size * segs[i].count;
        CHECK(g.p == block + offs[i]);                                    // the same offsets as the sizing walk
        CHECK((uintptr_t)(g.p - block) % align == 0);
        CHECK(offs[i] >= end);                                            // in order and disjoint
        end = offs[i] + len;
        CHECK(end <= bytes);
        if (len) { g.p[0] = (char)i; g.p[len - 1] = (char)i; }            // a write outside the block ends the sanitized build
        if (i == pad_after) carve.pad(256);
    }
    CHECK(carve.bytes() == bytes);
    for (size_t i = 0; i < segs.size(); ++i) {                            // nothing overwrote a neighbour
        const size_t len = segs[i].size * segs[i].count;
        if (len) CHECK(block[offs[i]] == (char)i && block[offs[i] + len - 1] == (char)i);
    }
    std::free(block);
    return 0;
}

int main()
{
    CHECK(gs_align_up(0, 256) == 0 && gs_align_up(1, 256) == 256 && gs_align_up(256, 256) == 256 && gs_align_up(257, 256) == 512);
    CHECK(gs_align_up(15, 16) == 16 && gs_align_up(16, 16) == 16 && gs_align_up(17, 16) == 32);
    const std::vector<std::vector<Seg>> lists = {
        { { 16, 1, false }, { 16, 1, false }, { 4, 1, false }, { 4, 64, false }, { 4, 64, false }, { 16, 4, false } },        // one-tile image
        { { 4, 2049, false }, { 8, 0, false }, { 1, 257, false }, { 8, 33, false }, { 4, 7, false } },                      // a zero-count segment
        { { 4, 100000, false }, { 4, 391, false }, { 8, 391, true } },                                                      // unrounded tail
        { { 4, 4, false }, { 8, 4 * 7680, false } },                                                                        // ctrl + descriptors
    };
    int n = 0;
    for (size_t align : { (size_t)16, (size_t)256 })
        for (size_t k = 0; k < lists.size(); ++k, ++n)
            if (run(align, lists[k], k % 2 ? 1 : lists[k].size() - 1)) return 1;
    // 2^33 eight-byte items: 2^36 bytes, no wrap, and the next segment starts behind them
    for (size_t align : { (size_t)16, (size_t)256 }) {
        GsWs w(nullptr, align);
        w.take<int32_t>(3);
        const size_t b = w.bytes();
        w.take<uint64_t>((size_t)1 << 33);
        CHECK(w.bytes() == b + ((size_t)1 << 36));
        w.take<char>(1);
        CHECK(w.bytes() == b + ((size_t)1 << 36) + align);
    }
    std::printf("ok %d\n", n);
    return 0;
}
