// tests/query_buffer_check.cpp — host check of the bookkeeping of a context's
// device buffers (go-pbrt_amd/csrc/query_buffers.h), with malloc standing in
// for the device allocator:
//   - range_ok accepts exactly the ranges inside a buffer, with no overflow for
//     offsets and sizes near SIZE_MAX;
//   - create / destroy in every order (head, middle, tail, random) keep the
//     list and its count consistent, and every pointer is released exactly once;
//   - a zero-byte buffer and a failed allocation add nothing;
//   - free-all releases whatever is left (the case of pbrt_gpu_destroy with
//     buffers still open) and leaves an empty list that can be used again.
// Compiled with -fsanitize=address,undefined and run by tests/test_query_abi.py:
// a leak, a double free or a use after free fails the run. Prints
// "ranges=.. buffers=.. freed=.. bad=..".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../go-pbrt_amd/csrc/query_buffers.h"

using namespace pbrtq;

static std::set<void*> g_live;   // what the stand-in allocator handed out
static long g_freed = 0, g_bad = 0;

static void* dev_alloc(size_t n) {
    void* p = std::malloc(n);
    g_live.insert(p);
    return p;
}
static void dev_free(void* p) {
    if (!g_live.erase(p)) g_bad++;   // released twice, or never allocated
    std::free(p);
    g_freed++;
}

static size_t walk(const BufferList& l) {   // length, checking the back links
    size_t n = 0;
    const pbrt_gpu_buffer* prev = nullptr;
    for (const pbrt_gpu_buffer* b = l.head; b; prev = b, b = b->next, n++)
        if (b->prev != prev) g_bad++;
    return n;
}

int main() {
    long ranges = 0, buffers = 0;
    // ---- range_ok against the definition, small sizes exhaustively
    for (size_t size = 0; size <= 12; size++)
        for (size_t off = 0; off <= 14; off++)
            for (size_t n = 0; n <= 14; n++) {
                ranges++;
                if (range_ok(size, off, n) != (off + n <= size)) g_bad++;
            }
    const size_t M = SIZE_MAX;
    const struct { size_t size, off, n; bool ok; } edge[] = {
        {16, M, 2, false}, {16, 2, M, false}, {16, M, M, false}, {16, 8, M - 7, false}, {M, M, 0, true},
        {M, 1, M - 1, true}, {M, 2, M - 1, false}, {0, 0, 0, true}, {0, 0, 1, false}, {16, 16, 0, true},
    };
    for (const auto& e : edge) {
        ranges++;
        if (range_ok(e.size, e.off, e.n) != e.ok) g_bad++;
    }

    // ---- the list
    pbrt_gpu_ctx* ctx = reinterpret_cast<pbrt_gpu_ctx*>(uintptr_t(0x1000));   // only stored, never followed
    BufferList l;
    if (list_create(l, ctx, 0, dev_alloc) != nullptr || l.count != 0 || l.head) g_bad++;            // zero bytes
    if (list_create(l, ctx, 64, [](size_t) -> void* { return nullptr; }) != nullptr || l.count != 0) g_bad++;   // out of memory
    uint32_t rng = 12345;
    auto next = [&rng]() { return rng = rng * 1664525u + 1013904223u; };
    for (int round = 0; round < 50; round++) {
        std::vector<pbrt_gpu_buffer*> mine;
        const int n = 1 + (int)(next() >> 8) % 40;
        for (int i = 0; i < n; i++) {
            const size_t bytes = 1 + (next() >> 8) % 512;
            pbrt_gpu_buffer* b = list_create(l, ctx, bytes, dev_alloc);
            buffers++;
            if (!b || b->ctx != ctx || b->bytes != bytes || !b->ptr || l.head != b) { g_bad++; continue; }
            static_cast<unsigned char*>(b->ptr)[bytes - 1] = 1;   // the allocation really has that size
            mine.push_back(b);
        }
        if (l.count != mine.size() || walk(l) != mine.size()) g_bad++;
        for (pbrt_gpu_buffer* b : mine)
            if (!list_owns(l, b)) g_bad++;
        pbrt_gpu_buffer other{ctx, nullptr, 1, nullptr, nullptr};
        if (list_owns(l, &other)) g_bad++;
        // destroy some: head, tail, middle, then random ones; leave the rest open
        const int leave = round % 4;   // 0..3 buffers left for free-all (0: none)
        while ((int)mine.size() > leave) {
            size_t k = mine.size() % 3 == 0 ? mine.size() - 1 : mine.size() % 3 == 1 ? 0 : (next() >> 8) % mine.size();
            list_destroy(l, mine[k], dev_free);
            mine.erase(mine.begin() + (long)k);
            if (l.count != mine.size() || walk(l) != mine.size()) g_bad++;
        }
        // what pbrt_gpu_destroy does
        if (list_free_all(l, dev_free) != mine.size()) g_bad++;
        if (l.head || l.count != 0 || !g_live.empty()) g_bad++;
    }
    if (g_freed != buffers) g_bad++;
    std::printf("ranges=%ld buffers=%ld freed=%ld bad=%ld\n", ranges, buffers, g_freed, g_bad);
    return g_bad == 0 ? 0 : 1;
}
