// query_buffers.h — bookkeeping of the device buffers a context owns
// (pbrt_gpu_buffer, include/pbrt_gpu.h): the context's list of live buffers,
// the range check of upload / download, and free-all when the context is
// destroyed. A buffer's device memory must never outlive its context's stream,
// so the context, not the caller, is the owner of last resort.
// Plain C++ with no dependency on HIP: the device allocator and its free are
// passed in, and tests/query_buffer_check.cpp compiles this header on its own.
#pragma once

#include <cstddef>
#include <cstdint>

struct pbrt_gpu_ctx;

// the handle of include/pbrt_gpu.h: a node of its context's list
struct pbrt_gpu_buffer {
    pbrt_gpu_ctx* ctx;
    void* ptr;        // device memory
    size_t bytes;
    pbrt_gpu_buffer *prev, *next;
};

namespace pbrtq {

struct BufferList {
    pbrt_gpu_buffer* head = nullptr;
    size_t count = 0;
};

// [offset, offset + bytes) lies inside a buffer of `size` bytes (no overflow)
inline bool range_ok(size_t size, size_t offset, size_t bytes) { return offset <= size && bytes <= size - offset; }

// A new buffer of `bytes` bytes from alloc(bytes) (nullptr: out of memory), at
// the head of the list; nullptr when bytes is 0 or the allocation fails.
template <class Alloc>
pbrt_gpu_buffer* list_create(BufferList& l, pbrt_gpu_ctx* ctx, size_t bytes, Alloc alloc) {
    if (bytes == 0) return nullptr;
    void* p = alloc(bytes);
    if (!p) return nullptr;
    pbrt_gpu_buffer* b = new pbrt_gpu_buffer{ctx, p, bytes, nullptr, l.head};
    if (l.head) l.head->prev = b;
    l.head = b;
    l.count++;
    return b;
}

// b is on l
inline bool list_owns(const BufferList& l, const pbrt_gpu_buffer* b) {
    for (const pbrt_gpu_buffer* q = l.head; q; q = q->next)
        if (q == b) return true;
    return false;
}

// unlinks b, frees its device memory with release(ptr) and deletes the node
template <class Free>
void list_destroy(BufferList& l, pbrt_gpu_buffer* b, Free release) {
    if (b->prev) b->prev->next = b->next;
    else l.head = b->next;
    if (b->next) b->next->prev = b->prev;
    l.count--;
    release(b->ptr);
    delete b;
}

// what pbrt_gpu_destroy does with the buffers still alive; returns how many
template <class Free>
size_t list_free_all(BufferList& l, Free release) {
    size_t n = 0;
    while (l.head) {
        list_destroy(l, l.head, release);
        n++;
    }
    return n;
}

}  // namespace pbrtq
