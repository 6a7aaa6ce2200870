// devmem.h -- THE owner of the host side's device and pinned memory: a DevScope is a list of blocks with one lifetime, allocated through it (checked: a refusal is reported through fail() and latched) and released
// with it; an alias of another block is assigned and never registered.  Host only.  The allocator sits behind four macros that default to the HIP calls: with them defined, no HIP include is needed (tests/host/devmem_main.cpp)
#pragma once
#include <assert.h>
#include <stddef.h>
#include <algorithm>
#include <atomic>
#include <vector>
#ifndef DQN_DEV_ALLOC      // each allocation macro yields nullptr, or the text of the refusal
#include <hip/hip_runtime.h>
static inline const char* devmem_hip_err(hipError_t e) { return e == hipSuccess ? nullptr : hipGetErrorString(e); }
#define DQN_DEV_ALLOC(pp, bytes) devmem_hip_err(hipMalloc((pp), (bytes)))
#define DQN_DEV_FREE(p) (void)hipFree(p)
#define DQN_HOST_ALLOC(pp, bytes, flags) devmem_hip_err(hipHostMalloc((pp), (bytes), (flags)))
#define DQN_HOST_FREE(p) (void)hipHostFree(p)
#endif
int fail(const char* fmt, ...);      // records the message for dqn_last_error(), returns -1
inline std::atomic<size_t> g_devmem_blocks{0}, g_devmem_bytes{0};      // live blocks and bytes of every scope of the process (dqn_debug_devmem): written here only
struct DevScope {
    struct Block { void* p; size_t bytes; bool pinned; };
    std::vector<Block> blocks;
    bool failed = false;      // latched by any refused get, cleared by release(): a builder that allocates many blocks tests it once at its end
    DevScope() = default; DevScope(const DevScope&) = delete; DevScope& operator=(const DevScope&) = delete;
    ~DevScope() { assert(blocks.empty() && "a DevScope must be released before it is destroyed"); }      // (no free here: a scope is released where the device is known to be idle, and never synchronises)
    // n elements (room for at least one) of device memory / of pinned host memory; *p is null after a refusal
    template <class T> int get(T** p, size_t n) { return get_block((void**)p, n * sizeof(T), std::max<size_t>(n, 1) * sizeof(T), false, 0); }
    template <class T> int get_pinned(T** p, size_t n, unsigned flags) { return get_block((void**)p, n * sizeof(T), std::max<size_t>(n, 1) * sizeof(T), true, flags); }
    // one block released early (null, or a pointer the scope does not hold such as an alias: nothing happens); everything, newest first
    void drop(void* p) { for (size_t i = blocks.size(); i-- > 0;) if (blocks[i].p == p) { free_block(blocks[i]); blocks.erase(blocks.begin() + (ptrdiff_t)i); return; } }
    void release() { for (size_t i = blocks.size(); i-- > 0;) free_block(blocks[i]); blocks.clear(); failed = false; }
    int get_block(void** p, size_t asked, size_t bytes, bool pinned, unsigned flags) {
        *p = nullptr; (void)flags;
        const char* err = pinned ? DQN_HOST_ALLOC(p, bytes, flags) : DQN_DEV_ALLOC(p, bytes);
        if (err) { *p = nullptr; failed = true; return fail("%s of %zu bytes failed: %s", pinned ? "hipHostMalloc" : "hipMalloc", asked, err); }
        blocks.push_back({*p, bytes, pinned}); g_devmem_blocks += 1; g_devmem_bytes += bytes; return 0;
    }
    static void free_block(const Block& b) { if (b.pinned) DQN_HOST_FREE(b.p); else DQN_DEV_FREE(b.p); g_devmem_blocks -= 1; g_devmem_bytes -= b.bytes; }
};
#define DM(scope, p, n) do { if ((scope).get(&(p), (n))) return -1; } while (0)
// a grow-only buffer: kept while need <= *cap, else dropped and allocated again with max(floor, 2 * need) elements (the caller has synchronised whatever reads the block)
template <class T> int grow(DevScope& s, T** p, size_t* cap, size_t need, size_t floor) {
    if (need <= *cap) return 0;
    s.drop(*p); *p = nullptr; *cap = 0;
    const size_t n = std::max(floor, 2 * need); if (s.get(p, n)) return -1;
    *cap = n; return 0;
}
