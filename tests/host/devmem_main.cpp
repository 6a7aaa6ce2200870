// devmem_main.cpp -- stand-alone check of csrc/devmem.h (DevScope, grow, the live counters) against a counting malloc / free that can be told to refuse the k-th
// request.  Built with -fsanitize=address,undefined and run directly by tests/test_devmem_cpu.py: the sanitizer's exit status (leaks, double frees, use after
// free) is part of the verdict.  No HIP: the four allocator macros are defined here, before the header.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>
#include <vector>

struct Rec { size_t bytes; bool pinned; };
static std::map<void*, Rec> g_live;             // the model: what is allocated now
static std::vector<void*> g_freed;              // every free, in order
static std::vector<void*> g_alloced;            // every successful allocation, in order
static int g_req = 0, g_fail_at = 0;            // requests so far; the request to refuse (0: none)
static unsigned g_last_flags = 0;
static int g_errors = 0;
static char g_msg[256] = "";

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); g_errors++; } } while (0)

static const char* t_alloc(void** pp, size_t bytes, bool pinned, unsigned flags) {
    g_req++; g_last_flags = flags;
    if (g_req == g_fail_at) return "out of memory (test)";
    *pp = malloc(bytes); g_live[*pp] = Rec{bytes, pinned}; g_alloced.push_back(*pp);
    return nullptr;
}
static void t_free(void* p, bool pinned) {
    auto it = g_live.find(p);
    CHECK(it != g_live.end());                           // a block the model holds: not freed twice, not foreign
    if (it == g_live.end()) return;
    CHECK(it->second.pinned == pinned);                  // pinned and device blocks go to their own free function
    g_live.erase(it); g_freed.push_back(p); free(p);
}
#define DQN_DEV_ALLOC(pp, bytes) t_alloc((pp), (bytes), false, 0)
#define DQN_DEV_FREE(p) t_free((p), false)
#define DQN_HOST_ALLOC(pp, bytes, flags) t_alloc((pp), (bytes), true, (flags))
#define DQN_HOST_FREE(p) t_free((p), true)
#include "devmem.h"

int fail(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_msg, sizeof g_msg, fmt, ap); va_end(ap); return -1; }

// the library's counters equal the model's: called after every operation
static void same() {
    size_t bytes = 0; for (auto& kv : g_live) bytes += kv.second.bytes;
    CHECK(g_devmem_blocks.load() == g_live.size());
    CHECK(g_devmem_bytes.load() == bytes);
}
static void reset_log() { g_freed.clear(); g_alloced.clear(); g_req = 0; g_fail_at = 0; }

static void test_release_order() {
    reset_log(); DevScope s;
    float* a = nullptr; double* b = nullptr; char* c = nullptr; int* h = nullptr; long long* d = nullptr;
    CHECK(s.get(&a, 3) == 0); same(); CHECK(g_live[a].bytes == 12);
    CHECK(s.get(&b, 0) == 0); same(); CHECK(b != nullptr && g_live[b].bytes == 8);      // the max(n, 1) rule: room for one element
    CHECK(s.get_pinned(&h, 5, 7u) == 0); same(); CHECK(g_live[h].pinned && g_live[h].bytes == 20 && g_last_flags == 7u);
    CHECK(s.get(&c, 100) == 0); same(); CHECK(!g_live[c].pinned);
    CHECK(s.get(&d, 2) == 0); same();
    CHECK(g_live.size() == 5 && !s.failed);
    const std::vector<void*> order = g_alloced;
    s.release(); same();
    CHECK(g_live.empty() && s.blocks.empty());
    CHECK(g_freed.size() == 5);                          // each block exactly once ...
    for (size_t i = 0; i < g_freed.size() && i < order.size(); i++) CHECK(g_freed[i] == order[order.size() - 1 - i]);      // ... newest first
    s.release(); same(); CHECK(g_freed.size() == 5);     // an empty scope releases nothing
}
static void test_drop_then_release() {
    reset_log(); DevScope s;
    float *a = nullptr, *b = nullptr, *c = nullptr;
    CHECK(!s.get(&a, 4) && !s.get(&b, 4) && !s.get(&c, 4)); same();
    float* alias = a + 1;                                // assigned, never registered
    s.drop(b); same(); CHECK(g_freed.size() == 1 && g_freed[0] == (void*)b);
    s.drop(b); s.drop(nullptr); s.drop(alias); same(); CHECK(g_freed.size() == 1);      // not held: nothing happens
    s.release(); same();
    CHECK(g_freed.size() == 3 && g_freed[1] == (void*)c && g_freed[2] == (void*)a);      // b is not freed twice
    CHECK(g_live.empty());
}
static void test_grow() {
    reset_log(); DevScope s; float* p = nullptr; size_t cap = 0;
    CHECK(grow(s, &p, &cap, 10, 256) == 0); same();
    CHECK(cap == 256 && p && g_live.size() == 1 && g_live[p].bytes == 256 * sizeof(float));      // max(floor, 2 * need)
    float* p0 = p; const int req0 = g_req;
    CHECK(grow(s, &p, &cap, 200, 256) == 0); same(); CHECK(p == p0 && cap == 256 && g_req == req0);      // need <= cap: the block is kept
    CHECK(grow(s, &p, &cap, 256, 256) == 0); same(); CHECK(p == p0 && cap == 256 && g_req == req0);
    CHECK(grow(s, &p, &cap, 300, 256) == 0); same();
    CHECK(cap == 600 && g_live.size() == 1 && g_live.count(p) && g_live[p].bytes == 600 * sizeof(float));      // exactly one live block, of 2 * need
    CHECK(g_freed.size() == 1 && g_freed[0] == (void*)p0);
    double* q = nullptr; size_t qcap = 0;
    CHECK(grow(s, &q, &qcap, 5, 0) == 0); same(); CHECK(qcap == 10 && g_live[q].bytes == 80);
    g_fail_at = g_req + 1;                               // a refused regrow: the old block is gone, the pointer null, the cap 0, the latch set
    CHECK(grow(s, &q, &qcap, 11, 0) == -1); same(); CHECK(q == nullptr && qcap == 0 && s.failed && g_live.size() == 1);
    s.release(); same(); CHECK(g_live.empty() && !s.failed);
}
// a builder that allocates N blocks and tests the latch once at its end
static const int N_BUILD = 6;
static int build(DevScope& s, void** out /* [N_BUILD] */, size_t* cap) {
    float* a = nullptr; int* b = nullptr; unsigned* h = nullptr; char* c = nullptr; float* g = nullptr; double* d = nullptr;
    s.get(&a, 7); same(); s.get(&b, 1); same(); s.get_pinned(&h, 3, 0); same(); s.get(&c, 33); same(); grow(s, &g, cap, 9, 4); same(); s.get(&d, 2); same();
    out[0] = a; out[1] = b; out[2] = h; out[3] = c; out[4] = g; out[5] = d;
    return s.failed ? -1 : 0;
}
static void test_failure_at_every_request() {
    const size_t blocks0 = g_devmem_blocks.load(), bytes0 = g_devmem_bytes.load();
    for (int k = 0; k <= N_BUILD; k++) {                 // k = 0: nothing is refused
        reset_log(); g_fail_at = k; g_msg[0] = 0;
        DevScope s; void* out[N_BUILD]; size_t cap = 0;
        const int rc = build(s, out, &cap);
        CHECK(g_req == N_BUILD);                         // the builder went on: later requests were served
        CHECK(rc == (k ? -1 : 0) && s.failed == (k != 0));
        for (int i = 0; i < N_BUILD; i++) CHECK((out[i] == nullptr) == (i + 1 == k));      // *p == nullptr for the refused request, and only for it
        if (k) { CHECK(strstr(g_msg, "bytes failed: out of memory (test)") != nullptr); CHECK(strstr(g_msg, k == 3 ? "hipHostMalloc of" : "hipMalloc of") == g_msg); }
        if (k == 5) CHECK(cap == 0);
        CHECK(g_live.size() == (size_t)(k ? N_BUILD - 1 : N_BUILD));
        s.release(); same();
        CHECK(g_live.empty() && !s.failed);
        CHECK(g_devmem_blocks.load() == blocks0 && g_devmem_bytes.load() == bytes0);      // back at the starting values
    }
}
static void test_two_scopes_share_the_counters() {
    reset_log(); DevScope s, t; float *a = nullptr, *b = nullptr;
    CHECK(!s.get(&a, 10) && !t.get(&b, 20)); same(); CHECK(g_devmem_blocks.load() == 2);
    s.release(); same(); CHECK(g_live.count(b) == 1 && g_devmem_blocks.load() == 1);
    t.drop(b); same(); CHECK(t.blocks.empty());
}

int main() {
    test_release_order();
    test_drop_then_release();
    test_grow();
    test_failure_at_every_request();
    test_two_scopes_share_the_counters();
    CHECK(g_devmem_blocks.load() == 0 && g_devmem_bytes.load() == 0 && g_live.empty());
    if (g_errors) { fprintf(stderr, "devmem: %d check(s) failed\n", g_errors); return 1; }
    printf("devmem OK\n");
    return 0;
}
