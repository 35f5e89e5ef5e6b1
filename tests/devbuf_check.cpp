// devbuf_check.cpp -- DevBuf (csrc/devbuf.h) against a cache of this program's own: genphi::cached_malloc / cached_free are defined
// here on host malloc, with a table of the live blocks and a switch that fails the k-th allocation.  No GPU, no HIP runtime: the header
// only needs hipError_t.  tests/test_devbuf_host.py builds and runs it, plain and under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>

#include "../genlib.jl_amd/csrc/devbuf.h"

namespace {
std::map<void *, size_t> g_live;       // block -> bytes asked for
long g_allocs = 0, g_frees = 0, g_bad_frees = 0;
long g_fail_at = 0;                    // > 0: the allocation with this number (counted from the last arming) fails
long g_since_armed = 0;
int g_violations = 0, g_checks = 0;

void fail_allocation(long k) { g_fail_at = k; g_since_armed = 0; }

void check(bool ok, const char *what, int line)
{
    ++g_checks;
    if (!ok) { ++g_violations; std::fprintf(stderr, "VIOLATION line %d: %s\n", line, what); }
}
#define CHECK(cond) check((cond), #cond, __LINE__)
}  // namespace

namespace genphi {
hipError_t cached_malloc(void **ptr, size_t bytes)
{
    *ptr = nullptr;
    if (g_fail_at > 0 && ++g_since_armed == g_fail_at) return hipErrorOutOfMemory;
    if (bytes == 0) { ++g_violations; std::fprintf(stderr, "VIOLATION: an allocation of 0 bytes\n"); return hipErrorInvalidValue; }
    void *q = std::malloc(bytes);
    if (!q) return hipErrorOutOfMemory;
    g_live[q] = bytes;
    ++g_allocs;
    *ptr = q;
    return hipSuccess;
}
hipError_t cached_free(void *ptr)
{
    if (!ptr) return hipSuccess;
    auto it = g_live.find(ptr);
    if (it == g_live.end()) { ++g_bad_frees; return hipErrorInvalidValue; }      // a double free, or a pointer that was never handed out
    g_live.erase(it);
    ++g_frees;
    std::free(ptr);
    return hipSuccess;
}
}  // namespace genphi

using genphi::DevBuf;

static void grows_and_never_shrinks()
{
    DevBuf<float> b;
    CHECK(b.get() == nullptr && b.count() == 0 && b.bytes() == 0);
    CHECK(b.reserve(100) == hipSuccess);
    float *first = b.get();
    CHECK(first != nullptr && b.count() == 100 && b.bytes() == 400 && g_live[first] == 400);
    for (size_t i = 0; i < 100; ++i) first[i] = 1.0f;      // (the sanitizer build checks the block's extent)
    const long allocs = g_allocs;
    CHECK(b.reserve(40) == hipSuccess && b.get() == first && b.count() == 100);      // smaller: kept, the count too
    CHECK(b.reserve(100) == hipSuccess && b.get() == first && g_allocs == allocs);
    CHECK(b.reserve(0) == hipSuccess && b.get() == first && b.count() == 100);
    const long frees = g_frees;
    CHECK(b.reserve(101) == hipSuccess && b.count() == 101 && g_allocs == allocs + 1 && g_frees == frees + 1);
    CHECK(g_live.size() == 1 && g_live.count(b.get()) == 1 && g_live[b.get()] == 404);
    float *as_pointer = b;                                  // reads like the raw pointer
    CHECK(as_pointer == b.get() && b + 1 == b.get() + 1);
}

static void a_request_of_zero()
{
    DevBuf<double> b;
    CHECK(b.reserve(0) == hipSuccess);
    CHECK(b.get() != nullptr && b.count() == 0 && b.bytes() == 0);      // a pointer, and the count is the request
    CHECK(g_live.size() == 1 && g_live[b.get()] == sizeof(double));
    double *p = b.get();
    CHECK(b.reserve(0) == hipSuccess && b.get() == p);
    CHECK(b.reserve(3) == hipSuccess && b.count() == 3 && b.bytes() == 24);
}

// The d_perm_rows case: a failed growth must not leave a capacity behind that a later, smaller request trusts.
static void a_failed_reserve_leaves_nothing()
{
    DevBuf<int> b;
    CHECK(b.reserve(50) == hipSuccess);
    fail_allocation(1);
    CHECK(b.reserve(80) == hipErrorOutOfMemory);
    CHECK(b.get() == nullptr && b.count() == 0 && b.bytes() == 0 && g_live.empty());
    const long allocs = g_allocs;
    CHECK(b.reserve(20) == hipSuccess);                     // fewer than ever held: allocates again
    CHECK(b.get() != nullptr && b.count() == 20 && g_allocs == allocs + 1 && g_live[b.get()] == 80);
    for (int i = 0; i < 20; ++i) b.get()[i] = i;
    // the k-th allocation of a sequence: the ones before it stand, the one after it is served
    DevBuf<int> c, d, e;
    fail_allocation(2);
    CHECK(c.reserve(1) == hipSuccess && d.reserve(1) == hipErrorOutOfMemory && e.reserve(1) == hipSuccess);
    CHECK(c.get() && !d.get() && d.count() == 0 && e.get());
    fail_allocation(0);
    // an empty buffer whose first allocation fails
    DevBuf<char> f;
    fail_allocation(1);
    CHECK(f.reserve(7) == hipErrorOutOfMemory && f.get() == nullptr && f.count() == 0);
    fail_allocation(0);
}

static void release_is_idempotent()
{
    DevBuf<char> b;
    b.release();
    CHECK(b.get() == nullptr && b.count() == 0);
    CHECK(b.reserve(9) == hipSuccess);
    const long frees = g_frees;
    b.release();
    CHECK(b.get() == nullptr && b.count() == 0 && g_frees == frees + 1 && g_live.empty());
    b.release();
    CHECK(g_frees == frees + 1 && g_bad_frees == 0);
    CHECK(b.reserve(2) == hipSuccess && b.count() == 2);    // usable again
}

static void moves()
{
    DevBuf<float> a;
    CHECK(a.reserve(10) == hipSuccess);
    float *pa = a.get();
    DevBuf<float> b(std::move(a));                          // construction: the source is empty, nothing is freed
    CHECK(a.get() == nullptr && a.count() == 0 && b.get() == pa && b.count() == 10 && g_live.size() == 1);
    DevBuf<float> c;
    CHECK(c.reserve(5) == hipSuccess);
    float *pc = c.get();
    const long frees = g_frees;
    c = std::move(b);                                       // assignment: the destination's old block is freed, once
    CHECK(g_frees == frees + 1 && g_live.count(pc) == 0 && g_live.count(pa) == 1);
    CHECK(b.get() == nullptr && b.count() == 0 && c.get() == pa && c.count() == 10);
    DevBuf<float> &self = c;
    c = std::move(self);                                    // onto itself: nothing happens
    CHECK(c.get() == pa && c.count() == 10 && g_frees == frees + 1);
    c = DevBuf<float>();                                    // what releasing a plan's device state does to every buffer
    CHECK(c.get() == nullptr && c.count() == 0 && g_frees == frees + 2 && g_live.empty());
    // grow by "allocate the new block, copy, drop the old one" (the row-list arenas): both alive until the assignment
    DevBuf<int> arena, larger;
    CHECK(arena.reserve(4) == hipSuccess && larger.reserve(8) == hipSuccess && g_live.size() == 2);
    for (int i = 0; i < 4; ++i) arena.get()[i] = i;
    for (int i = 0; i < 4; ++i) larger.get()[i] = arena.get()[i];
    arena = std::move(larger);
    CHECK(arena.count() == 8 && arena.get()[3] == 3 && g_live.size() == 1);
    // an array of buffers resets member by member
    struct State { DevBuf<float> buf[2]; DevBuf<char> blob; int n = 0; } s;
    CHECK(s.buf[0].reserve(3) == hipSuccess && s.buf[1].reserve(4) == hipSuccess && s.blob.reserve(5) == hipSuccess);
    s.n = 7;
    s = State();
    CHECK(!s.buf[0].get() && !s.buf[1].get() && !s.blob.get() && s.n == 0 && g_live.size() == 1);      // (`arena` is still alive)
}

int main()
{
    grows_and_never_shrinks();
    CHECK(g_live.empty());                                  // every destructor gave its block back
    a_request_of_zero();
    CHECK(g_live.empty());
    a_failed_reserve_leaves_nothing();
    CHECK(g_live.empty());
    release_is_idempotent();
    CHECK(g_live.empty());
    moves();
    CHECK(g_live.empty() && g_bad_frees == 0 && g_allocs == g_frees);
    std::printf("devbuf check: %d checks, %ld allocations, %ld frees, %ld bad frees, %zu live blocks; %d violations\n", g_checks, g_allocs, g_frees,
                g_bad_frees, g_live.size(), g_violations);
    return (g_violations || g_bad_frees || !g_live.empty()) ? 1 : 0;
}
