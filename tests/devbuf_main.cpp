// devbuf_main.cpp -- rr::DevBuf (river_route_amd/csrc/rr_devbuf.hpp) over a fake device: the two memory functions the header only
// declares are malloc / free here, with a count of the blocks alive and a flag that refuses the next allocation.  Built with
// -fsanitize=address,undefined and run by tests/test_devbuf.py: a double free, a leak or a use after a move ends the run.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "rr_devbuf.hpp"

static int64_t g_live = 0, g_made = 0, g_live_at_last_alloc = -1;
static bool g_fail_next = false;

namespace rr {
int dev_mem_alloc(void **p, size_t bytes)
{
    *p = nullptr;
    g_live_at_last_alloc = g_live;
    if (g_fail_next) { g_fail_next = false; return -6; }
    *p = std::malloc(bytes);
    if (!*p) return -6;
    ++g_live; ++g_made;
    return 0;
}
void dev_mem_free(void *p)
{
    if (!p) return;
    std::free(p);
    --g_live;
}
}  // namespace rr

using rr::DevBuf;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++g_failures; } } while (0)

int main()
{
    {   // empty by default; the destructor frees
        DevBuf<double> a;
        CHECK(a.get() == nullptr && a.count() == 0 && !a && g_live == 0);
        {
            DevBuf<double> b;
            CHECK(b.alloc(10) == 0 && b.count() == 10 && b.get() != nullptr && g_live == 1);
            double *raw = b;      // the implicit conversion
            CHECK(raw == b.get());
            raw[9] = 1.0;         // ten elements are there (the sanitizer checks)
        }
        CHECK(g_live == 0);
    }
    {   // move construction, move assignment (onto an empty and onto a non-empty buffer), self-move
        DevBuf<int> a;
        CHECK(a.alloc(4) == 0);
        int *pa = a.get();
        DevBuf<int> b(std::move(a));
        CHECK(a.get() == nullptr && a.count() == 0 && b.get() == pa && b.count() == 4 && g_live == 1);
        DevBuf<int> c;
        c = std::move(b);
        CHECK(b.get() == nullptr && b.count() == 0 && c.get() == pa && c.count() == 4 && g_live == 1);
        DevBuf<int> d;
        CHECK(d.alloc(7) == 0 && g_live == 2);
        d = std::move(c);      // d's old block goes
        CHECK(g_live == 1 && d.get() == pa && d.count() == 4 && c.get() == nullptr && c.count() == 0);
        DevBuf<int> &self = d;
        d = std::move(self);
        CHECK(g_live == 1 && d.get() == pa && d.count() == 4);
        d.reset();
        CHECK(g_live == 0 && d.get() == nullptr && d.count() == 0);
        d.reset();             // twice is harmless
        CHECK(g_live == 0);
    }
    {   // alloc over a live block: the old block is gone BEFORE the new one is asked for
        DevBuf<double> a;
        CHECK(a.alloc(100) == 0 && g_live == 1);
        CHECK(a.alloc(200) == 0 && g_live == 1 && a.count() == 200);
        CHECK(g_live_at_last_alloc == 0);
        a.get()[199] = 2.0;
    }
    CHECK(g_live == 0);
    {   // reserve: nothing at sufficient capacity, a new block above it (released first, as alloc does)
        DevBuf<double> a;
        CHECK(a.reserve(0) == 0 && a.get() == nullptr && a.count() == 0);      // nothing asked for, nothing there
        CHECK(a.reserve(50) == 0 && a.count() == 50);
        double *p = a.get();
        const int64_t made = g_made;
        CHECK(a.reserve(50) == 0 && a.reserve(20) == 0 && a.reserve(0) == 0 && a.get() == p && a.count() == 50 && g_made == made);
        CHECK(a.reserve(51) == 0 && a.count() == 51 && g_made == made + 1 && g_live == 1 && g_live_at_last_alloc == 0);
        a.get()[50] = 3.0;
    }
    CHECK(g_live == 0);
    {   // a refused allocation leaves the buffer empty -- also one that held a block
        DevBuf<double> a;
        g_fail_next = true;
        CHECK(a.alloc(8) != 0 && a.get() == nullptr && a.count() == 0 && g_live == 0);
        CHECK(a.alloc(8) == 0 && g_live == 1);
        g_fail_next = true;
        CHECK(a.alloc(16) != 0 && a.get() == nullptr && a.count() == 0 && g_live == 0);
        g_fail_next = true;
        CHECK(a.reserve(4) != 0 && a.count() == 0 && g_live == 0);
        CHECK(a.reserve(4) == 0 && a.count() == 4 && g_live == 1);
    }
    CHECK(g_live == 0);
    {   // count <= 0: one element
        DevBuf<double> a, b;
        CHECK(a.alloc(0) == 0 && a.count() == 1 && a.get() != nullptr);
        CHECK(b.alloc(-5) == 0 && b.count() == 1 && b.get() != nullptr);
        a.get()[0] = b.get()[0] = 4.0;
        CHECK(g_live == 2);
    }
    CHECK(g_live == 0);
    {   // an array of two, and a vector that grows (its elements move)
        DevBuf<int> pair[2];
        CHECK(pair[0].alloc(3) == 0 && pair[1].alloc(5) == 0 && g_live == 2);
        std::swap(pair[0], pair[1]);
        CHECK(pair[0].count() == 5 && pair[1].count() == 3 && g_live == 2);
        std::vector<DevBuf<double>> v;
        for (int k = 0; k < 40; ++k) {
            v.emplace_back();
            CHECK(v.back().alloc(k + 1) == 0);
            v.back().get()[k] = (double)k;
        }
        CHECK(g_live == 42);
        bool kept = true;
        for (int k = 0; k < 40; ++k) kept = kept && v[k].count() == k + 1 && v[k].get()[k] == (double)k;
        CHECK(kept);
        v.erase(v.begin() + 3);
        CHECK(g_live == 41 && v[3].count() == 5);
        v.resize(10);
        CHECK(g_live == 12);
    }
    CHECK(g_live == 0);
    std::printf("allocations %lld live %lld failures %d\n", (long long)g_made, (long long)g_live, g_failures);
    return g_failures == 0 && g_live == 0 ? 0 : 1;
}
