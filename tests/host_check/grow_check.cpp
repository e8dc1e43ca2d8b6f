// grow_check.cpp -- csrc/rg_grow.h over malloc / free, a stand-alone program (tests/test_grow_host.py builds it plainly and with
// -fsanitize=address,undefined and runs it directly). The allocator counts what lives and can be told to fail its k-th call from
// now; the sanitizers see the rest: a write past the padding, a double free, a leak.
#include "rg_grow.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

static std::set<void *> g_live;
static int g_fail_in = 0;  // 1: the next allocation fails, 2: the one after it, 0: none
static int g_allocs = 0, g_syncs = 0;
static size_t g_last_bytes = 0;

static int t_alloc(void **p, size_t bytes) {
    if (g_fail_in && --g_fail_in == 0) {
        *p = nullptr;
        return 2; // (any non-zero code: it must come back unchanged)
    }
    *p = malloc(bytes);
    g_live.insert(*p);
    g_allocs++;
    g_last_bytes = bytes;
    return 0;
}
static void t_free(void *p) {
    if (!g_live.erase(p)) {
        fprintf(stderr, "free of a pointer that is not live\n");
        abort();
    }
    free(p);
}
static int t_sync() {
    g_syncs++;
    return 0;
}

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
            return 1;                                                 \
        }                                                             \
    } while (0)

struct Elem { char b[24]; };
static const uint64_t FIRST = 16;
static const size_t PAD = 40;

static int grow(Elem **p, uint64_t *cap, uint64_t need) { return rg_grow(p, cap, need, FIRST, sizeof(Elem), PAD, t_alloc, t_free, t_sync); }
static int grow2(char **a, char **b, uint64_t *cap, uint64_t need) {
    return rg_grow_pair(a, b, cap, need, FIRST, sizeof(Elem), PAD, t_alloc, t_free, t_alloc, t_free, t_sync);
}

static int check_single() {
    Elem *p = nullptr;
    uint64_t cap = 0;
    // need = first - 1, first, first + 1, 4 * first + 1 -> 1x, 1x (no reallocation), 2x, 8x
    CHECK(grow(&p, &cap, FIRST - 1) == 0 && p && cap == FIRST && g_allocs == 1 && g_syncs == 0); // (no old buffer: no hook)
    CHECK(g_last_bytes == FIRST * sizeof(Elem) + PAD);
    Elem *p0 = p;
    CHECK(grow(&p, &cap, FIRST) == 0 && p == p0 && cap == FIRST && g_allocs == 1 && g_syncs == 0);
    CHECK(grow(&p, &cap, 0) == 0 && p == p0 && cap == FIRST && g_allocs == 1);
    CHECK(grow(&p, &cap, FIRST + 1) == 0 && p && cap == 2 * FIRST && g_allocs == 2 && g_syncs == 1 && g_live.size() == 1);
    reinterpret_cast<char *>(p)[cap * sizeof(Elem) + PAD - 1] = 1; // the padding is really there (ASan)
    CHECK(grow(&p, &cap, 4 * FIRST + 1) == 0 && p && cap == 8 * FIRST && g_allocs == 3 && g_syncs == 2 && g_live.size() == 1);
    CHECK(g_last_bytes == 8 * FIRST * sizeof(Elem) + PAD);
    reinterpret_cast<char *>(p)[cap * sizeof(Elem) + PAD - 1] = 1;
    memset(p, 0, cap * sizeof(Elem) + PAD);
    // a failed regrowth: the old buffer is gone, (nullptr, 0), the allocator's code comes back
    g_fail_in = 1;
    CHECK(grow(&p, &cap, 8 * FIRST + 1) == 2 && !p && cap == 0 && g_live.empty() && g_syncs == 3);
    // ... a need that fitted the OLD capacity allocates again (it never meets the null pointer), and no hook: nothing to drain
    CHECK(grow(&p, &cap, 3) == 0 && p && cap == FIRST && g_live.size() == 1 && g_syncs == 3);
    t_free(p);
    // a failed first growth, then recovery
    p = nullptr;
    cap = 0;
    g_fail_in = 1;
    CHECK(grow(&p, &cap, 5) == 2 && !p && cap == 0 && g_live.empty());
    CHECK(grow(&p, &cap, 2 * FIRST) == 0 && p && cap == 2 * FIRST && g_live.size() == 1);
    t_free(p);
    CHECK(g_live.empty());
    return 0;
}

static int check_pair() {
    char *a = nullptr, *b = nullptr;
    uint64_t cap = 0;
    const int syncs0 = g_syncs;
    CHECK(grow2(&a, &b, &cap, 1) == 0 && a && b && a != b && cap == FIRST && g_live.size() == 2 && g_syncs == syncs0);
    a[cap * sizeof(Elem) + PAD - 1] = b[cap * sizeof(Elem) + PAD - 1] = 1;
    char *a0 = a, *b0 = b;
    CHECK(grow2(&a, &b, &cap, FIRST) == 0 && a == a0 && b == b0 && cap == FIRST);
    CHECK(grow2(&a, &b, &cap, 4 * FIRST + 1) == 0 && a && b && cap == 8 * FIRST && g_live.size() == 2 && g_syncs == syncs0 + 1);
    a[cap * sizeof(Elem) + PAD - 1] = b[cap * sizeof(Elem) + PAD - 1] = 1;
    // the SECOND allocation fails: the first one of this call is freed, and so were both old buffers
    g_fail_in = 2;
    CHECK(grow2(&a, &b, &cap, 8 * FIRST + 1) == 2 && !a && !b && cap == 0 && g_live.empty());
    // the first allocation fails, on first growth
    g_fail_in = 1;
    CHECK(grow2(&a, &b, &cap, 1) == 2 && !a && !b && cap == 0 && g_live.empty());
    CHECK(grow2(&a, &b, &cap, FIRST + 1) == 0 && a && b && cap == 2 * FIRST && g_live.size() == 2);
    t_free(a);
    t_free(b);
    CHECK(g_live.empty());
    return 0;
}

int main() {
    if (check_single() || check_pair()) return 1;
    printf("ok\n");
    return 0;
}
