// Checks of the part fan-out of bwa-mem2_amd/csrc/host_pool.h (built and run by tests/test_host_parts.py): the parts rule against the
// expression the hooks used to write out, the part bounds, which thread runs which part with which host-thread budget, whose error is
// reported and under what prefix.  Prints "ok" or the first failed check.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <condition_variable>
#include <mutex>
#include <set>
#include "host_pool.h"

static thread_local char g_err[512] = "";                         // (as bm2_api.hip keeps it)
void bm2_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); }
extern "C" const char *bm2_last_error(void) { return g_err; }

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

static int check_parts_rule() {
    const int64_t ns[] = { 0, 1, 8191, 8192, 8193, 65535, 65536, 65537, 131072, 2147483647 }, mins[] = { -1, 0, 1, 16, 8192, 65536 };
    const int ctxs[] = { 1, 2, 3, 8 };
    for (int64_t n : ns) for (int64_t part_min : mins) for (int n_ctx : ctxs) {
        int G = (int)(n / (part_min > 0 ? part_min : 1) + 1 < n_ctx ? n / (part_min > 0 ? part_min : 1) + 1 : n_ctx);      // the hooks' expression, literally
        if (G < 1) G = 1;
        CHECK(bm2_parts(n, part_min, n_ctx) == G, "n %lld part_min %lld n_ctx %d: %d, expected %d", (long long)n, (long long)part_min, n_ctx, bm2_parts(n, part_min, n_ctx), G);
    }
    return 0;
}

static int check_part_bounds() {
    const int64_t ns[] = { 0, 1, 7, 2147483647 };
    for (int64_t n : ns) for (int G : { 1, 2, 3, 8 }) {
        CHECK(bm2_part_lo(n, 0, G) == 0 && bm2_part_lo(n, G, G) == n, "n %lld G %d: ends %lld %lld", (long long)n, G, (long long)bm2_part_lo(n, 0, G), (long long)bm2_part_lo(n, G, G));
        for (int g = 0; g < G; ++g) CHECK(bm2_part_lo(n, g, G) <= bm2_part_lo(n, g + 1, G), "n %lld G %d: part %d runs backwards", (long long)n, G, g);
    }
    CHECK(bm2_part_lo(2147483647, 7, 8) == 1879048191, "2^31 - 1 in 8 parts: part 7 starts at %lld", (long long)bm2_part_lo(2147483647, 7, 8));
    return 0;
}

// every g once, part 0 on the caller's thread and the others on G - 1 distinct other threads, the budgets as promised
static int check_fan_out(int G, int budget) {
    bm2_host_thread_budget() = 3;
    std::vector<int> calls((size_t)G, 0), seen((size_t)G, -1);
    std::vector<std::thread::id> who((size_t)G);
    const int rc = bm2_run_parts(G, budget, "context", [&](int g) {
        ++calls[(size_t)g]; who[(size_t)g] = std::this_thread::get_id(); seen[(size_t)g] = bm2_host_thread_budget();
        return 0;
    });
    CHECK(rc == 0, "G %d budget %d: rc %d", G, budget, rc);
    std::set<std::thread::id> others;
    for (int g = 0; g < G; ++g) {
        CHECK(calls[(size_t)g] == 1, "G %d: part %d ran %d times", G, g, calls[(size_t)g]);
        const int want = budget > 0 ? budget : g == 0 ? 3 : 0;
        CHECK(seen[(size_t)g] == want, "G %d budget %d: part %d read a budget of %d, expected %d", G, budget, g, seen[(size_t)g], want);
        if (g > 0) others.insert(who[(size_t)g]);
    }
    CHECK(who[0] == std::this_thread::get_id(), "G %d: part 0 ran on another thread", G);
    CHECK((int)others.size() == G - 1 && !others.count(std::this_thread::get_id()), "G %d: parts 1.. ran on %d other threads", G, (int)others.size());
    CHECK(bm2_host_thread_budget() == 3, "G %d budget %d: the caller's budget came back as %d", G, budget, bm2_host_thread_budget());
    return 0;
}

// parts 2 and 5 fail, 5 first (part 2 waits for it); part 3 succeeds after setting a message of its own
static int check_errors(const char *label, const char *expect) {
    std::mutex m; std::condition_variable cv; bool five_done = false;
    bm2_host_thread_budget() = 3;
    bm2_set_error("stale");
    const int rc = bm2_run_parts(8, 5, label, [&](int g) {
        if (g == 5) {
            bm2_set_error("five");
            { std::lock_guard<std::mutex> l(m); five_done = true; }
            cv.notify_all();
            return 55;
        }
        if (g == 2) {
            std::unique_lock<std::mutex> l(m); cv.wait(l, [&]() { return five_done; });
            bm2_set_error("two");
            return 22;
        }
        if (g == 3) bm2_set_error("three, but fine");
        return 0;
    });
    CHECK(rc == 22, "label %s: rc %d", label ? label : "(null)", rc);
    CHECK(!strcmp(bm2_last_error(), expect), "label %s: text \"%s\", expected \"%s\"", label ? label : "(null)", bm2_last_error(), expect);
    CHECK(bm2_host_thread_budget() == 3, "the caller's budget came back as %d after a failure", bm2_host_thread_budget());
    return 0;
}

int main() {
    if (check_parts_rule() || check_part_bounds()) return 1;
    for (int G : { 1, 2, 3, 8 }) if (check_fan_out(G, 5) || check_fan_out(G, 0)) return 1;
    if (check_errors("context", "context 2: two") || check_errors(nullptr, "two")) return 1;
    const int rc = bm2_run_parts(1, 0, "context", [](int) { bm2_set_error("alone"); return 7; });
    CHECK(rc == 7 && !strcmp(bm2_last_error(), "context 0: alone"), "one failing part: rc %d, text \"%s\"", rc, bm2_last_error());
    for (int round = 0; round < 2000; ++round) {                  // joins and restores, over and over
        std::atomic<int> ran(0);
        bm2_host_thread_budget() = 1 + round % 7;
        const int r = bm2_run_parts(8, 2, nullptr, [&](int g) { ran += g + 1; return bm2_host_thread_budget() == 2 ? 0 : 1; });
        CHECK(r == 0 && ran.load() == 36 && bm2_host_thread_budget() == 1 + round % 7, "round %d: rc %d, parts %d, budget %d", round, r, ran.load(), bm2_host_thread_budget());
    }
    printf("ok\n");
    return 0;
}
