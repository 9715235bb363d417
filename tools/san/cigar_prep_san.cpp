// cigar_prep_san.cpp -- bm2_cigar_prep (cigar_prep.cpp: the CIGAR batch prepared on the host, the oracle of cgprep.hip) under
// AddressSanitizer and UBSan, stand-alone: TEST INFRASTRUCTURE.  Built by tests/test_cigar_prep_sanitizer.py together with cigar_prep.cpp:
//     c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread tools/san/cigar_prep_san.cpp bwa-mem2_amd/csrc/cigar_prep.cpp
// It reads the batches tests/cigar_prep_cases.py dumps (dump_tasks), prepares each with 1 and with 4 host threads into arrays of exactly
// n entries, and checks what holds for any input: both runs give the same bytes, order is a permutation, the four slice offsets start at
// 0 and never decrease, the totals close them, every z_off is a multiple of 4, the shape counts sum to n.  A task that names a read that
// does not exist is refused and leaves the arrays as they were.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/bm2.h"
#include "../../bwa-mem2_amd/csrc/host_pool.h"

static char g_err[512];
void bm2_set_error(const char *fmt, ...) {                      // (the library's lives in bm2_api.hip)
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
}
extern "C" const char *bm2_last_error(void) { return g_err; }

static void need(bool ok, const char *what, long long a = 0, long long b = 0) {
    if (ok) return;
    fprintf(stderr, "cigar_prep_san: %s (%lld, %lld)\n", what, a, b);
    exit(1);
}
template <class T> static void get(FILE *f, T *p, size_t n) { need(fread(p, sizeof(T), n, f) == n, "short read"); }

int main(int argc, char **argv) {
    need(argc == 2, "usage: cigar_prep_san DUMP");
    FILE *f = fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the dump");
    int64_t head[5];
    get(f, head, 5);                                             // batches, sizeof(bm2_opt), and the sizes of the three records
    need(head[1] == (int64_t)sizeof(bm2_opt) && head[2] == (int64_t)sizeof(bm2_cigar_hit_t) && head[3] == (int64_t)sizeof(bm2_cigar_task_t) &&
         head[4] == (int64_t)sizeof(bm2_cigar_prep_t), "the dump's structs are not this build's", head[1], head[2]);
    long long tasks_seen = 0;
    for (int64_t s = 0; s < head[0]; ++s) {
        bm2_opt opt;
        get(f, &opt, 1);
        int64_t dims[3];
        get(f, dims, 3);                                         // l_pac, reads, tasks
        const int32_t n_reads = (int32_t)dims[1], n = (int32_t)dims[2];
        std::vector<int64_t> off((size_t)n_reads); std::vector<int32_t> len((size_t)n_reads);
        get(f, off.data(), off.size()); get(f, len.data(), len.size());
        std::vector<bm2_cigar_hit_t> hits((size_t)n);            // (exactly n of everything: one past is the sanitizer's to catch)
        get(f, hits.data(), hits.size());
        const bm2_reads reads = { n_reads, nullptr, off.data(), len.data() };
        std::vector<bm2_cigar_task_t> ta((size_t)n), tb((size_t)n);
        std::vector<int32_t> oa((size_t)n), ob((size_t)n);
        bm2_cigar_prep_t pa, pb;
        bm2_host_thread_budget() = 1;
        need(bm2_cigar_prep(&opt, dims[0], &reads, n, hits.data(), ta.data(), oa.data(), &pa) == BM2_OK, g_err);
        bm2_host_thread_budget() = 4;
        need(bm2_cigar_prep(&opt, dims[0], &reads, n, hits.data(), tb.data(), ob.data(), &pb) == BM2_OK, g_err);
        need(memcmp(ta.data(), tb.data(), (size_t)n * sizeof(bm2_cigar_task_t)) == 0 && oa == ob && memcmp(&pa, &pb, sizeof pa) == 0, "1 thread and 4 threads differ", s);
        std::vector<int32_t> seen = oa;
        std::sort(seen.begin(), seen.end());
        for (int32_t i = 0; i < n; ++i) need(seen[(size_t)i] == i, "order is no permutation", s, i);
        for (int32_t i = 0; i < n; ++i) {
            const bm2_cigar_task_t &T = ta[(size_t)i];
            need(T.z_off % 4 == 0, "z_off is no multiple of 4", s, i);
            need(T.q_off == off[(size_t)hits[(size_t)i].read] + hits[(size_t)i].qb && T.q_len == hits[(size_t)i].qe - hits[(size_t)i].qb, "q_off / q_len", s, i);
            const bm2_cigar_task_t *N = i + 1 < n ? &ta[(size_t)i + 1] : nullptr;
            need(i > 0 || (T.z_off == 0 && T.eh_off == 0 && T.cg_off == 0 && T.md_off == 0), "the slices do not start at 0", s);
            need((N ? N->z_off : pa.z_bytes) >= T.z_off && (N ? N->eh_off : pa.eh_items) >= T.eh_off && (N ? N->cg_off : pa.cg_items) >= T.cg_off &&
                 (N ? N->md_off : pa.md_bytes) >= T.md_off, "a slice offset decreases", s, i);
        }
        need((int64_t)pa.n_shape[0] + pa.n_shape[1] + pa.n_shape[2] + pa.n_shape[3] == n, "the shape counts do not sum to n", s);
        if (n > 2) {                                             // a read that does not exist: refused, the lowest offender named, nothing touched
            std::vector<bm2_cigar_hit_t> bad = hits;
            bad[(size_t)n - 1].read = n_reads; bad[(size_t)n / 2].read = -1;
            std::vector<bm2_cigar_task_t> tc = ta; std::vector<int32_t> oc = oa; bm2_cigar_prep_t pc = pa;
            need(bm2_cigar_prep(&opt, dims[0], &reads, n, bad.data(), tc.data(), oc.data(), &pc) == BM2_EINVAL, "a read that does not exist was accepted", s);
            char want[64];
            snprintf(want, sizeof want, "task %d ", n / 2);
            need(strstr(g_err, want) != nullptr, "the lowest offender is not the one named", s, n / 2);
            need(memcmp(tc.data(), ta.data(), (size_t)n * sizeof(bm2_cigar_task_t)) == 0 && oc == oa && memcmp(&pc, &pa, sizeof pa) == 0, "a refused call wrote", s);
        }
        tasks_seen += n;
    }
    fclose(f);
    printf("ok %lld batches %lld tasks\n", (long long)head[0], tasks_seen);
    return 0;
}
