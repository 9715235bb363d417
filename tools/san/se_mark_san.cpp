// se_mark_san.cpp -- bm2_se_mark (sam_tail.cpp: the single-end tail's decide step, the oracle of semark.hip) under AddressSanitizer and
// UBSan, stand-alone: TEST INFRASTRUCTURE.  Built by tests/test_se_mark_sanitizer.py together with sam_tail.cpp:
//     c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread tools/san/se_mark_san.cpp bwa-mem2_amd/csrc/sam_tail.cpp
// It reads the batches tests/se_mark_cases.py dumps (dump_lists), marks each in place with 1 and with 4 threads, with and without n_pri,
// and checks what holds for any input: both runs give the same bytes, every list is a permutation of itself (pad names a hit), n_pri
// counts the hits that are not on an ALT contig, secondary and secondary_all point into the list.  Offsets that decrease are refused.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/bm2.h"

static char g_err[512];
void bm2_set_error(const char *fmt, ...) {                      // (the library's lives in bm2_api.hip)
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
}

static void need(bool ok, const char *what, long long a = 0, long long b = 0) {
    if (ok) return;
    fprintf(stderr, "se_mark_san: %s (%lld, %lld)\n", what, a, b);
    exit(1);
}
template <class T> static void get(FILE *f, T *p, size_t n) { need(fread(p, sizeof(T), n, f) == n, "short read"); }

int main(int argc, char **argv) {
    need(argc == 2, "usage: se_mark_san DUMP");
    FILE *f = fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the dump");
    int64_t head[4];
    get(f, head, 4);                                             // batches, sizeof(bm2_opt), sizeof(bm2_sam_opt), sizeof(bm2_alnreg_t)
    need(head[1] == (int64_t)sizeof(bm2_opt) && head[2] == (int64_t)sizeof(bm2_sam_opt) && head[3] == (int64_t)sizeof(bm2_alnreg_t), "the dump's structs are not this build's", head[1], head[2]);
    long long lists_seen = 0, hits_seen = 0;
    for (int64_t s = 0; s < head[0]; ++s) {
        bm2_opt opt; bm2_sam_opt so;
        get(f, &opt, 1); get(f, &so, 1);
        so.rg_id = nullptr;
        int64_t dims[3];
        get(f, dims, 3);                                         // lists, first_id, hits in the array
        const int32_t n_lists = (int32_t)dims[0];
        std::vector<int64_t> off((size_t)n_lists + 1);
        get(f, off.data(), off.size());
        std::vector<bm2_alnreg_t> hits((size_t)dims[2]);         // (exactly as many as the offsets reach: one past is the sanitizer's to catch)
        if (dims[2]) get(f, hits.data(), hits.size());
        need(off[(size_t)n_lists] == dims[2], "the offsets do not end at the array's end", off[(size_t)n_lists], dims[2]);
        std::vector<bm2_alnreg_t> a = hits, b = hits;
        std::vector<int32_t> n_pri((size_t)n_lists + 1, -7);
        so.n_threads = 1;
        need(bm2_se_mark(&opt, &so, n_lists, a.data(), off.data(), dims[1], n_pri.data()) == BM2_OK, g_err);
        so.n_threads = 4;
        need(bm2_se_mark(&opt, &so, n_lists, b.data(), off.data(), dims[1], nullptr) == BM2_OK, g_err);
        need(a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(bm2_alnreg_t)) == 0), "1 thread and 4 threads differ", s);
        need(off[0] == 0 || memcmp(a.data(), hits.data(), (size_t)off[0] * sizeof(bm2_alnreg_t)) == 0, "hits before the first list were touched", s);
        for (int32_t li = 0; li < n_lists; ++li) {
            const int64_t lo = off[(size_t)li], n = off[(size_t)li + 1] - lo;
            std::vector<int32_t> was, is;
            int assembly = 0;
            for (int64_t k = 0; k < n; ++k) {
                was.push_back(hits[(size_t)(lo + k)].pad); is.push_back(a[(size_t)(lo + k)].pad);
                const bm2_alnreg_t &h = a[(size_t)(lo + k)];
                assembly += !h.is_alt;
                need(h.secondary < n || h.secondary == 0x7fffffff, "secondary points outside its list", s, li);
                need(h.secondary_all < n, "secondary_all points outside its list", s, li);
            }
            std::sort(was.begin(), was.end()); std::sort(is.begin(), is.end());
            need(was == is, "a list is no permutation of itself", s, li);
            need(n_pri[(size_t)li] == assembly, "n_pri", n_pri[(size_t)li], assembly);
        }
        need(n_pri[(size_t)n_lists] == -7, "n_pri written past its end", s);
        if (n_lists >= 2 && off[1] > off[0]) {                   // decreasing offsets: refused, nothing touched
            std::vector<int64_t> bad = off;
            bad[2] = bad[1] - 1;
            std::vector<bm2_alnreg_t> c = hits;
            need(bm2_se_mark(&opt, &so, n_lists, c.data(), bad.data(), dims[1], nullptr) == BM2_EINVAL, "decreasing offsets accepted", s);
            need(memcmp(c.data(), hits.data(), c.size() * sizeof(bm2_alnreg_t)) == 0, "a refused call touched the hits", s);
        }
        lists_seen += n_lists; hits_seen += dims[2];
    }
    fclose(f);
    printf("ok %lld batches %lld lists %lld hits\n", (long long)head[0], lists_seen, hits_seen);
    return 0;
}
