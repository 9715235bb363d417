// ksw_san.cpp -- bm2_ksw_align2 (sam_tail.cpp: the host twin of the mate-rescue Smith-Waterman, the oracle of matesw.hip) under AddressSanitizer
// and UBSan, stand-alone: TEST INFRASTRUCTURE.  Built by tests/test_ksw_sanitizer.py together with sam_tail.cpp:
//     c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread tools/san/ksw_san.cpp bwa-mem2_amd/csrc/sam_tail.cpp
// It reads the sets tests/tail_dp_cases.py dumps (dump_ksw: the hand-made tasks of every edge -- byte saturation with and without the start
// pass, KSW_XSTOP, empty and one-base targets, the list of local maxima at its capacity ...), aligns each set as one batch and once more
// task by task from exact-size private copies of the two sequences (a read one past either end is the sanitizer's to catch), checks that
// both give the same bytes and what holds for any input, and writes the results for the test to compare with the library's.  An empty query,
// a negative length and a gap extension of 0 are refused with nothing written.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/bm2.h"

static char g_err[512];
void bm2_set_error(const char *fmt, ...) {                      // (the library's lives in bm2_api.hip)
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
}

static void need(bool ok, const char *what, long long a = 0, long long b = 0) {
    if (ok) return;
    fprintf(stderr, "ksw_san: %s (%lld, %lld)\n", what, a, b);
    exit(1);
}
template <class T> static void get(FILE *f, T *p, size_t n) { need(n == 0 || fread(p, sizeof(T), n, f) == n, "short read"); }

enum { XBYTE = 0x10000, XSUBO = 0x40000, XSTART = 0x80000 };

int main(int argc, char **argv) {
    need(argc == 3, "usage: ksw_san DUMP OUT");
    FILE *f = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    need(f != nullptr && fo != nullptr, "cannot open the files");
    int64_t n_sets = 0;
    get(f, &n_sets, 1);
    long long tasks_seen = 0, saturated = 0;
    for (int64_t s = 0; s < n_sets; ++s) {
        int8_t mat[32]; int32_t gap[4]; int64_t dims[2];
        get(f, mat, 32); get(f, gap, 4); get(f, dims, 2);        // the matrix (25 + 7 pad), o_del e_del o_ins e_ins, tasks and sequence bytes
        const int32_t n = (int32_t)dims[0];
        std::vector<int64_t> q_off((size_t)n), t_off((size_t)n);
        std::vector<int32_t> q_len((size_t)n), t_len((size_t)n), xtra((size_t)n);
        get(f, q_off.data(), (size_t)n); get(f, t_off.data(), (size_t)n);
        get(f, q_len.data(), (size_t)n); get(f, t_len.data(), (size_t)n); get(f, xtra.data(), (size_t)n);
        std::vector<uint8_t> seqs((size_t)dims[1]);              // (exactly as many bytes as the offsets reach)
        get(f, seqs.data(), seqs.size());
        std::vector<bm2_ksw_result> all((size_t)n), one((size_t)n);
        need(bm2_ksw_align2(n, seqs.data(), q_off.data(), q_len.data(), t_off.data(), t_len.data(), xtra.data(), mat, gap[0], gap[1], gap[2], gap[3], all.data()) == BM2_OK, g_err);
        for (int32_t i = 0; i < n; ++i) {
            need(q_off[(size_t)i] + q_len[(size_t)i] <= dims[1] && t_off[(size_t)i] + t_len[(size_t)i] <= dims[1], "a task reaches past the sequences", s, i);
            std::vector<uint8_t> own(seqs.begin() + q_off[(size_t)i], seqs.begin() + q_off[(size_t)i] + q_len[(size_t)i]);      // query, then target, nothing after
            own.insert(own.end(), seqs.begin() + t_off[(size_t)i], seqs.begin() + t_off[(size_t)i] + t_len[(size_t)i]);
            const int64_t qo = 0, to = q_len[(size_t)i];
            need(bm2_ksw_align2(1, own.data(), &qo, &q_len[(size_t)i], &to, &t_len[(size_t)i], &xtra[(size_t)i], mat, gap[0], gap[1], gap[2], gap[3], &one[(size_t)i]) == BM2_OK, g_err);
            const bm2_ksw_result &r = one[(size_t)i];
            need(memcmp(&r, &all[(size_t)i], sizeof r) == 0, "a task alone and in its batch differ", s, i);
            need(r.te >= -1 && r.te < (t_len[(size_t)i] > 0 ? t_len[(size_t)i] : 1) && r.qe >= -1 && r.qe < q_len[(size_t)i], "an end lies outside its sequence", s, i);
            need((r.tb < 0) == (r.qb < 0), "one start without the other", s, i);
            const bool sat = (xtra[(size_t)i] & XBYTE) && r.score == 255;
            if (sat) need(r.qe == -1 && r.tb == -1 && r.qb == -1 && r.score2 == -1, "a saturated byte pass answered more than its score", s, i);
            if (!(xtra[(size_t)i] & XSTART)) need(r.tb == -1 && r.qb == -1, "a start without KSW_XSTART", s, i);
            saturated += sat;
        }
        fwrite(all.data(), sizeof(bm2_ksw_result), all.size(), fo);
        if (n >= 3) {                                            // the refusals: nothing is written
            std::vector<bm2_ksw_result> was((size_t)n);
            memset(was.data(), 0x5a, was.size() * sizeof(bm2_ksw_result));
            std::vector<bm2_ksw_result> out = was;
            std::vector<int32_t> bad = q_len;
            bad[(size_t)n - 1] = 0; bad[(size_t)n / 2] = 0;
            need(bm2_ksw_align2(n, seqs.data(), q_off.data(), bad.data(), t_off.data(), t_len.data(), xtra.data(), mat, gap[0], gap[1], gap[2], gap[3], out.data()) == BM2_EINVAL, "an empty query accepted", s);
            char want[64]; snprintf(want, sizeof want, "pair %d has an empty query", n / 2);
            need(strstr(g_err, want) != nullptr, "the lowest offender is not named", s, n / 2);
            bad = t_len; bad[1] = -1;
            need(bm2_ksw_align2(n, seqs.data(), q_off.data(), q_len.data(), t_off.data(), bad.data(), xtra.data(), mat, gap[0], gap[1], gap[2], gap[3], out.data()) == BM2_EINVAL, "a negative length accepted", s);
            need(bm2_ksw_align2(n, seqs.data(), q_off.data(), q_len.data(), t_off.data(), t_len.data(), xtra.data(), mat, gap[0], 0, gap[2], gap[3], out.data()) == BM2_EINVAL, "e_del 0 accepted", s);
            need(bm2_ksw_align2(n, seqs.data(), q_off.data(), q_len.data(), t_off.data(), t_len.data(), xtra.data(), mat, gap[0], gap[1], gap[2], 0, out.data()) == BM2_EINVAL, "e_ins 0 accepted", s);
            need(memcmp(out.data(), was.data(), was.size() * sizeof(bm2_ksw_result)) == 0, "a refused call wrote", s);
        }
        tasks_seen += n;
    }
    fclose(f); fclose(fo);
    need(saturated > 0, "no task saturated the byte pass");
    printf("ok %lld sets %lld tasks %lld saturated\n", (long long)n_sets, tasks_seen, saturated);
    return 0;
}
