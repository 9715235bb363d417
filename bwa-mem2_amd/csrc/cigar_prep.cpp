// cigar_prep.cpp -- the CIGAR batch prepared on the host threads: bm2_cigar_prep (the record-level form, the oracle of cgprep.hip) and
// bm2h_cigar_prep_tasks, which the flag-off path of cigar.hip runs on tasks it has made itself.  Host-only code: the rule is cigar_prep.h's.
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <vector>
#include "../../include/bm2.h"
#include "cigar_prep.h"
#include "host_tail.h"
#include "host_pool.h"

CgpKnobs bm2h_cigar_prep_knobs() {
    static const int no_lds = getenv("BM2_CIGAR_NO_LDS") ? atoi(getenv("BM2_CIGAR_NO_LDS")) : 0;
    static const int no_ring = getenv("BM2_CIGAR_NO_RING") ? atoi(getenv("BM2_CIGAR_NO_RING")) : 0;
    const char *rb = getenv("BM2_CIGAR_RING_BY_BAND");          // (a launch-policy knob: read on every use, see bm2_ctx.h)
    return CgpKnobs{ no_lds, no_ring, rb && *rb ? atoi(rb) : 1 };
}

// Slices of the scratch buffers (sized for the widest band a task can come to) and the cost class of every task: sizes per piece of the
// task list on the host's worker threads, offsets by a scan over the pieces, then the tasks' slices.  Then the order: lanes of a
// wavefront run their tasks side by side, so neighbours should be of one shape (see k_gen_cigar) and cost alike -- a counting sort by
// class key; the order array is the four shapes' task lists one after the other.  tasks: q_off .. re and q_len .. retry are set.
int bm2h_cigar_prep_tasks(const char *who, const CgpPrm &P, int32_t n, bm2_cigar_task_t *tasks, int32_t *order, bm2_cigar_prep_t *tot, TailProf *prof) {
    memset(tot, 0, sizeof *tot);
    const int host_threads = bm2_host_threads();
    const int64_t grain = 16384, pieces = ((int64_t)n + grain - 1) / grain;
    static thread_local std::vector<int64_t> cost_tl; static thread_local std::vector<int32_t> wb_tl;
    std::vector<int64_t> &cost = cost_tl; std::vector<int32_t> &wb1 = wb_tl;
    if (cost.size() < (size_t)n) { cost.resize((size_t)n); wb1.resize((size_t)n); }
    std::vector<CgpSizes> at((size_t)pieces + 1, CgpSizes{ 0, 0, 0, 0, -1 });
    std::atomic<int> too_long(0);
    auto sizes = [&](const bm2_cigar_task_t &T, CgpSizes &s) {
        if (!cgp_sizes(P, T.q_len, T.rb, T.re, T.w, T.truesc, P.force_retry ? 1 : T.retry, s)) too_long = 1;
    };
    bm2_parallel_ranges(n, grain, host_threads, [&](int64_t lo, int64_t hi) {
        CgpSizes sum{ 0, 0, 0, 0, -1 }, s;
        for (int64_t i = lo; i < hi; ++i) {
            sizes(tasks[i], s);
            cost[(size_t)i] = s.z; wb1[(size_t)i] = s.wb_first;
            sum.z += s.z; sum.e += s.e; sum.c += s.c; sum.m += s.m;
        }
        at[(size_t)(lo / grain) + 1] = sum;
    });
    if (too_long.load()) { bm2_set_error("%s: reference range too long", who); return BM2_EINVAL; }
    for (int64_t p = 0; p < pieces; ++p) { CgpSizes &x = at[(size_t)p + 1]; const CgpSizes &y = at[(size_t)p]; x.z += y.z; x.e += y.e; x.c += y.c; x.m += y.m; }
    tot->z_bytes = at[(size_t)pieces].z; tot->eh_items = at[(size_t)pieces].e; tot->cg_items = at[(size_t)pieces].c; tot->md_bytes = at[(size_t)pieces].m;
    bm2_parallel_ranges(n, grain, host_threads, [&](int64_t lo, int64_t hi) {
        CgpSizes o = at[(size_t)(lo / grain)], s;
        for (int64_t i = lo; i < hi; ++i) {
            bm2_cigar_task_t &T = tasks[i];
            T.z_off = o.z; T.eh_off = o.e; T.cg_off = o.c; T.md_off = o.m;
            sizes(T, s);
            o.z += s.z; o.e += s.e; o.c += s.c; o.m += s.m;
        }
    });
    if (prof) prof->mark("slices");
    auto shape = [&](int i) { const bm2_cigar_task_t &T = tasks[i]; return cgp_shape(P, T.q_len, T.rb, T.re, cost[(size_t)i], wb1[(size_t)i]); };
    auto cls = [&](int i) { return cgp_cls(P, shape(i), cost[(size_t)i], wb1[(size_t)i]); };
    bm2_counting_order(n, 256, host_threads, cls, order);
    std::atomic<int> ns[4], qm(0);
    for (auto &x : ns) x = 0;
    bm2_parallel_ranges(n, grain, host_threads, [&](int64_t lo, int64_t hi) {
        int c[4] = { 0, 0, 0, 0 }, q = 0;
        for (int64_t i = lo; i < hi; ++i) { const int sh = shape((int)i); ++c[sh]; if ((sh == CG_SH_RING || sh == CG_SH_ROW) && tasks[i].q_len > q) q = tasks[i].q_len; }
        for (int k = 0; k < 4; ++k) ns[k] += c[k];
        for (int cur = qm.load(); q > cur && !qm.compare_exchange_weak(cur, q);) {}
    });
    for (int k = 0; k < 4; ++k) tot->n_shape[k] = ns[k].load();
    tot->qmax = qm.load();
    if (prof) prof->mark("order");
    return BM2_OK;
}

// what both record-level forms refuse before they look at a task
int bm2h_cigar_prep_args(const char *who, const void *ctx_or_self, const bm2_opt *opt, const bm2_reads *reads, int32_t n, const void *hits, const void *tasks,
                         const void *order, const void *tot) {
    if (!ctx_or_self || !opt || !reads || n < 0 || !tot || (n > 0 && (!hits || !tasks || !order || !reads->off || !reads->len)) || reads->n_reads < 0) {
        bm2_set_error("%s: bad argument", who); return BM2_EINVAL;
    }
    if (n == 0) return BM2_OK;
    if (opt->e_del <= 0 || opt->e_ins <= 0) { bm2_set_error("%s: gap extension penalties must be > 0", who); return BM2_EINVAL; }
    if (!cgp_scmat_ok(opt)) { bm2_set_error("%s: scoring matrix is not of the bwa_fill_scmat form", who); return BM2_EUNSUP; }
    return BM2_OK;
}

extern "C" int bm2_cigar_prep(const bm2_opt *opt, int64_t l_pac, const bm2_reads *reads, int32_t n, const bm2_cigar_hit_t *hits,
                              bm2_cigar_task_t *tasks, int32_t *order, bm2_cigar_prep_t *tot) {
    const char *who = "bm2_cigar_prep";
    int rc = bm2h_cigar_prep_args(who, who, opt, reads, n, hits, tasks, order, tot);
    if (rc || n == 0) return rc;
    const int host_threads = bm2_host_threads();
    std::atomic<int64_t> bad((int64_t)n);
    bm2_parallel_ranges(n, 16384, host_threads, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const bm2_cigar_hit_t &h = hits[i];
            if (h.read < 0 || h.read >= reads->n_reads || h.qb < 0 || h.qb > h.qe || h.qe > reads->len[h.read]) {
                for (int64_t cur = bad.load(); i < cur && !bad.compare_exchange_weak(cur, i);) {}
                return;                                          // (a piece is walked upwards: its first offender is its lowest)
            }
        }
    });
    if (bad.load() < n) { bm2_set_error("%s: task %lld names a read or a stretch of it that does not exist", who, (long long)bad.load()); return BM2_EINVAL; }
    const CgpKnobs kn = bm2h_cigar_prep_knobs();
    const CgpPrm P = cgp_prm(opt, l_pac, kn.no_lds, kn.no_ring, kn.ring_by_band, 0);
    static thread_local std::vector<bm2_cigar_task_t> work_tl;  // (a refused batch leaves the caller's arrays as they were)
    std::vector<bm2_cigar_task_t> &work = work_tl;
    static thread_local std::vector<int32_t> ord_tl;
    std::vector<int32_t> &ord = ord_tl;
    if (work.size() < (size_t)n) { work.resize((size_t)n); ord.resize((size_t)n); }
    bm2_parallel_ranges(n, 16384, host_threads, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const bm2_cigar_hit_t &h = hits[i]; bm2_cigar_task_t &T = work[(size_t)i];
            memset(&T, 0, sizeof T);
            T.q_off = reads->off[h.read] + h.qb; T.q_len = h.qe - h.qb; T.rb = h.rb; T.re = h.re; T.w = h.w; T.truesc = h.truesc; T.retry = h.retry;
        }
    });
    bm2_cigar_prep_t t;
    if ((rc = bm2h_cigar_prep_tasks(who, P, n, work.data(), ord.data(), &t, nullptr))) return rc;
    memcpy(tasks, work.data(), (size_t)n * sizeof(bm2_cigar_task_t));
    memcpy(order, ord.data(), (size_t)n * sizeof(int32_t));
    *tot = t;
    return BM2_OK;
}

static std::atomic<long long> g_cpp_tasks{0}, g_cpp_shape[4], g_cpp_up{0}, g_cpp_fallback{0};
void bm2h_cgprep_stats_reset() { g_cpp_tasks = 0; for (auto &x : g_cpp_shape) x = 0; g_cpp_up = 0; g_cpp_fallback = 0; }
void bm2h_cgprep_stats_add(const bm2_cigar_prep_t *tot, long long bytes_up, long long fallbacks) {
    if (tot) for (int k = 0; k < 4; ++k) { g_cpp_shape[k] += tot->n_shape[k]; g_cpp_tasks += tot->n_shape[k]; }
    g_cpp_up += bytes_up; g_cpp_fallback += fallbacks;
}
extern "C" void bm2_sam_cigar_prep_stats(int64_t *tasks, int64_t shape[4], int64_t *bytes_up, int64_t *host_fallbacks) {
    if (tasks) *tasks = g_cpp_tasks.load();
    if (shape) for (int k = 0; k < 4; ++k) shape[k] = g_cpp_shape[k].load();
    if (bytes_up) *bytes_up = g_cpp_up.load();
    if (host_fallbacks) *host_fallbacks = g_cpp_fallback.load();
}
