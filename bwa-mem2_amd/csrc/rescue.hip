// rescue.hip -- what mem_matesw (bwamem_pair.cpp:150-283) does to a pair's hit lists once its alignments are known, on the device, for a
// batch of pairs: per anchor (end 0 then end 1, the candidates of mem_sam_pe in order, at most max_matesw) the directions that are not
// served by the mate's CURRENT list, each planned result inserted in front of the first hit that scores less, and after every such
// direction mem_sort_dedup_patch without a query (no merging: three sweeps over an order array).  Host oracle: bm2_pe_rescue_apply of
// sam_tail.cpp (rescue_skip / rescue_apply / dedup_rescued), compared field by field.
//
//   k_rescue_init    one lane per list: the list's length as it came, redo = 0 (what a pair without tasks, or a redo pair, keeps)
//   k_rescue_lane    one lane per pair of a cost class (tasks x hits), the class's pairs in their own order; the serial flow of the pair
//   bm2_scan_i32     the lists' final lengths -> their places in the output
//   k_rescue_gather  a 16-lane row per list: the hits in their final order, 16 bytes per lane and step
//
// Two orders of the flow are not total (by reference end; by (score desc, rb, qb) with "the first of equals stays"), so the permutation
// klib's introsort gives to equal keys is visible: both sorts are k_introsort_flat, the comparison sequence of the host's k_introsort.
// A pair's working set is a slice of the batch's arrays sized n0 + n1 + tasks (a task adds at most one hit), at an offset the host
// knows from hit_off and task_off alone: hits are appended to the slice and never move, a list is an array of indices into it.
// With a `plans` array (the tail with the decide bit as well) the gathered lists are not downloaded: decide.hip's resident form packs,
// decides and permutes them where they lie and the decided lists come down (bm2h_decide_resident).
// No alignment runs here: a direction that is open, has a valid window and no task sets the pair's redo flag and leaves its lists as
// they came (the caller runs that pair the old way).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include <string>
#include <vector>
#include "../../include/bm2.h"
#include "bm2_ctx.h"
#include "host_tail.h"
#include "host_pool.h"
#include "pipeline.h"
#include "ksort_dev.h"
#include "rescue_dev.h"                 /* rs_infer_dir, rs_pos2rid, rs_window: shared with plan.hip */

#pragma clang fp contract(off)      /* mask_level_redun * min rounds as in sam_tail.cpp's object code; holds to the end of the file */

#define RS_LANE_THREADS 64
#define RS_CLASSES 3                // lane classes by cost = tasks x (hits + tasks): <= 64, <= 1024, beyond

struct RsPrm {
    const bm2_alnreg_t *in; const int64_t *hit_off;              // the lists as they came (offsets from 0)
    const bm2_rescue_task_t *tasks; const bm2_ksw_result *res;   // res = NULL: the results are in the tasks
    const int64_t *task_off; const int32_t *read_len;
    bm2_alnreg_t *pool; int32_t *L, *ord, *keep, *gone;          // working slices: pair p at hit_off[2p] + task_off[p]
    int32_t *out_n, *redo, *added, *l1_at;                      // l1_at[p]: where list 1 of a worked pair begins in its slice
    const int32_t *order;                                        // the pairs with tasks, class by class
    const int64_t *ann_off; const int32_t *ann_len;
    int64_t l_pac, pad_first;                                    // pad_first >= 0: input hit i gets pad = pad_first + i + 1 (the tail's hit numbers)
    int32_t n_pairs, n_seqs, min_seed_len, max_chain_gap, pen_unpaired, max_matesw;
    float mask_level_redun;
    int32_t low[4], high[4], failed[4];
};

struct RsByEnd { const bm2_alnreg_t *A; __device__ bool operator()(int32_t x, int32_t y) const { return A[x].re < A[y].re; } };
struct RsByScore {
    const bm2_alnreg_t *A;
    __device__ bool operator()(int32_t x, int32_t y) const {
        const bm2_alnreg_t &a = A[x], &b = A[y];
        return a.score > b.score || (a.score == b.score && (a.rb < b.rb || (a.rb == b.rb && a.qb < b.qb)));
    }
};
static __device__ __attribute__((noinline)) void rs_sort_by_end(int n, int32_t *ord, const bm2_alnreg_t *A) { RsByEnd lt = { A }; k_introsort_flat(n, ord, lt); }
static __device__ __attribute__((noinline)) void rs_sort_by_score(int n, int32_t *ord, const bm2_alnreg_t *A) { RsByScore lt = { A }; k_introsort_flat(n, ord, lt); }

struct RsList { bm2_alnreg_t *pool; int32_t *L; int n, used, cap; };         // hits pool[0, used), the list = pool[L[0 .. n)]

// mem_sort_dedup_patch without a query (dedup_rescued of sam_tail.cpp), on indices into the list's pool
static __device__ void rs_dedup(const RsPrm &P, RsList &M, int32_t *ord, int32_t *keep, int32_t *gone) {
    const int n = M.n;
    if (n <= 1) return;
    const bm2_alnreg_t *A = M.pool;
    for (int i = 0; i < n; ++i) { ord[i] = M.L[i]; M.pool[M.L[i]].n_comp = 1; gone[M.L[i]] = 0; }
    rs_sort_by_end(n, ord, A);
    for (int i = 1; i < n; ++i) {
        const bm2_alnreg_t &p = A[ord[i]];
        for (int j = i - 1; j >= 0 && !gone[ord[i]]; --j) {
            const bm2_alnreg_t &q = A[ord[j]];
            if (q.rid != p.rid || p.rb >= q.re + P.max_chain_gap) break;
            if (gone[ord[j]]) continue;
            const int64_t on_ref = q.re - p.rb, on_read = q.qb < p.qb ? q.qe - p.qb : p.qe - q.qb;
            const int64_t sq = q.re - q.rb, sp = p.re - p.rb, min_ref = sq < sp ? sq : sp;
            const int64_t tq = q.qe - q.qb, tp = p.qe - p.qb, min_read = tq < tp ? tq : tp;
            if (on_ref > P.mask_level_redun * min_ref && on_read > P.mask_level_redun * min_read)
                gone[ord[p.score < q.score ? i : j]] = 1;
        }
    }
    int nk = 0;
    for (int i = 0; i < n; ++i) if (!gone[ord[i]]) keep[nk++] = ord[i];
    rs_sort_by_score(nk, keep, A);
    int m = 0;
    for (int k = 0; k < nk; ++k) {
        const bm2_alnreg_t &a = A[keep[k]];
        if (k > 0) { const bm2_alnreg_t &b = A[keep[k - 1]]; if (a.score == b.score && a.rb == b.rb && a.qb == b.qb) continue; }
        M.L[m++] = keep[k];
    }
    M.n = m;
}

// One pair, start to end.  Returns false when the pair has to be redone by the caller (an open direction without a task).
static __device__ bool rs_pair(const RsPrm &P, int64_t p, int *n_added) {
    const int64_t ib[2] = { P.hit_off[2 * p], P.hit_off[2 * p + 1] };
    const int n_in[2] = { (int)(P.hit_off[2 * p + 1] - ib[0]), (int)(P.hit_off[2 * p + 2] - ib[1]) };
    const int64_t t0 = P.task_off[p];
    const int nt = (int)(P.task_off[p + 1] - t0);
    const bm2_rescue_task_t *T = P.tasks + t0;
    int e[2] = { 0, 0 };                                         // hits the tasks may add to list i: those whose anchor is on the other end
    for (int t = 0; t < nt; ++t) ++e[T[t].end ? 0 : 1];
    const int64_t w0 = ib[0] + t0;
    RsList Ls[2];
    Ls[0].pool = P.pool + w0; Ls[0].L = P.L + w0; Ls[0].cap = n_in[0] + e[0];
    Ls[1].pool = Ls[0].pool + Ls[0].cap; Ls[1].L = Ls[0].L + Ls[0].cap; Ls[1].cap = n_in[1] + e[1];
    for (int i = 0; i < 2; ++i) {
        for (int k = 0; k < n_in[i]; ++k) {
            Ls[i].pool[k] = P.in[ib[i] + k];
            if (P.pad_first >= 0) Ls[i].pool[k].pad = (int32_t)(P.pad_first + ib[i] + k + 1);
            Ls[i].L[k] = k;
        }
        Ls[i].n = Ls[i].used = n_in[i];
    }
    int t = 0, added = 0;
    for (int i = 0; i < 2; ++i) {
        RsList &M = Ls[!i];
        const int64_t wm = (!i) ? w0 + Ls[0].cap : w0;           // the mate's slice of the scratch arrays
        int32_t *ord = P.ord + wm, *keep = P.keep + wm, *gone = P.gone + wm;
        const int l_ms = P.read_len[2 * p + !i];
        const bm2_alnreg_t *in = P.in + ib[i];
        int jr = 0;
        for (int k = 0; k < n_in[i] && jr < P.max_matesw; ++k) {
            if (!(in[k].score >= in[0].score - P.pen_unpaired)) continue;
            const int64_t a_rb = in[k].rb; const int a_rid = in[k].rid, a_alt = in[k].is_alt;
            while (t < nt && (T[t].end < i || (T[t].end == i && T[t].j < jr))) ++t;
            int t1 = t;
            while (t1 < nt && T[t1].end == i && T[t1].j == jr) ++t1;
            ++jr;
            unsigned served = 0;                                 // rescue_skip, on the mate's list as it is now
            for (int h = 0; h < M.n; ++h) {
                int64_t dist;
                const int r = rs_infer_dir(P.l_pac, a_rb, M.pool[M.L[h]].rb, &dist);
                served |= (unsigned)(dist >= P.low[r] && dist <= P.high[r]) << r;
            }
            int skip[4], n = 0;
            for (int r = 0; r < 4; ++r) skip[r] = P.failed[r] || (served >> r & 1) ? 1 : 0;
            if (skip[0] + skip[1] + skip[2] + skip[3] == 4) continue;
            for (int r = 0; r < 4; ++r) {
                if (skip[r]) continue;
                int hit = -1;
                for (int x = t; x < t1; ++x) if (T[x].r == r) { hit = x; break; }
                if (hit >= 0) {
                    ++n;
                    const bm2_ksw_result aln = P.res ? P.res[t0 + hit] : T[hit].res;
                    if (!(aln.score < P.min_seed_len || aln.qb < 0)) {
                        if (M.used >= M.cap) return false;       // (cannot happen: a task adds one hit at most and the slice counts every task)
                        const bool flip = (r >> 1) != (r & 1);
                        const int64_t rb = T[hit].rb, l2 = P.l_pac << 1;
                        int64_t qb = aln.qb, qe = (int64_t)aln.qe + 1, b = rb + aln.tb, en = rb + aln.te + 1;
                        if (flip) { const int64_t x0 = l_ms - qe, x1 = l_ms - qb, y0 = l2 - en, y1 = l2 - b; qb = x0; qe = x1; b = y0; en = y1; }
                        bm2_alnreg_t h;
                        memset(&h, 0, sizeof h);
                        h.rid = a_rid; h.is_alt = a_alt;
                        h.qb = (int)qb; h.qe = (int)qe; h.rb = b; h.re = en;
                        h.score = aln.score; h.csub = aln.score2; h.secondary = -1;
                        h.seedcov = (int)((en - b < qe - qb ? en - b : qe - qb) >> 1);
                        int at = 0;                              // in front of the first hit that scores less
                        while (at < M.n && !(M.pool[M.L[at]].score < h.score)) ++at;
                        for (int x = M.n; x > at; --x) M.L[x] = M.L[x - 1];
                        M.pool[M.used] = h; M.L[at] = M.used; ++M.used; ++M.n; ++added;
                    }
                } else { int64_t wb, we; if (rs_window(P, a_rb, a_rid, l_ms, r, &wb, &we)) return false; }
                if (n) rs_dedup(P, M, ord, keep, gone);
            }
        }
    }
    P.out_n[2 * p] = Ls[0].n; P.out_n[2 * p + 1] = Ls[1].n; P.l1_at[p] = Ls[0].cap;
    *n_added = added;
    return true;
}

__global__ void k_rescue_init(RsPrm P) {
    const int64_t li = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= 2 * (int64_t)P.n_pairs) return;
    P.out_n[li] = (int32_t)(P.hit_off[li + 1] - P.hit_off[li]);
    if (!(li & 1)) { P.redo[li >> 1] = 0; P.added[li >> 1] = 0; }
}
__global__ __launch_bounds__(RS_LANE_THREADS) void k_rescue_lane(RsPrm P, int lo, int hi) {
    const int x = lo + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (x >= hi) return;
    const int p = P.order[x];
    int added = 0;
    if (rs_pair(P, p, &added)) P.added[p] = added; else P.redo[p] = 1;
}
// out[out_off[li] + k] = the k-th hit of list li: from the working slice, or as it came (no tasks, or redo)
__global__ __launch_bounds__(256) void k_rescue_gather(RsPrm P, const int64_t *__restrict__ out_off, bm2_alnreg_t *__restrict__ out) {
    const int64_t li = (int64_t)blockIdx.x * (256 / 16) + (threadIdx.x >> 4);
    const int lane = threadIdx.x & 15;
    if (li >= 2 * (int64_t)P.n_pairs) return;
    const int64_t p = li >> 1;
    const int64_t t0 = P.task_off[p], ib = P.hit_off[li];
    const bool plain = P.task_off[p + 1] == t0 || P.redo[p];
    const int n = plain ? (int)(P.hit_off[li + 1] - ib) : P.out_n[li];
    int64_t w = P.hit_off[2 * p] + t0;
    if (!plain && (li & 1)) w += P.l1_at[p];                     // list 1 lies behind list 0's capacity
    const int per = (int)(sizeof(bm2_alnreg_t) / 16);
    for (int x = lane; x < n * per; x += 16) {
        const int k = x / per, q = x - k * per;
        const bm2_alnreg_t *src = plain ? P.in + ib + k : P.pool + w + P.L[w + k];
        uint4 v = ((const uint4 *)src)[q];
        if (plain && P.pad_first >= 0 && q == 5) v.y = (uint32_t)(int32_t)(P.pad_first + ib + k + 1);      // pad: bytes 84..87 of the hit
        ((uint4 *)(out + out_off[li] + k))[q] = v;
    }
}
static_assert(sizeof(bm2_alnreg_t) == 96 && offsetof(bm2_alnreg_t, pad) == 84, "k_rescue_gather moves a hit as six 16-byte words and knows where pad lies");

// The batch on one context.  Offsets may start anywhere (a part of a larger batch); out_off comes back from 0.  The caller has
// checked offsets and tasks.  out_cap < what the lists need: BM2_ECAP with the need in *n_out and nothing written to `out`.
int bm2h_rescue_run(bm2_ctx *c, const char *who, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits,
                    const int64_t *hit_off, const int32_t *read_len, const bm2_pestat pes[4], const bm2_rescue_task_t *tasks,
                    const bm2_ksw_result *res, const int64_t *task_off, int64_t pad_first, bm2_alnreg_t *out, int64_t out_cap,
                    int64_t *out_off, int32_t *redo, int64_t *n_out, int64_t first_pair = 0, bm2_pairplan_t *plans = nullptr) {
    if (n_pairs == 0) { if (out_off) out_off[0] = 0; if (n_out) *n_out = 0; return BM2_OK; }
    int rc = bm2_check(hipSetDevice(c->device), "hipSetDevice");
    if (rc) return rc;
    TailProf prof("pe_rescue_dev");
    const int64_t n_lists = 2 * (int64_t)n_pairs, hbase = hit_off[0], n_hits = hit_off[n_lists] - hbase;
    const int64_t tbase = task_off[0], n_tasks = task_off[n_pairs] - tbase;
    if (n_hits + n_tasks > 0x7fffffff) { bm2_set_error("%s: more than 2^31 hits and tasks in one batch", who); return BM2_EINVAL; }
    const std::vector<int64_t> hoff = bm2h_hit_off_from0(hit_off, n_lists);
    std::vector<int64_t> toff((size_t)n_pairs + 1);
    for (int64_t p = 0; p <= n_pairs; ++p) toff[(size_t)p] = task_off[p] - tbase;
    // the pairs with tasks, in classes of cost, each class in the pairs' own order
    int cnt[RS_CLASSES + 1] = { 0 };
    auto cls = [&](int64_t p) {
        const int64_t nt = toff[(size_t)p + 1] - toff[(size_t)p], cost = nt * (hoff[(size_t)(2 * p + 2)] - hoff[(size_t)(2 * p)] + nt);
        return nt == 0 ? -1 : cost <= 64 ? 0 : cost <= 1024 ? 1 : 2;
    };
    for (int64_t p = 0; p < n_pairs; ++p) { const int k = cls(p); if (k >= 0) ++cnt[k + 1]; }
    for (int k = 0; k < RS_CLASSES; ++k) cnt[k + 1] += cnt[k];
    const int n_order = cnt[RS_CLASSES];
    std::vector<int32_t> order((size_t)n_order + 1);
    { int at[RS_CLASSES]; for (int k = 0; k < RS_CLASSES; ++k) at[k] = cnt[k];
      for (int64_t p = 0; p < n_pairs; ++p) { const int k = cls(p); if (k >= 0) order[(size_t)at[k]++] = (int32_t)p; } }
    prof.mark("classes");
    const size_t W = (size_t)(n_hits + n_tasks);
    const size_t in_b = up256((size_t)n_hits * sizeof(bm2_alnreg_t)), hoff_b = up256((size_t)(n_lists + 1) * 8), toff_b = up256((size_t)(n_pairs + 1) * 8),
                 task_b = up256((size_t)n_tasks * sizeof(bm2_rescue_task_t)), res_b = res ? up256((size_t)n_tasks * sizeof(bm2_ksw_result)) : 0,
                 len_b = up256((size_t)n_lists * 4), ord_b = up256(((size_t)n_order + 1) * 4);
    const size_t pool_b = up256(W * sizeof(bm2_alnreg_t)), idx_b = up256(W * 4), outn_b = up256((size_t)n_lists * 4), flag_b = up256((size_t)n_pairs * 4),
                 ooff_b = up256((size_t)(n_lists + 1) * 8);
    if ((rc = bm2_reserve(c->b_rs_in, in_b + hoff_b + toff_b + task_b + res_b + len_b + ord_b + 256))) return rc;
    if ((rc = bm2_reserve(c->b_rs_work, pool_b + 4 * idx_b + outn_b + 3 * flag_b + ooff_b + 256))) return rc;
    RsPrm P;
    memset(&P, 0, sizeof P);
    char *d = (char *)c->b_rs_in.p;
    P.in = (const bm2_alnreg_t *)d; d += in_b;
    P.hit_off = (const int64_t *)d; d += hoff_b;
    P.task_off = (const int64_t *)d; d += toff_b;
    P.tasks = (const bm2_rescue_task_t *)d; d += task_b;
    P.res = res ? (const bm2_ksw_result *)d : nullptr; d += res_b;
    P.read_len = (const int32_t *)d; d += len_b;
    P.order = (const int32_t *)d;
    char *w = (char *)c->b_rs_work.p;
    P.pool = (bm2_alnreg_t *)w; w += pool_b;
    P.L = (int32_t *)w; w += idx_b; P.ord = (int32_t *)w; w += idx_b; P.keep = (int32_t *)w; w += idx_b; P.gone = (int32_t *)w; w += idx_b;
    P.out_n = (int32_t *)w; w += outn_b; P.redo = (int32_t *)w; w += flag_b; P.added = (int32_t *)w; w += flag_b; P.l1_at = (int32_t *)w; w += flag_b;
    int64_t *d_out_off = (int64_t *)w;
    P.ann_off = c->ix.ann_offset; P.ann_len = c->ix.ann_len; P.l_pac = c->ix.l_pac; P.n_seqs = c->ix.n_seqs;
    P.pad_first = pad_first < 0 ? -1 : pad_first + hbase;
    P.n_pairs = n_pairs; P.min_seed_len = opt->min_seed_len; P.max_chain_gap = opt->max_chain_gap; P.pen_unpaired = so->pen_unpaired; P.max_matesw = so->max_matesw;
    P.mask_level_redun = opt->mask_level_redun;
    for (int k = 0; k < 4; ++k) { P.low[k] = pes[k].low; P.high[k] = pes[k].high; P.failed[k] = pes[k].failed; }
    if (n_hits && (rc = bm2_copy_h2d(c, (void *)P.in, hits + hbase, (size_t)n_hits * sizeof(bm2_alnreg_t)))) return rc;
    if ((rc = bm2_copy_h2d(c, (void *)P.hit_off, hoff.data(), (size_t)(n_lists + 1) * 8))) return rc;
    if ((rc = bm2_copy_h2d(c, (void *)P.task_off, toff.data(), (size_t)(n_pairs + 1) * 8))) return rc;
    if (n_tasks && (rc = bm2_copy_h2d(c, (void *)P.tasks, tasks + tbase, (size_t)n_tasks * sizeof(bm2_rescue_task_t)))) return rc;
    if (n_tasks && res && (rc = bm2_copy_h2d(c, (void *)P.res, res + tbase, (size_t)n_tasks * sizeof(bm2_ksw_result)))) return rc;
    if ((rc = bm2_copy_h2d(c, (void *)P.read_len, read_len, (size_t)n_lists * 4))) return rc;
    if (n_order && (rc = bm2_copy_h2d(c, (void *)P.order, order.data(), (size_t)n_order * 4))) return rc;
    prof.mark("H2D");
    hipLaunchKernelGGL(k_rescue_init, dim3((unsigned)((n_lists + 255) / 256)), dim3(256), 0, c->stream, P);
    if ((rc = bm2_check(hipGetLastError(), "k_rescue_init launch"))) return rc;
    for (int k = 0; k < RS_CLASSES; ++k) {
        const int lo = cnt[k], hi = cnt[k + 1];
        if (hi == lo) continue;
        hipLaunchKernelGGL(k_rescue_lane, dim3((unsigned)((hi - lo + RS_LANE_THREADS - 1) / RS_LANE_THREADS)), dim3(RS_LANE_THREADS), 0, c->stream, P, lo, hi);
        if ((rc = bm2_check(hipGetLastError(), "k_rescue_lane launch"))) return rc;
    }
    if ((rc = bm2_scan_i32(c, P.out_n, n_lists, d_out_off, c->b_rs_scan))) return rc;
    int64_t need = -1;
    if ((rc = bm2_check(hipMemcpyAsync(&need, d_out_off + n_lists, 8, hipMemcpyDeviceToHost, c->stream), "D2H output size"))) return rc;
    if ((rc = bm2_check(hipStreamSynchronize(c->stream), "k_rescue"))) return rc;
    prof.mark("kernels");
    if (need < 0 || need > n_hits + n_tasks) { bm2_set_error("%s: the device counted %lld hits for %lld hits and %lld tasks", who, (long long)need, (long long)n_hits, (long long)n_tasks); return BM2_ENODEV; }
    *n_out = need;
    if (need > out_cap) { bm2_set_error("%s: the lists hold %lld hits, the output has room for %lld", who, (long long)need, (long long)out_cap); return BM2_ECAP; }
    if ((rc = bm2_reserve(c->b_rs_out, up256((size_t)need * sizeof(bm2_alnreg_t)) + 256))) return rc;
    hipLaunchKernelGGL(k_rescue_gather, dim3((unsigned)((n_lists + 15) / 16)), dim3(256), 0, c->stream, P, (const int64_t *)d_out_off, (bm2_alnreg_t *)c->b_rs_out.p);
    if ((rc = bm2_check(hipGetLastError(), "k_rescue_gather launch"))) return rc;
    if ((rc = bm2_check(hipStreamSynchronize(c->stream), "k_rescue_gather"))) return rc;
    prof.mark("gather");
    std::vector<int32_t> added((size_t)n_pairs);
    if ((rc = bm2_copy_d2h(c, out_off, d_out_off, (size_t)(n_lists + 1) * 8))) return rc;
    if (plans) {                                                 // the decisions on the lists where they lie; the decided lists come down once
        if ((rc = bm2h_decide_resident(c, who, opt, so, n_pairs, (const bm2_alnreg_t *)c->b_rs_out.p, d_out_off, out_off, first_pair, pes, plans, out))) return rc;
        prof.mark("decide");
    } else if (need && (rc = bm2_copy_d2h(c, out, c->b_rs_out.p, (size_t)need * sizeof(bm2_alnreg_t)))) return rc;
    if ((rc = bm2_copy_d2h(c, redo, P.redo, (size_t)n_pairs * 4))) return rc;
    if ((rc = bm2_copy_d2h(c, added.data(), P.added, (size_t)n_pairs * 4))) return rc;
    prof.mark("D2H");
    long long a = 0, r = 0;
    for (int64_t p = 0; p < n_pairs; ++p) { a += added[(size_t)p]; r += redo[p] != 0; }
    bm2h_rescue_stats_add(n_pairs, n_tasks, a, r);
    return BM2_OK;
}

extern "C" int bm2_pe_rescue_apply_dev(bm2_ctx *c, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits,
                                       const int64_t *hit_off, const int32_t *read_len, const bm2_pestat pes[4], const bm2_rescue_task_t *tasks,
                                       const int64_t *task_off, bm2_alnreg_t *out, int64_t out_cap, int64_t *out_off, int32_t *redo, int64_t *n_out) {
    if (!c || !opt || !so || n_pairs < 0 || !hit_off || !task_off || !pes || !n_out || !out_off || out_cap < 0 || (n_pairs > 0 && (!read_len || !redo))) {
        bm2_set_error("bm2_pe_rescue_apply_dev: bad argument"); return BM2_EINVAL;
    }
    if (!bm2_ann_ready(c, "bm2_pe_rescue_apply_dev")) return BM2_EINVAL;
    int rc = bm2h_check_rescue_tasks("bm2_pe_rescue_apply_dev", so, n_pairs, hits, hit_off, tasks, task_off);
    if (rc) return rc;
    if (out_cap > 0 && !out) { bm2_set_error("bm2_pe_rescue_apply_dev: bad argument"); return BM2_EINVAL; }
    bm2h_rescue_stats_reset();
    return bm2h_rescue_run(c, "bm2_pe_rescue_apply_dev", opt, so, n_pairs, hits, hit_off, read_len, pes, tasks, nullptr, task_off, -1, out, out_cap, out_off, redo, n_out);
}

// ---- the hook of the SAM tail (bm2h_rescue_batch_fn; user = bm2h_text_ctxs): the chunk's pairs cut into contiguous parts, one context
// and one host thread per part (bm2_run_parts).  A pair's lists depend on its own hits, tasks and the chunk's model only.
int bm2h_dev_rescue_apply_batch(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits, const int64_t *hit_off,
                                const int32_t *read_len, const bm2_pestat pes[4], const bm2_rescue_task_t *tasks, const bm2_ksw_result *res,
                                const int64_t *task_off, bm2_alnreg_t *out, int64_t out_cap, int64_t *out_off, int32_t *redo, int64_t first_pair,
                                bm2_pairplan_t *plans) {
    const bm2h_text_ctxs *m = (const bm2h_text_ctxs *)user;
    for (int g = 0; g < m->n; ++g) if (!bm2_ann_ready(m->ctx[g], "BM2_SAM_F_DEVICE_RESCUE")) return BM2_EINVAL;
    bm2h_rescue_stats_reset();
    if (plans) bm2h_decide_stats_reset();
    const int G = bm2_parts(n_pairs, bm2_knob("BM2_RESCUE_PART", 65536), m->n);      // knob: pairs that are worth a context of their own (launch policy)
    int64_t n_out = 0;
    if (G == 1) return bm2h_rescue_run(m->ctx[0], "BM2_SAM_F_DEVICE_RESCUE", opt, so, n_pairs, hits, hit_off, read_len, pes, tasks, res, task_off, 0, out, out_cap, out_off, redo, &n_out, first_pair, plans);
    // every part's output lies where its input hits and tasks would: room for whatever the part can make; then the parts are closed up
    std::vector<int64_t> got((size_t)G, 0), at((size_t)G + 1, 0);
    std::vector<std::vector<int64_t>> poff((size_t)G);
    for (int g = 0; g < G; ++g) {
        const int64_t lo = (int64_t)n_pairs * g / G, hi = (int64_t)n_pairs * (g + 1) / G;
        at[(size_t)g + 1] = at[(size_t)g] + (hit_off[2 * hi] - hit_off[2 * lo]) + (task_off[hi] - task_off[lo]);
    }
    if (at[(size_t)G] > out_cap) { bm2_set_error("BM2_SAM_F_DEVICE_RESCUE: the output has room for %lld hits, the parts may need %lld", (long long)out_cap, (long long)at[(size_t)G]); return BM2_ECAP; }
    const int rc = bm2_run_parts(G, bm2_part_budget(G), nullptr, [&](int g) {
        const int64_t lo = bm2_part_lo(n_pairs, g, G), hi = bm2_part_lo(n_pairs, g + 1, G);
        poff[(size_t)g].resize((size_t)(2 * (hi - lo) + 1));
        return bm2h_rescue_run(m->ctx[g], "BM2_SAM_F_DEVICE_RESCUE", opt, so, (int32_t)(hi - lo), hits, hit_off + 2 * lo, read_len + 2 * lo, pes, tasks, res,
                                         task_off + lo, 0, out + at[(size_t)g], at[(size_t)g + 1] - at[(size_t)g], poff[(size_t)g].data(), redo + lo, &got[(size_t)g], first_pair + lo, plans ? plans + lo : nullptr);
    });
    if (rc) return rc;
    int64_t base = 0;
    for (int g = 0; g < G; ++g) {
        const int64_t lo = (int64_t)n_pairs * g / G, hi = (int64_t)n_pairs * (g + 1) / G;
        if (got[(size_t)g] && base != at[(size_t)g]) memmove(out + base, out + at[(size_t)g], (size_t)got[(size_t)g] * sizeof(bm2_alnreg_t));
        for (int64_t i = 0; i < 2 * (hi - lo); ++i) out_off[2 * lo + i] = base + poff[(size_t)g][(size_t)i];
        base += got[(size_t)g];
    }
    out_off[2 * (int64_t)n_pairs] = base;
    return BM2_OK;
}

bm2h_rescue_scope::bm2h_rescue_scope(bm2_ctx *const *ctx, int n) : bm2h_ctx_scope(ctx, n), hook(bm2h_dev_rescue_apply_batch, &tc) {}
