// plan.hip -- the first step of mate rescue on the device: which (anchor, direction) alignments the pairs of a batch may ask for
// (rescue_plan of sam_tail.cpp: the candidates of mem_sam_pe, bwamem_pair.cpp:371-376, the skip test of mem_matesw, :165-174, and its
// windows, :176-186), judged on the hit lists as they stand, and the oriented queries of a task list (rescue_query).  Host oracles:
// bm2_pe_rescue_plan and bm2_pe_rescue_queries, compared byte by byte.
//
//   k_plan_count     one lane per (pair, end): the tasks its anchors give
//   bm2_scan_i32     the counts -> every lane's place in the task list: (pair, end, j, r) order comes from the scan, never from atomics
//   k_plan_write     the same walk again, writing the tasks below `cap` (recomputing is cheaper than storing what the count pass saw);
//                    the even lanes also leave task_off
//   k_plan_queries   a 16-lane row per task: aligned words of the mate's codes, copied or reverse-complemented into the task's query
//
// A lane walks its end's candidates (score >= best - pen_unpaired, at most max_matesw); per candidate the mate's hits close directions
// in a 4-bit mask, so a lane holds no array and needs no scratch.  Its cost is candidates x the mate's hits: heavy-tailed, and left so
// (DESIGN.md 6f says what the kernel trace showed).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <functional>
#include <string>
#include <vector>
#include "../../include/bm2.h"
#include "bm2_ctx.h"
#include "host_tail.h"
#include "host_pool.h"
#include "pipeline.h"
#include "rescue_dev.h"

struct PlPrm {
    const bm2_alnreg_t *hits; const int64_t *hit_off;            // the lists (offsets from 0)
    const int32_t *read_len;
    const int64_t *ann_off; const int32_t *ann_len;
    int64_t l_pac;
    int32_t n_pairs, n_seqs, min_seed_len, pen_unpaired, max_matesw, pair_base;      // pair_base: the number of pair 0 in the caller's batch
    int32_t low[4], high[4], failed[4];
};

// (a direction that comes out of a computation selects its bound without indexing the parameter block: no scratch copy of it)
static __device__ __forceinline__ int pl_sel(const int32_t v[4], int r) { return r == 0 ? v[0] : r == 1 ? v[1] : r == 2 ? v[2] : v[3]; }

// The tasks of list li's anchors against the other list of the pair.  WRITE: task i of the lane goes to out[g0 + i] when that is below cap.
template <bool WRITE>
static __device__ __forceinline__ int pl_lane(const PlPrm &P, int64_t li, bm2_rescue_task_t *out, int64_t g0, int64_t cap) {
    const int64_t ab = P.hit_off[li], ae = P.hit_off[li + 1], mb = P.hit_off[li ^ 1], me = P.hit_off[(li ^ 1) + 1];
    if (ab == ae) return 0;
    unsigned live = 0;
    for (int r = 0; r < 4; ++r) live |= (unsigned)(P.failed[r] == 0) << r;
    if (!live) return 0;
    const int l_ms = P.read_len[li ^ 1];
    const int least = P.hits[ab].score - P.pen_unpaired;
    int n = 0, jr = 0;
    for (int64_t k = ab; k < ae && jr < P.max_matesw; ++k) {
        if (!(P.hits[k].score >= least)) continue;
        const int64_t a_rb = P.hits[k].rb;
        const int a_rid = P.hits[k].rid;
        unsigned open = live;                                    // rescue_skip: a direction the mate serves at a plausible distance is closed
        for (int64_t h = mb; h < me && open; ++h) {
            int64_t dist;
            const int r = rs_infer_dir(P.l_pac, a_rb, P.hits[h].rb, &dist);
            if (dist >= pl_sel(P.low, r) && dist <= pl_sel(P.high, r)) open &= ~(1u << r);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (!(open >> r & 1)) continue;
            int64_t rb, re;
            if (!rs_window(P, a_rb, a_rid, l_ms, r, &rb, &re)) continue;
            if (WRITE && g0 + n < cap) {
                bm2_rescue_task_t t;
                memset(&t, 0, sizeof t);
                t.pair = P.pair_base + (int32_t)(li >> 1); t.j = jr; t.end = (int32_t)(li & 1); t.r = r; t.rb = rb; t.re = re;
                out[g0 + n] = t;
            }
            ++n;
        }
        ++jr;
    }
    return n;
}

__global__ __launch_bounds__(256) void k_plan_count(PlPrm P, int32_t *__restrict__ cnt) {
    const int64_t li = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= 2 * (int64_t)P.n_pairs) return;
    cnt[li] = pl_lane<false>(P, li, nullptr, 0, 0);
}
__global__ __launch_bounds__(256) void k_plan_write(PlPrm P, const int64_t *__restrict__ off, bm2_rescue_task_t *__restrict__ out, int64_t cap,
                                                    int64_t *__restrict__ task_off) {
    const int64_t li = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= 2 * (int64_t)P.n_pairs) return;
    const int64_t g0 = off[li];
    if (!(li & 1)) task_off[li >> 1] = g0;
    if (li == 0) task_off[P.n_pairs] = off[2 * (int64_t)P.n_pairs];
    if (off[li + 1] > g0 && g0 < cap) pl_lane<true>(P, li, out, g0, cap);
}

// One query: len codes from enc[src ..), to out[dst ..); rev: reversed, c < 4 ? 3 - c : 4.
struct PlQuery { int64_t src, dst; int32_t len, rev; };         // 24 B
// Row lane w takes the query's bytes [4w, 4w + 4), then 64 further on, ...: their four source codes lie in two aligned words of enc (which
// has 4 readable bytes in front of its first code and 8 behind its last).  Every lane stores only bytes of its own query, one by one: two
// queries that share a dword never see a store to a byte that is not theirs.
__global__ __launch_bounds__(256) void k_plan_queries(const uint8_t *__restrict__ enc, const PlQuery *__restrict__ q, int64_t n, uint8_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * (256 / 16) + (threadIdx.x >> 4);
    if (t >= n) return;
    const PlQuery Q = q[t];
    const uint8_t *src = enc + Q.src;
    uint8_t *dst = out + Q.dst;
    for (int at = (int)(threadIdx.x & 15) * 4; at < Q.len; at += 64) {
        const int s0 = Q.rev ? Q.len - at - 4 : at;             // (>= -3: the bytes in front of the read are loaded and not used)
        const uintptr_t u = (uintptr_t)(src + s0);
        const uint32_t *wp = (const uint32_t *)(u & ~(uintptr_t)3);
        const uint32_t x = (uint32_t)((((uint64_t)wp[1] << 32) | wp[0]) >> (8 * (unsigned)(u & 3)));
        const int nb = Q.len - at < 4 ? Q.len - at : 4;
        for (int k = 0; k < nb; ++k) {
            const unsigned c = x >> (8 * (Q.rev ? 3 - k : k)) & 0xff;
            dst[at + k] = (uint8_t)(Q.rev ? (c < 4 ? 3 - c : 4) : c);
        }
    }
}
#define PL_ENC_FRONT 256            // bytes in front of the uploaded codes (k_plan_queries reads up to 4), keeping their alignment
#define PL_ENC_BACK 8

namespace {
typedef std::function<bm2_rescue_task_t *(int64_t)> PlRoom;      // room for n tasks (NULL: none to be had)
}  // namespace

// The batch on one context.  Offsets may start anywhere (a part of a larger batch); task_off comes back from 0, the tasks name pairs
// from pair_base on.  The caller has checked the offsets.  *n_out = the tasks the pairs need; min(*n_out, cap) of them are written to
// what room(min(*n_out, cap)) answers.  epoch = the number of the tail call this belongs to when its model was counted on the device
// (bm2h_tail_epoch; 0: none): the hits and offsets that pass left in b_pl_in are used where they lie when they are exactly these.
static int plan_run(bm2_ctx *c, const char *who, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits,
                    const int64_t *hit_off, const int32_t *read_len, const bm2_pestat pes[4], int32_t pair_base, const PlRoom &room, int64_t cap,
                    int64_t *task_off, int64_t *n_out, uint64_t epoch = 0) {
    *n_out = 0;
    task_off[0] = 0;
    if (n_pairs == 0) return BM2_OK;
    int rc = bm2_check(hipSetDevice(c->device), "hipSetDevice");
    if (rc) return rc;
    TailProf prof("pe_plan_dev");
    const int64_t n_lists = 2 * (int64_t)n_pairs, hbase = hit_off[0], n_hits = hit_off[n_lists] - hbase;
    const size_t in_b = up256((size_t)n_hits * sizeof(bm2_alnreg_t)), hoff_b = up256((size_t)(n_lists + 1) * 8), len_b = up256((size_t)n_lists * 4);
    const size_t cnt_b = up256((size_t)n_lists * 4), off_b = up256((size_t)(n_lists + 1) * 8), toff_b = up256((size_t)(n_pairs + 1) * 8);
    const bm2_ctx::PlResident &have = c->pl_res;
    const bool resident = epoch != 0 && have.epoch == epoch && have.hits == (hits ? (const void *)(hits + hbase) : nullptr) && have.hit_off == (const void *)hit_off &&
                          have.hbase == hbase && have.n_hits == n_hits && have.n_pairs == n_pairs && c->b_pl_in.cap >= in_b + hoff_b + len_b + 256;
    c->pl_res.epoch = 0;                                         // (one reader; a miss overwrites the buffer)
    if ((rc = bm2_reserve(c->b_pl_in, in_b + hoff_b + len_b + 256))) return rc;
    if ((rc = bm2_reserve(c->b_pl_work, cnt_b + off_b + toff_b + 256))) return rc;
    PlPrm P;
    memset(&P, 0, sizeof P);
    char *d = (char *)c->b_pl_in.p;
    P.hits = (const bm2_alnreg_t *)d; d += in_b;
    P.hit_off = (const int64_t *)d; d += hoff_b;
    P.read_len = (const int32_t *)d;
    char *w = (char *)c->b_pl_work.p;
    int32_t *d_cnt = (int32_t *)w; w += cnt_b;
    int64_t *d_off = (int64_t *)w; w += off_b;
    int64_t *d_toff = (int64_t *)w;
    P.ann_off = c->ix.ann_offset; P.ann_len = c->ix.ann_len; P.l_pac = c->ix.l_pac; P.n_seqs = c->ix.n_seqs;
    P.n_pairs = n_pairs; P.min_seed_len = opt->min_seed_len; P.pen_unpaired = so->pen_unpaired; P.max_matesw = so->max_matesw; P.pair_base = pair_base;
    for (int k = 0; k < 4; ++k) { P.low[k] = pes[k].low; P.high[k] = pes[k].high; P.failed[k] = pes[k].failed; }
    if (!resident) {
        const std::vector<int64_t> hoff = bm2h_hit_off_from0(hit_off, n_lists);
        if (n_hits && (rc = bm2_copy_h2d(c, (void *)P.hits, hits + hbase, (size_t)n_hits * sizeof(bm2_alnreg_t)))) return rc;
        if ((rc = bm2_copy_h2d(c, (void *)P.hit_off, hoff.data(), (size_t)(n_lists + 1) * 8))) return rc;
    } else bm2h_pestat_stats_shared((long long)((size_t)n_hits * sizeof(bm2_alnreg_t)), true);
    if ((rc = bm2_copy_h2d(c, (void *)P.read_len, read_len, (size_t)n_lists * 4))) return rc;
    prof.mark("H2D");
    const dim3 grid((unsigned)((n_lists + 255) / 256)), block(256);
    hipLaunchKernelGGL(k_plan_count, grid, block, 0, c->stream, P, d_cnt);
    if ((rc = bm2_check(hipGetLastError(), "k_plan_count launch"))) return rc;
    if ((rc = bm2_scan_i32(c, d_cnt, n_lists, d_off, c->b_pl_scan))) return rc;
    int64_t need = -1;
    if ((rc = bm2_check(hipMemcpyAsync(&need, d_off + n_lists, 8, hipMemcpyDeviceToHost, c->stream), "D2H task count"))) return rc;
    if ((rc = bm2_check(hipStreamSynchronize(c->stream), "k_plan_count"))) return rc;
    if (need < 0 || need > 4 * (int64_t)(so->max_matesw > 0 ? so->max_matesw : 0) * n_lists) {
        bm2_set_error("%s: the device counted %lld tasks for %lld lists", who, (long long)need, (long long)n_lists); return BM2_ENODEV;
    }
    *n_out = need;
    const int64_t n_write = need < cap ? need : cap;
    bm2_rescue_task_t *dst = n_write > 0 ? room(n_write) : nullptr;
    if (n_write > 0 && !dst) { bm2_set_error("%s: out of memory for %lld tasks", who, (long long)n_write); return BM2_ENOMEM; }
    if ((rc = bm2_reserve(c->b_pl_out, up256((size_t)n_write * sizeof(bm2_rescue_task_t)) + 256))) return rc;
    hipLaunchKernelGGL(k_plan_write, grid, block, 0, c->stream, P, (const int64_t *)d_off, (bm2_rescue_task_t *)c->b_pl_out.p, n_write, d_toff);
    if ((rc = bm2_check(hipGetLastError(), "k_plan_write launch"))) return rc;
    if ((rc = bm2_check(hipStreamSynchronize(c->stream), "k_plan_write"))) return rc;
    prof.mark("kernels");
    if (n_write > 0 && (rc = bm2_copy_d2h(c, dst, c->b_pl_out.p, (size_t)n_write * sizeof(bm2_rescue_task_t)))) return rc;
    if ((rc = bm2_copy_d2h(c, task_off, d_toff, (size_t)(n_pairs + 1) * 8))) return rc;
    prof.mark("D2H");
    return BM2_OK;
}

extern "C" int bm2_pe_rescue_plan_dev(bm2_ctx *c, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits,
                                      const int64_t *hit_off, const int32_t *read_len, const bm2_pestat pes[4], bm2_rescue_task_t *tasks, int64_t cap,
                                      int64_t *task_off, int64_t *n_out) {
    if (!c || !opt || !so || n_pairs < 0 || !hit_off || !pes || !task_off || !n_out || cap < 0 || (cap > 0 && !tasks) || (n_pairs > 0 && !read_len)) {
        bm2_set_error("bm2_pe_rescue_plan_dev: bad argument"); return BM2_EINVAL;
    }
    if (!bm2_ann_ready(c, "bm2_pe_rescue_plan_dev")) return BM2_EINVAL;
    int rc = bm2h_check_hit_off("bm2_pe_rescue_plan_dev", n_pairs, hit_off);
    if (rc) return rc;
    if (hit_off[2 * (int64_t)n_pairs] > hit_off[0] && !hits) { bm2_set_error("bm2_pe_rescue_plan_dev: bad argument"); return BM2_EINVAL; }
    bm2h_plan_stats_set(0, 0, 0);
    rc = plan_run(c, "bm2_pe_rescue_plan_dev", opt, so, n_pairs, hits, hit_off, read_len, pes, 0, [&](int64_t) { return tasks; }, cap, task_off, n_out);
    if (rc) return rc;
    bm2h_plan_stats_set(n_pairs, *n_out, 0);
    if (*n_out > cap) { bm2_set_error("bm2_pe_rescue_plan_dev: %lld tasks, room for %lld", (long long)*n_out, (long long)cap); return BM2_ECAP; }
    return BM2_OK;
}

// ---- queries.  The codes of the reads the tasks [0, n) align (their mates), as one run of `enc`, go up; the queries are made in
// d_out (room for q_off[n] - q_off[0] bytes) at q_off[t] - q_off[0].  The caller has checked the tasks against the reads.
int bm2h_plan_queries_resident(bm2_ctx *c, const bm2_reads *reads, int64_t n, const bm2_rescue_task_t *tasks, const int64_t *q_off, uint8_t *d_out) {
    if (n <= 0) return BM2_OK;
    const int host_threads = bm2_host_threads();
    const int64_t grain = 16384, pieces = (n + grain - 1) / grain;
    std::vector<int64_t> lo_of((size_t)pieces, INT64_MAX), hi_of((size_t)pieces, 0);
    bm2_parallel_ranges(n, grain, host_threads, [&](int64_t a, int64_t b) {
        int64_t lo = INT64_MAX, hi = 0;
        for (int64_t t = a; t < b; ++t) {
            const int m = 2 * tasks[t].pair + !tasks[t].end;
            if (reads->off[m] < lo) lo = reads->off[m];
            if (reads->off[m] + reads->len[m] > hi) hi = reads->off[m] + reads->len[m];
        }
        lo_of[(size_t)(a / grain)] = lo; hi_of[(size_t)(a / grain)] = hi;
    });
    int64_t lo = INT64_MAX, hi = 0;
    for (int64_t p = 0; p < pieces; ++p) { if (lo_of[(size_t)p] < lo) lo = lo_of[(size_t)p]; if (hi_of[(size_t)p] > hi) hi = hi_of[(size_t)p]; }
    if (hi < lo) hi = lo;
    static thread_local std::vector<PlQuery> q_tl;
    std::vector<PlQuery> &q = q_tl;
    if (q.size() < (size_t)n) q.resize((size_t)n);
    bm2_parallel_ranges(n, grain, host_threads, [&](int64_t a, int64_t b) {
        for (int64_t t = a; t < b; ++t) {
            const int m = 2 * tasks[t].pair + !tasks[t].end, r = tasks[t].r;
            q[(size_t)t] = PlQuery{ reads->off[m] - lo, q_off[t] - q_off[0], reads->len[m], (r >> 1) != (r & 1) };
        }
    });
    const size_t enc_b = up256(PL_ENC_FRONT + (size_t)(hi - lo) + PL_ENC_BACK), q_b = up256((size_t)n * sizeof(PlQuery));
    c->pl_res.epoch = 0;                                         // (b_pl_in changes hands)
    int rc = bm2_reserve(c->b_pl_in, enc_b + q_b + 256);
    if (rc) return rc;
    uint8_t *d_enc = (uint8_t *)c->b_pl_in.p + PL_ENC_FRONT;
    PlQuery *d_q = (PlQuery *)((char *)c->b_pl_in.p + enc_b);
    if (hi > lo && (rc = bm2_copy_h2d(c, d_enc, reads->enc + lo, (size_t)(hi - lo)))) return rc;
    if ((rc = bm2_copy_h2d(c, d_q, q.data(), (size_t)n * sizeof(PlQuery)))) return rc;
    hipLaunchKernelGGL(k_plan_queries, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, c->stream, (const uint8_t *)d_enc, (const PlQuery *)d_q, n, d_out);
    return bm2_check(hipGetLastError(), "k_plan_queries launch");
}

extern "C" int bm2_pe_rescue_queries_dev(bm2_ctx *c, const bm2_reads *reads, int64_t n_tasks, const bm2_rescue_task_t *tasks, uint8_t *out, int64_t cap,
                                         int64_t *q_off, int64_t *n_out) {
    if (!c) { bm2_set_error("bm2_pe_rescue_queries_dev: bad argument"); return BM2_EINVAL; }
    int rc = bm2h_plan_query_offsets("bm2_pe_rescue_queries_dev", reads, n_tasks, tasks, out, cap, q_off, n_out);      // (*n_out, q_off; BM2_ECAP)
    if (rc) return rc;
    const int64_t bytes = *n_out;
    if (bytes == 0) return BM2_OK;
    if ((rc = bm2_check(hipSetDevice(c->device), "hipSetDevice"))) return rc;
    if ((rc = bm2_reserve(c->b_pl_out, up256((size_t)bytes) + 256))) return rc;
    if ((rc = bm2h_plan_queries_resident(c, reads, n_tasks, tasks, q_off, (uint8_t *)c->b_pl_out.p))) return rc;
    return bm2_copy_d2h(c, out, c->b_pl_out.p, (size_t)bytes);       // (waits for the kernel: same stream)
}

int bm2h_plan_parts(int64_t n_pairs, int n_ctx) { return bm2_parts(n_pairs, bm2_knob("BM2_PLAN_PART", 65536), n_ctx); }      // knob: pairs that are worth a context of their own (launch policy)

// ---- the hook of the SAM tail (bm2h_plan_batch_fn; user = bm2h_text_ctxs): the chunk's pairs cut into contiguous parts, one context
// and one host thread per part (bm2_run_parts).  A pair's tasks depend on its own lists and the chunk's model only.
int bm2h_dev_plan_batch(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits, const int64_t *hit_off,
                        const int32_t *read_len, const bm2_pestat pes[4], bm2_rescue_task_t *(*room)(void *arg, int64_t n), void *arg,
                        int64_t *task_off, int64_t *n_out) {
    const bm2h_text_ctxs *m = (const bm2h_text_ctxs *)user;
    for (int g = 0; g < m->n; ++g) if (!bm2_ann_ready(m->ctx[g], "BM2_SAM_F_DEVICE_PLAN")) return BM2_EINVAL;
    bm2h_plan_stats_set(0, 0, 0);
    bm2h_pestat_stats_shared(0, false);
    const uint64_t epoch = bm2h_tail_epoch();
    const int G = bm2h_plan_parts(n_pairs, m->n);
    if (G == 1) {
        const int rc = plan_run(m->ctx[0], "BM2_SAM_F_DEVICE_PLAN", opt, so, n_pairs, hits, hit_off, read_len, pes, 0, [&](int64_t n) { return room(arg, n); },
                                INT64_MAX, task_off, n_out, epoch);
        if (!rc) bm2h_plan_stats_set(n_pairs, *n_out, 0);
        return rc;
    }
    std::vector<int64_t> got((size_t)G, 0);
    std::vector<std::vector<bm2_rescue_task_t>> part((size_t)G);
    std::vector<std::vector<int64_t>> poff((size_t)G);
    const int rc = bm2_run_parts(G, bm2_part_budget(G), nullptr, [&](int g) {
        const int64_t lo = bm2_part_lo(n_pairs, g, G), hi = bm2_part_lo(n_pairs, g + 1, G);
        poff[(size_t)g].resize((size_t)(hi - lo + 1));
        return plan_run(m->ctx[g], "BM2_SAM_F_DEVICE_PLAN", opt, so, (int32_t)(hi - lo), hits, hit_off + 2 * lo, read_len + 2 * lo, pes, (int32_t)lo,
                                  [&, g](int64_t n) { part[(size_t)g].resize((size_t)n); return part[(size_t)g].data(); }, INT64_MAX, poff[(size_t)g].data(), &got[(size_t)g], epoch);
    });
    if (rc) return rc;
    int64_t tot = 0;
    for (int g = 0; g < G; ++g) tot += got[(size_t)g];
    bm2_rescue_task_t *dst = tot > 0 ? room(arg, tot) : nullptr;
    if (tot > 0 && !dst) { bm2_set_error("BM2_SAM_F_DEVICE_PLAN: out of memory for %lld tasks", (long long)tot); return BM2_ENOMEM; }
    int64_t base = 0;
    for (int g = 0; g < G; ++g) {
        const int64_t lo = (int64_t)n_pairs * g / G, hi = (int64_t)n_pairs * (g + 1) / G;
        if (got[(size_t)g]) memcpy(dst + base, part[(size_t)g].data(), (size_t)got[(size_t)g] * sizeof(bm2_rescue_task_t));
        for (int64_t p = 0; p < hi - lo; ++p) task_off[lo + p] = base + poff[(size_t)g][(size_t)p];
        base += got[(size_t)g];
    }
    task_off[n_pairs] = base;
    *n_out = tot;
    bm2h_plan_stats_set(n_pairs, tot, 0);
    return BM2_OK;
}

bm2h_plan_scope::bm2h_plan_scope(bm2_ctx *const *ctx, int n)
    : bm2h_ctx_scope(ctx, n), hook(bm2h_dev_plan_batch, bm2h_dev_rescue_batch_resident, &tc) {}
