// pestat.hip -- the counting half of the chunk's insert-size model on the device (pestat_count of sam_tail.cpp: the pair filter of
// mem_pestat, bwamem_pair.cpp:88-101, with cal_sub, :67-79, and mem_infer_dir, :58-65).  Host oracle: bm2_pe_stat, compared bin for bin.
// The model half (quartiles, trimmed mean and deviation, bounds, the `failed` marks) is pestat_model of sam_tail.cpp for both forms:
// double arithmetic in the reference's order stays on the host.
//
//   k_pestat          one lane per pair: both lists non-empty, both best hits unique enough, one contig -> one add to bin [dir][is]
//   k_pestat_reduce   the privatised copies of the histogram summed into copy 0 (only when there is more than one)
//
// Counts are 32-bit integers added with non-returning atomics, so the order of the adds cannot show.  A real chunk sends half a million
// pairs to a few hundred neighbouring bins of one orientation; block b adds into copy b % K of the histogram (knob BM2_PESTAT_COPIES)
// so that those adds meet K-fold fewer others on their cache lines.  K falls to 1 as the bins grow.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/bm2.h"
#include "bm2_ctx.h"
#include "host_tail.h"
#include "host_pool.h"
#include "rescue_dev.h"

struct PsPrm {
    const bm2_alnreg_t *hits; const int64_t *hit_off;            // the lists (offsets from 0)
    int64_t l_pac, bins;                                         // bins = max_ins + 1: one orientation's counts, bin 0 unused
    int32_t n_pairs, max_ins, min_seed_len, a, copies;
    float mask_level;
};

// cal_sub (sam_tail.cpp; bwamem_pair.cpp:67-79) of the list [b, e): the score of the first hit after the best whose query span overlaps
// the best's by at least mask_level of the shorter span -- a float product, compared as floats, as the host compiles it.
static __device__ __forceinline__ int ps_cal_sub(const PsPrm &P, int64_t b, int64_t e) {
    const int qb0 = P.hits[b].qb, qe0 = P.hits[b].qe;
    for (int64_t j = b + 1; j < e; ++j) {
        const int qb = P.hits[j].qb, qe = P.hits[j].qe;
        const int b_max = qb > qb0 ? qb : qb0, e_min = qe < qe0 ? qe : qe0;
        if (e_min > b_max) {
            const int min_l = qe - qb < qe0 - qb0 ? qe - qb : qe0 - qb0;
            if ((float)(e_min - b_max) >= (float)min_l * P.mask_level) return P.hits[j].score;
        }
    }
    return P.min_seed_len * P.a;
}

__global__ __launch_bounds__(256) void k_pestat(PsPrm P, uint32_t *__restrict__ hist) {
    const int64_t pi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pi >= P.n_pairs) return;
    const int64_t b0 = P.hit_off[2 * pi], b1 = P.hit_off[2 * pi + 1], e1 = P.hit_off[2 * pi + 2];
    if (b0 == b1 || b1 == e1) return;
    if ((double)ps_cal_sub(P, b0, b1) > 0.8 * (double)P.hits[b0].score) return;
    if ((double)ps_cal_sub(P, b1, e1) > 0.8 * (double)P.hits[b1].score) return;
    if (P.hits[b0].rid != P.hits[b1].rid) return;
    int64_t is;
    const int dir = rs_infer_dir(P.l_pac, P.hits[b0].rb, P.hits[b1].rb, &is);
    if (is == 0 || is > P.max_ins) return;
    const int64_t copy = blockIdx.x % (unsigned)P.copies;
    atomicAdd(hist + (copy * 4 + dir) * P.bins + is, 1u);         // (the result is not used: a non-returning add)
}
// hist[v] += hist[k * n + v] for the copies k = 1 .. copies - 1; n = 4 * bins
__global__ __launch_bounds__(256) void k_pestat_reduce(uint32_t *__restrict__ hist, int64_t n, int copies) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    uint32_t s = hist[v];
    for (int k = 1; k < copies; ++k) s += hist[(int64_t)k * n + v];
    hist[v] = s;
}

namespace {
// Copies of the histogram for `blocks` blocks adding into 4 * bins counts: the knob, at most one per block, and no more than fit 32 MB
// -- 16 at the default max_ins (160 KB a copy), 1 from max_ins = 2^20 on (16 MB a copy; 268 MB at the 2^24 limit).
int pestat_copies(int64_t bins, int64_t blocks) {
    int64_t k = bm2_knob("BM2_PESTAT_COPIES", 16);
    const int64_t fit = ((int64_t)32 << 20) / (16 * bins);
    if (k > fit) k = fit;
    if (k > blocks) k = blocks;
    if (k > 256) k = 256;
    return k < 1 ? 1 : (int)k;
}
}  // namespace

// The counts of one batch on one context: hist[4 * (max_ins + 1)] (host) is filled.  Offsets may start anywhere (a part of a larger
// batch); the caller has checked them and max_ins is in [1, 2^24].  The hits and the re-based offsets go into b_pl_in in plan_run's
// layout, and with epoch != 0 the context remembers whose they are, so that the plan of the same tail call finds them there.
static int pestat_run(bm2_ctx *c, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits, const int64_t *hit_off,
                      uint32_t *hist, uint64_t epoch, int64_t *hit_bytes_up) {
    const int64_t bins = (int64_t)so->max_ins + 1, n_cnt = 4 * bins;
    *hit_bytes_up = 0;
    memset(hist, 0, (size_t)n_cnt * 4);
    if (n_pairs == 0) return BM2_OK;
    int rc = bm2_check(hipSetDevice(c->device), "hipSetDevice");
    if (rc) return rc;
    TailProf prof("pe_stat_dev");
    const int64_t n_lists = 2 * (int64_t)n_pairs, hbase = hit_off[0], n_hits = hit_off[n_lists] - hbase;
    const int64_t blocks = ((int64_t)n_pairs + 255) / 256;
    const int copies = pestat_copies(bins, blocks);
    // (b_pl_in sized as plan_run sizes it, the read lengths' room included: its reserve then keeps the buffer)
    const size_t in_b = up256((size_t)n_hits * sizeof(bm2_alnreg_t)), hoff_b = up256((size_t)(n_lists + 1) * 8), len_b = up256((size_t)n_lists * 4);
    c->pl_res.epoch = 0;
    if ((rc = bm2_reserve(c->b_pl_in, in_b + hoff_b + len_b + 256))) return rc;
    if ((rc = bm2_reserve(c->b_pl_work, up256((size_t)copies * (size_t)n_cnt * 4) + 256))) return rc;
    PsPrm P;
    memset(&P, 0, sizeof P);
    P.hits = (const bm2_alnreg_t *)c->b_pl_in.p;
    P.hit_off = (const int64_t *)((char *)c->b_pl_in.p + in_b);
    P.l_pac = c->ix.l_pac; P.bins = bins; P.n_pairs = n_pairs; P.max_ins = so->max_ins; P.min_seed_len = opt->min_seed_len; P.a = opt->a;
    P.copies = copies; P.mask_level = opt->mask_level;
    uint32_t *d_hist = (uint32_t *)c->b_pl_work.p;
    const std::vector<int64_t> hoff = bm2h_hit_off_from0(hit_off, n_lists);
    if (n_hits && (rc = bm2_copy_h2d(c, (void *)P.hits, hits + hbase, (size_t)n_hits * sizeof(bm2_alnreg_t)))) return rc;
    if ((rc = bm2_copy_h2d(c, (void *)P.hit_off, hoff.data(), (size_t)(n_lists + 1) * 8))) return rc;
    *hit_bytes_up = (int64_t)((size_t)n_hits * sizeof(bm2_alnreg_t));
    prof.mark("H2D");
    if ((rc = bm2_check(hipMemsetAsync(d_hist, 0, (size_t)copies * (size_t)n_cnt * 4, c->stream), "memset histogram"))) return rc;
    hipLaunchKernelGGL(k_pestat, dim3((unsigned)blocks), dim3(256), 0, c->stream, P, d_hist);
    if ((rc = bm2_check(hipGetLastError(), "k_pestat launch"))) return rc;
    if (copies > 1) {
        hipLaunchKernelGGL(k_pestat_reduce, dim3((unsigned)((n_cnt + 255) / 256)), dim3(256), 0, c->stream, d_hist, n_cnt, copies);
        if ((rc = bm2_check(hipGetLastError(), "k_pestat_reduce launch"))) return rc;
    }
    if ((rc = bm2_check(hipStreamSynchronize(c->stream), "k_pestat"))) return rc;
    prof.mark("kernels");
    if ((rc = bm2_copy_d2h(c, hist, d_hist, (size_t)n_cnt * 4))) return rc;
    prof.mark("D2H");
    if (epoch) {
        bm2_ctx::PlResident &t = c->pl_res;
        t.hits = hits ? (const void *)(hits + hbase) : nullptr; t.hit_off = hit_off; t.hbase = hbase; t.n_hits = n_hits; t.n_pairs = n_pairs; t.epoch = epoch;
    }
    return BM2_OK;
}

static long long pestat_counted(const std::vector<uint32_t> &h) { long long n = 0; for (uint32_t v : h) n += v; return n; }

extern "C" int bm2_pe_stat_dev(bm2_ctx *c, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits,
                               const int64_t *hit_off, bm2_pestat pes[4], uint32_t *hist, int64_t hist_cap) {
    if (!c || !opt || !so || n_pairs < 0 || !hit_off || !pes || hist_cap < 0) { bm2_set_error("bm2_pe_stat_dev: bad argument"); return BM2_EINVAL; }
    if (!bm2_ann_ready(c, "bm2_pe_stat_dev")) return BM2_EINVAL;
    int rc = bm2h_check_hit_off("bm2_pe_stat_dev", n_pairs, hit_off);
    if (rc) return rc;
    if (hit_off[2 * (int64_t)n_pairs] > hit_off[0] && !hits) { bm2_set_error("bm2_pe_stat_dev: bad argument"); return BM2_EINVAL; }
    if (so->max_ins > (1 << 24)) { bm2_set_error("bm2_pe_stat_dev: max_ins above 2^24 is not supported (the insert sizes are counted in a histogram)"); return BM2_EUNSUP; }
    const int64_t top = so->max_ins > 0 ? so->max_ins : 0;
    if (hist && hist_cap < 4 * (top + 1)) { bm2_set_error("bm2_pe_stat_dev: the histogram takes %lld counts, room for %lld", (long long)(4 * (top + 1)), (long long)hist_cap); return BM2_ECAP; }
    bm2h_pestat_stats_set(0, 0, 0);
    std::vector<uint32_t> h((size_t)(4 * (top + 1)), 0);
    int64_t up = 0;
    if (top > 0 && (rc = pestat_run(c, opt, so, n_pairs, hits, hit_off, h.data(), 0, &up))) return rc;
    bm2h_pestat_model(h.data(), top, pes);
    if (hist) memcpy(hist, h.data(), h.size() * sizeof(uint32_t));
    bm2h_pestat_stats_set(n_pairs, pestat_counted(h), up);
    return BM2_OK;
}

// ---- the hook of the SAM tail (bm2h_pestat_batch_fn; user = bm2h_text_ctxs): the chunk's pairs cut into the parts of the plan hook, one
// context and one host thread per part; a pair's bin depends on its own lists only, the parts' counts are summed here (integers) and
// the model is read off the sum once.
int bm2h_dev_pestat_batch(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits, const int64_t *hit_off,
                          bm2_pestat pes[4]) {
    const bm2h_text_ctxs *m = (const bm2h_text_ctxs *)user;
    for (int g = 0; g < m->n; ++g) if (!bm2_ann_ready(m->ctx[g], "BM2_SAM_F_DEVICE_PESTAT")) return BM2_EINVAL;
    bm2h_pestat_stats_set(0, 0, 0);
    int rc = bm2h_check_hit_off("BM2_SAM_F_DEVICE_PESTAT", n_pairs, hit_off);
    if (rc) return rc;
    if (so->max_ins > (1 << 24)) { bm2_set_error("BM2_SAM_F_DEVICE_PESTAT: max_ins above 2^24 is not supported"); return BM2_EUNSUP; }
    const int64_t top = so->max_ins > 0 ? so->max_ins : 0;
    const size_t n_cnt = (size_t)(4 * (top + 1));
    const uint64_t epoch = bm2h_tail_epoch();
    const int G = bm2h_plan_parts(n_pairs, m->n);
    std::vector<uint32_t> h(n_cnt, 0);
    int64_t up = 0;
    if (top > 0 && G == 1) {
        if ((rc = pestat_run(m->ctx[0], opt, so, n_pairs, hits, hit_off, h.data(), epoch, &up))) return rc;
    } else if (top > 0) {
        std::vector<int64_t> ups((size_t)G, 0);
        std::vector<std::vector<uint32_t>> part((size_t)G);
        rc = bm2_run_parts(G, bm2_part_budget(G), nullptr, [&](int g) {
            const int64_t lo = bm2_part_lo(n_pairs, g, G), hi = bm2_part_lo(n_pairs, g + 1, G);
            part[(size_t)g].resize(n_cnt);
            return pestat_run(m->ctx[g], opt, so, (int32_t)(hi - lo), hits, hit_off + 2 * lo, part[(size_t)g].data(), epoch, &ups[(size_t)g]);
        });
        if (rc) return rc;
        for (int g = 0; g < G; ++g) {
            const uint32_t *o = part[(size_t)g].data();
            for (size_t v = 0; v < n_cnt; ++v) h[v] += o[v];
            up += ups[(size_t)g];
        }
    }
    bm2h_pestat_model(h.data(), top, pes);
    bm2h_pestat_stats_set(n_pairs, pestat_counted(h), up);
    return BM2_OK;
}

bm2h_pestat_scope::bm2h_pestat_scope(bm2_ctx *const *ctx, int n)
    : bm2h_ctx_scope(ctx, n), hook(bm2h_dev_pestat_batch, &tc) {}
bm2h_pestat_scope::~bm2h_pestat_scope() { for (int g = 0; g < tc.n; ++g) if (tc.ctx[g]) tc.ctx[g]->pl_res.epoch = 0; }
