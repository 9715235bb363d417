// decide.hip -- the pairing decisions of mem_sam_pe (bwamem_pair.cpp:353-551) on the device, for a batch of pairs whose hit lists are
// final (mate rescue applied): mem_mark_primary_se on both lists, mem_reorder_primary5, mem_pair, q_pe / q_se, the rewrite of the chosen
// hits and the primary / secondary switch.  Host oracle: pe_decide_marked of sam_tail.cpp behind bm2_pe_decide, compared field by field.
//
//   k_decide_class   one lane per pair: light (<= 16 hits in all) or heavy, and the heavy pair's share of the global workspace
//   bm2_scan_i32     two scans: the heavy pairs' numbers in the heavy list, their workspace offsets
//   k_decide_list    the heavy list
//   k_decide_light   a 16-lane row per pair, both lists in LDS
//   k_decide_heavy   a wavefront per heavy pair: lists in LDS up to DC_HEAVY_LDS hits in all, in the global workspace beyond.  EVERY pair
//                    is decided by one of the two; nothing goes back to the host.
// Both kernels run the SAME code (decide_pair<W>): the lanes of a group stride over the hits, exchange through the group's memory and
// meet at group barriers, so the one difference between the forms is the group's width and where its memory lies.
//
// Why any way of sorting gives the reference's order: every ordering involved is TOTAL.  alnreg_hlt / alnreg_hlt2 end in
// hash_64(id + i), and hash_64 is a bijection of 64-bit words (each of its eight steps is invertible), so two hits of one list never
// compare equal; the ends of mem_pair are ordered by (position, score, index in the list, strand, read), and (index, read) names an
// end.  A hit's rank is therefore the number of hits that compare smaller, whatever the method (here: counting).
// mem_pair visits its pairings through windows over the sorted ends; its outcome is a function of the SET of pairings -- the maximum
// of (key, ranks), the best score among the others, how many of the others lie within `gap` of that -- so the lanes visit all
// n_pri[0] x n_pri[1] combinations and keep those the windows would have reached (the earlier end first, low <= dist <= high of the
// orientation strand_k << 1 | strand_i, that orientation not failed).
//
// No transcendental function runs here: log and erfc of the device library need not round like the host's libm, and every such call
// of the flow has an integer argument.  The host tabulates, per call: the insert-size term of a pairing per live orientation over
// dist in [low, high]; log(v) over the spans and seed coverages of the batch; the thresholds of the step function
// (int)(4.343 log(n + 1) + .499).  The arithmetic around them rounds after every operation, as the host's object code does.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
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

#pragma clang fp contract(off)      /* x * y + z rounds twice, as in sam_tail.cpp's object code (no FMA there); holds to the end of the file */

#define DC_LIGHT_MAX 16             // hits of a pair (both lists) the row form takes
#define DC_HEAVY_LDS 96             // hits of a pair the wavefront form keeps in LDS
#define DC_LIGHT_THREADS 128
#define DC_TAB_MAX (1 << 22)

enum { DC_F_NOPAIRING = 0x4, DC_F_PRIMARY5 = 0x800 };

struct DcIn { int64_t rb, re; int32_t qb, qe, rid, score, csub, sub_n, seedcov, is_alt; float frac_rep; int32_t pad; };     // 56 B up per hit
struct DcOut { uint64_t hash; int32_t orig, sub, alt_sc, sub_n, secondary, secondary_all; };                              // 32 B down per hit
struct DcHit {                      // a hit while its pair is being decided (96 B)
    int64_t rb, re; uint64_t hash, epos;
    int32_t qb, qe, rid, score, csub, sub_n, seedcov, is_alt; float frac_rep;
    int32_t sub, alt_sc, secondary, secondary_all, orig, tmp, erank;
};
struct DcPrm {
    const DcIn *in; DcOut *out; const int64_t *hit_off; bm2_pairplan_t *plans; const int64_t *ann_off;
    int64_t l_pac, first_pair;
    int32_t n_pairs, a, b, o_del, e_del, o_ins, e_ins, min_seed_len;
    float mask_level, coef_len;
    int32_t T, flag, pen_unpaired, coef_fac;
    int32_t low[4], high[4], failed[4]; int64_t tab_off[4];
    const double *ptab, *logtab; const int64_t *step_thr; int32_t log_n, n_step;
    const int32_t *heavy_list; const int64_t *heavy_at, *work_off; DcHit *work; int32_t n_heavy, pad;
};

// the group, the rankings, mem_mark_primary_se and mem_reorder_primary5 (shared with semark.hip); what they take of a DcIn beyond the fields they set
static __device__ __forceinline__ void dc_load(DcHit &h, const DcIn &s) {
    h.rb = s.rb; h.re = s.re; h.qb = s.qb; h.qe = s.qe; h.rid = s.rid; h.score = s.score; h.csub = s.csub; h.sub_n = s.sub_n;
    h.seedcov = s.seedcov; h.is_alt = s.is_alt; h.frac_rep = s.frac_rep; h.erank = 0; h.epos = 0;
}
#include "mark_dev.h"
// (int)x as the host's cvttsd2si delivers it: INT_MIN for a NaN and for anything outside the range
static __device__ __forceinline__ int dc_d2i(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT_MIN; }
static __device__ __forceinline__ double dc_log(const DcPrm &P, int v) { return (v < 0 || v > P.log_n) ? (double)NAN : P.logtab[v]; }
// (int)(4.343 * log(n + 1) + .499) for n >= 1: a step function of n, given by the smallest n of every step
static __device__ __forceinline__ int dc_step(const DcPrm &P, int n) {
    int lo = 0, hi = P.n_step;                                   // step_thr ascends; the answer is how many thresholds are <= n
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (P.step_thr[mid] <= (int64_t)n) lo = mid + 1; else hi = mid; }
    return lo;
}
static __device__ __forceinline__ int dc_raw_mapq(int diff, int a) { return dc_d2i(6.02 * diff / a + .499); }

static __device__ int dc_approx_mapq_se(const DcPrm &P, const DcHit &a) {                // mem_approx_mapq_se, bwamem.cpp:1470-1494
    int mapq, l, sub = a.sub ? a.sub : P.min_seed_len * P.a;
    double identity;
    sub = a.csub > sub ? a.csub : sub;
    if (sub >= a.score) return 0;
    l = a.qe - a.qb > a.re - a.rb ? a.qe - a.qb : (int)(a.re - a.rb);
    identity = 1. - (double)(l * P.a - a.score) / (P.a + P.b) / l;
    if (a.score == 0) mapq = 0;
    else if (P.coef_len > 0) {
        double tmp = l < P.coef_len ? 1. : P.coef_fac / dc_log(P, l);
        tmp *= identity * identity;
        mapq = dc_d2i(6.02 * (a.score - sub) / P.a * tmp * tmp + .499);
    } else {
        mapq = dc_d2i(30.0 * (1. - (double)sub / a.score) * dc_log(P, a.seedcov) + .499);
        mapq = identity < 0.95 ? dc_d2i(mapq * identity * identity + .499) : mapq;
    }
    if (a.sub_n > 0) mapq -= dc_step(P, a.sub_n);
    if (mapq > 60) mapq = 60;
    if (mapq < 0) mapq = 0;
    mapq = dc_d2i(mapq * (1. - a.frac_rep) + .499);
    return mapq;
}


struct DcPairing { uint64_t key, ranks; int q; };
// the pairing of hit x of read 1 with hit y of read 2, if mem_pair's windows reach it
static __device__ __forceinline__ bool dc_pairing(const DcPrm &P, const DcHit &h0, const DcHit &h1, uint64_t idw, DcPairing &o) {
    const bool first0 = h0.erank < h1.erank;
    const DcHit &k = first0 ? h0 : h1, &i = first0 ? h1 : h0;
    const int dir = (k.rb >= P.l_pac ? 2 : 0) | (i.rb >= P.l_pac ? 1 : 0);
    if (P.failed[dir]) return false;
    const int64_t dist = (int64_t)(i.epos - k.epos);
    if (dist < (int64_t)P.low[dir] || dist > (int64_t)P.high[dir]) return false;
    const double term = P.ptab[P.tab_off[dir] + (dist - (int64_t)P.low[dir])];
    int q = dc_d2i((uint64_t)(uint32_t)i.score + (uint64_t)(uint32_t)k.score + term + .499);
    if (q < 0) q = 0;
    o.q = q;
    o.ranks = (uint64_t)(uint32_t)k.erank << 32 | (uint64_t)(uint32_t)i.erank;
    o.key = (uint64_t)(uint32_t)q << 32 | (dc_hash_64(o.ranks ^ idw) & 0xffffffffU);
    return true;
}

template <int W> static __device__ void decide_pair(const Grp<W> &G, const DcPrm &P, int p, DcHit *A, DcHit *B) {
    const int64_t o0 = P.hit_off[2 * (int64_t)p], o1 = P.hit_off[2 * (int64_t)p + 1], o2 = P.hit_off[2 * (int64_t)p + 2];
    const int n[2] = { (int)(o1 - o0), (int)(o2 - o1) };
    DcHit *a[2] = { A, A + n[0] };
    const uint64_t id = (uint64_t)(P.first_pair + p);
    int n_pri[2];
    n_pri[0] = dc_mark_primary<W>(G, P, n[0], P.in + o0, a[0], B, (int64_t)(id << 1 | 0));
    n_pri[1] = dc_mark_primary<W>(G, P, n[1], P.in + o1, a[1], B + n[0], (int64_t)(id << 1 | 1));
    if (P.flag & DC_F_PRIMARY5) { dc_reorder_primary5<W>(G, P.T, n[0], a[0]); dc_reorder_primary5<W>(G, P.T, n[1], a[1]); }
    bm2_pairplan_t plan;
    plan.z[0] = plan.z[1] = 0; plan.n_pri[0] = n_pri[0]; plan.n_pri[1] = n_pri[1]; plan.q_se[0] = plan.q_se[1] = 0; plan.extra_flag = 1; plan.paired = 0;
    bool go = !(P.flag & DC_F_NOPAIRING) && n_pri[0] && n_pri[1];
    int o = 0, subo = 0, n_sub = 0;
    if (go) {                                                    // mem_pair (bwamem_pair.cpp:285-346)
        const int m = n_pri[0] + n_pri[1];
        auto end_of = [&](int e) -> DcHit & { return e < n_pri[0] ? a[0][e] : a[1][e - n_pri[0]]; };
        for (int e = G.lane; e < m; e += W) {
            DcHit &h = end_of(e);
            const int64_t fwd = h.rb >= P.l_pac ? (P.l_pac << 1) - 1 - h.rb : h.rb;
            h.epos = (uint64_t)(int64_t)h.rid << 32 | ((uint64_t)fwd - (uint64_t)P.ann_off[h.rid]);
        }
        grp_sync<W>();
        for (int e = G.lane; e < m; e += W) {                    // the rank of every end in (position, score, index, strand, read)
            const DcHit &h = end_of(e);
            const int rd = e >= n_pri[0], idx = rd ? e - n_pri[0] : e, st = h.rb >= P.l_pac;
            int r = 0;
            for (int f = 0; f < m; ++f) {
                const DcHit &g = end_of(f);
                const int rd2 = f >= n_pri[0], idx2 = rd2 ? f - n_pri[0] : f, st2 = g.rb >= P.l_pac;
                bool less;
                if (g.epos != h.epos) less = g.epos < h.epos;
                else if (g.score != h.score) less = (uint32_t)g.score < (uint32_t)h.score;
                else if (idx2 != idx) less = idx2 < idx;
                else if (st2 != st) less = st2 < st;
                else less = rd2 < rd;
                r += less ? 1 : 0;
            }
            end_of(e).erank = r;
        }
        grp_sync<W>();
        const uint64_t idw = (uint64_t)(int64_t)(int32_t)((uint32_t)id << 8);        // (int)id << 8, sign-extended; the shift wraps
        const int64_t combos = (int64_t)n_pri[0] * n_pri[1];
        DcPairing best = { 0, 0, 0 }, c;
        uint64_t mine = 0; int bx = 0, by = 0;
        for (int64_t t = G.lane; t < combos; t += W) {
            const int x = (int)(t / n_pri[1]), y = (int)(t % n_pri[1]);
            if (!dc_pairing(P, a[0][x], a[1][y], idw, c)) continue;
            if (!mine || c.key > best.key || (c.key == best.key && c.ranks > best.ranks)) { best = c; bx = x; by = y; }
            ++mine;
        }
        const uint64_t total = G.sum(mine);
        if (total == 0) go = false;
        else {
            const uint64_t best_key = G.max(mine ? best.key : 0);
            const uint64_t best_ranks = G.max(mine && best.key == best_key ? best.ranks : 0);      // (ranks of a pairing are >= 1)
            if (mine && best.key == best_key && best.ranks == best_ranks) { G.red[W] = (uint64_t)(uint32_t)bx << 32 | (uint32_t)by; }
            grp_sync<W>();
            const uint64_t zz = G.red[W];
            grp_sync<W>();
            plan.z[0] = (int)(zz >> 32); plan.z[1] = (int)(zz & 0xffffffffU);
            o = (int)(best_key >> 32);
            if (total > 1) {
                int second = -1;
                for (int64_t t = G.lane; t < combos; t += W)
                    if (dc_pairing(P, a[0][(int)(t / n_pri[1])], a[1][(int)(t % n_pri[1])], idw, c) && c.ranks != best_ranks && c.q > second) second = c.q;
                second = (int)G.max((uint64_t)(second + 1)) - 1;
                int gap = P.a + P.b;
                if (gap < P.o_del + P.e_del) gap = P.o_del + P.e_del;
                if (gap < P.o_ins + P.e_ins) gap = P.o_ins + P.e_ins;
                uint64_t near = 0;
                for (int64_t t = G.lane; t < combos; t += W)
                    if (dc_pairing(P, a[0][(int)(t / n_pri[1])], a[1][(int)(t % n_pri[1])], idw, c) && c.ranks != best_ranks && second - c.q <= gap) ++near;
                subo = second; n_sub = (int)G.sum(near);
            }
            if (o <= 0) go = false;
        }
    }
    if (go)                                                      // a second primary hit above the threshold: the reads go out one by one
        for (int i = 0; i < 2 && go; ++i) {
            uint64_t any = 0;
            for (int j = 1 + G.lane; j < n_pri[i]; j += W) if (a[i][j].secondary < 0 && a[i][j].score >= P.T) any = 1;
            if (G.max(any)) go = false;
        }
    if (go && G.lane == 0) {
        int *z = plan.z, *q_se = plan.q_se;
        plan.paired = 1;
        const int score_un = a[0][0].score + a[1][0].score - P.pen_unpaired;
        subo = subo > score_un ? subo : score_un;
        int q_pe = dc_raw_mapq(o - subo, P.a);
        if (n_sub > 0) q_pe -= dc_step(P, n_sub);
        if (q_pe < 0) q_pe = 0;
        if (q_pe > 60) q_pe = 60;
        q_pe = dc_d2i(q_pe * (1. - .5 * (a[0][0].frac_rep + a[1][0].frac_rep)) + .499);
        if (o > score_un) {
            DcHit *c[2] = { &a[0][z[0]], &a[1][z[1]] };
            for (int i = 0; i < 2; ++i) {
                if (c[i]->secondary >= 0) { c[i]->sub = a[i][c[i]->secondary].score; c[i]->secondary = -2; }
                q_se[i] = dc_approx_mapq_se(P, *c[i]);
            }
            q_se[0] = q_se[0] > q_pe ? q_se[0] : q_pe < q_se[0] + 40 ? q_pe : q_se[0] + 40;
            q_se[1] = q_se[1] > q_pe ? q_se[1] : q_pe < q_se[1] + 40 ? q_pe : q_se[1] + 40;
            plan.extra_flag |= 2;
            q_se[0] = q_se[0] < dc_raw_mapq(c[0]->score - c[0]->csub, P.a) ? q_se[0] : dc_raw_mapq(c[0]->score - c[0]->csub, P.a);
            q_se[1] = q_se[1] < dc_raw_mapq(c[1]->score - c[1]->csub, P.a) ? q_se[1] : dc_raw_mapq(c[1]->score - c[1]->csub, P.a);
        } else {
            z[0] = z[1] = 0;
            q_se[0] = dc_approx_mapq_se(P, a[0][0]);
            q_se[1] = dc_approx_mapq_se(P, a[1][0]);
        }
        for (int i = 0; i < 2; ++i) {
            const int k = a[i][z[i]].secondary_all;
            if (k >= 0 && k < n_pri[i]) {                        // switch secondary and primary if both are non-ALT
                for (int j = 0; j < n[i]; ++j)
                    if (a[i][j].secondary_all == k || j == k) a[i][j].secondary_all = z[i];
                a[i][z[i]].secondary_all = -1;
            }
        }
    }
    if (G.lane == 0) P.plans[p] = plan;
    grp_sync<W>();
    for (int i = G.lane; i < n[0] + n[1]; i += W) {              // what the host needs to reorder and annotate its hits
        const DcHit &h = A[i];
        DcOut r; r.hash = h.hash; r.orig = h.orig; r.sub = h.sub; r.alt_sc = h.alt_sc; r.sub_n = h.sub_n; r.secondary = h.secondary; r.secondary_all = h.secondary_all;
        P.out[o0 + i] = r;
    }
}

__global__ void k_decide_class(const int64_t *__restrict__ hit_off, int n_pairs, int32_t *__restrict__ heavy, int32_t *__restrict__ wsize) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const int64_t tot = hit_off[2 * (int64_t)p + 2] - hit_off[2 * (int64_t)p];
    heavy[p] = tot > DC_LIGHT_MAX;
    wsize[p] = tot > DC_HEAVY_LDS ? (int32_t)tot : 0;
}
__global__ void k_decide_list(const int32_t *__restrict__ heavy, const int64_t *__restrict__ heavy_at, int n_pairs, int32_t *__restrict__ list) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    if (heavy[p]) list[heavy_at[p]] = p;
}
__global__ __launch_bounds__(DC_LIGHT_THREADS) void k_decide_light(DcPrm P) {
    __shared__ DcHit lds[DC_LIGHT_THREADS / 16][2 * DC_LIGHT_MAX];
    __shared__ uint64_t red[DC_LIGHT_THREADS / 16][16 + 1];
    const int row = threadIdx.x >> 4;
    const int64_t p = (int64_t)blockIdx.x * (DC_LIGHT_THREADS / 16) + row;
    if (p >= P.n_pairs) return;                                  // (row-uniform, like everything below)
    if (P.hit_off[2 * p + 2] - P.hit_off[2 * p] > DC_LIGHT_MAX) return;
    Grp<16> G; G.red = red[row]; G.lane = threadIdx.x & 15;
    decide_pair<16>(G, P, (int)p, lds[row], lds[row] + DC_LIGHT_MAX);
}
__global__ __launch_bounds__(64) void k_decide_heavy(DcPrm P) {
    __shared__ DcHit lds[2 * DC_HEAVY_LDS];
    __shared__ uint64_t red[64 + 1];
    if ((int)blockIdx.x >= P.n_heavy) return;
    const int p = P.heavy_list[blockIdx.x];
    const int64_t tot = P.hit_off[2 * (int64_t)p + 2] - P.hit_off[2 * (int64_t)p];
    Grp<64> G; G.red = red; G.lane = threadIdx.x;
    DcHit *A = lds, *B = lds + DC_HEAVY_LDS;
    if (tot > DC_HEAVY_LDS) { A = P.work + 2 * P.work_off[p]; B = A + tot; }
    decide_pair<64>(G, P, p, A, B);
}

// ---- the resident form (BM2_SAM_F_DEVICE_RESCUE | BM2_SAM_F_DEVICE_DECIDE): the lists lie in HBM where rescue.hip's gather left them
// k_decide_pack: what the host's pack loop does, a lane per hit; stat[0] = the largest argument log will see, stat[1] = 1 + a hit on no contig
__global__ void k_decide_pack(const bm2_alnreg_t *__restrict__ H, int64_t n_hits, int n_seqs, DcIn *__restrict__ in, int *__restrict__ stat) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_hits) return;
    const bm2_alnreg_t &h = H[i];
    DcIn d;
    d.rb = h.rb; d.re = h.re; d.qb = h.qb; d.qe = h.qe; d.rid = h.rid; d.score = h.score; d.csub = h.csub; d.sub_n = h.sub_n;
    d.seedcov = h.seedcov; d.is_alt = h.is_alt; d.frac_rep = h.frac_rep; d.pad = 0;
    in[i] = d;
    const int64_t sr = h.re - h.rb;
    int64_t top = h.qe - h.qb > sr ? h.qe - h.qb : (int64_t)(int)sr;
    if (h.seedcov > top) top = h.seedcov;
    if (top > DC_TAB_MAX) top = DC_TAB_MAX + 1;
    if (top > 0) atomicMax(stat, (int)top);
    if (h.rid < 0 || h.rid >= n_seqs) atomicMax(stat + 1, (int)(i < 0x7ffffffe ? i + 1 : 0x7fffffff));
}
// k_decide_permute: what the host's apply loop does, a 16-lane row per list: every list in the decided order, the six rewritten fields from
// the kernels, everything else with its hit.  stat[2] = 1 + a pair whose permutation is broken.
__global__ __launch_bounds__(256) void k_decide_permute(const bm2_alnreg_t *__restrict__ H, const DcOut *__restrict__ out, const int64_t *__restrict__ hit_off,
                                                        int64_t n_lists, bm2_alnreg_t *__restrict__ fin, int *__restrict__ stat) {
    const int64_t li = (int64_t)blockIdx.x * (256 / 16) + (threadIdx.x >> 4);
    if (li >= n_lists) return;
    const int64_t b0 = hit_off[li], k = hit_off[li + 1] - b0;
    for (int64_t i = threadIdx.x & 15; i < k; i += 16) {
        const DcOut r = out[b0 + i];
        if (r.orig < 0 || r.orig >= k) { atomicMax(stat + 2, (int)((li >> 1) + 1)); continue; }
        bm2_alnreg_t h = H[b0 + r.orig];
        h.hash = r.hash; h.sub = r.sub; h.alt_sc = r.alt_sc; h.sub_n = r.sub_n; h.secondary = r.secondary; h.secondary_all = r.secondary_all;
        fin[b0 + i] = h;
    }
}

namespace {
std::atomic<long long> g_dc_pairs{0}, g_dc_hits{0}, g_dc_heavy{0};

// (int)(4.343 * log(n + 1) + .499) with the host's log: the smallest n >= 1 of every step (the function does not descend)
void step_thresholds(std::vector<int64_t> &thr) {
    auto f = [](int64_t n) { return (int)(4.343 * log((double)(n + 1)) + .499); };
    const int64_t top = 0x7ffffffe;
    thr.clear();
    for (int s = 1; s <= f(top); ++s) {
        int64_t lo = 0, hi = top;                                // the smallest n with f(n) >= s
        while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (f(mid) >= s) hi = mid; else lo = mid + 1; }
        thr.push_back(lo);
    }
}

// d_hits / d_off = NULL: the lists come from and go back to `hits` (host).  Otherwise the resident form: d_hits[hit_off[0] ..] and d_off (the
// offsets from 0, as hit_off minus hit_off[0]) lie in HBM already, hit_off is their host copy, and the decided lists are written to `hits`.
int decide_run(bm2_ctx *c, const char *who, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, bm2_alnreg_t *hits, const int64_t *hit_off,
               int64_t first_pair, const bm2_pestat pes[4], bm2_pairplan_t *plans, const bm2_alnreg_t *d_hits = nullptr, const int64_t *d_off = nullptr) {
    if (n_pairs == 0) return BM2_OK;
    int rc = bm2_check(hipSetDevice(c->device), "hipSetDevice");
    if (rc) return rc;
    TailProf prof("pe_decide_dev");
    const int64_t n_lists = 2 * (int64_t)n_pairs, base = hit_off[0], n_hits = hit_off[n_lists] - base;
    bm2_alnreg_t *const H = hits + base;
    const int nt = bm2_host_threads();
    // the offsets from 0; what the kernels will bin (known here from the offsets alone: the buffers are sized without a round trip)
    std::vector<int64_t> off((size_t)n_lists + 1);
    int64_t n_heavy = 0, work_hits = 0;
    for (int64_t i = 0; i <= n_lists; ++i) off[(size_t)i] = hit_off[i] - base;
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t tot = off[(size_t)(2 * p + 2)] - off[(size_t)(2 * p)];
        if (tot > 0x3fffffff) { bm2_set_error("%s: pair %lld has too many hits", who, (long long)p); return BM2_EINVAL; }
        n_heavy += tot > DC_LIGHT_MAX; if (tot > DC_HEAVY_LDS) work_hits += tot;
    }
    // pack: the 52 bytes of a hit the decisions read; on the way the largest argument log will see and the contigs' range
    static thread_local std::vector<DcIn> in_of_this_thread;
    static thread_local std::vector<DcOut> out_of_this_thread;
    std::vector<DcIn> &in = in_of_this_thread;
    std::vector<DcOut> &out = out_of_this_thread;
    if (in.size() < (size_t)n_hits + 1) in.resize((size_t)n_hits + 1);
    if (out.size() < (size_t)n_hits + 1) out.resize((size_t)n_hits + 1);
    std::atomic<int64_t> log_top(0), bad_rid(-1);
    const int n_seqs = c->ix.n_seqs;
    int *d_stat = nullptr;
    if (d_hits) {                                                // pack on the device; two numbers come back
        if ((rc = bm2_reserve(c->b_dc_pack, up256((size_t)n_hits * sizeof(DcIn)) + 512))) return rc;
        d_stat = (int *)((char *)c->b_dc_pack.p + up256((size_t)n_hits * sizeof(DcIn)));
        if ((rc = bm2_check(hipMemsetAsync(d_stat, 0, 16, c->stream), "memset decide stat"))) return rc;
        if (n_hits) {
            hipLaunchKernelGGL(k_decide_pack, dim3((unsigned)((n_hits + 255) / 256)), dim3(256), 0, c->stream, d_hits, n_hits, n_seqs, (DcIn *)c->b_dc_pack.p, d_stat);
            if ((rc = bm2_check(hipGetLastError(), "k_decide_pack launch"))) return rc;
        }
        int st[4] = { 0, 0, 0, 0 };
        if ((rc = bm2_check(hipMemcpyAsync(st, d_stat, 16, hipMemcpyDeviceToHost, c->stream), "D2H decide stat"))) return rc;
        if ((rc = bm2_check(hipStreamSynchronize(c->stream), "k_decide_pack"))) return rc;
        log_top = st[0];
        if (st[1]) { bm2_set_error("%s: hit %d lies on no contig of the context's index", who, st[1] - 1); return BM2_EINVAL; }
    } else bm2_parallel_ranges(n_hits, 32768, nt, [&](int64_t lo, int64_t hi) {
        int64_t top = 0;
        for (int64_t i = lo; i < hi; ++i) {
            const bm2_alnreg_t &h = H[i];
            DcIn &d = in[(size_t)i];
            d.rb = h.rb; d.re = h.re; d.qb = h.qb; d.qe = h.qe; d.rid = h.rid; d.score = h.score; d.csub = h.csub; d.sub_n = h.sub_n;
            d.seedcov = h.seedcov; d.is_alt = h.is_alt; d.frac_rep = h.frac_rep; d.pad = 0;
            const int l = h.qe - h.qb > h.re - h.rb ? h.qe - h.qb : (int)(h.re - h.rb);
            if (l > top) top = l;
            if (h.seedcov > top) top = h.seedcov;
            if (h.rid < 0 || h.rid >= n_seqs) { int64_t e = -1; bad_rid.compare_exchange_strong(e, i); }
        }
        int64_t seen = log_top.load();
        while (top > seen && !log_top.compare_exchange_weak(seen, top)) {}
    });
    if (!d_hits && bad_rid.load() >= 0) { bm2_set_error("%s: hit %lld lies on no contig of the context's index (rid %d)", who, (long long)bad_rid.load(), H[bad_rid.load()].rid); return BM2_EINVAL; }
    if (log_top.load() > DC_TAB_MAX) { bm2_set_error("%s: a hit spans %lld bases (or has that seed coverage); above 2^22 the device form has no table of log", who, (long long)log_top.load()); return BM2_EUNSUP; }
    prof.mark("pack");
    // tables (the host's libm): the insert-size term of a pairing, log, the steps of 4.343 log(n + 1)
    DcPrm P;
    memset(&P, 0, sizeof P);
    int64_t span = 0;
    for (int d = 0; d < 4; ++d) {
        P.low[d] = pes[d].low; P.high[d] = pes[d].high; P.failed[d] = pes[d].failed; P.tab_off[d] = span;
        if (!pes[d].failed && pes[d].high >= pes[d].low) span += (int64_t)pes[d].high - pes[d].low + 1;
        if (span > DC_TAB_MAX) { bm2_set_error("%s: the insert-size ranges [low, high] of the live orientations hold more than 2^22 distances together; the device form tabulates them", who); return BM2_EUNSUP; }
    }
    const int log_n = (int)log_top.load();
    std::vector<int64_t> thr;
    step_thresholds(thr);
    static thread_local std::vector<double> tab_of_this_thread;
    std::vector<double> &tab = tab_of_this_thread;
    if (tab.size() < (size_t)span + (size_t)log_n + 2) tab.resize((size_t)span + (size_t)log_n + 2);
    for (int d = 0; d < 4; ++d) {
        if (pes[d].failed || pes[d].high < pes[d].low) continue;
        const bm2_pestat &m = pes[d];
        double *t = tab.data() + P.tab_off[d];
        bm2_parallel_ranges((int64_t)m.high - m.low + 1, 4096, nt, [&](int64_t lo, int64_t hi) {
            for (int64_t k = lo; k < hi; ++k) {
                const int64_t dist = (int64_t)m.low + k;
                const double ns = (dist - m.avg) / m.std;
                t[k] = .721 * log(2. * erfc(fabs(ns) * M_SQRT1_2)) * opt->a;
            }
        });
    }
    for (int v = 0; v <= log_n; ++v) tab[(size_t)span + (size_t)v] = log((double)v);
    prof.mark("tables");
    // device buffers
    const size_t in_b = d_hits ? 0 : up256((size_t)n_hits * sizeof(DcIn)), off_b = up256((size_t)(n_lists + 1) * 8), tab_b = up256(((size_t)span + (size_t)log_n + 1) * 8),
                 thr_b = up256(thr.size() * 8);
    const size_t out_b = up256((size_t)n_hits * sizeof(DcOut)), plan_b = up256((size_t)n_pairs * sizeof(bm2_pairplan_t));
    const size_t flag_b = up256((size_t)n_pairs * 4), at_b = up256((size_t)(n_pairs + 1) * 8), list_b = up256((size_t)(n_heavy + 1) * 4),
                 work_b = up256((size_t)work_hits * 2 * sizeof(DcHit));
    if ((rc = bm2_reserve(c->b_dc_in, in_b + off_b + tab_b + thr_b + 256))) return rc;
    if ((rc = bm2_reserve(c->b_dc_out, out_b + plan_b + 256))) return rc;
    if ((rc = bm2_reserve(c->b_dc_work, 2 * flag_b + 2 * at_b + list_b + work_b + 256))) return rc;
    char *d = (char *)c->b_dc_in.p;
    P.in = d_hits ? (const DcIn *)c->b_dc_pack.p : (const DcIn *)d; P.hit_off = d_off ? d_off : (const int64_t *)(d + in_b); P.ptab = (const double *)(d + in_b + off_b); P.logtab = P.ptab + span;
    P.step_thr = (const int64_t *)(d + in_b + off_b + tab_b);
    P.out = (DcOut *)c->b_dc_out.p; P.plans = (bm2_pairplan_t *)((char *)c->b_dc_out.p + out_b);
    char *w = (char *)c->b_dc_work.p;
    int32_t *d_heavy = (int32_t *)w, *d_wsize = (int32_t *)(w + flag_b);
    int64_t *d_heavy_at = (int64_t *)(w + 2 * flag_b), *d_work_off = (int64_t *)(w + 2 * flag_b + at_b);
    int32_t *d_list = (int32_t *)(w + 2 * flag_b + 2 * at_b);
    // (ix.ann_offset: d_ann_off of the context that owns the replica; a shared context reaches it through ix)
    P.heavy_list = d_list; P.heavy_at = d_heavy_at; P.work_off = d_work_off; P.work = (DcHit *)(w + 2 * flag_b + 2 * at_b + list_b); P.n_heavy = (int32_t)n_heavy;
    P.ann_off = c->ix.ann_offset; P.l_pac = c->ix.l_pac; P.first_pair = first_pair; P.n_pairs = n_pairs;
    P.a = opt->a; P.b = opt->b; P.o_del = opt->o_del; P.e_del = opt->e_del; P.o_ins = opt->o_ins; P.e_ins = opt->e_ins; P.min_seed_len = opt->min_seed_len;
    P.mask_level = opt->mask_level; P.coef_len = so->mapQ_coef_len; P.T = so->T; P.flag = so->flag; P.pen_unpaired = so->pen_unpaired; P.coef_fac = so->mapQ_coef_fac;
    P.log_n = log_n; P.n_step = (int32_t)thr.size();
    if (!d_hits && n_hits && (rc = bm2_copy_h2d(c, (void *)P.in, in.data(), (size_t)n_hits * sizeof(DcIn)))) return rc;
    if (!d_off && (rc = bm2_copy_h2d(c, (void *)P.hit_off, off.data(), (size_t)(n_lists + 1) * 8))) return rc;
    if ((rc = bm2_copy_h2d(c, (void *)P.ptab, tab.data(), ((size_t)span + (size_t)log_n + 1) * 8))) return rc;
    if ((rc = bm2_copy_h2d(c, (void *)P.step_thr, thr.data(), thr.size() * 8))) return rc;
    prof.mark("H2D");
    const unsigned g256 = (unsigned)((n_pairs + 255) / 256);
    hipLaunchKernelGGL(k_decide_class, dim3(g256), dim3(256), 0, c->stream, P.hit_off, n_pairs, d_heavy, d_wsize);
    if ((rc = bm2_check(hipGetLastError(), "k_decide_class launch"))) return rc;
    if ((rc = bm2_scan_i32(c, d_heavy, n_pairs, d_heavy_at, c->b_dc_scan))) return rc;
    if ((rc = bm2_scan_i32(c, d_wsize, n_pairs, d_work_off, c->b_dc_scan2))) return rc;
    hipLaunchKernelGGL(k_decide_list, dim3(g256), dim3(256), 0, c->stream, (const int32_t *)d_heavy, (const int64_t *)d_heavy_at, n_pairs, d_list);
    if ((rc = bm2_check(hipGetLastError(), "k_decide_list launch"))) return rc;
    const int per_block = DC_LIGHT_THREADS / 16;
    hipLaunchKernelGGL(k_decide_light, dim3((unsigned)((n_pairs + per_block - 1) / per_block)), dim3(DC_LIGHT_THREADS), 0, c->stream, P);
    if ((rc = bm2_check(hipGetLastError(), "k_decide_light launch"))) return rc;
    if (n_heavy) {
        hipLaunchKernelGGL(k_decide_heavy, dim3((unsigned)n_heavy), dim3(64), 0, c->stream, P);
        if ((rc = bm2_check(hipGetLastError(), "k_decide_heavy launch"))) return rc;
    }
    int64_t heavy_seen = -1;
    if ((rc = bm2_check(hipMemcpyAsync(&heavy_seen, d_heavy_at + n_pairs, 8, hipMemcpyDeviceToHost, c->stream), "D2H heavy count"))) return rc;
    if ((rc = bm2_check(hipStreamSynchronize(c->stream), "k_decide"))) return rc;
    prof.mark("kernels");
    if (heavy_seen != n_heavy) { bm2_set_error("%s: the device binned %lld heavy pairs, the host counted %lld", who, (long long)heavy_seen, (long long)n_heavy); return BM2_ENODEV; }
    if (d_hits) {                                                // the permutation on the device, the decided lists down once
        if ((rc = bm2_reserve(c->b_dc_final, up256((size_t)n_hits * sizeof(bm2_alnreg_t)) + 256))) return rc;
        hipLaunchKernelGGL(k_decide_permute, dim3((unsigned)((n_lists + 15) / 16)), dim3(256), 0, c->stream, d_hits, (const DcOut *)P.out, P.hit_off, n_lists,
                           (bm2_alnreg_t *)c->b_dc_final.p, d_stat);
        if ((rc = bm2_check(hipGetLastError(), "k_decide_permute launch"))) return rc;
        int st[4] = { 0, 0, 0, 0 };
        if ((rc = bm2_check(hipMemcpyAsync(st, d_stat, 16, hipMemcpyDeviceToHost, c->stream), "D2H decide stat"))) return rc;
        if ((rc = bm2_check(hipStreamSynchronize(c->stream), "k_decide_permute"))) return rc;
        prof.mark("permute");
        if (st[2]) { bm2_set_error("%s: pair %d came back with a broken permutation", who, st[2] - 1); return BM2_ENODEV; }
        if (n_hits && (rc = bm2_copy_d2h(c, H, c->b_dc_final.p, (size_t)n_hits * sizeof(bm2_alnreg_t)))) return rc;
        if ((rc = bm2_copy_d2h(c, plans, P.plans, (size_t)n_pairs * sizeof(bm2_pairplan_t)))) return rc;
        prof.mark("D2H");
        g_dc_pairs += n_pairs; g_dc_hits += (long long)n_hits; g_dc_heavy += (long long)n_heavy;
        return BM2_OK;
    }
    if (n_hits && (rc = bm2_copy_d2h(c, out.data(), P.out, (size_t)n_hits * sizeof(DcOut)))) return rc;
    if ((rc = bm2_copy_d2h(c, plans, P.plans, (size_t)n_pairs * sizeof(bm2_pairplan_t)))) return rc;
    prof.mark("D2H");
    // in place: every list in the device's order, the six rewritten fields from the device, everything else with its hit
    std::atomic<int> bad(-1);
    bm2_parallel_ranges(n_lists, 4096, nt, [&](int64_t lo, int64_t hi) {
        std::vector<bm2_alnreg_t> old;
        for (int64_t li = lo; li < hi; ++li) {
            const int64_t b0 = off[(size_t)li], k = off[(size_t)li + 1] - b0;
            if (!k) continue;
            old.assign(H + b0, H + b0 + k);
            for (int64_t i = 0; i < k; ++i) {
                const DcOut &r = out[(size_t)(b0 + i)];
                if (r.orig < 0 || r.orig >= k) { int e = -1; bad.compare_exchange_strong(e, (int)(li >> 1)); continue; }
                bm2_alnreg_t &h = H[b0 + i];
                h = old[(size_t)r.orig];
                h.hash = r.hash; h.sub = r.sub; h.alt_sc = r.alt_sc; h.sub_n = r.sub_n; h.secondary = r.secondary; h.secondary_all = r.secondary_all;
            }
        }
    });
    prof.mark("apply");
    if (bad.load() >= 0) { bm2_set_error("%s: pair %d came back with a broken permutation", who, bad.load()); return BM2_ENODEV; }
    g_dc_pairs += n_pairs; g_dc_hits += (long long)n_hits; g_dc_heavy += (long long)n_heavy;
    return BM2_OK;
}
bool decide_ready(const bm2_ctx *c, const char *who) {
    if (!c || !c->has_index || !c->ix.ann_offset) { bm2_set_error("%s: the context holds no index", who); return false; }
    return true;
}
}  // namespace

// The decisions of pairs whose lists lie in HBM (rescue.hip calls this between its gather and its download): see decide_run.
int bm2h_decide_resident(bm2_ctx *c, const char *who, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *d_hits,
                         const int64_t *d_off, const int64_t *h_off, int64_t first_pair, const bm2_pestat pes[4], bm2_pairplan_t *plans, bm2_alnreg_t *out) {
    if (!decide_ready(c, who)) return BM2_EINVAL;
    return decide_run(c, who, opt, so, n_pairs, out, h_off, first_pair, pes, plans, d_hits, d_off);
}
void bm2h_decide_stats_reset() { g_dc_pairs = 0; g_dc_hits = 0; g_dc_heavy = 0; }

extern "C" void bm2_sam_decide_stats(int64_t *pairs, int64_t *hits, int64_t *pairs_heavy) {
    if (pairs) *pairs = g_dc_pairs.load();
    if (hits) *hits = g_dc_hits.load();
    if (pairs_heavy) *pairs_heavy = g_dc_heavy.load();
}

extern "C" int bm2_pe_decide_dev(bm2_ctx *c, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, bm2_alnreg_t *hits,
                                 const int64_t *hit_off, int64_t first_pair, const bm2_pestat pes[4], bm2_pairplan_t *plans) {
    if (!c || !opt || !so || n_pairs < 0 || !hit_off || !pes || (n_pairs > 0 && !plans)) { bm2_set_error("bm2_pe_decide_dev: bad argument"); return BM2_EINVAL; }
    if (!decide_ready(c, "bm2_pe_decide_dev")) return BM2_EINVAL;
    int rc = bm2h_check_hit_off("bm2_pe_decide_dev", n_pairs, hit_off);
    if (rc) return rc;
    if (hit_off[2 * (int64_t)n_pairs] > hit_off[0] && !hits) { bm2_set_error("bm2_pe_decide_dev: bad argument"); return BM2_EINVAL; }
    g_dc_pairs = 0; g_dc_hits = 0; g_dc_heavy = 0;
    return decide_run(c, "bm2_pe_decide_dev", opt, so, n_pairs, hits, hit_off, first_pair, pes, plans);
}

// ---- the hook of the SAM tail (bm2h_decide_batch_fn; user = bm2h_text_ctxs): the chunk's pairs cut into contiguous parts, one context
// and one host thread per part.  A pair's decisions depend on its own lists, its number and the chunk's model, so the parts do not
// depend on one another and the result does not depend on their number.
int bm2h_dev_decide_batch(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, bm2_alnreg_t *hits,
                          const int64_t *hit_off, int64_t first_pair, const bm2_pestat pes[4], bm2_pairplan_t *plans) {
    const bm2h_text_ctxs *m = (const bm2h_text_ctxs *)user;
    for (int g = 0; g < m->n; ++g) if (!decide_ready(m->ctx[g], "BM2_SAM_F_DEVICE_DECIDE")) return BM2_EINVAL;
    int rc = bm2h_check_hit_off("BM2_SAM_F_DEVICE_DECIDE", n_pairs, hit_off);
    if (rc) return rc;
    g_dc_pairs = 0; g_dc_hits = 0; g_dc_heavy = 0;
    const int G = bm2_parts(n_pairs, bm2_knob("BM2_DECIDE_PART", 65536), m->n);      // knob: pairs that are worth a context of their own (launch policy)
    if (G == 1) return decide_run(m->ctx[0], "BM2_SAM_F_DEVICE_DECIDE", opt, so, n_pairs, hits, hit_off, first_pair, pes, plans);
    return bm2_run_parts(G, bm2_part_budget(G), nullptr, [&](int g) {
        const int64_t lo = bm2_part_lo(n_pairs, g, G), hi = bm2_part_lo(n_pairs, g + 1, G);
        return decide_run(m->ctx[g], "BM2_SAM_F_DEVICE_DECIDE", opt, so, (int32_t)(hi - lo), hits, hit_off + 2 * lo, first_pair + lo, pes, plans + lo);
    });
}

bm2h_decide_scope::bm2h_decide_scope(bm2_ctx *const *ctx, int n) : bm2h_ctx_scope(ctx, n), hook(bm2h_dev_decide_batch, &tc) {}
