// cgplan.hip -- WHICH hits of a chunk's decided lists the text will ask mem_reg2aln for, on the device: the dry emit pass of the tail's
// CIGAR session (mem_gen_alt, bwamem_extra.cpp:118-183; mem_reg2sam, bwamem.cpp:1521-1577; the emit half of mem_sam_pe,
// bwamem_pair.cpp:487-551) as a function of four fields of a hit and the pair's plan.  Host oracle: bm2_cigar_plan, compared index for index.
//
//   k_cg_light   a 16-lane row per unit (a single-end list, or a pair's two lists) of up to 16 hits, the XA counters in LDS
//   k_cg_heavy   a wavefront per heavier unit: the counters of a list in LDS up to CG_LDS_CAP hits, in a global workspace carved per
//                wavefront beyond.  EVERY list is marked by one of the two; nothing goes back to the host.
//   k_cg_count / bm2_scan_i32 / k_cg_write   the marks (one byte per hit) compacted in hit order: sel and its length come down
// Both marking kernels run the SAME code (cg_list<W>): the lanes of a group stride over the hits of a list; the only data they hand each
// other are the counters cnt[r] (how many hits name r as their XA primary, bit 31: one of them is an ALT hit), added with non-returning
// atomics between two group barriers, so the order of the adds cannot show.  A mark is written by the lane that owns the hit.
//
// The two floating-point tests are one operation each (int -> double, a multiply by the float ratio widened on the host, a compare; int ->
// float, a float multiply, a compare), so IEEE arithmetic gives the host's answer; contraction is off for the file all the same.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/bm2.h"
#include "bm2_ctx.h"
#include "host_tail.h"
#include "host_pool.h"
#include "pipeline.h"

#pragma clang fp contract(off)

#define CG_LIGHT_MAX 16             // hits of a unit the row form takes
#define CG_LDS_CAP 256              // hits of a LIST whose counters the wavefront form keeps in LDS
#define CG_LIGHT_THREADS 256
#define CG_BLOCK_HITS 1024          // hits per block of the compaction: 256 lanes x 4 marks
#define CG_F_ALL 0x8

struct CgPrm {
    const bm2h_cg_mark *hits; const int64_t *hit_off; const bm2_pairplan_t *plans;      // offsets from 0; plans == NULL: single-end lists
    uint8_t *mark; int32_t *stat;                                                       // stat[0] = 1 + a unit with an index outside its list
    const int32_t *heavy_list; const int64_t *heavy_work; uint32_t *work;               // unit k of the wavefront form, its counters' place or -1
    double xa_ratio; float drop_ratio;
    int32_t n_units, n_heavy, per_unit, T, all, max_xa, max_xa_alt;
};

// ---- the group's barrier (decide.hip's): the lanes of a group belong to one wavefront and reach a barrier site together, so it has to
// order the memory operations around it.  LDS counters want workgroup scope; counters in the global workspace are added at the L2 and
// read there (agent-scope atomic loads), and the release before the barrier waits for the adds.
#ifdef BM2_EMU_ROW_PRIMS
template <int W> static __device__ __forceinline__ void cg_sync(bool) { if (W == 16) emu_rsync(); else emu_wsync(); }
#else
template <int W> static __device__ __forceinline__ void cg_sync(bool global) {
    if (global) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    if (global) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); else __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
#endif

// pri_idx of gen_alt: the hit whose XA value hit h goes into, or -1.  (k >= n is reported by the caller and never followed.)
static __device__ __forceinline__ int cg_pri(const CgPrm &P, const bm2h_cg_mark *a, int n, const bm2h_cg_mark &h) {
    const int k = h.secondary_all;
    if (k < 0 || k >= n) return -1;
    return (double)h.score >= (double)a[k].score * P.xa_ratio ? k : -1;
}

// One list a[0, n) with its marks m[0, n).  plan: an end of a pair, with `paired`, n_pri and z of its plan (by value: a plan kept in
// memory would be the wavefront form's only scratch); otherwise a single-end list.  cnt: n words, zero on entry when they lie in the
// global workspace (in_global), zeroed here when they are the group's LDS.
template <int W, bool in_global> static __device__ void cg_list(int lane, const CgPrm &P, const bm2h_cg_mark *a, int n, uint8_t *m, bool plan, bool paired,
                                                                 int n_pri, int z, uint32_t *cnt, int unit) {
    bool bad = (plan && (n_pri < 0 || n_pri > n)) || (paired && (z < 0 || z >= n));
    for (int i = lane; i < n; i += W) {
        const bm2h_cg_mark h = a[i];
        if ((h.secondary >= n && h.secondary != INT_MAX) || h.secondary_all >= n) bad = true;
        if (!P.all && !in_global) cnt[i] = 0;
    }
    if (bad) atomicMax(P.stat, unit + 1);
    if (!P.all) {                                                // gen_alt's counting loop
        cg_sync<W>(in_global);
        for (int i = lane; i < n; i += W) {
            const bm2h_cg_mark h = a[i];
            const int r = cg_pri(P, a, n, h);
            if (r < 0) continue;
            atomicAdd(&cnt[r], 1u);                              // (results unused: non-returning adds)
            if (h.is_alt) atomicOr(&cnt[r], 0x80000000u);
        }
        cg_sync<W>(in_global);
    }
    int which = -1;                                              // pe_emit, no_pairing: the mate's representative
    if (plan && !paired && n > 0) {
        if (a[0].score >= P.T) which = 0;
        else if (n_pri >= 0 && n_pri < n && a[n_pri].score >= P.T) which = n_pri;
    }
    for (int i = lane; i < n; i += W) {
        const bm2h_cg_mark h = a[i];
        bool want = false;
        if (!P.all) {
            const int r = cg_pri(P, a, n, h);
            if (r >= 0) {
                const uint32_t v = in_global ? __hip_atomic_load(&cnt[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ((volatile uint32_t *)cnt)[r];
                const int c = (int)(v & 0x7fffffffu);
                if (!(c > P.max_xa_alt || (!(v >> 31) && c > P.max_xa))) want = true;
            }
        }
        if (paired) {                                            // pe_emit: the chosen hit, and the first ALT hit when it is a primary one at or above T
            if (i == z) want = true;
            if (i == n_pri && h.score >= P.T && h.secondary < 0 && h.is_alt) want = true;
        } else {                                                 // reg2sam
            if (i == which) want = true;
            if (h.score >= P.T && !(h.secondary >= 0 && (h.is_alt || !P.all))) {
                bool drop = false;
                if (h.secondary >= 0 && h.secondary < n) drop = (float)h.score < (float)a[h.secondary].score * P.drop_ratio;
                if (!drop) want = true;
            }
        }
        m[i] = want ? 1 : 0;
    }
    if (!P.all && !in_global) cg_sync<W>(false);                 // (the LDS counters serve the unit's next list)
}

// an empty unit has no hit to mark, but a plan that points into it is still an error
static __device__ __forceinline__ void cg_empty_unit(const CgPrm &P, int u) {
    if (!P.plans) return;
    const bm2_pairplan_t pl = P.plans[u];
    if (pl.paired || pl.n_pri[0] || pl.n_pri[1]) atomicMax(P.stat, u + 1);
}

__global__ __launch_bounds__(CG_LIGHT_THREADS) void k_cg_light(CgPrm P) {
    __shared__ uint32_t cnt[CG_LIGHT_THREADS / 16][CG_LIGHT_MAX];
    const int row = threadIdx.x >> 4, lane = threadIdx.x & 15;
    const int64_t u = (int64_t)blockIdx.x * (CG_LIGHT_THREADS / 16) + row;
    if (u >= P.n_units) return;                                  // (row-uniform, like everything below)
    const int64_t l0 = u * P.per_unit, b0 = P.hit_off[l0], e1 = P.hit_off[l0 + P.per_unit];
    if (e1 - b0 > CG_LIGHT_MAX) return;
    if (e1 == b0) { if (lane == 0) cg_empty_unit(P, (int)u); return; }
    if (!P.plans) { cg_list<16, false>(lane, P, P.hits + b0, (int)(e1 - b0), P.mark + b0, false, false, 0, 0, cnt[row], (int)u); return; }
    const bm2_pairplan_t pl = P.plans[u];
    const int64_t b1 = P.hit_off[l0 + 1];
    cg_list<16, false>(lane, P, P.hits + b0, (int)(b1 - b0), P.mark + b0, true, pl.paired != 0, pl.n_pri[0], pl.z[0], cnt[row], (int)u);
    cg_list<16, false>(lane, P, P.hits + b1, (int)(e1 - b1), P.mark + b1, true, pl.paired != 0, pl.n_pri[1], pl.z[1], cnt[row], (int)u);
}
__global__ __launch_bounds__(64) void k_cg_heavy(CgPrm P) {
    __shared__ uint32_t cnt[CG_LDS_CAP];
    if ((int)blockIdx.x >= P.n_heavy) return;
    const int u = P.heavy_list[blockIdx.x], lane = threadIdx.x;
    const int64_t wk = P.heavy_work[blockIdx.x];
    const int64_t l0 = (int64_t)u * P.per_unit, b0 = P.hit_off[l0];
    const bool plan = P.plans != nullptr;
    for (int e = 0; e < P.per_unit; ++e) {
        const int64_t b = P.hit_off[l0 + e];
        const int n = (int)(P.hit_off[l0 + e + 1] - b);
        const bool paired = plan && P.plans[u].paired != 0;
        const int n_pri = plan ? P.plans[u].n_pri[e] : 0, z = plan ? P.plans[u].z[e] : 0;
        if (n > CG_LDS_CAP) cg_list<64, true>(lane, P, P.hits + b, n, P.mark + b, plan, paired, n_pri, z, P.work + wk + (b - b0), u);      // (wk >= 0: the host carved the unit's hits in words)
        else cg_list<64, false>(lane, P, P.hits + b, n, P.mark + b, plan, paired, n_pri, z, cnt, u);
    }
}

// ---- compaction: block b owns marks [b * CG_BLOCK_HITS, +CG_BLOCK_HITS), lane t the four marks of word b * 256 + t (the mark array is
// zero beyond the last hit up to a multiple of four)
static __device__ __forceinline__ uint32_t cg_marks4(const uint8_t *mark, int64_t n_hits, int64_t w) {
    return 4 * w < n_hits ? ((const uint32_t *)mark)[w] & 0x01010101u : 0u;
}
__global__ __launch_bounds__(256) void k_cg_count(const uint8_t *__restrict__ mark, int64_t n_hits, int32_t *__restrict__ bcnt) {
    __shared__ int32_t sh[256];
    sh[threadIdx.x] = __popc(cg_marks4(mark, n_hits, (int64_t)blockIdx.x * 256 + threadIdx.x));
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) { if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d]; __syncthreads(); }
    if (threadIdx.x == 0) bcnt[blockIdx.x] = sh[0];
}
// sel[boff[b] + rank in the block] = base + hit, for the ranks below cap
__global__ __launch_bounds__(256) void k_cg_write(const uint8_t *__restrict__ mark, int64_t n_hits, const int64_t *__restrict__ boff, int64_t base,
                                                  int32_t *__restrict__ sel, int64_t cap) {
    __shared__ int32_t sh[256];
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t v = cg_marks4(mark, n_hits, w);
    const int mine = __popc(v);
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int t = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    int64_t at = boff[blockIdx.x] + sh[threadIdx.x] - mine;
    for (int k = 0; k < 4; ++k)
        if ((v >> (8 * k)) & 1u) { if (at < cap) sel[at] = (int32_t)(base + 4 * w + k); ++at; }
}

namespace {
// The selection of one batch on one context.  hits[k] is hit hit_off[0] + k (packed); hit_off has n_lists + 1 checked entries and may
// start anywhere; sel speaks its numbering.  *heavy = units that took the wavefront form.
// d_hits / d_off != NULL: the resident form -- the packed hits and the offsets from 0 lie in HBM already (semark.hip's kernels left them),
// `hits` is not read and neither is uploaded.
int cgplan_run(bm2_ctx *c, const char *who, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_lists, const bm2h_cg_mark *hits, const int64_t *hit_off,
               const bm2_pairplan_t *plans, int32_t *sel, int64_t cap, int64_t *n_out, int64_t *heavy, int64_t first_unit = 0,
               const bm2h_cg_mark *d_hits = nullptr, const int64_t *d_off = nullptr) {
    *n_out = 0; *heavy = 0;
    if (n_lists == 0) return BM2_OK;
    if (hit_off[n_lists] > 0x7fffffff) { bm2_set_error("%s: hit numbers beyond 2^31 do not fit sel", who); return BM2_EUNSUP; }
    int rc = bm2_check(hipSetDevice(c->device), "hipSetDevice");
    if (rc) return rc;
    TailProf prof("cigar_plan_dev");
    const int per_unit = plans ? 2 : 1;
    const int64_t n_units = n_lists / per_unit, hbase = hit_off[0], n_hits = hit_off[n_lists] - hbase;
    // the units of the wavefront form and their share of the global workspace, known from the offsets alone
    const std::vector<int64_t> hoff = bm2h_hit_off_from0(hit_off, n_lists);
    std::vector<int32_t> heavy_list; std::vector<int64_t> heavy_work;
    int64_t work_words = 0;
    for (int64_t u = 0; u < n_units; ++u) {
        const int64_t b0 = hoff[(size_t)(u * per_unit)], tot = hoff[(size_t)((u + 1) * per_unit)] - b0;
        if (tot <= CG_LIGHT_MAX) continue;
        bool big = false;
        for (int e = 0; e < per_unit; ++e) big |= hoff[(size_t)(u * per_unit + e + 1)] - hoff[(size_t)(u * per_unit + e)] > CG_LDS_CAP;
        heavy_list.push_back((int32_t)u); heavy_work.push_back(big ? work_words : -1);
        if (big) work_words += tot;
    }
    const int64_t n_heavy = (int64_t)heavy_list.size(), nb = (n_hits + CG_BLOCK_HITS - 1) / CG_BLOCK_HITS, room = cap < n_hits ? cap : n_hits;
    prof.mark("pack");
    const size_t in_b = d_hits ? 0 : up256((size_t)n_hits * sizeof(bm2h_cg_mark)), off_b = up256((size_t)(n_lists + 1) * 8), plan_b = up256(plans ? (size_t)n_units * sizeof(bm2_pairplan_t) : 0),
                 hl_b = up256((size_t)n_heavy * 4), hw_b = up256((size_t)n_heavy * 8);
    const size_t mark_b = up256((size_t)n_hits + 4), stat_b = 256, bcnt_b = up256((size_t)(nb + 1) * 4), boff_b = up256((size_t)(nb + 2) * 8), work_b = up256((size_t)work_words * 4);
    if ((rc = bm2_reserve(c->b_cg_in, in_b + off_b + plan_b + hl_b + hw_b + 256))) return rc;
    if ((rc = bm2_reserve(c->b_cg_work, mark_b + stat_b + bcnt_b + boff_b + work_b + 256))) return rc;
    if ((rc = bm2_reserve(c->b_cg_out, up256((size_t)room * 4) + 256))) return rc;
    char *d = (char *)c->b_cg_in.p, *w = (char *)c->b_cg_work.p;
    CgPrm P;
    memset(&P, 0, sizeof P);
    P.hits = d_hits ? d_hits : (const bm2h_cg_mark *)d; P.hit_off = d_off ? d_off : (const int64_t *)(d + in_b); P.plans = plans ? (const bm2_pairplan_t *)(d + in_b + off_b) : nullptr;
    P.heavy_list = (const int32_t *)(d + in_b + off_b + plan_b); P.heavy_work = (const int64_t *)(d + in_b + off_b + plan_b + hl_b);
    P.mark = (uint8_t *)w; P.stat = (int32_t *)(w + mark_b);
    int32_t *d_bcnt = (int32_t *)(w + mark_b + stat_b);
    int64_t *d_boff = (int64_t *)(w + mark_b + stat_b + bcnt_b);
    P.work = (uint32_t *)(w + mark_b + stat_b + bcnt_b + boff_b);
    P.xa_ratio = (double)so->XA_drop_ratio; P.drop_ratio = opt->drop_ratio;
    P.n_units = (int32_t)n_units; P.n_heavy = (int32_t)n_heavy; P.per_unit = per_unit; P.T = so->T; P.all = (so->flag & CG_F_ALL) != 0;
    P.max_xa = so->max_XA_hits; P.max_xa_alt = so->max_XA_hits_alt;
    int32_t *d_sel = (int32_t *)c->b_cg_out.p;
    if (!d_hits && n_hits && (rc = bm2_copy_h2d(c, (void *)P.hits, hits, (size_t)n_hits * sizeof(bm2h_cg_mark)))) return rc;
    if (!d_off && (rc = bm2_copy_h2d(c, (void *)P.hit_off, hoff.data(), (size_t)(n_lists + 1) * 8))) return rc;
    if (plans && n_units && (rc = bm2_copy_h2d(c, (void *)P.plans, plans, (size_t)n_units * sizeof(bm2_pairplan_t)))) return rc;
    if (n_heavy) {
        if ((rc = bm2_copy_h2d(c, (void *)P.heavy_list, heavy_list.data(), (size_t)n_heavy * 4))) return rc;
        if ((rc = bm2_copy_h2d(c, (void *)P.heavy_work, heavy_work.data(), (size_t)n_heavy * 8))) return rc;
    }
    prof.mark("H2D");
    // (marks and stat lie back to back: one memset; the marks' tail must read as zero, the workspace's counters start at zero)
    if ((rc = bm2_check(hipMemsetAsync(w, 0, mark_b + stat_b, c->stream), "memset marks"))) return rc;
    if (work_words && (rc = bm2_check(hipMemsetAsync(P.work, 0, (size_t)work_words * 4, c->stream), "memset counters"))) return rc;
    const int per_block = CG_LIGHT_THREADS / 16;
    hipLaunchKernelGGL(k_cg_light, dim3((unsigned)((n_units + per_block - 1) / per_block)), dim3(CG_LIGHT_THREADS), 0, c->stream, P);
    if ((rc = bm2_check(hipGetLastError(), "k_cg_light launch"))) return rc;
    if (n_heavy) {
        hipLaunchKernelGGL(k_cg_heavy, dim3((unsigned)n_heavy), dim3(64), 0, c->stream, P);
        if ((rc = bm2_check(hipGetLastError(), "k_cg_heavy launch"))) return rc;
    }
    if (nb) {
        hipLaunchKernelGGL(k_cg_count, dim3((unsigned)nb), dim3(256), 0, c->stream, (const uint8_t *)P.mark, n_hits, d_bcnt);
        if ((rc = bm2_check(hipGetLastError(), "k_cg_count launch"))) return rc;
    }
    if ((rc = bm2_scan_i32(c, d_bcnt, nb, d_boff, c->b_cg_scan))) return rc;
    if (nb) {
        hipLaunchKernelGGL(k_cg_write, dim3((unsigned)nb), dim3(256), 0, c->stream, (const uint8_t *)P.mark, n_hits, (const int64_t *)d_boff, hbase, d_sel, room);
        if ((rc = bm2_check(hipGetLastError(), "k_cg_write launch"))) return rc;
    }
    int32_t st = 0; int64_t total = -1;
    if ((rc = bm2_check(hipMemcpyAsync(&st, P.stat, 4, hipMemcpyDeviceToHost, c->stream), "D2H plan stat"))) return rc;
    if ((rc = bm2_check(hipMemcpyAsync(&total, d_boff + nb, 8, hipMemcpyDeviceToHost, c->stream), "D2H plan count"))) return rc;
    if ((rc = bm2_check(hipStreamSynchronize(c->stream), "k_cg"))) return rc;
    prof.mark("kernels");
    if (st) {
        bm2_set_error("%s: %s %lld has a secondary, secondary_all, z or n_pri that points outside its list", who, plans ? "pair" : "list", (long long)(first_unit + st - 1));
        return BM2_EINVAL;
    }
    if (total < 0 || total > n_hits) { bm2_set_error("%s: the device selected %lld of %lld hits", who, (long long)total, (long long)n_hits); return BM2_ENODEV; }
    const int64_t down = total < room ? total : room;
    if (down && (rc = bm2_copy_d2h(c, sel, d_sel, (size_t)down * 4))) return rc;
    prof.mark("D2H");
    *n_out = total; *heavy = n_heavy;
    if (total > cap) { bm2_set_error("%s: %lld hits are selected, room for %lld", who, (long long)total, (long long)cap); return BM2_ECAP; }
    return BM2_OK;
}
}  // namespace

// The selection of single-end lists whose 16 bytes a hit lie in HBM in decided order (semark.hip calls this between its kernels and its
// download): d_hits[k] = hit h_off[0] + k, d_off = the offsets from 0 on the device, h_off their host copy in the caller's numbering, which
// sel speaks.  See cgplan_run.
int bm2h_cgplan_resident(bm2_ctx *c, const char *who, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_lists, const bm2h_cg_mark *d_hits,
                         const int64_t *d_off, const int64_t *h_off, int32_t *sel, int64_t cap, int64_t *n_out, int64_t *heavy, int64_t first_list) {
    return cgplan_run(c, who, opt, so, n_lists, nullptr, h_off, nullptr, sel, cap, n_out, heavy, first_list, d_hits, d_off);
}

extern "C" int bm2_cigar_plan_dev(bm2_ctx *c, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_lists, const bm2_alnreg_t *hits,
                                  const int64_t *hit_off, const bm2_pairplan_t *plans, int32_t *sel, int64_t cap, int64_t *n_out) {
    if (!c || !opt || !so || n_lists < 0 || !hit_off || !n_out || cap < 0 || (cap > 0 && !sel)) { bm2_set_error("bm2_cigar_plan_dev: bad argument"); return BM2_EINVAL; }
    if (plans && (n_lists & 1)) { bm2_set_error("bm2_cigar_plan_dev: %d lists with plans (a pair has two)", n_lists); return BM2_EINVAL; }
    int rc = bm2h_check_list_off("bm2_cigar_plan_dev", n_lists, hit_off);
    if (rc) return rc;
    const int64_t hbase = hit_off[0], n_hits = hit_off[n_lists] - hbase;
    if (n_hits > 0 && !hits) { bm2_set_error("bm2_cigar_plan_dev: bad argument"); return BM2_EINVAL; }
    bm2h_cgplan_stats_set(0, 0, 0, 0);
    static thread_local std::vector<bm2h_cg_mark> packed_of_this_thread;
    std::vector<bm2h_cg_mark> &packed = packed_of_this_thread;
    if (packed.size() < (size_t)n_hits + 1) packed.resize((size_t)n_hits + 1);
    bm2_parallel_ranges(n_hits, 65536, bm2_host_threads(), [&](int64_t lo, int64_t hi) {
        for (int64_t k = lo; k < hi; ++k) {
            const bm2_alnreg_t &a = hits[hbase + k]; bm2h_cg_mark &m = packed[(size_t)k];
            m.score = a.score; m.secondary = a.secondary; m.secondary_all = a.secondary_all; m.is_alt = a.is_alt;
        }
    });
    int64_t heavy = 0;
    rc = cgplan_run(c, "bm2_cigar_plan_dev", opt, so, n_lists, packed.data(), hit_off, plans, sel, cap, n_out, &heavy);
    if (rc == BM2_OK || rc == BM2_ECAP) bm2h_cgplan_stats_set(n_lists, n_hits, *n_out, heavy);
    return rc;
}

// ---- the hook of the SAM tail (bm2h_cgplan_batch_fn; user = bm2h_text_ctxs): the lists cut into contiguous parts at pair boundaries,
// one context and one host thread per part.  A list's marks depend on the list and its pair's plan alone, and a part's selection is
// in hit_off's numbering already, so the parts' selections appended in part order are the whole batch's.
int bm2h_dev_cgplan_batch(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_lists, const bm2h_cg_mark *hits,
                          const int64_t *hit_off, const bm2_pairplan_t *plans, int32_t *sel, int64_t cap, int64_t *n_out) {
    const bm2h_text_ctxs *m = (const bm2h_text_ctxs *)user;
    const char *who = "BM2_SAM_F_DEVICE_CGPLAN";
    bm2h_cgplan_stats_set(0, 0, 0, 0);
    *n_out = 0;
    if (plans && (n_lists & 1)) { bm2_set_error("%s: %d lists with plans (a pair has two)", who, n_lists); return BM2_EINVAL; }
    int rc = bm2h_check_list_off(who, n_lists, hit_off);
    if (rc) return rc;
    for (int g = 0; g < m->n; ++g) if (!m->ctx[g]) { bm2_set_error("%s: no context", who); return BM2_EINVAL; }
    const int per_unit = plans ? 2 : 1;
    const int64_t n_units = n_lists / per_unit, n_hits = hit_off[n_lists] - hit_off[0];
    const int G = bm2_parts(n_units, bm2_knob("BM2_CGPLAN_PART", 65536), m->n);        // knob: units that are worth a context of their own (launch policy)
    int64_t heavy = 0;
    if (G == 1) {
        rc = cgplan_run(m->ctx[0], who, opt, so, n_lists, hits, hit_off, plans, sel, cap, n_out, &heavy);
        if (rc == BM2_OK || rc == BM2_ECAP) bm2h_cgplan_stats_set(n_lists, n_hits, *n_out, heavy);
        return rc;
    }
    std::vector<std::vector<int32_t>> part((size_t)G);
    std::vector<int64_t> got((size_t)G, 0), hv((size_t)G, 0);
    rc = bm2_run_parts(G, bm2_part_budget(G), nullptr, [&](int g) {
        const int64_t lo = bm2_part_lo(n_units, g, G) * per_unit, hi = bm2_part_lo(n_units, g + 1, G) * per_unit;
        const int64_t k = hit_off[hi] - hit_off[lo];
        part[(size_t)g].resize((size_t)k + 1);
        return cgplan_run(m->ctx[g], who, opt, so, (int32_t)(hi - lo), hits + (hit_off[lo] - hit_off[0]), hit_off + lo, plans ? plans + lo / 2 : nullptr,
                          part[(size_t)g].data(), k, &got[(size_t)g], &hv[(size_t)g], lo / per_unit);
    });
    if (rc) return rc;
    int64_t at = 0;
    for (int g = 0; g < G; ++g) {
        for (int64_t k = 0; k < got[(size_t)g]; ++k, ++at) if (at < cap) sel[at] = part[(size_t)g][(size_t)k];
        heavy += hv[(size_t)g];
    }
    *n_out = at;
    bm2h_cgplan_stats_set(n_lists, n_hits, at, heavy);
    if (at > cap) { bm2_set_error("%s: %lld hits are selected, room for %lld", who, (long long)at, (long long)cap); return BM2_ECAP; }
    return BM2_OK;
}

bm2h_cgplan_scope::bm2h_cgplan_scope(bm2_ctx *const *ctx, int n) : bm2h_ctx_scope(ctx, n), hook(bm2h_dev_cgplan_batch, &tc) {}
