// semark.hip -- the `decide` phase of the single-end tail on the device, for a batch of hit lists: mem_mark_primary_se (bwamem.cpp:1392-1465)
// and, under MEM_F_PRIMARY5, mem_reorder_primary5 (:1496-1519) of every list.  Host oracle: bm2_se_mark of sam_tail.cpp (mark_primary_se /
// reorder_primary5 behind a C name), compared field by field.
//
//   k_sm_class     one lane per list: light (<= 16 hits) or heavy, and the heavy list's share of the global workspace
//   bm2_scan_i32   two scans: the heavy lists' numbers in the heavy list, their workspace offsets
//   k_sm_list      the heavy list
//   k_sm_light     a 16-lane row per list of up to SM_LIGHT_MAX hits, the list in LDS
//   k_sm_heavy     a wavefront per longer list: in LDS up to SM_HEAVY_LDS hits, in the global workspace beyond.  EVERY list is marked by
//                  one of the two; nothing goes back to the host.
// Both kernels run the SAME code (sm_list<W>), which is mark_dev.h's -- the group primitives and the marking code decide.hip runs on a
// pair's two lists -- instantiated over a record that holds what the single-end rule reads: qb, qe, score, sub_n, is_alt go up (20 B a
// hit), the permutation and the six rewritten fields come down (32 B a hit, decide.hip's DcOut layout), and the host moves its 96-byte
// hits accordingly.  With the CIGAR plan asked for as well, the kernels also leave the 16 bytes a hit cgplan.hip reads (bm2h_cg_mark)
// in decided order in HBM, and cgplan.hip's kernels run on them there (bm2h_cgplan_resident): no second upload, no host pack pass.
//
// No transcendental function runs here; the one floating-point test is dc_covered's float multiply and compare.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include <vector>
#include "../../include/bm2.h"
#include "bm2_ctx.h"
#include "host_tail.h"
#include "host_pool.h"
#include "pipeline.h"

#pragma clang fp contract(off)      /* as in sam_tail.cpp's object code (no FMA there); holds to the end of the file */

#define SM_LIGHT_MAX 16             // hits of a list the row form takes
#define SM_HEAVY_LDS 128            // hits of a list the wavefront form keeps in LDS (2 x 128 x 56 B = 14 KiB a wavefront)
#define SM_LIGHT_THREADS 128        // 8 rows a block
#define SM_REDUCE_UNROLL 8          // words of a group reduction in flight (mark_dev.h: Grp)

enum { SM_F_PRIMARY5 = 0x800 };

struct SmIn { int32_t qb, qe, score, sub_n, is_alt; };                                                                     // 20 B up per hit
struct SmOut { uint64_t hash; int32_t orig, sub, alt_sc, sub_n, secondary, secondary_all; };                              // 32 B down per hit
struct SmHit {                      // a hit while its list is being marked (56 B)
    uint64_t hash;
    int32_t qb, qe, score, sub_n, is_alt, sub, alt_sc, secondary, secondary_all, orig, tmp, pad;
};
struct SmPrm {
    const SmIn *in; SmOut *out; const int64_t *hit_off; int32_t *n_pri; bm2h_cg_mark *cg;      // offsets from 0; cg == NULL: no CIGAR plan follows
    int64_t first_id;
    int32_t n_lists, a, b, o_del, e_del, o_ins, e_ins;
    float mask_level;
    int32_t T, flag;
    const int32_t *heavy_list; const int64_t *work_off; SmHit *work; int32_t n_heavy, pad;
};
static_assert(sizeof(SmIn) == 20 && sizeof(SmOut) == 32 && sizeof(SmHit) == 56, "the compact records of semark.hip");

static __device__ __forceinline__ void dc_load(SmHit &h, const SmIn &s) {
    h.qb = s.qb; h.qe = s.qe; h.score = s.score; h.sub_n = s.sub_n; h.is_alt = s.is_alt; h.pad = 0;
}
#include "mark_dev.h"

// list li: A, B = room for its hits twice
template <int W, int U> static __device__ void sm_list(const Grp<W, U> &G, const SmPrm &P, int64_t li, SmHit *A, SmHit *B) {
    const int64_t o0 = P.hit_off[li];
    const int n = (int)(P.hit_off[li + 1] - o0);
    const int n_pri = dc_mark_primary<W>(G, P, n, P.in + o0, A, B, P.first_id + li);
    if (P.flag & SM_F_PRIMARY5) dc_reorder_primary5<W>(G, P.T, n, A);
    if (G.lane == 0) P.n_pri[li] = n_pri;
    grp_sync<W>();
    for (int i = G.lane; i < n; i += W) {                        // what the host needs to reorder and annotate its hits; what the CIGAR plan reads
        const SmHit &h = A[i];
        SmOut r; r.hash = h.hash; r.orig = h.orig; r.sub = h.sub; r.alt_sc = h.alt_sc; r.sub_n = h.sub_n; r.secondary = h.secondary; r.secondary_all = h.secondary_all;
        P.out[o0 + i] = r;
        if (P.cg) { bm2h_cg_mark m; m.score = h.score; m.secondary = h.secondary; m.secondary_all = h.secondary_all; m.is_alt = h.is_alt; P.cg[o0 + i] = m; }
    }
}

__global__ void k_sm_class(const int64_t *__restrict__ hit_off, int n_lists, int32_t *__restrict__ heavy, int32_t *__restrict__ wsize) {
    const int li = blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= n_lists) return;
    const int64_t n = hit_off[li + 1] - hit_off[li];
    heavy[li] = n > SM_LIGHT_MAX;
    wsize[li] = n > SM_HEAVY_LDS ? (int32_t)n : 0;
}
__global__ void k_sm_list(const int32_t *__restrict__ heavy, const int64_t *__restrict__ heavy_at, int n_lists, int32_t *__restrict__ list) {
    const int li = blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= n_lists) return;
    if (heavy[li]) list[heavy_at[li]] = li;
}
__global__ __launch_bounds__(SM_LIGHT_THREADS) void k_sm_light(SmPrm P) {
    __shared__ SmHit lds[SM_LIGHT_THREADS / 16][2 * SM_LIGHT_MAX];
    __shared__ uint64_t red[SM_LIGHT_THREADS / 16][16];
    const int row = threadIdx.x >> 4;
    const int64_t li = (int64_t)blockIdx.x * (SM_LIGHT_THREADS / 16) + row;
    if (li >= P.n_lists) return;                                 // (row-uniform, like everything below)
    if (P.hit_off[li + 1] - P.hit_off[li] > SM_LIGHT_MAX) return;
    Grp<16, SM_REDUCE_UNROLL> G; G.red = red[row]; G.lane = threadIdx.x & 15;
    sm_list<16>(G, P, li, lds[row], lds[row] + SM_LIGHT_MAX);
}
__global__ __launch_bounds__(64) void k_sm_heavy(SmPrm P) {
    __shared__ SmHit lds[2 * SM_HEAVY_LDS];
    __shared__ uint64_t red[64];
    if ((int)blockIdx.x >= P.n_heavy) return;
    const int li = P.heavy_list[blockIdx.x];
    const int64_t n = P.hit_off[(int64_t)li + 1] - P.hit_off[li];
    Grp<64, SM_REDUCE_UNROLL> G; G.red = red; G.lane = threadIdx.x;
    SmHit *A = lds, *B = lds + SM_HEAVY_LDS;
    if (n > SM_HEAVY_LDS) { A = P.work + 2 * P.work_off[li]; B = A + n; }
    sm_list<64>(G, P, li, A, B);
}

namespace {
std::atomic<long long> g_sm_lists{0}, g_sm_hits{0}, g_sm_heavy{0};

// The lists [hit_off[0], hit_off[n_lists]) of `hits` marked on one context, in place.  n_sel != NULL: the CIGAR plan of the marked lists as
// well, from the marks where the kernels left them (sel, cap, *n_sel and *cg_heavy as for bm2h_cgplan_resident; first_list names a list in
// its message).
int semark_run(bm2_ctx *c, const char *who, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_lists, bm2_alnreg_t *hits, const int64_t *hit_off,
               int64_t first_id, int32_t *n_pri, int32_t *sel = nullptr, int64_t cap = 0, int64_t *n_sel = nullptr, int64_t *cg_heavy = nullptr, int64_t first_list = 0) {
    if (n_sel) { *n_sel = 0; *cg_heavy = 0; }
    if (n_lists == 0) return BM2_OK;
    int rc = bm2_check(hipSetDevice(c->device), "hipSetDevice");
    if (rc) return rc;
    TailProf prof("se_mark_dev");
    const int64_t base = hit_off[0], n_hits = hit_off[n_lists] - base;
    bm2_alnreg_t *const H = hits + base;
    const int nt = bm2_host_threads();
    // the offsets from 0; what the kernels will bin (known here from the offsets alone: the buffers are sized without a round trip)
    const std::vector<int64_t> off = bm2h_hit_off_from0(hit_off, n_lists);
    int64_t n_heavy = 0, work_hits = 0;
    for (int64_t li = 0; li < n_lists; ++li) {
        const int64_t n = off[(size_t)li + 1] - off[(size_t)li];
        n_heavy += n > SM_LIGHT_MAX; if (n > SM_HEAVY_LDS) work_hits += n;
    }
    // pack: the 20 bytes of a hit the rule reads
    static thread_local std::vector<SmIn> in_of_this_thread;
    static thread_local std::vector<SmOut> out_of_this_thread;
    std::vector<SmIn> &in = in_of_this_thread;
    std::vector<SmOut> &out = out_of_this_thread;
    if (in.size() < (size_t)n_hits + 1) in.resize((size_t)n_hits + 1);
    if (out.size() < (size_t)n_hits + 1) out.resize((size_t)n_hits + 1);
    bm2_parallel_ranges(n_hits, 65536, nt, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const bm2_alnreg_t &h = H[i];
            SmIn &d = in[(size_t)i];
            d.qb = h.qb; d.qe = h.qe; d.score = h.score; d.sub_n = h.sub_n; d.is_alt = h.is_alt;
        }
    });
    prof.mark("pack");
    // device buffers
    const size_t in_b = up256((size_t)n_hits * sizeof(SmIn)), off_b = up256((size_t)(n_lists + 1) * 8);
    const size_t out_b = up256((size_t)n_hits * sizeof(SmOut)), npri_b = up256((size_t)n_lists * 4), cg_b = n_sel ? up256((size_t)n_hits * sizeof(bm2h_cg_mark)) : 0;
    const size_t flag_b = up256((size_t)n_lists * 4), at_b = up256((size_t)(n_lists + 1) * 8), list_b = up256((size_t)(n_heavy + 1) * 4),
                 work_b = up256((size_t)work_hits * 2 * sizeof(SmHit));
    if ((rc = bm2_reserve(c->b_sm_in, in_b + off_b + 256))) return rc;
    if ((rc = bm2_reserve(c->b_sm_out, out_b + npri_b + cg_b + 256))) return rc;
    if ((rc = bm2_reserve(c->b_sm_work, 2 * flag_b + 2 * at_b + list_b + work_b + 256))) return rc;
    char *d = (char *)c->b_sm_in.p, *o = (char *)c->b_sm_out.p, *w = (char *)c->b_sm_work.p;
    SmPrm P;
    memset(&P, 0, sizeof P);
    P.in = (const SmIn *)d; P.hit_off = (const int64_t *)(d + in_b);
    P.out = (SmOut *)o; P.n_pri = (int32_t *)(o + out_b); P.cg = n_sel ? (bm2h_cg_mark *)(o + out_b + npri_b) : nullptr;
    int32_t *d_heavy = (int32_t *)w, *d_wsize = (int32_t *)(w + flag_b);
    int64_t *d_heavy_at = (int64_t *)(w + 2 * flag_b), *d_work_off = (int64_t *)(w + 2 * flag_b + at_b);
    int32_t *d_list = (int32_t *)(w + 2 * flag_b + 2 * at_b);
    P.heavy_list = d_list; P.work_off = d_work_off; P.work = (SmHit *)(w + 2 * flag_b + 2 * at_b + list_b); P.n_heavy = (int32_t)n_heavy;
    P.first_id = first_id; P.n_lists = n_lists;
    P.a = opt->a; P.b = opt->b; P.o_del = opt->o_del; P.e_del = opt->e_del; P.o_ins = opt->o_ins; P.e_ins = opt->e_ins;
    P.mask_level = opt->mask_level; P.T = so->T; P.flag = so->flag;
    if (n_hits && (rc = bm2_copy_h2d(c, (void *)P.in, in.data(), (size_t)n_hits * sizeof(SmIn)))) return rc;
    if ((rc = bm2_copy_h2d(c, (void *)P.hit_off, off.data(), (size_t)(n_lists + 1) * 8))) return rc;
    prof.mark("H2D");
    const unsigned g256 = (unsigned)((n_lists + 255) / 256);
    hipLaunchKernelGGL(k_sm_class, dim3(g256), dim3(256), 0, c->stream, P.hit_off, n_lists, d_heavy, d_wsize);
    if ((rc = bm2_check(hipGetLastError(), "k_sm_class launch"))) return rc;
    if ((rc = bm2_scan_i32(c, d_heavy, n_lists, d_heavy_at, c->b_sm_scan))) return rc;
    if ((rc = bm2_scan_i32(c, d_wsize, n_lists, d_work_off, c->b_sm_scan2))) return rc;
    hipLaunchKernelGGL(k_sm_list, dim3(g256), dim3(256), 0, c->stream, (const int32_t *)d_heavy, (const int64_t *)d_heavy_at, n_lists, d_list);
    if ((rc = bm2_check(hipGetLastError(), "k_sm_list launch"))) return rc;
    const int per_block = SM_LIGHT_THREADS / 16;
    hipLaunchKernelGGL(k_sm_light, dim3((unsigned)((n_lists + per_block - 1) / per_block)), dim3(SM_LIGHT_THREADS), 0, c->stream, P);
    if ((rc = bm2_check(hipGetLastError(), "k_sm_light launch"))) return rc;
    if (n_heavy) {
        hipLaunchKernelGGL(k_sm_heavy, dim3((unsigned)n_heavy), dim3(64), 0, c->stream, P);
        if ((rc = bm2_check(hipGetLastError(), "k_sm_heavy launch"))) return rc;
    }
    int64_t heavy_seen = -1;
    if ((rc = bm2_check(hipMemcpyAsync(&heavy_seen, d_heavy_at + n_lists, 8, hipMemcpyDeviceToHost, c->stream), "D2H heavy count"))) return rc;
    if ((rc = bm2_check(hipStreamSynchronize(c->stream), "k_sm"))) return rc;
    prof.mark("kernels");
    if (heavy_seen != n_heavy) { bm2_set_error("%s: the device binned %lld heavy lists, the host counted %lld", who, (long long)heavy_seen, (long long)n_heavy); return BM2_ENODEV; }
    if (n_sel) {                                                 // the CIGAR plan on the marks where they lie (its own phases: cigar_plan_dev)
        if ((rc = bm2h_cgplan_resident(c, who, opt, so, n_lists, P.cg, P.hit_off, hit_off, sel, cap, n_sel, cg_heavy, first_list))) return rc;
        prof.mark("cigar plan");
    }
    if (n_hits && (rc = bm2_copy_d2h(c, out.data(), P.out, (size_t)n_hits * sizeof(SmOut)))) return rc;
    if (n_pri && (rc = bm2_copy_d2h(c, n_pri, P.n_pri, (size_t)n_lists * 4))) return rc;
    prof.mark("D2H");
    // in place: every list in the device's order, the six rewritten fields from the device, everything else with its hit
    std::atomic<int64_t> bad(-1);
    bm2_parallel_ranges(n_lists, 4096, nt, [&](int64_t lo, int64_t hi) {
        std::vector<bm2_alnreg_t> old;
        for (int64_t li = lo; li < hi; ++li) {
            const int64_t b0 = off[(size_t)li], k = off[(size_t)li + 1] - b0;
            if (!k) continue;
            old.assign(H + b0, H + b0 + k);
            for (int64_t i = 0; i < k; ++i) {
                const SmOut &r = out[(size_t)(b0 + i)];
                if (r.orig < 0 || r.orig >= k) { int64_t e = -1; bad.compare_exchange_strong(e, li); continue; }
                bm2_alnreg_t &h = H[b0 + i];
                h = old[(size_t)r.orig];
                h.hash = r.hash; h.sub = r.sub; h.alt_sc = r.alt_sc; h.sub_n = r.sub_n; h.secondary = r.secondary; h.secondary_all = r.secondary_all;
            }
        }
    });
    prof.mark("apply");
    if (bad.load() >= 0) { bm2_set_error("%s: list %lld came back with a broken permutation", who, (long long)(first_list + bad.load())); return BM2_ENODEV; }
    g_sm_lists += n_lists; g_sm_hits += (long long)n_hits; g_sm_heavy += (long long)n_heavy;
    return BM2_OK;
}
}  // namespace

extern "C" void bm2_sam_se_mark_stats(int64_t *lists, int64_t *hits, int64_t *lists_heavy) {
    if (lists) *lists = g_sm_lists.load();
    if (hits) *hits = g_sm_hits.load();
    if (lists_heavy) *lists_heavy = g_sm_heavy.load();
}

extern "C" int bm2_se_mark_dev(bm2_ctx *c, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_lists, bm2_alnreg_t *hits,
                               const int64_t *hit_off, int64_t first_id, int32_t *n_pri) {
    if (!c || !opt || !so || n_lists < 0 || !hit_off) { bm2_set_error("bm2_se_mark_dev: bad argument"); return BM2_EINVAL; }
    int rc = bm2h_check_list_off("bm2_se_mark_dev", n_lists, hit_off);
    if (rc) return rc;
    if (hit_off[n_lists] > hit_off[0] && !hits) { bm2_set_error("bm2_se_mark_dev: bad argument"); return BM2_EINVAL; }
    g_sm_lists = 0; g_sm_hits = 0; g_sm_heavy = 0;
    return semark_run(c, "bm2_se_mark_dev", opt, so, n_lists, hits, hit_off, first_id, n_pri);
}

// ---- the hook of the SAM tail (bm2h_semark_batch_fn; user = bm2h_text_ctxs): the chunk's lists cut into contiguous parts, one context
// and one host thread per part.  A list's marks depend on the list and its number alone, so the parts do not depend on one another and
// the result does not depend on their number; a part's selection is in hit_off's numbering already, so the parts' selections appended
// in part order are the whole batch's.
int bm2h_dev_semark_batch(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_lists, bm2_alnreg_t *hits, const int64_t *hit_off,
                          int64_t first_id, int32_t *n_pri, int32_t *sel, int64_t cap, int64_t *n_out) {
    const bm2h_text_ctxs *m = (const bm2h_text_ctxs *)user;
    const char *who = "BM2_SAM_F_DEVICE_SEMARK";
    g_sm_lists = 0; g_sm_hits = 0; g_sm_heavy = 0;
    if (n_out) { *n_out = 0; bm2h_cgplan_stats_set(0, 0, 0, 0); }
    if (n_out && (cap < 0 || (cap > 0 && !sel))) { bm2_set_error("%s: bad argument", who); return BM2_EINVAL; }
    int rc = bm2h_check_list_off(who, n_lists, hit_off);
    if (rc) return rc;
    for (int g = 0; g < m->n; ++g) if (!m->ctx[g]) { bm2_set_error("%s: no context", who); return BM2_EINVAL; }
    const int64_t n_hits = hit_off[n_lists] - hit_off[0];
    const int G = bm2_parts(n_lists, bm2_knob("BM2_SEMARK_PART", 65536), m->n);        // knob: lists that are worth a context of their own (launch policy)
    int64_t heavy = 0;
    if (G == 1) {
        rc = semark_run(m->ctx[0], who, opt, so, n_lists, hits, hit_off, first_id, n_pri, sel, cap, n_out, n_out ? &heavy : nullptr);
        if (n_out && (rc == BM2_OK || rc == BM2_ECAP)) bm2h_cgplan_stats_set(n_lists, n_hits, *n_out, heavy);
        return rc;
    }
    std::vector<std::vector<int32_t>> part((size_t)G);
    std::vector<int64_t> got((size_t)G, 0), hv((size_t)G, 0);
    rc = bm2_run_parts(G, bm2_part_budget(G), nullptr, [&](int g) {
        const int64_t lo = bm2_part_lo(n_lists, g, G), hi = bm2_part_lo(n_lists, g + 1, G);
        const int64_t k = hit_off[hi] - hit_off[lo];
        if (n_out) part[(size_t)g].resize((size_t)k + 1);
        return semark_run(m->ctx[g], who, opt, so, (int32_t)(hi - lo), hits, hit_off + lo, first_id + lo, n_pri ? n_pri + lo : nullptr,
                          n_out ? part[(size_t)g].data() : nullptr, k, n_out ? &got[(size_t)g] : nullptr, n_out ? &hv[(size_t)g] : nullptr, lo);
    });
    if (rc || !n_out) return rc;
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

bm2h_semark_scope::bm2h_semark_scope(bm2_ctx *const *ctx, int n) : bm2h_ctx_scope(ctx, n), hook(bm2h_dev_semark_batch, &tc) {}
