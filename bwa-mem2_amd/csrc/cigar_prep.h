// cigar_prep.h -- the rule that prepares a CIGAR batch, stated once: what a task takes of the four scratch buffers, its shape and its
// cost class.  Plain C++ and HIP: the host form (cigar_prep.cpp: bm2_cigar_prep, the oracle; the flag-off path of cigar.hip), the device
// form (cgprep.hip) and the CIGAR kernels themselves (cigar.hip) all evaluate these functions, so the slices a kernel walks are the
// slices that were sized for it.
#pragma once
#include <stdint.h>
#include "../../include/bm2.h"
#if defined(__HIPCC__) || defined(__host__)
#define CGP_HD __host__ __device__
#else
#define CGP_HD
#endif

// the band of ksw_global2 as bwa_gen_cigar2 sets it (bwa.cpp:289-301); host and device size and run with the same number
static CGP_HD inline int cigar_band(int l_query, int rlen, int w_, int mat0, int o_del, int e_del, int o_ins, int e_ins) {
    int max_ins = (int)((double)(((l_query + 1) >> 1) * mat0 - o_ins) / e_ins + 1.);
    int max_del = (int)((double)(((l_query + 1) >> 1) * mat0 - o_del) / e_del + 1.);
    int max_gap = max_ins > max_del ? max_ins : max_del;
    max_gap = max_gap > 1 ? max_gap : 1;
    const int dl = rlen > l_query ? rlen - l_query : l_query - rlen;
    int w = (max_gap + dl + 1) >> 1;
    w = w < w_ ? w : w_;
    const int min_w = dl + 3;
    return w > min_w ? w : min_w;
}
static CGP_HD inline bool cigar_range_ok(int64_t l_pac, int l_query, int64_t rb, int64_t re) {
    if (l_query <= 0 || rb >= re || (rb < l_pac && re > l_pac)) return false;
    return rb >= 0 && re <= (l_pac << 1);                       // bns_get_seq would clamp: a clamped range is the NULL return
}
// infer_bw, bwamem.cpp:1811-1818, and the band of mem_reg2aln's first try (:1743-1747)
static CGP_HD inline int cigar_infer_bw(int l1, int l2, int score, int a, int q, int r) {
    if (l1 == l2 && l1 * a - score < (q + r - a) << 1) return 0;
    int w = (int)((double)((l1 < l2 ? l1 : l2) * a - score - q) / r + 2.);
    const int d = l1 > l2 ? l1 - l2 : l2 - l1;
    return w < d ? d : w;
}
static CGP_HD inline int cigar_first_band(int lq, int rlen, int truesc, int w_hit, int a, int w_opt, int o_del, int e_del, int o_ins, int e_ins) {
    const int t = cigar_infer_bw(lq, rlen, truesc, a, o_del, e_del);
    int w2 = cigar_infer_bw(lq, rlen, truesc, a, o_ins, e_ins);
    w2 = w2 > t ? w2 : t;
    if (w2 > w_opt) w2 = w2 < w_hit ? w2 : w_hit;
    return w2;
}

// the LDS shapes keep scores in 16 bits: a task is `small` when no score of it can leave (-CG_SMALL, CG_SMALL); the RING shape keeps
// CG_RING columns of the row (see cigar.hip)
#define CG_SMALL 10000
#define CG_RING 64
// the four shapes in the order of the batch's four task lists (and of bm2_cigar_prep_t::n_shape)
enum { CG_SH_RING = 0, CG_SH_ROW = 1, CG_SH_GLOBAL = 2, CG_SH_FLAT = 3 };
#define CG_RANGE_MAX 0x3fffffff       // a longer reference range is refused

// what the rule reads besides the task: scoring, the band option, and the three launch knobs (read on the host, passed down)
struct CgpPrm {
    int64_t l_pac;
    int32_t mat0, o_del, e_del, o_ins, e_ins, a, w, pen;          // pen = the largest magnitude a cell can add to a score
    int32_t no_lds, no_ring, ring_by_band, force_retry;           // force_retry: every task is a retried one whatever its record says
};
struct CgpSizes { int64_t z, e, c, m; int32_t wb_first; };      // wb_first: the band of the first (or only) alignment, -1 = none (flat / NULL)

static inline CgpPrm cgp_prm(const bm2_opt *opt, int64_t l_pac, int no_lds, int no_ring, int ring_by_band, int force_retry) {
    CgpPrm P;
    P.l_pac = l_pac; P.mat0 = opt->mat[0]; P.o_del = opt->o_del; P.e_del = opt->e_del; P.o_ins = opt->o_ins; P.e_ins = opt->e_ins; P.a = opt->a; P.w = opt->w;
    int pen = 1;
    for (int k = 0; k < 25; ++k) { const int v = opt->mat[k] < 0 ? -(int)opt->mat[k] : (int)opt->mat[k]; pen = pen > v ? pen : v; }
    const int od = opt->o_del + opt->e_del, oi = opt->o_ins + opt->e_ins;
    pen = pen > od ? pen : od; pen = pen > oi ? pen : oi;
    P.pen = pen; P.no_lds = no_lds; P.no_ring = no_ring; P.ring_by_band = ring_by_band; P.force_retry = force_retry;
    return P;
}
// the kernels compute scores from (match, mismatch, ambiguous), as the hot path does: the bwa_fill_scmat form
static inline bool cgp_scmat_ok(const bm2_opt *opt) {
    for (int i = 0; i < 5; i++) for (int j = 0; j < 5; j++) {
        const int want = (i == 4 || j == 4) ? opt->mat[4] : (i == j ? opt->mat[0] : opt->mat[1]);
        if (opt->mat[i * 5 + j] != want) return false;
    }
    return true;
}

// What the task takes of the four buffers; s.z = its DP area = its cost.  false: its reference range is longer than CG_RANGE_MAX.
static CGP_HD inline bool cgp_sizes(const CgpPrm &P, int q_len, int64_t rb, int64_t re, int w_hit, int truesc, int retry, CgpSizes &s) {
    s.z = 0; s.e = 0; s.c = 0; s.m = 0; s.wb_first = -1;
    if (!cigar_range_ok(P.l_pac, q_len, rb, re)) return true;
    const int64_t rlen = re - rb;
    if (rlen > CG_RANGE_MAX) return false;
    const int w_first = retry ? cigar_first_band(q_len, (int)rlen, truesc, w_hit, P.a, P.w, P.o_del, P.e_del, P.o_ins, P.e_ins) : w_hit;
    if (!(q_len == rlen && w_first == 0)) {                     // (a retried task never starts from band 0: the first score ends its loop)
        const int w_cap = retry ? (w_first < P.w << 2 ? P.w << 2 : w_first) : w_hit;
        const int wb = cigar_band(q_len, (int)rlen, w_cap, P.mat0, P.o_del, P.e_del, P.o_ins, P.e_ins);
        const int n_col = ((q_len < 2 * wb + 1 ? q_len : 2 * wb + 1) + 3) & ~3;      // a multiple of 4: every z slice starts 4-aligned
        s.z = (int64_t)n_col * rlen; s.e = (int64_t)q_len + 1;
        const int w0 = retry ? (w_first < P.w << 2 ? w_first : P.w << 2) : w_hit;      // (the kernel's clamp of the first try)
        s.wb_first = cigar_band(q_len, (int)rlen, w0, P.mat0, P.o_del, P.e_del, P.o_ins, P.e_ins);
    }
    s.c = (int64_t)q_len + rlen + 2; s.m = 2 * ((int64_t)q_len + rlen) + 16;
    return true;
}
static CGP_HD inline bool cgp_small(const CgpPrm &P, int q_len, int64_t rlen) { return !P.no_lds && q_len <= 220 && ((int64_t)q_len + rlen) * P.pen < CG_SMALL; }
// z, wb_first: of cgp_sizes
static CGP_HD inline int cgp_shape(const CgpPrm &P, int q_len, int64_t rb, int64_t re, int64_t z, int wb_first) {
    if (z == 0) return CG_SH_FLAT;                               // (no DP area: the one-M case, or a NULL return)
    if (!cgp_small(P, q_len, re - rb)) return CG_SH_GLOBAL;      // (z != 0: the range is a valid one)
    return (!P.no_ring && 2 * (int64_t)wb_first + 2 <= CG_RING) ? CG_SH_RING : CG_SH_ROW;
}
// The class key, one byte: (shape, cost on a log scale, expensive first).  The RING tasks by the band of their FIRST try, exactly: a
// wavefront steps through the widest band among its 64 tasks, and z -- the DP area the task's slices are sized for, i.e. of the widest
// band its retry loop can come to -- is the same for nearly all of them.
static CGP_HD inline int cgp_cls(const CgpPrm &P, int sh, int64_t z, int wb_first) {
    if (sh == CG_SH_RING && P.ring_by_band) { const int b = wb_first < 0 ? 0 : (wb_first > 31 ? 31 : wb_first); return sh * 64 + 31 - b; }
    const int k = z > 0 ? 64 - __builtin_clzll((unsigned long long)z) : 0;      // bits of z
    return sh * 64 + 63 - k;
}
