// cgprep.hip -- the CIGAR batch prepared on the device: the 40-byte hits become the 72-byte tasks of cigar.hip's kernels with their slices
// of the four scratch buffers, and the batch is ordered by class key, where the batch is about to run.  The rule is cigar_prep.h's (the
// functions the CIGAR kernels evaluate themselves); host oracle: bm2_cigar_prep (cigar_prep.cpp), compared field for field.
//
//   k_cgp_size      a lane per task: the task is validated (an offender is named, never followed), its four sizes, its query offset and
//                   its class key are written; shape counts and qmax are reduced per block in LDS, one atomic per block and value
//   bm2_scan_i32    x 4: the slices' offsets
//   k_cgp_task      a lane per task: the 72 bytes of the task from registers, nine 8-byte stores; lane 0 of block 0 files the totals
//   k_cgp_hist      per-block counts per key, key-major [256][n_blocks]; bm2_scan_i32 over them is every (key, block)'s first place
//   k_cgp_scatter   place = scanned[key][block] + the earlier tasks of the block with the same key, counted over the block's keys in
//                   LDS (four to a word): the order is the stable one, whatever order the lanes run in
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <string.h>
#include "../../include/bm2.h"
#include "bm2_ctx.h"
#include "host_tail.h"
#include "host_pool.h"
#include "pipeline.h"

#pragma clang fp contract(off)

#define CGP_THREADS 256             // tasks per block of every kernel here
#define CGP_KEYS 256

struct CgpDown { bm2_cigar_prep_t tot; int32_t err[4]; };         // err[k] = n - (the lowest task with error k), 0 = none: bad read / stretch, range too long, a size at 2^31
struct CgpArgs {
    const bm2_cigar_hit_t *hits; const int64_t *roff; const int32_t *rlen;
    int32_t *sz; int64_t *pos; int64_t *q_off; uint8_t *key;      // sz: [4][sz_stride], pos: [4][pos_stride] (z, eh, cg, md)
    int32_t *hist; const int64_t *hpos;                           // [CGP_KEYS][nb] and its exclusive scan
    CgpDown *down; bm2_cigar_task_t *tasks; int32_t *order;
    int64_t sz_stride, pos_stride;
    int32_t n, n_reads, nb, pad;
    CgpPrm P;
};

__global__ __launch_bounds__(CGP_THREADS) void k_cgp_size(CgpArgs A) {
    __shared__ int32_t red[8];                                  // [0..3] tasks of each shape, [4] the longest query among RING and ROW
    if (threadIdx.x < 8) red[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * CGP_THREADS + threadIdx.x;
    if (i < A.n) {
        const bm2_cigar_hit_t h = A.hits[i];
        CgpSizes s; s.z = 0; s.e = 0; s.c = 0; s.m = 0; s.wb_first = -1;
        int64_t qo = 0;
        const int q_len = (int)((uint32_t)h.qe - (uint32_t)h.qb);      // (of a stretch that exists: qe - qb)
        bool ok = h.read >= 0 && h.read < A.n_reads && h.qb >= 0 && h.qb <= h.qe;
        if (ok) ok = h.qe <= A.rlen[h.read];
        if (!ok) atomicMax(&A.down->err[0], A.n - i);
        else {
            qo = A.roff[h.read] + h.qb;
            if (!cgp_sizes(A.P, q_len, h.rb, h.re, h.w, h.truesc, A.P.force_retry ? 1 : h.retry, s)) atomicMax(&A.down->err[1], A.n - i);
            else if (s.z > INT_MAX || s.e > INT_MAX || s.c > INT_MAX || s.m > INT_MAX) {
                atomicMax(&A.down->err[2], A.n - i);
                s.z = 0; s.e = 0; s.c = 0; s.m = 0; s.wb_first = -1;
            }
        }
        const int sh = cgp_shape(A.P, q_len, h.rb, h.re, s.z, s.wb_first);
        A.sz[i] = (int32_t)s.z; A.sz[A.sz_stride + i] = (int32_t)s.e; A.sz[2 * A.sz_stride + i] = (int32_t)s.c; A.sz[3 * A.sz_stride + i] = (int32_t)s.m;
        A.q_off[i] = qo;
        A.key[i] = (uint8_t)cgp_cls(A.P, sh, s.z, s.wb_first);
        atomicAdd(&red[sh], 1);
        if (sh == CG_SH_RING || sh == CG_SH_ROW) atomicMax(&red[4], q_len);
    }
    __syncthreads();
    if (threadIdx.x < 4 && red[threadIdx.x]) atomicAdd(&A.down->tot.n_shape[threadIdx.x], red[threadIdx.x]);
    if (threadIdx.x == 4 && red[4]) atomicMax(&A.down->tot.qmax, red[4]);
}

__global__ __launch_bounds__(CGP_THREADS) void k_cgp_task(CgpArgs A) {
    const int i = blockIdx.x * CGP_THREADS + threadIdx.x;
    if (i == 0) {
        A.down->tot.z_bytes = A.pos[A.n]; A.down->tot.eh_items = A.pos[A.pos_stride + A.n];
        A.down->tot.cg_items = A.pos[2 * A.pos_stride + A.n]; A.down->tot.md_bytes = A.pos[3 * A.pos_stride + A.n];
    }
    if (i >= A.n) return;
    const bm2_cigar_hit_t h = A.hits[i];
    const int32_t retry = A.P.force_retry ? 1 : h.retry;
    int64_t *o = (int64_t *)(A.tasks + i);                       // 72 bytes, 8-aligned: nine whole stores
    o[0] = A.q_off[i]; o[1] = h.rb; o[2] = h.re;
    o[3] = A.pos[i]; o[4] = A.pos[A.pos_stride + i]; o[5] = A.pos[2 * A.pos_stride + i]; o[6] = A.pos[3 * A.pos_stride + i];
    o[7] = (int64_t)((uint64_t)((uint32_t)h.qe - (uint32_t)h.qb) | (uint64_t)(uint32_t)h.w << 32);
    o[8] = (int64_t)((uint64_t)(uint32_t)h.truesc | (uint64_t)(uint32_t)retry << 32);
}

__global__ __launch_bounds__(CGP_THREADS) void k_cgp_hist(CgpArgs A) {
    __shared__ int32_t cnt[CGP_KEYS];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * CGP_THREADS + threadIdx.x;
    if (i < A.n) atomicAdd(&cnt[A.key[i]], 1);
    __syncthreads();
    A.hist[(int64_t)threadIdx.x * A.nb + blockIdx.x] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(CGP_THREADS) void k_cgp_scatter(CgpArgs A) {
    __shared__ uint32_t kw[CGP_THREADS / 4];                    // the block's keys, four to a word (lanes past the batch: never counted, they follow every task)
    const int t = threadIdx.x, i = blockIdx.x * CGP_THREADS + t;
    const uint32_t key = i < A.n ? A.key[i] : 0u;
    ((uint8_t *)kw)[t] = (uint8_t)key;
    __syncthreads();
    if (i >= A.n) return;
    const uint32_t rep = key * 0x01010101u;
    int before = 0;
    for (int w = 0; w <= (t >> 2); ++w) {
        uint32_t x = kw[w] ^ rep;                                // a zero byte = a task with this key
        if (w == (t >> 2)) x |= ~((1u << (8 * (t & 3))) - 1u);   // (only the lanes before this one)
        before += ((x & 0xffu) == 0) + ((x & 0xff00u) == 0) + ((x & 0xff0000u) == 0) + ((x & 0xff000000u) == 0);
    }
    A.order[A.hpos[(int64_t)key * A.nb + blockIdx.x] + before] = i;
}

static_assert(sizeof(bm2h_cg_hit) == sizeof(bm2_cigar_hit_t), "bm2h_cg_hit is bm2_cigar_hit_t with its last word named pad");

// See host_tail.h.  Every workspace is reserved before a pointer into one is taken; d_task / d_order are the caller's.
int bm2h_cgprep_dev(bm2_ctx *c, const char *who, const CgpPrm &P, const bm2_reads *reads, int32_t n, const bm2_cigar_hit_t *hits, const bm2_cigar_hit_t *d_hits,
                    bm2_cigar_task_t *d_task, int32_t *d_order, bm2_cigar_prep_t *tot, int64_t *bytes_up) {
    *bytes_up = 0;
    const int64_t nr = reads->n_reads, nb = ((int64_t)n + CGP_THREADS - 1) / CGP_THREADS, nh = nb * CGP_KEYS;
    const size_t hit_b = d_hits ? 0 : up256((size_t)n * sizeof(bm2_cigar_hit_t)), roff_b = up256((size_t)(nr + 1) * 8), rlen_b = up256((size_t)(nr + 1) * 4);
    const size_t sz_stride = up256((size_t)n * 4) / 4, pos_stride = up256((size_t)(n + 1) * 8) / 8;
    const size_t sz_b = 4 * sz_stride * 4, pos_b = 4 * pos_stride * 8, qo_b = up256((size_t)n * 8), key_b = up256((size_t)n);
    const size_t hist_b = up256((size_t)nh * 4), hpos_b = up256((size_t)(nh + 1) * 8), down_b = 256;
    int rc;
    if ((rc = bm2_reserve(c->b_cp_in, hit_b + roff_b + rlen_b + 256))) return rc;
    if ((rc = bm2_reserve(c->b_cp_work, sz_b + pos_b + qo_b + key_b + hist_b + hpos_b + down_b + 256))) return rc;
    if ((rc = bm2_reserve(c->b_cp_scan, (size_t)((nh > n ? nh : n) / 2048 + 4) * 8))) return rc;       // (what bm2_scan_i32 asks for: it will not move the buffer)
    char *d = (char *)c->b_cp_in.p, *w = (char *)c->b_cp_work.p;
    CgpArgs A;
    memset(&A, 0, sizeof A);
    A.hits = d_hits ? d_hits : (const bm2_cigar_hit_t *)d; A.roff = (const int64_t *)(d + hit_b); A.rlen = (const int32_t *)(d + hit_b + roff_b);
    A.sz = (int32_t *)w; A.pos = (int64_t *)(w + sz_b); A.q_off = (int64_t *)(w + sz_b + pos_b); A.key = (uint8_t *)(w + sz_b + pos_b + qo_b);
    A.hist = (int32_t *)(w + sz_b + pos_b + qo_b + key_b);
    int64_t *d_hpos = (int64_t *)(w + sz_b + pos_b + qo_b + key_b + hist_b);
    A.hpos = d_hpos;
    A.down = (CgpDown *)(w + sz_b + pos_b + qo_b + key_b + hist_b + hpos_b);
    A.tasks = d_task; A.order = d_order;
    A.sz_stride = (int64_t)sz_stride; A.pos_stride = (int64_t)pos_stride;
    A.n = n; A.n_reads = (int32_t)nr; A.nb = (int32_t)nb; A.P = P;
    if (!d_hits) { if ((rc = bm2_copy_h2d(c, (void *)A.hits, hits, (size_t)n * sizeof(bm2_cigar_hit_t)))) return rc; *bytes_up += (int64_t)n * (int64_t)sizeof(bm2_cigar_hit_t); }
    if (nr) {
        if ((rc = bm2_copy_h2d(c, (void *)A.roff, reads->off, (size_t)nr * 8))) return rc;
        if ((rc = bm2_copy_h2d(c, (void *)A.rlen, reads->len, (size_t)nr * 4))) return rc;
        *bytes_up += nr * 12;
    }
    hipStream_t s = c->stream;
    if ((rc = bm2_check(hipMemsetAsync(A.down, 0, sizeof(CgpDown), s), "memset prep totals"))) return rc;
    const dim3 grid((unsigned)nb), block(CGP_THREADS);
    hipLaunchKernelGGL(k_cgp_size, grid, block, 0, s, A);
    if ((rc = bm2_check(hipGetLastError(), "k_cgp_size launch"))) return rc;
    for (int k = 0; k < 4; ++k)
        if ((rc = bm2_scan_i32(c, A.sz + (size_t)k * sz_stride, n, A.pos + (size_t)k * pos_stride, c->b_cp_scan))) return rc;
    hipLaunchKernelGGL(k_cgp_task, grid, block, 0, s, A);
    hipLaunchKernelGGL(k_cgp_hist, grid, block, 0, s, A);
    if ((rc = bm2_check(hipGetLastError(), "k_cgp_task / k_cgp_hist launch"))) return rc;
    if ((rc = bm2_scan_i32(c, A.hist, nh, d_hpos, c->b_cp_scan))) return rc;
    hipLaunchKernelGGL(k_cgp_scatter, grid, block, 0, s, A);
    if ((rc = bm2_check(hipGetLastError(), "k_cgp_scatter launch"))) return rc;
    CgpDown down;
    if ((rc = bm2_check(hipMemcpyAsync(&down, A.down, sizeof down, hipMemcpyDeviceToHost, s), "D2H prep totals"))) return rc;
    if ((rc = bm2_check(hipStreamSynchronize(s), "k_cgp"))) return rc;
    if (down.err[0]) { bm2_set_error("%s: task %lld names a read or a stretch of it that does not exist", who, (long long)n - down.err[0]); return BM2_EINVAL; }
    if (down.err[1]) { bm2_set_error("%s: reference range too long", who); return BM2_EINVAL; }
    if (down.err[2]) {
        bm2_set_error("%s: task %lld has a DP area or a slice of 2^31 bytes or more, which the device form's 32-bit sizes do not hold", who, (long long)n - down.err[2]);
        return BM2_EUNSUP;
    }
    *tot = down.tot;
    return BM2_OK;
}

extern "C" int bm2_cigar_prep_dev(bm2_ctx *c, const bm2_opt *opt, int64_t l_pac, const bm2_reads *reads, int32_t n, const bm2_cigar_hit_t *hits,
                                  bm2_cigar_task_t *tasks, int32_t *order, bm2_cigar_prep_t *tot) {
    const char *who = "bm2_cigar_prep_dev";
    int rc = bm2h_cigar_prep_args(who, c, opt, reads, n, hits, tasks, order, tot);
    if (rc || n == 0) return rc;
    if ((rc = bm2_check(hipSetDevice(c->device), "hipSetDevice"))) return rc;
    bm2h_cgprep_stats_reset();
    const CgpKnobs kn = bm2h_cigar_prep_knobs();
    const CgpPrm P = cgp_prm(opt, l_pac, kn.no_lds, kn.no_ring, kn.ring_by_band, 0);
    const size_t task_b = up256((size_t)n * sizeof(bm2_cigar_task_t));
    if ((rc = bm2_reserve(c->b_cp_out, task_b + up256((size_t)n * 4) + 256))) return rc;
    bm2_cigar_task_t *d_task = (bm2_cigar_task_t *)c->b_cp_out.p;
    int32_t *d_order = (int32_t *)((char *)c->b_cp_out.p + task_b);
    bm2_cigar_prep_t t; int64_t up = 0;
    if ((rc = bm2h_cgprep_dev(c, who, P, reads, n, hits, nullptr, d_task, d_order, &t, &up))) return rc;
    if ((rc = bm2_copy_d2h(c, tasks, d_task, (size_t)n * sizeof(bm2_cigar_task_t)))) return rc;
    if ((rc = bm2_copy_d2h(c, order, d_order, (size_t)n * 4))) return rc;
    *tot = t;
    bm2h_cgprep_stats_add(&t, up, 0);
    return BM2_OK;
}

bm2h_cgprep_scope::bm2h_cgprep_scope(bm2_ctx *const *ctx, int n, const bm2_sam_opt *so) : bm2h_ctx_scope(ctx, n), mark(true) {
    const bool on = so && (so->flag & BM2_SAM_F_DEVICE_CGPREP);
    for (int g = 0; g < tc.n; ++g) if (tc.ctx[g]) tc.ctx[g]->cgprep = on;
    if (on) bm2h_cgprep_stats_reset();
}
bm2h_cgprep_scope::~bm2h_cgprep_scope() { for (int g = 0; g < tc.n; ++g) if (tc.ctx[g]) tc.ctx[g]->cgprep = false; }
