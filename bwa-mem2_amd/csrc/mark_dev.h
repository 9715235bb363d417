// mark_dev.h -- mem_mark_primary_se (bwamem.cpp:1392-1465) and mem_reorder_primary5 (:1496-1519) as group-cooperative device code, shared
// by decide.hip (a pair's two lists, 96-byte working records) and semark.hip (a single-end list, 56-byte records).  The code is templated
// over the group's width W (a 16-lane row or a wavefront), the working record H and the uploaded record In; the including file defines,
// BEFORE the include, its records and
//     static __device__ __forceinline__ void dc_load(H &h, const In &s);      // the fields of `s` the file's rule reads, and H's own extras
// H must have: uint64_t hash; int32_t qb, qe, score, sub_n, is_alt, sub, alt_sc, secondary, secondary_all, orig, tmp.  The parameter
// block Prm must have: int32_t a, b, o_del, e_del, o_ins, e_ins; float mask_level.
//
// Why any way of sorting gives the reference's order: every ordering involved is TOTAL.  alnreg_hlt / alnreg_hlt2 end in
// hash_64(id + i), and hash_64 is a bijection of 64-bit words (each of its eight steps is invertible), so two hits of one list never
// compare equal.  A hit's rank is therefore the number of hits that compare smaller, whatever the method (here: counting).
//
// The one floating-point test is dc_covered's float multiply and compare: the including file keeps `#pragma clang fp contract(off)`.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

// ---- the group: W lanes, a barrier, W words to exchange through
#ifdef BM2_EMU_ROW_PRIMS            /* the host emulator: a rendezvous of the row's / the wavefront's threads */
template <int W> static __device__ __forceinline__ void grp_sync() { if (W == 16) emu_rsync(); else emu_wsync(); }
#else
// The lanes of a group belong to one wavefront and execute a barrier site together, so what a barrier has to do is order the memory
// operations around it: everything written before it is visible to the group's lanes after it.
template <int W> static __device__ __forceinline__ void grp_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
#endif
// U: how many of a reduction's W reads are in flight at a time.  U = W (decide.hip) unrolls the loop whole -- the wavefront form then holds
// 64 words in 128 registers across it; semark.hip takes U = 8.
template <int W, int U = W> struct Grp {
    volatile uint64_t *red; int lane;
    template <class Op> __device__ __forceinline__ uint64_t reduce(uint64_t v, Op op) const {
        red[lane] = v; grp_sync<W>();
        uint64_t r = red[0];
        if (U == W) for (int i = 1; i < W; ++i) r = op(r, red[i]);
        else {
#pragma unroll U
            for (int i = 1; i < W; ++i) r = op(r, red[i]);
        }
        grp_sync<W>();
        return r;
    }
    __device__ __forceinline__ uint64_t sum(uint64_t v) const { return reduce(v, [](uint64_t x, uint64_t y) { return x + y; }); }
    __device__ __forceinline__ uint64_t max(uint64_t v) const { return reduce(v, [](uint64_t x, uint64_t y) { return x > y ? x : y; }); }
    __device__ __forceinline__ uint64_t min(uint64_t v) const { return reduce(v, [](uint64_t x, uint64_t y) { return x < y ? x : y; }); }
};

static __device__ __forceinline__ uint64_t dc_hash_64(uint64_t key) {      // utils.h:117-128
    key += ~(key << 32); key ^= (key >> 22); key += ~(key << 13); key ^= (key >> 8);
    key += (key << 3); key ^= (key >> 15); key += ~(key << 27); key ^= (key >> 31);
    return key;
}
static __device__ __forceinline__ bool dc_covered(int xb, int xe, int yb, int ye, float mask_level) {
    const int from = xb > yb ? xb : yb, to = xe < ye ? xe : ye;
    const int lx = xe - xb, ly = ye - yb;
    return to > from && to - from >= (lx < ly ? lx : ly) * mask_level;
}
template <class H> static __device__ __forceinline__ bool dc_by_score(const H &x, const H &y) {      // alnreg_hlt
    if (x.score != y.score) return x.score > y.score;
    if (x.is_alt != y.is_alt) return x.is_alt < y.is_alt;
    return x.hash < y.hash;
}
template <class H> static __device__ __forceinline__ bool dc_assembly_first(const H &x, const H &y) { // alnreg_hlt2
    if (x.is_alt != y.is_alt) return x.is_alt < y.is_alt;
    if (x.score != y.score) return x.score > y.score;
    return x.hash < y.hash;
}
// dst = src in ascending order: the orders are total, so a hit's place is the number of hits before it
template <int W, int U, class H, class Less> static __device__ void dc_sort(const Grp<W, U> &G, int n, const H *src, H *dst, Less less) {
    for (int i = G.lane; i < n; i += W) {
        const H h = src[i];
        int r = 0;
        for (int j = 0; j < n; ++j) r += less(src[j], h) ? 1 : 0;
        dst[r] = h;
    }
    grp_sync<W>();
}
// mem_mark_primary_se_core over a[0, n): the ranks one after the other; the lanes search the leaders so far (a[t].tmp = the t-th
// leader, in the order they were made, so the first covering one is the smallest t), lane 0 books the result
template <int W, int U, class Prm, class H> static __device__ void dc_follow_leaders(const Grp<W, U> &G, const Prm &P, int n, H *a) {
    int close = P.a + P.b;
    if (close < P.o_del + P.e_del) close = P.o_del + P.e_del;
    if (close < P.o_ins + P.e_ins) close = P.o_ins + P.e_ins;
    int n_lead = 0;
    for (int i = 0; i < n; ++i) {
        const int qb = a[i].qb, qe = a[i].qe;
        uint64_t found = ~0ull;
        for (int t = G.lane; t < n_lead; t += W) {
            const H &L = a[a[t].tmp];
            if (dc_covered(L.qb, L.qe, qb, qe, P.mask_level)) { found = (uint64_t)t; break; }
        }
        found = G.min(found);
        if (found == ~0ull) {
            if (G.lane == 0) a[n_lead].tmp = i;
            ++n_lead;
        } else if (G.lane == 0) {
            const int j = a[(int)found].tmp;
            if (a[j].sub == 0) a[j].sub = a[i].score;
            if (a[j].score - a[i].score <= close && (a[j].is_alt || !a[i].is_alt)) ++a[j].sub_n;
            a[i].secondary = j;
        }
        grp_sync<W>();
    }
}
// mem_mark_primary_se (bwamem.cpp:1420-1465) of one list: in[0, n) -> a[0, n) (b: as much room again), -> hits on the primary assembly
template <int W, int U, class Prm, class In, class H> static __device__ int dc_mark_primary(const Grp<W, U> &G, const Prm &P, int n, const In *in, H *a, H *b, int64_t id) {
    if (n == 0) return 0;
    int cnt = 0;
    for (int i = G.lane; i < n; i += W) {
        const In s = in[i];
        H h;
        dc_load(h, s);
        h.sub = h.alt_sc = 0; h.secondary = h.secondary_all = -1; h.hash = dc_hash_64((uint64_t)(id + i));
        h.orig = i; h.tmp = 0;
        b[i] = h;
        cnt += !s.is_alt;
    }
    const int n_assembly = (int)G.sum((uint64_t)cnt);            // (its barriers publish b)
    dc_sort<W>(G, n, b, a, [](const H &x, const H &y) { return dc_by_score(x, y); });
    dc_follow_leaders<W>(G, P, n, a);
    for (int i = G.lane; i < n; i += W) {
        a[i].secondary_all = i;
        const int lead = a[i].secondary;
        if (!a[i].is_alt && lead >= 0 && a[lead].is_alt) a[i].alt_sc = a[lead].score;
    }
    grp_sync<W>();
    if (n_assembly == n) {
        for (int i = G.lane; i < n; i += W) a[i].secondary_all = a[i].secondary;
        grp_sync<W>();
        return n_assembly;
    }
    if (n_assembly > 0) {
        dc_sort<W>(G, n, a, b, [](const H &x, const H &y) { return dc_assembly_first(x, y); });
        for (int i = G.lane; i < n; i += W) a[i] = b[i];
        grp_sync<W>();
    }
    for (int i = G.lane; i < n; i += W) a[a[i].secondary_all].tmp = i;      // rank in the all-hits ranking -> position now
    grp_sync<W>();
    for (int i = G.lane; i < n; i += W) {
        const int lead = a[i].secondary;
        if (lead < 0) { a[i].secondary_all = -1; continue; }
        a[i].secondary_all = a[lead].tmp;
        if (a[i].is_alt) a[i].secondary = INT_MAX;
    }
    grp_sync<W>();
    if (n_assembly > 0) {
        for (int i = G.lane; i < n_assembly; i += W) { a[i].sub = 0; a[i].secondary = -1; }
        grp_sync<W>();
        dc_follow_leaders<W>(G, P, n_assembly, a);
    }
    return n_assembly;
}
// mem_reorder_primary5 (bwamem.cpp:1496-1519)
template <int W, int U, class H> static __device__ void dc_reorder_primary5(const Grp<W, U> &G, int T, int n, H *a) {
    if (G.lane == 0) {
        int count = 0, leftmost = -1;
        for (int k = 0; k < n; ++k) {
            if (!(a[k].secondary < 0 && !a[k].is_alt && a[k].score >= T)) continue;
            ++count;
            if (leftmost < 0 || a[k].qb < a[leftmost].qb) leftmost = k;
        }
        if (count > 1 && leftmost != 0) {
            const H t = a[0]; a[0] = a[leftmost]; a[leftmost] = t;
            for (int k = 1; k < n; ++k) {
                const int s = a[k].secondary, sa = a[k].secondary_all;
                a[k].secondary = s == 0 ? leftmost : s == leftmost ? 0 : s;
                a[k].secondary_all = sa == 0 ? leftmost : sa == leftmost ? 0 : sa;
            }
        }
    }
    grp_sync<W>();
}
