// rescue_dev.h -- the geometry of mate rescue on the device, shared by plan.hip (which alignments a pair may ask for) and rescue.hip
// (what their results do to the lists).  P is the kernel's parameter block: it holds l_pac, n_seqs, ann_off, ann_len, min_seed_len and
// the insert-size model as low[4] / high[4].
#pragma once
#include <stdint.h>

static __device__ __forceinline__ int rs_infer_dir(int64_t l_pac, int64_t b1, int64_t b2, int64_t *dist) {      // bwamem_pair.cpp:58-65
    const int r1 = (b1 >= l_pac), r2 = (b2 >= l_pac);
    const int64_t p2 = r1 == r2 ? b2 : (l_pac << 1) - 1 - b2;
    *dist = p2 > b1 ? p2 - b1 : b1 - p2;
    return (r1 == r2 ? 0 : 1) ^ (p2 > b1 ? 0 : 3);
}
template <class Prm> static __device__ int rs_pos2rid(const Prm &P, int64_t pos_f) {      // bntseq.cpp:378-392
    if (pos_f >= P.l_pac) return -1;
    int left = 0, mid = 0, right = P.n_seqs;
    while (left < right) {
        mid = (left + right) >> 1;
        if (pos_f >= P.ann_off[mid]) {
            if (mid == P.n_seqs - 1) break;
            if (pos_f < P.ann_off[mid + 1]) break;
            left = mid + 1;
        } else right = mid;
    }
    return mid;
}
// Is there a window for direction r of this anchor (rescue_window of sam_tail.cpp: bwamem_pair.cpp:176-186 with bns_fetch_seq's clamp)?
// [*rb_, *re_) = the window clamped to the anchor's contig, set when the answer is yes.
template <class Prm> static __device__ bool rs_window(const Prm &P, int64_t a_rb, int a_rid, int l_ms, int r, int64_t *rb_, int64_t *re_) {
    const int is_rev = (r >> 1 != (r & 1)), is_larger = !(r >> 1);
    int64_t rb, re;
    if (!is_rev) {
        rb = is_larger ? a_rb + P.low[r] : a_rb - P.high[r];
        re = (is_larger ? a_rb + P.high[r] : a_rb - P.low[r]) + l_ms;
    } else {
        rb = (is_larger ? a_rb + P.low[r] : a_rb - P.high[r]) - l_ms;
        re = is_larger ? a_rb + P.high[r] : a_rb - P.low[r];
    }
    if (rb < 0) rb = 0;
    if (re > P.l_pac << 1) re = P.l_pac << 1;
    if (rb >= re) return false;
    const int64_t mid = (rb + re) >> 1;
    const int rev = mid >= P.l_pac;
    const int rid = rs_pos2rid(P, rev ? (P.l_pac << 1) - 1 - mid : mid);
    if (rid < 0) return false;
    int64_t far_beg = P.ann_off[rid], far_end = far_beg + P.ann_len[rid];
    if (rev) { const int64_t t = far_beg; far_beg = (P.l_pac << 1) - far_end; far_end = (P.l_pac << 1) - t; }
    rb = rb > far_beg ? rb : far_beg;
    re = re < far_end ? re : far_end;
    if (a_rid != rid || re - rb < P.min_seed_len) return false;
    *rb_ = rb; *re_ = re;
    return true;
}
