// samfmt.hip -- SAM text on the device: mem_aln2sam (bwamem.cpp:1592-1730) for a batch of DECIDED records (bm2_samrec_t, include/bm2.h).
// Integer and byte work only: what is rare or floating point (SA:Z:, pa:f:, XA:Z:, the -C comment, XR:Z:) arrives pre-formatted as one
// blob per record and is copied.  Host oracle: aln2sam in sam_tail.cpp, pinned byte for byte against the reference.
//
//   k_sam_size   one lane per record: the line's exact length from the record alone (digit counts, stored string lengths, separators)
//   bm2_scan_i32 exclusive scan of the lengths in 64 bits -> where every line starts; the total goes to the host for the cap check
//   k_sam_write  one workgroup per TILE bytes of the OUTPUT: the lines that overlap the tile are found by bisection of the offsets, the
//                tile is assembled in LDS (a wavefront per line; all four on a line when a tile holds one or two, i.e. long reads -- a
//                line of any length is simply visited by every tile it crosses), then flushed with 16-byte stores, lane i on bytes
//                [16 i, 16 i + 16) of the tile: tiles start at multiples of TILE in a 256-byte-aligned buffer, so every store of the
//                stream is aligned and full except the last few bytes of the last tile.  No lane walks a string: names, MD, blobs are
//                copied a byte per lane, SEQ is made four bases per lane from word loads of the codes, QUAL is a (reversed) word copy.
// Both kernels lay a line out with the SAME function (sam_line), so the sizes and the text cannot disagree.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <string>
#include <vector>
#include "../../include/bm2.h"
#include "bm2_ctx.h"
#include "host_tail.h"
#include "host_pool.h"
#include "pipeline.h"

#define SAMFMT_TILE 16384           // bytes of output per workgroup = its LDS window
#define SAMFMT_THREADS 256

struct SamRecTxt { int64_t seq_off, name_off, qual_off; int32_t name_len, pad; };    // per record: where its read's codes, name and the qualities it prints lie (qual_off < 0: none)
struct SamFmtArgs {
    const bm2_samrec_t *recs; const SamRecTxt *rtx; const uint32_t *cg; const char *side;
    const uint8_t *txt; int64_t txt_lim;                        // names and quality slices of the call, back to back; *_lim = readable bytes (a multiple of 4)
    const uint8_t *enc; int64_t enc_lim;                        // the reads' codes
    const char *cname; const int32_t *cname_off;                // contig names
    int64_t rg_off; int32_t rg_len; int32_t pad;                // RG:Z: value inside txt
    int64_t n_rec;
};
struct SamTile { char *lds; int rel, tid, nth, lane; bool cgw; };     // rel = line start - tile start; (tid, nth) = this thread among those working on the line

static __device__ __forceinline__ int ndig32(uint32_t v) {
    return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}
static __device__ __forceinline__ int ndig64(uint64_t v) {
    if (!(v >> 32)) return ndig32((uint32_t)v);
    int d = 10; uint64_t p = 10000000000ull;
    while (d < 20 && v >= p) { ++d; if (d < 20) p *= 10; }
    return d;
}
static __device__ __forceinline__ int ndig_s(int64_t v) { return v < 0 ? 1 + ndig64(0ull - (uint64_t)v) : ndig64((uint64_t)v); }
static __device__ __forceinline__ uint64_t pow10_u64(int e) { uint64_t p = 1; for (int i = 0; i < e; ++i) p *= 10; return p; }

static __device__ __forceinline__ void wr(const SamTile &T, int p, int b) {
    const int q = T.rel + p;
    if ((unsigned)q < (unsigned)SAMFMT_TILE) T.lds[q] = (char)b;
}
// four consecutive bytes (little end first), the first `nv` of them valid: one LDS word store when they lie aligned inside the tile
static __device__ __forceinline__ void wr4(const SamTile &T, int p, uint32_t w, int nv) {
    const int q = T.rel + p;
    if (nv == 4 && !(q & 3) && (unsigned)q < (unsigned)SAMFMT_TILE) { *(uint32_t *)(T.lds + q) = w; return; }
    for (int k = 0; k < 4; ++k) if (k < nv) wr(T, p + k, (int)(w >> (8 * k) & 0xff));
}
// the part [lo, hi) of a piece of L bytes at line position p that falls into the tile
static __device__ __forceinline__ void clip(const SamTile &T, int p, int L, int &lo, int &hi) {
    const int q = T.rel + p;
    lo = q < 0 ? -q : 0;
    hi = L < SAMFMT_TILE - q ? L : SAMFMT_TILE - q;
}
// four bytes from byte address a of a 4-byte-aligned array (a may be unaligned, and up to 3 bytes outside [0, lim)): two aligned word loads
static __device__ __forceinline__ uint32_t ld4(const uint8_t *__restrict__ base, int64_t a, int64_t lim) {
    const int64_t wa = a & ~(int64_t)3; const int s = (int)(a & 3) * 8;
    const uint32_t lo = (wa >= 0 && wa < lim) ? *(const uint32_t *)(base + wa) : 0u;
    if (!s) return lo;
    const uint32_t hi = (wa + 4 >= 0 && wa + 4 < lim) ? *(const uint32_t *)(base + wa + 4) : 0u;
    return lo >> s | hi << (32 - s);
}
static __device__ __forceinline__ uint32_t bswap4(uint32_t w) { return w >> 24 | (w >> 8 & 0xff00u) | (w << 8 & 0xff0000u) | w << 24; }
// "ACGTN"[c] / "TGCAN"[c] for four codes at once (a code above 4 prints N)
static __device__ __forceinline__ uint32_t bases4(uint32_t w, bool rev) {
    const uint64_t tab = rev ? 0x4e41434754ull : 0x4e54474341ull;
    uint32_t o = 0;
    for (int k = 0; k < 4; ++k) { uint32_t c = w >> (8 * k) & 0xff; c = c > 4 ? 4 : c; o |= (uint32_t)(tab >> (8 * c) & 0xff) << (8 * k); }
    return o;
}

static __device__ __forceinline__ void put_bytes(const SamTile &T, int p, const char *__restrict__ src, int L) {
    int lo, hi; clip(T, p, L, lo, hi);
    for (int i = lo + T.tid; i < hi; i += T.nth) T.lds[T.rel + p + i] = src[i];
}
static __device__ __forceinline__ void put_const(const SamTile &T, int p, uint64_t packed, int n) {        // up to 8 bytes, little end first
    if (T.tid < n) wr(T, p + T.tid, (int)(packed >> (8 * T.tid) & 0xff));
}
static __device__ __forceinline__ void put_dec(const SamTile &T, int p, int64_t v, int d) {                 // d = ndig_s(v): one digit per lane
    const int neg = v < 0;
    const uint64_t x = neg ? 0ull - (uint64_t)v : (uint64_t)v;
    const int k = T.tid - neg;                                   // digit k of d - neg, most significant first
    if (T.tid >= d) return;
    if (k < 0) { wr(T, p, '-'); return; }
    const int e = d - neg - 1 - k;
    const int digit = (x >> 32) ? (int)(x / pow10_u64(e) % 10) : (int)((uint32_t)x / (uint32_t)pow10_u64(e) % 10u);
    wr(T, p + T.tid, '0' + digit);
}
// a CIGAR's text: op k starts where the widths of the ops before it end (a scan over the wavefront, 64 ops a round); every lane writes its op
static __device__ __forceinline__ void put_cigar(const SamTile &T, int p, const uint32_t *__restrict__ cg, int n, int text_len) {
    int lo, hi; clip(T, p, text_len, lo, hi);
    if (lo >= hi) return;                                        // (wave-uniform: a whole wavefront works on a line)
    int base = 0;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + T.lane;
        const uint32_t c = k < n ? cg[k] : 0u;
        const int w = k < n ? ndig32(c >> 4) + 1 : 0;
        int incl = w;
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl(incl, (T.lane - d) & 63); if (T.lane >= d) incl += t; }
        const int at = p + base + incl - w;
        if (k < n && T.cgw) {
            uint32_t v = c >> 4;
            for (int j = w - 2; j >= 0; --j) { wr(T, at + j, '0' + (int)(v % 10u)); v /= 10u; }
            const uint32_t op = (c & 0xf) > 4 ? 4 : (c & 0xf);
            wr(T, at + w - 1, (int)(0x485344494dull >> (8 * op) & 0xff));         // "MIDSH"
        }
        base += __shfl(incl, 63);
    }
}
// SEQ (map = true: codes -> letters, complemented when reversed) or QUAL (a copy) of L bytes whose source starts at byte a0 of `src`: four output bytes
// per lane from word loads, consecutive lanes on consecutive words
static __device__ __forceinline__ void put_run(const SamTile &T, int p, const uint8_t *__restrict__ src, int64_t lim, int64_t a0, int L, bool rev, bool map) {
    int lo, hi; clip(T, p, L, lo, hi);
    for (int j = (lo >> 2) + T.tid; j * 4 < hi; j += T.nth) {
        const int i = j * 4;
        uint32_t w = rev ? bswap4(ld4(src, a0 + L - 4 - i, lim)) : ld4(src, a0 + i, lim);
        if (map) w = bases4(w, rev);
        wr4(T, p + i, w, L - i < 4 ? L - i : 4);
    }
}

static constexpr uint64_t pk8(const char *s) { uint64_t v = 0; for (int i = 0; s[i]; ++i) v |= (uint64_t)(unsigned char)s[i] << (8 * i); return v; }

// One line, piece by piece in mem_aln2sam's order.  WRITE = false: only the position advances (k_sam_size); true: the pieces are written by the
// threads of T.  cg_len / mc_len = bytes of the two CIGARs' text.  -> the line's length.
template <bool WRITE>
static __device__ __forceinline__ int sam_line(const SamFmtArgs &A, const bm2_samrec_t &R, const SamRecTxt &X, int cg_len, int mc_len, const SamTile &T) {
    int p = 0;
#define SAM_TAB() do { if (WRITE && T.tid == 0) wr(T, p, '\t'); ++p; } while (0)
#define SAM_DEC(v) do { const int64_t v_ = (int64_t)(v); const int d_ = ndig_s(v_); if (WRITE) put_dec(T, p, v_, d_); p += d_; } while (0)
#define SAM_CONST(str, n) do { if (WRITE) put_const(T, p, pk8(str), (n)); p += (n); } while (0)
#define SAM_BYTES(src, n) do { const int n_ = (n); if (WRITE) put_bytes(T, p, (src), n_); p += n_; } while (0)
    SAM_BYTES((const char *)A.txt + X.name_off, X.name_len); SAM_TAB();
    SAM_DEC((uint32_t)R.flag); SAM_TAB();
    if (R.rid >= 0) {
        const int o = A.cname_off[R.rid];
        SAM_BYTES(A.cname + o, A.cname_off[R.rid + 1] - o); SAM_TAB();
        SAM_DEC(R.pos); SAM_TAB();
        SAM_DEC(R.mapq); SAM_TAB();
        if (R.n_cigar > 0) { if (WRITE) put_cigar(T, p, A.cg + R.cigar_off, R.n_cigar, cg_len); p += cg_len; }
        else SAM_CONST("*", 1);
    } else SAM_CONST("*\t0\t0\t*", 7);
    SAM_TAB();
    if (R.mrid >= 0) {
        if (R.rnext_eq) SAM_CONST("=", 1);
        else { const int o = A.cname_off[R.mrid]; SAM_BYTES(A.cname + o, A.cname_off[R.mrid + 1] - o); }
        SAM_TAB();
        SAM_DEC(R.mpos); SAM_TAB();
        SAM_DEC(R.tlen);
    } else SAM_CONST("*\t0\t0", 5);
    SAM_TAB();
    if (R.no_seq) SAM_CONST("*\t*", 3);
    else {
        const int L = R.qe - R.qb;
        if (WRITE) put_run(T, p, A.enc, A.enc_lim, X.seq_off + R.qb, L, R.is_rev != 0, true);
        p += L; SAM_TAB();
        if (X.qual_off >= 0) { if (WRITE) put_run(T, p, A.txt, A.txt_lim, X.qual_off, L, R.is_rev != 0, false); p += L; }
        else SAM_CONST("*", 1);
    }
    if (R.n_cigar > 0) { SAM_CONST("\tNM:i:", 6); SAM_DEC(R.nm); SAM_CONST("\tMD:Z:", 6); SAM_BYTES(A.side + R.md_off, R.md_len); }
    if (R.n_mc > 0) { SAM_CONST("\tMC:Z:", 6); if (WRITE) put_cigar(T, p, A.cg + R.mc_off, R.n_mc, mc_len); p += mc_len; }
    if (R.score >= 0) { SAM_CONST("\tAS:i:", 6); SAM_DEC(R.score); }
    if (R.sub >= 0) { SAM_CONST("\tXS:i:", 6); SAM_DEC(R.sub); }
    if (A.rg_len > 0) { SAM_CONST("\tRG:Z:", 6); SAM_BYTES((const char *)A.txt + A.rg_off, A.rg_len); }
    SAM_BYTES(A.side + R.blob_off, R.blob_len);
    SAM_CONST("\n", 1);
#undef SAM_TAB
#undef SAM_DEC
#undef SAM_CONST
#undef SAM_BYTES
    return p;
}

__global__ void __launch_bounds__(256) k_sam_size(SamFmtArgs A, int32_t *__restrict__ len, int2 *__restrict__ aux) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= A.n_rec) return;
    const bm2_samrec_t R = A.recs[r];
    const SamRecTxt X = A.rtx[r];
    int cg = 0, mc = 0;
    for (int k = 0; k < R.n_cigar; ++k) cg += ndig32(A.cg[R.cigar_off + k] >> 4) + 1;
    for (int k = 0; k < R.n_mc; ++k) mc += ndig32(A.cg[R.mc_off + k] >> 4) + 1;
    SamTile T; T.lds = nullptr; T.rel = 0; T.tid = 0; T.nth = 1; T.lane = 0; T.cgw = false;
    len[r] = sam_line<false>(A, R, X, cg, mc, T);
    aux[r] = make_int2(cg, mc);
}

__global__ void __launch_bounds__(SAMFMT_THREADS) k_sam_write(SamFmtArgs A, const int64_t *__restrict__ off, const int2 *__restrict__ aux, char *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) char win[SAMFMT_TILE];
    const int64_t total = off[A.n_rec];
    const int64_t t0 = (int64_t)blockIdx.x * SAMFMT_TILE, t1 = t0 + SAMFMT_TILE < total ? t0 + SAMFMT_TILE : total;
    int64_t first = 0, last = A.n_rec;                          // lines [first, last) overlap [t0, t1): first = the last line that starts at or before t0
    for (int64_t hi = A.n_rec; hi - first > 1;) { const int64_t mid = (first + hi) >> 1; if (off[mid] <= t0) first = mid; else hi = mid; }
    for (int64_t lo = first; lo < last;) { const int64_t mid = (lo + last) >> 1; if (off[mid] < t1) lo = mid + 1; else last = mid; }
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const bool coop = last - first <= 2;                        // long lines: the whole workgroup on each
    SamTile T; T.lds = win; T.lane = (int)threadIdx.x & 63;
    T.tid = coop ? (int)threadIdx.x : T.lane; T.nth = coop ? SAMFMT_THREADS : 64; T.cgw = !coop || wave == 0;
    for (int64_t r = first + (coop ? 0 : wave); r < last; r += coop ? 1 : SAMFMT_THREADS / 64) {
        const bm2_samrec_t R = A.recs[r];
        const SamRecTxt X = A.rtx[r];
        const int2 a = aux[r];
        T.rel = (int)(off[r] - t0);
        sam_line<true>(A, R, X, a.x, a.y, T);
    }
    __syncthreads();
    const int valid = (int)(t1 - t0);
    for (int o = (int)threadIdx.x * 16; o < valid; o += SAMFMT_THREADS * 16) {
        if (o + 16 <= valid) *(uint4 *)(out + t0 + o) = *(const uint4 *)(win + o);
        else for (int k = o; k < valid; ++k) out[t0 + k] = win[k];                 // the last bytes of the stream
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
namespace {
std::atomic<long long> g_txt_records{0}, g_txt_dev{0}, g_txt_host{0};      // bm2_sam_text_stats

struct SamFmtJob { SamFmtArgs A; int64_t total = 0, blob = 0; int32_t *d_len = nullptr; int2 *d_aux = nullptr; int64_t *d_off = nullptr; };
inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// inputs to the device, sizes, offsets; J.total = bytes of the text.  Offsets of the records index cigar / side after cg_base / side_base are taken off.
int samfmt_prepare(bm2_ctx *c, const bm2_sam_opt *so, const bm2_reads *reads, const bm2_read_text *txt, int64_t n_rec, const bm2_samrec_t *recs,
                   const uint32_t *cigar, int64_t cg_base, int64_t n_cigar, const char *side, int64_t side_base, int64_t side_bytes, bool reuse_enc,
                   SamFmtJob &J) {
    int rc = bm2_check(hipSetDevice(c->device), "hipSetDevice");
    if (rc) return rc;
    TailProf prof("sam_format_dev");
    const int host_threads = bm2_host_threads();
    const int n_reads = reads->n_reads;
    const int n_seqs = c->ix.n_seqs;
    const int64_t grain = 16384, pieces = (n_rec + grain - 1) / grain;
    static thread_local std::vector<SamRecTxt> rtx_tl; static thread_local std::vector<bm2_samrec_t> recs_tl;
    std::vector<SamRecTxt> &rtx = rtx_tl;
    rtx.resize((size_t)n_rec);
    const bool rebase = cg_base != 0 || side_base != 0;
    if (rebase) recs_tl.resize((size_t)n_rec);
    std::vector<int64_t> piece_at((size_t)pieces + 1, 0), piece_blob((size_t)pieces, 0);
    std::atomic<int64_t> bad(-1);
    bm2_parallel_ranges(n_rec, grain, host_threads, [&](int64_t lo, int64_t hi) {      // every offset the kernels will follow is checked here
        int64_t bytes = 0, blob = 0;
        for (int64_t i = lo; i < hi; ++i) {
            bm2_samrec_t r = recs[i];
            r.cigar_off -= cg_base; r.mc_off -= cg_base; r.md_off -= side_base; r.blob_off -= side_base;
            bool ok = r.read >= 0 && r.read < n_reads && r.rid < n_seqs && r.mrid < n_seqs && r.n_cigar >= 0 && r.n_mc >= 0 && r.md_len >= 0 && r.blob_len >= 0 &&
                      r.cigar_off >= 0 && r.cigar_off + r.n_cigar <= n_cigar && r.mc_off >= 0 && r.mc_off + r.n_mc <= n_cigar &&
                      r.md_off >= 0 && r.md_off + r.md_len <= side_bytes && r.blob_off >= 0 && r.blob_off + r.blob_len <= side_bytes;
            if (ok && !r.no_seq) ok = r.qb >= 0 && r.qb <= r.qe && r.qe <= reads->len[r.read];
            if (ok && !txt->name[r.read]) ok = false;
            if (!ok) { int64_t e = -1; bad.compare_exchange_strong(e, i); continue; }
            if (rebase) recs_tl[(size_t)i] = r;
            SamRecTxt &x = rtx[(size_t)i];
            x.seq_off = reads->off[r.read];
            x.name_len = (int32_t)strlen(txt->name[r.read]); x.pad = 0;
            const bool q = !r.no_seq && txt->qual && txt->qual[r.read];
            x.qual_off = q ? 0 : -1;
            bytes += x.name_len + (q ? r.qe - r.qb : 0);
            blob += r.blob_len;
        }
        piece_at[(size_t)(lo / grain) + 1] = bytes; piece_blob[(size_t)(lo / grain)] = blob;
    });
    if (bad.load() >= 0) { bm2_set_error("bm2_sam_format_dev: record %lld points outside the reads, the contigs, the CIGAR ops or the side bytes", (long long)bad.load()); return BM2_EINVAL; }
    const char *rg = so->rg_id && so->rg_id[0] ? so->rg_id : nullptr;
    const size_t rg_len = rg ? strlen(rg) : 0;
    piece_at[0] = (int64_t)rg_len;
    J.blob = 0;
    for (int64_t k = 0; k < pieces; ++k) { piece_at[(size_t)k + 1] += piece_at[(size_t)k]; J.blob += piece_blob[(size_t)k]; }
    const size_t txt_bytes = (size_t)piece_at[(size_t)pieces];
    // names and quality slices, packed into page-locked memory on the pool's threads (the copy to the device is then plain DMA)
    if (c->txt_pin_cap < txt_bytes + 64) {
        if (c->txt_pin) { (void)hipHostFree(c->txt_pin); c->txt_pin = nullptr; c->txt_pin_cap = 0; }
        const size_t want = txt_bytes + txt_bytes / 8 + ((size_t)1 << 20);
        if (bm2_check(hipHostMalloc(&c->txt_pin, want, 0), "hipHostMalloc(text staging)")) { c->txt_pin = nullptr; return BM2_ENOMEM; }
        c->txt_pin_cap = want;
    }
    char *const pack = (char *)c->txt_pin;
    if (rg_len) memcpy(pack, rg, rg_len);
    const bm2_samrec_t *const use = rebase ? recs_tl.data() : recs;
    bm2_parallel_ranges(n_rec, grain, host_threads, [&](int64_t lo, int64_t hi) {
        int64_t at = piece_at[(size_t)(lo / grain)];
        for (int64_t i = lo; i < hi; ++i) {
            const bm2_samrec_t &r = use[i];
            SamRecTxt &x = rtx[(size_t)i];
            x.name_off = at; memcpy(pack + at, txt->name[r.read], (size_t)x.name_len); at += x.name_len;
            if (x.qual_off >= 0) { x.qual_off = at; memcpy(pack + at, txt->qual[r.read] + r.qb, (size_t)(r.qe - r.qb)); at += r.qe - r.qb; }
        }
    });
    prof.mark("pack");
    int64_t enc_bytes = 0;
    for (int i = 0; i < n_reads; ++i) if (reads->off[i] + reads->len[i] > enc_bytes) enc_bytes = reads->off[i] + reads->len[i];
    const size_t rec_b = up16((size_t)n_rec * sizeof(bm2_samrec_t)), rtx_b = up16((size_t)n_rec * sizeof(SamRecTxt)), cg_b = up16((size_t)n_cigar * 4),
                 side_b = up16((size_t)side_bytes), txt_b = up16(txt_bytes);
    if ((rc = bm2_reserve(c->b_txt_in, rec_b + rtx_b + cg_b + side_b + txt_b + 64))) return rc;
    const size_t len_b = up16((size_t)(n_rec + 1) * 4), aux_b = up16((size_t)n_rec * sizeof(int2));
    if ((rc = bm2_reserve(c->b_txt_pos, len_b + aux_b + (size_t)(n_rec + 2) * 8 + 64))) return rc;
    char *d = (char *)c->b_txt_in.p;
    SamFmtArgs &A = J.A;
    A.recs = (const bm2_samrec_t *)d; A.rtx = (const SamRecTxt *)(d + rec_b); A.cg = (const uint32_t *)(d + rec_b + rtx_b);
    A.side = d + rec_b + rtx_b + cg_b; A.txt = (const uint8_t *)(d + rec_b + rtx_b + cg_b + side_b); A.txt_lim = (int64_t)((txt_bytes + 3) & ~(size_t)3);
    A.cname = (const char *)c->d_ann_names; A.cname_off = (const int32_t *)c->d_ann_name_off;
    A.rg_off = 0; A.rg_len = (int32_t)rg_len; A.pad = 0; A.n_rec = n_rec;
    rc = bm2_copy_h2d(c, (void *)A.recs, use, (size_t)n_rec * sizeof(bm2_samrec_t));
    if (!rc) rc = bm2_copy_h2d(c, (void *)A.rtx, rtx.data(), (size_t)n_rec * sizeof(SamRecTxt));
    if (!rc && n_cigar) rc = bm2_copy_h2d(c, (void *)A.cg, cigar + cg_base, (size_t)n_cigar * 4);
    if (!rc && side_bytes) rc = bm2_copy_h2d(c, (void *)A.side, side + side_base, (size_t)side_bytes);
    if (!rc && txt_bytes) rc = bm2_copy_h2d(c, (void *)A.txt, pack, txt_bytes);
    if (rc) return rc;
    if (reuse_enc && c->tail_enc == (const void *)reads->enc && c->tail_enc_bytes == (size_t)enc_bytes && c->b_ref.p && c->b_ref.cap >= (size_t)enc_bytes + 4) {
        A.enc = (const uint8_t *)c->b_ref.p;                     // the copy the CIGAR batch of this call uploaded
    } else {
        if ((rc = bm2_reserve(c->b_txt_enc, (size_t)enc_bytes + 64))) return rc;
        if (enc_bytes && (rc = bm2_copy_h2d(c, c->b_txt_enc.p, reads->enc, (size_t)enc_bytes))) return rc;
        A.enc = (const uint8_t *)c->b_txt_enc.p;
    }
    A.enc_lim = (enc_bytes + 3) & ~(int64_t)3;
    prof.mark("H2D");
    J.d_len = (int32_t *)c->b_txt_pos.p; J.d_aux = (int2 *)((char *)c->b_txt_pos.p + len_b); J.d_off = (int64_t *)((char *)c->b_txt_pos.p + len_b + aux_b);
    hipLaunchKernelGGL(k_sam_size, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, c->stream, A, J.d_len, J.d_aux);
    if ((rc = bm2_check(hipGetLastError(), "k_sam_size launch"))) return rc;
    if ((rc = bm2_scan_i32(c, J.d_len, n_rec, J.d_off, c->b_txt_scan))) return rc;
    if ((rc = bm2_check(hipMemcpyAsync(&J.total, J.d_off + n_rec, 8, hipMemcpyDeviceToHost, c->stream), "D2H text size"))) return rc;
    rc = bm2_check(hipStreamSynchronize(c->stream), "k_sam_size");
    prof.mark("size + scan");
    return rc;
}
// the text of a prepared job -> out (J.total bytes)
int samfmt_finish(bm2_ctx *c, const SamFmtJob &J, char *out) {
    if (J.total <= 0) return BM2_OK;
    int rc = bm2_check(hipSetDevice(c->device), "hipSetDevice");
    if (rc) return rc;
    TailProf prof("sam_format_dev");
    if ((rc = bm2_reserve(c->b_txt_out, (size_t)J.total + 64))) return rc;
    const int64_t tiles = (J.total + SAMFMT_TILE - 1) / SAMFMT_TILE;
    hipLaunchKernelGGL(k_sam_write, dim3((unsigned)tiles), dim3(SAMFMT_THREADS), 0, c->stream, J.A, (const int64_t *)J.d_off, (const int2 *)J.d_aux, (char *)c->b_txt_out.p);
    if ((rc = bm2_check(hipGetLastError(), "k_sam_write launch"))) return rc;
    rc = bm2_copy_d2h(c, out, c->b_txt_out.p, (size_t)J.total);
    prof.mark("write + D2H");
    return rc;
}
bool text_ready(const bm2_ctx *c, const char *who) {
    if (!c || !c->has_index) { bm2_set_error("%s: the context holds no index", who); return false; }
    if (!c->d_ann_names || !c->d_ann_name_off) { bm2_set_error("%s: the context was created from a descriptor without contig names", who); return false; }
    return true;
}
}  // namespace

extern "C" void bm2_sam_text_stats(int64_t *records, int64_t *device_bytes, int64_t *host_bytes) {
    if (records) *records = g_txt_records.load();
    if (device_bytes) *device_bytes = g_txt_dev.load();
    if (host_bytes) *host_bytes = g_txt_host.load();
}

extern "C" int bm2_sam_format_dev(bm2_ctx *c, const bm2_sam_opt *so, const bm2_reads *reads, const bm2_read_text *txt, int64_t n_rec,
                                  const bm2_samrec_t *recs, const uint32_t *cigar, int64_t n_cigar, const char *side, int64_t side_bytes,
                                  char *out, int64_t cap, int64_t *n_out) {
    if (!c || !so || !reads || !txt || !txt->name || !n_out || n_rec < 0 || n_rec > 0x7fffffff || n_cigar < 0 || side_bytes < 0 || cap < 0 ||
        (n_rec > 0 && (!recs || !reads->off || !reads->len || (!reads->enc && reads->n_reads > 0))) || (n_cigar > 0 && !cigar) || (side_bytes > 0 && !side)) {
        bm2_set_error("bm2_sam_format_dev: bad argument"); return BM2_EINVAL;
    }
    if (!text_ready(c, "bm2_sam_format_dev")) return BM2_EINVAL;
    *n_out = 0;
    g_txt_records = 0; g_txt_dev = 0; g_txt_host = 0;
    if (n_rec == 0) return BM2_OK;
    SamFmtJob J;
    int rc = samfmt_prepare(c, so, reads, txt, n_rec, recs, cigar, 0, n_cigar, side, 0, side_bytes, false, J);
    if (rc) return rc;
    *n_out = J.total;
    if (J.total > cap) return BM2_ECAP;
    if (!out) { bm2_set_error("bm2_sam_format_dev: no output buffer"); return BM2_EINVAL; }
    if ((rc = samfmt_finish(c, J, out))) return rc;
    g_txt_records = (long long)n_rec; g_txt_host = (long long)J.blob; g_txt_dev = (long long)(J.total - J.blob);
    return BM2_OK;
}

// ---- the hook of the SAM tail (bm2h_text_batch_fn; user = bm2h_text_ctxs): the chunk's records cut into contiguous parts, one context and
// one host thread per part; every part is sized first, so the cap is checked before a byte reaches `out`, then written to its place.
// (The records of the tail come block after block: their offsets into the ops and the side bytes rise with the record, so a part's share
// of both arrays is the stretch between its first record's offsets and the next part's.)
int bm2h_dev_text_batch(void *user, const bm2_sam_opt *so, const bm2_reads *reads, const bm2_read_text *txt, int64_t n_rec, const bm2_samrec_t *recs,
                        const uint32_t *cigar, int64_t n_cigar, const char *side, int64_t side_bytes, char *out, int64_t cap, int64_t *n_out) {
    const bm2h_text_ctxs *m = (const bm2h_text_ctxs *)user;
    *n_out = 0;
    g_txt_records = 0; g_txt_dev = 0; g_txt_host = 0;
    for (int g = 0; g < m->n; ++g) if (!text_ready(m->ctx[g], "BM2_SAM_F_DEVICE_TEXT")) return BM2_EINVAL;
    if (n_rec > 0x7fffffff) { bm2_set_error("BM2_SAM_F_DEVICE_TEXT: too many records in one chunk"); return BM2_EINVAL; }
    if (n_rec == 0) return BM2_OK;
    const int G = bm2_parts(n_rec, bm2_knob("BM2_TEXT_PART", 65536), m->n);      // knob: records that are worth a context of their own (launch policy)
    std::vector<SamFmtJob> jobs((size_t)G);
    const int budget = G > 1 ? bm2_part_budget(G) : 0;           // (one part: the caller's own budget)
    int rc = bm2_run_parts(G, budget, nullptr, [&](int g) {
        const int64_t lo = bm2_part_lo(n_rec, g, G), hi = bm2_part_lo(n_rec, g + 1, G);
        const int64_t c0 = g ? recs[lo].cigar_off : 0, c1 = g + 1 < G ? recs[hi].cigar_off : n_cigar;
        const int64_t s0 = g ? recs[lo].md_off : 0, s1 = g + 1 < G ? recs[hi].md_off : side_bytes;
        if (c0 < 0 || c1 < c0 || c1 > n_cigar || s0 < 0 || s1 < s0 || s1 > side_bytes) { bm2_set_error("BM2_SAM_F_DEVICE_TEXT: record offsets out of order"); return BM2_EINVAL; }
        return samfmt_prepare(m->ctx[g], so, reads, txt, hi - lo, recs + lo, cigar, c0, c1 - c0, side, s0, s1 - s0, true, jobs[(size_t)g]);
    });
    if (rc) return rc;
    int64_t total = 0, blob = 0;
    std::vector<int64_t> at((size_t)G, 0);
    for (int g = 0; g < G; ++g) { at[(size_t)g] = total; total += jobs[(size_t)g].total; blob += jobs[(size_t)g].blob; }
    *n_out = total;
    if (total > cap) return BM2_ECAP;
    if (!out) { bm2_set_error("BM2_SAM_F_DEVICE_TEXT: no output buffer"); return BM2_EINVAL; }
    if ((rc = bm2_run_parts(G, budget, nullptr, [&](int g) { return samfmt_finish(m->ctx[g], jobs[(size_t)g], out + at[(size_t)g]); }))) return rc;
    g_txt_records = (long long)n_rec; g_txt_host = (long long)blob; g_txt_dev = (long long)(total - blob);
    return BM2_OK;
}

bm2h_text_scope::bm2h_text_scope(bm2_ctx *const *ctx, int n) : bm2h_ctx_scope(ctx, n), hook(bm2h_dev_text_batch, &tc) {
    for (int g = 0; g < tc.n; ++g) if (tc.ctx[g]) { tc.ctx[g]->tail_enc = nullptr; tc.ctx[g]->tail_enc_bytes = 0; }
}
bm2h_text_scope::~bm2h_text_scope() {
    for (int g = 0; g < tc.n; ++g) if (tc.ctx[g]) { tc.ctx[g]->tail_enc = nullptr; tc.ctx[g]->tail_enc_bytes = 0; }
}
