// host_tail.h -- seams of the host tail (sam_tail.cpp) the device batches plug into (matesw.hip, cigar.hip)
#pragma once
#include <stdint.h>
#include "../../include/bm2.h"

// The batch of mate-rescue alignments of one chunk, flat: query i = qbuf[q_off[i], +q_len[i]) (the mate, already oriented), target i
// = ref_string[t_pos[i], +t_len[i]), xtra[i] as mem_matesw builds it.  A hook of this type runs the batch (bm2_ksw_align2
// semantics, out[i] = 7 result fields); 0 = success.  The device kernel plugs in here with ref_string resident in HBM.
typedef int (*bm2h_ksw_batch_fn)(void *user, int32_t n, const uint8_t *qbuf, int64_t qbuf_bytes, const int64_t *q_off, const int32_t *q_len,
                                 const int64_t *t_pos, const int32_t *t_len, const int32_t *xtra, const bm2_opt *opt,
                                 const uint8_t *ref_string, bm2_ksw_result *out);
// The batch of CIGAR alignments of one chunk.  An alignment is a function of the HIT alone -- mem_reg2aln (bwamem.cpp:1732-1766) reads
// qb, qe, rb, re, truesc and w of the hit and the read's bases, derives its band, and retries with doubled bands while the score keeps
// improving -- so the tail numbers the chunk's hits, finds out in a dry run of the pairing flow WHICH hits get printed, and hands
// those to a hook of this type in one call; the hook runs the whole retry loop per hit (the device kernel of cigar.hip, or the host
// code for tests) and returns compact arrays: CIGAR ops of hit i at cigar[cigar_off[i] .. +n_cigar[i]) (n_cigar < 0: the reference
// returns NULL), its MD string NUL-terminated at md[md_off[i]].  0 = success.
#include <vector>
struct bm2h_cg_hit { int64_t rb, re; int32_t read, qb, qe, truesc, w, pad; };
struct bm2h_cg_out {
    std::vector<int32_t> score, nm, n_cigar;
    std::vector<int64_t> cigar_off, md_off;
    std::vector<uint32_t> cigar; std::vector<char> md;
};
typedef int (*bm2h_cigar_batch_fn)(void *user, const bm2_opt *opt, const bm2_reads *reads, int64_t enc_bytes, int32_t n, const bm2h_cg_hit *hits,
                                   bm2h_cg_out *out);
// The text of one chunk from its decided records (bm2_sam_format_dev's arguments after the context; offsets of the records index
// `cigar` / `side`).  Set through bm2h_text_hook for the calling thread; when it is set AND so->flag has BM2_SAM_F_DEVICE_TEXT the last
// pass of bm2h_sam_pe / bm2h_sam_se appends records instead of text and hands them to the hook in one call.  The host-only entry
// points never set it.  0 = success.
typedef int (*bm2h_text_batch_fn)(void *user, const bm2_sam_opt *so, const bm2_reads *reads, const bm2_read_text *txt, int64_t n_rec,
                                  const bm2_samrec_t *recs, const uint32_t *cigar, int64_t n_cigar, const char *side, int64_t side_bytes,
                                  char *out, int64_t cap, int64_t *n_out);
struct bm2h_text_hook {             // scoped: the hook of the calling thread for the bm2h_sam_* call made inside the scope
    bm2h_text_hook(bm2h_text_batch_fn fn, void *user);
    ~bm2h_text_hook();
};
// The device's hook (samfmt.hip) and the scope the _dev entry points open around their bm2h_sam_* call: the hook over their context(s), and
// no context believing that it still holds the reads of an earlier call.
struct bm2_ctx;
struct bm2h_text_ctxs { bm2_ctx *const *ctx; int n; };
struct bm2h_ctx_scope {             // what every scope below holds: the contexts its hook works on (a lone one is kept here, not with the caller)
    bm2_ctx *one; bm2h_text_ctxs tc;
    bm2h_ctx_scope(bm2_ctx *const *ctx, int n) : one(n == 1 ? ctx[0] : nullptr), tc{ n == 1 ? &one : ctx, n } {}
};
int bm2h_dev_text_batch(void *user, const bm2_sam_opt *so, const bm2_reads *reads, const bm2_read_text *txt, int64_t n_rec, const bm2_samrec_t *recs,
                        const uint32_t *cigar, int64_t n_cigar, const char *side, int64_t side_bytes, char *out, int64_t cap, int64_t *n_out);
struct bm2h_text_scope : bm2h_ctx_scope {
    bm2h_text_hook hook;
    bm2h_text_scope(bm2_ctx *const *ctx, int n);
    ~bm2h_text_scope();
};
// The pairing decisions of one chunk (bm2_pe_decide_dev's arguments after the context).  Set through bm2h_decide_hook for the calling
// thread; when it is set AND so->flag has BM2_SAM_F_DEVICE_DECIDE, the CIGAR session of bm2h_sam_pe applies the rescue results on the
// host threads, gathers every pair's lists into one array, calls the hook once and puts the lists back.  0 = success.
typedef int (*bm2h_decide_batch_fn)(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, bm2_alnreg_t *hits,
                                    const int64_t *hit_off, int64_t first_pair, const bm2_pestat pes[4], bm2_pairplan_t *plans);
int bm2h_check_hit_off(const char *who, int32_t n_pairs, const int64_t *hit_off);       // non-negative, non-decreasing, every list below 2^30 hits
// the n_lists + 1 offsets counted from the first list's (what a batch that starts anywhere in hit_off uploads)
inline std::vector<int64_t> bm2h_hit_off_from0(const int64_t *hit_off, int64_t n_lists) {
    std::vector<int64_t> hoff((size_t)n_lists + 1);
    for (int64_t i = 0; i <= n_lists; ++i) hoff[(size_t)i] = hit_off[i] - hit_off[0];
    return hoff;
}
struct bm2h_decide_hook {
    bm2h_decide_hook(bm2h_decide_batch_fn fn, void *user);
    ~bm2h_decide_hook();
};
// The device's hook (decide.hip; user = bm2h_text_ctxs: the pairs are cut into contiguous parts, one context and host thread per part)
// and the scope the _dev entry points of the paired tail open around their bm2h_sam_pe call.
int bm2h_dev_decide_batch(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, bm2_alnreg_t *hits,
                          const int64_t *hit_off, int64_t first_pair, const bm2_pestat pes[4], bm2_pairplan_t *plans);
struct bm2h_decide_scope : bm2h_ctx_scope {
    bm2h_decide_hook hook;
    bm2h_decide_scope(bm2_ctx *const *ctx, int n);
};
// The rescue results of one chunk applied to its lists (bm2_pe_rescue_apply_dev's arguments after the context, with the results of the
// rescue batch beside the tasks: res[t] belongs to tasks[t]; out_cap >= hits + tasks).  Set through bm2h_rescue_hook for the calling
// thread; when it is set AND so->flag has BM2_SAM_F_DEVICE_RESCUE, bm2h_sam_pe calls it once with the chunk's alnregs, numbers its hits
// through it (pad = index + 1) and walks only the redo pairs on the host.  0 = success.
typedef int (*bm2h_rescue_batch_fn)(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits,
                                    const int64_t *hit_off, const int32_t *read_len, const bm2_pestat pes[4], const bm2_rescue_task_t *tasks,
                                    const bm2_ksw_result *res, const int64_t *task_off, bm2_alnreg_t *out, int64_t out_cap, int64_t *out_off,
                                    int32_t *redo, int64_t first_pair, bm2_pairplan_t *plans);
struct bm2h_rescue_hook {
    bm2h_rescue_hook(bm2h_rescue_batch_fn fn, void *user);
    ~bm2h_rescue_hook();
};
// grouped by pair, strictly ascending in (end, j, r), end / j / r in range for the pair's lists (bm2h_check_hit_off has passed)
int bm2h_check_rescue_tasks(const char *who, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits, const int64_t *hit_off,
                            const bm2_rescue_task_t *tasks, const int64_t *task_off);
void bm2h_rescue_stats_reset();
void bm2h_rescue_stats_add(long long pairs, long long tasks, long long added, long long redone);
// The device's hook (rescue.hip; user = bm2h_text_ctxs: contiguous parts of the pairs, one context and host thread per part) and its scope
int bm2h_dev_rescue_apply_batch(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits,
                                const int64_t *hit_off, const int32_t *read_len, const bm2_pestat pes[4], const bm2_rescue_task_t *tasks,
                                const bm2_ksw_result *res, const int64_t *task_off, bm2_alnreg_t *out, int64_t out_cap, int64_t *out_off,
                                int32_t *redo, int64_t first_pair, bm2_pairplan_t *plans);
// plans != NULL (BM2_SAM_F_DEVICE_DECIDE as well): the pairs' decisions are taken on the grown lists where they lie in HBM (decide.hip's
// kernels, packed and permuted on the device) and `out` receives the DECIDED lists; the lists cross the bus once each way.  A redo pair's
// lists and plan are then of no use: the caller rescues and decides it from its input.
int bm2h_decide_resident(bm2_ctx *c, const char *who, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *d_hits,
                         const int64_t *d_off, const int64_t *h_off, int64_t first_pair, const bm2_pestat pes[4], bm2_pairplan_t *plans, bm2_alnreg_t *out);
void bm2h_decide_stats_reset();
struct bm2h_rescue_scope : bm2h_ctx_scope {
    bm2h_rescue_hook hook;
    bm2h_rescue_scope(bm2_ctx *const *ctx, int n);
};
// The plan of one chunk's mate rescue (bm2_pe_rescue_plan_dev's arguments after the context; the tasks go to what room(arg, n) answers
// once their number is known, task_off[n_pairs + 1] and *n_out are filled), and the rescue batch with its queries made where it runs:
// the flat arrays of bm2h_ksw_batch_fn without qbuf -- query i is the mate of tasks[i] as its direction reads it, q_off[n] = their bytes.
// Set through bm2h_plan_hook for the calling thread; when they are set AND so->flag has BM2_SAM_F_DEVICE_PLAN, bm2h_sam_pe walks no pair
// to plan and copies no mate: it sizes its lists from the tasks and describes the batch from task fields and read lengths.  0 = success.
typedef int (*bm2h_plan_batch_fn)(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits, const int64_t *hit_off,
                                  const int32_t *read_len, const bm2_pestat pes[4], bm2_rescue_task_t *(*room)(void *arg, int64_t n), void *arg,
                                  int64_t *task_off, int64_t *n_out);
typedef int (*bm2h_ksw_resident_fn)(void *user, int32_t n, const bm2_rescue_task_t *tasks, const bm2_reads *reads, const int64_t *q_off, const int32_t *q_len,
                                    const int64_t *t_pos, const int32_t *t_len, const int32_t *xtra, const bm2_opt *opt, bm2_ksw_result *out);
struct bm2h_plan_hook {
    bm2h_plan_hook(bm2h_plan_batch_fn fn, bm2h_ksw_resident_fn qfn, void *user);
    ~bm2h_plan_hook();
};
int bm2h_plan_query_offsets(const char *who, const bm2_reads *reads, int64_t n_tasks, const bm2_rescue_task_t *tasks, const uint8_t *out, int64_t cap,
                            int64_t *q_off, int64_t *n_out);
void bm2h_plan_stats_set(long long pairs, long long tasks, long long query_bytes);
void bm2h_plan_stats_add_query_bytes(long long query_bytes);
// The device's hooks (plan.hip, matesw.hip; user = bm2h_text_ctxs: contiguous parts of the pairs / of the tasks, one context and host
// thread per part) and their scope.  bm2h_plan_queries_resident: the queries of tasks [0, n) into d_out (device memory) at
// q_off[t] - q_off[0], from the run of the reads' codes that holds their mates, uploaded here; asynchronous on the context's stream.
int bm2h_dev_plan_batch(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits, const int64_t *hit_off,
                        const int32_t *read_len, const bm2_pestat pes[4], bm2_rescue_task_t *(*room)(void *arg, int64_t n), void *arg,
                        int64_t *task_off, int64_t *n_out);
int bm2h_dev_rescue_batch_resident(void *user, int32_t n, const bm2_rescue_task_t *tasks, const bm2_reads *reads, const int64_t *q_off, const int32_t *q_len,
                                   const int64_t *t_pos, const int32_t *t_len, const int32_t *xtra, const bm2_opt *opt, bm2_ksw_result *out);
int bm2h_plan_queries_resident(bm2_ctx *c, const bm2_reads *reads, int64_t n, const bm2_rescue_task_t *tasks, const int64_t *q_off, uint8_t *d_out);
struct bm2h_plan_scope : bm2h_ctx_scope {
    bm2h_plan_hook hook;
    bm2h_plan_scope(bm2_ctx *const *ctx, int n);
};
// The contiguous parts a chunk's pairs are cut into by the hooks that read its hit lists (the plan's and the model's: the same parts, so
// that what one of them uploads serves the other): knob BM2_PLAN_PART = pairs that are worth a context of their own, at most n_ctx parts;
// part g = pairs [n_pairs * g / G, n_pairs * (g + 1) / G).
int bm2h_plan_parts(int64_t n_pairs, int n_ctx);
// The insert-size model of one chunk (bm2_pe_stat_dev's arguments after the context, without the histogram).  Set through
// bm2h_pestat_hook for the calling thread; when it is set AND so->flag has BM2_SAM_F_DEVICE_PESTAT AND the caller gave no model,
// bm2h_sam_pe takes pes[4] from the hook instead of counting the pairs on its threads.  0 = success.
typedef int (*bm2h_pestat_batch_fn)(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits, const int64_t *hit_off,
                                    bm2_pestat pes[4]);
struct bm2h_pestat_hook {
    bm2h_pestat_hook(bm2h_pestat_batch_fn fn, void *user);
    ~bm2h_pestat_hook();
};
// pestat_model of sam_tail.cpp behind a name: the four models read off the merged histogram hist[4][top + 1] (top = max(max_ins, 0))
void bm2h_pestat_model(const uint32_t *hist, int64_t top, bm2_pestat pes[4]);
void bm2h_pestat_stats_set(long long pairs, long long counted, long long hit_bytes_up);       // (and no byte shared)
void bm2h_pestat_stats_shared(long long hit_bytes, bool add);                                 // add = false: set
// The number of the bm2h_sam_pe call in progress on this thread that took its model from the hook (0: none).  What the model's hook
// leaves in a context's b_pl_in is tagged with it, and only the plan hook of the same call may find it there.
uint64_t bm2h_tail_epoch();
// The device's hook (pestat.hip; user = bm2h_text_ctxs: the parts of bm2h_plan_parts, one context and host thread per part, their
// histograms summed on the host) and its scope, which also forgets what the contexts hold in b_pl_in when the call ends.
int bm2h_dev_pestat_batch(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits, const int64_t *hit_off,
                          bm2_pestat pes[4]);
struct bm2h_pestat_scope : bm2h_ctx_scope {
    bm2h_pestat_hook hook;
    bm2h_pestat_scope(bm2_ctx *const *ctx, int n);
    ~bm2h_pestat_scope();
};
// The hits of one chunk whose CIGARs the text will ask for (bm2_cigar_plan_dev's arguments after the context, with the hits packed to the
// 16 bytes the rule reads: hits[k] is hit hit_off[0] + k, and sel speaks hit_off's numbering).  Set through bm2h_cgplan_hook for the calling
// thread; when it is set AND so->flag has BM2_SAM_F_DEVICE_CGPLAN, the CIGAR session of bm2h_sam_pe / bm2h_sam_se runs no dry emit: it packs
// the decided lists on its threads, calls the hook once and fills its batch from sel.  0 = success.
struct bm2h_cg_mark { int32_t score, secondary, secondary_all, is_alt; };      // 16 B
typedef int (*bm2h_cgplan_batch_fn)(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_lists, const bm2h_cg_mark *hits,
                                    const int64_t *hit_off, const bm2_pairplan_t *plans, int32_t *sel, int64_t cap, int64_t *n_out);
struct bm2h_cgplan_hook {
    bm2h_cgplan_hook(bm2h_cgplan_batch_fn fn, void *user);
    ~bm2h_cgplan_hook();
};
int bm2h_check_list_off(const char *who, int64_t n_lists, const int64_t *hit_off);      // bm2h_check_hit_off over any number of lists
void bm2h_cgplan_stats_set(long long lists, long long hits, long long selected, long long heavy);
// The device's hook (cgplan.hip; user = bm2h_text_ctxs: the lists cut into contiguous parts at pair boundaries, one context and host thread
// per part, the parts' selections appended in order) and its scope.
int bm2h_dev_cgplan_batch(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_lists, const bm2h_cg_mark *hits,
                          const int64_t *hit_off, const bm2_pairplan_t *plans, int32_t *sel, int64_t cap, int64_t *n_out);
struct bm2h_cgplan_scope : bm2h_ctx_scope {
    bm2h_cgplan_hook hook;
    bm2h_cgplan_scope(bm2_ctx *const *ctx, int n);
};
// cgplan.hip's kernels on single-end lists whose packed hits lie in HBM in decided order (semark.hip's kernels left them): d_hits[k] = hit
// h_off[0] + k, d_off = the n_lists + 1 offsets from 0 on the device, h_off = their host copy in the caller's numbering, which sel speaks.
// Nothing is uploaded but the heavy list.  *heavy = lists that took the wavefront form; first_list names a list in a message.
int bm2h_cgplan_resident(bm2_ctx *c, const char *who, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_lists, const bm2h_cg_mark *d_hits,
                         const int64_t *d_off, const int64_t *h_off, int32_t *sel, int64_t cap, int64_t *n_out, int64_t *heavy, int64_t first_list);
// The `decide` phase of the single-end tail for one chunk (bm2_se_mark_dev's arguments after the context), and with n_out != NULL the CIGAR
// plan of the marked lists as well (sel, cap, *n_out as for bm2h_cgplan_batch_fn; sel speaks hit_off's numbering AFTER the lists have been
// reordered).  Set through bm2h_semark_hook for the calling thread; when it is set AND so->flag has BM2_SAM_F_DEVICE_SEMARK, the CIGAR session
// of bm2h_sam_se marks no read on its threads: it calls the hook once on alnregs / reg_off / n_processed -- with n_out when
// BM2_SAM_F_DEVICE_CGPLAN is set too, and then packs nothing either.  0 = success.
typedef int (*bm2h_semark_batch_fn)(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_lists, bm2_alnreg_t *hits, const int64_t *hit_off,
                                    int64_t first_id, int32_t *n_pri, int32_t *sel, int64_t cap, int64_t *n_out);
struct bm2h_semark_hook {
    bm2h_semark_hook(bm2h_semark_batch_fn fn, void *user);
    ~bm2h_semark_hook();
};
// The device's hook (semark.hip; user = bm2h_text_ctxs: the lists cut into contiguous parts, knob BM2_SEMARK_PART, one context and host
// thread per part, part g's ids from first_id + its first list, the parts' selections appended in order) and its scope.
int bm2h_dev_semark_batch(void *user, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_lists, bm2_alnreg_t *hits, const int64_t *hit_off,
                          int64_t first_id, int32_t *n_pri, int32_t *sel, int64_t cap, int64_t *n_out);
struct bm2h_semark_scope : bm2h_ctx_scope {
    bm2h_semark_hook hook;
    bm2h_semark_scope(bm2_ctx *const *ctx, int n);
};
// The CIGAR batch prepared where it runs (BM2_SAM_F_DEVICE_CGPREP; cgprep.hip).  Unlike the hooks above this one is no function of the
// calling thread: the CIGAR hook of the _multi forms runs every part of a batch on a host thread of its own, one context per part, so
// the scope sets a field on each of its contexts (bm2_ctx::cgprep) for the duration of the call and bm2_dev_cigar_batch reads it from
// the context it was given.  What the scope leaves with the calling thread is only the fact that contexts exist, for bm2h_sam_pe /
// bm2h_sam_se to refuse the bit without one.
struct bm2h_cgprep_mark {
    explicit bm2h_cgprep_mark(bool on);
    ~bm2h_cgprep_mark();
};
struct bm2h_cgprep_scope : bm2h_ctx_scope {
    bm2h_cgprep_mark mark;
    bm2h_cgprep_scope(bm2_ctx *const *ctx, int n, const bm2_sam_opt *so);
    ~bm2h_cgprep_scope();
};
void bm2h_cgprep_stats_reset();
void bm2h_cgprep_stats_add(const bm2_cigar_prep_t *tot, long long bytes_up, long long fallbacks);
// bm2_sam_pe / bm2_sam_se with the rescue batch routed through `fn` and the CIGAR batch through `cfn` (NULL: host code in place)
int bm2h_sam_pe(const bm2_index_desc *idx, const bm2_opt *opt, const bm2_sam_opt *so, const bm2_reads *reads, const bm2_read_text *txt,
                const bm2_alnreg_t *alnregs, const int64_t *reg_off, int64_t n_processed, const bm2_pestat *pes_in, bm2_pestat *pes_out,
                char *out, int64_t cap, int64_t *n_out, bm2h_ksw_batch_fn fn, void *user, bm2h_cigar_batch_fn cfn, void *cuser);
int bm2h_sam_se(const bm2_index_desc *idx, const bm2_opt *opt, const bm2_sam_opt *so, const bm2_reads *reads, const bm2_read_text *txt,
                bm2_alnreg_t *alnregs, const int64_t *reg_off, int64_t n_processed, char *out, int64_t cap, int64_t *n_out,
                bm2h_cigar_batch_fn cfn, void *cuser);

// Phase clock of the tail (BM2_TAIL_PROF=1 prints the phases of every call to stderr): where the host time of a chunk goes.
#include <chrono>
#include <stdio.h>
#include <stdlib.h>
struct TailProf {
    bool on; const char *who; std::chrono::steady_clock::time_point t0, t;
    explicit TailProf(const char *w) : on(getenv("BM2_TAIL_PROF") != nullptr), who(w) { t0 = t = std::chrono::steady_clock::now(); }
    void mark(const char *what) {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "[tail] %-14s %-22s %8.1f ms\n", who, what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
    ~TailProf() { if (on) fprintf(stderr, "[tail] %-14s %-22s %8.1f ms\n", who, "TOTAL", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); }
};

// ---- the CIGAR batch's preparation (cigar_prep.h states the rule).  Host side, cigar_prep.cpp: the three launch knobs as the process
// reads them; what both record-level forms refuse before they look at a task (who = the entry point; self = its context, or anything
// non-NULL); and slices, order and totals of tasks whose q_off .. re and q_len .. retry are set (prof: the phases `slices` and `order`).
// Device side, cgprep.hip: bm2h_cgprep_dev writes tasks and order of the batch into DEVICE memory (d_task, d_order: n entries each, not
// in the b_cp_* workspaces) and brings the totals down, one synchronising copy.  hits: the host array, uploaded here -- or d_hits != NULL:
// the hits lie in device memory already and nothing but the reads' offsets and lengths goes up.  *bytes_up = what went up.
#include "cigar_prep.h"
struct CgpKnobs { int no_lds, no_ring, ring_by_band; };
CgpKnobs bm2h_cigar_prep_knobs();
int bm2h_cigar_prep_args(const char *who, const void *self, const bm2_opt *opt, const bm2_reads *reads, int32_t n, const void *hits, const void *tasks,
                         const void *order, const void *tot);
int bm2h_cigar_prep_tasks(const char *who, const CgpPrm &P, int32_t n, bm2_cigar_task_t *tasks, int32_t *order, bm2_cigar_prep_t *tot, TailProf *prof);
int bm2h_cgprep_dev(bm2_ctx *c, const char *who, const CgpPrm &P, const bm2_reads *reads, int32_t n, const bm2_cigar_hit_t *hits, const bm2_cigar_hit_t *d_hits,
                    bm2_cigar_task_t *d_task, int32_t *d_order, bm2_cigar_prep_t *tot, int64_t *bytes_up);
