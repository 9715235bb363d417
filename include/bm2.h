/* include/bm2.h -- C ABI of the MI355X seed -> chain -> extend library (libbm2.so).
 *
 * bwa-mem2 has no plugin/FFI interface; the seams this library replaces are ordinary C++
 * calls inside libbwa.  Every entry point below names the reference
 * interface it stands in for (paths relative to the reference's src/).  Plain pointers and
 * sizes only; no C++ or torch types.  All functions return 0 on success or a negative
 * BM2_E* code (the reference exit()s or assert()s instead); outputs are caller-allocated
 * with a capacity and an n_out so the caller can grow and retry (the reference reallocs
 * inside the callee, e.g. bwamem.cpp:718-739).  One bm2_ctx per GPU, used from one host
 * thread at a time.  There is NO CPU fallback: without a usable HIP device every call
 * fails with BM2_ENODEV.
 */
#ifndef BM2_H
#define BM2_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BM2_OK        0
#define BM2_ENODEV   -1   /* no HIP device / HIP runtime error (message: bm2_last_error) */
#define BM2_ENOMEM   -2   /* host or device allocation failed */
#define BM2_EINVAL   -3   /* bad argument */
#define BM2_ECAP     -4   /* caller-provided output too small; *n_out holds the needed count */
#define BM2_EUNSUP   -5   /* a path of the reference that is not implemented (stated in DESIGN.md) */
#define BM2_EIO      -6   /* index file missing / malformed */

typedef struct bm2_ctx bm2_ctx;

/* ---- index ---------------------------------------------------------------------------------
 * The arrays FMI_search::load_index (FMI_search.cpp:384-494) and main_mem (fastmap.cpp:860-888)
 * read from <prefix>.bwt.2bit.64 / .0123 / .ann / .alt, as host pointers.  `count` is the
 * on-disk cumulative count (the +1 of FMI_search.cpp:433-436 is applied inside the library). */
typedef struct {
    int64_t ref_len;                /* reference_seq_len = 2*l_pac + 1 */
    int64_t count[5];
    int64_t sentinel_index;
    const void     *cp_occ;         /* (ref_len>>6)+1 CP_OCC blocks of 64 B (FMI_search.h:54-58) */
    const int8_t   *sa_ms_byte;     /* (ref_len>>3)+1 */
    const uint32_t *sa_ls_word;     /* (ref_len>>3)+1 */
    const uint8_t  *ref_string;     /* 2*l_pac bytes, values 0..3 (.0123); the device copy holds four per byte (a value above 3 anywhere keeps bytes) */
    int64_t l_pac;
    int32_t n_seqs;
    const int64_t *ann_offset;      /* bntann1_t.offset, .len, .is_alt (bntseq.h:42-49) */
    const int32_t *ann_len;
    const int32_t *ann_is_alt;
    const char *const *ann_name;    /* bntann1_t.name / .anno: only the SAM writer reads them (may be NULL otherwise) */
    const char *const *ann_anno;
} bm2_index_desc;

/* Read the reference's index files into malloc'd host arrays (stands in for
 * FMI_search::load_index + bwa_idx_load_ele + the .0123 fread).  Free with bm2_index_free. */
int  bm2_index_load(const char *prefix, bm2_index_desc *out);
/* Build <prefix>.pac/.ann/.amb/.0123/.bwt.2bit.64 from a plain FASTA, byte-identical to `bwa-mem2 index`
 * (bns_fasta2bntseq bntseq.cpp:249-357; FMI_search::build_index FMI_search.cpp:306-382) but on n_threads host cores
 * (n_threads <= 0: all).  The <prefix>.alt list, if any, is the caller's to provide, as with the reference. */
int  bm2_index_build(const char *fasta, const char *prefix, int n_threads);
void bm2_index_free(bm2_index_desc *d);

/* ---- options: the fields of mem_opt_t (bwamem.h:76-108) the hot path reads ------------------ */
typedef struct {
    int32_t a, b, o_del, e_del, o_ins, e_ins, pen_clip5, pen_clip3, w, zdrop;
    int32_t min_seed_len, split_width, max_occ, max_chain_gap, min_chain_weight, max_chain_extend;
    int64_t max_mem_intv;
    float   split_factor, mask_level, drop_ratio, mask_level_redun;
    int8_t  mat[25];                /* bwa_fill_scmat (bwa.cpp:248-257) */
    int8_t  pad[3];
} bm2_opt;
void bm2_opt_init(bm2_opt *o);      /* mem_opt_init defaults, bwamem.cpp:107-143 */
void bm2_opt_fill_scmat(bm2_opt *o);

/* ---- records (byte-compatible with the reference where a reference struct exists) ----------- */
typedef struct {                    /* SMEM, FMI_search.h:75-83 (40 B) */
    uint32_t rid, m, n, pad;
    int64_t  k, l, s;
} bm2_smem_t;

typedef struct {                    /* SeqPair, bandedSWA.h:90-99 (56 B) */
    int32_t idr, idq, id, len1, len2, h0;
    int32_t seqid, regid;
    int32_t score, tle, gtle, qle, gscore, max_off;
} bm2_seqpair_t;

typedef struct {                    /* BandedPairWiseSW ctor arguments, bandedSWA.h:118-124 */
    int32_t o_del, e_del, o_ins, e_ins, zdrop, end_bonus, w_match, w_mismatch;
    int8_t  mat[25];
    int8_t  pad[3];
} bm2_sw_params;

typedef struct {                    /* the fields of mem_alnreg_t (bwamem.h:137-160) that mem_kernel2_core has
                                     * written when it reaches bwamem.cpp:1152 (before mem_sort_dedup_patch) */
    int64_t rb, re;
    int32_t qb, qe, rid, score, truesc, w, seedcov, seedlen0;
    float   frac_rep;
    int32_t pad;
} bm2_reg_t;

typedef struct {                    /* mem_alnreg_t (bwamem.h:137-160) without the chain pointer: what mem_kernel2_core returns */
    int64_t rb, re;
    int32_t qb, qe, rid, score, truesc, sub, alt_sc, csub, sub_n, w, seedcov, secondary, secondary_all, seedlen0;
    int32_t n_comp, is_alt;
    float   frac_rep;
    int32_t pad;
    uint64_t hash;
} bm2_alnreg_t;

typedef struct {                    /* reads of one chunk: 2-bit codes (0..3, 4 = N), as after bwamem.cpp:992-1000 */
    int32_t n_reads;
    const uint8_t *enc;             /* concatenated codes */
    const int64_t *off;             /* [n_reads] start of read i in enc */
    const int32_t *len;             /* [n_reads] */
} bm2_reads;

typedef struct {                    /* work counters measured by the kernels themselves */
    int64_t n_reads, n_bases;
    int64_t n_smem, n_sa, n_chain, n_reg_raw, n_reg;
    int64_t n_ext;                  /* backwardExt calls                -> 128 B each */
    int64_t n_lf;                   /* LF steps in the SA walk          ->  64 B each */
    int64_t n_sw_cells;             /* DP cells actually computed */
    int64_t n_sw_tasks;
} bm2_stats;

/* ---- lifetime ---------------------------------------------------------------------------- */
bm2_ctx *bm2_create(int device, const bm2_index_desc *idx);     /* uploads the index replica to HBM */
/* a second context on the same device sharing the parent's index replica (own streams / workspaces): overlap two chunks on one
 * GPU, or split one chunk over several contexts, without another upload.  Valid while the parent lives. */
bm2_ctx *bm2_create_shared(bm2_ctx *parent);
void     bm2_destroy(bm2_ctx *c);
/* the context's main stream at a hardware queue priority (level > 0: highest, < 0: lowest, 0: default): e.g. high for the contexts that
 * run the short device batches of the SAM tail beside another context's seeding .. extension */
int      bm2_set_stream_priority(bm2_ctx *c, int level);
const char *bm2_last_error(void);
int      bm2_device_count(void);
/* the CPUs this process can really use: hardware threads it may run on, capped by its cgroup CPU-time quota (a GPU slice of a shared node
 * sees every hardware thread of the host but is given the time of a few); the default of every n_threads <= 0 in this library */
int      bm2_host_cpus(void);
/* page-locked host memory for a caller's large per-chunk arrays (reads, hits, text): the library's copies from / to it are plain DMA at
 * PCIe speed instead of a staged copy through 16 MB bounce buffers; anything else the caller passes is staged, as before */
/* (hardware queues: the HIP runtime reads GPU_MAX_HW_QUEUES when it starts; libbm2 asks for 16 when it is loaded unless the variable is set.
 * A host that initialises HIP BEFORE loading libbm2 must export GPU_MAX_HW_QUEUES=16 itself, or the concurrent launches of the extension stage
 * share four queues -- about 2 ms per million-read chunk.) */
void    *bm2_host_alloc(int64_t bytes);
void     bm2_host_free(void *p);

/* ---- S1: BandedPairWiseSW::getScores8 / getScores16 / scalarBandedSWAWrapper (bandedSWA.h:126-135,
 * 199-211; call sites bwamem.cpp:2476,2544,2613,2692,2757,2828).  Fills score,tle,gtle,qle,gscore,max_off
 * of every pair; the per-pair band clamp follows the pair's class (int8/int16/scalar), as the reference's
 * three entry points do.  ref/qer are the flat seqBuf arrays indexed by idr/idq. */
int bm2_bsw(bm2_ctx *c, bm2_seqpair_t *pairs, const uint8_t *ref, int64_t ref_bytes, const uint8_t *qer,
            int64_t qer_bytes, int32_t n, int32_t w, const bm2_sw_params *p);
/* The same with the batch resident in HBM (BASELINE.json config 2: the banded-SW kernel alone, timed without the copies): upload once,
 * run any number of times (the kernel writes only the six output fields), download.  kernel_ms = duration of the kernel from HIP
 * events on its stream, cells = DP cells computed (either may be NULL; counting costs an atomic per pair: ask for it in an untimed run). */
int bm2_bsw_upload(bm2_ctx *c, const bm2_seqpair_t *pairs, const uint8_t *ref, int64_t ref_bytes, const uint8_t *qer,
                   int64_t qer_bytes, int32_t n);
int bm2_bsw_run(bm2_ctx *c, int32_t w, const bm2_sw_params *p, float *kernel_ms, int64_t *cells);
int bm2_bsw_download(bm2_ctx *c, bm2_seqpair_t *pairs, int32_t n);

/* ---- S2: mem_collect_smem (bwamem.cpp:626-803) = getSMEMsAllPosOneThread + the pass-2 selection +
 * getSMEMsOnePosOneThread + bwtSeedStrategyAllPosOneThread + sortSMEMs (FMI_search.h:106-165).
 * out is sorted by (rid, m, n); rid is the index of the read in `reads`. */
int bm2_smem(bm2_ctx *c, const bm2_reads *reads, const bm2_opt *opt, bm2_smem_t *out, int64_t cap, int64_t *n_out);

/* ---- S2: FMI_search::get_sa_entries_prefetch (FMI_search.cpp:1257-1375): coordinates of up to max_occ
 * sampled occurrences of each SMEM, in (SMEM, occurrence) order. */
int bm2_sal(bm2_ctx *c, const bm2_smem_t *smems, int64_t n, int32_t max_occ, int64_t *coords, int64_t cap,
            int64_t *n_out);

/* ---- S3: mem_kernel1_core + mem_kernel2_core up to bwamem.cpp:1152 for a whole chunk
 * (worker_bwt / worker_aln over all 512-read blocks, bwamem.cpp:1175-1214).
 * regs of read i = regs[reg_off[i] .. reg_off[i+1]); reg_off has n_reads+1 entries. */
int bm2_seed_chain_extend(bm2_ctx *c, const bm2_reads *reads, const bm2_opt *opt, bm2_reg_t *regs, int64_t cap,
                          int64_t *reg_off, int64_t *n_out, bm2_stats *stats);

/* ---- the tail of mem_kernel2_core (bwamem.cpp:1154-1169) = mem_sort_dedup_patch (bwamem.cpp:292-353, with mem_patch_reg :175-225 ->
 * bwa_gen_cigar2 -> ksw_global2) and the ALT flag, ON THE DEVICE (finish.hip).  Out: exactly the mem_alnreg_v contents the reference
 * hands to worker_sam.  bm2_batch_finish works on the regs the last bm2_batch_run left in HBM; bm2_batch_download_alnregs copies the
 * result (hits of read i = out[aln_off[i] .. aln_off[i+1])); bm2_finish_regs_dev takes the hits of any producer as host arrays
 * (regs grouped by read: reg_off has n_reads+1 entries). */
int bm2_batch_finish(bm2_ctx *c, const bm2_opt *opt);
int bm2_batch_download_alnregs(bm2_ctx *c, bm2_alnreg_t *out, int64_t cap, int64_t *aln_off, int64_t *n_out);
int bm2_finish_regs_dev(bm2_ctx *c, const bm2_opt *opt, const bm2_reads *reads, const bm2_reg_t *regs, const int64_t *reg_off,
                        bm2_alnreg_t *out, int64_t cap, int64_t *out_off, int64_t *n_out);

/* ---- one chunk over several contexts (several GPUs of a node with a replica each, or contexts sharing one replica): the chunk is
 * cut at multiples of 512 reads (the kt_for block, the only cross-read rule of the path: bwamem.cpp:834), the parts run through
 * bm2_batch_upload / run / finish on one host thread per context, and the hits come back in read order -- ready for ONE
 * bm2_sam_pe[_dev] over the whole chunk (mem_pestat is chunk-wide, bwamem.cpp:1375).  No collective.  The result does not depend on
 * n_ctx. */
int bm2_chunk_hits_sharded(bm2_ctx *const *ctxs, int n_ctx, const bm2_reads *reads, const bm2_opt *opt, bm2_alnreg_t *out, int64_t cap,
                           int64_t *aln_off, int64_t *n_out);

/* ---- host side, next row of SURVEY.md 8(f): single-end records of worker_sam (bwamem.cpp:1320-1335) =
 * mem_mark_primary_se (:1420-1465) + mem_reorder_primary5 (:1496-1519) + mem_reg2sam (:1521-1577) with mem_gen_alt
 * (bwamem_extra.cpp:130-183), mem_reg2aln (:1732-1805: mem_approx_mapq_se, bwa_gen_cigar2 -> ksw_global2 with backtrack,
 * NM / MD) and mem_aln2sam (:1592-1730).  Text is byte-identical to the alignment lines `bwa-mem2 mem` prints for
 * single-end input (header lines are the caller's).  Pure host code. */
typedef struct {                    /* the fields of mem_opt_t (bwamem.h:74-110) this tail reads beyond bm2_opt */
    int32_t T;                      /* -T: minimum score to output (30) */
    int32_t flag;                   /* MEM_F_ALL 0x8, MEM_F_NO_MULTI 0x10, MEM_F_REF_HDR 0x100, MEM_F_SOFTCLIP 0x200,
                                     * MEM_F_PRIMARY5 0x800, MEM_F_KEEP_SUPP_MAPQ 0x1000; pairs: MEM_F_NOPAIRING 0x4, MEM_F_NO_RESCUE 0x20 */
    int32_t max_XA_hits, max_XA_hits_alt;   /* 5, 200 */
    float   XA_drop_ratio;          /* 0.80 */
    float   mapQ_coef_len;          /* 50 */
    int32_t mapQ_coef_fac;          /* (int)log(50) = 3: an int in the reference */
    int32_t pen_unpaired;           /* -U, 17 */
    int32_t max_ins;                /* 10000: pairs further apart are ignored by the insert-size statistics */
    int32_t max_matesw;             /* -m, 50: mate-rescue rounds per end */
    int32_t n_threads;              /* host threads for this tail; 0 = all hardware threads (the text does not depend on it) */
    int32_t rescue_inline;          /* 0: the mate-rescue alignments of a chunk are planned up front and run as one batch (the shape the
                                     * device kernel needs); 1: aligned inside the pair loop as mem_sam_pe does.  Same output. */
    const char *rg_id;              /* bwa_rg_id: RG:Z: value, NULL or "" = none */
} bm2_sam_opt;
void bm2_sam_opt_init(bm2_sam_opt *o);                  /* the defaults of mem_opt_init, bwamem.cpp:107-143 */

typedef struct {                    /* what bseq1_t carries besides the bases (kseq) */
    const char *const *name;        /* [n_reads] */
    const char *const *comment;     /* [n_reads] or NULL; an entry may be NULL (only printed with `mem -C`) */
    const char *const *qual;        /* [n_reads] or NULL; an entry may be NULL */
} bm2_read_text;

/* alnregs: the output of bm2_batch_finish / bm2_finish_regs_dev, regs of read i = [reg_off[i], reg_off[i+1]); they are reordered and annotated in
 * place exactly as mem_mark_primary_se does.  n_processed = reads of earlier chunks (it seeds the tie-breaking hash).
 * out/cap: caller's buffer; *n_out = bytes needed.  BM2_ECAP if cap is too small: NOTHING has been written to `out` then (the text is
 * formatted into per-thread buffers first and copied once every block's place is known) -- grow and call again with FRESH alnregs.
 * Process-wide settings: none unless the host asks.  BM2_MALLOC_TUNE=1 in the environment makes the first bm2_sam_* call set glibc's
 * M_TRIM_THRESHOLD / M_MMAP_THRESHOLD / M_TOP_PAD for the whole process (the tail's threads allocate small blocks at a high rate; see
 * sam_tail.cpp) -- the host's own allocations then stop returning memory to the OS as well, which is why it is the host's choice. */
int bm2_sam_se(const bm2_index_desc *idx, const bm2_opt *opt, const bm2_sam_opt *so, const bm2_reads *reads, const bm2_read_text *txt,
               bm2_alnreg_t *alnregs, const int64_t *reg_off, int64_t n_processed, char *out, int64_t cap, int64_t *n_out);

/* Counters of the last bm2_sam_pe call on this process (diagnostic, not synchronised between concurrent calls): rescue alignments
 * planned up front, those the pairs then used, and those a pair asked for that had not been planned (computed in place). */
void bm2_sam_rescue_stats(int64_t *planned, int64_t *used, int64_t *missed);

/* The local Smith-Waterman of mate rescue for a batch of (query, target) pairs: ksw_align2 (ksw.cpp:340-381) = a forward pass
 * (score, target end, query end, second-best score / its target end outside the best's neighbourhood) and, with KSW_XSTART, a
 * reverse pass for the start.  This is the HOST implementation (the SSE2 kernel's striping is observable and kept): the oracle of the
 * device kernel below and the code that aligns the few rescues a pair asks for outside its chunk's batch.  xtra = KSW_X* flags | minimum score, as mem_matesw builds it
 * (bwamem_pair.cpp:205).  out[i] = { score, te, qe, score2, te2, tb, qb }.
 * Refused with BM2_EINVAL before anything is written: a gap extension penalty <= 0 ("bad argument"), a pair with q_len <= 0 or
 * t_len < 0 ("pair <i> has an empty query", the lowest such i).  A byte pass (KSW_XBYTE) that saturates answers score 255 with
 * qe = -1 and no second-best hit; the start pass of KSW_XSTART is then skipped (tb = qb = -1): the reference's is undefined there. */
typedef struct { int32_t score, te, qe, score2, te2, tb, qb; } bm2_ksw_result;
int bm2_ksw_align2(int32_t n, const uint8_t *seqs, const int64_t *q_off, const int32_t *q_len, const int64_t *t_off, const int32_t *t_len,
                   const int32_t *xtra, const int8_t mat[25], int o_del, int e_del, int o_ins, int e_ins, bm2_ksw_result *out);

/* The same on the device (matesw.hip: one task per 16-lane row, the lanes of the reference's SSE2 register).  seq_bytes = size of
 * seqs.  Results identical to bm2_ksw_align2, and the same refusals in the same words under its own name: nothing is launched or
 * written.  Beyond them: BM2_EUNSUP for a batch with a query of more than 448 bases on word lanes or 896 on byte lanes (its rows do not
 * fit the LDS layout). */
int bm2_ksw_align2_dev(bm2_ctx *c, int32_t n, const uint8_t *seqs, int64_t seq_bytes, const int64_t *q_off, const int32_t *q_len,
                       const int64_t *t_off, const int32_t *t_len, const int32_t *xtra, const int8_t mat[25], int o_del, int e_del,
                       int o_ins, int e_ins, bm2_ksw_result *out);

/* The @SQ lines of bwa_print_sam_hdr (bwa.cpp:523-556): one per contig, "\tAH:*" for ALT contigs; followed by hdr_line (the
 * caller's @RG / extra header lines, may be NULL) and a newline, as the reference prints them.  The @PG line carries the
 * command line and stays with the caller.  *n_out = bytes needed (BM2_ECAP when cap is smaller). */
int bm2_sam_header(const bm2_index_desc *idx, const char *hdr_line, char *out, int64_t cap, int64_t *n_out);

/* CIGAR generation for a batch of hits: bwa_gen_cigar2 (bwa.cpp:260-347) = banded global alignment with backtrack of the
 * query against reference [rb, re) (ksw_global2, ksw.cpp:558-668; both reversed first for hits on the reverse strand so that
 * gaps end up leftmost on the forward strand), NM and the MD string.  This is the HOST implementation: the oracle of the device
 * kernel below and the code behind bm2_sam_se / bm2_sam_pe (no GPU) and behind the CIGARs of rescued hits.  Task i: query codes seqs[q_off[i] .. +q_len[i]), reference range [rb[i], re[i]), band w[i].
 * Out: score[i], nm[i], n_cigar[i] (-1 = the reference returns NULL: empty or strand-bridging range), its ops at
 * cigar[cigar_off[i] ..] (BAM encoding len<<4|op) and the NUL-terminated MD at md[md_off[i] ..].  cigar_cap / md_cap are the
 * callers' capacities; BM2_ECAP with the needed sizes in *cigar_need / *md_need otherwise. */
int bm2_gen_cigar(const bm2_index_desc *idx, const bm2_opt *opt, int32_t n, const uint8_t *seqs, const int64_t *q_off, const int32_t *q_len,
                  const int64_t *rb, const int64_t *re, const int32_t *w, int32_t *score, int32_t *nm, int32_t *n_cigar,
                  int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, int64_t *cigar_need,
                  int64_t *md_off, char *md, int64_t md_cap, int64_t *md_need);

/* The same on the device (cigar.hip: one task per lane, targets from the context's resident reference).  The context must have
 * been created with the index; seq_bytes = size of seqs.  Results identical to bm2_gen_cigar. */
int bm2_gen_cigar_dev(bm2_ctx *c, const bm2_opt *opt, int32_t n, const uint8_t *seqs, int64_t seq_bytes, const int64_t *q_off,
                      const int32_t *q_len, const int64_t *rb, const int64_t *re, const int32_t *w, int32_t *score, int32_t *nm,
                      int32_t *n_cigar, int64_t *cigar_off, uint32_t *cigar, int64_t cigar_cap, int64_t *cigar_need,
                      int64_t *md_off, char *md, int64_t md_cap, int64_t *md_need);

/* FASTA / FASTQ text -> packed reads + names / comments / qualities: kseq's record grammar (kseq.h:185-227), trim_readno
 * (bwa.cpp:62-66: a trailing "/<digit>" is cut off the name) and the nst_nt4_table base codes (bwamem.cpp:992-1000).  The
 * arrays are owned by the library until bm2_fastq_free; comment[i] / qual[i] are NULL when the record has none. */
typedef struct {
    int32_t n_reads; int32_t pad; int64_t n_bases;
    uint8_t *enc; int64_t *off; int32_t *len;       /* what bm2_reads points at */
    char **name, **comment, **qual;                  /* what bm2_read_text points at */
    char *arena;                                     /* internal: non-NULL when the strings share one allocation */
} bm2_fastq;
int  bm2_fastq_parse(const char *text, int64_t n_bytes, bm2_fastq *out);
/* The reader of a whole chunk on n_threads host threads (<= 0: all): one file (text2 == NULL) or two files whose records are
 * interleaved 2i, 2i+1 as bseq_read_orig delivers paired input (bwa.cpp:170-216; the shorter file ends the input).  Same result as
 * bm2_fastq_parse on each file; strict four-line FASTQ is scanned in parallel, anything else falls back to the sequential parser. */
int  bm2_fastq_parse_mt(const char *text1, int64_t n1, const char *text2, int64_t n2, int n_threads, bm2_fastq *out);
void bm2_fastq_free(bm2_fastq *f);

/* Paired-end chunks (reads interleaved: 2i, 2i+1): mem_pestat over the chunk (bwamem_pair.cpp:81-148) unless pes_in is
 * given, then per pair mem_sam_pe (:353-551): mate rescue (mem_matesw :150-283 -> ksw_align2, ksw.cpp:340-381), mem_pair
 * (:285-346), mapping qualities, the records of both ends.  alnregs are not modified.  pes_out (optional) receives the four
 * orientation models (FF, FR, RF, RR). */
typedef struct { int32_t low, high, failed, pad; double avg, std; } bm2_pestat;      /* mem_pestat_t, bwamem.h:162-166 */
int bm2_sam_pe(const bm2_index_desc *idx, const bm2_opt *opt, const bm2_sam_opt *so, const bm2_reads *reads, const bm2_read_text *txt,
               const bm2_alnreg_t *alnregs, const int64_t *reg_off, int64_t n_processed, const bm2_pestat *pes_in, bm2_pestat *pes_out,
               char *out, int64_t cap, int64_t *n_out);

/* bm2_sam_pe / bm2_sam_se with the chunk's mate-rescue alignments (PE) and CIGAR alignments run as device batches against the
 * context's resident reference (the context must have been created with this index).  Same output.  bm2_sam_cigar_stats: CIGAR
 * alignments planned by the dry pass / looked up / computed in place by the last call. */
int bm2_sam_se_dev(bm2_ctx *c, const bm2_index_desc *idx, const bm2_opt *opt, const bm2_sam_opt *so, const bm2_reads *reads,
                   const bm2_read_text *txt, bm2_alnreg_t *alnregs, const int64_t *reg_off, int64_t n_processed, char *out, int64_t cap,
                   int64_t *n_out);
void bm2_sam_cigar_stats(int64_t *planned, int64_t *used, int64_t *missed);
int bm2_sam_pe_dev(bm2_ctx *c, const bm2_index_desc *idx, const bm2_opt *opt, const bm2_sam_opt *so, const bm2_reads *reads,
                   const bm2_read_text *txt, const bm2_alnreg_t *alnregs, const int64_t *reg_off, int64_t n_processed,
                   const bm2_pestat *pes_in, bm2_pestat *pes_out, char *out, int64_t cap, int64_t *n_out);
/* The same over SEVERAL contexts (one per GPU, or contexts sharing one replica): the chunk's rescue batch and CIGAR batch are cut into
 * contiguous parts, one context and one host thread per part, results back in task order -- same text whatever n_ctx is.  What a host that
 * shards the hot path with bm2_chunk_hits_sharded calls afterwards, so that the tail's device work shrinks with the number of GPUs too
 * (worker_sam, bwamem.cpp:1366-1381; mem_matesw, bwamem_pair.cpp:150-283). */
int bm2_sam_se_dev_multi(bm2_ctx *const *ctxs, int n_ctx, const bm2_index_desc *idx, const bm2_opt *opt, const bm2_sam_opt *so, const bm2_reads *reads,
                         const bm2_read_text *txt, bm2_alnreg_t *alnregs, const int64_t *reg_off, int64_t n_processed, char *out, int64_t cap,
                         int64_t *n_out);
int bm2_sam_pe_dev_multi(bm2_ctx *const *ctxs, int n_ctx, const bm2_index_desc *idx, const bm2_opt *opt, const bm2_sam_opt *so, const bm2_reads *reads,
                         const bm2_read_text *txt, const bm2_alnreg_t *alnregs, const int64_t *reg_off, int64_t n_processed,
                         const bm2_pestat *pes_in, bm2_pestat *pes_out, char *out, int64_t cap, int64_t *n_out);

/* ---- SAM text on the device (samfmt.hip): mem_aln2sam (bwamem.cpp:1592-1730) for a batch of records whose fields are all DECIDED.
 * bm2_samrec_t is what mem_aln2sam holds in its locals once the mate copies and the flags are through: no host pointers, every
 * variable-length piece with its length, so that the device sizes a line without scanning a string. */
typedef struct {
    int32_t read;                   /* index into reads / txt: QNAME, SEQ, QUAL */
    int32_t flag;                   /* FLAG as printed */
    int32_t rid;                    /* contig of RNAME; < 0: the `*\t0\t0\t*` form (pos, mapq, CIGAR not printed) */
    int32_t mapq;
    int64_t pos;                    /* POS as printed (1-based) */
    int32_t mrid;                   /* contig of RNEXT; < 0: no mate position, `*\t0\t0` */
    int32_t rnext_eq;               /* != 0: RNEXT prints `=` */
    int64_t mpos;                   /* PNEXT as printed */
    int64_t tlen;                   /* TLEN as printed */
    int32_t is_rev;                 /* != 0: SEQ reverse-complemented, QUAL reversed */
    int32_t no_seq;                 /* != 0: SEQ and QUAL print `*\t*` (flag 0x100) */
    int32_t qb, qe;                 /* the stretch [qb, qe) of the read SEQ / QUAL print (hard clips of supplementary lines), read coordinates */
    int64_t cigar_off;              /* ops of this line in `cigar` (S or H already chosen); n_cigar == 0 prints `*` and no NM / MD */
    int32_t n_cigar;
    int32_t n_mc;                   /* ops of the mate's CIGAR (MC:Z:) at mc_off; 0: no MC tag */
    int64_t mc_off;
    int32_t nm;                     /* NM:i: */
    int32_t md_len;                 /* bytes of the MD:Z: value at side[md_off] */
    int64_t md_off;
    int32_t score, sub;             /* AS:i: / XS:i:; negative: not printed */
    int64_t blob_off;               /* pre-formatted bytes appended verbatim before the newline (SA:Z:, pa:f:, XA:Z:, the -C comment, */
    int32_t blob_len;               /* XR:Z:, each with its leading tab), at side[blob_off] */
    int32_t pad;
} bm2_samrec_t;                     /* 128 B */
#ifdef __cplusplus
static_assert(sizeof(bm2_samrec_t) == 128, "bm2_samrec_t is 128 bytes (mirrored by bm2.py)");
#endif
/* n_rec records -> their SAM lines, in order, formatted by k_sam_size / k_sam_write.  cigar: BAM-encoded ops (len << 4 | index into
 * "MIDSH"); side: MD strings and blobs.  Contig names come from the context (uploaded by bm2_create; BM2_EINVAL when its descriptor
 * had none), RG:Z: from so->rg_id, names / qualities from txt, bases from reads.  *n_out = bytes needed; BM2_ECAP when cap is
 * smaller, and then nothing has been written to `out`. */
int bm2_sam_format_dev(bm2_ctx *c, const bm2_sam_opt *so, const bm2_reads *reads, const bm2_read_text *txt,
                       int64_t n_rec, const bm2_samrec_t *recs, const uint32_t *cigar, int64_t n_cigar,
                       const char *side, int64_t side_bytes, char *out, int64_t cap, int64_t *n_out);
/* A library-private bit of bm2_sam_opt.flag (outside the reference's MEM_F_* range): bm2_sam_se_dev / bm2_sam_pe_dev and their _multi
 * forms make records instead of text in their last pass and take the text from bm2_sam_format_dev on the same context(s).  Same
 * bytes.  Off by default.  bm2_sam_se / bm2_sam_pe have no context and answer BM2_EINVAL to it. */
#define BM2_SAM_F_DEVICE_TEXT 0x01000000
/* Counters of the last call on this process that formatted on the device: lines written, bytes the kernel produced, bytes that
 * arrived pre-formatted (the blobs). */
void bm2_sam_text_stats(int64_t *records, int64_t *device_bytes, int64_t *host_bytes);

/* ---- pairing decisions on the device (decide.hip): what mem_sam_pe (bwamem_pair.cpp:353-551) does to a pair's two hit lists AFTER
 * mate rescue and before any text: mem_mark_primary_se on both lists (ids (first_pair + p) << 1 | end), mem_reorder_primary5 under
 * MEM_F_PRIMARY5, mem_pair, q_pe, the two q_se of mem_approx_mapq_se, the sub / secondary = -2 rewrite of the chosen hits and the
 * primary / secondary switch of secondary_all.  Lists 2p and 2p + 1 of pair p are hits[hit_off[2p] .. hit_off[2p + 1]) and
 * hits[hit_off[2p + 1] .. hit_off[2p + 2]); hit_off (2 n_pairs + 1 entries) must be non-negative and non-decreasing, and
 * hit_off[2 n_pairs] is the length of hits (checked before anything follows an offset).  The hits are reordered and annotated IN
 * PLACE, every field travelling with its hit (pad and hash included), as bm2_sam_se documents for its alnregs; plans[p] is the
 * pair's outcome.  bm2_pe_decide is the host code of bm2_sam_pe behind a C name and the oracle of bm2_pe_decide_dev, which takes
 * l_pac and the contig offsets from its context (BM2_EINVAL for a context created without an index) and decides EVERY pair on the
 * device, whatever its list lengths.  No transcendental function runs there: the host tabulates the insert-size term of mem_pair
 * per live orientation over [low, high] with its own libm, per call; the four spans together may not exceed 2^22 entries, nor may a
 * hit's span or seedcov (the arguments of log in mem_approx_mapq_se): BM2_EUNSUP otherwise (the host form has neither limit). */
typedef struct { int32_t z[2], n_pri[2], q_se[2], extra_flag, paired; } bm2_pairplan_t;     /* 32 B */
int bm2_pe_decide(const bm2_index_desc *idx, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, bm2_alnreg_t *hits,
                  const int64_t *hit_off, int64_t first_pair, const bm2_pestat pes[4], bm2_pairplan_t *plans);
int bm2_pe_decide_dev(bm2_ctx *c, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, bm2_alnreg_t *hits,
                      const int64_t *hit_off, int64_t first_pair, const bm2_pestat pes[4], bm2_pairplan_t *plans);
/* A library-private bit of bm2_sam_opt.flag, combinable with BM2_SAM_F_DEVICE_TEXT: bm2_sam_pe_dev and bm2_sam_pe_dev_multi apply the
 * mate-rescue results on the host and then take every pair's decisions from bm2_pe_decide_dev on their context(s) in one batch.
 * Same bytes.  Off by default.  bm2_sam_pe and the single-end entry points answer BM2_EINVAL to it. */
#define BM2_SAM_F_DEVICE_DECIDE 0x02000000
/* What the decide kernels of the last call on this process worked on: pairs, hits, and the pairs that took the wavefront-per-pair
 * form (more than 16 hits in all). */
void bm2_sam_decide_stats(int64_t *pairs, int64_t *hits, int64_t *pairs_heavy);

/* ---- mate-rescue results applied on the device (rescue.hip): what mem_sam_pe's mem_matesw calls (bwamem_pair.cpp:150-283, :371-376)
 * do to a pair's two hit lists once the alignments they ask for are known.  A task is one planned (anchor, direction) alignment:
 * `end` = the read the anchor belongs to (the mate, !end, is the read that is aligned), j = the anchor's rank among that end's
 * candidates (hits within pen_unpaired of the best, at most max_matesw), r = direction 0..3, [rb, re) = the window clamped to the
 * anchor's contig, res = what ksw_align2 answered there for the mate as direction r reads it.
 * bm2_pe_rescue_plan (host; the oracle of bm2_pe_rescue_plan_dev below) lists the tasks of a batch of pairs, judged on the lists as they stand, in (pair, end, j, r) order;
 * tasks of pair p = [task_off[p], task_off[p + 1]); res is zeroed.  *n_out = tasks needed; BM2_ECAP when cap is smaller (task_off is
 * complete even then).  Lists and offsets as for bm2_pe_decide; read_len[2 n_pairs] = the reads' lengths.
 * bm2_pe_rescue_apply (host; the oracle) and bm2_pe_rescue_apply_dev (l_pac and the contigs from the context: BM2_EINVAL for one
 * created without an index) take the same lists and the tasks with their results and write the grown lists to `out`: list i =
 * out[out_off[i], out_off[i + 1]), out_off from 0 with 2 n_pairs + 1 entries; *n_out = hits needed, BM2_ECAP when out_cap is smaller
 * (hits + tasks always suffices).  Per pair the result is what mem_sam_pe's rescue loop leaves: anchors from the lists as they came,
 * end 0 then end 1, directions 0..3, each direction re-judged on the mate's current list, a result inserted in front of the first
 * hit that scores less, mem_sort_dedup_patch (without a query: nothing merges) after every open direction once the anchor has
 * applied one; every field travels with its hit, n_comp = 1 as the de-duplication sets it.  The window of a task is taken from the
 * task.  No alignment runs in either form: when a direction is open, has a valid window and NO task (the mate's list lost the hit
 * that served it at planning time), redo[p] = 1 and the pair's lists are returned as they came -- the caller runs that pair through
 * the aligning code.  A pair without any task is copied through unjudged (the plan gives a pair no task when nothing is open).
 * Tasks must be grouped by pair and strictly ascending in (end, j, r) with end, j, r in range: BM2_EINVAL. */
typedef struct { int32_t pair, j, end, r; int64_t rb, re; bm2_ksw_result res; int32_t pad; } bm2_rescue_task_t;      /* 64 B */
#ifdef __cplusplus
static_assert(sizeof(bm2_rescue_task_t) == 64, "bm2_rescue_task_t is 64 bytes (mirrored by bm2.py)");
#endif
int bm2_pe_rescue_plan(const bm2_index_desc *idx, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits,
                       const int64_t *hit_off, const int32_t *read_len, const bm2_pestat pes[4], bm2_rescue_task_t *tasks, int64_t cap,
                       int64_t *task_off, int64_t *n_out);
int bm2_pe_rescue_apply(const bm2_index_desc *idx, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits,
                        const int64_t *hit_off, const int32_t *read_len, const bm2_pestat pes[4], const bm2_rescue_task_t *tasks,
                        const int64_t *task_off, bm2_alnreg_t *out, int64_t out_cap, int64_t *out_off, int32_t *redo, int64_t *n_out);
int bm2_pe_rescue_apply_dev(bm2_ctx *c, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits,
                            const int64_t *hit_off, const int32_t *read_len, const bm2_pestat pes[4], const bm2_rescue_task_t *tasks,
                            const int64_t *task_off, bm2_alnreg_t *out, int64_t out_cap, int64_t *out_off, int32_t *redo, int64_t *n_out);
/* A library-private bit of bm2_sam_opt.flag, alone or with BM2_SAM_F_DEVICE_DECIDE and / or BM2_SAM_F_DEVICE_TEXT: bm2_sam_pe_dev and
 * bm2_sam_pe_dev_multi hand the rescue batch's results to bm2_pe_rescue_apply_dev's kernels on their context(s) in one call instead
 * of walking the pairs on the host; redo pairs go through the host code.  With BM2_SAM_F_DEVICE_DECIDE as well the grown lists stay
 * on the device, the decide kernels run on them there and the decided lists come down once.  Same bytes.  Off by default.  bm2_sam_pe, the single-end
 * entry points and calls with MEM_F_NO_RESCUE or rescue_inline answer BM2_EINVAL to it. */
#define BM2_SAM_F_DEVICE_RESCUE 0x04000000
/* What the last rescue-apply call on this process (either form, or the tail with the bit) worked on: pairs, tasks, rescued hits
 * inserted into the lists, and the pairs that came back with redo. */
void bm2_sam_rescue_apply_stats(int64_t *pairs, int64_t *tasks, int64_t *hits_added, int64_t *pairs_redone);

/* ---- mate rescue planned on the device (plan.hip).  bm2_pe_rescue_plan_dev takes the arguments of bm2_pe_rescue_plan after the context
 * (l_pac and the contigs from the context: BM2_EINVAL for one created without an index) and keeps its contract to the letter: tasks in
 * (pair, end, j, r) order, j = the anchor's rank among the CANDIDATES (hits with score >= best - pen_unpaired, at most max_matesw), not
 * its index in the list; res and pad zero, so that a task's 64 bytes equal the host's; task_off complete and *n_out = the tasks needed
 * even under BM2_ECAP, when the tasks below cap have been written.
 * bm2_pe_rescue_queries (host: the flatten loop of bm2_sam_pe behind a C name) and bm2_pe_rescue_queries_dev build the oriented queries
 * of a task list: query t = the mate of task t (read 2 * pair + !end of `reads`) as direction r reads it -- a plain copy when
 * (r >> 1) == (r & 1), otherwise reversed with c < 4 ? 3 - c : 4 -- written back to back to `out`; q_off[n_tasks + 1] = where each
 * begins, *n_out = their bytes; BM2_ECAP when cap is smaller (q_off and *n_out are complete, nothing has been written).  Of a task
 * they read pair, end and r (each checked against the reads: BM2_EINVAL). */
int bm2_pe_rescue_plan_dev(bm2_ctx *c, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits,
                           const int64_t *hit_off, const int32_t *read_len, const bm2_pestat pes[4], bm2_rescue_task_t *tasks, int64_t cap,
                           int64_t *task_off, int64_t *n_out);
int bm2_pe_rescue_queries(const bm2_reads *reads, int64_t n_tasks, const bm2_rescue_task_t *tasks, uint8_t *out, int64_t cap, int64_t *q_off,
                          int64_t *n_out);
int bm2_pe_rescue_queries_dev(bm2_ctx *c, const bm2_reads *reads, int64_t n_tasks, const bm2_rescue_task_t *tasks, uint8_t *out, int64_t cap,
                              int64_t *q_off, int64_t *n_out);
/* A library-private bit of bm2_sam_opt.flag, alone or with any of the three bits above: bm2_sam_pe_dev and bm2_sam_pe_dev_multi take the
 * chunk's rescue tasks from bm2_pe_rescue_plan_dev's kernels on their context(s) (hits, offsets and read lengths go up, tasks and
 * task_off come down) and run the rescue batch on queries made on the device from the reads' codes: the host walks no pair to plan and
 * copies no mate.  Same bytes.  Off by default.  bm2_sam_pe, the single-end entry points and calls with MEM_F_NO_RESCUE or rescue_inline
 * answer BM2_EINVAL to it. */
#define BM2_SAM_F_DEVICE_PLAN 0x08000000
/* pairs and tasks of the last bm2_pe_rescue_plan_dev call on this process (or of the last tail with the bit), and the query bytes made
 * since: by that tail's rescue batch, or by a bm2_pe_rescue_queries call of either form (which reports no pairs). */
void bm2_sam_rescue_plan_stats(int64_t *pairs, int64_t *tasks, int64_t *query_bytes);

/* ---- the insert-size model of a batch of pairs (mem_pestat, bwamem_pair.cpp:81-148).  A pair whose ends both have hits, whose best
 * hits are unique enough (cal_sub <= 0.8 * score on either end) and lie on one contig adds one to bin [dir][is] of four histograms when
 * its insert size is in [1, max_ins]; quartiles, the trimmed mean and deviation, the bounds and the `failed` marks are read off the counts.
 * bm2_pe_stat (host; the oracle) and bm2_pe_stat_dev (pestat.hip: the counting on the device, l_pac from the context -- BM2_EINVAL for
 * one created without an index -- the model by the same host code) fill pes[4].  Lists and offsets as for bm2_pe_rescue_plan: hit_off has
 * 2 * n_pairs + 1 entries and may start anywhere.  hist = NULL, or room for 4 * (max(max_ins, 0) + 1) counts, which receives the merged
 * histogram laid out [dir][v]; BM2_ECAP when hist_cap is smaller.  max_ins > 2^24: BM2_EUNSUP.  n_pairs == 0 or max_ins <= 0: four failed
 * models, every count zero. */
int bm2_pe_stat(const bm2_index_desc *idx, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits,
                const int64_t *hit_off, bm2_pestat pes[4], uint32_t *hist, int64_t hist_cap);
int bm2_pe_stat_dev(bm2_ctx *c, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_pairs, const bm2_alnreg_t *hits,
                    const int64_t *hit_off, bm2_pestat pes[4], uint32_t *hist, int64_t hist_cap);
/* A library-private bit of bm2_sam_opt.flag, alone or with any of the four bits above, with or without mate rescue: bm2_sam_pe_dev and
 * bm2_sam_pe_dev_multi called without a model (pes_in == NULL) take the chunk's model from bm2_pe_stat_dev's kernel on their context(s)
 * (hits and offsets go up, four histograms come down).  With BM2_SAM_F_DEVICE_PLAN as well, the plan reads the hits where the model left
 * them and uploads only the read lengths.  With pes_in given there is nothing to compute and the bit does nothing.  Same bytes.  Off by
 * default.  bm2_sam_pe and the single-end entry points answer BM2_EINVAL to it. */
#define BM2_SAM_F_DEVICE_PESTAT 0x10000000
/* of the last bm2_pe_stat_dev call on this process, or of the last tail with the bit: its pairs, the pairs counted into a bin, the bytes
 * of hits it uploaded, and how many bytes of hits the plan of the same tail call found resident and did not send again. */
void bm2_sam_pestat_stats(int64_t *pairs, int64_t *counted, int64_t *hit_bytes_up, int64_t *hit_bytes_shared);

/* ---- the CIGAR batch of a chunk picked without an emit pass (cgplan.hip): WHICH hits the text of decided lists will ask mem_reg2aln
 * for (bwamem.cpp:1732) -- a function of score, secondary, secondary_all and is_alt of the hits and of the pairs' plans, nothing else.
 * plans == NULL: n_lists single-end lists, each judged as mem_reg2sam judges it (bwamem.cpp:1521-1577, with mem_gen_alt unless
 * MEM_F_ALL).  plans != NULL: n_lists is even (BM2_EINVAL otherwise) and lists 2p, 2p + 1 are judged under plans[p] as the emit half of
 * mem_sam_pe does (bwamem_pair.cpp:487-551): paired -> mem_gen_alt, hit z[i], and hit n_pri[i] when it is a primary ALT hit at or
 * above T; not paired -> the mate's representative (hit 0 at or above T, else hit n_pri[i] at or above T) and mem_reg2sam.  hit_off
 * (n_lists + 1 entries) as for bm2_pe_decide; it may start anywhere.  sel receives, ascending, the indices into `hits` (hit_off's
 * numbering) of the hits asked for, each once; *n_out = their number, BM2_ECAP when cap is smaller (*n_out is complete, nothing is
 * written at or above cap).  The XA comparison is done in double and the drop_ratio one in float, one operation each, as the host
 * compiles them.  A secondary (other than INT_MAX) or secondary_all at or beyond its list's length, an n_pri outside [0, n] or, for
 * a paired pair, a z outside [0, n) is BM2_EINVAL: detected, never followed.  bm2_cigar_plan is the host statement of the rule and
 * the oracle; bm2_cigar_plan_dev marks and compacts on the device, reads nothing of an index (a context created without one will do)
 * and handles every list there, whatever its length. */
int bm2_cigar_plan(const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_lists, const bm2_alnreg_t *hits, const int64_t *hit_off,
                   const bm2_pairplan_t *plans, int32_t *sel, int64_t cap, int64_t *n_out);
int bm2_cigar_plan_dev(bm2_ctx *c, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_lists, const bm2_alnreg_t *hits,
                       const int64_t *hit_off, const bm2_pairplan_t *plans, int32_t *sel, int64_t cap, int64_t *n_out);
/* A library-private bit of bm2_sam_opt.flag, alone or with any of the five bits above: the CIGAR session of bm2_sam_pe_dev,
 * bm2_sam_se_dev and their _multi forms runs no dry emit pass; the decided lists (16 B a hit) and the plans go through
 * bm2_cigar_plan_dev's kernels on their context(s) once and the batch is made from what comes back.  Same bytes, same
 * bm2_sam_cigar_stats.  Off by default.  bm2_sam_se / bm2_sam_pe have no context and answer BM2_EINVAL to it. */
#define BM2_SAM_F_DEVICE_CGPLAN 0x20000000
/* of the last bm2_cigar_plan_dev call on this process, or of the last tail with the bit: lists, hits, hits selected, and the lists
 * (single-end) or pairs that took the wavefront form (more than 16 hits). */
void bm2_sam_cigar_plan_stats(int64_t *lists, int64_t *hits, int64_t *selected, int64_t *lists_heavy);

/* ---- the `decide` phase of the single-end tail for a batch of hit lists (semark.hip): which hits of a read are primary.  List i is
 * hits[hit_off[i], hit_off[i + 1]), n_lists + 1 offsets, checked (non-negative, non-decreasing: BM2_EINVAL) before anything follows one;
 * hit_off[0] need not be 0.  The id of list i is first_id + i: it seeds hash_64(id + k) of hit k, the tie-break of both rankings, as
 * bm2_sam_se does with n_processed + i.  Per list: mem_mark_primary_se (bwamem.cpp:1392-1465), then mem_reorder_primary5 (:1496-1519)
 * with so->T when so->flag has MEM_F_PRIMARY5.  The hits are reordered and annotated IN PLACE: sub, alt_sc, secondary, secondary_all and
 * hash are set, sub_n is incremented (not reset), and every other field travels with its hit, pad included.  n_pri[i] = the hits of
 * list i on the primary assembly (not on an ALT contig); n_pri may be NULL.  n_lists == 0 is a success that touches nothing.
 * bm2_se_mark is the host code of bm2_sam_se's decide step behind a C name, and the oracle; bm2_se_mark_dev reads nothing of an index (a
 * context created without one will do) and marks EVERY list on the device, whatever its length: 20 B a hit go up, 32 B a hit come down. */
int bm2_se_mark(const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_lists, bm2_alnreg_t *hits, const int64_t *hit_off, int64_t first_id,
                int32_t *n_pri);
int bm2_se_mark_dev(bm2_ctx *c, const bm2_opt *opt, const bm2_sam_opt *so, int32_t n_lists, bm2_alnreg_t *hits, const int64_t *hit_off,
                    int64_t first_id, int32_t *n_pri);
/* A library-private bit of bm2_sam_opt.flag, alone or with BM2_SAM_F_DEVICE_CGPLAN and / or BM2_SAM_F_DEVICE_TEXT: the CIGAR session of
 * bm2_sam_se_dev and bm2_sam_se_dev_multi marks no read on the host threads; the chunk's lists go through bm2_se_mark_dev's kernels on
 * their context(s) in one call.  With BM2_SAM_F_DEVICE_CGPLAN as well the marked lists stay on the device, the plan's kernels read them
 * there, and the host packs nothing for the plan.  Same bytes, same bm2_sam_cigar_stats.  Off by default.  bm2_sam_se has no context and
 * answers BM2_EINVAL to it; so do bm2_sam_pe and its _dev forms (a flag of the single-end tail). */
#define BM2_SAM_F_DEVICE_SEMARK 0x40000000
/* of the last bm2_se_mark_dev call on this process, or of the last tail with the bit: lists, hits, and the lists that took the
 * wavefront form (more than 16 hits). */
void bm2_sam_se_mark_stats(int64_t *lists, int64_t *hits, int64_t *lists_heavy);

/* ---- the CIGAR batch of a chunk prepared for its kernels (cigar_prep.h states the rule; cgprep.hip is its device form): every hit
 * becomes a task with its slices of the four scratch buffers (direction bytes, the global row of (H, E), CIGAR ops, MD bytes), and the
 * batch is ordered by shape and cost class.  Of `reads` only n_reads, off and len are read (enc may be NULL); l_pac is an argument, so a
 * context created without an index will do.  tasks[i] is task i: q_off = reads->off[read] + qb, q_len = qe - qb, and its four slices laid
 * out in task order from 0 (every z_off a multiple of 4).  order = the tasks by class key, ascending, tasks of one key in ascending
 * index; the keys run RING, ROW, GLOBAL, FLAT, the costliest class of a shape first.  tot = the four totals, the tasks of each shape
 * and qmax, the longest q_len among RING and ROW tasks.  The launch knobs BM2_CIGAR_NO_LDS, BM2_CIGAR_NO_RING and
 * BM2_CIGAR_RING_BY_BAND are read on the host by both forms.  n == 0 succeeds and touches nothing.  A NULL argument, n < 0, or a gap
 * extension penalty <= 0 is BM2_EINVAL; a scoring matrix not of the bwa_fill_scmat form is BM2_EUNSUP; a `read` outside [0, n_reads) or
 * 0 <= qb <= qe <= len[read] not holding is BM2_EINVAL naming the lowest offending task (detected, never followed); a valid reference
 * range longer than 0x3fffffff is BM2_EINVAL.  bm2_cigar_prep is the host statement and the oracle.  bm2_cigar_prep_dev carries the
 * per-task sizes as 32-bit values: a task one of whose slices reaches 2^31 (a DP area of 2^31 bytes) is BM2_EUNSUP there. */
typedef struct { int64_t rb, re; int32_t read, qb, qe, truesc, w, retry; } bm2_cigar_hit_t;          /* 40 B; retry != 0: mem_reg2aln's retry loop runs around the alignment, w is the hit's band */
typedef struct { int64_t q_off, rb, re, z_off, eh_off, cg_off, md_off;
                 int32_t q_len, w, truesc, retry; } bm2_cigar_task_t;                               /* 72 B */
typedef struct { int64_t z_bytes, eh_items, cg_items, md_bytes;
                 int32_t n_shape[4]; int32_t qmax, pad; } bm2_cigar_prep_t;                         /* 56 B; n_shape in order RING, ROW, GLOBAL, FLAT */
int bm2_cigar_prep    (const bm2_opt *opt, int64_t l_pac, const bm2_reads *reads, int32_t n, const bm2_cigar_hit_t *hits,
                       bm2_cigar_task_t *tasks, int32_t *order, bm2_cigar_prep_t *tot);
int bm2_cigar_prep_dev(bm2_ctx *c, const bm2_opt *opt, int64_t l_pac, const bm2_reads *reads, int32_t n, const bm2_cigar_hit_t *hits,
                       bm2_cigar_task_t *tasks, int32_t *order, bm2_cigar_prep_t *tot);
/* A library-private bit of bm2_sam_opt.flag (outside the reference's MEM_F_* range), alone or with any of the seven bits above, on
 * single-end and paired runs: the CIGAR batch of bm2_sam_se_dev, bm2_sam_pe_dev and their _multi forms is prepared by
 * bm2_cigar_prep_dev's kernels where it runs -- the 40-byte hits and the reads' offsets and lengths go up, the tasks and their order
 * are written in device memory, 56 bytes of totals come down.  A batch the device form refuses with BM2_EUNSUP is prepared on the host
 * for that call.  Same bytes, same bm2_sam_cigar_stats.  Off by default.  bm2_sam_se / bm2_sam_pe have no context and answer
 * BM2_EINVAL to it. */
#define BM2_SAM_F_DEVICE_CGPREP 0x00800000
/* of the last bm2_cigar_prep_dev call on this process, or of the last tail with the bit (summed over its contexts): tasks, tasks by
 * shape (RING, ROW, GLOBAL, FLAT), bytes uploaded for the prep, and batches prepared on the host after a refusal. */
void bm2_sam_cigar_prep_stats(int64_t *tasks, int64_t shape[4], int64_t *bytes_up, int64_t *host_fallbacks);
#ifdef __cplusplus
static_assert(sizeof(bm2_cigar_hit_t) == 40 && sizeof(bm2_cigar_task_t) == 72 && sizeof(bm2_cigar_prep_t) == 56, "CIGAR prep records");
#endif


/* ---- the same path split so that a caller can keep inputs resident in HBM and time only the device work */
int bm2_batch_upload(bm2_ctx *c, const bm2_reads *reads);                 /* H2D (pinned staging) */
int bm2_batch_run(bm2_ctx *c, const bm2_opt *opt);                         /* device only, returns after sync */
int bm2_batch_stats(bm2_ctx *c, bm2_stats *stats);
int bm2_batch_download(bm2_ctx *c, bm2_reg_t *regs, int64_t cap, int64_t *reg_off, int64_t *n_out);
/* wall time of the last bm2_batch_run measured with hipEvents on the library's stream, per kernel: SUMMED over the parts of the chunk */
int bm2_batch_kernel_ms(bm2_ctx *c, float *ms, int32_t cap, int32_t *n_out, const char **names);
/* parts the last uploaded chunk was cut into (at multiples of 512 reads, the one cross-read rule of the path: bwamem.cpp:834): each part
 * runs on streams and a workspace of its own, beside the others (launch policy BM2_N_SUB, default 1; a chunk below 64 blocks per part: 1) */
int bm2_batch_parts(const bm2_ctx *c);
/* diagnostic: copy a raw device array of the last bm2_batch_run to the host ("smem", "sa_coord", "chn", "seeds",
 * "regs_raw", ... see pipeline.hip); lets tests pin every stage against the oracle (level ii) */
int bm2_batch_fetch(bm2_ctx *c, const char *what, void *out, int64_t cap_bytes, int64_t *n_bytes);

#ifdef __cplusplus
}
#endif
#endif
