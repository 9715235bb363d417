"""Shared by tests/test_pe_decide_emu.py (the device sources on the host emulator) and tests/test_zzz_pe_decide_gpu.py (the MI355X): the
pairing decisions of mem_sam_pe on the device -- bm2_pe_decide_dev against bm2_pe_decide (the host code of bm2_sam_pe behind a C name) on
lists made here, and the tail with BM2_SAM_F_DEVICE_DECIDE against the flag-off tail and the compiled reference.  Every comparison is
exact: the plans and every byte of every hit."""
import numpy as np

import bm2

LIGHT_MAX = 16        # hits of a pair (both lists) the 16-lane form takes (decide.hip: DC_LIGHT_MAX)
HEAVY_LDS = 96        # hits of a pair the wavefront form keeps in LDS (DC_HEAVY_LDS)
READ_LEN = 150


def contigs(prefix):
    """(offsets, lengths) of the .ann file (bntseq.cpp:113-140: a header line, then two lines per contig)"""
    with open(prefix + ".ann") as f:
        lines = f.read().splitlines()
    n = int(lines[0].split()[1])
    rows = [lines[2 + 2 * i].split() for i in range(n)]
    return np.array([int(r[0]) for r in rows], np.int64), np.array([int(r[1]) for r in rows], np.int64)


def pestat(models):
    """models: {orientation: (low, high, avg, std)}; an orientation that is not named has failed"""
    out = []
    for d in range(4):
        if d in models:
            low, high, avg, std = models[d]
            out.append(bm2.PeStat(low, high, 0, 0, avg, std))
        else:
            out.append(bm2.PeStat(0, 0, 1, 0, 0.0, 0.0))
    return out


FR = {1: (100, 700, 380.5, 61.3)}
ALL4 = {0: (50, 900, 400.25, 130.0), 1: (100, 700, 380.5, 61.3), 2: (1, 500, 200.0, 77.7), 3: (30, 1000, 512.0, 200.0)}


class Maker:
    """Hit lists with the structure the decisions look at: hits that share a stretch of the read (leaders and followers), ALT hits above,
    below and beside primary ones, mates inside and outside the insert-size window on both strands, the same offsets on two contigs."""

    def __init__(self, prefix, seed):
        self.rng = np.random.default_rng(seed)
        self.off, self.len = contigs(prefix)
        self.l_pac = int(self.off[-1] + self.len[-1])
        self.hits, self.hit_off = [], [0]
        self.serial = 0

    def hit(self, contig, pos, rev, qb, qe, score, is_alt=0, span=None, csub=0, sub_n=0, seedcov=None, frac_rep=0.0):
        """a hit whose leftmost forward base is `pos` of `contig` (for a reverse hit mem_pair looks at the forward coordinate of rb, its rightmost base)"""
        span = qe - qb if span is None else span
        fwd = int(self.off[contig]) + int(pos)
        h = np.zeros(1, bm2.ALNREG_DT)[0]
        if rev:
            h["rb"] = 2 * self.l_pac - 1 - (fwd + span - 1)
        else:
            h["rb"] = fwd
        h["re"] = h["rb"] + span
        h["qb"], h["qe"], h["rid"], h["score"], h["truesc"] = qb, qe, contig, score, score
        h["csub"], h["sub_n"], h["seedcov"], h["is_alt"], h["frac_rep"] = csub, sub_n, (qe - qb) if seedcov is None else seedcov, is_alt, frac_rep
        h["w"], h["seedlen0"], h["n_comp"] = 100, 19, 1
        h["sub"], h["alt_sc"], h["secondary"], h["secondary_all"] = 7, 7, 7, 7          # (overwritten by the marking: must not leak)
        self.serial += 1
        h["pad"] = self.serial                                                          # the hit's number: travels with the hit
        h["hash"] = 0x1234567800000000 + self.serial
        return h

    def end_list(self, hits):
        self.hits += hits
        self.hit_off.append(len(self.hits))

    def arrays(self):
        a = np.array(self.hits, bm2.ALNREG_DT) if self.hits else np.zeros(0, bm2.ALNREG_DT)
        return a, np.array(self.hit_off, np.int64)

    def random_list(self, n, locus, mate, equal_scores=False, p_alt=0.0, p_rev=0.5):
        """n hits of one read.  locus = (contig, pos) of the pair; mate: the read whose hits lie `insert` further on, on the other strand"""
        rng = self.rng
        segs = [(0, READ_LEN), (0, 70), (60, READ_LEN), (20, 120)]
        out = []
        for k in range(n):
            qb, qe = segs[int(rng.integers(0, len(segs)))]
            qb, qe = qb + int(rng.integers(0, 6)), qe - int(rng.integers(0, 6))
            score = 100 if equal_scores else int(rng.integers(25, qe - qb + 1))
            kind = rng.random()
            contig, pos = locus
            rev = mate
            if kind < 0.55:                                      # at the pair's locus, in the expected orientation
                pos = pos + (int(rng.integers(150, 650)) if mate else int(rng.integers(0, 40)))
            elif kind < 0.7:                                     # at the locus, the other strand
                pos, rev = pos + int(rng.integers(0, 900)), not mate
            elif kind < 0.8:                                     # the same offsets on another contig
                contig = (contig + 1) % len(self.off)
                pos = pos + (int(rng.integers(150, 650)) if mate else 0)
            else:                                                # somewhere else
                contig = int(rng.integers(0, len(self.off)))
                pos, rev = int(rng.integers(0, max(1, int(self.len[contig]) - 400))), rng.random() < p_rev
            pos = min(max(0, pos), int(self.len[contig]) - 200)
            out.append(self.hit(contig, pos, rev, qb, qe, score, is_alt=int(rng.random() < p_alt), span=qe - qb + int(rng.integers(-3, 4)),
                                csub=int(rng.integers(0, 40)) if rng.random() < 0.3 else 0, sub_n=int(rng.integers(0, 3)),
                                seedcov=int(rng.integers(19, qe - qb + 1)), frac_rep=float(np.float32(rng.choice([0.0, 0.0, 0.1, 0.37, 0.9])))))
        return out

    def pair(self, n0, n1, **kw):
        contig = int(self.rng.integers(0, len(self.off)))
        locus = (contig, int(self.rng.integers(100, max(101, int(self.len[contig]) - 2000))))
        self.end_list(self.random_list(n0, locus, False, **kw))
        self.end_list(self.random_list(n1, locus, True, **kw))


def count_pairings(a0, a1, n_pri, pes, l_pac, offs):
    """how many pairings mem_pair has for the two lists (integers only: positions, ranks, the window of the orientation)"""
    ends = []
    for rd, lst in ((0, a0), (1, a1)):
        for i in range(n_pri[rd]):
            h = lst[i]
            strand = int(h["rb"] >= l_pac)
            fwd = 2 * l_pac - 1 - int(h["rb"]) if strand else int(h["rb"])
            ends.append(((int(h["rid"]) << 32) + fwd - int(offs[int(h["rid"])]), int(h["score"]) & 0xffffffff, i, strand, rd))
    order = sorted(ends)
    n = 0
    for x in range(len(order)):
        for y in range(x + 1, len(order)):
            k, i = order[x], order[y]
            if k[4] == i[4]:
                continue
            m = pes[k[3] << 1 | i[3]]
            if not m.failed and m.low <= i[0] - k[0] <= m.high:
                n += 1
    return n


def outcomes(hits, hit_off, plans, so, pes, l_pac, offs):
    """what the HOST form's results say happened to every pair -> a count per outcome"""
    seen = dict(nopairing=0, empty=0, no_pairing_found=0, second_primary=0, paired_above=0, paired_below=0, switched=0, n_sub=0, alt_shadow=0)
    for p in range(len(plans)):
        P = plans[p]
        a = [hits[hit_off[2 * p]:hit_off[2 * p + 1]], hits[hit_off[2 * p + 1]:hit_off[2 * p + 2]]]
        n_pri = [int(P["n_pri"][0]), int(P["n_pri"][1])]
        seen["alt_shadow"] += int(any((l["alt_sc"] > 0).any() for l in a if len(l)))
        if so.flag & 0x4:
            seen["nopairing"] += 1
            continue
        if not n_pri[0] or not n_pri[1]:
            seen["empty"] += 1
            continue
        n_pairings = count_pairings(a[0], a[1], n_pri, pes, l_pac, offs)
        if n_pairings > 1:
            seen["n_sub"] += 1
        if not P["paired"]:
            second = any(a[i][j]["secondary"] < 0 and a[i][j]["score"] >= so.T for i in range(2) for j in range(1, n_pri[i]))
            if n_pairings == 0:
                seen["no_pairing_found"] += 1
            elif second:
                seen["second_primary"] += 1
            continue
        assert n_pairings > 0, p
        if P["extra_flag"] & 2:
            seen["paired_above"] += 1
        else:
            seen["paired_below"] += 1
        for i in range(2):
            c = a[i][int(P["z"][i])]
            if c["secondary"] == -2 and c["secondary_all"] == -1:
                seen["switched"] += 1
    return seen


def compare(ctx, prefix, opt, so, hits, hit_off, pes, first_pair=0, what=""):
    """bm2_pe_decide_dev against bm2_pe_decide on copies of the same lists: plans and every byte of every hit -> the host's results"""
    h_hits, h_plans = bm2.pe_decide(prefix, opt, so, hits, hit_off, pes, first_pair)
    d_hits, d_plans = ctx.pe_decide(opt, so, hits, hit_off, pes, first_pair)
    if h_plans.tobytes() != d_plans.tobytes():
        for p in range(len(h_plans)):
            assert h_plans[p] == d_plans[p], "%s: pair %d (lists of %d and %d hits, id %d)\n  host   %s\n  device %s" % (
                what, p, hit_off[2 * p + 1] - hit_off[2 * p], hit_off[2 * p + 2] - hit_off[2 * p + 1], first_pair + p, h_plans[p], d_plans[p])
    if h_hits.tobytes() != d_hits.tobytes():
        for i in range(len(h_hits)):
            if h_hits[i] != d_hits[i]:
                li = int(np.searchsorted(hit_off, i, side="right")) - 1
                assert False, "%s: hit %d (list %d, place %d of %d)\n  fields %s\n  host   %s\n  device %s" % (
                    what, i, li, i - hit_off[li], hit_off[li + 1] - hit_off[li], h_hits.dtype.names, h_hits[i], d_hits[i])
    # every input hit is in its list exactly once (the number travels with the hit)
    for li in (0, len(hit_off) // 2, len(hit_off) - 2):
        if li >= 0 and li + 1 < len(hit_off):
            assert sorted(h_hits["pad"][hit_off[li]:hit_off[li + 1]]) == sorted(np.asarray(hits)["pad"][hit_off[li]:hit_off[li + 1]])
    return h_hits, h_plans


def size_mix(big=True):
    """list lengths: 0 .. 17 on either side (both sides of the 16-lane bound), the LDS range of the wavefront form and one above its bound,
    and a pair with more than 700 hits per read"""
    sizes = [(i, (i * 7 + 3) % 18) for i in range(18)] + [((i * 5 + 1) % 18, i) for i in range(18)]
    sizes += [(8, 8), (9, 8), (16, 0), (0, 17), (17, 17), (1, 1), (1, 1), (2, 1), (30, 25), (48, 48), (HEAVY_LDS - 47, 48)]
    if big:
        sizes += [(705, 722)]
    return sizes


def check_lists(ctx, prefix, quick=False):
    """Item 1 of the issue: hand-made and random lists under every option the decisions read.  quick: the emulator's share (the big pair once)."""
    offs, _ = contigs(prefix)
    with bm2.Index(prefix) as ix:
        l_pac = ix.l_pac
    total = dict()
    heavy_seen = light_seen = 0
    configs = [
        ("default", {}, {}, FR, 0, {}),
        ("all orientations", {}, {}, ALL4, 12345, {}),
        ("equal scores", {}, {}, FR, 7, dict(equal_scores=True)),
        ("ALT hits", {}, {}, ALL4, 3, dict(p_alt=0.35)),
        ("ALT hits, equal scores", {}, {}, FR, 3, dict(p_alt=0.5, equal_scores=True)),
        ("only ALT hits", {}, {}, FR, 3, dict(p_alt=1.0)),
        ("-5", {}, dict(flag=0x800), FR, 11, dict(p_alt=0.1)),
        ("no pairing", {}, dict(flag=0x4), FR, 11, {}),
        ("id wraps in (int)id << 8", {}, {}, FR, (1 << 23) - 1, {}),
        ("id above 2^31", {}, {}, ALL4, (1 << 31) + 5, dict(p_alt=0.2)),
        ("scoring", dict(a=2, b=7, o_del=9, e_del=2, o_ins=5, e_ins=3, mask_level=0.7, min_seed_len=23), dict(pen_unpaired=9, T=60), ALL4, 1, dict(p_alt=0.2)),
        ("log(seedcov) branch", {}, dict(mapQ_coef_len=0.0, mapQ_coef_fac=0), FR, 2, dict(p_alt=0.1)),
        ("T 20, -U 40", {}, dict(T=20, pen_unpaired=40), ALL4, 2, {}),
        ("erfc underflows", {}, {}, {1: (1, 2000, 400.0, 1.0)}, 5, {}),
        ("all failed", {}, {}, {}, 5, {}),
    ] + [("orientation %d failed" % d, {}, {}, {k: v for k, v in ALL4.items() if k != d}, 9, {}) for d in range(4)] \
      + [("orientation %d alone" % d, {}, {}, {d: ALL4[d]}, 9, {}) for d in (0, 2, 3)]
    for ci, (name, okw, skw, models, first_pair, mk) in enumerate(configs):
        M = Maker(prefix, 1000 + ci)
        for n0, n1 in size_mix(big=(ci < 1) if quick else (ci % 4 < 2)):
            M.pair(n0, n1, **mk)
        hits, hit_off = M.arrays()
        opt, so, pes = bm2.default_opt(**okw), bm2.default_sam_opt(**skw), pestat(models)
        h_hits, h_plans = compare(ctx, prefix, opt, so, hits, hit_off, pes, first_pair, name)
        pairs, n_hits, heavy = bm2.sam_decide_stats()
        assert pairs == len(h_plans) and n_hits == len(hits), (pairs, n_hits)
        tot = np.diff(hit_off)[0::2] + np.diff(hit_off)[1::2]
        assert heavy == int((tot > LIGHT_MAX).sum()), (heavy, int((tot > LIGHT_MAX).sum()))
        heavy_seen += heavy
        light_seen += pairs - heavy
        for k, v in outcomes(h_hits, hit_off, h_plans, so, pes, l_pac, offs).items():
            total[k] = total.get(k, 0) + v
    assert heavy_seen > 0 and light_seen > 0, (heavy_seen, light_seen)
    missing = [k for k, v in total.items() if v == 0]
    assert not missing, "the inputs never reach: %s (%s)" % (missing, total)
    return total


def sweep_arrays(prefix, n, seed, stride=1):
    """The arithmetic sweep: pairs of one or two hits per read, drawn (seeded) from a grid of score, second score, csub, incoming sub_n, spans
    on read and reference, seed coverage, frac_rep and distance.  stride: every stride-th pair of the same sequence (the emulator's subsample)."""
    rng = np.random.default_rng(seed)
    M = Maker(prefix, seed)
    scores = [30, 31, 45, 60, 75, 99, 100, 120, 149, 150]
    fracs = [0.0, 0.0, 0.0, 0.05, 0.1, 0.25, 0.3333, 0.5, 0.75, 0.9, 1.0]
    for p in range(n):
        draw = rng.integers(0, 1 << 30, 40)
        if p % stride:
            continue
        contig = int(draw[0] % len(M.off))
        x = 200 + int(draw[1] % max(1, int(M.len[contig]) - 3000))
        dist = int([90, 100, 101, 250, 380, 381, 400, 550, 699, 700, 701][draw[2] % 11]) if draw[3] % 4 == 0 else 80 + int(draw[2] % 640)
        lists = []
        for rd in range(2):
            d = draw[4 + 16 * rd:20 + 16 * rd]
            span = int([30, 49, 50, 51, 75, 100, 149, 150][d[0] % 8])
            qb = int(d[1] % (READ_LEN - span + 1))
            sc = min(int(scores[d[2] % len(scores)]), span)
            first = M.hit(contig, x + (dist if rd else 0), bool(rd), qb, qb + span, sc, span=span + int(d[3] % 7) - 3,
                          csub=int([0, 0, 10, 25, sc - 1, sc, sc + 5][d[4] % 7]), sub_n=int([0, 0, 1, 2, 5, 30][d[5] % 6]),
                          seedcov=int([1, 19, 20, 50, span][d[6] % 5]), frac_rep=float(np.float32(fracs[d[7] % len(fracs)])))
            lst = [first]
            mode = d[8] % 4                                      # none / a hit under the first (sub, sub_n) / a hit beside it (a second primary) / both near
            if mode:
                sc2 = max(1, int([sc, sc - 1, sc - 5, sc - 6, sc - 20, sc // 2][d[9] % 6]))
                if mode == 2 and span <= READ_LEN // 2:
                    qb2 = qb + span if qb + 2 * span <= READ_LEN else qb - span
                    qb2 = max(0, qb2)
                else:
                    qb2 = qb
                c2 = (contig + 1) % len(M.off) if d[10] % 2 else contig
                near = mode == 3
                pos2 = x + (dist if rd else 0) + int(d[11] % 40) - 20 if near else 100 + int(d[11] % max(1, int(M.len[c2]) - 2000))
                lst.append(M.hit(contig if near else c2, max(0, pos2), bool(rd) if near or d[12] % 2 else not rd, qb2, qb2 + span, sc2, span=span,
                                 csub=int(d[13] % 30) if d[14] % 3 == 0 else 0, sub_n=int(d[14] % 2), frac_rep=float(np.float32(fracs[d[15] % len(fracs)]))))
            lists.append(lst)
        M.end_list(lists[0])
        M.end_list(lists[1])
    return M.arrays()


def check_sweep(ctx, prefix, n, stride=1):
    """-> pairs compared; both mapQ_coef_len branches, the outcomes asserted from the host's plans"""
    offs, _ = contigs(prefix)
    with bm2.Index(prefix) as ix:
        l_pac = ix.l_pac
    total, done = dict(), 0
    for seed, skw in ((501, {}), (502, dict(mapQ_coef_len=0.0, mapQ_coef_fac=0))):
        hits, hit_off = sweep_arrays(prefix, n, seed, stride)
        so, pes = bm2.default_sam_opt(**skw), pestat(FR)
        h_hits, h_plans = compare(ctx, prefix, bm2.default_opt(), so, hits, hit_off, pes, 1 << 20, "sweep %d" % seed)
        done += len(h_plans)
        for k, v in outcomes(h_hits, hit_off, h_plans, so, pes, l_pac, offs).items():
            total[k] = total.get(k, 0) + v
        assert len(set(h_plans["q_se"].ravel().tolist())) > 30, "the sweep reaches few mapping qualities"
    missing = [k for k in ("no_pairing_found", "second_primary", "paired_above", "paired_below", "switched", "n_sub") if not total.get(k)]
    assert not missing, "the sweep never reaches: %s (%s)" % (missing, total)
    return done, total


def check_refusals(ctx, prefix):
    """a context without an index; the table-span rule; offsets out of order; a hit on no contig"""
    M = Maker(prefix, 5)
    M.pair(3, 3)
    hits, hit_off = M.arrays()
    opt, so = bm2.default_opt(), bm2.default_sam_opt()

    def refused(rc, word, f):
        try:
            f()
        except bm2.Bm2Error as e:
            assert e.rc == rc and word in str(e), (rc, word, e)
            return
        raise AssertionError("accepted: " + word)
    bare = bm2.Context(0, None)
    try:
        refused(bm2.BM2_EINVAL, "no index", lambda: bare.pe_decide(opt, so, hits, hit_off, pestat(FR)))
    finally:
        bare.close()
    wide = {0: (0, 1 << 21, 400.0, 50.0), 1: (0, 1 << 21, 400.0, 50.0), 2: (1, 100, 50.0, 5.0)}
    refused(bm2.BM2_EUNSUP, "2^22", lambda: ctx.pe_decide(opt, so, hits, hit_off, pestat(wide)))
    ok = {0: (0, (1 << 21) - 2, 400.0, 50.0), 1: (0, (1 << 21) - 2, 400.0, 50.0)}           # just inside: accepted, and equal to the host
    compare(ctx, prefix, opt, so, hits, hit_off, pestat(ok), 0, "wide model")
    bad_off = hit_off.copy()
    bad_off[1] = hit_off[2] + 1
    refused(bm2.BM2_EINVAL, "hit_off", lambda: ctx.pe_decide(opt, so, hits, bad_off, pestat(FR)))
    refused(bm2.BM2_EINVAL, "hit_off", lambda: bm2.pe_decide(prefix, opt, so, hits, bad_off, pestat(FR)))
    off_contig = hits.copy()
    off_contig["rid"][2] = 1000
    refused(bm2.BM2_EINVAL, "contig", lambda: ctx.pe_decide(opt, so, off_contig, hit_off, pestat(FR)))
    empty_h, empty_p = ctx.pe_decide(opt, so, hits[:0], np.zeros(1, np.int64), pestat(FR))
    assert len(empty_h) == 0 and len(empty_p) == 0
    return True


class PeTail:
    """One paired input through the tail many times: the FASTQ files, the hits (oracle + bm2_finish_regs: no GPU involved) and the
    reference's text per option set are made once.  M = the test_sam_tail module."""

    def __init__(self, M, d, fa, r1, r2):
        import subprocess
        from helpers import oracle_finish_regs, ref_binary
        from tools import oracle, refio
        self.M, self.fa, self.n_pairs = M, fa, len(r1)
        rng = np.random.default_rng(9)
        reads, self.quals, self.names = [], [], []
        for i in range(len(r1)):
            for r in (r1[i], r2[i]):
                reads.append(r)
                self.quals.append(bytes(rng.integers(40, 74, size=len(r), dtype=np.uint8)))
                self.names.append("p%d" % i)
        self.f1, self.f2 = str(d / "d1.fq"), str(d / "d2.fq")
        for path, sel in ((self.f1, 0), (self.f2, 1)):
            with open(path, "wb") as f:
                for i in range(sel, len(reads), 2):
                    f.write(b"@" + self.names[i].encode() + b"\n" + bytes(b"ACGTN"[c] for c in reads[i]) + b"\n+\n" + self.quals[i] + b"\n")
        self.enc, self.off, self.ln = refio.pack_reads(reads)
        ix = oracle.Index(fa)
        try:
            exp = ix.run(self.enc, self.off, self.ln, oracle.default_opt())
        finally:
            ix.close()
        self.opt = bm2.default_opt()
        regs, reg_off = M._prg_to_regs(exp["REGPRG"], len(self.ln))
        self.aln, self.aln_off = oracle_finish_regs(fa, self.enc, self.off, self.ln, self.opt, regs, reg_off)
        self._ref, self._run, self._exe = {}, subprocess.run, ref_binary()

    def reference(self, extra):
        key = tuple(extra)
        if key not in self._ref:
            p = self._run([self._exe, "mem", "-t", "1"] + list(extra) + [self.fa, self.f1, self.f2], stdout=-1, stderr=-3, check=True)
            self._ref[key] = b"".join(l for l in p.stdout.splitlines(keepends=True) if not l.startswith(b"@"))
        return self._ref[key]

    def ours(self, flag, ctx, **skw):
        return bm2.sam_pe(self.fa, self.enc, self.off, self.ln, self.opt, self.aln, self.aln_off, self.names, self.quals, None,
                          bm2.default_sam_opt(flag=flag, **skw), ctx=ctx)

    def check(self, extra, ctx, flag=0, both=False, **skw):
        """the tail with the bit == without == `bwa-mem2 mem`, pes_out equal; both: also the bit together with SAM_F_DEVICE_TEXT.  The rescue
        and CIGAR counters do not move.  -> (text, pes)"""
        ref = self.reference(extra)
        off_text, pes_off = self.ours(flag, ctx, **skw)
        st_off = (bm2.sam_rescue_stats(), bm2.sam_cigar_stats())
        assert ref == off_text, self.M._diff(ref, off_text)
        for bits in [bm2.SAM_F_DEVICE_DECIDE] + ([bm2.SAM_F_DEVICE_DECIDE | bm2.SAM_F_DEVICE_TEXT] if both else []):
            on_text, pes_on = self.ours(flag | bits, ctx, **skw)
            assert (bm2.sam_rescue_stats(), bm2.sam_cigar_stats()) == st_off, (st_off, bm2.sam_rescue_stats(), bm2.sam_cigar_stats())
            assert ref == on_text, self.M._diff(ref, on_text)
            assert [bytes(x) for x in pes_on] == [bytes(x) for x in pes_off]
            pairs, n_hits, heavy = bm2.sam_decide_stats()
            assert pairs == self.n_pairs and n_hits >= len(self.aln), (pairs, n_hits, heavy, len(self.aln))
        return ref, pes_off

    def option_sets(self, ctx, ctx2=None, part_knob=None):
        """the option sets of the issue: default (1 against 7 host threads, both bits), -a, -Y -M, -5 -T 50, -S, -P, two contexts"""
        import os
        ref, pes = self.check([], ctx, both=True, n_threads=1)
        assert self.check([], ctx, n_threads=7)[0] == ref
        self.check(["-a"], ctx, flag=0x8)
        self.check(["-Y", "-M"], ctx, flag=0x200 | 0x10, both=True)
        self.check(["-5", "-T", "50"], ctx, flag=0x800 | 0x1000, T=50)
        self.check(["-S"], ctx, flag=0x20)
        self.check(["-P"], ctx, flag=0x4)
        if ctx2 is not None:
            os.environ["BM2_DECIDE_PART"] = str(part_knob)       # (launch policy: pairs per context; small, so that both contexts decide a part)
            os.environ["BM2_TEXT_PART"] = str(part_knob)
            try:
                assert self.check([], [ctx, ctx2], both=True)[0] == ref
            finally:
                del os.environ["BM2_DECIDE_PART"], os.environ["BM2_TEXT_PART"]
        return pes

    def host_outcomes(self, pes, **skw):
        """what the host form decides on the INPUT lists (the lists of a -S run: no hit is added) under the chunk's model"""
        so = bm2.default_sam_opt(**skw)
        h_hits, h_plans = bm2.pe_decide(self.fa, self.opt, so, self.aln, self.aln_off, pes, 0)
        offs, _ = contigs(self.fa)
        with bm2.Index(self.fa) as ix:
            l_pac = ix.l_pac
        return outcomes(h_hits, np.asarray(self.aln_off), h_plans, so, pes, l_pac, offs)


def constructed_case(M, d):
    """The PE input that reaches what the synthetic reads never do (the issue's construction): the genome of M._pe_case(61, ...) with twenty
    150-base stretches of contig 0 copied, 7 substitutions each, 250 bases behind twenty other places; 400 ordinary pairs; 20 pairs whose
    mate maps better to the source of the copy than beside read 1 (paired, but not above the unpaired score); 20 pairs whose read 1 is two
    halves from far apart (a second primary hit above T: the reads go out one by one)."""
    import subprocess
    from helpers import ref_binary
    import helpers
    from tools import synth
    if ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present (build it with `make -C oracle ref`)")
    names, ctg, alts = synth.make_genome(61, [300000, 150000, 60000], alt_contigs=1, alt_len=4000, n_repeat_families=8, repeat_len=(200, 2500),
                                         copies=(3, 30), divergence=(0.0, 0.06))
    c0 = ctg[0]
    for k in range(20):
        src = c0[200000 + 1000 * k:200000 + 1000 * k + 150].copy()
        src[10::20] = (src[10::20] + 1) % 4                      # (ACGT codes; an N of the source becomes an A)
        assert len(src[10::20]) == 7
        c0[50000 + 2000 * k + 250:50000 + 2000 * k + 400] = src
    fa = str(d / "gc.fa")
    synth.write_fasta(fa, names, ctg)
    synth.write_alt(fa + ".alt", alts)
    subprocess.check_call([ref_binary(), "index", fa], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r1, r2 = synth.make_reads_pe(62, ctg, 400, L=150, sub_rate=0.02, indel_frac=0.2, random_frac=0.03)
    r1, r2 = list(r1), list(r2)

    def revcomp(x):
        x = np.asarray(x, np.uint8)[::-1]
        return np.where(x < 4, 3 - x, 4).astype(np.uint8)
    for k in range(20):
        r1.append(c0[50000 + 2000 * k:50000 + 2000 * k + 150].copy())
        r2.append(revcomp(c0[200000 + 1000 * k:200000 + 1000 * k + 150]))
    for k in range(20):
        r1.append(np.concatenate([c0[120000 + 1500 * k:120000 + 1500 * k + 75], c0[250000 + 1200 * k:250000 + 1200 * k + 75]]))
        r2.append(revcomp(c0[120000 + 1500 * k + 250:120000 + 1500 * k + 400]))
    return fa, r1, r2
