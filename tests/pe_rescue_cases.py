"""Shared by tests/test_pe_rescue_emu.py (the device sources on the host emulator) and tests/test_zzzz_pe_rescue_gpu.py (the MI355X):
mate-rescue results applied to the hit lists on the device -- bm2_pe_rescue_apply_dev against bm2_pe_rescue_apply (the host code of
bm2_sam_pe's rescue loop without its aligner) on lists made here with fabricated results, the host form on real tasks against the text
of bm2_sam_pe's own flow, and the tail with BM2_SAM_F_DEVICE_RESCUE against the flag-off tail and the compiled reference.  Every
comparison is exact: offsets, redo flags and every byte of every hit, padding included."""
import ctypes as C
import os

import numpy as np

import bm2
import pe_decide_cases as D
from test_ksw_align2 import KSW_XBYTE, KSW_XSTART, KSW_XSUBO

READ_LEN = D.READ_LEN
HEAVY_COST = 1024     # tasks x (hits + tasks) above which a pair is in the heaviest class of launches (rescue.hip: cls)


def flip_of(r):
    return (r >> 1) != (r & 1)


def rescued_hit(task, res, l_ms, l_pac):
    """(rb, re, qb, qe) of the hit mem_matesw makes of a result (bwamem_pair.cpp:205-222)"""
    qb, qe, b, e = int(res[6]), int(res[2]) + 1, int(task["rb"]) + int(res[5]), int(task["rb"]) + int(res[1]) + 1
    if flip_of(int(task["r"])):
        qb, qe, b, e = l_ms - qe, l_ms - qb, 2 * l_pac - e, 2 * l_pac - b
    return b, e, qb, qe


def fabricate(tasks, hits, hit_off, l_pac, seed, p_low=0.08, p_neg=0.05):
    """Results for planned tasks, made up (the apply step never looks at the bases).  A task's result lands at an absolute place of its
    window quantised to 64 bases, with a score that depends on the place alone: anchors of one read near each other get the SAME hit
    (the later one is a duplicate: removed, or equal in (score, rb, qb)), places 64 apart overlap by less than mask_level_redun.  Where
    a hit of the mate lies inside the window (beyond `high`: not at a plausible distance, so the direction is open) the result copies
    its place with a score above or below it.  Some results score below min_seed_len, some have qb < 0."""
    rng = np.random.default_rng(seed)
    t = tasks.copy()
    for k in range(len(t)):
        T = t[k]
        rb, re, r = int(T["rb"]), int(T["re"]), int(T["r"])
        u = rng.random()
        mate = hits[hit_off[2 * T["pair"] + (1 - T["end"])]:hit_off[2 * T["pair"] + (1 - T["end"]) + 1]]
        res = None
        if u < 0.5 and len(mate):                               # on top of a hit of the mate that lies in the window
            for h in mate[rng.permutation(len(mate))]:
                hb, he = (2 * l_pac - int(h["re"]), 2 * l_pac - int(h["rb"])) if flip_of(r) else (int(h["rb"]), int(h["re"]))
                if hb >= rb and he <= re:
                    qb, qe = (READ_LEN - int(h["qe"]), READ_LEN - int(h["qb"])) if flip_of(r) else (int(h["qb"]), int(h["qe"]))
                    res = [int(h["score"]) + int(rng.integers(-6, 7)), he - 1 - rb, qe - 1, int(rng.integers(0, 40)), -1, hb - rb, qb]
                    break
        if res is None:
            g = ((rb + 63) // 64) * 64
            g += 64 * int(rng.integers(0, 3))
            span = 140 + g // 64 % 7
            if g + span > re:
                res = [5, 9, 9, 0, -1, 0, 0]                     # a window too short for the made-up hit: a result below min_seed_len
            else:
                qb = g // 64 % 8
                res = [60 + g // 64 * 7 % 80, g + span - 1 - rb, qb + 139, g // 64 % 50, -1, g - rb, qb]
        if u > 1 - p_low:
            res[0] = int(rng.integers(0, 19))
        elif u > 1 - p_low - p_neg:
            res[5], res[6] = -1, -1
        t["res"][k] = res
    return t


class Lists(D.Maker):
    """pe_decide_cases.Maker plus the hand-made pairs of the issue"""

    def far_pair(self, model, score_in, n_anchor=1, alt=0, contig=0, x=None, rev=False):
        """read 0: n_anchor full-length hits at x .. ; read 1: one hit on the anchor's strand `high + 10` bases further on: not at a
        plausible distance (the direction stays open), yet inside the window, which reaches l_ms beyond `high`"""
        x = int(self.rng.integers(3000, int(self.len[contig]) - 5000)) if x is None else x
        low, high = model[0][0], model[0][1]
        self.end_list([self.hit(contig, x + 3 * k, rev, 0, READ_LEN, 140 - k, is_alt=alt) for k in range(n_anchor)])
        self.end_list([self.hit(contig, x + (-high if rev else high + 10), rev, 0, 140, score_in, span=140)])      # (a reverse hit's rb is its last base)

    def tie_pair(self, model, contig=0):
        """read 1 holds what a de-duplication cannot order by its keys: two hits that end at the same base (apart on the read: both
        stay), and two equal in (score, rb, qb) that the overlap sweep never compares (a hit of another contig ends between them)"""
        x = int(self.rng.integers(3000, int(self.len[contig]) - 5000))
        far = x + model[0][1] + 400                              # beyond every window of the anchor
        self.end_list([self.hit(contig, x, False, 0, READ_LEN, 140)])
        a = self.hit(contig, far, False, 0, 70, 60, span=100)
        b = self.hit(contig, far + 40, False, 80, 150, 60, span=60)          # ends where a ends
        q = self.hit(contig, far + 300, False, 0, 100, 90, span=100)
        xh = self.hit(contig, far + 350, False, 0, 30, 30, span=70)
        xh["rid"] = (contig + 1) % len(self.off)                 # (fabricated: the apply step takes rid as it comes)
        p = self.hit(contig, far + 300, False, 0, 140, 90, span=140)
        assert a["re"] == b["re"] and q["rb"] == p["rb"] and q["re"] < xh["re"] < p["re"]
        self.end_list([q, p, a, b, xh])


def with_tasks_for_failed_orientations(tasks, task_off, models, n_pairs):
    """For every planned task a twin in each FAILED orientation that (end, j) does not hold yet, with a result that would make a hit of
    its own (score 149, a place no other result has) and pad = 1 to tell it by.  rescue_skip skips a failed orientation whatever the
    lists say, so neither form may apply such a task.  -> (tasks, task_off) in (pair, end, j, r) order"""
    failed = [d for d in range(4) if d not in models]
    if not failed or not len(tasks):
        return tasks, task_off
    have = set(zip(tasks["pair"].tolist(), tasks["end"].tolist(), tasks["j"].tolist(), tasks["r"].tolist()))
    extra = []
    for t in tasks:
        for d in failed:
            key = (int(t["pair"]), int(t["end"]), int(t["j"]), d)
            if key not in have and int(t["re"] - t["rb"]) > 160:
                have.add(key)
                x = t.copy()
                x["r"], x["pad"] = d, 1
                x["res"] = [149, 3 + 147, 148, 0, -1, 3, 1]
                extra.append(x)
    if not extra:
        return tasks, task_off
    t = np.concatenate([tasks, np.array(extra, tasks.dtype)])
    t = t[np.lexsort((t["r"], t["j"], t["end"], t["pair"]))]
    return t, np.concatenate([[0], np.cumsum(np.bincount(t["pair"], minlength=n_pairs))]).astype(np.int64)


def compare(ctx, prefix, opt, so, hits, hit_off, read_len, pes, tasks, task_off, what=""):
    """bm2_pe_rescue_apply_dev against bm2_pe_rescue_apply -> the host's (out, out_off, redo)"""
    h_out, h_off, h_redo = bm2.pe_rescue_apply(prefix, opt, so, hits, hit_off, read_len, pes, tasks, task_off)
    h_st = bm2.sam_rescue_apply_stats()
    d_out, d_off, d_redo = ctx.pe_rescue_apply(opt, so, hits, hit_off, read_len, pes, tasks, task_off)
    d_st = bm2.sam_rescue_apply_stats()
    assert (h_redo == d_redo).all(), "%s: redo differs at pairs %s" % (what, np.nonzero(h_redo != d_redo)[0][:10])
    if (h_off != d_off).any():
        li = int(np.nonzero(h_off != d_off)[0][0]) - 1
        assert False, "%s: list %d (pair %d) holds %d hits on the host, %d on the device" % (what, li, li // 2, h_off[li + 1] - h_off[li], d_off[li + 1] - d_off[li])
    if h_out.tobytes() != d_out.tobytes():
        for i in range(len(h_out)):
            if h_out[i].tobytes() != d_out[i].tobytes():
                li = int(np.searchsorted(h_off, i, side="right")) - 1
                assert False, "%s: hit %d (list %d of pair %d, place %d of %d)\n  fields %s\n  host   %s\n  device %s" % (
                    what, i, li, li // 2, i - h_off[li], h_off[li + 1] - h_off[li], h_out.dtype.names, h_out[i], d_out[i])
    assert h_st == d_st, (h_st, d_st)
    return h_out, h_off, h_redo, h_st


def occurrences(hits, hit_off, tasks, task_off, out, out_off, redo, l_pac, so, opt):
    """what the HOST form's output says happened -> a count per event of the issue's list"""
    seen = dict(both_empty=0, one_empty=0, low_score=0, neg_qb=0, dir0=0, dir1=0, dir2=0, dir3=0, plain=0, mirrored=0, equal_score_insert=0,
                input_removed=0, rescued_present=0, tie_re=0, tie_key=0, list_over_16=0, heavy=0, matesw_cut=0, alt_anchor=0, redo=0, failed_orientation=0)
    for p in range(len(redo)):
        n0, n1 = int(hit_off[2 * p + 1] - hit_off[2 * p]), int(hit_off[2 * p + 2] - hit_off[2 * p + 1])
        T = tasks[task_off[p]:task_off[p + 1]]
        seen["both_empty"] += n0 == 0 and n1 == 0
        seen["one_empty"] += (n0 == 0) != (n1 == 0)
        seen["redo"] += int(redo[p])
        if redo[p] or not len(T):
            continue
        seen["heavy"] += len(T) * (n0 + n1 + len(T)) > HEAVY_COST
        for e in range(2):
            lst = hits[hit_off[2 * p + e]:hit_off[2 * p + e + 1]]
            if len(lst):
                n_cand = int((lst["score"] >= lst["score"][0] - so.pen_unpaired).sum())
                seen["matesw_cut"] += n_cand > so.max_matesw and int(T["j"][T["end"] == e].max(initial=-1)) == so.max_matesw - 1
        for m in range(2):                                       # the list of read m: grown by the tasks whose anchor is on the other end
            got = out[out_off[2 * p + m]:out_off[2 * p + m + 1]]
            was = hits[hit_off[2 * p + m]:hit_off[2 * p + m + 1]]
            mine = T[T["end"] == 1 - m]
            if not len(mine):
                continue
            new = got[got["pad"] == 0]                           # (input hits are numbered from 1, a rescued hit's pad is zero)
            places = set((int(h["rb"]), int(h["re"]), int(h["qb"]), int(h["qe"])) for h in new)
            usable = 0
            for t in mine:
                res = t["res"]
                if t["pad"]:                                     # a task slipped in for a FAILED orientation: both forms must pass it by
                    assert rescued_hit(t, res, READ_LEN, l_pac) not in places, (p, t)
                    seen["failed_orientation"] += 1
                elif res[0] < opt.min_seed_len:
                    seen["low_score"] += 1
                elif res[6] < 0:
                    seen["neg_qb"] += 1
                else:
                    usable += 1
                    if rescued_hit(t, res, READ_LEN, l_pac) in places:
                        seen["dir%d" % int(t["r"])] += 1
                        seen["mirrored" if flip_of(int(t["r"])) else "plain"] += 1
            if len(new):
                seen["input_removed"] += len(set(was["pad"].tolist()) - set(got["pad"].tolist())) > 0
                seen["equal_score_insert"] += any(int((got["score"] == h["score"]).sum()) > 1 for h in new)
                seen["alt_anchor"] += int((new["is_alt"] != 0).any())
                seen["list_over_16"] += len(got) > 16
                seen["tie_re"] += len(set(got["re"].tolist())) < len(got)
            # equal in (score, rb, qb): of two such input hits one is gone although they do not overlap on the read's and the
            # reference's shorter span -- only the third sweep removes such a hit
            keys = {}
            for h in was:
                keys.setdefault((int(h["score"]), int(h["rb"]), int(h["qb"])), []).append(int(h["pad"]))
            for k, pads in keys.items():
                if len(pads) > 1 and 0 < len(set(pads) & set(got["pad"].tolist())) < len(pads):
                    seen["tie_key"] += 1
            seen["rescued_present"] += len(new)
    return {k: int(v) for k, v in seen.items()}


def check_lists(ctx, prefix, quick=False):
    """Item 1 of the issue.  quick: the emulator's share (the big pair once, fewer random configurations)."""
    with bm2.Index(prefix) as ix:
        l_pac = ix.l_pac
    total = dict()
    configs = [
        ("all orientations", {}, {}, D.ALL4, 21, {}),
        ("FR only", {}, {}, D.FR, 22, {}),
        ("equal scores", {}, {}, D.ALL4, 23, dict(equal_scores=True)),
        ("ALT hits", {}, {}, D.ALL4, 24, dict(p_alt=0.5)),
        ("-m 3", {}, dict(max_matesw=3), D.ALL4, 25, dict(equal_scores=True)),
        ("-U 40, mask_level_redun 0.5, max_chain_gap 100", dict(mask_level_redun=0.5, max_chain_gap=100), dict(pen_unpaired=40), D.ALL4, 26, {}),
        ("min_seed_len 30", dict(min_seed_len=30), dict(pen_unpaired=3), D.ALL4, 27, {}),
    ] + [("orientation %d failed" % d, {}, {}, {k: v for k, v in D.ALL4.items() if k != d}, 30 + d, {}) for d in range(4)]
    if quick:
        configs = configs[:5] + configs[7:8]
    for ci, (name, okw, skw, models, seed, mk) in enumerate(configs):
        M = Lists(prefix, 2000 + seed)
        for n0, n1 in D.size_mix(big=(ci == 0) if quick else (ci % 3 == 0)):
            M.pair(n0, n1, **mk)
        M.pair(0, 0)
        M.pair(110, 120, equal_scores=True)                      # enough anchors and hits for a wavefront of its own
        if 0 in models:
            for score_in in (100, 120, 131, 140):
                M.far_pair(models, score_in)
                M.far_pair(models, score_in, n_anchor=5, alt=1)
                M.far_pair(models, score_in, n_anchor=2, rev=True)
            for _ in range(4):
                M.tie_pair(models)
        hits, hit_off = M.arrays()
        n_pairs = (len(hit_off) - 1) // 2
        read_len = np.full(2 * n_pairs, READ_LEN, np.int32)
        opt, so, pes = bm2.default_opt(**okw), bm2.default_sam_opt(**skw), D.pestat(models)
        tasks, task_off = bm2.pe_rescue_plan(prefix, opt, so, hits, hit_off, read_len, pes)
        assert len(tasks) > 100, (name, len(tasks))
        for d in range(4):
            assert (d in models) == bool((tasks["r"] == d).any()), (name, d)          # a failed orientation plans nothing
        tasks = fabricate(tasks, hits, hit_off, l_pac, seed)
        tasks, task_off = with_tasks_for_failed_orientations(tasks, task_off, models, n_pairs)
        out, out_off, redo, st = compare(ctx, prefix, opt, so, hits, hit_off, read_len, pes, tasks, task_off, name)
        assert st[0] == n_pairs and st[1] == len(tasks) and st[3] == int(redo.sum()), (st, n_pairs, len(tasks))
        for k, v in occurrences(hits, hit_off, tasks, task_off, out, out_off, redo, l_pac, so, opt).items():
            total[k] = total.get(k, 0) + v
        total["hits_added"] = total.get("hits_added", 0) + st[2]
        total["rescued_removed"] = total["hits_added"] - total["rescued_present"]      # inserted, and gone from the output
        # a needed task left out: the first task of a pair is judged on the lists as they came, exactly as the plan judged it, so
        # its direction is open and its window valid -- without it the pair must come back with redo and its lists as they came
        real = tasks["pad"] == 0                                 # (not the twins in failed orientations: those are passed by anyway)
        grew = [p for p in range(n_pairs) if int(real[task_off[p]:task_off[p + 1]].sum()) >= 2 and not redo[p]]       # (a pair left without any task is copied through)
        drop = [int(task_off[p]) + int(np.argmax(real[task_off[p]:task_off[p + 1]])) for p in grew[::7]]
        keep = np.ones(len(tasks), bool)
        keep[drop] = False
        cut_off = np.concatenate([[0], np.cumsum(keep)])[task_off]
        out2, out_off2, redo2, st2 = compare(ctx, prefix, opt, so, hits, hit_off, read_len, pes, tasks[keep], cut_off, name + ", tasks left out")
        for p in grew[::7]:
            assert redo2[p] == 1, (name, p)
            for li in (2 * p, 2 * p + 1):
                assert out2[out_off2[li]:out_off2[li + 1]].tobytes() == hits[hit_off[li]:hit_off[li + 1]].tobytes(), (name, p)
        assert int(redo2.sum()) == int(redo.sum()) + len(drop) and st2[3] == int(redo2.sum())
        total["redo_by_omission"] = total.get("redo_by_omission", 0) + len(drop)
    missing = [k for k, v in total.items() if v == 0 and k != "redo"]
    assert not missing, "the inputs never reach: %s (%s)" % (missing, total)
    return total


def check_refusals(ctx, prefix):
    """§1 of the issue: bad offsets, tasks out of order / not grouped by pair, end / j / r out of range, a context without an index"""
    M = Lists(prefix, 5)
    for _ in range(6):
        M.pair(4, 0)
        M.pair(3, 2)
    hits, hit_off = M.arrays()
    n_pairs = (len(hit_off) - 1) // 2
    read_len = np.full(2 * n_pairs, READ_LEN, np.int32)
    opt, so, pes = bm2.default_opt(), bm2.default_sam_opt(), D.pestat(D.ALL4)
    tasks, task_off = bm2.pe_rescue_plan(prefix, opt, so, hits, hit_off, read_len, pes)
    tasks = fabricate(tasks, hits, hit_off, 0, 1)
    p = int(np.argmax(np.diff(task_off) >= 2))
    assert task_off[p + 1] - task_off[p] >= 2

    def refused(word, f):
        try:
            f()
        except bm2.Bm2Error as e:
            assert e.rc == bm2.BM2_EINVAL and word in str(e), (word, e)
            return
        raise AssertionError("accepted: " + word)

    def both(word, h=hits, ho=hit_off, t=tasks, to=task_off):
        refused(word, lambda: bm2.pe_rescue_apply(prefix, opt, so, h, ho, read_len, pes, t, to))
        refused(word, lambda: ctx.pe_rescue_apply(opt, so, h, ho, read_len, pes, t, to))
    bad_off = hit_off.copy()
    bad_off[1] = hit_off[2] + 1
    both("hit_off", ho=bad_off)
    refused("hit_off", lambda: bm2.pe_rescue_plan(prefix, opt, so, hits, bad_off, read_len, pes))
    bad_to = task_off.copy()
    bad_to[p + 1] = task_off[p + 2] + 1
    both("task_off", to=bad_to)
    t = tasks.copy()
    t[[task_off[p], task_off[p] + 1]] = t[[task_off[p] + 1, task_off[p]]]
    both("order", t=t)
    t = tasks.copy()
    t["pair"][task_off[p]] = p + 1
    both("grouped by pair", t=t)
    for field, value in (("end", 2), ("r", 4), ("r", -1), ("j", 50), ("j", -1)):
        t = tasks.copy()
        t[field][task_off[p + 1] - 1] = value
        both("out of range", t=t)
    bare = bm2.Context(0, None)
    try:
        refused("no index", lambda: bare.pe_rescue_apply(opt, so, hits, hit_off, read_len, pes, tasks, task_off))
    finally:
        bare.close()
    e_out, e_off, e_redo = ctx.pe_rescue_apply(opt, so, hits[:0], np.zeros(1, np.int64), read_len[:0], pes, tasks[:0], np.zeros(1, np.int64))
    assert len(e_out) == 0 and len(e_redo) == 0 and e_off.tolist() == [0]
    return True


def ref_bases(prefix):
    """the doubled reference as the host descriptor holds it (one code per base, forward then reverse complement) -> a copy"""
    ix = bm2.Index(prefix)
    try:
        n = 2 * ix.l_pac
        return np.ctypeslib.as_array((C.c_uint8 * n).from_address(ix._desc.ref_string)).copy()
    finally:
        ix.close()


def real_results(prefix, opt, tasks, enc, off, ln):
    """the results of planned tasks from bm2_ksw_align2: the mate as direction r reads it against the window (mem_matesw's call)"""
    ref = ref_bases(prefix)
    pairs, xtra = [], []
    for T in tasks:
        m = 2 * int(T["pair"]) + (1 - int(T["end"]))
        q = np.asarray(enc[off[m]:off[m] + ln[m]], np.uint8)
        if flip_of(int(T["r"])):
            q = np.where(q[::-1] < 4, 3 - q[::-1], 4).astype(np.uint8)
        pairs.append((q, ref[int(T["rb"]):int(T["re"])]))
        xtra.append(KSW_XSUBO | KSW_XSTART | (KSW_XBYTE if int(ln[m]) * opt.a < 250 else 0) | (opt.min_seed_len * opt.a))
    t = tasks.copy()
    if len(t):
        t["res"] = bm2.ksw_align2(pairs, xtra, opt)
    return t


def lines_by_pair(text):
    out = {}
    for line in text.splitlines(keepends=True):
        out.setdefault(line.split(b"\t", 1)[0], []).append(line)
    return out


def check_real_tasks(tail):
    """Item 2: bm2_pe_rescue_plan on a case's hits, results from bm2_ksw_align2, bm2_pe_rescue_apply; the grown lists through the tail
    WITHOUT rescue (-S) under the chunk's insert-size model must print what the tail's own flow prints.  A redo pair's lists come back
    as they were, so its lines are left out of the comparison; there may be no more of them than the flow's `missed`."""
    so = bm2.default_sam_opt()
    text, pes = tail.ours(0, None)
    planned, used, missed = bm2.sam_rescue_stats()
    assert planned > 0 and missed <= planned // 100, (planned, used, missed)
    tasks, task_off = bm2.pe_rescue_plan(tail.fa, tail.opt, so, tail.aln, tail.aln_off, tail.ln, pes)
    assert len(tasks) == planned, (len(tasks), planned)
    tasks = real_results(tail.fa, tail.opt, tasks, tail.enc, tail.off, tail.ln)
    out, out_off, redo = bm2.pe_rescue_apply(tail.fa, tail.opt, so, tail.aln, tail.aln_off, tail.ln, pes, tasks, task_off)
    st = bm2.sam_rescue_apply_stats()
    assert st[1] == planned and st[2] > 0 and st[3] == int(redo.sum()) <= missed, (st, planned, missed)
    grown, _ = bm2.sam_pe(tail.fa, tail.enc, tail.off, tail.ln, tail.opt, out, out_off, tail.names, tail.quals, None,
                          bm2.default_sam_opt(flag=0x20), pes_in=pes)
    a, b = lines_by_pair(text), lines_by_pair(grown)
    assert a.keys() == b.keys()
    for p in range(tail.n_pairs):
        if not redo[p]:
            assert a[b"p%d" % p] == b[b"p%d" % p], (p, a[b"p%d" % p], b[b"p%d" % p])
    return st, out, out_off, redo, tasks, task_off, pes


def check_tail(tail, extra, ctx, flag=0, combos=None, **skw):
    """Item 3: the tail with the bit (alone, with DECIDE, with DECIDE | TEXT) == without == `bwa-mem2 mem`, pes_out equal, and the
    conditions that keep the test from passing without the work."""
    ref = tail.reference(extra)
    off_text, pes_off = tail.ours(flag, ctx, **skw)
    planned, used, missed = bm2.sam_rescue_stats()
    assert ref == off_text, tail.M._diff(ref, off_text)
    assert missed <= planned // 100, (planned, used, missed)
    R, Dc, Tx = bm2.SAM_F_DEVICE_RESCUE, bm2.SAM_F_DEVICE_DECIDE, bm2.SAM_F_DEVICE_TEXT
    for bits in combos if combos is not None else (R, R | Dc, R | Dc | Tx):
        on_text, pes_on = tail.ours(flag | bits, ctx, **skw)
        assert ref == on_text, tail.M._diff(ref, on_text)
        assert [bytes(x) for x in pes_on] == [bytes(x) for x in pes_off]
        pairs, n_tasks, added, redone = bm2.sam_rescue_apply_stats()
        assert pairs == tail.n_pairs and added > 0 and n_tasks == planned and redone <= missed, (pairs, n_tasks, added, redone, planned, missed)
        assert bm2.sam_rescue_stats()[0] == planned
        if bits & Dc:
            assert bm2.sam_decide_stats()[0] == tail.n_pairs
    return ref, pes_off


def check_tail_two_contexts(tail, ctx, ctx2, part_knob):
    """the same through two contexts sharing a replica: every hook cuts the pairs into two parts"""
    for k in ("BM2_RESCUE_PART", "BM2_DECIDE_PART", "BM2_TEXT_PART"):
        os.environ[k] = str(part_knob)
    try:
        return check_tail(tail, [], [ctx, ctx2])
    finally:
        for k in ("BM2_RESCUE_PART", "BM2_DECIDE_PART", "BM2_TEXT_PART"):
            del os.environ[k]


def check_tail_refusals(tail, ctx):
    """§3: the bit without a context, with MEM_F_NO_RESCUE, with rescue_inline"""
    def refused(f):
        try:
            f()
        except bm2.Bm2Error as e:
            assert e.rc == bm2.BM2_EINVAL and "DEVICE_RESCUE" in str(e), e
            return
        raise AssertionError("accepted")
    refused(lambda: tail.ours(bm2.SAM_F_DEVICE_RESCUE, None))
    refused(lambda: tail.ours(bm2.SAM_F_DEVICE_RESCUE | 0x20, ctx))
    refused(lambda: tail.ours(bm2.SAM_F_DEVICE_RESCUE, ctx, rescue_inline=1))
    return True
