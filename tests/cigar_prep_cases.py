"""Shared by tests/test_cigar_prep_emu.py (the device sources on the host emulator), tests/test_zzzzzzzzz_cigar_prep_gpu.py (the MI355X)
and tests/test_cigar_prep_sanitizer.py: the CIGAR batch prepared on the device -- bm2_cigar_prep_dev against bm2_cigar_prep on tasks made
here (every task, the order and the totals, byte for byte), bm2_cigar_prep itself against properties that do not depend on it and against
the rule of cigar_prep.h restated below in numpy, and the SAM tails with BM2_SAM_F_DEVICE_CGPREP against the flag-off text and the compiled
reference.  Every comparison is exact; every event a check names is counted from the tasks and the restated rule, and asserted to occur."""
import ctypes as C
import os

import numpy as np

import bm2

CGPREP, CGPLAN, SEMARK, TEXT = bm2.SAM_F_DEVICE_CGPREP, bm2.SAM_F_DEVICE_CGPLAN, bm2.SAM_F_DEVICE_SEMARK, bm2.SAM_F_DEVICE_TEXT
PAIRED_SIX = bm2.SAM_F_DEVICE_TEXT | bm2.SAM_F_DEVICE_DECIDE | bm2.SAM_F_DEVICE_RESCUE | bm2.SAM_F_DEVICE_PLAN | bm2.SAM_F_DEVICE_PESTAT | bm2.SAM_F_DEVICE_CGPLAN
RING, ROW, GLOBAL, FLAT = 0, 1, 2, 3
CG_SMALL, CG_RING, RANGE_MAX = 10000, 64, 0x3fffffff
BLOCK = 256           # tasks per block of every kernel of cgprep.hip (CGP_THREADS)
L_PAC = 1 << 24
HIT_FIELDS = ("rb", "re", "read", "qb", "qe", "truesc", "w", "retry")


# ---- the rule of cigar_prep.h on arrays (int64 throughout; the two divisions in double, truncated as a C cast truncates)
class Rule:
    def __init__(self, opt, l_pac=L_PAC, no_lds=0, no_ring=0, ring_by_band=1):
        self.l_pac, self.mat0, self.a, self.w = l_pac, int(opt.mat[0]), int(opt.a), int(opt.w)
        self.o_del, self.e_del, self.o_ins, self.e_ins = int(opt.o_del), int(opt.e_del), int(opt.o_ins), int(opt.e_ins)
        self.pen = max([1] + [abs(int(v)) for v in opt.mat] + [self.o_del + self.e_del, self.o_ins + self.e_ins])
        self.no_lds, self.no_ring, self.ring_by_band = no_lds, no_ring, ring_by_band

    def band(self, lq, rlen, w_):
        half = ((lq + 1) >> 1) * self.mat0
        max_ins = np.trunc((half - self.o_ins) / float(self.e_ins) + 1.0).astype(np.int64)
        max_del = np.trunc((half - self.o_del) / float(self.e_del) + 1.0).astype(np.int64)
        max_gap = np.maximum(np.maximum(max_ins, max_del), 1)
        dl = np.abs(rlen - lq)
        return np.maximum(np.minimum((max_gap + dl + 1) >> 1, w_), dl + 3)

    def infer_bw(self, l1, l2, score, q, r):
        w = np.trunc((np.minimum(l1, l2) * self.a - score - q) / float(r) + 2.0).astype(np.int64)
        w = np.maximum(w, np.abs(l1 - l2))
        return np.where((l1 == l2) & (l1 * self.a - score < ((q + r - self.a) << 1)), 0, w)

    def first_band(self, lq, rlen, truesc, w_hit):
        w2 = np.maximum(self.infer_bw(lq, rlen, truesc, self.o_ins, self.e_ins), self.infer_bw(lq, rlen, truesc, self.o_del, self.e_del))
        return np.where(w2 > self.w, np.minimum(w2, w_hit), w2)

    def null_kind(self, lq, rb, re):
        """0 = a valid range, else which clause of cigar_range_ok fails first"""
        k = np.zeros(len(lq), np.int64)
        for code, cond in ((5, re > (self.l_pac << 1)), (4, rb < 0), (3, (rb < self.l_pac) & (re > self.l_pac)), (2, rb >= re), (1, lq <= 0)):
            k = np.where(cond, code, k)
        return k

    def __call__(self, lq, rb, re, w_hit, truesc, retry):
        """-> dict of arrays: z, e, c, m, wb_first, w_first, w0, shape, key, ok"""
        lq, rb, re, w_hit, truesc = (np.asarray(x, np.int64) for x in (lq, rb, re, w_hit, truesc))
        retry = np.asarray(retry) != 0
        ok = self.null_kind(lq, rb, re) == 0
        rlen = np.where(ok, re - rb, 1)
        q = np.where(ok, lq, 1)
        w_first = np.where(retry, self.first_band(q, rlen, truesc, w_hit), w_hit)
        flat = (q == rlen) & (w_first == 0)
        w4 = self.w << 2
        wb = self.band(q, rlen, np.where(retry, np.maximum(w_first, w4), w_hit))
        n_col = (np.minimum(q, 2 * wb + 1) + 3) & ~3
        dp = ok & ~flat
        w0 = np.where(retry, np.minimum(w_first, w4), w_hit)
        out = {"ok": ok, "flat": ok & flat, "w_first": w_first, "w0": w0, "rlen": rlen,
               "z": np.where(dp, n_col * rlen, 0), "e": np.where(dp, q + 1, 0), "c": np.where(ok, q + rlen + 2, 0), "m": np.where(ok, 2 * (q + rlen) + 16, 0),
               "wb_first": np.where(dp, self.band(q, rlen, w0), -1)}
        small = (not self.no_lds) & (q <= 220) & ((q + rlen) * self.pen < CG_SMALL)
        ring = (not self.no_ring) & (2 * out["wb_first"] + 2 <= CG_RING)
        sh = np.where(out["z"] == 0, FLAT, np.where(~small, GLOBAL, np.where(ring, RING, ROW)))
        bits = np.array([int(v).bit_length() for v in out["z"]], np.int64)
        by_band = (sh == RING) & bool(self.ring_by_band)
        out["shape"], out["small"] = sh, small
        out["key"] = np.where(by_band, sh * 64 + 31 - np.clip(out["wb_first"], 0, 31), sh * 64 + 63 - bits)
        return out

    def of_hits(self, hits):
        return self(hits["qe"].astype(np.int64) - hits["qb"], hits["rb"], hits["re"], hits["w"], hits["truesc"], hits["retry"])


# ---- reads and hits
READ_LENS = [150] * 6 + [250, 221, 220, 1000, 1500, 30000, 1, 150]


def make_reads(lens=READ_LENS, lead=17, gap=3):
    """-> (off, ln): offsets that do not start at 0 and leave gaps (only off and len of the reads are read)"""
    ln = np.array(lens, np.int32)
    off = np.zeros(len(ln), np.int64)
    at = lead
    for i, n in enumerate(ln):
        off[i] = at
        at += int(n) + gap
    return off, ln


def hit_array(rows):
    h = np.zeros(len(rows), bm2.CIGAR_HIT_DT)
    for i, r in enumerate(rows):
        for f, v in zip(HIT_FIELDS, r):
            h[f][i] = v
    return h


def read_with(ln, need):
    return int(np.flatnonzero(ln >= need)[0])


def hand_made(opt, ln):
    """the named tasks: (rb, re, read, qb, qe, truesc, w, retry); what each is for is counted in `events`"""
    H = []

    def add(q_len, rb, rlen, truesc=0, w=100, retry=0, qb=0):
        H.append((rb, rb + rlen, read_with(ln, qb + q_len), qb, qb + q_len, truesc, w, retry))
    two = L_PAC << 1
    add(100, 5000, 0); add(100, 5000, -3)                        # rb >= re
    add(0, 5000, 100)                                            # q_len == 0
    add(100, L_PAC - 50, 100)                                    # bridges l_pac
    add(100, -1, 100)                                            # rb < 0
    add(100, two - 50, 51)                                       # re > 2 l_pac
    add(100, two - 100, 100, w=5)                                # (the last valid range of the reverse strand)
    add(150, 7000, 150, w=0); add(150, 7000, 151, w=0)           # flat, and its neighbour one base longer
    add(150, 7000, 150, truesc=150, w=100, retry=1)              # flat through infer_bw's zero
    add(150, 7000, 150, truesc=140, w=100, retry=1)
    for w in (0, 1, 31, 32, 40):                                 # first bands 0, 1, 31, above; with rlen == q_len the band IS w up to 35: the ring's edge 31 | 32
        add(150, 9000, 150 + (w < 2), w=w)
        add(150, L_PAC + 9000, 150 + (w < 2), w=w)
    for q in (219, 220, 221):                                    # `small` at the query length
        add(q, 12000, q + 4, w=10, qb=1)
    # `small` at the score bound: (q_len + rlen) * pen one below, at, above CG_SMALL where pen divides it
    pen = Rule(opt).pen
    for tot in sorted({(CG_SMALL - 1) // pen, CG_SMALL // pen, CG_SMALL // pen + 1, -(-CG_SMALL // pen)}):
        add(200, 20000, tot - 200, w=20)
    for L in (255, 256):                                         # DP areas on both sides of a power of two (GLOBAL: sorted by cost): 16 columns x L rows
        add(L, 30000, L, w=6)
    for sc in range(350, 821):                                   # w_first of a retried task sweeps through opt->w << 2
        add(1000, 40000, 1000, truesc=sc, w=1000, retry=1)
    add(1000, 40000, 1010, truesc=500, w=300, retry=1)           # (w_first capped by the hit's band)
    add(1500, 50000, 1400, truesc=900, w=80, retry=1)
    return hit_array(H)


def random_hits(rng, n, ln):
    reads = rng.integers(0, len(ln), size=n)
    L = ln[reads].astype(np.int64)
    qb = (rng.random(n) * np.minimum(L, 40)).astype(np.int64)
    q_len = np.minimum(1 + (rng.random(n) * np.minimum(L, 400)).astype(np.int64), L - qb)
    d = np.where(rng.random(n) < 0.5, 0, rng.integers(-20, 60, size=n))
    rlen = np.maximum(q_len + d, np.where(rng.random(n) < 0.02, 0, 1))
    rb = np.where(rng.random(n) < 0.5, 0, L_PAC) + rng.integers(0, L_PAC - 2000, size=n)
    h = np.zeros(n, bm2.CIGAR_HIT_DT)
    h["rb"], h["re"], h["read"], h["qb"], h["qe"] = rb, rb + rlen, reads, qb, qb + q_len
    h["truesc"] = (q_len * rng.random(n)).astype(np.int64)
    h["w"] = np.where(rng.random(n) < 0.3, rng.integers(0, 40, size=n), rng.integers(40, 500, size=n))
    h["retry"] = rng.random(n) < 0.7
    return h


# ---- checks
def check_properties(rule, off, ln, hits, tasks, order, tot):
    """what holds for any batch, from the answer and the restated rule: the task fields, the permutation, the keys along it, the slices"""
    n = len(hits)
    R = rule.of_hits(hits)
    assert (tasks["q_off"] == off[hits["read"]] + hits["qb"]).all() and (tasks["q_len"] == hits["qe"] - hits["qb"]).all()
    for f in ("rb", "re", "w", "truesc", "retry"):
        assert (tasks[f] == hits[f]).all(), f
    assert sorted(order.tolist()) == list(range(n)), "order is no permutation"
    key = R["key"][order]
    assert (np.diff(key) >= 0).all(), "class keys decrease along order"
    assert ((np.diff(key) > 0) | (np.diff(order) > 0)).all(), "indices do not ascend within a key"
    for f, size, total in (("z_off", "z", "z_bytes"), ("eh_off", "e", "eh_items"), ("cg_off", "c", "cg_items"), ("md_off", "m", "md_bytes")):
        o = tasks[f].astype(np.int64)
        assert n == 0 or o[0] == 0, f
        assert (np.diff(o) >= R[size][:-1]).all(), (f, "a slice is smaller than the rule's size or out of task order")
        assert int(tot[total]) >= (int(o[-1]) + int(R[size][-1]) if n else 0), total
    assert (tasks["z_off"] % 4 == 0).all()
    ns = [int((R["shape"] == k).sum()) for k in range(4)]
    assert [int(v) for v in tot["n_shape"]] == ns and sum(ns) == n, (tot["n_shape"], ns)
    lds = (R["shape"] == RING) | (R["shape"] == ROW)
    assert int(tot["qmax"]) == (int(tasks["q_len"][lds].max()) if lds.any() else 0)
    return R


def compare(ctx, opt, off, ln, hits, rule=None, what=""):
    """device == host: tasks, order, totals; the host's answer has the properties -> (tasks, order, tot, R)"""
    th, oh, toth = bm2.cigar_prep(opt, L_PAC, off, ln, hits)
    td, od, totd = ctx.cigar_prep(opt, L_PAC, off, ln, hits)
    if td.tobytes() != th.tobytes():
        for f in bm2.CIGAR_TASK_DT.names:
            bad = np.flatnonzero(td[f] != th[f])
            assert len(bad) == 0, (what, f, bad[:5], td[f][bad[:5]], th[f][bad[:5]])
    assert (od == oh).all(), (what, "order", np.flatnonzero(od != oh)[:5])
    assert totd.tobytes() == toth.tobytes(), (what, totd, toth)
    n = len(hits)
    if n:
        t, sh, up, fb = bm2.sam_cigar_prep_stats()
        assert (t, sum(sh), fb, up) == (n, n, 0, 40 * n + 12 * len(ln)), (what, t, sh, up, fb)
    R = check_properties(rule or Rule(opt), off, ln, hits, th, oh, toth)
    return th, oh, toth, R


def events(rule, hits, R, off, seen):
    def note(k, c=1):
        if c:
            seen[k] = seen.get(k, 0) + int(c)
    lq = hits["qe"].astype(np.int64) - hits["qb"]
    for k, nm in enumerate(("shape_ring", "shape_row", "shape_global", "shape_flat")):
        note(nm, (R["shape"] == k).sum())
    kind = rule.null_kind(lq, hits["rb"].astype(np.int64), hits["re"].astype(np.int64))
    for k, nm in ((1, "null_q_len_0"), (2, "null_rb_ge_re"), (3, "null_bridges_l_pac"), (4, "null_rb_negative"), (5, "null_re_past_2_l_pac")):
        note(nm, (kind == k).sum())
        assert (R["shape"][kind == k] == FLAT).all()
    note("retry_0", (hits["retry"] == 0).sum()); note("retry_1", (hits["retry"] != 0).sum())
    note("flat_case", R["flat"].sum())
    note("flat_neighbour", (R["ok"] & (R["rlen"] == lq + 1) & (R["w_first"] == 0) & (R["z"] > 0)).sum())
    small_ok = R["small"] & (R["z"] > 0)
    note("ring_edge_31", (small_ok & (R["wb_first"] == 31) & (R["shape"] == RING)).sum())
    note("ring_edge_32", (small_ok & (R["wb_first"] == 32) & (R["shape"] == ROW)).sum())
    note("small_q_220", (R["ok"] & (lq == 220) & (R["shape"] != GLOBAL)).sum())
    note("small_q_221", (R["ok"] & (lq == 221) & (R["shape"] == GLOBAL)).sum())
    sc = (lq + R["rlen"]) * rule.pen
    note("small_score_below", (R["ok"] & (lq <= 220) & (sc == CG_SMALL - 1) & (R["shape"] != GLOBAL)).sum())
    note("small_score_at", (R["ok"] & (lq <= 220) & (sc == CG_SMALL) & (R["shape"] == GLOBAL)).sum())
    dp = R["z"] > 0
    for b, nm in ((0, "first_band_0"), (1, "first_band_1"), (31, "first_band_31")):
        note(nm, (dp & (R["w0"] == b)).sum())
    note("first_band_above_31", (dp & (R["w0"] > 31)).sum())
    by_cost = dp & (R["shape"] != RING)
    z = R["z"]
    note("area_pow2_at", (by_cost & ((z & (z - 1)) == 0)).sum())
    bl = lambda v: np.array([int(x).bit_length() for x in v], np.int64)
    note("area_pow2_below", (by_cost & (bl(z + 16) > bl(z)) & ((z & (z - 1)) != 0)).sum())       # (the next class is 16 bytes away)
    rt = (hits["retry"] != 0) & dp
    w4 = rule.w << 2
    note("w_first_below_4w", (rt & (R["w_first"] == w4 - 1)).sum()); note("w_first_at_4w", (rt & (R["w_first"] == w4)).sum()); note("w_first_above_4w", (rt & (R["w_first"] == w4 + 1)).sum())
    if (rule.o_del, rule.e_del) != (rule.o_ins, rule.e_ins):
        a = rule.infer_bw(lq[rt], R["rlen"][rt], hits["truesc"][rt].astype(np.int64), rule.o_del, rule.e_del)
        b = rule.infer_bw(lq[rt], R["rlen"][rt], hits["truesc"][rt].astype(np.int64), rule.o_ins, rule.e_ins)
        note("divisions_differ", (a != b).sum())
    note("read_off_not_from_0", int(off[0] != 0))
    note("q_off_inside_read", (hits["qb"] > 0).sum())


# default; gaps that differ with pen = 9 (9999 = 9 x 1111: one below CG_SMALL); pen = 10 (10000 = 10 x 1000: at CG_SMALL) and another band option
OPTION_SETS = [{}, dict(o_del=7, e_del=2, o_ins=6, e_ins=1), dict(o_del=6, e_del=1, o_ins=8, e_ins=2, w=50)]
WANTED = ["shape_ring", "shape_row", "shape_global", "shape_flat", "null_q_len_0", "null_rb_ge_re", "null_bridges_l_pac", "null_rb_negative",
          "null_re_past_2_l_pac", "retry_0", "retry_1", "flat_case", "flat_neighbour", "ring_edge_31", "ring_edge_32", "small_q_220", "small_q_221",
          "small_score_below", "small_score_at", "first_band_0", "first_band_1", "first_band_31", "first_band_above_31", "area_pow2_at",
          "area_pow2_below", "w_first_below_4w", "w_first_at_4w", "w_first_above_4w", "divisions_differ", "read_off_not_from_0", "q_off_inside_read"]


def check_tasks(ctx, quick=False, knobs=None):
    """bm2_cigar_prep_dev against bm2_cigar_prep on the named tasks and random ones under every option set.  knobs: what the environment of
    this process sets of (no_lds, no_ring, ring_by_band), for the restated rule"""
    total = {}
    off, ln = make_reads()
    for k, okw in enumerate(OPTION_SETS):
        opt = bm2.default_opt(**okw)
        rule = Rule(opt, **(knobs or {}))
        rng = np.random.default_rng(500 + k)
        hits = np.concatenate([hand_made(opt, ln), random_hits(rng, 700 if quick else 5000, ln)])
        rng.shuffle(hits)
        _, _, _, R = compare(ctx, opt, off, ln, hits, rule, "set %d" % k)
        seen = {}
        events(rule, hits, R, off, seen)
        for ev, c in seen.items():
            total[ev] = total.get(ev, 0) + c
    if not knobs:
        missing = [ev for ev in WANTED if not total.get(ev)]
        assert not missing, (missing, total)
    return total


def varied_pool(rng, ln, opt, n=4000):
    """one task per class key the rule can give these reads (the device form's sizes stay below 2^31, and a FLAT task has one key)"""
    h = random_hits(rng, n, ln)
    big = np.flatnonzero(ln >= 30000)[0]
    extra = []
    for q in (300, 1000, 5000, 30000):
        for d in (0, 50, 3000, 40000):
            extra.append((1000, 1000 + q + d, big, 0, q, 0, 1000000, 0))
    for b in range(3, 36):
        extra.append((1000, 1150, 0, 0, 150, 0, b, 0))
    for q, d in ((4, 30), (10, 30), (30, 40), (100, 200), (200, 900)):
        extra.append((1000, 1000 + q + d, read_with(ln, q), 0, q, 0, 2000, 0))
    h = np.concatenate([h, hit_array(extra)])
    key = Rule(opt).of_hits(h)["key"]
    _, first = np.unique(key, return_index=True)
    return h[np.sort(first)]


def check_batches(ctx, quick=False):
    """n = 0, 1, 63, 64, 65, around the block of 256, several blocks; one class for a whole batch; every class the rule can give in every
    block; and (not under quick) 70 000 tasks: 274 blocks, whose [256][274] counts take 35 blocks of the scan"""
    opt = bm2.default_opt()
    off, ln = make_reads()
    rng = np.random.default_rng(77)
    done = []
    for n in (0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 4 * BLOCK + 3):
        compare(ctx, opt, off, ln, random_hits(rng, n, ln), None, "%d tasks" % n)
        done.append(n)
    one = hit_array([(1000, 1150, 0, 0, 150, 0, 9, 0)] * (3 * BLOCK + 5))       # every lane of a block shares a key
    _, order, tot, R = compare(ctx, opt, off, ln, one, None, "one class")
    assert (order == np.arange(len(one))).all() and len(set(R["key"].tolist())) == 1
    pool = varied_pool(rng, ln, opt)
    assert len(pool) >= 30, len(pool)
    cyc = pool[np.arange(5 * BLOCK + 9) % len(pool)]                            # every key present in every block
    _, order, tot, R = compare(ctx, opt, off, ln, cyc, None, "classes cycling")
    assert all(int(tot["n_shape"][k]) > 0 for k in range(4)), tot
    for b in range(5):
        assert set(R["key"][b * BLOCK:(b + 1) * BLOCK].tolist()) == set(R["key"].tolist())
    done.append("cycling %d keys" % len(pool))
    if not quick:
        big = np.concatenate([random_hits(rng, 70000 - len(pool), ln), pool])
        rng.shuffle(big)
        compare(ctx, opt, off, ln, big, None, "70 000 tasks")
        done.append(70000)
    return done


def _raw(fn, head, opt, l_pac, reads, n, hits, tasks, order, tot):
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(None)
    return fn(*head, C.byref(opt) if opt is not None else None, C.c_int64(l_pac), C.byref(reads) if reads is not None else None, C.c_int32(n), p(hits), p(tasks), p(order), p(tot))


def big_area_hits(ln):
    """q_len 30 000 against a range of 80 000 with a band wider than the query: 30 000 columns x 80 000 rows = 2.4e9 bytes of directions"""
    return hit_array([(1000, 1150, 0, 0, 150, 0, 9, 0), (2000, 82000, read_with(ln, 30000), 0, 30000, 0, 100000, 0), (1000, 1150, 0, 0, 150, 0, 9, 0)])


def check_arguments(ctx):
    """every BM2_EINVAL / BM2_EUNSUP of the contract in both forms, the lowest offender named; n == 0; the 2^31 case"""
    L = bm2.lib()
    L.bm2_cigar_prep.restype = L.bm2_cigar_prep_dev.restype = C.c_int
    opt = bm2.default_opt()
    off, ln = make_reads()
    rng = np.random.default_rng(5)
    hits = random_hits(rng, 600, ln)
    reads = bm2.Reads(len(ln), None, off.ctypes.data, ln.ctypes.data)
    forms = (("bm2_cigar_prep", L.bm2_cigar_prep, ()), ("bm2_cigar_prep_dev", L.bm2_cigar_prep_dev, (C.c_void_p(ctx.h),)))
    want = bm2.cigar_prep(opt, L_PAC, off, ln, hits)
    for who, fn, head in forms:
        def fresh():
            return np.full(len(hits), 7, bm2.CIGAR_TASK_DT), np.full(len(hits), -7, np.int32), np.full(1, 7, bm2.CIGAR_PREP_DT)

        def refused(rc, word, o=opt, r=reads, n=len(hits), h=hits, drop=None, lp=L_PAC, touched_ok=False):
            t, od, tt = fresh()
            a = [t, od, tt]
            if drop is not None:
                a[drop] = None
            got = _raw(fn, head, o, lp, r, n, h, *a)
            assert got == rc, (who, word, got, L.bm2_last_error())
            assert word.encode() in L.bm2_last_error() and who.encode() in L.bm2_last_error(), (who, word, L.bm2_last_error())
            f = fresh()
            assert all(x.tobytes() == y.tobytes() for x, y in zip((t, od, tt), f)), (who, word, "a refused call wrote")
        refused(bm2.BM2_EINVAL, "bad argument", o=None)
        refused(bm2.BM2_EINVAL, "bad argument", r=None)
        refused(bm2.BM2_EINVAL, "bad argument", h=None)
        for drop in (0, 1, 2):
            refused(bm2.BM2_EINVAL, "bad argument", drop=drop)
        refused(bm2.BM2_EINVAL, "bad argument", n=-1)
        refused(bm2.BM2_EINVAL, "gap extension", o=bm2.default_opt(e_del=0))
        refused(bm2.BM2_EINVAL, "gap extension", o=bm2.default_opt(e_ins=-1))
        odd = bm2.default_opt()
        odd.mat[7] = -3
        refused(bm2.BM2_EUNSUP, "bwa_fill_scmat", o=odd)
        # an offender first, in the middle and last, a second one after it: the lowest is named
        offenders = (("read", -1), ("read", len(ln)), ("qb", -1), ("qe", None), ("qb", None))
        for k, (f, v) in enumerate(offenders):
            for at in (0, len(hits) // 2, len(hits) - 1):
                bad = hits.copy()
                for j in {at, min(at + 3, len(hits) - 1), len(hits) - 1}:
                    if v is not None:
                        bad[f][j] = v
                    elif f == "qe":
                        bad["qe"][j] = ln[bad["read"][j]] + 1
                    else:
                        bad["qb"][j] = bad["qe"][j] + 1
                refused(bm2.BM2_EINVAL, "task %d names" % at, h=bad)
        long_ = hits.copy()                                      # a valid range of 2^30 bases
        long_["rb"][5], long_["re"][5] = 0, RANGE_MAX + 1
        refused(bm2.BM2_EINVAL, "reference range too long", h=long_, lp=1 << 32)
        ok_ = hits.copy()
        ok_["rb"][5], ok_["re"][5] = 0, RANGE_MAX
        if not head:                                             # (the longest range the host form takes; on the device its slices pass 2^31)
            t, od, tt = fresh()
            assert _raw(fn, head, opt, 1 << 32, reads, len(hits), ok_, t, od, tt) == bm2.BM2_OK, L.bm2_last_error()
        t, od, tt = fresh()                                      # no task: success, nothing touched, whatever else is passed
        assert _raw(fn, head, opt, L_PAC, reads, 0, None, None, None, tt) == bm2.BM2_OK, (who, L.bm2_last_error())
        assert tt.tobytes() == fresh()[2].tobytes()
        t, od, tt = fresh()
        assert _raw(fn, head, opt, L_PAC, reads, len(hits), hits, t, od, tt) == bm2.BM2_OK, (who, L.bm2_last_error())
        assert t.tobytes() == want[0].tobytes() and (od == want[1]).all() and tt[0].tobytes() == want[2].tobytes(), who
    # the 2^31 case: the area by the header's formulas, confirmed on the host form first; the device form refuses it
    big = big_area_hits(ln)
    R = Rule(opt).of_hits(big)
    assert int(R["z"][1]) == 30000 * 80000 >= 1 << 31
    tasks, order, tot = bm2.cigar_prep(opt, L_PAC, off, ln, big)
    assert int(tasks["z_off"][2]) - int(tasks["z_off"][1]) == 30000 * 80000 and int(tot["z_bytes"]) == 30000 * 80000 + 2 * int(R["z"][0])
    check_properties(Rule(opt), off, ln, big, tasks, order, tot)
    try:
        ctx.cigar_prep(opt, L_PAC, off, ln, big)
    except bm2.Bm2Error as e:
        assert e.rc == bm2.BM2_EUNSUP and "task 1 " in str(e) and "2^31" in str(e), e
    else:
        raise AssertionError("the device form took a DP area of 2^31 bytes")
    bare = bm2.Context(0, None)                                  # a context without an index will do
    try:
        got = bare.cigar_prep(opt, L_PAC, off, ln, hits)
        assert got[0].tobytes() == want[0].tobytes() and (got[1] == want[1]).all()
    finally:
        bare.close()
    return True


def check_knob(ctx, name):
    """one of the three launch knobs, set in this process's environment before the library read it: both forms follow it, as the rule restated
    with the knob does"""
    knobs = {"BM2_CIGAR_NO_LDS": dict(no_lds=1), "BM2_CIGAR_NO_RING": dict(no_ring=1), "BM2_CIGAR_RING_BY_BAND": dict(ring_by_band=0)}[name]
    assert os.environ.get(name) == ("0" if name == "BM2_CIGAR_RING_BY_BAND" else "1")
    tot = check_tasks(ctx, quick=True, knobs=knobs)
    if name == "BM2_CIGAR_NO_LDS":
        assert not tot.get("shape_ring") and not tot.get("shape_row") and tot["shape_global"] > 0
    if name == "BM2_CIGAR_NO_RING":
        assert not tot.get("shape_ring") and tot["shape_row"] > 0
    if name == "BM2_CIGAR_RING_BY_BAND":
        assert tot["shape_ring"] > 0
    return sorted(tot.items())


def dump_tasks(path):
    """the hand-made tasks under every option set, as tools/san/cigar_prep_san.cpp reads them: a header (batches, the sizes of bm2_opt and
    of the three records), then per batch the options, (l_pac, reads, tasks), the reads' offsets and lengths, the hits -> batches"""
    off, ln = make_reads()
    sets = []
    for k, okw in enumerate(OPTION_SETS):
        opt = bm2.default_opt(**okw)
        rng = np.random.default_rng(500 + k)
        hits = np.concatenate([hand_made(opt, ln), random_hits(rng, 300, ln), big_area_hits(ln)])
        sets.append((opt, hits))
    with open(path, "wb") as f:
        f.write(np.array([len(sets), C.sizeof(bm2.Opt), 40, 72, 56], np.int64).tobytes())
        for opt, hits in sets:
            f.write(bytes(opt))
            f.write(np.array([L_PAC, len(ln), len(hits)], np.int64).tobytes())
            f.write(off.tobytes() + ln.tobytes() + hits.tobytes())
    return len(sets)


# ---- the tails with the bit
def _prep_stats_of(planned, n_reads, parts):
    t, sh, up, fb = bm2.sam_cigar_prep_stats()
    assert t == planned and sum(sh) == t and fb == 0, (t, sh, fb, planned)
    assert up == 40 * t + 12 * n_reads * parts, (up, t, n_reads, parts)


def check_se_tail(T, M, d, make_ctx, n_reads):
    """bm2_sam_se_dev / _multi with the bit alone, with CGPLAN, with SEMARK | CGPLAN | TEXT against the flag-off text, its planned / used /
    missed and the reference; bm2_sam_se refuses it.  M = se_mark_cases (its SeTail)"""
    tail = M.SeTail(T, d, n_reads)
    ctx = make_ctx(tail.fa)
    ctx2 = bm2.Context(0, share=ctx)
    ref = T._reference_sam(tail.fa, tail.fq, [])
    knobs = ("BM2_CIGAR_PART", "BM2_SEMARK_PART", "BM2_CGPLAN_PART", "BM2_TEXT_PART")
    try:
        off_text = tail.ours(0, ctx)
        st_off = bm2.sam_cigar_stats()
        assert ref == off_text, T._diff(ref, off_text)
        assert st_off[0] > 10
        for k in knobs:
            os.environ[k] = str(max(st_off[0] // 3, 1) if k == "BM2_CIGAR_PART" else n_reads // 3)
        for bits in (CGPREP, CGPREP | CGPLAN, CGPREP | SEMARK | CGPLAN | TEXT):
            for cx, parts in ((ctx, 1), ([ctx, ctx2], 2)):
                on_text = tail.ours(bits, cx)
                assert ref == on_text, (bits, T._diff(ref, on_text))
                assert bm2.sam_cigar_stats() == st_off, (bits, bm2.sam_cigar_stats(), st_off)
                _prep_stats_of(st_off[0], len(tail.reads), parts)
        try:
            tail.ours(CGPREP, None)
        except bm2.Bm2Error as e:
            assert e.rc == bm2.BM2_EINVAL and "BM2_SAM_F_DEVICE_CGPREP" in str(e) and "needs a context" in str(e), e
        else:
            raise AssertionError("bm2_sam_se accepted the bit")
    finally:
        for k in knobs:
            os.environ.pop(k, None)
        ctx2.close()
    return True


def check_pe_tail(tail, ctx, ctx2):
    """bm2_sam_pe_dev / _multi with the bit alone, with CGPLAN, with all six paired bits.  tail = pe_decide_cases.PeTail"""
    ref = tail.reference([])
    knobs = ("BM2_CIGAR_PART", "BM2_CGPLAN_PART", "BM2_TEXT_PART", "BM2_PLAN_PART", "BM2_KSW_PART")
    try:
        off_text, pes_off = tail.ours(0, ctx)
        st_off = bm2.sam_cigar_stats()
        assert ref == off_text, tail.M._diff(ref, off_text)
        assert st_off[0] > 10
        for k in knobs:
            os.environ[k] = str(max(st_off[0] // 3, 1) if k == "BM2_CIGAR_PART" else max(tail.n_pairs // 3, 1))
        for bits in (CGPREP, CGPREP | CGPLAN, CGPREP | PAIRED_SIX):
            for cx, parts in ((ctx, 1), ([ctx, ctx2], 2)):
                if bits & ~CGPREP:                               # (the same bits without this one: its flag-off call)
                    base, _ = tail.ours(bits & ~CGPREP, cx)
                    assert base == ref
                    st_off = bm2.sam_cigar_stats()
                on_text, pes_on = tail.ours(bits, cx)
                assert ref == on_text, (bits, tail.M._diff(ref, on_text))
                assert bm2.sam_cigar_stats() == st_off, (bits, bm2.sam_cigar_stats(), st_off)
                assert [bytes(x) for x in pes_on] == [bytes(x) for x in pes_off]
                _prep_stats_of(st_off[0], 2 * tail.n_pairs, parts)
        try:
            tail.ours(CGPREP, None)
        except bm2.Bm2Error as e:
            assert e.rc == bm2.BM2_EINVAL and "BM2_SAM_F_DEVICE_CGPREP" in str(e) and "needs a context" in str(e), e
        else:
            raise AssertionError("bm2_sam_pe accepted the bit")
    finally:
        for k in knobs:
            os.environ.pop(k, None)
    return True


def tail_phases(T, M, d, make_ctx, n_reads):
    """one single-end call with the bit (for BM2_TAIL_PROF=1 in the environment: the caller reads stderr)"""
    tail = M.SeTail(T, d, n_reads)
    tail.ours(CGPREP, make_ctx(tail.fa))
    return bm2.sam_cigar_prep_stats()
