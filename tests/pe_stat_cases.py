"""Shared by tests/test_pe_stat_emu.py (the device sources on the host emulator) and tests/test_zzzzzz_pe_stat_gpu.py (the MI355X): the
chunk's insert-size model counted on the device -- bm2_pe_stat_dev against bm2_pe_stat (pestat() of the host tail behind a C name) on
lists made here, bin for bin and model for model, and the tail with BM2_SAM_F_DEVICE_PESTAT (alone and with the plan bit and its
companions) against the flag-off tail and the compiled reference.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np

import bm2
import pe_decide_cases as D

PESTAT, PLAN, RESCUE, DECIDE, TEXT = bm2.SAM_F_DEVICE_PESTAT, bm2.SAM_F_DEVICE_PLAN, bm2.SAM_F_DEVICE_RESCUE, bm2.SAM_F_DEVICE_DECIDE, bm2.SAM_F_DEVICE_TEXT
COMBOS = [0, PLAN, PLAN | RESCUE, PLAN | RESCUE | DECIDE | TEXT]
PART_KNOBS = ("BM2_PLAN_PART", "BM2_KSW_PART", "BM2_RESCUE_PART", "BM2_DECIDE_PART", "BM2_TEXT_PART")
HIT_BYTES = bm2.ALNREG_DT.itemsize
BLOCK = 256           # lanes of a k_pestat block (pestat.hip)


def same_pes(a, b):
    return [bytes(x) for x in a] == [bytes(x) for x in b]


def infer_dir(l_pac, b1, b2):
    """mem_infer_dir, bwamem_pair.cpp:58-65"""
    r1, r2 = b1 >= l_pac, b2 >= l_pac
    p2 = b2 if r1 == r2 else 2 * l_pac - 1 - b2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), (p2 - b1 if p2 > b1 else b1 - p2)


def cal_sub(opt, a, ev):
    """cal_sub, bwamem_pair.cpp:67-79, with the overlap test in float32 as the C code has it; ev collects what was met"""
    m = np.float32(opt.mask_level)
    qb0, qe0 = int(a["qb"][0]), int(a["qe"][0])
    for j in range(1, len(a)):
        qb, qe = int(a["qb"][j]), int(a["qe"][j])
        b_max, e_min = max(qb, qb0), min(qe, qe0)
        if e_min > b_max:
            min_l = min(qe - qb, qe0 - qb0)
            need = np.float32(min_l) * m                        # one float32 product
            ov = e_min - b_max
            ok = bool(np.float32(ov) >= need)
            if ok != (float(ov) >= float(min_l) * float(m)):
                ev.add("float_matters")
            if ok and not np.float32(ov - 1) >= need:
                ev.add("overlap_at_threshold")
            if not ok and np.float32(ov + 1) >= need:
                ev.add("overlap_one_less")
            if ok:
                ev.add("sub_j1" if j == 1 else "sub_last" if j == len(a) - 1 else "sub_mid")
                return int(a["score"][j])
    if len(a) > 1:
        ev.add("sub_absent")
    return opt.min_seed_len * opt.a


def stat_in_python(l_pac, opt, so, hits, hit_off, skip_above=200):
    """the counting half of pestat() written again with Python numbers -> (hist[4, max(max_ins, 0) + 1], events, pairs left out).
    Pairs with a list above skip_above hits are left out of the events AND counted by the caller from the host's result only."""
    top = max(int(so.max_ins), 0)
    hist = np.zeros((4, top + 1), np.int64)
    seen, left_out = {}, []

    def note(k):
        seen[k] = seen.get(k, 0) + 1
    for p in range((len(hit_off) - 1) // 2):
        a = [hits[hit_off[2 * p + e]:hit_off[2 * p + e + 1]] for e in range(2)]
        if max(len(a[0]), len(a[1])) > skip_above:
            left_out.append(p)
            continue
        if not len(a[0]) or not len(a[1]):
            note("both_empty" if not len(a[0]) and not len(a[1]) else "first_empty" if not len(a[0]) else "second_empty")
            continue
        unique = True
        for e in range(2):
            ev = set()
            sub, score = cal_sub(opt, a[e], ev), int(a[e]["score"][0])
            for k in ev:
                note(k)
            if len(a[e]) == 1:
                note("sub_default_rejects" if sub > 0.8 * score else "sub_default_passes")
            if 5 * sub == 4 * score:
                note("sub_is_0.8_score")
            if sub > 0.8 * score:                               # a double product, as the C code has it
                note("sub_above")
                unique = False
                break
        if not unique:
            continue
        if int(a[0]["rid"][0]) != int(a[1]["rid"][0]):
            note("rid_differs")
            continue
        b1, b2 = int(a[0]["rb"][0]), int(a[1]["rb"][0])
        d, dist = infer_dir(l_pac, b1, b2)
        note("dir%d_%s" % (d, "rev" if b1 >= l_pac else "fwd"))
        if (b1 >= l_pac) != (b2 >= l_pac):
            note("across_l_pac")
        if dist == 0:
            note("dist_0")
        elif dist == top:
            note("dist_max_ins")
        elif dist == top + 1:
            note("dist_max_ins_plus_1")
        if dist and dist <= top:
            hist[d, dist] += 1
            note("counted")
    return hist, seen, left_out


def compare(ctx, prefix, opt, so, hits, hit_off, what=""):
    """bm2_pe_stat_dev against bm2_pe_stat: every bin, the four models, the counters -> the host's (pes, hist)"""
    h_pes, h_hist = bm2.pe_stat(prefix, opt, so, hits, hit_off)
    d_pes, d_hist = ctx.pe_stat(opt, so, hits, hit_off)
    st = bm2.sam_pestat_stats()
    assert h_hist.shape == d_hist.shape == (4, max(int(so.max_ins), 0) + 1), (what, h_hist.shape, d_hist.shape)
    if (h_hist != d_hist).any():
        d, v = [int(x[0]) for x in np.nonzero(h_hist != d_hist)]
        assert False, "%s: bin [%d][%d] holds %d on the host, %d on the device (%d bins differ)" % (what, d, v, h_hist[d, v], d_hist[d, v], int((h_hist != d_hist).sum()))
    assert same_pes(h_pes, d_pes), "%s:\n  host   %s\n  device %s" % (what, [(x.low, x.high, x.failed, x.avg, x.std) for x in h_pes], [(x.low, x.high, x.failed, x.avg, x.std) for x in d_pes])
    n_pairs = (len(hit_off) - 1) // 2
    n_hits = int(hit_off[-1] - hit_off[0])
    want_up = n_hits * HIT_BYTES if n_pairs and so.max_ins > 0 else 0
    assert st == (n_pairs, int(h_hist.sum()), want_up, 0), (what, st, n_pairs, int(h_hist.sum()), want_up)
    d_only, none = ctx.pe_stat(opt, so, hits, hit_off, hist=False)                   # NULL hist: the same models
    assert none is None and same_pes(d_only, h_pes), what
    return h_pes, h_hist


class Lists(D.Maker):
    """pe_decide_cases.Maker plus hits placed by their rb"""

    def at(self, rb, rid, qb, qe, score):
        h = self.hit(0, 0, False, qb, qe, score)
        h["rb"], h["re"], h["rid"] = rb, rb + (qe - qb), rid
        return h

    def simple(self, b1, b2, rid1=0, rid2=0, score=100):
        """one unique hit an end"""
        self.end_list([self.at(b1, rid1, 0, 100, score)])
        self.end_list([self.at(b2, rid2, 0, 100, score)])

    def oriented(self, d, dist, b1):
        """a pair of direction d at distance dist whose first read's best hit lies at b1 (either strand); False where the doubled
        reference has no such place"""
        l2 = 2 * self.l_pac
        p2 = b1 + dist if d in (0, 1) else b1 - dist
        if d in (1, 2):
            p2 = l2 - 1 - p2
        if not 0 <= p2 < l2 or infer_dir(self.l_pac, b1, p2) != (d, dist):
            return False
        self.simple(b1, p2)
        return True


def hand_made(M, opt, top):
    """the lists of the issue's item 1 for min_seed_len / a / mask_level of `opt` and bins up to `top` (> 0)"""
    l_pac = M.l_pac
    msl = opt.min_seed_len * opt.a
    # list shape
    M.end_list([]); M.end_list([])
    M.end_list([]); M.end_list([M.at(500, 0, 0, 100, 90)])
    M.end_list([M.at(500, 0, 0, 100, 90)]); M.end_list([])
    # the default sub-score at its boundary: 0.8 * score against min_seed_len * a, one score below and the first that passes
    lo = next(s for s in range(1, 1000) if not msl > 0.8 * s)
    for s in (lo - 1, lo):
        M.simple(1000, 1000 + min(200, top), score=s)
    # a sub-score exactly 0.8 * score and one above, for every score that is a multiple of 5 from 5 to 250
    for s in range(5, 255, 5):
        for sub in (4 * s // 5, 4 * s // 5 + 1):
            M.end_list([M.at(3000 + s, 1, 0, 100, s), M.at(9000, 1, 0, 100, sub)])
            M.end_list([M.at(3000 + s + min(150, top), 1, 0, 100, 300)])
    # the first overlapping hit at j = 1, at j = last, absent (with the two that do not overlap scoring above 0.8 * score: they must not count)
    far = [M.at(20000 + k, 2, 100, 150, 99) for k in range(2)]
    near = M.at(20100, 2, 10, 90, 30)
    for lst in ([near] + far, far + [near], far):
        M.end_list([M.at(2000, 2, 0, 100, 100)] + [h.copy() for h in lst])
        M.end_list([M.at(2000 + min(300, top), 2, 0, 100, 100)])
    # an overlap exactly min_l * mask_level and one base less, for spans where the float product is and is not exact
    for min_l in (10, 20, 60, 100, 150):
        need = float(np.float32(min_l) * np.float32(opt.mask_level))
        first = int(np.ceil(need))
        for ov in (first, first - 1):
            if ov < 1:
                continue
            # the best hit spans [0, 200); hit 1 spans [200 - ov, 200 - ov + min_l): they share ov bases
            M.end_list([M.at(5000, 0, 0, 200, 100), M.at(7000, 0, 200 - ov, 200 - ov + min_l, 95)])
            M.end_list([M.at(5000 + min(250, top), 0, 0, 100, 100)])
    # one pair with 500 hits an end whose only overlap is the last (sub-score 10: unique), and the same with a last hit that scores 90
    for last_score in (10, 90):
        for_end = lambda base: [M.at(base, 3, 0, 100, 100)] + [M.at(base + 7 * k, 3, 100, 160, 99) for k in range(1, 499)] + [M.at(base + 9, 3, 50, 150, last_score)]
        M.end_list(for_end(30000)); M.end_list(for_end(30000 + min(400, top)))
    # contig and direction
    M.simple(8000, 8000 + min(100, top), rid1=0, rid2=1)
    for b1 in (700, l_pac - 1, l_pac, l_pac + 700, 2 * l_pac - 1, 0, l_pac - 40, l_pac + 40):
        for d in range(4):
            for dist in sorted({0, 1, 2, 37, top - 1, top, top + 1, min(top, l_pac - 1), min(top, l_pac - 2)}):      # (two places of one strand are less than l_pac apart)
                if dist >= 0:
                    M.oriented(d, dist, b1)
    return M


def random_pairs(M, n, top, max_hits=12):
    """n pairs of lists of 0 .. max_hits hits whose best hits lie anywhere on the doubled reference, mostly within `top` of each other"""
    rng = M.rng
    l2 = 2 * M.l_pac
    for _ in range(n):
        b1 = int(rng.integers(0, l2))
        if rng.random() < 0.7:
            d, dist = int(rng.integers(0, 4)), int(rng.integers(0, top + 3))
            if not M.oriented(d, dist, b1):
                M.simple(b1, int(rng.integers(0, l2)))
            lists = [M.hits[M.hit_off[-3]:M.hit_off[-2]], M.hits[M.hit_off[-2]:M.hit_off[-1]]]
            del M.hits[M.hit_off[-3]:]
            del M.hit_off[-2:]
        else:
            lists = [[M.at(b1, int(rng.integers(0, 2)), 0, 100, 100)], [M.at(int(rng.integers(0, l2)), int(rng.integers(0, 2)), 0, 100, 100)]]
        for e in range(2):
            k = int(rng.integers(0, max_hits + 1))
            if k == 0 and rng.random() < 0.5:
                lists[e] = []
            best = lists[e][0] if lists[e] else None
            for _j in range(k if best is not None else 0):
                qb = int(rng.integers(0, 120))
                qe = qb + int(rng.integers(5, 120))
                lists[e].append(M.at(int(rng.integers(0, l2)), int(rng.integers(0, 3)), qb, qe, int(rng.integers(10, 101))))
            M.end_list(lists[e])
    return M


def check_lists(ctx, prefix, quick=False):
    """Item 1 of the issue.  quick: the emulator's share (fewer random pairs per configuration)."""
    with bm2.Index(prefix) as ix:
        l_pac = ix.l_pac
    need = ["both_empty", "first_empty", "second_empty", "sub_default_rejects", "sub_default_passes", "sub_is_0.8_score", "sub_above", "sub_j1", "sub_last",
            "sub_absent", "overlap_at_threshold", "overlap_one_less", "rid_differs", "across_l_pac", "dist_0", "dist_max_ins", "dist_max_ins_plus_1", "counted"] + \
           ["dir%d_%s" % (d, s) for d in range(4) for s in ("fwd", "rev")]
    configs = [("max_ins 500", {}, dict(max_ins=500)), ("max_ins 10000", {}, dict(max_ins=10000)), ("max_ins 70000", {}, dict(max_ins=70000)),
               ("max_ins 1", {}, dict(max_ins=1)), ("mask_level 0.3", dict(mask_level=0.3), dict(max_ins=500)),
               ("min_seed_len 19, a 1", dict(min_seed_len=19, a=1), dict(max_ins=500)), ("min_seed_len 30, a 2", dict(min_seed_len=30, a=2), dict(max_ins=500))]
    n_random = 150 if quick else 1500
    total = {}
    for ci, (name, okw, skw) in enumerate(configs):
        opt, so = bm2.default_opt(**okw), bm2.default_sam_opt(**skw)
        M = hand_made(Lists(prefix, 500 + ci), opt, so.max_ins)
        n_hand = (len(M.hit_off) - 1) // 2
        random_pairs(M, n_random, so.max_ins)
        hits, hit_off = M.arrays()
        pes, hist = compare(ctx, prefix, opt, so, hits, hit_off, name)
        mine, seen, left_out = stat_in_python(l_pac, opt, so, hits, hit_off)
        # the rules leave out at most the two 500-hit pairs of the hand-made set and at most 1 % of the random pairs (here: none)
        assert [p for p in left_out if p >= n_hand] == [] and len([p for p in left_out if p < n_hand]) == 2, (name, left_out)
        assert len([p for p in left_out if p >= n_hand]) * 100 <= n_random
        rest = hist.astype(np.int64) - mine
        assert (rest >= 0).all() and rest.sum() <= len(left_out), (name, int(rest.sum()))
        # the two heavy pairs by the rules as well, written for them alone: the only overlap is the last hit; sub-score 10 counts the
        # pair, 90 does not
        heavy_counted = 0
        for p in left_out:
            a = [hits[hit_off[2 * p + e]:hit_off[2 * p + e + 1]] for e in range(2)]
            assert len(a[0]) == len(a[1]) == 500
            sub = [cal_sub(opt, x, set()) for x in a]
            assert sub[0] == sub[1] == int(a[0]["score"][-1]) and sub[0] in (10, 90)
            d, dist = infer_dir(l_pac, int(a[0]["rb"][0]), int(a[1]["rb"][0]))
            if sub[0] == 10 and 0 < dist <= so.max_ins:
                assert rest[d, dist] == 1, (name, p)
                heavy_counted += 1
        assert rest.sum() == heavy_counted == 1, (name, int(rest.sum()), heavy_counted)
        if name.startswith("mask_level"):
            assert seen.get("float_matters", 0) > 0, (name, seen)
        if name == "min_seed_len 19, a 1":                       # scores 23 and 24: 18.4 < 19 <= 19.2
            s = [int(hits["score"][hit_off[2 * p]]) for p in (3, 4)]
            assert s == [23, 24], s
        for k, v in seen.items():
            total[k] = total.get(k, 0) + v
        if so.max_ins >= 500:
            reach = [k for k in need if so.max_ins < l_pac or not k.startswith("dist_max_ins")]     # (no distance of l_pac or more exists)
            missing = [k for k in reach if not seen.get(k)]
            if so.max_ins >= l_pac:
                assert hist[:, 40000:].sum() > 10 and hist[:, l_pac - 1].sum() > 0, name       # bins whose number takes more than 15 bits
            assert not missing, "%s: the inputs never reach %s (%s)" % (name, missing, seen)
    # max_ins <= 0: four failed models and an all-zero histogram
    for max_ins in (0, -5):
        opt, so = bm2.default_opt(), bm2.default_sam_opt(max_ins=max_ins)
        M = random_pairs(Lists(prefix, 9), 50, 500)
        hits, hit_off = M.arrays()
        pes, hist = compare(ctx, prefix, opt, so, hits, hit_off, "max_ins %d" % max_ins)
        assert hist.shape == (4, 1) and not hist.any() and all(x.failed == 1 and x.low == 0 and x.high == 0 for x in pes)
    # hit_off that does not start at 0: the same lists behind 7 hits that belong to nobody
    opt, so = bm2.default_opt(), bm2.default_sam_opt(max_ins=500)
    M = random_pairs(hand_made(Lists(prefix, 21), opt, 500), 100, 500)
    hits, hit_off = M.arrays()
    base_pes, base_hist = compare(ctx, prefix, opt, so, hits, hit_off, "offsets from 0")
    junk = np.array([M.at(123, 0, 0, 100, 250) for _ in range(7)], bm2.ALNREG_DT)
    pes, hist = compare(ctx, prefix, opt, so, np.concatenate([junk, hits]), hit_off + 7, "offsets from 7")
    assert same_pes(pes, base_pes) and (hist == base_hist).all() and hist.sum() > 50
    return total


def oriented_batch(prefix, counts, seed=3, spread=100):
    """counts[d] unique pairs of direction d at distances 200 + (7 i) % spread"""
    M = Lists(prefix, seed)
    for d, n in enumerate(counts):
        for i in range(n):
            assert M.oriented(d, 200 + (7 * i) % spread, 5000 + 11 * i if d in (0, 1) else 9000 + 11 * i)
    return M.arrays()


def check_thresholds(ctx, prefix):
    """the `failed` threshold (9 and 10 counted pairs) and the 5 % rule (4 % and 6 % of the largest orientation)"""
    opt, so = bm2.default_opt(), bm2.default_sam_opt()
    hits, hit_off = oriented_batch(prefix, [10, 9, 0, 0])
    pes, hist = compare(ctx, prefix, opt, so, hits, hit_off, "9 and 10")
    assert hist.sum(axis=1).tolist() == [10, 9, 0, 0] and [x.failed for x in pes] == [0, 1, 1, 1], [x.failed for x in pes]
    hits, hit_off = oriented_batch(prefix, [250, 10, 15, 9])
    pes, hist = compare(ctx, prefix, opt, so, hits, hit_off, "4 % and 6 %")
    assert hist.sum(axis=1).tolist() == [250, 10, 15, 9] and [x.failed for x in pes] == [0, 1, 0, 1], [x.failed for x in pes]
    assert pes[0].low >= 1 and pes[0].high > pes[0].low and pes[0].std > 0
    return True


def check_contention(ctx, prefix, n=70000):
    """Item 2: n pairs of one hit an end, all in ONE bin of one orientation -- the bin holds exactly n (above any 16-bit counter), with
    one copy of the histogram and with the default number"""
    with bm2.Index(prefix) as ix:
        l_pac = ix.l_pac
    one = Lists(prefix, 1)
    assert one.oriented(1, 300, 4000)
    two, _ = one.arrays()
    hits = np.tile(two, n)
    hit_off = np.arange(2 * n + 1, dtype=np.int64)
    opt, so = bm2.default_opt(), bm2.default_sam_opt()
    out = {}
    for copies in ("1", None):
        if copies is not None:
            os.environ["BM2_PESTAT_COPIES"] = copies
        try:
            pes, hist = compare(ctx, prefix, opt, so, hits, hit_off, "contention, copies %s" % copies)
        finally:
            os.environ.pop("BM2_PESTAT_COPIES", None)
        assert hist[1, 300] == n and hist.sum() == n and n > 65535, (copies, int(hist[1, 300]))
        assert [x.failed for x in pes] == [1, 0, 1, 1] and pes[1].avg == 300.0 and pes[1].std == 0.0
        out[copies] = int(hist[1, 300])
    # several copies with counts in more than one orientation and bin: what the reduce kernel sums is every copy, every bin
    hits, hit_off = oriented_batch(prefix, [700, 900, 300, 400], seed=8, spread=64)
    for copies in ("1", "3", None):
        if copies is not None:
            os.environ["BM2_PESTAT_COPIES"] = copies
        try:
            pes, hist = compare(ctx, prefix, opt, so, hits, hit_off, "four orientations, copies %s" % copies)
        finally:
            os.environ.pop("BM2_PESTAT_COPIES", None)
        assert hist.sum(axis=1).tolist() == [700, 900, 300, 400]
    return out


def check_sizes(ctx, prefix):
    """Item 3: n_pairs 0, 1, 63, 64, 65, 255, 256, 257 and two blocks plus one -- prefixes of one batch"""
    opt, so = bm2.default_opt(), bm2.default_sam_opt(max_ins=500)
    M = random_pairs(Lists(prefix, 77), 2 * BLOCK + 1, 500, max_hits=4)
    hits, hit_off = M.arrays()
    counts = {}
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 2 * BLOCK + 1):
        pes, hist = compare(ctx, prefix, opt, so, hits[:hit_off[2 * n]], hit_off[:2 * n + 1], "%d pairs" % n)
        counts[n] = int(hist.sum())
    assert counts[0] == 0 and counts[2 * BLOCK + 1] > counts[257] >= counts[256] >= counts[255] > counts[65] >= counts[63] > 0, counts
    e_pes, e_hist = ctx.pe_stat(opt, so, hits[:0], np.zeros(1, np.int64))
    assert not e_hist.any() and all(x.failed == 1 for x in e_pes)
    return counts


def check_capacity_and_refusals(ctx, prefix):
    """Item 4: hist_cap one short, exact room, NULL hist; NULL arguments, a context without an index, a decreasing hit_off, max_ins above
    2^24 -- in both forms where both have the argument"""
    opt, so = bm2.default_opt(), bm2.default_sam_opt(max_ins=500)
    hits, hit_off = oriented_batch(prefix, [30, 40, 12, 0])
    n_pairs = (len(hit_off) - 1) // 2
    pes, hist = compare(ctx, prefix, opt, so, hits, hit_off, "refusals")
    before = bm2.sam_pestat_stats()
    assert before == (n_pairs, 82, len(hits) * HIT_BYTES, 0), before
    room = 4 * 501
    for form in (lambda **k: bm2.pe_stat(prefix, opt, so, hits, hit_off, **k), lambda **k: ctx.pe_stat(opt, so, hits, hit_off, **k)):
        rc, _, buf = form(hist_cap=room - 1)
        assert rc == bm2.BM2_ECAP and (buf == 0xeeeeeeee).all(), rc
        rc, got, buf = form(hist_cap=room)
        assert rc == bm2.BM2_OK and same_pes(got, pes) and (buf.reshape(4, 501) == hist).all()
        rc, got, buf = form(hist_cap=room + 5)                   # more room than needed: the counts, the rest untouched
        assert rc == bm2.BM2_OK and (buf[:room].reshape(4, 501) == hist).all() and (buf[room:] == 0xeeeeeeee).all()

    def refused(rc_want, word, f):
        try:
            f()
        except bm2.Bm2Error as e:
            assert e.rc == rc_want and word in str(e), (word, e)
            return
        raise AssertionError("accepted: " + word)
    bad_off = hit_off.copy()
    bad_off[1] = hit_off[2] + 1
    refused(bm2.BM2_EINVAL, "hit_off", lambda: ctx.pe_stat(opt, so, hits, bad_off))
    refused(bm2.BM2_EINVAL, "hit_off", lambda: bm2.pe_stat(prefix, opt, so, hits, bad_off))
    big = bm2.default_sam_opt(max_ins=(1 << 24) + 1)
    refused(bm2.BM2_EUNSUP, "max_ins", lambda: ctx.pe_stat(opt, big, hits, hit_off, hist=False))
    refused(bm2.BM2_EUNSUP, "max_ins", lambda: bm2.pe_stat(prefix, opt, big, hits, hit_off, hist=False))
    bare = bm2.Context(0, None)
    try:
        refused(bm2.BM2_EINVAL, "no index", lambda: bare.pe_stat(opt, so, hits, hit_off))
    finally:
        bare.close()
    assert bm2.sam_pestat_stats() == before                      # nothing ran
    L = bm2.lib()
    pq = (bm2.PeStat * 4)()
    buf = np.zeros(room, np.uint32)
    good = [C.c_void_p(ctx.h), C.byref(opt), C.byref(so), C.c_int32(n_pairs), C.c_void_p(hits.ctypes.data), C.c_void_p(hit_off.ctypes.data), pq,
            C.c_void_p(buf.ctypes.data), C.c_int64(room)]
    L.bm2_pe_stat_dev.restype = C.c_int
    assert L.bm2_pe_stat_dev(*good) == bm2.BM2_OK and (buf.reshape(4, 501) == hist).all() and same_pes(list(pq), pes)
    for k in (0, 1, 2, 4, 5, 6):                                # every pointer but hist in turn (hits: NULL with a non-empty batch)
        args = list(good)
        args[k] = None
        assert L.bm2_pe_stat_dev(*args) == bm2.BM2_EINVAL, k
        assert b"bad argument" in L.bm2_last_error(), k
    for k, v in ((3, C.c_int32(-1)), (8, C.c_int64(-1))):
        args = list(good)
        args[k] = v
        assert L.bm2_pe_stat_dev(*args) == bm2.BM2_EINVAL, k
    return True


def check_tail(tail, extra, ctx, flag=0, combos=COMBOS, **skw):
    """Items 5 and 6: the tail with the bit, alone and with PLAN, PLAN | RESCUE, PLAN | RESCUE | DECIDE | TEXT == the flag-off text ==
    `bwa-mem2 mem`; pes_out equal; the model's counters say the count happened on the device; with PLAN the plan found the hits resident
    (and planned what PLAN alone plans); with pes_in given the bit changes nothing and the counters read 0."""
    ref = tail.reference(extra)
    off_text, pes_off = tail.ours(flag, ctx, **skw)
    assert ref == off_text, tail.M._diff(ref, off_text)
    so = bm2.default_sam_opt(flag=flag, **skw)
    h_pes, h_hist = bm2.pe_stat(tail.fa, tail.opt, so, tail.aln, tail.aln_off)
    assert same_pes(h_pes, pes_off)                              # (bm2_pe_stat IS the tail's model)
    counted, hit_bytes = int(h_hist.sum()), len(tail.aln) * HIT_BYTES
    assert counted > 10 and hit_bytes > 0
    for bits in combos:
        plan_alone = None
        if bits & PLAN:
            base_text, _ = tail.ours(flag | bits, ctx, **skw)
            assert base_text == off_text
            plan_alone = (bm2.sam_rescue_plan_stats(), bm2.sam_rescue_stats())
            assert bm2.sam_pestat_stats()[3] == 0                # the plan bit without the model's: nothing was resident
        on_text, pes_on = tail.ours(flag | bits | PESTAT, ctx, **skw)
        assert ref == on_text, tail.M._diff(ref, on_text)
        assert same_pes(pes_on, pes_off)
        st = bm2.sam_pestat_stats()
        assert st == (tail.n_pairs, counted, hit_bytes, hit_bytes if bits & PLAN else 0), (bits, st, tail.n_pairs, counted, hit_bytes)
        if bits & PLAN:
            assert (bm2.sam_rescue_plan_stats(), bm2.sam_rescue_stats()) == plan_alone, (bits, plan_alone)
    return ref, pes_off


def check_tail_given_model(tail, ctx):
    """with pes_in given there is nothing to compute: the bit is accepted, the text is that of the same call without it, the counters read 0"""
    _, pes = tail.ours(0, ctx)
    model = D.pestat(D.FR)
    texts = {}
    for given in (pes, model):
        for bits in (0, PESTAT, PESTAT | PLAN):
            texts[bits], pes_out = bm2.sam_pe(tail.fa, tail.enc, tail.off, tail.ln, tail.opt, tail.aln, tail.aln_off, tail.names, tail.quals, None,
                                              bm2.default_sam_opt(flag=bits), pes_in=given, ctx=ctx)
            assert same_pes(pes_out, given)
            if bits:
                assert bm2.sam_pestat_stats() == (0, 0, 0, 0), (bits, bm2.sam_pestat_stats())
        assert texts[0] == texts[PESTAT] == texts[PESTAT | PLAN]
    return True


def check_tail_two_contexts(tail, ctx, ctx2, part_knob, combos=COMBOS):
    """the same through two contexts sharing a replica: the model's hook and the plan's cut the pairs into the same two parts"""
    for k in PART_KNOBS:
        os.environ[k] = str(part_knob)
    try:
        assert tail.n_pairs > part_knob                          # (two parts)
        return check_tail(tail, [], [ctx, ctx2], combos=combos)
    finally:
        for k in PART_KNOBS:
            del os.environ[k]


def check_tail_no_rescue(tail, ctx):
    """the model does not depend on mate rescue: the bit with MEM_F_NO_RESCUE (-S) and with rescue_inline"""
    check_tail(tail, ["-S"], ctx, flag=0x20, combos=[0])
    check_tail(tail, [], ctx, combos=[0], rescue_inline=1)
    return True


def check_tail_refusals(tail):
    """the bit without a context"""
    try:
        tail.ours(PESTAT, None)
    except bm2.Bm2Error as e:
        assert e.rc == bm2.BM2_EINVAL and "DEVICE_PESTAT" in str(e), e
        return True
    raise AssertionError("accepted")
