"""Shared by tests/test_cigar_plan_emu.py (the device sources on the host emulator) and tests/test_zzzzzzz_cigar_plan_gpu.py (the MI355X):
which hits the SAM text asks a CIGAR for, picked on the device -- bm2_cigar_plan_dev against bm2_cigar_plan (the dry emit pass of the
tail's CIGAR session as a function of its inputs) on lists made here, index for index, and the tails with BM2_SAM_F_DEVICE_CGPLAN (alone
and with the other device bits) against the flag-off tail and the compiled reference.  Every comparison is exact; every event a check
names is counted and asserted to occur."""
import ctypes as C
import os

import numpy as np

import bm2

CGPLAN = bm2.SAM_F_DEVICE_CGPLAN
PESTAT, PLAN, RESCUE, DECIDE, TEXT = bm2.SAM_F_DEVICE_PESTAT, bm2.SAM_F_DEVICE_PLAN, bm2.SAM_F_DEVICE_RESCUE, bm2.SAM_F_DEVICE_DECIDE, bm2.SAM_F_DEVICE_TEXT
COMBOS = [0, DECIDE, PLAN | RESCUE | DECIDE, PESTAT | PLAN | RESCUE | DECIDE | TEXT]
PART_KNOBS = ("BM2_CGPLAN_PART", "BM2_PLAN_PART", "BM2_KSW_PART", "BM2_RESCUE_PART", "BM2_DECIDE_PART", "BM2_TEXT_PART")
F_ALL = 0x8
INT_MAX = 0x7fffffff
LIGHT_MAX = 16        # hits of a unit (a single-end list, a pair's two lists) the 16-lane form takes (cgplan.hip: CG_LIGHT_MAX)
LDS_CAP = 256         # hits of a list whose counters the wavefront form keeps in LDS (CG_LDS_CAP)
BLOCK_HITS = 1024     # hits per block of the compaction (CG_BLOCK_HITS)
LENGTHS = [0, 1, 2, 15, 16, 17, 63, 64, 65, LDS_CAP - 1, LDS_CAP, LDS_CAP + 1, 500]


# ---- lists: a hit is (score, secondary, secondary_all, is_alt); everything else of the 96-byte record is noise the rule must not read
def arrays(lists, rng, lead=0):
    """-> (hits ALNREG_DT, hit_off): the lists back to back behind `lead` hits that belong to no list"""
    n = lead + sum(len(x) for x in lists)
    hits = np.zeros(max(n, 1), bm2.ALNREG_DT)
    for f in ("rb", "re", "qb", "qe", "rid", "truesc", "sub", "csub", "w", "seedcov", "pad"):
        hits[f] = rng.integers(0, 1000, size=len(hits))
    off, at = [lead], lead
    for x in lists:
        for h in x:
            hits["score"][at], hits["secondary"][at], hits["secondary_all"][at], hits["is_alt"][at] = h
            at += 1
        off.append(at)
    return hits[:n], np.array(off, np.int64)


def plans_array(plans):
    a = np.zeros(max(len(plans), 1), bm2.PAIRPLAN_DT)
    for i, (paired, z, n_pri) in enumerate(plans):
        a["paired"][i], a["z"][i], a["n_pri"][i] = paired, z, n_pri
        a["q_se"][i], a["extra_flag"][i] = (17, 23), 1
    return a[:len(plans)]


def random_list(rng, n, p_alt=0.2):
    """n hits as mark_primary leaves them in shape: a few leaders, the others pointing at an earlier hit"""
    out = []
    for i in range(n):
        score = int(rng.integers(10, 200))
        alt = int(rng.random() < p_alt)
        if i == 0 or rng.random() < 0.15:
            sec, sa = -1, -1
        else:
            few = max(1, min(i, 4))
            sa = int(rng.integers(0, few)) if rng.random() < 0.8 else int(rng.integers(0, i))
            sec = sa if rng.random() < 0.7 else int(rng.choice([-1, -2, INT_MAX, int(rng.integers(0, i))]))
        out.append((score, sec, sa, alt))
    return out


def random_plan(rng, a0, a1):
    paired = int(len(a0) > 0 and len(a1) > 0 and rng.random() < 0.5)
    return (paired, (int(rng.integers(0, max(len(a0), 1))) if paired else 0, int(rng.integers(0, max(len(a1), 1))) if paired else 0),
            (int(rng.integers(0, len(a0) + 1)), int(rng.integers(0, len(a1) + 1))))


# ---- the rule written again with Python numbers (numpy float32 / Python float for the two floating-point tests)
def plan_in_python(opt, so, hits, hit_off, plans, seen):
    """-> the selected indices (ascending); seen[event] counts what was met"""
    T, all_ = int(so.T), bool(so.flag & F_ALL)
    xr = float(np.float32(so.XA_drop_ratio))                     # the float ratio widened to double
    dr = np.float32(opt.drop_ratio)
    max_xa, max_alt = int(so.max_XA_hits), int(so.max_XA_hits_alt)
    sel = []

    def note(k):
        seen[k] = seen.get(k, 0) + 1
    for li in range(len(hit_off) - 1):
        b, e = int(hit_off[li]), int(hit_off[li + 1])
        n = e - b
        sc = [int(v) for v in hits["score"][b:e]]
        sec = [int(v) for v in hits["secondary"][b:e]]
        sa = [int(v) for v in hits["secondary_all"][b:e]]
        alt = [int(v) for v in hits["is_alt"][b:e]]
        why = [set() for _ in range(n)]
        plan = None if plans is None else plans[li >> 1]
        end = li & 1
        note("len_%d" % n if n in LENGTHS else "len_other")
        if not all_:
            def pri(i, quiet=True):
                k = sa[i]
                if k < 0:
                    return -1
                lim = float(sc[k]) * xr                          # one double product
                ok = float(sc[i]) >= lim
                if not quiet:
                    if ok and not float(sc[i] - 1) >= lim:
                        note("xa_smallest_kept")
                    if not ok and float(sc[i] + 1) >= lim:
                        note("xa_largest_dropped")
                    if ok != (np.float32(sc[i]) >= np.float32(sc[k]) * np.float32(so.XA_drop_ratio)):
                        note("xa_double_matters")
                return k if ok else -1
            cnt, has_alt = [0] * n, [0] * n
            for i in range(n):
                r = pri(i, quiet=False)
                if r >= 0:
                    cnt[r] += 1
                    has_alt[r] |= int(alt[i] != 0)
            for r in range(n):
                if cnt[r]:
                    for k, v in (("max", max_xa), ("max_alt", max_alt)):
                        if cnt[r] == v:
                            note("cnt_eq_%s_%s" % (k, "alt" if has_alt[r] else "noalt"))
                        if cnt[r] == v + 1:
                            note("cnt_%s_plus_1_%s" % (k, "alt" if has_alt[r] else "noalt"))
            for i in range(n):
                r = pri(i)
                if r < 0:
                    continue
                if cnt[r] > max_alt or (not has_alt[r] and cnt[r] > max_xa):
                    note("xa_too_many")
                    continue
                why[i].add("xa")
        else:
            note("list_under_F_ALL")
        if plan is not None and plan["paired"]:
            note("paired")
            z, n_pri = int(plan["z"][end]), int(plan["n_pri"][end])
            why[z].add("z")
            if n_pri == n:
                note("n_pri_eq_n")
            else:
                note("n_pri_lt_n")
                fails = [sc[n_pri] < T, sec[n_pri] >= 0, not alt[n_pri]]
                if not any(fails):
                    why[n_pri].add("alt_at_n_pri")
                    note("alt_at_n_pri_passes")
                elif sum(fails) == 1:
                    note("alt_at_n_pri_fails_" + ("score", "secondary", "is_alt")[fails.index(True)])
        else:
            if plan is not None:
                note("unpaired")
                n_pri = int(plan["n_pri"][end])
                if n:
                    if sc[0] >= T:
                        why[0].add("rep")
                        note("rep_is_hit_0")
                    elif n_pri < n and sc[n_pri] >= T:
                        why[n_pri].add("rep")
                        note("rep_falls_back_to_n_pri")
                    else:
                        note("no_rep")
            for k in range(n):
                if sc[k] == T - 1:
                    note("score_T_minus_1")
                if sc[k] == T:
                    note("score_T")
                if sc[k] < T:
                    continue
                note("secondary_%s" % ("-2" if sec[k] == -2 else "-1" if sec[k] == -1 else "INT_MAX" if sec[k] == INT_MAX else "index"))
                if sec[k] >= 0 and (alt[k] or not all_):
                    continue
                if 0 <= sec[k] < INT_MAX:
                    lim = np.float32(sc[sec[k]]) * dr           # one float32 product
                    dropped = bool(np.float32(sc[k]) < lim)
                    if dropped and not np.float32(sc[k] + 1) < lim:
                        note("drop_largest_dropped")
                    if not dropped and np.float32(sc[k] - 1) < lim:
                        note("drop_smallest_kept")
                    if dropped:
                        continue
                why[k].add("reg2sam")
        for i in range(n):
            if why[i]:
                sel.append(b + i)
                for k in why[i]:
                    note("by_" + k)
                if len(why[i]) > 1:
                    note("two_rules")
            else:
                note("not_selected")
    return np.array(sel, np.int32)


def heavy_units(hit_off, per_unit):
    off = np.asarray(hit_off)
    tot = off[per_unit::per_unit] - off[:-per_unit:per_unit] if len(off) > per_unit else np.zeros(0, np.int64)
    return int((tot > LIGHT_MAX).sum())


def compare(ctx, opt, so, hits, hit_off, plans, seen, what=""):
    """device == host == the Python restatement; the device's counters"""
    want = plan_in_python(opt, so, hits, hit_off, plans, seen)
    keep = hits.copy()
    host = bm2.cigar_plan(opt, so, hits, hit_off, plans)
    assert (host == want).all() and len(host) == len(want), (what, "host", len(host), len(want))
    dev = ctx.cigar_plan(opt, so, hits, hit_off, plans)
    assert len(dev) == len(host) and (dev == host).all(), (what, "device", len(dev), len(host), np.flatnonzero(dev[:min(len(dev), len(host))] != host[:min(len(dev), len(host))])[:5])
    assert hits.tobytes() == keep.tobytes()                       # read only
    n_lists, n_hits = len(hit_off) - 1, int(hit_off[-1] - hit_off[0])
    assert bm2.sam_cigar_plan_stats() == (n_lists, n_hits, len(host), heavy_units(hit_off, 1 if plans is None else 2) if n_lists else 0), (what, bm2.sam_cigar_plan_stats())
    return host


def largest_below(limit_of, top):
    """the largest s in [0, top] for which limit_of(s) holds (limit_of is true up to a threshold), or -1"""
    s = -1
    for v in range(top + 1):
        if limit_of(v):
            s = v
    return s


def hand_made(opt, so, rng):
    """-> (lists, plans for their pairs): the named cases under this option set; pairs (2k, 2k + 1) share plans[k]"""
    T = int(so.T)
    xr, dr = float(np.float32(so.XA_drop_ratio)), np.float32(opt.drop_ratio)
    mx, ma = int(so.max_XA_hits), int(so.max_XA_hits_alt)
    L, P = [], []

    def pair(a0, a1, paired=0, z=(0, 0), n_pri=None):
        L.extend([a0, a1])
        P.append((paired, z, n_pri if n_pri is not None else (len(a0), len(a1))))
    for n in LENGTHS:                                            # every length beside an empty list, a short one and itself
        for m in (0, 3, n):
            a0, a1 = random_list(rng, n), random_list(rng, m)
            pair(a0, a1, *random_plan(rng, a0, a1))
    pair([(T - 1, -1, -1, 0)], [(T, -1, -1, 0)])                 # T - 1 / T
    pair([(T - 1, -1, -1, 0)], [(T, -1, -1, 0)], 1)
    for s in (-2, -1, 0, INT_MAX):                               # secondary in {-2, -1, an index, INT_MAX}, with and without ALT
        for alt in (0, 1):
            pair([(120, -1, -1, 0), (110, s, -1, alt)], [(120, -1, -1, 0), (110, s, 0, alt)])
    for p in range(5, 251):                                      # the two floating-point boundaries for primary scores 5 .. 250
        d = largest_below(lambda s: bool(np.float32(s) < np.float32(p) * dr), 300)
        x = largest_below(lambda s: not float(s) >= float(p) * xr, 300)
        pair([(p, -1, -1, 0), (d, 0, -1, 0), (d + 1, 0, -1, 0)], [(p, -1, -1, 0), (max(x, 0), 0, 0, 0), (x + 1, 0, 0, 0)])
    for k, alt in ((mx, 0), (mx + 1, 0), (mx, 1), (mx + 1, 1), (ma, 1), (ma + 1, 1), (ma, 0), (ma + 1, 0)):      # cnt[r] at its two limits
        if k < 1:
            continue
        a = [(150, -1, -1, 0)] + [(140, 0, 0, 0)] * k
        if alt:
            a[1 + k // 2] = (140, 0, 0, 1)
        pair(a, list(a), 1, (0, k // 2))
    # paired: n_pri == n; n_pri < n with the ALT hit at n_pri passing and failing each of its three tests
    pair([(100, -1, -1, 0), (90, 0, 0, 0)], [(100, -1, -1, 0)], 1, (1, 0), (2, 1))
    for hit in ((T, -1, -1, 1), (T - 1, -1, -1, 1), (T, 0, -1, 1), (T, -1, -1, 0), (T + 5, -2, 0, 1)):
        pair([(100, -1, -1, 0), hit], [(100, -1, -1, 0), (60, 0, 0, 0), hit], 1, (0, 1), (1, 2))
    # not paired: the representative is hit 0, falls back to hit n_pri, or is nobody
    pair([(T, -1, -1, 0), (T + 9, -1, -1, 1)], [(T - 1, -1, -1, 0), (T + 9, -1, -1, 1)], 0, (0, 0), (1, 1))
    pair([(T - 1, -1, -1, 0), (T - 1, -1, -1, 1)], [(T - 1, -1, -1, 0), (T + 9, 0, 0, 1)], 0, (0, 0), (1, 1))
    pair([(T - 1, -1, -1, 0)], [(T - 1, -1, -1, 0), (T + 9, 0, 0, 1)], 0, (0, 0), (1, 2))
    # a hit two rules ask for: XA and reg2sam (secondary_all set, secondary not), XA and z, z and the ALT hit at n_pri
    pair([(100, -1, -1, 0), (95, -1, 0, 1)], [(100, -1, -1, 0), (95, -2, 0, 0)])
    pair([(100, -1, -1, 0), (95, 0, 0, 0)], [(100, -1, -1, 0), (95, -1, -1, 1)], 1, (1, 1), (2, 1))
    return L, P


OPTION_SETS = [({}, {}), ({}, dict(flag=F_ALL)), (dict(drop_ratio=0.3), dict(flag=F_ALL, T=1)), ({}, dict(XA_drop_ratio=0.3, T=1)),
               ({}, dict(max_XA_hits=2, max_XA_hits_alt=7, T=20))]
WANTED = (["len_%d" % n for n in LENGTHS] +
          ["score_T_minus_1", "score_T", "secondary_-2", "secondary_-1", "secondary_index", "secondary_INT_MAX", "list_under_F_ALL", "paired", "unpaired",
           "n_pri_eq_n", "n_pri_lt_n", "alt_at_n_pri_passes", "alt_at_n_pri_fails_score", "alt_at_n_pri_fails_secondary", "alt_at_n_pri_fails_is_alt",
           "rep_is_hit_0", "rep_falls_back_to_n_pri", "no_rep", "two_rules", "by_xa", "by_reg2sam", "by_rep", "by_z", "by_alt_at_n_pri", "not_selected",
           "xa_too_many", "xa_double_matters", "cnt_eq_max_noalt", "cnt_max_plus_1_noalt", "cnt_eq_max_alt", "cnt_max_plus_1_alt",
           "cnt_eq_max_alt_alt", "cnt_max_alt_plus_1_alt", "cnt_eq_max_alt_noalt", "cnt_max_alt_plus_1_noalt"])


def check_lists(ctx, quick=False):
    """bm2_cigar_plan_dev against bm2_cigar_plan, single-end form and paired form, under every option set"""
    total = {}
    for k, (okw, skw) in enumerate(OPTION_SETS):
        if quick and k in (3,):                                  # (quick: the XA boundary at 0.3 is left to the long form; 0.8 stays)
            continue
        opt, so = bm2.default_opt(**okw), bm2.default_sam_opt(**skw)
        rng = np.random.default_rng(100 + k)
        seen = {}
        lists, plans = hand_made(opt, so, rng)
        for lead in (0, 7):                                      # an hit_off that does not start at 0
            hits, hit_off = arrays(lists, rng, lead)
            compare(ctx, opt, so, hits, hit_off, None, seen, "set %d, single-end, lead %d" % (k, lead))
            compare(ctx, opt, so, hits, hit_off, plans_array(plans), seen, "set %d, paired, lead %d" % (k, lead))
        assert seen["drop_largest_dropped"] >= 246 and seen["drop_smallest_kept"] >= 246 if so.flag & F_ALL and so.T <= 1 else True, (k, seen)      # (T = 1: every score reaches the test)
        assert seen["xa_largest_dropped"] >= 246 and seen["xa_smallest_kept"] >= 246 if not so.flag & F_ALL else True, (k, seen)
        for ev, c in seen.items():
            total[ev] = total.get(ev, 0) + c
    missing = [ev for ev in WANTED if not total.get(ev)]
    assert not missing, (missing, total)
    return total


def check_sizes(ctx):
    """0, 1, 2, 255, 256, 257 lists and 2 x 4097 lists of one hit each (and the hit counts around one compaction block), everything
    selected and nothing selected"""
    opt, so = bm2.default_opt(), bm2.default_sam_opt()
    rng = np.random.default_rng(5)
    seen = {}
    for n in (0, 1, 2, 255, 256, 257, BLOCK_HITS - 1, BLOCK_HITS, BLOCK_HITS + 1, 2 * 4097):
        for score in (so.T, so.T - 1):
            hits, hit_off = arrays([[(score, -1, -1, 0)]] * n, rng)
            got = compare(ctx, opt, so, hits, hit_off, None, seen, "%d single-end lists" % n)
            assert len(got) == (n if score >= so.T else 0)
            if n % 2 == 0:
                got = compare(ctx, opt, so, hits, hit_off, plans_array([(0, (0, 0), (1, 1))] * (n // 2)), seen, "%d paired lists" % n)
                assert len(got) == (n if score >= so.T else 0)
    return seen.get("by_reg2sam", 0), seen.get("not_selected", 0)


def check_capacity_and_refusals(ctx):
    opt, so = bm2.default_opt(), bm2.default_sam_opt()
    rng = np.random.default_rng(6)
    lists = [random_list(rng, n) for n in (3, 0, 40, 7, 300, 1)]
    plans = plans_array([random_plan(rng, lists[2 * p], lists[2 * p + 1]) for p in range(3)])
    hits, hit_off = arrays(lists, rng, 5)
    L = bm2.lib()
    L.bm2_cigar_plan.restype = L.bm2_cigar_plan_dev.restype = C.c_int
    forms = ((L.bm2_cigar_plan, ()), (L.bm2_cigar_plan_dev, (C.c_void_p(ctx.h),)))
    for pl in (None, plans):
        want = bm2.cigar_plan(opt, so, hits, hit_off, pl)
        n = len(want)
        assert n > 3
        for fn, head in forms:
            for cap in (0, n - 1, n, n + 3):
                buf = np.full(n + 8, -7, np.int32)
                n_out = C.c_int64(-1)
                rc = fn(*head, C.byref(opt), C.byref(so), C.c_int32(len(lists)), C.c_void_p(hits.ctypes.data), C.c_void_p(hit_off.ctypes.data),
                        C.c_void_p(pl.ctypes.data if pl is not None else None), C.c_void_p(buf.ctypes.data), C.c_int64(cap), C.byref(n_out))
                assert rc == (bm2.BM2_ECAP if cap < n else bm2.BM2_OK), (cap, rc)
                assert n_out.value == n                            # complete under BM2_ECAP
                k = min(cap, n)
                assert (buf[:k] == want[:k]).all() and (buf[k:] == -7).all(), cap      # nothing at or above cap
    bare = bm2.Context(0, None)                                  # a context without an index will do
    try:
        assert (bare.cigar_plan(opt, so, hits, hit_off, plans) == bm2.cigar_plan(opt, so, hits, hit_off, plans)).all()
    finally:
        bare.close()
    empty = np.zeros(1, np.int64)
    for pl in (None, plans[:0]):
        assert len(bm2.cigar_plan(opt, so, hits[:0], empty, pl)) == 0 and len(ctx.cigar_plan(opt, so, hits[:0], empty, pl)) == 0

    def refused(word, *a):
        for who, f in (("host", lambda: bm2.cigar_plan(opt, so, *a)), ("device", lambda: ctx.cigar_plan(opt, so, *a))):
            try:
                f()
            except bm2.Bm2Error as e:
                assert e.rc == bm2.BM2_EINVAL and word in str(e), (who, word, e)
                continue
            raise AssertionError("%s accepted: %s" % (who, word))
    refused("a pair has two", hits, hit_off[:-1], plans)          # an odd number of lists with plans
    bad_off = hit_off.copy()
    bad_off[3] = hit_off[4] + 1
    refused("hit_off", hits, bad_off, None)
    refused("hit_off", hits, bad_off, plans)
    # an index that points outside its list, in each of the four fields, in a short list and in a long one
    for li in (0, 2, 4):
        b, n = int(hit_off[li]), int(hit_off[li + 1] - hit_off[li])
        for f in ("secondary", "secondary_all"):
            for v in (n, n + 100):
                bad = hits.copy()
                bad[f][b + n - 1] = v
                refused("points outside", bad, hit_off, None)
                refused("points outside", bad, hit_off, plans)
        ok = hits.copy()
        ok["secondary"][b + n - 1] = INT_MAX                      # (INT_MAX is no index)
        assert (ctx.cigar_plan(opt, so, ok, hit_off, None) == bm2.cigar_plan(opt, so, ok, hit_off, None)).all()
        for f, v, paired in (("z", n, 1), ("z", -1, 1), ("n_pri", n + 1, 0), ("n_pri", -1, 0), ("n_pri", n + 1, 1)):
            bad = plans.copy()
            bad["paired"][li >> 1] = paired
            if paired:
                bad["z"][li >> 1] = (0, 0)
                bad["n_pri"][li >> 1] = (min(1, int(hit_off[li + 1] - hit_off[li])), min(1, int(hit_off[li + 2] - hit_off[li + 1])))
            bad[f][li >> 1][0] = v
            refused("points outside", hits, hit_off, bad)
    bad = plans.copy()                                           # a paired plan over an empty list: z = 0 points outside it
    bad["paired"][0] = 1
    refused("points outside", hits, hit_off, bad)
    only_empty = np.array([5, 5, 5], np.int64)
    refused("points outside", hits, only_empty, plans_array([(1, (0, 0), (0, 0))]))
    return True


# ---- the tails with the bit
def cigar_and_text(tail, flag, ctx, **skw):
    text, pes = tail.ours(flag, ctx, **skw)
    return text, pes, bm2.sam_cigar_stats()


def check_tail(tail, ctx, combos=COMBOS, extra=(), flag=0, **skw):
    """bm2_sam_pe_dev with the bit, alone and with the other device bits: the reference's bytes, the flag-off call's bytes and its
    planned / used / missed; the plan's counters say the selection came from the device"""
    ref = tail.reference(list(extra))
    off_text, pes_off, st_off = cigar_and_text(tail, flag, ctx, **skw)
    assert ref == off_text, tail.M._diff(ref, off_text)
    assert st_off[0] > 10 and st_off[1] >= st_off[0]
    for bits in combos:
        if bits:
            base_text, _, st_off = cigar_and_text(tail, flag | bits, ctx, **skw)      # (the same bits without this one: its flag-off call)
            assert base_text == ref
        on_text, pes_on, st_on = cigar_and_text(tail, flag | bits | CGPLAN, ctx, **skw)
        assert ref == on_text, (bits, tail.M._diff(ref, on_text))
        assert st_on == st_off, (bits, st_on, st_off)
        assert [bytes(x) for x in pes_on] == [bytes(x) for x in pes_off]
        lists, n_hits, selected, heavy = bm2.sam_cigar_plan_stats()
        assert lists == 2 * tail.n_pairs and n_hits >= len(tail.aln) and selected >= st_on[0] > 0, (bits, lists, n_hits, selected, st_on)
    return ref


def check_tail_two_contexts(tail, ctx, ctx2, part_knob, combos=COMBOS):
    for k in PART_KNOBS:
        os.environ[k] = str(part_knob)
    try:
        assert tail.n_pairs > part_knob                          # (two parts)
        return check_tail(tail, [ctx, ctx2], combos=combos)
    finally:
        for k in PART_KNOBS:
            del os.environ[k]


def check_tail_options(tail, ctx):
    """MEM_F_NO_RESCUE (-S), MEM_F_ALL (-a), -5"""
    check_tail(tail, ctx, combos=[0, DECIDE], extra=["-S"], flag=0x20)
    check_tail(tail, ctx, combos=[0, PLAN | RESCUE | DECIDE], extra=["-a"], flag=F_ALL)
    check_tail(tail, ctx, combos=[0, PLAN | RESCUE | DECIDE], extra=["-5"], flag=0x800 | 0x1000)
    return True


def check_tail_refusals(tail):
    """the bit without a context"""
    try:
        tail.ours(CGPLAN, None)
    except bm2.Bm2Error as e:
        assert e.rc == bm2.BM2_EINVAL and "DEVICE_CGPLAN" in str(e), e
        return True
    raise AssertionError("accepted")


def check_se_tail(T, d, make_ctx, n_reads=300):
    """bm2_sam_se_dev with the bit (alone and with TEXT; one context, then two sharing the replica) against the flag-off call and the
    reference; bm2_sam_se refuses it.  make_ctx(fa) -> a context holding the index (closed by its maker)"""
    fa, reads = T._case(d, 59, n_reads, L=100)
    names = ["q%d" % i for i in range(len(reads))]
    quals = [b"F" * len(r) for r in reads]
    fq = str(d / "se.fq")
    T._write_fastq(fq, reads, quals)
    ctx = make_ctx(fa)
    ctx2 = bm2.Context(0, share=ctx)
    os.environ["BM2_CGPLAN_PART"] = os.environ["BM2_TEXT_PART"] = str(n_reads // 3)
    try:
        for extra, flag in (([], 0), (["-a"], F_ALL)):
            ref = T._reference_sam(fa, fq, extra)
            off_text = T._ours(fa, reads, names, quals, None, bm2.default_sam_opt(flag=flag), ctx=ctx)
            st_off = bm2.sam_cigar_stats()
            assert ref == off_text, T._diff(ref, off_text)
            assert st_off[0] > 10
            for bits, cx in ((0, ctx), (TEXT, ctx), (0, [ctx, ctx2])):
                on_text = T._ours(fa, reads, names, quals, None, bm2.default_sam_opt(flag=flag | bits | CGPLAN), ctx=cx)
                assert ref == on_text, T._diff(ref, on_text)
                assert bm2.sam_cigar_stats() == st_off, (bm2.sam_cigar_stats(), st_off)
                lists, n_hits, selected, heavy = bm2.sam_cigar_plan_stats()
                assert lists == len(reads) and selected >= st_off[0], (lists, selected, st_off)
        try:
            T._ours(fa, reads, names, quals, None, bm2.default_sam_opt(flag=CGPLAN))
        except bm2.Bm2Error as e:
            assert e.rc == bm2.BM2_EINVAL and "DEVICE_CGPLAN" in str(e), e
        else:
            raise AssertionError("bm2_sam_se accepted the bit")
    finally:
        del os.environ["BM2_CGPLAN_PART"], os.environ["BM2_TEXT_PART"]
        ctx2.close()
    return True
