"""Shared by tests/test_se_mark_emu.py (the device sources on the host emulator) and tests/test_zzzzzzzz_se_mark_gpu.py (the MI355X): the
`decide` phase of the single-end tail on the device -- bm2_se_mark_dev against bm2_se_mark (mem_mark_primary_se and mem_reorder_primary5 as
the host tail runs them) on lists made here, every field of every hit and n_pri, and bm2_sam_se_dev / _multi with
BM2_SAM_F_DEVICE_SEMARK (alone, with CGPLAN, with CGPLAN | TEXT) against the flag-off text and the compiled reference.  Every comparison is
exact; every event a check names is counted from the lists and the oracle's answer, and asserted to occur."""
import ctypes as C
import os

import numpy as np

import bm2

SEMARK, CGPLAN, TEXT = bm2.SAM_F_DEVICE_SEMARK, bm2.SAM_F_DEVICE_CGPLAN, bm2.SAM_F_DEVICE_TEXT
PAIRED_BITS = (bm2.SAM_F_DEVICE_DECIDE, bm2.SAM_F_DEVICE_RESCUE, bm2.SAM_F_DEVICE_PLAN, bm2.SAM_F_DEVICE_PESTAT)
F_ALL, F_PRIMARY5, F_KEEP_SUPP_MAPQ = 0x8, 0x800, 0x1000
INT_MAX = 0x7fffffff
LIGHT_MAX = 16        # hits of a list the 16-lane form takes (semark.hip: SM_LIGHT_MAX)
LDS_CAP = 128         # hits of a list the wavefront form keeps in LDS (SM_HEAVY_LDS)
ROWS = 8              # lists a block of k_sm_light takes (SM_LIGHT_THREADS / 16)
LENGTHS = [0, 1, 2, 15, 16, 17, LDS_CAP - 1, LDS_CAP, LDS_CAP + 1, 4 * LDS_CAP + 7]
BIG_ID = (1 << 33) + 5
FIELDS = [n for n in bm2.ALNREG_DT.names]


# ---- lists: a hit is (qb, qe, score, is_alt, sub_n); everything else of the 96-byte record is noise that must travel with its hit
def arrays(lists, rng, lead=0):
    """-> (hits ALNREG_DT, hit_off): the lists back to back behind `lead` hits that belong to no list; pad = a serial number"""
    n = lead + sum(len(x) for x in lists)
    hits = np.zeros(max(n, 1), bm2.ALNREG_DT)
    for f in ("rb", "re", "rid", "truesc", "sub", "alt_sc", "csub", "w", "seedcov", "secondary", "secondary_all", "seedlen0", "n_comp"):
        hits[f] = rng.integers(0, 1000, size=len(hits))
    hits["frac_rep"] = rng.random(len(hits)).astype(np.float32)
    hits["hash"] = rng.integers(0, 1 << 62, size=len(hits)).astype(np.uint64)
    hits["pad"] = np.arange(1, len(hits) + 1)
    off, at = [lead], lead
    for x in lists:
        for h in x:
            hits["qb"][at], hits["qe"][at], hits["score"][at], hits["is_alt"][at], hits["sub_n"][at] = h
            at += 1
        off.append(at)
    return hits[:n], np.array(off, np.int64)


def random_list(rng, n, p_alt=0.25, lo=20, hi=60):
    """n hits on a read of 150 bases; a narrow score range, so that scores tie and the hash decides"""
    out = []
    for _ in range(n):
        qb = int(rng.integers(0, 110))
        qe = qb + int(rng.integers(20, 150 - qb + 1))
        out.append((qb, qe, int(rng.integers(lo, hi)), int(rng.random() < p_alt), int(rng.integers(0, 4)) if rng.random() < 0.3 else 0))
    return out


def close_of(opt):
    return max(opt.a + opt.b, opt.o_del + opt.e_del, opt.o_ins + opt.e_ins)


def hand_made(opt, so, rng):
    """-> {name: list}: the named cases under this option set (what each is for is asserted in `named_outcomes`)"""
    T, close, ml = int(so.T), close_of(opt), np.float32(opt.mask_level)
    L = {}
    for n in LENGTHS:                                            # every length: all on the assembly, mixed, ALT only
        L["len_%d_noalt" % n] = random_list(rng, n, 0.0)
        L["len_%d_mixed" % n] = random_list(rng, n, 0.3)
        if n in (1, 2, 17, LDS_CAP + 1):
            L["len_%d_altonly" % n] = random_list(rng, n, 1.0)
    # the overlap at mask_level of the shorter stretch, and one base to either side (the shorter stretch: 100 bases, and 101 when the
    # product is no integer)
    for short in (100, 101):
        need = 0
        while not np.float32(need) >= np.float32(short) * ml:   # the smallest overlap that covers, in float as the rule computes it
            need += 1
        for name, ov in (("at", need), ("below", need - 1), ("above", need + 1)):
            L["overlap_%s_%d" % (name, short)] = [(0, 120, 100, 0, 0), (120 - ov, 120 - ov + short, 90, 0, 0)]
    L["sub_stays_0"] = [(0, 100, 50, 0, 0), (0, 100, 0, 0, 0), (5, 100, 0, 0, 0)]
    L["sub_n_close"] = [(0, 100, 100, 0, 0), (0, 100, 100 - close, 0, 0)]
    L["sub_n_close_plus_1"] = [(0, 100, 100, 0, 0), (0, 100, 100 - close - 1, 0, 0)]
    L["sub_n_alt_follower"] = [(0, 100, 100, 0, 0), (0, 100, 100 - close, 1, 0), (0, 90, 20, 0, 0)]      # (the clause: an ALT follower of an assembly leader does not count)
    L["sub_n_alt_leader"] = [(0, 100, 100, 1, 0), (0, 100, 100 - close, 0, 0), (0, 100, 100 - close, 1, 0)]
    L["sub_n_incoming"] = [(0, 100, 100, 0, 5), (0, 100, 99, 0, 7), (0, 100, 98, 0, 0)]
    L["tie_same_alt"] = [(0, 100, 70, 0, 0)] * 5
    L["tie_diff_alt"] = [(0, 100, 70, 1, 0), (0, 100, 70, 0, 0), (0, 100, 70, 1, 0), (0, 100, 70, 0, 0)]
    # an assembly hit shadowed by an ALT leader (alt_sc), ALT followers (secondary = INT_MAX), a leader whose position the second ranking
    # changes (secondary_all renamed)
    L["alt_shadow"] = [(0, 100, 90, 0, 0), (0, 100, 100, 1, 0), (0, 100, 80, 1, 0), (100, 150, 40, 0, 0), (100, 150, 30, 1, 0), (100, 150, 35, 0, 0)]
    # -5: one reportable hit; several with the leftmost first already; several with it elsewhere and followers that name position 0 and
    # the swapped position, through secondary and (an ALT follower) through secondary_all alone; T at the second hit's score and one above
    L["T_edges"] = [(0, 50, T, 0, 0), (60, 110, T - 1, 0, 0)]
    L["p5_one"] =[(40, 150, 100, 0, 0), (45, 150, 90, 0, 0)]
    L["p5_first"] = [(0, 100, 100, 0, 0), (100, 150, max(T, 60), 0, 0), (5, 100, 90, 0, 0)]
    L["p5_swap"] = [(50, 150, 100, 0, 0), (0, 50, 60, 0, 0), (55, 150, 90, 0, 0), (0, 45, 55, 0, 0), (60, 150, 85, 1, 0), (0, 40, 50, 1, 0)]
    L["p5_swap_long"] = L["p5_swap"] + [(52, 150, s, s & 1, 0) for s in range(20, 45)]
    return L


def named_outcomes(name, opt, so, before, after, n_pri, seen):
    """what the named case is for, read off the oracle's answer (before / after: the list's hits; pad names a hit)"""
    def note(k):
        seen[k] = seen.get(k, 0) + 1
    sec = [int(v) for v in after["secondary"]]
    if name.startswith("overlap_"):
        follower = int(np.flatnonzero(after["score"] == 90)[0])
        covered = sec[follower] >= 0
        assert covered == (not name.startswith("overlap_below")), (name, sec)
        note(name[:name.rindex("_")])
    if name == "sub_stays_0":
        assert int(after["sub"][0]) == 0 and sec[1] == 0 and sec[2] == 0, (name, after["sub"], sec)
        note("leader_sub_stays_0")
    if name in ("sub_n_close", "sub_n_close_plus_1", "sub_n_alt_follower", "sub_n_incoming"):
        lead = int(np.flatnonzero(after["score"] == 100)[0])
        want = {"sub_n_close": 1, "sub_n_close_plus_1": 0, "sub_n_alt_follower": 0, "sub_n_incoming": 5 + 2}[name]
        assert int(after["sub_n"][lead]) == want, (name, after["sub_n"])
        note(name)
    if name == "sub_n_alt_leader":                               # the ALT leader counts both followers in the all-hits ranking
        lead = int(np.flatnonzero(after["score"] == 100)[0])
        assert int(after["sub_n"][lead]) == 2 and int(after["is_alt"][lead]) == 1, (name, after["sub_n"])
        note(name)


def events(opt, so, before, after, plain, n_pri, seen):
    """the events of one list, from its hits as they came (before), as the oracle left them (after) and as it leaves them without
    MEM_F_PRIMARY5 (plain)"""
    def note(k):
        seen[k] = seen.get(k, 0) + 1
    n, T, close = len(before), int(so.T), close_of(opt)
    note("len_%d" % n if n in LENGTHS else "len_other")
    if n == 0:
        return
    sc, alt = [int(v) for v in after["score"]], [int(v) for v in after["is_alt"]]
    sec, sa = [int(v) for v in after["secondary"]], [int(v) for v in after["secondary_all"]]
    note("no_alt" if not any(alt) else "only_alt" if all(alt) else "mixed_alt")
    assert n_pri == n - sum(alt)
    by = {}
    for s, a in zip(before["score"], before["is_alt"]):
        by.setdefault(int(s), set()).add(int(a))
    cnt = {}
    for s, a in zip(before["score"], before["is_alt"]):
        cnt[(int(s), int(a))] = cnt.get((int(s), int(a)), 0) + 1
    if any(v > 1 for v in cnt.values()):
        note("tie_same_alt")
    if any(len(v) > 1 for v in by.values()):
        note("tie_diff_alt")
    if (before["sub_n"] != 0).any():
        note("incoming_sub_n")
    for i in range(n):
        if after["alt_sc"][i] > 0:
            assert not alt[i]
            note("alt_sc_set")
        if sec[i] == INT_MAX:
            assert alt[i]
            note("alt_follower_int_max")
        if 0 <= sa[i] and alt[sa[i]] and sa[i] >= n_pri and any(not alt[j] and sc[j] < sc[sa[i]] for j in range(sa[i])):
            note("secondary_all_renamed")                        # (its leader ranked before an assembly hit that now stands in front of it)
        if 0 <= sec[i] < n:
            d = sc[sec[i]] - sc[i]
            if after["sub"][sec[i]] == 0:
                note("leader_sub_0_with_follower")
            if d == close:
                note("diff_eq_close")
            if d == close + 1:
                note("diff_eq_close_plus_1")
        if sec[i] < 0 and not alt[i]:
            if sc[i] == T:
                note("primary_at_T")
            if sc[i] == T - 1:
                note("primary_at_T_minus_1")
    if so.flag & F_PRIMARY5:
        reportable = [k for k in range(n) if plain["secondary"][k] < 0 and not plain["is_alt"][k] and plain["score"][k] >= T]
        if len(reportable) == 1:
            note("p5_one_reportable")
        if len(reportable) > 1:
            left = min(reportable, key=lambda k: (int(plain["qb"][k]), k))
            if left == 0:
                assert after.tobytes() == plain.tobytes()
                note("p5_leftmost_first")
            else:
                assert after["pad"][0] == plain["pad"][left] and after["pad"][left] == plain["pad"][0]
                note("p5_swapped")
                for k in range(1, n):
                    for f in ("secondary", "secondary_all"):
                        if plain[f][k] == 0:
                            assert after[f][k] == left
                            note("p5_%s_named_0" % f)
                        if plain[f][k] == left:
                            assert after[f][k] == 0
                            note("p5_%s_named_swapped" % f)


def same(a, b, what):
    if a.tobytes() == b.tobytes():
        return
    for f in FIELDS:
        bad = np.flatnonzero(a[f] != b[f])
        assert len(bad) == 0, (what, f, bad[:5], a[f][bad[:5]], b[f][bad[:5]])
    raise AssertionError((what, "bytes differ"))


def heavy_lists(hit_off):
    return int((np.diff(np.asarray(hit_off)) > LIGHT_MAX).sum())


def compare(ctx, opt, so, hits, hit_off, first_id, what=""):
    """device == host, every field of every hit and n_pri; hits outside the lists untouched; the device's counters -> (host's hits, n_pri)"""
    host, dev = hits.copy(), hits.copy()
    np_host = bm2.se_mark(opt, so, host, hit_off, first_id)
    np_dev = ctx.se_mark(opt, so, dev, hit_off, first_id)
    same(dev, host, what)
    assert (np_dev == np_host).all(), (what, np.flatnonzero(np_dev != np_host)[:5])
    b, e = int(hit_off[0]), int(hit_off[-1])
    assert host[:b].tobytes() == hits[:b].tobytes() and host[e:].tobytes() == hits[e:].tobytes()
    assert sorted(host["pad"][b:e]) == sorted(hits["pad"][b:e])
    n_lists = len(hit_off) - 1
    assert bm2.sam_se_mark_stats() == ((n_lists, e - b, heavy_lists(hit_off)) if n_lists else (0, 0, 0)), (what, bm2.sam_se_mark_stats())
    return host, np_host


OPTION_SETS = [({}, {}), ({}, dict(flag=F_PRIMARY5)), ({}, dict(flag=F_PRIMARY5, T=60)), ({}, dict(flag=F_PRIMARY5, T=61)),
               (dict(mask_level=0.3, b=2, o_del=3, o_ins=3), dict(flag=F_PRIMARY5 | F_ALL))]
WANTED = (["len_%d" % n for n in LENGTHS] +
          ["no_alt", "only_alt", "mixed_alt", "tie_same_alt", "tie_diff_alt", "incoming_sub_n", "alt_sc_set", "alt_follower_int_max", "secondary_all_renamed",
           "leader_sub_0_with_follower", "leader_sub_stays_0", "diff_eq_close", "diff_eq_close_plus_1", "sub_n_close", "sub_n_close_plus_1",
           "sub_n_alt_follower", "sub_n_alt_leader", "sub_n_incoming", "overlap_at", "overlap_below", "overlap_above",
           "primary_at_T", "primary_at_T_minus_1", "p5_one_reportable", "p5_leftmost_first", "p5_swapped",
           "p5_secondary_named_0", "p5_secondary_named_swapped", "p5_secondary_all_named_0", "p5_secondary_all_named_swapped",
           "id_64_bits_matter", "empty_between_full", "hit_off_not_from_0"])


def check_lists(ctx, quick=False):
    """bm2_se_mark_dev against bm2_se_mark on the named lists and random ones, under every option set, first_id 0 and above 2^32"""
    total = {}
    for k, (okw, skw) in enumerate(OPTION_SETS):
        if quick and k == 3:                                     # (quick: T one above the score is left to the long form; T at the score stays)
            continue
        opt, so = bm2.default_opt(**okw), bm2.default_sam_opt(**skw)
        plain_so = bm2.default_sam_opt(**dict(skw, flag=skw.get("flag", 0) & ~F_PRIMARY5))
        rng = np.random.default_rng(300 + k)
        seen = {}
        named = hand_made(opt, so, rng)
        names, lists = [], []
        for nm, x in named.items():                              # an empty list between full ones, now and then
            names.append(nm)
            lists.append(x)
            if len(lists) % 5 == 0:
                names.append("")
                lists.append([])
                seen["empty_between_full"] = seen.get("empty_between_full", 0) + 1
        for lead, first_id in ((0, 0), (7, BIG_ID)):
            hits, hit_off = arrays(lists, rng, lead)
            if lead:
                seen["hit_off_not_from_0"] = seen.get("hit_off_not_from_0", 0) + 1
            what = "set %d, lead %d, first_id %d" % (k, lead, first_id)
            host, n_pri = compare(ctx, opt, so, hits, hit_off, first_id, what)
            plain = hits.copy()
            bm2.se_mark(opt, plain_so, plain, hit_off, first_id)
            for li, nm in enumerate(names):
                b, e = int(hit_off[li]), int(hit_off[li + 1])
                events(opt, so, hits[b:e], host[b:e], plain[b:e], int(n_pri[li]), seen)
                named_outcomes(nm, opt, so, hits[b:e], host[b:e], int(n_pri[li]), seen)
            if first_id > 0xffffffff:                            # the same lists under the id's low 32 bits alone: another order somewhere
                low = hits.copy()
                bm2.se_mark(opt, so, low, hit_off, first_id & 0xffffffff)
                if (low["pad"] != host["pad"]).any():
                    seen["id_64_bits_matter"] = seen.get("id_64_bits_matter", 0) + 1
        for ev, c in seen.items():
            total[ev] = total.get(ev, 0) + c
    missing = [ev for ev in WANTED if not total.get(ev)]
    assert not missing, (missing, total)
    return total


def dump_lists(path):
    """the hand-made lists of check_lists under every option set, as tools/san/se_mark_san.cpp reads them (no device involved): a header
    (batches and the three struct sizes), then per batch the option structs, (lists, first_id, hits), the offsets, the hits -> batches"""
    sets = []
    for k, (okw, skw) in enumerate(OPTION_SETS):
        opt, so = bm2.default_opt(**okw), bm2.default_sam_opt(**skw)
        rng = np.random.default_rng(300 + k)
        lists = []
        for x in hand_made(opt, so, rng).values():
            lists.append(x)
            if len(lists) % 5 == 0:
                lists.append([])
        for lead, first_id in ((0, 0), (7, BIG_ID)):
            hits, hit_off = arrays(lists, rng, lead)
            sets.append((opt, so, first_id, hits, hit_off))
    with open(path, "wb") as f:
        f.write(np.array([len(sets), C.sizeof(bm2.Opt), C.sizeof(bm2.SamOpt), bm2.ALNREG_DT.itemsize], np.int64).tobytes())
        for opt, so, first_id, hits, hit_off in sets:
            f.write(bytes(opt) + bytes(so))
            f.write(np.array([len(hit_off) - 1, first_id, len(hits)], np.int64).tobytes())
            f.write(hit_off.tobytes() + hits.tobytes())
    return len(sets)


def check_batches(ctx):
    """1, 7, 8, 9 lists (a block of k_sm_light takes 8) and 8 blocks + 1; only heavy lists, no heavy list; no list at all"""
    opt, so = bm2.default_opt(), bm2.default_sam_opt(flag=F_PRIMARY5)
    rng = np.random.default_rng(8)
    done = []
    for n in (1, ROWS - 1, ROWS, ROWS + 1, 8 * ROWS + 1):
        lists = [random_list(rng, int(rng.integers(0, LIGHT_MAX + 1))) for _ in range(n)]
        lists[-1] = random_list(rng, LIGHT_MAX)                  # (the last row of the last block works)
        hits, hit_off = arrays(lists, rng, 3)
        compare(ctx, opt, so, hits, hit_off, 11, "%d light lists" % n)
        assert bm2.sam_se_mark_stats()[2] == 0
        done.append(n)
    for n in (1, 3):
        lists = [random_list(rng, m) for m in (LIGHT_MAX + 1, LDS_CAP, LDS_CAP + 3)[:n]]
        hits, hit_off = arrays(lists, rng)
        compare(ctx, opt, so, hits, hit_off, 0, "%d heavy lists" % n)
        assert bm2.sam_se_mark_stats()[2] == n
    lists = [random_list(rng, m) for m in (LDS_CAP + 1, 3, 2 * LDS_CAP, 0, 40, LDS_CAP + 9, 16, 17)]      # two lists in the global workspace, not adjacent
    hits, hit_off = arrays(lists, rng, 2)
    compare(ctx, opt, so, hits, hit_off, 5, "mixed forms")
    hits, hit_off = arrays([[], [], []], rng, 2)                 # lists, and no hit in any
    compare(ctx, opt, so, hits, hit_off, 5, "empty lists only")
    return done


def check_arguments(ctx):
    opt, so = bm2.default_opt(), bm2.default_sam_opt()
    rng = np.random.default_rng(9)
    lists = [random_list(rng, n) for n in (3, 0, 40, 7, 150, 1)]
    hits, hit_off = arrays(lists, rng, 5)
    L = bm2.lib()
    L.bm2_se_mark.restype = L.bm2_se_mark_dev.restype = C.c_int
    forms = (("host", L.bm2_se_mark, ()), ("device", L.bm2_se_mark_dev, (C.c_void_p(ctx.h),)))

    def call(fn, head, a, off, n_lists, n_pri):
        return fn(*head, C.byref(opt), C.byref(so), C.c_int32(n_lists), C.c_void_p(a.ctypes.data), C.c_void_p(off.ctypes.data), C.c_int64(3),
                  C.c_void_p(n_pri.ctypes.data if n_pri is not None else None))
    want = hits.copy()
    want_pri = bm2.se_mark(opt, so, want, hit_off, 3)
    for who, fn, head in forms:
        for bad_off in (np.array([5, 8, 7, 9], np.int64), np.array([-1, 2, 3], np.int64), np.array([4, 3], np.int64)):      # decreasing, negative
            a = hits.copy()
            assert call(fn, head, a, bad_off, len(bad_off) - 1, None) == bm2.BM2_EINVAL, who
            assert b"hit_off" in L.bm2_last_error(), (who, L.bm2_last_error())
            assert a.tobytes() == hits.tobytes()
        a = hits.copy()                                          # no list: success, nothing touched
        pri = np.full(4, -7, np.int32)
        assert call(fn, head, a, hit_off[:1].copy(), 0, pri) == bm2.BM2_OK, who
        assert a.tobytes() == hits.tobytes() and (pri == -7).all()
        a = hits.copy()                                          # n_pri == NULL
        assert call(fn, head, a, hit_off, len(lists), None) == bm2.BM2_OK, (who, L.bm2_last_error())
        same(a, want, who + ", n_pri == NULL")
    a = hits.copy()
    assert (ctx.se_mark(opt, so, a, hit_off, 3) == want_pri).all()
    assert bm2.sam_se_mark_stats() == (len(lists), int(hit_off[-1] - hit_off[0]), 2)
    bare = bm2.Context(0, None)                                  # a context without an index will do
    try:
        a = hits.copy()
        assert (bare.se_mark(opt, so, a, hit_off, 3) == want_pri).all()
        same(a, want, "a context without an index")
    finally:
        bare.close()
    return True


# ---- the tail with the bit
class SeTail:
    """One single-end input through the tail many times: the hits (oracle + bm2_finish_regs: no GPU involved) are made once.
    T = the test_sam_tail module."""

    def __init__(self, T, d, n_reads):
        oracle, refio, oracle_finish_regs = T.oracle, T.refio, T.oracle_finish_regs
        self.T = T
        self.fa, self.reads = T._case(d, 41, n_reads)
        self.names = ["q%d" % i for i in range(len(self.reads))]
        self.quals = [b"F" * len(r) for r in self.reads]
        self.fq = str(d / "r.fq")
        T._write_fastq(self.fq, self.reads, self.quals)
        self.enc, self.off, self.ln = refio.pack_reads(self.reads)
        ix = oracle.Index(self.fa)
        try:
            exp = ix.run(self.enc, self.off, self.ln, oracle.default_opt())
        finally:
            ix.close()
        self.opt = bm2.default_opt()
        regs, reg_off = T._prg_to_regs(exp["REGPRG"], len(self.ln))
        self.aln, self.aln_off = oracle_finish_regs(self.fa, self.enc, self.off, self.ln, self.opt, regs, reg_off)

    def ours(self, flag, ctx, paired=False, **skw):
        f = bm2.sam_pe if paired else bm2.sam_se
        return f(self.fa, self.enc, self.off, self.ln, self.opt, self.aln, self.aln_off, self.names, self.quals, None,
                 bm2.default_sam_opt(flag=flag, **skw), ctx=ctx)


def check_se_tail(T, d, make_ctx, n_reads):
    """bm2_sam_se_dev with the bit -- alone, with CGPLAN, with CGPLAN | TEXT; one context, then two sharing the replica with
    BM2_SEMARK_PART at a third of the reads; no option, -a, -T 50 -5 -- against the flag-off call (text, planned / used / missed) and the
    reference; the refusals.  make_ctx(fa) -> a context holding the index (closed by its maker)"""
    tail = SeTail(T, d, n_reads)
    assert len(tail.reads) % 2 == 0
    ctx = make_ctx(tail.fa)
    ctx2 = bm2.Context(0, share=ctx)
    knobs = ("BM2_SEMARK_PART", "BM2_CGPLAN_PART", "BM2_TEXT_PART")
    for k in knobs:
        os.environ[k] = str(n_reads // 3)
    try:
        for extra, flag, Tmin in (([], 0, 30), (["-a"], F_ALL, 30), (["-T", "50", "-5"], F_PRIMARY5 | F_KEEP_SUPP_MAPQ, 50)):
            ref = T._reference_sam(tail.fa, tail.fq, extra)
            off_text = tail.ours(flag, ctx, T=Tmin)
            st_off = bm2.sam_cigar_stats()
            assert ref == off_text, T._diff(ref, off_text)
            assert st_off[0] > 10
            for bits in (SEMARK, SEMARK | CGPLAN, SEMARK | CGPLAN | TEXT):
                for cx in (ctx, [ctx, ctx2]):
                    on_text = tail.ours(flag | bits, cx, T=Tmin)
                    assert ref == on_text, (bits, T._diff(ref, on_text))
                    assert bm2.sam_cigar_stats() == st_off, (bits, bm2.sam_cigar_stats(), st_off)
                    lists, n_hits, heavy = bm2.sam_se_mark_stats()
                    assert lists == len(tail.reads) and n_hits == int(tail.aln_off[-1] - tail.aln_off[0]), (bits, lists, n_hits)
                    if bits & CGPLAN:
                        assert bm2.sam_cigar_plan_stats()[0] == lists and bm2.sam_cigar_plan_stats()[2] >= st_off[0]
        # the refusals: bm2_sam_se has no context; the paired tail in its three forms; the five paired bits stay refused here
        for who, f, word in (("bm2_sam_se", lambda: tail.ours(SEMARK, None), "needs a context"),
                             ("bm2_sam_pe", lambda: tail.ours(SEMARK, None, paired=True), "a flag of the single-end tail"),
                             ("bm2_sam_pe_dev", lambda: tail.ours(SEMARK, ctx, paired=True), "a flag of the single-end tail"),
                             ("bm2_sam_pe_dev_multi", lambda: tail.ours(SEMARK, [ctx, ctx2], paired=True), "a flag of the single-end tail")):
            try:
                f()
            except bm2.Bm2Error as e:
                assert e.rc == bm2.BM2_EINVAL and "BM2_SAM_F_DEVICE_SEMARK" in str(e) and word in str(e), (who, e)
            else:
                raise AssertionError("%s accepted the bit" % who)
        for bit in PAIRED_BITS:
            try:
                tail.ours(SEMARK | bit, ctx)
            except bm2.Bm2Error as e:
                assert e.rc == bm2.BM2_EINVAL and "a flag of the paired tail" in str(e), e
            else:
                raise AssertionError("bm2_sam_se_dev accepted a paired bit")
    finally:
        for k in knobs:
            del os.environ[k]
        ctx2.close()
    return True


def tail_phases(T, d, make_ctx, n_reads):
    """one call with SEMARK | CGPLAN (for BM2_TAIL_PROF=1 in the environment: the caller reads stderr)"""
    tail = SeTail(T, d, n_reads)
    tail.ours(SEMARK | CGPLAN, make_ctx(tail.fa))
    return bm2.sam_se_mark_stats()
