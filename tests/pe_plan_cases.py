"""Shared by tests/test_pe_plan_emu.py (the device sources on the host emulator) and tests/test_zzzzz_pe_plan_gpu.py (the MI355X): mate
rescue planned on the device -- bm2_pe_rescue_plan_dev against bm2_pe_rescue_plan on lists made here, bm2_pe_rescue_queries in both
forms against a construction in numpy, and the tail with BM2_SAM_F_DEVICE_PLAN (alone and with every subset of the three other device
bits) against the flag-off tail and the compiled reference.  Every comparison is exact and covers every pair: the tasks' bytes, task_off,
n_out, every byte of every query."""
import ctypes as C
import os

import numpy as np

import bm2
import pe_decide_cases as D
import pe_rescue_cases as R

READ_LENS = (1, 30, 150, 251)
PLAN, RESCUE, DECIDE, TEXT = bm2.SAM_F_DEVICE_PLAN, bm2.SAM_F_DEVICE_RESCUE, bm2.SAM_F_DEVICE_DECIDE, bm2.SAM_F_DEVICE_TEXT
SUBSETS = [0, RESCUE, DECIDE, TEXT, RESCUE | DECIDE, RESCUE | TEXT, DECIDE | TEXT, RESCUE | DECIDE | TEXT]
PART_KNOBS = ("BM2_PLAN_PART", "BM2_KSW_PART", "BM2_RESCUE_PART", "BM2_DECIDE_PART", "BM2_TEXT_PART")

# insert-size models beside pe_decide_cases.ALL4 / FR: windows below 0 and beyond 2 l_pac (g60k: l_pac = 64000), and windows that are
# shorter than min_seed_len whatever the anchor (high - low + l_ms = 11 with a mate of one base)
HUGE = {d: (0, 70000, 35000.0, 9000.0) for d in range(4)}
NARROW = {d: (100, 110, 105.0, 2.0) for d in range(4)}


def read_lengths(n_pairs):
    """1, 30, 150 and 251, unequal within every pair"""
    ln = np.zeros(2 * n_pairs, np.int32)
    ln[0::2] = [READ_LENS[p % 4] for p in range(n_pairs)]
    ln[1::2] = [READ_LENS[(p + 1 + p // 4 % 3) % 4] for p in range(n_pairs)]
    assert (ln[0::2] != ln[1::2]).all()
    return ln


def infer_dir(l_pac, b1, b2):
    """mem_infer_dir, bwamem_pair.cpp:58-65"""
    r1, r2 = b1 >= l_pac, b2 >= l_pac
    p2 = b2 if r1 == r2 else 2 * l_pac - 1 - b2
    return (0 if r1 == r2 else 1) ^ (0 if p2 > b1 else 3), (p2 - b1 if p2 > b1 else b1 - p2)


def window(G, pes, min_seed_len, a_rb, a_rid, l_ms, r):
    """mem_matesw's window for direction r of an anchor (bwamem_pair.cpp:176-186 with bns_fetch_seq's clamp to the contig of the
    window's midpoint) -> (outcome, rb, re, the events met on the way)"""
    offs, lens, l_pac = G
    is_rev, is_larger = (r >> 1) != (r & 1), not (r >> 1)
    low, high = pes[r].low, pes[r].high
    if not is_rev:
        rb = a_rb + low if is_larger else a_rb - high
        re = (a_rb + high if is_larger else a_rb - low) + l_ms
    else:
        rb = (a_rb + low if is_larger else a_rb - high) - l_ms
        re = a_rb + high if is_larger else a_rb - low
    ev = set()
    if rb < l_pac < re:
        ev.add("junction")
    if rb < 0:
        rb = 0
        ev.add("below_zero")
    if re > 2 * l_pac:
        re = 2 * l_pac
        ev.add("beyond_2_l_pac")
    if rb >= re:
        return "empty", rb, re, ev
    mid = (rb + re) >> 1
    rev = mid >= l_pac
    rid = int(np.searchsorted(offs, 2 * l_pac - 1 - mid if rev else mid, side="right")) - 1
    fb, fe = int(offs[rid]), int(offs[rid] + lens[rid])
    if rev:
        fb, fe = 2 * l_pac - fe, 2 * l_pac - fb
    strand = "rev" if rev else "fwd"
    if rb < fb:
        rb = fb
        ev.add("clamp_start_" + strand)
    if re > fe:
        re = fe
        ev.add("clamp_end_" + strand)
    if rid != a_rid:
        return "contig_mismatch", rb, re, ev
    if re - rb < min_seed_len:
        return "short", rb, re, ev
    return "ok", rb, re, ev


def plan_in_python(G, opt, so, hits, hit_off, read_len, pes, skip_above=200):
    """rescue_plan of the host tail written again with Python integers -> ({pair: [(end, j, r, rb, re)]}, a count per event of the
    issue's list).  Pairs with a list above skip_above hits are left out (None): the heavy pair is compared device against host only."""
    l_pac = G[2]
    seen = dict(served=0, cap_bites=0, contig_mismatch=0, short=0, empty=0, junction=0, below_zero=0, beyond_2_l_pac=0, clamp_start_fwd=0,
                clamp_end_fwd=0, clamp_start_rev=0, clamp_end_rev=0)
    out = {}
    for p in range((len(hit_off) - 1) // 2):
        lists = [hits[hit_off[2 * p + e]:hit_off[2 * p + e + 1]] for e in range(2)]
        if max(len(lists[0]), len(lists[1])) > skip_above:
            out[p] = None
            continue
        tasks = []
        for e in range(2):
            a, m = lists[e], lists[1 - e]
            if not len(a):
                continue
            cand = [k for k in range(len(a)) if int(a["score"][k]) >= int(a["score"][0]) - so.pen_unpaired]
            seen["cap_bites"] += len(cand) > so.max_matesw > 0
            m_rb = [int(x) for x in m["rb"]]
            for j, k in enumerate(cand[:max(so.max_matesw, 0)]):
                a_rb, a_rid = int(a["rb"][k]), int(a["rid"][k])
                served = set()
                for b2 in m_rb:
                    r, dist = infer_dir(l_pac, a_rb, b2)
                    if pes[r].low <= dist <= pes[r].high:
                        served.add(r)
                for r in range(4):
                    if pes[r].failed:
                        continue
                    if r in served:
                        seen["served"] += 1
                        continue
                    what, rb, re, ev = window(G, pes, opt.min_seed_len, a_rb, a_rid, int(read_len[2 * p + 1 - e]), r)
                    for x in ev:
                        seen[x] += 1
                    if what == "ok":
                        tasks.append((e, j, r, rb, re))
                    else:
                        seen[what] += 1
        out[p] = tasks
    return out, seen


def compare(ctx, prefix, opt, so, hits, hit_off, read_len, pes, what=""):
    """bm2_pe_rescue_plan_dev against bm2_pe_rescue_plan: the tasks' bytes, task_off, n_out -> the host's (tasks, task_off)"""
    h_t, h_off = bm2.pe_rescue_plan(prefix, opt, so, hits, hit_off, read_len, pes)
    d_t, d_off = ctx.pe_rescue_plan(opt, so, hits, hit_off, read_len, pes)
    st = bm2.sam_rescue_plan_stats()
    assert len(h_t) == len(d_t), "%s: %d tasks on the host, %d on the device" % (what, len(h_t), len(d_t))
    if (h_off != d_off).any():
        p = int(np.nonzero(h_off != d_off)[0][0]) - 1
        assert False, "%s: pair %d has %d tasks on the host, %d on the device" % (what, p, h_off[p + 1] - h_off[p], d_off[p + 1] - d_off[p])
    if h_t.tobytes() != d_t.tobytes():
        for i in range(len(h_t)):
            assert h_t[i].tobytes() == d_t[i].tobytes(), "%s: task %d\n  fields %s\n  host   %s\n  device %s" % (what, i, h_t.dtype.names, h_t[i], d_t[i])
    assert not h_t["res"].any() and not h_t["pad"].any()
    assert st == ((len(hit_off) - 1) // 2, len(h_t), 0), st
    return h_t, h_off


class Lists(R.Lists):
    """pe_rescue_cases.Lists plus pairs whose second read has no hit: every live direction of the anchor is open"""

    def lone(self, contig, pos, rev=False, n=1):
        self.end_list([self.hit(contig, pos + 3 * k, rev, 0, 150, 140 - k) for k in range(n)])
        self.end_list([])

    def lone_second(self, contig, pos, rev=False):
        self.end_list([])
        self.end_list([self.hit(contig, pos, rev, 0, 150, 140)])


def edge_pairs(M):
    """anchors beside both ends of every contig on both strands (windows cross contig ends, the ends of the doubled reference and the
    forward / reverse junction; beside a contig's start the windows of the `smaller` directions have their midpoint on the contig
    before), and anchors 350 bases into a contig (with min_seed_len 400 the clamped window is too short)"""
    for contig in range(len(M.off)):
        last = int(M.len[contig])
        for rev in (False, True):
            for pos in (5, 350, last - 350, last - 160):
                M.lone(contig, pos, rev)
                M.lone_second(contig, pos, rev)


def check_plan(ctx, prefix, quick=False):
    """Item 1 of the issue.  quick: the emulator's share (fewer random pairs per configuration)."""
    offs, lens = D.contigs(prefix)
    with bm2.Index(prefix) as ix:
        l_pac = ix.l_pac
    G = (offs, lens, l_pac)
    configs = [
        ("all orientations", {}, {}, D.ALL4, 41, {}),
        ("FR only, -m 3, equal scores", {}, dict(max_matesw=3), D.FR, 42, dict(equal_scores=True)),
        ("-m 1, -U 0", {}, dict(max_matesw=1, pen_unpaired=0), D.ALL4, 43, dict(equal_scores=True)),
        ("min_seed_len 400", dict(min_seed_len=400), {}, D.ALL4, 44, {}),
        ("all failed", {}, {}, {}, 45, {}),
        ("windows below 0 and beyond 2 l_pac", {}, {}, HUGE, 46, {}),
        ("windows shorter than min_seed_len", {}, {}, NARROW, 47, {}),
    ] + [("orientation %d failed" % d, {}, {}, {k: v for k, v in D.ALL4.items() if k != d}, 50 + d, {}) for d in range(4)]
    total, by_r, by_end, j_max = dict(), set(), set(), 0
    for ci, (name, okw, skw, models, seed, mk) in enumerate(configs):
        M = Lists(prefix, 3000 + seed)
        sizes = D.size_mix(big=False)
        for n0, n1 in sizes[::3] if quick else sizes:
            M.pair(n0, n1, **mk)
        M.pair(0, 0)
        edge_pairs(M)
        if ci == 0:
            M.pair(60, 700, equal_scores=True)                   # the heavy pair: 50 candidates (the cap bites) x 700 hits of the mate
            M.pair(700, 2, equal_scores=True)
        hits, hit_off = M.arrays()
        n_pairs = (len(hit_off) - 1) // 2
        read_len = read_lengths(n_pairs)
        opt, so, pes = bm2.default_opt(**okw), bm2.default_sam_opt(**skw), D.pestat(models)
        tasks, task_off = compare(ctx, prefix, opt, so, hits, hit_off, read_len, pes, name)
        if not models:
            assert len(tasks) == 0, name
        for d in range(4):
            assert d in models or not (tasks["r"] == d).any(), (name, d)
        # the host's tasks are what the rules say, pair by pair (and so the events counted on the way did happen)
        mine, seen = plan_in_python(G, opt, so, hits, hit_off, read_len, pes)
        for p in range(n_pairs):
            if mine[p] is None:
                continue
            T = tasks[task_off[p]:task_off[p + 1]]
            got = list(zip(T["end"].tolist(), T["j"].tolist(), T["r"].tolist(), T["rb"].tolist(), T["re"].tolist()))
            assert got == mine[p] and (T["pair"] == p).all(), "%s: pair %d\n  host  %s\n  rules %s" % (name, p, got, mine[p])
        if ci == 0:
            heavy = [p for p in range(n_pairs) if mine[p] is None]
            assert len(heavy) == 2, heavy
            for p in heavy:                                      # more candidates than max_matesw in the long list: no task beyond the cap
                T = tasks[task_off[p]:task_off[p + 1]]
                assert 2 <= int(T["j"].max()) < so.max_matesw and len(T) > 20, (p, len(T))
        if so.max_matesw < 50:
            assert seen["cap_bites"] > 0 and int(tasks["j"].max()) == so.max_matesw - 1, (name, seen)
        if name.startswith("windows shorter"):
            assert seen["short"] > 0, (name, seen)
        if models is HUGE:
            assert seen["below_zero"] > 0 and seen["beyond_2_l_pac"] > 0, (name, seen)
        for k, v in seen.items():
            total[k] = total.get(k, 0) + v
        by_r |= set(tasks["r"].tolist())
        by_end |= set(tasks["end"].tolist())
        j_max = max(j_max, int(tasks["j"].max(initial=0)))
    assert by_r == {0, 1, 2, 3} and by_end == {0, 1} and j_max >= 2, (by_r, by_end, j_max)
    missing = [k for k, v in total.items() if v == 0 and k != "empty"]
    assert not missing, "the inputs never reach: %s (%s)" % (missing, total)
    return total


def check_sizes(ctx, prefix):
    """n_pairs 0, 1, 255, 256, 257 and 5000 (block and scan-tile edges): prefixes of one batch of small lists"""
    M = Lists(prefix, 77)
    for p in range(5000):
        if p % 50 == 7:
            M.lone(p % 4, 5 + p % 300, rev=bool(p & 64))
        else:
            M.pair(p % 5, (p // 5 + p // 3) % 4)
    hits, hit_off = M.arrays()
    read_len = read_lengths(5000)
    opt, so, pes = bm2.default_opt(), bm2.default_sam_opt(), D.pestat(D.ALL4)
    counts = {}
    for n in (0, 1, 255, 256, 257, 5000):
        t, off = compare(ctx, prefix, opt, so, hits[:hit_off[2 * n]], hit_off[:2 * n + 1], read_len[:2 * n], pes, "%d pairs" % n)
        assert len(off) == n + 1 and off[n] == len(t)
        counts[n] = len(t)
    assert counts[0] == 0 and counts[5000] > 5000, counts
    return counts


def check_ecap(ctx, prefix):
    """Item 2: cap = n - 1 and cap = 0 -- the return code, *n_out, task_off and the tasks below cap equal the host's"""
    M = Lists(prefix, 78)
    for n0, n1 in D.size_mix(big=False)[::2]:
        M.pair(n0, n1)
    edge_pairs(M)
    hits, hit_off = M.arrays()
    read_len = read_lengths((len(hit_off) - 1) // 2)
    opt, so, pes = bm2.default_opt(), bm2.default_sam_opt(), D.pestat(D.ALL4)
    full, full_off = compare(ctx, prefix, opt, so, hits, hit_off, read_len, pes, "ecap")
    n = len(full)
    assert n > 50
    for cap in (n - 1, 0):
        h_rc, h_t, h_off, h_n = bm2.pe_rescue_plan(prefix, opt, so, hits, hit_off, read_len, pes, cap=cap)
        d_rc, d_t, d_off, d_n = ctx.pe_rescue_plan(opt, so, hits, hit_off, read_len, pes, cap=cap)
        assert h_rc == d_rc == bm2.BM2_ECAP, (cap, h_rc, d_rc)
        assert h_n == d_n == n, (cap, h_n, d_n, n)
        assert (h_off == full_off).all() and (d_off == full_off).all(), cap
        assert h_t.tobytes() == d_t.tobytes() == full[:cap].tobytes(), cap
    rc, t, off, got = ctx.pe_rescue_plan(opt, so, hits, hit_off, read_len, pes, cap=n)       # exactly enough
    assert rc == bm2.BM2_OK and got == n and t.tobytes() == full.tobytes()
    return n


def check_refusals(ctx, prefix):
    """Item 3: NULL arguments, a context without an index, a decreasing hit_off -- BM2_EINVAL, and nothing ran (the counters of the
    last call that did run stay)"""
    M = Lists(prefix, 5)
    for _ in range(6):
        M.pair(4, 0)
        M.pair(3, 2)
    hits, hit_off = M.arrays()
    n_pairs = (len(hit_off) - 1) // 2
    read_len = read_lengths(n_pairs)
    opt, so, pes = bm2.default_opt(), bm2.default_sam_opt(), D.pestat(D.ALL4)
    tasks, task_off = compare(ctx, prefix, opt, so, hits, hit_off, read_len, pes, "refusals")
    before = bm2.sam_rescue_plan_stats()
    assert before == (n_pairs, len(tasks), 0) and len(tasks) > 0

    def refused(word, f):
        try:
            f()
        except bm2.Bm2Error as e:
            assert e.rc == bm2.BM2_EINVAL and word in str(e), (word, e)
            assert bm2.sam_rescue_plan_stats() == before
            return
        raise AssertionError("accepted: " + word)
    bad_off = hit_off.copy()
    bad_off[1] = hit_off[2] + 1
    refused("hit_off", lambda: ctx.pe_rescue_plan(opt, so, hits, bad_off, read_len, pes))
    bare = bm2.Context(0, None)
    try:
        refused("no index", lambda: bare.pe_rescue_plan(opt, so, hits, hit_off, read_len, pes))
    finally:
        bare.close()
    L = bm2.lib()
    room = np.zeros(len(tasks) + 1, bm2.RESCUE_TASK_DT)
    off = np.zeros(n_pairs + 1, np.int64)
    need = C.c_int64(0)
    pq = (bm2.PeStat * 4)(*pes)
    good = [C.c_void_p(ctx.h), C.byref(opt), C.byref(so), C.c_int32(n_pairs), C.c_void_p(hits.ctypes.data), C.c_void_p(hit_off.ctypes.data),
            C.c_void_p(read_len.ctypes.data), pq, C.c_void_p(room.ctypes.data), C.c_int64(len(room)), C.c_void_p(off.ctypes.data), C.byref(need)]
    L.bm2_pe_rescue_plan_dev.restype = C.c_int
    assert L.bm2_pe_rescue_plan_dev(*good) == bm2.BM2_OK and need.value == len(tasks) and room[:len(tasks)].tobytes() == tasks.tobytes()
    for k in (0, 1, 2, 4, 5, 6, 7, 8, 10, 11):                  # every pointer in turn (hits: NULL with a non-empty batch)
        args = list(good)
        args[k] = None
        assert L.bm2_pe_rescue_plan_dev(*args) == bm2.BM2_EINVAL, k
        assert b"bad argument" in L.bm2_last_error() and bm2.sam_rescue_plan_stats() == before, k
    for k, v in ((3, C.c_int32(-1)), (9, C.c_int64(-1))):
        args = list(good)
        args[k] = v
        assert L.bm2_pe_rescue_plan_dev(*args) == bm2.BM2_EINVAL, k
    e_t, e_off = ctx.pe_rescue_plan(opt, so, hits[:0], np.zeros(1, np.int64), read_len[:0], pes)
    assert len(e_t) == 0 and e_off.tolist() == [0]
    return True


def check_queries(ctx):
    """Item 4: reads with N's, lengths 1 .. 251, every direction, both ends -- device = host = numpy"""
    rng = np.random.default_rng(91)
    ln = np.array(list(range(1, 252)) + [77], np.int32)
    off = np.concatenate([[3], 3 + np.cumsum(ln[:-1])]).astype(np.int64)                   # (codes that start at no aligned address)
    enc = rng.integers(0, 4, int(off[-1] + ln[-1]) + 5).astype(np.uint8)
    enc[rng.random(len(enc)) < 0.1] = 4
    n_pairs = len(ln) // 2
    tasks = np.zeros(n_pairs * 8, bm2.RESCUE_TASK_DT)
    tasks["pair"] = np.repeat(np.arange(n_pairs), 8)
    tasks["end"] = np.tile(np.repeat([0, 1], 4), n_pairs)
    tasks["r"] = np.tile(np.arange(4), 2 * n_pairs)
    tasks["rb"], tasks["re"], tasks["j"] = 12345, 23456, 7       # (not read)
    want, want_off = [], [0]
    for T in tasks:
        m = 2 * int(T["pair"]) + 1 - int(T["end"])
        q = enc[off[m]:off[m] + ln[m]]
        if R.flip_of(int(T["r"])):
            q = np.where(q[::-1] < 4, 3 - q[::-1], 4).astype(np.uint8)
        want.append(q)
        want_off.append(want_off[-1] + len(q))
    want = np.concatenate(want)
    h_q, h_off = bm2.pe_rescue_queries(enc, off, ln, tasks)
    assert bm2.sam_rescue_plan_stats() == (0, len(tasks), len(want))
    d_q, d_off = ctx.pe_rescue_queries(enc, off, ln, tasks)
    assert bm2.sam_rescue_plan_stats() == (0, len(tasks), len(want))
    assert h_off.tolist() == want_off and d_off.tolist() == want_off
    assert h_q.tobytes() == want.tobytes(), "host form: first difference at byte %d" % int(np.nonzero(h_q != want)[0][0])
    assert d_q.tobytes() == want.tobytes(), "device form: first difference at byte %d" % int(np.nonzero(d_q != want)[0][0])
    sub = tasks[5::7]                                            # a list that is no multiple of the row count, mates in no regular order
    sub = sub[rng.permutation(len(sub))]
    s_h, s_hoff = bm2.pe_rescue_queries(enc, off, ln, sub)
    s_d, s_doff = ctx.pe_rescue_queries(enc, off, ln, sub)
    assert s_h.tobytes() == s_d.tobytes() and (s_hoff == s_doff).all() and len(s_h) > 0
    for form in (bm2.pe_rescue_queries, ctx.pe_rescue_queries):  # BM2_ECAP: offsets and the need are complete, nothing is written
        rc, buf, q_off, need = form(enc, off, ln, tasks, cap=len(want) - 1)
        assert rc == bm2.BM2_ECAP and need == len(want) and q_off.tolist() == want_off and (buf == 0xee).all()
        for field, value in (("pair", n_pairs), ("pair", -1), ("end", 2), ("r", 4)):
            t = tasks.copy()
            t[field][9] = value
            try:
                form(enc, off, ln, t)
            except bm2.Bm2Error as e:
                assert e.rc == bm2.BM2_EINVAL and "out of range" in str(e), e
            else:
                raise AssertionError("accepted: %s = %d" % (field, value))
        e_q, e_off = form(enc, off, ln, tasks[:0])
        assert len(e_q) == 0 and e_off.tolist() == [0]
    return len(want)


def check_tail(tail, extra, ctx, flag=0, subsets=SUBSETS, base_runs=True, **skw):
    """Item 5: the tail with the bit, alone and with every subset of the three other bits, == the flag-off text == `bwa-mem2 mem`;
    pes_out equal; the rescue counters those of the same run without the bit; the plan counters say the work happened on the device.
    base_runs=False (the emulator, where a run takes seconds): the subset is not run again without the bit -- `planned` is compared
    with the flag-off run's for every subset, (planned, used, missed) for the subsets that leave applying the results to the host."""
    ref = tail.reference(extra)
    off_text, pes_off = tail.ours(flag, ctx, **skw)
    assert ref == off_text, tail.M._diff(ref, off_text)
    st_off = bm2.sam_rescue_stats()
    planned = st_off[0]
    so = bm2.default_sam_opt(flag=flag, **skw)
    h_tasks, _ = bm2.pe_rescue_plan(tail.fa, tail.opt, so, tail.aln, tail.aln_off, tail.ln, pes_off)
    q_bytes = int(np.asarray(tail.ln, np.int64)[2 * h_tasks["pair"] + 1 - h_tasks["end"]].sum())
    assert len(h_tasks) == planned > 0 and q_bytes > 0
    for bits in subsets:
        st_base = st_off
        if bits and base_runs:
            base_text, _ = tail.ours(flag | bits, ctx, **skw)
            assert base_text == off_text
            st_base = bm2.sam_rescue_stats()
        on_text, pes_on = tail.ours(flag | bits | PLAN, ctx, **skw)
        assert ref == on_text, tail.M._diff(ref, on_text)
        assert [bytes(x) for x in pes_on] == [bytes(x) for x in pes_off]
        st_on = bm2.sam_rescue_stats()
        assert st_on[0] == st_base[0] == planned, (bits, st_base, st_on)
        if base_runs or not bits & RESCUE:
            assert st_on == st_base, (bits, st_base, st_on)
        assert bm2.sam_rescue_plan_stats() == (tail.n_pairs, planned, q_bytes), (bits, bm2.sam_rescue_plan_stats(), tail.n_pairs, planned, q_bytes)
    return ref, pes_off


def check_tail_two_contexts(tail, ctx, ctx2, part_knob, subsets=SUBSETS, base_runs=True):
    """the same through two contexts sharing a replica: the plan hook cuts the pairs, the rescue batch its tasks, into two parts"""
    for k in PART_KNOBS:
        os.environ[k] = str(part_knob)
    try:
        return check_tail(tail, [], [ctx, ctx2], subsets=subsets, base_runs=base_runs)
    finally:
        for k in PART_KNOBS:
            del os.environ[k]


def check_tail_refusals(tail, ctx):
    """the bit without a context, with MEM_F_NO_RESCUE, with rescue_inline"""
    def refused(f):
        try:
            f()
        except bm2.Bm2Error as e:
            assert e.rc == bm2.BM2_EINVAL and "DEVICE_PLAN" in str(e), e
            return
        raise AssertionError("accepted")
    refused(lambda: tail.ours(PLAN, None))
    refused(lambda: tail.ours(PLAN | 0x20, ctx))
    refused(lambda: tail.ours(PLAN, ctx, rescue_inline=1))
    return True
