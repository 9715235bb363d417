"""Shared by tests/test_tail_dp_edges.py (the host twins, the lane emulator, the emulator library, the compiled reference),
tests/test_zzzzzzzzzz_tail_dp_edges_gpu.py (the MI355X) and tests/test_ksw_sanitizer.py: the two dynamic-programming kernel families of the
device SAM tail at their edges -- the mate-rescue Smith-Waterman (matesw.hip / matesw_dev.h: k_ksw_align2, k_ksw_align2_reg) and the CIGAR
kernels (cigar.hip: k_cigar_flat, k_gen_cigar<RING | ROW | GLOBAL>).  The tasks are made by hand, one group per edge of a kernel, plus
random ones; a form under test is compared with the host twin field by field, the host twin with what the construction of a task says
about its answer and with properties that depend on neither twin (a CIGAR re-scored, NM and MD rebuilt, a plain Needleman-Wunsch).  Every
comparison is exact; every event a check names is counted from the inputs, the restated launch rules and the host twin's answer, and
asserted to occur."""
import ctypes as C
import re
import subprocess

import numpy as np

import bm2
import cigar_prep_cases as CP
from test_gen_cigar import make_tasks
from test_ksw_align2 import KSW_XBYTE, KSW_XSTART, KSW_XSTOP, KSW_XSUBO, _pairs

OPTION_SETS = [{}, dict(a=2, b=5, o_del=7, o_ins=8, e_del=2, e_ins=1), dict(b=1, o_del=1, o_ins=1)]
REF_ARGS = [[], ["-A", "2", "-B", "5", "-O", "7,8", "-E", "2,1"], ["-B", "1", "-O", "1,1", "-E", "1,1"]]      # the same sets for refdump
KSW_REG_SL = 10          # matesw_dev.h: segments the register pass holds
FIELDS = ("score", "te", "qe", "score2", "te2", "tb", "qb")
SCORE, TE, QE, SCORE2, TE2, TB, QB = range(7)


def _note(seen, k, c=1):
    if c:
        seen[k] = seen.get(k, 0) + int(c)


def _rand(rng, n):
    return rng.integers(0, 4, int(n), dtype=np.uint8)


def _cat(*parts):
    return np.concatenate([np.asarray(p, np.uint8) for p in parts]).astype(np.uint8)


# ================================================================================================ the rescue SW
# ---- the launch rules of matesw.hip, restated
def shift_of(opt):
    return (256 - (min(int(v) for v in opt.mat) & 0xff)) & 0xff


def slen_of(qlen, x):
    P = 16 if x & KSW_XBYTE else 8
    return (qlen + P - 1) // P


def fits_regs(qlen, x, reg=True):
    """ksw_task_fits_regs, and the knob BM2_KSW_REG"""
    return bool(reg) and bool(x & KSW_XBYTE) and (qlen + 15) // 16 <= KSW_REG_SL


def lds_rows(slen_max):
    """tasks per block of k_ksw_align2: as many as fit 64 KB; None = refused"""
    for rows in (16, 8, 4):
        if 32 + rows * 9 * slen_max * 16 * 2 <= 64 * 1024:
            return rows
    return None


def _noisy_pair(rng, ql, tl):
    """a random query with a noisy copy of its larger part somewhere in a random target"""
    q, t = _rand(rng, ql), _rand(rng, tl)
    l = min(max(ql * 2 // 3, 1), tl)
    if l > 0:
        a, p = int(rng.integers(0, ql - l + 1)), int(rng.integers(0, tl - l + 1))
        piece = q[a:a + l].copy()
        m = rng.random(l) < 0.04
        piece[m] = (piece[m] + 1) % 4
        t[p:p + l] = piece
    return q, t


class Batch:
    """one call of the form under test: tasks, their xtra words, and a tag per task naming what it was made for"""
    def __init__(self, name):
        self.name, self.pairs, self.xtra, self.tags = name, [], [], []

    def add(self, q, t, x, tag=None):
        self.pairs.append((np.ascontiguousarray(q, np.uint8), np.ascontiguousarray(t, np.uint8)))
        self.xtra.append(int(x))
        self.tags.append(tag)
        return self


def ksw_hand_made(opt, seed):
    """-> list of Batch"""
    rng = np.random.default_rng(seed)
    a, sh = int(opt.a), shift_of(opt)
    base = 19 * a
    B = []

    def batch(name):
        B.append(Batch(name))
        return B[-1]
    # byte saturation: the byte pass clamps at 255 - shift; an exact copy of n_sat bases reaches it, one base less stays below
    n_sat = -(-(255 - sh) // a)
    b = batch("saturation")
    for n, tag in ((n_sat, "sat_at"), (n_sat - 1, "sat_below")):
        X = _rand(rng, n)
        t = _cat(_rand(rng, 13), X, _rand(rng, 17))
        for start in (0, KSW_XSTART):
            for minsc in (base, 300):
                b.add(X, t, KSW_XBYTE | KSW_XSUBO | start | minsc, (tag, 13, n))
            b.add(X, t, KSW_XBYTE | start | base, (tag, 13, n))
            b.add(X, t, KSW_XSUBO | start | base, ("word_twin", 13, n))          # (the word lanes do not saturate)
    X = _rand(rng, n_sat)
    for start in (0, KSW_XSTART):                                  # a query that goes on beyond the saturating copy
        b.add(_cat(X, _rand(rng, 9)), _cat(_rand(rng, 30), X, _rand(rng, 9)), KSW_XBYTE | KSW_XSUBO | start | base, ("sat_at", 30, n_sat))
    # KSW_XSTOP: the same pair without and with the bit, the stop score half the copy's
    b = batch("stop")
    for lanes in (KSW_XBYTE, 0):
        for ql in (100, 170):
            X = _rand(rng, ql)
            t = _cat(_rand(rng, 20), X, _rand(rng, 30))
            s = (ql // 2) * a
            for more in (KSW_XSUBO | KSW_XSTART, KSW_XSTART, 0):
                b.add(X, t, lanes | more | s, "stop_off")
                b.add(X, t, lanes | more | KSW_XSTOP | s, "stop_on")
    # the register / LDS split at KSW_REG_SL: 160 | 161 bases on byte lanes; batches of one kind and mixed, sizes around the kernels' blocks
    full = KSW_XBYTE | KSW_XSUBO | KSW_XSTART | base
    for n in (1, 15, 16, 17):
        b = batch("reg_only_%d" % n)
        for i in range(n):
            ql = (160, 1, 16, 17, 150, 100, 159, 33)[i % 8]
            b.add(*_noisy_pair(rng, ql, int(rng.integers(30, 200))), full, "reg_160" if ql == 160 else None)
    lds_kinds = {16: ((161, KSW_XBYTE), (224, KSW_XBYTE), (112, 0), (20, 0), (8, 0), (200, KSW_XBYTE), (100, 0)),
                 8: ((300, KSW_XBYTE), (161, KSW_XBYTE), (224, 0), (50, 0), (225, KSW_XBYTE)),
                 4: ((300, 0), (161, KSW_XBYTE), (448, 0), (30, 0))}
    for rows, kinds in lds_kinds.items():
        for n in (rows - 1, rows, rows + 1):
            b = batch("lds_only_%d_%d" % (rows, n))
            for i in range(n):
                ql, lanes = kinds[i % len(kinds)]
                b.add(*_noisy_pair(rng, ql, int(rng.integers(30, 200))), lanes | KSW_XSUBO | KSW_XSTART | base, "lds_161" if (ql, lanes) == (161, KSW_XBYTE) else None)
    b = batch("mixed")
    for i in range(40):
        ql, lanes = ((160, KSW_XBYTE), (161, KSW_XBYTE), (90, 0), (150, KSW_XBYTE), (12, 0), (200, KSW_XBYTE), (1, KSW_XBYTE))[i % 7]
        b.add(*_noisy_pair(rng, ql, int(rng.integers(30, 200))), lanes | KSW_XSUBO | KSW_XSTART | base,
              {(160, KSW_XBYTE): "reg_160", (161, KSW_XBYTE): "lds_161"}.get((ql, lanes)))
    # the LDS row tiers: slen_max of the batch 14 | 15 (16 -> 8 rows per block), 28 | 29 (8 -> 4), 56 (the last); the short tasks stride by it
    for ql, lanes in ((224, KSW_XBYTE), (225, KSW_XBYTE), (112, 0), (113, 0), (224, 0), (225, 0), (448, 0)):
        b = batch("tier_%s_%d" % ("byte" if lanes else "word", ql))
        b.add(*_noisy_pair(rng, ql, 300), lanes | KSW_XSUBO | KSW_XSTART | base, "tier_longest")
        for i in range(50):
            b.add(*_noisy_pair(rng, int(rng.integers(10, 61)), int(rng.integers(30, 100))), (KSW_XBYTE if i % 3 == 2 else 0) | KSW_XSUBO | KSW_XSTART | base)
    # the list of local maxima at its capacity (tlen + 1) / 2 + 1: every other row reaches the minimum score, none adjacent
    b = batch("blist")
    for tl in (300, 301):
        t = (np.arange(tl) & 1).astype(np.uint8)                  # ACAC...
        for lanes in (KSW_XBYTE, 0):
            for start in (0, KSW_XSTART):
                b.add(np.zeros(20, np.uint8), t, lanes | KSW_XSUBO | start | a, "blist_full")
    # the exclusion window te +- ceil(score / maxsc) of the second-best score: two copies of a 30-mer whose ends lie d and d + 1 apart, the
    # better one first and second (the other has one mismatch); the target ends with the second copy
    b = batch("window")
    for lanes in (KSW_XBYTE, 0):
        for best_first in (True, False):
            for gap in (0, 1):
                X = _rand(rng, 30)
                Y = X.copy()
                Y[5] = (Y[5] + 1) % 4
                one, two = (X, Y) if best_first else (Y, X)
                t = _cat(_rand(rng, 5), one, _rand(rng, gap), two)
                b.add(X, t, lanes | KSW_XSUBO | KSW_XSTART | base, "win_outside" if gap else "win_inside")
    # the tie rule of qe: the smallest query position among equals
    b = batch("tie")
    for lanes in (KSW_XBYTE, 0):
        for n in (20, 33):
            X = _rand(rng, n)
            for start in (0, KSW_XSTART):
                b.add(_cat(X, X), X, lanes | KSW_XSUBO | start | (n * a // 2), ("qe_tie", n))
    # an insertion longer than a stripe segment: the lazy-F loop carries it across a lane border
    b = batch("insertion")
    for lanes, k in ((KSW_XBYTE, 8), (0, 13)):
        for rep in range(3):
            Lf, Rf = _rand(rng, 40), _rand(rng, 40)
            q = _cat(Lf, _rand(rng, k), Rf)
            assert k > slen_of(len(q), lanes)
            b.add(q, _cat(_rand(rng, 10), Lf, Rf, _rand(rng, 10)), lanes | KSW_XSUBO | KSW_XSTART | base, ("ins_across_lanes", 40))
    # N in the target (and in the query); target lengths 0, 1 and beyond the sort key's clamp (tlen >> 3 > 511)
    b = batch("odd_targets")
    for lanes in (KSW_XBYTE, 0):
        for rep in range(4):
            q, t = _noisy_pair(rng, 70, 150)
            t[rng.integers(0, 150, 6)] = 4
            if rep & 1:
                q[rng.integers(0, 70, 2)] = 4
            b.add(q, t, lanes | KSW_XSUBO | KSW_XSTART | base, "target_N")
        for tl in (0, 1, 4096, 5000):
            q = _rand(rng, 50)
            t = _rand(rng, tl)
            if tl > 100:
                t[tl - 60:tl - 10] = q
            b.add(q, t, lanes | KSW_XSUBO | KSW_XSTART | base, "tlen_%d" % tl)
            b.add(q, t, lanes | KSW_XSTART | base, "tlen_%d" % tl)
    return B


def ksw_random(opt, seed, n):
    """_pairs of tests/test_ksw_align2.py under every flag: KSW_XBYTE whatever the length (long copies saturate), KSW_XSTOP now and then"""
    rng = np.random.default_rng(seed)
    b = Batch("random")
    for q, t in _pairs(seed, n):
        x = 19 * int(opt.a)
        for bit, p in ((KSW_XSUBO, 0.9), (KSW_XSTART, 0.9), (KSW_XBYTE, 0.5), (KSW_XSTOP, 0.1)):
            if rng.random() < p:
                x |= bit
        b.add(q, t, x)
    return b


def ksw_expectations(opt, b, exp):
    """what the construction of a tagged task says about the host twin's answer"""
    a = int(opt.a)
    for i, tag in enumerate(b.tags):
        r, x = exp[i], b.xtra[i]
        q, t = b.pairs[i]
        what = (b.name, i, tag, r.tolist())
        assert -1 <= r[TE] < max(len(t), 1) and -1 <= r[QE] < len(q), what
        assert 0 <= r[SCORE] <= a * min(len(q), len(t)) or (r[SCORE] == 255 and x & KSW_XBYTE), what
        assert (r[TB] < 0) == (r[QB] < 0) and (len(t) == 0 or (r[TB] <= r[TE] and r[QB] <= r[QE])), what
        if tag is None:
            continue
        started = bool(x & KSW_XSTART) and not (x & KSW_XSUBO and r[SCORE] < (x & 0xffff))
        kind = tag[0] if isinstance(tag, tuple) else tag
        if kind == "sat_at":
            assert tuple(r[[SCORE, QE, SCORE2, TE2, TB, QB]]) == (255, -1, -1, -1, -1, -1), what
        elif kind in ("sat_below", "word_twin"):
            p, n = tag[1], tag[2]
            assert tuple(r[[SCORE, TE, QE]]) == (n * a, p + n - 1, n - 1), what
            assert tuple(r[[TB, QB]]) == ((p, 0) if started else (-1, -1)), what
        elif kind == "stop_on":
            off = exp[i - 1]
            assert b.tags[i - 1] == "stop_off" and r[TE] < off[TE] and r[SCORE] >= (x & 0xffff), (what, off.tolist())
        elif kind == "blist_full":
            assert tuple(r[[SCORE, TE, SCORE2, TE2]]) == (a, 0, a, 2), what
        elif kind == "win_inside":
            assert r[SCORE] == 30 * a and r[SCORE2] == -1, what
        elif kind == "win_outside":
            assert r[SCORE] == 30 * a and r[SCORE2] > 0 and abs(int(r[TE2]) - int(r[TE])) == 31, what
        elif kind == "qe_tie":
            n = tag[1]
            assert tuple(r[[SCORE, TE, QE]]) == (n * a, n - 1, n - 1), what
        elif kind == "ins_across_lanes":
            assert r[SCORE] > tag[1] * a and started and r[QB] >= 0 and r[QE] - r[QB] + 1 > (r[TE] - r[TB] + 1) + slen_of(len(q), x), what


def ksw_events(opt, b, exp, seen, reg=True):
    qlen = [len(q) for q, t in b.pairs]
    n_reg = sum(fits_regs(l, x, reg) for l, x in zip(qlen, b.xtra))
    n_lds = len(qlen) - n_reg
    slen_max = max(slen_of(l, x) for l, x in zip(qlen, b.xtra))
    rows = lds_rows(slen_max)
    assert rows is not None, b.name
    hand = b.name != "random"
    if hand:
        _note(seen, "batch_reg_only", n_lds == 0); _note(seen, "batch_lds_only", n_reg == 0); _note(seen, "batch_mixed", n_reg > 0 and n_lds > 0)
        if n_lds == 0 and b.name.startswith("reg_only"):
            _note(seen, "reg_n_%d" % n_reg)
        if n_reg == 0 and b.name.startswith("lds_only"):
            _note(seen, "lds_rows_%d_n_%d" % (rows, n_lds), abs(n_lds - rows) <= 1)
        if b.name.startswith("tier_") and len(qlen) == 51:
            _note(seen, "tier_%d" % slen_max)
            _note(seen, "tier_short_strides_by_the_longest", sum(1 for l, x in zip(qlen, b.xtra) if not fits_regs(l, x, reg) and slen_of(l, x) < slen_max))
    for i, tag in enumerate(b.tags):
        r, x, l = exp[i], b.xtra[i], qlen[i]
        q, t = b.pairs[i]
        byte = bool(x & KSW_XBYTE)
        sat = byte and r[SCORE] == 255
        _note(seen, "sat_any", sat)
        _note(seen, "sat_on_registers", sat and fits_regs(l, x, reg)); _note(seen, "sat_on_lds", sat and not fits_regs(l, x, reg))
        _note(seen, "start_pass_skipped_after_saturation", bool(sat and x & KSW_XSTART and not (x & KSW_XSUBO and 255 < (x & 0xffff))))
        _note(seen, "xstop_set", bool(x & KSW_XSTOP))
        _note(seen, "second_best_found", r[SCORE2] > 0)
        _note(seen, "reg_160", byte and l == 160 and fits_regs(l, x, reg)); _note(seen, "lds_160", byte and l == 160 and not fits_regs(l, x, reg))
        _note(seen, "lds_161", byte and l == 161 and not fits_regs(l, x, reg))
        if tag is None:
            continue
        kind = tag[0] if isinstance(tag, tuple) else tag
        if kind in ("sat_at", "sat_below"):
            _note(seen, kind)
            _note(seen, kind + ("_with_xstart" if x & KSW_XSTART else "_without_xstart"))
            if x & KSW_XSUBO:
                _note(seen, kind + ("_minsc_above_255" if (x & 0xffff) > 255 else "_minsc_below_255"))
        elif kind == "stop_on":
            _note(seen, "stop_cut", r[TE] < exp[i - 1][TE])
            _note(seen, "stop_cut_" + ("byte" if byte else "word"), r[TE] < exp[i - 1][TE])
        elif kind == "blist_full":
            rows_at_minsc = int((t == 0).sum())                    # the A rows, none adjacent
            capacity = (len(t) + 1) // 2 + 1                     # (matesw.hip; the scan stops at the entry count, so one slot is spare)
            _note(seen, "blist_full", rows_at_minsc == capacity - 1 and not (np.diff(np.flatnonzero(t == 0)) == 1).any())
        elif kind in ("win_inside", "win_outside", "qe_tie", "ins_across_lanes", "target_N"):
            _note(seen, kind)
            _note(seen, kind + ("_byte" if byte else "_word"))
        elif kind.startswith("tlen_"):
            assert len(t) == int(kind[5:])
            _note(seen, kind)
    return seen


KSW_WANTED = (["sat_at", "sat_below", "sat_at_with_xstart", "sat_at_without_xstart", "sat_below_with_xstart", "sat_below_without_xstart",
               "sat_at_minsc_above_255", "sat_at_minsc_below_255", "sat_below_minsc_above_255", "sat_below_minsc_below_255", "sat_on_lds",
               "start_pass_skipped_after_saturation", "stop_cut", "stop_cut_byte", "stop_cut_word", "xstop_set", "second_best_found", "lds_161",
               "batch_lds_only", "tier_14", "tier_15", "tier_28", "tier_29", "tier_56", "tier_short_strides_by_the_longest", "blist_full",
               "win_inside", "win_outside", "win_inside_byte", "win_inside_word", "win_outside_byte", "win_outside_word", "qe_tie", "qe_tie_byte", "qe_tie_word",
               "ins_across_lanes", "ins_across_lanes_byte", "ins_across_lanes_word", "target_N", "tlen_0", "tlen_1", "tlen_4096", "tlen_5000"]
              + ["lds_rows_%d_n_%d" % (r, n) for r in (16, 8, 4) for n in (r - 1, r, r + 1)])
KSW_WANTED_REG = ["reg_160", "sat_on_registers", "batch_reg_only", "batch_mixed", "reg_n_1", "reg_n_15", "reg_n_16", "reg_n_17"]      # with the register kernel on
KSW_WANTED_NO_REG = ["lds_160"]                                   # BM2_KSW_REG=0: every task on the LDS kernel


def _first_diff(b, exp, got, who):
    bad = np.nonzero((exp != got).any(axis=1))[0]
    assert len(bad) == 0, "%s, batch %s: %d of %d differ; first: task %d (qlen %d, tlen %d, xtra %#x, made for %s) host %s, %s %s" % (
        who, b.name, len(bad), len(exp), bad[0], len(b.pairs[bad[0]][0]), len(b.pairs[bad[0]][1]), b.xtra[bad[0]], b.tags[bad[0]],
        dict(zip(FIELDS, exp[bad[0]].tolist())), who, dict(zip(FIELDS, got[bad[0]].tolist())))


def check_ksw(run, opt_sets=None, n_random=1500, reg=True, who="device"):
    """run(pairs, xtra, opt) = the form under test (None: the host twin alone, against the tasks' construction).  reg: what BM2_KSW_REG is in
    the process of `run`.  -> the event counts"""
    total = {}
    for k, kw in enumerate(OPTION_SETS if opt_sets is None else opt_sets):
        opt = bm2.default_opt(**kw)
        batches = ksw_hand_made(opt, 900 + k)
        if n_random:
            batches.append(ksw_random(opt, 950 + k, n_random))
        for b in batches:
            exp = bm2.ksw_align2(b.pairs, b.xtra, opt)
            ksw_expectations(opt, b, exp)
            if run is not None:
                _first_diff(b, exp, np.asarray(run(b.pairs, b.xtra, opt)), who)
            ksw_events(opt, b, exp, total, reg)
    wanted = KSW_WANTED + (KSW_WANTED_REG if reg else KSW_WANTED_NO_REG)
    if not any(160 * int(o.a) >= 255 - shift_of(o) for o in (bm2.default_opt(**kw) for kw in (OPTION_SETS if opt_sets is None else opt_sets))):
        wanted = [ev for ev in wanted if ev != "sat_on_registers"]      # (no query of 160 bases can saturate under these sets)
    missing = [ev for ev in wanted if not total.get(ev)]
    assert not missing, (missing, sorted(total.items()))
    if not reg:
        assert not total.get("reg_160") and not total.get("sat_on_registers") and not total.get("batch_reg_only"), total
    return total


def ksw_small_tasks(opt, seed, max_q=161, max_t=200):
    """the hand-made tasks the lane emulator runs in reasonable time, one Batch (it runs them one by one)"""
    out = Batch("small")
    for b in ksw_hand_made(opt, seed):
        for (q, t), x, tag in zip(b.pairs, b.xtra, b.tags):
            if len(q) <= max_q and len(t) <= max_t and not (b.name.startswith("tier_") and tag is None):      # (a tier's short fillers matter in their batch only)
                out.add(q, t, x, tag)
    return out


def write_pairs(path, pairs, xtra):
    """the text form `refdump ksw` and tools/emu/matesw_emu read"""
    with open(path, "w") as f:
        for (q, t), x in zip(pairs, xtra):
            f.write("%d %s %s\n" % (x, "".join("ACGTN"[c] for c in q), "".join("ACGTN"[c] for c in t)))


def check_ksw_against_reference(dump, tmp, set_no, form=None, n_random=1500):
    """the reference's own ksw_align2 (oracle/_ref/refdump ksw) where its behaviour is defined: not the saturated tasks with KSW_XSTART (it
    builds a profile of an empty query there), not the empty targets.  form(pairs, xtra, opt): the form compared (default: the host twin)"""
    opt = bm2.default_opt(**OPTION_SETS[set_no])
    pairs, xtra, tags = [], [], []
    for b in ksw_hand_made(opt, 900 + set_no) + [ksw_random(opt, 950 + set_no, n_random)]:
        pairs += b.pairs; xtra += b.xtra; tags += b.tags
    ours = bm2.ksw_align2(pairs, xtra, opt) if form is None else np.asarray(form(pairs, xtra, opt))
    host = ours if form is None else bm2.ksw_align2(pairs, xtra, opt)
    keep = [i for i in range(len(pairs)) if len(pairs[i][1]) > 0 and not (host[i][SCORE] == 255 and xtra[i] & KSW_XBYTE and xtra[i] & KSW_XSTART)]
    left_out = len(pairs) - len(keep)
    assert 0 < left_out < len(pairs) // 4
    pf, of = str(tmp / "pairs.txt"), str(tmp / "out.bin")
    write_pairs(pf, [pairs[i] for i in keep], [xtra[i] for i in keep])
    subprocess.check_call([dump] + REF_ARGS[set_no] + ["ksw", pf, of], stderr=subprocess.DEVNULL)
    ref = np.fromfile(of, "<i4").reshape(-1, 7)
    assert len(ref) == len(keep)
    got = ours[keep]
    bad = np.nonzero((ref != got).any(axis=1))[0]
    assert len(bad) == 0, "%d of %d differ; first: task %d (qlen %d, tlen %d, xtra %#x, made for %s) reference %s ours %s" % (
        len(bad), len(keep), keep[bad[0]], len(pairs[keep[bad[0]]][0]), len(pairs[keep[bad[0]]][1]), xtra[keep[bad[0]]], tags[keep[bad[0]]], ref[bad[0]].tolist(), got[bad[0]].tolist())
    assert sum(1 for i in keep if host[i][SCORE] == 255 and xtra[i] & KSW_XBYTE) > 0          # saturation itself IS compared (without the start pass)
    return len(keep), left_out


# ---- arguments: what both twins refuse, with no launch behind it
def _ksw_raw(who, ctx, pairs, xtra, opt, out, e_del=None, e_ins=None, q_len=None, t_len=None):
    L = bm2.lib()
    buf, q_off, ql, t_off, tl = [], [], [], [], []
    p = 0
    for q, t in pairs:
        q_off.append(p); ql.append(len(q)); buf.append(q); p += len(q)
        t_off.append(p); tl.append(len(t)); buf.append(t); p += len(t)
    seqs = np.concatenate(buf + [np.zeros(8, np.uint8)]).astype(np.uint8)
    q_off, t_off = np.array(q_off, np.int64), np.array(t_off, np.int64)
    ql = np.array(ql if q_len is None else q_len, np.int32); tl = np.array(tl if t_len is None else t_len, np.int32)
    xt = np.array(xtra, np.int32)
    mat = (C.c_int8 * 25)(*opt.mat)
    gaps = (opt.o_del, opt.e_del if e_del is None else e_del, opt.o_ins, opt.e_ins if e_ins is None else e_ins)
    if who == "bm2_ksw_align2_dev":
        L.bm2_ksw_align2_dev.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        return L.bm2_ksw_align2_dev(ctx.h, len(pairs), seqs.ctypes.data, len(seqs), q_off.ctypes.data, ql.ctypes.data, t_off.ctypes.data, tl.ctypes.data,
                                    xt.ctypes.data, C.cast(mat, C.c_void_p), *gaps, out.ctypes.data)
    L.bm2_ksw_align2.argtypes = [C.c_int32] + [C.c_void_p] * 6 + [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L.bm2_ksw_align2(len(pairs), seqs.ctypes.data, q_off.ctypes.data, ql.ctypes.data, t_off.ctypes.data, tl.ctypes.data, xt.ctypes.data,
                            C.cast(mat, C.c_void_p), *gaps, out.ctypes.data)


def check_ksw_arguments(ctx=None):
    """bm2_ksw_align2, and with a context bm2_ksw_align2_dev: an empty query, a negative length (the lowest offender named) and a gap extension
    <= 0 are refused in the same words, and a refused call writes nothing.  The device form alone refuses what does not fit its LDS layout.
    Nothing here reaches a kernel: every call is refused, or is the host's."""
    L = bm2.lib()
    opt = bm2.default_opt()
    rng = np.random.default_rng(8)
    pairs = [_noisy_pair(rng, 40, 90) for _ in range(9)]
    xtra = [KSW_XBYTE | KSW_XSUBO | KSW_XSTART | 19] * 9
    want = bm2.ksw_align2(pairs, xtra, opt)
    forms = ["bm2_ksw_align2"] + (["bm2_ksw_align2_dev"] if ctx is not None else [])
    done = 0
    for who in forms:
        def refused(rc, word, p=pairs, x=xtra, **kw):
            out = np.full((len(p), 7), 7, np.int32)
            got = _ksw_raw(who, ctx, p, x, opt, out, **kw)
            msg = L.bm2_last_error()
            assert got == rc, (who, word, got, msg)
            assert word.encode() in msg and msg.startswith(who.encode() + b":"), (who, word, msg)
            assert (out == 7).all(), (who, word, "a refused call wrote")
            return 1
        lens = [len(q) for q, t in pairs]
        for at in (0, 4, 8):                                     # an offender first, in the middle and last, a second one after it
            for v in (0, -1):
                bad = list(lens)
                for j in {at, min(at + 2, 8), 8}:
                    bad[j] = v
                done += refused(bm2.BM2_EINVAL, "pair %d has an empty query" % at, q_len=bad)
            bad = [len(t) for q, t in pairs]
            bad[at] = -1
            done += refused(bm2.BM2_EINVAL, "pair %d has an empty query" % at, t_len=bad)
        for kw in (dict(e_del=0), dict(e_ins=0), dict(e_del=-1), dict(e_ins=-2)):
            done += refused(bm2.BM2_EINVAL, "bad argument", **kw)
        out = np.full((len(pairs), 7), 7, np.int32)
        assert _ksw_raw(who, ctx, pairs, xtra, opt, out) == bm2.BM2_OK and (out == want).all(), (who, L.bm2_last_error())
    # 449 bases on word lanes are 57 stripe segments: the host takes them, the device names the limit and writes nothing
    big = pairs + [_noisy_pair(rng, 449, 500)]
    bx = xtra + [KSW_XSUBO | KSW_XSTART | 19]
    host = bm2.ksw_align2(big, bx, opt)
    assert host[9][SCORE] > 19
    if ctx is not None:
        out = np.full((len(big), 7), 7, np.int32)
        rc = _ksw_raw("bm2_ksw_align2_dev", ctx, big, bx, opt, out)
        msg = L.bm2_last_error()
        assert rc == bm2.BM2_EUNSUP and b"448" in msg and b"57" in msg and (out == 7).all(), (rc, msg)
        done += 1
    return {"refused_calls": done, "tier_refused": int(ctx is not None)}


# ================================================================================================ the CIGAR kernels
CONTIGS = (25000, 15000)
TWO_LETTER = (10000, 16000)      # this stretch of the first contig holds A and C only: a query of G and T mismatches it in EVERY cell


def genome():
    rng = np.random.default_rng(4040)
    ctg = [_rand(rng, n) for n in CONTIGS]
    lo, hi = TWO_LETTER
    ctg[0][lo:hi] = rng.integers(0, 2, hi - lo, dtype=np.uint8)
    return ctg


def write_index(d):
    """the 40 kbp two-contig genome written and indexed by bm2.index_build -> the index prefix"""
    fa = str(d / "tail_dp.fa")
    with open(fa, "w") as f:
        for k, c in enumerate(genome()):
            f.write(">ctg%d\n" % k)
            s = "".join("ACGT"[v] for v in c)
            for i in range(0, len(s), 60):
                f.write(s[i:i + 60] + "\n")
    bm2.index_build(fa, None, 2)
    return fa


class Strands:
    """the reference as the kernels see it: forward strand, then its reverse complement; a range of the second half is aligned reversed"""
    def __init__(self, ctg):
        G = np.concatenate(ctg)
        self.l_pac = len(G)
        self.S = np.concatenate([G, (3 - G[::-1]).astype(np.uint8)])

    def aln(self, rb, re_):
        """the range in alignment order"""
        r = self.S[rb:re_]
        return r[::-1] if rb >= self.l_pac else r


def cigar_hand_made(opt, ctg, seed):
    """-> (tasks [(query, rb, re, w)], tags).  Queries are made in alignment order and stored as the caller holds them (reversed for a range
    of the reverse strand)"""
    rng = np.random.default_rng(seed)
    st = Strands(ctg)
    l_pac = st.l_pac
    tasks, tags = [], []

    def add(q_aln, rb, rlen, w, tag):
        q = np.ascontiguousarray(q_aln[::-1] if rb >= l_pac else q_aln, np.uint8)
        tasks.append((q, int(rb), int(rb + rlen), int(w)))
        tags.append(tag)

    def mutate(r, n):
        q = r.copy()
        at = rng.choice(len(q), size=min(n, len(q)), replace=False)
        q[at] = (q[at] + 1 + rng.integers(0, 3, len(at))) % 4
        return q
    # the ring at its widest band, 31, and the neighbour that goes to ROW: 150 x 150, plain and with one indel of each kind that runs the
    # path along the band's edge (k bases off the diagonal), the insertion first and the deletion first
    for w in (31, 32):
        for rb in (3000, l_pac + 3000, 20100, l_pac + 31000):
            R = st.aln(rb, rb + 150)
            add(mutate(R, 3), rb, 150, w, "band_%d" % w)
            for k in (w, w - 2):
                mid = 120 - k
                add(_cat(R[:10], _rand(rng, k), R[10:10 + mid], R[10 + mid + k:]), rb, 150, w, "band_%d_indel" % w)
                add(_cat(R[:10], R[10 + k:10 + k + mid], _rand(rng, k), R[130:]), rb, 150, w, "band_%d_indel" % w)
    # the packed 16-bit words: query lengths 220 | 221 and (q_len + rlen) * pen around CG_SMALL, with every cell a mismatch and a length
    # difference that sets the band (dl + 3)
    lo, hi = TWO_LETTER
    pen = CP.Rule(opt).pen
    tots = sorted({(CP.CG_SMALL - 1) // pen, CP.CG_SMALL // pen, CP.CG_SMALL // pen + 1, -(-CP.CG_SMALL // pen)})
    for fwd in (True, False):
        def lowest(q_len, rlen, w, tag):
            rb = lo + 100 if fwd else 2 * l_pac - hi + 100
            assert rlen <= hi - lo - 100
            add((rng.integers(2, 4, q_len) if fwd else rng.integers(0, 2, q_len)).astype(np.uint8), rb, rlen, w, tag)
        for q_len in (220, 221):
            for dl, w in ((0, 3), (5, 0), (-5, 0), (40, 10)):
                lowest(q_len, q_len + dl, w, "all_mismatch")
        for tot in tots:
            lowest(200, tot - 200, 5, "all_mismatch")
    # the first and last base of either strand, query lengths around the eight-base loads, flat and DP
    for q_len in (7, 8, 9, 15, 16, 17):
        for rlen, w in ((q_len, 0), (q_len + 1, 5)):
            for rb in (0, l_pac - rlen, l_pac, 2 * l_pac - rlen):
                R = st.aln(rb, rb + rlen)
                q = R.copy() if rlen == q_len else np.delete(R, q_len // 2)
                if q_len & 1:
                    q[0] = (q[0] + 1) % 4
                else:
                    q[-1] = (q[-1] + 2) % 4
                add(q, rb, rlen, w, "strand_edge")
    # ranges shorter than one load, a query of one base, bands wider than the query
    for rb in (700, l_pac + 700):
        for rlen in range(1, 8):
            R = st.aln(rb, rb + rlen)
            add(_cat(R, _rand(rng, 3)), rb, rlen, 5, "short_range")
            add(R[:max(rlen - 2, 1)], rb, rlen, 2, "short_range")
        add(st.aln(rb, rb + 1), rb, 1, 0, "q_len_1")
        add(st.aln(rb + 1, rb + 2), rb, 3, 5, "q_len_1")
        add(_rand(rng, 1), rb, 9, 100, "q_len_1")
        for q_len, rlen in ((5, 12), (12, 5), (10, 30)):
            R = st.aln(rb, rb + rlen)
            add(R[:q_len] if q_len <= rlen else _cat(R, _rand(rng, q_len - rlen)), rb, rlen, 100, "wide_band")
    # row lengths (end - beg) & 3: bands whose rows are 2 w + 1 = 7, 9, 11, 13 cells, and queries of every length mod 4
    for w in (3, 4, 5, 6):
        for q_len in (40, 41, 42, 43):
            rb = int(rng.integers(100, 9000)) + (l_pac if q_len & 1 else 0)
            R = st.aln(rb, rb + q_len)
            add(np.delete(mutate(R, 2), [7, 8]), rb, q_len, w, "row_lengths")
    # put_dec with four and five digits: exact copies of 1000 and 10000 bases (flat), and the same with one base of the range deleted (DP)
    for n in (1000, 10000):
        for rb in (200, l_pac + 14000):
            R = st.aln(rb, rb + n)
            add(R.copy(), rb, n, 0, "md_digits")
            R = st.aln(rb, rb + n + 5)
            add(np.delete(R, n), rb, n + 5, 5, "md_digits")
    # the NULL returns: a range that bridges the strands, one that runs past the end of the second
    add(_rand(rng, 100), l_pac - 50, 100, 5, "null")
    add(_rand(rng, 70), 2 * l_pac - 30, 70, 5, "null")
    # bands that cover the whole matrix, at most 300 x 300: the score is a plain Needleman-Wunsch's
    for i in range(40):
        n = int(rng.integers(20, 295))
        rb = int(rng.integers(0, l_pac - 400)) + (l_pac if i & 1 else 0)
        if rb < l_pac < rb + n + 5:
            rb -= 400
        R = st.aln(rb, rb + n)
        q = mutate(R, n // 15)
        for _ in range(int(rng.integers(0, 3))):
            c = int(rng.integers(3, max(len(q) - 3, 4)))
            q = np.delete(q, slice(c, c + int(rng.integers(1, 5)))) if rng.random() < 0.5 else np.insert(q, c, _rand(rng, int(rng.integers(1, 5))))
        if len(q) > 300:
            q = q[:300]
        if i % 7 == 0:
            q[len(q) // 2] = 4
        add(q.astype(np.uint8), rb, n, 1000, "whole_matrix")
    return tasks, tags


def needleman_wunsch(opt, qa, ra):
    """the global alignment score of ksw_global2's recurrence (gaps open from a match state only) with no band: int64, one numpy row at a
    time, the insertion state F by a running maximum along the row"""
    a, b_, amb = int(opt.mat[0]), int(opt.mat[1]), int(opt.mat[4])
    od, ed, oi, ei = int(opt.o_del), int(opt.e_del), int(opt.o_ins), int(opt.e_ins)
    qa = np.asarray(qa, np.int64); ra = np.asarray(ra, np.int64)
    lq = len(qa)
    NEG = np.int64(-(1 << 40))
    j = np.arange(lq, dtype=np.int64)
    H = np.concatenate([[0], -(oi + ei * (j + 1))]).astype(np.int64)       # row -1: H[0] is the corner, H[j + 1] = column j
    E = np.full(lq, NEG, np.int64)
    for i in range(len(ra)):
        t = ra[i]
        s = np.where((qa == t) & (t < 4), a, np.where((qa > 3) | (t > 3), amb, b_)).astype(np.int64)
        M = H[:-1] + s                                           # the diagonal
        G = np.maximum.accumulate(M + ei * j)                    # F[j] = max over k < j of M[k] - oi - ei (j - k)
        F = np.concatenate([[NEG], G[:-1] - oi - ei * j[1:]]) if lq > 1 else np.array([NEG])
        Hrow = np.maximum(np.maximum(M, E), F)
        E = np.maximum(E - ed, M - (od + ed))
        H = np.concatenate([[-(od + ed * (i + 1))], Hrow])
    return int(H[-1])


def cigar_independent(opt, st, task, ans, what):
    """an answer against its own inputs: the ops consume query and range, re-scored they give the score, NM and MD rebuilt from them are the
    reported ones -> what the walk saw"""
    q, rb, re_, w = task
    score, nm, ops, md = ans
    rev = rb >= st.l_pac
    qa = (q[::-1] if rev else q).astype(np.int64)
    ra = st.aln(rb, re_).astype(np.int64)
    a, b_, amb = int(opt.mat[0]), int(opt.mat[1]), int(opt.mat[4])
    letters = "TGCAN" if rev else "ACGTN"
    x = y = u = n_mm = n_gap = sc = 0
    out = []
    for k, c in enumerate(ops):
        op, ln = c & 15, c >> 4
        assert op in (0, 1, 2) and ln > 0 and (k == 0 or op != (ops[k - 1] & 15)), (what, ops)
        if op == 0:
            qs, rs = qa[x:x + ln], ra[y:y + ln]
            assert len(qs) == ln and len(rs) == ln, (what, "an M runs past an end")
            sc += int(np.where((qs == rs) & (rs < 4), a, np.where((qs > 3) | (rs > 3), amb, b_)).sum())
            prev = 0
            for p in np.flatnonzero(qs != rs):
                out.append("%d%s" % (u + p - prev, letters[rs[p]]))
                u, prev = 0, p + 1
                n_mm += 1
            u += ln - prev
            x += ln; y += ln
        elif op == 2:
            sc -= int(opt.o_del) + int(opt.e_del) * ln
            if 0 < k < len(ops) - 1:
                out.append("%d^%s" % (u, "".join(letters[v] for v in ra[y:y + ln])))
                u = 0
                n_gap += ln
            y += ln
        else:
            sc -= int(opt.o_ins) + int(opt.e_ins) * ln
            x += ln
            n_gap += ln
    out.append("%d" % u)
    assert (x, y) == (len(qa), len(ra)), (what, "the ops consume", x, y, "of", len(qa), len(ra))
    assert sc == score, (what, "re-scored", sc, "reported", score)
    assert n_mm + n_gap == nm, (what, "NM rebuilt", n_mm + n_gap, "reported", nm)
    assert "".join(out).encode() == md, (what, "MD rebuilt", "".join(out)[:80], "reported", md[:80])
    return qa, ra


def cigar_row_lengths(lq, rlen, wb):
    i = np.arange(rlen, dtype=np.int64)
    return (np.minimum(i + wb + 1, lq) - np.maximum(i - wb, 0)) & 3


def cigar_events(opt, st, rule, tasks, tags, exp, seen, nw_done):
    lq = np.array([len(t[0]) for t in tasks], np.int64)
    rb = np.array([t[1] for t in tasks], np.int64); re_ = np.array([t[2] for t in tasks], np.int64)
    w = np.array([t[3] for t in tasks], np.int64)
    R = rule(lq, rb, re_, w, np.zeros(len(tasks), np.int64), np.zeros(len(tasks), np.int64))
    sh, wb = R["shape"], R["wb_first"]
    for k, nm in enumerate(("shape_ring", "shape_row", "shape_global", "shape_flat")):
        _note(seen, nm, (sh == k).sum())
    dp = R["z"] > 0
    sc = (lq + R["rlen"]) * rule.pen
    for i, (task, tag, ans) in enumerate(zip(tasks, tags, exp)):
        assert (ans[2] is None) == (not R["ok"][i]), (i, task[1:], ans)
        if ans[2] is None:
            _note(seen, "null_return")
            continue
        qa, ra = cigar_independent(opt, st, task, ans, (i, tag, task[1:]))
        ops = [(c & 15, c >> 4) for c in ans[2]]
        longest_gap = max([ln for op, ln in ops if op], default=0)
        n, r = int(lq[i]), int(R["rlen"][i])
        if task[3] >= n + r and n <= 300 and r <= 300:
            key = (qa.tobytes(), ra.tobytes())
            if key not in nw_done:
                nw_done[key] = needleman_wunsch(opt, qa, ra)
            assert nw_done[key] == ans[0], (i, tag, task[1:], "Needleman-Wunsch", nw_done[key], "reported", ans[0])
            _note(seen, "whole_matrix_equals_needleman_wunsch")
        if tag is None:
            continue
        _note(seen, "ring_31", tag.startswith("band_31") and sh[i] == CP.RING and wb[i] == 31)
        _note(seen, "row_32", tag.startswith("band_32") and sh[i] == CP.ROW and wb[i] == 32)
        if tag.endswith("_indel") and longest_gap >= wb[i] - 2:
            assert {op for op, ln in ops if ln >= wb[i] - 2} >= {1, 2}, (i, tag, ops)
            _note(seen, "ring_31_indel_at_the_edge", sh[i] == CP.RING and longest_gap == 31)
            _note(seen, "row_32_indel_at_the_edge", sh[i] == CP.ROW and longest_gap == 32)
            _note(seen, "band_31_indel_beside_the_edge", wb[i] == 31 and longest_gap == 29)
        if tag == "all_mismatch":
            assert all((qa[:, None] != ra[None, :max(1, min(len(ra), 300))]).all(axis=1)) and ans[1] >= n, (i, task[1:])
            _note(seen, "small_220", n == 220 and sh[i] != CP.GLOBAL); _note(seen, "global_221", n == 221 and sh[i] == CP.GLOBAL)
            _note(seen, "small_score_below", n <= 220 and CP.CG_SMALL - rule.pen <= sc[i] < CP.CG_SMALL and sh[i] != CP.GLOBAL)
            _note(seen, "small_score_at", n <= 220 and CP.CG_SMALL <= sc[i] < CP.CG_SMALL + rule.pen and sh[i] == CP.GLOBAL)
            _note(seen, "all_mismatch_reverse_strand", task[1] >= st.l_pac)
        if tag == "strand_edge":
            kind = "flat" if sh[i] == CP.FLAT else "dp"
            _note(seen, "strand_first_" + kind, task[1] in (0, st.l_pac)); _note(seen, "strand_last_" + kind, task[2] in (st.l_pac, 2 * st.l_pac))
            _note(seen, "strand_edge_q_len_%d" % n)
        _note(seen, "rlen_lt_8", tag == "short_range" and r < 8 and dp[i])
        _note(seen, "q_len_1", tag == "q_len_1" and n == 1)
        _note(seen, "band_wider_than_query", dp[i] and wb[i] >= n)
        if tag == "row_lengths":
            for m in set(cigar_row_lengths(n, r, int(wb[i])).tolist()):
                _note(seen, "row_length_mod_%d" % m)
            _note(seen, "row_length_steady_mod_%d" % ((2 * int(wb[i]) + 1) & 3), n > 2 * wb[i] + 1)
        if tag == "md_digits":
            digits = max(len(d) for d in re.findall(rb"\d+", ans[3]))
            _note(seen, "md_4_digits", digits == 4); _note(seen, "md_5_digits", digits == 5)
            _note(seen, "md_digits_flat", sh[i] == CP.FLAT); _note(seen, "md_digits_dp", dp[i])
    return seen


CIGAR_WANTED = (["shape_row", "shape_global", "shape_flat", "null_return", "whole_matrix_equals_needleman_wunsch", "row_32", "row_32_indel_at_the_edge",
                 "global_221", "small_score_at", "all_mismatch_reverse_strand", "strand_first_flat", "strand_first_dp", "strand_last_flat", "strand_last_dp",
                 "rlen_lt_8", "q_len_1", "band_wider_than_query", "md_4_digits", "md_5_digits", "md_digits_flat", "md_digits_dp", "row_length_steady_mod_1", "row_length_steady_mod_3"]
                + ["strand_edge_q_len_%d" % n for n in (7, 8, 9, 15, 16, 17)] + ["row_length_mod_%d" % m for m in range(4)])
CIGAR_WANTED_LDS = ["small_220", "small_score_below"]             # unless BM2_CIGAR_NO_LDS=1
CIGAR_WANTED_RING = ["shape_ring", "ring_31", "ring_31_indel_at_the_edge", "band_31_indel_beside_the_edge"]      # unless BM2_CIGAR_NO_RING=1 (or NO_LDS)


def _cigar_diff(tasks, tags, exp, got, who):
    assert len(exp) == len(got) == len(tasks)
    bad = [i for i, (x, y) in enumerate(zip(exp, got)) if x != y]
    assert not bad, "%s: %d of %d differ; first: task %d (q_len %d, %d..%d, w %d, made for %s) host %s, %s %s" % (
        who, len(bad), len(tasks), bad[0], len(tasks[bad[0]][0]), tasks[bad[0]][1], tasks[bad[0]][2], tasks[bad[0]][3], tags[bad[0]],
        str(exp[bad[0]])[:300], who, str(got[bad[0]])[:300])


def check_cigar(run, index_prefix, opt_sets=None, n_random=1000, knobs=None, who="device"):
    """run(tasks, opt) = the form under test with this index (None: the host twin alone).  knobs: what the environment of run's process sets of
    (no_lds, no_ring), for the restated shape rule.  -> the event counts"""
    ctg = genome()
    st = Strands(ctg)
    total = {}
    for k, kw in enumerate(OPTION_SETS if opt_sets is None else opt_sets):
        opt = bm2.default_opt(**kw)
        rule = CP.Rule(opt, l_pac=st.l_pac, **(knobs or {}))
        nw_done = {}                                             # (a pair of sequences comes once per band and batch size)
        tasks, tags = cigar_hand_made(opt, ctg, 700 + k)
        if n_random:
            more = make_tasks(ctg, 750 + k, n_random)
            tasks += more; tags += [None] * len(more)
        exp = bm2.gen_cigar(index_prefix, opt, tasks)
        if run is not None:
            _cigar_diff(tasks, tags, exp, run(tasks, opt), who)
            for n in (1, 63, 64, 65):                            # batches around the block of the DP kernels: the first hand-made tasks
                _cigar_diff(tasks[:n], tags[:n], exp[:n], run(tasks[:n], opt), "%s, %d tasks" % (who, n))
                _note(total, "batch_of_%d" % n)
        cigar_events(opt, st, rule, tasks, tags, exp, total, nw_done)
    kn = knobs or {}
    wanted = CIGAR_WANTED + ([] if kn.get("no_lds") else CIGAR_WANTED_LDS) + ([] if kn.get("no_lds") or kn.get("no_ring") else CIGAR_WANTED_RING)
    wanted = [ev for ev in wanted if not (kn.get("no_lds") and ev in ("shape_row", "row_32", "row_32_indel_at_the_edge"))]
    if run is not None:
        wanted += ["batch_of_%d" % n for n in (1, 63, 64, 65)]
    missing = [ev for ev in wanted if not total.get(ev)]
    assert not missing, (missing, sorted(total.items()))
    if kn.get("no_ring") or kn.get("no_lds"):
        assert not total.get("shape_ring"), total
    if kn.get("no_lds"):
        assert not total.get("shape_row"), total
    return total


def parse_refdump_cigar(raw):
    exp, p = [], 0
    while p < len(raw):
        sc, nc, nm = np.frombuffer(raw, "<i4", 3, p); p += 12
        if nc < 0:
            exp.append((int(sc), int(nm), None, b"")); continue
        ops = [int(x) for x in np.frombuffer(raw, "<u4", nc, p)]; p += 4 * nc
        e = raw.index(b"\0", p); md = raw[p:e]; p += (e - p + 1 + 3) & ~3
        exp.append((int(sc), int(nm), ops, md))
    return exp


def check_cigar_against_reference(dump, tmp, index_prefix, set_no, form=None, n_random=1000):
    """the reference's own bwa_gen_cigar2 (oracle/_ref/refdump cigar) on the same tasks; form(tasks, opt): the form compared (default: host)"""
    ctg = genome()
    opt = bm2.default_opt(**OPTION_SETS[set_no])
    tasks, tags = cigar_hand_made(opt, ctg, 700 + set_no)
    more = make_tasks(ctg, 750 + set_no, n_random)
    tasks += more; tags += [None] * len(more)
    tf, of = str(tmp / "tasks.txt"), str(tmp / "out.bin")
    with open(tf, "w") as f:
        for q, rb, re_, w in tasks:
            f.write("%d %d %d %s\n" % (w, rb, re_, "".join("ACGTN"[c] for c in q)))
    subprocess.check_call([dump] + REF_ARGS[set_no] + ["cigar", index_prefix, tf, of], stderr=subprocess.DEVNULL)
    ref = parse_refdump_cigar(open(of, "rb").read())
    got = bm2.gen_cigar(index_prefix, opt, tasks) if form is None else form(tasks, opt)
    assert len(ref) == len(got) == len(tasks)
    for i, (x, y) in enumerate(zip(ref, got)):
        if x[2] is None:
            assert y[2] is None, "task %d: the reference returns NULL" % i
        else:
            assert x == y, "task %d (made for %s; w %d, %d..%d): reference %s ours %s" % (i, tags[i], tasks[i][3], tasks[i][1], tasks[i][2], str(x)[:300], str(y)[:300])
    return len(tasks)


# ================================================================================================ the sanitizer program's input
def dump_ksw(path):
    """the hand-made rescue tasks under every option set, as tools/san/ksw_san.cpp reads them: int64 sets; per set the 25 matrix bytes, 7 pad
    bytes, int32 o_del, e_del, o_ins, e_ins, int64 tasks, int64 sequence bytes, then q_off, t_off (int64), q_len, t_len, xtra (int32) and the
    sequences -> (sets, tasks)"""
    sets = []
    for k, kw in enumerate(OPTION_SETS):
        opt = bm2.default_opt(**kw)
        pairs, xtra = [], []
        for b in ksw_hand_made(opt, 900 + k):
            pairs += b.pairs; xtra += b.xtra
        sets.append((opt, pairs, xtra))
    with open(path, "wb") as f:
        f.write(np.array([len(sets)], np.int64).tobytes())
        for opt, pairs, xtra in sets:
            q_off, t_off, ql, tl, buf = [], [], [], [], []
            p = 0
            for q, t in pairs:
                q_off.append(p); ql.append(len(q)); buf.append(q); p += len(q)
                t_off.append(p); tl.append(len(t)); buf.append(t); p += len(t)
            f.write(np.array(list(opt.mat) + [0] * 7, np.int8).tobytes())
            f.write(np.array([opt.o_del, opt.e_del, opt.o_ins, opt.e_ins], np.int32).tobytes())
            f.write(np.array([len(pairs), p], np.int64).tobytes())
            f.write(np.array(q_off, np.int64).tobytes() + np.array(t_off, np.int64).tobytes())
            f.write(np.array(ql, np.int32).tobytes() + np.array(tl, np.int32).tobytes() + np.array(xtra, np.int32).tobytes())
            f.write(np.concatenate(buf).astype(np.uint8).tobytes())                      # (exactly the bytes the offsets reach: one past is the sanitizer's to catch)
    return len(sets), sum(len(s[1]) for s in sets)


def ksw_hand_made_answers():
    """the host twin's answers to the same tasks, in the dump's order: what the sanitizer build must print"""
    out = []
    for k, kw in enumerate(OPTION_SETS):
        opt = bm2.default_opt(**kw)
        pairs, xtra = [], []
        for b in ksw_hand_made(opt, 900 + k):
            pairs += b.pairs; xtra += b.xtra
        out.append(bm2.ksw_align2(pairs, xtra, opt))
    return np.concatenate(out)
