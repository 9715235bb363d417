"""The seeding K-mer table (BM2_SEED_KMER = K; smem.hip): forward walks of passes 1 and 2 that start from the table entry of their first K bases, and backward
phases that hold the candidates of forward length 1..K-1 back until the row in which they are one table entry.  Against the oracle, byte for byte (the SMEM
stage and the final regs), and against the same batch with BM2_SEED_KMER=0.

The genome is small (about 1 Mbp), so K is forced small: 4 (every entry's size is in the thousands), 6, 8 and 10 (most entries hold 0..3 occurrences, so pass 2's
min_intv fails when a candidate arrives).  The batch is made here: a genome with a few high-copy diverged repeat families (as test_pipeline_gpu._repeat_case
makes them: lists beyond the slot and k_bwd_heavy) with EXACT repeat families of 2..64 copies planted on it (as in test_chain_group_gpu.py); reads of the exact
units, whole and with one or two substitutions (equal sizes on arrival), reads with a substitution every 8..10 bases (walks that end below K), reads of K-1, K,
K+1, 19, 20 and 25 bases, reads with an ambiguous base at 0, K-1, K, the middle, L-K and L-1, ordinary reads and reads of the diverged families.
Which paths a case took is asserted from the kernels' own counters (seed_counters_all[27..36]): every one of them is non-zero in the case built for it, and
the jump counter is zero where the rule has to switch itself off (min_seed_len <= K).
Runs on the device, and on the host emulator of the device sources with BM2_EMU_LIB set."""
import numpy as np
import pytest

import bm2
import helpers
from helpers import ONT2D, build_index, first_diff, regs_to_records
from tools import oracle, refio, synth

pytestmark = pytest.mark.gpu

KS = (4, 6, 8, 10)
UNIT = 220
FAMILIES = (2, 3, 8, 24, 64)
# seed_counters_all, from 27 on (SC_KJ_* / SC_KV_* of smem.hip)
JUMP, FB_END, FB_AMB, FB_SIZE, KEPT, DROP_SIZE, DROP_EQ, PENDING_END, HEAVY, POSTPONED = range(27, 37)
NAMES = {JUMP: "walks that jumped", FB_END: "fallback: end of read", FB_AMB: "fallback: ambiguous base", FB_SIZE: "fallback: size below min_intv",
         KEPT: "arrivals kept", DROP_SIZE: "arrivals dropped for size", DROP_EQ: "arrivals dropped for equality", PENDING_END: "tasks ended with arrivals pending",
         HEAVY: "arrivals in k_bwd_heavy", POSTPONED: "hand-overs postponed"}


def _make_case(tmp):
    rng = np.random.default_rng(20261101)
    names, contigs, _ = synth.make_genome(61, [700000, 350000], alt_contigs=0, n_repeat_families=4, repeat_len=(1500, 4000), copies=(150, 300),
                                          divergence=(0.005, 0.04))
    contigs = [np.asarray(c, np.uint8).copy() for c in contigs]
    rich = [np.asarray(r, np.uint8) for r in synth.make_reads_se(62, contigs, 500, L=150)]      # (before the exact units go in: mostly reads of the diverged families)
    slots = [(ci, p) for ci, c in enumerate(contigs) for p in range(1000, len(c) - 1000, 256)]
    order = rng.permutation(len(slots))
    at = 0
    fam = []
    for k in FAMILIES:
        unit = rng.integers(0, 4, size=UNIT, dtype=np.uint8)
        for _ in range(k):
            ci, p = slots[order[at]]
            at += 1
            contigs[ci][p:p + UNIT] = unit if rng.random() < 0.5 else synth._revcomp_codes(unit)
        fam.append(unit[35:185].copy())
        for n_sub in (1, 2):
            r = unit[35:185].copy()
            for p in ((75,), (50, 100))[n_sub - 1]:
                r[p] = (r[p] + 1 + rng.integers(0, 3)) % 4
            fam.append(r)
    fa = str(tmp / "kmer.fa")
    synth.write_fasta(fa, names, contigs)
    if not build_index(fa):
        helpers.no_checker("oracle/_ref reference binary not present (build it with `make -C oracle ref`)")
    genome = np.concatenate([c for c in contigs])

    def clean_slice(L):                                           # L bases of the genome without an ambiguous one
        while True:
            p = int(rng.integers(0, len(genome) - L))
            if (genome[p:p + L] < 4).all():
                return genome[p:p + L].copy()
    ordinary = [np.asarray(r, np.uint8) for r in synth.make_reads_se(63, contigs, 120, L=150)]
    dense = []
    for _ in range(24):                                           # a substitution every 8..10 bases
        r = clean_slice(150)
        p = int(rng.integers(0, 8))
        while p < 150:
            r[p] = (r[p] + 1 + rng.integers(0, 3)) % 4
            p += int(rng.integers(8, 11))
        dense.append(r)
    short = [clean_slice(L) for L in sorted({K + d for K in KS for d in (-1, 0, 1)} | {19, 20, 25}) for _ in range(2)]
    ambig = []
    for K in KS:
        for p in (0, K - 1, K, 75, 150 - K, 149):
            r = clean_slice(150)
            r[p] = 4
            ambig.append(r)
    head = fam + ordinary + dense + short + ambig                 # (the min_seed_len cases run this part alone)
    longs = [np.asarray(r, np.uint8) for r in synth.make_reads_long(64, contigs, 6, mean_len=3000, max_len=5000)]
    return fa, refio.pack_reads(head + rich), refio.pack_reads(head), refio.pack_reads(longs)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    fa, full, head, longs = _make_case(tmp_path_factory.mktemp("kmer"))
    return {"fa": fa, "full": full, "head": head, "long": longs, "exp": {}, "off": {}}


def _oracle(case, batch, kw):
    key = (batch, tuple(sorted(kw.items())))
    if key not in case["exp"]:
        enc, off, ln = case[batch]
        ix = oracle.Index(case["fa"])
        try:
            case["exp"][key] = ix.run(enc, off, ln, oracle.default_opt(**kw))
        finally:
            ix.close()
    return case["exp"][key]


def _smem_records(sm):
    got = np.zeros(len(sm), refio.SMEM_DT)
    for a, b in (("read", "rid"), ("m", "m"), ("n", "n"), ("k", "k"), ("l", "l"), ("s", "s")):
        got[a] = sm[b]
    return got


def _run(gpu_ctx_factory, monkeypatch, case, batch, kw, K, env=None, share=False):
    """one batch through the pipeline and the SMEM entry point -> (SMEM records, REGPRG records, n_ext, counters)"""
    monkeypatch.setenv("BM2_SEED_KMER", str(K))
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    enc, off, ln = case[batch]
    opt = bm2.default_opt(**kw)
    ctx = gpu_ctx_factory(case["fa"])
    outs = []
    for c in ([ctx, bm2.Context(0, share=ctx)] if share else [ctx]):
        try:
            regs, reg_off, st = c.seed_chain_extend(enc, off, ln, opt)
            sc = [int(v) for v in c.batch_fetch("seed_counters_all", np.uint64)]
            outs.append((_smem_records(c.smem(enc, off, ln, opt)), regs_to_records(regs, reg_off), st["n_ext"], sc))
        finally:
            if c is not ctx:
                c.close()
    return outs if share else outs[0]


def _off(gpu_ctx_factory, monkeypatch, case, batch, kw, env=None):
    key = (batch, tuple(sorted(kw.items())), tuple(sorted((env or {}).items())))
    if key not in case["off"]:
        case["off"][key] = _run(gpu_ctx_factory, monkeypatch, case, batch, kw, 0, env)
    return case["off"][key]


def _check(case, batch, kw, on, off, table_in_use=True):
    exp = _oracle(case, batch, kw)
    sm, rec, n_ext, sc = on
    sm0, rec0, n_ext0, sc0 = off
    print("n_ext: oracle %d, table off %d, table on %d" % (exp["counters"]["n_ext"], n_ext0, n_ext))
    print("counters:", {NAMES[i]: sc[i] for i in NAMES})
    assert len(exp["SMEM"]) == len(sm) and exp["SMEM"].tobytes() == sm.tobytes(), "SMEM: %s" % first_diff(exp["SMEM"], sm)
    assert len(exp["REGPRG"]) == len(rec) and exp["REGPRG"].tobytes() == rec.tobytes(), "REGPRG: %s" % first_diff(exp["REGPRG"], rec)
    assert sm0.tobytes() == sm.tobytes() and rec0.tobytes() == rec.tobytes(), "differs from the same batch with BM2_SEED_KMER=0"
    assert n_ext0 == exp["counters"]["n_ext"], "without the table every backwardExt of the reference is executed"
    assert not any(sc0[i] for i in NAMES), "BM2_SEED_KMER=0 and a table counter moved (%s)" % sc0[27:]
    if table_in_use:
        assert n_ext < n_ext0
        assert sc[JUMP] > 0
    else:
        assert n_ext == n_ext0 and not any(sc[i] for i in NAMES), "the rule did not switch itself off (%s)" % sc[27:]
    return sc


@pytest.mark.parametrize("K", KS)
def test_table_keeps_every_record(gpu_ctx_factory, case, monkeypatch, K):
    on = _run(gpu_ctx_factory, monkeypatch, case, "full", {}, K)
    sc = _check(case, "full", {}, on, _off(gpu_ctx_factory, monkeypatch, case, "full", {}))
    want = [JUMP, FB_END, FB_AMB, KEPT, PENDING_END, HEAVY]
    if K == 10:
        # entries of 0..3 occurrences: below pass 2's min_intv, in the walk and on arrival, and as many as the next longer candidate's (at K = 4 and 6
        # the sizes are in the thousands and hundreds: two candidates of one row never have the same)
        want += [FB_SIZE, DROP_SIZE, DROP_EQ]
    missing = [NAMES[i] for i in want if sc[i] == 0]
    assert not missing, "the batch never took: %s" % missing


@pytest.mark.parametrize("K", KS)
def test_handover_waits_for_the_last_arrival(gpu_ctx_factory, case, monkeypatch, K):
    env = {"BM2_BWD_EXPORT_AGE": 8}           # a hand-over wanted before row K - 1
    on = _run(gpu_ctx_factory, monkeypatch, case, "full", {}, K, env)
    sc = _check(case, "full", {}, on, _off(gpu_ctx_factory, monkeypatch, case, "full", {}, env))
    assert sc[21] > 0 and sc[22] > 0, "no backward task was handed over (%s)" % sc
    assert sc[POSTPONED] > 0, "no hand-over ever waited for an arrival"


@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("K", KS)
def test_rule_switches_itself_off(gpu_ctx_factory, case, monkeypatch, K, d):
    # a string of K bases must be too short to be a seed: in use at K + 1, off at K  (max_occ: seeds of 4..11 bases occur everywhere; the SMEMs do not depend on it)
    kw = {"min_seed_len": K + d, "max_occ": 20}
    on = _run(gpu_ctx_factory, monkeypatch, case, "head", kw, K)
    _check(case, "head", kw, on, _off(gpu_ctx_factory, monkeypatch, case, "head", kw), table_in_use=d == 1)


@pytest.mark.parametrize("K", KS)
def test_ont2d_long_reads(gpu_ctx_factory, case, monkeypatch, K):
    on = _run(gpu_ctx_factory, monkeypatch, case, "long", ONT2D, K)
    sc = _check(case, "long", ONT2D, on, _off(gpu_ctx_factory, monkeypatch, case, "long", ONT2D))
    assert sc[KEPT] > 0


def test_contexts_sharing_a_replica(gpu_ctx_factory, case, monkeypatch):
    a, b = _run(gpu_ctx_factory, monkeypatch, case, "head", {}, 8, share=True)
    _check(case, "head", {}, a, _off(gpu_ctx_factory, monkeypatch, case, "head", {}))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and b[3][JUMP] == a[3][JUMP] > 0
