"""k_chain_heavy with a staged read's working set in the COMPACT LDS form (BM2_CHAIN_LDS_COMPACT, chain_dev.h: 40-byte chains and nodes, a 16-bit successor per
staged seed, 16-bit order entries) against the oracle, byte for byte, beside the old layout (0) and with mem_chain_flt's walk by one lane or by the wavefront
(BM2_CHAIN_COOP_FLT).  BM2_HEAVY_SA=8 sends nearly every read to a tier; BM2_CHAIN_TIER_MAX is lifted so that all five tiers are launched and the last one
takes the read beyond its capacity on its global slices, in the same launch.

The batch is made here: a small genome with EXACT repeat families of chosen copy numbers.  A read that lies inside a unit of a family of K > 20 copies has one
SMEM with K occurrences -- K seeds, K chains of one seed, all of one weight, all kept -- so the shapes at which the layout can go wrong are there by
construction, and the test asserts from the batch's own seed counts that they are:
  a read just above the threshold (9 seeds); a read of more than 9 chains (the first split of the tree); reads of 128 / 129 and 256 / 257 seeds (tier edges);
  a read above the largest capacity (1000: three pieces of families of 400 copies); a read with more than 64 kept chains (the cooperative filter's second block).
Runs on the device, and on the host emulator of the device sources with BM2_EMU_LIB set."""
import numpy as np
import pytest

import bm2
import helpers
from helpers import build_index, first_diff, regs_to_records
from tools import oracle, refio, synth

pytestmark = pytest.mark.gpu

UNIT = 220                                   # bases of a repeat unit; a read is the 150 bases from 35 on
FAMILIES = [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 24, 70, 128, 129, 256, 257]
PIECE_COPIES = 400                           # three families of 60-base units: a read of three 50-base pieces has ~1200 seeds


def _make_case(tmp):
    rng = np.random.default_rng(20261018)
    contigs = [rng.integers(0, 4, size=n, dtype=np.uint8) for n in (700000, 350000)]
    slots = [(ci, p) for ci, c in enumerate(contigs) for p in range(1000, len(c) - 1000, 256)]      # one unit per slot: copies never overlap
    order = rng.permutation(len(slots))
    at = 0

    def plant(unit, copies):
        nonlocal at
        for _ in range(copies):
            ci, p = slots[order[at]]
            at += 1
            contigs[ci][p:p + len(unit)] = unit if rng.random() < 0.5 else synth._revcomp_codes(unit)

    reads = []
    for k in FAMILIES:
        unit = rng.integers(0, 4, size=UNIT, dtype=np.uint8)
        plant(unit, k)
        reads.append(unit[35:185].copy())
        for _ in range(2):                                         # the same read with one or two substitutions: two or three SMEMs of K occurrences each
            r = unit[35:185].copy()
            for p in rng.integers(25, 125, size=int(rng.integers(1, 3))):
                r[p] = (r[p] + 1 + rng.integers(0, 3)) % 4
            reads.append(r)
    pieces = []
    for _ in range(3):
        unit = rng.integers(0, 4, size=60, dtype=np.uint8)
        plant(unit, PIECE_COPIES)
        pieces.append(unit[5:55])
    reads.append(np.concatenate(pieces))
    reads.append(np.concatenate(pieces[::-1]))
    assert at <= len(slots)
    names = ["chr%d" % (i + 1) for i in range(len(contigs))]
    fa = str(tmp / "exact.fa")
    synth.write_fasta(fa, names, contigs)
    if not build_index(fa):
        helpers.no_checker("oracle/_ref reference binary not present (build it with `make -C oracle ref`)")
    more = synth.make_reads_se(20261019, contigs, 200, L=150)       # ordinary reads, some of them across the planted units
    allr = [np.asarray(r, np.uint8) for r in reads] + [np.asarray(r, np.uint8) for r in more]
    return fa, refio.pack_reads(allr)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    fa, (enc, off, ln) = _make_case(tmp_path_factory.mktemp("cpt"))
    ix = oracle.Index(fa)
    try:
        exp = ix.run(enc, off, ln)["REGPRG"]
    finally:
        ix.close()
    return fa, enc, off, ln, exp


@pytest.mark.parametrize("compact,coop", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_compact_lds_form_keeps_every_reg(gpu_ctx_factory, case, monkeypatch, compact, coop):
    fa, enc, off, ln, exp = case
    for k, v in (("BM2_HEAVY_SA", 8), ("BM2_CHAIN_TIER_MAX", 1000000), ("BM2_CHAIN_LDS_COMPACT", compact), ("BM2_CHAIN_COOP_FLT", coop)):
        monkeypatch.setenv(k, str(v))
    ctx = gpu_ctx_factory(fa)
    regs, reg_off, st = ctx.seed_chain_extend(enc, off, ln, bm2.default_opt())
    # the shapes, from the batch's own counts (n_sa_read of the pipeline: the SA coordinates between the read's first and last SMEM)
    n = len(ln)
    cnt = ctx.batch_fetch("smem_cnt", "<i4")[:n].astype(np.int64)
    so = ctx.batch_fetch("smem_off", "<i8")[:n]
    sa_off = ctx.batch_fetch("sa_off", "<i8")
    n_sa_read = np.where(cnt > 0, sa_off[so + cnt] - sa_off[so], 0)
    have = set(int(x) for x in n_sa_read)
    print("seeds per read:", sorted(have))
    for want in (9, 128, 129, 256, 257):
        assert want in have, "no read with %d seeds (%s)" % (want, sorted(have))
    assert n_sa_read.max() > 1000, "no read beyond the last tier's capacity (%d)" % n_sa_read.max()
    assert (n_sa_read > 8).sum() > 0.25 * n
    n_chain0 = ctx.batch_fetch("n_chain0", "<i4")[:n]
    assert ((n_chain0 > 9) & (n_sa_read <= 1000)).any(), "no tree in LDS ever split"
    base = ctx.batch_fetch("read_base", "<i8")[:n]
    n_chain = ctx.batch_fetch("n_chain", "<i4")[:n]
    chn = ctx.batch_fetch("chn", bm2.DEVCHAIN_DT)
    # mem_chain_flt drops a chain only against a kept one of at least twice its weight: where all chains of a read weigh the same, every one of them is kept
    kept = max(int(c) for b, c, c0, s in zip(base, n_chain, n_chain0, n_sa_read)
               if 8 < s <= 1000 and c == c0 and len(set(chn["w"][int(b):int(b) + int(c)].tolist())) == 1)
    assert kept > 64, "no read in LDS whose kept chains go beyond one block of the cooperative filter (%d)" % kept
    got = regs_to_records(regs, reg_off)
    assert len(exp) == len(got) and exp.tobytes() == got.tobytes(), first_diff(exp, got)
