"""k_chain_group (BM2_CHAIN_GROUP = G): light reads chained by groups of G adjacent lanes on records staged in the group's share of the workgroup's LDS, against
the oracle, byte for byte, and against the same batch with the knob off.  Parameters: G, the bound to the wavefront-per-read tiers (BM2_HEAVY_SA), the bound
to k_chain (BM2_CHAIN_GROUP_MIN) and who builds the extension tasks (BM2_CHAIN_FUSE_FINISH).

The batch is made here, as in test_chain_lds_compact_gpu.py: a small genome with EXACT repeat families of chosen copy numbers.  A read inside a unit of a
family of K > 20 copies has one SMEM with K occurrences; with one or two substitutions it has two or three; below 20 copies the third seeding pass adds
seeds of 20 bases (eight times K seeds in all).  Reads cut short bring the seed counts below those of a whole ordinary read.  The test asserts from the batch's own counts that
  every class edge of the launches is there on both sides (4, 5, 8, 9, 16, 17, 32, 33, 56, 57, 64, 65 seeds);
  a read of a group launch has more than 9 chains (a tree in a group's LDS has split);
  some wavefront of every launch holds reads of different seed counts in its groups (the class partition's order, restated here);
  the cases with BM2_CHAIN_GROUP_CAP_MAX=32 have reads of a group launch beyond that capacity (chained by the group's first lane on their global slices),
  the others have every read of theirs staged, up to the bound to the tiers.
Runs on the device, and on the host emulator of the device sources with BM2_EMU_LIB set."""
import numpy as np
import pytest

import bm2
import helpers
from helpers import build_index, first_diff, regs_to_records
from tools import oracle, refio, synth

pytestmark = pytest.mark.gpu

UNIT = 220                                   # bases of a repeat unit; a read is the 150 bases from 35 on
FAMILIES = [2, 3, 4, 5, 6, 7, 8, 17, 24, 28, 32, 33, 40, 56, 57, 64, 65]
SHORT_OF = 17                                # this family's read also comes in its first 19, 25 and 39 bases
EDGES = (4, 5, 8, 9, 16, 17, 32, 33, 56, 57, 64, 65)
CLASS_LO = (64, 32, 16, 8, 4, -1)            # light classes of the partition (scan.hip: work_class), falling: > 64, > 32, > 16, > 8, > 4, the rest


def _make_case(tmp):
    rng = np.random.default_rng(20261019)
    contigs = [rng.integers(0, 4, size=n, dtype=np.uint8) for n in (700000, 350000)]
    slots = [(ci, p) for ci, c in enumerate(contigs) for p in range(1000, len(c) - 1000, 256)]      # one unit per slot: copies never overlap
    order = rng.permutation(len(slots))
    at = 0
    reads = []
    for k in FAMILIES:
        unit = rng.integers(0, 4, size=UNIT, dtype=np.uint8)
        for _ in range(k):
            ci, p = slots[order[at]]
            at += 1
            contigs[ci][p:p + UNIT] = unit if rng.random() < 0.5 else synth._revcomp_codes(unit)
        reads.append(unit[35:185].copy())
        for n_sub in (1, 2):                                       # the same read with one or two substitutions: two or three SMEMs of K occurrences each
            r = unit[35:185].copy()
            for p in ((75,), (50, 100))[n_sub - 1]:
                r[p] = (r[p] + 1 + rng.integers(0, 3)) % 4
            reads.append(r)
        if k == SHORT_OF:
            reads += [unit[35:35 + L].copy() for L in (19, 25, 39)]
    assert at <= len(slots)
    names = ["chr%d" % (i + 1) for i in range(len(contigs))]
    fa = str(tmp / "exact.fa")
    synth.write_fasta(fa, names, contigs)
    if not build_index(fa):
        helpers.no_checker("oracle/_ref reference binary not present (build it with `make -C oracle ref`)")
    more = synth.make_reads_se(20261020, contigs, 200, L=150)       # ordinary reads, some of them across the planted units
    shorts = [np.asarray(more[i], np.uint8)[:L].copy() for i, L in enumerate(range(40, 150, 5))]      # ordinary reads cut short: fewer seeds than any whole one
    allr = [np.asarray(r, np.uint8) for r in reads] + shorts + [np.asarray(r, np.uint8) for r in more]
    return fa, refio.pack_reads(allr)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    fa, (enc, off, ln) = _make_case(tmp_path_factory.mktemp("grp"))
    ix = oracle.Index(fa)
    try:
        exp = ix.run(enc, off, ln)["REGPRG"]
    finally:
        ix.close()
    return fa, enc, off, ln, exp, {}


def _run(gpu_ctx_factory, monkeypatch, fa, enc, off, ln, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))
    ctx = gpu_ctx_factory(fa)
    regs, reg_off, st = ctx.seed_chain_extend(enc, off, ln, bm2.default_opt())
    return ctx, regs_to_records(regs, reg_off)


def _wave_mixes(n_sa_read, heavy_sa, lo, hi, per_wave):
    """For every light class with reads of the group launches (lo < seeds <= hi): does some wavefront of its launch hold reads of different seed counts?
    (class k of the partition = the reads of that class in their own order; wavefront w of a launch starts at the class's read w * per_wave)"""
    out = {}
    for k, c_lo in enumerate(CLASS_LO):
        c_hi = heavy_sa if k == 0 else CLASS_LO[k - 1]
        members = n_sa_read[(n_sa_read > c_lo) & (n_sa_read <= min(c_hi, heavy_sa))]
        mixed, any_mine = False, False
        for w in range(0, len(members), per_wave):
            mine = [int(x) for x in members[w:w + per_wave] if lo < x <= hi]
            any_mine = any_mine or bool(mine)
            mixed = mixed or len(set(mine)) > 1
        if any_mine and k > 0:
            out[k] = mixed
    return out


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("grp_min", [0, 4])
@pytest.mark.parametrize("heavy_sa", [56, 64])
@pytest.mark.parametrize("g", [2, 4, 8])
def test_lane_groups_keep_every_reg(gpu_ctx_factory, case, monkeypatch, g, heavy_sa, grp_min, fuse):
    fa, enc, off, ln, exp, off_runs = case
    cap_max = 32 if grp_min == 4 else 64                     # (half of the cases put the reads of 33..64 seeds on the not-staged path of their launch)
    common = {"BM2_HEAVY_SA": heavy_sa, "BM2_CHAIN_FUSE_FINISH": fuse}
    if (heavy_sa, fuse) not in off_runs:                      # the same batch with the knob off, once per setting of the other two
        _, rec0 = _run(gpu_ctx_factory, monkeypatch, fa, enc, off, ln, dict(common, BM2_CHAIN_GROUP=0))
        off_runs[(heavy_sa, fuse)] = rec0.tobytes()
    ctx, got = _run(gpu_ctx_factory, monkeypatch, fa, enc, off, ln,
                    dict(common, BM2_CHAIN_GROUP=g, BM2_CHAIN_GROUP_MIN=grp_min, BM2_CHAIN_GROUP_CAP_MAX=cap_max))
    # the shapes, from the batch's own counts (n_sa_read of the pipeline: the SA coordinates between the read's first and last SMEM)
    n = len(ln)
    cnt = ctx.batch_fetch("smem_cnt", "<i4")[:n].astype(np.int64)
    so = ctx.batch_fetch("smem_off", "<i8")[:n]
    sa_off = ctx.batch_fetch("sa_off", "<i8")
    n_sa_read = np.where(cnt > 0, sa_off[so + cnt] - sa_off[so], 0)
    have = set(int(x) for x in n_sa_read)
    print("seeds per read:", sorted(have))
    missing = [e for e in EDGES if e not in have]
    assert not missing, "no read with %s seeds (%s)" % (missing, sorted(have))
    hi = min(64, heavy_sa)
    mine = (n_sa_read > grp_min) & (n_sa_read <= hi)
    assert mine.sum() > 100, "the group launches have %d reads" % mine.sum()
    n_chain0 = ctx.batch_fetch("n_chain0", "<i4")[:n]
    assert (mine & (n_sa_read <= 56) & (n_sa_read <= cap_max) & (n_chain0 > 9)).any(), "no tree in a group's LDS ever split"
    mixes = _wave_mixes(n_sa_read, heavy_sa, grp_min, hi, 64 // g)
    print("launch classes with a wavefront of mixed seed counts:", mixes)
    assert mixes and all(mixes.values()), "a group launch without a wavefront that holds reads of different seed counts (%s)" % mixes
    if cap_max < 64:
        assert (mine & (n_sa_read > cap_max)).sum() >= 3, "no read of a group launch fails the staging guard"
    else:
        assert (mine & (n_sa_read > 32)).any() and int(n_sa_read[mine].max()) == hi, "no staged read at the bound to the tiers"
    assert len(exp) == len(got) and exp.tobytes() == got.tobytes(), first_diff(exp, got)
    assert got.tobytes() == off_runs[(heavy_sa, fuse)], "differs from the same batch with BM2_CHAIN_GROUP=0"
