"""The pairing decisions of mem_sam_pe on the MI355X (decide.hip) -- sorted after the text file on purpose.  bm2_pe_decide_dev against
bm2_pe_decide on lists made by hand and at random and on the arithmetic sweep (2 x 60 000 pairs), the refusals, and bm2_sam_pe_dev / the
_multi form with BM2_SAM_F_DEVICE_DECIDE (alone and with BM2_SAM_F_DEVICE_TEXT) against the flag-off text and `bwa-mem2 mem`'s.  All
comparisons are exact.  The checks themselves are in pe_decide_cases.py, shared with the emulator tests."""
import os
import subprocess

import numpy as np
import pytest

import bm2
import helpers
import pe_decide_cases as S
import test_sam_tail as T
from helpers import ref_binary
from tools import synth

pytestmark = pytest.mark.gpu
SWEEP_PAIRS = 60000


def test_lists_made_by_hand_and_at_random_device_against_host(gpu_ctx_factory, golden_dir):
    pre = os.path.join(golden_dir, "g60k.fa")
    total = S.check_lists(gpu_ctx_factory(pre), pre)
    print(total)


def test_arithmetic_sweep_device_against_host(gpu_ctx_factory, golden_dir):
    pre = os.path.join(golden_dir, "g60k.fa")
    done, total = S.check_sweep(gpu_ctx_factory(pre), pre, SWEEP_PAIRS)
    print(done, total)
    assert done >= 100000, done


def test_refusals_of_the_record_level_entry_points(gpu_ctx_factory, golden_dir):
    pre = os.path.join(golden_dir, "g60k.fa")
    assert S.check_refusals(gpu_ctx_factory(pre), pre)


def test_sam_pe_dev_with_device_decide(gpu_ctx_factory, tmp_path):
    fa, r1, r2 = T._pe_case(tmp_path, 61, 3000, sub_rate=0.02, indel_frac=0.2, random_frac=0.03)
    ctx = gpu_ctx_factory(fa)
    ctx2 = bm2.Context(0, share=ctx)
    try:
        tail = S.PeTail(T, tmp_path, fa, r1, r2)
        tail.option_sets(ctx, ctx2, part_knob=1000)
        assert bm2.sam_decide_stats()[2] > 0                      # (pairs with more than 16 hits in all: 511 of the default run)
    finally:
        ctx2.close()


def test_sam_pe_dev_constructed_case_reaches_the_rare_branches(gpu_ctx_factory, tmp_path):
    fa, r1, r2 = S.constructed_case(T, tmp_path)
    tail = S.PeTail(T, tmp_path, fa, r1, r2)
    ctx = gpu_ctx_factory(fa)
    ref, pes = tail.check([], ctx, both=True)
    tail.check(["-S"], ctx, flag=0x20)
    seen = tail.host_outcomes(pes)
    print(seen, len(ref.splitlines()))
    assert seen["paired_below"] > 0 and seen["second_primary"] > 0 and seen["paired_above"] > 0 and seen["empty"] > 0, seen


def test_sam_se_dev_rejects_the_bit(gpu_ctx_factory, tmp_path):
    fa, reads = T._case(tmp_path, 59, 8, L=100)
    with pytest.raises(bm2.Bm2Error) as e:
        T._ours(fa, reads, ["q%d" % i for i in range(len(reads))], [b"F" * len(r) for r in reads], None,
                bm2.default_sam_opt(flag=bm2.SAM_F_DEVICE_DECIDE), ctx=gpu_ctx_factory(fa))
    assert e.value.rc == bm2.BM2_EINVAL and "DEVICE_DECIDE" in str(e.value)


def test_fastq_to_sam_through_the_device_with_device_decide(gpu_ctx_factory, tmp_path):
    # as tests/test_zzz_sam_text_gpu.py: genome seed 81 with an ALT contig, device hits, batch_finish, then the PE tail with the bit(s)
    exe = ref_binary()
    if exe is None:
        helpers.no_checker("oracle/_ref reference binary not present")
    names, ctg, alts = synth.make_genome(81, [300000, 150000, 60000], alt_contigs=1, alt_len=4000, n_repeat_families=8, repeat_len=(200, 2500),
                                         copies=(3, 30), divergence=(0.0, 0.06))
    fa = str(tmp_path / "g.fa")
    synth.write_fasta(fa, names, ctg)
    synth.write_alt(fa + ".alt", alts)
    subprocess.check_call([exe, "index", fa], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r1, r2 = synth.make_reads_pe(82, ctg, 3000, L=150, sub_rate=0.015, indel_frac=0.15, random_frac=0.01)
    rng = np.random.default_rng(5)
    f1, f2 = str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq")
    for path, rr, suffix in ((f1, r1, b"/1"), (f2, r2, b"/2")):
        with open(path, "wb") as f:
            for i, r in enumerate(rr):
                q = bytes(rng.integers(40, 74, size=len(r), dtype=np.uint8))
                f.write(b"@pair%d" % i + suffix + b"\n" + bytes(b"ACGTN"[c] for c in r) + b"\n+\n" + q + b"\n")
    p = subprocess.run([exe, "mem", "-t", "1", fa, f1, f2], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
    ref = b"".join(l for l in p.stdout.splitlines(keepends=True) if not l.startswith(b"@"))
    opt = bm2.default_opt()
    ctx = gpu_ctx_factory(fa)
    with bm2.FastqChunk(open(f1, "rb").read(), open(f2, "rb").read()) as chunk:
        ctx.batch_upload_chunk(chunk)
        ctx.batch_run(opt)
        ctx.batch_finish(opt)
        aln, aln_off = ctx.batch_download_alnregs()
        off_text = ctx.sam(chunk, opt, bm2.default_sam_opt(), aln, aln_off).tobytes()
        assert ref == off_text, T._diff(ref, off_text)
        for bits in (bm2.SAM_F_DEVICE_DECIDE, bm2.SAM_F_DEVICE_DECIDE | bm2.SAM_F_DEVICE_TEXT):
            on_text = ctx.sam(chunk, opt, bm2.default_sam_opt(flag=bits), aln, aln_off).tobytes()
            assert ref == on_text, T._diff(ref, on_text)
            pairs, n_hits, heavy = bm2.sam_decide_stats()
            assert pairs == 3000 and n_hits >= len(aln), (pairs, n_hits, heavy)
