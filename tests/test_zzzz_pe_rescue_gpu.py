"""Mate-rescue results applied to the hit lists on the MI355X (rescue.hip) -- sorted after the decide file on purpose.
bm2_pe_rescue_apply_dev against bm2_pe_rescue_apply on lists made by hand and at random with fabricated results, the refusals, and
bm2_sam_pe_dev / the _multi form with BM2_SAM_F_DEVICE_RESCUE (alone, with BM2_SAM_F_DEVICE_DECIDE, with that and
BM2_SAM_F_DEVICE_TEXT) against the flag-off text and `bwa-mem2 mem`'s.  All comparisons are exact.  The checks themselves are in
pe_rescue_cases.py, shared with the emulator tests."""
import os
import subprocess

import numpy as np
import pytest

import bm2
import helpers
import pe_decide_cases as S
import pe_rescue_cases as R
import test_sam_tail as T
from helpers import ref_binary
from tools import synth

pytestmark = pytest.mark.gpu


def test_lists_made_by_hand_and_at_random_device_against_host(gpu_ctx_factory, golden_dir):
    pre = os.path.join(golden_dir, "g60k.fa")
    total = R.check_lists(gpu_ctx_factory(pre), pre)
    print(total)
    assert total["heavy"] > 0 and total["list_over_16"] > 0, total


def test_refusals_of_the_record_level_entry_points(gpu_ctx_factory, golden_dir):
    pre = os.path.join(golden_dir, "g60k.fa")
    assert R.check_refusals(gpu_ctx_factory(pre), pre)


def test_real_tasks_host_form_against_the_flow_and_device_form_against_host(gpu_ctx_factory, tmp_path):
    fa, r1, r2 = T._pe_case(tmp_path, 61, 3000, sub_rate=0.02, indel_frac=0.2, random_frac=0.03)
    tail = S.PeTail(T, tmp_path, fa, r1, r2)
    st, out, out_off, redo, tasks, task_off, pes = R.check_real_tasks(tail)
    print(st)
    R.compare(gpu_ctx_factory(fa), fa, tail.opt, bm2.default_sam_opt(), tail.aln, np.asarray(tail.aln_off), tail.ln, pes, tasks, task_off, "real tasks")


def test_sam_pe_dev_with_device_rescue(gpu_ctx_factory, tmp_path):
    fa, r1, r2 = T._pe_case(tmp_path, 61, 3000, sub_rate=0.02, indel_frac=0.2, random_frac=0.03)
    ctx = gpu_ctx_factory(fa)
    ctx2 = bm2.Context(0, share=ctx)
    try:
        tail = S.PeTail(T, tmp_path, fa, r1, r2)
        ref, pes = R.check_tail(tail, [], ctx, n_threads=1)
        assert R.check_tail(tail, [], ctx, n_threads=7)[0] == ref
        R.check_tail(tail, ["-a"], ctx, flag=0x8)
        R.check_tail(tail, ["-5", "-T", "50"], ctx, flag=0x800 | 0x1000, T=50)
        assert R.check_tail_two_contexts(tail, ctx, ctx2, 1000)[0] == ref
        R.check_tail_refusals(tail, ctx)
    finally:
        ctx2.close()


def test_sam_pe_dev_constructed_case(gpu_ctx_factory, tmp_path):
    fa, r1, r2 = S.constructed_case(T, tmp_path)
    tail = S.PeTail(T, tmp_path, fa, r1, r2)
    ref, pes = R.check_tail(tail, [], gpu_ctx_factory(fa))
    print(len(ref.splitlines()), bm2.sam_rescue_apply_stats())


def test_sam_se_dev_rejects_the_bit_and_still_rejects_the_decide_bit(gpu_ctx_factory, tmp_path):
    fa, reads = T._case(tmp_path, 59, 8, L=100)
    ctx = gpu_ctx_factory(fa)
    for bit, word in ((bm2.SAM_F_DEVICE_RESCUE, "DEVICE_RESCUE"), (bm2.SAM_F_DEVICE_DECIDE, "DEVICE_DECIDE")):
        with pytest.raises(bm2.Bm2Error) as e:
            T._ours(fa, reads, ["q%d" % i for i in range(len(reads))], [b"F" * len(r) for r in reads], None, bm2.default_sam_opt(flag=bit), ctx=ctx)
        assert e.value.rc == bm2.BM2_EINVAL and word in str(e.value)


def test_fastq_to_sam_through_the_device_with_device_rescue(gpu_ctx_factory, tmp_path):
    # as tests/test_zzz_pe_decide_gpu.py: genome seed 81 with an ALT contig, device hits, batch_finish, then the PE tail with the bit(s)
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
    ctx2 = bm2.Context(0, share=ctx)
    try:
        with bm2.FastqChunk(open(f1, "rb").read(), open(f2, "rb").read()) as chunk:
            ctx.batch_upload_chunk(chunk)
            ctx.batch_run(opt)
            ctx.batch_finish(opt)
            aln, aln_off = ctx.batch_download_alnregs()
            off_text = ctx.sam(chunk, opt, bm2.default_sam_opt(), aln, aln_off).tobytes()
            planned, used, missed = bm2.sam_rescue_stats()
            assert ref == off_text, T._diff(ref, off_text)
            assert missed <= planned // 100, (planned, used, missed)
            Rb, Db, Tb = bm2.SAM_F_DEVICE_RESCUE, bm2.SAM_F_DEVICE_DECIDE, bm2.SAM_F_DEVICE_TEXT
            for bits in (Rb, Rb | Db, Rb | Db | Tb):
                on_text = ctx.sam(chunk, opt, bm2.default_sam_opt(flag=bits), aln, aln_off).tobytes()
                assert ref == on_text, T._diff(ref, on_text)
                pairs, n_tasks, added, redone = bm2.sam_rescue_apply_stats()
                assert pairs == 3000 and added > 0 and n_tasks == planned and redone <= missed, (pairs, n_tasks, added, redone, planned, missed)
            # the same through two contexts sharing the replica: every hook cuts the pairs into two parts
            for k in ("BM2_RESCUE_PART", "BM2_DECIDE_PART", "BM2_TEXT_PART"):
                os.environ[k] = "1000"
            try:
                for bits in (Rb, Rb | Db, Rb | Db | Tb):
                    on_text = ctx.sam(chunk, opt, bm2.default_sam_opt(flag=bits), aln, aln_off, also=[ctx2]).tobytes()
                    assert ref == on_text, T._diff(ref, on_text)
                    pairs, n_tasks, added, redone = bm2.sam_rescue_apply_stats()
                    assert pairs == 3000 and added > 0 and n_tasks == planned and redone <= missed, (pairs, n_tasks, added, redone, planned, missed)
            finally:
                for k in ("BM2_RESCUE_PART", "BM2_DECIDE_PART", "BM2_TEXT_PART"):
                    del os.environ[k]
    finally:
        ctx2.close()
