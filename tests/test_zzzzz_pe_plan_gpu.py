"""Mate rescue planned on the MI355X (plan.hip) -- sorted after the rescue file on purpose.
bm2_pe_rescue_plan_dev against bm2_pe_rescue_plan on lists made by hand and at random, BM2_ECAP, the refusals, bm2_pe_rescue_queries in
both forms against numpy, and bm2_sam_pe_dev / the _multi form with BM2_SAM_F_DEVICE_PLAN (alone and with every subset of
BM2_SAM_F_DEVICE_RESCUE, _DECIDE and _TEXT) against the flag-off text and `bwa-mem2 mem`'s.  All comparisons are exact.  The checks
themselves are in pe_plan_cases.py, shared with the emulator tests."""
import os
import subprocess

import numpy as np
import pytest

import bm2
import helpers
import pe_decide_cases as S
import pe_plan_cases as P
import test_sam_tail as T
from helpers import ref_binary
from tools import synth

pytestmark = pytest.mark.gpu


def test_plan_device_against_host_on_lists_made_by_hand_and_at_random(gpu_ctx_factory, golden_dir):
    pre = os.path.join(golden_dir, "g60k.fa")
    total = P.check_plan(gpu_ctx_factory(pre), pre)
    print(total)


def test_plan_batch_sizes_at_block_and_scan_tile_edges(gpu_ctx_factory, golden_dir):
    pre = os.path.join(golden_dir, "g60k.fa")
    print(P.check_sizes(gpu_ctx_factory(pre), pre))


def test_plan_ecap(gpu_ctx_factory, golden_dir):
    pre = os.path.join(golden_dir, "g60k.fa")
    assert P.check_ecap(gpu_ctx_factory(pre), pre) > 0


def test_plan_refusals(gpu_ctx_factory, golden_dir):
    pre = os.path.join(golden_dir, "g60k.fa")
    assert P.check_refusals(gpu_ctx_factory(pre), pre)


def test_queries_device_and_host_against_numpy(gpu_ctx_factory, golden_dir):
    assert P.check_queries(gpu_ctx_factory(os.path.join(golden_dir, "g60k.fa"))) > 0


def test_sam_pe_dev_with_device_plan(gpu_ctx_factory, tmp_path):
    fa, r1, r2 = T._pe_case(tmp_path, 61, 3000, sub_rate=0.02, indel_frac=0.2, random_frac=0.03)
    ctx = gpu_ctx_factory(fa)
    ctx2 = bm2.Context(0, share=ctx)
    try:
        tail = S.PeTail(T, tmp_path, fa, r1, r2)
        ref, pes = P.check_tail(tail, [], ctx)
        assert P.check_tail(tail, [], ctx, subsets=[0], n_threads=1)[0] == ref
        P.check_tail(tail, ["-a"], ctx, flag=0x8, subsets=[0, P.RESCUE])
        assert P.check_tail_two_contexts(tail, ctx, ctx2, 1000, subsets=[0, P.RESCUE, P.RESCUE | P.DECIDE | P.TEXT])[0] == ref
        P.check_tail_refusals(tail, ctx)
    finally:
        ctx2.close()


def test_sam_pe_dev_constructed_case(gpu_ctx_factory, tmp_path):
    fa, r1, r2 = S.constructed_case(T, tmp_path)
    tail = S.PeTail(T, tmp_path, fa, r1, r2)
    ref, pes = P.check_tail(tail, [], gpu_ctx_factory(fa))
    print(len(ref.splitlines()), bm2.sam_rescue_plan_stats())


def test_sam_se_dev_rejects_the_bit(gpu_ctx_factory, tmp_path):
    fa, reads = T._case(tmp_path, 59, 8, L=100)
    ctx = gpu_ctx_factory(fa)
    with pytest.raises(bm2.Bm2Error) as e:
        T._ours(fa, reads, ["q%d" % i for i in range(len(reads))], [b"F" * len(r) for r in reads], None, bm2.default_sam_opt(flag=bm2.SAM_F_DEVICE_PLAN), ctx=ctx)
    assert e.value.rc == bm2.BM2_EINVAL and "DEVICE_PLAN" in str(e.value)


def test_fastq_to_sam_through_the_device_with_device_plan(gpu_ctx_factory, tmp_path):
    # as tests/test_zzzz_pe_rescue_gpu.py: genome seed 81 with an ALT contig, device hits, batch_finish, then the PE tail with the bit(s)
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
            st_off = bm2.sam_rescue_stats()
            assert ref == off_text, T._diff(ref, off_text)
            for bits in P.SUBSETS:
                on_text = ctx.sam(chunk, opt, bm2.default_sam_opt(flag=bits | P.PLAN), aln, aln_off).tobytes()
                assert ref == on_text, T._diff(ref, on_text)
                pairs, n_tasks, q_bytes = bm2.sam_rescue_plan_stats()
                assert pairs == 3000 and n_tasks == st_off[0] == bm2.sam_rescue_stats()[0] and q_bytes >= n_tasks > 0, (pairs, n_tasks, q_bytes, st_off)
                if not bits & P.RESCUE:
                    assert bm2.sam_rescue_stats() == st_off, (bits, bm2.sam_rescue_stats(), st_off)
            # the same through two contexts sharing the replica: the plan hook cuts the pairs, the rescue batch its tasks, into two parts
            for k in P.PART_KNOBS:
                os.environ[k] = "1000"
            try:
                for bits in (0, P.RESCUE, P.RESCUE | P.DECIDE | P.TEXT):
                    on_text = ctx.sam(chunk, opt, bm2.default_sam_opt(flag=bits | P.PLAN), aln, aln_off, also=[ctx2]).tobytes()
                    assert ref == on_text, T._diff(ref, on_text)
                    assert bm2.sam_rescue_plan_stats()[:2] == (3000, st_off[0])
            finally:
                for k in P.PART_KNOBS:
                    del os.environ[k]
    finally:
        ctx2.close()
