"""SAM text formatted on the MI355X (samfmt.hip: k_sam_size, the scan, k_sam_write) -- sorted after the tail-kernel file on purpose.
bm2_sam_format_dev on records made by hand, and bm2_sam_se_dev / bm2_sam_pe_dev / the _multi form with BM2_SAM_F_DEVICE_TEXT against the
flag-off text and `bwa-mem2 mem`'s.  The cap that keeps the blob from hiding the kernel: in every case that runs with default options the
pre-formatted bytes (SA:Z:, XA:Z:, pa:f:, XR:Z:) are at most 10 % of the text -- counted from the reference's own output, 3.6 % for the SE
case (seed 41) and 1.7 % for the PE case of seed 53; it is a condition on the inputs, not a measurement.  The checks themselves are in
sam_text_cases.py, shared with the emulator tests."""
import os
import subprocess

import numpy as np
import pytest

import bm2
import helpers
import sam_text_cases as S
import test_sam_tail as T
from helpers import ONT2D, ref_binary
from tools import synth

pytestmark = pytest.mark.gpu
BLOB_CAP = 0.10


def test_records_made_by_hand_through_bm2_sam_format_dev(gpu_ctx_factory, golden_dir):
    pre = os.path.join(golden_dir, "g60k.fa")
    n_cases, n_bytes = S.check_hand_made_records(gpu_ctx_factory(pre), pre)
    assert n_cases > 50 and n_bytes > 3 * 40000


def test_sam_se_dev_with_device_text(gpu_ctx_factory, tmp_path):
    # the 4000-read case of test_sam_se_with_the_cigar_alignments_on_the_device, random qualities; then -a, -Y -M, -T 50 -5
    fa, reads = T._case(tmp_path, 41, 4000)
    rng = np.random.default_rng(3)
    quals = [bytes(rng.integers(35, 74, size=len(r), dtype=np.uint8)) for r in reads]
    fq = str(tmp_path / "r.fq")
    T._write_fastq(fq, reads, quals)
    names = ["q%d" % i for i in range(len(reads))]
    ctx = gpu_ctx_factory(fa)
    n_rec, dev, host = S.tail_se(T, fa, reads, names, quals, T._reference_sam(fa, fq), ctx, blob_cap=BLOB_CAP)
    assert n_rec >= 4000 and host > 0
    for extra, flag, Tmin in ((["-a"], 0x8, 30), (["-Y", "-M"], 0x200 | 0x10, 30), (["-T", "50", "-5"], 0x800 | 0x1000, 50)):
        S.tail_se(T, fa, reads, names, quals, T._reference_sam(fa, fq, extra), ctx, flag=flag, Tmin=Tmin)


def test_sam_se_dev_with_device_text_non_default_scoring(gpu_ctx_factory, tmp_path):
    # the scoring of test_sam_se_options
    fa, reads = T._case(tmp_path, 43, 1500, L=120)
    quals = [b"F" * len(r) for r in reads]
    fq = str(tmp_path / "r.fq")
    T._write_fastq(fq, reads, quals)
    names = ["q%d" % i for i in range(len(reads))]
    ref = T._reference_sam(fa, fq, ["-B", "3", "-O", "5,7", "-E", "2,1", "-L", "4,6"])
    S.tail_se(T, fa, reads, names, quals, ref, gpu_ctx_factory(fa), okw=dict(b=3, o_del=5, o_ins=7, e_del=2, e_ins=1, pen_clip5=4, pen_clip3=6))


def test_sam_se_dev_with_device_text_and_comments(gpu_ctx_factory, tmp_path):
    # -C: the comment joins the pre-formatted bytes, so the 10 % cap is left out for this one case
    fa, reads = T._case(tmp_path, 45, 1000)
    quals = [b"F" * len(r) for r in reads]
    names = ["q%d" % i for i in range(len(reads))]
    comments = ["BC:Z:ACGT%d" % i if i % 3 else None for i in range(len(reads))]
    fq = str(tmp_path / "r.fq")
    with open(fq, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@q%d" % i + (b" " + comments[i].encode() if comments[i] else b"") + b"\n" + bytes(b"ACGTN"[c] for c in r) + b"\n+\n" + quals[i] + b"\n")
    S.tail_se(T, fa, reads, names, quals, T._reference_sam(fa, fq, ["-C"]), gpu_ctx_factory(fa), comments=comments)


def test_sam_pe_dev_with_device_text(gpu_ctx_factory, tmp_path):
    fa, r1, r2 = T._pe_case(tmp_path, 61, 3000, sub_rate=0.02, indel_frac=0.2, random_frac=0.03)
    ctx = gpu_ctx_factory(fa)
    ref = S.tail_pe(T, tmp_path, fa, r1, r2, [], ctx, blob_cap=BLOB_CAP)
    assert bm2.sam_text_stats()[0] >= 6000
    # two contexts sharing the replica, each formatting a part of the records: the same text as one
    ctx2 = bm2.Context(0, share=ctx)
    os.environ["BM2_TEXT_PART"] = "1000"                         # (launch policy: records per context)
    try:
        assert S.tail_pe(T, tmp_path, fa, r1, r2, [], [ctx, ctx2], blob_cap=BLOB_CAP) == ref
    finally:
        del os.environ["BM2_TEXT_PART"]
        ctx2.close()


def test_long_reads_with_device_text(gpu_ctx_factory, tmp_path):
    # the -x ont2d case of test_sam_se_long_reads_ont2d: reads up to 6 kb, lines that fill most of a window
    if ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")
    names, ctg, alts = synth.make_genome(47, [180000, 90000], alt_contigs=0, n_repeat_families=3, repeat_len=(300, 2000), copies=(3, 8),
                                         divergence=(0.0, 0.05))
    fa = str(tmp_path / "g.fa")
    synth.write_fasta(fa, names, ctg)
    subprocess.check_call([ref_binary(), "index", fa], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    reads = synth.make_reads_long(48, ctg, 60, mean_len=2500, max_len=6000, err=0.08)
    quals = [b"5" * len(r) for r in reads]
    fq = str(tmp_path / "r.fq")
    T._write_fastq(fq, reads, quals)
    ref = T._reference_sam(fa, fq, ["-x", "ont2d"])
    S.tail_se(T, fa, reads, ["q%d" % i for i in range(len(reads))], quals, ref, gpu_ctx_factory(fa), okw=ONT2D, Tmin=ONT2D.get("T", 30))


def test_fastq_to_sam_through_the_device_with_device_text(gpu_ctx_factory, tmp_path):
    # as tests/test_end_to_end_gpu.py: device hits, batch_finish, then the PE tail with the bit
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
        on_text = ctx.sam(chunk, opt, bm2.default_sam_opt(flag=bm2.SAM_F_DEVICE_TEXT), aln, aln_off).tobytes()
    assert ref == off_text, T._diff(ref, off_text)
    assert ref == on_text, T._diff(ref, on_text)
    S.check_text_stats(on_text, BLOB_CAP)
