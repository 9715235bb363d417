"""SAM text formatted by the device kernels (samfmt.hip: k_sam_size, the scan, k_sam_write), executed on the host emulator (tools/emu): the
record-level entry point bm2_sam_format_dev on records made by hand, and the tail with BM2_SAM_F_DEVICE_TEXT against the flag-off tail and
the compiled reference.  Each test runs in a process of its own (bm2 binds one library).  The checks themselves are in sam_text_cases.py,
shared with the GPU tests."""
import os
import subprocess

import pytest

import bm2
import helpers  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = r'''
import sys, pathlib
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, bm2
bm2.LIB_PATH = %r
import sam_text_cases as S
import test_sam_tail as T
'''


def _child(emu_lib, body, timeout=1500):
    script = HEAD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "bwa-mem2_amd"), emu_lib) + body
    p = subprocess.run(["python", "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0 and p.stdout.startswith(b"ok"), (p.stdout.decode()[-500:], p.stderr.decode()[-3000:])
    return p.stdout


def test_records_made_by_hand_through_bm2_sam_format_dev(emu_lib, golden_dir):
    # every form of a line, names of every length (lines start at every residue modulo 16), a 40 kb read that crosses three LDS windows, the
    # cap rule with guard bytes, the counters: against a formatter written from the SAM field order (sam_text_cases.expected_line)
    _child(emu_lib, r'''
pre = %r + "/g60k.fa"
ctx = bm2.Context(0, pre)
print("ok", S.check_hand_made_records(ctx, pre))
''' % golden_dir)


def test_a_context_without_contig_names_is_refused(emu_lib):
    _child(emu_lib, r'''
ctx = bm2.Context(0, None)
try:
    ctx.sam_format(bm2.default_sam_opt(), np.zeros(4, np.uint8), np.zeros(1, np.int64), np.array([4], np.int32), ["r"], [bm2.SamRec()])
    raise SystemExit("accepted")
except bm2.Bm2Error as e:
    assert e.rc == bm2.BM2_EINVAL, e
print("ok")
''')


def test_se_tail_with_device_text_equals_host_text_and_reference(emu_lib, tmp_path):
    # T._case(59, 60 reads of 100 bp): the reference's text holds SA:Z:, XA:Z: and an unmapped line (asserted); flag combinations, comments,
    # a read group, 1 against 7 host threads.  After each call the counters describe the text.
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, reads = T._case(d, 59, 60, L=100)
rng = np.random.default_rng(3)
quals = [bytes(rng.integers(35, 74, size=len(r), dtype=np.uint8)) for r in reads]
names = ["q%%d" %% i for i in range(len(reads))]
fq = str(d / "r.fq")
T._write_fastq(fq, reads, quals)
ctx = bm2.Context(0, fa)
ref = T._reference_sam(fa, fq)
assert ref.count(b"SA:Z:") > 0 and ref.count(b"XA:Z:") > 0 and ref.count(b"\t4\t*\t0\t0\t*") > 0
out = [S.tail_se(T, fa, reads, names, quals, ref, ctx, n_threads=1), S.tail_se(T, fa, reads, names, quals, ref, ctx, n_threads=7)]
assert out[0] == out[1] and out[0][2] > 0, out                      # (the blobs: SA / XA)
for extra, flag, Tmin in ((["-a"], 0x8, 30), (["-Y", "-M"], 0x200 | 0x10, 30), (["-5", "-T", "50"], 0x800 | 0x1000, 50)):
    S.tail_se(T, fa, reads, names, quals, T._reference_sam(fa, fq, extra), ctx, flag=flag, Tmin=Tmin)
S.tail_se(T, fa, reads, names, quals, T._reference_sam(fa, fq, ["-R", r"@RG\tID:grp1\tSM:x"]), ctx, rg=b"grp1")
comments = ["BC:Z:ACGT%%d" %% i if i %% 3 else None for i in range(len(reads))]
with open(fq, "wb") as f:
    for i, r in enumerate(reads):
        f.write(b"@q%%d" %% i + (b" " + comments[i].encode() if comments[i] else b"") + b"\n" + bytes(b"ACGTN"[c] for c in r) + b"\n+\n" + quals[i] + b"\n")
S.tail_se(T, fa, reads, names, quals, T._reference_sam(fa, fq, ["-C"]), ctx, comments=comments)
print("ok", out)
''' % str(tmp_path))


def test_pe_tail_with_device_text_equals_host_text_and_reference(emu_lib, tmp_path):
    # the small PE case of test_rescue_kernel_and_sam_pe_dev_on_the_emulator; two contexts sharing the replica through the _multi form
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, r1, r2 = T._pe_case(d, 61, 40, L=100, sub_rate=0.02, indel_frac=0.2, random_frac=0.05)
ctx = bm2.Context(0, fa)
ref = S.tail_pe(T, d, fa, r1, r2, [], ctx, n_threads=1)
assert S.tail_pe(T, d, fa, r1, r2, [], ctx, n_threads=7) == ref
S.tail_pe(T, d, fa, r1, r2, ["-a"], ctx, flag=0x8)
S.tail_pe(T, d, fa, r1, r2, ["-Y", "-M"], ctx, flag=0x200 | 0x10)
S.tail_pe(T, d, fa, r1, r2, ["-5", "-T", "50"], ctx, flag=0x800 | 0x1000, T=50)
S.tail_pe(T, d, fa, r1, r2, ["-R", r"@RG\tID:grp1\tSM:x"], ctx, rg_id=b"grp1")
ctx2 = bm2.Context(0, share=ctx)
import os
os.environ["BM2_TEXT_PART"] = "16"                                   # (launch policy: records per context; small, so that both contexts format a part)
assert S.tail_pe(T, d, fa, r1, r2, [], [ctx, ctx2]) == ref
print("ok")
''' % str(tmp_path))


def test_host_only_entry_points_reject_the_bit(tmp_path):
    import test_sam_tail as T
    fa, reads = T._case(tmp_path, 59, 8, L=100)
    names = ["q%d" % i for i in range(len(reads))]
    quals = [b"F" * len(r) for r in reads]
    for paired in (False, True):
        with pytest.raises(bm2.Bm2Error) as e:
            if paired:
                T._pe_run(tmp_path, fa, reads[0::2], reads[1::2], [], flag=bm2.SAM_F_DEVICE_TEXT)
            else:
                T._ours(fa, reads, names, quals, None, bm2.default_sam_opt(flag=bm2.SAM_F_DEVICE_TEXT))
        assert e.value.rc == bm2.BM2_EINVAL and "DEVICE_TEXT" in str(e.value)
