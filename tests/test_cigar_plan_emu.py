"""Which hits the SAM text asks a CIGAR for, picked by the device kernels (cgplan.hip: k_cg_light, k_cg_heavy, k_cg_count, k_cg_write),
executed on the host emulator (tools/emu): bm2_cigar_plan_dev against bm2_cigar_plan on lists made by hand and at random in the
single-end and the paired form, list and batch sizes at the kernels' edges, capacity and refusals, and the tails with
BM2_SAM_F_DEVICE_CGPLAN (alone and with the other device bits, through one and two contexts) against the flag-off tails and the compiled
reference.  Each test runs in a process of its own (bm2 binds one library).  The checks themselves are in cigar_plan_cases.py, shared
with the GPU tests.  The last test runs the existing tail cases of the HOST library with BM2_CGPLAN_CHECK=1: the dry emit pass and
bm2_cigar_plan must name the same hits."""
import os
import subprocess

import bm2
import helpers  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = r'''
import sys, pathlib
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, bm2
bm2.LIB_PATH = %r
import pe_decide_cases as S
import cigar_plan_cases as P
import test_sam_tail as T
'''


def _child(lib, body, timeout=1500, env=None):
    script = HEAD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "bwa-mem2_amd"), lib) + body
    p = subprocess.run(["python", "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
    assert p.returncode == 0 and p.stdout.startswith(b"ok"), (p.stdout.decode()[-500:], p.stderr.decode()[-3000:])
    return p


def test_plan_device_against_host_on_lists_made_by_hand_and_at_random(emu_lib, golden_dir):
    # list lengths 0 .. 500 around the row form's 16 hits and the LDS capacity; T - 1 / T; secondary in {-2, -1, an index, INT_MAX}; the
    # drop_ratio boundary in float and the XA boundary in double for primary scores 5 .. 250; cnt[r] at max_XA_hits and max_XA_hits_alt
    # and one more, with and without an ALT hit; MEM_F_ALL; paired 0 and 1; the ALT hit at n_pri; the fallback of the mate's
    # representative; a hit two rules ask for; offsets that do not start at 0.  Every event is asserted to occur.
    _child(emu_lib, r'''
ctx = bm2.Context(0, %r + "/g60k.fa")
tot = P.check_lists(ctx, quick=True)
print("ok", len(tot))
''' % golden_dir)


def test_plan_batch_sizes_at_block_edges(emu_lib, golden_dir):
    _child(emu_lib, r'''
ctx = bm2.Context(0, %r + "/g60k.fa")
print("ok", P.check_sizes(ctx))
''' % golden_dir)


def test_plan_capacity_and_refusals(emu_lib, golden_dir):
    _child(emu_lib, r'''
ctx = bm2.Context(0, %r + "/g60k.fa")
print("ok", P.check_capacity_and_refusals(ctx))
''' % golden_dir)


def test_pe_tail_with_device_cgplan_equals_host_text_and_reference(emu_lib, tmp_path):
    # the bit alone, with DECIDE, with PLAN | RESCUE | DECIDE, with all six; one context, then two sharing the replica; -S, -a, -5;
    # planned / used / missed as without the bit
    if helpers.ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, r1, r2 = T._pe_case(d, 61, 60, L=100, sub_rate=0.02, indel_frac=0.2, random_frac=0.05)
ctx = bm2.Context(0, fa)
ctx2 = bm2.Context(0, share=ctx)
tail = S.PeTail(T, d, fa, r1, r2)
ref = P.check_tail(tail, ctx)
assert P.check_tail_two_contexts(tail, ctx, ctx2, 16) == ref
P.check_tail_options(tail, ctx)
P.check_tail_refusals(tail)
print("ok", len(ref.splitlines()), bm2.sam_cigar_plan_stats())
''' % str(tmp_path))


def test_pe_tail_constructed_case(emu_lib, tmp_path):
    if helpers.ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, r1, r2 = S.constructed_case(T, d)
ctx = bm2.Context(0, fa)
tail = S.PeTail(T, d, fa, r1, r2)
ref = P.check_tail(tail, ctx, combos=[0, P.PESTAT | P.PLAN | P.RESCUE | P.DECIDE | P.TEXT])
print("ok", len(ref.splitlines()), bm2.sam_cigar_plan_stats())
''' % str(tmp_path))


def test_se_tail_with_device_cgplan_and_host_only_refusal(emu_lib, tmp_path):
    if helpers.ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")
    _child(emu_lib, r'''
d = pathlib.Path(%r)
made = []
def make(fa):
    made.append(bm2.Context(0, fa))
    return made[-1]
print("ok", P.check_se_tail(T, d, make, n_reads=120))
''' % str(tmp_path))


def test_dry_pass_of_the_host_tails_agrees_with_the_rule(tmp_path):
    # BM2_CGPLAN_CHECK=1 on the existing SE and PE tail cases (CIGARs as a session: BM2_CIGAR_FLAT=1), against the HOST library: the
    # flag-off tails compare what their dry pass recorded with bm2_cigar_plan and fail the call on a difference
    if helpers.ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")
    env = dict(os.environ, BM2_CGPLAN_CHECK="1", BM2_CIGAR_FLAT="1", BM2_TAIL_PROF="1")
    p = _child(bm2.LIB_PATH, r'''
d = pathlib.Path(%r)
(d / "se").mkdir(); (d / "pe").mkdir(); (d / "c").mkdir()
fa, reads = T._case(d / "se", 41, 1500)
names, quals = ["q%%d" %% i for i in range(len(reads))], [b"F" * len(r) for r in reads]
fq = str(d / "se" / "r.fq")
T._write_fastq(fq, reads, quals)
for extra, flag, Tmin in (([], 0, 30), (["-a"], 0x8, 30), (["-T", "50", "-5"], 0x800 | 0x1000, 50)):
    ref = T._reference_sam(fa, fq, extra)
    got = T._ours(fa, reads, names, quals, None, bm2.default_sam_opt(flag=flag, T=Tmin))
    assert ref == got, T._diff(ref, got)
    assert bm2.sam_cigar_stats()[0] > 1000
fa, r1, r2 = T._pe_case(d / "pe", 61, 1500, sub_rate=0.02, indel_frac=0.2, random_frac=0.03)
for extra, flag in (([], 0), (["-S"], 0x20), (["-a"], 0x8), (["-5"], 0x800 | 0x1000)):
    ref, got, pes = T._pe_run(d / "pe", fa, r1, r2, extra, flag=flag)
    assert ref == got, T._diff(ref, got)
    assert bm2.sam_cigar_stats()[0] > 1000
fa, r1, r2 = S.constructed_case(T, d / "c")
ref, got, pes = T._pe_run(d / "c", fa, r1, r2, [])
assert ref == got, T._diff(ref, got)
print("ok")
''' % str(tmp_path), env=env)
    assert p.stderr.count(b"cgplan check:") == 8, p.stderr.decode()[-2000:]      # (every call ran the comparison)
