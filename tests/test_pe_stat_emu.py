"""The chunk's insert-size model counted by the device kernels (pestat.hip: k_pestat, k_pestat_reduce), executed on the host emulator
(tools/emu): bm2_pe_stat_dev against bm2_pe_stat on lists made by hand and at random, the thresholds of the model, one bin under 70 000
adds with one and with several copies of the histogram, batch sizes at block edges, capacity and refusals, and the tail with
BM2_SAM_F_DEVICE_PESTAT (alone and with the plan bit and its companions, through one and two contexts) against the flag-off tail and the
compiled reference, with the hits uploaded once for the model and the plan.  Each test runs in a process of its own (bm2 binds one
library).  The checks themselves are in pe_stat_cases.py, shared with the GPU tests."""
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
import pe_decide_cases as S
import pe_stat_cases as P
import test_sam_tail as T
'''


def _child(emu_lib, body, timeout=1500):
    script = HEAD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "bwa-mem2_amd"), emu_lib) + body
    p = subprocess.run(["python", "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0 and p.stdout.startswith(b"ok"), (p.stdout.decode()[-500:], p.stderr.decode()[-3000:])
    return p.stdout


def test_stat_device_against_host_on_lists_made_by_hand_and_at_random(emu_lib, golden_dir):
    # empty ends; the 0.8 * score boundary of the default sub-score and of every score 5 .. 250; the first overlap at j = 1, last, absent;
    # overlaps at min_l * mask_level and one base less at 0.5 and 0.3; 500 hits an end; contigs, directions, strands, distances 0,
    # max_ins, max_ins + 1; max_ins 1 .. 70000 and <= 0; offsets that do not start at 0.  Every event is asserted to occur.
    _child(emu_lib, r'''
pre = %r + "/g60k.fa"
ctx = bm2.Context(0, pre)
print("ok", P.check_lists(ctx, pre, quick=True))
''' % golden_dir)


def test_stat_model_thresholds(emu_lib, golden_dir):
    _child(emu_lib, r'''
pre = %r + "/g60k.fa"
ctx = bm2.Context(0, pre)
print("ok", P.check_thresholds(ctx, pre))
''' % golden_dir)


def test_stat_one_bin_under_contention_with_one_copy_and_with_several(emu_lib, golden_dir):
    _child(emu_lib, r'''
pre = %r + "/g60k.fa"
ctx = bm2.Context(0, pre)
print("ok", P.check_contention(ctx, pre))
''' % golden_dir)


def test_stat_batch_sizes_at_block_edges(emu_lib, golden_dir):
    _child(emu_lib, r'''
pre = %r + "/g60k.fa"
ctx = bm2.Context(0, pre)
print("ok", P.check_sizes(ctx, pre))
''' % golden_dir)


def test_stat_capacity_and_refusals(emu_lib, golden_dir):
    _child(emu_lib, r'''
pre = %r + "/g60k.fa"
ctx = bm2.Context(0, pre)
print("ok", P.check_capacity_and_refusals(ctx, pre))
''' % golden_dir)


def test_pe_tail_with_device_pestat_equals_host_text_and_reference(emu_lib, tmp_path):
    # the bit alone and with PLAN, PLAN | RESCUE, PLAN | RESCUE | DECIDE | TEXT; one context, then two sharing the replica; a model that
    # is given; no rescue and inline rescue; the shared upload's counters
    if helpers.ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, r1, r2 = T._pe_case(d, 61, 60, L=100, sub_rate=0.02, indel_frac=0.2, random_frac=0.05)
ctx = bm2.Context(0, fa)
ctx2 = bm2.Context(0, share=ctx)
tail = S.PeTail(T, d, fa, r1, r2)
ref, pes = P.check_tail(tail, [], ctx)
assert P.check_tail_two_contexts(tail, ctx, ctx2, 16)[0] == ref
P.check_tail_given_model(tail, ctx)
P.check_tail_no_rescue(tail, ctx)
P.check_tail_refusals(tail)
print("ok", len(ref.splitlines()), bm2.sam_pestat_stats())
''' % str(tmp_path))


def test_pe_tail_constructed_case(emu_lib, tmp_path):
    if helpers.ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, r1, r2 = S.constructed_case(T, d)
ctx = bm2.Context(0, fa)
tail = S.PeTail(T, d, fa, r1, r2)
ref, pes = P.check_tail(tail, [], ctx, combos=[0, P.PLAN | P.RESCUE | P.DECIDE | P.TEXT])
print("ok", len(ref.splitlines()), bm2.sam_pestat_stats())
''' % str(tmp_path))


def test_host_only_and_single_end_entry_points_reject_the_bit(emu_lib, tmp_path):
    import test_sam_tail as T
    if helpers.ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")
    fa, reads = T._case(tmp_path, 59, 8, L=100)
    names = ["q%d" % i for i in range(len(reads))]
    quals = [b"F" * len(r) for r in reads]
    for paired in (False, True):
        with pytest.raises(bm2.Bm2Error) as e:
            if paired:
                T._pe_run(tmp_path, fa, reads[0::2], reads[1::2], [], flag=bm2.SAM_F_DEVICE_PESTAT)
            else:
                T._ours(fa, reads, names, quals, None, bm2.default_sam_opt(flag=bm2.SAM_F_DEVICE_PESTAT))
        assert e.value.rc == bm2.BM2_EINVAL and "DEVICE_PESTAT" in str(e.value)
    # the single-end tail WITH a context refuses it as well
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, reads = T._case(d, 59, 8, L=100)
ctx = bm2.Context(0, fa)
try:
    T._ours(fa, reads, ["q%%d" %% i for i in range(len(reads))], [b"F" * len(r) for r in reads], None, bm2.default_sam_opt(flag=bm2.SAM_F_DEVICE_PESTAT), ctx=ctx)
    raise SystemExit("accepted")
except bm2.Bm2Error as e:
    assert e.rc == bm2.BM2_EINVAL and "DEVICE_PESTAT" in str(e), e
print("ok")
''' % str(tmp_path))
