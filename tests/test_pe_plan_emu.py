"""Mate rescue planned by the device kernels (plan.hip: k_plan_count, the scan, k_plan_write, k_plan_queries), executed on the host
emulator (tools/emu): bm2_pe_rescue_plan_dev against bm2_pe_rescue_plan on lists made by hand and at random, BM2_ECAP, the refusals,
bm2_pe_rescue_queries in both forms against numpy, and the tail with BM2_SAM_F_DEVICE_PLAN (alone and with every subset of the three
other device bits, through one and two contexts) against the flag-off tail and the compiled reference.  Each test runs in a process of
its own (bm2 binds one library).  The checks themselves are in pe_plan_cases.py, shared with the GPU tests."""
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
import pe_plan_cases as P
import test_sam_tail as T
'''


def _child(emu_lib, body, timeout=1500):
    script = HEAD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "bwa-mem2_amd"), emu_lib) + body
    p = subprocess.run(["python", "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0 and p.stdout.startswith(b"ok"), (p.stdout.decode()[-500:], p.stderr.decode()[-3000:])
    return p.stdout


def test_plan_device_against_host_on_lists_made_by_hand_and_at_random(emu_lib, golden_dir):
    # either or both sides empty; read lengths 1, 30, 150, 251; -m 1, 3, 50; -U 0 and 17; min_seed_len 400; every orientation failed in
    # turn and all of them; windows below 0, beyond 2 l_pac, across contig ends on both strands and across the forward / reverse
    # junction; one heavy pair.  Every event of the issue's list is asserted to occur, from the rules written again in Python.
    _child(emu_lib, r'''
pre = %r + "/g60k.fa"
ctx = bm2.Context(0, pre)
print("ok", P.check_plan(ctx, pre, quick=True))
''' % golden_dir)


def test_plan_batch_sizes_at_block_and_scan_tile_edges(emu_lib, golden_dir):
    _child(emu_lib, r'''
pre = %r + "/g60k.fa"
ctx = bm2.Context(0, pre)
print("ok", P.check_sizes(ctx, pre))
''' % golden_dir)


def test_plan_ecap_and_refusals(emu_lib, golden_dir):
    _child(emu_lib, r'''
pre = %r + "/g60k.fa"
ctx = bm2.Context(0, pre)
print("ok", P.check_ecap(ctx, pre), P.check_refusals(ctx, pre))
''' % golden_dir)


def test_queries_device_and_host_against_numpy(emu_lib, golden_dir):
    _child(emu_lib, r'''
ctx = bm2.Context(0, %r + "/g60k.fa")
print("ok", P.check_queries(ctx))
''' % golden_dir)


def test_pe_tail_with_device_plan_equals_host_text_and_reference(emu_lib, tmp_path):
    # the bit alone and with the seven other subsets of {RESCUE, DECIDE, TEXT}; one context, then two sharing the replica; the refusals
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, r1, r2 = T._pe_case(d, 61, 60, L=100, sub_rate=0.02, indel_frac=0.2, random_frac=0.05)
ctx = bm2.Context(0, fa)
ctx2 = bm2.Context(0, share=ctx)
tail = S.PeTail(T, d, fa, r1, r2)
ref, pes = P.check_tail(tail, [], ctx, base_runs=False)
assert P.check_tail_two_contexts(tail, ctx, ctx2, 16, subsets=[0, P.RESCUE | P.DECIDE | P.TEXT], base_runs=False)[0] == ref
P.check_tail_refusals(tail, ctx)
print("ok", len(ref.splitlines()), bm2.sam_rescue_plan_stats())
''' % str(tmp_path))


def test_pe_tail_constructed_case(emu_lib, tmp_path):
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, r1, r2 = S.constructed_case(T, d)
ctx = bm2.Context(0, fa)
tail = S.PeTail(T, d, fa, r1, r2)
ref, pes = P.check_tail(tail, [], ctx, subsets=[P.RESCUE | P.DECIDE | P.TEXT], base_runs=False)
print("ok", len(ref.splitlines()), bm2.sam_rescue_plan_stats())
''' % str(tmp_path))


def test_host_only_and_single_end_entry_points_reject_the_bit(emu_lib, tmp_path):
    import test_sam_tail as T
    fa, reads = T._case(tmp_path, 59, 8, L=100)
    names = ["q%d" % i for i in range(len(reads))]
    quals = [b"F" * len(r) for r in reads]
    for paired in (False, True):
        with pytest.raises(bm2.Bm2Error) as e:
            if paired:
                T._pe_run(tmp_path, fa, reads[0::2], reads[1::2], [], flag=bm2.SAM_F_DEVICE_PLAN)
            else:
                T._ours(fa, reads, names, quals, None, bm2.default_sam_opt(flag=bm2.SAM_F_DEVICE_PLAN))
        assert e.value.rc == bm2.BM2_EINVAL and "DEVICE_PLAN" in str(e.value)
    # the single-end tail WITH a context refuses it as well, and the existing bits keep their refusals
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, reads = T._case(d, 59, 8, L=100)
ctx = bm2.Context(0, fa)
for bit, word in ((bm2.SAM_F_DEVICE_PLAN, "DEVICE_PLAN"), (bm2.SAM_F_DEVICE_RESCUE, "DEVICE_RESCUE"), (bm2.SAM_F_DEVICE_DECIDE, "DEVICE_DECIDE")):
    try:
        T._ours(fa, reads, ["q%%d" %% i for i in range(len(reads))], [b"F" * len(r) for r in reads], None, bm2.default_sam_opt(flag=bit), ctx=ctx)
        raise SystemExit("accepted")
    except bm2.Bm2Error as e:
        assert e.rc == bm2.BM2_EINVAL and word in str(e), e
print("ok")
''' % str(tmp_path))
