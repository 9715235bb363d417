"""Mate-rescue results applied to the hit lists by the device kernels (rescue.hip: k_rescue_init, k_rescue_lane, the scan,
k_rescue_gather), executed on the host emulator (tools/emu): bm2_pe_rescue_apply_dev against bm2_pe_rescue_apply on lists made by hand
and at random with fabricated results, the host form on real tasks against the text of bm2_sam_pe's own flow, the refusals, and the tail
with BM2_SAM_F_DEVICE_RESCUE (alone, with the decide bit, with the decide and text bits, through one and two contexts) against the
flag-off tail and the compiled reference.  Each test runs in a process of its own (bm2 binds one library).  The checks themselves are in
pe_rescue_cases.py, shared with the GPU tests."""
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
import pe_rescue_cases as R
import test_sam_tail as T
'''


def _child(emu_lib, body, timeout=1500):
    script = HEAD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "bwa-mem2_amd"), emu_lib) + body
    p = subprocess.run(["python", "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0 and p.stdout.startswith(b"ok"), (p.stdout.decode()[-500:], p.stderr.decode()[-3000:])
    return p.stdout


def test_lists_made_by_hand_and_at_random_device_against_host(emu_lib, golden_dir):
    # lists of 0 .. 17 hits on either side, 48 + 48, 110 + 120 and 705 + 722 (the heaviest class); results below min_seed_len and with
    # qb < 0; every direction, both mirrorings; equal scores; rescued hits on top of input hits, above and below their scores; ties in
    # re and in (score, rb, qb); -m 3; every orientation failed in turn; ALT anchors; a first task left out of every seventh pair.
    # Every event is asserted to occur, from the host form's output.
    _child(emu_lib, r'''
pre = %r + "/g60k.fa"
ctx = bm2.Context(0, pre)
print("ok", R.check_lists(ctx, pre, quick=True))
''' % golden_dir)


def test_refusals_of_the_record_level_entry_points(emu_lib, golden_dir):
    _child(emu_lib, r'''
pre = %r + "/g60k.fa"
ctx = bm2.Context(0, pre)
print("ok", R.check_refusals(ctx, pre))
''' % golden_dir)


def test_host_form_on_real_tasks_prints_what_the_flow_prints(tmp_path):
    # no device involved: plan, bm2_ksw_align2, bm2_pe_rescue_apply, then the -S tail over the grown lists
    import pe_decide_cases as S
    import pe_rescue_cases as R
    import test_sam_tail as T
    fa, r1, r2 = T._pe_case(tmp_path, 61, 300, sub_rate=0.02, indel_frac=0.2, random_frac=0.03)
    tail = S.PeTail(T, tmp_path, fa, r1, r2)
    st = R.check_real_tasks(tail)[0]
    print(st)


def test_pe_tail_with_device_rescue_equals_host_text_and_reference(emu_lib, tmp_path):
    # the bit alone, with the decide bit, with the decide and text bits; one context, then two sharing the replica; the refusals of the tail
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, r1, r2 = T._pe_case(d, 61, 60, L=100, sub_rate=0.02, indel_frac=0.2, random_frac=0.05)
ctx = bm2.Context(0, fa)
ctx2 = bm2.Context(0, share=ctx)
tail = S.PeTail(T, d, fa, r1, r2)
ref, pes = R.check_tail(tail, [], ctx)
assert R.check_tail(tail, ["-a"], ctx, flag=0x8)[0] != ref
R.check_tail_two_contexts(tail, ctx, ctx2, 16)
R.check_tail_refusals(tail, ctx)
print("ok", len(ref.splitlines()), bm2.sam_rescue_apply_stats())
''' % str(tmp_path))


def test_pe_tail_constructed_case(emu_lib, tmp_path):
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, r1, r2 = S.constructed_case(T, d)
ctx = bm2.Context(0, fa)
tail = S.PeTail(T, d, fa, r1, r2)
ref, pes = R.check_tail(tail, [], ctx, combos=(bm2.SAM_F_DEVICE_RESCUE, bm2.SAM_F_DEVICE_RESCUE | bm2.SAM_F_DEVICE_DECIDE))
print("ok", len(ref.splitlines()), bm2.sam_rescue_apply_stats())
''' % str(tmp_path))


def test_host_only_and_single_end_entry_points_reject_the_bit(emu_lib, tmp_path):
    import test_sam_tail as T
    fa, reads = T._case(tmp_path, 59, 8, L=100)
    names = ["q%d" % i for i in range(len(reads))]
    quals = [b"F" * len(r) for r in reads]
    for paired in (False, True):
        with pytest.raises(bm2.Bm2Error) as e:
            if paired:
                T._pe_run(tmp_path, fa, reads[0::2], reads[1::2], [], flag=bm2.SAM_F_DEVICE_RESCUE)
            else:
                T._ours(fa, reads, names, quals, None, bm2.default_sam_opt(flag=bm2.SAM_F_DEVICE_RESCUE))
        assert e.value.rc == bm2.BM2_EINVAL and "DEVICE_RESCUE" in str(e.value)
    # the single-end tail WITH a context refuses it as well, and still refuses the decide bit
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, reads = T._case(d, 59, 8, L=100)
ctx = bm2.Context(0, fa)
for bit, word in ((bm2.SAM_F_DEVICE_RESCUE, "DEVICE_RESCUE"), (bm2.SAM_F_DEVICE_DECIDE, "DEVICE_DECIDE")):
    try:
        T._ours(fa, reads, ["q%%d" %% i for i in range(len(reads))], [b"F" * len(r) for r in reads], None, bm2.default_sam_opt(flag=bit), ctx=ctx)
        raise SystemExit("accepted")
    except bm2.Bm2Error as e:
        assert e.rc == bm2.BM2_EINVAL and word in str(e), e
print("ok")
''' % str(tmp_path))
