"""The pairing decisions of mem_sam_pe made by the device kernels (decide.hip: k_decide_class, the scans, k_decide_list, k_decide_light,
k_decide_heavy), executed on the host emulator (tools/emu): the record-level entry point bm2_pe_decide_dev against bm2_pe_decide on lists
made by hand and at random, the arithmetic sweep, the refusals, and the tail with BM2_SAM_F_DEVICE_DECIDE against the flag-off tail and the
compiled reference.  Each test runs in a process of its own (bm2 binds one library).  The checks themselves are in pe_decide_cases.py,
shared with the GPU tests.

The sweep here is a fixed subsample of the GPU's: every 12th pair of the same two seeded sequences of 60 000, i.e. 2 x 5 000 pairs.
Measured on the build host with nothing beside it: the sweep 13 s, the whole file 4 min 42 s (50 s of it the session's emulator build,
120 s the constructed tail case while it also ran with both bits; that variant has since been left to the GPU file, which is about 30 s
less here)."""
import os
import subprocess

import pytest

import bm2
import helpers  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_PAIRS, SWEEP_STRIDE = 60000, 12

HEAD = r'''
import sys, pathlib
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, bm2
bm2.LIB_PATH = %r
import pe_decide_cases as S
import test_sam_tail as T
'''


def _child(emu_lib, body, timeout=1500):
    script = HEAD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "bwa-mem2_amd"), emu_lib) + body
    p = subprocess.run(["python", "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0 and p.stdout.startswith(b"ok"), (p.stdout.decode()[-500:], p.stderr.decode()[-3000:])
    return p.stdout


def test_lists_made_by_hand_and_at_random_device_against_host(emu_lib, golden_dir):
    # lists of 0 .. 17 hits on either side, 48 + 48 (the wavefront form's LDS), 49 + 48 (its workspace), 705 + 722; equal scores; ALT hits;
    # -5; no pairing; every orientation failed, alone, all; a model whose table holds -inf; ids at 2^23 - 1 and above 2^31; scoring options;
    # the log(seedcov) branch.  Every outcome is asserted to occur, from the host form's results; both kernels must have decided pairs.
    _child(emu_lib, r'''
pre = %r + "/g60k.fa"
ctx = bm2.Context(0, pre)
print("ok", S.check_lists(ctx, pre, quick=True))
''' % golden_dir)


def test_arithmetic_sweep_device_against_host(emu_lib, golden_dir):
    _child(emu_lib, r'''
pre = %r + "/g60k.fa"
ctx = bm2.Context(0, pre)
done, total = S.check_sweep(ctx, pre, %d, %d)
assert done == 2 * %d, done
print("ok", done, total)
''' % (golden_dir, SWEEP_PAIRS, SWEEP_STRIDE, SWEEP_PAIRS // SWEEP_STRIDE))


def test_refusals_of_the_record_level_entry_points(emu_lib, golden_dir):
    _child(emu_lib, r'''
pre = %r + "/g60k.fa"
ctx = bm2.Context(0, pre)
print("ok", S.check_refusals(ctx, pre))
''' % golden_dir)


def test_pe_tail_with_device_decide_equals_host_text_and_reference(emu_lib, tmp_path):
    # the small PE case of the text tests under every option set of the issue; two contexts sharing the replica through the _multi form
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, r1, r2 = T._pe_case(d, 61, 40, L=100, sub_rate=0.02, indel_frac=0.2, random_frac=0.05)
ctx = bm2.Context(0, fa)
ctx2 = bm2.Context(0, share=ctx)
tail = S.PeTail(T, d, fa, r1, r2)
tail.option_sets(ctx, ctx2, part_knob=16)
print("ok")
''' % str(tmp_path))


def test_pe_tail_constructed_case_reaches_the_rare_branches(emu_lib, tmp_path):
    # 440 pairs: 20 paired without exceeding the unpaired score, 20 that leave by a second primary hit; counted from the host form's plans
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, r1, r2 = S.constructed_case(T, d)
ctx = bm2.Context(0, fa)
tail = S.PeTail(T, d, fa, r1, r2)
ref, pes = tail.check([], ctx)
tail.check(["-S"], ctx, flag=0x20)
seen = tail.host_outcomes(pes)
assert seen["paired_below"] > 0 and seen["second_primary"] > 0 and seen["paired_above"] > 0 and seen["empty"] > 0, seen
print("ok", seen, len(ref.splitlines()))
''' % str(tmp_path))


def test_host_only_and_single_end_entry_points_reject_the_bit(emu_lib, tmp_path):
    import test_sam_tail as T
    fa, reads = T._case(tmp_path, 59, 8, L=100)
    names = ["q%d" % i for i in range(len(reads))]
    quals = [b"F" * len(r) for r in reads]
    for paired in (False, True):
        with pytest.raises(bm2.Bm2Error) as e:
            if paired:
                T._pe_run(tmp_path, fa, reads[0::2], reads[1::2], [], flag=bm2.SAM_F_DEVICE_DECIDE)
            else:
                T._ours(fa, reads, names, quals, None, bm2.default_sam_opt(flag=bm2.SAM_F_DEVICE_DECIDE))
        assert e.value.rc == bm2.BM2_EINVAL and "DEVICE_DECIDE" in str(e.value)
    # the single-end tail WITH a context refuses it as well
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, reads = T._case(d, 59, 8, L=100)
ctx = bm2.Context(0, fa)
try:
    T._ours(fa, reads, ["q%%d" %% i for i in range(len(reads))], [b"F" * len(r) for r in reads], None, bm2.default_sam_opt(flag=bm2.SAM_F_DEVICE_DECIDE), ctx=ctx)
    raise SystemExit("accepted")
except bm2.Bm2Error as e:
    assert e.rc == bm2.BM2_EINVAL and "DEVICE_DECIDE" in str(e), e
print("ok")
''' % str(tmp_path))
