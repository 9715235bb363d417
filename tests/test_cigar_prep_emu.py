"""The CIGAR batch prepared by the device kernels (cgprep.hip: k_cgp_size, k_cgp_task, k_cgp_hist, k_cgp_scatter, with scan.hip's prefix
sums between them), executed on the host emulator (tools/emu): bm2_cigar_prep_dev against bm2_cigar_prep on tasks made by hand and at
random, batch sizes at the kernels' edges, arguments and refusals, the three launch knobs, and the SAM tails with
BM2_SAM_F_DEVICE_CGPREP against the flag-off tail and the compiled reference.  Each test runs in a process of its own (bm2 binds one
library; the knobs are read once per process).  The checks themselves are in cigar_prep_cases.py, shared with the GPU tests; the
emulator runs their `quick` sizes -- the batch of 70 000 tasks, whose block counts take more than one block of the scan, is left to the
GPU."""
import os
import re
import subprocess

import pytest

import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = r'''
import sys, pathlib
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, bm2
bm2.LIB_PATH = %r
import cigar_prep_cases as P
import se_mark_cases as M
import pe_decide_cases as S
import test_sam_tail as T
'''


def _child(lib, body, timeout=1500, env=None):
    script = HEAD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "bwa-mem2_amd"), lib) + body
    p = subprocess.run(["python", "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
    assert p.returncode == 0 and p.stdout.startswith(b"ok"), (p.stdout.decode()[-500:], p.stderr.decode()[-3000:])
    return p


def test_cigar_prep_device_against_host_on_tasks_made_by_hand_and_at_random(emu_lib):
    # all four shapes; the NULL returns filed under FLAT (rb >= re, q_len == 0, a range bridging l_pac, rb < 0, re > 2 l_pac); retry 0 and
    # 1; the flat case and its neighbour one base longer; the ring's edge at a first band of 31 | 32; `small` at q_len 220 | 221 and at
    # (q_len + rlen) * pen one below and at CG_SMALL; first bands 0, 1, 31 and above; DP areas on both sides of a power of two; w_first
    # below, at and above opt->w << 2; gap penalties under which the two divisions differ; read offsets that do not start at 0.  Every
    # event is asserted to occur; the host form is also held against properties that do not depend on it.
    _child(emu_lib, r'''
ctx = bm2.Context(0, None)
tot = P.check_tasks(ctx, quick=True)
print("ok", len(tot))
''')


def test_cigar_prep_batch_sizes_at_block_edges(emu_lib):
    _child(emu_lib, r'''
ctx = bm2.Context(0, None)
print("ok", P.check_batches(ctx, quick=True))
''')


def test_cigar_prep_arguments_and_refusals(emu_lib):
    _child(emu_lib, r'''
ctx = bm2.Context(0, None)
print("ok", P.check_arguments(ctx))
''')


@pytest.mark.parametrize("knob,value", [("BM2_CIGAR_NO_LDS", "1"), ("BM2_CIGAR_NO_RING", "1"), ("BM2_CIGAR_RING_BY_BAND", "0")])
def test_cigar_prep_follows_the_launch_knob(emu_lib, knob, value):
    _child(emu_lib, r'''
ctx = bm2.Context(0, None)
print("ok", P.check_knob(ctx, %r))
''' % knob, env=dict(os.environ, **{knob: value}))


def test_se_tail_with_device_cgprep_equals_host_text_and_reference(emu_lib, tmp_path):
    if helpers.ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")
    _child(emu_lib, r'''
d = pathlib.Path(%r)
made = []
def make(fa):
    made.append(bm2.Context(0, fa))
    return made[-1]
print("ok", P.check_se_tail(T, M, d, make, n_reads=120))
''' % str(tmp_path))


def test_pe_tail_with_device_cgprep_equals_host_text_and_reference(emu_lib, tmp_path):
    if helpers.ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")
    _child(emu_lib, r'''
d = pathlib.Path(%r)
fa, r1, r2 = T._pe_case(d, 61, 60, L=100, sub_rate=0.02, indel_frac=0.2, random_frac=0.05)
ctx = bm2.Context(0, fa)
ctx2 = bm2.Context(0, share=ctx)
tail = S.PeTail(T, d, fa, r1, r2)
print("ok", P.check_pe_tail(tail, ctx, ctx2))
''' % str(tmp_path))


def test_tail_phases_name_the_device_prep(emu_lib, tmp_path):
    # BM2_TAIL_PROF=1 with the bit: the CIGAR batch reports `prep (device)` and neither `slices` nor `order`
    if helpers.ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")
    p = _child(emu_lib, r'''
d = pathlib.Path(%r)
print("ok", P.tail_phases(T, M, d, lambda fa: bm2.Context(0, fa), n_reads=120))
''' % str(tmp_path), env=dict(os.environ, BM2_TAIL_PROF="1"))
    err = p.stderr.decode()
    assert re.search(r"gen_cigar_dev\s+prep \(device\)", err), err[-2000:]
    assert not re.search(r"gen_cigar_dev\s+slices", err) and not re.search(r"gen_cigar_dev\s+order", err), err[-2000:]
