"""The CIGAR batch prepared on the MI355X (cgprep.hip) -- sorted after the SEMARK file on purpose.  bm2_cigar_prep_dev against
bm2_cigar_prep on tasks made by hand and at random (every event of the rule), batch sizes at the kernels' block edges up to 70 000 tasks,
arguments and refusals, the three launch knobs (a child process each), and bm2_sam_se_dev / bm2_sam_pe_dev / the _multi forms with
BM2_SAM_F_DEVICE_CGPREP (alone, with CGPLAN, with every other bit of the tail) against the flag-off text, its planned / used / missed,
and `bwa-mem2 mem`'s text.  All comparisons are exact.  The checks themselves are in cigar_prep_cases.py, shared with the emulator tests."""
import os
import re
import subprocess
import sys

import pytest

import bm2
import helpers
import cigar_prep_cases as P
import pe_decide_cases as S
import se_mark_cases as M
import test_sam_tail as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _needs_reference():
    if helpers.ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")


def _child(body, env=None, timeout=300):
    script = ("import sys, pathlib\n"
              "sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
              "import bm2, cigar_prep_cases as P, se_mark_cases as M, test_sam_tail as T\n"
              % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "bwa-mem2_amd"))) + body
    p = subprocess.run([sys.executable, "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
    assert p.returncode == 0 and p.stdout.startswith(b"ok"), (p.stdout.decode()[-500:], p.stderr.decode()[-3000:])
    return p


def test_cigar_prep_device_against_host_on_tasks_made_by_hand_and_at_random(gpu_ctx_factory):
    tot = P.check_tasks(gpu_ctx_factory(None))
    print(sorted(tot.items()))


def test_cigar_prep_batch_sizes_at_block_edges(gpu_ctx_factory):
    print(P.check_batches(gpu_ctx_factory(None)))


def test_cigar_prep_arguments_and_refusals(gpu_ctx_factory):
    assert P.check_arguments(gpu_ctx_factory(None))


@pytest.mark.parametrize("knob,value", [("BM2_CIGAR_NO_LDS", "1"), ("BM2_CIGAR_NO_RING", "1"), ("BM2_CIGAR_RING_BY_BAND", "0")])
def test_cigar_prep_follows_the_launch_knob(knob, value):
    _child("ctx = bm2.Context(0, None)\nprint('ok', P.check_knob(ctx, %r))\n" % knob, env=dict(os.environ, **{knob: value}))


def test_sam_se_dev_with_device_cgprep(gpu_ctx_factory, tmp_path):
    _needs_reference()
    assert P.check_se_tail(T, M, tmp_path, gpu_ctx_factory, n_reads=1500)


def test_sam_pe_dev_with_device_cgprep(gpu_ctx_factory, tmp_path):
    _needs_reference()
    fa, r1, r2 = T._pe_case(tmp_path, 61, 750, sub_rate=0.02, indel_frac=0.2, random_frac=0.03)
    ctx = gpu_ctx_factory(fa)
    ctx2 = bm2.Context(0, share=ctx)
    try:
        assert P.check_pe_tail(S.PeTail(T, tmp_path, fa, r1, r2), ctx, ctx2)
    finally:
        ctx2.close()


def test_tail_phases_name_the_device_prep(tmp_path):
    # BM2_TAIL_PROF=1 with the bit, in a child whose stderr is read: `prep (device)` and neither `slices` nor `order`
    _needs_reference()
    p = _child("print('ok', P.tail_phases(T, M, pathlib.Path(%r), lambda fa: bm2.Context(0, fa), n_reads=300))\n" % str(tmp_path),
               env=dict(os.environ, BM2_TAIL_PROF="1"))
    err = p.stderr.decode()
    assert re.search(r"gen_cigar_dev\s+prep \(device\)", err), err[-2000:]
    assert not re.search(r"gen_cigar_dev\s+slices", err) and not re.search(r"gen_cigar_dev\s+order", err), err[-2000:]
