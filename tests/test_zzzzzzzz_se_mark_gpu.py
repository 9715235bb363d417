"""The `decide` phase of the single-end tail on the MI355X (semark.hip) -- sorted after the CIGAR-plan file on purpose.  bm2_se_mark_dev
against bm2_se_mark on lists made by hand and at random (list lengths around the row form and the LDS capacity, every event of the rule),
batch sizes at the kernels' block edges, arguments, and bm2_sam_se_dev / bm2_sam_se_dev_multi with BM2_SAM_F_DEVICE_SEMARK (alone, with
CGPLAN, with CGPLAN | TEXT) against the flag-off text, its planned / used / missed, and `bwa-mem2 mem`'s text.  All comparisons are
exact.  The checks themselves are in se_mark_cases.py, shared with the emulator tests."""
import os
import re
import subprocess
import sys

import pytest

import bm2
import helpers
import se_mark_cases as M
import test_sam_tail as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _needs_reference():
    if helpers.ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")


def test_se_mark_device_against_host_on_lists_made_by_hand_and_at_random(gpu_ctx_factory):
    tot = M.check_lists(gpu_ctx_factory(None))
    print(sorted(tot.items()))


def test_se_mark_batch_sizes_at_block_edges(gpu_ctx_factory):
    print(M.check_batches(gpu_ctx_factory(None)))


def test_se_mark_arguments(gpu_ctx_factory):
    assert M.check_arguments(gpu_ctx_factory(None))


def test_sam_se_dev_with_device_semark(gpu_ctx_factory, tmp_path):
    _needs_reference()
    assert M.check_se_tail(T, tmp_path, gpu_ctx_factory, n_reads=1500)


def test_sam_se_dev_phases_name_the_device(tmp_path):
    # BM2_TAIL_PROF=1 with SEMARK | CGPLAN, in a child whose stderr is read: `decide (device)` and no `decide` phase of the host threads
    _needs_reference()
    script = ("import sys, pathlib\n"
              "sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
              "import bm2, se_mark_cases as M, test_sam_tail as T\n"
              "print('ok', M.tail_phases(T, pathlib.Path(%r), lambda fa: bm2.Context(0, fa), n_reads=300))\n"
              % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "bwa-mem2_amd"), str(tmp_path)))
    p = subprocess.run([sys.executable, "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=dict(os.environ, BM2_TAIL_PROF="1"))
    err = p.stderr.decode()
    assert p.returncode == 0 and p.stdout.startswith(b"ok"), (p.stdout.decode()[-500:], err[-3000:])
    assert re.search(r"\[tail\] sam_se\s+decide \(device\)\s", err), err[-2000:]
    assert not re.search(r"\[tail\] sam_se\s+decide\s+\d", err), err[-2000:]
    for phase in ("pack", "H2D", "kernels", "D2H", "apply"):
        assert re.search(r"\[tail\] se_mark_dev\s+%s\s" % phase, err), (phase, err[-2000:])
