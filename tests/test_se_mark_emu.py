"""The `decide` phase of the single-end tail by the device kernels (semark.hip: k_sm_class, k_sm_list, k_sm_light, k_sm_heavy, and
cgplan.hip's kernels on the marks they leave in device memory), executed on the host emulator (tools/emu): bm2_se_mark_dev against
bm2_se_mark on lists made by hand and at random, list and batch sizes at the kernels' edges, arguments and refusals, and bm2_sam_se_dev /
bm2_sam_se_dev_multi with BM2_SAM_F_DEVICE_SEMARK (alone, with CGPLAN, with CGPLAN | TEXT) against the flag-off tail and the compiled
reference.  Each test runs in a process of its own (bm2 binds one library).  The checks themselves are in se_mark_cases.py, shared with
the GPU tests."""
import os
import re
import subprocess

import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = r'''
import sys, pathlib
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, bm2
bm2.LIB_PATH = %r
import se_mark_cases as M
import test_sam_tail as T
'''


def _child(lib, body, timeout=1500, env=None):
    script = HEAD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "bwa-mem2_amd"), lib) + body
    p = subprocess.run(["python", "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
    assert p.returncode == 0 and p.stdout.startswith(b"ok"), (p.stdout.decode()[-500:], p.stderr.decode()[-3000:])
    return p


def test_se_mark_device_against_host_on_lists_made_by_hand_and_at_random(emu_lib):
    # list lengths 0 .. 519 around the row form's 16 hits and the LDS capacity of 128; ties the hash decides, with first_id 0 and above
    # 2^32; overlaps at mask_level of the shorter stretch and one base to either side; a leader whose sub stays 0; sub_n at `close` and
    # one more, the is_alt clause, an incoming sub_n; no / only / mixed ALT hits, alt_sc, secondary = INT_MAX, secondary_all renamed;
    # MEM_F_PRIMARY5 with one reportable hit, the leftmost first or not, followers naming both positions, T at a score and one above;
    # empty lists between full ones; offsets that do not start at 0.  Every event is asserted to occur.
    _child(emu_lib, r'''
ctx = bm2.Context(0, None)
tot = M.check_lists(ctx, quick=True)
print("ok", len(tot))
''')


def test_se_mark_batch_sizes_at_block_edges(emu_lib):
    _child(emu_lib, r'''
ctx = bm2.Context(0, None)
print("ok", M.check_batches(ctx))
''')


def test_se_mark_arguments(emu_lib):
    _child(emu_lib, r'''
ctx = bm2.Context(0, None)
print("ok", M.check_arguments(ctx))
''')


def test_se_tail_with_device_semark_equals_host_text_and_reference(emu_lib, tmp_path):
    if helpers.ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")
    _child(emu_lib, r'''
d = pathlib.Path(%r)
made = []
def make(fa):
    made.append(bm2.Context(0, fa))
    return made[-1]
print("ok", M.check_se_tail(T, d, make, n_reads=120))
''' % str(tmp_path))


def test_se_tail_phases_name_the_device(emu_lib, tmp_path):
    # BM2_TAIL_PROF=1 with SEMARK | CGPLAN: the tail reports `decide (device)` and no `decide` phase of its own threads
    if helpers.ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")
    p = _child(emu_lib, r'''
d = pathlib.Path(%r)
print("ok", M.tail_phases(T, d, lambda fa: bm2.Context(0, fa), n_reads=120))
''' % str(tmp_path), env=dict(os.environ, BM2_TAIL_PROF="1"))
    err = p.stderr.decode()
    assert re.search(r"\[tail\] sam_se\s+decide \(device\)\s", err), err[-2000:]
    assert not re.search(r"\[tail\] sam_se\s+decide\s+\d", err), err[-2000:]
    for phase in ("pack", "H2D", "kernels", "D2H", "apply"):
        assert re.search(r"\[tail\] se_mark_dev\s+%s\s" % phase, err), (phase, err[-2000:])
