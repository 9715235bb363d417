"""The device tail's two alignment kernel families at their edges on the MI355X -- sorted after the CGPREP file on purpose.  The cases of
tail_dp_cases.py (shared with the emulator tests): k_ksw_align2 / k_ksw_align2_reg through bm2_ksw_align2_dev and k_cigar_flat /
k_gen_cigar<RING | ROW | GLOBAL> through bm2_gen_cigar_dev against the host twins, field by field, on the hand-made tasks of every edge and
random ones, under three option sets; the refusals of both forms; the launch knobs BM2_KSW_REG=0, BM2_CIGAR_NO_RING=1 and
BM2_CIGAR_NO_LDS=1 in a child process each on the hand-made tasks (the shape rule restated with the knob); and the device against the
compiled reference's own ksw_align2 / bwa_gen_cigar2.  Every comparison is exact; every named event is asserted to occur."""
import os
import subprocess
import sys

import pytest

import bm2
import helpers
import tail_dp_cases as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def index_prefix(tmp_path_factory):
    return D.write_index(tmp_path_factory.mktemp("tail_dp"))


@pytest.fixture(scope="module")
def bare_ctx(gpu_ctx_factory):
    return gpu_ctx_factory()


@pytest.fixture(scope="module")
def index_ctx(gpu_ctx_factory, index_prefix):
    return gpu_ctx_factory(index_prefix)


def _child(body, env=None, timeout=300):
    script = ("import sys, pathlib\n"
              "sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
              "import bm2, tail_dp_cases as D\n"
              % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "bwa-mem2_amd"))) + body
    p = subprocess.run([sys.executable, "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
    assert p.returncode == 0 and p.stdout.startswith(b"ok"), (p.stdout.decode()[-500:], p.stderr.decode()[-3000:])
    return p


def test_rescue_kernels_arguments_and_refusals(bare_ctx):
    # (first: what is refused never reaches a kernel)
    ref = D.check_ksw_arguments(bare_ctx)
    assert ref["tier_refused"] == 1
    print(ref)


def test_rescue_kernels_against_host_at_their_edges(bare_ctx):
    ctx = bare_ctx
    tot = D.check_ksw(lambda p, x, o: bm2.ksw_align2(p, x, o, ctx=ctx))
    print(sorted(tot.items()))


def test_rescue_lds_kernel_alone_follows_the_knob():
    p = _child("ctx = bm2.Context(0, None)\n"
               "tot = D.check_ksw(lambda p, x, o: bm2.ksw_align2(p, x, o, ctx=ctx), n_random=0, reg=False)\n"
               "print('ok', sorted(tot.items()))\n", env=dict(os.environ, BM2_KSW_REG="0"))
    print(p.stdout.decode())


def test_cigar_kernels_against_host_at_their_edges(index_ctx, index_prefix):
    ctx = index_ctx
    tot = D.check_cigar(lambda tasks, opt: bm2.gen_cigar(index_prefix, opt, tasks, ctx=ctx), index_prefix)
    print(sorted(tot.items()))


@pytest.mark.parametrize("knob,knobs", [("BM2_CIGAR_NO_RING", dict(no_ring=1)), ("BM2_CIGAR_NO_LDS", dict(no_lds=1))])
def test_cigar_kernels_follow_the_launch_knob(index_prefix, knob, knobs):
    p = _child("fa = %r\nctx = bm2.Context(0, fa)\n"
               "tot = D.check_cigar(lambda tasks, opt: bm2.gen_cigar(fa, opt, tasks, ctx=ctx), fa, n_random=0, knobs=%r)\n"
               "print('ok', sorted(tot.items()))\n" % (index_prefix, knobs), env=dict(os.environ, **{knob: "1"}))
    print(p.stdout.decode())


@pytest.mark.parametrize("set_no", [0, 1, 2])
def test_rescue_kernels_edges_against_the_reference(bare_ctx, tmp_path, set_no):
    dump = helpers.ref_binary("refdump")
    if dump is None:
        helpers.no_checker("oracle/_ref not built (make -C oracle ref)")
    ctx = bare_ctx
    print(D.check_ksw_against_reference(dump, tmp_path, set_no, form=lambda p, x, o: bm2.ksw_align2(p, x, o, ctx=ctx)))


@pytest.mark.parametrize("set_no", [0, 1, 2])
def test_cigar_kernels_edges_against_the_reference(index_ctx, tmp_path, index_prefix, set_no):
    dump = helpers.ref_binary("refdump")
    if dump is None:
        helpers.no_checker("oracle/_ref not built (make -C oracle ref)")
    ctx = index_ctx
    print(D.check_cigar_against_reference(dump, tmp_path, index_prefix, set_no, form=lambda tasks, opt: bm2.gen_cigar(index_prefix, opt, tasks, ctx=ctx)))
