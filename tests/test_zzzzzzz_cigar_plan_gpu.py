"""Which hits the SAM text asks a CIGAR for, picked on the MI355X (cgplan.hip) -- sorted after the pestat file on purpose.
bm2_cigar_plan_dev against bm2_cigar_plan on lists made by hand and at random (single-end and paired form, every option the rule reads,
list lengths around the row form and the LDS capacity), batch sizes at the kernels' block edges, capacity and refusals, and
bm2_sam_pe_dev / bm2_sam_se_dev / the _multi forms with BM2_SAM_F_DEVICE_CGPLAN (alone, with DECIDE, with PLAN | RESCUE | DECIDE, with
all six) against the flag-off text, its planned / used / missed, and `bwa-mem2 mem`'s text.  All comparisons are exact.  The checks
themselves are in cigar_plan_cases.py, shared with the emulator tests."""
import os

import pytest

import bm2
import helpers
import cigar_plan_cases as P
import pe_decide_cases as S
import test_sam_tail as T

pytestmark = pytest.mark.gpu


def _needs_reference():
    if helpers.ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")


def test_plan_device_against_host_on_lists_made_by_hand_and_at_random(gpu_ctx_factory, golden_dir):
    tot = P.check_lists(gpu_ctx_factory(os.path.join(golden_dir, "g60k.fa")))
    print(sorted(tot.items()))


def test_plan_batch_sizes_at_block_edges(gpu_ctx_factory, golden_dir):
    print(P.check_sizes(gpu_ctx_factory(os.path.join(golden_dir, "g60k.fa"))))


def test_plan_capacity_and_refusals(gpu_ctx_factory, golden_dir):
    assert P.check_capacity_and_refusals(gpu_ctx_factory(os.path.join(golden_dir, "g60k.fa")))


def test_sam_pe_dev_with_device_cgplan(gpu_ctx_factory, tmp_path):
    _needs_reference()
    fa, r1, r2 = T._pe_case(tmp_path, 61, 3000, sub_rate=0.02, indel_frac=0.2, random_frac=0.03)
    ctx = gpu_ctx_factory(fa)
    ctx2 = bm2.Context(0, share=ctx)
    try:
        tail = S.PeTail(T, tmp_path, fa, r1, r2)
        ref = P.check_tail(tail, ctx)
        assert P.check_tail_two_contexts(tail, ctx, ctx2, 1000, combos=[0, P.PESTAT | P.PLAN | P.RESCUE | P.DECIDE | P.TEXT]) == ref
        P.check_tail_options(tail, ctx)
        P.check_tail_refusals(tail)
    finally:
        ctx2.close()


def test_sam_pe_dev_constructed_case(gpu_ctx_factory, tmp_path):
    _needs_reference()
    fa, r1, r2 = S.constructed_case(T, tmp_path)
    tail = S.PeTail(T, tmp_path, fa, r1, r2)
    ref = P.check_tail(tail, gpu_ctx_factory(fa), combos=[0, P.PESTAT | P.PLAN | P.RESCUE | P.DECIDE | P.TEXT])
    print(len(ref.splitlines()), bm2.sam_cigar_plan_stats())


def test_sam_se_dev_with_device_cgplan(gpu_ctx_factory, tmp_path):
    _needs_reference()
    assert P.check_se_tail(T, tmp_path, gpu_ctx_factory, n_reads=1500)
