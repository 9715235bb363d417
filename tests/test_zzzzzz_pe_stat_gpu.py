"""The chunk's insert-size model counted on the MI355X (pestat.hip) -- sorted after the plan file on purpose.
bm2_pe_stat_dev against bm2_pe_stat on lists made by hand and at random (every bin, the four models), the thresholds of the model, one
bin under 70 000 adds with one and with several copies of the histogram, batch sizes at block edges, capacity and refusals, and
bm2_sam_pe_dev / the _multi form with BM2_SAM_F_DEVICE_PESTAT (alone and with PLAN, PLAN | RESCUE, PLAN | RESCUE | DECIDE | TEXT) against
the flag-off text and `bwa-mem2 mem`'s, with the hits uploaded once for the model and the plan.  All comparisons are exact.  The checks
themselves are in pe_stat_cases.py, shared with the emulator tests."""
import os

import pytest

import bm2
import helpers
import pe_decide_cases as S
import pe_stat_cases as P
import test_sam_tail as T

pytestmark = pytest.mark.gpu


def _needs_reference():
    if helpers.ref_binary() is None:
        helpers.no_checker("oracle/_ref reference binary not present")


def test_stat_device_against_host_on_lists_made_by_hand_and_at_random(gpu_ctx_factory, golden_dir):
    pre = os.path.join(golden_dir, "g60k.fa")
    print(P.check_lists(gpu_ctx_factory(pre), pre))


def test_stat_model_thresholds(gpu_ctx_factory, golden_dir):
    pre = os.path.join(golden_dir, "g60k.fa")
    assert P.check_thresholds(gpu_ctx_factory(pre), pre)


def test_stat_one_bin_under_contention_with_one_copy_and_with_several(gpu_ctx_factory, golden_dir):
    pre = os.path.join(golden_dir, "g60k.fa")
    print(P.check_contention(gpu_ctx_factory(pre), pre))


def test_stat_batch_sizes_at_block_edges(gpu_ctx_factory, golden_dir):
    pre = os.path.join(golden_dir, "g60k.fa")
    print(P.check_sizes(gpu_ctx_factory(pre), pre))


def test_stat_capacity_and_refusals(gpu_ctx_factory, golden_dir):
    pre = os.path.join(golden_dir, "g60k.fa")
    assert P.check_capacity_and_refusals(gpu_ctx_factory(pre), pre)


def test_sam_pe_dev_with_device_pestat(gpu_ctx_factory, tmp_path):
    _needs_reference()
    fa, r1, r2 = T._pe_case(tmp_path, 61, 3000, sub_rate=0.02, indel_frac=0.2, random_frac=0.03)
    ctx = gpu_ctx_factory(fa)
    ctx2 = bm2.Context(0, share=ctx)
    try:
        tail = S.PeTail(T, tmp_path, fa, r1, r2)
        ref, pes = P.check_tail(tail, [], ctx)
        assert P.check_tail_two_contexts(tail, ctx, ctx2, 1000)[0] == ref
        P.check_tail_given_model(tail, ctx)
        P.check_tail_no_rescue(tail, ctx)
        P.check_tail_refusals(tail)
    finally:
        ctx2.close()


def test_sam_pe_dev_constructed_case(gpu_ctx_factory, tmp_path):
    _needs_reference()
    fa, r1, r2 = S.constructed_case(T, tmp_path)
    tail = S.PeTail(T, tmp_path, fa, r1, r2)
    ref, pes = P.check_tail(tail, [], gpu_ctx_factory(fa), combos=[0, P.PLAN | P.RESCUE | P.DECIDE | P.TEXT])
    print(len(ref.splitlines()), bm2.sam_pestat_stats())


def test_sam_se_dev_rejects_the_bit(gpu_ctx_factory, tmp_path):
    _needs_reference()
    fa, reads = T._case(tmp_path, 59, 8, L=100)
    ctx = gpu_ctx_factory(fa)
    with pytest.raises(bm2.Bm2Error) as e:
        T._ours(fa, reads, ["q%d" % i for i in range(len(reads))], [b"F" * len(r) for r in reads], None, bm2.default_sam_opt(flag=bm2.SAM_F_DEVICE_PESTAT), ctx=ctx)
    assert e.value.rc == bm2.BM2_EINVAL and "DEVICE_PESTAT" in str(e.value)
