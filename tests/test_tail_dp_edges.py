"""The device tail's two alignment kernel families at their edges, without a GPU: the cases of tail_dp_cases.py on the host twins
(bm2_ksw_align2, bm2_gen_cigar) against the cases' own properties and the compiled reference's ksw_align2 / bwa_gen_cigar2, on the lane
emulator of matesw_dev.h (tools/emu/matesw_emu.cpp, LDS rows and register rows), and on the emulator library through the real launchers
(task records, the register / LDS split, the row tiers, the four CIGAR shapes).  The same checks run on the MI355X in
tests/test_zzzzzzzzzz_tail_dp_edges_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

import bm2
import helpers
import tail_dp_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def index_prefix(tmp_path_factory):
    return D.write_index(tmp_path_factory.mktemp("tail_dp"))


def test_host_ksw_align2_at_the_edges_of_the_rescue_kernels():
    # byte saturation at and below the clamp (with / without KSW_XSTART, minimum score above / below 255), KSW_XSTOP, the register / LDS split,
    # the row tiers, the list of local maxima at its capacity, the exclusion window, the tie rule of qe, an insertion across lanes, N, target
    # lengths 0, 1, 4096, 5000: what the construction of each task says about its answer; every event counted and asserted
    print(sorted(D.check_ksw(None).items()))


def test_host_ksw_align2_arguments():
    print(D.check_ksw_arguments(None))


def test_host_gen_cigar_at_the_edges_of_the_cigar_kernels(index_prefix):
    # every non-NULL answer re-scored from its ops, NM and MD rebuilt, whole-matrix bands against a plain Needleman-Wunsch
    print(sorted(D.check_cigar(None, index_prefix).items()))


@pytest.mark.parametrize("set_no", [0, 1, 2])
def test_host_ksw_align2_edges_against_the_reference(tmp_path, set_no):
    dump = helpers.ref_binary("refdump")
    if dump is None:
        helpers.no_checker("oracle/_ref not built (make -C oracle ref)")
    print(D.check_ksw_against_reference(dump, tmp_path, set_no))


@pytest.mark.parametrize("set_no", [0, 1, 2])
def test_host_gen_cigar_edges_against_the_reference(tmp_path, index_prefix, set_no):
    dump = helpers.ref_binary("refdump")
    if dump is None:
        helpers.no_checker("oracle/_ref not built (make -C oracle ref)")
    print(D.check_cigar_against_reference(dump, tmp_path, index_prefix, set_no))


@pytest.fixture(scope="module")
def matesw_emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emu") / "matesw_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(ROOT, "tools", "emu", "matesw_emu.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("reg", [0, 1], ids=["lds_rows", "register_rows"])
@pytest.mark.parametrize("set_no", [0, 1, 2])
def test_rescue_device_source_on_the_lane_emulator_at_the_edges(matesw_emu, tmp_path, set_no, reg):
    # the hand-made tasks of at most 161 x 200 (the emulator runs a task at a time on 16 threads, so the fifty short fillers of a tier batch,
    # which are there for the batch's stride, stay with the launcher tests below)
    opt = bm2.default_opt(**D.OPTION_SETS[set_no])
    b = D.ksw_small_tasks(opt, 900 + set_no)
    exp = bm2.ksw_align2(b.pairs, b.xtra, opt)
    pf, of = str(tmp_path / "pairs.txt"), str(tmp_path / "out.bin")
    D.write_pairs(pf, b.pairs, b.xtra)
    env = dict(os.environ, A=str(opt.a), B=str(opt.b), O_DEL=str(opt.o_del), E_DEL=str(opt.e_del), O_INS=str(opt.o_ins), E_INS=str(opt.e_ins))
    env.pop("EMU_KSW_REG", None)
    if reg:
        env["EMU_KSW_REG"] = "1"
    subprocess.check_call([matesw_emu, pf, of], env=env, timeout=900)
    got = np.fromfile(of, "<i4").reshape(-1, 7)
    D._first_diff(b, exp, got, "lane emulator")
    seen = D.ksw_events(opt, b, exp, {}, reg)                    # (only under a = 2 is a saturating copy, 125 bases, short enough for the emulator)
    print(sorted(seen.items()))
    want = (["sat_at", "sat_below"] if set_no == 1 else []) + ["stop_cut_byte", "stop_cut_word", "win_inside", "win_outside", "qe_tie", "ins_across_lanes_byte", "ins_across_lanes_word",
            "target_N", "tlen_0", "tlen_1", "lds_161", "reg_160" if reg else "lds_160"] + (["sat_on_registers"] if reg and set_no == 1 else [])
    assert not [ev for ev in want if not seen.get(ev)], seen


HEAD = r'''
import sys, pathlib
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, bm2
bm2.LIB_PATH = %r
import tail_dp_cases as D
'''


def _child(lib, body, timeout=1500, env=None):
    script = HEAD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "bwa-mem2_amd"), lib) + body
    p = subprocess.run(["python", "-c", script], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
    assert p.returncode == 0 and p.stdout.startswith(b"ok"), (p.stdout.decode()[-500:], p.stderr.decode()[-3000:])
    return p


def test_cigar_kernels_on_the_emulator_at_the_edges(emu_lib, index_prefix):
    # the hand-made CIGAR tasks through bm2_gen_cigar_dev: the ring at band 31 and ROW at 32 with indels along the band's edge, the packed
    # 16-bit words driven down by all-mismatch queries at q_len 220 | 221 and at the CG_SMALL bound, the strands' first and last bases,
    # ranges below eight bases, partial row stores, MD runs of four and five digits, batches of 1, 63, 64, 65
    _child(emu_lib, r'''
fa = %r
ctx = bm2.Context(0, fa)
tot = D.check_cigar(lambda tasks, opt: bm2.gen_cigar(fa, opt, tasks, ctx=ctx), fa, n_random=0, who="emulator")
print("ok", sorted(tot.items()))
''' % index_prefix)


def test_rescue_launcher_on_the_emulator_at_the_edges(emu_lib):
    # the hand-made rescue batches through bm2_ksw_align2_dev's launcher (all-register, all-LDS and mixed batches, 16 / 8 / 4 rows per block, the
    # short tasks striding by the batch's longest), and the refusals of both forms: no launch behind any of them, nothing written
    _child(emu_lib, r'''
ctx = bm2.Context(0, None)
ref = D.check_ksw_arguments(ctx)
assert ref["tier_refused"] == 1
tot = D.check_ksw(lambda p, x, o: bm2.ksw_align2(p, x, o, ctx=ctx), n_random=0, who="emulator")
print("ok", ref, sorted(tot.items()))
''')
