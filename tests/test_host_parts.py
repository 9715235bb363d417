"""The part fan-out of the device hooks and the sharded hot path (bwa-mem2_amd/csrc/host_pool.h: bm2_parts, bm2_part_lo, bm2_run_parts):
the parts rule against the expression it replaced, the part bounds, threads and budgets per part, the lowest failing part's code and
message.  Compiled with g++ here (the header is plain C++; the library builds it with hipcc)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parts_rule_bounds_fan_out_and_errors(tmp_path):
    exe = str(tmp_path / "run_parts_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "bwa-mem2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "run_parts_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok", (p.stdout[-500:], p.stderr[-500:])
