"""bm2_ksw_align2 (the host twin of the mate-rescue Smith-Waterman, the oracle of matesw.hip) under AddressSanitizer and UBSan, as a
stand-alone program on the CPU: tools/san/ksw_san.cpp and sam_tail.cpp compiled together with -fsanitize=address,undefined, run over the
hand-made tasks of tail_dp_cases.py (every edge of the kernels under every option set: among them the byte passes that saturate with
KSW_XSTART set, where the start pass used to build a profile of an empty query), which this test dumps to a file.  The program's results
must be the library's.  Nothing is loaded into Python and no device is involved."""
import os
import shutil
import subprocess

import numpy as np

import tail_dp_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ksw_align2_host_code_under_address_and_ub_sanitizer(tmp_path):
    cxx = "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "ksw_san")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-w", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "san", "ksw_san.cpp"), os.path.join(ROOT, "bwa-mem2_amd", "csrc", "sam_tail.cpp"), "-o", exe])
    dump, out = str(tmp_path / "tasks.bin"), str(tmp_path / "out.bin")
    sets, n = D.dump_ksw(dump)
    p = subprocess.run([exe, dump, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and p.stdout.startswith(b"ok %d sets %d tasks" % (sets, n)), (p.stdout.decode()[-300:], p.stderr.decode()[-3000:])
    got = np.fromfile(out, "<i4").reshape(-1, 7)
    assert (got == D.ksw_hand_made_answers()).all()
