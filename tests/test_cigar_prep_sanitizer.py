"""bm2_cigar_prep (the host statement of the CIGAR batch's preparation, the oracle of cgprep.hip) under AddressSanitizer and UBSan, as a
stand-alone program on the CPU: tools/san/cigar_prep_san.cpp and cigar_prep.cpp compiled together with -fsanitize=address,undefined, run
over the hand-made tasks of cigar_prep_cases.py (every event of the rule, the NULL returns with their out-of-range coordinates, the DP area
beyond 2^31), which this test dumps to a file.  Nothing is loaded into Python and no device is involved."""
import os
import shutil
import subprocess

import cigar_prep_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cigar_prep_host_code_under_address_and_ub_sanitizer(tmp_path):
    cxx = "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "cigar_prep_san")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-w", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "san", "cigar_prep_san.cpp"), os.path.join(ROOT, "bwa-mem2_amd", "csrc", "cigar_prep.cpp"), "-o", exe])
    dump = str(tmp_path / "tasks.bin")
    n = P.dump_tasks(dump)
    p = subprocess.run([exe, dump], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and p.stdout.startswith(b"ok %d batches" % n), (p.stdout.decode()[-300:], p.stderr.decode()[-3000:])
