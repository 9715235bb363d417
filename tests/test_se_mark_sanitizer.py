"""bm2_se_mark (the single-end tail's decide step behind a C name, the oracle of semark.hip) under AddressSanitizer and UBSan, as a
stand-alone program on the CPU: tools/san/se_mark_san.cpp and sam_tail.cpp compiled together with -fsanitize=address,undefined, run over
the hand-made lists of se_mark_cases.py (every length around the kernels' edges, every option set), which this test dumps to a file.
Nothing is loaded into Python and no device is involved."""
import os
import shutil
import subprocess

import se_mark_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_se_mark_host_code_under_address_and_ub_sanitizer(tmp_path):
    cxx = "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "se_mark_san")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-w", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "san", "se_mark_san.cpp"), os.path.join(ROOT, "bwa-mem2_amd", "csrc", "sam_tail.cpp"), "-o", exe])
    dump = str(tmp_path / "lists.bin")
    n = M.dump_lists(dump)
    p = subprocess.run([exe, dump], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and p.stdout.startswith(b"ok %d batches" % n), (p.stdout.decode()[-300:], p.stderr.decode()[-3000:])
