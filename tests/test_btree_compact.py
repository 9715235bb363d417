"""The COMPACT form of chain.hip's kbtree restatement (CTree / CNode / CChain of chain_dev.h: what k_chain_heavy keeps in LDS -- 40-byte nodes with 16-bit keys
and pointers and NO copy of the keys' sort fields, which a probe reads from the chain records instead) must be the same tree as the memory form it restates
(bt_put / bt_lower / bt_traverse over BtNode with reg = false): same split points, same placement of equal keys, same in-order sequence, same lower bounds.
Both are compiled for the host and driven by one thread over the same random insertion sequences; after EVERY insertion the in-order key sequences and
the lower-bound look-ups are compared, at the end the trees node for node.  Sizes: the first split (9 / 10 keys), the tiers' capacities (128, 512, 1000) and
the largest one without staging (1184); for each, key spans small enough that equal keys are the rule, and one of 2^34 (keys beyond 32 bits, all distinct).
(The kernel on these trees: tests/test_chain_lds_compact_gpu.py.)"""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bt_lib(emu_lib, tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools", "emu"))
    import build_emu
    d = str(tmp_path_factory.mktemp("btcompact"))
    src = os.path.join(d, "chain_emu.cpp")
    with open(os.path.join(ROOT, "bwa-mem2_amd", "csrc", "chain.hip")) as g:
        open(src, "w").write(build_emu.rewrite(g.read()))
    so = os.path.join(d, "libbtcompact.so")
    cxx = "/opt/rocm/lib/llvm/bin/clang++" if os.path.exists("/opt/rocm/lib/llvm/bin/clang++") else "g++"
    emu_dir = os.path.dirname(emu_lib)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-pthread", "-w", "-fPIC", "-shared", "-I", os.path.join(ROOT, "tools", "emu", "fakehip"),
                           "-I", os.path.join(ROOT, "bwa-mem2_amd", "csrc"), '-DCHAIN_EMU_CPP="%s"' % src, os.path.join(ROOT, "tests", "btree_compact", "driver.cpp"),
                           "-L", emu_dir, "-l:" + os.path.basename(emu_lib), "-Wl,-rpath," + emu_dir, "-o", so])
    lib = ctypes.CDLL(so)
    lib.bt_compact_check.restype = ctypes.c_int
    lib.bt_compact_check.argtypes = [ctypes.c_uint, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]
    return lib


SIZES = [9, 10, 128, 512, 1000, 1184]


# spans: 1 (every key equal), 3, n / 8 + 2 and n / 2 + 1 (equal keys the rule), 2^34 (none equal, sort fields wider than a word)
@pytest.mark.parametrize("n,span", [(n, s) for n in SIZES for s in sorted({1, 3, n // 8 + 2, n // 2 + 1})] + [(n, 1 << 34) for n in SIZES])
def test_the_compact_tree_is_the_same_tree(bt_lib, n, span):
    detail = (ctypes.c_longlong * 4)()
    for seed in range(8):
        rc = bt_lib.bt_compact_check(seed * 7919 + n, n, span, 3, detail)
        assert rc == 0, "check %d failed (seed %d): %s" % (rc, seed, list(detail))
        assert detail[1] == n and 1 <= detail[0] <= n // 4 + 2
