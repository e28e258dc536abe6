"""adelie_amd/csrc/multi_shape.hpp -- the host-side decisions of the multi-response kernels -- as a stand-alone program under the
address and undefined-behaviour sanitizers, on the CPU; and the restatement of the sweep's plan in tests/multi_checks.py against
the header's.  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

import multi_checks as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shape_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required (the oracle needs one as well)"
    src = os.path.join(ROOT, "tests", "native", "multi_shape_main.cpp")
    exe = str(tmp_path_factory.mktemp("multi_shape") / "multi_shape")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    return exe


def test_shape_functions_under_sanitizers(shape_exe):
    """nb in 1 .. 10000, nfeat in {1, 7, 8, 9, 31, 32, 33, 1000, 20000}, K in 1 .. 17, vec in {1, 2, 4}, the two alignment
    conditions: the splits cover the rows in whole units of 256 * vec with none empty and at most 65535 of them, the work size
    covers nsplit * nfeat * K of the variant picked, the staged variant needs K > 4 and both alignment conditions."""
    out = subprocess.run([shape_exe], capture_output=True, text=True)
    assert out.returncode == 0 and "multi_shape: ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    counts = [int(x) for x in re.search(r"plans (\d+) staged (\d+) four-wave (\d+) plain (\d+) with several splits (\d+)", out.stdout).groups()]
    assert all(c > 0 for c in counts), counts


def test_python_plan_restates_the_header(shape_exe):
    """The plan tests/multi_checks.py emulates and expects of every sweep case, and over a grid, is the header's."""
    keys = set()
    for c in mc.SWEEP_CASES:
        a = dict(nb=c.nb, pb=c.pb, icpt=c.icpt, K=c.K, v_off=c.v_off, ld=(c.nb // 32 + 1) * 32 + (c.base == "oddld"), x_off=int(c.base == "xoff"))
        if c.base == "snp":
            a["bits"] = True
        es = 8 if c.dtype == "f64" else 4
        keys.add((c.nb, c.pb + c.icpt, c.K, mc.VEC[c.dtype], int(mc.base_vec_of(a, c.dtype)),
                  int(c.nb % mc.VEC[c.dtype] == 0 and (c.v_off * es) % 16 == 0)))
    for nb in (1, 63, 511, 512, 513, 2047, 2048, 2049, 4096, 4097, 9999):
        for nfeat in (1, 8, 9, 33, 1000, 20000):
            for K in (1, 3, 5, 9, 17):
                for vec in (2, 4):
                    for al in range(4):
                        keys.add((nb, nfeat, K, vec, al & 1, al >> 1))
    keys = sorted(keys)
    for k0 in range(0, len(keys), 500):
        chunk = keys[k0:k0 + 500]
        out = subprocess.run([shape_exe, "--plan"] + [str(x) for k in chunk for x in k], capture_output=True, text=True, check=True)
        rows = [tuple(int(x) for x in ln.split()) for ln in out.stdout.splitlines()]
        assert len(rows) == len(chunk)
        for k, row in zip(chunk, rows):
            assert tuple(mc.sweep_plan(k[0], k[1], k[2], k[3], bool(k[4]), bool(k[5]))) == row, k
            assert mc.sweep_work_elems(k[0], k[1], k[2], k[3]) >= row[5] * k[1] * k[2]


def test_constants_match_the_header():
    txt = open(os.path.join(ROOT, "adelie_amd", "csrc", "multi_shape.hpp")).read()
    for name, val in (("kMultiSweepThreads", mc.MT), ("kMultiBlock", mc.MAXB), ("kMultiFusedWaves", mc.MFS)):
        assert int(re.search(rf"constexpr int {name} = (\d+);", txt).group(1)) == val
    kern = open(os.path.join(ROOT, "adelie_amd", "csrc", "kernels_multi.hip")).read()
    assert '#include "multi_shape.hpp"' in kern and "inline void msweep_shape" not in kern and "inline int kt_of" not in kern
