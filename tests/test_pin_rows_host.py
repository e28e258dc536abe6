"""The host side of the one-launch pin path (adelie_amd/csrc/pin_rows_host.hpp): the CSR rows of ``betas`` assembled from the
kernel's snapshot block, as a stand-alone program under the address and undefined-behaviour sanitizers, on the CPU."""
import os
import shutil
import subprocess


def test_pin_rows_host_under_sanitizers(tmp_path):
    """Rows written out by hand, in float64 and float32: an active set given out of column order, groups of sizes 1 and 3
    mixed, a row with no active group, fewer rows than lambdas, an active group whose coefficients are all zero at an early row;
    ``active_order`` / ``active_begins``; and the refusals (shrinking active size, entries outside the screen set)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required (the oracle needs one as well)"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "pin_rows_main.cpp")
    exe = str(tmp_path / "pin_rows")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "pin_rows: ok" in out.stdout, out.stdout + out.stderr
