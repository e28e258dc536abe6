"""The pivot rule's reading of the sorted scores as a free function, and the depth rule that places the filtered sweep's
threshold by it (adelie_amd/csrc/screen_reads_host.hpp, what Solver::screen() calls), as a stand-alone program under the address
and undefined-behaviour sanitizers, on the CPU."""
import os
import shutil
import subprocess


def test_screen_reads_under_sanitizers(tmp_path):
    """20 000 random score sets (ties at the cap, screen groups scattered and clustered, n_new_active 0..50, G 1..20 000): for
    every M from 0 to G the function on the sorted top M appends what it appends on all G whenever it reports `sufficient`,
    and reports it exactly when no read goes below position G - M; then the threshold depth, the byte rule and the list
    capacity at their edges."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required (the oracle needs one as well)"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "screen_reads_main.cpp")
    exe = str(tmp_path / "screen_reads")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "screen_reads: ok" in out.stdout, out.stdout + out.stderr
