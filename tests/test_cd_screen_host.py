"""The host-only decisions of the screen-set coordinate descents, bvls and pinball (adelie_amd/csrc/cd_screen_host.hpp, what
CdScreenDriver::run and the two C entry points call), as a stand-alone program under the address and undefined-behaviour
sanitizers, on the CPU."""
import os
import shutil
import subprocess


def test_cd_screen_host_under_sanitizers(tmp_path):
    """Admission of a KKT round, in float64 and float32, against expectations written out by hand: ties to the lower index,
    +-inf, kappa of 1 / exactly / above the number of violators, all violators members, a violator left over when kappa is
    exhausted, p = 1; then the warm-start validation: duplicates, indices out of range, active indices that are no members."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required (the oracle needs one as well)"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "cd_screen_main.cpp")
    exe = str(tmp_path / "cd_screen")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "cd_screen: ok" in out.stdout, out.stdout + out.stderr
