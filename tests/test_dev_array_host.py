"""The array type that the design handles own their device memory with (adelie_amd/csrc/dev_array_host.hpp) as a stand-alone
program under the address and undefined-behaviour sanitizers: no device, nothing loaded into Python.  The program
(tests/native/dev_array_main.cpp) runs the type on malloc/free and prints the bytes it owns after every step; the numbers are
judged here, and a double free, a use after release or a leak is the sanitizers' report."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# step -> bytes owned after it
EXPECTED = [
    ("start", 0),
    ("alloc", 37 * 8),
    ("destroyed", 0),
    ("alloc_void", 13),
    ("try_alloc_refused", 0),
    ("alloc_refused", 0),
    ("try_alloc_refused_over_owner", 0),
    ("move_construct", 8 * 4),
    ("second_owner", 8 * 4 + 3 * 4),
    ("move_assign", 8 * 4),
    ("self_move", 8 * 4),
    ("moved_destroyed", 0),
    ("borrowed", 4 * 8),
    ("borrow_over_owner", 4 * 8),
    ("borrowers_destroyed", 4 * 8),
    ("self_borrow", 4 * 8),
    ("reset", 0),
    ("reset_twice", 0),
    ("struct_alloc_threw", 10 * 8 + 6 * 4),
    ("struct_destroyed", 0),
    ("end", 0),
]


def test_owned_array_counts_and_frees_exactly_what_it_owns(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required"
    src = os.path.join(ROOT, "tests", "native", "dev_array_main.cpp")
    exe = str(tmp_path / "dev_array")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    report = out.stdout + out.stderr[-3000:]
    assert out.returncode == 0, report
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr and "LeakSanitizer" not in out.stderr, report
    got = [(ln.split()[0], int(ln.split()[1])) for ln in out.stdout.splitlines()]
    assert got == EXPECTED
