"""The unphased .snpdat reader of adelie_amd/csrc/snp_decode_host.hpp as a stand-alone program under the address and
undefined-behaviour sanitizers: no device, nothing loaded into Python."""
import os
import shutil
import subprocess

import numpy as np

import adelie_amd as ad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unphased_decoder_under_sanitizers(tmp_path):
    """snp_unphased_header / snp_unphased_decode_column (tests/native/snp_decode_main.cpp, -fsanitize=address,undefined): an
    image written by io.snp_unphased decodes to the int8 matrix it was written from (n = 700 is no multiple of 256: the last
    chunk of a column is short), and every directed damage -- truncations at the ends of the header, of the offset table, of a
    chunk header and of a chunk's rows, an outer entry past the end / huge / inside the header, a category offset within 3
    bytes of its column's end, a raised count byte, one chunk too many, a chunk index at ceil(n / 256) and at 2^32 - 1,
    n = 2^45 -- ends in the error return, each in a heap block of exactly its length, with nothing for the sanitizers to
    report.  The byte sweep of test_snpdat_decoder_rejects_corrupt_images (byte 4 excluded for the reason given there) runs
    under the sanitizers too."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required"
    src = os.path.join(ROOT, "tests", "native", "snp_decode_main.cpp")
    exe = str(tmp_path / "snp_decode")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    rng = np.random.RandomState(0)
    n, p = 700, 5
    cd = rng.choice(np.array([0, 1, 2, -9], dtype=np.int8), size=(n, p), p=[0.5, 0.3, 0.1, 0.1])
    image, calls = str(tmp_path / "a.snpdat"), str(tmp_path / "calls.bin")
    ad.io.snp_unphased(image).write(np.asfortranarray(cd))
    cd.ravel(order="F").tofile(calls)
    out = subprocess.run([exe, image, calls], capture_output=True, text=True)
    assert out.returncode == 0 and "snp_decode: ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    lines = out.stdout.splitlines()
    hdr = 17 + 24 * p + 8 * (p + 1)
    for cut in (0, 5, 16, hdr - 1, hdr, hdr + 10, hdr + 23, hdr + 24, os.path.getsize(image) - 1):
        assert any(ln.startswith(f"truncated at {cut} ") for ln in lines), cut
    assert sum("truncated at" in ln for ln in lines) >= 20
    for msg in ("category offset", "chunk (overrun)", "column index"):                    # the cuts inside the last column, re-indexed
        assert any(ln.startswith("cut and re-indexed at") and msg in ln for ln in lines), msg
    for what in ("outer[p] past the end", "outer[0] huge", "outer[0] inside the header", "cat_off[2] 0 bytes", "cat_off[2] 3 bytes",
                 "chunk count byte raised", "one chunk too many", "chunk_idx past the rows", "chunk_idx 2^32 - 1", "n = 2^45"):
        assert any(ln.startswith(what) and "(decoded)" not in ln for ln in lines), what
    assert "(decoded)" not in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
