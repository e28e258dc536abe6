"""Host side of matrix.snp_phased_ancestry, none of which needs a device: the numpy codec io.snp_phased_ancestry against the
definition of the matrix and against an image assembled byte by byte from the reference's layout
(io_snp_phased_ancestry.ipp:143-347), the writer's four errors, the decoder / packer of adelie_amd/csrc/phased_decode_host.hpp
as a stand-alone program under the address and undefined-behaviour sanitizers (valid and damaged images), the generator,
and the entry points' place in the ABI tables."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import adelie_amd as ad
from adelie_amd import _abi
from phased_checks import altered, expand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unused_ancestry(A):
    return None if A == 1 else (0 if A == 2 else 1)


def make_case(n, s, A, seed=0):
    """Random calls / ancestries with, where the sizes allow it: a SNP with no mutation (the first, s > 1), an ancestry
    never used (unused_ancestry(A)), both haplotypes of a sample mutated in one ancestry and in two, a mutation in the last
    row of the last haplotype with the last ancestry."""
    rng = np.random.RandomState(seed)
    cal = (rng.uniform(size=(n, 2 * s)) < 0.3).astype(np.int8)
    anc = rng.randint(0, A, size=(n, 2 * s)).astype(np.int8)
    if A > 1:
        anc[anc == unused_ancestry(A)] = A - 1
    if s > 1:
        cal[:, 0:2] = 0
    cal[0, -2:] = 1
    anc[0, -2:] = A - 1
    if A > 2:
        cal[1, -2:] = 1
        anc[1, -2:] = (0, 2)
    cal[n - 1, -1] = 1
    anc[n - 1, -1] = A - 1
    return cal, anc


CASES = [(5, 2, 2), (300, 3, 4), (513, 1, 1)]


@pytest.mark.parametrize("n,s,A", CASES)
@pytest.mark.parametrize("read_mode", ["file", "mmap"])
def test_codec_round_trip(tmp_path, n, s, A, read_mode):
    cal, anc = make_case(n, s, A)
    E = expand(cal, anc, A)
    if s > 1:
        assert not E[:, :A].any()                       # a SNP with no mutation
    if A > 1:
        assert not E[:, unused_ancestry(A)::A].any() and E[:, A - 1::A].any()  # an ancestry never used
    assert E[n - 1].any() and (E == 2).any()
    if n == 513:
        assert E[512].any()                             # the third chunk holds one row
    path = str(tmp_path / "phased.snpdat")
    w = ad.io.snp_phased_ancestry(path)
    assert not w.is_read
    nbytes, bench = w.write(cal, anc, A)
    assert nbytes == os.path.getsize(path) and isinstance(bench, dict)
    h = ad.io.snp_phased_ancestry(path, read_mode=read_mode)
    with pytest.raises(RuntimeError, match="not read yet"):
        h.rows
    assert h.read() == nbytes and h.is_read
    assert h.endian == (not np.little_endian)
    assert (h.rows, h.snps, h.ancestries, h.cols) == (n, s, A, s * A)
    nnz0 = np.array([np.count_nonzero((cal[:, 2 * (c // A)] == 1) & (anc[:, 2 * (c // A)] == c % A)) for c in range(s * A)])
    nnz1 = np.array([np.count_nonzero((cal[:, 2 * (c // A) + 1] == 1) & (anc[:, 2 * (c // A) + 1] == c % A)) for c in range(s * A)])
    assert np.array_equal(h.nnz0, nnz0) and np.array_equal(h.nnz1, nnz1)
    assert h.outer.shape == (s + 1,) and int(h.outer[0]) == 18 + 16 * s * A + 8 * (s + 1) and int(h.outer[-1]) == nbytes
    D = h.to_dense()
    assert D.dtype == np.int8 and D.shape == (n, s * A) and np.array_equal(D, E)


def test_hand_assembled_image(tmp_path):
    """n = 3, s = 1, A = 2 written out from the layout: haplotype 0 is mutated in rows 0 (ancestry 0) and 1 (ancestry 1),
    haplotype 1 in rows 1 (ancestry 1) and 2 (ancestry 0)."""
    def hap(rows):  # one chunk (index 0) holding `rows`
        return struct.pack("<IIB", 1, 0, len(rows) - 1) + bytes(rows)

    anc0 = struct.pack("<QQ", 16, 26) + hap([0]) + hap([2])   # ancestry 0: haplotype 0 row 0, haplotype 1 row 2
    anc1 = struct.pack("<QQ", 16, 26) + hap([1]) + hap([1])   # ancestry 1: row 1 on both
    assert len(anc0) == len(anc1) == 36
    snp = struct.pack("<QQ", 16, 52) + anc0 + anc1
    head = (struct.pack("<BQQB", 0, 3, 1, 2) + struct.pack("<QQ", 1, 1) + struct.pack("<QQ", 1, 1)
            + struct.pack("<QQ", 66, 66 + len(snp)))
    assert len(head) == 66
    image = head + snp
    E = np.array([[1, 0], [0, 2], [1, 0]], dtype=np.int8)

    path = str(tmp_path / "hand.snpdat")
    with open(path, "wb") as f:
        f.write(image)
    h = ad.io.snp_phased_ancestry(path)
    assert h.read() == len(image) == 154
    assert (h.rows, h.snps, h.ancestries) == (3, 1, 2)
    assert np.array_equal(h.to_dense(), E)

    cal = np.array([[1, 0], [1, 1], [0, 1]], dtype=np.int8)
    anc = np.array([[0, 1], [1, 1], [1, 0]], dtype=np.int8)   # (ancestries of the two calls that are 0: in-range noise)
    assert np.array_equal(expand(cal, anc, 2), E)
    path2 = str(tmp_path / "written.snpdat")
    assert ad.io.snp_phased_ancestry(path2).write(cal, anc, 2)[0] == len(image)
    assert open(path2, "rb").read() == image


def test_write_errors(tmp_path):
    w = ad.io.snp_phased_ancestry(str(tmp_path / "e.snpdat"))
    cal, anc = make_case(5, 2, 2)
    with pytest.raises(RuntimeError, match=r"calldata and ancestries must have shape \(n, 2\*s\)\."):
        w.write(cal[:, :3], anc[:, :3], 2)
    with pytest.raises(RuntimeError, match=r"calldata and ancestries must have shape \(n, 2\*s\)\."):
        w.write(cal, anc[:4], 2)
    with pytest.raises(RuntimeError, match=r"Number of ancestries A must be < 256\."):
        w.write(cal, anc, 256)
    bad = anc.copy()
    bad[2, 1] = 2
    with pytest.raises(RuntimeError, match=r"Detected an ancestry not in the range \[0, A\)\."):
        w.write(cal, bad, 2)
    bad[2, 1] = -1
    with pytest.raises(RuntimeError, match=r"Detected an ancestry not in the range \[0, A\)\."):
        w.write(cal, bad, 2)
    bad = cal.copy()
    bad[4, 0] = 2
    with pytest.raises(RuntimeError, match=r"Detected a non-binary value\."):
        w.write(bad, anc, 2)
    assert not os.path.exists(str(tmp_path / "e.snpdat"))


def test_read_checks(tmp_path):
    path = str(tmp_path / "x.snpdat")
    cal, anc = make_case(5, 2, 2)
    ad.io.snp_phased_ancestry(path).write(cal, anc, 2)
    raw = bytearray(open(path, "rb").read())
    raw[0] = 1 if np.little_endian else 0
    open(path, "wb").write(bytes(raw))
    with pytest.raises(RuntimeError, match="Endianness is inconsistent"):
        ad.io.snp_phased_ancestry(path).read()
    open(path, "wb").write(bytes(raw[:10]))
    with pytest.raises(RuntimeError, match="too small"):
        ad.io.snp_phased_ancestry(path).read()
    with pytest.raises(RuntimeError, match="read_mode"):
        ad.io.snp_phased_ancestry(path, read_mode="pipe")


def test_decoder_under_sanitizers(tmp_path):
    """phased_header / phased_decode / phased_pack as a stand-alone program (tests/native/phased_decode_main.cpp) built with
    -fsanitize=address,undefined: an image written by the codec decodes to numpy's code table, the pair packs to the same
    table, and every damaged copy -- truncations, an outer entry and a haplotype offset past the end, a chunk count that
    overruns, a chunk index past the rows, A = 0 -- ends in the error return with nothing for the sanitizers to report."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required"
    src = os.path.join(ROOT, "tests", "native", "phased_decode_main.cpp")
    exe = str(tmp_path / "phased_decode")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    for n, s, A in [(300, 3, 4), (513, 1, 1), (5, 2, 2)]:
        cal, anc = make_case(n, s, A, seed=1)
        image = str(tmp_path / f"img_{n}.snpdat")
        ad.io.snp_phased_ancestry(image).write(cal, anc, A)
        table = np.where(cal == 1, anc, -1).astype(np.uint8)
        assert set(np.unique(table)) <= set(range(A)) | {255}
        files = {"table": table, "cal": cal, "anc": anc}
        paths = []
        for name, arr in files.items():
            paths.append(str(tmp_path / f"{name}_{n}.bin"))
            np.asfortranarray(arr).ravel(order="F").tofile(paths[-1])
        out = subprocess.run([exe, image] + paths, capture_output=True, text=True)
        assert out.returncode == 0 and "phased_decode: ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
        lines = out.stdout.splitlines()
        assert sum("truncated at" in ln for ln in lines) >= 10
        for what in ("outer[s] past the end", "hap_off[1] past the end", "chunk count byte raised", "chunk_idx past the rows", "A = 0"):
            assert any(ln.startswith(what) and "(decoded)" not in ln for ln in lines), what
        assert "(decoded)" not in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_tile_height_matches_the_header():
    import re

    txt = open(os.path.join(ROOT, "adelie_amd", "csrc", "phased_decode_host.hpp")).read()
    assert int(re.search(r"constexpr int64_t kPhasedTileRows = (\d+);", txt).group(1)) == ad.matrix._PHASED_TILE_ROWS == 4096


def test_generator():
    d = ad.data.snp_phased_ancestry(200, 30, 4, seed=3)
    X, anc = d["X"], d["ancestries"]
    assert X.dtype == np.int8 and anc.dtype == np.int8 and X.shape == anc.shape == (200, 60)
    assert X.flags.f_contiguous and anc.flags.f_contiguous
    assert set(np.unique(X)) == {0, 1} and anc.min() >= 0 and anc.max() == 3 and not anc[X == 0].any()
    cells = X[:, 0::2] + X[:, 1::2]                       # the unphased matrix the recipe draws first
    stored = int((0.25 + 0.05) * 200 * 30)
    assert np.count_nonzero(cells) == stored
    assert np.count_nonzero(cells == 2) == stored - int(0.25 / (0.25 + 0.05) * stored)
    assert np.array_equal(d["groups"], 4 * np.arange(30)) and np.array_equal(d["group_sizes"], np.full(30, 4))
    assert d["penalty"].shape == (30,) and np.isclose(np.sum(d["penalty"] ** 2), 120)
    assert d["y"].shape == (200,) and np.array_equal(d["y"], d["glm"].y)
    cal, anc2, E = altered(d, 4)                          # (the GPU tests' cases: the properties are asserted inside)
    assert cal.shape == X.shape and E.shape == (200, 120) and anc2.max() < 4
    again = ad.data.snp_phased_ancestry(200, 30, 4, seed=3)
    assert np.array_equal(again["X"], X) and np.array_equal(again["y"], d["y"])
    assert ad.data.snp_phased_ancestry(50, 4, 2, glm="binomial", sparsity=0.5, seed=1)["glm"].y.shape == (50,)


def test_abi_tables_name_the_entry_points():
    for name in ("design_create_snp_phased_ancestry", "design_create_snp_phased_calldata", "design_csc_download"):
        assert name in _abi.HIP_SYMBOLS
    assert _abi.ABI_VERSION == 14


def test_front_door_checks_need_no_device():
    assert callable(ad.matrix.snp_phased_ancestry) and callable(ad.matrix.snp_phased_calldata)
    cal, anc = make_case(5, 2, 2)
    with pytest.raises(RuntimeError, match="n_threads must be >= 1"):
        ad.matrix.snp_phased_calldata(cal, anc, 2, n_threads=0)
    with pytest.raises(RuntimeError, match=r"must have shape \(n, 2\*s\)"):
        ad.matrix.snp_phased_calldata(cal[:, :3], anc[:, :3], 2)
