"""The host side of ``matrix.concatenate(..., resident="pieces")`` without a GPU: the rules of
``adelie_amd/csrc/pieces_host.hpp`` (refusals and their messages, the column -> piece map, range splits, the cap, the rule for
16-byte loads) as a stand-alone program under the address and undefined-behaviour sanitizers, the value check of the
``resident`` keyword, and the entry point's place in the ABI list."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import adelie_amd as ad
from adelie_amd import _abi


def test_pieces_rules_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is required (the oracle needs one as well)"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "pieces_main.cpp")
    exe = str(tmp_path / "pieces_host")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "pieces_host: ok" in out.stdout, out.stdout + out.stderr


def test_resident_keyword_is_checked_before_any_piece_is_touched():
    A = np.zeros((4, 2))
    with pytest.raises(ValueError, match="resident"):
        ad.matrix.concatenate([A, A], axis=1, resident="tiles")
    with pytest.raises(ValueError, match="resident"):
        ad.matrix.concatenate([object()], axis=1, resident=None)


def test_pieces_refusals_that_need_no_device():
    A = np.zeros((4, 2))
    with pytest.raises(RuntimeError, match=r'axis must be 1.*resident="pieces"'):
        ad.matrix.concatenate([A, A], axis=0, resident="pieces")
    with pytest.raises(RuntimeError, match=r'9 pieces given, at most 8.*resident="pieces"'):
        ad.matrix.concatenate([A] * 9, axis=1, resident="pieces")
    with pytest.raises(RuntimeError, match=r'piece 1 \(dense\) differs in dtype.*resident="pieces"'):
        ad.matrix.concatenate([A, A.astype(np.float32)], axis=1, resident="pieces")
    with pytest.raises(RuntimeError, match=r'piece 1 \(dense\) differs in its number of rows.*resident="pieces"'):
        ad.matrix.concatenate([A, np.zeros((5, 2))], axis=1, resident="pieces")
    with pytest.raises(RuntimeError, match=r'piece 0 \(multi-response view\).*resident="pieces"'):
        ad.matrix.concatenate([ad.matrix.kronecker_eye(np.ones((4, 1)), 3), A], axis=1, resident="pieces")


def test_entry_point_is_listed_and_the_abi_version_stays():
    assert "design_create_pieces" in _abi.HIP_SYMBOLS
    assert _abi.ABI_VERSION == 14
    assert _abi.S["engine_panel"] == 96
    assert ad.matrix._MAX_PIECES == 8
