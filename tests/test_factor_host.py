"""Host-side logic of matrix.one_hot / matrix.interaction: intr_map -> pairs and (levels, pairs) -> block offsets.
Restates reference matrix.py:876-904 and init_outer (matrix_naive_interaction.ipp:10-26).  No GPU needed."""
import warnings

import numpy as np
import pytest

from adelie_amd import matrix as M

LEVELS = np.array([0, 1, 3, 0, 70, 2])


def _pairs(intr_map, d):
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # an in-range map must not warn
        return [tuple(int(x) for x in r) for r in M._interaction_pairs(intr_map, d)]


def test_pairs_none_means_every_column():
    assert _pairs({0: None}, 4) == [(0, 1), (0, 2), (0, 3)]


def test_pairs_sorted_unique_no_self_no_reversed_duplicate():
    assert _pairs({2: [0, 0, 2, 3], 0: [2]}, 4) == [(0, 2), (2, 3)]


def test_pairs_keep_key_first():
    # the pair is (key, value), not (min, max): block layout depends on which column is A
    assert _pairs({3: [1]}, 4) == [(3, 1)]
    out = M._interaction_pairs({0: None, 2: [4, 5], 4: [3]}, 6)
    assert out.shape == (8, 2) and out.dtype.kind == "i"
    assert [tuple(r) for r in out] == [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (2, 4), (2, 5), (4, 3)]


def test_pairs_errors_are_the_references():
    with pytest.raises(ValueError, match=r"^intr_map must be non-empty\.$"):
        M._interaction_pairs({}, 4)
    with pytest.raises(ValueError, match=r"^No valid pairs exist\. There must be at least one valid pair\.$"):
        M._interaction_pairs({1: [1]}, 4)


def test_pairs_out_of_range_warns():
    with pytest.warns(UserWarning, match=r"key not in range \[0,4\): 7\."):
        M._interaction_pairs({7: [1]}, 4)
    with pytest.warns(UserWarning, match=r"value not in range \[0,4\): 9\."):
        M._interaction_pairs({0: [9]}, 4)
    with pytest.warns(UserWarning, match=r"value not in range \[0,4\): -1\."):
        M._interaction_pairs({0: [-1, 1]}, 4)


def test_one_hot_offsets():
    outer = M._factor_outer(LEVELS)
    sizes = [1, 1, 3, 1, 70, 2]  # continuous: 1 column; one level: 1 column; L levels: L columns
    assert outer.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    assert outer[-1] == 78
    assert M._factor_outer(np.array([-3, 0])).tolist() == [0, 1, 2]  # any non-positive level count is continuous


@pytest.mark.parametrize("pair, size", [
    ((0, 3), 2 * 2 - 1),   # cont, cont: [Z_i, Z_j, Z_i Z_j]
    ((2, 0), 3 * 2),       # disc 3, cont
    ((0, 2), 2 * 3),       # cont, disc 3
    ((2, 5), 3 * 2),       # disc 3, disc 2
    ((2, 4), 3 * 70),      # a block of 210 columns
    ((1, 3), 1 * 2),       # one level, cont
    ((1, 5), 1 * 2),       # one level, disc 2
    ((4, 1), 70 * 1),
])
def test_interaction_block_size(pair, size):
    outer = M._factor_outer(LEVELS, np.array([pair]))
    assert outer.tolist() == [0, size]


def test_interaction_offsets_accumulate():
    pairs = M._interaction_pairs({0: None, 2: [4, 5], 4: [3]}, 6)
    outer = M._factor_outer(LEVELS, pairs)
    sizes = []
    for i, j in pairs:
        l0, l1 = LEVELS[i], LEVELS[j]
        both_cont = int(l0 <= 0 and l1 <= 0)
        sizes.append((2 if l0 <= 0 else l0) * (2 if l1 <= 0 else l1) - both_cont)
    assert sizes == [2, 6, 3, 140, 4, 210, 6, 140]
    groups, group_sizes, P = outer[:-1], np.diff(outer), outer[-1]
    assert group_sizes.tolist() == sizes and P == sum(sizes) == 511
    assert groups.tolist() == np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    assert outer.dtype == np.int64


def test_public_names_exist():
    import adelie_amd as ad

    assert callable(ad.matrix.one_hot) and callable(ad.matrix.interaction)
    with pytest.raises(RuntimeError, match="n_threads must be >= 1"):
        ad.matrix.one_hot(np.zeros((3, 2), order="F"), n_threads=0)
    with pytest.raises(ValueError, match="intr_map must be non-empty"):
        ad.matrix.interaction(np.zeros((3, 2), order="F"), {})
