"""Shared by tests/test_phased_host.py and tests/test_gpu_phased.py: the numpy definition of the phased-ancestry matrix and
the generator's data altered so that every case holds the cells a build can get wrong."""
import numpy as np


def expand(calldata, ancestries, A):
    """X[i, j*A + a] = sum_k 1[calldata[i, 2j+k] == 1 and ancestries[i, 2j+k] == a], int8."""
    n, s = calldata.shape[0], calldata.shape[1] // 2
    E = np.zeros((n, s * A), dtype=np.int8)
    for j in range(s):
        for k in range(2):
            for a in range(A):
                E[:, j * A + a] += (calldata[:, 2 * j + k] == 1) & (ancestries[:, 2 * j + k] == a)
    return E


def altered(data, A, seed=0):
    """``(calldata, ancestries)`` of ``data.snp_phased_ancestry`` output, altered to hold, as far as (n, s, A) allow:

    * SNP 0 without a mutation;
    * with s >= 3 and A > 1, ancestry 0 unused at SNP 1 (an empty column inside a SNP that has mutations);
    * row 0 with both haplotypes mutated in ancestry A - 1 (one entry of value 2), at SNP 1 when s >= 3, else at the last SNP;
    * with A > 1, row min(1, n - 1) with its haplotypes mutated in ancestries 0 and A - 1 at the last SNP (two entries of 1);
    * a mutation in the last row (second haplotype of the last SNP);
    * ``ancestries`` filled with in-range garbage wherever the call is 0.

    The properties are asserted on the expansion before the arrays are returned."""
    cal, anc = np.array(data["X"], dtype=np.int8, order="F"), np.array(data["ancestries"], dtype=np.int8, order="F")
    n, s = cal.shape[0], cal.shape[1] // 2
    assert s >= 2 and (n > 1 or s >= 3)
    L = s - 1
    cal[:, 0:2] = 0
    v2 = 1 if s >= 3 else L
    cal[0, 2 * v2:2 * v2 + 2] = 1
    anc[0, 2 * v2:2 * v2 + 2] = A - 1
    r = min(1, n - 1)
    if A > 1:
        cal[r, 2 * L:2 * L + 2] = 1
        anc[r, 2 * L:2 * L + 2] = (0, A - 1)
    if n - 1 != r or A == 1:
        cal[n - 1, 2 * L + 1] = 1
        anc[n - 1, 2 * L + 1] = A - 1
    if s >= 3 and A > 1:
        blk = anc[:, 2:4]
        blk[(cal[:, 2:4] == 1) & (blk == 0)] = A - 1
    rng = np.random.RandomState(seed)
    noise = rng.randint(0, A, size=anc.shape).astype(np.int8)
    anc[cal == 0] = noise[cal == 0]

    E = expand(cal, anc, A)
    assert not E[:, :A].any()
    assert E[0, v2 * A + A - 1] == 2 and E[n - 1].any()
    if A > 1:
        assert E[r, L * A] == 1 and E[r, L * A + A - 1] == 1
    if s >= 3 and A > 1:
        assert not E[:, A].any() and E[:, A:2 * A].any()
    return cal, anc, E
