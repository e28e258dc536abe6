"""The sparse pinball problems of tests/pinball_sparse_checks.py qualify for the exact checks of test_gpu_pinball_sparse.py: no
decision of the float64 restatement hangs on rounding, so the GPU tests skip nothing.  No GPU here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pinball_checks as pc  # noqa: E402
import pinball_sparse_checks as ps  # noqa: E402


def test_sgen_strikes_entries_out():
    A = ps.sgen(130, 40, 0, 0.3, 0.1)[0]
    full = pc.gen(130, 40, 0, 0.3)[0]
    kept = A != 0
    assert np.array_equal(A[kept], full[kept]) and 0.05 < kept.mean() < 0.15
    assert not A[65].any()  # row m // 2 is emptied
    wide = ps.sgen(130, 300, 1, 0.3, 0.5, True)[0]
    assert np.array_equal(wide[1], pc.gen(130, 300, 1, 0.3)[0][1]) and not wide[65].any()
    assert ps.sgen(3, 1, 0, 1.0, 1.0)[0].all()  # m <= 4: no row is emptied
    E = ps.sedge(0)[0]
    assert not E[5].any() and np.array_equal(E[6], E[7]) and E[6].any()
    assert np.isinf(ps.sedge(0)[3][0]) and np.isinf(ps.sedge(0)[4][1])


@pytest.mark.parametrize("m, d, kappa, pen, density, wide", ps.GRID)
def test_float64_cases_qualify(m, d, kappa, pen, density, wide):
    for seed in ps.SEEDS:
        own = ps.cached_run(m, d, seed, pen, density, wide, kappa, "float64")
        print(f"({m}, {d}) seed {seed}: ns {len(own.screen)}, iters {own.iters}, n_kkt {own.n_kkt}, exit {own.exit}, "
              f"min_gap {own.min_gap:.3e}")
        assert own.error == ""
        assert own.min_gap >= ps.GAP64


def test_float32_cases_qualify():
    """Skipping may not hide a failure: at most one of the nine float32 cases is too close to a decision for an exact check."""
    gaps = {(m, d, s): ps.cached_run(m, d, s, pen, density, wide, kappa, "float64", True).min_gap
            for (m, d, kappa, pen, density, wide) in ps.GRID32 for s in ps.SEEDS}
    print("float64 restatement on the rounded inputs, min_gap:", {k: f"{g:.2e}" for k, g in gaps.items()})
    assert sum(g < ps.GAP32 for g in gaps.values()) <= 1


def test_warm_start_and_edge_cases_qualify():
    m, d, kappa, pen, density, wide = ps.GRID[2]
    own1 = ps.cached_run(m, d, 0, pen, density, wide, kappa, "float64", tol=1e-4)
    A, S, v, pneg, ppos = ps.cached_inputs(m, d, 0, pen, density, wide)
    own2 = pc.solve(A, S, v, pneg, ppos, np.float64, tol=1e-9, warm_start=own1)
    print(f"warm start: coarse min_gap {own1.min_gap:.3e}, fine min_gap {own2.min_gap:.3e}")
    assert own1.min_gap >= ps.GAP64 and own2.min_gap >= ps.GAP64
    for seed in ps.SEEDS:
        own = ps.cached_run("edge", 0, seed, 1.0, ps.EDGE_DENSITY, False, None, "float64")
        print(f"edge seed {seed}: ns {len(own.screen)}, min_gap {own.min_gap:.3e}")
        assert own.error == "" and own.min_gap >= ps.GAP64
