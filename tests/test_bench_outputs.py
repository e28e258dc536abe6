"""bench.py --dump-outputs: what the timed path hands its caller, as float .npy files within the size budget."""
import os
import sys

import numpy as np

import adelie_amd as ad
from adelie_amd.cv import CVGrpnetResult
from util import make_gaussian

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _path(oracle):
    d = make_gaussian(300, 50, seed=0)
    st = ad.grpnet(oracle.dense(d["X"]), ad.glm.gaussian(d["y"]), early_exit=False, progress_bar=False)
    assert st.error == ""
    return st


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_grpnet_whole(oracle, tmp_path):
    st = _path(oracle)
    bench.dump_outputs(str(tmp_path), 2, st, np.float64)
    out = _load(tmp_path)
    assert sorted(out) == ["betas", "devs", "intercepts", "lmdas"]
    assert all(a.dtype == np.float64 for a in out.values())
    np.testing.assert_array_equal(out["betas"], st.betas.toarray())
    np.testing.assert_array_equal(out["lmdas"], st.lmdas)
    np.testing.assert_array_equal(out["intercepts"], st.intercepts)
    np.testing.assert_array_equal(out["devs"], st.devs)


def test_dump_grpnet_sampled_within_budget(oracle, tmp_path, monkeypatch):
    st = _path(oracle)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 20_000)
    bench.dump_outputs(str(tmp_path), 2, st, np.float32)
    out = _load(tmp_path)
    assert sorted(out) == ["betas_sample", "betas_sample_columns", "devs", "intercepts", "lmdas"]
    assert all(a.dtype == np.float32 for a in out.values())
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= 20_000
    cols = out["betas_sample_columns"].astype(int)
    assert 0 < len(cols) < st.betas.shape[1] and np.all(np.diff(cols) > 0)
    np.testing.assert_array_equal(out["betas_sample"], st.betas.toarray()[:, cols].astype(np.float32))
    # the sample is fixed: a second dump picks the same columns
    d2 = tmp_path / "again"
    bench.dump_outputs(str(d2), 2, st, np.float32)
    np.testing.assert_array_equal(_load(d2)["betas_sample_columns"], out["betas_sample_columns"])


def test_dump_cv(tmp_path):
    rng = np.random.default_rng(0)
    losses = rng.random((8, 20))
    res = CVGrpnetResult(lmdas=np.logspace(0, -1, 20), losses=losses, avg_losses=losses.mean(0),
                         best_idx=int(np.argmin(losses.mean(0))))
    bench.dump_outputs(str(tmp_path), 5, res, np.float64)
    out = _load(tmp_path)
    assert sorted(out) == ["avg_losses", "best_idx", "lmdas", "losses"]
    np.testing.assert_array_equal(out["losses"], losses)
    assert out["best_idx"].tolist() == [res.best_idx]
