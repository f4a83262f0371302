"""bench.py --dump-outputs: what the last timed step computed, as float64 .npy files -- on the CPU with a stand-in
hierarchy (sampling, dtypes, the size bound, the same files from the same inputs), and on the GPU through a plain
run of a small workload (the result line's keys, no extra legs without --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Hierarchy(object):
    def __init__(self, Ac):
        self.Ac = Ac

    def get_csr(self, level, which):
        assert which == "Ac"
        return self.Ac


def _dump(tmp_path, name, n, nc):
    import torch
    x = torch.linspace(-1.0, 1.0, n, dtype=torch.float64)
    Ac = sp.random(nc, nc, density=min(1.0, 8.0 / nc), format="csr", random_state=1) + sp.identity(nc, format="csr")
    infos = [{"n": n, "ncoarse": 1000}, {"n": 1000, "ncoarse": nc}]
    out = tmp_path / name
    bench.dump_outputs(str(out), _Hierarchy(Ac.tocsr()), x, np.array([1.0, 0.1, 0.01]), 2, infos)
    return out, x.numpy(), Ac.tocoo()


def test_dump_small_outputs_whole(tmp_path):
    out, x, Ac = _dump(tmp_path, "d", 1000, 50)
    files = {f[:-4]: np.load(str(out / f)) for f in os.listdir(str(out))}
    assert all(f.dtype == np.float64 for f in files.values())
    assert "x_index" not in files
    np.testing.assert_array_equal(files["x"], x)
    np.testing.assert_array_equal(files["pcg_residual_history"], [1.0, 0.1, 0.01])
    np.testing.assert_array_equal(files["pcg_iterations"], [2])
    np.testing.assert_array_equal(files["level_dims"], [1000, 1000, 50])
    M = sp.coo_matrix((files["coarse_operator_vals"], (files["coarse_operator_rows"].astype(int),
                                                       files["coarse_operator_cols"].astype(int))), shape=(50, 50))
    assert abs(M - Ac).max() == 0
    r, c = files["coarse_operator_rows"], files["coarse_operator_cols"]
    assert np.all((r[1:] > r[:-1]) | ((r[1:] == r[:-1]) & (c[1:] > c[:-1])))       # (row, col)-sorted


def test_dump_large_outputs_sampled_and_repeatable(tmp_path):
    n = 3 * bench.DUMP_SAMPLE + 7
    out, x, _ = _dump(tmp_path, "a", n, 600)
    out2, _, _ = _dump(tmp_path, "b", n, 600)
    idx = np.load(str(out / "x_index.npy"))
    assert idx.size == bench.DUMP_SAMPLE and np.all(np.diff(idx) > 0) and idx[-1] < n
    np.testing.assert_array_equal(np.load(str(out / "x.npy")), x[idx.astype(np.int64)])
    total = 0
    for f in os.listdir(str(out)):
        a, b = np.load(str(out / f)), np.load(str(out2 / f))
        np.testing.assert_array_equal(a, b)
        total += os.path.getsize(str(out / f))
    assert total <= 64 * 2 ** 20


@pytest.mark.gpu
def test_plain_bench_run_dumps_outputs(tmp_path):
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--n", "32", "--levels", "2", "--dump-outputs", str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["steps"] == 2 and res["ms_per_step"] > 0 and res["unit"] == "DoF/s" and res["dtype"] == "f64"
    assert res["value"] > 0 and res["higher_is_better"] is True
    assert "roofline" not in res and "cpu_baseline" not in res          # the extra legs belong to --full
    x = np.load(str(out / "x.npy"))
    assert x.dtype == np.float64 and x.size == res["config"]["dofs"] and np.all(np.isfinite(x))
    assert int(np.load(str(out / "pcg_iterations.npy"))[0]) == res["config"]["pcg_iterations"]
    np.testing.assert_array_equal(np.load(str(out / "level_dims.npy")), res["config"]["level_dims"])
