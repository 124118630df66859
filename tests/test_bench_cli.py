"""bench.py's command line: a plain run measures the headline only, ``--dump-outputs DIR`` writes what the last timed step
computed (CPU: the writer on a stand-in runner; GPU: the whole plain run)."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP_LIMIT = 64 << 20


def _dumped(d):
    return {fn[:-4]: np.load(os.path.join(d, fn)) for fn in sorted(os.listdir(d)) if fn.endswith(".npy")}


def test_dump_outputs_writes_losses_and_a_fixed_sample_of_the_buckets(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    n_g, n_d = bench.DUMP_SAMPLE * 3 + 17, 1000
    st_g = dict(flat=torch.arange(n_g, dtype=torch.float32), flat_grad=-torch.arange(n_g, dtype=torch.float32),
                m=torch.full((n_g,), 0.5))
    st_d = dict(flat=torch.ones(n_d), flat_grad=torch.zeros(n_d), m=torch.zeros(n_d), v=torch.ones(n_d))
    runner = types.SimpleNamespace(model=types.SimpleNamespace(_opt_state=dict(g=st_g, d=st_d)),
                                   losses=dict(loss_g=torch.tensor(1.25), recon=torch.tensor(0.5)), _groups=lambda: ('g', 'd'))
    bench.dump_outputs(runner, str(tmp_path / "a"))
    bench.dump_outputs(runner, str(tmp_path / "b"))
    a, b = _dumped(str(tmp_path / "a")), _dumped(str(tmp_path / "b"))
    assert set(a) == {"loss_g", "recon", "variables_g", "gradients_g", "optimizer_m_g",
                      "variables_d", "gradients_d", "optimizer_m_d", "optimizer_v_d"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["loss_g"] == 1.25 and a["recon"] == 0.5 and a["loss_g"].dtype == np.float64
    # the long bucket: a sorted sample without repeats, the same indices for every buffer and every run
    idx = a["variables_g"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE and (np.diff(idx) > 0).all() and idx[-1] < n_g
    assert np.array_equal(a["gradients_g"], -a["variables_g"]) and (a["optimizer_m_g"] == 0.5).all()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # a short bucket is written whole
    assert len(a["variables_d"]) == n_d and (a["optimizer_v_d"] == 1).all()
    assert sum(os.path.getsize(os.path.join(str(tmp_path / "a"), k + ".npy")) for k in a) <= DUMP_LIMIT


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_the_last_step(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: K timed steps, the headline fields, none of the side
    measurements of --full, and the last step's losses / variables / gradients / optimiser state under DIR."""
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["unit"] == "meshes/s" and res["higher_is_better"] is True
    assert res["dtype"] == "f32" and res["ms_per_step"] > 0
    assert abs(res["value"] - 16 * 1e3 / res["ms_per_step"]) <= 1e-3 * res["value"]
    assert res["roofline"] is None and res["cpu_baseline"] is None
    assert not {"kernels", "exact_fp32_mfma", "bf16x6_split", "extra_configs", "scaling_model"} & set(res)
    d = _dumped(out)
    assert {"loss_g", "recon", "variables_g", "gradients_g", "optimizer_m_g"} <= set(d)
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in d.values())
    assert abs(float(d["loss_g"]) - res["config"]["final_loss_g"]) <= 1e-6 * abs(res["config"]["final_loss_g"])
    assert np.abs(d["gradients_g"]).max() > 0 and np.abs(d["optimizer_m_g"]).max() > 0
    assert sum(os.path.getsize(os.path.join(out, k + ".npy")) for k in d) <= DUMP_LIMIT
