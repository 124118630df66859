"""The call traces of the reference's own entry scripts, executed UNMODIFIED against cape_amd (SURVEY 7.3 / INTEGRATION.md
section 1), checked on the host.

`run_simple_demo.py` and `main.py --mode train` (the shipped affine-nz64 configuration; `lib/models.py` replaced by the one-file
shim INTEGRATION.md prescribes; packages the image lacks answered by tests/dropin_stubs (configargparse / trimesh / smplx /
psbody) and the numpy TF1 shim; main.py's dataset from tests/entry_synth.py) were run with recorders in place of the entry points
that need the device.  What the scripts handed cape_amd -- constructor keywords, method calls, every array passed in -- is
committed as tests/golden/run_simple_demo_trace.npz and tests/golden/main_train_trace.npz.  The reference's sources are not part
of this repository, so the suite works from these fixtures alone:

  * HERE (CPU, this file): the recorded calls follow the scripts' flow with arrays of the documented shapes, the operators the
    scripts' loader handed the constructor are the ones cape_amd ships, cape_amd's REAL constructor accepts the recorded keywords,
    and tests/entry_synth.py rebuilds the BodyData main.py loaded.
  * ON THE GPU (tests/test_gpu_dropin_api.py::test_reference_demo_trace_on_device and
    ::test_reference_main_train_trace_on_device): the same traces are replayed against the real model, the training one with a
    real fit.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONFIG = "configs/CAPE-affineconv_nz64_pose32_clotype32_male.yaml"


def _trace(fn):
    g = np.load(os.path.join(GOLDEN, fn))
    return g, json.loads(str(g["meta"]))


def _model_from_trace(meta, tmp_path):
    """cape_amd's real constructor (host side: no device needed) on the shipped operators, with the recorded keywords."""
    from cape_amd.load_data import load_graph_mtx
    from cape_amd.models import CAPE
    L, D, U, p, L_d, D_d, _ = load_graph_mtx(None, load_for_demo=True)
    ops = dict(L=L, D=D, U=U, L_d=L_d, D_d=D_d)
    for k, mats in ops.items():
        assert [list(m.shape) for m in mats] == meta["operator_shapes"][k], k
        assert [int(m.nnz) for m in mats] == meta["operator_nnz"][k], k
    assert meta["ctor"]["p"] == list(p)
    return CAPE(**ops, **dict(meta["ctor"], project_dir=str(tmp_path)))


def _check_affine_nz64_ctor(c):
    assert c["F"] == [64, 64, 128, 128, 256, 256, 512, 512] and c["K"] == [2] * 8 and c["affine"] is True
    assert c["cond_dim"] == 126 and c["batch_size"] == 16 and c["p"] == [6890, 6890, 3445, 3445, 1723, 1723, 862, 862, 862]


def test_run_simple_demo_trace_fits_the_host_side(tmp_path):
    g, meta = _trace("run_simple_demo_trace.npz")
    calls = meta["calls"]
    assert meta["config"] == CONFIG
    assert calls[0] == ["build_graph", 6890, 3, "demo"]
    assert [c[0] for c in calls] == ["build_graph", "encode_only_condition"] + ["decode"] * 4
    assert g["eoc_cond"].shape == (4, 126) and g["eoc_cond2"].shape == (4, 4)
    assert all(g["dec%d_z" % i].shape == (3, 64 + 32 + 32) and g["dec%d_cond" % i].shape == (1, 32) for i in range(4))
    assert g["train_mean"].shape == g["train_std"].shape == (6890, 3) and (g["train_std"] > 0).all()
    _check_affine_nz64_ctor(meta["ctor"])
    assert meta["operator_shapes"]["L"][0] == [6890, 6890] and meta["operator_shapes"]["L_d"][-1] == [431, 431]
    model = _model_from_trace(meta, tmp_path)
    assert (model.input_num_verts, model.nn_input_channel) == tuple(calls[0][1:3])
    assert g["dec0_z"].shape[1] == int(model.nz) + model.nz_cond + model.nz_cond2


def test_main_train_trace_fits_the_host_side(tmp_path):
    """main.py --mode train: BodyData -> generate_transform_matrices -> CAPE(**params) -> build_graph('train') -> fit ->
    build_graph('demo') -> demo_full.test_model -> demo_full.run."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import entry_synth
    finally:
        sys.path.pop(0)
    g, meta = _trace("main_train_trace.npz")
    calls, n_pose = meta["calls"], meta["n_pose"]
    assert meta["argv"][:3] == ["main.py", "--config", CONFIG] and meta["argv"][meta["argv"].index("--mode") + 1] == "train"
    assert [c[0] for c in calls] == (["build_graph", "fit", "build_graph", "predict", "encode_only_condition"] + ["decode"] * n_pose
                                     + ["encode_only_condition"] + ["decode"] * 4)         # main.py:91-101, demos.py:47-219,329-331
    assert calls[0] == ["build_graph", 6890, 3, "train"] and calls[2] == ["build_graph", 6890, 3, "demo"]
    assert calls[1] == ["fit", "bodydata"] and calls[3][-1] == "test"
    c = meta["ctor"]
    _check_affine_nz64_ctor(c)
    assert c["num_epochs"] == 1 and c["decay_steps"] == 2 * entry_synth.N_TRAIN / 16                  # main.py:69-70
    # the BodyData the script built from the synthetic dataset files is what entry_synth rebuilds (and the device half trains on)
    bodydata = entry_synth.Wrapper()
    for k in entry_synth.Wrapper.FIELDS:
        assert entry_synth.summaries_match(entry_synth.summary(getattr(bodydata, k)), meta["summaries"]["bodydata." + k]), k
    for tag, arr in zip(calls[3][1:4], (bodydata.vertices_test, bodydata.cond1_test, bodydata.cond2_test)):
        assert entry_synth.summaries_match(entry_synth.summary(arr), meta["summaries"][tag]), tag
    assert g["eoc0_cond"].shape == (n_pose, 126) and g["eoc1_cond"].shape == (4, 126) and g["eoc1_cond2"].shape == (4, 4)
    assert all(g["dec%d_z" % i].shape == (2, 128) and g["dec%d_cond" % i].shape == (1, 32) for i in range(n_pose + 4))
    model = _model_from_trace(meta, tmp_path)
    assert (model.input_num_verts, model.nn_input_channel) == tuple(calls[0][1:3]) and model.num_epochs == 1
    assert g["dec0_z"].shape[1] == int(model.nz) + model.nz_cond + model.nz_cond2
