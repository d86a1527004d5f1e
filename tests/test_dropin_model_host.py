"""CPU: dropin.install(model=True) -- a test.py / train.py-shaped import sequence lands on this package's fused model,
device criteria and native NMS (geoformer_amd.reference_names).  The driver's tree is a skeleton in tmp_path: an empty
util package with a stand-in util/config.py and NO model/ directory, so the parent packages of the model names are
stand-ins too.  With the reference tree present (build container only) its four unmodified drivers are imported in a
child process."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from tests.dropin_model_tree import driver_tree  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
REF = os.environ.get("GEOFORMER_REFERENCE", "/root/reference")
NAMES = ("model.geoformer.geoformer", "model.geoformer.geoformer_fs", "criterion", "criterion_fs", "util.utils_3d")


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def test_test_py_import_sequence_lands_on_the_facades(driver_tree):
    import geoformer_amd.model as gm
    from geoformer_amd import dropin, postprocess, reference_names

    driver_tree("test_geoformer_scannet.yaml")
    mods = dropin.install(model=True)
    assert set(mods) == {"spconv", "PG_OP", "pointnet2._ext", "faiss", *NAMES}
    assert all(sys.modules[n] is mods[n] for n in NAMES)
    # test.py:7-15
    from util.config import cfg
    from model.geoformer.geoformer import GeoFormer
    from util.utils_3d import load_ids, non_max_suppression_gpu, matrix_non_max_suppression
    import util.utils_3d as util_3d  # util/eval.py:5

    assert GeoFormer is reference_names.GeoFormer and GeoFormer.__name__ == "GeoFormer"
    assert non_max_suppression_gpu is postprocess.non_max_suppression_gpu
    assert matrix_non_max_suppression is postprocess.matrix_non_max_suppression
    assert load_ids is reference_names.load_ids and util_3d.get_instances is reference_names.get_instances
    assert not os.path.exists(os.path.join(sys.path[0], "model"))  # the parents are stand-ins
    m = GeoFormer()
    assert isinstance(m, gm.GeoFormer) and m.cfg is cfg
    cfg.resume = "later.pth"  # what a driver sets after the import stays visible
    assert m.cfg.resume == "later.pth"
    direct = gm.GeoFormer(gm.load_config("test_geoformer_scannet.yaml"))
    assert _shapes(m) == _shapes(direct) and list(m.state_dict()) == list(direct.state_dict())
    other = gm.load_config("test_geoformer_scannet.yaml")
    assert GeoFormer(other).cfg is other  # an explicit cfg wins
    # train.py:10
    from criterion import InstSetCriterion

    c = InstSetCriterion()
    assert isinstance(c, gm.InstSetCriterion) and c.cfg is cfg and InstSetCriterion.__name__ == "InstSetCriterion"
    assert _shapes(c) == _shapes(gm.InstSetCriterion(other))
    # a second call changes nothing
    again = dropin.install(model=True)
    assert all(again[n] is mods[n] for n in NAMES)
    assert gm.GeoFormer is not GeoFormer and gm.cfg is not cfg  # geoformer_amd.model is untouched


def test_few_shot_names(driver_tree):
    import geoformer_amd.model as gm
    from geoformer_amd import dropin

    driver_tree("test_geoformer_fs_scannet.yaml")
    dropin.install(model=True)
    from util.config import cfg
    from criterion_fs import FSInstSetCriterion  # train_fs.py:10-12
    from model.geoformer.geoformer_fs import GeoFormerFS
    from util.utils_3d import load_ids, matrix_non_max_suppression  # noqa: F401  test_fs.py:17

    m = GeoFormerFS()
    assert isinstance(m, gm.GeoFormerFS) and m.cfg is cfg and GeoFormerFS.__name__ == "GeoFormerFS"
    direct = gm.GeoFormerFS(gm.load_config("test_geoformer_fs_scannet.yaml"))
    assert _shapes(m) == _shapes(direct) and list(m.state_dict()) == list(direct.state_dict())
    c = FSInstSetCriterion()
    assert isinstance(c, gm.FSInstSetCriterion) and c.cfg is cfg
    assert _shapes(c) == _shapes(gm.FSInstSetCriterion(direct.cfg))


def test_facade_forward_reproduces_the_reference_golden(driver_tree, oracle):
    """The checks of tests/golden/route_a_check.py on the model's outputs: floats to 1e-4 abs, integer fields identical."""
    from geoformer_amd import dropin, scene
    from oracle import cpu_backend
    from tests.util import synthetic_state_dict

    driver_tree("test_geoformer_scannet.yaml")
    dropin.install(model=True)
    from model.geoformer.geoformer import GeoFormer

    z = np.load(os.path.join(G, "geoformer_s8k_eval.npz"))
    m = GeoFormer()  # (imports util.config itself, as the reference's model module does)
    assert m.cfg is sys.modules["util.config"].cfg
    m.load_state_dict(synthetic_state_dict(m.state_dict(), int(z["weight_seed"])))
    m.eval()
    batch = scene.make_batch([scene.make_small_scene(int(z["scene_points"]), int(z["scene_seed"]))])
    np.random.seed(int(z["numpy_seed"]))
    with cpu_backend.installed(), torch.no_grad():
        out = m(batch, 300, training=False)
    assert np.abs(out["semantic_scores"].numpy() - z["semantic_scores"]).max() < 1e-4
    assert (out["fg_idxs"].numpy() == z["fg_idxs"]).all()
    assert (m.last_sampling_indices.numpy() == z["sampling_indices"]).all()
    mp = out["mask_predictions"][-1]
    assert np.abs(mp["cls_logits"].numpy() - z["cls_logits"]).max() < 1e-4
    assert np.abs(mp["mask_logits"][0].numpy()[::8, ::4] - z["mask_logits_sub"]).max() < 1e-4
    cls_final, scores_final, _ = out["proposal_scores"]
    assert (cls_final.numpy() == z["proposal_cls"]).all()
    assert np.abs(scores_final.numpy() - z["proposal_scores"]).max() < 1e-4


def test_utils_3d_host_helpers(tmp_path):
    """The ground-truth layout evaluation.py's matching works on (instance_id = label_id * 1000 + k)."""
    from geoformer_amd.reference_names import Instance, get_instances, load_ids

    ids = np.array([0, 3001, 3001, 5002, 0, 3003, 5002, 5002, 39001], np.int64)
    f = tmp_path / "scene.txt"
    f.write_text("\n".join(str(i) for i in ids) + "\n")
    got = load_ids(str(f))
    assert got.dtype == np.int64 and (got == ids).all()
    inst = Instance(ids, 5002)
    assert (inst.instance_id, inst.label_id, inst.vert_count) == (5002, 5, 3)
    assert inst.to_dict() == {"instance_id": 5002, "label_id": 5, "vert_count": 3, "med_dist": -1, "dist_conf": 0.0}
    assert Instance(ids, -1).vert_count == 0
    res = get_instances(ids, [3, 5], ["cabinet", "chair"], {3: "cabinet", 5: "chair"})
    assert list(res) == ["cabinet", "chair"]
    assert [(g["instance_id"], g["vert_count"]) for g in res["cabinet"]] == [(3001, 2), (3003, 1)]
    assert [(g["instance_id"], g["vert_count"]) for g in res["chair"]] == [(5002, 3)]  # 39001: not an evaluated class
    assert all(type(v) is int for g in res["cabinet"] for k, v in g.items() if k != "dist_conf")


def test_install_after_the_drivers_import_raises(driver_tree):
    import types

    from geoformer_amd import dropin

    driver_tree("test_geoformer_scannet.yaml")
    for pkg in ("model", "model.geoformer"):
        sys.modules[pkg] = types.ModuleType(pkg)
        sys.modules[pkg].__path__ = []
    sys.modules["model.geoformer.geoformer"] = types.ModuleType("model.geoformer.geoformer")  # somebody else's
    with pytest.raises(RuntimeError, match=r"model\.geoformer\.geoformer\b"):
        dropin.install(model=True)
    assert "criterion" not in sys.modules and "util.utils_3d" not in sys.modules  # nothing half-installed


def test_driver_tree_put_on_the_path_after_install(driver_tree, tmp_path):
    from geoformer_amd import dropin

    dropin.install(model=True)  # no util package anywhere yet: a stand-in
    assert not hasattr(sys.modules["util"], "__file__")
    driver_tree("test_geoformer_scannet.yaml")
    from util.config import cfg
    from model.geoformer.geoformer import GeoFormer  # noqa: F401

    assert cfg.TEST_NMS_THRESH == 0.3 and sys.modules["util.config"].__file__.startswith(str(tmp_path))


def test_plain_install_is_unchanged(driver_tree):
    from geoformer_amd import dropin

    driver_tree("test_geoformer_scannet.yaml")
    assert set(dropin.install()) == set(dropin.install(model=False)) == {"spconv", "PG_OP", "pointnet2._ext", "faiss"}
    assert not any(n in sys.modules for n in NAMES)


_CHILD = """
import os, sys, types
sys.argv = ["driver", "--config", os.path.join({ref!r}, "config", {yaml!r})]
os.chdir({ref!r})
sys.path.insert(0, {ref!r})  # what `python test.py` started in the reference tree gives
sys.path.insert(0, {root!r})
import torch
import geoformer_amd.dropin as dropin
mods = dropin.install(model=True)
for dummy in ("trimesh", "tensorboardX"):
    sys.modules.setdefault(dummy, types.ModuleType(dummy))
sys.modules["tensorboardX"].SummaryWriter = object
assert os.path.samefile(os.path.dirname(sys.modules["util"].__file__), os.path.join({ref!r}, "util"))
# the reference's datasets/ has no __init__.py: an installed distribution of that name would win over it
sys.modules["datasets"] = types.ModuleType("datasets")
sys.modules["datasets"].__path__ = [os.path.join({ref!r}, "datasets")]
import geoformer_amd.model as gm
from geoformer_amd import postprocess, reference_names as rn
import util.config
{body}
import util.eval, util.utils_3d
assert util.eval.util_3d is mods["util.utils_3d"]
assert os.path.samefile(os.path.dirname(util.eval.__file__), os.path.join({ref!r}, "util"))
print("child ok")
"""
_BODY = {
    "test_geoformer_scannet.yaml": """
import test, train
assert test.GeoFormer is rn.GeoFormer and train.GeoFormer is rn.GeoFormer
assert train.InstSetCriterion is rn.InstSetCriterion
assert test.non_max_suppression_gpu is postprocess.non_max_suppression_gpu
assert test.matrix_non_max_suppression is postprocess.matrix_non_max_suppression
assert test.cfg is util.config.cfg
c = train.InstSetCriterion()
assert isinstance(c, gm.InstSetCriterion) and c.cfg is util.config.cfg
""",
    "test_geoformer_fs_scannet.yaml": """
import test_fs, train_fs
assert test_fs.GeoFormerFS is rn.GeoFormerFS and train_fs.GeoFormerFS is rn.GeoFormerFS
assert train_fs.FSInstSetCriterion is rn.FSInstSetCriterion
assert test_fs.matrix_non_max_suppression is postprocess.matrix_non_max_suppression
c = train_fs.FSInstSetCriterion()
assert isinstance(c, gm.FSInstSetCriterion) and c.cfg is util.config.cfg
""",
}


@pytest.mark.parametrize("yaml", list(_BODY))
def test_unmodified_reference_drivers_import_the_facades(yaml):
    if not os.path.isfile(os.path.join(REF, "test.py")):
        pytest.skip("needs the reference tree (build container only)")
    code = _CHILD.format(ref=REF, root=ROOT, yaml=yaml, body=textwrap.dedent(_BODY[yaml]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
