"""The fused model, the device criteria and the native post-processing under the names the reference's drivers import.

``dropin.install(model=True)`` registers the modules built here, so that an UNMODIFIED train.py / test.py / train_fs.py /
test_fs.py lands on this package's classes:

    model.geoformer.geoformer      GeoFormer            (train.py:12, test.py:13)
    model.geoformer.geoformer_fs   GeoFormerFS          (train_fs.py:12, test_fs.py:13)
    criterion                      InstSetCriterion     (train.py:10)
    criterion_fs                   FSInstSetCriterion   (train_fs.py:10)
    util.utils_3d                  load_ids, Instance, get_instances, non_max_suppression_gpu,
                                   matrix_non_max_suppression   (test.py:15, test_fs.py:17, util/eval.py:5)

The classes are thin subclasses of the geoformer_amd.model classes (same ``__name__``, same state_dict): the reference
builds them without arguments and reads its configuration from ``util.config.cfg``, the namespace its drivers import
first and keep writing to (``cfg.resume``, ...), so a facade built without arguments takes THAT object, not a copy.  An
explicit ``cfg`` still wins.  geoformer_amd.model and model.config are not touched.
"""
from __future__ import annotations

import types

import numpy as np

from . import model as _model
from . import postprocess

MODEL_NAMES = ("model.geoformer.geoformer", "model.geoformer.geoformer_fs", "criterion", "criterion_fs", "util.utils_3d")
PARENT_PACKAGES = ("model", "model.geoformer", "util")
_MARK = "__geoformer_amd_facade__"


def reference_cfg():
    """``util.config.cfg`` of the running driver (imported here if the driver has not yet, as the reference's model
    modules do at their top)."""
    import importlib

    try:
        return importlib.import_module("util.config").cfg
    except (ImportError, AttributeError) as e:
        raise RuntimeError("no configuration: the reference's util.config (which reads --config) is not importable "
                           f"({e}); run from the reference tree, or pass cfg") from e


class GeoFormer(_model.GeoFormer):
    def __init__(self, cfg=None):
        super().__init__(cfg if cfg is not None else reference_cfg())


class GeoFormerFS(_model.GeoFormerFS):
    def __init__(self, cfg=None):
        super().__init__(cfg if cfg is not None else reference_cfg())


class InstSetCriterion(_model.InstSetCriterion):
    def __init__(self, cfg=None):
        super().__init__(cfg if cfg is not None else reference_cfg())


class FSInstSetCriterion(_model.FSInstSetCriterion):
    def __init__(self, cfg=None):
        super().__init__(cfg if cfg is not None else reference_cfg())


# ---- util.utils_3d: the host helpers util/eval.py uses (util/utils_3d.py:9-73) -------------------------------------------
def load_ids(filename):
    """One integer per line of a val_gt file -> int64 [N]."""
    with open(filename) as f:
        return np.array(f.read().splitlines(), dtype=np.int64)


class Instance(object):
    """A ground-truth instance of an id array (id = label_id * 1000 + running number): its id, label and point count."""
    instance_id = 0
    label_id = 0
    vert_count = 0
    med_dist = -1
    dist_conf = 0.0

    def __init__(self, mesh_vert_instances, instance_id):
        if instance_id == -1:
            return
        self.instance_id = int(instance_id)
        self.label_id = int(self.get_label_id(instance_id))
        self.vert_count = int(self.get_instance_verts(mesh_vert_instances, instance_id))

    def get_label_id(self, instance_id):
        return int(instance_id // 1000)

    def get_instance_verts(self, mesh_vert_instances, instance_id):
        return (mesh_vert_instances == instance_id).sum()

    def to_dict(self):
        return {"instance_id": self.instance_id, "label_id": self.label_id, "vert_count": self.vert_count,
                "med_dist": self.med_dist, "dist_conf": self.dist_conf}

    def to_json(self):
        import json

        return json.dumps(vars(self), sort_keys=True, indent=4)

    def from_json(self, data):
        self.instance_id, self.label_id = int(data["instance_id"]), int(data["label_id"])
        self.vert_count = int(data["vert_count"])
        if "med_dist" in data:
            self.med_dist, self.dist_conf = float(data["med_dist"]), float(data["dist_conf"])

    def __str__(self):
        return f"({self.instance_id})"


def get_instances(ids, class_ids, class_labels, id2label):
    """{label name: [Instance.to_dict(), ...]} of the instances of ``ids`` (0 = no instance) whose label is one of
    class_ids, in ascending id order."""
    instances = {label: [] for label in class_labels}
    for i in np.unique(ids):
        if i == 0:
            continue
        inst = Instance(ids, i)
        if inst.label_id in class_ids:
            instances[id2label[inst.label_id]].append(inst.to_dict())
    return instances


# ---- the modules -----------------------------------------------------------------------------------------------------------
def build_modules():
    """{import name: module} of MODEL_NAMES (fresh module objects; install() keeps the first set)."""
    def mod(name, **members):
        m = types.ModuleType(name)
        m.__dict__.update(members)
        m.__dict__[_MARK] = True
        m.__doc__ = f"geoformer_amd.reference_names under the reference's import name {name}"
        return m

    return {
        "model.geoformer.geoformer": mod("model.geoformer.geoformer", GeoFormer=GeoFormer),
        "model.geoformer.geoformer_fs": mod("model.geoformer.geoformer_fs", GeoFormerFS=GeoFormerFS),
        "criterion": mod("criterion", InstSetCriterion=InstSetCriterion),
        "criterion_fs": mod("criterion_fs", FSInstSetCriterion=FSInstSetCriterion),
        "util.utils_3d": mod("util.utils_3d", load_ids=load_ids, Instance=Instance, get_instances=get_instances,
                             non_max_suppression_gpu=postprocess.non_max_suppression_gpu,
                             matrix_non_max_suppression=postprocess.matrix_non_max_suppression),
    }


def is_facade(module):
    return bool(getattr(module, _MARK, False))
