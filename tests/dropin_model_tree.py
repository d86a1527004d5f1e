"""Fixture of the install(model=True) tests: the import state of a driver started in a skeleton of the reference's tree."""
import sys

import pytest


def _is_driver_name(k):
    return k in ("model", "util", "criterion", "criterion_fs") or k.startswith(("model.", "util."))


@pytest.fixture
def driver_tree(tmp_path):
    """sys.modules / sys.path as a driver started in the skeleton tree would see them; restored afterwards."""
    saved_mods = {k: v for k, v in sys.modules.items() if _is_driver_name(k)}
    saved_path = list(sys.path)
    for k in saved_mods:
        del sys.modules[k]

    def make(yaml):
        (tmp_path / "util").mkdir(exist_ok=True)
        (tmp_path / "util" / "__init__.py").write_text("")
        (tmp_path / "util" / "config.py").write_text(
            "from geoformer_amd.model.config import load_config\n\ncfg = load_config(%r)\n" % yaml)
        sys.path.insert(0, str(tmp_path))

    yield make
    for k in [k for k in sys.modules if _is_driver_name(k)]:
        del sys.modules[k]
    sys.modules.update(saved_mods)
    sys.path[:] = saved_path
