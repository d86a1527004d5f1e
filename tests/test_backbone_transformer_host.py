"""The inference voxel transformer's argument checks (bt_forward, csrc/backbone_attn.hip) against the Python predicate
that routes a U-Net level to it (pointops.backbone_transformer_supported).  No GPU: the entry's checks run before its
first HIP call, and an empty batch returns before any launch, so fake device pointers are never dereferenced."""
import ctypes

import pytest

from tests.test_host_logic import lib  # noqa: F401  (the library, built for gfx950 if missing)

OK, INVALID = 0, -1
FAKE = ctypes.c_void_p(0x1000)


def _call(lib, c, n_layers, M=0, n_scenes=0):
    np_ = lib.gf_backbone_transformer_num_params(max(n_layers, 1))
    params = (ctypes.c_void_p * np_)(*([0x1000] * np_))
    return lib.gf_backbone_transformer(FAKE, FAKE, FAKE, n_scenes, M, c, n_layers, params, FAKE, FAKE, None)


def _stack(n_layers=2, d_model=128, heads=4, d_ff=64):
    from geoformer_amd.model.layers import BackboneTransformer

    return BackboneTransformer(d_model=d_model, N=n_layers, heads=heads, d_ff=d_ff)


@pytest.mark.parametrize("c", [0, 8, 400, 512, -16, 24])
def test_rejected_widths(lib, c):
    assert _call(lib, c, 2) == INVALID


@pytest.mark.parametrize("n_layers", [0, 5])
def test_rejected_layer_counts(lib, n_layers):
    assert _call(lib, 16, n_layers) == INVALID


def test_predicate_mirrors_native_checks(lib):
    """For every width 8..512 in steps of 8 and 1..4 layers: the predicate admits exactly what the entry accepts (an
    empty batch: the checks pass and nothing is launched)."""
    from geoformer_amd import pointops

    admitted = []
    for n_layers in (1, 2, 3, 4):
        tr = _stack(n_layers)
        for c in range(8, 513, 8):
            native = _call(lib, c, n_layers) == OK
            assert pointops.backbone_transformer_supported(c, tr) == native, (c, n_layers)
            if native:
                admitted.append(c)
    assert sorted(set(admitted)) == list(range(16, 385, 16))
    # the kernels' fixed shape: d_model 128, 4 heads, d_ff 64, at most BT_MAXL = 4 layers
    assert not pointops.backbone_transformer_supported(64, _stack(5))
    assert not pointops.backbone_transformer_supported(64, _stack(d_model=64))
    assert not pointops.backbone_transformer_supported(64, _stack(heads=8))
    assert not pointops.backbone_transformer_supported(64, _stack(d_ff=128))
