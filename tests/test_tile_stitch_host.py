"""CPU: the statement of the tile stitch (postprocess.stitch_tiles_host) against the rule restated point by point, bit
patterns compared; what the two modes share and where they part; hand-built tables; the errors; the stitch= keyword of
the loops, the command line and the derived binding."""
import numpy as np
import pytest
import torch

from tests.tile_stitch_cases import (MODES, brute_force, edge_plan, gap_plan, hand_plan, random_scores, same_bits,
                                     uniform_plan)


@pytest.fixture(scope="module")
def plan33():
    plan = uniform_plan()
    assert plan.T == 9 and plan.N == 4000
    return plan


def _counts(plan):
    return (plan.tile_of >= 0).sum(1)


@pytest.mark.parametrize("C", [1, 13, 20])
@pytest.mark.parametrize("mode", MODES)
def test_statement_equals_the_rule_point_by_point(plan33, C, mode):
    from geoformer_amd import postprocess

    scores = random_scores(plan33, C, seed=3)
    got = postprocess.stitch_tiles_host(plan33, scores, mode)
    assert same_bits(got, brute_force(plan33, scores, mode, C))


def test_tile_plan_counts_are_1_2_and_4(plan33):
    counts = np.bincount(_counts(plan33), minlength=5)
    print(f"points in 1 / 2 / 3 / 4 tiles: {counts[1:].tolist()}")
    assert counts[0] == 0 and counts[3] == 0 and counts[1] > 0 and counts[2] > 0 and counts[4] > 0


def test_modes_agree_in_one_tile_and_part_on_shared_points(plan33):
    from geoformer_amd import evaluation, postprocess

    scores = random_scores(plan33, 20, seed=3)
    core = postprocess.stitch_tiles_host(plan33, scores, "core")
    mean = postprocess.stitch_tiles_host(plan33, scores, "mean")
    one = _counts(plan33) == 1
    assert same_bits(core[one], mean[one])
    differ = evaluation.semantic_preds_host(core) != evaluation.semantic_preds_host(mean)
    print(f"{int(differ.sum())} of {int((~one).sum())} shared points change their class between the modes")
    assert differ.sum() > 0 and not differ[one].any()


def test_one_tile_returns_the_tile_itself():
    from geoformer_amd import postprocess

    plan = uniform_plan(n=500, tile=100.0)
    assert plan.T == 1
    scores = random_scores(plan, 13, seed=4)
    for mode in MODES:
        assert same_bits(postprocess.stitch_tiles_host(plan, scores, mode), scores[0])


def test_zero_halo_mean_is_core():
    from geoformer_amd import postprocess

    plan = uniform_plan(n=1500, halo=0.0)
    assert plan.T == 9 and (plan.tile_of[:, 1] == -1).all()
    scores = random_scores(plan, 13, seed=5)
    core = postprocess.stitch_tiles_host(plan, scores, "core")
    assert same_bits(core, postprocess.stitch_tiles_host(plan, scores, "mean"))
    assert same_bits(core, brute_force(plan, scores, "core", 13))


@pytest.mark.parametrize("empty", ["none", "zero"])
def test_empty_tile(empty):
    from geoformer_amd import postprocess

    plan = gap_plan()
    scores = random_scores(plan, 13, seed=6, empty=empty)
    assert (scores[1] is None) if empty == "none" else scores[1].shape == (0, 13)
    for mode in MODES:
        assert same_bits(postprocess.stitch_tiles_host(plan, scores, mode), brute_force(plan, scores, mode, 13))


def test_closed_upper_edge_and_corner_points():
    from geoformer_amd import postprocess

    plan, corner_ids = edge_plan()
    assert (_counts(plan)[corner_ids] == 4).all()  # the points where four tiles meet lie in all four
    assert plan.core_of[1] == 8 and _counts(plan)[1] == 1  # the scan's upper corner belongs to the last tile alone
    scores = random_scores(plan, 20, seed=7)
    for mode in MODES:
        got = postprocess.stitch_tiles_host(plan, scores, mode)
        assert same_bits(got, brute_force(plan, scores, mode, 20))
    g = int(corner_ids[0])
    rows = [scores[plan.tile_of[g, j]][plan.local_of[g, j]] for j in range(4)]
    want = (((rows[0] + rows[1]) + rows[2]) + rows[3]) / np.float32(4)
    assert same_bits(postprocess.stitch_tiles_host(plan, scores, "mean")[g], want)


def test_hand_tables_count_3_and_no_slot():
    from geoformer_amd import postprocess

    plan = hand_plan()
    scores = random_scores(plan, 13, seed=8)
    mean = postprocess.stitch_tiles_host(plan, scores, "mean")
    core = postprocess.stitch_tiles_host(plan, scores, "core")
    assert same_bits(mean, brute_force(plan, scores, "mean", 13)) and same_bits(core, brute_force(plan, scores, "core", 13))
    a, b, c = scores[0][1], scores[1][2], scores[2][0]
    want = ((a + b) + c) / np.float32(3)  # sequential float32 sum, then the correctly rounded division
    assert same_bits(mean[0], want)
    # the division is a division: a product with float32(1 / 3) differs somewhere
    assert not same_bits(mean[0], ((a + b) + c) * np.float32(1.0 / 3.0))
    assert same_bits(core[0], b)
    zeros = np.zeros(13, np.float32)
    assert same_bits(mean[1], zeros) and same_bits(core[1], zeros)  # no slot at all
    assert same_bits(core[2], scores[2][1]) and same_bits(mean[2], (scores[0][0] + scores[2][1]) / np.float32(2))
    assert same_bits(core[3], zeros) and same_bits(mean[3], scores[2][0])  # the core slot names no row
    assert same_bits(core[4], scores[1][1]) and same_bits(mean[4], scores[1][1])


def test_errors(plan33):
    from geoformer_amd import postprocess

    scores = random_scores(plan33, 13, seed=9)
    with pytest.raises(ValueError, match="mode"):
        postprocess.stitch_tiles_host(plan33, scores, "median")
    with pytest.raises(ValueError, match="9 tiles"):
        postprocess.stitch_tiles_host(plan33, scores[:-1], "core")
    for bad in (scores[2][:-1], scores[2][:, :12], scores[2].astype(np.float64), scores[2].reshape(-1), None):
        wrong = list(scores)
        wrong[2] = bad
        with pytest.raises(ValueError, match="tile 2"):
            postprocess.stitch_tiles_host(plan33, wrong, "mean")
        with pytest.raises(ValueError, match="tile 2"):
            postprocess.stitch_tiles(plan33, wrong, "mean")
        with pytest.raises(ValueError, match="tile 2"):
            postprocess.stitch_tiles(plan33, [None if x is None else torch.from_numpy(x) for x in wrong], "core")
    with pytest.raises(ValueError, match="mode"):
        postprocess.stitch_tiles(plan33, scores, "max")


def test_stitch_tiles_dispatches_host_input_to_the_statement(plan33):
    from geoformer_amd import postprocess

    scores = random_scores(plan33, 13, seed=10)
    for mode in MODES:
        want = postprocess.stitch_tiles_host(plan33, scores, mode)
        got = postprocess.stitch_tiles(plan33, scores, mode)
        assert isinstance(got, np.ndarray) and same_bits(got, want)
        got = postprocess.stitch_tiles(plan33, [torch.from_numpy(x) for x in scores], mode)
        assert torch.is_tensor(got) and same_bits(got.numpy(), want)


def test_loops_validate_stitch_before_they_touch_the_model():
    from geoformer_amd import batch_eval

    tiling = batch_eval.Tiling()
    for loop in (batch_eval.predict_batches, batch_eval.semantic_batches):
        with pytest.raises(ValueError, match="stitch must be"):
            list(loop(None, [], 1, stitch="median"))
        with pytest.raises(ValueError, match="stitch must be"):
            list(loop(None, [], 1, tiles=tiling, stitch="median"))
        with pytest.raises(ValueError, match="stitch= goes with tiles="):
            list(loop(None, [], 1, stitch="core"))
    with pytest.raises(ValueError, match="needs stitch="):
        list(batch_eval.semantic_batches(None, [], 1, tiles=tiling))
    with pytest.raises(ValueError, match="a Tiling"):
        list(batch_eval.semantic_batches(None, [], 1, tiles="yes", stitch="core"))


def test_a_tiled_scene_that_shares_its_name_is_refused_before_the_model_is_touched():
    """The kept scores and the labels of a scan go by its name: a second scene of that name would be counted against
    the wrong labels."""
    from geoformer_amd import batch_eval

    raw = np.zeros((1000, 8))
    raw[:, :3] = np.random.default_rng(0).uniform(0, 8, (1000, 3))
    tiling = batch_eval.Tiling(max_points=500)
    items = [("a", raw), ("a", raw[:100]), ("b", raw[:50])]
    _, plans = batch_eval.tile_items(items, tiling)
    assert list(plans) == ["a"]
    with pytest.raises(ValueError, match="share their name"):
        batch_eval._tiled_raws(items, plans)
    with pytest.raises(ValueError, match="share their name"):
        list(batch_eval.semantic_batches(None, items, 2, tiles=tiling, stitch="core"))

    class Ev:
        pass

    with pytest.raises(ValueError, match="share their name"):
        list(batch_eval.predict_batches(None, items, 2, tiles=tiling, stitch="mean", semantic=Ev()))
    ok = batch_eval._tiled_raws([("a", raw), ("b", raw[:50]), ("b", raw[:60])], plans)  # untiled twins are not its matter
    assert list(ok) == ["a"] and ok["a"] is raw


def test_command_line_flag_and_derived_binding():
    import importlib.util
    import os
    from ctypes import c_int, c_longlong, c_void_p

    from geoformer_amd import _abi, pointops, postprocess

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "predict_scenes.py")
    spec = importlib.util.spec_from_file_location("predict_scenes_cli_stitch", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    assert ap.parse_args(["--synthetic", "1"]).tile_stitch is None
    assert ap.parse_args(["--tile", "4", "a.npy"]).tile_stitch is None
    a = ap.parse_args(["--tile", "4", "--tile-stitch", "core", "--panoptic", "a.npy"])
    assert (a.tile, a.tile_stitch, a.panoptic) == (4.0, "core", True)
    assert ap.parse_args(["--tile", "4", "--tile-stitch", "mean", "a.npy"]).tile_stitch == "mean"
    with pytest.raises(SystemExit):
        ap.parse_args(["--tile", "4", "--tile-stitch", "median", "a.npy"])
    fns = _abi.functions()
    assert fns["gf_tile_stitch_max_classes"] == (c_int, [])
    assert fns["gf_tile_stitch_scores"] == (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_longlong,
                                                    c_int, c_int, c_void_p, c_void_p])
    assert _abi.const("GF_TILE_SCORE_FIELDS") == 2 == pointops.TILE_SCORE_FIELDS == postprocess.TILE_SCORE_FIELDS
    assert (_abi.const("GF_TILE_STITCH_CORE"), _abi.const("GF_TILE_STITCH_MEAN")) == (0, 1)
    assert pointops.TILE_STITCH_MODES == {"core": 0, "mean": 1} and postprocess.STITCH_MODES == ("core", "mean")
    assert _abi.const("GF_ABI_VERSION") == 7
