"""Host (no GPU): holds the cases and float64 statements of tests/proposal_cases.py to account -- every case meets its
margins and caps, the sweep thresholds tell three wrong matrix NMS statements from the right one, picks_statement gives
the REFERENCE's picks (tests/golden/matrix_nms_sizes.npz and the older matrix_nms.npz), the CPU path of
postprocess.matrix_non_max_suppression gives the statement's, and the statistics / scatter / intersection statements agree
with the scalar oracle."""
import os

import numpy as np
import pytest
import torch

from tests import proposal_cases as pc

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- statistics, select, scatter, intersections: the cases are what they claim to be ---------------------------------
def test_stats_cases_meet_margins_and_plant_their_rows():
    cases = pc.stats_cases()
    assert len(cases) == len(pc.STATS_N) * 3 * 2
    decided_by_tie = 0
    for c in cases.values():
        pc.check_stats_margins(c)
        N, ncls = c.logits.shape[1], c.cls_logits.shape[1]
        assert c.logits.shape == (pc.STATS_NQ, N) and c.sem_prob.shape == (N, ncls) and c.npoint_thresh >= 1
        s = c.statement()
        t = c.npoint_thresh
        assert s["npoints"][0] == N and s["npoints"][1] == 0 and s["score"][1] == 0.0 and s["final"][1] == 0
        assert s["npoints"][2] == min(t, N) and s["npoints"][3] == min(t - 1, N)
        if 0 <= c.min_class - 1 < ncls:
            assert s["cls_pred"][4] == c.min_class - 1 and s["final"][4] == 0
        if ncls >= 2:  # two equal maxima: the lower index
            row = c.cls_logits[5]
            top = np.nonzero(row == row.max())[0]
            assert len(top) == 2 and s["cls_pred"][5] == top[0]
            decided_by_tie += int(top[0] < c.min_class <= top[1])
        rel = (s["mask_score"][6:8] - c.score_thresh) / c.score_thresh
        assert 2 * pc.SCORE_MARGIN < rel[0] < 6 * pc.SCORE_MARGIN and -6 * pc.SCORE_MARGIN < rel[1] < -2 * pc.SCORE_MARGIN
        if ncls > c.min_class:
            assert s["final"][[0, 2, 3, 6, 7]].tolist() == [1, int(N >= t), 0, 1, 0], c.name
        else:
            assert not s["final"].any()
        f = c.statement_fs()
        assert f["final"][0] == 1 and f["final"][2] == 0 and f["npoints"][2] >= t  # the similarity decides both
        assert np.isnan(f["score"][3]) and f["final"][3] == 0 and np.isfinite(np.delete(f["score"], 3)).all()
    assert decided_by_tie == len(pc.STATS_N)  # ncls = 20, min_class = 4: the tie-break decides `final`


def test_batched_stats_cases():
    cases = pc.batched_stats_cases()
    assert [Ns.index(0) for Ns in pc.BATCHED_STATS_N.values()] == [0, 2, 3]
    for name, scenes in cases.items():
        assert tuple(c.logits.shape[1] for c in scenes) == pc.BATCHED_STATS_N[name]
        assert all(N in pc.STATS_N or N == 0 for N in pc.BATCHED_STATS_N[name])
        for c in scenes:
            pc.check_stats_margins(c)
            assert (c.npoint_thresh, c.min_class, c.cls_logits.shape[1]) == (pc.BATCHED_NPOINT_THRESH, 4, 20)
            if c.logits.shape[1] == 0:
                s = c.statement()
                assert not s["npoints"].any() and not s["score"].any() and not s["final"].any()


def test_select_cases():
    cases = pc.select_cases()
    assert len(cases) == len(pc.SELECT_NQ) * 4
    for nq in pc.SELECT_NQ:
        assert pc.select_statement(cases[f"nq{nq}-all"].final).tolist() == list(range(nq))
        assert pc.select_statement(cases[f"nq{nq}-none"].final).tolist() == []
        assert pc.select_statement(cases[f"nq{nq}-alternating"].final).tolist() == list(range(1, nq, 2))
        r = cases[f"nq{nq}-random"].final
        assert nq < 63 or 0.15 * nq < r.sum() < 0.45 * nq
    assert all(len(v) == 3 and len({c.final.shape for c in v}) == 1 for v in pc.batched_select_cases().values())


def test_scatter_cases(oracle):
    for c in pc.scatter_cases().values():
        N = c.logits.shape[1]
        assert pc.logit_margin_ok(c.logits, c.logit_thresh) and c.num_points == N + N // 2
        assert (np.diff(c.fg_idxs) > 0).all() and 0 <= c.fg_idxs[0] and c.fg_idxs[-1] < c.num_points
        want = c.statement()
        assert want.dtype == np.int32 and set(np.unique(want)) <= {0, 1}
        assert (want == oracle.proposal_scatter(c.logits, c.sel, c.fg_idxs, c.logit_thresh, c.num_points)).all(), c.name
    for name, scenes in pc.batched_scatter_cases().items():
        assert [cnt for _, cnt in scenes].index(0) == pc.BATCHED_SCATTER_EMPTY[name] and len(scenes) == 4
        assert sum(cnt == 0 for _, cnt in scenes) == 1


def test_intersection_cases(oracle):
    cases = pc.intersection_cases()
    assert [m.shape for m in cases.values()] == list(pc.INTERSECTION_SIZES)
    waves = {m.shape: m.shape[0] * ((m.shape[1] + 63) // 64) for m in cases.values()}
    assert waves[(64, 33281)] == 33344 > pc.BATCH_STRIDE_LIMIT and 200 * 200 == 40000 > pc.BATCH_STRIDE_LIMIT
    for name, m in cases.items():
        n, N = m.shape
        want = pc.intersections_statement(m)
        assert want.dtype == np.int64 and (want == oracle.mask_intersections(m)).all(), name
        if n >= 2:
            assert not m[0].any() and m[1].all() and not want[0].any() and (want[1] == m.sum(1)).all()
        else:
            assert m.all()


def _rel_close(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all()
    zero = want == 0
    assert (got[zero & ~nan] == 0).all()
    ok = ~nan & ~zero
    return float((np.abs(got[ok] - want[ok]) / np.abs(want[ok])).max() / tol) if ok.any() else 0.0


def test_stats_statements_against_the_scalar_oracle(oracle):
    """Integers equal, scores to 1e-6 relative."""
    worst = 0.0
    for c in list(pc.stats_cases().values()) + [c for v in pc.batched_stats_cases().values() for c in v]:
        s = c.statement()
        cls, npts, sc, fin = oracle.proposal_stats(c.logits, c.cls_logits, c.sem_prob, c.logit_thresh, c.score_thresh,
                                                   c.npoint_thresh, c.min_class)
        assert (cls == s["cls_pred"]).all() and (npts == s["npoints"]).all() and (fin == s["final"]).all(), c.name
        worst = max(worst, _rel_close(sc, s["score"], 1e-6))
        f = c.statement_fs()
        npts, sc, fin = oracle.proposal_stats_fs(c.logits, c.sim, c.logit_thresh, c.score_thresh, c.npoint_thresh,
                                                 c.sim_thresh)
        assert (npts == f["npoints"]).all() and (fin == f["final"]).all(), c.name
        worst = max(worst, _rel_close(sc, f["score"], 1e-6))
    print(f"oracle scores: worst relative error / 1e-6 = {worst:.3f}")
    assert worst <= 1.0


# ---- matrix NMS ----------------------------------------------------------------------------------------------------------
HAND_DECAYED = {  # the values written out in tests/proposal_cases.py
    "one": ([0.7], [0.7]),
    "pair": ([0.9, 0.485225], [0.9, 0.4]),
    "chain3": ([0.9, 0.485225, 0.393674], [0.9, 0.4, 0.373333]),
    "chain3x": ([0.9, 0.8, 0.584689], [0.9, 0.8, 0.49]),
    "dup3": ([0.9, 0.108268, 0.094735, 0.6], [0.9, 0.0, np.nan, 0.6]),
    "ties": ([0.7, 0.9, 0.7, 0.7, 0.7], [0.7, 0.9, 0.7, 0.7, 0.7]),
}


def test_hand_built_cases_have_the_documented_decayed_scores():
    assert tuple(HAND_DECAYED) == pc.NMS_HAND
    for name, per_kernel in HAND_DECAYED.items():
        for kernel, want in zip(pc.KERNELS, per_kernel):
            np.testing.assert_allclose(pc.nms_decayed(name, kernel), want, rtol=0, atol=1.5e-6, equal_nan=True)
    c = pc.nms_cases()["pair"]
    inter = pc.intersections_statement(c.masks)
    assert inter[0, 1] / (inter[0, 0] + inter[1, 1] - inter[0, 1]) == 0.5
    # chain3 without the division: C moves, so the compensation term is what its picks test
    nc = [pc.nms_decayed("chain3", k, "no_compensation")[2] for k in pc.KERNELS]
    np.testing.assert_allclose(nc, [0.238776, 0.186667], rtol=0, atol=1.5e-6)
    assert pc.nms_picks("ties", "gaussian", 0.05) == [1, 0, 2, 3, 4] and pc.nms_picks("ties", "linear", 0.8) == [1]
    assert pc.nms_picks("dup3", "linear", 0.05) == [0, 3] and pc.nms_picks("dup3", "linear", -1.0) == [0, 1, 3]
    assert not pc.nms_cases()["ties"].distinct and all(pc.nms_cases()[k].distinct for k in pc.NMS_HAND[:-1])
    assert all(c.masks.any(1).all() for c in pc.nms_cases().values())


def test_sweep_thresholds_sit_in_usable_gaps_and_the_cap_holds():
    shares = {}
    for name, c in pc.nms_cases().items():
        for kernel in pc.KERNELS:
            dec = pc.nms_decayed(name, kernel)
            thr, bad = pc.nms_sweep(name, kernel)
            shares[name, kernel] = bad
            v = dec[np.isfinite(dec)]
            for t in thr:  # nothing within GAP_REL / 2 relative of a threshold
                assert (np.abs(v - t) > 0.5 * pc.GAP_REL * np.maximum(v, t) * (1 - 1e-9)).all(), (name, kernel, t)
            lo, hi, usable = pc.gaps(dec)
            mids = set((0.5 * (lo + hi))[usable].tolist())
            sweep = pc.sweep_midpoints(dec, c.n)
            assert set(sweep) <= mids and set(sweep) <= set(thr) and set(thr) - set(sweep) <= set(pc.STD_THRESHOLDS)
            assert len(sweep) == (len(mids) if c.n <= 65 else min(16, len(mids))) and len(thr) <= 66
            if c.random:
                assert bad <= pc.GAP_CAP, (name, kernel, bad)
                assert len(sweep) >= min(c.n - 1, 16) * (1 - pc.GAP_CAP)
                kept = [len(pc.nms_picks(name, kernel, t)) for t in sweep]
                assert kept == sorted(kept, reverse=True) and len(set(kept)) >= 0.9 * len(kept)
    print("share of unusable gaps: " + ", ".join(f"{n}/{k[:3]} {100 * b:.1f}%" for (n, k), b in shares.items() if b > 0))
    assert max(shares[n, k] for n, k in shares if pc.nms_cases()[n].random) < pc.GAP_CAP


@pytest.mark.parametrize("name", [k for k, c in pc.nms_cases().items() if c.random and c.n >= 63 and c.n_classes == 3])
def test_sweep_thresholds_catch_the_mutants(name):
    """Each of three wrong statements (no compensation, class-agnostic labels, compensation taken from column a instead of
    row r) must disagree with the right one at a third or more of the case's sweep thresholds."""
    for kernel in pc.KERNELS:
        thr, _ = pc.nms_sweep(name, kernel)
        right = [pc.nms_picks(name, kernel, t) for t in thr]
        for mutant in pc.MUTANTS:
            caught = sum(pc.nms_picks(name, kernel, t, mutant) != r for t, r in zip(thr, right))
            print(f"{name} {kernel} {mutant}: caught at {caught} of {len(thr)}")
            assert 3 * caught >= len(thr), (name, kernel, mutant, caught, len(thr))


def test_statement_gives_the_references_picks():
    """tests/golden/matrix_nms_sizes.npz holds the picks of the reference's own function at every sweep threshold: the
    statement is tied to the reference, not to a reading of it."""
    z = np.load(os.path.join(G, "matrix_nms_sizes.npz"))
    assert [str(x) for x in z["names"]] == pc.golden_case_ids()
    checked = 0
    for name in pc.golden_case_ids():
        c = pc.nms_cases()[name]
        n, N = (int(v) for v in z[f"{name}_shape"])
        assert (np.unpackbits(z[f"{name}_bits"])[:n * N].reshape(n, N) == c.masks).all()
        assert (z[f"{name}_scores"] == c.scores).all() and (z[f"{name}_cats"] == c.cats).all()
        for kernel in pc.KERNELS:
            thr, _ = pc.nms_sweep(name, kernel)
            assert z[f"{name}_{kernel}_thr"].tolist() == list(thr), (name, kernel)
            ends = np.cumsum(z[f"{name}_{kernel}_count"])
            flat = z[f"{name}_{kernel}_picks"]
            for k, t in enumerate(thr):
                want = flat[ends[k] - z[f"{name}_{kernel}_count"][k]:ends[k]].tolist()
                assert pc.nms_picks(name, kernel, t) == want, (name, kernel, t)
                checked += 1
    assert checked > 500


def test_statement_gives_the_picks_of_the_older_golden():
    z = np.load(os.path.join(G, "matrix_nms.npz"))
    for key in z.files:
        if key.startswith("pick_"):
            _, kernel, thr = key.split("_")
            got = pc.picks_statement(z["masks"], z["scores"], z["categories"], kernel, float(thr))
            assert got == z[key].tolist(), key


@pytest.mark.parametrize("name", [k for k, c in pc.nms_cases().items() if c.distinct])
def test_cpu_path_equals_the_statement(name):
    from geoformer_amd.postprocess import matrix_non_max_suppression

    c = pc.nms_cases()[name]
    masks, scores, cats = torch.from_numpy(c.masks.astype(np.int32)), torch.from_numpy(c.scores), torch.from_numpy(c.cats)
    for kernel in pc.KERNELS:
        for t in pc.nms_sweep(name, kernel)[0]:
            got = matrix_non_max_suppression(masks, scores, cats, kernel=kernel, sigma=pc.SIGMA, final_score_thresh=t)
            assert got.dtype == torch.int64 and got.tolist() == pc.nms_picks(name, kernel, t), (name, kernel, t)
