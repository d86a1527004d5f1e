"""GPU: every launch regime of the proposal stage against the float64 statements of tests/proposal_cases.py --
generate_proposal's fused statistics (k_proposal_stats / _fs / k_bp_stats), select (pr_select_rows), membership scatter
(k_proposal_scatter / k_bp_scatter), the bit-packed intersections (k_mask_* / k_bp_pack_bits / k_bp_intersections) and
matrix NMS (k_bp_matrix_nms and the torch algebra over the popcount kernel).

Everything but the scores is an integer and compared exactly: the cases keep every logit 1e-6 away from the membership
threshold and every deciding mask score / similarity 1e-4 (relative) away from its threshold, and the matrix NMS
thresholds are midpoints of gaps between float64 decayed scores that are at least 1e-4 (relative) wide
(tests/proposal_cases.py; tests/test_proposal_cases_host.py holds the cases to that on the CPU).

SCORE BOUND.  score = mask_score * sqrt(cls_score) * sem_score with mask_score = sum_members(sigmoid) / n and sem_score =
sum_members(sem_prob[:, cls]) / n.  All terms of both sums are positive, so a sum's relative error is at most (number of
additions on the longest chain) * u, u = 2^-24, to first order.  A thread of the 1024-thread workgroup adds at most
4 * ceil(N / 4096) terms (four per trip of the sweep), then come the 6 levels of the wave butterfly and the 16 serial
adds over the waves: depth D = 4 * ceil(N / 4096) + 22.  Two such means: 2 D u.  cls_score = 1 / sum of ncls expf: at most
ncls u from the additions (the square root halves it; not counted).  expf, sqrtf, the sigmoid's and the means' divisions,
(float)n + 1e-6f and the two products: 16 u allowed.  The test asserts TWICE this first-order bound,
    rel_tol = (2 D + ncls + 16) * 2^-23      (1.2e-5 at N = 8193, ncls = 20),
and the few-shot score (one mean times sqrtf(sim)) (D + 16) * 2^-23, beside the project's own 1e-4 absolute.  A score
whose statement is 0 (no member) must be exactly 0, a NaN (negative similarity) a NaN.  Each case prints its worst error
as a fraction of the bound.
"""
import numpy as np
import pytest
import torch

from tests import proposal_cases as pc

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ints(*ts):
    return [t.cpu().numpy().astype(np.int64) for t in ts]


def _score_ratio(got, want, rel_tol, what):
    """Asserts the score bound; returns the worst relative error as a fraction of rel_tol."""
    got = np.asarray(got, np.float64)
    nan, zero = np.isnan(want), want == 0
    assert (np.isnan(got) == nan).all(), what
    assert (got[zero] == 0).all(), what
    ok = ~nan & ~zero
    if not ok.any():
        return 0.0
    err = np.abs(got[ok] - want[ok])
    ratio = float((err / np.abs(want[ok])).max() / rel_tol)
    print(f"  {what}: worst score error = {ratio:.3f} of the bound {rel_tol:.2e}")
    assert ratio <= 1.0 and err.max() < 1e-4, (what, ratio, err.max())
    return ratio


# ---- statistics -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", pc.STATS_N)
def test_stats_equal_the_statement(hip, N):
    from geoformer_amd import pointops

    worst = 0.0
    for c in (c for c in pc.stats_cases().values() if c.logits.shape[1] == N):
        ncls = c.cls_logits.shape[1]
        s, f = c.statement(), c.statement_fs()
        logits = _dev(c.logits)
        cls, npts, sc, fin = pointops.proposal_stats(logits, _dev(c.cls_logits), _dev(c.sem_prob), c.logit_thresh,
                                                     c.score_thresh, c.npoint_thresh, c.min_class)
        cls, npts, fin = _ints(cls, npts, fin)
        assert (cls == s["cls_pred"]).all() and (npts == s["npoints"]).all() and (fin == s["final"]).all(), c.name
        worst = max(worst, _score_ratio(sc.cpu().numpy(), s["score"], pc.score_rel_tol(N, ncls), c.name))
        npts, sc, fin = pointops.proposal_stats_fs(logits, _dev(c.sim), c.logit_thresh, c.score_thresh, c.npoint_thresh,
                                                   c.sim_thresh)
        npts, fin = _ints(npts, fin)
        assert (npts == f["npoints"]).all() and (fin == f["final"]).all(), c.name
        worst = max(worst, _score_ratio(sc.cpu().numpy(), f["score"], pc.score_rel_tol_fs(N), c.name + " few-shot"))
    print(f"N = {N}: worst score error / bound = {worst:.3f}")


@pytest.mark.parametrize("name", list(pc.BATCHED_STATS_N))
def test_stats_batched_bit_equal_single_and_equal_the_statement(hip, name):
    from geoformer_amd import pointops, postprocess

    scenes = pc.batched_stats_cases()[name]
    c0 = scenes[0]
    logits = [_dev(c.logits) for c in scenes]
    Ns = [c.logits.shape[1] for c in scenes]
    fo = np.concatenate([[0], np.cumsum(Ns)])
    sem_t = _dev(np.concatenate([c.sem_prob.T for c in scenes], 1))  # class-major [ncls, sum N_b]
    cls_logits = _dev(np.stack([c.cls_logits for c in scenes]))
    table = postprocess.proposal_scene_table([t.data_ptr() for t in logits], fo, fo[:-1], Ns)
    got = pointops.proposal_stats_batched(pointops._table_dev(table, "cuda"), pc.STATS_NQ, cls_logits, sem_t,
                                          c0.logit_thresh, c0.score_thresh, c0.npoint_thresh, c0.min_class)
    assert all(g.shape == (len(scenes), pc.STATS_NQ) for g in got)
    for b, c in enumerate(scenes):
        one = pointops.proposal_stats(logits[b], cls_logits[b].contiguous(), _dev(c.sem_prob.T), c.logit_thresh,
                                      c.score_thresh, c.npoint_thresh, c.min_class, class_major=True)
        for g, o in zip(got, one):  # the promise of csrc/proposal_rows.h: the same bits
            assert torch.equal(g[b], o), (c.name, "batched != single launch")
        s = c.statement()
        cls, npts, fin = _ints(got[0][b], got[1][b], got[3][b])
        assert (cls == s["cls_pred"]).all() and (npts == s["npoints"]).all() and (fin == s["final"]).all(), c.name
        _score_ratio(got[2][b].cpu().numpy(), s["score"], pc.score_rel_tol(Ns[b], 20), c.name)


# ---- select ---------------------------------------------------------------------------------------------------------------
TAIL, SENTINEL = 257, -7


def _check_select(c, sel, cls, sc, count):
    want = pc.select_statement(c.final)
    assert count == len(want)
    assert sel[:count].tolist() == want.tolist()
    assert cls.dtype == np.int64 and (cls[:count] == c.cls_pred[want]).all() and (sc[:count] == c.scores[want]).all()


def _select_into_sentinels(hip, scenes, batched):
    """The library call into sentinel-filled buffers with a tail: only the first count entries of a scene's row change."""
    from geoformer_amd.pointops import ptr, stream_ptr

    S, nq = len(scenes), scenes[0].final.shape[0]
    final, cls_pred, scores = (_dev(np.stack([getattr(c, k) for c in scenes])) for k in ("final", "cls_pred", "scores"))
    sel = torch.full((S * nq + TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
    cls = torch.full((S * nq + TAIL,), SENTINEL, dtype=torch.int64, device="cuda")
    sc = torch.full((S * nq + TAIL,), float(SENTINEL), dtype=torch.float32, device="cuda")
    counts = torch.full((S + TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
    if batched:
        st = hip.gf_proposal_select_batched(ptr(final), ptr(cls_pred), ptr(scores), S, nq, ptr(sel), ptr(cls), ptr(sc),
                                            ptr(counts), stream_ptr())
    else:
        st = hip.gf_proposal_select(ptr(final), ptr(cls_pred), ptr(scores), nq, ptr(sel), ptr(cls), ptr(sc), ptr(counts),
                                    stream_ptr())
    assert st == 0, hip.gf_last_error()
    sel, cls, sc, counts = sel.cpu().numpy(), cls.cpu().numpy(), sc.cpu().numpy(), counts.cpu().numpy()
    assert (counts[S:] == SENTINEL).all()
    for b, c in enumerate(scenes):
        n, row = int(counts[b]), slice(b * nq, (b + 1) * nq)
        _check_select(c, sel[row], cls[row], sc[row], n)
        assert (sel[row][n:] == SENTINEL).all() and (cls[row][n:] == SENTINEL).all() and (sc[row][n:] == SENTINEL).all()
    assert (sel[S * nq:] == SENTINEL).all() and (cls[S * nq:] == SENTINEL).all() and (sc[S * nq:] == SENTINEL).all()


@pytest.mark.parametrize("nq", pc.SELECT_NQ)
def test_select_equals_the_statement(hip, nq):
    from geoformer_amd import pointops

    for flags in pc.SELECT_FLAGS:
        c = pc.select_cases()[f"nq{nq}-{flags}"]
        sel, cls, sc, cnt = pointops.proposal_select(_dev(c.final), _dev(c.cls_pred), _dev(c.scores))
        assert sel.dtype == torch.int32 and sel.shape == (nq,)
        _check_select(c, sel.cpu().numpy(), cls.cpu().numpy(), sc.cpu().numpy(), int(cnt.item()))
        _select_into_sentinels(hip, [c], False)
    for name in (f"nq{nq}-a", f"nq{nq}-b"):
        scenes = pc.batched_select_cases()[name]
        sel, cls, sc, counts = pointops.proposal_select_batched(_dev(np.stack([c.final for c in scenes])),
                                                                _dev(np.stack([c.cls_pred for c in scenes])),
                                                                _dev(np.stack([c.scores for c in scenes])))
        assert counts.shape == (3,)
        for b, c in enumerate(scenes):
            _check_select(c, sel[b].cpu().numpy(), cls[b].cpu().numpy(), sc[b].cpu().numpy(), int(counts[b].item()))
        _select_into_sentinels(hip, scenes, True)


# ---- scatter --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.scatter_cases()))
def test_scatter_equals_the_statement(hip, name):
    from geoformer_amd import pointops

    c = pc.scatter_cases()[name]
    want = c.statement()
    logits, sel, fg = _dev(c.logits), _dev(c.sel), _dev(c.fg_idxs)
    got = pointops.proposal_scatter(logits, sel, fg, c.logit_thresh, c.num_points)
    assert got.dtype == torch.int32 and (got.cpu().numpy() == want).all()
    # the library call into a buffer with a sentinel tail: nothing behind the rows is written
    buf = torch.full((want.size + TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
    buf[:want.size] = 0
    st = hip.gf_proposal_scatter(pointops.ptr(logits), pointops.ptr(sel), len(c.sel), c.logits.shape[1], pointops.ptr(fg),
                                 c.logit_thresh, c.num_points, pointops.ptr(buf), pointops.stream_ptr())
    buf = buf.cpu().numpy()
    assert st == 0 and (buf[:want.size].reshape(want.shape) == want).all() and (buf[want.size:] == SENTINEL).all()


@pytest.mark.parametrize("name", list(pc.BATCHED_SCATTER))
def test_scatter_batched_equals_the_statement(hip, name):
    from geoformer_amd import pointops, postprocess

    scenes = pc.batched_scatter_cases()[name]
    cases, counts = [c for c, _ in scenes], [n for _, n in scenes]
    Ns, widths = [c.logits.shape[1] for c in cases], [c.num_points for c in cases]
    fo = np.concatenate([[0], np.cumsum(Ns)])
    starts = pc.BATCHED_SCATTER_PT0 + np.concatenate([[0], np.cumsum(widths)[:-1]])
    assert (starts > 0).all()
    logits = [_dev(c.logits) for c in cases]
    fg_all = _dev(np.concatenate([c.fg_idxs + int(p0) for c, p0 in zip(cases, starts)]))  # batch-wide point indices
    sel = np.zeros((len(cases), pc.SCATTER_NQ), np.int32)
    for b, c in enumerate(cases):
        sel[b, :len(c.sel)] = c.sel
    table = postprocess.proposal_scene_table([t.data_ptr() for t in logits], fo, starts, widths)
    table_d = pointops._table_dev(table, "cuda")
    rows, elems = postprocess.packed_layout(counts, widths)
    total = int(elems[-1])
    sel_d, counts_d = _dev(sel), _dev(np.asarray(counts, np.int32))
    want = [pc.scatter_statement(c.logits, c.sel[:n], c.fg_idxs, c.logit_thresh, c.num_points)
            for c, n in zip(cases, counts)]

    def check(packed):
        for b, w in enumerate(want):  # block by block
            blk = packed[int(elems[b]):int(elems[b + 1])].reshape(counts[b], widths[b])
            assert (blk == w).all(), (name, b)

    got = pointops.proposal_scatter_batched(table_d, sel_d, counts_d, int(rows[-1]), total, max(Ns), fg_all,
                                            pc.LOGIT_THRESH)
    assert got.shape == (total,) and got.dtype == torch.int32
    check(got.cpu().numpy())
    for blk, w in zip(postprocess.split_packed(got, counts, widths), want):
        assert blk.shape == w.shape and (blk.cpu().numpy() == w).all()
    buf = torch.full((total + TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
    buf[:total] = 0
    st = hip.gf_proposal_scatter_batched(pointops.ptr(table_d), len(cases), pc.SCATTER_NQ, pointops.ptr(sel_d),
                                         pointops.ptr(counts_d), int(rows[-1]), max(Ns), pointops.ptr(fg_all),
                                         pc.LOGIT_THRESH, pointops.ptr(buf), pointops.stream_ptr())
    buf = buf.cpu().numpy()
    assert st == 0 and (buf[total:] == SENTINEL).all()  # words outside every block stay untouched
    check(buf[:total])


# ---- intersections -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.intersection_cases()))
def test_intersections_equal_the_statement(hip, name):
    from geoformer_amd import pointops, postprocess

    m = pc.intersection_cases()[name]
    want = pc.intersections_statement(m)
    md = _dev(m)
    got = pointops.mask_intersections(md)
    assert got.dtype == torch.int32 and (got.cpu().numpy().astype(np.int64) == want).all()
    # batched: an empty scene between this case and a small one
    other = pc.intersection_cases()["n3-N65"]
    od = _dev(other)
    table, sizes = postprocess.nms_scene_table([md.data_ptr(), 0, od.data_ptr()], [m.shape[1], 0, 65],
                                               [m.shape[0], 0, 3], [0, 0, 0], [0, 0, 0])
    inter = pointops.mask_intersections_batched(pointops._table_dev(table, "cuda"), sizes).cpu().numpy().astype(np.int64)
    n2 = m.shape[0] ** 2
    assert inter.shape == (n2 + 9,)
    assert (inter[:n2].reshape(want.shape) == want).all()
    assert (inter[n2:].reshape(3, 3) == pc.intersections_statement(other)).all()


# ---- matrix NMS ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nms_tensors(hip):
    """name -> (masks int32 [n, N], scores fp32, cats int64) on the device; the three category variants of a random size
    share one mask tensor."""
    out, shared = {}, {}
    for name, c in pc.nms_cases().items():
        key = c.masks.shape if c.random else name
        if key not in shared:
            shared[key] = _dev(c.masks.astype(np.int32))
        out[name] = (shared[key], _dev(c.scores), _dev(c.cats))
    return out


@pytest.mark.parametrize("kernel", pc.KERNELS)
@pytest.mark.parametrize("name", pc.nms_case_ids())
def test_matrix_nms_sweep_equals_the_statement(nms_tensors, name, kernel):
    """The fused kernel, one scene per launch, at every sweep threshold: the same indices in the same order."""
    from geoformer_amd import postprocess

    m, s, c = nms_tensors[name]
    thr, _ = pc.nms_sweep(name, kernel)
    assert len(thr) >= 1
    for t in thr:
        (got,) = postprocess.matrix_nms_batched([m], [s], [c], kernel=kernel, sigma=pc.SIGMA, final_score_thresh=t)
        assert got.dtype == torch.int64
        assert got.cpu().tolist() == pc.nms_picks(name, kernel, t), (name, kernel, t)


@pytest.mark.parametrize("kernel", pc.KERNELS)
def test_matrix_nms_all_cases_in_one_launch(nms_tensors, kernel):
    """Every case a scene of ONE launch, with empty scenes first, in the middle and last, at the standard thresholds."""
    from geoformer_amd import postprocess

    names = pc.nms_case_ids()
    order = [None] + names[:len(names) // 2] + [None] + names[len(names) // 2:] + [None]
    masks, scores, cats = ([nms_tensors[k][i] if k else [] for k in order] for i in range(3))
    for t in pc.STD_THRESHOLDS:
        picks = postprocess.matrix_nms_batched(masks, scores, cats, kernel=kernel, sigma=pc.SIGMA, final_score_thresh=t)
        assert len(picks) == len(order)
        checked = 0
        for k, got in zip(order, picks):
            assert got.dtype == torch.int64
            if k is None:
                assert got.numel() == 0
            elif t in pc.nms_sweep(k, kernel)[0]:  # the standard threshold is usable for this case
                assert got.cpu().tolist() == pc.nms_picks(k, kernel, t), (k, kernel, t)
                checked += 1
        assert checked >= len(names) - 6, (kernel, t, checked)


@pytest.mark.parametrize("name", [k for k, c in pc.nms_cases().items() if c.distinct])
def test_matrix_nms_torch_algebra_on_the_popcount_kernel(nms_tensors, name):
    from geoformer_amd.postprocess import matrix_non_max_suppression

    m, s, c = nms_tensors[name]
    for kernel in pc.KERNELS:
        for t in (t for t in pc.STD_THRESHOLDS if t in pc.nms_sweep(name, kernel)[0]):
            got = matrix_non_max_suppression(m, s, c, kernel=kernel, sigma=pc.SIGMA, final_score_thresh=t)
            assert got.dtype == torch.int64 and got.is_cuda
            assert got.cpu().tolist() == pc.nms_picks(name, kernel, t), (name, kernel, t)


def test_matrix_nms_more_than_the_capacity_raises_before_a_launch(hip):
    from geoformer_amd import postprocess

    n = postprocess.NMS_MAX_N + 1
    assert n == 1025
    before = hip.gf_last_error()
    with pytest.raises(ValueError, match="at most 1024"):
        postprocess.matrix_nms_batched([torch.zeros((n, 64), dtype=torch.int32, device="cuda")],
                                       [torch.zeros(n, device="cuda")], [torch.zeros(n, dtype=torch.int64, device="cuda")])
    assert hip.gf_last_error() == before  # nothing reached the library
