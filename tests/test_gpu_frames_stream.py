"""csrc/frames_stream.hip on the GPU: frames.Fuser bit for bit against frames.FuserHost after EVERY add -- the cells it
returns, a snapshot's four fields, new_id (the snapshot of the identity cells) and the map's keys, counts and sums --
each case from a fresh Fuser twice, the second time without the lane-run aggregation.  The shapes and what each straddles
are named in tests/frames_cases.py and tests/frames_stream_cases.py."""
import numpy as np
import pytest
import torch

from geoformer_amd import frames
from tests import frames_cases as fc
from tests import frames_stream_cases as sc

pytestmark = pytest.mark.gpu


def _identity(M):
    return torch.arange(M, dtype=torch.int32).reshape(1, 1, M)


def _host_run(parts, kw, min_obs, points):
    """The statement's answers after every add: (cells, [(snapshot, new_id) per min_obs], state)."""
    fz, seen, out = frames.FuserHost(**kw), [], []
    for p in parts:
        seen.append(fz.add_points(*p) if points else fz.add(p))
        both = torch.cat(seen)
        out.append((seen[-1], [(fz.snapshot(m, both), fz.snapshot(m, _identity(fz.cells)).point_of) for m in min_obs],
                    fz.state()))
    return fz, out


def _same_state(got, want):
    return all(x.dtype == y.dtype and x.shape == y.shape and (x == y).all() for x, y in zip(got, want))


def _check(parts, kw, dev_kw=None, min_obs=(1,), points=False):
    """Both device runs of a case against the statement; returns (the FuserHost, the two Fusers)."""
    fz, want = _host_run(parts, kw, min_obs, points)
    fus = []
    for aggregate in (None, False):
        fu = frames.Fuser(**kw, aggregate=aggregate, **(dev_kw or {}))
        seen = []
        for p, (cells_w, snaps_w, state_w) in zip(parts, want):
            c = fu.add_points(*p) if points else fu.add(p)
            assert c.is_cuda and c.dtype == torch.int32 and torch.equal(c.cpu(), cells_w)
            seen.append(c)
            both = torch.cat(seen)
            for m, (snap_w, new_id_w) in zip(min_obs, snaps_w):
                got = fu.snapshot(m, both)
                assert all(t.is_cuda for t in got) and sc.same_fused(got, snap_w), m
                assert torch.equal(fu.snapshot(m, _identity(fu.cells)).point_of.cpu(), new_id_w), m
            assert _same_state(fu.state(), state_w)
        assert fu.cells == fz.cells and fu.pixels == fz.pixels
        assert (fu.origin is None and fz.origin is None) or np.array_equal(fu.origin.view(np.int32), fz.origin.view(np.int32))
        fus.append(fu)
    return fz, fus


def test_limits(hip):
    from geoformer_amd import _lib

    lib = _lib.load()
    assert frames.stream_limits() == (sc.MAX_PROBES, sc.REACH, 2 ** 31 - 1)
    for M, T in ((0, 0), (0, 1), (0, 4800), (2500, 4800), (7242, 0), (1, 1 << 29), (1 << 20, 100), (3, 511), (3, 513), (16, 512)):
        assert lib.gf_frames_map_default_slots(M, T) == frames.stream_slots(M, T)[0], (M, T)
    assert lib.gf_frames_map_default_slots(-1, 0) == 0 and lib.gf_frames_map_default_slots(0, 1 << 31) == 0
    assert lib.gf_frames_map_insert_scratch_bytes(1000, 0) >= 4000 + 16 * 8
    assert lib.gf_frames_map_insert_scratch_bytes(1000, 65) == 0 and lib.gf_frames_map_insert_scratch_bytes(-1, 0) == 0
    assert lib.gf_frames_map_means_scratch_bytes(0, 0) == 0 and lib.gf_frames_map_means_scratch_bytes(64, 64) >= 8 + 8


@pytest.mark.parametrize("stride", [1, 2, 3])
def test_narrow_frames_one_by_one(hip, stride):
    fr = sc.narrow3("u16" if stride != 2 else "f32")
    fz, _ = _check(sc.chunks(fr, (1, 1, 1)), dict(stride=stride, edge=0.05 if stride == 2 else None))
    assert fz.cells > 20


@pytest.mark.parametrize("chunk", [fc.SMALL_CHUNK, None])
@pytest.mark.parametrize("split", ["1+3", "2+2", "4x1"])
@pytest.mark.parametrize("kind,edge,color", [("u16", None, True), ("f32", 0.05, False), ("u16", None, False), ("u16", 0.05, True)])
def test_dense_frames_in_chunks(hip, kind, edge, color, split, chunk):
    fr = sc.dense4(kind, color)
    fz, _ = _check(sc.chunks(fr, sc.SPLITS[split]), dict(edge=edge), dict(chunk=chunk))
    assert fz.cells > 5000 and fr.depth.numel() // fc.SMALL_CHUNK > fc.TOP  # at chunk 64: the scan's carry
    assert sc.same_fused(frames.Fuser(edge=edge, origin=fz.origin).snapshot(), frames.FuserHost().snapshot())  # both empty


@pytest.mark.parametrize("case", ["gaps3", "nasty3"])
def test_empty_and_full_workgroups_and_bad_depths(hip, case):
    fr = getattr(sc, case)()
    fz, _ = _check(sc.chunks(fr, (1, 1, 1)), dict(), dict(chunk=fc.SMALL_CHUNK))
    assert fz.cells > 1000
    if case == "gaps3":  # a first add without a valid pixel: nothing is fixed, and nothing is launched into the map
        fu = frames.Fuser()
        c = fu.add(sc.sub(fr, 1, 2))
        assert bool((c == -1).all()) and fu.origin is None and fu.cells == 0 and fu.slots is None
        assert fu.snapshot(1, c).point_of.shape == c.shape


MARGIN_SLOTS = 4096  # free slots the bounded table below keeps: no probe sequence comes near MAX_PROBES


def test_table_regimes(hip):
    fr = sc.dense4()
    parts = sc.chunks(fr, (1, 1, 1, 1))
    first_cells = frames.FuserHost()
    n0 = int((first_cells.add(parts[0]) >= 0).sum())
    M0 = first_cells.cells
    # the default table: smaller than the first frame's cells, so the first insert overflows (pigeonhole), the table is
    # rehashed once to the proven size and the insert run once more; then doubled until 4 M' after every add
    default, proven = frames.stream_slots(0, n0)
    assert default < M0 < proven // 2 + 1
    fz, fus = _check(parts, dict())
    for fu in fus:
        assert fu.retries >= 1 and fu.rehashes >= fu.retries + 2 and 4 * fu.cells <= fu.slots < 8 * fu.cells
    # the unbounded regime: never a rehash
    _, fus = _check(parts, dict(), dict(slots=sc.UNBOUNDED_SLOTS))
    assert all(fu.rehashes == 0 and fu.retries == 0 and fu.slots == sc.UNBOUNDED_SLOTS for fu in fus)
    # a bounded table with room: below 2 (M + n) at the later adds, never full
    small = 1 << 14
    assert small < 2 * (fz.cells + n0) and small >= fz.cells + MARGIN_SLOTS
    _, fus = _check(parts, dict(), dict(slots=small))
    assert all(fu.rehashes == 0 and fu.slots == small for fu in fus)
    # ids do not change across a rehash, growing or shrinking
    fu = fus[0]
    before = fu.state()
    for s in (small * 4, small):
        fu._rehash(s)
        assert fu.slots == s and _same_state(fu.state(), before)
    assert fu.rehashes == 2


def test_a_given_table_that_overflows(hip):
    fr = sc.dense4()
    parts = sc.chunks(fr, (1, 3))
    fu = frames.Fuser(slots=sc.MIN_SLOTS, origin=(-70, -70, -70))
    with pytest.raises(ValueError, match=r"overflowed; \d+ slots are always enough"):
        fu.add(parts[0])
    assert fu.cells == 0 and fu.pixels == 0 and fu.rehashes == 1 and fu.slots == sc.MIN_SLOTS
    keys, count, sums = fu.state()
    assert keys.shape == (0,) and int(fu._ids.max()) == -1 and int(fu._count.abs().sum()) == 0 and int(fu._sums.abs().sum()) == 0
    # the map is intact: a chunk that fits is exact, and then the overflow again leaves that state alone
    fz = frames.FuserHost(origin=(-70, -70, -70))
    few = np.array([[0, 0, 0], [1, 1, 1], [0, 0, 0.001], [2, 2, 2]], np.float32)
    assert torch.equal(fu.add_points(few).cpu(), fz.add_points(few)) and fu.cells == fz.cells >= 3
    before = fu.state()
    with pytest.raises(ValueError, match="overflowed"):
        fu.add(parts[0])
    assert _same_state(fu.state(), before) and _same_state(before, fz.state())
    assert sc.same_fused(fu.snapshot(), fz.snapshot())


def test_a_failed_add_into_a_given_table_more_than_half_full(hip):
    # A given table is kept, so successful adds take it above half full; the rehash that cleans up after a failed add
    # must still find room (one slot per cell is enough), and the error must be the ValueError, not the library's.
    fr = sc.dense4()
    origin = frames.backproject_host(fr)[0].min(0) - np.float32(1.0)
    parts = sc.chunks(fr, (1, 1, 1, 1))
    fz = frames.FuserHost(origin=origin)
    fu = frames.Fuser(origin=origin, slots=sc.CROWDED_SLOTS)
    for p in parts[:3]:
        assert torch.equal(fu.add(p).cpu(), fz.add(p))
    assert fu.cells > sc.CROWDED_SLOTS // 2 and fu.rehashes == 0 and fu.slots == sc.CROWDED_SLOTS

    def intact(state, count, sums):
        assert fu.slots == sc.CROWDED_SLOTS and _same_state(fu.state(), state)
        assert torch.equal(fu._count, count) and torch.equal(fu._sums, sums)
        assert int((fu._ids >= 0).sum()) == fu.cells and int((fu._keys != -1).sum()) == fu.cells  # no claim is left
        assert int((fu._first != 2 ** 31 - 1).sum()) == 0

    state, count, sums = fu.state(), fu._count.clone(), fu._sums.clone()
    with pytest.raises(ValueError, match="origin="):
        fu.add(sc.moved(parts[3], (-50.0, 0.0, 0.0)))
    intact(state, count, sums)
    with pytest.raises(ValueError, match="origin="):
        fu.add(sc.moved(parts[3], (0.0, sc.REACH, 0.0)))
    intact(state, count, sums)
    # more new cells than the table has free slots: the overflow, by pigeonhole
    xyz, rgb = fc.random_points()
    far = (xyz + (origin + np.float32(0.5))).astype(np.float32)
    assert np.unique(np.floor((far - origin) / np.float32(0.02)).astype(np.int64), axis=0).shape[0] > sc.CROWDED_SLOTS
    with pytest.raises(ValueError, match=r"overflowed; \d+ slots are always enough"):
        fu.add_points(far, rgb)
    intact(state, count, sums)
    assert fu.rehashes == 3
    # the map still works: points that fall into cells it knows, and a few new ones
    few = np.concatenate([frames.backproject_host(parts[0])[0][:100], far[:5]])
    assert torch.equal(fu.add_points(few).cpu(), fz.add_points(few)) and fu.cells == fz.cells
    assert _same_state(fu.state(), fz.state()) and sc.same_fused(fu.snapshot(), fz.snapshot())


def test_rows_grow(hip):
    fr = sc.dense4()
    fz, fus = _check(sc.chunks(fr, (1, 1, 2)), dict(), dict(capacity=sc.SMALL_CAPACITY))
    for fu in fus:
        assert fu.row_growths >= 2 and fu.capacity >= fu.cells
        assert int(fu._count[fu.cells:].abs().sum()) == 0 and int(fu._sums[fu.cells:].abs().sum()) == 0  # zero beyond M


def test_every_point_alone_in_its_cell(hip):
    xyz, rgb = fc.random_points()
    half = sc.CELL_POINTS // 2
    parts = [(xyz[:half], rgb[:half]), (xyz[half:], rgb[half:])]
    assert -(-half // fc.SMALL_CHUNK) < fc.TOP < sc.CELL_POINTS // fc.SMALL_CHUNK
    for chunk in (fc.SMALL_CHUNK, None):
        fz, _ = _check(parts, dict(cell=0.0005, origin=(0, 0, 0)), dict(chunk=chunk, capacity=256), points=True)
        assert fz.cells > sc.CELL_POINTS - 50  # (nearly) every point its own cell: no run, no shared atomic
    # one add of all 20000: 313 chunks of 64, the numbering scan's carry
    _check([(xyz, rgb)], dict(cell=0.0005, origin=(0, 0, 0)), dict(chunk=fc.SMALL_CHUNK), points=True)


def test_one_cell_full_contention(hip):
    fz, _ = _check(sc.chunks(sc.dense4(), (1, 3)), dict(cell=sc.ONE_CELL))
    assert fz.cells == 1 and fz.pixels == sc.DENSE4_PIXELS


def test_the_same_frames_twice(hip):
    fr = sc.sub(sc.dense4(), 0, 2)
    fz, fus = _check([fr, fr], dict(cell=sc.COARSE), min_obs=(1, 3))
    half = frames.FuserHost(sc.COARSE, origin=fz.origin)
    half.add(fr)
    assert fz.cells == half.cells and (fz.state()[1] == 2 * half.state()[1]).all()  # no new cell at the second add


def test_snapshots_of_one_state(hip):
    fr = sc.dense4()
    fz, fus = _check(sc.chunks(fr, (2, 2)), dict(cell=sc.COARSE), min_obs=(1, 3, 10 ** 6))
    fu = fus[0]
    cells = frames.Fuser(sc.COARSE, origin=fz.origin).add(fr)  # the whole input at once: the same numbers
    a, b = fu.snapshot(3, cells), fu.snapshot(1, cells)
    assert 100 < a.xyz.shape[0] < b.xyz.shape[0] and sc.same_fused(fu.snapshot(3, cells), a)
    none = fu.snapshot(10 ** 6, cells)
    assert none.xyz.shape == (0, 3) and none.rgb.shape == (0, 3) and none.count.shape == (0,) and bool((none.point_of == -1).all())
    assert sc.same_fused(a, frames.fuse(fr, sc.COARSE, min_obs=3, origin=fz.origin))  # the one-shot kernels agree
    for bad in (fu.cells, -2, 2 ** 31 - 1, -2 ** 31):  # checked by the lookup as it reads them: nothing out of the table
        with pytest.raises(ValueError, match="cells holds"):
            fu.snapshot(1, torch.tensor([0, -1, bad], dtype=torch.int32))
    assert fu.snapshot(1, torch.tensor([fu.cells - 1, -1], dtype=torch.int32)).point_of.tolist()[1] == -1


@pytest.mark.parametrize("trigger", ["below", "beyond"])
def test_a_failed_add_leaves_the_map_as_it_was(hip, trigger):
    fr = sc.dense4()
    good = sc.chunks(fr, (2, 1, 1))
    origin = frames.backproject_host(fr)[0].min(0) - np.float32(1.0)
    bad = sc.moved(good[1], (-50.0, 0.0, 0.0) if trigger == "below" else (0.0, sc.REACH, 0.0))
    fz = frames.FuserHost(origin=origin)
    want = [fz.add(p) for p in good]
    for aggregate in (None, False):
        fu = frames.Fuser(origin=origin, aggregate=aggregate)
        cells = [fu.add(good[0])]
        state, count, sums = fu.state(), fu._count.clone(), fu._sums.clone()
        snap, rehashes, slots = fu.snapshot(1, cells[0]), fu.rehashes, fu.slots
        with pytest.raises(ValueError, match="origin="):
            fu.add(bad)  # the numbering launches see the flag and write nothing; the rehash drops the claims
        assert fu.rehashes == rehashes + 1 and fu.slots == slots
        assert _same_state(fu.state(), state) and torch.equal(fu._count, count) and torch.equal(fu._sums, sums)
        assert int((fu._ids >= 0).sum()) == fu.cells and int((fu._keys != -1).sum()) == fu.cells  # no claim is left
        assert int((fu._first != 2 ** 31 - 1).sum()) == 0
        assert sc.same_fused(fu.snapshot(1, cells[0]), snap)
        cells += [fu.add(good[1]), fu.add(good[2])]
        assert all(torch.equal(c.cpu(), w) for c, w in zip(cells, want))
        assert sc.same_fused(fu.snapshot(1, torch.cat(cells)), fz.snapshot(1, torch.cat(want)))
        assert _same_state(fu.state(), fz.state())
    # a first add that fails fixes no origin
    fu = frames.Fuser(cell=0.00001)  # the 64 m of margin are 6 400 000 cells: beyond the grid's 2^21
    with pytest.raises(ValueError, match="margin="):
        fu.add(good[0])
    assert fu.origin is None and fu.cells == 0 and fu.pixels == 0 and int((fu._keys != -1).sum()) == 0
    fu = frames.Fuser(margin=0.0)
    fu.add(good[0])
    with pytest.raises(ValueError, match="margin="):
        fu.add(sc.moved(good[1], (-3.0, -3.0, -3.0)))  # below the first chunk's minimum
    with pytest.raises(ValueError, match="differs"):
        fu.add(sc.sub(sc.dense4("f32"), 0, 1))


def test_argument_checks_launch_nothing(hip):
    from geoformer_amd import _lib
    from geoformer_amd._lib import ptr

    lib = _lib.load()
    out = torch.full((4096,), 7, dtype=torch.int32, device="cuda")
    p = ptr(out)
    good = dict(n=10, cell=0.02, slots=64, M=0, chunk=0)
    for k, v in (("n", -1), ("n", (1 << 29) + 1), ("cell", 0.0), ("cell", float("inf")), ("cell", float("nan")), ("slots", 32),
                 ("slots", 96), ("slots", 1 << 32), ("M", -1), ("M", 2 ** 31 - 5), ("chunk", 32), ("chunk", 100),
                 ("chunk", 1 << 17)):
        a = dict(good, **{k: v})
        st = lib.gf_frames_map_insert(p, a["n"], a["cell"], p, p, p, p, a["slots"], a["M"], a["chunk"], p, p, p, None)
        assert st != 0, (k, v)
    for null in range(8):
        args = [p] * 8
        args[null] = None
        xyz, origin, keys, ids, first, scratch, cell_of, words = args
        assert lib.gf_frames_map_insert(xyz, 10, 0.02, origin, keys, ids, first, 64, 0, 0, scratch, cell_of, words, None) != 0, null
    assert lib.gf_frames_map_insert(None, 0, 0.02, None, None, None, None, 64, 0, 0, None, None, None, None) == 0  # n == 0
    for old_slots, cells, new_slots in ((32, 0, 64), (64, 0, 96), (0, 1, 64), (64, -1, 64), (64, 0, 1 << 32)):
        assert lib.gf_frames_map_rehash(p, p, old_slots, cells, ptr(out[2048:]), ptr(out[2048:]), ptr(out[2048:]), new_slots,
                                        None) != 0, (old_slots, cells, new_slots)
    assert lib.gf_frames_map_rehash(p, p, 64, 0, p, p, p, 64, None) != 0  # the tables overlap
    assert lib.gf_frames_map_rehash(None, None, 0, 0, None, p, p, 64, None) != 0
    for n, M in ((-1, 1), ((1 << 29) + 1, 1), (5, 0)):
        assert lib.gf_frames_map_accumulate(p, p, p, n, M, p, 1, p, p, p, None) != 0, (n, M)
    assert lib.gf_frames_map_accumulate(p, p, p, 5, 1, p, 1, p, p, None, None) != 0
    assert lib.gf_frames_map_accumulate(None, None, None, 0, 0, None, 1, None, None, None, None) == 0
    for M, min_obs, chunk in ((0, 1, 0), (2 ** 31 - 1, 1, 0), (5, 0, 0), (5, 1, 65)):
        assert lib.gf_frames_map_means(p, p, M, p, min_obs, chunk, p, p, p, p, p, p, None) != 0, (M, min_obs, chunk)
    assert lib.gf_frames_map_means(p, p, 5, p, 1, 0, p, p, p, p, p, None, None) != 0
    assert lib.gf_frames_map_lookup(p, -1, p, 5, p, None, None) != 0 and lib.gf_frames_map_lookup(p, 5, None, 5, p, None, None) != 0
    assert lib.gf_frames_map_lookup(p, 5, p, -1, p, None, None) != 0 and lib.gf_frames_map_lookup(p, 5, p, 5, None, p, None) != 0
    assert lib.gf_frames_map_lookup(None, 0, None, 0, None, None, None) == 0
    # a same-size rehash takes a table up to full: one slot per cell (more cells than slots is refused)
    assert lib.gf_frames_map_rehash(p, p, 64, 65, ptr(out[2048:]), ptr(out[2048:]), ptr(out[2048:]), 64, None) != 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())


# ---- through the model --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip):
    from geoformer_amd.model import GeoFormer, load_config
    from tests.util import synthetic_state_dict

    m = GeoFormer(load_config("test_geoformer_scannet.yaml"))
    m.load_state_dict(synthetic_state_dict(m.state_dict(), 0))
    m.cuda()
    m.eval()
    return m


def test_a_stream_through_the_model_equals_the_one_shot_fusion(model):
    from geoformer_amd import batch_eval
    from tests import frames_lift_cases as lc

    fr = fc.make(fc.dense(), "u16")
    fu = frames.Fuser(0.02)
    cells = torch.cat([fu.add(sc.sub(fr, k, k + 1)) for k in range(3)])
    stream, one = fu.snapshot(1, cells), frames.fuse(fr, 0.02, origin=fu.origin)
    assert sc.same_fused(stream, one) and stream.xyz.shape[0] > 1000
    got = []
    for fused in (stream, one):
        raw, shift = fused.raw_scene()
        np.random.seed(0)
        (name, labels), = batch_eval.label_batches(model, [("frames", raw)], 1)
        ids = np.asarray(labels.ids)
        sem, inst = frames.lift_scene(fused, *lc.images("dense"), ignore=lc.IGNORE)
        got.append((raw, shift, ids, frames.gather(fused, ids, fill=-5).cpu().numpy(), sem.cpu().numpy(), inst.cpu().numpy()))
    for a, b in zip(*got):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert got[0][3].shape == (3, fc.DENSE[1], fc.DENSE[0]) and (got[0][3] >= 0).any() and (got[0][5] >= 0).any()
