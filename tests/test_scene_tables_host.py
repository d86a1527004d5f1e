"""The scene tables of the batched post-processing (no GPU): a table's layout is its row struct in
include/geoformer_hip.h, which the kernels read by member (csrc/*.hip) and geoformer_amd/postprocess.py reads as a numpy
record dtype.  Checked here: the columns did not move (literal matrices for the tables without a literal test of their
own elsewhere), and every row struct is the int64 record the builders fill."""
import types

import numpy as np

from geoformer_amd import _abi
from geoformer_amd import postprocess as pp


class _Tensor:
    """What the tile builders read of a device tensor: its address and its shape."""

    def __init__(self, address, *shape):
        self._address, self.shape = address, shape

    def data_ptr(self):
        return self._address


def _tile_inputs():
    plan = types.SimpleNamespace(T=3, offsets=np.array([0, 70, 70, 130]))
    rows = [(_Tensor(5000, 6, 70), _Tensor(5100, 40), None, None), (None, None, None, None),
            (_Tensor(7000, 9, 60), _Tensor(7100, 3), None, None)]
    return plan, rows


# Every expected matrix below is a literal: what the builder of the commit before the row structs (bare column numbers)
# returned for these inputs, three scenes or tiles with an empty one in the middle; none is computed by the code under
# test.
def test_label_scene_table_columns():
    t, sz = pp.label_scene_table([1000, 0, 3000], [100, 0, 5000], [4, 0, 7], [3, 0, 5], [1100, 0, 3100], [1200, 0, 3200],
                                 [1300, 0, 3300], [1400, 2400, 3400])
    assert t.dtype == np.int64 and t.shape == (3, pp.LBL_SCENE_FIELDS)
    assert t.tolist() == [[1000, 100, 4, 3, 1100, 1200, 1300, 1400, 0, 0, 0, 0],
                          [0, 0, 0, 0, 0, 0, 0, 2400, 6, 3, 3, 100],
                          [3000, 5000, 7, 5, 3100, 3200, 3300, 3400, 6, 3, 3, 100]]
    assert sz == {"bits": 401, "parts": 13, "rows": 8, "points": 5100, "max_points": 5000, "max_picks": 5}
    assert pp.label_scene_table(*[[]] * 8)[0].shape == (0, pp.LBL_SCENE_FIELDS)


def test_segment_scene_table_columns():
    t = pp.segment_scene_table([100, 0, 300], [1100, 0, 1300], [0, 40, 40, 95])
    assert t.dtype == np.int64 and t.tolist() == [[100, 1100, 40, 0], [0, 0, 0, 40], [300, 1300, 55, 40]]
    assert pp.segment_scene_table([], [], [0]).shape == (0, 4)


def test_tile_scene_table_columns():
    t, sz = pp.tile_scene_table(*_tile_inputs())
    assert t.dtype == np.int64 and t.shape == (3, pp.TILE_SCENE_FIELDS)
    assert t.tolist() == [[5000, 6, 70, 5100, 40, 0, 0], [0, 0, 0, 0, 0, 40, 140], [7000, 9, 60, 7100, 3, 40, 140]]
    assert sz["rows"] == 43 and sz["words"] == 200 and sz["row_tile"].tolist() == [0] * 40 + [2] * 3


def test_tile_score_table_columns():
    # (the commit before had no builder of its own for this table: stitch_tiles wrote (x.data_ptr(), x.shape[0]) into
    # the row of every tile with points, which for these tiles is the matrix below)
    t = pp.tile_score_table([_Tensor(9000, 70, 20), None, _Tensor(9900, 60, 20)])
    assert t.dtype == np.int64 and t.shape == (3, pp.TILE_SCORE_FIELDS)
    assert t.tolist() == [[9000, 70], [0, 0], [9900, 60]]


def test_row_structs_are_the_tables_records():
    """Every table struct: int64 members only, GF_*_FIELDS of them, and the record view of a builder's result is the
    returned array's own memory."""
    plan, rows = _tile_inputs()
    built = {
        "GfPropScene": (pp.PROP_ROW, "GF_PROP_SCENE_FIELDS",
                        pp.proposal_scene_table([1000, 2000], [0, 30, 75], [0, 900], [900, 400])),
        "GfNmsScene": (pp.NMS_ROW, "GF_NMS_SCENE_FIELDS",
                       pp.nms_scene_table([11, 0, 33], [100, 50, 64], [3, 0, 1], [5, 0, 6], [8, 0, 9])[0]),
        "GfLblScene": (pp.LBL_ROW, "GF_LBL_SCENE_FIELDS",
                       pp.label_scene_table([1, 0], [100, 0], [4, 0], [3, 0], [2, 0], [3, 0], [4, 0], [5, 6])[0]),
        "GfSegScene": (pp.SEG_ROW, None, pp.segment_scene_table([100, 0], [1100, 0], [0, 40, 40])),
        "GfTileScene": (pp.TILE_ROW, "GF_TILE_SCENE_FIELDS", pp.tile_scene_table(plan, rows)[0]),
        "GfTileScore": (pp.TILE_SCORE_ROW, "GF_TILE_SCORE_FIELDS", pp.tile_score_table([_Tensor(9000, 70, 20), None])),
        "GfBoxScene": (pp.BOX_SCENE_ROW, "GF_BOX_SCENE_FIELDS",
                       pp.box_scene_table(["rows", "ids"], [50, 60], [4, 0], [2, 3], [10, 20], [30, 0], [40, 50])[0]),
        "GfBoxIouScene": (pp.BOX_IOU_ROW, "GF_BOX_IOU_FIELDS", pp.box_iou_table([2, 0, 3], [1, 4, 2])[0]),
    }
    for name, (row, fields, table) in built.items():
        assert row == np.dtype(_abi.struct(name)), name
        F = len(row.names)
        assert all(row.fields[m][0] == np.int64 for m in row.names), name
        assert [row.fields[m][1] for m in row.names] == list(range(0, 8 * F, 8)), name  # column k at byte 8 k
        assert row.itemsize == 8 * F == 8 * (4 if fields is None else _abi.const(fields)), name
        assert table.dtype == np.int64 and table.shape == (table.shape[0], F) and table.shape[0] >= 2, name
        recs = pp.scene_rows(table, row)
        assert recs.shape == (table.shape[0],) and np.shares_memory(recs, table), name
        for k, m in enumerate(row.names):
            assert recs[m].tolist() == table[:, k].tolist(), (name, m)
        last = row.names[-1]
        recs[last][1] = 123456789  # through the record view ...
        assert table[1, F - 1] == 123456789, name
        table[0, 0] = -5  # ... and through the array
        assert recs[row.names[0]][0] == -5, name
        fresh, view = pp.scene_table(3, row)
        assert fresh.shape == (3, F) and not fresh.any() and np.shares_memory(fresh, view), name
        view[2] = tuple(range(F))  # a row takes a tuple, as the tables' users write it
        assert fresh[2].tolist() == list(range(F)), name


def test_output_row_columns():
    """The rows the kernels write, by member: the columns the Python side has always read."""
    i, f, m, b = pp._LBL_I, pp._LBL_F, pp._MSP, pp._BOX
    assert (i.count, i.owned, i.label_id, i.pick, i.kept) == (0, 1, 2, 3, 4) and pp.LBL_TABLE_INTS == 5
    assert (f.centroid, f.box_min, f.box_max, f.score) == (slice(0, 3), slice(3, 6), slice(6, 9), 9)
    assert pp.LBL_TABLE_FLOATS == 10
    assert (m.members, m.clusters, m.kept_points, m.largest, m.largest_size) == (0, 1, 2, 3, 4) and pp.MSP_TABLE_INTS == 5
    assert (b.cx, b.cy, b.cz, b.du, b.dv, b.dz, b.c, b.s, b.angle, b.count) == tuple(range(10)) and pp.BOX_FLOATS == 10
    row = pp._box_row(1.0, 3.0, 2.0, 6.0, -1.0, 1.0, np.float32(1), np.float32(0), 7, 12)
    assert row.tolist() == [2.0, 4.0, 0.0, 2.0, 4.0, 2.0, 1.0, 0.0, 7.0, 12.0]
