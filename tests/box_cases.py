"""Case builders shared by tests/test_boxes_host.py and tests/test_gpu_boxes.py: scenes of groups in the two forms of
gf_instance_boxes_batched (a dict per scene), the statements' rows of a scene, and hand-made boxes for the IoU."""
import numpy as np

MEMBER_EDGE = (0, 1, 63, 64, 65)  # next to the wave; the chunk's neighbours c - 1, c, c + 1, 2 c + 1 are added per chunk


def rows_case(masks, pick, xyz):
    return {"form": "rows", "masks": np.asarray(masks, np.int32), "pick": np.asarray(pick, np.int64),
            "xyz": np.ascontiguousarray(xyz, np.float32)}


def ids_case(group, n_groups, xyz):
    return {"form": "ids", "group": np.asarray(group, np.int32), "n_groups": int(n_groups),
            "xyz": np.ascontiguousarray(xyz, np.float32)}


def scene_xyz(rng, N, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """N points of mixed sign with a few exact zeros of both signs in every column."""
    xyz = ((rng.random((N, 3)) - 0.5) * np.array([6.0, 4.0, 2.5]) * scale + np.asarray(shift)).astype(np.float32)
    if N >= 8:
        z = rng.choice(N, size=8, replace=False)
        xyz[z[:4], rng.integers(0, 3, 4)] = 0.0
        xyz[z[4:], rng.integers(0, 3, 4)] = -0.0
    return xyz


def member_counts(c):
    return MEMBER_EDGE + (c - 1, c, c + 1, 2 * c + 1)


def member_count_rows_case(rng, c, **kw):
    """Rows form: one mask per member count of member_counts(c) over a scene of 2 c + 38 points, the members scattered
    (so the masks overlap), mask values other than 1, the picks shuffled with two out of range among them."""
    counts = member_counts(c)
    N = 2 * c + 38
    masks = np.zeros((len(counts), N), np.int32)
    for r, m in enumerate(counts):
        masks[r, rng.choice(N, size=m, replace=False)] = rng.choice([1, 2, -3, 255, 1 << 30], size=m)
    pick = np.concatenate([rng.permutation(len(counts)), [-1, len(counts)]])
    return rows_case(masks, rng.permutation(pick), scene_xyz(rng, N, **kw))


def member_count_ids_case(rng, c, counts, **kw):
    """Ids form: disjoint groups of the given member counts scattered through a scene with 29 points of no group."""
    N = int(sum(counts)) + 29
    group = np.full(N, -1, np.int32)
    group[:sum(counts)] = np.repeat(np.arange(len(counts)), counts)
    return ids_case(rng.permutation(group), len(counts), scene_xyz(rng, N, **kw))


def host_rows(case, angles):
    """(count, aligned rows, oriented rows) of a case by the numpy statements."""
    from geoformer_amd import postprocess

    if case["form"] == "rows":
        return postprocess.instance_boxes_host(case["masks"], case["pick"], case["xyz"], angles)
    return postprocess.id_boxes_host(case["group"], case["n_groups"], case["xyz"], angles)


def lattice(index, angles=90, shift=(3.0, -1.0, 0.25)):
    """A 5 x 3 lattice with spacing 0.5 and 0.25, turned by entry `index` of the angle table and shifted; z in [0, 1]."""
    from geoformer_amd import postprocess

    t = postprocess.box_angle_table(angles).astype(np.float64)
    c, s = t[index]
    u, v = [a.ravel() for a in np.meshgrid(np.arange(5) * 0.5, np.arange(3) * 0.25, indexing="ij")]
    z = np.linspace(0.0, 1.0, u.shape[0])
    return (np.stack([u * c - v * s, u * s + v * c, z], axis=1) + np.asarray(shift)).astype(np.float32)


def box_rows(*boxes):
    """Packed rows of hand-made boxes: (centre, size) or (centre, size, (c, s))."""
    out = []
    for b in boxes:
        c, s = b[2] if len(b) > 2 else (1.0, 0.0)
        out.append([*b[0], *b[1], float(c), float(s), 0.0, 1.0])
    return np.array(out, np.float64).reshape(-1, 10)


def table_entry(index, angles=90):
    from geoformer_amd import postprocess

    return tuple(np.float64(v) for v in postprocess.box_angle_table(angles)[index])


UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def iou_pairs():
    """(a rows, b rows, expected IoU, tolerance) of the hand-derived pairs; tolerance 0 means exactly."""
    e45 = table_entry(45)
    return [
        (box_rows(UNIT), box_rows(UNIT), 1.0, 0.0),
        (box_rows(((0.3, -2.0, 7.0), (0.7, 1.3, 2.9))), box_rows(((0.3, -2.0, 7.0), (0.7, 1.3, 2.9))), 1.0, 0.0),
        (box_rows(UNIT), box_rows(((0.5, 0.0, 0.0), (1.0, 1.0, 1.0))), 1.0 / 3.0, 0.0),
        (box_rows(UNIT), box_rows(((1.0, 0.0, 0.0), (1.0, 1.0, 1.0))), 0.0, 0.0),  # a shared face
        (box_rows(UNIT), box_rows(((0.0, 0.0, 1.0), (1.0, 1.0, 1.0))), 0.0, 0.0),
        (box_rows(UNIT), box_rows(((3.0, 0.5, 0.0), (1.0, 1.0, 1.0))), 0.0, 0.0),  # disjoint
        (box_rows(UNIT), box_rows(((0.125, -0.25, 0.0), (0.5, 0.5, 0.5))), 0.125, 0.0),  # contains a cube of half the side
        # c and s are fp32 roundings of sqrt(1/2), relative error 2^-24; the IoU moves by a small multiple of that
        (box_rows(UNIT), box_rows((*UNIT, e45)), 1.0 / np.sqrt(2.0), 1e-6),
        (box_rows((*UNIT, e45)), box_rows(UNIT), 1.0 / np.sqrt(2.0), 1e-6),
        (box_rows(((0.0, 0.0, 0.0), (0.0, 1.0, 1.0))), box_rows(UNIT), 0.0, 0.0),  # no volume
        (box_rows(UNIT), box_rows(((0.0, 0.0, 0.0), (1.0, 0.0, 1.0), e45)), 0.0, 0.0),
        (box_rows(((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))), box_rows(((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))), 0.0, 0.0),
    ]


def mixed_iou_case(rng, P=7, G=5, angles=90):
    """(a rows [P, 10], b rows [G, 10]) of overlapping random groups, oriented, from the box statement itself; the last
    box of b is made axis-aligned by hand so that some pairs have exactly one s == 0."""
    from geoformer_amd import postprocess

    def boxes(k, seed_shift):
        xyz, group = [], []
        for r in range(k):
            m = int(rng.integers(5, 40))
            th = rng.random() * np.pi
            p = rng.standard_normal((m, 3)) * np.array([0.9, 0.3, 0.4])
            rot = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
            xyz.append(p @ rot.T + rng.random(3) * 0.8 + seed_shift)
            group += [r] * m
        return postprocess.id_boxes_host(np.array(group, np.int32), k, np.concatenate(xyz).astype(np.float32), angles)[2]

    a, b = boxes(P, 0.0), boxes(G, 0.1).copy()
    b[-1, 6:9] = (1.0, 0.0, 0.0)
    return a, b
