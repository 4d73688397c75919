"""The oracle of the simplification (tests/simplify_ref.py) checked against itself, without a GPU: its dedupe against a Python set, its
quadric solution against the stationarity of the objective, and every property and inequality that tests/test_gpu_simplify.py asserts of
the device -- identity, weld, crease, sphere distance -- on the oracle first."""
import numpy as np
import pytest

from tests import simplify_cases as cases
from tests import simplify_ref as ref


def rotations(t):
    a, b, c = (int(x) for x in t)
    return {(a, b, c), (b, c, a), (c, a, b)}


@pytest.mark.parametrize("name", ["duplicates", "grid_coarse", "tsdf_3.7", "long_run", "nonfinite"])
def test_dedupe_equals_a_set_of_rotated_triples(name):
    c = cases.case(name)
    cl, _ = cases.reference(name)
    v, f = c["vertices"], c["faces"]
    cell_of = lambda i: tuple(ref.cells_of(v[i:i + 1], cl.cell, cl.origin)[0]) if np.isfinite(v[i]).all() else None
    ids = {}                                                    # cell -> an id of its own
    seen, keep, counts = set(), [], {"dropped_faces": 0, "degenerate_faces": 0, "duplicate_faces": 0}
    for k, face in enumerate(f):
        cs = [cell_of(int(i)) for i in face]
        if None in cs:
            counts["dropped_faces"] += 1
            continue
        t = tuple(ids.setdefault(x, len(ids)) for x in cs)
        if len(set(t)) < 3:
            counts["degenerate_faces"] += 1
        elif rotations(t) & seen:
            counts["duplicate_faces"] += 1
        else:
            seen.add(t)
            keep.append(k)
    assert cl.face_source.tolist() == keep
    assert {k: cl.counts[k] for k in counts} == counts
    assert cl.counts["nonfinite_vertices"] == int((~np.isfinite(v).all(axis=1)).sum())
    # the output: no unused vertex, roots ascending, the members a partition in ascending vertex id, corner order kept
    assert np.array_equal(np.unique(cl.faces), np.arange(len(cl.root))) and (np.diff(cl.root) > 0).all()
    assert np.array_equal(cl.faces, cl.vertex_cluster[f[cl.face_source]])
    for d in range(len(cl.root)):
        m = cl.members[cl.member_starts[d]:cl.member_starts[d + 1]]
        assert m[0] == cl.root[d] and (np.diff(m) > 0).all() and (cl.vertex_cluster[m] == d).all() and len(m) == cl.num_vertices[d]
    assert cl.member_starts[-1] == (cl.vertex_cluster >= 0).sum() == len(cl.members)


def test_duplicates_by_hand():
    cl, _ = cases.reference("duplicates")
    assert cl.face_source.tolist() == [0, 3, 5, 10, 11]
    assert cl.counts == {"nonfinite_vertices": 0, "dropped_faces": 0, "degenerate_faces": 2, "duplicate_faces": 5}
    assert cl.vertex_cluster.tolist() == [0, 1, 2, 3, 4, 5, 0] and cl.root.tolist() == [0, 1, 2, 3, 4, 5] and cl.num_vertices.tolist() == [2, 1, 1, 1, 1, 1]
    assert cl.faces.tolist() == [[0, 1, 2], [0, 2, 1], [3, 4, 5], [1, 3, 2], [4, 3, 5]]


@pytest.mark.parametrize("name", ["grid_coarse", "tsdf_2.0", "crease", "long_run"])
def test_quadric_solution_is_stationary_where_the_clamp_is_inactive(name):
    """d/d delta of sum w (n . delta - e)^2 + lambda t |delta|^2 = 2 (A delta - g + lambda t delta) = 0."""
    c = cases.case(name)
    cl, _ = cases.reference(name)
    lam = 1e-3
    cbar, A, g, t = ref.quadrics(cl, c["vertices"], c["faces"])
    _, free, clamped, (dmin, dmax) = ref.solve(cl, c["vertices"], c["faces"], lam)
    inactive = (free == clamped).all(axis=1) & (t > 0)
    assert inactive.sum() > 0.5 * len(t)
    grad = np.einsum("nij,nj->ni", A, clamped) - g + lam * t[:, None] * clamped
    scale = np.abs(g).max(axis=1) + t * np.abs(clamped).max(axis=1) + 1e-300
    assert (np.abs(grad[inactive]).max(axis=1) <= 1e-11 * scale[inactive]).all()
    # the clamp keeps the vertex in the closed cell and never moves a zero
    lo, hi = ref.cell_box(cl, c["vertices"])
    assert ((cbar + clamped >= lo - 1e-9) & (cbar + clamped <= hi + 1e-9)).all()
    assert (dmin <= 0).all() and (dmax >= 0).all()


@pytest.mark.parametrize("name", cases.TINY)
def test_tiny(name):
    c = cases.case(name)
    cl, placed = cases.reference(name)
    if name == "three_cells":
        assert np.array_equal(cl.faces, c["faces"]) and cl.vertex_cluster.tolist() == [0, 1, 2]
        for p in placed.values():
            assert np.array_equal(p[0].view(np.uint32), c["vertices"].view(np.uint32)) and np.array_equal(p[1], c["colors"])
        return
    assert len(cl.root) == len(cl.faces) == len(cl.members) == 0 and cl.member_starts.tolist() == [0] and (cl.vertex_cluster == -1).all()
    assert cl.counts["degenerate_faces"] == (1 if name == "one_cell" else 0)
    assert all(p[0].shape == (0, 3) for p in placed.values())


def test_identity():
    c = cases.case("identity")
    cl, placed = cases.reference("identity")
    V, F = len(c["vertices"]), len(c["faces"])
    assert V == 20480 and np.array_equal(cl.vertex_cluster, np.arange(V)) and np.array_equal(cl.face_source, np.arange(F))
    assert np.array_equal(cl.faces, c["faces"]) and np.array_equal(cl.root, np.arange(V)) and (cl.num_vertices == 1).all()
    for p in placed.values():
        assert np.array_equal(p[0].view(np.uint32), c["vertices"].view(np.uint32))
        assert np.array_equal(p[1].view(np.uint32), c["colors"].view(np.uint32))


def test_grid_coarse_has_cells_of_both_signs_and_merges():
    c = cases.case("grid_coarse")
    cl, _ = cases.reference("grid_coarse")
    cells = ref.cells_of(c["vertices"], cl.cell, cl.origin)
    assert (cells.min(axis=0) < 0).all() and (cells.max(axis=0)[:2] > 0).all()
    # 6.25 vertices per cell column, split over the two z cells the jitter reaches
    assert 0 < len(cl.root) < len(c["vertices"]) / 2 and cl.counts["degenerate_faces"] > 0 and cl.counts["duplicate_faces"] > 0


@pytest.mark.parametrize("name", ["tsdf_2.0", "tsdf_3.7"])
def test_quadric_placement_is_nearer_the_spheres(name):
    _, placed = cases.reference(name)
    roots = cases.sphere_roots(name)
    q, a = cases.sphere_distance(placed["quadric"][0], roots), cases.sphere_distance(placed["average"][0], roots)
    print("%s: %d vertices on the spheres; mean distance quadric %.4f, average %.4f" % (name, roots.sum(), q, a))
    assert roots.sum() > 50 and q < a


def test_crease_quadric_vertex_lies_on_both_planes():
    """A straddling cluster has equal areas on both sides: the quadric vertex is at 2 lambda / (1 + 2 lambda) of the mean's distance from
    each plane, about 0.002; the bound 0.01 leaves a factor 5 for the end clusters, whose two sides are not quite equal."""
    _, placed = cases.reference("crease")
    s = cases.crease_straddlers()
    assert s.sum() >= 3
    q, a = placed["quadric"][0].astype(np.float64)[s], placed["average"][0].astype(np.float64)[s]
    for axis in (0, 2):                                         # the planes x = 0 and z = 0
        ratio = np.abs(q[:, axis]) / np.abs(a[:, axis])
        print("crease: distance to the plane %s = 0: quadric / average %.5f .. %.5f" % ("xyz"[axis], ratio.min(), ratio.max()))
        assert (np.abs(a[:, axis]) > 0.2).all() and (ratio <= 0.01).all()


def test_long_run_and_nonfinite():
    cl, _ = cases.reference("long_run")
    assert cl.num_vertices.max() == 5000 and cl.counts["duplicate_faces"] == 4999 and len(cl.faces) == 2
    c = cases.case("nonfinite")
    cl, placed = cases.reference("nonfinite")
    assert cl.counts["nonfinite_vertices"] == 4 and cl.counts["dropped_faces"] > 0
    assert (cl.vertex_cluster[[17, 40, 41, 100]] == -1).all() and all(np.isfinite(p[0]).all() for p in placed.values())


def test_weld_removes_exactly_the_seam():
    c = cases.case("weld")
    cl, placed = cases.reference("weld")
    V, ny = len(c["vertices"]), cases.GRID[1]
    assert V == 20480 + ny and len(cl.root) == V - ny and cl.counts["degenerate_faces"] == cl.counts["duplicate_faces"] == 0
    assert len(cl.faces) == len(c["faces"]) and sorted(np.unique(cl.num_vertices).tolist()) == [1, 2]
    # the welded vertices are where they were: the mean of two equal positions
    assert np.array_equal(placed["quadric"][0].view(np.uint32), c["vertices"][cl.root].view(np.uint32))


def test_refusals():
    v = np.zeros((3, 3), np.float32)
    with pytest.raises(ValueError, match="2 faces index outside the 3 vertices"):
        ref.cluster(v, [[0, 1, 2], [0, 1, 3], [-1, 1, 2]], 1.0)
    with pytest.raises(ValueError, match="enlarge cell_size or move origin"):
        ref.cluster(np.array([[0, 0, 0], [1e9, 0, 0], [0, 1, 0]], np.float32), [[0, 1, 2]], 0.01)
