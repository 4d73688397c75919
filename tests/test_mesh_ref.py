"""The numpy reference of the mesh clean-up (tests/mesh_ref.py) against independent statements of include/adgs_mesh.h, on the cases of
tests/mesh_cases.py: what the GPU tests compare against must itself be right."""
import numpy as np
import pytest

from tests import mesh_cases as cases
from tests import mesh_ref as ref

ALL = cases.NAMES + (cases.BAD,)


@pytest.mark.parametrize("name", ALL)
def test_components_equal_a_breadth_first_search(name):
    v, f = cases.mesh(name)
    comps, _ = cases.reference(name)
    V = len(v)
    label = ref.bfs_components(f, V)
    assert np.array_equal(comps.root[comps.vertex_component] if V else np.zeros(0), label)
    assert np.array_equal(comps.root, np.unique(label)) and (np.diff(comps.root) > 0).all()
    assert comps.num_vertices.sum() == V and comps.num_faces.sum() == ref.valid_faces(f, V).sum()
    assert np.array_equal(comps.num_vertices, np.bincount(comps.vertex_component, minlength=len(comps.root)))
    want = {"empty": 0, "points": 7, "triangle": 1, "bowtie": 1, "strip": 1, "strip_reversed": 1, "strip_permuted": 1, "fan": 1, "scattered": 4000,
            "tsdf": 2 + len(cases.BLOBS), "tsdf_perm": 2 + len(cases.BLOBS), "repeated": 2, cases.BAD: 2}
    assert len(comps.root) == want[name]
    if len(f):
        assert np.isclose(comps.area.sum(), ref.face_areas(v, f[ref.valid_faces(f, V)]).sum(), rtol=1e-12)


@pytest.mark.parametrize("a, b", [("strip", "strip_reversed"), ("strip", "strip_permuted"), ("tsdf", "tsdf_perm")])
def test_components_are_invariant_under_permutation(a, b):
    """The same partition with the same counts; only the numbering (by smallest vertex index) moves."""
    ca, cb = cases.reference(a)[0], cases.reference(b)[0]
    assert sorted(zip(ca.num_faces.tolist(), ca.num_vertices.tolist())) == sorted(zip(cb.num_faces.tolist(), cb.num_vertices.tolist()))
    assert np.allclose(np.sort(ca.area), np.sort(cb.area), rtol=1e-12)
    if a == "tsdf":
        va, _ = cases.mesh(a)
        vb, _ = cases.mesh(b)
        # the vertex at the same position lies in a component of the same size
        key = lambda v: [tuple(r) for r in v.view(np.uint32).tolist()]
        size_a = dict(zip(key(va), ca.num_vertices[ca.vertex_component].tolist()))
        assert all(size_a[k] == n for k, n in zip(key(vb), cb.num_vertices[cb.vertex_component].tolist()))


def test_select_is_the_2dgs_rule():
    n = np.array([500, 40, 60, 60, 7, 300, 60, 55])
    # sort(n)[-K], then max with min_faces, then num_faces >= threshold
    for K, m in ((1, 50), (2, 50), (3, 50), (4, 50), (5, 50), (6, 50), (3, 0), (8, 0), (8, 50), (2, 400)):
        thr = max(np.sort(n)[-K], m)
        assert np.array_equal(ref.select(n, K, m), n >= thr), (K, m)
    assert ref.select(n, 3, 50).tolist() == [True, False, True, True, False, True, True, False]      # the tie at 60: all three stay
    assert ref.select(n, 50, 50).tolist() == (n >= 50).tolist()                                       # C < K: the smallest count, then min_faces
    assert ref.select(n, 50, 0).all()
    assert ref.select(np.zeros(0, int)).shape == (0,)
    assert ref.select(n, 8, 0, area=np.arange(8.0), min_area=3.0).tolist() == [False] * 3 + [True] * 5


@pytest.mark.parametrize("name", ALL)
def test_keep_preserves_order_and_leaves_nothing_of_a_dropped_component(name):
    v, f = cases.mesh(name)
    comps, _ = cases.reference(name)
    C = len(comps.root)
    for mask in (np.ones(C, bool), np.zeros(C, bool), np.arange(C) % 2 == 0, comps.num_faces == 0):
        v2, f2, _, _ = ref.keep(comps, mask, v, f)
        kv = mask[comps.vertex_component] if len(v) else np.zeros(0, bool)
        assert np.array_equal(v2.view(np.uint32), v[kv].view(np.uint32))
        assert len(v2) == comps.num_vertices[mask].sum() and len(f2) == comps.num_faces[mask].sum()
        if len(f2):
            assert f2.min() >= 0 and f2.max() < len(v2)
            old = np.nonzero(kv)[0]
            kept_faces = f[ref.valid_faces(f, len(v))]
            kept_faces = kept_faces[kv[kept_faces[:, 0]]]
            assert np.array_equal(old[f2], kept_faces)           # the same faces, in order, corner order kept
        c2 = ref.components(f2, len(v2))
        assert np.array_equal(c2.num_faces, comps.num_faces[mask]) and np.array_equal(c2.num_vertices, comps.num_vertices[mask])


def test_removing_small_components_leaves_the_two_spheres():
    v, f, c = cases.tsdf_mesh()
    comps, _ = cases.reference("tsdf")
    counts = np.sort(comps.num_faces)
    assert 0 < counts[0] < 50 < counts[-3] < counts[-2]          # blobs on both sides of min_faces, all smaller than a sphere
    v2, f2, c2 = ref.remove_small_components(v, f, c, largest=2)
    on = cases.sphere_vertices(v2)
    assert (on[0] ^ on[1]).all() and on[0].any() and on[1].any()
    assert len(v2) == np.sort(comps.num_vertices)[-2:].sum() and len(f2) == np.sort(comps.num_faces)[-2:].sum()
    assert len(ref.components(f2, len(v2)).root) == 2
    assert tsdf_edge_stats(f2) == (0, 0)                         # still closed surfaces
    assert c2.shape == v2.shape
    # canonical order is kept: vertices in their old order
    kv = np.isin(comps.vertex_component, np.argsort(comps.num_faces)[-2:])
    assert np.array_equal(v2.view(np.uint32), v[kv].view(np.uint32))
    # the defaults (K = 50 > C): min_faces alone decides, and the blobs of three lattice points stay
    assert len(ref.remove_small_components(v, f)[1]) == comps.num_faces[comps.num_faces >= 50].sum() > len(f2)


def tsdf_edge_stats(faces):
    from tests import tsdf_ref
    return tsdf_ref.edge_stats(faces)[:2]


def test_normals_point_outwards_on_the_spheres():
    v, f = cases.mesh("tsdf")
    n, S, flagged = cases.reference("tsdf")[1]
    for (centre, _), on in zip(cases.SPHERES, cases.sphere_vertices(v)):
        radial = v[on].astype(np.float64) - np.array(centre)
        dots = (n[on] * radial).sum(1) / np.linalg.norm(radial, axis=1)
        assert on.sum() > 500 and (dots > 0).all() and dots.mean() > 0.95
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("name", cases.NO_FLAG)
def test_the_reference_flags_no_vertex(name):
    """The GPU test allows 0.5 % flagged vertices; the reference has none in cases 5 to 8."""
    n, S, flagged = cases.reference(name)[1]
    assert not flagged.any()


def test_degenerate_faces_give_exact_zero_normals():
    n, S, flagged = cases.reference("repeated")[1]
    assert (n[[1, 3, 5, 6]] == 0).all() and S[3] == 0 and S[5] == 0 and S[1] > 0 and not flagged.any()
    assert np.allclose(np.linalg.norm(n[[0, 2, 4]], axis=1), 1.0)
    # the out-of-range faces are left out
    v, f = cases.mesh(cases.BAD)
    ok = ref.valid_faces(f, len(v))
    assert ok.tolist() == [True, False, True, False, True]
    assert np.array_equal(cases.reference(cases.BAD)[1][0], ref.normals(v, f[ok])[0])
