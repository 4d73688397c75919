"""Pins tests/smooth_ref.py, the oracle of tests/test_gpu_smooth.py, without a GPU: its adjacency against a plain Python construction with
sets, its step against a per-vertex Python loop, the exact properties of the definition (include/adgs_smooth.h), and that the operator
does what it is for: it removes noise, and Taubin's variant does not shrink the mesh where Laplacian smoothing does."""
import numpy as np
import pytest

from tests import mesh_cases
from tests import smooth_cases as cases
from tests import smooth_ref as ref

SMALL = ("triangle", "bowtie", "repeated", "patch", "patch_dup")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def python_adjacency(faces, V):
    rows = [set() for _ in range(V)]
    inc, degenerate, bad = {}, 0, 0
    for face in faces.tolist():
        if not all(0 <= i < V for i in face):
            bad += 1
            continue
        repeated = False
        for k in range(3):
            a, b = face[k], face[(k + 1) % 3]
            if a == b:
                repeated = True
                continue
            rows[a].add(b)
            rows[b].add(a)
            e = frozenset((a, b))
            inc[e] = inc.get(e, 0) + 1
        degenerate += repeated
    boundary = [False] * V
    for e, n in inc.items():
        if n == 1:
            for i in e:
                boundary[i] = True
    counts = dict(edges=len(inc), boundary_edges=sum(n == 1 for n in inc.values()), nonmanifold_edges=sum(n > 2 for n in inc.values()),
                  degenerate_faces=degenerate, isolated_vertices=sum(not r for r in rows), bad_faces=bad)
    return [sorted(r) for r in rows], boundary, counts


@pytest.mark.parametrize("name", cases.NAMES + (mesh_cases.BAD,))
def test_adjacency_equals_a_construction_with_sets(name):
    v, f = cases.mesh(name)
    V = len(v)
    adj = cases.adjacency(name)
    rows, boundary, counts = python_adjacency(f, V)
    assert adj.starts.dtype == np.int32 and adj.neighbors.dtype == np.int32 and adj.boundary.dtype == bool
    assert adj.starts.shape == (V + 1,) and adj.starts[0] == 0 and adj.starts[-1] == len(adj.neighbors) == 2 * counts["edges"]
    assert [adj.neighbors[adj.starts[i]:adj.starts[i + 1]].tolist() for i in range(V)] == rows
    assert adj.boundary.tolist() == boundary and adj.counts == counts
    assert adj.degree().tolist() == [len(r) for r in rows]


def test_what_the_cases_are():
    """The figures the cases were chosen for."""
    c = cases.adjacency("tsdf").counts
    assert (c["edges"], c["boundary_edges"], c["nonmanifold_edges"], c["degenerate_faces"]) == (14118, 0, 0, 0) and cases.adjacency("tsdf").degree().max() == 10
    assert cases.adjacency("fan").degree().max() == 4096
    c = cases.adjacency("repeated").counts
    assert (c["boundary_edges"], c["nonmanifold_edges"], c["degenerate_faces"], c["isolated_vertices"]) == (2, 2, 4, 1)
    for name in ("strip", "scattered"):
        a = cases.adjacency(name)
        assert a.boundary[a.degree() > 0].all() and a.counts["boundary_edges"] > 0
    assert cases.adjacency(mesh_cases.BAD).counts["bad_faces"] == 2
    v, f = cases.mesh("patch")
    a = cases.adjacency("patch")
    assert (len(v), len(f)) == (612, 1122) and len(v) % 256 != 0 and (6 * len(f)) % 256 != 0
    assert a.counts == dict(edges=612 + 1122 - 1, boundary_edges=2 * (33 + 17), nonmanifold_edges=0, degenerate_faces=0, isolated_vertices=0, bad_faces=0)
    assert 0 < a.boundary.sum() == 2 * (33 + 17) < len(v)       # interior and boundary vertices together
    d = cases.adjacency("patch_dup")
    assert d.counts["degenerate_faces"] == 1 and d.counts["isolated_vertices"] == 1 and d.counts["nonmanifold_edges"] > 0
    assert d.counts["edges"] == a.counts["edges"] + 1          # the degenerate face's edge is a new one


def python_step(x, rows, s, fixed):
    out = [list(p) for p in x.tolist()]
    for i, row in enumerate(rows):
        if not row or fixed[i]:
            continue
        for c in range(3):
            S = 0.0
            for j in row:
                S = S + float(x[j, c])
            out[i][c] = float(x[i, c]) + s * (S / float(len(row)) - float(x[i, c]))
    return np.array(out, np.float64).reshape(-1, 3)


@pytest.mark.parametrize("name", SMALL)
def test_step_equals_a_loop_over_the_vertices(name):
    v, f = cases.mesh(name)
    adj = cases.adjacency(name)
    rows, _, _ = python_adjacency(f, len(v))
    x = v.astype(np.float64)
    for s, fixed in ((0.5, adj.boundary), (-0.53, np.zeros(len(v), bool)), (0.37, cases.user_mask(name))):
        got, want = ref.step(x, adj, s, fixed), python_step(x, rows, s, fixed)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (name, s)
        x = got
    # the whole operator is the steps in their order and one rounding
    y = v.astype(np.float64)
    for s in (0.5, -0.53, 0.5, -0.53):
        y = python_step(y, rows, s, adj.boundary)
    assert np.array_equal(bits(ref.smooth(v, f, 2)), bits(y.astype(np.float32)))
    y = v.astype(np.float64)
    for s in (0.3, 0.3, 0.3):
        y = python_step(y, rows, s, np.zeros(len(v), bool))
    assert np.array_equal(bits(ref.smooth(v, f, 3, "laplacian", lam=0.3, boundary="free")), bits(y.astype(np.float32)))


@pytest.mark.parametrize("name", cases.SMOOTHED)
def test_exact_properties(name):
    v, f = cases.mesh(name)
    adj = cases.adjacency(name)
    for method in ("taubin", "laplacian"):
        for boundary in ("fixed", "free"):
            assert np.array_equal(bits(ref.smooth(v, f, 0, method, boundary=boundary, adj=adj)), bits(v))
    mask = cases.user_mask(name)
    out = cases.smoothed(name, 2, "taubin", masked=True)
    still = mask | adj.boundary | (adj.degree() == 0)
    assert np.array_equal(bits(out)[still], bits(v)[still])
    free = cases.smoothed(name, 2, "laplacian", boundary="free")
    isolated = adj.degree() == 0
    assert np.array_equal(bits(free)[isolated], bits(v)[isolated])
    if (~still).any():
        assert (bits(out)[~still] != bits(v)[~still]).any()     # the others did move


def test_face_order_and_duplicates():
    v, f = cases.mesh("patch")
    a = cases.adjacency("patch")
    p = cases.adjacency("patch_perm")
    for field in ("starts", "neighbors", "boundary"):
        assert np.array_equal(getattr(a, field), getattr(p, field)), field
    assert a.counts == p.counts
    for boundary in ("fixed", "free"):
        assert np.array_equal(bits(cases.smoothed("patch", 2, boundary=boundary)), bits(cases.smoothed("patch_perm", 2, boundary=boundary)))
    twice = np.concatenate([f, f[::3]])
    d = ref.adjacency(twice, len(v))
    assert np.array_equal(d.starts, a.starts) and np.array_equal(d.neighbors, a.neighbors)
    assert d.counts["nonmanifold_edges"] > 0 and not np.array_equal(d.incidence, a.incidence) and not np.array_equal(d.boundary, a.boundary)
    assert np.array_equal(bits(ref.smooth(v, twice, 2, boundary="free")), bits(cases.smoothed("patch", 2, boundary="free")))
    # tsdf_perm permutes the vertices too: the smoothed mesh is the permuted smoothed mesh in value (the rows are summed in another order)
    assert cases.adjacency("tsdf").counts == cases.adjacency("tsdf_perm").counts


def test_a_mesh_of_boundary_vertices_stays_with_a_fixed_boundary():
    v, f = cases.mesh("strip")
    assert np.array_equal(bits(ref.smooth(v, f, 10, adj=cases.adjacency("strip"))), bits(v))
    assert not np.array_equal(bits(ref.smooth(v, f, 1, boundary="free", adj=cases.adjacency("strip"))), bits(v))


def test_non_finite_values_spread_to_the_neighbours_only():
    v, f = cases.mesh("patch")
    adj = cases.adjacency("patch")
    w = v.copy()
    w[200, 1] = np.nan
    out = ref.smooth(w, f, 1, "laplacian", boundary="free", adj=adj)
    bad = np.zeros(len(v), bool)
    bad[200] = True
    bad[adj.neighbors[adj.starts[200]:adj.starts[201]]] = True
    assert np.isnan(out[bad, 1]).all() and np.isfinite(out[~bad]).all() and np.isfinite(out[:, [0, 2]]).all()


def test_removes_noise_and_taubin_does_not_shrink():
    """tsdf plus Gaussian noise of 0.25 median edge lengths.  Measured with this reference: the RMS umbrella residual goes from 0.360 to
    0.070 after 10 Taubin iterations (0.032 after 10 Laplacian steps), the mean distance to the centroid by a factor of 0.99997 (Taubin)
    and 0.99494 (Laplacian).  The residual's threshold is twice what was measured; the two shrinkages are compared with each other."""
    v, f = cases.mesh("tsdf")
    adj = cases.adjacency("tsdf")
    x = v.astype(np.float64)
    length = np.median(np.linalg.norm(x[adj.edges[:, 0]] - x[adj.edges[:, 1]], axis=1))
    noisy = (x + 0.25 * length * np.random.default_rng(7).standard_normal(x.shape)).astype(np.float32)
    taubin = ref.smooth(noisy, f, 10, "taubin", adj=adj)
    laplacian = ref.smooth(noisy, f, 10, "laplacian", adj=adj)
    r0, rt, rl = (ref.umbrella_residual(m, adj) for m in (noisy, taubin, laplacian))
    spread = lambda m: np.linalg.norm(m.astype(np.float64) - m.astype(np.float64).mean(0), axis=1).mean()
    st, sl = spread(taubin) / spread(noisy), spread(laplacian) / spread(noisy)
    print("median edge %.4f; residual %.4f -> taubin %.4f, laplacian %.4f; mean distance to the centroid x %.5f (taubin), x %.5f (laplacian)" % (
        length, r0, rt, rl, st, sl))
    assert rt < r0 and rt < 0.14 and rl < r0
    assert abs(st - 1.0) < abs(sl - 1.0) and sl < 1.0
