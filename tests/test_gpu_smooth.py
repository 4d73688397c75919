"""The adjacency and the smoothing on the GPU (adgs.smooth over include/adgs_smooth.h, csrc/smooth.hip) against tests/smooth_ref.py on the
cases of tests/smooth_cases.py.

Integers.  starts, neighbors, boundary and the counts are functions of the mesh alone: EQUAL to the oracle as integers, from run to run and
in any face order.
Smoothed vertices: EQUAL to the oracle AS BITS.  Derived, not measured: the state is float64 on both sides, a row is summed in ascending
neighbour order from 0.0 on both sides, a step is one IEEE division, subtraction, multiplication and addition per component (the object is
built without FMA contraction), and the float32 rounding happens once -- there is no operation whose result may differ.
Every property asserted here is asserted of the oracle in tests/test_smooth_ref.py."""
import numpy as np
import pytest
import torch

from tests import mesh_cases
from tests import smooth_cases as cases

pytestmark = pytest.mark.gpu

ITERATIONS = (0, 1, 2, 10)


def up(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def device_case(name):
    v, f = cases.mesh(name)
    return up(v), up(f)


def same_adjacency(got, want, what):
    for field, dtype in (("starts", np.int32), ("neighbors", np.int32), ("boundary", np.bool_)):
        g = host(getattr(got, field))
        w = getattr(want, field)
        w = host(w) if torch.is_tensor(w) else w
        assert getattr(got, field).is_cuda and g.dtype == dtype and g.shape == w.shape and np.array_equal(g, w), (what, field)
    assert got.counts == want.counts, (what, got.counts, want.counts)


@pytest.mark.parametrize("name", cases.NAMES)
def test_adjacency_equals_the_oracle(name):
    from adgs import smooth
    v, f = device_case(name)
    want = cases.adjacency(name)
    before = f.clone()
    got = smooth.mesh_adjacency(f, v.shape[0])
    same_adjacency(got, want, name)
    assert len(got) == want.counts["edges"] and torch.equal(got.degree(), got.starts[1:] - got.starts[:-1])
    assert all(isinstance(n, int) for n in got.counts.values()) and got.counts["bad_faces"] == 0
    same_adjacency(smooth.mesh_adjacency(f, v.shape[0]), got, name + " again")
    assert torch.equal(f, before)


def test_adjacency_does_not_depend_on_the_face_order():
    from adgs import smooth
    (v, f), (_, fp) = device_case("patch"), device_case("patch_perm")
    assert not torch.equal(f, fp)
    same_adjacency(smooth.mesh_adjacency(fp, v.shape[0]), smooth.mesh_adjacency(f, v.shape[0]), "patch_perm")


@pytest.mark.parametrize("boundary", ("fixed", "free"))
@pytest.mark.parametrize("method", ("taubin", "laplacian"))
@pytest.mark.parametrize("name", cases.SMOOTHED)
def test_smoothed_bits_equal_the_oracle(name, method, boundary):
    from adgs import smooth
    v, f = device_case(name)
    vin, fin = v.clone(), f.clone()
    adj = smooth.mesh_adjacency(f, v.shape[0])
    for it in ITERATIONS:
        want = cases.smoothed(name, it, method, boundary=boundary)
        got = smooth.smooth_mesh(v, f, it, method=method, boundary=boundary, adjacency=adj)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == v.shape and got.data_ptr() != v.data_ptr()
        differ = int((bits(host(got)) != bits(want)).sum())
        print("%s %s %s iterations %d: %d of %d coordinates differ from the oracle" % (name, method, boundary, it, differ, want.size))
        assert differ == 0, (name, method, boundary, it)
        if it == 0:
            assert np.array_equal(bits(host(got)), bits(cases.mesh(name)[0]))
    # built inside the call: the same bits
    inside = smooth.smooth_mesh(v, f, 2, method=method, boundary=boundary)
    assert np.array_equal(bits(host(inside)), bits(cases.smoothed(name, 2, method, boundary=boundary)))
    assert torch.equal(v, vin) and torch.equal(f, fin)          # neither input is written


def test_the_hub_of_the_fan_moves_with_a_free_boundary():
    from adgs import smooth
    v, f = device_case("fan")
    out = smooth.smooth_mesh(v, f, 1, method="laplacian", boundary="free")
    assert cases.adjacency("fan").degree()[2048] == 4096 and not torch.equal(out[2048], v[2048])
    held = smooth.smooth_mesh(v, f, 1, method="laplacian")      # the rim is all boundary: only the hub moves
    rim = torch.ones(v.shape[0], dtype=torch.bool, device="cuda")
    rim[2048] = False
    assert torch.equal(held[rim].view(torch.int32), v[rim].view(torch.int32)) and torch.equal(held[2048], out[2048])


@pytest.mark.parametrize("name", ("tsdf", "patch_dup"))
def test_other_factors_and_a_user_mask(name):
    from adgs import smooth
    v, f = device_case(name)
    mask = up(cases.user_mask(name))
    for method, boundary in (("taubin", "fixed"), ("laplacian", "free")):
        got = smooth.smooth_mesh(v, f, 2, method=method, lam=0.33, mu=-0.34, boundary=boundary)
        assert np.array_equal(bits(host(got)), bits(cases.smoothed(name, 2, method, 0.33, -0.34, boundary))), (name, method)
        got = smooth.smooth_mesh(v, f, 2, method=method, boundary=boundary, fixed=mask)
        assert np.array_equal(bits(host(got)), bits(cases.smoothed(name, 2, method, boundary=boundary, masked=True))), (name, method)
        assert torch.equal(got[mask].view(torch.int32), v[mask].view(torch.int32))
    got = smooth.smooth_mesh(v, f, 1, lam=1.0, mu=-1.5, check=False)
    assert np.array_equal(bits(host(got)), bits(cases.smoothed(name, 1, "taubin", 1.0, -1.5)))


@pytest.mark.parametrize("name", ("repeated", "patch", "patch_dup", "strip"))
def test_fixed_boundary_and_isolated_vertices_keep_their_bits(name):
    from adgs import smooth
    v, f = device_case(name)
    adj = smooth.mesh_adjacency(f, v.shape[0])
    isolated = adj.degree() == 0
    for method in ("taubin", "laplacian"):
        out = smooth.smooth_mesh(v, f, 10, method=method, adjacency=adj)
        still = adj.boundary | isolated
        assert torch.equal(out[still].view(torch.int32), v[still].view(torch.int32)), (name, method)
        if name == "strip":
            assert bool(still.all())
        elif name != "repeated":
            assert not torch.equal(out[~still], v[~still])
        free = smooth.smooth_mesh(v, f, 10, method=method, boundary="free", adjacency=adj)
        assert torch.equal(free[isolated].view(torch.int32), v[isolated].view(torch.int32)), (name, method)


def test_faces_outside_the_vertices_and_non_finite_vertices_are_refused():
    from adgs import smooth
    v, f = device_case(mesh_cases.BAD)
    assert int(f.min()) == -1 and int(f.max()) == v.shape[0]
    with pytest.raises(ValueError, match="mesh_adjacency: 2 faces index outside the 7 vertices"):
        smooth.mesh_adjacency(f, v.shape[0])
    with pytest.raises(ValueError, match="smooth_mesh: 2 faces index outside the 7 vertices"):
        smooth.smooth_mesh(v, f)
    with pytest.raises(ValueError, match="mesh_adjacency: 1 faces index outside the 0 vertices"):
        smooth.mesh_adjacency(up(np.zeros((1, 3), np.int32)), 0)
    v, f = device_case("patch")
    w = v.clone()
    w[200, 1] = float("nan")
    with pytest.raises(ValueError, match="smooth_mesh: vertices must be finite"):
        smooth.smooth_mesh(w, f)
    got = smooth.smooth_mesh(w, f, 1, method="laplacian", boundary="free", check=False)
    from tests import smooth_ref
    want = smooth_ref.smooth(host(w), host(f), 1, "laplacian", boundary="free")
    assert np.array_equal(np.isnan(host(got)), np.isnan(want)) and np.isnan(want).sum() == 1 + cases.adjacency("patch").degree()[200]
    ok = ~np.isnan(want)
    assert np.array_equal(bits(host(got))[ok], bits(want)[ok])


@pytest.mark.parametrize("name", ("points", "empty", "no_faces"))
def test_meshes_without_faces_come_back_as_they_are(name):
    from adgs import smooth
    if name == "no_faces":
        v, f = device_case("tsdf")
        f = f[:0]
    else:
        v, f = device_case(name)
    V = v.shape[0]
    adj = smooth.mesh_adjacency(f, V)
    assert len(adj) == 0 and adj.neighbors.shape == (0,) and adj.starts.tolist() == [0] * (V + 1) and adj.boundary.tolist() == [False] * V
    assert adj.counts == dict(edges=0, boundary_edges=0, nonmanifold_edges=0, degenerate_faces=0, isolated_vertices=V, bad_faces=0)
    for method in ("taubin", "laplacian"):
        out = smooth.smooth_mesh(v, f, method=method, boundary="free")
        assert out.shape == (V, 3) and torch.equal(out.view(torch.int32), v.view(torch.int32))
        assert V == 0 or out.data_ptr() != v.data_ptr()


def test_composes_with_vertex_normals():
    """The next step of the pipeline on the smoothed mesh: the device's normals of the device's smoothed vertices are those of
    tests/mesh_ref.py on the oracle's smoothed vertices, within the 2^-23 that tests/test_gpu_mesh.py allows a normal (the vertices are
    equal as bits), the vertices whose sum is a cancellation left out as there."""
    from adgs import mesh, smooth
    from tests import mesh_ref
    v, f = device_case("tsdf")
    out = smooth.smooth_mesh(v, f)
    want = cases.smoothed("tsdf")
    assert np.array_equal(bits(host(out)), bits(want))
    normals = mesh.vertex_normals(out, f)
    n, _, flagged = mesh_ref.normals(want, cases.mesh("tsdf")[1])
    g = host(normals)
    assert normals.dtype == torch.float32 and g.shape == n.shape and np.isfinite(g).all() and flagged.sum() <= 0.005 * len(n)
    assert (np.abs(g.astype(np.float64) - n)[~flagged] <= 2.0 ** -23).all()
