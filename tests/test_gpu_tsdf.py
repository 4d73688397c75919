"""TSDF fusion and marching tetrahedra on the GPU (adgs.tsdf over include/adgs_tsdf.h, csrc/tsdf.hip) against tests/tsdf_ref.py (float64
numpy) on the cases of tests/tsdf_cases.py.

Integration.  The views of a case are applied in sequence; after every view, outside the lattice points the reference has flagged as
near a gate in this or an earlier view: a point the reference did not update keeps its BITS, an updated one has tsdf and colour within
2^-22 absolute and wsum within 2^-22 relative.  Both sides evaluate the same double chain from the same float32 inputs and round once per
stored value; they differ by contraction and double rounding only, and 2^-22 is 2 float32 ulps at 1 (every tsdf and colour lies in
[-1, 1]).  A poisoned volume (0.123 / 7 / 0.5) shows that a skipped point is not written.  Edge lattices: 300 x 5 x 4 and 257 x 3 x 2 at
2 cm (chunk and wave boundaries in x inside the frustum), 1 x 1 x 1 and 5 x 1 x 7 (no cells).

Extraction from host-made float32 volumes: both sides see the same bits, so the signs agree exactly and `faces` must be EQUAL as integers;
vertices and colours within 2^-21 max(|coordinate| over the lattice, voxel_size): t = T_p / (T_p - T_q) carries at most 3 float roundings
and the position 3 more relative to the coordinate (a kernel that forms them in double beats it).

End to end: exact depths of the sphere from six cameras, integrated and extracted on the device; the faces equal the reference
pipeline's (tests/test_tsdf_ref.py: no reference value is within 1e-5 of zero and no lattice point is near a gate)."""
import numpy as np
import pytest
import torch

from tests import tsdf_cases as cases
from tests import tsdf_ref as ref
from tests.multiview_cases import TAN

pytestmark = pytest.mark.gpu
TOL = 2.0 ** -22


def device_volume(rv, trunc=cases.TRUNC, max_weight=64.0):
    """An adgs.tsdf.TSDFVolume holding the bits of the reference volume `rv`."""
    from adgs import tsdf
    v = tsdf.TSDFVolume(tuple(rv.origin), rv.voxel_size, rv.dims, trunc=trunc, max_weight=max_weight, color=rv.color is not None)
    assert v.tsdf.shape == rv.tsdf.shape and bool((v.tsdf == 1).all()) and not bool(v.wsum.any())
    v.tsdf.copy_(torch.from_numpy(rv.tsdf))
    v.wsum.copy_(torch.from_numpy(rv.wsum))
    if rv.color is not None:
        assert v.color.shape == rv.color.shape and not bool(v.color.any())
        v.color.copy_(torch.from_numpy(rv.color))
    return v


def snapshot(v):
    return (v.tsdf.cpu().numpy(), v.wsum.cpu().numpy(), None if v.color is None else v.color.cpu().numpy())


def bits(a):
    return a.view(np.uint32)


def integrate_view(v, view, name, tan=TAN):
    up = lambda a: None if a is None else torch.from_numpy(a).cuda()
    v.integrate(up(view.D), up(view.O), (tan, torch.from_numpy(view.pose)), image=up(view.image), weight=up(view.weight), **cases.integrate_kwargs(name))


def check_sequence(name, start, what):
    """Fuses the case's views into a device copy of `start` and into `start` itself (the reference), comparing after every view."""
    c = cases.BY_NAME[name]
    v = device_volume(start, max_weight=c.max_weight)
    prev = snapshot(v)
    excluded = np.zeros(start.tsdf.shape, bool)
    for view, (rv, upd, flagged) in zip(cases.views(name), cases.fuse(name, start)):
        integrate_view(v, view, name)
        now = snapshot(v)
        excluded |= flagged
        keep, hit = ~upd & ~excluded, upd & ~excluded
        e_t = np.abs(now[0].astype(np.float64) - rv.tsdf)[hit].max() if hit.any() else 0.0
        e_w = (np.abs(now[1].astype(np.float64) - rv.wsum)[hit] / rv.wsum[hit]).max() if hit.any() else 0.0
        e_c = np.abs(now[2].astype(np.float64) - rv.color)[:, hit].max() if rv.color is not None and hit.any() else 0.0
        print("%s: %d updated, %d excluded; max error tsdf %.2e, wsum %.2e (relative), colour %.2e" % (what, hit.sum(), excluded.sum(), e_t, e_w, e_c))
        assert np.array_equal(bits(now[0])[keep], bits(prev[0])[keep]) and np.array_equal(bits(now[1])[keep], bits(prev[1])[keep]), what
        if rv.color is not None:
            assert np.array_equal(bits(now[2])[:, keep], bits(prev[2])[:, keep]), what
        assert np.isfinite(now[0]).all() and np.isfinite(now[1]).all()
        assert e_t <= TOL and e_w <= TOL and e_c <= TOL, what
        prev = now
    return v


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_integration_matches_the_reference(name):
    check_sequence(name, cases.new_volume(name), name)


@pytest.mark.parametrize("name", ["base", "maxdepth"])
def test_a_skipped_point_is_not_written(name):
    """The cull and skip contract: a poisoned volume keeps its bits wherever the reference does not update (and does not flag)."""
    start = cases.new_volume(name)
    start.tsdf[:], start.wsum[:] = 0.123, 7.0
    if start.color is not None:
        start.color[:] = 0.5
    v = check_sequence(name, start.copy(), name + " poisoned")
    never = np.ones(start.tsdf.shape, bool)
    for _, upd, flagged in cases.fuse(name, start.copy()):
        never &= ~upd & ~flagged
    t, w, c = snapshot(v)
    assert never.mean() > 0.2
    assert (bits(t)[never] == bits(np.float32(0.123).reshape(1))[0]).all() and (w[never] == 7.0).all()
    if c is not None:
        assert (c[:, never] == 0.5).all()


@pytest.mark.parametrize("dims", [(300, 5, 4), (257, 3, 2), (1, 1, 1), (5, 1, 7)])
def test_edge_lattices(dims):
    """2 cm voxels across the ground plane 6 m ahead: the whole 6 m row of 300 lies inside every view's image."""
    start = ref.Volume((-3.0, 1.45, 6.0), 0.02, dims, color=True)
    v = check_sequence("base", start, "base %d x %d x %d" % dims)
    assert v.wsum.max().item() > 0
    verts, faces, colors = v.extract_mesh(min_weight=0.0)
    if min(dims) < 2:
        assert verts.shape == (0, 3) and faces.shape == (0, 3) and colors.shape == (0, 3)


def check_mesh(got, want, rv, what):
    verts, faces, colors = got
    V, F, C = want
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32 and verts.is_cuda and faces.is_cuda
    assert tuple(verts.shape) == V.shape and tuple(faces.shape) == F.shape, (what, verts.shape, faces.shape, V.shape, F.shape)
    assert (colors is None) == (C is None)
    assert np.array_equal(faces.cpu().numpy(), F), what
    corner = np.abs(np.stack([rv.origin, rv.origin + rv.voxel_size * (np.array(rv.dims) - 1)])).max()
    tol = 2.0 ** -21 * max(corner, rv.voxel_size)
    e_v = np.abs(verts.cpu().numpy().astype(np.float64) - V).max() if len(V) else 0.0
    e_c = np.abs(colors.cpu().numpy().astype(np.float64) - C).max() if C is not None and len(V) else 0.0
    print("%s: V %d, F %d; max error vertices %.2e, colours %.2e (tolerance %.2e)" % (what, len(V), len(F), e_v, e_c, tol))
    assert e_v <= tol and e_c <= tol, what


@pytest.mark.parametrize("name", cases.EXTRACTION)
def test_extraction_matches_the_reference(name):
    rv, min_weight = cases.extraction_volume(name)
    v = device_volume(rv)
    before = snapshot(v)
    got = v.extract_mesh(min_weight=min_weight)
    check_mesh(got, cases.extraction_reference(name), rv, name)
    if name == "all_positive":
        assert got[0].shape == (0, 3) and got[1].shape == (0, 3)
    after = snapshot(v)                                          # extraction reads the volume only
    assert all(a is None or np.array_equal(bits(a), bits(b)) for a, b in zip(after, before))
    again = v.extract_mesh(min_weight=min_weight)                # and is deterministic to the bit
    assert all(a is None or torch.equal(a, b) for a, b in zip(again, got))


def test_end_to_end_sphere():
    rv, _ = cases.sphere_fused()
    v = device_volume(ref.Volume((0.0, 0.0, 0.0), 1.0, cases.SPHERE_DIMS, color=False), trunc=cases.E2E_TRUNC)
    for view in cases.sphere_views():
        up = lambda a: torch.from_numpy(a).cuda()
        v.integrate(up(view.D), up(view.O), (cases.E2E_TAN, torch.from_numpy(view.pose)), inv_depth=True)
    t, w, _ = snapshot(v)
    assert np.array_equal(w, rv.wsum) and np.abs(t.astype(np.float64) - rv.tsdf).max() <= TOL
    check_mesh(v.extract_mesh(min_weight=1.0), ref.extract(rv, 1.0), rv, "sphere, six views")
    v.reset()
    assert bool((v.tsdf == 1).all()) and not bool(v.wsum.any())
    assert v.extract_mesh()[1].shape == (0, 3)


def test_around_and_camera_input():
    """TSDFVolume.around boxes a point set; a camera object alone (FoV + world_view_transform) is accepted."""
    from adgs import tsdf
    pts = torch.tensor([[-1.0, 0.5, 2.0], [1.0, 1.5, 4.0], [0.2, 1.0, 3.0]], device="cuda")
    v = tsdf.TSDFVolume.around(pts, 0.25, margin=0.5, color=False)
    assert v.dims == (13, 9, 13) and v.origin == (-1.5, 0.0, 1.5) and v.trunc == 1.0 and v.color is None and v.tsdf.is_cuda
    view = cases.views("noimage")[0]
    pose4 = np.eye(4)
    pose4[:3] = view.pose
    Cam = type("Cam", (), dict(FoVx=2 * np.arctan(TAN[0]), FoVy=2 * np.arctan(TAN[1]), world_view_transform=torch.from_numpy(pose4.T).float().cuda()))
    a, b = cases.new_volume("noimage"), None
    va, vb = device_volume(a), device_volume(a)
    D, O = torch.from_numpy(view.D).cuda(), torch.from_numpy(view.O).cuda()
    va.integrate(D, O, Cam())
    vb.integrate(D, O, (Cam(), tsdf.camera_pose(Cam())))
    assert torch.equal(va.tsdf, vb.tsdf) and torch.equal(va.wsum, vb.wsum) and bool((va.wsum > 0).float().mean() > 0.15)
