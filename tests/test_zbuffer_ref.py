"""Pins the numpy reference of the mesh z-buffer (tests/zbuffer_ref.py, the definition of include/adgs_zbuffer.h) by its properties, without
a GPU: coverage is a partition along shared edges, the depth of a plane is the plane's, ties and face order do not matter, and an
independent float64 ray caster sees the same faces.  The device is compared with this reference in tests/test_gpu_zbuffer.py."""
import numpy as np
import pytest

from tests import zbuffer_cases as cases
from tests import zbuffer_ref as ref


def test_quad_fullscreen_covers_every_pixel_once_at_its_depth():
    r = cases.reference("quad_fullscreen")
    assert (r.cover == 1).all() and (r.face >= 0).all()
    assert set(np.unique(r.face)) == {0, 1}
    assert (r.depth.view(np.uint32) == cases.QUAD_Z.view(np.uint32)).all()      # a float32 z is the centre of its rounding interval
    assert r.counts.tolist() == [0, 0, 0, 0, 0]
    assert np.array_equal(r.normal, np.broadcast_to(np.array([0, 0, -1], np.float32)[:, None, None], r.normal.shape))


def test_quad_on_centres_is_half_open():
    r = cases.reference("quad_on_centres")
    assert r.cover.sum() == 256 and r.cover.max() == 1
    ys, xs = np.nonzero(r.cover)
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (6, 21, 4, 19)           # the top and right edges are in, the left and bottom out
    diag = r.face[np.arange(5, 20), np.arange(6, 21)]
    assert len(set(diag.tolist())) == 1                                       # the centres on the diagonal all go to one of the two faces


def test_fan_on_centre_shares_no_pixel():
    r = cases.reference("fan_on_centre")
    assert r.cover.max() == 1 and r.cover[14, 18] == 1 and r.cover.sum() > 100
    assert len(np.unique(r.face[r.face >= 0])) == 11


def test_subpixel_draws_nothing_and_empty_is_empty():
    for name in ("subpixel", "empty"):
        r = cases.reference(name)
        assert (r.face == -1).all() and (r.depth.view(np.uint32) == 0).all() and (r.normal.view(np.uint32) == 0).all() and r.cover.sum() == 0
    assert cases.reference("subpixel").counts[:3].tolist() == [0, 0, 0]


def test_coplanar_duplicates_go_to_the_lowest_index():
    c, r = cases.case("coplanar_duplicates"), cases.reference("coplanar_duplicates")
    dup = [k for k in range(len(c.faces)) if c.faces[k].tolist() == [27, 28, 29]]
    assert dup == [2, 6, 9]
    assert (r.face == 2).sum() > 100 and not np.isin(r.face, dup[1:]).any()
    assert (r.cover[r.face == 2] >= 3).all()


def test_interpenetrating_faces_split_the_overlap():
    r = cases.reference("interpenetrating")
    both = r.cover == 2
    assert both.sum() > 50 and (r.face[both] == 0).sum() > 10 and (r.face[both] == 1).sum() > 10


def test_rejected_faces_land_in_their_counters():
    c, r = cases.case("near_and_guard"), cases.reference("near_and_guard")
    assert r.setup.status.tolist() == [0, 2, 2, 3, 4, 0, 2, 4, 2]
    assert r.counts.tolist() == [0, 4, 1, 2, 0]
    assert set(np.unique(r.face)) == {-1, 0, 5}
    c, r = cases.case("bad_index"), cases.reference("bad_index")
    assert r.counts.tolist() == [3, 0, 0, 0, 0] and r.setup.status.tolist().count(1) == 3
    assert not np.isin(r.face, np.nonzero(r.setup.status == 1)[0]).any()


def test_back_face_culling_changes_nothing_on_an_outward_sphere():
    a, b = cases.reference("sphere_outward"), cases.reference("sphere_outward", cull=1)
    assert (a.face >= 0).sum() > 1000
    assert np.array_equal(a.face, b.face) and np.array_equal(a.depth.view(np.uint32), b.depth.view(np.uint32))
    assert b.counts[4] > 50 and a.counts[4] == 0
    assert (a.setup.A[np.unique(a.face[a.face >= 0])] < 0).all()               # towards the camera: A < 0
    assert (a.normal[2][a.face >= 0] < 0).all()


@pytest.mark.parametrize("name", ["random_big", "mixed_sizes", "coplanar_duplicates"])
def test_face_order_does_not_matter(name):
    c, r = cases.case(name), cases.reference(name)
    perm = np.random.default_rng(1).permutation(len(c.faces))                  # new face k is old face perm[k]
    if name == "coplanar_duplicates":                                          # equal keys but for the index: keep the duplicates' order
        perm = np.concatenate([np.sort(perm[:5]), np.sort(perm[5:])])
    p = ref.render(c.vertices, c.faces[perm], c.view)
    assert np.array_equal(p.depth.view(np.uint32), r.depth.view(np.uint32))
    if name != "coplanar_duplicates":
        assert np.array_equal(np.where(p.face >= 0, perm[np.maximum(p.face, 0)], -1), r.face)


def test_mixed_sizes_has_every_size():
    c, r = cases.case("mixed_sizes"), cases.reference("mixed_sizes")
    assert len(c.faces) >= 300
    s = r.setup
    n = []
    for k in np.nonzero(s.status == 0)[0]:
        bw = min(s.U[k].max() // 256, c.view.W - 1) - max(-((-s.U[k].min()) // 256), 0) + 1
        bh = min(s.V[k].max() // 256, c.view.H - 1) - max(-((-s.V[k].min()) // 256), 0) + 1
        n.append(max(bw, 0) * max(bh, 0))
    n = np.array(n)
    # on both sides of the default threshold (64) and of the largest one the GPU tests set (4096), up to the whole image
    assert (n == 0).sum() > 30 and ((n > 0) & (n <= 64)).sum() > 100 and ((n > 64) & (n <= 4096)).sum() > 50 and (n > 4096).sum() >= 2
    assert n.max() == c.view.W * c.view.H
    assert (r.cover >= 3).sum() > 500


def test_the_tsdf_and_huge_cases_show_what_they_are_for():
    c, r = cases.case("tsdf"), cases.reference("tsdf")
    won = np.unique(r.face[r.face >= 0])
    assert (r.face >= 0).sum() > 3000 and 300 < len(won) < len(c.faces) // 2    # both spheres; most of the mesh is hidden or off screen
    assert r.counts[1] > 0                                                    # seen from inside: faces behind the camera
    assert not np.allclose(np.array(c.view.pose[:9]).reshape(3, 3), np.eye(3))
    assert all((ref.render(c.vertices, c.faces, w).face >= 0).sum() > 3000 for w in cases.views3("tsdf")[1:])
    c, r = cases.case("huge_faces"), cases.reference("huge_faces")
    s = r.setup
    tiles = [((min(s.U[k].max() // 256, c.view.W - 1) - max(-((-s.U[k].min()) // 256), 0) + 8) // 8)
             * ((min(s.V[k].max() // 256, c.view.H - 1) - max(-((-s.V[k].min()) // 256), 0) + 8) // 8) for k in np.nonzero(s.status == 0)[0]]
    assert sum(t > 256 for t in tiles) >= 3 and sum(4 < t <= 256 for t in tiles) >= 5


def test_ray_caster_sees_the_same_faces():
    """On random_big: face equals the ray caster's nearest hit, except at pixels within one pixel of an edge of the triangle either of the
    two names there, or whose two nearest hits differ by less than 1e-3 relative; the pixels excused in this way -- the disagreements
    -- are at most 2 % of the covered ones; where both agree the depths agree within 1e-3 relative.  (The snap moves a corner by at most
    1 / 512 pixel.)  The cap counts the pixels excused BECAUSE THEY DISAGREE: 9 055 pixels are covered, 3 disagree, all three excused, and the
    largest depth difference is 1.7e-4 relative -- while 1 439 covered pixels (15.9 %) meet the excusing conditions at all, as they must with
    40 random faces over 128 x 96: a cap on that set would test the case, not the z-buffer."""
    c, r = cases.case("random_big"), cases.reference("random_big")
    face, z, z2 = ref.ray_cast(c.vertices, c.faces, c.view)
    covered = r.face >= 0
    assert covered.sum() > 5000 and (r.cover >= 3).sum() > 1000
    differ = face != r.face
    near_edge = np.minimum(ref.edge_distance(c.vertices, c.faces, c.view, face), ref.edge_distance(c.vertices, c.faces, c.view, r.face)) <= 1.0
    with np.errstate(invalid="ignore"):
        close = (z2 - z) < 1e-3 * z
    excused = differ & (near_edge | close)
    print("covered %d, disagreeing %d, excused %d, excusable %d" % (covered.sum(), differ.sum(), excused.sum(), (covered & (near_edge | close)).sum()))
    assert not (differ & ~excused).any()
    assert excused.sum() <= 0.02 * covered.sum()
    same = covered & ~differ
    rel = np.abs(r.depth[same].astype(np.float64) - z[same]) / z[same]
    print("largest relative depth difference %.3g" % rel.max())
    assert rel.max() < 1e-3


def test_interpolation_of_the_depth_is_the_depth():
    """Interpolating the attribute z_c reproduces the depth map (two evaluations of the same point), and a constant stays constant."""
    c, r = cases.case("random_big"), cases.reference("random_big")
    zc = ref.to_camera(c.view, c.vertices.astype(np.float64))[:, 2:3].astype(np.float32)
    out = ref.interpolate(r, c.faces, np.concatenate([zc, np.full_like(zc, 0.625)], 1), c.view, background=-1.0)
    won = r.face >= 0
    assert (out[:, ~won] == -1.0).all() and np.abs(out[1][won] - 0.625).max() < 1e-7
    assert np.abs(out[0][won] / r.depth[won] - 1).max() < 1e-6


def test_counts_and_keep_references():
    maps = [np.array([[0, 0, -1], [2, 7, 2]]), np.array([[2, 2, 2], [-1, -1, 5]])]
    views, pixels = ref.count_faces(maps, 6)
    assert views.tolist() == [1, 0, 2, 0, 0, 1] and pixels.tolist() == [2, 0, 5, 0, 0, 1]
    v = np.arange(15, dtype=np.float32).reshape(5, 3)
    f = np.array([[0, 1, 2], [2, 3, 5], [4, 2, 1], [0, 3, 4]], np.int32)
    vo, fo, ao, dropped = ref.keep_faces([True, True, True, False], v, f, v * 2)
    assert fo.tolist() == [[0, 1, 2], [3, 2, 1]] and vo.tolist() == v[[0, 1, 2, 4]].tolist() and ao.tolist() == (v * 2)[[0, 1, 2, 4]].tolist() and dropped == 1
