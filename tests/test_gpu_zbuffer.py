"""The mesh z-buffer on the GPU (adgs.zbuffer and adgs.mesh.keep_faces over include/adgs_zbuffer.h, csrc/zbuffer.hip, csrc/mesh.hip) against
tests/zbuffer_ref.py on the cases of tests/zbuffer_cases.py.

face is EQUAL as integers, depth and the interpolated attributes as bits, counts as integers: the object is built without FMA contraction
and only IEEE + - * /, rint and conversions occur, in the order the reference writes out.  The normals take a square root and a division of
double values and are rounded once: within 2^-23 absolute (one float32 rounding of a value in [-1, 1]), exactly 0 where nothing was drawn.
Visibility counts and the kept mesh are integers / gathered bits: equal.  Every result is equal as bits from run to run, whichever path
(wave expansion, ticketed big faces, shared huge faces) a face takes."""
import numpy as np
import pytest
import torch

from tests import zbuffer_cases as cases
from tests import zbuffer_ref as ref

pytestmark = pytest.mark.gpu


def up(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def host(t):
    return None if t is None else t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def camera(view):
    """What render_mesh takes: ((tanfovx, tanfovy), the [3, 4] host matrix R | t)."""
    return view.tan, torch.tensor([list(view.pose[3 * r:3 * r + 3]) + [view.pose[9 + r]] for r in range(3)], dtype=torch.float64)


def draw(name, view=None, faces=None, **kw):
    from adgs import zbuffer
    c = cases.case(name)
    view = c.view if view is None else view
    v, f = up(c.vertices), up(c.faces if faces is None else faces)
    r = zbuffer.render_mesh(v, f, camera(view), (view.H, view.W), near=view.near, max_depth=view.max_depth, cull="back" if view.cull else "none", **kw)
    return r, v, f


def check_render(r, want, what, normals=True):
    assert r.face.dtype == torch.int32 and r.depth.dtype == torch.float32 and r.counts.dtype == torch.int64 and r.face.is_cuda
    assert np.array_equal(host(r.counts), want.counts), (what, host(r.counts), want.counts)
    assert np.array_equal(host(r.face), want.face), what
    assert np.array_equal(bits(host(r.depth)), bits(want.depth)), what
    if normals:
        n = host(r.normal)
        err = np.abs(n.astype(np.float64) - want.normal.astype(np.float64)).max() if n.size else 0.0
        print("%s: %d faces, %d pixels drawn, max normal error %.2e" % (what, len(want.setup.status), (want.face >= 0).sum(), err))
        assert err <= 2.0 ** -23, what
        assert (bits(n)[:, want.face < 0] == 0).all(), what


@pytest.mark.parametrize("name", cases.NAMES)
def test_render_equals_the_reference(name):
    r, _, _ = draw(name, normals=True)
    check_render(r, cases.reference(name), name)
    again, _, _ = draw(name, normals=True)
    for a, b in ((r.face, again.face), (r.depth, again.depth), (r.normal, again.normal), (r.counts, again.counts)):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), name


@pytest.mark.parametrize("name", ["sphere_outward", "tsdf", "mixed_sizes"])
def test_back_face_culling_equals_the_reference(name):
    r, _, _ = draw(name, view=cases.case(name).view._replace(cull=1), normals=True)
    check_render(r, cases.reference(name, cull=1), name + " cull")


@pytest.mark.parametrize("small_max", [1, 16, 4096])
@pytest.mark.parametrize("name", ["mixed_sizes", "huge_faces", "random_big"])
def test_the_result_does_not_depend_on_the_path(name, small_max):
    r, _, _ = draw(name, _small_max=small_max)
    check_render(r, cases.reference(name), "%s small_max %d" % (name, small_max), normals=False)


def test_max_depth_drops_samples():
    c = cases.case("random_big")
    view = c.view._replace(max_depth=3.75)
    r, _, _ = draw("random_big", view=view, normals=True)
    want = ref.render(c.vertices, c.faces, view, normals=True)
    assert 0 < (want.face >= 0).sum() < (cases.reference("random_big").face >= 0).sum() and want.depth.max() <= 3.75
    check_render(r, want, "random_big max_depth")


@pytest.mark.parametrize("name", ["random_big", "mixed_sizes", "tsdf", "coplanar_duplicates"])
def test_face_order_does_not_matter(name):
    c, want = cases.case(name), cases.reference(name)
    perm = np.random.default_rng(2).permutation(len(c.faces))
    r, _, _ = draw(name, faces=c.faces[perm])
    assert np.array_equal(bits(host(r.depth)), bits(want.depth)), name
    if name != "coplanar_duplicates":                           # there the tie goes to whichever duplicate comes first
        g = host(r.face)
        assert np.array_equal(np.where(g >= 0, perm[np.maximum(g, 0)], -1), want.face), name


@pytest.mark.parametrize("name", cases.NAMES)
def test_interpolate_equals_the_reference(name):
    from adgs import zbuffer
    c, want = cases.case(name), cases.reference(name)
    r, v, f = draw(name)
    rng = np.random.default_rng(7)
    for C, bg in ((3, 0.0), (1, -2.5)):
        a = rng.uniform(-1, 1, (len(c.vertices), C)).astype(np.float32)
        got = host(zbuffer.interpolate(r, v, f, up(a), background=bg))
        exp = ref.interpolate(want, c.faces, a, c.view, background=bg)
        assert got.shape == (C, c.view.H, c.view.W) and np.array_equal(bits(got), bits(exp)), (name, C)
        assert (got[:, want.face < 0] == np.float32(bg)).all(), (name, C)


@pytest.mark.parametrize("name", ["quad_fullscreen", "mixed_sizes", "tsdf", "bad_index", "empty"])
def test_face_visibility_equals_the_reference(name):
    from adgs import zbuffer
    c = cases.case(name)
    views = cases.views3(name)
    v, f = up(c.vertices), up(c.faces)
    F = len(c.faces)
    want_views, want_pixels = ref.count_faces([ref.render(c.vertices, c.faces, w).face for w in views], F)
    vis = zbuffer.visible_faces(v, f, [camera(w) for w in views], (views[0].H, views[0].W))
    assert vis.num_views == 3 and vis.views.dtype == torch.int32 and vis.pixels.dtype == torch.int64
    assert np.array_equal(host(vis.views), want_views) and np.array_equal(host(vis.pixels), want_pixels), name
    assert not host(vis._scratch).any(), name
    assert np.array_equal(host(vis.seen(2, 5)), (want_views >= 2) & (want_pixels >= 5))
    if name == "quad_fullscreen":                               # the contended case: two faces share every pixel of three views
        assert want_pixels.sum() == 3 * views[0].H * views[0].W and want_views.tolist() == [3, 3]


def check_keep(keep, c, colors, normals, what):
    from adgs import mesh
    vo, fo, co, no = mesh.keep_faces(up(keep), up(c.vertices), up(c.faces), colors=up(colors), normals=up(normals))
    wv, wf, wc, wn, _ = ref.keep_faces(keep, c.vertices, c.faces, colors, normals)
    assert fo.dtype == torch.int32 and np.array_equal(host(fo), wf), what
    for g, w in ((vo, wv), (co, wc), (no, wn)):
        assert (g is None) == (w is None), what
        if w is not None:
            assert g.shape == (len(wv), 3) and np.array_equal(bits(host(g)), bits(w)), what
    return vo, fo


@pytest.mark.parametrize("name", ["tsdf", "mixed_sizes", "bad_index", "random_big", "empty"])
def test_keep_faces_equals_the_reference(name):
    c = cases.case(name)
    F, V = len(c.faces), len(c.vertices)
    rng = np.random.default_rng(9)
    colors, normals = rng.uniform(0, 1, (V, 3)).astype(np.float32), rng.normal(size=(V, 3)).astype(np.float32)
    seen = ref.count_faces([cases.reference(name).face], F)[0] > 0
    for what, keep in (("all", np.ones(F, bool)), ("none", np.zeros(F, bool)), ("random", rng.random(F) < 0.4), ("seen", seen)):
        check_keep(keep, c, colors, normals, (name, what))
    check_keep(np.ones(F, bool), c, None, None, (name, "no attributes"))
    if name == "tsdf":                                          # every vertex is used: `all` returns the mesh itself
        vo, fo = check_keep(np.ones(F, bool), c, colors, None, (name, "all again"))
        assert np.array_equal(host(fo), c.faces) and np.array_equal(bits(host(vo)), bits(c.vertices))
    if name == "bad_index":                                     # the count of the kept faces the index check dropped
        import ctypes
        from adgs import _lib
        f, k = up(c.faces), up(np.ones(F, np.uint8))
        temp = torch.empty(int(_lib.lib().adgs_mesh_keep_temp_bytes(V, F)), dtype=torch.uint8, device="cuda")
        counts = (ctypes.c_longlong * 3)(0, 0, 0)
        _lib.call("adgs_zbuffer_keep_faces_count", f.device, V, F, f.data_ptr(), k.data_ptr(), temp.data_ptr(), counts)
        assert list(counts)[1:] == [F - 3, 3]


def test_culling_the_unseen_faces_end_to_end():
    """tsdf -> visible_faces -> keep_faces: every face that remains won a pixel in some view, checked by rendering the result again."""
    from adgs import mesh, zbuffer
    c = cases.case("tsdf")
    views = cases.views3("tsdf")
    size, cams = (views[0].H, views[0].W), [camera(w) for w in views]
    v, f = up(c.vertices), up(c.faces)
    vis = zbuffer.visible_faces(v, f, cams, size)
    keep = vis.seen()
    v2, f2, _, _ = mesh.keep_faces(keep, v, f)
    n = int(keep.sum())
    assert 0 < n < len(c.faces) and f2.shape == (n, 3) and int(f2.max()) == v2.shape[0] - 1
    again = zbuffer.visible_faces(v2, f2, cams, size)
    assert bool(again.seen().all())
    # the kept faces keep their order, so the second pass sees what the first saw
    assert torch.equal(again.pixels, vis.pixels[keep]) and torch.equal(again.views, vis.views[keep])
