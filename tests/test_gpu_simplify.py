"""The simplification on the GPU (adgs.simplify over include/adgs_simplify.h, csrc/simplify.hip) against tests/simplify_ref.py on the cases
of tests/simplify_cases.py.

Integers.  vertex_cluster, root, num_vertices, members, member_starts, faces, face_source and the counts are functions of the mesh and the
lattice alone: EQUAL to the oracle as integers, and from run to run.
"average" positions and all colours: EQUAL to the oracle as bits -- a sum of doubles in ascending vertex id, one division, one rounding.
"quadric" positions: within ONE float32 ulp of the oracle's rounded value.  Derived, not measured: the matrix A + lambda t I has a condition
number of at most (1 + lambda) / lambda, about 10^3, so two double evaluations of the solution (Cholesky here, LU there) differ by about
10^3 x 2^-52 ~ 10^-13 relative to the cell -- nine orders below a float32 ulp of a coordinate -- and can only disagree when that sliver
straddles a rounding boundary.
Every inequality asserted here (sphere distance, crease) is asserted of the oracle in tests/test_simplify_ref.py."""
import numpy as np
import pytest
import torch

from tests import simplify_cases as cases

pytestmark = pytest.mark.gpu

INT_FIELDS = ("vertex_cluster", "root", "num_vertices", "members", "member_starts", "faces", "face_source")


def up(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def host(t):
    return None if t is None else t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def within_one_ulp(got, want):
    return (got == want) | (got == np.nextafter(want, np.float32(np.inf))) | (got == np.nextafter(want, np.float32(-np.inf)))


def device_case(name):
    c = cases.case(name)
    return up(c["vertices"]), up(c["faces"]), up(c["colors"])


def run(name):
    """The device's clustering and both placements of a case."""
    from adgs import simplify
    c = cases.case(name)
    v, f, col = device_case(name)
    cl = simplify.cluster_vertices(v, f, c["cell_size"], c["origin"])
    placed = {p: simplify.place_vertices(cl, v, f, colors=col, placement=p) for p in ("quadric", "average")}
    return cl, placed


def check(name, cl, placed):
    want, wplaced = cases.reference(name)
    c = cases.case(name)
    for field in INT_FIELDS:
        g = host(getattr(cl, field))
        assert g.dtype == np.int32 and getattr(cl, field).is_cuda, (name, field)
        assert g.shape == getattr(want, field).shape and np.array_equal(g, getattr(want, field)), (name, field)
    assert cl.counts == want.counts, name
    assert len(cl) == len(want.root)
    for p, (gv, gc) in placed.items():
        wv, wc = wplaced[p]
        gv, gc = host(gv), host(gc)
        assert gv.dtype == np.float32 and gv.shape == wv.shape and gc.shape == wc.shape, (name, p)
        assert np.array_equal(bits(gc), bits(wc)), (name, p, "colours")
        if p == "average":
            assert np.array_equal(bits(gv), bits(wv)), (name, p)
        else:
            ok = within_one_ulp(gv, wv)
            print("%s: V %d -> %d, F %d -> %d; quadric: %d of %d coordinates differ from the oracle, all by one ulp: %s" % (
                name, len(c["vertices"]), len(wv), len(c["faces"]), len(want.faces), int((bits(gv) != bits(wv)).sum()), gv.size, bool(ok.all())))
            assert ok.all(), (name, p)


@pytest.mark.parametrize("name", cases.NAMES)
def test_equals_the_oracle(name):
    cl, placed = run(name)
    check(name, cl, placed)


@pytest.mark.parametrize("name", cases.TINY)
def test_tiny(name):
    from adgs import simplify
    c = cases.case(name)
    v, f, col = device_case(name)
    cl, placed = run(name)
    if name == "three_cells":
        assert torch.equal(cl.faces, f) and cl.vertex_cluster.tolist() == [0, 1, 2]
        for gv, gc in placed.values():
            assert np.array_equal(bits(host(gv)), bits(c["vertices"])) and torch.equal(gc, col)
    else:
        assert len(cl) == 0 and cl.faces.shape == (0, 3) and cl.members.shape == (0,) and cl.member_starts.tolist() == [0]
        assert cl.face_source.shape == (0,) and (cl.vertex_cluster == -1).all() and cl.vertex_cluster.shape == (len(c["vertices"]),)
        assert cl.counts["degenerate_faces"] == (1 if name == "one_cell" else 0)
        for gv, gc in placed.values():
            assert gv.shape == (0, 3) and gc.shape == (0, 3)
    vo, fo, co = simplify.simplify_mesh(v, f, cell_size=c["cell_size"])
    assert vo.shape == (len(cl), 3) and fo.shape == tuple(cl.faces.shape) and co is None


def test_identity_returns_the_mesh_unchanged():
    from adgs import simplify
    c = cases.case("identity")
    v, f, col = device_case("identity")
    V, F = v.shape[0], f.shape[0]
    for p in ("quadric", "average"):
        vo, fo, co = simplify.simplify_mesh(v, f, col, cell_size=c["cell_size"], placement=p)
        assert torch.equal(fo, f) and np.array_equal(bits(host(vo)), bits(c["vertices"])) and np.array_equal(bits(host(co)), bits(c["colors"])), p
    cl = simplify.cluster_vertices(v, f, c["cell_size"])
    ar = lambda n: torch.arange(n, dtype=torch.int32, device="cuda")
    assert torch.equal(cl.vertex_cluster, ar(V)) and torch.equal(cl.face_source, ar(F)) and torch.equal(cl.root, ar(V))
    assert torch.equal(cl.members, ar(V)) and torch.equal(cl.member_starts, ar(V + 1)) and (cl.num_vertices == 1).all()
    assert cl.counts == {"nonfinite_vertices": 0, "dropped_faces": 0, "degenerate_faces": 0, "duplicate_faces": 0}


@pytest.mark.parametrize("name", ["tsdf_2.0", "tsdf_3.7"])
def test_quadric_placement_is_nearer_the_spheres(name):
    _, placed = run(name)
    roots = cases.sphere_roots(name)
    q, a = cases.sphere_distance(host(placed["quadric"][0]), roots), cases.sphere_distance(host(placed["average"][0]), roots)
    print("%s: %d vertices on the spheres; mean distance quadric %.4f, average %.4f" % (name, roots.sum(), q, a))
    assert q < a


def test_crease_quadric_vertex_lies_on_both_planes():
    _, placed = run("crease")
    s = cases.crease_straddlers()
    q, a = host(placed["quadric"][0]).astype(np.float64)[s], host(placed["average"][0]).astype(np.float64)[s]
    for axis in (0, 2):
        ratio = np.abs(q[:, axis]) / np.abs(a[:, axis])
        print("crease: distance to the plane %s = 0: quadric / average %.5f .. %.5f" % ("xyz"[axis], ratio.min(), ratio.max()))
        assert (ratio <= 0.01).all()


def test_duplicates_by_hand():
    cl, _ = run("duplicates")
    assert cl.face_source.tolist() == [0, 3, 5, 10, 11]
    assert cl.counts == {"nonfinite_vertices": 0, "dropped_faces": 0, "degenerate_faces": 2, "duplicate_faces": 5}
    assert cl.faces.tolist() == [[0, 1, 2], [0, 2, 1], [3, 4, 5], [1, 3, 2], [4, 3, 5]]


def test_nonfinite_vertices_are_dropped_and_nothing_else_moves():
    from adgs import simplify
    c = cases.case("nonfinite")
    cl, placed = run("nonfinite")
    assert cl.counts["nonfinite_vertices"] == 4 and cl.counts["dropped_faces"] > 0
    assert (cl.vertex_cluster[[17, 40, 41, 100]] == -1).all()
    assert all(torch.isfinite(gv).all() and torch.isfinite(gc).all() for gv, gc in placed.values())
    # the same mesh with those vertices moved far away (finite, in cells of their own) and their faces removed: the same output
    v, f = c["vertices"].copy(), c["faces"]
    bad = ~np.isfinite(v).all(axis=1)
    v[bad] = np.array([[500.0, 500.0, 500.0]], np.float32) + 10.0 * np.arange(bad.sum(), dtype=np.float32)[:, None]
    f2 = f[~bad[f].any(axis=1)]
    cl2 = simplify.cluster_vertices(up(v), up(f2), c["cell_size"], c["origin"])
    assert torch.equal(cl2.faces, cl.faces) and torch.equal(cl2.root, cl.root) and torch.equal(cl2.members, cl.members)
    for p in ("quadric", "average"):
        gv, _ = simplify.place_vertices(cl2, up(v), up(f2), placement=p)
        assert torch.equal(gv, placed[p][0]), p


def test_refusals():
    from adgs import simplify
    v = up(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [2, 0, 1], [2, 1, 1], [3, 0, 0]], np.float32))
    f = up(np.array([[0, 1, 2], [1, -1, 2], [1, 3, 2], [4, 5, 7], [4, 5, 6]], np.int32))
    with pytest.raises(ValueError, match="2 faces index outside the 7 vertices"):
        simplify.cluster_vertices(v, f, 0.5)
    with pytest.raises(ValueError, match="2 faces index outside the 7 vertices"):
        simplify.simplify_mesh(v, f, cell_size=0.5)
    far = up(np.array([[0, 0, 0], [1e9, 0, 0], [0, 1, 0]], np.float32))
    tri = up(np.array([[0, 1, 2]], np.int32))
    with pytest.raises(ValueError, match="1 vertices lie .* enlarge cell_size or move origin"):
        simplify.cluster_vertices(far, tri, 0.01)
    with pytest.raises(ValueError, match="enlarge cell_size or move origin"):
        simplify.simplify_mesh(far, tri, cell_size=0.01)
    # the device is still in order: the valid faces alone give the oracle's answer
    ok = up(np.array([[0, 1, 2], [1, 3, 2], [4, 5, 6]], np.int32))
    assert simplify.cluster_vertices(v, ok, 0.5).faces.tolist() == [[0, 1, 2], [1, 3, 2], [4, 5, 6]]
    # moving the origin to the far vertex makes it keyable
    assert simplify.cluster_vertices(far[1:2].repeat(3, 1) + torch.eye(3, device="cuda") * 64, tri, 0.01, origin=(1e9, 0.0, 0.0)).faces.tolist() == [[0, 1, 2]]


def test_weld_joins_two_halves():
    from adgs import mesh, simplify
    c = cases.case("weld")
    v, f, col = device_case("weld")
    ny = cases.GRID[1]
    assert len(mesh.connected_components(f, v.shape[0])) == 2
    vo, fo, co = simplify.simplify_mesh(v, f, col, cell_size=2.0 ** -10)
    assert len(mesh.connected_components(fo, vo.shape[0])) == 1
    assert vo.shape[0] == v.shape[0] - ny and fo.shape[0] == f.shape[0]


def test_outputs_are_equal_from_run_to_run():
    a, pa = run("grid_coarse")
    b, pb = run("grid_coarse")
    for field in INT_FIELDS:
        assert torch.equal(getattr(a, field), getattr(b, field)), field
    assert a.counts == b.counts
    for p in pa:
        assert np.array_equal(bits(host(pa[p][0])), bits(host(pb[p][0]))) and np.array_equal(bits(host(pa[p][1])), bits(host(pb[p][1]))), p


def test_end_to_end(tmp_path):
    from adgs import io, mesh, simplify
    c = cases.case("tsdf_2.0")
    v, f, col = device_case("tsdf_2.0")
    cl, placed = run("tsdf_2.0")
    for p in ("quadric", "average"):
        vo, fo, co = simplify.simplify_mesh(v, f, col, cell_size=c["cell_size"], origin=c["origin"], placement=p)
        assert torch.equal(fo, cl.faces) and torch.equal(vo, placed[p][0]) and torch.equal(co, placed[p][1]), p
    n = mesh.vertex_normals(vo, fo)
    assert n.shape == vo.shape and torch.isfinite(n).all()
    path = str(tmp_path / "simplified.ply")
    io.write_mesh_ply(path, vo, fo, co, normals=n)
    rv, rf, rc = io.read_mesh_ply(path)
    assert np.array_equal(rv, host(vo)) and np.array_equal(rf, host(fo)) and rc.shape == (vo.shape[0], 3)
    # carrying another attribute across with the CSR: the member mean of a per-vertex scalar
    attr = torch.arange(v.shape[0], device="cuda", dtype=torch.float64)
    seg = torch.repeat_interleave(torch.arange(len(cl), device="cuda"), cl.num_vertices.long())
    mean = torch.zeros(len(cl), device="cuda", dtype=torch.float64).index_add_(0, seg, attr[cl.members.long()]) / cl.num_vertices
    assert (mean >= cl.root).all() and torch.equal(cl.member_starts[1:].long(), torch.cumsum(cl.num_vertices.long(), 0))
