"""The mesh clean-up on the GPU (adgs.mesh over include/adgs_mesh.h, csrc/mesh.hip) against tests/mesh_ref.py on the cases of
tests/mesh_cases.py.

Components.  vertex_component, root, num_faces and num_vertices are functions of the mesh alone: EQUAL as integers to the reference, and from
run to run.
Area.  |gpu - ref| <= (n_c + 8) 2^-52 S_c per component, n_c its face count and S_c the sum of 0.5 |p1 - p0| |p2 - p0|: each double cross
product and norm carries a few 2^-53 relative to |e1| |e2|, and a sum of n non-negative terms in any order carries n 2^-53.
Keep.  faces equal as integers; vertices, colours and normals equal as bits to the reference's gather.
Normals.  Outside the vertices the reference flags (|sum| < 2^-20 S_v; at most 0.5 % of V, none in the cases here): within 2^-23 absolute
per component -- the double sum is accurate to about (d + 4) 2^-32 relative there, far below a float32 ulp, and what remains is one rounding
to float32 of a value in [-1, 1].  Exactly zero where the definition says zero; equal bits from run to run.
Out-of-range indices are refused where the call reads back, and skipped -- checked before every dereference -- where it does not."""
import numpy as np
import pytest
import torch

from tests import mesh_cases as cases
from tests import mesh_ref as ref

pytestmark = pytest.mark.gpu


def up(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def host(t):
    return None if t is None else t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def device_mesh(name):
    v, f = cases.mesh(name)
    return up(v), up(f)


def check_components(got, want, what):
    assert got.vertex_component.dtype == torch.int32 and got.vertex_component.is_cuda
    for field in ("vertex_component", "root", "num_faces", "num_vertices"):
        g = host(getattr(got, field))
        assert g.dtype == np.int32 and np.array_equal(g, getattr(want, field)), (what, field)
    assert len(got) == len(want.root)


@pytest.mark.parametrize("name", cases.NAMES)
def test_components_equal_the_reference(name):
    from adgs import mesh
    v, f = device_mesh(name)
    want, _ = cases.reference(name)
    got = mesh.connected_components(f, v.shape[0], vertices=v)
    check_components(got, want, name)
    assert got.area.dtype == torch.float64 and got.area.shape == (len(want.root),)
    bound = (want.num_faces + 8) * 2.0 ** -52 * ref.area_bounds(want, *cases.mesh(name))
    err = np.abs(host(got.area) - want.area)
    print("%s: V %d, F %d, C %d; max area error %.2e (bound there %.2e)" % (name, v.shape[0], f.shape[0], len(got), err.max() if err.size else 0.0,
                                                                              bound[err.argmax()] if err.size else 0.0))
    assert (err <= bound).all(), name
    without = mesh.connected_components(f, v.shape[0])
    assert without.area is None
    check_components(without, want, name + " without vertices")


def test_components_are_equal_from_run_to_run():
    from adgs import mesh
    v, f = device_mesh("tsdf_perm")
    a, b = mesh.connected_components(f, v.shape[0], vertices=v), mesh.connected_components(f, v.shape[0], vertices=v)
    for field in ("vertex_component", "root", "num_faces", "num_vertices"):
        assert torch.equal(getattr(a, field), getattr(b, field)), field


def masks(want):
    C = len(want.root)
    rng = np.random.default_rng(3)
    return {"all": np.ones(C, bool), "none": np.zeros(C, bool), "faceless": want.num_faces == 0, "random": rng.random(C) < 0.5,
            "selected": ref.select(want.num_faces, 2, 30)}


@pytest.mark.parametrize("name", ["points", "bowtie", "strip_permuted", "scattered", "tsdf", "tsdf_perm", "repeated"])
def test_keep_equals_the_reference_gather(name):
    from adgs import mesh
    v, f = cases.mesh(name)
    want, (n, _, _) = cases.reference(name)
    rng = np.random.default_rng(9)
    c, n = rng.random(v.shape).astype(np.float32), n.astype(np.float32)
    dv, df, dc, dn = up(v), up(f), up(c), up(n)
    comps = mesh.connected_components(df, len(v))
    for label, mask in masks(want).items():
        for with_c, with_n in ((True, True), (False, False), (True, False), (False, True)):
            gv, gf, gc, gn = mesh.keep_components(comps, up(mask), dv, df, colors=dc if with_c else None, normals=dn if with_n else None)
            wv, wf, wc, wn = ref.keep(want, mask, v, f, c if with_c else None, n if with_n else None)
            what = (name, label, with_c, with_n)
            assert gf.dtype == torch.int32 and tuple(gf.shape) == wf.shape and np.array_equal(host(gf), wf), what
            assert gv.dtype == torch.float32 and tuple(gv.shape) == wv.shape and np.array_equal(bits(host(gv)), bits(wv)), what
            assert (gc is None) == (wc is None) and (gn is None) == (wn is None), what
            assert gc is None or np.array_equal(bits(host(gc)), bits(wc)), what
            assert gn is None or np.array_equal(bits(host(gn)), bits(wn)), what
            if label == "none":
                assert gv.shape == (0, 3) and gf.shape == (0, 3)
            if label == "faceless":
                assert gf.shape == (0, 3) and gv.shape[0] == int((want.num_faces == 0).sum())
            if label == "all":
                assert np.array_equal(host(gf), f) and np.array_equal(bits(host(gv)), bits(v))


def device_volume(rv):
    """An adgs.tsdf.TSDFVolume holding the bits of the reference volume `rv`."""
    from adgs import tsdf
    v = tsdf.TSDFVolume(tuple(rv.origin), rv.voxel_size, rv.dims, trunc=4.0 * rv.voxel_size, color=rv.color is not None)
    v.tsdf.copy_(torch.from_numpy(rv.tsdf))
    v.wsum.copy_(torch.from_numpy(rv.wsum))
    if rv.color is not None:
        v.color.copy_(torch.from_numpy(rv.color))
    return v


@pytest.mark.parametrize("kw", [dict(largest=2), dict(), dict(largest=3, min_faces=0), dict(largest=50, min_faces=0, min_area=3.0)])
def test_remove_small_components_end_to_end(kw):
    from adgs import mesh
    v, f, c = cases.tsdf_mesh()
    wv, wf, wc = ref.remove_small_components(v, f, c, **kw)
    gv, gf, gc = mesh.remove_small_components(up(v), up(f), up(c), **kw)
    assert np.array_equal(host(gf), wf) and np.array_equal(bits(host(gv)), bits(wv)) and np.array_equal(bits(host(gc)), bits(wc))
    if kw == dict(largest=2):
        on = cases.sphere_vertices(host(gv))
        assert (on[0] ^ on[1]).all() and len(wf) == 6008 + 2928
    assert mesh.remove_small_components(up(v), up(f), **kw)[2] is None
    # the same from a mesh extracted on the device from the same volume bits: its faces are the reference's to the integer
    vol = device_volume(cases.tsdf_volume())
    ev, ef, ec = vol.extract_mesh(min_weight=1.0)
    assert np.array_equal(host(ef), f)
    gv2, gf2, gc2 = mesh.remove_small_components(ev, ef, ec, **kw)
    # (the device's float32 positions may differ from the reference's in the last bit; no area is within 10 % of the threshold used here)
    assert np.array_equal(host(gf2), wf)
    comps = ref.components(f, len(v), v)
    kv = ref.select(comps.num_faces, kw.get("largest", 50), kw.get("min_faces", 50), comps.area, kw.get("min_area"))[comps.vertex_component]
    assert torch.equal(gv2, ev[up(kv)]) and torch.equal(gc2, ec[up(kv)])


def check_normals(name, got, want):
    n, S, flagged = want
    g = host(got)
    assert got.dtype == torch.float32 and g.shape == n.shape and np.isfinite(g).all()
    assert flagged.sum() <= 0.005 * len(n), name
    ok = ~flagged
    err = np.abs(g.astype(np.float64) - n)[ok]
    print("%s: V %d, %d flagged; max error %.2e (2^-23 = %.2e)" % (name, len(n), flagged.sum(), err.max() if err.size else 0.0, 2.0 ** -23))
    assert (err <= 2.0 ** -23).all(), name
    zero = (n == 0).all(1) & ok
    assert (bits(g[zero]) == 0).all(), name                     # exactly +0
    return g


@pytest.mark.parametrize("name", cases.NAMES)
def test_normals_match_the_reference(name):
    from adgs import mesh
    v, f = device_mesh(name)
    got = mesh.vertex_normals(v, f)
    g = check_normals(name, got, cases.reference(name)[1])
    again = mesh.vertex_normals(v, f, check=False)
    assert np.array_equal(bits(host(again)), bits(g)), name     # equal bits from run to run
    if name == "repeated":
        assert (bits(g[[1, 3, 5, 6]]) == 0).all() and (np.abs(np.linalg.norm(g[[0, 2, 4]], axis=1) - 1) < 1e-6).all()
    if name == "fan":
        assert abs(g[2048, 2] - 1.0) < 1e-3                     # the hub of the cone: its 4 096 corners summed


def test_normals_of_an_extracted_mesh_point_to_free_space():
    from adgs import mesh
    vol = device_volume(cases.tsdf_volume())
    ev, ef, _ = vol.extract_mesh(min_weight=1.0)
    n = host(mesh.vertex_normals(ev, ef)).astype(np.float64)
    v = host(ev)
    for (centre, _), on in zip(cases.SPHERES, cases.sphere_vertices(v)):
        radial = v[on].astype(np.float64) - np.array(centre)
        assert ((n[on] * radial).sum(1) > 0).all()


def test_out_of_range_indices_are_refused_or_skipped():
    from adgs import mesh
    v, f = cases.mesh(cases.BAD)
    dv, df = up(v), up(f)
    with pytest.raises(ValueError, match="2 faces index outside the 7 vertices"):
        mesh.connected_components(df, len(v))
    with pytest.raises(ValueError, match="2 faces index outside the 7 vertices"):
        mesh.connected_components(df, len(v), vertices=dv)
    with pytest.raises(ValueError, match="2 faces index outside the 7 vertices"):
        mesh.remove_small_components(dv, df, largest=1, min_faces=0)
    with pytest.raises(ValueError, match="faces index outside the 7 vertices"):
        mesh.vertex_normals(dv, df)
    with pytest.raises(ValueError, match="faces index outside the 7 vertices"):
        mesh.vertex_normals(dv, df, check=True)
    got = mesh.vertex_normals(dv, df, check=False)
    ok = ref.valid_faces(f, len(v))
    want = ref.normals(v, f[ok])
    g = check_normals(cases.BAD, got, want)
    assert (bits(g[3]) != 0).any() and (g[6] != 0).any()        # the valid faces around them still count
    # the device is still in order: the same call on the valid faces gives the same bits
    assert np.array_equal(bits(host(mesh.vertex_normals(dv, up(f[ok])))), bits(g))
