"""The float64 reference of the TSDF fusion and of marching tetrahedra (tests/tsdf_ref.py) and the cases of tests/tsdf_cases.py, on the
CPU: the cases meet the condition the GPU comparison relies on, the orientation rule the reference derives geometrically is the
constant table the kernel carries, and the reference's meshes are what a mesh of a surface must be.

The condition (not a tolerance): per view at most 0.5 % of the lattice is flagged as near a gate and at least 15 % is updated.  The one
exception is written out in test_cases_meet_the_condition: with max_depth = 6 the first three cameras lose every ray that ends on the
wall at z = 8, which is most of what they see of this lattice (5.9 %, 5.6 %, 4.9 % of it remain; the fourth camera keeps 25 %)."""
import re
import os

import numpy as np
import pytest

from tests import tsdf_cases as cases
from tests import tsdf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_orientation_rule_is_a_constant_of_the_split():
    """The reversal depends on (parity of the axis order, inside set) alone; the kernel's two 16-bit constants are this table."""
    even = [{1}, {3}, {0, 2}, {1, 3}, {0, 1, 2}, {0, 2, 3}]
    even_mask = sum(1 << sum(1 << q for q in s) for s in even)
    odd_mask = 0x7FFE & ~even_mask
    for t in range(6):
        got = sum(1 << m for m in ref.reversed_sets(t))
        assert got == (even_mask if ref.EVEN[t] else odd_mask), t
    # parity of ORDERS as permutations
    for t, o in enumerate(ref.ORDERS):
        inversions = sum(o[a] > o[b] for a in range(3) for b in range(a + 1, 3))
        assert (inversions % 2 == 0) == ref.EVEN[t]
    src = open(os.path.join(ROOT, "ad-gs_amd", "csrc", "tsdf.hip")).read()
    k = re.search(r"REV_EVEN\s*=\s*(0x[0-9A-Fa-f]+)\s*,\s*REV_ODD\s*=\s*(0x[0-9A-Fa-f]+)", src)
    assert (int(k.group(1), 16), int(k.group(2), 16)) == (even_mask, odd_mask) == (0x25A4, 0x5A5A)


@pytest.mark.parametrize("name", [c.name for c in cases.CASES])
def test_cases_meet_the_condition(name):
    n = float(np.prod(cases.DIMS))
    steps = cases.reference(name)
    assert len(steps) == 4
    for view, (_, upd, flagged) in enumerate(steps):
        print("%s view %d: %.1f %% updated, %d flagged (%.2f %%)" % (name, view, 100 * upd.sum() / n, flagged.sum(), 100 * flagged.sum() / n))
        assert flagged.sum() <= 0.005 * n, (name, view)
        if name == "maxdepth" and view < 3:
            # the cut removes every ray that ends on the wall: what is left is the near part of the ground, and it must be LESS than without the cut
            assert 0.04 * n <= upd.sum() < 0.5 * cases.reference("noweight")[view][1].sum(), (name, view)
        else:
            assert upd.sum() >= 0.15 * n, (name, view)


def test_every_skip_branch_occurs():
    """Behind the camera (the fourth view), outside the image, an invalid pixel, beyond -trunc: each takes a share of the lattice."""
    vol = cases.new_volume(cases.BASE)
    X = vol.points()
    steps = cases.reference(cases.BASE)
    for view, (v, (_, upd, _)) in enumerate(zip(cases.views(cases.BASE), steps)):
        Xc = X @ v.pose[:, :3].T + v.pose[:, 3]
        front = Xc[..., 2] > 0.2
        u = (Xc[..., 0] / np.where(front, Xc[..., 2], 1)) / cases.TAN[0] * cases.W / 2 + (cases.W - 1) / 2
        w = (Xc[..., 1] / np.where(front, Xc[..., 2], 1)) / cases.TAN[1] * cases.H / 2 + (cases.H - 1) / 2
        inside = front & (u + 0.5 >= 0) & (u + 0.5 < cases.W) & (w + 0.5 >= 0) & (w + 0.5 < cases.H)
        shares = [(~front).mean(), (front & ~inside).mean(), (inside & ~upd).mean()]
        print("view %d: behind %.1f %%, outside the image %.1f %%, inside but skipped %.1f %%" % (view, *[100 * s for s in shares]))
        assert shares[1] > 0.15 and shares[2] > 0.10
        if view == 3:
            assert shares[0] > 0.10                              # the camera that stands inside the volume
    assert steps[3][1].sum() < steps[0][1].sum()
    # the clamp acts: the weight sum reaches max_weight
    assert (cases.reference("clamp")[-1][0].wsum == np.float32(1.5)).mean() > 0.05
    assert cases.reference("base")[-1][0].wsum.max() > 1.5


def test_reference_sphere_is_a_closed_oriented_manifold():
    V, F, _ = cases.extraction_reference("sphere")
    twice, unmatched, edges = ref.edge_stats(F)
    assert twice == 0 and unmatched == 0                        # every directed edge once, its opposite present
    assert (len(V), edges, len(F)) == (1248, 3738, 2492) and len(V) - edges + len(F) == 2
    assert ref.signed_volume(V, F) > 0
    assert np.unique(F).size == len(V)
    err = np.abs(np.linalg.norm(V - np.array(cases.SPHERE_C), axis=-1) - cases.SPHERE_R).max()
    print("largest distance from the sphere: %.4f voxel" % err)
    assert err <= 0.08


def test_reference_mesh_of_the_fused_base_case():
    V, F, C = cases.extraction_reference("fused_base")
    assert len(V) > 1000 and len(F) > 1000 and C.shape == V.shape
    assert np.unique(F).size == len(V)                           # every vertex is used
    twice, _, _ = ref.edge_stats(F)
    assert twice == 0                                            # every directed edge at most once
    nrm, cen = ref.face_normals(V, F), V[F].mean(1)
    seen = np.zeros(len(F), bool)
    for _, _, centre in cases.CAMERAS:                           # the normals face the cameras: every face shows its front to one of them
        seen |= np.einsum("ij,ij->i", nrm, np.array(centre) - cen) > 0
    assert seen.all()
    d = np.minimum(np.abs(V[:, 1] - 1.5), np.abs(V[:, 2] - 8.0)) / cases.VOXEL
    print("V %d, F %d, at most %.2f voxel from the true planes" % (len(V), len(F), d.max()))
    assert d.max() <= 1.0                                        # the surface is the planes', to within the lattice's resolution


@pytest.mark.parametrize("name", ["half_unseen", "min_weight", "slanted_300x5x4", "exact_zeros"])
def test_reference_meshes_with_a_boundary_use_every_vertex(name):
    V, F, _ = cases.extraction_reference(name)
    assert len(F) and np.unique(F).size == len(V)
    assert ref.edge_stats(F)[0] == 0


def test_end_to_end_volume_is_decided():
    """The device's fused sphere differs from the reference's by rounding only; the faces can be equal because no value is near zero and no
    lattice point of any view is near a gate."""
    vol, flags = cases.sphere_fused()
    assert not flags.any()
    assert np.abs(vol.tsdf).min() >= 1e-5
    V, F, _ = ref.extract(vol, 1.0)
    assert len(F) > 500 and np.unique(F).size == len(V)
