"""Pins tests/normals_ref.py, the float64 yardstick of tests/test_gpu_normals.py, to facts that hold independently of it: the depth normal
of a plane is the plane's normal, a fronto-parallel plane gives (0, 0, -1), autograd equals central finite differences, the Gaussian normal
does not depend on the quaternion's length (its gradient is orthogonal to q), equal scales pick axis 0, and the flip follows n_c . p_c."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import normals_ref as ref  # noqa: E402

TAN = (0.47, 0.31)


def plane_inputs(H, W, n, d, tan=TAN, inv_depth=True, opacity=0.9):
    """float32 (depth, opacity) of the plane n . P = d as the rasterizer would render it with a constant opacity, and the unit normal
    that faces the camera (float64)."""
    n = torch.tensor(n, dtype=torch.float64)
    n = n / n.norm()
    z = d / (n[:, None, None] * ref.rays(H, W, *tan)).sum(0)
    assert (z > 0).all()
    O = torch.full((H, W), opacity, dtype=torch.float64)
    D = O / z if inv_depth else O * z
    facing = -n if n[2] > 0 else n
    return D.float(), O.float(), facing


def test_plane_gives_its_normal_and_zero_loss():
    H, W = 17, 33
    worst = 0.0
    for inv in (True, False):
        for n, d in (((0.3, -0.2, 1.0), 7.0), ((-0.5, 0.4, 1.0), 12.0), ((0.1, 0.6, -1.0), -5.0)):
            D, O, facing = plane_inputs(H, W, n, d, inv_depth=inv)
            nd, m = ref.depth_normals(D.double(), O.double(), *TAN, inv_depth=inv)
            assert m[1:-1, 1:-1].all() and not m[0].any() and not m[-1].any() and not m[:, 0].any() and not m[:, -1].any()
            err = (nd[:, 1:-1, 1:-1] - facing[:, None, None]).abs().max()
            worst = max(worst, float(err))
            assert float(nd[:, 0].abs().max()) == 0.0
            L = ref.normal_consistency(O.double()[None] * nd, D.double(), O.double(), *TAN, inv_depth=inv)
            assert abs(float(L)) <= 5e-6
    print("plane: max |n_d - n| = %.2e" % worst)
    assert worst <= 5e-6


def test_fronto_parallel_plane_faces_the_camera():
    D, O, facing = plane_inputs(9, 11, (0.0, 0.0, 1.0), 4.0)
    nd, m = ref.depth_normals(D.double(), O.double(), *TAN)
    want = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64)
    assert torch.equal(facing, want)
    assert (nd[:, 1:-1, 1:-1] - want[:, None, None]).abs().max() <= 1e-6


def _noisy(H, W, seed, inv=True):
    g = torch.Generator().manual_seed(seed)
    z = 4 + 20 * torch.rand(H, W, generator=g, dtype=torch.float64)
    O = 0.6 + 0.4 * torch.rand(H, W, generator=g, dtype=torch.float64)
    O[2, 3] = 0.2
    D = O / z if inv else O * z
    N = torch.randn(3, H, W, generator=g, dtype=torch.float64)
    w = torch.rand(H, W, generator=g, dtype=torch.float64)
    return N, D, O, w


def test_autograd_matches_central_differences():
    for inv in (True, False):
        N, D, O, w = _noisy(7, 9, 3, inv)
        f = lambda n, d, o: ref.normal_consistency(n, d, o, *TAN, weight=w, inv_depth=inv)
        L, gN, gD, gO = ref.normal_consistency_with_grads(N, D, O, *TAN, weight=w, inv_depth=inv)
        assert float(L) > 0.1
        assert float(gD[2, 3]) == 0.0 and float(gO[2, 3]) == 0.0 and float(gN[:, 2, 3].abs().max()) == 0.0
        for t, g, idx in ((N, gN, (1, 3, 4)), (N, gN, (0, 1, 1)), (D, gD, (3, 4)), (D, gD, (1, 1)), (D, gD, (0, 4)), (O, gO, (3, 4)), (O, gO, (5, 7)), (O, gO, (3, 0))):
            h = 1e-6 * max(abs(float(t[idx])), 1e-3)
            args = [N.clone(), D.clone(), O.clone()]
            k = 0 if t is N else (1 if t is D else 2)
            args[k][idx] += h
            up = float(f(*args))
            args[k][idx] -= 2 * h
            dn = float(f(*args))
            fd = (up - dn) / (2 * h)
            assert abs(fd - float(g[idx])) <= 1e-6 * max(abs(float(g[idx])), float(g.abs().max())), (inv, k, idx, fd, float(g[idx]))


def _rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    scales = torch.rand(n, 3, generator=g, dtype=torch.float64) + 0.1
    q = torch.randn(n, 4, generator=g, dtype=torch.float64)
    p = torch.randn(n, 3, generator=g, dtype=torch.float64) * 3
    A = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))[0]
    view = torch.eye(4, dtype=torch.float64)
    view[:3, :3] = A                    # the transposed layout: rows 0..2 hold the rotation, row 3 the translation
    view[3, :3] = torch.tensor([0.3, -0.2, 5.0], dtype=torch.float64)
    return scales, q, p, view


def test_gaussian_normal_ignores_the_length_of_q_and_its_gradient_is_orthogonal_to_q():
    scales, q, p, view = _rows(40, 5)
    a = ref.gaussian_normals(scales, q, p, view)
    b = ref.gaussian_normals(scales, q * torch.linspace(0.3, 3.0, 40, dtype=torch.float64)[:, None], p, view)
    assert (a - b).abs().max() <= 1e-14
    assert ((a.norm(dim=-1) - 1).abs() <= 1e-14).all()
    qg = q.clone().requires_grad_(True)
    g = torch.randn(40, 3, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    (ref.gaussian_normals(scales, qg, p, view) * g).sum().backward()
    assert float(qg.grad.abs().max()) > 0.1
    assert ((qg.grad * q).sum(-1).abs() <= 1e-13 * qg.grad.abs().max()).all()


def test_equal_scales_pick_axis_zero_and_ties_the_lowest_index():
    s = torch.tensor([[0.5, 0.5, 0.5], [0.7, 0.2, 0.2], [0.2, 0.7, 0.2], [0.3, 0.2, 0.1], [0.3, 0.1, 0.2], [0.1, 0.1, 0.3]], dtype=torch.float64)
    assert ref.shortest_axis(s).tolist() == [0, 1, 0, 2, 1, 0]
    _, q, p, view = _rows(6, 7)
    n_c, _, k = ref.gaussian_normals_parts(s, q, p, view)
    R = ref.rotation_matrix(q / q.norm(dim=-1, keepdim=True))
    assert (R @ R.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max() <= 1e-14 and (torch.linalg.det(R) - 1).abs().max() <= 1e-14
    assert torch.allclose(n_c[0], R[0][:, 0] @ view[:3, :3], atol=1e-15)


def test_flip_negates_exactly_when_the_normal_points_away():
    scales, q, p, view = _rows(200, 8)
    n_c, p_c, _ = ref.gaussian_normals_parts(scales, q, p, view)
    out = ref.gaussian_normals(scales, q, p, view)
    away = (n_c * p_c).sum(-1) > 0
    assert 40 < int(away.sum()) < 160
    assert torch.equal(out[away], -n_c[away]) and torch.equal(out[~away], n_c[~away])
    assert ((out * p_c).sum(-1) <= 0).all()
    # the camera-space position is the view transform of the mean: row-vector times the transposed matrix
    hom = torch.cat([p, torch.ones(200, 1, dtype=torch.float64)], 1) @ view
    assert (hom[:, :3] - p_c).abs().max() <= 1e-14


def test_float32_restatement_holds_a_quarter_of_the_tolerance_on_the_small_shapes_only():
    """What float32 itself holds (tests/test_gpu_normals.py compares at 1e-4): well inside a quarter of that up to 121 columns; at 1025
    columns it is not, whatever the field of view -- the figures are printed, and are why the kernels work in double."""
    from tests import normals_cases as cases
    for H, W in ((17, 33), (37, 121)):
        for case in cases.LARGE_CASES:
            e_n, e_g = cases.float32_errors(H, W, cases.TAN, case)
            assert e_n <= 2.5e-5 and e_g <= 2.5e-5, (H, W, case, e_n, e_g)
    for case in cases.LARGE_CASES:
        print("float32 on %s at tanfov %s, %s: normals %.1e, gradients %.1e of max" % ((cases.LARGE, cases.LARGE_TAN, case) + cases.float32_errors(*cases.LARGE, cases.LARGE_TAN, case)))
