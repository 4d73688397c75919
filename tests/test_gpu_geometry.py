"""The geometry evaluation on the GPU (adgs.geometry over include/adgs_geometry.h, csrc/geometry.hip) against tests/geometry_ref.py on the
cases of tests/geometry_cases.py.

Nearest neighbour.  idx EQUAL as integers and dist2 EQUAL as bits to the brute force in float32 (the object is built without FMA
contraction, so the device's d2 is the same one-rounding-per-operation value), and from run to run.
Sampling.  face equal as integers to the reference's cdf search; the points within 2^-23 of the largest |coordinate| of the face's corners
(one float32 rounding of a double that the reference forms in the same order; whether they are bit-equal is printed -- expected, with
contraction off).  sample_surface end to end: every point in its face, and the per-face counts within 6 sqrt(n p (1 - p)) + 1 of n p.
Metrics.  Counts equal as integers; each mean within (n + 4) 2^-52 relative: a sum of n non-negative doubles in any order carries
n 2^-53 and each square root 2^-53.  The sums are equal as bits from run to run (fixed partition, no atomics).
evaluate_points reads back ONCE (the stacked statistics), after the one synchronisation of each of its two PointGrids; no existing test
counts read-backs, so this is stated here and in the docstring and not tested."""
import numpy as np
import pytest
import torch

from tests import geometry_cases as cases
from tests import geometry_ref as ref

pytestmark = pytest.mark.gpu


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def device_nearest(name):
    from adgs import geometry as geo
    t, q, cell, md = cases.nn(name)
    grid = geo.PointGrid(up(t), cell)
    d2, idx = grid.nearest(up(q), md)
    assert d2.dtype == torch.float32 and idx.dtype == torch.int32 and d2.shape == idx.shape == (len(q),) and d2.is_cuda
    return grid, host(d2), host(idx)


@pytest.mark.parametrize("name", cases.NN_NAMES)
def test_nearest_equals_the_brute_force(name):
    from adgs import geometry as geo
    t, q, cell, md = cases.nn(name)
    want_d2, want_idx = cases.nn_reference(name)
    grid, d2, idx = device_nearest(name)
    wrong = np.flatnonzero((idx != want_idx) | (bits(d2) != bits(want_d2)))
    print("%s: M %d, N %d, dims %s, R %d, found %d; %d differ" % (name, len(t), len(q), grid.dims, geo.search_radius(md, cell), (want_idx >= 0).sum(), len(wrong)))
    assert len(wrong) == 0, (name, wrong[:5], idx[wrong[:5]], want_idx[wrong[:5]], d2[wrong[:5]], want_d2[wrong[:5]])
    if name in cases.EXPECTED_RADIUS:
        assert geo.search_radius(md, cell) == cases.EXPECTED_RADIUS[name]
    if name == "plane":
        assert grid.dims[2] == 1
    if name == "nonfinite":
        assert grid.num_finite == len(t) - 3 and (idx[[0, 64, 129]] == -1).all() and not np.isin(idx, [7, 100, 299]).any()
    if name == "no_targets":
        assert grid.dims == (0, 0, 0) and (idx == -1).all() and np.isposinf(d2).all()
    if name == "tie_across_cells":
        assert idx.tolist() == [0, 2, 4]


def test_no_finite_target_and_too_many_cells():
    from adgs import geometry as geo
    t = torch.full((5, 3), float("nan"), device="cuda")
    grid = geo.PointGrid(t, 0.5)
    d2, idx = grid.nearest(torch.zeros(3, 3, device="cuda"), 0.5)
    assert grid.num_finite == 0 and grid.dims == (0, 0, 0) and (host(idx) == -1).all() and np.isposinf(host(d2)).all()
    with pytest.raises(ValueError, match="enlarge cell_size"):
        geo.PointGrid(up(np.float32([[0, 0, 0], [3000, 0, 0]])), 0.001)
    grid = geo.PointGrid(up(np.float32([[0, 0, 0], [1, 0, 0]])), 0.1)
    with pytest.raises(ValueError, match="enlarge cell_size"):
        grid.nearest(torch.zeros(3, 3, device="cuda"), 0.9)


def test_nearest_is_equal_from_run_to_run():
    _, d2a, idxa = device_nearest("clustered1")
    _, d2b, idxb = device_nearest("clustered1")
    assert np.array_equal(idxa, idxb) and np.array_equal(bits(d2a), bits(d2b))


@pytest.mark.parametrize("name", tuple(cases.SAMPLING))
def test_sample_from_cdf_equals_the_reference(name):
    from adgs import geometry as geo
    v, f = cases.sampling_mesh(name)
    cdf, want_points, want_face, _ = cases.sampling_reference(name)
    n = cases.SAMPLING[name]
    areas = host(geo.face_areas(up(v), up(f)))
    # each cross-product component carries a few 2^-53 |a| |b|, and |a|, |b| <= 2 sqrt(3) max |coordinate|
    assert areas.dtype == np.float64 and (np.abs(areas - ref.face_areas(v, f)) <= 2.0 ** -48 * np.abs(v).max() ** 2).all()
    print("%s: areas bit-equal: %s" % (name, np.array_equal(areas, ref.face_areas(v, f))))
    points, face = geo.sample_from_cdf(up(v), up(f), up(cdf), n, seed=3)
    assert points.dtype == torch.float32 and face.dtype == torch.int32 and points.shape == (n, 3) and face.shape == (n,)
    points, face = host(points), host(face)
    assert np.array_equal(face, want_face)
    if n == 0:
        return
    tol = 2.0 ** -23 * np.abs(v[f[want_face]]).max((1, 2))
    err = np.abs(points.astype(np.float64) - want_points.astype(np.float64)).max(1)
    print("%s: n %d, max error %.3g (bound there %.3g); bit-equal: %s" % (name, n, err.max(), tol[err.argmax()], np.array_equal(bits(points), bits(want_points))))
    assert (err <= tol).all()


def test_sample_surface_end_to_end():
    from adgs import geometry as geo
    v, f = cases.sampling_mesh("tsdf")
    points, face = geo.sample_surface(up(v), up(f), 20000, seed=5)
    points, face = host(points), host(face)
    area = ref.face_areas(v, f)
    assert (area[face] > 0).all()
    bary, off = ref.barycentric(v, f, points, face)
    # a float32 point is within sqrt(3) 2^-24 `scale` of the double one; in barycentric coordinates that is at most this over the face's
    # smallest height, 2 area / longest edge (marching tetrahedra leave slivers)
    p = v[f[face]].astype(np.float64)
    scale = np.abs(p).max((1, 2))
    longest = np.max([np.linalg.norm(p[:, a] - p[:, b], axis=1) for a, b in ((0, 1), (1, 2), (2, 0))], axis=0)
    assert (off <= 2.0 ** -23 * scale).all() and (bary >= (-2.0 ** -22 * scale * longest / (2 * area[face]))[:, None]).all()
    # the same seed gives the same samples, another seed others
    again, _ = geo.sample_surface(up(v), up(f), 20000, seed=5)
    other, _ = geo.sample_surface(up(v), up(f), 20000, seed=6)
    assert np.array_equal(bits(host(again)), bits(points)) and not np.array_equal(bits(host(other)), bits(points))
    v, f = cases.count_mesh()
    _, face = geo.sample_surface(up(v), up(f), cases.COUNT_N, seed=cases.COUNT_SEED)
    counts, expected, bound = cases.count_condition(v, f, host(face), cases.COUNT_N)
    print("counts %s, expected %s, bound %s" % (counts, np.round(expected, 1), np.round(bound, 1)))
    assert counts.sum() == cases.COUNT_N and (np.abs(counts - expected) <= bound).all()
    for name in ("zero_area", "out_of_range"):
        v, f = cases.sampling_mesh(name)
        _, face = geo.sample_surface(up(v), up(f), 3000, seed=1)
        area = ref.face_areas(v, f)
        assert (area[host(face)] > 0).all() and ref.valid_faces(v, f[host(face)]).all()
    with pytest.raises(ValueError, match="total area"):
        geo.sample_surface(up(v), up(np.array([[1, 1, 3], [4, 4, 4]], np.int32)), 5)


def check_stats(got, want, n, what):
    assert got.shape == (8,) and got.dtype == np.float64
    assert np.array_equal(got[1:], want[1:]), (what, got, want)                          # the counts, as integers
    assert abs(got[0] - want[0]) <= (n + 4) * 2.0 ** -52 * want[0], (what, got[0], want[0])


@pytest.mark.parametrize("name", tuple(cases.metric_sets()))
def test_metrics_equal_the_reference(name):
    from adgs import geometry as geo
    pred, gt, taus, md, expected = cases.metric_sets()[name]
    want, to_gt, to_pred = ref.evaluate_points(pred, gt, taus, md)
    for d2, n in ((to_gt, len(pred)), (to_pred, len(gt))):
        a, b = geo.distance_stats(up(d2), taus, md), geo.distance_stats(up(d2), taus, md)
        assert a.is_cuda and torch.equal(a.view(torch.int64), b.view(torch.int64))       # equal as bits from run to run
        check_stats(host(a), ref.distance_stats(d2, taus, md), n, name)
    got = geo.evaluate_points(up(pred), up(gt), taus, md)
    for key in ("num_pred", "num_gt", "pred_without_neighbour", "gt_without_neighbour", "pred_below", "gt_below", "precision", "recall", "fscore"):
        assert got[key] == want[key], (name, key, got[key], want[key])
    for key, n in (("accuracy", len(pred)), ("completeness", len(gt)), ("chamfer", max(len(pred), len(gt)) + 1)):     # half the sum of the two means
        assert isinstance(got[key], float) and abs(got[key] - want[key]) <= (n + 4) * 2.0 ** -52 * want[key], (name, key, got[key], want[key])
    print("%s: accuracy %.6g, completeness %.6g, chamfer %.6g, fscore %s" % (name, got["accuracy"], got["completeness"], got["chamfer"], got["fscore"]))
    for key, value in (expected or {}).items():
        assert got[key] == value, (name, key, got[key], value)
    again = geo.evaluate_points(up(pred), up(gt), taus, md)
    assert again == got


def test_distance_stats_partition_sizes():
    """N below, at and beyond one workgroup, beyond one row per workgroup (N > 1024 * 256), N = 0 and no thresholds."""
    from adgs import geometry as geo
    rng = np.random.default_rng(8)
    for n in (0, 1, 255, 256, 257, 70000, 1024 * 256 + 300):
        d2 = rng.uniform(0, 0.3, n).astype(np.float32) ** 2
        d2[rng.random(n) < 0.1] = np.inf
        for taus in ((0.05, 0.1, 0.2, 0.25), ()):
            got = host(geo.distance_stats(up(d2), taus, 0.25))
            check_stats(got, ref.distance_stats(d2, taus, 0.25), n, (n, taus))


def test_evaluate_mesh_against_its_own_samples():
    from adgs import geometry as geo
    v, f = cases.sampling_mesh("tsdf")
    n = 6000
    gt, _ = geo.sample_surface(up(v), up(f), n, seed=21)
    spacing = float(np.sqrt(ref.face_areas(v, f).sum() / n))                             # the mean sample spacing
    taus, md = (2 * spacing,), 4 * spacing
    got = geo.evaluate_mesh(up(v), up(f), gt, taus, md, samples=n, seed=22)
    samples = got.pop("samples")
    assert samples.is_cuda and samples.shape == (n, 3)
    want_samples, _ = geo.sample_surface(up(v), up(f), n, seed=22)
    assert torch.equal(samples, want_samples)
    want, _, _ = ref.evaluate_points(host(samples), host(gt), taus, md)
    print("tsdf mesh, %d samples each side, spacing %.3f: precision %.4f, recall %.4f, chamfer %.4f" % (n, spacing, got["precision"][0], got["recall"][0],
                                                                                                    got["chamfer"]))
    assert got["precision"] == want["precision"] and got["recall"] == want["recall"] and got["fscore"] == want["fscore"]
    assert 0.5 < got["precision"][0] <= 1.0 and 0.5 < got["recall"][0] <= 1.0
