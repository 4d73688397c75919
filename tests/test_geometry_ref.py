"""tests/geometry_ref.py, the reference of the geometry evaluation, against independent statements (no GPU): the brute force against a
float64 distance matrix where there are no near-ties, the sampler against a barycentric recomputation and the binomial count condition,
the metrics against hand-computed sets."""
import numpy as np
import pytest

from tests import geometry_cases as cases
from tests import geometry_ref as ref


@pytest.mark.parametrize("name", ("odd", "outside", "plane", "nonfinite", "one_cell"))
def test_brute_force_against_float64(name):
    t, q, _, md = cases.nn(name)
    d2, idx = cases.nn_reference(name)
    t64, q64 = t.astype(np.float64), q.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        D = ((q64[:, None, :] - t64[None, :, :]) ** 2).sum(-1)
    D[:, ~np.isfinite(t).all(1)] = np.inf
    D[~np.isfinite(q).all(1), :] = np.inf
    D[np.isnan(D)] = np.inf
    order = np.sort(D, axis=1)
    limit = float(np.float32(md)) ** 2
    # decided cases only: the nearest is clear of the second nearest and of the limit by far more than float32 rounding
    with np.errstate(invalid="ignore"):                        # inf - inf where a query has no finite distance at all
        clear = (order[:, 1] - order[:, 0] > 1e-5 * limit) & (np.abs(order[:, 0] - limit) > 1e-5 * limit)
    clear |= np.isinf(order[:, 0])
    assert clear.mean() > 0.9
    want = np.where(order[:, 0] <= limit, D.argmin(1), -1)
    assert np.array_equal(idx[clear], want[clear])
    found = clear & (want >= 0)
    assert found.any() and (~found & clear).any()
    assert np.allclose(d2[found], order[found, 0], rtol=1e-6, atol=0)
    assert np.isposinf(d2[idx < 0]).all() and (d2[idx >= 0] < np.inf).all()


def test_brute_force_ties_and_boundary():
    t, q, _, md = cases.nn("tie_across_cells")
    d2, idx = cases.nn_reference("tie_across_cells")
    assert idx.tolist() == [0, 2, 4] and d2.tolist() == [0.25, 0.25, 0.25]
    for name in ("lattice_r2", "lattice_r1", "lattice_r3"):
        t, q, cs, md = cases.nn(name)
        assert ref.search_radius(md, cs) == cases.EXPECTED_RADIUS[name]
        d2, idx = cases.nn_reference(name)
        n = round(len(t) ** (1 / 3))
        low = slice(0, n * n)                                   # the queries max_dist below the x = 0 face: exactly max_dist away, inclusive
        assert (idx[low] >= 0).all() and (d2[low] == np.float32(md) * np.float32(md)).all()
    t, q, _, md = cases.nn("duplicates")
    d2, idx = cases.nn_reference("duplicates")
    same = (t[None, :, :] == q[:100, None, :]).all(-1)
    assert (same.sum(1) == 3).all() and np.array_equal(idx[:100], same.argmax(1)) and (d2[:100] == 0).all()


def test_splitmix_words():
    # the published splitmix64 sequence from state 0: the first outputs of the generator are the finaliser of GOLDEN, 2 GOLDEN, ...
    first = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    u = ref.splitmix_units(0, 2)
    assert [int(x * 2.0 ** 53) for x in u[0]] == [w >> 11 for w in first]
    assert ((u >= 0) & (u < 1)).all()
    big = ref.splitmix_units(2 ** 64 - 1, 100000)
    assert abs(big.mean() - 0.5) < 0.005 and not np.array_equal(big[:2], u)


@pytest.mark.parametrize("name", ("triangle", "two_1_1000", "zero_area", "out_of_range", "tsdf", "one_sample", "no_sample"))
def test_samples_lie_in_their_faces(name):
    v, f = cases.sampling_mesh(name)
    cdf, points, face, exact = cases.sampling_reference(name)
    n = cases.SAMPLING[name]
    assert points.shape == (n, 3) and face.shape == (n,) and points.dtype == np.float32 and face.dtype == np.int32
    if n == 0:
        return
    area = ref.face_areas(v, f)
    assert ref.valid_faces(v, f[face]).all() and (area[face] > 0).all()         # never a zero-area or out-of-range face
    bary, off = ref.barycentric(v, f, exact, face)
    scale = np.abs(v[f[face]]).max((1, 2))
    assert (bary > -1e-9).all() and (off < 1e-9 * np.maximum(scale, 1)).all()
    if name == "zero_area":
        assert set(np.unique(face)) == {0, 3, 4}
    if name == "out_of_range":
        assert set(np.unique(face)) <= {0, 2, 4} and area[1] == 0 and area[3] == 0


def test_per_face_counts_meet_the_condition():
    v, f = cases.count_mesh()
    area = ref.face_areas(v, f)
    assert 999 < area.max() / area.min() < 1001
    _, face, _ = ref.sample_surface(v, f, cases.COUNT_N, cases.COUNT_SEED)[:3]
    counts, expected, bound = cases.count_condition(v, f, face, cases.COUNT_N)
    assert counts.sum() == cases.COUNT_N and (np.abs(counts - expected) <= bound).all(), (counts, expected, bound)
    v, f = cases.sampling_mesh("two_1_1000")
    _, _, face, _ = cases.sampling_reference("two_1_1000")
    counts, expected, bound = cases.count_condition(v, f, face, cases.SAMPLING["two_1_1000"])
    assert (np.abs(counts - expected) <= bound).all()


@pytest.mark.parametrize("name", ("identical", "shift_below", "shift_at", "shift_above", "apart"))
def test_metrics_on_hand_computed_sets(name):
    pred, gt, taus, md, want = cases.metric_sets()[name]
    got, _, _ = ref.evaluate_points(pred, gt, taus, md)
    for key, value in want.items():
        assert got[key] == value, (name, key, got[key], value)
    assert got["num_pred"] == got["num_gt"] == 64
