"""The scan level of the bucket binning (ad-gs_amd/csrc/binning.hip: the cell-major counts matrix the preprocess writes, cell_colscan's
coalesced 16-byte reads of a cell's row, cell_scan, cell_scatter) and slab_sort's key stream (which keys a thread keeps: compares, one
popcount, one prefix sum per wave and batch -- the kept keys land in another order than the sort's ranking ever sees) on the shapes where
they can go wrong: workgroup counts around the row padding and around the one-trip / looping forms of the row read, one and two cells,
nothing visible, empty cells, a camera's own bounds against sampled ones, unsorted bounds rows, forced slab counts, the capacity re-run,
graph replays and cell-wide depth ties.  Every frame must be what the device-wide sort (ADGS_BINNING=sort) renders, bit for bit."""
import pytest
import torch

from adgs import _lib, graph, synthetic
from tests.test_gpu_raster import compare, dev, run_hip

pytestmark = pytest.mark.gpu

KEYS = ("color", "depth", "img_opacity", "img_flow", "img_semantic", "radii")


@pytest.fixture(autouse=True)
def _bucket_binning_on_128_pixel_cells(monkeypatch):
    monkeypatch.setenv("ADGS_BINNING", "bucket")
    monkeypatch.setenv("ADGS_CELL_TILES", "8")
    _lib.lib().adgs_test_set_capacity_hints(0, 0)
    yield
    _lib.lib().adgs_test_set_capacity_hints(0, 0)


def _bucket(fn):
    out = fn()
    assert _lib.frame_stats()["bucket_binning"] == 1
    return out


def _sorted(monkeypatch, fn):
    """The same frame through the device-wide sort; the bucket path is switched back on afterwards."""
    monkeypatch.setenv("ADGS_BINNING", "sort")
    out = fn()
    assert _lib.frame_stats()["bucket_binning"] == 0
    monkeypatch.setenv("ADGS_BINNING", "bucket")
    return out


def _equal(a, b, what=""):
    for k in KEYS:
        assert torch.equal(a[k], b[k]), (what, k)


def _bucket_equals_sort(monkeypatch, sc, what=""):
    a = _bucket(lambda: run_hip(sc))
    _equal(a, _sorted(monkeypatch, lambda: run_hip(sc)), what)
    return a


def _oracle(sc, seed):
    compare(sc, grads=synthetic.make_upstream_grads(sc, seed))
    assert _lib.frame_stats()["bucket_binning"] == 1


# ---- workgroup counts: 15 cells (no multiple of 4); P = 256 k - 37: k preprocess workgroups, the last one partly filled.  k = 1, 2, 5, 255, 257,
# 1025: rows with pad words; 1024 / 1025 / 4100: one trip of cell_colscan (<= 4096 workgroups) and two; 4100: ~70 k pairs and 32 slabs per cell
@pytest.mark.parametrize("k", [1, 2, 4, 5, 255, 256, 257, 1024, 1025, 4100])
def test_workgroup_counts(monkeypatch, k):
    sc = synthetic.make_scene(256 * k - 37, 640, 384, 620.0, n_objects=2)
    a = _bucket_equals_sort(monkeypatch, sc, k)
    assert int((a["radii"] > 0).sum()) > 0
    if k == 5:
        _oracle(sc, 5)


@pytest.mark.parametrize("W", [128, 256])
def test_one_cell_and_two_cells(monkeypatch, W):
    sc = synthetic.make_scene(6000, W, 128, 120.0, seed=91, n_objects=2)
    _bucket_equals_sort(monkeypatch, sc, W)
    if W == 256:
        _oracle(sc, 91)


def test_everything_culled(monkeypatch):
    sc = synthetic.make_scene(3000, 640, 384, 620.0, seed=92)
    sc["means3D"][:, 2] = -sc["means3D"][:, 2].abs() - 1.0              # behind the camera
    sc["flow_points"] = sc["means3D"].clone()
    a = _bucket_equals_sort(monkeypatch, sc)
    assert _lib.frame_stats()["num_rendered"] == 0 and int((a["radii"] > 0).sum()) == 0
    _oracle(sc, 92)
    assert _lib.frame_stats()["num_rendered"] == 0


def test_empty_cells(monkeypatch):
    """Everything inside the top-left of the 5 x 3 cells (64 / 51 pixels from its right / lower edge: further than any splat reaches): the
    other 14 cells own no pair and no slab_sort workgroup."""
    sc = synthetic.make_scene(30000, 640, 384, 620.0, seed=93, scale_mult=0.0008, near_frac=0.0)
    m = sc["means3D"].clone()
    z = m[:, 2]
    m[:, 0] = z * sc["tanfovx"] * (-0.875 + 0.075 * m[:, 0] / (1.1 * z * sc["tanfovx"]))
    m[:, 1] = z * sc["tanfovy"] * (-0.75 + 0.15 * m[:, 1] / (1.1 * z * sc["tanfovy"]))
    sc["means3D"] = m.contiguous(); sc["flow_points"] = m.clone()
    a = _bucket(lambda: run_hip(sc))
    assert 0 < _lib.frame_stats()["num_rendered"] <= int((a["radii"] > 0).sum())      # one cell per Gaussian at the most
    _equal(a, _sorted(monkeypatch, lambda: run_hip(sc)))
    _oracle(sc, 93)


# ---- slab bounds
def _render(sc, cam, train):
    """One forward with FIXED camera tensors: a camera's own slab bounds are kept under the addresses of its matrices."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    s = GaussianRasterizationSettings(sc["H"], sc["W"], cam["tanfovx"], cam["tanfovy"], cam["bg"], 1.0, cam["viewmatrix"], cam["projmatrix"],
                                      sc["sh_degree"], cam["campos"], False, True, False)
    with torch.set_grad_enabled(train):
        out = GaussianRasterizer(s)(means3D=dev(sc["means3D"]).requires_grad_(train), means2D=torch.zeros(sc["P"], 3, device="cuda"),
                                    opacities=dev(sc["opacities"]), shs=dev(sc["shs"]), scales=dev(sc["scales"]), rotations=dev(sc["rotations"]),
                                    flow_points=dev(sc["flow_points"]), semantic=dev(sc["semantic"]))
    torch.cuda.synchronize()
    color, radii, depth, op, flow, sem = [o.detach().clone() for o in out]
    return dict(color=color, radii=radii, depth=depth, img_opacity=op, img_flow=flow, img_semantic=sem)


def _device_camera(W, H, focal, seed):
    c = synthetic.make_camera(W, H, focal, cam_seed=seed)
    cam = {k: dev(c[k]) for k in ("viewmatrix", "projmatrix", "campos")}
    cam.update(tanfovx=c["tanfovx"], tanfovy=c["tanfovy"], bg=torch.zeros(3, device="cuda"))
    return cam


def test_a_cameras_own_bounds_and_sampled_bounds(monkeypatch):
    """A B A B A B, training renders of one scene: B's first render has no bounds of its own (they are sampled), A's third one splits by
    the quantiles its second one left in its own table.  A large tile grid: only there does a camera keep a table."""
    monkeypatch.delenv("ADGS_CELL_TILES")
    sc = synthetic.make_scene(120000, 1024, 768, 800.0, seed=94, n_objects=3, scale_mult=0.01)
    cams = [_device_camera(1024, 768, 800.0, seed) for seed in (1, 2)]
    refs = [_sorted(monkeypatch, lambda c=c: _render(sc, c, False)) for c in cams]
    _lib.lib().adgs_test_set_capacity_hints(0, 0)                        # (a sorted frame teaches bounds too: forget them)
    for rep in range(3):
        for cam, ref in zip(cams, refs):
            out = _bucket(lambda: _render(sc, cam, True))
            assert _lib.frame_stats()["tiles"] >= 2048
            _equal(out, ref, rep)
    assert _lib.frame_status()["fullest_slab_units"] == 1                # own bounds: every slab in one piece
    small = synthetic.make_scene(20000, 1024, 768, 800.0, seed=95, n_objects=2, scale_mult=0.01)
    _oracle(small, 95)


def test_scrambled_bounds_rows(monkeypatch):
    """Random words in the bounds table: rows that are not sorted send their slabs to slab_sort_slow; same lists."""
    monkeypatch.setenv("ADGS_SLAB_SAMPLE", "0")                          # split by the table, whatever it holds
    sc = synthetic.make_scene(90000, 512, 384, 400.0, seed=96, scale_mult=0.004, near_frac=0.0)
    ref = _sorted(monkeypatch, lambda: run_hip(sc))
    first = _bucket(lambda: run_hip(sc))                                 # creates the table
    assert _lib.lib().adgs_test_scramble_slab_bounds(7) == 0
    second = _bucket(lambda: run_hip(sc))
    _equal(first, ref, "first"); _equal(second, ref, "scrambled")
    sc2 = synthetic.make_scene(8000, 512, 384, 400.0, seed=97, n_objects=2)
    assert _lib.lib().adgs_test_scramble_slab_bounds(8) == 0
    _oracle(sc2, 97)


@pytest.mark.parametrize("lg", [0, 7])
def test_forced_slab_counts(monkeypatch, lg):
    sc = synthetic.make_scene(60000, 640, 384, 620.0, seed=98, n_objects=2)
    ref = _sorted(monkeypatch, lambda: run_hip(sc))
    monkeypatch.setenv("ADGS_SLABS_LG", str(lg))
    for rep in range(2):                                                 # unknown bounds, learned bounds
        _equal(_bucket(lambda: run_hip(sc)), ref, rep)
    if lg == 7:
        small = synthetic.make_scene(5000, 640, 384, 620.0, seed=99, n_objects=2)
        _oracle(small, 99)


def test_capacity_rerun(monkeypatch):
    """Large splats: several times the floor capacity of P + 4096 pairs.  The frame is binned a second time with exact sizes, from the
    counts and prefixes the first pass left."""
    sc = synthetic.make_scene(15000, 640, 384, 620.0, seed=100, scale_mult=0.025)
    ref = _sorted(monkeypatch, lambda: run_hip(sc))
    _lib.lib().adgs_test_set_capacity_hints(1, 1)
    before = _lib.frame_status()["eager_reruns"]
    out = _bucket(lambda: run_hip(sc))
    assert _lib.frame_status()["eager_reruns"] > before and _lib.frame_stats()["num_rendered"] > sc["P"] + 4096
    _equal(out, ref)
    _lib.lib().adgs_test_set_capacity_hints(1, 1)
    before = _lib.frame_status()["eager_reruns"]
    _oracle(sc, 100)
    assert _lib.frame_status()["eager_reruns"] > before


def test_graph_replays(monkeypatch):
    """Four replays of one captured frame: the first splits by the capture's empty table (everything bisected), the later ones by the
    bounds the replay before them left.  Images bit-identical to the eager frame, gradients within the rule of the graph tests."""
    from tests.test_gpu_graph_capacity import _static_step, same
    sc = synthetic.make_scene(60000, 640, 384, 620.0, sh_degree=3, seed=101, n_objects=2)
    fn, _ = _static_step(sc)
    eager = [t.clone() for t in _bucket(fn)]
    torch.cuda.synchronize()
    sorted_eager = [t.clone() for t in _sorted(monkeypatch, fn)]
    for i in range(4):
        assert torch.equal(eager[i], sorted_eager[i]), i
    cache = graph.GraphCache(lambda key: fn)
    for rep in range(4):
        got = cache(0)
        torch.cuda.synchronize()
        assert _lib.frame_stats()["bucket_binning"] == 1
        for i, (a, b) in enumerate(zip(eager, got)):
            if i < 4:
                assert torch.equal(a, b), (rep, i)                       # colour, depth, accumulated opacity, radii
            else:
                same(b, a, (rep, i))
    assert cache.validate(repair=False)


def test_one_depth_for_a_whole_cell(monkeypatch):
    """60 000 Gaussians at z = 5 exactly over two cells: every key of a cell is equal, the whole order is the index tie-break -- on entries
    the key stream now collects thread-major."""
    P = 60000
    sc = synthetic.make_scene(P, 256, 128, 250.0, seed=43, scale_mult=0.004, near_frac=0.0)
    z = sc["means3D"][:, 2].clone()
    sc["means3D"][:, 0] *= 5.0 / z
    sc["means3D"][:, 1] *= 5.0 / z
    sc["means3D"][:, 2] = 5.0
    sc["scales"] = (sc["scales"] * (5.0 / z)[:, None]).contiguous()
    sc["flow_points"] = sc["means3D"].clone()
    a = _bucket(lambda: run_hip(sc))
    assert _lib.frame_stats()["num_rendered"] > 2 * 8192
    _equal(a, _sorted(monkeypatch, lambda: run_hip(sc)))
    _oracle(sc, 43)
