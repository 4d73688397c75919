"""The 3D smoothing filter without a GPU: the float64 restatement of include/adgs_filter3d.h (tests/filter3d_ref.py) against autograd
and against the released trainer's `min z / max fx` form, the loader's view of the new entry points and their host-side refusals,
and the extra PLY property through adgs.io."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import filter3d_ref as ref  # noqa: E402

ENTRIES = ("adgs_filter3d_accumulate", "adgs_filter3d_finalize", "adgs_filter3d_apply_forward", "adgs_filter3d_apply_backward")


def test_apply_backward_is_the_gradient_of_the_forward():
    s, o, f, gS, gO = (t.double() for t in ref.make_apply_case(24, 1))
    s, f = s.clamp(min=1e-2), f        # gradcheck differentiates numerically: keep the scales where a 1e-6 step is small
    ss, oo = s.clone().requires_grad_(True), o.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: ref.apply_forward(a, b, f), (ss, oo), eps=1e-7, atol=1e-7, rtol=1e-5)
    # the analytic form against autograd on the full range of scales (1e-4 .. 10)
    s, o, f, gS, gO = (t.double() for t in ref.make_apply_case(257, 2))
    ss, oo = s.clone().requires_grad_(True), o.clone().requires_grad_(True)
    S, O = ref.apply_forward(ss, oo, f)
    torch.autograd.backward([S, O], [gS, gO])
    gs, go = ref.apply_backward(s, o, f, gS, gO)
    # the two terms of dL/ds may cancel: the bound is relative to their magnitudes.  Autograd forms f^2 / d as 1 - s^2 / d, which loses
    # digits for f << s: its own error is the unit round-off of gO O / s
    O = ref.apply_forward(s, o, f)[1]
    terms = (gS * s / torch.sqrt(s * s + f * f)).abs() + (gO * O * f * f / (s * (s * s + f * f))).abs()
    assert ((gs - ss.grad).abs() <= 1e-12 * terms + 1e-14 * (gO * O / s).abs() + 1e-300).all()
    assert ((go - oo.grad).abs() <= 1e-12 * oo.grad.abs() + 1e-300).all()


def test_zero_filter_is_the_identity():
    s, o, f, gS, gO = (t.double() for t in ref.make_apply_case(100, 3))
    S, O = ref.apply_forward(s, o, torch.zeros_like(f))
    assert torch.equal(S, s) and torch.equal(O, o)
    gs, go = ref.apply_backward(s, o, torch.zeros_like(f), gS, gO)
    assert torch.equal(gs, gS) and torch.equal(go, gO)


def test_equal_focal_lengths_give_the_released_trainers_min_z_over_max_fx():
    kinds = ((75.0, 75.0, 64.0, 48.0),)
    recs = ref.random_cameras(9, 4, kinds).double()
    xyz = ref.random_points(400, 4, recs).double()
    (x, y, z), _ = ref.camera_space(xyz, recs)
    W, H, fx = 64.0, 48.0, 75.0
    u, v = x / z.clamp(min=0.001) * fx + W / 2, y / z.clamp(min=0.001) * fx + H / 2
    seen = (z > 0.2) & (u >= -0.15 * W) & (u <= 1.15 * W) & (v >= -0.15 * H) & (v <= 1.15 * H)
    distance = torch.where(seen, z, torch.full_like(z, float("inf"))).amin(dim=1)
    got = ref.rate(xyz, recs)
    some = torch.isfinite(distance)
    assert 50 < int(some.sum()) < 400
    # exactly: a quotient is monotonic in its divisor (tensor / tensor: torch evaluates float / tensor as a product with the reciprocal)
    assert torch.equal(got[some], recs[0, 12] / distance[some]) and not got[~some].any()
    flt = ref.filter_from_rate(got)
    assert ((flt[some] - distance[some] / fx * ref.SQRT02).abs() <= 4e-16 * flt[some]).all()
    assert torch.equal(flt[~some], flt[some].max().expand_as(flt[~some]))
    assert not ref.filter_from_rate(torch.zeros(5, dtype=torch.float64)).any()


def test_marginal_bookkeeping_and_gate_outcomes():
    recs = ref.random_cameras(65, 1)
    xyz = ref.random_points(1000, 1, recs)
    r = ref.rates(xyz, recs)
    assert (r["rate_lo"] <= r["rate_hi"]).all()
    plain = ref.rate(xyz.double(), recs.double())
    assert ((r["rate_lo"] <= plain) & (plain <= r["rate_hi"])).all()
    for name, (yes, no) in r["outcomes"].items():
        assert yes > 0 and no > 0, name
    # the planted rows against camera 0: behind, nearer than 0.2, outside the margin, centred (rate = fx / 3)
    one = ref.rates(xyz[:4], recs[:1])
    assert one["rate_hi"][:3].tolist() == [0.0, 0.0, 0.0] and abs(float(one["rate_lo"][3]) - 20.0) < 1e-4
    assert not ref.rate(xyz.double(), recs[:0].double()).any()


def test_entries_are_declared_exported_and_bound():
    from adgs import _lib
    from adgs.filter3d import CAMERA_FLOATS, CameraRecord
    header = open(os.path.join(ROOT, "include", "adgs_filter3d.h")).read()
    lib = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is ctypes.c_int
        assert getattr(lib, name) is not None
    assert ctypes.sizeof(CameraRecord) == 64 == 4 * CAMERA_FLOATS
    assert int(re.search(r"#define\s+ADGS_FILTER3D_CAMERA_FLOATS\s+(\d+)", header).group(1)) == CAMERA_FLOATS


def test_null_pointers_and_negative_sizes_are_refused_on_the_host():
    """Every refusal is decided from the arguments alone, before any launch: without a GPU the pointers are made up (never followed);
    with one they are a real buffer large enough for any of the calls."""
    from adgs import _lib
    lib = _lib.lib()
    if torch.cuda.is_available():
        buf = torch.zeros(4096, device="cuda")
        ok = buf.data_ptr()
    else:
        ok = 0x1000
    acc = lambda xyz=ok, row0=0, rows=8, cams=ok, n=1, rate=ok: lib.adgs_filter3d_accumulate(xyz, row0, rows, cams, n, rate, 1, None)
    fin = lambda rate=ok, P=8, out=ok, work=ok: lib.adgs_filter3d_finalize(rate, P, out, work, None)
    fwd = lambda P=8, a=ok, b=ok, c=ok, d=ok, e=ok: lib.adgs_filter3d_apply_forward(P, a, b, c, d, e, None)
    bwd = lambda P=8, a=ok, b=ok, c=ok, d=ok, e=ok, f=ok, g=ok: lib.adgs_filter3d_apply_backward(P, a, b, c, d, e, f, g, None)
    calls = [lambda: acc(xyz=None), lambda: acc(cams=None), lambda: acc(rate=None), lambda: acc(row0=-1), lambda: acc(rows=-1), lambda: acc(n=-1),
             lambda: acc(row0=2 ** 31 - 4), lambda: acc(cams=ok + 4),
             lambda: fin(rate=None), lambda: fin(out=None), lambda: fin(work=None), lambda: fin(P=-1), lambda: fwd(P=-1), lambda: bwd(P=-1)]
    calls += [lambda k=k: fwd(**{k: None}) for k in "abcde"] + [lambda k=k: bwd(**{k: None}) for k in "abcdefg"]
    for k, call in enumerate(calls):
        assert call() < 0, "refusal %d was accepted" % k
        assert _lib.last_error().startswith("adgs_filter3d_"), _lib.last_error()
    # a size of zero is a no-op
    assert acc(rows=0) == 0 and fin(P=0) == 0 and fwd(P=0) == 0 and bwd(P=0) == 0


def test_cpu_tensors_never_reach_the_library(monkeypatch):
    from adgs import _lib, filter3d

    def no_native_call():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(_lib, "lib", no_native_call)
    s, o, f, _, _ = ref.make_apply_case(8, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        filter3d.apply(s, o, f)
    with pytest.raises(RuntimeError, match="no CPU path"):
        filter3d.accumulate(torch.zeros(8, 3), ref.random_cameras(2, 0), torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        filter3d.finalize(torch.zeros(8))


def test_camera_records_follow_the_transposed_view_matrix():
    from adgs import filter3d, synthetic
    cam = synthetic.camera_to_z_up(synthetic.make_camera(96, 64, 80.0, cam_seed=3))
    c = synthetic.camera_object(cam, time=0.25)
    rec = filter3d.camera_records([c], "cpu")
    assert rec.shape == (1, 16) and rec.dtype == torch.float32
    p = torch.tensor([[0.3, -1.2, 2.0]])
    want = (torch.cat([p, torch.ones(1, 1)], 1) @ c.world_view_transform)[0, :3]          # the project's row-vector convention
    (x, y, z), _ = ref.camera_space(p, rec)
    assert torch.allclose(torch.stack([x[0, 0], y[0, 0], z[0, 0]]), want, atol=1e-6)
    assert abs(float(rec[0, 12]) - 96 / (2 * np.tan(0.5 * c.FoVx))) < 1e-4 and abs(float(rec[0, 12]) - 80.0) < 1e-3
    assert rec[0, 14:].tolist() == [96.0, 64.0]
    assert filter3d.camera_records([], "cpu").shape == (0, 16)


def test_ply_round_trip_and_unchanged_bytes_without_a_filter(tmp_path):
    from adgs import io as aio
    from tests.test_io_checkpoint import _M, _model
    m = _model(9, 4, 3)
    plain = os.path.join(str(tmp_path), "plain", "point_cloud.ply")
    aio.save_ply(m, plain)
    # the parent's writer, called as it always was
    cat = lambda a, b: torch.cat([a.detach(), b.detach()], dim=0)
    dc = cat(m._scene_shs_dc, m._obj_shs_dc).transpose(1, 2).flatten(start_dim=1).numpy()
    rest = cat(m._scene_shs_rest, m._obj_shs_rest).transpose(1, 2).flatten(start_dim=1).numpy()
    xyz = cat(m._scene_xyz, m._obj_xyz).numpy()
    obj = np.r_[np.zeros(9), np.ones(4)].astype(np.float32)[:, None]
    names = aio.construct_list_of_attributes(3, 45, 3, 4)
    today = os.path.join(str(tmp_path), "today.ply")
    aio.write_ply(today, names, np.concatenate((xyz, np.zeros_like(xyz), dc, rest, cat(m._scene_opacity, m._obj_opacity).numpy(),
                                                cat(m._scene_scaling, m._obj_scaling).numpy(), cat(m._scene_rotation, m._obj_rotation).numpy(), obj), axis=1))
    assert open(plain, "rb").read() == open(today, "rb").read()
    m.filter_3D = None                                       # an explicit None writes the same file
    aio.save_ply(m, plain)
    assert open(plain, "rb").read() == open(today, "rb").read()
    loaded = _M()
    loaded.filter_3D = torch.ones(3, 1)
    assert aio.load_ply(loaded, plain, device="cpu").filter_3D is None
    # with a filter: one more float property, last, restored bit for bit
    m.filter_3D = torch.rand(13, 1, generator=torch.Generator().manual_seed(1)) * 0.05
    with_filter = os.path.join(str(tmp_path), "filtered", "point_cloud.ply")
    aio.save_ply(m, with_filter)
    head = open(with_filter, "rb").read().split(b"end_header\n", 1)[0].decode().splitlines()
    assert head[-1] == "property float filter_3D" and [l.split()[2] for l in head[3:-1]] == names
    n = aio.load_ply(_M(), with_filter, device="cpu")
    assert n.filter_3D.shape == (13, 1) and n.filter_3D.dtype == torch.float32 and torch.equal(n.filter_3D, m.filter_3D)
    assert torch.equal(n._obj_xyz.detach(), m._obj_xyz)


def test_model_surface():
    from adgs.model import SyntheticGaussianModel
    assert SyntheticGaussianModel.filter_3D is None
    for name in ("compute_3d_filter", "get_scaling_with_3D_filter", "get_opacity_with_3D_filter"):
        assert hasattr(SyntheticGaussianModel, name)
