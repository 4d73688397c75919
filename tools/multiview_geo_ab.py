"""Cost of the multi-view geometric consistency term (adgs.multiview; include/adgs_multiview_geo.h) against the same definition composed
from float32 torch operations on the device (the published trainer's form: two F.grid_sample calls over the neighbour's maps and some
thirty element-wise full-resolution tensors) -- what a run has without the fused kernels.

    python tools/multiview_geo_ab.py [--height 1280] [--width 1920] [--rounds 15] [--inner 20] [--out FILE]

A ground plane and a wall seen from two cameras 0.35 m apart (exact ray-plane intersection), both depth maps with 0.3 % noise (errors of a
settled geometry: around the 1-pixel gate), a weight with the bottom fifth of the rows zero.  HIP-event medians (rounds of `inner`
back-to-back calls, ms per call), through the library entry points: the forward (tile pass + finish kernel), the backward with the
neighbour's gradients (zero fill of two maps + one launch) and without them (one launch); forward + backward through autograd, fused and
torch composition in alternating rounds of one process.  Both forms are also compared, on the timed inputs, with the same composition
evaluated in float64 on the device (loss, number of valid pixels, every gradient), so a wrong fast kernel is not reported as fast -- and
the float32 composition's own error at this size is on record.

Byte model (compulsory HBM traffic; the gathers of neighbouring pixels share lines): forward 12 HW (D, O, weight) + 8 HnWn read;
backward the same read + 8 HW written, with the neighbour's gradients + 8 HnWn of fill and up to 16 HnWn of atomic read-modify-write.

Prints one JSON line; --out also writes it to a file.
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PLANES = (((0.0, -1.0, 0.0), -1.5), ((0.0, 0.0, -1.0), -30.0))          # (n, d): n . X = d -- the road and a wall across it


def depth_of_planes(H, W, tan, R, t, device):
    """The depth (along the ray with r.z = 1) of the planes seen by the camera X_c = R X + t, float64."""
    import torch
    y, x = torch.meshgrid(torch.arange(H, device=device, dtype=torch.float64), torch.arange(W, device=device, dtype=torch.float64), indexing="ij")
    rays = torch.stack([((2 * x + 1) / W - 1) * tan[0], ((2 * y + 1) / H - 1) * tan[1], torch.ones_like(x)], dim=-1)
    origin, dirs = -R.T @ t, rays @ R
    best = torch.full((H, W), float("inf"), dtype=torch.float64, device=device)
    for n, d in PLANES:
        n = torch.tensor(n, dtype=torch.float64, device=device)
        tau = (d - (n * origin).sum()) / (dirs * n).sum(-1)
        best = torch.where((tau > 0) & (tau < best), tau, best)
    return best


def f32(x):
    """x rounded to float32 (what the C ABI receives), as a Python float."""
    import torch
    return float(torch.tensor(float(x), dtype=torch.float32))


def torch_geometric(D, O, Dn, On, w, R, t, tan, tan_n, min_opacity=0.5, max_pixel_error=1.0, stats=None):
    """include/adgs_multiview_geo.h (inv_depth) in torch operations of the maps' dtype (float32: what a trainer composes; float64: the
    yardstick of the agreement figures); every pixel goes through the chain, the invalid ones on stand-in inputs."""
    import torch
    import torch.nn.functional as F
    H, W = D.shape
    Hn, Wn = Dn.shape
    y, x = torch.meshgrid(torch.arange(H, device=D.device, dtype=D.dtype), torch.arange(W, device=D.device, dtype=D.dtype), indexing="ij")
    ok = (O >= min_opacity) & (D > 0)
    one = torch.ones_like(D)
    z = torch.where(ok, O, one) / torch.where(ok, D, one)
    rx, ry = ((2 * x + 1) / W - 1) * tan[0], ((2 * y + 1) / H - 1) * tan[1]
    X = (z * rx, z * ry, z)
    Y = [R[i, 0] * X[0] + R[i, 1] * X[1] + R[i, 2] * X[2] + t[i] for i in range(3)]
    front = Y[2] > 1e-6
    Yz = torch.where(front, Y[2], one)
    a, b = Y[0] / Yz, Y[1] / Yz
    u = a / tan_n[0] * (Wn / 2) + (Wn - 1) / 2
    v = b / tan_n[1] * (Hn / 2) + (Hn - 1) / 2
    ok = ok & front & (u >= 0) & (u <= Wn - 1) & (v >= 0) & (v <= Hn - 1)
    grid = torch.stack([2 * u / (Wn - 1) - 1, 2 * v / (Hn - 1) - 1], dim=-1)[None]
    okn = ((On >= min_opacity) & (Dn > 0))
    zn = torch.where(okn, On, torch.ones_like(On)) / torch.where(okn, Dn, torch.ones_like(Dn))
    both = torch.stack([zn, okn.to(D.dtype)])[None]                     # the depth and the corners' validity in one gather
    zh, all4 = F.grid_sample(both, grid, mode="bilinear", padding_mode="border", align_corners=True)[0]
    ok = ok & (all4.detach() > 1 - 1e-6)                                # every corner with a non-zero bilinear weight is valid
    q = (a * zh - t[0], b * zh - t[1], zh - t[2])
    Xp = [R[0, i] * q[0] + R[1, i] * q[1] + R[2, i] * q[2] for i in range(3)]
    ok = ok & (Xp[2].detach() > 1e-6)
    Xz = torch.where(ok, Xp[2], one)
    dx = (Xp[0] / Xz) / tan[0] * (W / 2) + (W - 1) / 2 - x
    dy = (Xp[1] / Xz) / tan[1] * (H / 2) + (H - 1) / 2 - y
    err = torch.sqrt(torch.where(ok, dx * dx + dy * dy, one) + 1e-30)
    valid = ok & (err.detach() < max_pixel_error)
    wv = w * valid
    if stats is not None:
        stats["valid"], stats["valid_map"] = int(valid.sum()), valid
    return (wv * torch.exp(-err.detach()) * torch.where(valid, err, torch.zeros_like(err))).sum() / wv.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from adgs import _lib, multiview

    if not torch.cuda.is_available():
        raise SystemExit("multiview_geo_ab: no HIP device; nothing is measured without one")
    lib = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = _lib.stream_ptr(dev)
    H, W = a.height, a.width
    res = {"tool": "multiview_geo_ab", "image": [H, W], "rounds": a.rounds, "calls_per_round": a.inner}

    def events(fn, inner):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(inner):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / inner

    def summary(ms):
        return dict(ms_median=round(statistics.median(ms), 5), ms_min=round(min(ms), 5), ms_max=round(max(ms), 5))

    def alternating(fns, inner):
        for f in fns.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                ms[k].append(events(f, inner))
        return {k: summary(v) for k, v in ms.items()}

    # ---- the two views and their rendered maps
    gen = torch.Generator(device=dev).manual_seed(0)
    tan = (f32(W / (2 * 2050.0)), f32(H / (2 * 2050.0)))               # float32 values: the three forms evaluate the same numbers
    tan_n = (f32(1.05 * tan[0]), f32(1.05 * tan[1]))
    yaw = 0.02
    R = torch.tensor([[math.cos(yaw), 0.0, -math.sin(yaw)], [0.0, 1.0, 0.0], [math.sin(yaw), 0.0, math.cos(yaw)]], dtype=torch.float64)
    pose = torch.cat([R, (-R @ torch.tensor([0.0, 0.0, 0.35], dtype=torch.float64))[:, None]], dim=1)
    z = depth_of_planes(H, W, tan, torch.eye(3, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.float64, device=dev), dev)
    zn = depth_of_planes(H, W, tan_n, pose[:, :3].to(dev), pose[:, 3].to(dev), dev)

    def rendered(depth):
        O = torch.where(torch.rand(H, W, generator=gen, device=dev) < 0.1, 0.1 + 0.3 * torch.rand(H, W, generator=gen, device=dev),
                        0.6 + 0.4 * torch.rand(H, W, generator=gen, device=dev))
        return (O / (depth * (1 + 0.003 * torch.randn(H, W, generator=gen, device=dev, dtype=torch.float64)))).float(), O
    (D, O), (Dn, On) = rendered(z), rendered(zn)
    w = torch.rand(H, W, generator=gen, device=dev)
    w[H - H // 5:] = 0                                                  # an ego-vehicle mask under fractional weights
    # The composition gates the corners through a bilinear sample of their validity and its float64 form rounds differently from the
    # kernel at the 1-pixel gate: the few pixels the two decide differently get weight 0, so the agreement figures compare arithmetic.
    R64, t64 = pose[:, :3].float().double().to(dev), pose[:, 3].float().double().to(dev)
    with torch.no_grad():
        gates = {}
        torch_geometric(D.double(), O.double(), Dn.double(), On.double(), w.double(), R64, t64, tan, tan_n, stats=gates)
        differ = gates["valid_map"] != (multiview.reprojection_errors(D, O, tan, Dn, On, tan_n, pose)[1] > 0)
        res["pixels_gated_differently_weight_zero"] = int(differ.sum())
        w[differ] = 0
    leaves = [t.clone().requires_grad_(True) for t in (D, O, Dn, On)]
    Rf, tf = pose[:, :3].float().to(dev), pose[:, 3].float().to(dev)

    def step(term):
        for t in leaves:
            t.grad = None
        term(*leaves).backward()
    fused = lambda d_, o_, dn_, on_: multiview.geometric_consistency_loss(d_, o_, tan, dn_, on_, tan_n, pose, weight=w)
    composed = lambda d_, o_, dn_, on_: torch_geometric(d_, o_, dn_, on_, w, Rf, tf, tan, tan_n)
    step(fused)
    Lf, gF = fused(*leaves).item(), [t.grad.clone() for t in leaves]
    step(composed)
    Lt, gT = composed(*leaves).item(), [t.grad.clone() for t in leaves]
    # the same composition in float64 on the device: what both are measured against
    leaves64 = [t.double().requires_grad_(True) for t in (D, O, Dn, On)]
    L64 = torch_geometric(*leaves64, w.double(), R64, t64, tan, tan_n, stats=gates)
    L64.backward()
    g64 = [t.grad for t in leaves64]
    _, gw = multiview.reprojection_errors(D, O, tan, Dn, On, tan_n, pose, weight=w)
    off = lambda gs: [float((x.double() - y).abs().max() / y.abs().max()) for x, y in zip(gs, g64)]
    res["agreement"] = dict(loss_float64=L64.item(), loss_fused=Lf, loss_torch=Lt, valid_pixels=int((gw > 0).sum()), valid_pixels_float64=gates["valid"],
                            fused_grad_max_abs_diff_over_max=off(gF), torch_grad_max_abs_diff_over_max=off(gT))
    del leaves64, g64
    fb = res["forward_backward"] = alternating({"fused": lambda: step(fused), "torch": lambda: step(composed)}, max(1, a.inner // 2))
    fb["torch_over_fused"] = round(fb["torch"]["ms_median"] / fb["fused"]["ms_median"], 2)

    # ---- the entry points apart
    p = lambda t: t.data_ptr()
    desc = multiview.make_geo_desc(H, W, H, W, True, tan, tan_n, 0.5, 1.0, pose[:, :3].reshape(-1).tolist() + pose[:, 3].tolist())
    work = torch.zeros(multiview.MULTIVIEW_GEO_WORK_DOUBLES, dtype=torch.float64, device=dev)
    out, gl = torch.zeros(1, device=dev), torch.ones(1, device=dev)
    gD, gO, gDn, gOn = (torch.empty_like(t) for t in (D, O, Dn, On))

    def forward():
        _lib.check(lib.adgs_multiview_geo_forward(ctypes.byref(desc), p(D), p(O), p(Dn), p(On), p(w), p(work), p(out), None, None, st), "forward")

    def backward():
        _lib.check(lib.adgs_multiview_geo_backward(ctypes.byref(desc), p(D), p(O), p(Dn), p(On), p(w), p(work), p(gl), p(gD), p(gO), p(gDn), p(gOn), st), "backward")

    def backward_ref_only():
        _lib.check(lib.adgs_multiview_geo_backward(ctypes.byref(desc), p(D), p(O), p(Dn), p(On), p(w), p(work), p(gl), p(gD), p(gO), None, None, st), "backward")
    k = res["kernels"] = alternating({"forward": forward, "backward": backward, "backward_without_neighbour_gradients": backward_ref_only}, a.inner)
    read = 12 * H * W + 8 * H * W
    for name, nbytes in (("forward", read), ("backward", read + 8 * H * W + 24 * H * W), ("backward_without_neighbour_gradients", read + 8 * H * W)):
        k[name].update(model_bytes=nbytes, GBps=round(nbytes / (k[name]["ms_median"] * 1e-3) / 1e9, 1))

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
