"""Cost of the multi-view photometric consistency term (adgs.multiview; include/adgs_multiview.h) against the same definition composed from
float32 torch operations on the device (the published trainer's form: a [S, T, 2] grid through F.grid_sample plus some forty element-wise
tensors) -- what a run has without the fused kernels.

    python tools/multiview_ab.py [--height 1280] [--width 1920] [--samples 102400] [--radius 3] [--rounds 15] [--inner 20] [--out FILE]

A textured ground plane and a wall seen from two cameras 0.35 m apart (exact ray-plane intersection), the reference's depth with 1 % noise
and its normal with 0.05 noise, a weight with the bottom fifth of the rows zero.  HIP-event medians (rounds of `inner` back-to-back
calls, ms per call): the forward (sum + finish kernel) and the backward (zero fill + one launch) apart through the library entry points,
with the bytes of their model and the rate that implies; forward + backward through autograd, fused and torch composition in alternating
rounds of one process.  Both forms are also compared, on the timed inputs, with the same composition evaluated in float64 on the device
(loss, number of valid samples, every gradient), so a wrong fast kernel is not reported as fast -- and the float32 composition's own error
at this size is on record.

Byte model (an upper bound: neighbouring samples share cache lines, and at this size both images live in the Infinity Cache):
forward S (4 index + 20 N, D, O + 4 weight + 4 T taps of I_r + 16 T taps of I_n) bytes read; backward the same, plus 20 H W bytes of zero
fill and 20 S bytes of float atomics.

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


def texture(X):
    import torch
    out = torch.full(X.shape[:-1], 0.5, dtype=X.dtype, device=X.device)
    for (kx, ky, kz, ph), a in zip(((1.9, 0.3, 0.7, 0.0), (-0.6, 1.1, 1.7, 1.0), (2.9, -2.3, 0.4, 2.0), (0.5, 3.1, -1.3, 0.5), (4.3, 0.9, 2.6, 4.0)),
                                   (0.16, 0.12, 0.08, 0.07, 0.04)):
        out = out + a * torch.sin(kx * X[..., 0] + ky * X[..., 1] + kz * X[..., 2] + ph)
    return out


def view_of_planes(H, W, tan, R, t, device):
    """(grey image, depth along the ray with r.z = 1, normal [3, H, W]) of the planes seen by the camera X_c = R X + t, float64."""
    import torch
    y, x = torch.meshgrid(torch.arange(H, device=device, dtype=torch.float64), torch.arange(W, device=device, dtype=torch.float64), indexing="ij")
    rays = torch.stack([((2 * x + 1) / W - 1) * tan[0], ((2 * y + 1) / H - 1) * tan[1], torch.ones_like(x)], dim=-1)
    origin, dirs = -R.T @ t, rays @ R
    best = torch.full((H, W), float("inf"), dtype=torch.float64, device=device)
    normal = torch.zeros(H, W, 3, dtype=torch.float64, device=device)
    for n, d in PLANES:
        n = torch.tensor(n, dtype=torch.float64, device=device)
        tau = (d - (n * origin).sum()) / (dirs * n).sum(-1)
        hit = (tau > 0) & (tau < best)
        best = torch.where(hit, tau, best)
        normal = torch.where(hit[..., None], n.expand(H, W, 3), normal)
    return texture(origin + best[..., None] * dirs), best, normal.permute(2, 0, 1)


def f32(x):
    """x rounded to float32 (what the C ABI receives), as a Python float."""
    import torch
    return float(torch.tensor(float(x), dtype=torch.float32))


def torch_photometric(N, D, O, Ir, In, w, samples, R, t, tan, tan_n, radius, min_opacity=0.5, min_cos=f32(0.1), max_error=f32(0.9), eps=f32(1e-8), stats=None):
    """include/adgs_multiview.h (inv_depth) in torch operations of the maps' dtype (float32: what a trainer composes; float64: the
    yardstick of the agreement figures); every sample goes through the chain, the invalid ones on stand-in inputs."""
    import torch
    import torch.nn.functional as F
    H, W = D.shape
    Hn, Wn = In.shape
    idx = samples.long()
    y0, x0 = (idx // W).to(D.dtype), (idx % W).to(D.dtype)
    n, d, o = N.reshape(3, -1)[:, idx].T, D.reshape(-1)[idx], O.reshape(-1)[idx]
    ok = (o >= min_opacity) & (d > 0)
    one = torch.ones_like(d)
    z = torch.where(ok, o, one) / torch.where(ok, d, one)
    nh = n / torch.sqrt((n * n).sum(-1, keepdim=True) + 1e-12)
    r0x, r0y = ((2 * x0 + 1) / W - 1) * tan[0], ((2 * y0 + 1) / H - 1) * tan[1]
    c0 = nh[:, 0] * r0x + nh[:, 1] * r0y + nh[:, 2]
    ok = ok & (-c0 >= min_cos * torch.sqrt(r0x * r0x + r0y * r0y + 1))
    c0 = torch.where(ok, c0, -one)
    k = torch.arange(-radius, radius + 1, device=D.device)
    dy, dx = torch.meshgrid(k, k, indexing="ij")
    qx, qy = x0[:, None] + dx.reshape(1, -1), y0[:, None] + dy.reshape(1, -1)          # integers held exactly in the floating type
    rqx, rqy = ((2 * qx + 1) / W - 1) * tan[0], ((2 * qy + 1) / H - 1) * tan[1]
    s = (nh[:, 0:1] * rqx + nh[:, 1:2] * rqy + nh[:, 2:3]) / (z * c0)[:, None]
    m = [R[i, 0] * rqx + R[i, 1] * rqy + R[i, 2] + t[i] * s for i in range(3)]
    front = m[2] > 1e-6
    mz = torch.where(front, m[2], torch.ones_like(m[2]))
    u = (m[0] / mz) / tan_n[0] * (Wn / 2) + (Wn - 1) / 2
    v = (m[1] / mz) / tan_n[1] * (Hn / 2) + (Hn - 1) / 2
    ok = ok & (front & (u >= 0) & (u <= Wn - 1) & (v >= 0) & (v <= Hn - 1)).all(-1)
    grid = torch.stack([2 * u / (Wn - 1) - 1, 2 * v / (Hn - 1) - 1], dim=-1)[None]
    b = F.grid_sample(In[None, None], grid, mode="bilinear", padding_mode="border", align_corners=True)[0, 0]
    a = Ir[qy.long(), qx.long()]
    T = a.shape[1]
    Sa, Sb = a.sum(-1), b.sum(-1)
    C = (a * b).sum(-1) - Sa * Sb / T
    Va = (a * a).sum(-1) - Sa * Sa / T
    Vb = (b * b).sum(-1) - Sb * Sb / T
    e = 1 - C * C / (Va * Vb + eps)
    valid = ok & (e.detach() < max_error)
    wv = w.reshape(-1)[idx] * valid
    if stats is not None:
        stats["valid"] = int(valid.sum())
    return (wv * torch.where(valid, e, torch.zeros_like(e))).sum() / wv.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--samples", type=int, default=102400)
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from adgs import _lib, multiview

    if not torch.cuda.is_available():
        raise SystemExit("multiview_ab: no HIP device; nothing is measured without one")
    lib = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = _lib.stream_ptr(dev)
    H, W, S, radius = a.height, a.width, a.samples, a.radius
    T = (2 * radius + 1) ** 2
    res = {"tool": "multiview_ab", "image": [H, W], "radius": radius, "taps": T, "rounds": a.rounds, "calls_per_round": a.inner}

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

    # ---- the two views and the rendered maps
    gen = torch.Generator(device=dev).manual_seed(0)
    tan = (f32(W / (2 * 2050.0)), f32(H / (2 * 2050.0)))               # float32 values: the three forms evaluate the same numbers
    tan_n = (f32(1.05 * tan[0]), f32(1.05 * tan[1]))
    yaw = 0.02
    R = torch.tensor([[math.cos(yaw), 0.0, -math.sin(yaw)], [0.0, 1.0, 0.0], [math.sin(yaw), 0.0, math.cos(yaw)]], dtype=torch.float64)
    pose = torch.cat([R, (-R @ torch.tensor([0.0, 0.0, 0.35], dtype=torch.float64))[:, None]], dim=1)
    eye = torch.eye(3, dtype=torch.float64, device=dev)
    Ir, z, n = view_of_planes(H, W, tan, eye, torch.zeros(3, dtype=torch.float64, device=dev), dev)
    In, _, _ = view_of_planes(H, W, tan_n, pose[:, :3].to(dev), pose[:, 3].to(dev), dev)
    Ir, In = Ir.float().contiguous(), In.float().contiguous()
    O = torch.where(torch.rand(H, W, generator=gen, device=dev) < 0.1, 0.1 + 0.3 * torch.rand(H, W, generator=gen, device=dev),
                    0.6 + 0.4 * torch.rand(H, W, generator=gen, device=dev))
    D = (O / (z * (1 + 0.01 * torch.randn(H, W, generator=gen, device=dev, dtype=torch.float64)))).float()
    N = ((n + 0.05 * torch.randn(3, H, W, generator=gen, device=dev, dtype=torch.float64)) * O).float()
    w = torch.rand(H, W, generator=gen, device=dev)
    w[H - H // 5:] = 0                                                  # an ego-vehicle mask under fractional weights
    samples = multiview.sample_pixels(torch.ones(H, W, device=dev), S, radius, generator=gen)
    S = samples.numel()
    res["samples"] = S
    leaves = [t.clone().requires_grad_(True) for t in (N, D, O)]
    Rf, tf = pose[:, :3].float().to(dev), pose[:, 3].float().to(dev)

    def step(term):
        for t in leaves:
            t.grad = None
        term(*leaves).backward()
    fused = lambda n_, d_, o_: multiview.photometric_consistency_loss(n_, d_, o_, tan, Ir, In, tan_n, pose, samples, weight=w, radius=radius)
    composed = lambda n_, d_, o_: torch_photometric(n_, d_, o_, Ir, In, w, samples, Rf, tf, tan, tan_n, radius)
    step(fused)
    Lf, gF = fused(*leaves).item(), [t.grad.clone() for t in leaves]
    step(composed)
    Lt, gT = composed(*leaves).item(), [t.grad.clone() for t in leaves]
    # the same composition in float64 on the device: what both are measured against
    leaves64 = [t.double().requires_grad_(True) for t in (N, D, O)]
    L64 = torch_photometric(*leaves64, Ir.double(), In.double(), w.double(), samples, pose[:, :3].float().double().to(dev), pose[:, 3].float().double().to(dev),
                            tan, tan_n, radius, stats=res.setdefault("float64", {}))
    L64.backward()
    g64 = [t.grad for t in leaves64]
    _, valid = multiview.patch_errors(N, D, O, tan, Ir, In, tan_n, pose, samples, weight=w, radius=radius)
    off = lambda gs: [float((x.double() - y).abs().max() / y.abs().max()) for x, y in zip(gs, g64)]
    res["agreement"] = dict(loss_float64=L64.item(), loss_fused=Lf, loss_torch=Lt, valid_samples=int(valid.sum()), valid_samples_float64=res.pop("float64")["valid"],
                            fused_grad_max_abs_diff_over_max=off(gF), torch_grad_max_abs_diff_over_max=off(gT))
    del leaves64, g64
    fb = res["forward_backward"] = alternating({"fused": lambda: step(fused), "torch": lambda: step(composed)}, max(1, a.inner // 2))
    fb["torch_over_fused"] = round(fb["torch"]["ms_median"] / fb["fused"]["ms_median"], 2)

    # ---- the two entry points apart
    p = lambda t: t.data_ptr()
    desc = multiview.make_desc(H, W, H, W, radius, True, tan, tan_n, 0.5, 0.1, 0.9, multiview.EPS, pose[:, :3].reshape(-1).tolist() + pose[:, 3].tolist())
    work = torch.zeros(multiview.MULTIVIEW_WORK_DOUBLES, dtype=torch.float64, device=dev)
    out, gl = torch.zeros(1, device=dev), torch.ones(1, device=dev)
    gN, gD, gO = torch.empty_like(N), torch.empty_like(D), torch.empty_like(O)

    def forward():
        _lib.check(lib.adgs_multiview_ncc_forward(ctypes.byref(desc), p(N), p(D), p(O), p(Ir), p(In), p(w), p(samples), S, p(work), p(out), None, None, st), "forward")

    def backward():
        _lib.check(lib.adgs_multiview_ncc_backward(ctypes.byref(desc), p(N), p(D), p(O), p(Ir), p(In), p(w), p(samples), S, p(work), p(gl), p(gN), p(gD), p(gO), st), "backward")
    k = res["kernels"] = alternating({"forward": forward, "backward": backward}, a.inner)
    read = S * (4 + 20 + 4 + 4 * T + 16 * T)
    for name, nbytes in (("forward", read), ("backward", read + 20 * H * W + 20 * S)):
        k[name].update(model_bytes=nbytes, GBps=round(nbytes / (k[name]["ms_median"] * 1e-3) / 1e9, 1))
    k["taps_per_s_forward"] = round(S * T / (k["forward"]["ms_median"] * 1e-3) / 1e9, 2)          # 1e9 taps / s

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
