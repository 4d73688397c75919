"""Cost of the TSDF integration (adgs.tsdf; include/adgs_tsdf.h) against the same definition composed from float32 torch operations on
the device (projection of the lattice, index gather from the maps, torch.where) -- what a run has without the fused kernel -- and of one
mesh extraction.

    python tools/tsdf_ab.py [--height 1280] [--width 1920] [--dims 1024 256 512] [--voxel 0.04] [--views 40] [--out FILE]

A ground plane 1.5 m below the cameras and a wall across the road, seen by `views` cameras that advance 0.25 m per view with a slowly
swinging yaw (exact ray-plane depths with 0.3 % noise, 10 % of the pixels below min_opacity, a weight whose bottom fifth is zero), fused
with colour into a dims lattice that starts 1 m ahead of the first camera.  Per view: HIP events around ONE integrate of each side,
the sides alternating view by view on volumes of their own, the median over the views.  The two volumes are then compared (the float32
composition decides some gates differently; the share is reported, the values are compared elsewhere), and extract_mesh is timed once.

Byte model of an integrate (compulsory HBM traffic): the updated lattice points read and write tsdf, wsum and three colours, 2 x 20 bytes
each, plus the maps read once (24 H W with colour and weight); the rate over that model is also given as a share of the rate of a
device-to-device copy of 1 GiB.  The requirement: the fused integrate is not slower than the composition (the tool exits non-zero
if it is).

Prints one JSON line; --out also writes it to a file.
"""
import argparse
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


def torch_integrate(T, Ws, C, axes, D, O, img, w, pose, tan, trunc, max_weight, min_opacity=0.5, near=0.2, max_depth=float("inf")):
    """include/adgs_tsdf.h (inv_depth, with colour and weight) in float32 torch operations, in place on T, Ws [nz, ny, nx] and C [3, ...];
    axes: the world coordinates of the lattice along x [1, 1, nx], y [1, ny, 1] and z [nz, 1, 1]; pose: 12 floats.  -> the updated mask."""
    import torch
    H, W = D.shape
    X0, X1, X2 = axes
    R, t = pose[:9], pose[9:]
    x = R[0] * X0 + R[1] * X1 + R[2] * X2 + t[0]
    y = R[3] * X0 + R[4] * X1 + R[5] * X2 + t[1]
    z = R[6] * X0 + R[7] * X1 + R[8] * X2 + t[2]
    front = z > near
    zs = torch.where(front, z, torch.ones_like(z))
    uf = torch.floor((x / zs) / tan[0] * (W / 2) + (W - 1) / 2 + 0.5)
    vf = torch.floor((y / zs) / tan[1] * (H / 2) + (H - 1) / 2 + 0.5)
    inside = front & (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
    pix = (vf.clamp(0, H - 1) * W + uf.clamp(0, W - 1)).long()
    Op, Dp, wp = O.reshape(-1)[pix], D.reshape(-1)[pix], w.reshape(-1)[pix]
    good = inside & (Op >= min_opacity) & (Dp > 0) & (wp > 0)
    zd = Op / torch.where(good, Dp, torch.ones_like(Dp))
    sdf = zd - z
    upd = good & (zd <= max_depth) & (sdf >= -trunc)
    d = (sdf / trunc).clamp(max=1.0)
    Wn = torch.where(upd, Ws + wp, torch.ones_like(Ws))
    T.copy_(torch.where(upd, (T * Ws + d * wp) / Wn, T))
    C.copy_(torch.where(upd[None], (C * Ws + img.reshape(3, -1)[:, pix] * wp) / Wn, C))
    Ws.copy_(torch.where(upd, (Ws + wp).clamp(max=max_weight), Ws))
    return upd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--dims", type=int, nargs=3, default=[1024, 256, 512])
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from adgs import tsdf

    if not torch.cuda.is_available():
        raise SystemExit("tsdf_ab: no HIP device; nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    H, W = a.height, a.width
    nx, ny, nz = a.dims
    f32 = lambda v: float(torch.tensor(float(v), dtype=torch.float32))
    vs = f32(a.voxel)
    origin = (f32(-0.5 * vs * (nx - 1)), f32(1.9 - vs * (ny - 1)), 1.0)      # centred on the road, down to 0.4 m under it
    tan = (f32(W / (2 * 2050.0)), f32(H / (2 * 2050.0)))
    res = {"tool": "tsdf_ab", "image": [H, W], "dims": [nx, ny, nz], "voxel_size": vs, "views": a.views}

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e), out

    summary = lambda ms: dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))

    # ---- the views
    gen = torch.Generator(device=dev).manual_seed(0)
    w = torch.rand(H, W, generator=gen, device=dev)
    w[H - H // 5:] = 0                                                  # an ego-vehicle mask under fractional weights
    views = []
    for i in range(a.views):
        yaw = 0.15 * math.sin(0.4 * i)
        R = torch.tensor([[math.cos(yaw), 0.0, -math.sin(yaw)], [0.0, 1.0, 0.0], [math.sin(yaw), 0.0, math.cos(yaw)]], dtype=torch.float64)
        pose = torch.cat([R, (-R @ torch.tensor([0.0, 0.0, 0.25 * i], dtype=torch.float64))[:, None]], dim=1)
        z = depth_of_planes(H, W, tan, pose[:, :3].to(dev), pose[:, 3].to(dev), dev)
        O = torch.where(torch.rand(H, W, generator=gen, device=dev) < 0.1, 0.1 + 0.3 * torch.rand(H, W, generator=gen, device=dev),
                        0.6 + 0.4 * torch.rand(H, W, generator=gen, device=dev))
        D = (O / (z * (1 + 0.003 * torch.randn(H, W, generator=gen, device=dev, dtype=torch.float64)))).float()
        views.append((D, O, torch.rand(3, H, W, generator=gen, device=dev), pose))

    fused = tsdf.TSDFVolume(origin, vs, (nx, ny, nz), max_weight=64.0, color=True, device=dev)
    T, Ws, C = torch.ones_like(fused.tsdf), torch.zeros_like(fused.wsum), torch.zeros_like(fused.color)
    axes = (origin[0] + vs * torch.arange(nx, device=dev, dtype=torch.float32).reshape(1, 1, nx),
            origin[1] + vs * torch.arange(ny, device=dev, dtype=torch.float32).reshape(1, ny, 1),
            origin[2] + vs * torch.arange(nz, device=dev, dtype=torch.float32).reshape(nz, 1, 1))
    compose = lambda D, O, img, pose: torch_integrate(T, Ws, C, axes, D, O, img, w, pose[:, :3].reshape(-1).tolist() + pose[:, 3].tolist(), tan,
                                                      fused.trunc, fused.max_weight)
    D, O, img, pose = views[0]                                          # warm both sides up on scratch state, then start over
    fused.integrate(D, O, (tan, pose), image=img, weight=w)
    compose(D, O, img, pose)
    fused.reset()
    T.fill_(1.0), Ws.zero_(), C.zero_()
    torch.cuda.synchronize()
    ms = {"fused": [], "torch": []}
    updated = []
    for D, O, img, pose in views:
        ms["fused"].append(timed(lambda: fused.integrate(D, O, (tan, pose), image=img, weight=w))[0])
        t_ms, upd = timed(lambda: compose(D, O, img, pose))
        ms["torch"].append(t_ms)
        updated.append(int(upd.sum()))
    it = res["integrate"] = {k: summary(v) for k, v in ms.items()}
    it["torch_over_fused"] = round(it["torch"]["ms_median"] / it["fused"]["ms_median"], 2)
    it["updated_share_median"] = round(statistics.median(updated) / (nx * ny * nz), 4)
    nbytes = 2 * 20 * statistics.median(updated) + 24 * H * W
    src = torch.empty(2 ** 28, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    copy_ms = statistics.median(timed(lambda: dst.copy_(src))[0] for _ in range(9))
    copy_rate = 2 * src.numel() * 4 / (copy_ms * 1e-3) / 1e9
    del src, dst
    rate = nbytes / (it["fused"]["ms_median"] * 1e-3) / 1e9
    it.update(model_bytes=int(nbytes), fused_GBps=round(rate, 1), copy_GBps=round(copy_rate, 1), share_of_copy=round(rate / copy_rate, 3))
    # the two volumes: where they observed the same points, how far apart the values are
    same = (fused.wsum > 0) == (Ws > 0)
    res["agreement"] = dict(points_observed_by_one_side_only=int((~same).sum()),
                            tsdf_max_abs_diff_where_both=float((fused.tsdf - T)[same].abs().max()),
                            tsdf_mean_abs_diff_where_both=float((fused.tsdf - T)[same].abs().mean()))
    del T, Ws, C
    ex_ms, (verts, faces, colors) = timed(lambda: fused.extract_mesh(min_weight=2.0))
    ex_ms2, _ = timed(lambda: fused.extract_mesh(min_weight=2.0))
    res["extract_mesh"] = dict(ms_first=round(ex_ms, 3), ms_second=round(ex_ms2, 3), vertices=int(verts.shape[0]), faces=int(faces.shape[0]))
    res["fused_not_slower"] = it["fused"]["ms_median"] <= it["torch"]["ms_median"]

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not res["fused_not_slower"]:
        raise SystemExit("tsdf_ab: the fused integrate is slower than the torch composition")


if __name__ == "__main__":
    main()
