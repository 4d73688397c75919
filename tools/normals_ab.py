"""Cost of the normal-map prior (adgs.normals; include/adgs_normals.h) against the same definitions composed from torch operations in float32
on the device -- what a run has without the fused kernels -- and what pipe.render_normals adds to a training frame.

    python tools/normals_ab.py [--gaussians 1000000] [--height 1280] [--width 1920] [--config C3] [--rounds 15] [--inner 20] [--skip-frame] [--out FILE]

HIP-event medians (rounds of `inner` back-to-back calls, ms per call):
1. gaussian_normals forward and forward + backward at --gaussians rows with the object mask in column 0, fused and torch composition
   (quaternion to matrix, gather, view rotation, flip, cat), in alternating rounds of one process;
2. normal_consistency_loss at --height x --width, weighted: forward and backward apart through the library entry points, with the fraction of
   the copy rate their byte model implies (forward reads 6 * 4 * H * W bytes, backward reads the same and writes 5 * 4 * H * W), and forward +
   backward through autograd, fused and torch composition;
3. the training frame of --config (render + backward of the image, raw-scene model) with and without pipe.render_normals, the consistency
   loss included in the frame with the flag: the honest cost of the feature -- the three extra channels are blended by replays of the tile
   lists, one per four channels forward and one per channel backward.
The two forms are also compared on the timed inputs, so a wrong fast kernel is not reported as fast.

Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def torch_gaussian_normals(scales, rotations, means3D, view, mask=None):
    """include/adgs_normals.h in float32 torch operations."""
    import torch
    q = rotations / rotations.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    k = scales.detach().argmin(dim=1)
    n_w = R.gather(2, k[:, None, None].expand(-1, 3, 1)).squeeze(2)
    n_c = n_w @ view[:3, :3]
    p_c = means3D.detach() @ view[:3, :3] + view[3, :3]
    flip = (n_c.detach() * p_c).sum(-1, keepdim=True) > 0
    n = torch.where(flip, -n_c, n_c)
    return n if mask is None else torch.cat([mask, n], dim=1)


def torch_consistency(N, D, O, w, tanfovx, tanfovy, inv_depth=True, min_opacity=0.5):
    """include/adgs_normals.h in float32 torch operations: unprojection, four shifted differences, cross product, two normalisations, masked mean."""
    import torch
    H, W = D.shape
    ok = (O >= min_opacity) & (D > 0)
    one = torch.ones_like(D)
    sd, so = torch.where(ok, D, one), torch.where(ok, O, one)
    z = so / sd if inv_depth else sd / so
    xs = ((2 * torch.arange(W, device=D.device, dtype=torch.float32) + 1) / W - 1) * tanfovx
    ys = ((2 * torch.arange(H, device=D.device, dtype=torch.float32) + 1) / H - 1) * tanfovy
    P = torch.stack([z * xs[None, :], z * ys[:, None], z])
    t_x = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    t_y = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    c = torch.cross(t_y, t_x, dim=0)
    n_d = c / torch.sqrt((c * c).sum(0, keepdim=True) + 1e-30)
    Ni = N[:, 1:-1, 1:-1]
    nh = Ni / torch.sqrt((Ni * Ni).sum(0, keepdim=True) + 1e-12)
    m = ok[1:-1, 1:-1] & ok[1:-1, :-2] & ok[1:-1, 2:] & ok[:-2, 1:-1] & ok[2:, 1:-1]
    v = w[1:-1, 1:-1] * m
    return (v * (1.0 - (nh * n_d).sum(0))).sum() / v.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--skip-frame", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from adgs import _lib, normals

    if not torch.cuda.is_available():
        raise SystemExit("normals_ab: no HIP device; nothing is measured without one")
    lib = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = _lib.stream_ptr(dev)
    res = {"tool": "normals_ab", "rounds": a.rounds, "calls_per_round": a.inner}

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

    def alternating(fns, inner, rounds=None):
        """{name: summary} of several callables timed in alternating rounds"""
        for f in fns.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(rounds or a.rounds):
            for k, f in fns.items():
                ms[k].append(events(f, inner))
        return {k: summary(v) for k, v in ms.items()}

    gen = torch.Generator(device="cpu").manual_seed(0)

    # ---- 1. per-Gaussian normals
    P = a.gaussians
    scales = torch.exp(0.6 * torch.randn(P, 3, generator=gen)).to(dev)
    rot = torch.randn(P, 4, generator=gen).to(dev)
    xyz = (torch.randn(P, 3, generator=gen) * 20).to(dev)
    mask = (torch.rand(P, 1, generator=gen) > 0.8).float().to(dev)
    A = torch.linalg.qr(torch.randn(3, 3, generator=gen))[0]
    view = torch.eye(4)
    view[:3, :3] = A
    view[3, :3] = torch.tensor([0.5, -0.3, 4.0])
    view = view.to(dev)
    g_out = torch.randn(P, 4, generator=gen).to(dev)
    q = rot.clone().requires_grad_(True)
    fused = lambda: normals.gaussian_normals(scales, q, xyz, view, mask=mask)
    composed = lambda: torch_gaussian_normals(scales, q, xyz, view, mask=mask)

    def step(f):
        q.grad = None
        f().backward(g_out)
    step(fused)
    of, gf = fused().detach(), q.grad.clone()
    step(composed)
    ot, gt = composed().detach(), q.grad.clone()
    agree = (of - ot).abs().amax(dim=1) < 1e-4          # rows on a flip or an axis switch may differ between two float32 evaluations
    r = res["gaussian_normals"] = {"gaussians": P, "columns": 4}
    r["agreement"] = dict(rows_agreeing=int(agree.sum()), value_max_abs_diff=float((of - ot)[agree].abs().max()),
                          grad_max_abs_diff=float((gf - gt)[agree].abs().max()), grad_max_abs=float(gt.abs().max()))
    with torch.no_grad():
        r["forward"] = alternating({"fused": fused, "torch": composed}, a.inner)
    r["forward_backward"] = alternating({"fused": lambda: step(fused), "torch": lambda: step(composed)}, max(1, a.inner // 2))
    for k in ("forward", "forward_backward"):
        r[k]["torch_over_fused"] = round(r[k]["torch"]["ms_median"] / r[k]["fused"]["ms_median"], 2)
    # forward reads 3 + 4 + 3 + 1 floats per row and writes 4; backward reads 3 + 4 + 3 + 4 (the upstream rows whole) and writes 4
    r["model_bytes"] = dict(forward=15 * 4 * P, backward=18 * 4 * P)

    # ---- 2. the consistency loss
    H, W = a.height, a.width
    tan = (W / (2 * 2050.0), H / (2 * 2050.0))
    yy, xx = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing="ij")
    z = 12 + 3 * torch.sin(xx / 70) + 2 * torch.cos(yy / 50) + 0.5 * torch.rand(H, W, generator=gen)
    O = torch.where(torch.rand(H, W, generator=gen) < 0.1, 0.1 + 0.3 * torch.rand(H, W, generator=gen), 0.6 + 0.4 * torch.rand(H, W, generator=gen))
    D = (O / z).to(dev)
    O = O.to(dev)
    N = (torch.randn(3, H, W, generator=gen)).to(dev) * O
    w = torch.rand(H, W, generator=gen).to(dev)
    w[H - H // 5:] = 0                                                  # an ego-vehicle mask under fractional weights
    n_copy = 6 * H * W
    src, dst = torch.rand(n_copy, device=dev), torch.empty(n_copy, device=dev)
    copy = alternating({"copy": lambda: dst.copy_(src)}, a.inner)["copy"]
    copy_rate = 2 * 4 * n_copy / (copy["ms_median"] * 1e-3)
    r = res["normal_consistency"] = {"image": [H, W], "tanfov": [round(t, 4) for t in tan], "weighted": True,
                                     "copy": dict(copy, bytes=2 * 4 * n_copy, GBps=round(copy_rate / 1e9, 1))}
    leaves = [t.clone().requires_grad_(True) for t in (N, D, O)]

    def lstep(term):
        for t in leaves:
            t.grad = None
        term(*leaves).backward()
    lf = lambda n, d, o: normals.normal_consistency_loss(n, d, o, tan, weight=w)
    lt = lambda n, d, o: torch_consistency(n, d, o, w, *tan)
    lstep(lf)
    Lf, gF = lf(*leaves).item(), [t.grad.clone() for t in leaves]
    lstep(lt)
    Lt, gT = lt(*leaves).item(), [t.grad.clone() for t in leaves]
    r["agreement"] = dict(loss_fused=Lf, loss_torch=Lt, grad_max_abs_diff_over_max=[float((x - y).abs().max() / y.abs().max()) for x, y in zip(gF, gT)])
    fb = r["forward_backward"] = alternating({"fused": lambda: lstep(lf), "torch": lambda: lstep(lt)}, max(1, a.inner // 2))
    fb["torch_over_fused"] = round(fb["torch"]["ms_median"] / fb["fused"]["ms_median"], 2)
    p = lambda t: t.data_ptr()
    work = torch.zeros(normals.NORMAL_WORK_DOUBLES, dtype=torch.float64, device=dev)
    out, gl = torch.zeros(1, device=dev), torch.ones(1, device=dev)
    gN, gD, gO = torch.empty_like(N), torch.empty_like(D), torch.empty_like(O)

    def forward():
        _lib.check(lib.adgs_normal_consistency_forward(H, W, p(N), p(D), p(O), p(w), tan[0], tan[1], 1, 0.5, p(work), p(out), st), "forward")

    def backward():
        _lib.check(lib.adgs_normal_consistency_backward(H, W, p(N), p(D), p(O), p(w), tan[0], tan[1], 1, 0.5, p(work), p(gl), p(gN), p(gD), p(gO), st), "backward")
    k = r["kernels"] = alternating({"forward": forward, "backward": backward}, a.inner)
    for name, nbytes in (("forward", 6 * 4 * H * W), ("backward", 11 * 4 * H * W)):
        rate = nbytes / (k[name]["ms_median"] * 1e-3)
        k[name].update(model_bytes=nbytes, GBps=round(rate / 1e9, 1), fraction_of_copy_rate=round(rate / copy_rate, 3))
    del src, dst, leaves, gF, gT

    # ---- 3. the training frame
    if not a.skip_frame:
        from adgs import synthetic
        from adgs.model import SyntheticGaussianModel
        from gaussian_renderer import render
        cfg = synthetic.CONFIGS[a.config]
        sc = synthetic.make_config_scene(a.config)
        cam = synthetic.camera_object(synthetic.make_camera(cfg["W"], cfg["H"], cfg["focal"]), time=0.5)
        for name in ("world_view_transform", "full_proj_transform", "camera_center"):
            setattr(cam, name, getattr(cam, name).to(dev))
        g_img = (torch.randn(3, cfg["H"], cfg["W"], generator=torch.Generator().manual_seed(1)) / (cfg["H"] * cfg["W"])).to(dev)
        m = SyntheticGaussianModel.from_scene(sc, device=dev, seed=0)
        m.raw_sh, m.raw_scene = True, True
        off, on = types.SimpleNamespace(inv_depth=True, debug=False), types.SimpleNamespace(inv_depth=True, debug=False, render_normals=True)

        def frame_off():
            m.zero_grad()
            render(cam, m, None, off, render_objmask=True)["render"].backward(g_img)

        def frame_rows():                                               # the flag's other cost: a raw-scene model materialises its scene rows
            m.zero_grad()
            m.raw_scene = False
            try:
                render(cam, m, None, off, render_objmask=True)["render"].backward(g_img)
            finally:
                m.raw_scene = True

        def frame_on():
            m.zero_grad()
            o = render(cam, m, None, on, render_objmask=True)
            L = normals.normal_consistency_loss(o["img_normal"], o["depth"], o["img_opacity"], cam)
            torch.autograd.backward([o["render"], L], [g_img, torch.ones_like(L) * 0.05])
        f = res["training_frame"] = {"config": a.config, "gaussians": int(sc["P"]), "image": [cfg["H"], cfg["W"]], "model": "raw_scene", "render_objmask": True}
        f.update(alternating({"render_normals_off": frame_off, "render_normals_off_full_rows": frame_rows, "render_normals_on_with_loss": frame_on},
                             max(1, a.inner // 4), rounds=max(3, a.rounds // 2)))
        f["on_minus_off_ms"] = round(f["render_normals_on_with_loss"]["ms_median"] - f["render_normals_off"]["ms_median"], 5)

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
