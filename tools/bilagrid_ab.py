"""Cost of the bilateral-grid appearance compensation (adgs.bilagrid; include/adgs_bilagrid.h) at the training resolution.

    python tools/bilagrid_ab.py [--height 1280] [--width 1920] [--images 200] [--rounds 15] [--inner 20] [--out FILE]

HIP-event medians (rounds of `inner` back-to-back calls, ms per call) with the default 16 x 16 x 8 grid of
1. the slice forward and backward (the library entry points; the backward accumulates into one gradient buffer, both outputs asked),
2. the same function through F.grid_sample and autograd on the same GPU -- what a user has without the feature,
3. the total variation forward and backward over `images` grids,
4. the Adam step over `images` grids, dense and visibility-masked with one image used.
For the slice also the achieved fraction of its algorithmic bytes (forward 24 H W, backward 36 H W) over the copy rate of
profiles/r06/hbm_rates.txt (the row nearest in size), and which path the backward takes at this shape.

Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import math
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def copy_rate(nbytes):
    """(TB/s, MB of the row) of the copy rate measured nearest to a working set of nbytes"""
    rows = []
    for line in open(os.path.join(ROOT, "profiles", "r06", "hbm_rates.txt")):
        m = re.match(r"\s*(\d+) MB: copy ([\d.]+) TB/s", line)
        if m:
            rows.append((int(m.group(1)), float(m.group(2))))
    mb, rate = min(rows, key=lambda r: abs(math.log(r[0] * 1e6 / nbytes)))
    return rate, mb


def timed(fn, rounds, inner):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return dict(ms_median=round(statistics.median(ms), 5), ms_min=round(min(ms), 5), ms_max=round(max(ms), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F
    from adgs import _lib, bilagrid
    from adgs.optim import FusedAdam

    lib = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = _lib.stream_ptr(dev)
    H, W, N = a.height, a.width, a.images
    L, Hg, Wg = 8, 16, 16
    gen = torch.Generator(device="cpu").manual_seed(0)
    # a smooth image with pixel noise, like a render: neighbouring pixels mostly share their luma level
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    img = torch.stack([0.5 + 0.4 * torch.sin(6 * xx + 3 * yy), 0.5 + 0.4 * torch.cos(5 * yy), 0.2 + 0.6 * xx * yy])
    img = (img + 0.02 * torch.randn(3, H, W, generator=gen)).contiguous().to(dev)
    noise = torch.rand(3, H, W, generator=gen).to(dev)            # every pixel its own luma level: no neighbours to merge
    grids = (bilagrid.identity_grids(N, Wg, Hg, L, "cpu") + 0.1 * torch.randn(N, 12, L, Hg, Wg, generator=gen)).to(dev)
    grid = grids[1]
    d_out = torch.randn(3, H, W, generator=gen).to(dev)
    out, d_img, d_grid = torch.empty_like(img), torch.empty_like(img), torch.zeros_like(grid)
    p = lambda t: t.data_ptr()

    res = {"tool": "bilagrid_ab", "image": [H, W], "grid": [L, Hg, Wg], "images": N, "rounds": a.rounds, "calls_per_round": a.inner,
           "backward_path": bilagrid.backward_path(grids, img)}
    sl = res["slice"] = {}
    for name, im in (("smooth_image", img), ("noise_image", noise)):
        sl[name] = {
            "forward": timed(lambda: _lib.check(lib.adgs_bilagrid_slice_forward(L, Hg, Wg, p(grid), H, W, p(im), p(out), st), "forward"), a.rounds, a.inner),
            "backward": timed(lambda: _lib.check(lib.adgs_bilagrid_slice_backward(L, Hg, Wg, p(grid), H, W, p(im), p(d_out), p(d_grid), p(d_img), st), "backward"),
                              a.rounds, a.inner),
            "backward_grid_only": timed(lambda: _lib.check(lib.adgs_bilagrid_slice_backward(L, Hg, Wg, p(grid), H, W, p(im), p(d_out), p(d_grid), None, st), "backward"),
                                        a.rounds, a.inner),
            "backward_image_only": timed(lambda: _lib.check(lib.adgs_bilagrid_slice_backward(L, Hg, Wg, p(grid), H, W, p(im), p(d_out), None, p(d_img), st), "backward"),
                                         a.rounds, a.inner),
        }
        for which, nbytes in (("forward", 24 * H * W), ("backward", 36 * H * W)):
            rate, mb = copy_rate(nbytes)
            t = sl[name][which]
            t["algorithmic_bytes"] = nbytes
            t["tb_per_s"] = round(nbytes / (t["ms_median"] * 1e-3) / 1e12, 3)
            t["fraction_of_copy_rate"] = round(t["tb_per_s"] / rate, 3)
            t["copy_rate_tb_per_s"], t["copy_rate_row_mb"] = rate, mb

    # the same function with torch: 5-D grid_sample + the affine map, autograd for the backward
    x = ((torch.arange(W, device=dev) + 0.5) / W)[None, :].expand(H, W)
    y = ((torch.arange(H, device=dev) + 0.5) / H)[:, None].expand(H, W)

    def torch_slice(g, im):
        gray = 0.299 * im[0] + 0.587 * im[1] + 0.114 * im[2]
        coords = torch.stack([x, y, gray], dim=-1) * 2 - 1
        A = F.grid_sample(g[None], coords[None, None], mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0]
        return torch.stack([A[4 * i] * im[0] + A[4 * i + 1] * im[1] + A[4 * i + 2] * im[2] + A[4 * i + 3] for i in range(3)])

    gs = res["grid_sample"] = {}
    for name, im in (("smooth_image", img), ("noise_image", noise)):
        with torch.no_grad():
            fwd = timed(lambda: torch_slice(grid, im), a.rounds, a.inner)
        gg, ii = grid.clone().requires_grad_(True), im.clone().requires_grad_(True)
        o = torch_slice(gg, ii)
        bwd = timed(lambda: torch.autograd.grad(o, (gg, ii), d_out, retain_graph=True), a.rounds, max(1, a.inner // 4))
        gs[name] = {"forward": fwd, "backward": bwd,
                    "forward_over_hip": round(fwd["ms_median"] / sl[name]["forward"]["ms_median"], 2),
                    "backward_over_hip": round(bwd["ms_median"] / sl[name]["backward"]["ms_median"], 2)}
        del o, gg, ii

    work = torch.zeros(bilagrid.TV_WORK_DOUBLES, dtype=torch.float64, device=dev)
    loss, g_loss, d_grids = torch.zeros(1, device=dev), torch.ones(1, device=dev), torch.empty_like(grids)
    res["total_variation"] = {
        "forward": timed(lambda: _lib.check(lib.adgs_bilagrid_tv_forward(N, L, Hg, Wg, p(grids), p(work), p(loss), st), "tv"), a.rounds, a.inner),
        "backward": timed(lambda: _lib.check(lib.adgs_bilagrid_tv_backward(N, L, Hg, Wg, p(grids), p(g_loss), p(d_grids), st), "tv"), a.rounds, a.inner),
    }

    adam = res["adam_step"] = {}
    grad = torch.zeros_like(grids)
    grad[1] = torch.randn_like(grid)
    used = torch.zeros(N, dtype=torch.uint8, device=dev)
    used[1] = 1
    for name, masked in (("dense", False), ("masked_one_image_used", True)):
        param = torch.nn.Parameter(grids.clone())
        group = {"params": [param], "lr": 2e-3, "name": "bilagrid"}
        if masked:
            group["visibility_rows"] = "head"
        opt = FusedAdam([group], lr=0.0, eps=1e-15)
        param.grad = grad.clone()
        adam[name] = timed((lambda: opt.step(visibility=used)) if masked else (lambda: opt.step()), a.rounds, a.inner)

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
