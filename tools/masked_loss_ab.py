"""Cost of the per-pixel supervision weight of the image losses (adgs.loss with `weight=`; include/adgs_loss.h) at the training resolution.

    python tools/masked_loss_ab.py [--height 1280] [--width 1920] [--rounds 15] [--inner 20] [--out FILE]

HIP-event medians (rounds of `inner` back-to-back forward + backward pairs, ms per pair) on a 3 x H x W image of
1. the unweighted l1_ssim -- the kernels every run without a weight uses: the yardstick,
2. the weighted form with a weight of ones (what the weight itself costs),
3. the weighted form with the bottom 20 % of the rows zero (an ego-vehicle mask: whether skipping all-zero tiles pays),
4. a torch composition of the same weighted loss (depthwise conv2d SSIM map, autograd backward) -- what a masked run has without the feature,
and of the fused image_losses node without and with the weight.  Forward and backward are also timed apart through the library entry
points for 1 - 3.

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
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F
    from adgs import _lib, loss

    lib = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = _lib.stream_ptr(dev)
    H, W = a.height, a.width
    gen = torch.Generator(device="cpu").manual_seed(0)
    gt = torch.rand(3, H, W, generator=gen).to(dev)
    img = (gt + 0.05 * torch.randn(3, H, W, generator=gen).to(dev)).clamp(0, 1)
    ones = torch.ones(H, W, device=dev)
    ego = ones.clone()
    ego[H - H // 5:] = 0
    weights = (("weighted_ones", ones), ("weighted_bottom_fifth_zero", ego))
    res = {"tool": "masked_loss_ab", "image": [3, H, W], "rounds": a.rounds, "calls_per_round": a.inner}

    def pair(fn, inner=a.inner):
        x = img.clone().requires_grad_(True)

        def step():
            l1, s = fn(x)
            x.grad = None
            (0.8 * l1 - 0.2 * s).backward()
        return timed(step, a.rounds, inner)

    # 1 - 3 through autograd, as a training iteration calls them
    fb = res["forward_backward"] = {"unweighted": pair(lambda x: loss.l1_ssim(x, gt))}
    for name, w in weights:
        fb[name] = pair(lambda x, w=w: loss.l1_ssim(x, gt, weight=w))

    # 4: the torch composition
    g1 = torch.tensor([math.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2)) for k in range(11)])
    g1 = g1 / g1.sum()
    window = (g1[:, None] * g1[None, :])[None, None].expand(3, 1, 11, 11).contiguous().to(dev)
    C1, C2 = 0.01 ** 2, 0.03 ** 2

    def torch_loss(x, w):
        conv = lambda t: F.conv2d(t[None], window, padding=5, groups=3)[0]
        mu1, mu2 = conv(x), conv(gt)
        s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(gt * gt) - mu2 * mu2, conv(x * gt) - mu1 * mu2
        smap = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
        n = 3 * w.sum()
        return (w * (x - gt).abs()).sum() / n, (w * smap).sum() / n
    fb["torch_weighted_bottom_fifth_zero"] = pair(lambda x: torch_loss(x, ego), max(1, a.inner // 4))
    for k in list(fb):
        if k != "unweighted":
            fb[k]["over_unweighted"] = round(fb[k]["ms_median"] / fb["unweighted"]["ms_median"], 3)

    # the same kernels apart, through the library entry points
    p = lambda t: t.data_ptr()
    maps = [torch.empty_like(img) for _ in range(3)]
    out2, gl, gs, d_img = torch.zeros(2, device=dev), torch.full((1,), 0.8, device=dev), torch.full((1,), -0.2, device=dev), torch.empty_like(img)
    sums = torch.zeros(2 * loss.SLOTS, dtype=torch.float64, device=dev)
    work = torch.zeros(loss.L1_SSIM_WEIGHTED_WORK_DOUBLES, dtype=torch.float64, device=dev)

    def unweighted_forward():
        _lib.check(lib.adgs_l1_ssim_forward(3, H, W, p(img), p(gt), p(sums), *[p(m) for m in maps], st), "forward")
        _lib.check(lib.adgs_l1_ssim_means(p(sums), img.numel(), p(out2), st), "means")
    ker = res["kernels"] = {"unweighted": {
        "forward": timed(unweighted_forward, a.rounds, a.inner),
        "backward": timed(lambda: _lib.check(lib.adgs_l1_ssim_backward(3, H, W, p(img), p(gt), *[p(m) for m in maps], p(gl), p(gs), p(d_img), st), "backward"),
                          a.rounds, a.inner)}}
    for name, w in weights:
        ker[name] = {
            "forward": timed(lambda w=w: _lib.check(lib.adgs_l1_ssim_weighted_forward(3, H, W, p(img), p(gt), p(w), p(work), *[p(m) for m in maps], p(out2), st),
                                                    "forward"), a.rounds, a.inner),
            "backward": timed(lambda w=w: _lib.check(lib.adgs_l1_ssim_weighted_backward(3, H, W, p(img), p(gt), p(w), *[p(m) for m in maps], p(work), p(gl), p(gs),
                                                                                        p(d_img), st), "backward"), a.rounds, a.inner)}

    # the fused node of a training iteration, without and with the weight
    r = lambda *s: torch.rand(*s, generator=gen).to(dev)
    K = torch.tensor([[1000.0, 0.0, W / 2.0], [0.0, 1000.0, H / 2.0], [0.0, 0.0, 1.0]], device=dev)
    flow_pkg = (None, K, torch.eye(3, device=dev), torch.tensor([0.05, -0.02, 0.1], device=dev), torch.stack([r(H, W) * (W - 1), r(H, W) * (H - 1)]),
                (r(H, W) > 0.3).float())
    gt_depth, gt_sem, gt_sky = r(H, W) * 0.5 + 0.01, (r(H, W) > 0.8).float(), (r(H, W) > 0.7).float()
    leaves = [t.requires_grad_(True) for t in (img.clone(), r(H, W) * 0.4 + 0.05, torch.cat([r(2, H, W) * 4 - 2, r(1, H, W) * 5 + 1]), r(H, W) * 0.98 + 0.01,
                                                r(1, H, W))]
    mix = torch.tensor([0.8, 0.2, 0.1, 0.1, 0.1, 0.05], device=dev)

    def node(w):
        x, dep, fl, op, sem = leaves
        terms = loss.image_losses(x, gt, dep, gt_depth, fl, flow_pkg, op, sem, gt_sem, gt_sky, dist=0.02, weight=w)
        for t in leaves:
            t.grad = None
        (torch.stack(terms) * mix).sum().backward()
    il = res["image_losses"] = {"unweighted": timed(lambda: node(None), a.rounds, a.inner), "weighted_bottom_fifth_zero": timed(lambda: node(ego), a.rounds, a.inner)}
    il["weighted_bottom_fifth_zero"]["over_unweighted"] = round(il["weighted_bottom_fifth_zero"]["ms_median"] / il["unweighted"]["ms_median"], 3)

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
