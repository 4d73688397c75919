#!/usr/bin/env python3
"""The evaluation loop of render.py:41-106 (`render_set`) on the HIP path: per view a forward-only render() under torch.no_grad()
and ONE fused metrics pass (adgs.metrics.Evaluator.add: clipping, PSNR sums, SSIM, L1, the same sums over the object mask and the sky
mask, the 8-bit image for the PNG / video writer); ONE results() at the end -- the loop's only host synchronisation, where the
reference has an `.item()` per metric and view.

    python examples/evaluate.py [--config C3] [--views 32] [--cameras 16] [--quantize] [--no-metrics] [--color-correct] [--json]

Synthetic scene and cameras.  There are no photographs to compare with, so the ground truth of a view is the scene
rendered at full Gaussian size, and the evaluated render draws the Gaussians at 90 % of it (render()'s scaling_modifier): a model that
is close to, but not, the truth.  The object mask is the ground truth's rendered object channel (> 0.5: the role of
`viewpoint.semantic > 0`, train.py:217), the sky mask its transparent pixels (`viewpoint.sky`, :238).

Prints SSIM, PSNR and FPS the way render.py:86-93 does (FPS = views / time spent in render(), as there), then the same per region and
the second PSNR of the reference (train.py:258: the mean of the per-channel PSNRs).  LPIPS (render.py:61-62) is out of scope: it needs
the pretrained VGG / AlexNet weights, which are not part of this repository.

--color-correct adds the colour-corrected figures that trainers with a bilateral grid report (cc_psnr, cc_ssim, cc_l1): per view
adgs.colorcorrect.color_correct fits a quadratic colour transform of the render to the ground truth and a SECOND Evaluator measures
the transformed render -- still one read-back per Evaluator.  Without the flag nothing changes.
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

REGION_NAMES = ("image", "objects", "sky")
EVAL_SCALING = 0.9


def build(scene, cameras, device, env_res=256):
    """(model, environment map, views): every view carries its ground truth, object mask and sky mask on the device, like the
    reference's Camera (scene/cameras.py: original_image, semantic, sky)."""
    import torch
    from adgs import env, synthetic
    from adgs.model import SyntheticGaussianModel
    from gaussian_renderer import render
    model = SyntheticGaussianModel.from_scene(scene, device=device, seed=0)
    model.raw_sh = True
    env_map = env.EnvironmentMap(env_res, 3, device=device)
    with torch.no_grad():
        env_map.grid_map.copy_(0.5 + 0.2 * torch.randn(env_map.grid_map.shape, generator=torch.Generator().manual_seed(5)).to(device))
    pipe = types.SimpleNamespace(inv_depth=True, debug=False)
    views = []
    for k, (cam, t) in enumerate(cameras):
        view = synthetic.camera_object(cam, time=t)
        view.cam_id = k
        for name in ("world_view_transform", "full_proj_transform", "camera_center"):
            setattr(view, name, getattr(view, name).to(device))
        with torch.no_grad():
            pkg = render(view, model, env_map, pipe, render_objmask=True)
            view.original_image = pkg["render"].clone()
            view.semantic = (pkg["img_semantic"][0] > 0.5).float()
            view.sky = (pkg["img_opacity"] < 0.5).float().reshape(view.semantic.shape)
        views.append(view)
    return model, env_map, views


def render_set(views, model, env_map, n_views=None, metrics=True, quantize=False, u8="round", color_correct=False):
    """render.py:41-106 without the file writing: -> (adgs.metrics.Evaluator.results() or None, seconds in render(), seconds in all,
    the last view's 8-bit image).  The renders are kept by nobody: a caller that wants the PNGs takes the uint8 tensor of each add().
    color_correct: every region's dict also has "cc", the same region of a second Evaluator fed with the colour-corrected render."""
    import torch
    from adgs import colorcorrect
    from adgs.metrics import Evaluator
    from gaussian_renderer import render
    pipe = types.SimpleNamespace(inv_depth=True, debug=False)
    n_views = n_views or len(views)
    dev = views[0].original_image.device
    ev = Evaluator(n_views, regions=2, quantize=quantize, device=dev) if metrics else None
    cc_ev = Evaluator(n_views, regions=2, quantize=quantize, device=dev) if metrics and color_correct else None
    frame = None
    torch.cuda.synchronize(dev)
    total_time, t_all = 0.0, time.perf_counter()
    with torch.no_grad():
        for idx in range(n_views):
            view = views[idx % len(views)]
            t = time.perf_counter()
            rendering = render(view, model, env_map, pipe, scaling_modifier=EVAL_SCALING)["render"]
            total_time += time.perf_counter() - t
            if ev is not None:
                _, frame = ev.add(rendering, view.original_image, masks=(view.semantic, view.sky), u8=u8)
            if cc_ev is not None:
                cc_ev.add(colorcorrect.color_correct(rendering, view.original_image)[0], view.original_image, masks=(view.semantic, view.sky))
    res = ev.results() if ev is not None else None                 # the one device-to-host copy
    if cc_ev is not None:
        for region, cc in zip(res, cc_ev.results()):               # ... and the second Evaluator's
            region["cc"] = cc
    torch.cuda.synchronize(dev)
    return res, total_time, time.perf_counter() - t_all, frame


def report(name, res, n_views, render_time):
    """render.py:86-93, then the regions"""
    print(name)
    print("  SSIM : {}".format(res[0]["mean"]["ssim"]))
    print("  PSNR : {}".format(res[0]["mean"]["psnr"]))
    print("  FPS  : {}".format(n_views / render_time))
    print("")
    for r, region in enumerate(REGION_NAMES):
        m = res[r]["mean"]
        print("  %-8s SSIM %.6f  PSNR %.4f dB  PSNR (mean of channels) %.4f dB  L1 %.6f  over %d of %d views" % (
            region, m["ssim"], m["psnr"], m["psnr_channel_mean"], m["l1"], res[r]["count"], n_views))
        if "cc" in res[r]:
            cc = res[r]["cc"]["mean"]
            print("  %-8s cc_ssim %.6f  cc_psnr %.4f dB  cc_l1 %.6f  (colour-corrected)" % ("", cc["ssim"], cc["psnr"], cc["l1"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--cameras", type=int, default=16)
    ap.add_argument("--quantize", action="store_true", help="metrics of the 8-bit rounded render, as computed from saved PNGs")
    ap.add_argument("--no-metrics", action="store_true", help="the render loop alone")
    ap.add_argument("--color-correct", action="store_true", help="also the metrics of the colour-corrected render (cc_psnr, cc_ssim, cc_l1)")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU fallback")
    import bench
    from adgs import synthetic
    device = torch.device("cuda", 0)
    cfg = synthetic.CONFIGS[args.config]
    model, env_map, views = build(synthetic.make_config_scene(args.config), bench.camera_pool(cfg, args.cameras), device)
    cc = args.color_correct
    render_set(views, model, env_map, min(args.views, 4), metrics=not args.no_metrics, quantize=args.quantize, color_correct=cc)        # warm-up
    res, render_time, all_time, _ = render_set(views, model, env_map, args.views, metrics=not args.no_metrics, quantize=args.quantize, color_correct=cc)
    out = {"config": args.config, "views": args.views, "metrics": not args.no_metrics, "quantize": args.quantize,
           "render_fps": round(args.views / render_time, 2), "views_per_s": round(args.views / all_time, 2)}
    if res is not None:
        out["regions"] = {name: dict(res[r]["mean"], count=res[r]["count"]) for r, name in enumerate(REGION_NAMES)}
        if cc:
            out["cc_regions"] = {name: {"cc_" + k: res[r]["cc"]["mean"][k] for k in ("psnr", "ssim", "l1")} for r, name in enumerate(REGION_NAMES)}
    if args.json:
        print(json.dumps(out))
    elif res is not None:
        report("synthetic " + args.config, res, args.views, render_time)
        print("  %.1f views/s with the metrics%s and the 8-bit image" % (out["views_per_s"], ", the colour correction" if cc else ""))
    else:
        print("synthetic %s\n  FPS  : %s (no metrics)" % (args.config, out["render_fps"]))


if __name__ == "__main__":
    main()
