"""Cost of the fused evaluation pass (adgs.metrics; include/adgs_metrics.h) at the evaluation resolution, against what a user had
without it.

    python tools/metrics_ab.py [--height 1280] [--width 1920] [--views 40] [--rounds 9] [--config C3] [--loop-views 48] [--no-loop] [--out FILE]

Per view, 3 channels:
1. `fused`: Evaluator.add with 2 regions and the rounded 8-bit image (one kernel + a finishing kernel); `fused_whole_image_only`: the
   same with no region -- exactly the work of the composition below.
2. `composition`: the loop body a user assembles from the parts of the parent commit: torch.clamp of the render and of the ground
   truth, adgs.loss.ssim (the training loss's kernel, forward only), a torch MSE -> PSNR, save_image's 8-bit conversion
   (mul, add, clamp, permute, to(uint8)) and an .item() per metric and view as in render.py:59-60.  No regions: the SSIM map is
   never materialised, so the composition cannot weigh it.
Each as the wall-clock time per view of `views` back-to-back views (the composition synchronises per view by construction; the fused
loop reads back once at the end) and, for the fused pass, as HIP-event time of the launches alone.  Medians over `rounds`.
3. views/s of examples/evaluate.py's loop on `config`, with and without the metrics.

Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--loop-views", type=int, default=48)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from adgs import loss, metrics

    dev = torch.device("cuda", torch.cuda.current_device())
    H, W, N = a.height, a.width, a.views
    gen = torch.Generator().manual_seed(0)
    gt = torch.rand(3, H, W, generator=gen).to(dev)
    img = (gt + 0.15 * torch.randn(3, H, W, generator=gen).to(dev)).contiguous()
    masks = (torch.rand(2, H, W, generator=gen) > 0.7).float().to(dev)

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.rounds):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t) * 1e3 / N)
        return dict(ms_per_view_median=round(statistics.median(ms), 5), ms_per_view_min=round(min(ms), 5), ms_per_view_max=round(max(ms), 5))

    def fused_loop(regions, u8):
        ev = metrics.Evaluator(N, regions=regions, device=dev)
        m = masks if regions else None

        def run():
            ev.reset()
            for _ in range(N):
                ev.add(img, gt, m, u8=u8)
            return ev.results()[0]["mean"]
        return run, ev

    def composition():
        psnrs, ssims, frame = [], [], None
        with torch.no_grad():
            for _ in range(N):
                rendering, ref = torch.clamp(img, 0.0, 1.0), torch.clamp(gt, 0.0, 1.0)
                mse = ((rendering - ref) ** 2).reshape(1, -1).mean(1, keepdim=True)
                psnrs.append((20 * torch.log10(1.0 / torch.sqrt(mse))).item())
                ssims.append(loss.ssim(rendering, ref).item())
                frame = rendering.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).contiguous()
        return {"psnr": sum(psnrs) / N, "ssim": sum(ssims) / N}, frame

    res = {"tool": "metrics_ab", "image": [3, H, W], "views_per_round": N, "rounds": a.rounds}
    run2, ev2 = fused_loop(2, "round")
    run0, _ = fused_loop(0, "round")
    res["fused"] = wall(run2)
    res["fused_whole_image_only"] = wall(run0)
    res["composition"] = wall(composition)
    # the launches alone
    ev2.reset()
    ms = []
    for _ in range(a.rounds):
        ev2.reset(zero=False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N):
            ev2.add(img, gt, masks, u8="round")
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / N)
    res["fused"]["device_ms_per_view_median"] = round(statistics.median(ms), 5)
    res["fused"]["algorithmic_bytes"] = (2 * 3 * 4 + 2 * 4 + 3) * H * W
    res["fused"]["tb_per_s"] = round(res["fused"]["algorithmic_bytes"] / (res["fused"]["device_ms_per_view_median"] * 1e-3) / 1e12, 3)
    res["composition_over_fused"] = round(res["composition"]["ms_per_view_median"] / res["fused"]["ms_per_view_median"], 2)
    res["composition_over_fused_whole_image_only"] = round(res["composition"]["ms_per_view_median"] / res["fused_whole_image_only"]["ms_per_view_median"], 2)
    want, got = composition()[0], run0()
    res["agreement"] = {"psnr_diff_db": abs(want["psnr"] - got["psnr"]), "ssim_diff": abs(want["ssim"] - got["ssim"])}

    if not a.no_loop:
        import bench
        from adgs import synthetic
        from examples import evaluate as example
        cfg = synthetic.CONFIGS[a.config]
        model, env_map, views = example.build(synthetic.make_config_scene(a.config), bench.camera_pool(cfg, 16), dev)
        loop = {"config": a.config, "views": a.loop_views}
        for name, on in (("with_metrics", True), ("without_metrics", False)):
            example.render_set(views, model, env_map, 8, metrics=on)
            rates = []
            for _ in range(3):
                _, render_time, all_time, _ = example.render_set(views, model, env_map, a.loop_views, metrics=on)
                rates.append(a.loop_views / all_time)
            loop[name + "_views_per_s"] = round(statistics.median(rates), 2)
        loop["metrics_cost_ms_per_view"] = round(1e3 / loop["with_metrics_views_per_s"] - 1e3 / loop["without_metrics_views_per_s"], 4)
        res["example_loop"] = loop

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
