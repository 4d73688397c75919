"""Cost of the colour fit (adgs.colorcorrect; include/adgs_colorcorrect.h) at the evaluation resolution, against the same algorithm
composed from torch operations.

    python tools/colorcorrect_ab.py [--height 1280] [--width 1920] [--views 40] [--rounds 9] [--composition-views N] [--composition-rounds N]
                                    [--model quadratic] [--out FILE]

Per view, at the default parameters (5 iterations, eps 0.5/255, ridge 1e-6):
1. `fit_apply`: colorcorrect.color_correct (per iteration an accumulate and a finishing launch, then the apply launch); `fit` and `apply`
   each alone.
2. `composition`: the definition written with torch operations that exist without the kernels: float64 on the device, the feature
   matrix A [N, 10] materialised per iteration, the masks as element-wise products, the normal equations by `A.T @ (m * A)` and
   torch.linalg.solve on the device (`solver: device`), or, where that is unavailable, on the host (`solver: host`: a read-back per
   iteration).
Each as the wall-clock time per view of `views` back-to-back views with ONE synchronisation at the end, and as HIP-event time of the
same loop.  Medians over `rounds`, after a warm-up round (the composition is slow -- a [10, N] x [N, 10] float64 product per channel
and iteration --: --composition-views / --composition-rounds shorten its part, and the result says what was used).  `agreement`: the
largest difference of the two corrected images.  Every part's figures are printed to stderr as soon as they exist.

Prints one JSON line; --out also writes it to a file (default: profiles/colorcorrect/colorcorrect_ab.json).
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
    ap.add_argument("--composition-views", type=int)
    ap.add_argument("--composition-rounds", type=int)
    ap.add_argument("--model", default="quadratic", choices=["affine", "quadratic"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colorcorrect", "colorcorrect_ab.json"))
    a = ap.parse_args()

    import torch
    from adgs import colorcorrect

    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: a time measured elsewhere says nothing")
    dev = torch.device("cuda", torch.cuda.current_device())
    H, W, N = a.height, a.width, a.views
    iters, eps, ridge = 5, colorcorrect.DEFAULT_EPS, colorcorrect.DEFAULT_RIDGE
    gen = torch.Generator().manual_seed(0)
    gt = (torch.rand(3, H, W, generator=gen) * 1.1 - 0.05).to(dev)
    img = (0.8 * gt + 0.07 + 0.05 * torch.randn(3, H, W, generator=gen).to(dev)).contiguous()
    fitter = colorcorrect.ColorFitter(dev)
    warp = fitter.fit(img, gt, model=a.model)

    def features(x):
        r, g, b = x
        if a.model == "affine":
            return torch.stack([r, g, b, torch.ones_like(r)], 1)
        return torch.stack([r, g, b, r * r, r * g, r * b, g * g, g * b, b * b, torch.ones_like(r)], 1)

    solver = {"used": "device"}

    def solve(A, b):
        if solver["used"] == "device":
            try:
                return torch.linalg.solve(A, b)
            except RuntimeError:
                solver["used"] = "host"
        return torch.linalg.solve(A.cpu(), b.cpu()).to(dev)

    def composed(image, ref):
        e = float(torch.tensor(eps, dtype=torch.float32))
        x0 = image.clamp(0.0, 1.0).double().reshape(3, -1)
        y = ref.clamp(0.0, 1.0).double().reshape(3, -1)
        ok = lambda z: (z >= e) & (z <= 1.0 - e)
        fixed = ok(x0) & ok(y)
        x = x0
        for _ in range(iters):
            A = features(x)
            n = A.shape[1]
            rows = []
            for c in range(3):
                m = (fixed[c] & ok(x[c])).double()
                G = A.T @ (m[:, None] * A) + ridge * torch.eye(n, dtype=torch.float64, device=dev)
                h = A.T @ (m * y[c])
                h[c] += ridge
                rows.append(solve(G, h))
            x = (torch.stack(rows) @ A.T).clamp(0.0, 1.0)
        return x.float().reshape(3, H, W)

    def timed(name, body, views=None, rounds=None):
        views, rounds = views or N, rounds or a.rounds

        def loop():
            for _ in range(views):
                body()
        loop()
        torch.cuda.synchronize()
        wall, device = [], []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = time.perf_counter()
            e0.record()
            loop()
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t) * 1e3 / views)
            device.append(e0.elapsed_time(e1) / views)
        out = dict(wall_ms_per_view_median=round(statistics.median(wall), 5), wall_ms_per_view_min=round(min(wall), 5),
                   wall_ms_per_view_max=round(max(wall), 5), device_ms_per_view_median=round(statistics.median(device), 5),
                   views_per_round=views, rounds=rounds)
        print(name, json.dumps(out), file=sys.stderr, flush=True)
        return out

    res = {"tool": "colorcorrect_ab", "image": [3, H, W], "model": a.model, "iters": iters}
    with torch.no_grad():
        res["fit_apply"] = timed("fit_apply", lambda: colorcorrect.apply(img, fitter.fit(img, gt, model=a.model)))
        res["fit"] = timed("fit", lambda: fitter.fit(img, gt, model=a.model))
        res["apply"] = timed("apply", lambda: colorcorrect.apply(img, warp))
        res["composition"] = timed("composition", lambda: composed(img, gt), a.composition_views, a.composition_rounds)
        res["composition"]["solver"] = solver["used"]
        res["composition_over_fit_apply"] = round(res["composition"]["device_ms_per_view_median"] / res["fit_apply"]["device_ms_per_view_median"], 2)
        # bytes the algorithm needs: per iteration the six image planes once, the apply three in and three out
        res["fit"]["algorithmic_bytes"] = iters * 6 * 4 * H * W
        res["apply"]["algorithmic_bytes"] = 6 * 4 * H * W
        res["agreement"] = {"max_abs_image_diff": float((composed(img, gt) - colorcorrect.apply(img, fitter.fit(img, gt, model=a.model))).abs().max())}

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
