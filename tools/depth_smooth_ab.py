"""Cost of the edge-aware depth smoothness term (adgs.loss.depth_smoothness_loss; include/adgs_loss.h) at the training resolution, against the
same definition composed from torch operations in float32 on the device -- what a run has without the fused kernels.

    python tools/depth_smooth_ab.py [--height 1280] [--width 1920] [--channels 3] [--rounds 15] [--inner 20] [--out FILE]

HIP-event medians (rounds of `inner` back-to-back calls, ms per call), weighted, with a C-channel guide, for order 1 and order 2:
1. forward + backward through autograd, fused and torch composition, in alternating rounds of one process,
2. the fused forward and backward apart, through the library entry points, with the fraction of the copy rate their byte model implies:
   forward reads (1 + C + 1) * 4 * H * W bytes, backward reads the same and writes 4 * H * W; the copy rate is measured here by a
   device-to-device copy of a buffer of the forward's size (read + write counted).
The two forms are also compared on the timed inputs (loss and gradient), so a wrong fast kernel is not reported as fast.

Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def torch_smoothness(d, img, w, order, normalize=True, gamma=1.0):
    """The definition of include/adgs_loss.h in float32 torch operations (the differences on the un-normalised depth, s on the total)."""
    import torch
    total = 0.0
    for dim in (1, 0):
        n = d.shape[dim] - order
        cut = lambda t, k, dm=dim: t.narrow(dm, k, n)
        if order == 1:
            delta, v = cut(d, 0) - cut(d, 1), cut(w, 0) * cut(w, 1)
            e = (cut(img, 0, dim + 1) - cut(img, 1, dim + 1)).abs().mean(0)
        else:
            delta, v = cut(d, 0) - 2.0 * cut(d, 1) + cut(d, 2), cut(w, 0) * cut(w, 1) * cut(w, 2)
            e = ((cut(img, 1, dim + 1) - cut(img, 0, dim + 1)).abs() + (cut(img, 2, dim + 1) - cut(img, 1, dim + 1)).abs()).mean(0) * 0.5
        total = total + (v * torch.exp(-gamma * e) * delta.abs()).sum() / v.sum()
    return total / ((w * d).sum() / w.sum() + 1e-7) if normalize else total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from adgs import _lib, loss

    if not torch.cuda.is_available():
        raise SystemExit("depth_smooth_ab: no HIP device; nothing is measured without one")
    lib = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = _lib.stream_ptr(dev)
    H, W, C = a.height, a.width, a.channels
    gen = torch.Generator(device="cpu").manual_seed(0)
    depth = (0.05 + 0.3 * torch.rand(H, W, generator=gen)).to(dev)
    img = torch.rand(C, H, W, generator=gen).to(dev)
    w = torch.rand(H, W, generator=gen).to(dev)
    w[H - H // 5:] = 0                                                  # an ego-vehicle mask under fractional weights
    res = {"tool": "depth_smooth_ab", "depth": [H, W], "guide_channels": C, "weighted": True, "rounds": a.rounds, "calls_per_round": a.inner}

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
        """{name: summary} of several callables timed in alternating rounds"""
        for f in fns.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                ms[k].append(events(f, inner))
        return {k: summary(v) for k, v in ms.items()}

    # the copy rate of this device at the forward's footprint
    n_copy = (2 + C) * H * W
    src, dst = torch.rand(n_copy, device=dev), torch.empty(n_copy, device=dev)
    copy = alternating({"copy": lambda: dst.copy_(src)}, a.inner)["copy"]
    copy_rate = 2 * 4 * n_copy / (copy["ms_median"] * 1e-3)
    res["copy"] = dict(copy, bytes=2 * 4 * n_copy, GBps=round(copy_rate / 1e9, 1))

    p = lambda t: t.data_ptr()
    work = torch.zeros(loss.SMOOTH_WORK_DOUBLES, dtype=torch.float64, device=dev)
    out, gl, grad = torch.zeros(1, device=dev), torch.ones(1, device=dev), torch.empty(H, W, device=dev)
    bytes_fwd, bytes_bwd = (2 + C) * 4 * H * W, (3 + C) * 4 * H * W
    for order in (1, 2):
        r = res["order%d" % order] = {}
        x = depth.clone().requires_grad_(True)

        def step(term):
            x.grad = None
            term(x).backward()
        fused = lambda t: loss.depth_smoothness_loss(t, img, w, order=order)
        composed = lambda t: torch_smoothness(t, img, w, order)
        # the same numbers first
        step(fused)
        Lf, gf = fused(x).item(), x.grad.clone()
        step(composed)
        Lt, gt = composed(x).item(), x.grad.clone()
        r["agreement"] = dict(loss_fused=Lf, loss_torch=Lt, grad_max_abs_diff=float((gf - gt).abs().max()), grad_max_abs=float(gt.abs().max()))
        fb = r["forward_backward"] = alternating({"fused": lambda: step(fused), "torch": lambda: step(composed)}, max(1, a.inner // 2))
        fb["torch_over_fused"] = round(fb["torch"]["ms_median"] / fb["fused"]["ms_median"], 2)

        def forward():
            _lib.check(lib.adgs_depth_smooth_forward(H, W, C, p(depth), p(img), p(w), order, 1, 1.0, p(work), p(out), st), "forward")

        def backward():
            _lib.check(lib.adgs_depth_smooth_backward(H, W, C, p(depth), p(img), p(w), order, 1, 1.0, p(work), p(gl), p(grad), st), "backward")
        k = r["kernels"] = alternating({"forward": forward, "backward": backward}, a.inner)
        for name, nbytes in (("forward", bytes_fwd), ("backward", bytes_bwd)):
            rate = nbytes / (k[name]["ms_median"] * 1e-3)
            k[name].update(model_bytes=nbytes, GBps=round(rate / 1e9, 1), fraction_of_copy_rate=round(rate / copy_rate, 3))

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
