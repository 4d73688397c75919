"""Cost of the absolute screen-space gradient (AbsGS; GaussianRasterizer.forward(means2D_abs=...), adgs_raster_backward_options) at a
benchmark config.

    python tools/absgrad_ab.py [--config C3] [--rounds 6] [--frames 20] [--no-profile] [--out FILE]

1. Frame times of the training frame (forward + backward through the drop-in GaussianRasterizer, the upstream gradients of bench.py's
   loss), the request off and on ALTERNATED in one process (rounds x frames of each, off / on / off / ...): median ms per frame.
2. Unless --no-profile: a separate child process of the same frames under `rocprofv3 --kernel-trace --stats`, for the per-kernel times
   of the blend backward (render_bwd_v2_kernel<PPL, FULL, ABS>: the instantiation without and with the two extra sums) and of the
   preprocess backward (the same kernel either way; it writes one more [P,3] row when asked).

Prints one JSON line; --out also writes it to a file.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _frames(cfg):
    import torch
    from adgs import _lib, synthetic
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    sc = synthetic.make_config_scene(cfg)
    g = synthetic.make_upstream_grads(sc, 0)
    d = lambda t: t.cuda()
    t = {k: d(sc[k]) for k in ("means3D", "opacities", "shs", "scales", "rotations", "flow_points", "semantic")}
    gd = {k: d(v) for k, v in g.items()}

    rast = GaussianRasterizer(GaussianRasterizationSettings(sc["H"], sc["W"], sc["tanfovx"], sc["tanfovy"], d(sc["bg"]), 1.0, d(sc["viewmatrix"]),
                                                            d(sc["projmatrix"]), sc["sh_degree"], d(sc["campos"]), False, True, False))
    leaf = {k: v.clone().requires_grad_(True) for k, v in t.items() if k not in ("flow_points", "semantic")}
    m2 = torch.zeros(sc["P"], 3, device="cuda", requires_grad=True)
    m2a = torch.zeros(sc["P"], 3, device="cuda", requires_grad=True)

    def train(absgrad):
        kw = dict(means2D_abs=m2a) if absgrad else {}
        color, radii, depth, op, flow, sem = rast(means3D=leaf["means3D"], means2D=m2, opacities=leaf["opacities"], shs=leaf["shs"], scales=leaf["scales"],
                                                  rotations=leaf["rotations"], flow_points=t["flow_points"], semantic=t["semantic"], **kw)
        n = _lib.frame_stats()["num_rendered"]
        # all five images carry a gradient: the training configuration (the blend backward's FULL instantiation)
        loss = (color * gd["color"]).sum() + (depth * gd["depth"]).sum() + (op * gd["img_opacity"]).sum() + (flow * gd["flow"]).sum() + (sem * gd["semantic"]).sum()
        for v in list(leaf.values()) + [m2, m2a]:
            v.grad = None
        loss.backward()
        return n
    return train


def measure(cfg, rounds, frames):
    import torch
    train = _frames(cfg)
    out = {}
    for name, fn in (("train_fwd_bwd", train),):
        for aa in (False, True):      # warm-up: capacity hints, tile orders, allocator
            for _ in range(3):
                fn(aa)
        torch.cuda.synchronize()
        per = {False: [], True: []}
        pairs = {}
        for r in range(rounds):
            for aa in ((False, True) if r % 2 == 0 else (True, False)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(frames):
                    pairs[aa] = fn(aa)
                b.record()
                torch.cuda.synchronize()
                per[aa].append(a.elapsed_time(b) / frames)
        out[name] = {("absgrad_on" if aa else "absgrad_off"): dict(ms_median=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4),
                                                         pairs=int(pairs[aa])) for aa, v in per.items()}
        off, on = out[name]["absgrad_off"]["ms_median"], out[name]["absgrad_on"]["ms_median"]
        out[name]["delta_ms"] = round(on - off, 4)
    return out


def child_kernels(cfg, frames):
    """What the profiled child runs: the same frames, the request off then on."""
    import torch
    train = _frames(cfg)
    for absgrad in (False, True):
        for _ in range(frames):
            train(absgrad)
    torch.cuda.synchronize()


def profile(cfg, frames, timeout):
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="absgrad_ab_")
    cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--",
           sys.executable, os.path.abspath(__file__), "--child-kernels", "--config", cfg, "--frames", str(frames)]
    r = subprocess.run(cmd, cwd=ROOT, timeout=timeout, capture_output=True, text=True)
    if r.returncode != 0:
        return {"error": "rocprofv3 exit %d" % r.returncode, "tail": (r.stdout + r.stderr)[-2000:]}
    files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return {"error": "no kernel_stats.csv under " + tmp}
    res = {}
    for row in csv.DictReader(open(files[0])):
        name = row["Name"]
        if "render_bwd_v2_kernel<" in name:
            args = name.split("render_bwd_v2_kernel<", 1)[1].split(">", 1)[0].replace(" ", "")      # "<PPL, FULL, ABS>"
            ppl, full, ab = args.split(",")[:3]
            key = "render_bwd_v2_kernel<ppl=%s,full=%s>" % (ppl, full)
            res.setdefault(key, {})["absgrad_on" if ab == "true" else "absgrad_off"] = dict(calls=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) / 1e3, 2))
        elif "preprocess_bwd_kernel<" in name:       # one instantiation serves both halves of the run
            res["preprocess_bwd_kernel (off and on together)"] = dict(calls=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) / 1e3, 2))
    for v in res.values():
        if "absgrad_on" in v and "absgrad_off" in v:
            v["delta_us"] = round(v["absgrad_on"]["avg_us"] - v["absgrad_off"]["avg_us"], 2)
            v["ratio"] = round(v["absgrad_on"]["avg_us"] / v["absgrad_off"]["avg_us"], 4)
    shutil.rmtree(tmp, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-timeout", type=float, default=600.0)
    ap.add_argument("--child-kernels", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child_kernels:
        child_kernels(a.config, a.frames)
        return
    res = {"tool": "absgrad_ab", "config": a.config, "rounds": a.rounds, "frames_per_round": a.frames}
    res.update(measure(a.config, a.rounds, a.frames))
    if not a.no_profile:
        res["kernels"] = profile(a.config, min(a.frames, 10), a.profile_timeout)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
