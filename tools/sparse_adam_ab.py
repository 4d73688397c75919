"""Cost of the visibility-masked Adam step (adgs_adam_step_rows, FusedAdam.step(visibility=...)) against the dense step.

    python tools/sparse_adam_ab.py [--config C3] [--rounds 9] [--reps 20] [--iters 60] [--parent-lib FILE] [--no-iteration] [--out FILE]

1. The Gaussian optimizer's step alone, at the size of the config: the 18 groups of SyntheticGaussianModel.training_setup with a gradient on
   every one, ONE launch per step, the variants ALTERNATED in one process (rounds x reps launches of each between two HIP events; median
   microseconds per launch over the rounds, and the 10 % / 90 % quantiles -- the spread between repeated runs of the same variant is the
   resolution of every difference below).  Variants: the dense step (`dense`, and `dense_again`, the same call measured a second time per
   round), the dense step of another build of the library (`--parent-lib`: the yardstick, e.g. the parent commit's libadgs_hip.so), and the
   masked step for these visibilities: all rows visible; the radii of the config's own first camera; fractions 0.5 / 0.25 / 0.05 of the
   rows visible, once in contiguous runs of 4096 rows (frustum-like) and once scattered uniformly.
   Next to each time: the bytes of DESIGN.md section 5's model (dense 28 B per element; masked 28 * L per visible row + 4 B of visibility
   per row), in all and per group, and the per-group times (each group launched alone) for the groups' row lengths L.
2. Unless --no-iteration: the whole training iteration of examples/train_iteration.py with the separate Adam step, dense against
   training_setup(sparse_adam=True) + step(visibility=radii), each `--iters` iterations after a warm-up, alternated over fresh models.

Prints one JSON line; --out also writes it to a file.  Needs an MI355X: there is no CPU path.
"""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _train_iteration():
    spec = importlib.util.spec_from_file_location("train_iteration", os.path.join(ROOT, "examples", "train_iteration.py"))
    ti = importlib.util.module_from_spec(spec); spec.loader.exec_module(ti)
    return ti


def _quantiles(v):
    v = sorted(v)
    q = lambda f: v[min(len(v) - 1, max(0, int(round(f * (len(v) - 1)))))]
    return dict(us_median=round(statistics.median(v), 2), us_p10=round(q(0.1), 2), us_p90=round(q(0.9), 2))


def _masks(N, radii, dev):
    import torch
    g = torch.Generator().manual_seed(17)
    out = {"all_visible": torch.ones(N, dtype=torch.int32), "camera_radii": radii.detach().cpu().to(torch.int32)}
    run = 4096
    for f in (0.5, 0.25, 0.05):
        runs = (torch.rand((N + run - 1) // run, generator=g) < f).to(torch.int32)
        out["runs_%g" % f] = runs.repeat_interleave(run)[:N].contiguous()
        out["scattered_%g" % f] = (torch.rand(N, generator=g) < f).to(torch.int32)
    return {k: v.to(dev) for k, v in out.items()}


def step_ab(config, rounds, reps, parent_lib):
    import torch
    from adgs import _lib
    from adgs.optim import AdamGroup, AdamRows, ROWS_DENSE, ROWS_INT32, mark_visibility_groups
    from gaussian_renderer import render
    import types
    ti = _train_iteration()
    dev = torch.device("cuda", 0)
    cfg, model, cams, env_map = ti.build(config, 256, dev, 2, False)
    marks = mark_visibility_groups(model.optimizer)
    with torch.no_grad():
        radii = render(cams[0], model, env_map, types.SimpleNamespace(inv_depth=True, debug=False), flow_pkg=cams[0].flow[0], render_objmask=True)["radii"]
    N = int(radii.numel())
    masks = _masks(N, radii, dev)
    g = torch.Generator(device=dev).manual_seed(3)
    groups, keep = [], []
    for grp in model.optimizer.param_groups:
        p = grp["params"][0]
        grad = torch.randn(p.shape, generator=g, device=dev) * 1e-3
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        keep += [grad, m, v]
        groups.append(dict(name=grp["name"], p=p, R=int(p.shape[0]), L=p.numel() // max(int(p.shape[0]), 1), where=marks.get(grp["name"]),
                           ag=AdamGroup(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(grp["lr"]), 10, None, 0, 0)))
    groups = [x for x in groups if x["p"].numel()]
    n = len(groups)
    arr = (AdamGroup * n)(*[x["ag"] for x in groups])

    def rows_for(vis, only=None):
        rs = []
        for x in (groups if only is None else [only]):
            if x["where"] is None:
                rs.append(AdamRows(None, 0, 1, ROWS_DENSE))
            else:
                off = 0 if x["where"] == "head" else N - x["R"]
                rs.append(AdamRows(vis.data_ptr() + 4 * off, x["R"], x["L"], ROWS_INT32))
        return (AdamRows * len(rs))(*rs)

    def model_bytes(vis):
        per, tot = {}, 0
        for x in groups:
            if vis is None or x["where"] is None:
                b = 28 * x["R"] * x["L"]
            else:
                on = vis[:x["R"]] if x["where"] == "head" else vis[N - x["R"]:]
                b = 28 * x["L"] * int((on > 0).sum()) + 4 * x["R"]
            per[x["name"]] = b
            tot += b
        return tot, per

    lib = _lib.lib()
    stream = _lib.stream_ptr(dev)
    b1, b2, eps = 0.9, 0.999, 1e-15
    variants = {"dense": lambda: lib.adgs_adam_step(arr, n, b1, b2, eps, 0, stream),
                "dense_again": lambda: lib.adgs_adam_step(arr, n, b1, b2, eps, 0, stream)}
    if parent_lib:
        parent = ctypes.CDLL(os.path.abspath(parent_lib))
        parent.adgs_adam_step.restype, parent.adgs_adam_step.argtypes = _lib.SIGNATURES["adgs_adam_step"]
        variants["dense_parent_lib"] = lambda: parent.adgs_adam_step(arr, n, b1, b2, eps, 0, stream)
    tables = {}
    for name, vis in masks.items():
        tables[name] = rows_for(vis)
        variants["masked_" + name] = (lambda t: (lambda: lib.adgs_adam_step_rows(arr, t, n, b1, b2, eps, 0, stream)))(tables[name])

    def timed(fn, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            if fn() < 0:
                raise RuntimeError(_lib.last_error())
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / k

    names = list(variants)
    for nm in names:
        timed(variants[nm], 3)
    per = {nm: [] for nm in names}
    for r in range(rounds):
        order = names[r % len(names):] + names[:r % len(names)]          # every variant meets every position
        for nm in order:
            per[nm].append(timed(variants[nm], reps))
    out = {"gaussians": N, "visible_fraction": {k: round(float((v > 0).float().mean()), 4) for k, v in masks.items()}, "step_us": {}}
    for nm in names:
        q = _quantiles(per[nm])
        tot, _ = model_bytes(None if nm.startswith("dense") else masks[nm[len("masked_"):]])
        q["model_MB"] = round(tot / 1e6, 2)
        q["model_GB_per_s"] = round(tot / (q["us_median"] * 1e-6) / 1e9, 1)
        out["step_us"][nm] = q
    out["dense_spread_us"] = round(max(out["step_us"][k]["us_p90"] for k in names if k.startswith("dense")) - min(out["step_us"][k]["us_p10"] for k in names if k.startswith("dense")), 2)

    # per group, each launched alone: where the row length decides what a skipped row saves
    per_group = {}
    for x in groups:
        one = (AdamGroup * 1)(x["ag"])
        fns = {"dense": lambda: lib.adgs_adam_step(one, 1, b1, b2, eps, 0, stream)}
        if x["where"] is not None:
            for name in ("all_visible", "camera_radii", "runs_0.25", "scattered_0.25", "runs_0.05", "scattered_0.05"):
                t = rows_for(masks[name], only=x)
                keep.append(t)
                fns["masked_" + name] = (lambda t: (lambda: lib.adgs_adam_step_rows(one, t, 1, b1, b2, eps, 0, stream)))(t)
        res = {}
        for nm, fn in fns.items():
            timed(fn, 2)
        for nm, fn in fns.items():
            us = statistics.median(timed(fn, reps) for _ in range(max(3, rounds // 2)))
            mb = model_bytes(None if nm == "dense" else masks[nm[len("masked_"):]])[1][x["name"]]
            res[nm] = dict(us=round(us, 2), model_MB=round(mb / 1e6, 3))
        per_group[x["name"]] = dict(rows=x["R"], row_len=x["L"], masked=x["where"], **res)
    out["per_group"] = per_group
    del model, cams, env_map
    torch.cuda.empty_cache()
    return out


def _mask_the_steps(model):
    """examples/train_iteration.py calls model.add_densification_stats(pkg) and then model.optimizer.step(zero_grad=True): hand the
    radii of the first to the second, without editing the example."""
    seen = {}
    stats, step = model.add_densification_stats, model.optimizer.step

    def add(pkg):
        seen["radii"] = pkg["radii"]
        stats(pkg)

    def masked_step(*a, **k):
        return step(*a, visibility=seen.pop("radii", None), **k)
    model.add_densification_stats, model.optimizer.step = add, masked_step


def iteration_ab(config, rounds, iters, env_res, cameras):
    import torch
    from adgs.optim import mark_visibility_groups
    ti = _train_iteration()
    dev = torch.device("cuda", 0)
    res = {"dense": [], "sparse_adam": []}
    for r in range(rounds):
        for mode in (("dense", "sparse_adam") if r % 2 == 0 else ("sparse_adam", "dense")):
            cfg, model, cams, env_map = ti.build(config, env_res, dev, cameras, False)
            if mode == "sparse_adam":
                mark_visibility_groups(model.optimizer)
                _mask_the_steps(model)
            state, off = {}, ti.StageClock(False)
            for i in range(12):
                ti.iteration(i, model, cams, env_map, off, state)
            torch.cuda.synchronize()
            clock = ti.StageClock(True)
            t0 = time.perf_counter()
            for i in range(12, 12 + iters):
                ti.iteration(i, model, cams, env_map, clock, state)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / iters
            s = clock.summary()
            res[mode].append(dict(ms_per_iteration=round(ms, 4), adam_gaussians_ms=s["adam_gaussians"], backward_ms=s["backward"],
                                  host_adam_gaussians_ms=clock.host_summary().get("adam_gaussians")))
            del model, cams, env_map, state
            torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--iteration-rounds", type=int, default=2)
    ap.add_argument("--env-res", type=int, default=8192)
    ap.add_argument("--cameras", type=int, default=16)
    ap.add_argument("--parent-lib", help="another build of libadgs_hip.so whose dense adgs_adam_step is measured in the same run")
    ap.add_argument("--no-iteration", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU fallback")
    res = {"tool": "sparse_adam_ab", "config": a.config, "rounds": a.rounds, "launches_per_round": a.reps}
    res.update(step_ab(a.config, a.rounds, a.reps, a.parent_lib))
    if a.out:                                    # the first part is kept even if the second is cut short
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")
    if not a.no_iteration:
        res["train_iteration"] = iteration_ab(a.config, a.iteration_rounds, a.iters, a.env_res, a.cameras)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
