"""Cost of the 3D smoothing filter of Mip-Splatting (adgs.filter3d; include/adgs_filter3d.h) at training size.

    python tools/filter3d_ab.py [--config C3] [--stamps 16] [--cameras-per-stamp 3] [--rounds 9] [--inner 5] [--out profiles/filter3d/filter3d_ab.json]

HIP-event medians (rounds of `inner` back-to-back calls, ms per call):
(a) model.compute_3d_filter over stamps x cameras-per-stamp cameras against a torch composition of the published trainer's
    per-camera loop (element-wise torch kernels over all Gaussians per camera, written here from the definition in the header);
    the two filters are compared (largest relative difference over the rows both call seen);
(b) the training frame (render + backward of the image sum) with pipe.filter_3d off and on, for a raw_scene model and for a plain
    one -- "off" is the frame without this feature; on the raw-scene path "on" also pays the scene rows' deformation pass that the
    raw-scene path otherwise skips, which is what applying the filter inside the preprocess kernels would save.

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


def timed(fn, rounds, inner):
    import torch
    for _ in range(2):
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


def torch_filter(model, cams, recs_by_cam):
    """The per-camera loop with torch: every camera transforms all positions of its time stamp and keeps the largest fx / z it sees."""
    import torch
    rate = None
    xyz_at = {}
    for cam, c in zip(cams, recs_by_cam):
        if cam.time not in xyz_at:
            xyz_at[cam.time] = model.get_deformed_xyz(cam.time)
        p = xyz_at[cam.time]
        R, t = c[:9].reshape(3, 3), c[9:12]
        q = p @ R.t() + t
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        zc = torch.clamp(z, min=0.001)
        u, v = x / zc * c[12] + c[14] / 2, y / zc * c[13] + c[15] / 2
        seen = (z > 0.2) & (u >= -0.15 * c[14]) & (u <= 1.15 * c[14]) & (v >= -0.15 * c[15]) & (v <= 1.15 * c[15])
        r = torch.where(seen, c[12] / z, torch.zeros_like(z))
        rate = r if rate is None else torch.maximum(rate, r)
    seen = rate > 0
    if not bool(seen.any()):
        return torch.zeros_like(rate)[:, None]
    return torch.where(seen, 0.2 ** 0.5 / rate.clamp(min=1e-30), 0.2 ** 0.5 / rate[seen].min())[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--stamps", type=int, default=16)
    ap.add_argument("--cameras-per-stamp", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    import bench
    from adgs import filter3d, synthetic
    from adgs.model import SyntheticGaussianModel
    from gaussian_renderer import render

    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = synthetic.CONFIGS[a.config]
    sc = synthetic.make_config_scene(a.config)
    pool = bench.camera_pool(cfg, a.stamps * a.cameras_per_stamp)
    cams = []
    for k, (cam, _t) in enumerate(pool):
        c = synthetic.camera_object(cam, time=(k // a.cameras_per_stamp + 0.5) / a.stamps)
        for name in ("world_view_transform", "full_proj_transform", "camera_center"):
            setattr(c, name, getattr(c, name).to(dev))
        cams.append(c)
    res = {"tool": "filter3d_ab", "config": a.config, "gaussians": int(sc["P"]), "image": [cfg["H"], cfg["W"]], "time_stamps": a.stamps,
           "cameras": len(cams), "rounds": a.rounds, "calls_per_round": a.inner}

    model = SyntheticGaussianModel.from_scene(sc, device=dev, seed=0)
    recs = filter3d.camera_records(cams, dev)
    with torch.no_grad():
        hip = timed(lambda: model.compute_3d_filter(cams), a.rounds, a.inner)
        tor = timed(lambda: torch_filter(model, cams, recs), max(3, a.rounds // 3), 1)
        f_hip, f_torch = model.compute_3d_filter(cams), torch_filter(model, cams, recs)
    both = (f_hip > 0) & (f_torch > 0)
    res["compute_3d_filter"] = {"hip": hip, "torch_per_camera_loop": tor, "torch_over_hip": round(tor["ms_median"] / hip["ms_median"], 1),
                                "rows_with_a_filter": int((f_hip > 0).sum()),
                                "max_relative_difference": float(((f_hip - f_torch).abs() / f_torch.clamp(min=1e-30))[both].max()) if bool(both.any()) else None,
                                "note": "hip: camera records, one deformation pass and one accumulate launch per time stamp for the object rows, one launch over "
                                        "all cameras for the scene rows, finalize; rows on a seen-gate may differ between the two float32 evaluations"}

    g_img = (torch.randn(3, cfg["H"], cfg["W"], generator=torch.Generator().manual_seed(1)) / (cfg["H"] * cfg["W"])).to(dev)
    frames = res["training_frame"] = {}
    for name, raw_scene in (("raw_scene", True), ("plain", False)):
        m = SyntheticGaussianModel.from_scene(sc, device=dev, seed=0)
        m.raw_sh, m.raw_scene = True, raw_scene
        m.compute_3d_filter(cams)
        entry = frames[name] = {}
        for flag in (False, True):
            pipe = types.SimpleNamespace(inv_depth=True, debug=False)
            if flag:
                pipe.filter_3d = True

            def frame():
                m.zero_grad()
                out = render(cams[0], m, None, pipe)
                out["render"].backward(g_img)
            entry["filter_3d_on" if flag else "filter_3d_off"] = timed(frame, a.rounds, a.inner)
        entry["on_minus_off_ms"] = round(entry["filter_3d_on"]["ms_median"] - entry["filter_3d_off"]["ms_median"], 5)

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
