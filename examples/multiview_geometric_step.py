#!/usr/bin/env python3
"""One step with both multi-view terms (adgs.multiview) on the HIP path: the geometric consistency term (PGSR's depth reprojection error)
between TWO renders, and the photometric term weighted and sampled by what the geometric one found consistent.

    render(camera), render(neighbour)                 the same time stamp, both with gradients
    -> geometric_consistency_loss(depth, img_opacity of both)          gradients into both renders
    -> reprojection_errors -> weight = static * geo_weight             exp(-err) where the round trip closes, 0 where it does not
    -> sample_pixels(weight) -> photometric_consistency_loss(..., weight=weight)
    -> one backward to the Gaussians.

    python examples/multiview_geometric_step.py [--config T3] [--samples 20000] [--radius 3] [--json]

Synthetic scene; the neighbour is the same camera 0.35 m further along its viewing direction, turned by 0.02 rad
(examples/multiview_step.py).  What a trainer adds around this: the neighbour of every camera chosen once with
multiview.nearest_cameras, the two lambdas, and a start iteration after the geometry has settled.
"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd"), os.path.join(ROOT, "examples")):
    if p not in sys.path:
        sys.path.insert(0, p)

from multiview_step import neighbour_of  # noqa: E402


def run(config="T3", samples=20000, radius=3, device=None):
    import torch
    from adgs import multiview, synthetic
    from adgs.model import SyntheticGaussianModel
    from gaussian_renderer import render
    device = device or torch.device("cuda", 0)
    cfg = synthetic.CONFIGS[config]
    model = SyntheticGaussianModel.from_scene(synthetic.make_config_scene(config), device=device, seed=0)
    ref_cam = synthetic.make_camera(cfg["W"], cfg["H"], cfg["focal"])
    cams = [synthetic.camera_object(c, time=0.5) for c in (ref_cam, neighbour_of(ref_cam))]
    for c in cams:
        for name in ("world_view_transform", "full_proj_transform", "camera_center"):
            setattr(c, name, getattr(c, name).to(device))
    cam, nbr = cams
    pipe = types.SimpleNamespace(inv_depth=True, debug=False, render_normals=True)
    with torch.no_grad():                                          # load time: the grey ground truth, each camera's neighbour, the pair's pose
        plain = types.SimpleNamespace(inv_depth=True, debug=False)
        cam.gray, nbr.gray = (multiview.gray(render(c, model, None, plain)["render"].clamp(0, 1)).contiguous() for c in (cam, nbr))
        assert multiview.nearest_cameras(cams) == [[1], [0]]
        rel = multiview.relative_pose(cam, nbr)                    # reads the two matrices back: once per pair
    # the step
    model.zero_grad()
    pkg = render(cam, model, None, pipe, render_objmask=True)
    pkg_n = render(nbr, model, None, plain)                        # the second render: its depth takes gradients too
    static = (pkg["img_semantic"].detach()[0] < 0.5).float()       # zero on the dynamic objects: both terms assume a static surface
    geo_args = (pkg["depth"], pkg["img_opacity"], cam, pkg_n["depth"], pkg_n["img_opacity"], nbr, rel)
    loss_geo = multiview.geometric_consistency_loss(*geo_args, weight=static, inv_depth=pipe.inv_depth)
    err, geo_weight = multiview.reprojection_errors(*geo_args, weight=static, inv_depth=pipe.inv_depth)
    weight = static * geo_weight
    idx = multiview.sample_pixels(weight, samples, radius)
    loss_ncc = multiview.photometric_consistency_loss(pkg["img_normal"], pkg["depth"], pkg["img_opacity"], cam, cam.gray, nbr.gray, nbr, rel, idx,
                                                      weight=weight, radius=radius, inv_depth=pipe.inv_depth)
    (loss_geo + loss_ncc).backward()
    torch.cuda.synchronize()
    grads = {n: float(getattr(model, n).grad.abs().max()) for n in ("_scene_xyz", "_scene_scaling", "_scene_opacity", "_scene_rotation")
             if getattr(model, n).grad is not None}
    valid = geo_weight > 0
    return {"config": config, "image": [cfg["H"], cfg["W"]], "gaussians": int(model.get_pts_num), "geometric_loss": loss_geo.item(),
            "valid_share": float(valid.float().mean()), "median_error_of_valid_px": float(err[valid].median()) if bool(valid.any()) else None,
            "samples": int(idx.numel()), "radius": radius, "photometric_loss": loss_ncc.item(), "max_abs_grad": grads}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="T3")
    ap.add_argument("--samples", type=int, default=20000)
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU fallback")
    res = run(a.config, a.samples, a.radius)
    if a.json:
        print(json.dumps(res))
    else:
        print("%s, %d Gaussians, %d x %d: geometric loss %.6f, %.1f %% of the pixels valid (median error %s px); photometric loss %.6f over %d samples "
              "(radius %d); largest gradients %s" % (
                  res["config"], res["gaussians"], res["image"][0], res["image"][1], res["geometric_loss"], 100 * res["valid_share"],
                  "%.4f" % res["median_error_of_valid_px"] if res["median_error_of_valid_px"] is not None else "-", res["photometric_loss"],
                  res["samples"], res["radius"], {k: "%.3e" % v for k, v in res["max_abs_grad"].items()}))


if __name__ == "__main__":
    main()
