#!/usr/bin/env python3
"""One step with the multi-view photometric consistency term (adgs.multiview; PGSR's plane-warped patch NCC) on the HIP path:

    render(camera) under pipe.render_normals -> img_normal, depth, img_opacity
    -> photometric_consistency_loss against ONE neighbouring training image (its grey ground truth and its pose: no second render)
    -> backward to the Gaussians.

    python examples/multiview_step.py [--config T3] [--samples 20000] [--radius 3] [--json]

Synthetic scene; the neighbour is the same camera 0.35 m further along its viewing direction, turned by 0.02 rad.
The two "ground-truth" images are renders of the scene as it stands (a training run has photographs there), so the term measures how far
the rendered depth and normals are from explaining the parallax between them.  What a trainer adds around this: a weight that zeroes
dynamic objects and the sky, a neighbour per camera chosen at load time, and the term's lambda.
"""
import argparse
import json
import math
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def neighbour_of(cam, forward=0.35, yaw=0.02):
    """The make_camera() dict of the camera `forward` metres ahead of `cam` along its viewing direction, turned by `yaw` about its y axis."""
    import torch
    from adgs import synthetic
    c, s = math.cos(yaw), math.sin(yaw)
    M = torch.eye(4)
    M[:3, :3] = torch.tensor([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])
    M[:3, 3] = -M[:3, :3] @ torch.tensor([0.0, 0.0, forward])
    view = (M @ cam["viewmatrix"].t()).t().contiguous()            # world_view_transform is the transposed world-to-camera matrix
    proj = synthetic.projection_matrix(0.01, 100.0, cam["fovx"], cam["fovy"]).transpose(0, 1)
    out = dict(cam)
    out.update(viewmatrix=view, projmatrix=(view @ proj).contiguous(), campos=view.inverse()[3, :3].contiguous())
    return out


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
    with torch.no_grad():                                          # load time: the grey ground truth of both cameras and the pair's pose
        plain = types.SimpleNamespace(inv_depth=True, debug=False)
        cam.gray, nbr.gray = (multiview.gray(render(c, model, None, plain)["render"].clamp(0, 1)).contiguous() for c in (cam, nbr))
        rel = multiview.relative_pose(cam, nbr)                    # reads the two matrices back: once per pair
    # the step
    model.zero_grad()
    pkg = render(cam, model, None, pipe, render_objmask=True)
    static = (pkg["img_semantic"].detach()[0] < 0.5).float()       # zero on the dynamic objects: the term assumes a static surface
    idx = multiview.sample_pixels(static, samples, radius)
    loss = multiview.photometric_consistency_loss(pkg["img_normal"], pkg["depth"], pkg["img_opacity"], cam, cam.gray, nbr.gray, nbr, rel, idx,
                                                  weight=static, radius=radius, inv_depth=pipe.inv_depth)
    loss.backward()
    with torch.no_grad():
        e, valid = multiview.patch_errors(pkg["img_normal"], pkg["depth"], pkg["img_opacity"], cam, cam.gray, nbr.gray, nbr, rel, idx,
                                          weight=static, radius=radius, inv_depth=pipe.inv_depth)
    torch.cuda.synchronize()
    grads = {n: float(getattr(model, n).grad.abs().max()) for n in ("_scene_xyz", "_scene_scaling", "_scene_opacity", "_scene_rotation")
             if getattr(model, n).grad is not None}
    return {"config": config, "image": [cfg["H"], cfg["W"]], "gaussians": int(model.get_pts_num), "samples": int(idx.numel()), "radius": radius,
            "valid_samples": int(valid.sum()), "loss": loss.item(), "median_error_of_valid": float(e[valid].median()) if bool(valid.any()) else None,
            "max_abs_grad": grads}


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
        print("%s, %d Gaussians, %d x %d: multi-view photometric loss %.6f over %d valid of %d samples (radius %d); largest gradients %s" % (
            res["config"], res["gaussians"], res["image"][0], res["image"][1], res["loss"], res["valid_samples"], res["samples"], res["radius"],
            {k: "%.3e" % v for k, v in res["max_abs_grad"].items()}))


if __name__ == "__main__":
    main()
