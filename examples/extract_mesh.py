#!/usr/bin/env python3
"""From a model to a mesh (adgs.tsdf) on the HIP path: render every camera, fuse depth and colour of the static regions into a TSDF
volume over the static Gaussians' box, extract the surface by marching tetrahedra, write a PLY.

    for camera:  render(camera)                         one time stamp per render
                 -> vol.integrate(depth, img_opacity, (camera, pose), image=render, weight=static)
    vol.extract_mesh() -> adgs.io.write_mesh_ply

    python examples/extract_mesh.py [--config T3] [--cameras 6] [--resolution 160] [--out mesh.ply] [--json]

Synthetic scene: a cloud of random Gaussians is no surface, so the mesh is a crust around what the cameras saw of it --
the point here is the loop and its cost.  The cameras advance 0.35 m per view along the viewing direction with a small alternating yaw
(examples/multiview_step.py).  What a user changes: the cameras of the data set, the static mask of the data set,
and a voxel size chosen against the depth noise.
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd"), os.path.join(ROOT, "examples")):
    if p not in sys.path:
        sys.path.insert(0, p)

from multiview_step import neighbour_of  # noqa: E402


def run(config="T3", cameras=6, resolution=160, out="mesh.ply", device=None):
    import torch
    from adgs import io, synthetic, tsdf
    from adgs.model import SyntheticGaussianModel
    from gaussian_renderer import render
    device = device or torch.device("cuda", 0)
    cfg = synthetic.CONFIGS[config]
    model = SyntheticGaussianModel.from_scene(synthetic.make_config_scene(config), device=device, seed=0)
    first = synthetic.make_camera(cfg["W"], cfg["H"], cfg["focal"])
    cams = [synthetic.camera_object(first if i == 0 else neighbour_of(first, forward=0.35 * i, yaw=0.03 * (-1) ** i), time=0.5) for i in range(cameras)]
    for c in cams:
        for name in ("world_view_transform", "full_proj_transform", "camera_center"):
            setattr(c, name, getattr(c, name).to(device))
    poses = [tsdf.camera_pose(c) for c in cams]                    # load time: reads each matrix back once
    pipe = types.SimpleNamespace(inv_depth=True, debug=False)
    xyz = model._scene_xyz.detach()                                # the static Gaussians' centres
    voxel = float((xyz.max(0).values - xyz.min(0).values).max()) / resolution
    vol = tsdf.TSDFVolume.around(xyz, voxel, margin=2 * voxel)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for cam, pose in zip(cams, poses):
            pkg = render(cam, model, None, pipe, render_objmask=True)
            static = (pkg["img_semantic"][0] < 0.5).float()        # zero on the dynamic objects: the volume assumes a static surface
            vol.integrate(pkg["depth"], pkg["img_opacity"], (cam, pose), image=pkg["render"].clamp(0, 1).contiguous(), weight=static,
                          inv_depth=pipe.inv_depth)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    vertices, faces, colors = vol.extract_mesh(min_weight=1.0)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    io.write_mesh_ply(out, vertices, faces, colors)
    v2, f2, c2 = io.read_mesh_ply(out)
    assert v2.shape == tuple(vertices.shape) and f2.shape == tuple(faces.shape) and c2.shape == tuple(colors.shape)
    return {"config": config, "image": [cfg["H"], cfg["W"]], "gaussians": int(model.get_pts_num), "cameras": cameras, "dims": list(vol.dims),
            "voxel_size": voxel, "observed_share": float((vol.wsum > 0).float().mean()), "vertices": int(vertices.shape[0]),
            "faces": int(faces.shape[0]), "render_and_integrate_ms": 1e3 * (t1 - t0), "extract_ms": 1e3 * (t2 - t1), "ply": out,
            "ply_bytes": os.path.getsize(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="T3")
    ap.add_argument("--cameras", type=int, default=6)
    ap.add_argument("--resolution", type=int, default=160, help="voxels along the longest side of the static Gaussians' box")
    ap.add_argument("--out", default="mesh.ply")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU fallback")
    res = run(a.config, a.cameras, a.resolution, a.out)
    if a.json:
        print(json.dumps(res))
    else:
        print("%s, %d Gaussians, %d cameras at %d x %d into %d x %d x %d voxels of %.3f (%.1f %% observed): V %d, F %d; render + integrate %.1f ms, "
              "extract %.1f ms; wrote %s (%d bytes)" % (
                  res["config"], res["gaussians"], res["cameras"], res["image"][0], res["image"][1], *res["dims"], res["voxel_size"],
                  100 * res["observed_share"], res["vertices"], res["faces"], res["render_and_integrate_ms"], res["extract_ms"], res["ply"],
                  res["ply_bytes"]))


if __name__ == "__main__":
    main()
