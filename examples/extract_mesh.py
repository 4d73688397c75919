#!/usr/bin/env python3
"""From a model to a mesh (adgs.tsdf) on the HIP path: render every camera, fuse depth and colour of the static regions into a TSDF
volume over the static Gaussians' box, extract the surface by marching tetrahedra, write a PLY.

    for camera:  render(camera)                         one time stamp per render
                 -> vol.integrate(depth, img_opacity, (camera, pose), image=render, weight=static)
    vol.extract_mesh() [-> adgs.mesh.remove_small_components] [-> adgs.zbuffer.visible_faces -> adgs.mesh.keep_faces]
        [-> adgs.smooth.smooth_mesh] [-> adgs.simplify.simplify_mesh] [-> adgs.mesh.vertex_normals]
        -> adgs.io.write_mesh_ply

    python examples/extract_mesh.py [--config T3] [--cameras 6] [--resolution 160] [--out mesh.ply] [--json] [--sparse [--margin 2]]
                                    [--keep-largest K] [--min-faces m] [--cull-unseen [MIN_VIEWS]]
                                    [--smooth ITER [--smooth-method taubin|laplacian] [--free-boundary]]
                                    [--simplify CELL [--placement quadric|average]] [--normals]

--sparse fuses into a block-sparse volume (adgs.tsdf_sparse) instead of the dense box: no box is chosen, only the 8 x 8 x 8 blocks near the
rendered surfaces are stored.  It allocates for ALL views first and then integrates them all with allocate=False -- the order that gives
the dense volume's values (a block allocated by a later view would otherwise miss the free space the earlier views saw) -- so the renders
are kept between the two loops.  Everything downstream is the same; --json then also reports the blocks and the bytes held.

--keep-largest / --min-faces (off by default; either one turns the clean-up on, the other then takes its 2DGS default of 50) drop the small
connected components of the mesh, --cull-unseen [MIN_VIEWS] (off by default; 1 when given without a number) renders the cleaned mesh again
from the cameras that were fused (adgs.zbuffer) and keeps the faces that won a pixel in at least MIN_VIEWS of them -- the closed back of
the truncation band and the far side of half-observed objects go --, --smooth ITER (off by default) smooths the vertices after the
clean-up and the culling and before the simplification and the normals (adgs.smooth: Taubin by default, which does not shrink the mesh;
boundary vertices stay where they are unless --free-boundary), --simplify CELL (in voxels of the volume; off by default) clusters the vertices on a lattice of that cell
between the clean-up and the normals (adgs.simplify; below one voxel it only welds), --normals writes area-weighted vertex normals into
the PLY (adgs.mesh).

Synthetic scene: a cloud of random Gaussians is no surface, so the mesh is a crust around what the cameras saw of it --
the point here is the loop and its cost.  The cameras advance 0.35 m per view along the viewing direction with a small alternating yaw
(examples/multiview_step.py).  What a user changes: the cameras of the data set, the static mask of the data set,
and a voxel size chosen against the depth noise.
"""
import argparse
import json
import math
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd"), os.path.join(ROOT, "examples")):
    if p not in sys.path:
        sys.path.insert(0, p)

from multiview_step import neighbour_of  # noqa: E402


def run(config="T3", cameras=6, resolution=160, out="mesh.ply", device=None, keep_largest=None, min_faces=None, normals=False,
        simplify=None, placement="quadric", sparse=False, margin=2.0, cull_unseen=None, smooth=None, smooth_method="taubin", free_boundary=False):
    import torch
    from adgs import io, mesh, synthetic, tsdf, tsdf_sparse, zbuffer
    from adgs import simplify as simplification
    from adgs import smooth as smoothing
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
    extent = (xyz.max(0).values - xyz.min(0).values + 4 * voxel).tolist()      # the box TSDFVolume.around would take, for comparison
    box_dims = [int(math.ceil(e / voxel)) + 1 for e in extent]
    vol = tsdf_sparse.SparseTSDFVolume(voxel, margin=margin, device=device) if sparse else tsdf.TSDFVolume.around(xyz, voxel, margin=2 * voxel)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        kept = []
        for cam, pose in zip(cams, poses):
            pkg = render(cam, model, None, pipe, render_objmask=True)
            static = (pkg["img_semantic"][0] < 0.5).float()        # zero on the dynamic objects: the volume assumes a static surface
            if sparse:                                             # first every view's blocks ...
                vol.allocate(pkg["depth"], pkg["img_opacity"], (cam, pose), weight=static, inv_depth=pipe.inv_depth)
                kept.append((pkg["depth"], pkg["img_opacity"], pkg["render"].clamp(0, 1).contiguous(), static))
                continue
            vol.integrate(pkg["depth"], pkg["img_opacity"], (cam, pose), image=pkg["render"].clamp(0, 1).contiguous(), weight=static,
                          inv_depth=pipe.inv_depth)
        for (depth, opacity, image, static), cam, pose in zip(kept, cams, poses):      # ... then every view into all of them
            vol.integrate(depth, opacity, (cam, pose), image=image, weight=static, inv_depth=pipe.inv_depth, allocate=False)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    vertices, faces, colors = vol.extract_mesh(min_weight=1.0)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    extracted = {"vertices": int(vertices.shape[0]), "faces": int(faces.shape[0])}
    cleanup = None
    if keep_largest is not None or min_faces is not None:
        K, m = 50 if keep_largest is None else keep_largest, 50 if min_faces is None else min_faces
        comps = mesh.connected_components(faces, vertices.shape[0])
        keep = comps.select(largest=K, min_faces=m)
        vertices, faces, colors, _ = mesh.keep_components(comps, keep, vertices, faces, colors=colors)
        cleanup = {"largest": K, "min_faces": m, "components": len(comps), "kept_components": int(keep.sum())}
    culled = None
    if cull_unseen is not None:                                    # after the clean-up, before the simplification
        before = (int(vertices.shape[0]), int(faces.shape[0]))
        vis = zbuffer.visible_faces(vertices, faces, list(zip(cams, poses)), (cfg["H"], cfg["W"]))
        vertices, faces, colors, _ = mesh.keep_faces(vis.seen(min_views=cull_unseen), vertices, faces, colors=colors)
        culled = {"min_views": cull_unseen, "views": vis.num_views, "vertices_before": before[0], "faces_before": before[1],
                  "vertices_after": int(vertices.shape[0]), "faces_after": int(faces.shape[0])}
    smoothed = None
    if smooth is not None:                                         # before the simplification and the normals: both read the faces' planes
        adj = smoothing.mesh_adjacency(faces, int(vertices.shape[0]))
        vertices = smoothing.smooth_mesh(vertices, faces, smooth, method=smooth_method, boundary="free" if free_boundary else "fixed", adjacency=adj)
        smoothed = dict(adj.counts, iterations=smooth, method=smooth_method, boundary="free" if free_boundary else "fixed")
    simplified = None
    if simplify is not None:
        before = (int(vertices.shape[0]), int(faces.shape[0]))
        vertices, faces, colors = simplification.simplify_mesh(vertices, faces, colors, cell_size=simplify * voxel, placement=placement)
        simplified = {"cell_voxels": simplify, "cell_size": simplify * voxel, "placement": placement, "vertices_before": before[0], "faces_before": before[1]}
    vnormals = mesh.vertex_normals(vertices, faces) if normals else None
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    io.write_mesh_ply(out, vertices, faces, colors, normals=vnormals)
    v2, f2, c2, n2 = io.read_mesh_ply(out, normals=True)
    assert v2.shape == tuple(vertices.shape) and f2.shape == tuple(faces.shape) and c2.shape == tuple(colors.shape)
    assert (n2 is None) == (vnormals is None) and (n2 is None or n2.shape == v2.shape)
    return {"extracted": extracted, "cleanup": cleanup, "cull_unseen": culled, "smooth": smoothed, "simplify": simplified, "normals": bool(normals), "cleanup_and_normals_ms": 1e3 * (t3 - t2),"config": config, "image": [cfg["H"], cfg["W"]], "gaussians": int(model.get_pts_num), "cameras": cameras,
            "dims": box_dims if sparse else list(vol.dims), "voxel_size": voxel, "observed_share": float((vol.wsum > 0).float().mean()),
            "sparse": {"blocks": vol.num_blocks, "bytes": int(vol.memory_bytes), "block_bytes": vol.num_blocks * 512 * 20, "margin": margin,
                       "dense_box_bytes": 20 * box_dims[0] * box_dims[1] * box_dims[2], "skipped_samples": vol.skipped_samples} if sparse else None, "vertices": int(vertices.shape[0]),
            "faces": int(faces.shape[0]), "render_and_integrate_ms": 1e3 * (t1 - t0), "extract_ms": 1e3 * (t2 - t1), "ply": out,
            "ply_bytes": os.path.getsize(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="T3")
    ap.add_argument("--cameras", type=int, default=6)
    ap.add_argument("--resolution", type=int, default=160, help="voxels along the longest side of the static Gaussians' box")
    ap.add_argument("--out", default="mesh.ply")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--keep-largest", type=int, default=None, metavar="K", help="keep the components with at least as many faces as the K-th largest")
    ap.add_argument("--min-faces", type=int, default=None, metavar="m", help="and with at least m faces")
    ap.add_argument("--cull-unseen", type=int, nargs="?", const=1, default=None, metavar="MIN_VIEWS",
                    help="keep the faces that win a pixel in at least MIN_VIEWS (default 1) of the fused cameras (adgs.zbuffer)")
    ap.add_argument("--smooth", type=int, default=None, metavar="ITER", help="smooth the vertices with ITER iterations (adgs.smooth)")
    ap.add_argument("--smooth-method", choices=("taubin", "laplacian"), default="taubin", help="taubin does not shrink the mesh, laplacian does")
    ap.add_argument("--free-boundary", action="store_true", help="with --smooth: let the boundary vertices move too")
    ap.add_argument("--simplify", type=float, default=None, metavar="CELL", help="cluster the vertices on a lattice of CELL voxels (adgs.simplify)")
    ap.add_argument("--placement", choices=("quadric", "average"), default="quadric", help="where the vertex of a cluster goes")
    ap.add_argument("--normals", action="store_true", help="write area-weighted vertex normals")
    ap.add_argument("--sparse", action="store_true", help="fuse into a block-sparse volume (adgs.tsdf_sparse): allocate for all views, then integrate them all")
    ap.add_argument("--margin", type=float, default=2.0, metavar="VOXELS", help="with --sparse: how far around a ray sample blocks are allocated (0 .. 4)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU fallback")
    res = run(a.config, a.cameras, a.resolution, a.out, keep_largest=a.keep_largest, min_faces=a.min_faces, normals=a.normals, simplify=a.simplify,
              placement=a.placement, sparse=a.sparse, margin=a.margin, cull_unseen=a.cull_unseen, smooth=a.smooth, smooth_method=a.smooth_method,
              free_boundary=a.free_boundary)
    if a.json:
        print(json.dumps(res))
    else:
        print("%s, %d Gaussians, %d cameras at %d x %d into %d x %d x %d voxels of %.3f (%.1f %% observed): V %d, F %d; render + integrate %.1f ms, "
              "extract %.1f ms; wrote %s (%d bytes)" % (
                  res["config"], res["gaussians"], res["cameras"], res["image"][0], res["image"][1], *res["dims"], res["voxel_size"],
                  100 * res["observed_share"], res["vertices"], res["faces"], res["render_and_integrate_ms"], res["extract_ms"], res["ply"],
                  res["ply_bytes"]))
        if res["sparse"]:
            b = res["sparse"]
            print("block-sparse volume: %d blocks, %d bytes held (%d in blocks) against %d for the dense box above; the observed share is of the blocks' points"
                  % (b["blocks"], b["bytes"], b["block_bytes"], b["dense_box_bytes"]))
        if res["cull_unseen"]:
            u = res["cull_unseen"]
            print("culled the faces seen in fewer than %d of %d views: F %d -> %d, V %d -> %d" % (
                u["min_views"], u["views"], u["faces_before"], u["faces_after"], u["vertices_before"], u["vertices_after"]))
        if res["smooth"]:
            m = res["smooth"]
            print("smoothed with %d %s iterations, boundary %s: %d edges, %d boundary, %d non-manifold; %d degenerate faces, %d isolated vertices" % (
                m["iterations"], m["method"], m["boundary"], m["edges"], m["boundary_edges"], m["nonmanifold_edges"], m["degenerate_faces"],
                m["isolated_vertices"]))
        s = res["simplify"]
        if res["cleanup"] or res["normals"] or s:
            c = res["cleanup"]
            print("extracted V %d, F %d%s%s -> V %d, F %d%s; clean-up, simplification and normals %.1f ms" % (
                res["extracted"]["vertices"], res["extracted"]["faces"],
                "; %d components, kept %d (largest %d, min_faces %d)" % (c["components"], c["kept_components"], c["largest"], c["min_faces"]) if c else "",
                "; V %d, F %d simplified at %.2f voxels (%s)" % (s["vertices_before"], s["faces_before"], s["cell_voxels"], s["placement"]) if s else "",
                res["vertices"], res["faces"], ", with vertex normals" if res["normals"] else "", res["cleanup_and_normals_ms"]))


if __name__ == "__main__":
    main()
