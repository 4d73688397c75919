#!/usr/bin/env python3
"""Geometry of a mesh against a ground truth (adgs.geometry) on the HIP path: sample the mesh's surface, take nearest-neighbour distances
to the ground-truth points and back, print accuracy / completeness / Chamfer distance and precision / recall / F-score.

    python examples/evaluate_mesh.py --mesh a.ply --gt b.ply [--thresholds 0.05 0.1] [--max-dist 0.5] [--samples 1000000] [--seed 0] [--json]
    python examples/evaluate_mesh.py                            the synthetic default

--gt with faces is sampled like the mesh (with seed + 1); --gt without faces is a point set (an aggregated LiDAR sweep).  Both files must
be in ONE frame and cover ONE region: crop them first.  Without --max-dist / --thresholds: max_dist is 2 % of
the ground truth's diagonal and the thresholds are max_dist / 4 and max_dist / 2.

Without arguments the mesh is what examples/extract_mesh.run() extracts from the synthetic scene and the ground truth the static Gaussians'
centres.  A cloud of random Gaussians is no surface, so the numbers say nothing about quality: the point is the loop.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd"), os.path.join(ROOT, "examples")):
    if p not in sys.path:
        sys.path.insert(0, p)


def load(path, device):
    """(vertices, faces) of a PLY on the device; faces is empty for a point cloud."""
    import torch
    from adgs import io
    try:
        v, f = io.read_mesh_ply(path)[:2]
    except ValueError as e:
        if "binary_little_endian" not in str(e):
            raise
        # ascii or big-endian: adgs.io reads the positions of such a file, not its faces -- fine for a point cloud, refused for a mesh
        import numpy as np
        with open(path, "rb") as fh:
            header = fh.read(1 << 16).split(b"end_header")[0].decode("ascii", "replace").split("\n")
        for line in header:
            tok = line.split()
            if len(tok) == 3 and tok[0] == "element" and tok[1] == "face" and int(tok[2]) > 0:
                raise SystemExit("evaluate_mesh: %s has %s faces but is not binary_little_endian, and only such meshes are read; convert it "
                                 "(its vertices alone would be evaluated as a point set)" % (path, tok[2]))
        v, f = io.read_points_ply(path), np.zeros((0, 3), np.int32)
    return torch.from_numpy(v).to(device), torch.from_numpy(f).to(device)


def synthetic_pair(device, config="T3"):
    """The mesh of examples/extract_mesh.run() and the static Gaussians' centres it was fused around."""
    import extract_mesh
    from adgs import synthetic
    from adgs.model import SyntheticGaussianModel
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "mesh.ply")
        extract_mesh.run(config=config, out=out, device=device)
        vertices, faces = load(out, device)
    model = SyntheticGaussianModel.from_scene(synthetic.make_config_scene(config), device=device, seed=0)
    return vertices, faces, model._scene_xyz.detach().float().contiguous()


def run(mesh=None, gt=None, thresholds=None, max_dist=None, samples=1_000_000, seed=0, device=None):
    import torch
    from adgs import geometry
    device = device or torch.device("cuda", 0)
    if mesh is None:
        vertices, faces, gt_points = synthetic_pair(device)
        source = {"mesh": "examples/extract_mesh.run()", "gt": "the static Gaussians' centres"}
    else:
        vertices, faces = load(mesh, device)
        gv, gf = load(gt, device)
        gt_points = geometry.sample_surface(gv, gf, samples, seed + 1)[0] if gf.shape[0] else gv
        source = {"mesh": mesh, "gt": gt, "gt_sampled": bool(gf.shape[0])}
    if faces.shape[0] == 0:
        raise SystemExit("evaluate_mesh: the mesh has no faces")
    finite = gt_points[torch.isfinite(gt_points).all(1)]
    if max_dist is None:
        max_dist = 0.02 * float((finite.max(0).values - finite.min(0).values).norm())
    if not thresholds:
        thresholds = [max_dist / 4, max_dist / 2]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = geometry.evaluate_mesh(vertices, faces, gt_points, thresholds, max_dist, samples=samples, seed=seed)
    torch.cuda.synchronize()
    res["evaluate_ms"] = 1e3 * (time.perf_counter() - t0)
    del res["samples"]
    res.update(source, vertices=int(vertices.shape[0]), faces=int(faces.shape[0]), samples=samples, seed=seed)
    return res


def table(res):
    lines = ["mesh %s (V %d, F %d, %d samples) against %s (%d points), max_dist %.4g" % (
        res["mesh"], res["vertices"], res["faces"], res["num_pred"], res["gt"], res["num_gt"], res["max_dist"]),
        "  accuracy      %.6g   (mesh -> gt; %d samples without a gt point within max_dist)" % (res["accuracy"], res["pred_without_neighbour"]),
        "  completeness  %.6g   (gt -> mesh; %d gt points without a sample within max_dist)" % (res["completeness"], res["gt_without_neighbour"]),
        "  chamfer       %.6g" % res["chamfer"], "  %-12s %10s %10s %10s" % ("threshold", "precision", "recall", "F-score")]
    for t, p, r, f in zip(res["thresholds"], res["precision"], res["recall"], res["fscore"]):
        lines.append("  %-12.4g %10.4f %10.4f %10.4f" % (t, p, r, f))
    lines.append("  evaluated in %.1f ms" % res["evaluate_ms"])
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", help="the reconstructed mesh (binary little-endian PLY with faces)")
    ap.add_argument("--gt", help="the ground truth: a PLY with faces (sampled) or without (a point set)")
    ap.add_argument("--thresholds", type=float, nargs="+", default=None, help="up to 4 distances for precision / recall / F-score, each <= max-dist")
    ap.add_argument("--max-dist", type=float, default=None, help="search radius; farther points count as max-dist")
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if (a.mesh is None) != (a.gt is None):
        ap.error("--mesh and --gt go together")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X: there is no CPU fallback")
    res = run(a.mesh, a.gt, a.thresholds, a.max_dist, a.samples, a.seed)
    print(json.dumps(res) if a.json else table(res))


if __name__ == "__main__":
    main()
