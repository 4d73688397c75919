"""Cost of the mesh clean-up (adgs.mesh; include/adgs_mesh.h) against the same definitions composed from torch operations on the device --
what a run has without the kernels -- on the mesh of tools/tsdf_ab.py's fused volume (about 368 k vertices and 565 k faces at the defaults).

    python tools/mesh_ab.py [--height 1280] [--width 1920] [--dims 1024 256 512] [--voxel 0.04] [--views 40] [--reps 9] [--out FILE]

The volume is fused exactly as tools/tsdf_ab.py fuses it (the same views from the same generator), then extracted once.  Timed, HIP events
around each call, the median over `reps` after one warm-up:
  clean-up   connected_components + select + keep_components (remove_small_components), colours carried along
             torch: min-label propagation over the faces with scatter_reduce_(amin) plus pointer jumping until nothing changes, unique for
             the numbering, bincount for the counts, the same select, boolean-mask compaction and a cumsum renumbering
  normals    vertex_normals
             torch: float64 cross products, index_add_ per corner, normalise
The integer results (vertex_component, root, num_faces, num_vertices, the kept faces) are compared for equality, the kept vertices and
colours as bits (the tool exits non-zero when they differ); the normals in value (index_add_ sums in arrival order, so cancelling sums differ).

Byte model (compulsory HBM traffic, every array once): clean-up reads faces three times (link, table, keep) and writes the kept ones,
reads and writes the kept vertex attributes, and passes over three [V] int arrays; normals read faces and vertices and write [V, 3].  The
rate over that model is given as a share of the rate of a device-to-device copy of 1 GiB.  Prints one JSON line; --out also writes it.
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def fused_volume(a, dev):
    """tools/tsdf_ab.py's volume: the same lattice, views and generator sequence, the fused side only."""
    import torch
    from adgs import tsdf
    from tsdf_ab import depth_of_planes
    H, W = a.height, a.width
    nx, ny, nz = a.dims
    f32 = lambda v: float(torch.tensor(float(v), dtype=torch.float32))
    vs = f32(a.voxel)
    origin = (f32(-0.5 * vs * (nx - 1)), f32(1.9 - vs * (ny - 1)), 1.0)
    tan = (f32(W / (2 * 2050.0)), f32(H / (2 * 2050.0)))
    gen = torch.Generator(device=dev).manual_seed(0)
    w = torch.rand(H, W, generator=gen, device=dev)
    w[H - H // 5:] = 0
    vol = tsdf.TSDFVolume(origin, vs, (nx, ny, nz), max_weight=64.0, color=True, device=dev)
    for i in range(a.views):
        yaw = 0.15 * math.sin(0.4 * i)
        R = torch.tensor([[math.cos(yaw), 0.0, -math.sin(yaw)], [0.0, 1.0, 0.0], [math.sin(yaw), 0.0, math.cos(yaw)]], dtype=torch.float64)
        pose = torch.cat([R, (-R @ torch.tensor([0.0, 0.0, 0.25 * i], dtype=torch.float64))[:, None]], dim=1)
        z = depth_of_planes(H, W, tan, pose[:, :3].to(dev), pose[:, 3].to(dev), dev)
        O = torch.where(torch.rand(H, W, generator=gen, device=dev) < 0.1, 0.1 + 0.3 * torch.rand(H, W, generator=gen, device=dev),
                        0.6 + 0.4 * torch.rand(H, W, generator=gen, device=dev))
        D = (O / (z * (1 + 0.003 * torch.randn(H, W, generator=gen, device=dev, dtype=torch.float64)))).float()
        vol.integrate(D, O, (tan, pose), image=torch.rand(3, H, W, generator=gen, device=dev), weight=w)
    return vol


def torch_components(faces, V):
    """(vertex_component, root, num_faces, num_vertices) by min-label propagation; -> also the number of sweeps."""
    import torch
    f = faces.long()
    flat = f.reshape(-1)
    label = torch.arange(V, device=faces.device)
    sweeps = 0
    while True:
        sweeps += 1
        m = label[f].amin(1)
        new = label.scatter_reduce(0, flat, m.repeat_interleave(3), "amin")
        while True:                                             # pointer jumping
            nxt = new[new]
            if torch.equal(nxt, new):
                break
            new = nxt
        if torch.equal(new, label):
            break
        label = new
    root, vc = torch.unique(label, return_inverse=True)
    C = root.shape[0]
    return vc.int(), root.int(), torch.bincount(vc[f[:, 0]], minlength=C).int(), torch.bincount(vc, minlength=C).int(), sweeps


def torch_cleanup(vertices, faces, colors, largest, min_faces):
    import torch
    vc, root, nf, nv, sweeps = torch_components(faces, vertices.shape[0])
    kth = torch.topk(nf, min(largest, nf.shape[0])).values[-1]
    keep = nf >= torch.clamp(kth, min=min_faces)
    kv = keep[vc.long()]
    kf = kv[faces[:, 0].long()]
    new = torch.cumsum(kv, 0) - 1
    return (vc, root, nf, nv), (vertices[kv], new[faces[kf].long()].int(), colors[kv]), sweeps


def torch_normals(vertices, faces):
    import torch
    f = faces.long()
    p = vertices.double()[f]
    n = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=1)
    total = torch.zeros(vertices.shape[0], 3, dtype=torch.float64, device=vertices.device)
    for c in range(3):
        total.index_add_(0, f[:, c], n)
    length = total.norm(dim=1, keepdim=True)
    return torch.where(length > 0, total / length.clamp_min(1e-300), torch.zeros_like(total)).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--dims", type=int, nargs=3, default=[1024, 256, 512])
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--largest", type=int, default=50)
    ap.add_argument("--min-faces", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from adgs import mesh

    if not torch.cuda.is_available():
        raise SystemExit("mesh_ab: no HIP device; nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    vol = fused_volume(a, dev)
    vertices, faces, colors = vol.extract_mesh(min_weight=2.0)
    del vol
    torch.cuda.empty_cache()
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    res = {"tool": "mesh_ab", "dims": list(a.dims), "views": a.views, "vertices": V, "faces": F, "largest": a.largest, "min_faces": a.min_faces}

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e), out

    def median_ms(fn):
        fn()
        runs = [timed(fn) for _ in range(a.reps)]
        ms = [r[0] for r in runs]
        return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4)), runs[-1][1]

    def hip_cleanup():
        comps = mesh.connected_components(faces, V)
        return comps, mesh.keep_components(comps, comps.select(a.largest, a.min_faces), vertices, faces, colors=colors)

    cl = res["cleanup"] = {}
    cl["hip"], (comps, (kv, kf, kc, _)) = median_ms(hip_cleanup)
    cl["torch"], (tcomps, (tv, tf, tc), sweeps) = median_ms(lambda: torch_cleanup(vertices, faces, colors, a.largest, a.min_faces))
    cl["torch_over_hip"] = round(cl["torch"]["ms_median"] / cl["hip"]["ms_median"], 2)
    cl["torch_sweeps"] = sweeps
    cl["components"], cl["kept_components"] = len(comps), int(comps.select(a.largest, a.min_faces).sum())
    cl["kept_vertices"], cl["kept_faces"] = int(kv.shape[0]), int(kf.shape[0])
    cl["integers_equal"] = bool(all(torch.equal(x, y) for x, y in zip((comps.vertex_component, comps.root, comps.num_faces, comps.num_vertices), tcomps))
                                and torch.equal(kf, tf))
    cl["attribute_bits_equal"] = bool(torch.equal(kv.view(torch.int32), tv.view(torch.int32)) and torch.equal(kc.view(torch.int32), tc.view(torch.int32)))
    part = {}
    part["label_and_table"], _ = median_ms(lambda: mesh.connected_components(faces, V))
    part["label_table_and_area"], _ = median_ms(lambda: mesh.connected_components(faces, V, vertices=vertices))
    keep = comps.select(a.largest, a.min_faces)
    part["keep"], _ = median_ms(lambda: mesh.keep_components(comps, keep, vertices, faces, colors=colors))
    cl["hip_parts"] = part

    nm = res["normals"] = {}
    nm["hip"], n = median_ms(lambda: mesh.vertex_normals(vertices, faces, check=False))
    nm["torch"], tn = median_ms(lambda: torch_normals(vertices, faces))
    nm["torch_over_hip"] = round(nm["torch"]["ms_median"] / nm["hip"]["ms_median"], 2)
    nm["max_abs_diff"] = float((n - tn).abs().max())
    nm["share_above_2^-22"] = float(((n - tn).abs().amax(1) > 2.0 ** -22).float().mean())
    nm["bits_equal_from_run_to_run"] = bool(torch.equal(n.view(torch.int32), mesh.vertex_normals(vertices, faces, check=False).view(torch.int32)))

    src = torch.empty(2 ** 28, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    copy_ms = statistics.median(timed(lambda: dst.copy_(src))[0] for _ in range(9))
    copy_rate = 2 * src.numel() * 4 / (copy_ms * 1e-3) / 1e9
    del src, dst
    cl_bytes = 3 * 12 * F + 12 * cl["kept_faces"] + 2 * 24 * cl["kept_vertices"] + 3 * 2 * 4 * V
    nm_bytes = 12 * F + 12 * V + 12 * V
    for d, nbytes in ((cl, cl_bytes), (nm, nm_bytes)):
        rate = nbytes / (d["hip"]["ms_median"] * 1e-3) / 1e9
        d.update(model_bytes=int(nbytes), hip_GBps=round(rate, 1), share_of_copy=round(rate / copy_rate, 4))
    res["copy_GBps"] = round(copy_rate, 1)
    res["results_equal"] = cl["integers_equal"] and cl["attribute_bits_equal"]

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not res["results_equal"]:
        raise SystemExit("mesh_ab: the two sides disagree")


if __name__ == "__main__":
    main()
