"""Cost of the block-sparse TSDF volume (adgs.tsdf_sparse; include/adgs_sparse_tsdf.h) against the dense TSDFVolume on the same views: the
scene of tools/tsdf_ab.py (a road 1.5 m below the cameras and a wall across it, `views` cameras advancing 0.25 m per view, exact depths with
0.3 % noise, 10 % of the pixels below min_opacity, a weight whose bottom fifth is zero), fused with colour.

    python tools/tsdf_sparse_ab.py [--height 1280] [--width 1920] [--dims 1024 256 512] [--voxel 0.04] [--views 40] [--margin 2] [--out FILE]

The sparse volume has the dense one's origin and voxel size, so both hold the same lattice points; it allocates for all views first and
then integrates them all with allocate=False (the order that gives the dense values).  Reported: the blocks, the bytes the sparse volume
holds, the bytes of the dense box; per view (HIP events, median over the views) `allocate`, `integrate(allocate=False)` and their sum, next
to the dense integrate of the same view; `extract_mesh` of each; and whether the two meshes are equal after reordering.  The sparse volume
also keeps what the views see OUTSIDE the dense box, so the two are compared on the box: the stored values as bits on the points of the box
that lie in an allocated block, and the mesh of `to_dense` over the box's blocks (the sparse values, 1 / 0 where no block is) against
the dense volume's mesh.  There is no pass / fail threshold.

Prints one JSON line; --out also writes it to a file.
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

from tsdf_ab import depth_of_planes  # noqa: E402


def same_mesh(a, b):
    """Whether two meshes (vertices, faces, colors) on the device are equal up to the order of vertices and faces: the rows of (position,
    colour) sorted lexicographically must be equal as bits, and the faces, mapped through the two sort permutations and sorted, equal."""
    import torch
    if a[0].shape != b[0].shape or a[1].shape != b[1].shape:
        return False
    if a[0].shape[0] == 0:
        return True

    def canonical(v, f, c):
        rows = torch.cat([v, c], dim=1).view(torch.int32).to(torch.int64)
        order = torch.arange(rows.shape[0], device=rows.device)
        for col in reversed(range(rows.shape[1])):                       # a stable sort per column, last column first: lexicographic
            order = order[torch.sort(rows[order, col], stable=True).indices]
        rank = torch.empty_like(order)
        rank[order] = torch.arange(order.numel(), device=order.device)
        ff = rank[f.long()]
        key = (ff[:, 0] * rows.shape[0] + ff[:, 1]) * rows.shape[0] + ff[:, 2]
        return rows[order], ff[torch.sort(key).indices]

    ra, fa = canonical(*a)
    rb, fb = canonical(*b)
    return bool(torch.equal(ra, rb) and torch.equal(fa, fb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--dims", type=int, nargs=3, default=[1024, 256, 512])
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--margin", type=float, default=2.0)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from adgs import tsdf, tsdf_sparse

    if not torch.cuda.is_available():
        raise SystemExit("tsdf_sparse_ab: no HIP device; nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    H, W = a.height, a.width
    nx, ny, nz = a.dims
    if any(d % 8 for d in a.dims):
        raise SystemExit("tsdf_sparse_ab: dims must be multiples of 8, the block size")
    f32 = lambda v: float(torch.tensor(float(v), dtype=torch.float32))
    vs = f32(a.voxel)
    origin = (f32(-0.5 * vs * (nx - 1)), f32(1.9 - vs * (ny - 1)), 1.0)      # tools/tsdf_ab.py's box
    tan = (f32(W / (2 * 2050.0)), f32(H / (2 * 2050.0)))
    res = {"tool": "tsdf_sparse_ab", "image": [H, W], "dims": [nx, ny, nz], "voxel_size": vs, "views": a.views, "margin": a.margin}

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e), out

    summary = lambda ms: dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))

    gen = torch.Generator(device=dev).manual_seed(0)
    w = torch.rand(H, W, generator=gen, device=dev)
    w[H - H // 5:] = 0
    views = []
    for i in range(a.views):
        yaw = 0.15 * math.sin(0.4 * i)
        R = torch.tensor([[math.cos(yaw), 0.0, -math.sin(yaw)], [0.0, 1.0, 0.0], [math.sin(yaw), 0.0, math.cos(yaw)]], dtype=torch.float64)
        pose = torch.cat([R, (-R @ torch.tensor([0.0, 0.0, 0.25 * i], dtype=torch.float64))[:, None]], dim=1)
        z = depth_of_planes(H, W, tan, pose[:, :3].to(dev), pose[:, 3].to(dev), dev)
        O = torch.where(torch.rand(H, W, generator=gen, device=dev) < 0.1, 0.1 + 0.3 * torch.rand(H, W, generator=gen, device=dev),
                        0.6 + 0.4 * torch.rand(H, W, generator=gen, device=dev))
        D = (O / (z * (1 + 0.003 * torch.randn(H, W, generator=gen, device=dev, dtype=torch.float64)))).float()
        views.append((D, O, torch.rand(3, H, W, generator=gen, device=dev), pose))

    dense = tsdf.TSDFVolume(origin, vs, (nx, ny, nz), max_weight=64.0, color=True, device=dev)
    sparse = tsdf_sparse.SparseTSDFVolume(vs, origin=origin, max_weight=64.0, color=True, margin=a.margin, device=dev)
    D, O, img, pose = views[0]                                          # warm both sides up on scratch state, then start over
    dense.integrate(D, O, (tan, pose), image=img, weight=w)
    sparse.integrate(D, O, (tan, pose), image=img, weight=w)
    sparse.extract_mesh(min_weight=1.0)
    dense.reset()
    sparse.reset()
    torch.cuda.synchronize()

    ms = {"dense_integrate": [], "sparse_allocate": [], "sparse_integrate": []}
    new_blocks = []
    for D, O, img, pose in views:
        t, n = timed(lambda: sparse.allocate(D, O, (tan, pose), weight=w))
        ms["sparse_allocate"].append(t)
        new_blocks.append(n)
    for D, O, img, pose in views:
        ms["sparse_integrate"].append(timed(lambda: sparse.integrate(D, O, (tan, pose), image=img, weight=w, allocate=False))[0])
        ms["dense_integrate"].append(timed(lambda: dense.integrate(D, O, (tan, pose), image=img, weight=w))[0])
    it = res["per_view"] = {k: summary(v) for k, v in ms.items()}
    it["sparse_allocate_plus_integrate_ms_median"] = round(statistics.median(x + y for x, y in zip(ms["sparse_allocate"], ms["sparse_integrate"])), 4)
    it["sparse_allocate_first_view_ms"] = round(ms["sparse_allocate"][0], 4)
    it["sparse_over_dense"] = round(it["sparse_allocate_plus_integrate_ms_median"] / it["dense_integrate"]["ms_median"], 2)
    dense_bytes = 20 * nx * ny * nz
    res["memory"] = dict(blocks=sparse.num_blocks, new_blocks_first_view=new_blocks[0], new_blocks_median_later=int(statistics.median(new_blocks[1:] or [0])),
                         capacity=sparse.capacity, sparse_bytes_held=int(sparse.memory_bytes), sparse_bytes_of_blocks=int(sparse.num_blocks * 512 * 20),
                         dense_box_bytes=dense_bytes, dense_over_sparse_held=round(dense_bytes / max(sparse.memory_bytes, 1), 2),
                         skipped_samples=sparse.skipped_samples)
    lo, hi = (0, 0, 0), (nx // 8, ny // 8, nz // 8)
    b = sparse.block_coords
    inside = ((b >= 0) & (b < torch.tensor(hi, device=dev))).all(1)
    res["memory"]["blocks_inside_the_dense_box"] = int(inside.sum())
    res["memory"]["dense_box_blocks"] = hi[0] * hi[1] * hi[2]

    mw = 2.0
    ex = res["extract_mesh"] = {}
    for name, vol in (("sparse", sparse), ("dense", dense)):
        first, mesh = timed(lambda: vol.extract_mesh(min_weight=mw))
        second, _ = timed(lambda: vol.extract_mesh(min_weight=mw))
        ex[name] = dict(ms_first=round(first, 3), ms_second=round(second, 3), vertices=int(mesh[0].shape[0]), faces=int(mesh[1].shape[0]))
        if name == "dense":
            dense_mesh = mesh
    # the values on the box, and the mesh of the box from the sparse volume's values
    boxed = sparse.to_dense(lo, hi)
    held = torch.zeros_like(dense.tsdf, dtype=torch.bool)                # the points of the box that lie in an allocated block
    bb = b[inside].long()
    held.view(hi[2], 8, hi[1], 8, hi[0], 8).permute(0, 2, 4, 1, 3, 5)[bb[:, 2], bb[:, 1], bb[:, 0]] = True
    same_bits = lambda x, y: bool(torch.equal(x.view(torch.int32)[..., held], y.view(torch.int32)[..., held]))
    res["agreement"] = dict(tsdf_bits_equal_in_the_blocks=same_bits(boxed.tsdf, dense.tsdf), wsum_bits_equal_in_the_blocks=same_bits(boxed.wsum, dense.wsum),
                            color_bits_equal_in_the_blocks=same_bits(boxed.color, dense.color), points_observed_dense=int((dense.wsum > 0).sum()),
                            points_observed_in_the_blocks=int((boxed.wsum > 0).sum()))
    boxed_mesh = boxed.extract_mesh(min_weight=mw)
    res["agreement"]["box_mesh_vertices"] = int(boxed_mesh[0].shape[0])
    res["agreement"]["box_mesh_faces"] = int(boxed_mesh[1].shape[0])
    res["agreement"]["meshes_equal_after_reordering"] = same_mesh(boxed_mesh, dense_mesh)
    res["sparse_slower_per_view"] = it["sparse_allocate_plus_integrate_ms_median"] > it["dense_integrate"]["ms_median"]

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
