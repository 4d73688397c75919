"""Cost of the geometry evaluation (adgs.geometry; include/adgs_geometry.h) on the mesh of tools/tsdf_ab.py's fused volume (about 368 k
vertices and 565 k faces at the defaults), and against what the tree had before it.

    python tools/geometry_ab.py [--samples 1000000] [--common 100000] [--reps 9] [--dims 1024 256 512] [--voxel 0.04] [--views 40] [--out FILE]

The volume is fused as tools/mesh_ab.py fuses it and extracted once.  pred = `samples` surface samples (seed 0); the pseudo ground truth =
`samples` samples with another seed, each moved by a normal deviate of one voxel per axis.  max_dist = 4 voxels, thresholds 1 and 2 voxels,
cell_size the default 1.001 max_dist (R = 1, 27 cells).  Timed with HIP events around each call, the median over `reps` after one warm-up,
with the minimum and maximum as the spread:
  sample        sample_surface(samples)
  build         PointGrid(gt): box, keys, sort, gather, cell table (synchronises once)
  nearest       grid.nearest(pred): keys, sort of the queries, the search
  both_ways     the two builds and the two searches
  evaluate_mesh the whole call, its one read-back included
  cell_size_sweep  build and nearest with cells of 1.001 max_dist / 1, 2, 4, 8 (R = 1, 2, 4, 8); the results must be equal bit for bit
  knn_points_full_size  adgs.knn.knn_points(K = 1) on the full sets (two runs)
At the COMMON size (`common` points on both sides, the first of each set) the alternatives of the parent commit, each forward only:
  grid          PointGrid + nearest
  knn_points    adgs.knn.knn_points(K = 1): exact, slab sweep along one axis
  cdist         torch.cdist in chunks of 4096 queries + min
knn_points and cdist have no max_dist; the grid's answers are compared with knn_points' where the grid found a neighbour (indices equal
unless the distances tie).

Candidates per query: the records of the 27 cells a query walks, counted with torch from the grid's own table (a check on the byte model, not
timed).  Byte model of nearest(): per query 12 B read + 8 B written + 8 B of sorted order, plus 16 B per candidate record; the rate over that
model is given as a share of the rate of a device-to-device copy of 1 GiB (candidates are re-read by neighbouring lanes from L2, so the share
can exceed what HBM alone would allow).  Prints one JSON line; --out also writes it.

Measured on one MI355X (profiles/geometry/geometry_ab.json; EXPERIMENTS.md): sample 0.158 ms, build 0.317 ms, nearest 1.10 ms (1.08 - 1.12; 1 322
candidates per query, 4.0 of the copy's rate over the byte model), both ways 2.69 ms, evaluate_mesh 2.90 ms, knn_points at the full size 5.74 ms;
at 100 000 points the grid 0.247 ms, knn_points 0.490 ms (1.99 x), cdist 46.4 ms (188 x).  The sweep at the end (cells of max_dist / 1, 2, 4, 8,
results equal bit for bit): 1.10, 1.08, 1.78, 4.61 ms.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def candidates_per_query(grid, queries, max_dist):
    """The mean number of records in the (2 R + 1)^3 cells around each query, from the grid's tables with torch (chunked)."""
    import torch
    from adgs import geometry
    R = geometry.search_radius(max_dist, grid.cell_size)
    C = int(grid.counts[0])
    keys, starts = grid.cell_keys[:C], grid.cell_starts[:C + 1].long()
    size = starts[1:] - starts[:-1]
    origin = torch.tensor(grid.origin, dtype=torch.float64, device=queries.device)
    nx, ny, nz = grid.dims
    total = 0
    for a in range(0, queries.shape[0], 1 << 18):
        c = torch.floor((queries[a:a + (1 << 18)].double() - origin) / grid.cell_size).long()
        for dz in range(-R, R + 1):
            for dy in range(-R, R + 1):
                for dx in range(-R, R + 1):
                    x, y, z = c[:, 0] + dx, c[:, 1] + dy, c[:, 2] + dz
                    ok = (x >= 0) & (x < nx) & (y >= 0) & (y < ny) & (z >= 0) & (z < nz)
                    key = (z * ny + y) * nx + x
                    pos = torch.searchsorted(keys, key.clamp(min=0)).clamp(max=C - 1)
                    hit = ok & (keys[pos] == key)
                    total += int(size[pos][hit].sum())
    return total / max(queries.shape[0], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--dims", type=int, nargs=3, default=[1024, 256, 512])
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--common", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from adgs import geometry, knn
    from mesh_ab import fused_volume

    if not torch.cuda.is_available():
        raise SystemExit("geometry_ab: no HIP device; nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    vol = fused_volume(a, dev)
    vertices, faces, _ = vol.extract_mesh(min_weight=2.0)
    del vol
    torch.cuda.empty_cache()
    n, voxel = a.samples, a.voxel
    md, taus = 4 * voxel, (voxel, 2 * voxel)
    res = {"tool": "geometry_ab", "dims": list(a.dims), "views": a.views, "vertices": int(vertices.shape[0]), "faces": int(faces.shape[0]), "samples": n,
           "max_dist": md, "thresholds": list(taus), "reps": a.reps}

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e), out

    def median_ms(fn, reps=a.reps):
        fn()
        runs = [timed(fn) for _ in range(reps)]
        ms = [r[0] for r in runs]
        return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4)), runs[-1][1]

    res["sample"], (pred, _) = median_ms(lambda: geometry.sample_surface(vertices, faces, n, seed=0))
    gen = torch.Generator(device=dev).manual_seed(1)
    gt = geometry.sample_surface(vertices, faces, n, seed=1)[0] + voxel * torch.randn(n, 3, generator=gen, device=dev)
    cell = 1.001 * md
    res["build"], grid = median_ms(lambda: geometry.PointGrid(gt, cell))
    res["nearest"], (d2, idx) = median_ms(lambda: grid.nearest(pred, md))
    res["both_ways"], _ = median_ms(lambda: (geometry.PointGrid(gt, cell).nearest(pred, md), geometry.PointGrid(pred, cell).nearest(gt, md)))
    res["evaluate_mesh"], metrics = median_ms(lambda: geometry.evaluate_mesh(vertices, faces, gt, taus, md, samples=n, seed=0))
    metrics.pop("samples")
    res["metrics"] = metrics
    res["grid_dims"], res["occupied_cells"] = list(grid.dims), int(grid.counts[0])
    res["found_share"] = float((idx >= 0).float().mean())
    again = grid.nearest(pred, md)
    res["equal_from_run_to_run"] = bool(torch.equal(again[1], idx) and torch.equal(again[0].view(torch.int32), d2.view(torch.int32)))

    cand = candidates_per_query(grid, pred, md)
    src = torch.empty(2 ** 28, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    copy_ms = statistics.median(timed(lambda: dst.copy_(src))[0] for _ in range(9))
    copy_rate = 2 * src.numel() * 4 / (copy_ms * 1e-3) / 1e9
    del src, dst
    model_bytes = n * (12 + 8 + 8) + 16 * cand * n
    rate = model_bytes / (res["nearest"]["ms_median"] * 1e-3) / 1e9
    res["nearest"].update(candidates_per_query=round(cand, 1), model_bytes=int(model_bytes), GBps=round(rate, 1), share_of_copy=round(rate / copy_rate, 4))
    res["copy_GBps"] = round(copy_rate, 1)

    # smaller cells: fewer candidates per query, more rows to search ((2 R + 1)^2 bisections of the cell table)
    sweep = res["cell_size_sweep"] = []
    for div in (1, 2, 4, 8):
        c = 1.001 * md / div
        row = {"cell_size_over_max_dist": round(1.001 / div, 5), "R": geometry.search_radius(md, c)}
        row["build"], gd = median_ms(lambda: geometry.PointGrid(gt, c))
        row["nearest"], (sd2, sidx) = median_ms(lambda: gd.nearest(pred, md))
        row.update(occupied_cells=int(gd.counts[0]), candidates_per_query=round(candidates_per_query(gd, pred[:100_000], md), 1),      # of the first 100 k queries
                   equal_to_default=bool(torch.equal(sidx, idx) and torch.equal(sd2.view(torch.int32), d2.view(torch.int32))))
        res["results_equal_across_cell_sizes"] = res.get("results_equal_across_cell_sizes", True) and row["equal_to_default"]
        sweep.append(row)
        del gd
    res["knn_points_full_size"], _ = median_ms(lambda: knn.knn_points(pred[None], gt[None], K=1), reps=2)

    # the common size
    m = min(a.common, n)
    p, g = pred[:m].contiguous(), gt[:m].contiguous()
    common = res["common"] = {"points_each_side": m}
    common["grid"], (cd2, cidx) = median_ms(lambda: geometry.PointGrid(g, cell).nearest(p, md))
    common["knn_points"], k = median_ms(lambda: knn.knn_points(p[None], g[None], K=1), reps=min(a.reps, 3))

    def cdist_min():
        best, arg = [], []
        for s in range(0, m, 4096):
            d, j = torch.cdist(p[s:s + 4096], g).min(1)
            best.append(d)
            arg.append(j)
        return torch.cat(best), torch.cat(arg)

    common["cdist"], (cd, cj) = median_ms(cdist_min, reps=min(a.reps, 3))
    common["knn_points_over_grid"] = round(common["knn_points"]["ms_median"] / common["grid"]["ms_median"], 2)
    common["cdist_over_grid"] = round(common["cdist"]["ms_median"] / common["grid"]["ms_median"], 2)
    found = cidx >= 0
    kidx, kd2 = k.idx[0, :, 0], k.dists[0, :, 0]
    differ = found & (kidx != cidx.long())
    common["found_share"] = float(found.float().mean())
    common["indices_differ_from_knn_points"] = int(differ.sum())
    common["of_those_with_unequal_distance"] = int((differ & (kd2 != cd2)).sum())
    res["results_equal"] = res["equal_from_run_to_run"] and res["results_equal_across_cell_sizes"] and common["of_those_with_unequal_distance"] == 0

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not res["results_equal"]:
        raise SystemExit("geometry_ab: results differ")


if __name__ == "__main__":
    main()
