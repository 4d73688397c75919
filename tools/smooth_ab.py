"""Cost of the mesh adjacency and smoothing (adgs.smooth; include/adgs_smooth.h) against the same definition composed from torch operations on
the device -- what a run has without the kernels -- on the mesh of tools/tsdf_ab.py's fused volume (about 368 k vertices and 565 k faces
at the defaults) and on its simplify_mesh output at 2 voxels.

    python tools/smooth_ab.py [--height 1280] [--width 1920] [--dims 1024 256 512] [--voxel 0.04] [--views 40] [--cell 2] [--iterations 10] [--reps 9] [--out FILE]

The volume is fused exactly as tools/tsdf_ab.py fuses it (tools/mesh_ab.py's fused_volume), then extracted once.  Timed per mesh, wall clock
between two device synchronisations so that the ONE read-back of mesh_adjacency is counted, the median over `reps` after one warm-up:
  adjacency  mesh_adjacency
  steps      smooth_mesh(adjacency=, check=False): `iterations` Taubin iterations over a prebuilt adjacency, no read-back
  whole      smooth_mesh with the defaults: the finiteness check, the adjacency and the steps
  torch      the same definition: int64 undirected edge keys, torch.unique(return_counts) for the edges and their incidence, a sort of the
             directed keys and searchsorted for the rows; per step a float64 gather and index_add_ over the 2 E entries
The adjacency is compared for equality and the positions in value (index_add_ sums in arrival order); the tool exits non-zero when the
adjacency differs or the device's bits change from run to run.

Byte model (compulsory HBM traffic of the steps as they are built, every pass once): adjacency = faces once + six 8-byte keys per face
written + ceil(2 bits(V) / 8) sort passes over 6 F pairs at 32 B (primitives.hip) + the head pass (8 B read, 4 B written per key)
+ the scan at 12 B per key + the emit pass (12 B per key read, 8 B per entry written) + 4 N + 8 V for the rows; a step = the row table
(4 V), the entries (4 N), every vertex's 32-byte state row read once and written once (the gathers of a row's neighbours are counted as
cache hits).  The rate over that model is given as a share of the rate of a device-to-device copy of 1 GiB.  Prints one JSON line; --out
also writes it.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def torch_adjacency(faces, V):
    """-> (starts int32 [V + 1], neighbors int32 [2 E], boundary bool [V], counts)."""
    import torch
    dev = faces.device
    f = faces.long()
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    same = a == b
    key, inc = torch.unique((torch.minimum(a, b) * V + torch.maximum(a, b))[~same], return_counts=True)
    lo, hi = key // V, key % V
    directed = torch.sort(torch.cat([lo * V + hi, hi * V + lo])).values
    src, nb = directed // V, directed % V
    starts = torch.searchsorted(src, torch.arange(V + 1, device=dev))
    boundary = torch.zeros(V, dtype=torch.bool, device=dev)
    single = inc == 1
    boundary[lo[single]] = True
    boundary[hi[single]] = True
    counts = dict(edges=int(key.shape[0]), boundary_edges=int(single.sum()), nonmanifold_edges=int((inc > 2).sum()),
                  degenerate_faces=int(same.reshape(-1, 3).any(1).sum()), isolated_vertices=int((starts[1:] == starts[:-1]).sum()), bad_faces=0)
    return starts.int(), nb.int(), boundary, counts


def torch_smooth(vertices, starts, neighbors, boundary, iterations, lam=0.5, mu=-0.53):
    """Taubin smoothing with the boundary fixed -> vertices' float32."""
    import torch
    V = vertices.shape[0]
    d = (starts[1:] - starts[:-1]).long()
    src = torch.repeat_interleave(torch.arange(V, device=vertices.device), d)
    nb = neighbors.long()
    move = ((d > 0) & ~boundary)[:, None]
    n = d.clamp_min(1).double()[:, None]
    x = vertices.double()
    for s in [lam, mu] * iterations:
        S = torch.zeros_like(x).index_add_(0, src, x[nb])
        x = torch.where(move, x + s * (S / n - x), x)
    return x.float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--dims", type=int, nargs=3, default=[1024, 256, 512])
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--cell", type=float, default=2.0, help="cell of the simplified mesh in voxels")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from adgs import simplify, smooth
    from mesh_ab import fused_volume

    if not torch.cuda.is_available():
        raise SystemExit("smooth_ab: no HIP device; nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    vol = fused_volume(a, dev)
    vertices, faces, colors = vol.extract_mesh(min_weight=2.0)
    voxel = float(vol.voxel_size)
    del vol
    torch.cuda.empty_cache()
    sv, sf, _ = simplify.simplify_mesh(vertices, faces, colors, cell_size=a.cell * voxel)
    res = {"tool": "smooth_ab", "dims": list(a.dims), "views": a.views, "voxel": voxel, "iterations": a.iterations, "meshes": {}}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def median_ms(fn):
        fn()
        runs = [timed(fn) for _ in range(a.reps)]
        ms = [r[0] for r in runs]
        return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4)), runs[-1][1]

    src = torch.empty(2 ** 28, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    copy_ms = statistics.median(timed(lambda: dst.copy_(src))[0] for _ in range(9))
    copy_rate = 2 * src.numel() * 4 / (copy_ms * 1e-3) / 1e9
    del src, dst
    res["copy_GBps"] = round(copy_rate, 1)
    equal = True
    for name, (v, f) in (("extracted", (vertices, faces)), ("simplified_%g" % a.cell, (sv, sf))):
        V, F = int(v.shape[0]), int(f.shape[0])
        d = res["meshes"][name] = {"vertices": V, "faces": F}
        d["adjacency"], adj = median_ms(lambda: smooth.mesh_adjacency(f, V))
        d["steps"], out = median_ms(lambda: smooth.smooth_mesh(v, f, a.iterations, adjacency=adj, check=False))
        d["whole"], whole = median_ms(lambda: smooth.smooth_mesh(v, f, a.iterations))
        d["torch_adjacency"], (ts, tn, tb, tc) = median_ms(lambda: torch_adjacency(f, V))
        d["torch_steps"], tv = median_ms(lambda: torch_smooth(v, ts, tn, tb, a.iterations))
        d["torch_over_hip"] = {"adjacency": round(d["torch_adjacency"]["ms_median"] / d["adjacency"]["ms_median"], 2),
                               "steps": round(d["torch_steps"]["ms_median"] / d["steps"]["ms_median"], 2),
                               "whole": round((d["torch_adjacency"]["ms_median"] + d["torch_steps"]["ms_median"]) / d["whole"]["ms_median"], 2)}
        N = int(adj.neighbors.shape[0])
        d.update(entries=N, counts=adj.counts, max_degree=int(adj.degree().max()) if V else 0)
        d["adjacency_equal"] = bool(torch.equal(ts, adj.starts) and torch.equal(tn, adj.neighbors) and torch.equal(tb, adj.boundary) and tc == adj.counts)
        d["max_abs_position_diff"] = float((tv - out).abs().max()) if V else None
        d["bits_equal_from_run_to_run"] = bool(torch.equal(out.view(torch.int32), whole.view(torch.int32)))
        equal = equal and d["adjacency_equal"] and d["bits_equal_from_run_to_run"]
        passes = -(-2 * max(V, 1).bit_length() // 8)
        adjacency_bytes = 12 * F + 48 * F + 32 * passes * 6 * F + 12 * 6 * F + 12 * 6 * F + 12 * 6 * F + 8 * N + 4 * N + 8 * V
        steps_bytes = 2 * a.iterations * (4 * V + 4 * N + 64 * V)
        for key, nbytes in (("adjacency", adjacency_bytes), ("steps", steps_bytes)):
            rate = nbytes / (d[key]["ms_median"] * 1e-3) / 1e9
            d[key].update(model_bytes=int(nbytes), GBps=round(rate, 1), share_of_copy=round(rate / copy_rate, 4))
    res["results_equal"] = equal

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not equal:
        raise SystemExit("smooth_ab: the two sides disagree")


if __name__ == "__main__":
    main()
