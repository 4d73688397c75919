"""Cost of the mesh simplification (adgs.simplify; include/adgs_simplify.h) against the same definition composed from torch operations on
the device -- what a run has without the kernels -- on the mesh of tools/tsdf_ab.py's fused volume (about 368 k vertices and 565 k faces
at the defaults), at cells of 2, 4 and 8 voxels.

    python tools/simplify_ab.py [--height 1280] [--width 1920] [--dims 1024 256 512] [--voxel 0.04] [--views 40] [--cells 2 4 8] [--reps 9] [--out FILE]

The volume is fused exactly as tools/tsdf_ab.py fuses it (tools/mesh_ab.py's fused_volume), then extracted once.  Timed per cell, wall clock
between two device synchronisations so that the ONE read-back of cluster_vertices is counted, the median over `reps` after one warm-up:
  cluster    cluster_vertices
  place      place_vertices, "quadric" and "average", colours carried along
  whole      simplify_mesh(placement="quadric")
  torch      the same definition: int64 cell keys, torch.unique for the clusters, scatter_reduce(amin) for the roots, a packed rotated
             triple and torch.unique for the duplicates, float64 index_add_ for the member and quadric sums, batched torch.linalg.solve
The faces are compared for equality and the positions in value (index_add_ sums in arrival order); the tool exits non-zero when the faces
differ.

Byte model (compulsory HBM traffic of the steps as they are built, every pass once): the radix sort moves 32 B per pair and 8-bit pass with
64-bit keys and 20 B with 32-bit keys (primitives.hip); cluster = 8 passes over V pairs + ceil(bits(V) / 8) 32-bit passes and
ceil((32 + bits(V)) / 8) 64-bit passes over F pairs + five reads of faces + four [V] scans at 12 B + the outputs; place = ceil(bits(V2) / 8)
32-bit passes over 3 F pairs + faces and vertices once + the member and corner rows.  The rate over that model is given as a share of the
rate of a device-to-device copy of 1 GiB.  Prints one JSON line; --out also writes it.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def float32(x):
    """x rounded to float32, as the library receives it."""
    return ctypes.c_float(x).value


def torch_simplify(vertices, faces, colors, cell, lam=1e-3):
    """The definition with the default origin, quadric placement -> (vertices2, faces2, colors2)."""
    import torch
    V, dev = vertices.shape[0], vertices.device
    v = vertices.double()
    c = torch.floor(v / cell).long()
    key = ((c[:, 0] + 2 ** 20) << 42) | ((c[:, 1] + 2 ** 20) << 21) | (c[:, 2] + 2 ** 20)
    _, kc = torch.unique(key, return_inverse=True)
    K = int(kc.max()) + 1
    ids = torch.arange(V, device=dev)
    kroot = torch.full((K,), V, device=dev).scatter_reduce(0, kc, ids, "amin")
    f = faces.long()
    fr = kroot[kc[f]]                                           # the roots of the corner clusters
    live = (fr[:, 0] != fr[:, 1]) & (fr[:, 1] != fr[:, 2]) & (fr[:, 0] != fr[:, 2])
    k = fr.argmin(1)
    rot = torch.gather(fr, 1, (k[:, None] + torch.arange(3, device=dev)[None]) % 3)
    assert V < 2 ** 21
    packed = (rot[:, 0] << 42) | (rot[:, 1] << 21) | rot[:, 2]
    packed = torch.where(live, packed, torch.full_like(packed, -1))
    _, tri = torch.unique(packed, return_inverse=True)
    fid = torch.arange(f.shape[0], device=dev)
    first = torch.full((int(tri.max()) + 1,), f.shape[0], device=dev).scatter_reduce(0, tri, fid, "amin")
    keep = live & (first[tri] == fid)
    used = torch.zeros(V, dtype=torch.bool, device=dev)
    used[fr[keep].reshape(-1)] = True                           # over the vertices: the used roots
    number = torch.cumsum(used, 0) - 1
    vc = torch.where(used[kroot[kc]], number[kroot[kc]], torch.full_like(kc, -1))
    V2 = int(used.sum())
    inside = vc >= 0
    n = torch.zeros(V2, dtype=torch.float64, device=dev).index_add_(0, vc[inside], torch.ones(int(inside.sum()), dtype=torch.float64, device=dev))
    cbar = torch.zeros(V2, 3, dtype=torch.float64, device=dev).index_add_(0, vc[inside], v[inside]) / n[:, None]
    col = (torch.zeros(V2, 3, dtype=torch.float64, device=dev).index_add_(0, vc[inside], colors.double()[inside]) / n[:, None]).float()
    p = v[f]
    kx = torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=1)
    L = kx.norm(dim=1)
    ok = L > 0
    nrm = kx / L.clamp_min(1e-300)[:, None]
    A = torch.zeros(V2, 3, 3, dtype=torch.float64, device=dev)
    g = torch.zeros(V2, 3, dtype=torch.float64, device=dev)
    t = torch.zeros(V2, dtype=torch.float64, device=dev)
    for corner in range(3):
        cc = vc[f[:, corner]]
        m = ok & (cc >= 0)
        cc, nn, w = cc[m], nrm[m], 0.5 * L[m]
        e = (nn * (p[m, corner] - cbar[cc])).sum(1)
        A.index_add_(0, cc, w[:, None, None] * nn[:, :, None] * nn[:, None, :])
        g.index_add_(0, cc, (w * e)[:, None] * nn)
        t.index_add_(0, cc, w)
    M = A + (lam * t)[:, None, None] * torch.eye(3, dtype=torch.float64, device=dev)[None] + (t <= 0)[:, None, None] * torch.eye(3, dtype=torch.float64, device=dev)[None]
    delta = torch.linalg.solve(M, g[:, :, None])[:, :, 0]
    cells = torch.floor(v[torch.nonzero(used)[:, 0]] / cell)
    lo, hi = cells * cell, (cells + 1.0) * cell
    delta = torch.minimum(torch.maximum(delta, (lo - cbar).clamp_max(0.0)), (hi - cbar).clamp_min(0.0))
    return (cbar + delta).float(), vc[f[keep]].int(), col


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--dims", type=int, nargs=3, default=[1024, 256, 512])
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0, 8.0], help="cell sizes in voxels")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()

    import torch
    from adgs import simplify
    from mesh_ab import fused_volume

    if not torch.cuda.is_available():
        raise SystemExit("simplify_ab: no HIP device; nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    vol = fused_volume(a, dev)
    vertices, faces, colors = vol.extract_mesh(min_weight=2.0)
    voxel = float(vol.voxel_size)
    del vol
    torch.cuda.empty_cache()
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    res = {"tool": "simplify_ab", "dims": list(a.dims), "views": a.views, "vertices": V, "faces": F, "voxel": voxel, "cells": {}}

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
    passes = lambda bits: -(-bits // 8)
    equal = True
    for cells in a.cells:
        cell = cells * voxel
        d = res["cells"]["%g" % cells] = {"cell_size": cell}
        d["cluster"], cl = median_ms(lambda: simplify.cluster_vertices(vertices, faces, cell))
        d["place_quadric"], (vq, cq) = median_ms(lambda: simplify.place_vertices(cl, vertices, faces, colors=colors, placement="quadric"))
        d["place_average"], _ = median_ms(lambda: simplify.place_vertices(cl, vertices, faces, colors=colors, placement="average"))
        d["whole"], (wv, wf, wc) = median_ms(lambda: simplify.simplify_mesh(vertices, faces, colors, cell_size=cell))
        d["torch"], (tv, tf, tc) = median_ms(lambda: torch_simplify(vertices, faces, colors, float32(cell)))
        d["torch_over_hip"] = round(d["torch"]["ms_median"] / d["whole"]["ms_median"], 2)
        V2, F2, M = len(cl), int(cl.faces.shape[0]), int(cl.members.shape[0])
        d.update(vertices_out=V2, faces_out=F2, counts=cl.counts)
        d["faces_equal"] = bool(tf.shape == wf.shape and torch.equal(tf, wf))
        d["max_abs_position_diff"] = float((tv - wv).abs().max()) if d["faces_equal"] and V2 else None
        d["bits_equal_from_run_to_run"] = bool(torch.equal(vq.view(torch.int32), wv.view(torch.int32)) and torch.equal(cq.view(torch.int32), wc.view(torch.int32)))
        equal = equal and d["faces_equal"] and d["bits_equal_from_run_to_run"]
        vb = V.bit_length()
        cluster_bytes = 12 * V + 32 * 8 * V + (20 * passes(vb) + 32 * passes(32 + vb) + 5 * 12) * F + 4 * 12 * V + 4 * V + 8 * V2 + 4 * M + 16 * F2
        place_bytes = 20 * passes(max(V2, 1).bit_length()) * 3 * F + 12 * F + 24 * V + 4 * M + 8 * 3 * F + 24 * V2
        for name, nbytes in (("cluster", cluster_bytes), ("place_quadric", place_bytes)):
            rate = nbytes / (d[name]["ms_median"] * 1e-3) / 1e9
            d[name].update(model_bytes=int(nbytes), GBps=round(rate, 1), share_of_copy=round(rate / copy_rate, 4))
    res["results_equal"] = equal

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not equal:
        raise SystemExit("simplify_ab: the two sides disagree")


if __name__ == "__main__":
    main()
