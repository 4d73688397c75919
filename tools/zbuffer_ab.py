"""Cost of the mesh z-buffer (adgs.zbuffer, adgs.mesh.keep_faces; include/adgs_zbuffer.h) on the mesh of tools/tsdf_ab.py's fused volume
(about 368 k vertices and 565 k faces at the defaults: mostly sub-pixel triangles) and on its simplify_mesh outputs at 2 and 8 voxels (few,
large faces), seen from the first fused camera.

    python tools/zbuffer_ab.py [--height 1280] [--width 1920] [--dims 1024 256 512] [--voxel 0.04] [--views 40] [--reps 9] [--out FILE]

Timed, HIP events around each call, the median over `reps` (at least 9) after one warm-up, per mesh:
  render_mesh   fill, setup + small faces, big faces, resolve; its parts from the entry's `stages` mask (1, 3, 7, 15: each adds one
                launch, the part is the difference of the medians)
  count_faces   FaceVisibility.add of that render
  keep_faces    the faces the view saw (with its one read-back)
  small_max     render_mesh at each threshold between the wave expansion and the list of big faces; all must give equal bits
The parent commit has no mesh renderer, so there is no other side; the tool checks that two runs and every threshold give equal bits and
exits non-zero otherwise.

Byte model of render_mesh (compulsory HBM traffic): 36 F gathered (three indices and nine floats per face) + 8 H W filled + 8 H W resolved
+ 8 H W outputs (face, depth).  The rate over that model is given as a share of the rate of a device-to-device copy of 1 GiB.  Prints one
JSON line; --out also writes it.
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

THRESHOLDS = (16, 64, 256, 1024, 4096)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1280)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--dims", type=int, nargs=3, default=[1024, 256, 512])
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    a.reps = max(a.reps, 9)

    import torch
    from adgs import mesh, simplify, zbuffer
    from mesh_ab import fused_volume

    if not torch.cuda.is_available():
        raise SystemExit("zbuffer_ab: no HIP device; nothing is measured without one")
    dev = torch.device("cuda", torch.cuda.current_device())
    vol = fused_volume(a, dev)
    vertices, faces, colors = vol.extract_mesh(min_weight=2.0)
    voxel = vol.voxel_size
    del vol
    torch.cuda.empty_cache()
    H, W = a.height, a.width
    f32 = lambda v: float(torch.tensor(float(v), dtype=torch.float32))
    cam = ((f32(W / (2 * 2050.0)), f32(H / (2 * 2050.0))), torch.eye(4, dtype=torch.float64)[:3])      # the first fused view
    meshes = {"extracted": (vertices, faces)}
    for cell in (2, 8):
        v, f, _ = simplify.simplify_mesh(vertices, faces, colors, cell_size=cell * voxel)
        meshes["simplified_%d" % cell] = (v, f)

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
        return round(statistics.median(r[0] for r in runs), 4), runs[-1][1]

    src = torch.empty(2 ** 28, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    copy_ms = statistics.median(timed(lambda: dst.copy_(src))[0] for _ in range(9))
    copy_rate = 2 * src.numel() * 4 / (copy_ms * 1e-3) / 1e9
    del src, dst

    same = lambda x, y: bool(torch.equal(x.face, y.face) and torch.equal(x.depth.view(torch.int32), y.depth.view(torch.int32)))
    res = {"tool": "zbuffer_ab", "image": [H, W], "dims": list(a.dims), "views": a.views, "reps": a.reps, "copy_GBps": round(copy_rate, 1), "meshes": {}}
    ok = True
    for name, (v, f) in meshes.items():
        V, F = int(v.shape[0]), int(f.shape[0])
        m = res["meshes"][name] = {"vertices": V, "faces": F}
        m["render_ms"], r = median_ms(lambda: zbuffer.render_mesh(v, f, cam, (H, W)))
        m["render_with_normals_ms"], _ = median_ms(lambda: zbuffer.render_mesh(v, f, cam, (H, W), normals=True))
        upto = [median_ms(lambda s=s: zbuffer.render_mesh(v, f, cam, (H, W), _stages=s))[0] for s in (1, 3, 7, 15)]
        m["parts_ms"] = dict(zip(("fill", "setup_and_small", "big", "resolve"), [round(upto[0], 4)] + [round(y - x, 4) for x, y in zip(upto, upto[1:])]))
        m["not_drawn"] = dict(zip(zbuffer.COUNTS, r.counts.tolist()))
        m["pixels_drawn"] = int((r.face >= 0).sum())
        nbytes = 36 * F + 3 * 8 * H * W
        rate = nbytes / (m["render_ms"] * 1e-3) / 1e9
        m.update(model_bytes=nbytes, GBps=round(rate, 1), share_of_copy=round(rate / copy_rate, 4))
        m["small_max_ms"] = {}
        for t in THRESHOLDS:
            m["small_max_ms"][str(t)], rt = median_ms(lambda t=t: zbuffer.render_mesh(v, f, cam, (H, W), _small_max=t))
            ok = ok and same(r, rt)
        ok = ok and same(r, zbuffer.render_mesh(v, f, cam, (H, W)))
        vis = zbuffer.FaceVisibility(F, dev)
        m["count_faces_ms"], _ = median_ms(lambda: vis.add(r))
        seen = vis.seen()
        m["faces_seen"] = int(seen.sum())
        m["keep_faces_ms"], kept = median_ms(lambda: mesh.keep_faces(seen, v, f))
        ok = ok and int(kept[1].shape[0]) == m["faces_seen"]
    res["results_equal"] = ok

    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not ok:
        raise SystemExit("zbuffer_ab: runs or thresholds disagree")


if __name__ == "__main__":
    main()
