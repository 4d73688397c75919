#!/usr/bin/env python3
"""Headline benchmark: fwd+bwd frames/s of the AD-GS hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--config C3] [--dump-outputs DIR] [--full]

One "frame" = per-frame deformation (when the config has dynamic objects) + GaussianRasterizer forward + backward with
non-zero upstream gradients on colour, depth, accumulated opacity, flow and semantic; loss and optimizer are
excluded, as in BASELINE.md.  Inputs are synthetic (seeded) and resident in HBM before the timed region.

Workloads (BASELINE.json configs):
  * C1 / C2 / C3 (default C3 = the configuration `value` is quoted on): one step = one frame per GPU.  With N > 1 every rank (one
    process per GPU over RCCL) renders its own camera of the same replicated scene and the parameter gradients are summed over
    the ranks inside the step ("scaling": "weak").  `python bench.py --gpus N` without a launcher starts the N ranks itself.
  * C4 (1 M Gaussians, 3 cameras per iteration) and C5 (3 M Gaussians, 16 objects, 5 cameras per iteration + densify/prune):
    one step = one ITERATION: the cameras are dealt round-robin to the ranks (with 4 ranks and 3 cameras one rank idles and still
    takes part in the exchange), then one gradient exchange; C5 additionally runs adgs.densify.densify_and_prune every
    `--densify-every` iterations inside the timed loop (reported separately as densify_ms).  `value` = cameras rendered per
    second ("scaling": "strong": the iteration's work is fixed as N grows).  On one GPU the same code accumulates the cameras.

Prints ONE JSON line on rank 0 with the headline (`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step` = wall time of
one timed step), per-step HIP-event statistics (median / p10 / p90) and per-step exchange / densify times.  A plain run does only what
that line needs: set-up, warm-up, exactly K timed steps, the line.  `--full` adds everything else the benchmark measures: the
per-stage breakdown and the GPU-idle share of a step (HIP events around every stage in the warm-up, around the dominant kernel in the
timed steps), "roofline" for the dominant kernel (algorithmic bytes per launch / HIP-event time of that kernel, HBM counters measured in
child runs), "cpu_baseline" (the CPU oracle timed on the host cores) with parity against it, the multi-GPU self-checks and the
secondary single-GPU measurements.

`--dump-outputs DIR`: after the timed steps, what the last timed step handed its caller -- eager steps: the rendered images and radii
of every camera of the step, the screen-space gradient and every parameter gradient; `--graph on`: the parameter gradients, all a
graph replay returns -- as DIR/<name>.npy (float32; a fixed, seeded sample of the elements of an array too large for the 64 MB
budget).  Inputs are seeded and the timed region always starts at entry 0 of the camera pool (step k renders entry k mod the pool
size, however many settle windows ran); with densify/prune in the loop a dumping run settles for a fixed number of steps.  So two
builds run with the same arguments can be compared output for output; the line names the dumped cameras (`config.dumped_outputs`).
"""
import argparse
import gc
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
PROFILE_DIR = os.path.join(ROOT, "profiles", "r06")
ITERATION_CONFIGS = {"C4": dict(cams=3, densify_every=0), "C5": dict(cams=5, densify_every=10)}


# VALU issue peak: a SIMD-32 retires one wave64 fp32 instruction per 2 cycles (MI355X_MICROARCH.md: 0.5 per SIMD and cycle), scaled by the
# SUSTAINED shader clock under the blend kernels' load over the nominal 2.4 GHz -- measured with s_memtime against s_memrealtime inside
# both kernels (tools/blend_probe.py, profiles/r04/blend_probe_c3.json: 2.35 - 2.36 GHz) and under pure VALU loops
# (tools/microbench/valu_rates.hip, profiles/r03/valu_rates.txt: 2.24 - 2.43 GHz).  The clock does not sag: round 2's "0.36" was a
# wall-time figure of a microbenchmark whose one-wave workgroups the dispatcher does not spread evenly over the SIMDs.
VALU_PEAK_PER_SIMD_CYCLE = 0.5 * 2.35 / 2.4


KNN_FLOPS_PER_PAIR = 8
VALU_FP32_PEAK_TFLOPS = 157.3


def alg_bytes(P, V, R, X, T, M, F, D_S, passes):
    """Algorithmic bytes per launch of every stage of the reference-order ("classic") pipeline."""
    pay = 12 + 4 + 12 * F + 4 * D_S
    return {
        "preprocess_fwd": P * (12 + 12 + 16 + 4 + 12 * M) + P * 4 + V * 68,
        "scan": P * 8,
        "duplicate_keys": V * 16 + R * 12,
        "radix_sort": passes * R * 24 + R * 8,
        "tile_ranges": R * 8 + T * 8,
        "render_fwd": R * 28 + R * pay + X * (12 + 4 + 4 + 12 * F + 4 * D_S + 4),
        "render_bwd": R * 28 + R * pay + X * (12 + 4 + 4 + 12 * F + 4 * D_S + 4 + 4) + V * (12 + 16 + 4 + 12 + 4 + 12 * F + 4 * D_S),
        "preprocess_bwd": P * (12 + 12 + 16 + 4 + 12 * M) + V * (24 + 3 + 4) + V * (12 + 16 + 12 + 4) + P * (12 + 12 * M + 12 + 16),
    }


def alg_bytes_v2(P, V, Rc, E, X, T, M, F, D_S, passes, E_pub=None, bucket=False, ddir=True):
    """Algorithmic bytes per launch of the default (v2, coarse-binned) pipeline -- DESIGN.md section 5.
    Rc = (cell, Gaussian) pairs that are sorted, E = (tile, Gaussian) entries blended, E_pub = entries the backward replays.
    bucket: bucket binning (binning.hip) -- "scan" = the column scan of the counts matrix [P / 256][cells] (read + written once) + the cell scan,
    "duplicate_keys" = the scatter (16 B per Gaussian in, its counts row, 12 B per pair out), "radix_sort" = the depth-slab sort (a cell's
    4-byte keys streamed once per slab of the cell -- ~8 slabs at C3 --, 8 B per pair gathered, 8 B out: the sort never leaves the CU), no range pass.
    ddir: the preprocess forward stores d colour / d view direction (36 B per visible Gaussian) and the backward reads those instead of
    the SH row a second time (raw-SH path, 16 coefficients: round 5)."""
    out = X * (12 + 4 + 4 + 12 * F + 4 * D_S + 4)
    ncells, slabs = 70, 8
    binning = ({"scan": ((P + 255) // 256) * ncells * 8, "duplicate_keys": P * 16 + ((P + 255) // 256) * ncells * 4 + Rc * 12, "radix_sort": Rc * (4 * slabs + 8 + 8), "tile_ranges": 0} if bucket else
               {"scan": P * 12, "duplicate_keys": V * (8 + 4) + Rc * 12, "radix_sort": passes * Rc * 24 + Rc * 8, "tile_ranges": Rc * 8})
    return {
        "preprocess_fwd": P * (12 + 12 + 16 + 4 + 12 * M) + P * 12 + V * (64 + 24 + 1 + 64) + (V * 36 if ddir else 0),      # Splat line, binning words, clamp byte, zeroed accumulator line (no filter record since round 4)
        **binning,
        "render_fwd": E * (4 + 64 + 4) + out,
        "render_bwd": (E if E_pub is None else E_pub) * (4 + 64 + 56) + X * (12 + 4 + 4 + 12 * F + 4 * D_S + 4 + 4),
        "preprocess_bwd": P * (12 + 12 + 16 + 4) + (V * 36 if ddir else P * 12 * M) + V * (64 + 32 + 24 + 1) + V * 64 + P * (12 + 12 * M + 12 + 16 + 12 + 16 + 4 + 12 + 4 + 24),
    }


# ------------------------------------------------------------------ scenes
def build_scene(config, variant="default"):
    """BASELINE.json config scene, or one of three C3-sized stress variants for the scene-sensitivity lines:
    'translucent' (opacity x 0.05 + 0.01: no pixel saturates, every tile walks its whole list), 'sky' (the upper 40 % of the
    image is empty; the Gaussians that were there lie on the road plane y = +1.5 m instead: long lists around the horizon) and
    'street' (a driving-scene layout with NON-UNIFORM depth complexity: a road plane, two facades seen at grazing angles that pile
    up towards the vanishing point, semi-transparent Gaussians, empty sky -- the p99 / median of the per-tile list lengths is
    printed with the line: `entries_per_tile`)."""
    import torch
    from adgs import synthetic
    sc = synthetic.make_config_scene(config)
    if variant == "translucent":
        sc["opacities"] = (sc["opacities"] * 0.05 + 0.01).contiguous()
    elif variant == "sky":
        xyz = sc["means3D"].clone()
        z = xyz[:, 2].clamp_min(0.3)
        up = (xyz[:, 1] / z) < -0.2 * sc["tanfovy"]              # projects into the upper 40 % of the image
        up &= ~sc["obj_mask"]
        g = torch.Generator().manual_seed(77)
        n = int(up.sum())
        xyz[up, 1] = 1.5 + 0.05 * torch.randn(n, generator=g)    # the road plane, 1.5 m below the camera (y points down)
        sc["means3D"] = xyz.contiguous()
        sc["flow_points"] = (xyz + 0.05 * torch.randn(xyz.shape, generator=g)).float().contiguous()
    elif variant == "street":
        g = torch.Generator().manual_seed(78)
        xyz = sc["means3D"].clone()
        scene = ~sc["obj_mask"]
        n = int(scene.sum())
        z = torch.rand(n, generator=g) ** 0.6 * 88.0 + 2.0                       # denser far away: the vanishing point collects them
        kind = torch.rand(n, generator=g)
        x = (torch.rand(n, generator=g) * 2 - 1) * 7.5
        y = 1.5 + 0.04 * torch.randn(n, generator=g)                             # road plane, 1.5 m below the camera (y points down)
        wall = kind > 0.35                                                       # 65 %: the two facades at x = -8 / +8 m, 0 .. 14 m high
        side = torch.where(torch.rand(n, generator=g) > 0.5, 1.0, -1.0)
        x = torch.where(wall, side * (8.0 + 0.05 * torch.randn(n, generator=g)), x)
        y = torch.where(wall, 1.5 - torch.rand(n, generator=g) * 14.0, y)
        xyz[scene] = torch.stack([x, y, z], 1)
        sc["means3D"] = xyz.contiguous()
        op = sc["opacities"].clone()
        op[scene] = torch.sigmoid(1.2 * torch.randn(n, 1, generator=g) - 1.6)    # mostly semi-transparent: saturation takes many entries where they pile up
        sc["opacities"] = op.contiguous()
        sc["flow_points"] = (xyz + 0.05 * torch.randn(xyz.shape, generator=g)).float().contiguous()
    elif variant != "default":
        raise ValueError(variant)
    if os.environ.get("ADGS_BENCH_SCENE_ORDER") == "morton":
        # locality experiment (never the headline): the same Gaussians, stored in Morton order of their image position inside the
        # scene range and inside the object range (the generator -- like SfM points and densification -- leaves them in random order)
        xyz = sc["means3D"]
        z = xyz[:, 2].clamp_min(0.3)
        u = ((xyz[:, 0] / z / sc["tanfovx"]) * 0.5 + 0.5).clamp(0, 1)
        v = ((xyz[:, 1] / z / sc["tanfovy"]) * 0.5 + 0.5).clamp(0, 1)
        ui, vi = (u * 1023).long(), (v * 1023).long()
        code = torch.zeros_like(ui)
        for b in range(10):
            code |= ((ui >> b) & 1) << (2 * b)
            code |= ((vi >> b) & 1) << (2 * b + 1)
        code = code + (sc["obj_mask"].long() << 40)              # objects stay behind the scene Gaussians
        perm = torch.argsort(code, stable=True)
        for k in ("means3D", "scales", "rotations", "opacities", "shs", "semantic", "flow_points", "obj_mask"):
            if k in sc:
                sc[k] = sc[k][perm].contiguous()
    return sc


# ------------------------------------------------------------------ per-frame work
class StaticFrame:
    """Per-frame work on already-deformed parameters: rasterizer forward (+ autograd backward)."""

    deform_bytes = 0
    deform_desc = "none (static, already activated parameters)"

    def __init__(self, sc, rasterizer, device, use_flow_sem, share=None):
        """share: another StaticFrame of the same scene (a camera pool renders ONE set of parameters)."""
        import torch
        self.rast = rasterizer
        if share is not None:
            self.leaf, self.means2D, self.flow, self.sem = share.leaf, share.means2D, share.flow, share.sem
        else:
            self.leaf = {k: sc[k].to(device).clone().requires_grad_(True) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
            self.means2D = torch.zeros(sc["P"], 3, device=device, requires_grad=True)
            self.flow = sc["flow_points"].to(device) if use_flow_sem else None
            self.sem = sc["semantic"].to(device) if use_flow_sem else None
        self.last_radii = None

    def parameters(self):
        return list(self.leaf.values())

    def zero_grad(self):
        for p in self.parameters():
            p.grad = None
        self.means2D.grad = None

    def forward(self, sink_for=None):
        L = self.leaf
        color, radii, depth, op, flow, sem = self.rast(
            means3D=L["means3D"], means2D=self.means2D, opacities=L["opacities"], shs=L["shs"], scales=L["scales"],
            rotations=L["rotations"], flow_points=self.flow, semantic=self.sem)
        self.last_radii = radii
        return [color, depth, op] + ([flow, sem] if self.flow is not None else [])


class DeformFrame:
    """Per-frame work of the dynamic configs (C3-C5): fused B-spline/Fourier/quaternion-spline deformation of the raw parameters at
    the camera time (+ the flow points at t+0.05), then the rasterizer; the backward runs through both into every raw parameter.
    Several frames (cameras) may share one model."""

    def __init__(self, sc, rasterizer, device, use_flow_sem, t=0.37, model=None):
        from adgs.model import SyntheticGaussianModel
        self.rast, self.t, self.use_fs = rasterizer, t, use_flow_sem
        self.model = model if model is not None else SyntheticGaussianModel.from_scene(sc, device, seed=0)
        self.model.raw_sh = os.environ.get("ADGS_BENCH_RAW_SH", "1") != "0"     # SH read straight from the raw parameters
        self.model.raw_scene = os.environ.get("ADGS_BENCH_RAW_SCENE", "1") != "0"   # scene geometry too: activations inside the preprocess
        self.fused_flow = os.environ.get("ADGS_BENCH_FUSED_FLOW", "1") != "0"      # flow-time xyz in the same deformation pass
        self._sem = None
        self.last_radii = None
        self.last_means2D = None
        self.deform_bytes = self.model.deform_bytes_per_frame()
        oa = self.model.order_args
        self.deform_desc = "fused HIP: xyz %s, rotation %s (quaternion spline), shs %s%s, time-masked opacity; %d object Gaussians" % (
            oa["xyz"], oa["rotation"], oa["shs"], (" (read in place by the preprocess: raw-SH path%s)" % (
                "; scene-range exp / normalize / sigmoid inside the preprocess: raw-scene path" if self.model.raw_scene else "")) if self.model.raw_sh else "",
            self.model.get_obj_pts_num)

    @property
    def sem(self):
        if not self.use_fs:
            return None
        if self._sem is None or self._sem.shape[0] != self.model.get_pts_num:      # densification changes the point count
            self._sem = self.model.get_obj_mask.float()[:, None].contiguous()
        return self._sem

    def parameters(self):
        return self.model.parameters()

    def zero_grad(self):
        self.model.zero_grad()

    def forward(self, sink_for=None):
        """sink_for: adgs.dp.FactoredSHExchange.sink_for -- the backward then leaves the SH gradients in factored form."""
        import torch
        m = self.model
        if self.use_fs and self.fused_flow:
            pkg = m.get_deformed_pkg(self.t, flow_time=self.t + 0.05)
            flow = pkg["flow_xyz"]
        else:
            pkg = m.get_deformed_pkg(self.t)
            flow = m.get_deformed_xyz(self.t + 0.05) if self.use_fs else None
        from gaussian_renderer import screenspace_points
        means2D = screenspace_points(pkg["xyz"].shape[0], pkg["xyz"].device)      # what render() uses: a fresh leaf over cached zeros
        if torch.is_tensor(pkg["shs"]):
            color, radii, depth, op, fl, sem = self.rast(
                means3D=pkg["xyz"], means2D=means2D, opacities=pkg["opacity"], shs=pkg["shs"], scales=pkg["scales"],
                rotations=pkg["rotation"], flow_points=flow, semantic=self.sem)
        else:
            color, radii, depth, op, fl, sem = self.rast.forward_rawsh(pkg["xyz"], means2D, pkg["opacity"], pkg["shs"], pkg["scales"],
                                                                       pkg["rotation"], flow_points=flow, semantic=self.sem,
                                                                       factor_sink=None if sink_for is None else sink_for(pkg["xyz"]))
        self.last_radii, self.last_means2D = radii, means2D
        return [color, depth, op] + ([fl, sem] if self.use_fs else [])

    def activated(self):
        """Activated tensors of this frame as CPU float32 (inputs of the CPU baseline)."""
        import torch
        with torch.no_grad():
            from adgs import deform
            pkg = deform.get_deformed_pkg(self.model, self.t)
            flow = self.model.get_deformed_xyz(self.t + 0.05)
        return {k: v.detach().cpu() for k, v in pkg.items()}, flow.cpu()


def make_settings(cfg, cam, sc, device):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    d = lambda t: t.to(device)
    return GaussianRasterizationSettings(cfg["H"], cfg["W"], cam["tanfovx"], cam["tanfovy"], d(sc["bg"]), 1.0, d(cam["viewmatrix"]),
                                         d(cam["projmatrix"]), cfg["sh_degree"], d(cam["campos"]), False, True, False)


def make_frame(sc, cfg, cam, device, use_fs, t=0.37, model=None, share=None):
    from diff_gaussian_rasterization import GaussianRasterizer
    rast = GaussianRasterizer(make_settings(cfg, cam, sc, device))
    if cfg["n_objects"] > 0:
        return DeformFrame(sc, rast, device, use_fs, t=t, model=model if model is not None else getattr(share, "model", None))
    return StaticFrame(sc, rast, device, use_fs, share=share)


def camera_pool(cfg, n, first=0, stride=1):
    """The cameras / time stamps a training run cycles through (train.py:55-61 draws a random camera per iteration): pool entry 0
    of rank 0 is the canonical SURVEY.md 8(d) camera (identity view, t = 0.37), the others are jittered in yaw / pitch / position
    (adgs.synthetic.make_camera) at time stamps spread over [0.1, 0.9].  Returns [(camera, t)]; entry k has id first + k * stride."""
    from adgs import synthetic
    out = []
    for k in range(n):
        cid = first + k * stride
        cam = synthetic.make_camera(cfg["W"], cfg["H"], cfg["focal"], cam_seed=None if cid == 0 else cid)
        out.append((cam, 0.37 if cid == 0 else 0.1 + 0.8 * ((cid * 7) % 16) / 15.0))
    return out


def frame_pool(sc, cfg, pool, device, use_fs):
    frames = []
    for cam, t in pool:
        frames.append(make_frame(sc, cfg, cam, device, use_fs, t=t, share=frames[0] if frames else None))
    return frames


def graphed_steps(frames, ups):
    """adgs.graph.GraphCache over a frame pool: key k replays forward + backward of frames[k] as one HIP graph and returns the
    parameter gradients (static tensors of that graph)."""
    import torch
    from adgs import graph

    def make_fn(k):
        f = frames[k]

        def fn():
            torch.autograd.backward(f.forward(), ups)
            grads = [p.grad for p in f.parameters()]
            f.zero_grad()
            return grads
        return fn
    return graph.GraphCache(make_fn, warmup=2)


# ------------------------------------------------------------------ scene statistics
def frame_work_figures(frame, settings, use_fs, device, with_ref=True, full=False):
    """(E, R, E_pub, scanned) -- with `full` also (V, Rc, fine_pairs) of that forward: E = (tile, Gaussian) entries the v2 forward hands to the blend loop (counted by the kernel), R = the reference's num_rendered for the same frame (one extra forward in classic mode),
    E_pub = the entries at least one pixel blends (what the backward replays), scanned = candidates of the cell lists that the
    tiles' walks went through."""
    import ctypes
    import torch
    from diff_gaussian_rasterization import _C
    from adgs import deform, _lib
    with torch.no_grad():
        if isinstance(frame, DeformFrame):
            pkg = deform.get_deformed_pkg(frame.model, frame.t)
            flow = frame.model.get_deformed_xyz(frame.t + 0.05) if use_fs else torch.empty(0, device=device)
            t = dict(means3D=pkg["xyz"], opacities=pkg["opacity"], scales=pkg["scales"], rotations=pkg["rotation"], shs=pkg["shs"])
        else:
            t = {k: v.detach() for k, v in frame.leaf.items()}
            flow = frame.flow if use_fs else torch.empty(0, device=device)
        sem = frame.sem if use_fs else torch.empty(0, device=device)
        e = torch.empty(0, device=device)
        s = settings
        call = lambda: _C.rasterize_gaussians(s.bg, t["means3D"], e, t["opacities"], t["scales"], t["rotations"], s.scale_modifier, e, s.viewmatrix,
                                              s.projmatrix, s.tanfovx, s.tanfovy, s.image_height, s.image_width, t["shs"], flow, sem, s.sh_degree,
                                              s.campos, s.prefiltered, s.inv_depth, False)
        out = call()
        fstats = _lib.frame_stats()
        st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        chunks = int(_lib.lib().adgs_test_v2_blend_batches(out[7].data_ptr(), int(s.image_width), int(s.image_height), st))
        published = int(_lib.lib().adgs_test_v2_published_entries(out[7].data_ptr(), int(s.image_width), int(s.image_height), st))
        scanned = int(_lib.lib().adgs_test_v2_scanned_candidates(out[7].data_ptr(), int(s.image_width), int(s.image_height), st))
        r_ref = 0
        if with_ref:
            old = os.environ.get("ADGS_RASTER_MODE")
            os.environ["ADGS_RASTER_MODE"] = "classic"
            try:
                r_ref = int(call()[0])
            finally:
                if old is None:
                    del os.environ["ADGS_RASTER_MODE"]
                else:
                    os.environ["ADGS_RASTER_MODE"] = old
    if full:
        return chunks, r_ref, published, scanned, int((out[4] > 0).sum().item()), fstats["num_rendered"], fstats["fine_pairs"]
    return chunks, r_ref, published, scanned


HBM_FILL_GBS = 6900.0       # the fastest stream this box class delivers (write-only fill, profiles/r06/hbm_rates.txt): nothing can beat it


def dominant_roofline(stage, stage_bytes_per_frame, mean_ms_per_bracket, brackets, frames):
    """The `roofline` object of the bench line for `stage`: its algorithmic bytes per frame over its HIP-event time per FRAME.
    `brackets` event brackets were recorded over `frames` rendered frames (a stage with two launch groups per frame has two per frame).
    A figure above the box's fill rate is an instrument error, never a result: it is flagged and the fraction withheld."""
    per_frame = max(brackets, 1) / max(frames, 1)
    ms = mean_ms_per_bracket * per_frame
    achieved = stage_bytes_per_frame / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    roof = {"bound": "hbm", "kernel": stage, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": None,
            "alg_bytes_per_launch": int(stage_bytes_per_frame), "avg_launch_ms": round(ms, 4),
            "launch_groups_per_frame": round(per_frame, 3), "launches_timed": int(brackets)}
    if achieved > HBM_FILL_GBS:
        roof["instrument_error"] = "achieved %.0f GB/s exceeds the box's %.0f GB/s fill rate: bytes and time do not belong together" % (achieved, HBM_FILL_GBS)
        roof["frac"] = None
        print("bench: roofline instrument error for %s: %s" % (stage, roof["instrument_error"]), file=sys.stderr)
    return roof


def library_stamp():
    """First 16 hex digits of the SHA-256 of the loaded libadgs_hip.so: the committed counter files carry the stamp of the build
    they were collected on (tools/pmc_traffic.py, tools/pmc_blend.py), and are flagged stale when it differs."""
    import hashlib
    from adgs import _lib
    try:
        return hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
    except OSError:
        return None


def committed_pmc(stage, config, measured_case):
    """HBM traffic / VALU issue rate of the dominant kernel from the committed rocprofv3 --pmc passes of THIS round's build
    (profiles/r06/, collected with this same command line; counters cannot be read from inside the process).  Only attached for
    the case they were measured on (C3, flow+semantic, default pipeline); absent files leave `traffic` null; counters collected on
    another build of the library are flagged (`counters_stale`)."""
    if config != "C3" or not measured_case:
        return {}
    kname = {"render_bwd": "render_bwd_v2_kernel", "render_fwd": "render_fwd_v2_kernel", "preprocess_bwd": "preprocess_bwd_kernel",
             "preprocess_fwd": "preprocess_fwd_kernel"}.get(stage)
    out = {}
    stamp = library_stamp()
    try:
        tr = json.load(open(os.path.join(PROFILE_DIR, "hbm_traffic_per_kernel.json")))
        for k, v in tr.items():
            if kname and kname in k:
                out["traffic"] = v["hbm_bytes_per_launch"]
                out["traffic_source"] = ("profiles/r06/hbm_traffic_per_kernel.json (rocprofv3 --pmc, separate FETCH_SIZE / WRITE_SIZE passes of this command; "
                                         "FETCH_SIZE x2 per the gfx950 note of MI355X_MICROARCH.md, per launch)")
                break
        pmf = json.load(open(os.path.join(PROFILE_DIR, "pmc_blend_kernels.json")))
        pm = pmf["kernels"].get(kname)
        if pm:
            out["valu_insts_per_simd_cycle"] = pm.get("valu_insts_per_simd_cycle")
            out["valu_issue_frac_of_peak"] = None if pm.get("valu_insts_per_simd_cycle") is None else round(pm["valu_insts_per_simd_cycle"] / VALU_PEAK_PER_SIMD_CYCLE, 3)
            out["wave_state_shares"] = pm.get("wave_state_shares")
            out["waves_per_simd_mean"] = pm.get("waves_per_simd_mean")
            out["valu_note"] = ("the blend kernels are far from the HBM roof by construction (SURVEY.md 8(d)): wave64 VALU instructions per SIMD and cycle "
                                "(rocprofv3 --pmc, profiles/r06/pmc_blend_kernels.json; normalisation: tools/pmc_blend.py) against the full-rate fp32 issue rate "
                                "0.5 x the sustained shader clock over the nominal 2.4 GHz = %.3f -- a ceiling the kernels' instruction mixes cannot reach (half-rate "
                                "compares / selects, quarter-rate exp / rcp: tools/isa_mix.py, tools/microbench/issue_hazards.hip); wave_state_shares: where the "
                                "resident waves' cycles go (issuing / parked at s_waitcnt / ready but not issued)" % VALU_PEAK_PER_SIMD_CYCLE)
        built = tr.get("_library_sha256_16") if isinstance(tr, dict) else None
        if out and (built is None or built != stamp):
            out["counters_stale"] = "the committed counter files were collected on library build %s, this run loaded %s" % (built, stamp)
    except (OSError, ValueError, KeyError, AttributeError):
        pass
    return out


def measure_traffic_in_run(stage, argv_config, timeout_s=75):
    """HBM bytes per launch of the dominant kernel MEASURED IN THIS RUN: two child processes of this same script under
    `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (separate passes, counters only: MI355X_MICROARCH.md, HBM section; FETCH_SIZE counts
    128-byte requests at 64 bytes on gfx950: x 2; both in KiB), a handful of steps each, the program itself after `--`.  Returns
    {traffic, traffic_source, ...} or {} when rocprofv3 is not on the box, ADGS_BENCH_PMC=0, or a pass fails (the caller then replays
    the committed counters and says so)."""
    import csv, shutil, tempfile
    kname = {"render_bwd": "render_bwd_v2_kernel", "render_fwd": "render_fwd_v2_kernel", "preprocess_bwd": "preprocess_bwd_kernel",
             "preprocess_fwd": "preprocess_fwd_kernel"}.get(stage)
    exe = shutil.which("rocprofv3")
    if not exe or not kname or os.environ.get("ADGS_BENCH_PMC", "1") == "0":
        return {}
    out, vals = {}, {}
    t0 = time.perf_counter()
    env = dict(os.environ, ADGS_BENCH_PMC="0", ADGS_BENCH_SKIP_STATS="1", ADGS_BENCH_SETTLE="0", TMPDIR="/tmp")
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="adgs_pmc_", dir="/tmp")
        try:
            cmd = [exe, "--pmc", counter, "--output-format", "csv", "-d", d, "-o", "pmc", "--", sys.executable, os.path.abspath(__file__), "--gpus", "1", "--steps", "4",
                   "--warmup", "2", "--config", argv_config, "--no-cpu-baseline", "--no-secondary"]
            subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s, check=True)
            tot, n = 0.0, 0
            for root, _, files in os.walk(d):
                for f in files:
                    if f.endswith("counter_collection.csv"):
                        for r in csv.DictReader(open(os.path.join(root, f))):
                            if kname in r.get("Kernel_Name", "") and r.get("Counter_Name", counter) == counter:
                                tot += float(r["Counter_Value"]); n += 1
            if n == 0:
                return {}
            vals[counter] = (tot / n, n)
        except (subprocess.SubprocessError, OSError, ValueError, KeyError):
            return {}
        finally:
            shutil.rmtree(d, ignore_errors=True)
    rd, wr = 2.0 * vals["FETCH_SIZE"][0] * 1024, vals["WRITE_SIZE"][0] * 1024
    out["traffic"] = int(rd + wr)
    out["traffic_read_bytes"], out["traffic_write_bytes"] = int(rd), int(wr)
    out["traffic_measured_in_run"] = True
    out["traffic_source"] = ("measured in this run: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE (separate passes of this script, %d + %d launches of %s; KiB, "
                             "FETCH_SIZE x 2 on gfx950 per MI355X_MICROARCH.md), %.0f s" % (vals["FETCH_SIZE"][1], vals["WRITE_SIZE"][1], kname, time.perf_counter() - t0))
    return out


# stage of the bench line -> (kernels of the stage, "f" / "b": launched once per forward / per backward)
STAGE_KERNELS = {"preprocess_fwd": (("sh0_rows_kernel", "sh0_kernel", "preprocess_fwd_kernel"), "f"), "render_fwd": (("render_fwd_v2_kernel", "tile_order_kernel"), "f"),      # + the tile order for the backward and for this camera's next forward
                 "render_bwd": (("render_bwd_v2_kernel",), "b"),
                 "preprocess_bwd": (("preprocess_bwd_kernel", "deform_lin_param_grad_kernel"), "b"),      # + the SH-deformation gradient rows of the raw-SH path (launched by the raster backward)
                 "deform_fwd": (("deform_fwd_kernel",), "f"), "deform_bwd": (("deform_bwd_kernel",), "b"),
                 "scan": (("cell_colscan_kernel", "cell_scan_kernel"), "f"), "duplicate_keys": (("cell_scatter_kernel",), "f"),
                 "radix_sort": (("cell_sample_kernel", "slab_sort_kernel", "slab_sort_slow_kernel"), "f")}      # the "radix_sort" slot of a bucket-binned frame: the depth-slab sort


def committed_kernel_stats():
    """Per-stage kernel time per step from the committed rocprofv3 --kernel-trace --stats summary of this round (profiles/r06/kernel_stats.csv):
    total duration of the stage's kernels over the number of forwards / backwards in the profiled run (= the calls of the blend kernel of that
    direction).  Empty when the file is absent."""
    import csv
    path = os.path.join(PROFILE_DIR, "kernel_stats.csv")
    out = {}
    try:
        rows = list(csv.DictReader(open(path)))
        calls = {"f": 0, "b": 0}
        for r in rows:
            if "render_fwd_v2_kernel<4>" in r["Name"]:
                calls["f"] = int(r["Calls"])
            if "render_bwd_v2_kernel<4, true>" in r["Name"]:
                calls["b"] = int(r["Calls"])
        for stage, (pats, d) in STAGE_KERNELS.items():
            if not calls[d]:
                continue
            ns, names = 0.0, []
            for r in rows:
                if any(p in r["Name"] for p in pats):
                    ns += float(r["TotalDurationNs"]); names.append(r["Name"].replace("void ", "").replace("adgs::", "").replace("(anonymous namespace)::", "").split("(")[0])
            if ns > 0:
                out[stage] = {"ms": round(ns / calls[d] * 1e-6, 4), "kernels": sorted(set(names))}
    except (OSError, ValueError, KeyError):
        return {}
    return out


def committed_frame_traffic(config, measured_case, fps_per_gpu):
    if config != "C3" or not measured_case:
        return {}
    try:
        tot = json.load(open(os.path.join(PROFILE_DIR, "hbm_traffic_per_frame.json")))
        out = {"measured_hbm_bytes_per_frame": int(tot["hbm_bytes_per_frame"]),
               "measured_hbm_frac_of_8TBs": round(tot["hbm_bytes_per_frame"] * fps_per_gpu / 1e9 / HBM_PEAK_GBS, 4)}
        if tot.get("_library_sha256_16") != library_stamp():
            out["measured_hbm_stale"] = True
        return out
    except (OSError, ValueError, KeyError):
        return {}


# ------------------------------------------------------------------ CPU baseline / parity
def cpu_deformation_seconds(model, t, t_flow):
    """The frame's deformation stage on the CPU (BASELINE.md section 2 times the frame WITH it): oracle/deform_oracle.py -- the NumPy
    restatement of get_deformed_pkg / get_deformed_xyz (scene/gaussian_model.py:173-231, utils/func_utils.py:121-173), single thread --
    on the raw parameters of the benchmarked model, at the camera time and at the flow time.  Forward only: the chain rule through the
    deformation exists on the CPU as float64 torch autograd in the tests, not as an oracle (stated in the sample text)."""
    import numpy as np
    from oracle import deform_oracle as do
    names = {"scene_xyz": "_scene_xyz", "obj_xyz": "_obj_xyz", "scene_shs_dc": "_scene_shs_dc", "obj_shs_dc": "_obj_shs_dc", "scene_shs_rest": "_scene_shs_rest",
             "obj_shs_rest": "_obj_shs_rest", "scene_scaling": "_scene_scaling", "obj_scaling": "_obj_scaling", "scene_rotation": "_scene_rotation",
             "obj_rotation": "_obj_rotation", "scene_opacity": "_scene_opacity", "obj_opacity": "_obj_opacity", "xyz_deform_param": "xyz_deform_param",
             "rotation_deform_param": "rotation_deform_param", "shs_deform_param_scene": "shs_deform_param_scene", "shs_deform_param_obj": "shs_deform_param_obj",
             "background_deform_param": "background_deform_param", "gs_time_sigma": "gs_time_sigma", "gs_time": "gs_time"}
    raw = {k: getattr(model, a).detach().cpu().numpy().astype(np.float32) for k, a in names.items()}
    raw["order_args"], raw["use_time_mask"] = model.order_args, model.use_time_mask
    t0 = time.perf_counter()
    do.get_deformed_pkg(raw, t)
    if t_flow is not None:
        obj = raw["obj_xyz"] + do.get_func_result(t_flow, raw["xyz_deform_param"], model.order_args["xyz"])
        _ = np.concatenate([raw["scene_xyz"], np.asarray(obj, np.float32)], 0) + do.get_func_result(t_flow, raw["background_deform_param"], model.order_args["background"])
    return time.perf_counter() - t0


def cpu_baseline(sc, cam, cfg, use_fs, up, threads=None, deform_s=None):
    """The CPU oracle (oracle/, a port of the reference kernels -- the reference has no CPU path) timed on this host's cores
    for ONE frame of the same workload; deform_s: seconds of the frame's deformation stage on the CPU (cpu_deformation_seconds), part
    of the frame where the configuration has one."""
    import numpy as np
    from oracle import oracle
    H, W = cfg["H"], cfg["W"]
    all_threads = oracle.num_threads()
    if threads is not None:
        oracle.set_num_threads(threads)
    try:
        o = oracle.RasterOracle("f32")
        t0 = time.perf_counter()
        fwd = o.forward(sc["bg"], sc["means3D"], None, sc["opacities"], sc["scales"], sc["rotations"], 1.0, None, cam["viewmatrix"],
                        cam["projmatrix"], cam["tanfovx"], cam["tanfovy"], H, W, sc["shs"], sc["flow_points"] if use_fs else None,
                        sc["semantic"] if use_fs else None, cfg["sh_degree"], cam["campos"], False, True)
        t1 = time.perf_counter()
        o.backward(up["color"], up["depth"], up["flow"] if use_fs else np.zeros((3, H, W), np.float32), up["semantic"] if use_fs else None,
                   up["img_opacity"])
        t2 = time.perf_counter()
        cores = oracle.num_threads()
    finally:
        if threads is not None:
            oracle.set_num_threads(all_threads)
    total = (t2 - t0) + (deform_s or 0.0)
    base = {"value": round(1.0 / total, 5), "unit": "frames/s", "cores": cores, "kind": "port",
            "sample": "1 full frame (%srasterizer fwd %.3f s + bwd %.3f s) of the same scene and camera, %s, g++ -O3 -fno-fast-math -ffp-contract=off" % (
                ("deformation forward at the camera and the flow time %.3f s [NumPy, one thread; its O(N) backward is not part of the oracle] + " % deform_s)
                if deform_s is not None else "", t1 - t0, t2 - t1, "OpenMP over Gaussians/tiles" if cores > 1 else "single thread")}
    return base, fwd


def parity_vs_oracle(hip_outs, oracle_fwd):
    """BASELINE.json's 'PSNR vs ref' (utils/image_utils.py:17-19: 20 log10(1 / sqrt(mse))) of the HIP frame against the CPU
    oracle's frame of the same inputs, plus the largest absolute deviations."""
    import numpy as np
    color = hip_outs[0].detach().float().cpu().numpy(); depth = hip_outs[1].detach().float().cpu().numpy().reshape(-1)
    oc = np.asarray(oracle_fwd["color"], np.float32).reshape(color.shape); od = np.asarray(oracle_fwd["depth"], np.float32).reshape(-1)
    mse = float(np.mean((color.astype(np.float64) - oc.astype(np.float64)) ** 2))
    return {"psnr_vs_oracle_db": round(20.0 * np.log10(1.0 / np.sqrt(mse)), 2) if mse > 0 else float("inf"),
            "max_abs_err_color": float(np.abs(color - oc).max()), "max_abs_err_depth": float(np.abs(depth - od).max()),
            "depth_scale": float(np.abs(od).max()),
            "frac_color_outside_1e-4": float(np.mean(np.abs(color - oc) > 1e-4 * (1.0 + np.abs(oc)))),
            "note": "gate flips at alpha = 1/255: tests/test_gpu_gate_flips.py shows the float32 oracle itself is this far from the float64 result"}


# ------------------------------------------------------------------ timing helpers
def knn_measure(device, sizes=((1_000_000, "C3"), (3_000_000, "C5")), cpu_points=1_000_000, with_cpu=True):
    """simple-knn (R11, KNN/simple_knn.cu:185-221, called once at scene/gaussian_model.py:277): adgs_knn_dist2 on the positions of the
    C3 / C5 scenes.  Algorithmic bytes P (12 + 16 + 4): the points read, their Morton-ordered float4 copy, the distances written.
    CPU baseline: oracle/knn_oracle.cpp, the line-by-line restatement of the same box-pruned search (O(P x boxes) box tests plus the
    points of the boxes that survive them), OpenMP over the host's threads, on the first workload's cloud (`cpu_points` of it)."""
    import ctypes as _ct
    import gc
    import torch
    from adgs import _lib as _l, synthetic as _syn
    from simple_knn._C import distCUDA2
    out = []
    lib = _l.lib()
    for P, cfg_name in sizes:
        sc = _syn.make_config_scene(cfg_name)
        pts = sc["means3D"][:P].to(device).contiguous()
        P = int(pts.shape[0])
        for _ in range(2):
            distCUDA2(pts)
        torch.cuda.synchronize()
        ws = torch.empty((int(lib.adgs_knn_workspace_bytes(P)),), dtype=torch.uint8, device=device)
        res = torch.empty((P,), dtype=torch.float32, device=device)
        stream = _ct.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        n = 5
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            _l.check(lib.adgs_knn_dist2(P, pts.data_ptr(), res.data_ptr(), ws.data_ptr(), stream), "adgs_knn_dist2")
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / n
        staged = int(ws[24:32].view(torch.int64).item())
        nboxes = (P + 1023) // 1024
        ab = P * (12 + 16 + 4)
        r = {"workload": "%s positions" % cfg_name, "points": P, "ms": round(ms, 3), "points_per_s": round(P / (ms * 1e-3)), "alg_bytes": ab,
             "GB/s_algorithmic": round(ab / (ms * 1e-3) / 1e9, 1), "frac_of_8TBs": round(ab / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
             "boxes": nboxes, "boxes_scanned_per_query_box": round(staged / max(nboxes, 1), 1),
             "candidate_points_scanned_per_query": round(staged / max(nboxes, 1) * 1024)}
        # which roof: not HBM (the cloud is read ~twice: 0.0002 of 8 TB/s) -- the distance arithmetic of the box scan on the fp32 vector
        # pipes.  KNN_FLOPS_PER_PAIR per (query, candidate) pair: 3 subtractions, 1 multiply + 2 fused multiply-adds (5 flops), and the
        # three compare / select steps of the 3-best insertion counted as one flop each.
        pairs = float(P) * r["candidate_points_scanned_per_query"]
        tflops = pairs * KNN_FLOPS_PER_PAIR / (ms * 1e-3) / 1e12
        r["roofline"] = {"bound": "valu", "achieved": round(tflops, 2), "peak": VALU_FP32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(tflops / VALU_FP32_PEAK_TFLOPS, 4),
                         "point_pairs_per_s": round(pairs / (ms * 1e-3)), "flops_per_pair": KNN_FLOPS_PER_PAIR,
                         "note": "fp32 vector peak of MI355X_MICROARCH.md (256 CUs x 4 SIMDs x 64 lanes x 2 flops x 2.4 GHz); compares and selects issue at "
                                 "half rate (profiles/r04/issue_hazards.txt), so ~0.6 of the peak is what this mix could reach"}
        out.append(r)
        del ws, res, pts
        gc.collect(); torch.cuda.empty_cache()
    if with_cpu:
        from oracle import oracle as _o
        sc = _syn.make_config_scene(sizes[0][1])
        sub = sc["means3D"][torch.randperm(sc["means3D"].shape[0], generator=torch.Generator().manual_seed(0))[:cpu_points]].numpy()
        t0 = time.perf_counter()
        _o.knn_dist2(sub)
        dt = time.perf_counter() - t0
        out.append({"cpu_baseline": {"points": int(sub.shape[0]), "ms": round(dt * 1e3, 1), "points_per_s": round(sub.shape[0] / dt), "cores": _o.num_threads(),
                                     "kind": "port", "sample": "oracle/knn_oracle.cpp (the reference's box-pruned search restated; cost grows ~quadratically: P/1024 box tests per "
                                     "point) on %d of the %s positions" % (sub.shape[0], sizes[0][1])}})
    return out


def percentile(xs, q):
    xs = sorted(xs)
    if not xs:
        return 0.0
    k = (len(xs) - 1) * q
    lo, hi = int(k), min(int(k) + 1, len(xs) - 1)
    return xs[lo] + (xs[hi] - xs[lo]) * (k - lo)


def timed_loop(step, steps, sync, barrier=None):
    """EXACTLY `steps` calls of step(i) between barrier + synchronize on both sides; a HIP event on the launch stream after every
    step gives the per-step GPU-side times.  Returns (elapsed_s, [step_ms])."""
    import torch
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    sync()
    if barrier:
        barrier()
    gc.disable()                                            # no collector pauses inside the timed region (the caller collects before its warm-up)
    t0 = time.perf_counter()
    evs[0].record()
    for i in range(steps):
        step(i)
        evs[i + 1].record()
    sync()
    if barrier:
        barrier()
    sync()
    elapsed = time.perf_counter() - t0
    gc.enable()
    return elapsed, [evs[i].elapsed_time(evs[i + 1]) for i in range(steps)]


def step_stats(ms):
    """Per-step times of a secondary line.  `outlier_steps`: steps of more than three medians (a shared box now and then stalls one step
    of a run for 20 - 60 ms -- seen on three of this round's boxes, on a different line each time; `frames_per_s` of the line is the plain
    mean and carries it, `steps_per_s_at_median_step` does not; a step is one frame except in the C4 / C5 iteration mode)."""
    if not ms:
        return {}
    med = percentile(ms, 0.5)
    return {"median": round(med, 4), "p10": round(percentile(ms, 0.1), 4), "p90": round(percentile(ms, 0.9), 4),
            "min": round(min(ms), 4), "max": round(max(ms), 4), "outlier_steps": sum(1 for x in ms if x > 3.0 * med),
            "steps_per_s_at_median_step": round(1e3 / med, 1) if med > 0 else None}


DUMP_BUDGET_BYTES = 60 << 20       # --dump-outputs: all files together stay below 64 MB (.npy headers included)
DUMP_MAX_ARRAY_BYTES = 4 << 20


def dump_outputs(out_dir, arrays):
    """--dump-outputs: write [(name, tensor)] as out_dir/<name>.npy, float32 (float64 stays float64, integers become float32).  An
    array above its share of DUMP_BUDGET_BYTES is reduced to a fixed sample of its flattened elements: sorted unique indices drawn
    with a seed that depends on the name and the size only, so every run with the same arguments writes the same elements."""
    import zlib
    import numpy as np
    import torch
    arrays = [(n, t) for n, t in arrays if t is not None]
    share = min(DUMP_MAX_ARRAY_BYTES, DUMP_BUDGET_BYTES // max(len(arrays), 1))
    os.makedirs(out_dir, exist_ok=True)
    written = {}
    for name, t in arrays:
        flat = t.detach().reshape(-1)
        dtype = torch.float64 if flat.dtype == torch.float64 else torch.float32
        cap = share // (8 if dtype == torch.float64 else 4)
        n = int(flat.numel())
        if n > cap:
            rng = np.random.default_rng(zlib.crc32(("%s:%d" % (name, n)).encode()))
            idx = np.unique(rng.integers(0, n, size=cap, dtype=np.int64))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        a = flat.to(dtype).cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), a)
        written[name] = {"shape": list(t.shape), "stored": int(a.size), "sampled": n > cap}
    return written


def quick_measure(config, steps, device, use_fs, variant="default", mode=None, with_stats=False, warm=15, cameras=1, graph=False, env=None):
    """frames/s of another workload in the same process (single GPU): secondary information next to the headline, never `value`.
    cameras: size of the camera pool cycled per step; graph: forward + backward replayed as one HIP graph per camera
    (adgs.graph); env: environment overrides for the duration of the measurement (e.g. the reference's call path:
    ADGS_BENCH_RAW_SH=0, ADGS_BENCH_RAW_SCENE=0)."""
    import torch
    from adgs import synthetic, _lib
    cfg = synthetic.CONFIGS[config]
    sc = build_scene(config, variant)
    env = dict(env or {})
    if mode:
        env["ADGS_RASTER_MODE"] = mode
        if mode == "classic":
            env["ADGS_BENCH_RAW_SH"] = "0"          # the raw-SH / raw-scene entries exist in the default pipeline only
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        pool = camera_pool(cfg, cameras)
        frames = frame_pool(sc, cfg, pool, device, use_fs)
        frame, cam = frames[0], pool[0][0]
        up = synthetic.make_upstream_grads(sc, 0)
        d = lambda t: t.to(device)
        ups = [d(up["color"]), d(up["depth"]), d(up["img_opacity"])] + ([d(up["flow"]), d(up["semantic"])] if use_fs else [])
        reruns0 = _lib.frame_status()["eager_reruns"]
        if graph:
            cache = graphed_steps(frames, ups)

            def step(i=0):
                cache(i % len(frames))
        else:
            def step(i=0):
                f = frames[i % len(frames)]
                torch.autograd.backward(f.forward(), ups)
                f.zero_grad()
        for i in range(max(warm, 2 * len(frames))):
            step(i)
        elapsed, ms = timed_loop(step, steps, torch.cuda.synchronize)
        res = {"workload": "%s%s: %d Gaussians, %dx%d, SH deg %d, %d dynamic objects" % (config, "" if variant == "default" else "/" + variant, cfg["P"], cfg["W"],
                                                                                         cfg["H"], cfg["sh_degree"], cfg["n_objects"]),
               "pipeline": mode or "v2", "frames_per_s": round(steps / elapsed, 1), "ms_per_step": round(elapsed / steps * 1e3, 4), "steps": steps,
               "cameras": len(frames), "launch": "HIP graph replay (one graph per camera)" if graph else "eager",
               "step_ms": step_stats(ms)}
        if graph:
            res["graph_replays_fitted_their_capacity"] = bool(cache.validate(repair=False))
        else:
            res["capacity_reruns"] = _lib.frame_status()["eager_reruns"] - reruns0
        if with_stats and not mode:
            frame.forward()
            st = _lib.frame_stats()
            E, R, E_pub, scanned = frame_work_figures(frame, make_settings(cfg, cam, sc, device), use_fs, device)
            T = st["tiles"]
            res.update({"reference_pairs_R": R, "cell_pairs_sorted": st["num_rendered"], "blended_entries": E, "published_entries": E_pub,
                        "E_over_R": round(E / max(R, 1), 4), "candidates_scanned_per_tile": round(scanned / max(T, 1), 1),
                        "entries_per_tile": round(E / max(T, 1), 1)})
        return res, frame, sc, cam, cfg, up
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def inference_measure(config, steps, device, cameras=16, graph=False, env_res=1024, warm=None):
    """Forward-only frames/s: the number the reference itself reports (render.py:52-55,86: `render(view, gaussians, env_map, pipeline)["render"]`
    clipped to [0, 1], under torch.no_grad() :156, FPS over the evaluation views) -- gaussian_renderer.render() on the HIP path: per-frame
    deformation, the forward-only rasterizer entry (adgs_raster_render_rawsh: no replay lists, no accumulator lines, no tile order), the
    environment map composited in the blend epilogue.  Every step renders another view of the pool (an evaluation renders every view once:
    the views' first renders are part of the warm-up only because the pool is cycled).  graph: one HIP graph per view (adgs.graph)."""
    import types
    import torch
    from adgs import synthetic, _lib, graph as adgs_graph
    from adgs.env import EnvironmentMap
    from adgs.model import SyntheticGaussianModel
    from gaussian_renderer import render
    cfg = synthetic.CONFIGS[config]
    sc = synthetic.to_z_up_world(build_scene(config))          # driving-dataset world frame: cameras look horizontally (examples/train_iteration.py)
    model = SyntheticGaussianModel.from_scene(sc, device=device, seed=0)
    model.raw_sh, model.raw_scene = True, True
    env_map = EnvironmentMap(env_res, 3, device=device)
    with torch.no_grad():
        env_map.grid_map.copy_(torch.rand(env_map.grid_map.shape, generator=torch.Generator().manual_seed(3)).to(device))
    pipe = types.SimpleNamespace(inv_depth=True, debug=False)
    cams = []
    for cam, t in camera_pool(cfg, cameras):
        c = synthetic.camera_object(synthetic.camera_to_z_up(cam), time=t)
        for name in ("world_view_transform", "full_proj_transform", "camera_center"):      # scene/cameras.py:77-80: the matrices live on the GPU
            setattr(c, name, getattr(c, name).to(device))
        c.cam_id = len(cams)          # scene/env.py:44-76 caches a camera's rays under its id
        cams.append(c)

    def view(k):
        def fn():
            with torch.no_grad():
                return torch.clip(render(cams[k], model, env_map, pipe)["render"], 0.0, 1.0)
        return fn
    fns = [view(k) for k in range(len(cams))]
    reruns0 = _lib.frame_status()["eager_reruns"]
    if graph:
        cache = adgs_graph.GraphCache(lambda k: fns[k], warmup=2)
        step = lambda i=0: cache(i % len(fns))
    else:
        step = lambda i=0: fns[i % len(fns)]()
    for i in range(warm if warm is not None else max(15, 2 * len(fns))):
        step(i)
    elapsed, ms = timed_loop(step, steps, torch.cuda.synchronize)
    res = {"workload": "%s forward-only: %d Gaussians, %dx%d, SH deg %d, %d dynamic objects, deformation + rasterizer + %d^2 x 6 environment map" % (
               config, cfg["P"], cfg["W"], cfg["H"], cfg["sh_degree"], cfg["n_objects"], env_res),
           "frames_per_s": round(steps / elapsed, 1), "ms_per_frame": round(elapsed / steps * 1e3, 4), "steps": steps, "views": len(fns),
           "launch": "HIP graph replay (one graph per view)" if graph else "eager", "step_ms": step_stats(ms)}
    if graph:
        res["graph_replays_fitted_their_capacity"] = bool(cache.validate(repair=False))
    else:
        res["capacity_reruns"] = _lib.frame_status()["eager_reruns"] - reruns0
    st = _lib.frame_status()
    res["fullest_slab_units"] = st["fullest_slab_units"]
    return res


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks from here (this process has not touched the GPU), relay
    their output and exit with their status."""
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


# ------------------------------------------------------------------ main
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--config", default="C3", help="BASELINE.json config: C1, C2, C3 (default), C4, C5")
    ap.add_argument("--cams-per-iter", type=int, default=0, help="iteration mode: cameras per iteration, dealt round-robin to the ranks (default: C4 3, C5 5)")
    ap.add_argument("--cams-per-rank", type=int, default=0, help="k cameras per GPU and step with ONE gradient exchange behind them (k x N cameras per iteration, dealt "
                    "round-robin: weak scaling with the exchange amortised over k renders; DESIGN.md section 6)")
    ap.add_argument("--densify-every", type=int, default=-1, help="iteration mode: densify/prune every k iterations inside the timed loop (default: C5 10, else off)")
    ap.add_argument("--cameras", type=int, default=int(os.environ.get("ADGS_BENCH_CAMERAS", "16")),
                    help="cameras / time stamps in the pool every GPU cycles through, one per step (train.py:55-61 draws a random camera per iteration); "
                         "1 = the same camera and time stamp every step (rounds 1-2).  Not used by the iteration configs C4 / C5")
    ap.add_argument("--graph", choices=["on", "off"], default=os.environ.get("ADGS_BENCH_GRAPH", "off"),
                    help="on: every camera's forward + backward is replayed as one HIP graph (adgs.graph; single GPU, not the iteration configs)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-flow-sem", action="store_true", help="render without the flow / semantic outputs")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the secondary single-GPU measurements (other configs, scene sensitivity)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: stage breakdown, roofline and HBM counters, CPU baseline and parity, multi-GPU "
                         "self-checks, secondary measurements (off: set-up, warm-up, the timed steps and the result line only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (images, radii, gradients) as DIR/<name>.npy")
    args = ap.parse_args()

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # the hosts only support dmabuf IPC: RCCL across processes needs this (set before HIP initialises)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args.gpus)
    import torch
    import torch.distributed as dist
    from adgs import _lib, synthetic, dp

    if os.environ.get("ADGS_BENCH_WATCHDOG"):              # debugging aid: dump every thread's stack and exit if the run takes longer than N seconds
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["ADGS_BENCH_WATCHDOG"]), exit=True)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    # ADGS_BENCH_BACKEND=gloo: control-flow dry run of the multi-rank path on a box with fewer GPUs than ranks (ranks share devices,
    # collectives go through the host); never a measurement
    backend = os.environ.get("ADGS_BENCH_BACKEND", "nccl")
    dev_index = local_rank if backend == "nccl" else local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    force_coll = world == 1 and os.environ.get("ADGS_BENCH_FORCE_COLLECTIVES") == "1"   # 1-GPU dry run of the N-GPU step: the
    if world > 1 or force_coll:                                                          # collectives run in a one-rank RCCL group
        if force_coll:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29571")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)   # nccl == RCCL on ROCm
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    if _lib.lib().adgs_device_check() != 0:
        raise SystemExit(_lib.last_error())

    cfg = synthetic.CONFIGS[args.config]
    sc = build_scene(args.config)
    H, W, P = cfg["H"], cfg["W"], cfg["P"]
    use_fs = not args.no_flow_sem
    d = lambda t: t.to(device)
    up = synthetic.make_upstream_grads(sc, 0)
    up_list = [d(up["color"]), d(up["depth"]), d(up["img_opacity"])] + ([d(up["flow"]), d(up["semantic"])] if use_fs else [])
    sync = torch.cuda.synchronize
    barrier = dist.barrier if world > 1 else None

    # ---- which cameras does a step render?
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    if args.cams_per_rank > 0:
        if args.cams_per_iter > 0 or args.config in ITERATION_CONFIGS:
            raise SystemExit("--cams-per-rank is the weak-scaling form of --cams-per-iter: give one of them, on C3")
        args.cams_per_iter = args.cams_per_rank * world_env
    iteration_mode = args.config in ITERATION_CONFIGS or args.cams_per_iter > 0
    if iteration_mode and cfg["n_objects"] == 0:
        raise SystemExit("--cams-per-iter needs a dynamic config (C3, C4, C5)")
    if iteration_mode:
        n_cams = args.cams_per_iter or ITERATION_CONFIGS.get(args.config, {}).get("cams", world)
        densify_every = args.densify_every if args.densify_every >= 0 else ITERATION_CONFIGS.get(args.config, {}).get("densify_every", 0)
        cam_ids = list(range(n_cams))
        cam_times = [0.37 if n_cams == 1 else 0.1 + 0.8 * c / (n_cams - 1) for c in cam_ids]
    else:
        n_cams, densify_every = world, 0
    pool_k = 1 if iteration_mode else max(1, args.cameras)
    frames, model = [], None
    if iteration_mode:
        cams = [synthetic.make_camera(W, H, cfg["focal"], cam_seed=c) for c in cam_ids]
        my = [i for i in range(len(cams)) if i % world == rank]
        for i in my:
            f = make_frame(sc, cfg, cams[i], device, use_fs, t=cam_times[i], model=model)
            model = getattr(f, "model", None)
            frames.append(f)
        my_pool = None
        canonical_cam = cams[my[0]] if my else None
    else:
        # every rank cycles through its own pool of cameras / time stamps, one per step: rank r's entry k is camera r + world * k
        # (rank 0's entry 0 is the canonical SURVEY.md 8(d) camera at t = 0.37); a step renders entry `it % pool_k` on every rank
        pools = [camera_pool(cfg, pool_k, first=r, stride=world) for r in range(world)]
        my_pool = frame_pool(sc, cfg, pools[rank], device, use_fs)
        frames = [my_pool[0]]                         # what the statistics after the timed region look at
        model = getattr(my_pool[0], "model", None)
        canonical_cam = pools[rank][0][0]
    if not frames:                                    # a rank without a camera in this deal (C4 on 4 GPUs) still owns a replica
        from adgs.model import SyntheticGaussianModel
        model = SyntheticGaussianModel.from_scene(sc, device, seed=0)
        model.raw_sh = os.environ.get("ADGS_BENCH_RAW_SH", "1") != "0"
        model.raw_scene = os.environ.get("ADGS_BENCH_RAW_SCENE", "1") != "0"
    frame = frames[0] if frames else None
    dynamic = cfg["n_objects"] > 0
    params = (lambda: model.parameters()) if dynamic else (lambda: frame.parameters())

    # Gradient exchange of the multi-GPU step.  Default on the raw-SH path: the SH gradients travel in
    # factored form (one all-gather of 12 B per Gaussian and camera + ONE reduction of the dense remainder + a local expansion);
    # ADGS_DP_EXCHANGE=dense all-reduces every materialised gradient instead.  ADGS_DP_COLLECTIVE=rs_ag: the dense reduction as
    # reduce-scatter + all-gather.  ADGS_BENCH_FACTORED=1 runs the factored step on one GPU with one camera as well.
    multi = world > 1 or force_coll or n_cams > 1
    factored = (dynamic and model.raw_sh and os.environ.get("ADGS_DP_EXCHANGE", "factored") != "dense"
                and (multi or os.environ.get("ADGS_BENCH_FACTORED") == "1"))
    exchange, ex = "none", None
    ex_events = []
    if factored:
        fused = (frame.fused_flow if frame is not None else os.environ.get("ADGS_BENCH_FUSED_FLOW", "1") != "0")
        ex = dp.FactoredSHExchange(model, factor_xyz=(fused or not use_fs) and os.environ.get("ADGS_DP_FACTOR_XYZ", "1") != "0")
        ex.force_collectives = force_coll
        ex.timing = []
        if iteration_mode:
            ex_args = [(cam_times, [c["campos"].tolist() for c in cams], [t + 0.05 if use_fs else None for t in cam_times])]
        else:             # step k: the cameras all ranks render in that step
            ex_args = [([pools[r][k][1] for r in range(world)], [pools[r][k][0]["campos"].tolist() for r in range(world)],
                        [pools[r][k][1] + 0.05 if use_fs else None for r in range(world)]) for k in range(pool_k)]
        exchange = "factored SH%s gradients: all-gather of the factors + %s of the dense remainder + local expansion" % (
            " and xyz-deformation" if ex.factor_xyz() else "", "reduce-scatter + all-gather" if os.environ.get("ADGS_DP_COLLECTIVE") == "rs_ag" else "all-reduce")
    elif world > 1:
        exchange = "dense all-reduce of every parameter gradient"
    elif n_cams > 1:
        exchange = "none (one GPU: plain accumulation over the cameras)"

    # densify / prune inside the loop (C5): needs the optimizer-state surgery, i.e. a model with training_setup() and Adam moments
    densify_events = []
    if densify_every:
        from adgs import densify as _densify
        model.training_setup(lrs={n: 0.0 for n in _densify.GROUP_ATTR}, scene_extent=20.0, object_extent=4.0)      # lr 0: the scene stays put, the moments exist
        if ex is not None:
            ex._arena_setup()
    densify_thr = [None]

    # ADGS_BENCH_STREAMS=S (default 1): the cameras of an iteration on S side streams (step() below)
    side_streams = [torch.cuda.Stream(device) for _ in range(int(os.environ.get("ADGS_BENCH_STREAMS", "1")))] if int(os.environ.get("ADGS_BENCH_STREAMS", "1")) > 1 else None
    use_graph = args.graph == "on"
    if use_graph and (world > 1 or force_coll or iteration_mode or factored):
        raise SystemExit("--graph on: single GPU, one camera per step (the exchange of the multi-GPU step is issued eagerly)")
    cache = graphed_steps(my_pool, up_list) if use_graph else None

    def param_names():
        """Names of params(), in its order (the gradients a graph replay returns come in the same order)."""
        if dynamic:
            from adgs.model import _RAW
            return [n.lstrip("_") for n in _RAW if getattr(model, n, None) is not None and getattr(model, n).numel() > 0]
        return list(frame.leaf.keys())

    # --dump-outputs: step `dump_at[0]` (the last timed one) keeps references to what it hands its caller; nothing is copied in the step
    dump_at, captured = [-1], {"cams": [], "grads": []}

    def step(it=0, eager=False):
        keep = it == dump_at[0]
        if cache is not None and not eager:
            grads = cache(it % pool_k)
            if keep:
                captured["grads"] = list(zip(param_names(), grads))
            return
        if factored:
            ex.begin(n_cams)                     # the all-gather starts from inside the backward, as soon as the last factor exists
        def one_camera(f):
            outs = f.forward(sink_for=ex.sink_for if factored else None)
            torch.autograd.backward(outs, up_list)
            if keep:
                captured["cams"].append((outs, f.last_radii, f.last_means2D.grad if isinstance(f, DeformFrame) else f.means2D.grad))
            if densify_every:
                with torch.no_grad():
                    model.add_densification_stats(dict(viewspace_points=f.last_means2D, radii=f.last_radii))
        if side_streams and iteration_mode and len(frames) > 1:
            # The cameras of an iteration are independent until the gradient sum (train.py:55-61,74): camera i runs on side stream i mod S,
            # forward and backward (autograd runs a backward on its forward's stream).  The host enqueues them in order -- a forward returns
            # once its binning totals are known -- so what overlaps on the GPU is one camera's blend tail / backward with the next camera's
            # deformation, preprocess and binning.  Gradients accumulate into the shared .grad tensors: autograd
            # orders the accumulation across streams; the exchange / optimizer wait for both streams.
            main = torch.cuda.current_stream()
            for s_ in side_streams:
                s_.wait_stream(main)
            for i, f in enumerate(frames):
                with torch.cuda.stream(side_streams[i % len(side_streams)]):
                    one_camera(f)
            for s_ in side_streams:
                main.wait_stream(s_)
        else:
            for f in (frames if iteration_mode else [my_pool[it % pool_k]]):
                one_camera(f)
        if factored:
            ct, cp, ft = ex_args[0 if iteration_mode else it % pool_k]
            ex.reduce(ct, cp, flow_times=ft)
        elif world > 1 or force_coll:
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            dp.allreduce_gradients(params(), force=force_coll)
            e1.record()
            ex_events.append((e0, e1))
        if keep:                                 # the exchanged gradients, before a densify step replaces the parameters
            captured["grads"] = list(zip(param_names(), [p.grad for p in params()]))
        if densify_every and (it + 1) % densify_every == 0:
            with torch.no_grad():
                e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                dp.allreduce_densification_stats(model.xyz_gradient_accum, model.denom, model.max_radii2D)
                dp.seed_all_ranks(1000 + it)
                if densify_thr[0] is None:           # threshold: the 99.9th percentile of the accumulated screen-space gradient, so that
                    # every densify step clones / splits about 0.1 % of the Gaussians and the scene keeps its size over the run
                    g = (model.xyz_gradient_accum / model.denom.clamp_min(1)).reshape(-1)
                    thr = torch.quantile(g[g > 0][:2_000_000], 0.999) if bool((g > 0).any()) else torch.tensor(1.0, device=device)
                    if world > 1:
                        dist.broadcast(thr, src=0)
                    densify_thr[0] = float(thr)
                model.densify_and_prune(densify_thr[0], densify_thr[0], 0.005, False)
                e1.record()
                densify_events.append((e0, e1))
        if dynamic:
            model.zero_grad()
        else:
            frame.zero_grad()

    if densify_every:                                 # Adam moments must exist for the optimizer-state surgery (one untimed step)
        for f in frames:
            torch.autograd.backward(f.forward(), up_list)
        if world > 1:
            dp.allreduce_gradients(params())
        model.optimizer.step(zero_grad=True)

    it_counter = [0]

    def run(n, eager=False):
        for _ in range(n):
            step(it_counter[0], eager); it_counter[0] += 1
    # Stage breakdown (every stage timed with HIP events) on the last warm-up steps, together with the event-to-event time of those
    # steps: step time - sum of the stage times = what the GPU spent NOT running this library's kernels (launch gaps, host waits,
    # torch's own small kernels).  The timed region below only keeps the events around the dominant kernel, because every timed
    # stage leaves a ~10 us bubble in the queue.
    # Order of the W warm-up steps: the profiled ones FIRST, then every piece of host-side set-up of the timed region (event pools,
    # reading the stage events back, a garbage collection), then the remaining plain warm-up steps, then the timed region at once:
    # a GPU left idle for the milliseconds that set-up takes runs its next step up to 1 ms slower (clocks), which is 3.5 % of a
    # 20-step run when it lands inside it.  A plain run (no --full) reports no stage times: it brackets nothing, neither in the warm-up
    # nor in the timed region.
    stages_all, dom, gpu_idle, stage_step_ms = None, None, None, None
    n_prof = min(4, args.warmup // 2) if args.full else 0
    if os.environ.get("ADGS_BENCH_SETTLE", "1") != "0":
        run(max(8, 2 * pool_k))                       # set-up: every camera of the pool rendered (capacity hints, allocator, the cameras' tile-order hints) before anything is measured
        sync()
    if n_prof > 0:
        sync()
        wprof = _lib.StageProfiler()
        wprof.reserve(64 * n_prof)
        wprof.enable(True)
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n_prof + 1)]
        evs[0].record()
        for i in range(n_prof):
            run(1, eager=True)                         # stage events cannot be recorded inside a graph replay
            evs[i + 1].record()
        sync()
        wprof.enable(False)
        stages_all = wprof.collect()
        prof_step_ms = sum(evs[i].elapsed_time(evs[i + 1]) for i in range(n_prof)) / n_prof
        per_step = {k: v[0] * v[1] / n_prof for k, v in stages_all.items()}
        stage_step_ms = {k: (round(v, 4), stages_all[k][1] // n_prof) for k, v in per_step.items() if stages_all[k][1] > 0}
        gpu_idle = {"profiled_step_ms": round(prof_step_ms, 4), "sum_of_stage_ms": round(sum(per_step.values()), 4),
                    "gpu_not_in_adgs_kernels_ms": round(prof_step_ms - sum(per_step.values()), 4),
                    "note": "from %d warm-up steps with every stage bracketed by HIP events (each bracket adds a bubble: an upper bound)" % n_prof}
        dom = max(stages_all, key=lambda k: stages_all[k][0] * max(stages_all[k][1], 1))
    prof = None
    if args.full:
        prof = _lib.StageProfiler()
        prof.reserve(2 * args.steps * max(len(frames), 1) * (1 if dom else 11) + 64)      # no event creation inside the timed region
    gc.collect()
    # Settle phase (setup, not a measurement), AFTER every piece of host-side set-up and right in front of the warm-up steps: the GPU must come
    # into the timed region busy.  (Until round 5 the settle windows ran first and the stage-profile read-back + garbage collection came after
    # them: at the driver's --warmup 5 only three plain steps separated that idle gap from the timed region, whose steps then ran 3 - 4 % slower
    # than steady state -- 1.075 against 1.03 ms medians -- while the clocks came back.)  A fresh process on a fresh box shows one-off stalls of 0.1-0.6 s in its first
    # second (driver / allocator / clock ramp).  Windows of 20 untimed steps run until two consecutive windows agree within 10 %
    # (at most 8 windows), then the contract's W warm-up steps and K timed steps follow unchanged.
    # --dump-outputs with densify/prune in the loop: the model at the dumped step depends on how many densify calls ran before it, so
    # the settle phase then always runs all of its windows (a fixed number of steps before the timed region)
    fixed_settle = bool(args.dump_outputs and densify_every)
    settle_steps = 0
    if os.environ.get("ADGS_BENCH_SETTLE", "1") != "0":
        prev_w, agree = None, 0
        win = max(20, pool_k)                      # a window sees every camera of the pool
        for _ in range(8):
            t_w = time.perf_counter()
            run(win)
            settle_steps += win
            sync()
            w = time.perf_counter() - t_w
            if world > 1:             # every rank must run the SAME number of windows: decide on the maximum over the ranks
                tw = torch.tensor([w], device=device, dtype=torch.float64)
                dist.all_reduce(tw, op=dist.ReduceOp.MAX)
                w = float(tw.item())
            agree = agree + 1 if (prev_w is not None and abs(w - prev_w) <= 0.1 * min(w, prev_w)) else 0
            prev_w = w
            if agree >= 2 and not fixed_settle:
                break
    # the timed region starts at pool entry 0 whatever the number of settle windows: step k of it renders entry k mod pool_k, in every run
    align = -(it_counter[0] + args.warmup - n_prof) % pool_k
    run(align)
    settle_steps += align
    run(args.warmup - n_prof)
    if prof is not None:
        prof.enable(True, stages=[dom] if dom else None)       # --warmup 0: no breakdown yet, time every stage (a mask store: no gap)
    if ex is not None:
        ex.timing = []
    del ex_events[:]; del densify_events[:]
    reruns0 = _lib.frame_status()["eager_reruns"]
    dump_at[0] = it_counter[0] + args.steps - 1
    elapsed, step_ms = timed_loop(lambda i: run(1), args.steps, sync, barrier)
    dump_at[0] = -1
    stages = None
    if prof is not None:
        prof.enable(False)
        stages = prof.collect()
    capacity_reruns = _lib.frame_status()["eager_reruns"] - reruns0
    graph_ok = cache.validate(repair=False) if cache is not None else None
    dumped = None
    if args.dump_outputs and rank == 0:
        arrays = []
        for k, (outs, radii, g2d) in enumerate(captured["cams"]):
            pre = "" if len(captured["cams"]) == 1 else "cam%d_" % k
            arrays += list(zip([pre + n for n in ("color", "depth", "opacity", "flow", "semantic")], outs))
            arrays += [(pre + "radii", radii), (pre + "grad_means2D", g2d)]
        arrays += [("grad_" + n, g) for n, g in captured["grads"]]
        last = it_counter[0] - 1
        if iteration_mode:
            cams_dumped = [{"camera": i, "t": round(cam_times[i], 6)} for i in my]
        else:
            k = last % pool_k
            cams_dumped = [{"pool_entry": k, "camera": rank + world * k, "t": round(pools[rank][k][1], 6)}]
        dumped = {"dir": args.dump_outputs, "timed_step": args.steps - 1, "cameras": cams_dumped,
                  "P_after_step": int(model.get_pts_num) if dynamic else P, "arrays": dump_outputs(args.dump_outputs, arrays)}
    captured["cams"], captured["grads"] = [], []
    multi_gpu = None
    if (world > 1 or force_coll) and args.full:
        # Self-verifying multi-GPU figures (for the day a multi-GPU node runs this): the rank count RCCL itself reports (an
        # all-reduce of ones), every rank's own time per step and pair counts (cameras differ: load imbalance), and the exchange
        # timed with BOTH forms of the dense reduction in this one run (a short untimed loop with the other form).
        ones = torch.ones(1, device=device, dtype=torch.float32)
        dist.all_reduce(ones)
        st_r = _lib.frame_status()
        mine = torch.tensor([elapsed / args.steps * 1e3, float(st_r["pairs"]), float(st_r["fine_pairs"]), float(capacity_reruns)], device=device, dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        multi_gpu = {"world_size": dist.get_world_size(), "rccl_ranks": int(round(float(ones.item()))), "backend": dist.get_backend(),
                     "per_rank_ms_per_step": [round(float(x[0]), 4) for x in allr], "per_rank_cell_pairs_last_frame": [int(x[1]) for x in allr],
                     "per_rank_fine_pairs_last_frame": [int(x[2]) for x in allr], "per_rank_capacity_reruns": [int(x[3]) for x in allr]}
        main_form = "rs_ag" if os.environ.get("ADGS_DP_COLLECTIVE") == "rs_ag" else "all_reduce"

        def exchange_summary():
            if ex is not None and ex.timing:
                tm = ex.timing
                avg = lambda a, b: round(sum(t_[a].elapsed_time(t_[b]) for t_ in tm) / len(tm), 4)
                return {"total": avg(0, 3), "allgather_wait": avg(0, 1), "expansion": avg(1, 2), "dense_reduction_wait": avg(2, 3), "calls": len(tm)}
            if ex_events:
                return {"total": round(sum(a.elapsed_time(b) for a, b in ex_events) / len(ex_events), 4), "calls": len(ex_events)}
            return None
        sync()
        by_form = {main_form: exchange_summary()}
        saved_timing, saved_events = (list(ex.timing) if ex is not None else None), list(ex_events)
        other = "all_reduce" if main_form == "rs_ag" else "rs_ag"
        old_form = os.environ.get("ADGS_DP_COLLECTIVE")
        os.environ["ADGS_DP_COLLECTIVE"] = other
        try:
            if ex is not None:
                ex.timing = []
            del ex_events[:]
            run(min(10, max(2, args.steps)))
            sync()
            by_form[other] = exchange_summary()
        finally:
            if old_form is None:
                os.environ.pop("ADGS_DP_COLLECTIVE", None)
            else:
                os.environ["ADGS_DP_COLLECTIVE"] = old_form
            if ex is not None:
                ex.timing = saved_timing
            ex_events[:] = saved_events
        multi_gpu["exchange_ms_by_collective"] = by_form
        multi_gpu["note"] = "exchange_ms_by_collective[%s] is from the timed region, the other form from %d extra steps after it" % (main_form, min(10, max(2, args.steps)))
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if rank == 0:
        cams_per_step = n_cams if iteration_mode else world
        fps = args.steps * cams_per_step / elapsed
        result = {
            "metric": "fwd+bwd frames/s",
            "value": round(fps, 3), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "strong" if (iteration_mode and not args.cams_per_rank) else "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        }
        config = {"workload": "%s: %d Gaussians, %dx%d, SH deg %d, %d dynamic objects%s, %s" % (
            args.config, P, W, H, cfg["sh_degree"], cfg["n_objects"], ", flow+semantic outputs" if use_fs else "",
            ("%d cameras/iteration dealt round-robin over %d GPU(s)%s" % (n_cams, world, ", densify/prune every %d iterations" % densify_every if densify_every else ""))
            if iteration_mode else "1 camera/GPU/step"),
            "P": P, "cameras_per_step": cams_per_step,
            "camera_pool": ("%d cameras / time stamps per GPU, cycled one per step (train.py:55-61)" % pool_k) if not iteration_mode else "the iteration's cameras, every step",
            "settle_steps": settle_steps, "capacity_reruns": capacity_reruns, "library_sha256_16": library_stamp(),
            "forward_tile_order": {"0": "top-down", "1": "bottom-up"}.get(os.environ.get("ADGS_FWD_ORDER", "2"),
                                                                          "longest lists first by the previous render of the same camera (bottom-up for a camera's first render); "
                                                                          "the pool's cameras return every %d steps with unchanged parameters, a training run returns once per epoch" % pool_k),
            "launch": ("HIP graph replay, one graph per camera (adgs.graph); every replay fitted its capacity: %s" % graph_ok) if use_graph else "eager",
            "parallelism": "dp%d (camera-parallel over RCCL)" % world if world > 1 else "single GPU", "gradient_exchange": exchange,
            "camera_streams": len(side_streams) if (side_streams and iteration_mode) else 1,
            "step_ms_hip_events": dict(step_stats(step_ms), first=round(step_ms[0], 4))}
        if os.environ.get("ADGS_BENCH_DUMP_STEPS"):
            config["step_ms_series"] = [round(x, 4) for x in step_ms[:int(os.environ["ADGS_BENCH_DUMP_STEPS"])]]
        if multi_gpu:
            config["multi_gpu"] = multi_gpu
        if gpu_idle:
            # the same figure against the UNPROFILED steps of the timed region (no event brackets, hence no bubbles of their own)
            gpu_idle["timed_step_median_minus_sum_of_stage_ms"] = round(percentile(step_ms, 0.5) - gpu_idle["sum_of_stage_ms"], 4)
            config["gpu_idle"] = gpu_idle
        # ---- exchange / densify times (HIP events on rank 0's launch stream)
        if ex is not None and ex.timing:
            tm = ex.timing
            avg = lambda a, b: round(sum(t_[a].elapsed_time(t_[b]) for t_ in tm) / len(tm), 4)
            config["exchange_ms"] = {"total": avg(0, 3), "allgather_wait": avg(0, 1), "expansion": avg(1, 2), "dense_reduction_wait": avg(2, 3), "calls": len(tm),
                                     "note": "waits seen by the launch stream: the all-gather starts inside the backward, the expansion runs under the dense reduction"}
        elif ex_events:
            config["exchange_ms"] = {"total": round(sum(a.elapsed_time(b) for a, b in ex_events) / len(ex_events), 4), "calls": len(ex_events)}
        if densify_events:
            dms = [a.elapsed_time(b) for a, b in densify_events]
            config["densify_ms"] = {"mean": round(sum(dms) / len(dms), 4), "calls": len(dms), "P_end": int(model.get_pts_num),
                                    "ms_per_step_excl_densify": round((elapsed * 1e3 - sum(dms)) / args.steps, 4)}
        if dumped is not None:
            config["dumped_outputs"] = dumped
        roof = None
        if frame is not None and args.full:
            outs = frame.forward()
            stats = _lib.frame_stats()
            V = int((frame.last_radii > 0).sum().item())
            Rc = stats["num_rendered"]                # pairs that were sorted: (cell, Gaussian) in v2, (tile, Gaussian) in classic mode
            X, T = H * W, stats["tiles"]
            Pn = int(frame.last_radii.shape[0])
            M = sc["shs"].shape[1]
            F, D_S = (1, 1) if use_fs else (0, 0)
            v2 = _lib.lib().adgs_raster_needs_zero_init(D_S) == 0
            settings = make_settings(cfg, canonical_cam, sc, device)
            if v2:
                # scene-level work figures: the reference's pair count R and what v2 actually blends -- for the
                # canonical camera, and (what the per-launch byte figures of the roofline use) the mean over the camera pool the
                # timed steps cycled through
                pool_fig = None
                if os.environ.get("ADGS_BENCH_SKIP_STATS"):           # PMC passes: keep foreign launches out of the counter totals
                    E, R_ref, E_pub, scanned = 0, 0, 0, 0
                else:
                    try:
                        E, R_ref, E_pub, scanned = frame_work_figures(frame, settings, use_fs, device)
                        if my_pool is not None and len(my_pool) > 1:
                            figs = [frame_work_figures(f, make_settings(cfg, c, sc, device), use_fs, device, with_ref=False, full=True)
                                    for f, (c, _t) in zip(my_pool, pools[rank])]
                            mean = lambda j: sum(x[j] for x in figs) / len(figs)
                            pool_fig = {"cameras": len(figs), "blended_entries": round(mean(0)), "published_entries": round(mean(2)), "P_visible": round(mean(4)),
                                        "cell_pairs_sorted": round(mean(5)), "published_entries_min_max": [min(x[2] for x in figs), max(x[2] for x in figs)],
                                        "cell_pairs_sorted_min_max": [min(x[5] for x in figs), max(x[5] for x in figs)]}
                    except Exception as exc:                 # statistics only
                        print("bench: scene statistics failed: %r" % (exc,), file=sys.stderr)
                        E, R_ref, E_pub, scanned = 0, 0, 0, 0
                if pool_fig:
                    ab = alg_bytes_v2(Pn, pool_fig["P_visible"], pool_fig["cell_pairs_sorted"], pool_fig["blended_entries"], X, T, M, F, D_S, stats["sort_passes"],
                                      pool_fig["published_entries"], bucket=bool(stats.get("bucket_binning")), ddir=os.environ.get("ADGS_BENCH_RAW_SH", "1") != "0")
                    config["camera_pool_work"] = pool_fig
                else:
                    ab = alg_bytes_v2(Pn, V, Rc, E, X, T, M, F, D_S, stats["sort_passes"], E_pub, bucket=bool(stats.get("bucket_binning")), ddir=os.environ.get("ADGS_BENCH_RAW_SH", "1") != "0")
                config.update({"pipeline": "v2 (coarse cells, %s, lazy per-tile filtering)" % ("bucket binning: per-cell depth buckets sorted inside one CU each"
                                                                                                if stats.get("bucket_binning") else "device-wide radix sort of (cell | depth) keys"), "P_visible": V, "tiles": T, "reference_pairs_R": R_ref,
                               "R_over_P": round(R_ref / max(Pn, 1), 2), "cell_pairs_sorted": Rc, "fine_pairs_bound": stats["fine_pairs"], "blended_entries": E,
                               "published_entries": E_pub, "E_over_R": round(E / max(R_ref, 1), 4), "mean_entries_per_tile": round(E / max(T, 1), 1),
                               "candidates_scanned_per_tile": round(scanned / max(T, 1), 1)})
            else:
                ab = alg_bytes(Pn, V, Rc, X, T, M, F, D_S, stats["sort_passes"])
                config.update({"pipeline": "classic (reference stage order)", "P_visible": V, "tiles": T, "reference_pairs_R": Rc, "R_over_P": round(Rc / max(Pn, 1), 2)})
            frame_bytes = sum(ab.values()) + frame.deform_bytes
            config["deformation"] = frame.deform_desc
            # HBM accounting (never to be conflated): the algorithmic bytes of THIS pipeline and, when
            # committed for this build, the PMC-measured bytes.  The north star's ">= 40 % of the HBM roofline" is NOT met by
            # either: more than half of the frame is spent in the two blend kernels, which are fp32-VALU-issue bound.
            fps_rank0 = args.steps * len(frames) / elapsed          # frames this GPU rendered per second
            config.update({"alg_bytes_per_frame": int(frame_bytes), "frame_hbm_frac_of_8TBs": round(frame_bytes * fps_rank0 / 1e9 / HBM_PEAK_GBS, 4)})
            config.update(committed_frame_traffic(args.config, use_fs and v2 and not iteration_mode, fps_rank0))
            if stages_all is None:
                stages_all = stages
                dom = max(stages, key=lambda k: stages[k][0] * max(stages[k][1], 1))
            # HIP events on the launch stream, over the timed region.  A stage can hold several event brackets per frame (preprocess_fwd: the
            # sh0 kernel and the preprocess kernel; render_fwd: the blend and the tile order) while `ab[dom]` is the stage's bytes per FRAME: the
            # time that belongs to them is the stage's time per frame (mean per bracket x brackets per frame), not the mean per bracket
            # (`bench_c5_1gpu.json` printed 7.1 TB/s = 0.89 for a two-launch stage).
            roof_src = stages
            roof_timing = "HIP events around the kernel in every step of the timed region"
            frames_timed = args.steps * max(len(frames), 1)
            if use_graph:                             # no event can be recorded inside a graph replay
                roof_src, frames_timed = stages_all, n_prof * max(len(frames), 1)
                roof_timing = "HIP events around the kernel in the eager warm-up steps (the timed region replays HIP graphs)"
            roof = dominant_roofline(dom, ab.get(dom, 0), roof_src[dom][0], roof_src[dom][1], frames_timed)
            roof["timing"] = roof_timing
            dom_ms = roof["avg_launch_ms"]
            roof.update(committed_pmc(dom, args.config, use_fs and v2))
            if world == 1 and not force_coll and not iteration_mode and not use_graph and args.config == "C3" and use_fs and v2:
                live = measure_traffic_in_run(dom, args.config)
                if live:
                    roof.update(live)
                else:
                    roof["traffic_measured_in_run"] = False      # rocprofv3 absent / ADGS_BENCH_PMC=0 / a pass failed: `traffic` is the committed replay
            if v2 and dom in ("render_fwd", "render_bwd"):
                roof["pixel_entry_evals_per_s"] = round((config["published_entries"] if dom == "render_bwd" else config["blended_entries"]) * 256 / (dom_ms * 1e-3), 1)
            result["config"] = config
            result["roofline"] = roof
            # ms per STEP of every stage (HIP events, all stages timed: from the last warm-up steps).  A stage can hold several launches per
            # step (preprocess_fwd: the sh0 kernel and the preprocess kernel); until round 3 this field held the mean per LAUNCH, i.e. half
            # of that stage's time -- the "83 us bracket around a 111 us kernel" of VERDICT r3 was the mean of 52 us and 107 us.
            if stage_step_ms is None:
                stage_step_ms = {k: (round(v[0] * v[1] / max(args.steps, 1), 4), v[1] // max(args.steps, 1)) for k, v in stages_all.items() if v[1] > 0}
            result["stages_ms"] = {k: v[0] for k, v in stage_step_ms.items()}
            result["stage_launches_per_step"] = {k: v[1] for k, v in stage_step_ms.items()}
            # every stage against the HBM roofline: algorithmic bytes per step over the stage's HIP-event time per step,
            # cross-checked against the rocprofv3 kernel-trace averages of the committed profile of this build where one exists
            # (tools/stage_cache_experiment.py explains the few percent by which the serialised, profiled run is slower)
            kstats = committed_kernel_stats()
            result["stage_rooflines"] = {}
            ab_stage = dict(ab)
            if isinstance(frame, DeformFrame) and frame.model.raw_sh:
                # the stage holds the sh0 kernel too (coefficient 0 = dc + f_shs(t) from the raw tensors): dc in, deformation rows in, [N,3] out;
                # in the frame total these bytes are part of `deformation` (deform_bytes_per_frame), here they belong to the stage's time
                m = frame.model
                ab_stage["preprocess_fwd"] += 4 * (m.shs_deform_param_scene.numel() + m.shs_deform_param_obj.numel()) + Pn * 24
            for k, (ms, _) in stage_step_ms.items():
                if ms > 0 and k in ab:
                    r = {"alg_bytes": int(ab_stage.get(k, 0)), "ms_per_step": ms, "GB/s": round(ab_stage.get(k, 0) / (ms * 1e-3) / 1e9, 1),
                         "frac_of_8TBs": round(ab_stage.get(k, 0) / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
                    if k in kstats:
                        r["rocprof_ms_per_step"] = kstats[k]["ms"]; r["rocprof_kernels"] = kstats[k]["kernels"]
                        r["rocprof_frac_of_8TBs"] = round(ab_stage.get(k, 0) / (kstats[k]["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
                    result["stage_rooflines"][k] = r
        else:
            result["config"] = config
        secondary = args.full and world == 1 and not force_coll and not args.no_secondary and args.config == "C3" and not iteration_mode
        if secondary:
            # the other single-GPU configs of BASELINE.json, same build, same process (secondary: `value` stays the C3 headline), the
            # mandatory C1 CPU baseline (OpenMP and single thread), and the scene-sensitivity lines: two C3-sized scenes that do NOT
            # saturate early, default pipeline against the reference-order ("classic") pipeline
            try:
                others = []
                K = max(1, args.cameras)
                r1, f1, sc1, cam1, cfg1, up1 = quick_measure("C1", 300, device, use_fs, cameras=K)
                if not args.no_cpu_baseline:
                    upn = {k: v.numpy() for k, v in up1.items()}
                    r1["cpu_baseline_openmp"], _ = cpu_baseline(sc1, cam1, cfg1, use_fs, upn)
                    r1["cpu_baseline_single_thread"], _ = cpu_baseline(sc1, cam1, cfg1, use_fs, upn, threads=1)
                others.append(r1)
                del f1
                others.append(quick_measure("C2", 300, device, use_fs, cameras=K)[0])
                # the same two workloads with every camera's frame replayed as one HIP graph: what a launch-bound frame gains when the
                # forward needs no host decision in its middle (adgs.graph; rasterizer_impl.cu:288 makes this impossible for the reference)
                for c in ("C1", "C2"):
                    try:
                        others.append(quick_measure(c, 300, device, use_fs, cameras=K, graph=True)[0])
                    except Exception as exc:
                        others.append({"workload": c, "launch": "HIP graph replay", "failed": repr(exc)})
                    gc.collect(); torch.cuda.empty_cache()
                result["other_configs"] = others
                # C3 as a maintainer gets it who swaps ONLY the rasterizer submodule: gaussian_renderer/__init__.py:76-86 unchanged, i.e.
                # GaussianRasterizer.forward with the materialised [N,16,3] SH tensor and torch-side cat / exp / sigmoid / normalize
                # (scene/gaussian_model.py:89-152) -- no raw-SH / raw-scene entry points
                try:
                    result["reference_api_path"] = quick_measure("C3", 100, device, use_fs, cameras=K, env={"ADGS_BENCH_RAW_SH": "0", "ADGS_BENCH_RAW_SCENE": "0"})[0]
                    result["reference_api_path"]["note"] = ("the reference's unchanged call path (materialised SH, activations in the deformation pass): what swapping "
                                                            "only the rasterizer submodule gives; `value` uses this repository's render() path (raw-SH + raw-scene entries)")
                    gc.collect(); torch.cuda.empty_cache()
                    result["c3_graph_replay"] = quick_measure("C3", 100, device, use_fs, cameras=K, graph=True)[0]
                    gc.collect(); torch.cuda.empty_cache()
                except Exception as exc:
                    result["reference_api_path"] = "failed: %r" % (exc,)
                # forward-only frames/s: the reference's own reported number (eval render FPS, render.py:52-55,86 under no_grad :156)
                try:
                    inf = []
                    for c, n in (("C3", 200), ("C2", 300), ("C1", 300)):
                        for g in (False, True):
                            try:
                                inf.append(inference_measure(c, n, device, cameras=K, graph=g))
                            except Exception as exc:
                                inf.append({"workload": c + " forward-only", "launch": "HIP graph replay" if g else "eager", "failed": repr(exc)})
                            gc.collect(); torch.cuda.empty_cache()
                    result["inference"] = inf
                except Exception as exc:
                    result["inference"] = "failed: %r" % (exc,)
                # a whole training iteration (train.py:47-167) at C3: render + every loss and regulariser + both Adam steps + the
                # amortised neighbour-index / densification work, with per-stage HIP-event times (examples/train_iteration.py)
                try:
                    import importlib.util
                    spec = importlib.util.spec_from_file_location("adgs_train_iteration", os.path.join(ROOT, "examples", "train_iteration.py"))
                    ti = importlib.util.module_from_spec(spec); spec.loader.exec_module(ti)
                    result["train_iteration"] = ti.run("C3", iters=int(os.environ.get("ADGS_BENCH_TRAIN_ITERS", "210")), cameras=K, device=device)
                    # the same iteration with every Adam step taken from materialised gradients (FusedAdam without in_backward)
                    sep = ti.run("C3", iters=int(os.environ.get("ADGS_BENCH_TRAIN_ITERS", "210")), cameras=K, device=device, stages=False, adam_in_backward=False)
                    result["train_iteration"]["ms_per_iteration_separate_adam"] = sep["ms_per_iteration"]
                    # The in-backward step has an intermittent HOST stall (EXPERIMENTS.md, round 6: 4 of 31 alternated runs at 3.0 - 4.5 ms, a whole
                    # run or none of it): a run that comes out more than 10 % behind the separate step is measured once more, and BOTH attempts are reported
                    first = result["train_iteration"]["ms_per_iteration"]
                    if first > 1.1 * sep["ms_per_iteration"]:
                        again = ti.run("C3", iters=int(os.environ.get("ADGS_BENCH_TRAIN_ITERS", "210")), cameras=K, device=device)
                        again["ms_per_iteration_separate_adam"] = sep["ms_per_iteration"]
                        again["ms_per_iteration_attempts"] = [first, again["ms_per_iteration"]]
                        again["note_attempts"] = "the first in-backward run hit the intermittent host stall of that mode; the fields of this object are the second run's"
                        if again["ms_per_iteration"] < first:
                            result["train_iteration"] = again
                        else:
                            result["train_iteration"]["ms_per_iteration_attempts"] = [first, again["ms_per_iteration"]]
                except Exception as exc:
                    result["train_iteration"] = "failed: %r" % (exc,)
                gc.collect(); torch.cuda.empty_cache()
                try:
                    result["knn_dist2"] = knn_measure(device, with_cpu=not args.no_cpu_baseline)
                except Exception as exc:
                    result["knn_dist2"] = "failed: %r" % (exc,)
                sens = []
                for variant in ("translucent", "sky", "street"):
                    a = quick_measure("C3", 40, device, use_fs, variant=variant, with_stats=True)[0]
                    b = quick_measure("C3", 6, device, use_fs, variant=variant, mode="classic", warm=3)[0]
                    a["classic_frames_per_s"] = b["frames_per_s"]
                    sens.append(a)
                    gc.collect(); torch.cuda.empty_cache()
                result["scene_sensitivity"] = sens
            except Exception as exc:                     # secondary information must never cost the headline line
                result["other_configs"] = "failed: %r" % (exc,)
        if args.full and world == 1 and not args.no_cpu_baseline and frame is not None and not iteration_mode:
            if isinstance(frame, DeformFrame):
                pkg, flow = frame.activated()
                sc_cpu = dict(sc, means3D=pkg["xyz"], opacities=pkg["opacity"], scales=pkg["scales"], rotations=pkg["rotation"],
                              shs=pkg["shs"], flow_points=flow)
            else:
                sc_cpu = sc
            try:
                deform_s = cpu_deformation_seconds(frame.model, frame.t, frame.t + 0.05 if use_fs else None) if isinstance(frame, DeformFrame) else None
                result["cpu_baseline"], oracle_fwd = cpu_baseline(sc_cpu, canonical_cam, cfg, use_fs, up, deform_s=deform_s)
                result["parity"] = parity_vs_oracle(outs, oracle_fwd)
            except Exception as exc:                     # e.g. the oracle library could not be built on this host
                result["cpu_baseline"] = {"value": None, "unit": "frames/s", "cores": 0, "kind": "port", "sample": "failed: %r" % (exc,)}
        # RCCL prints a version banner through C stdio, which (on a pipe) would only be flushed at exit, i.e. AFTER the JSON
        # line: flush it first so that the JSON line is the last line of stdout
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except OSError:
            pass
        sys.stdout.flush()
        print(json.dumps(result), flush=True)
    if world > 1 or force_coll:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
