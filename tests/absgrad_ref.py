"""Float64 torch restatement of the per-pair position terms of the rasterizer's HAND-WRITTEN backward -- test infrastructure for the
absolute screen-space gradient (include/adgs_rasterizer.h: adgs_raster_backward_options.dL_dmean2D_abs).

The rasterizer's dL/dmeans2D of a Gaussian g is a sum over the (pixel, Gaussian) pairs its backward replays,

    dL_dmeans2D[g].x = sum_pairs t_x,   t_x = dL/dG * dG/d(delta x) * W/2 = -o L (A dx + B dy) W/2,   L = G dL/dalpha
    dL_dmeans2D[g].y = sum_pairs t_y,   t_y =                             -o L (B dx + C dy) H/2

(backward.cu:545-644 of the reference: d = mean - pixel, (A, B, C) the conic, o the opacity, G = exp(power)), and the new output is
sum |t_x|, sum |t_y|.  Neither can be had from autograd of tests/torch_ref.render_dense: the per-pair terms are reduced inside it, and
the hand-written backward is not the true derivative (the gradient passes through the 0.99 alpha cap, the opacity term carries an extra
factor T -- backward.cu:612-614 --, the gates are constants).  So this file states the geometry of render_dense once more, tile by tile
(all pixels of a 16x16 tile x all Gaussians whose rectangle holds the tile, in depth order), with the pixel offsets dx, dy of every pair
as explicit tensors, replays the backward's recurrences in closed form and returns BOTH reductions.  tests/test_absgrad_ref.py pins the
signed one to the CPU oracle's dL_dmeans2D; the GPU tests then trust the absolute one.

Closed form of the replay for one pixel, contributing entries k = 1..n front to back, alpha a_k, T_k = prod_{j<k} (1 - a_j),
w_k = a_k T_k, per-entry channel dot cg_k = sum_ch c_k,ch dL/dC_ch (colour, depth, flow, semantic):
    blend of everything behind k, dotted with the upstream gradient:   B_k = (sum_{j>k} cg_j w_j) / (T_k (1 - a_k))
    dL/dalpha_k = (cg_k - B_k [+ T_final dL/dO / (1 - a_k)]) T_k  -  T_final (bg . dL/dC) / (1 - a_k)
"""
import numpy as np
import torch

from tests.torch_ref import ALPHA_MAX, ALPHA_MIN, CLAMP13, EIG_FLOOR, EPS7, LOWPASS, NEAR, T_STOP, _f, eval_sh, quat_to_R


def _t(x):
    return None if x is None else torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(torch.float64)


def mean2d_pair_sums(sc, grads, colors=None, cov3D=None, use_sh=True, flow=True, sem=True, inv_depth=True, scale_modifier=1.0, degree=None,
                     bg=None, opacity_factor=None):
    """sc: an adgs.synthetic scene; grads: upstream image gradients {color, depth, flow, semantic, img_opacity} ([C,H,W]); the keyword
    arguments are those of tests/test_gpu_raster.py: run_oracle.  opacity_factor [P] (anti-aliasing: tests/aa_ref.filter_factor): the
    opacity every use after the projection takes is opacity * factor.
    Returns dict(signed [P,3], abs [P,3], radii [P] int32, pairs [P] (replayed pairs per Gaussian)) -- third column 0, as the rasterizer's."""
    dt = torch.float64
    P, H, W = sc["P"], sc["H"], sc["W"]
    means3D = sc["means3D"].to(dt)
    tanfovx, tanfovy, scale_modifier = _f(sc["tanfovx"]), _f(sc["tanfovy"]), _f(scale_modifier)
    V, PM = sc["viewmatrix"].to(dt), sc["projmatrix"].to(dt)
    p_h = torch.cat([means3D, torch.ones(P, 1, dtype=dt)], 1)
    p_view = (p_h @ V)[:, :3]
    p_hom = p_h @ PM
    p_proj = p_hom[:, :3] * (1.0 / (p_hom[:, 3:4] + EPS7))
    visible = p_view[:, 2] > NEAR
    focal_x, focal_y = W / (2.0 * tanfovx), H / (2.0 * tanfovy)
    if cov3D is None:
        Mm = quat_to_R(sc["rotations"].to(dt)) @ torch.diag_embed(scale_modifier * sc["scales"].to(dt))
        Sigma = Mm @ Mm.transpose(1, 2)
    else:
        c = cov3D.to(dt)
        Sigma = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).reshape(-1, 3, 3)
    tz = p_view[:, 2]
    limx, limy = CLAMP13 * tanfovx, CLAMP13 * tanfovy
    txc = torch.clamp(p_view[:, 0] / tz, -limx, limx) * tz
    tyc = torch.clamp(p_view[:, 1] / tz, -limy, limy) * tz
    zero = torch.zeros_like(tz)
    J = torch.stack([focal_x / tz, zero, -(focal_x * txc) / (tz * tz), zero, focal_y / tz, -(focal_y * tyc) / (tz * tz)], 1).reshape(-1, 2, 3)
    T = J @ V[:3, :3].transpose(0, 1)
    cov = T @ Sigma @ T.transpose(1, 2)
    a, b, c = cov[:, 0, 0] + LOWPASS, cov[:, 0, 1], cov[:, 1, 1] + LOWPASS
    det = a * c - b * b
    visible = visible & (det != 0)
    det_safe = torch.where(det != 0, det, torch.ones_like(det))
    cA, cB, cC = c / det_safe, -b / det_safe, a / det_safe
    mid = 0.5 * (a + c)
    radius = torch.ceil(3.0 * torch.sqrt(mid + torch.sqrt(torch.clamp_min(mid * mid - det, EIG_FLOOR))))
    px = ((p_proj[:, 0] + 1.0) * W - 1.0) * 0.5
    py = ((p_proj[:, 1] + 1.0) * H - 1.0) * 0.5
    gx, gy = (W + 15) // 16, (H + 15) // 16
    rminx = torch.clamp(torch.trunc((px - radius) / 16), 0, gx)
    rminy = torch.clamp(torch.trunc((py - radius) / 16), 0, gy)
    rmaxx = torch.clamp(torch.trunc((px + radius + 15) / 16), 0, gx)
    rmaxy = torch.clamp(torch.trunc((py + radius + 15) / 16), 0, gy)
    visible = visible & ((rmaxx - rminx) * (rmaxy - rminy) > 0)
    radii = torch.where(visible, radius, torch.zeros_like(radius)).to(torch.int32)
    # per-Gaussian channel values
    deg = sc["sh_degree"] if degree is None else degree
    if colors is not None:
        feat = colors.to(dt)
    elif use_sh and sc.get("shs") is not None:
        d = means3D - sc["campos"].to(dt)[None]
        feat = eval_sh(deg, sc["shs"].to(dt), d / d.norm(dim=1, keepdim=True))
    else:
        feat = None
    dval = (1.0 / (tz + EPS7)) if inv_depth else tz
    opac = sc["opacities"].to(dt)[:, 0] * (1.0 if opacity_factor is None else opacity_factor.to(dt))
    # upstream gradients, channel gating as the rasterizer's (backward.cu:497-506)
    g = {k: _t(v) for k, v in grads.items()}
    chan_vals, chan_grads = [], []
    if feat is not None and g.get("color") is not None:
        chan_vals.append(feat); chan_grads.append(g["color"].reshape(3, -1))
    if g.get("depth") is not None:
        chan_vals.append(dval[:, None]); chan_grads.append(g["depth"].reshape(1, -1))
    if flow and sc.get("flow_points") is not None and g.get("flow") is not None:
        chan_vals.append(sc["flow_points"].to(dt)); chan_grads.append(g["flow"].reshape(3, -1))
    if sem and sc.get("semantic") is not None and g.get("semantic") is not None:
        assert sc["semantic"].shape[1] == 1, "the absolute sums are defined for one semantic channel"
        chan_vals.append(sc["semantic"].to(dt)); chan_grads.append(g["semantic"].reshape(1, -1))
    vals = torch.cat(chan_vals, 1)                  # [P, CH]
    gpix = torch.cat(chan_grads, 0)                 # [CH, H*W]
    gO = g["img_opacity"].reshape(-1) if g.get("img_opacity") is not None else None
    bgc = _t(sc["bg"] if bg is None else bg)
    bg_dot = (bgc[:, None] * g["color"].reshape(3, -1)).sum(0) if (feat is not None and g.get("color") is not None) else torch.zeros(H * W, dtype=dt)
    # depth order, ties by index (the reference's stable sort on the float32 depth)
    order = torch.argsort(tz.to(torch.float32), stable=True)
    order = order[visible[order]]
    o_rminx, o_rmaxx, o_rminy, o_rmaxy = rminx[order], rmaxx[order], rminy[order], rmaxy[order]
    signed = torch.zeros(P, 3, dtype=dt)
    absol = torch.zeros(P, 3, dtype=dt)
    pairs = torch.zeros(P, dtype=torch.int64)
    for ty in range(gy):
        in_row = (o_rminy <= ty) & (ty < o_rmaxy)
        for tx in range(gx):
            ids = order[in_row & (o_rminx <= tx) & (tx < o_rmaxx)]
            if ids.numel() == 0:
                continue
            ys, xs = torch.meshgrid(torch.arange(ty * 16, min(ty * 16 + 16, H)), torch.arange(tx * 16, min(tx * 16 + 16, W)), indexing="ij")
            pid = (ys * W + xs).reshape(-1)
            dx = px[ids][None, :] - xs.reshape(-1, 1).to(dt)             # [X, n]: mean - pixel
            dy = py[ids][None, :] - ys.reshape(-1, 1).to(dt)
            A, B, C, o = cA[ids][None], cB[ids][None], cC[ids][None], opac[ids][None]
            power = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy
            G = torch.exp(power)
            alpha = torch.clamp_max(o * G, ALPHA_MAX)
            gate = (power <= 0) & (alpha >= ALPHA_MIN)
            a_eff = torch.where(gate, alpha, torch.zeros_like(alpha))
            stop = gate & (torch.cumprod(1 - a_eff, dim=1) < T_STOP)
            contrib = gate & ~(torch.cumsum(stop.to(torch.int32), dim=1) > 0)
            a_eff = torch.where(contrib, alpha, torch.zeros_like(alpha))
            Tincl = torch.cumprod(1 - a_eff, dim=1)
            Texcl = torch.cat([torch.ones(Tincl.shape[0], 1, dtype=dt), Tincl[:, :-1]], 1)
            T_final = Tincl[:, -1:]
            cg = gpix[:, pid].transpose(0, 1) @ vals[ids].transpose(0, 1)          # [X, n]
            cw = cg * a_eff * Texcl
            behind = torch.flip(torch.cumsum(torch.flip(cw, [1]), 1), [1]) - cw    # sum_{j>k} cg_j w_j
            rinv = 1.0 / (1.0 - a_eff)
            dL_dalpha = cg - behind * rinv / Texcl
            if gO is not None:
                dL_dalpha = dL_dalpha + T_final * gO[pid][:, None] * rinv          # before the * T: the reference's quirk
            dL_dalpha = dL_dalpha * Texcl - T_final * bg_dot[pid][:, None] * rinv
            L = torch.where(contrib, G * dL_dalpha, torch.zeros_like(G))           # the gradient passes through the 0.99 cap: dalpha/dG = o
            t_x = -o * L * (A * dx + B * dy) * (0.5 * W)
            t_y = -o * L * (B * dx + C * dy) * (0.5 * H)
            signed[:, 0].index_add_(0, ids, t_x.sum(0)); signed[:, 1].index_add_(0, ids, t_y.sum(0))
            absol[:, 0].index_add_(0, ids, t_x.abs().sum(0)); absol[:, 1].index_add_(0, ids, t_y.abs().sum(0))
            pairs.index_add_(0, ids, contrib.sum(0))
    return dict(signed=signed.numpy(), abs=absol.numpy(), radii=radii.numpy(), pairs=pairs.numpy())
