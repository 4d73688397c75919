"""CPU restatement (NumPy) of the environment-map background of scene/env.py:11-76:
pixel -> camera ray (K^-1, normalise) -> world ray (world_view_transform[:3,:3] @ ray, normalise)
-> (azimuth, elevation) (utils/graphics_utils.py:95-100) -> scaled by (1/pi, 2/pi)
-> bilinear grid_sample (align_corners=True, zero padding) of grid_map -> sigmoid.
Plus the gradient w.r.t. grid_map for an upstream dL/dbackground.

TEST INFRASTRUCTURE ONLY.  Pinned against the reference's own Python (tests/golden/make_env_golden.py ->
tests/golden/env_golden.npz: backgrounds and reference-autograd gradients).
"""
import collections

import numpy as np


def world_rays(H, W, focal, R, dtype=np.float64):
    """Unit world ray [H, W, 3] of every pixel."""
    f = dtype(focal)
    xs, ys = np.meshgrid(np.arange(W, dtype=dtype), np.arange(H, dtype=dtype), indexing="xy")
    ray = np.stack([(xs - dtype(W) / 2) / f, (ys - dtype(H) / 2) / f, np.ones_like(xs)], -1)     # K^-1 [x, y, 1]
    ray = ray / np.maximum(np.linalg.norm(ray, axis=-1, keepdims=True), 1e-12)
    ray = ray @ np.asarray(R, dtype).T                                                            # R @ ray
    return ray / np.maximum(np.linalg.norm(ray, axis=-1, keepdims=True), 1e-12)


def sample_coords(H, W, focal, R, Hm, Wm, dtype=np.float64):
    """Continuous texel coordinates (ix, iy) [H, W] of every pixel."""
    ray = world_rays(H, W, focal, R, dtype)
    az = np.arctan2(ray[..., 1], ray[..., 0]); el = np.arctan2(ray[..., 2], np.hypot(ray[..., 0], ray[..., 1]))
    gx, gy = az * dtype(1.0 / np.pi), el * dtype(2.0 / np.pi)
    return (gx + 1) / 2 * (Wm - 1), (gy + 1) / 2 * (Hm - 1)


def _corners(ix, iy, Hm, Wm):
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    fx, fy = ix - x0, iy - y0
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx < Wm) & (yy >= 0) & (yy < Hm)                                    # padding_mode='zeros'
            yield xx, yy, wx * wy, ok


def background(grid_map, H, W, focal, R, dtype=np.float64):
    """grid_map [C, Hm, Wm] -> sigmoid(bilinear sample) [C, H, W]."""
    gm = np.asarray(grid_map, dtype)
    C, Hm, Wm = gm.shape
    ix, iy = sample_coords(H, W, focal, R, Hm, Wm, dtype)
    raw = np.zeros((C, H, W), dtype)
    for xx, yy, w, ok in _corners(ix, iy, Hm, Wm):
        raw += np.where(ok, w, 0)[None] * gm[:, np.clip(yy, 0, Hm - 1), np.clip(xx, 0, Wm - 1)]
    return 1.0 / (1.0 + np.exp(-raw))


def background_grad(grid_map, H, W, focal, R, g_bg, dtype=np.float64):
    """d(sum g_bg * background) / d grid_map."""
    gm = np.asarray(grid_map, dtype)
    C, Hm, Wm = gm.shape
    bg = background(gm, H, W, focal, R, dtype)
    g_raw = np.asarray(g_bg, dtype) * bg * (1 - bg)
    ix, iy = sample_coords(H, W, focal, R, Hm, Wm, dtype)
    out = np.zeros_like(gm)
    for xx, yy, w, ok in _corners(ix, iy, Hm, Wm):
        for c in range(C):
            np.add.at(out[c], (np.clip(yy, 0, Hm - 1), np.clip(xx, 0, Wm - 1)), np.where(ok, w, 0) * g_raw[c])
    return out


# ---- what the tests of csrc/envmap.hip need to know about a launch: which pixels are ill-conditioned, which backward path a
# ---- workgroup takes, how the lanes of a pixel pair relate, and which texels can be written at all

def unstable_pixels(H, W, focal, R, eps):
    """[H, W] bool: pixels whose float64 world ray lies within `eps` of a discontinuity of the mapping -- the azimuth seam
    (rx < 0, |ry| < eps: atan2 jumps between -pi and pi) or the pole (hypot(rx, ry) < eps: the azimuth is undefined).  The sample
    position jumps there, so a float32 and a float64 evaluation may legitimately land on opposite sides."""
    ray = world_rays(H, W, focal, R)
    rx, ry = ray[..., 0], ray[..., 1]
    return ((rx < 0) & (np.abs(ry) < eps)) | (np.hypot(rx, ry) < eps)


def _base_texel(H, W, focal, R, Hm, Wm):
    ix, iy = sample_coords(H, W, focal, R, Hm, Wm)
    return np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)


BlockBoxes = collections.namedtuple("BlockBoxes", "box area empty")


def block_boxes(H, W, focal, R, Hm, Wm, bw=64, bh=4, pixel_mask=None):
    """Per workgroup of bw x bh pixels (envmap_bwd_kernel: 64 x 4) the texel bounding box of its in-map corner taps, formed as the
    kernel forms it: per pixel [max(x0, 0), min(x0 + 1, Wm - 1)] x [max(y0, 0), min(y0 + 1, Hm - 1)], counted when not empty.
    Returns BlockBoxes(box [nby, nbx, 4] = (minx, miny, maxx, maxy), area [nby, nbx], empty [nby, nbx]); an empty block (no in-map
    tap) has area 0.  pixel_mask [H, W] bool: pixels to count (default: all)."""
    x0, y0 = _base_texel(H, W, focal, R, Hm, Wm)
    lox, hix, loy, hiy = np.maximum(x0, 0), np.minimum(x0 + 1, Wm - 1), np.maximum(y0, 0), np.minimum(y0 + 1, Hm - 1)
    ok = (lox <= hix) & (loy <= hiy)
    if pixel_mask is not None:
        ok &= np.asarray(pixel_mask, bool)
    nby, nbx = (H + bh - 1) // bh, (W + bw - 1) // bw
    box, area, empty = np.zeros((nby, nbx, 4), np.int64), np.zeros((nby, nbx), np.int64), np.ones((nby, nbx), bool)
    for by in range(nby):
        for bx in range(nbx):
            sl = (slice(by * bh, min((by + 1) * bh, H)), slice(bx * bw, min((bx + 1) * bw, W)))
            m = ok[sl]
            if not m.any():
                continue
            b = (lox[sl][m].min(), loy[sl][m].min(), hix[sl][m].max(), hiy[sl][m].max())
            box[by, bx], area[by, bx], empty[by, bx] = b, (b[2] - b[0] + 1) * (b[3] - b[1] + 1), False
    return BlockBoxes(box, area, empty)


SAME, ADJACENT, NEITHER, PARTNER_INVALID = 0, 1, 2, 3


def pair_classes(H, W, focal, R, Hm, Wm):
    """[H, ceil(W / 2)] class of every pixel pair (2j, 2j + 1) of a row, the two lanes whose contributions envmap_bwd_kernel merges:
    SAME (equal x0 and y0), ADJACENT (x0 of the odd pixel = x0 of the even one + 1, equal y0), NEITHER, or PARTNER_INVALID (the
    odd pixel lies beyond an odd W)."""
    x0, y0 = _base_texel(H, W, focal, R, Hm, Wm)
    cls = np.full((H, (W + 1) // 2), PARTNER_INVALID, np.int64)
    n = W // 2
    ex, ey, ox, oy = x0[:, 0:2 * n:2], y0[:, 0:2 * n:2], x0[:, 1:2 * n:2], y0[:, 1:2 * n:2]
    cls[:, :n] = np.where(ey != oy, NEITHER, np.where(ox == ex, SAME, np.where(ox == ex + 1, ADJACENT, NEITHER)))
    return cls


def tap_footprint(H, W, focal, R, Hm, Wm, pixel_mask=None, slack=0.0):
    """[Hm, Wm] bool: texels touched by at least one in-map tap of a counted pixel (pixel_mask [H, W] bool; default: all).
    slack (texels): a sample closer than this to a texel edge counts on both sides of it -- a float32 evaluation may floor it either way."""
    ix, iy = sample_coords(H, W, focal, R, Hm, Wm)
    m = np.ones((H, W), bool) if pixel_mask is None else np.asarray(pixel_mask, bool)
    out = np.zeros((Hm, Wm), bool)
    for sx in ((0.0,) if slack == 0 else (-slack, slack)):
        for sy in ((0.0,) if slack == 0 else (-slack, slack)):
            x0, y0 = np.floor(ix + sx).astype(np.int64), np.floor(iy + sy).astype(np.int64)
            for dy in (0, 1):
                for dx in (0, 1):
                    xx, yy = x0 + dx, y0 + dy
                    ok = m & (xx >= 0) & (xx < Wm) & (yy >= 0) & (yy < Hm)
                    out[yy[ok], xx[ok]] = True
    return out
