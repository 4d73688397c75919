"""Cameras, map / image configurations and cached float64 / float32 oracle references shared by tests/test_oracle_env.py (CPU)
and tests/test_gpu_env_paths.py (GPU).  Every number a camera is made of is exact in float32, so the library and the oracle
see the same camera."""
import collections
import functools
import os
import re

import numpy as np

from oracle import env_oracle

# what the premise assertions mirror of csrc/envmap.hip
TEXCAP = 2048                # envmap.hip TEXCAP: texels of the LDS footprint image; a larger box takes the direct-atomics path
BLOCK_W, BLOCK_H = 64, 4     # envmap.hip: the 64 x 4-pixel workgroup of envmap_fwd_kernel / envmap_bwd_kernel
MAXC = 8                     # envmap.hip MAXC
EPS = 1e-5                   # unstable_pixels: ~100 float32 roundings of a unit ray component


def kernel_constants():
    """(TEXCAP, MAXC, block width, block height) as csrc/envmap.hip states them."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ad-gs_amd", "csrc", "envmap.hip")).read()
    texcap, maxc = re.search(r"constexpr int TEXCAP = (\d+);", src), re.search(r"constexpr int MAXC = (\d+);", src)
    block = re.search(r"envmap_bwd_kernel\(.*?px = blockIdx\.x \* (\d+) \+ \(tid & \d+\), py = blockIdx\.y \* (\d+) \+", src, re.S)
    return int(texcap.group(1)), int(maxc.group(1)), int(block.group(1)), int(block.group(2))


def assert_mirrors_kernel():
    """The premise of every path test: block_boxes / pair_classes are evaluated with the kernel's own constants."""
    texcap, maxc, bw, bh = kernel_constants()
    assert texcap == TEXCAP, "env_cases.TEXCAP mirrors envmap.hip TEXCAP = %d: the LDS / direct-atomics premises must be re-derived" % texcap
    assert (bw, bh) == (BLOCK_W, BLOCK_H), "env_cases.BLOCK_W x BLOCK_H mirrors envmap.hip's %d x %d-pixel workgroup" % (bw, bh)
    assert maxc == MAXC, "env_cases.MAXC mirrors envmap.hip MAXC = %d" % maxc


def _f32(rows):
    return np.asarray(rows, np.float32)


def _quat(w, x, y, z):
    q = np.array([w, x, y, z], np.float64); q /= np.linalg.norm(q)
    w, x, y, z = q
    return _f32([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


# camera z -> world -x (the azimuth seam runs down the image's centre column: ry = -vx), camera x -> -y, camera y -> z
CAM_NEG_X = _f32([[0, 0, -1], [-1, 0, 0], [0, 1, 0]])
# camera z -> world +z (the pole is the principal point), turned about it so that the seam passes between pixel centres
CAM_POLE = _f32([[np.cos(0.3), -np.sin(0.3), 0], [np.sin(0.3), np.cos(0.3), 0], [0, 0, 1]])
CAM_GENERIC = _quat(0.9, 0.2, -0.3, 0.25)
# roughly along +x, away from seam and poles, azimuth growing with the pixel column (camera x -> world +y): every box is small
CAM_FRONT = (_f32([[0, 0, 1], [1, 0, 0], [0, 1, 0]]).astype(np.float64) @ _quat(1.0, 0.01, -0.01, 0.005)).astype(np.float32)

# the pair-merge configurations: name -> (Hm, Wm, focal, camera, the pair class it is there for)
PAIR_CONFIGS = {
    "same": (4, 8, 100.0, CAM_FRONT, env_oracle.SAME),                 # ~0.01 texel per pixel
    "neither": (16, 4096, 64.0, CAM_FRONT, env_oracle.NEITHER),        # ~10 texels per pixel
    "adjacent": (4, 378, 100.0, CAM_FRONT, env_oracle.ADJACENT),       # (Wm - 1) / (2 pi focal) = 0.6 texel per pixel
}
PAIR_WIDTHS, PAIR_HEIGHTS = (1, 63, 64, 65, 127), (1, 3, 4, 5)

Reference = collections.namedtuple("Reference", "gm w stable bg bg_d32 grad grad_d32 grad_scale coord_d32")


@functools.lru_cache(maxsize=None)
def _reference(C, Hm, Wm, H, W, focal, Rkey, seed):
    R = _f32(Rkey).reshape(3, 3)
    rng = np.random.default_rng(seed)
    gm = rng.normal(size=(C, Hm, Wm)).astype(np.float32)               # distinct data per channel
    stable = ~env_oracle.unstable_pixels(H, W, focal, R, EPS)
    w = (rng.normal(size=(C, H, W)) * stable).astype(np.float32)       # unstable pixels get zero upstream weight
    bg = env_oracle.background(gm, H, W, focal, R)
    bg32 = env_oracle.background(gm, H, W, focal, R, np.float32)
    grad = env_oracle.background_grad(gm, H, W, focal, R, w)
    grad32 = env_oracle.background_grad(gm, H, W, focal, R, w, np.float32)
    c64, c32 = env_oracle.sample_coords(H, W, focal, R, Hm, Wm), env_oracle.sample_coords(H, W, focal, R, Hm, Wm, np.float32)
    cd = max(float(np.abs((a - b) * stable).max()) for a, b in zip(c64, c32)) if stable.any() else 0.0
    for a in (gm, w, stable, bg, grad):
        a.setflags(write=False)                                         # shared among tests: nobody changes it
    return Reference(gm, w, stable, bg, float(np.abs((bg - bg32) * stable).max()) if stable.any() else 0.0, grad,
                     float(np.abs(grad - grad32).max()), float(np.abs(grad).max()), cd)


def reference(C, Hm, Wm, H, W, focal, R, seed=0):
    """Random map and upstream weights of a case with the float64 oracle's background and map gradient, and d32 = the largest
    deviation of the float32 oracle from it (background: over the stable pixels), computed once per case."""
    return _reference(C, Hm, Wm, H, W, float(focal), tuple(float(v) for v in np.asarray(R).reshape(-1)), seed)


def tolerance(d32, scale):
    """8 x the float32 oracle's own deviation (the device's atan2f / hypotf / expf are a few ulp off libm, and the float atomics sum
    in another order) + 2e-6 of the quantity's scale."""
    return 8.0 * d32 + 2e-6 * scale


def ceiling(Hm, Wm, scale):
    """The allowance of tests/test_gpu_env.py, which no tolerance here may exceed."""
    return (3e-5 + 4e-6 * max(Hm, Wm)) * scale
