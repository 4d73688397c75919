"""The scenes the mesh z-buffer (include/adgs_zbuffer.h) is tested on, shared by the CPU and GPU tests; at image sizes no kernel tile
divides (37 x 29; 128 x 96 where noted; one at 168 x 136), tan = (0.7, 0.55).  case(name) -> Case(vertices float32, faces int32, view);
reference(name) renders tests/zbuffer_ref.py on it once, with normals.  Nobody writes into what these return.

 1 quad_fullscreen      two faces at a float32 z, corners far outside the image but inside the guard band: every pixel, one deep box
 2 quad_on_centres      corners exactly on pixel centres, the diagonal through centres: the half-open rule, 16 x 16 pixels
 3 fan_on_centre        11 faces around a vertex that sits on a pixel centre
 4 subpixel             300 faces between the centres: nothing is drawn
 5 coplanar_duplicates  the same face 3 times among others: the tie goes to the lowest index
 6 interpenetrating     two big faces crossing
 7 near_and_guard       a corner before `near`, a NaN corner, a corner beyond the guard band, a zero-area face: one counter each
 8 bad_index            indices -1 and V among good faces
 9 sphere_outward       128 x 96, an outward-oriented sphere, the camera outside
10 random_big           128 x 96, 60 vertices in [-3, 3] x [-2, 2] x [2, 6], 40 random faces: many pixels see 3+ layers
11 mixed_sizes          128 x 96, 340 faces with boxes from 0 pixels to the whole image: the wave expansion across wave boundaries and the
                        list of big faces in one launch
12 huge_faces           168 x 136: faces of more than 256 tiles (the ones every workgroup of the big launch shares) beside big and small ones
13 tsdf                 128 x 96, the extracted mesh of tests/mesh_cases.py seen from inside its box with a non-identity pose
14 empty                F = 0
"""
import collections
import functools

import numpy as np

from tests import zbuffer_ref as ref

NAMES = ("quad_fullscreen", "quad_on_centres", "fan_on_centre", "subpixel", "coplanar_duplicates", "interpenetrating", "near_and_guard", "bad_index",
         "sphere_outward", "random_big", "mixed_sizes", "huge_faces", "tsdf", "empty")
SMALL, LARGE, HUGE = (29, 37), (96, 128), (136, 168)          # (H, W)
QUAD_Z = np.float32(3.3)

Case = collections.namedtuple("Case", "vertices faces view")


def at_pixel(view, px, py, z):
    """The float32 world position (identity pose) that projects to the pixel (px, py) at depth z."""
    z = np.asarray(z, np.float64)
    x = (np.asarray(px, np.float64) - (view.W - 1) * 0.5) / (view.W * 0.5) * view.tan[0] * z
    y = (np.asarray(py, np.float64) - (view.H - 1) * 0.5) / (view.H * 0.5) * view.tan[1] * z
    return np.stack(np.broadcast_arrays(x, y, z), -1).astype(np.float32)


def tri(*idx):
    return np.array(idx, np.int32).reshape(-1, 3)


def random_triangles(rng, view, n, lo, hi, z=(2.0, 6.0)):
    """n triangles with a bounding box of about lo .. hi pixels (log-uniform) anywhere over the image (and a little outside)."""
    size = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    cx, cy = rng.uniform(-4, view.W + 4, n), rng.uniform(-4, view.H + 4, n)
    off = rng.uniform(-0.5, 0.5, (n, 3, 2)) * size[:, None, None]
    zz = rng.uniform(z[0], z[1], (n, 3))
    v = at_pixel(view, cx[:, None] + off[..., 0], cy[:, None] + off[..., 1], zz).reshape(-1, 3)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def sphere(n_lat=12, n_lon=16, centre=(0.3, -0.2, 5.0), radius=1.7):
    """A UV sphere with pole fans, oriented outwards."""
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        v += [(np.sin(th) * np.cos(2 * np.pi * j / n_lon), np.sin(th) * np.sin(2 * np.pi * j / n_lon), np.cos(th)) for j in range(n_lon)]
    v.append((0.0, 0.0, -1.0))
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    f = [(0, ring(1, j), ring(1, j + 1)) for j in range(n_lon)]
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f += [(ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)), (ring(i, j), ring(i + 1, j + 1), ring(i, j + 1))]
    last = len(v) - 1
    f += [(last, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)) for j in range(n_lon)]
    v = np.array(v) * radius + np.array(centre)
    f = np.array(f, np.int32)
    p = v[f]
    out = (np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]) * (p.mean(1) - np.array(centre))).sum(1)
    assert (out > 0).all()
    return v.astype(np.float32), f


@functools.lru_cache(maxsize=None)
def case(name):
    small, large = ref.make_view(*SMALL), ref.make_view(*LARGE)
    if name == "quad_fullscreen":
        v = at_pixel(small, [-5000.0, 5037.0, 5037.0, -5000.0], [-4000.0, -4000.0, 4029.0, 4029.0], QUAD_Z)
        return Case(v, tri(0, 1, 2, 0, 2, 3), small)
    if name == "quad_on_centres":
        v = at_pixel(small, [5.0, 21.0, 21.0, 5.0], [4.0, 4.0, 20.0, 20.0], [2.0, 2.5, 3.0, 2.5])
        return Case(v, tri(0, 1, 2, 0, 2, 3), small)
    if name == "fan_on_centre":
        ang = np.sort(np.random.default_rng(3).uniform(0, 2 * np.pi, 11))
        rad = np.random.default_rng(4).uniform(6.0, 12.0, 11)
        rim = at_pixel(small, 18.0 + rad * np.cos(ang), 14.0 + rad * np.sin(ang), np.linspace(2.0, 3.0, 11))
        v = np.concatenate([at_pixel(small, 18.0, 14.0, 2.5)[None], rim])
        k = np.arange(11)
        return Case(v, np.stack([np.zeros(11, np.int64), 1 + k, 1 + (k + 1) % 11], 1).astype(np.int32), small)
    if name == "subpixel":
        rng = np.random.default_rng(5)
        n = 300
        cx, cy = rng.integers(-1, 37, n), rng.integers(-1, 29, n)
        off = rng.uniform(0.15, 0.85, (n, 3, 2))
        v = at_pixel(small, cx[:, None] + off[..., 0], cy[:, None] + off[..., 1], rng.uniform(1.0, 4.0, (n, 3))).reshape(-1, 3)
        return Case(v, np.arange(3 * n, dtype=np.int32).reshape(n, 3), small)
    if name == "coplanar_duplicates":
        rng = np.random.default_rng(6)
        v, f = random_triangles(rng, small, 9, 6, 30, z=(3.0, 5.0))
        dup = at_pixel(small, [3.3, 33.1, 12.7], [2.2, 9.4, 26.6], [2.0, 2.2, 2.4])         # in front of the others
        v = np.concatenate([v, dup])
        d = tri(27, 28, 29)
        return Case(v, np.concatenate([f[:2], d, f[2:5], d, f[5:7], d, f[7:]]).astype(np.int32), small)
    if name == "interpenetrating":
        a = at_pixel(small, [1.2, 35.5, 17.3], [2.1, 3.3, 27.9], [2.0, 2.0, 4.0])
        b = at_pixel(small, [2.4, 34.1, 18.8], [26.5, 25.2, 1.4], [2.2, 2.1, 3.8])
        return Case(np.concatenate([a, b]), tri(0, 1, 2, 3, 4, 5), small)
    if name == "near_and_guard":
        good = at_pixel(small, [4.5, 30.2, 11.1, 25.0], [3.3, 6.1, 24.4, 22.0], [2.0, 2.5, 3.0, 2.2])
        extra = np.array([[0.1, 0.1, 0.1],                       # 4: before near = 0.2
                          [np.nan, 0.0, 2.0],                    # 5
                          [0.0, 0.0, 0.0],                       # 6: replaced below, beyond the guard band
                          [np.inf, 1.0, 2.0]], np.float32)       # 7: not finite either
        extra[2] = at_pixel(small, 17000.0, 10.0, 2.0)
        v = np.concatenate([good, extra])
        f = tri(0, 1, 2,   0, 4, 1,   1, 5, 2,   0, 1, 6,   0, 1, 1,   2, 3, 0,   7, 0, 1,   0, 0, 0,   4, 6, 5)
        return Case(v, f, small)
    if name == "bad_index":
        v, f = random_triangles(np.random.default_rng(8), small, 6, 5, 25)
        f = np.concatenate([f[:2], tri(0, -1, 2), f[2:4], tri(3, 4, 18), f[4:], tri(-5, 1, 2)]).astype(np.int32)
        return Case(v, f, small)
    if name == "sphere_outward":
        v, f = sphere()
        return Case(v, f, large)
    if name == "random_big":
        rng = np.random.default_rng(10)
        v = rng.uniform([-3, -2, 2], [3, 2, 6], (60, 3)).astype(np.float32)
        f = np.stack([rng.choice(60, 3, replace=False) for _ in range(40)]).astype(np.int32)
        return Case(v, f, large)
    if name == "mixed_sizes":
        rng = np.random.default_rng(11)
        parts = [random_triangles(rng, large, 200, 0.3, 12), random_triangles(rng, large, 100, 8, 40), random_triangles(rng, large, 36, 30, 140),
                 (at_pixel(large, [-300.0, 500.0, 60.0, 70.0], [-200.0, -150.0, 600.0, -300.0], [5.5, 5.6, 5.7, 5.9]), tri(0, 1, 2, 1, 3, 2)),
                 random_triangles(rng, large, 2, 0.2, 0.4)]
        vs, fs, base = [], [], 0
        for v, f in parts:
            vs.append(v); fs.append(f + base); base += len(v)
        f = np.concatenate(fs)
        return Case(np.concatenate(vs), f[rng.permutation(len(f))].astype(np.int32), large)
    if name == "huge_faces":
        view = ref.make_view(*HUGE)
        rng = np.random.default_rng(12)
        parts = [(at_pixel(view, [-40.0, 230.0, 240.0, -60.0], [-30.0, -50.0, 180.0, 190.0], [4.0, 4.5, 5.0, 4.2]), tri(0, 1, 2, 0, 2, 3)),
                 random_triangles(rng, view, 8, 220, 420, z=(2.5, 4.4)), random_triangles(rng, view, 40, 1, 60, z=(2.0, 4.4))]
        vs, fs, base = [], [], 0
        for v, f in parts:
            vs.append(v); fs.append(f + base); base += len(v)
        return Case(np.concatenate(vs), np.concatenate(fs).astype(np.int32), view)
    if name == "tsdf":
        from tests import mesh_cases
        v, f = mesh_cases.tsdf_mesh()[:2]
        eye, target = np.array([21.0, 5.0, 27.0]), np.array([17.0, 16.0, 14.5])      # between the spheres, both in view
        z = (target - eye) / np.linalg.norm(target - eye)
        x = np.cross((0.1, 1.0, 0.05), z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        return Case(v, f, ref.make_view(*LARGE, pose=tuple(R.reshape(-1)) + tuple(-(R @ eye))))
    if name == "empty":
        return Case(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), small)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, cull=0):
    c = case(name)
    return ref.render(c.vertices, c.faces, c.view._replace(cull=cull), normals=True)


@functools.lru_cache(maxsize=None)
def views3(name):
    """Three views of a case: its own and two nearby poses (quad_fullscreen: shifted only -- a turn of the camera takes the far corners
    of the quad behind it, and the whole face goes with them)."""
    view = case(name).view
    R, t = np.array(view.pose[:9]).reshape(3, 3), np.array(view.pose[9:])
    out = [view]
    turns = ((0, 0, 0), (0, 0, 0)) if name == "quad_fullscreen" else ((0.03, -0.05, 0.02), (-0.06, 0.04, -0.03))
    for rv, dt in zip(turns, ((0.2, -0.1, 0.15), (-0.25, 0.12, -0.1))):
        D = np.array(ref.pose_from(rv, (0, 0, 0))[:9]).reshape(3, 3)
        out.append(view._replace(pose=tuple((D @ R).reshape(-1)) + tuple(D @ t + np.array(dt))))
    return tuple(out)
