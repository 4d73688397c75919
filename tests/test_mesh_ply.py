"""adgs.io.write_mesh_ply / read_mesh_ply: a triangle mesh survives the round trip through a binary PLY, with and without colours, and
so does an empty one.  Host code only."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def mesh(V=37, F=61, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(V, 3)).astype(np.float32), rng.integers(0, V, size=(F, 3)).astype(np.int32), rng.random((V, 3), dtype=np.float32))


@pytest.mark.parametrize("with_colors", [False, True])
@pytest.mark.parametrize("as_tensors", [False, True])
def test_round_trip(tmp_path, with_colors, as_tensors):
    from adgs import io
    v, f, c = mesh()
    c[0] = (-0.5, 1.5, 1.0)                                      # clipped
    c[1] = (0.999, 0.5, 0.0)                                     # truncated, not rounded: 254, 127, 0
    wrap = torch.from_numpy if as_tensors else (lambda a: a)
    path = str(tmp_path / "sub" / "mesh.ply")
    io.write_mesh_ply(path, wrap(v), wrap(f), wrap(c) if with_colors else None)
    head = open(path, "rb").read(400).decode("ascii", "replace")
    assert head.startswith("ply\nformat binary_little_endian 1.0\nelement vertex 37\n") and "property list uchar int vertex_indices" in head
    v2, f2, c2 = io.read_mesh_ply(path)
    assert v2.dtype == np.float32 and f2.dtype == np.int32
    assert np.array_equal(v2, v) and np.array_equal(f2, f)
    if with_colors:
        assert c2.dtype == np.uint8 and np.array_equal(c2, (255 * np.clip(c, 0, 1)).astype(np.uint8))
        assert tuple(c2[0]) == (0, 255, 255) and tuple(c2[1]) == (254, 127, 0)
    else:
        assert c2 is None
    assert os.path.getsize(path) == head.index("end_header\n") + 11 + 37 * (15 if with_colors else 12) + 61 * 13


@pytest.mark.parametrize("with_colors", [False, True])
def test_empty_mesh(tmp_path, with_colors):
    from adgs import io
    path = str(tmp_path / "empty.ply")
    io.write_mesh_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32) if with_colors else None)
    v, f, c = io.read_mesh_ply(path)
    assert v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == np.int32
    assert (c is not None and c.shape == (0, 3)) if with_colors else c is None


def test_vertices_without_faces_and_refusals(tmp_path):
    from adgs import io
    v, f, c = mesh()
    path = str(tmp_path / "points.ply")
    io.write_mesh_ply(path, v, np.zeros((0, 3), np.int32))
    v2, f2, _ = io.read_mesh_ply(path)
    assert np.array_equal(v2, v) and f2.shape == (0, 3)
    with pytest.raises(ValueError, match="vertices must be"):
        io.write_mesh_ply(path, v[:, :2], f)
    with pytest.raises(ValueError, match="faces must be"):
        io.write_mesh_ply(path, v, f.astype(np.float32))
    with pytest.raises(ValueError, match="faces must index"):
        io.write_mesh_ply(path, v, f + 37)
    with pytest.raises(ValueError, match="colors must be"):
        io.write_mesh_ply(path, v, f, c[:5])
    # the point-cloud reader still reads the vertex element of a mesh file
    io.write_mesh_ply(path, v, f, c)
    names, cols = io.read_ply(path)
    assert names == ["x", "y", "z", "red", "green", "blue"] and np.array_equal(cols["y"], v[:, 1])
