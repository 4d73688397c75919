"""Vertex normals in the mesh PLY (adgs.io.write_mesh_ply / read_mesh_ply): float nx, ny, nz after x, y, z and before the colours; a file
written without them is byte for byte the file the writer produced before the argument existed."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

V = np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, -2.25], [1, 1, 1e-3]], np.float32)
F = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
C = np.array([[0, 0.5, 1], [0.25, 0.25, 0.25], [1.5, -1, 0.999], [0.1, 0.2, 0.3]], np.float32)
N = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 0, 0], [-1, 0, 0]], np.float32)


def legacy_bytes(v, f, c):
    """The file of the writer before it knew normals, assembled by hand."""
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(v)
    if c is not None:
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    head += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(f)
    body = b""
    for i in range(len(v)):
        body += v[i].astype("<f4").tobytes()
        if c is not None:
            body += (255 * np.clip(c[i], 0, 1)).astype(np.uint8).tobytes()
    for t in f:
        body += b"\x03" + t.astype("<i4").tobytes()
    return head.encode("ascii") + body


@pytest.mark.parametrize("colors", [False, True])
@pytest.mark.parametrize("normals", [False, True])
def test_round_trip(tmp_path, colors, normals):
    from adgs import io
    path = str(tmp_path / "m.ply")
    io.write_mesh_ply(path, torch.from_numpy(V), torch.from_numpy(F), torch.from_numpy(C) if colors else None, normals=torch.from_numpy(N) if normals else None)
    v, f, c, n = io.read_mesh_ply(path, normals=True)
    assert np.array_equal(v, V) and np.array_equal(f, F) and v.dtype == np.float32 and f.dtype == np.int32
    assert (c is None) == (not colors) and (n is None) == (not normals)
    if colors:
        assert np.array_equal(c, (255 * np.clip(C, 0, 1)).astype(np.uint8))
    if normals:
        assert n.dtype == np.float32 and np.array_equal(n, N)
    three = io.read_mesh_ply(path)                              # the default call is unchanged
    assert len(three) == 3 and np.array_equal(three[0], V) and np.array_equal(three[1], F) and (three[2] is None) == (not colors)
    header = open(path, "rb").read().split(b"end_header\n")[0].decode("ascii").split("\n")
    names = [l.split()[-1] for l in header if l.startswith("property") and "list" not in l]
    assert names == ["x", "y", "z"] + (["nx", "ny", "nz"] if normals else []) + (["red", "green", "blue"] if colors else [])


@pytest.mark.parametrize("colors", [None, C])
def test_a_file_without_normals_is_byte_identical(tmp_path, colors):
    from adgs import io
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    io.write_mesh_ply(a, V, F, colors)                          # the call as it was before normals existed
    io.write_mesh_ply(b, V, F, colors, normals=None)
    want = legacy_bytes(V, F, colors)
    assert open(a, "rb").read() == want and open(b, "rb").read() == want


def test_empty_mesh_and_refusals(tmp_path):
    from adgs import io
    path = str(tmp_path / "e.ply")
    z = np.zeros((0, 3), np.float32)
    io.write_mesh_ply(path, z, np.zeros((0, 3), np.int32), normals=z)
    v, f, c, n = io.read_mesh_ply(path, normals=True)
    assert v.shape == (0, 3) and f.shape == (0, 3) and c is None and n.shape == (0, 3) and n.dtype == np.float32
    with pytest.raises(ValueError, match="normals must be"):
        io.write_mesh_ply(path, V, F, normals=N[:3])
