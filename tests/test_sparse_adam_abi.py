"""What the visibility-masked Adam step (adgs_adam_step_rows, FusedAdam.step(visibility=...)) promises without a GPU: the C entry is
declared, exported and bound; the ctypes mirror of adgs_adam_rows has the C struct's size; the entry refuses malformed row tables on
the host, before any launch; CPU tensors never reach the native library; allreduce_visibility is an element-wise maximum over the
ranks (gloo, two processes: the pattern of tests/test_dp_gloo.py).  The numerics are in tests/test_gpu_sparse_adam.py."""
import ctypes
import os
import re
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def test_entry_is_declared_exported_and_bound():
    from adgs import _lib
    from adgs.optim import AdamGroup, AdamRows
    header = open(os.path.join(ROOT, "include", "adgs_optim.h")).read()
    assert re.search(r"\bint\s+adgs_adam_step_rows\s*\(\s*const\s+adgs_adam_group\s*\*\s*groups\s*,\s*const\s+adgs_adam_rows\s*\*\s*rows", header)
    assert re.search(r"typedef\s+struct\s+adgs_adam_rows\s*\{", header)
    assert "adgs_adam_step_rows" in _lib.SIGNATURES and "adgs_adam_step" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["adgs_adam_step_rows"]
    assert res is ctypes.c_int and len(args) == len(_lib.SIGNATURES["adgs_adam_step"][1]) + 1
    lib = _lib.lib()                                           # resolves every declared symbol
    assert lib.adgs_adam_step_rows is not None
    assert ctypes.sizeof(AdamRows) == lib.adgs_test_abi_sizeof(8) == 24
    assert ctypes.sizeof(AdamGroup) == lib.adgs_test_abi_sizeof(5)          # the dense entry's struct kept its layout
    # the masked launch's argument table: <= 24 B per group on top of the dense one, far below the 4 KiB limit with 32 groups
    per_group = ctypes.sizeof(AdamGroup) + 3 * 4 + ctypes.sizeof(AdamRows)
    assert 32 * per_group + 64 < 4096


def test_malformed_row_tables_are_refused_on_the_host():
    """Every refusal is decided from the two tables alone: nothing is launched.  Without a GPU the pointers are made up (they are never
    followed); with one they are real buffers, large enough for any of the calls, so that a check that stopped refusing could not
    send a kernel to a wild address."""
    from adgs import _lib
    from adgs.optim import AdamGroup, AdamRows, ROWS_DENSE, ROWS_INT32, ROWS_UINT8
    lib = _lib.lib()
    if torch.cuda.is_available():
        buf = torch.zeros(64, device="cuda")
        fake = buf.data_ptr()
    else:
        fake = 0x1000

    def call(numel, rows, tile=None):
        grp = AdamGroup(fake, fake, fake, fake, numel, 1e-3, 1, tile, 0, 0)
        return lib.adgs_adam_step_rows(ctypes.byref(grp), ctypes.byref(rows), 1, 0.9, 0.999, 1e-15, 0, None)
    for what, code in (("n_rows * row_len != numel", call(12, AdamRows(fake, 5, 3, ROWS_INT32))),
                       ("numel not a multiple of row_len", call(13, AdamRows(fake, 4, 3, ROWS_UINT8))),
                       ("row_len < 1", call(12, AdamRows(fake, 12, 0, ROWS_INT32))),
                       ("negative row_len", call(12, AdamRows(fake, -4, -3, ROWS_INT32))),
                       ("unknown kind", call(12, AdamRows(fake, 4, 3, 3))),
                       ("tile_active on a masked group", call(12, AdamRows(fake, 4, 3, ROWS_INT32), tile=fake)),
                       ("NULL visibility", call(12, AdamRows(None, 4, 3, ROWS_UINT8)))):
        assert code < 0, what
        assert "adgs_adam_step_rows" in _lib.last_error(), (what, _lib.last_error())
    # an empty call and an empty masked group are no-ops, as for the dense entry
    assert lib.adgs_adam_step_rows(None, None, 0, 0.9, 0.999, 1e-15, 0, None) == 0
    assert call(0, AdamRows(None, 0, 3, ROWS_INT32)) == 0
    assert ROWS_DENSE == 0


def test_cpu_tensors_and_cpu_masks_never_reach_the_library(monkeypatch):
    from adgs import _lib
    from adgs.optim import FusedAdam, mark_visibility_groups, merge_visibility

    def no_native_call():
        raise AssertionError("the native library was asked for")
    monkeypatch.setattr(_lib, "lib", no_native_call)
    p = torch.zeros(10, 3, requires_grad=True)
    opt = FusedAdam([{"params": [p], "lr": 1e-2, "name": "scene_xyz"}, {"params": [torch.zeros(4, 3, 2, requires_grad=True)], "lr": 1e-2, "name": "deform_xyz"},
                     {"params": [torch.zeros(4, 4, requires_grad=True)], "lr": 1e-2, "name": "obj_rotation"}], lr=0.0, eps=1e-15)
    assert mark_visibility_groups(opt) == {"scene_xyz": "head", "deform_xyz": None, "obj_rotation": "tail"}
    assert mark_visibility_groups(opt, dense=()) == {"scene_xyz": "head", "deform_xyz": "tail", "obj_rotation": "tail"}
    p.grad = torch.ones(10, 3)
    with pytest.raises(ValueError, match="HIP device"):        # a CPU mask
        opt.step(visibility=torch.ones(14, dtype=torch.int32))
    with pytest.raises(ValueError):                            # ... of a dtype that is no visibility
        opt.step(visibility=torch.ones(14))
    with pytest.raises(RuntimeError, match="no CPU path"):     # CPU parameters, as without a visibility
        opt.step()
    assert p not in opt.state and float(p.detach().abs().max()) == 0.0
    with pytest.raises(TypeError):
        opt.step(visible=None)
    a, b = torch.tensor([0, 5, -1, 2], dtype=torch.int32), torch.tensor([3, 0, -1, 1], dtype=torch.int32)
    assert torch.equal(merge_visibility(merge_visibility(None, a), b), torch.maximum(a, b)) and a.tolist() == [0, 5, -1, 2]


def test_training_setup_takes_sparse_adam():
    import inspect
    from adgs.model import SyntheticGaussianModel
    from adgs.optim import FusedAdam
    assert inspect.signature(SyntheticGaussianModel.training_setup).parameters["sparse_adam"].default is False
    assert inspect.signature(FusedAdam.step).parameters["visibility"].default is None


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _radii(rank, dtype):
    g = torch.Generator().manual_seed(40 + rank)
    r = torch.randint(-2, 60, (5000,), generator=g, dtype=torch.int32)
    r[rank::3] = 0
    return r if dtype == torch.int32 else (r > 0).to(dtype)


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
        sys.path.insert(0, p)
    from adgs import dp
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for dtype in (torch.int32, torch.uint8, torch.bool):
        v = _radii(rank, dtype)
        res = dp.allreduce_visibility(v)
        assert res is v                                        # in place
        out[str(dtype)] = v
    torch.save(out, os.path.join(out_dir, "r%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_allreduce_visibility_is_the_maximum_on_every_rank(tmp_path):
    from adgs import dp
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    res = [torch.load(os.path.join(str(tmp_path), "r%d.pt" % r)) for r in range(world)]
    for dtype in (torch.int32, torch.uint8, torch.bool):
        a, b = _radii(0, dtype), _radii(1, dtype)
        want = (a | b) if dtype == torch.bool else torch.maximum(a, b)
        assert want.dtype == dtype
        for r in range(world):
            assert torch.equal(res[r][str(dtype)], want), (dtype, r)
    solo = _radii(0, torch.int32)
    assert dp.allreduce_visibility(solo) is solo and torch.equal(solo, _radii(0, torch.int32))      # no process group: unchanged
