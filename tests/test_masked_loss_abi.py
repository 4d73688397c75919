"""What the weighted losses and the sparse metric depth term (include/adgs_loss.h, adgs.loss) promise without a GPU: every new entry point
is declared, exported by the cross-compiled library and bound; the work-size constant equals the header's; malformed calls are refused
on the host, with a message, before anything is launched; the Python surface refuses malformed weights and CPU tensors.  The numerics
are in tests/test_gpu_masked_loss.py."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ad-gs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# symbol -> number of parameters, the stream included
ENTRIES = {"adgs_l1_ssim_weighted_forward": 12, "adgs_l1_ssim_weighted_backward": 14, "adgs_bce_clip_weighted_forward": 11,
           "adgs_bce_clip_weighted_backward": 12, "adgs_lidar_depth_loss_forward": 8, "adgs_lidar_depth_loss_backward": 9}


def test_entries_are_declared_exported_and_bound():
    from adgs import _lib, loss
    header = open(os.path.join(ROOT, "include", "adgs_loss.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.lib()                                           # resolves every declared symbol: AttributeError if one is not exported
    for name, n in ENTRIES.items():
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert decl, name
        assert len(decl.group(1).split(",")) == n, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n, name
        assert getattr(lib, name) is not None
    # the existing entry points keep their signatures
    assert re.search(r"\bint\s+adgs_bce_clip_forward\s*\(\s*int n, const float\* pred, const float\* target, float lo, float hi, int invert, int positive_target,\s*"
                     r"double\* work, float\* loss, void\* stream\)", code)
    assert len(_lib.SIGNATURES["adgs_bce_clip_forward"][1]) == 10 and len(_lib.SIGNATURES["adgs_l1_ssim_forward"][1]) == 10

    def define(name):
        return eval(re.search(r"#define\s+%s\s+\(([\d\s*+]+)\)" % name, header).group(1))
    slots = int(re.search(r"#define\s+ADGS_LOSS_SLOTS\s+(\d+)", header).group(1))
    assert define("ADGS_L1_SSIM_WEIGHTED_WORK_DOUBLES") == loss.L1_SSIM_WEIGHTED_WORK_DOUBLES >= slots * 3 + 3
    assert define("ADGS_AUX_WORK_DOUBLES") == loss.AUX_WORK_DOUBLES and slots == loss.SLOTS


def test_malformed_calls_are_refused_on_the_host():
    """Every refusal is decided from the arguments alone: nothing is launched, so the made-up pointer is never followed."""
    from adgs import _lib
    lib = _lib.lib()
    p = 0x1000
    calls = {
        "adgs_l1_ssim_weighted_forward": [
            lambda: lib.adgs_l1_ssim_weighted_forward(3, 8, 16, p, p, None, p, p, p, p, p, None),           # no weight
            lambda: lib.adgs_l1_ssim_weighted_forward(3, 8, 16, None, p, p, p, p, p, p, p, None),
            lambda: lib.adgs_l1_ssim_weighted_forward(3, 8, 16, p, p, p, None, p, p, p, p, None),           # no work buffer
            lambda: lib.adgs_l1_ssim_weighted_forward(3, 8, 16, p, p, p, p, p, p, p, None, None),           # no output
            lambda: lib.adgs_l1_ssim_weighted_forward(3, 8, 16, p, p, p, p, p, None, p, p, None),           # two of three maps
            lambda: lib.adgs_l1_ssim_weighted_forward(65536, 8, 16, p, p, p, p, p, p, p, p, None)],
        "adgs_l1_ssim_weighted_backward": [
            lambda: lib.adgs_l1_ssim_weighted_backward(3, 8, 16, p, p, None, p, p, p, p, p, p, p, None),
            lambda: lib.adgs_l1_ssim_weighted_backward(3, 8, 16, p, p, p, p, p, p, None, p, p, p, None),    # no work buffer: no sum of weights
            lambda: lib.adgs_l1_ssim_weighted_backward(3, 8, 16, p, p, p, p, p, p, p, p, p, None, None),
            lambda: lib.adgs_l1_ssim_weighted_backward(65536, 8, 16, p, p, p, p, p, p, p, p, p, p, None)],
        "adgs_bce_clip_weighted_forward": [
            lambda: lib.adgs_bce_clip_weighted_forward(128, p, p, None, 1e-3, 0.999, 0, 1, p, p, None),
            lambda: lib.adgs_bce_clip_weighted_forward(128, p, p, p, 1e-3, 0.999, 0, 1, None, p, None)],
        "adgs_bce_clip_weighted_backward": [
            lambda: lib.adgs_bce_clip_weighted_backward(128, p, p, None, 1e-3, 0.999, 0, 1, p, p, p, None),
            lambda: lib.adgs_bce_clip_weighted_backward(128, p, p, p, 1e-3, 0.999, 0, 1, None, p, p, None)],
        "adgs_lidar_depth_loss_forward": [
            lambda: lib.adgs_lidar_depth_loss_forward(128, p, None, p, 0, p, p, None),
            lambda: lib.adgs_lidar_depth_loss_forward(128, p, p, None, 1, p, p, None)],
        "adgs_lidar_depth_loss_backward": [
            lambda: lib.adgs_lidar_depth_loss_backward(128, p, p, p, 0, None, p, p, None),
            lambda: lib.adgs_lidar_depth_loss_backward(128, p, p, p, 0, p, p, None, None)],
    }
    assert set(calls) == set(ENTRIES)
    for name, cases in calls.items():
        for i, c in enumerate(cases):
            assert c() < 0, (name, i)
            assert _lib.last_error().startswith(name + ": "), (name, i, _lib.last_error())
    # an empty problem is not an error and launches nothing
    assert lib.adgs_l1_ssim_weighted_forward(0, 8, 16, p, p, p, p, p, p, p, p, None) == 0
    assert lib.adgs_bce_clip_weighted_forward(0, p, p, p, 1e-3, 0.999, 0, 1, p, p, None) == 0
    assert lib.adgs_lidar_depth_loss_forward(0, p, p, p, 0, p, p, None) == 0


def test_python_surface_refuses_malformed_weights_and_cpu_tensors():
    from adgs import loss
    img, gt = torch.rand(3, 8, 16), torch.rand(3, 8, 16)
    plane = torch.rand(8, 16)
    flow_pkg = (None, torch.eye(3), torch.eye(3), torch.zeros(3), torch.rand(2, 8, 16), torch.ones(8, 16))
    fused = lambda w: loss.image_losses(img, gt, plane, plane, torch.rand(3, 8, 16), flow_pkg, plane, plane[None], plane, plane, weight=w)
    surfaces = [lambda w: loss.l1_ssim(img, gt, weight=w), lambda w: loss.l1_loss(img, gt, weight=w), lambda w: loss.ssim(img, gt, weight=w),
                lambda w: loss.photometric_loss(img, gt, 0.2, weight=w), lambda w: loss.bce_clip_loss(plane, plane, weight=w),
                lambda w: loss.obj_loss(plane[None], plane, weight=w), lambda w: loss.sky_loss(plane, plane, weight=w), fused]
    for f in surfaces:
        for bad in (torch.ones(16, 8), torch.ones(3, 8, 16), torch.ones(8, 15), torch.ones(128)):
            with pytest.raises(ValueError, match="weight must be"):
                f(bad)
        for bad in (torch.ones(8, 16, dtype=torch.float64), torch.ones(8, 16, dtype=torch.bool), torch.ones(8, 16, dtype=torch.float16)):
            with pytest.raises(TypeError, match="weight must be float32"):
                f(bad)
        with pytest.raises(TypeError, match="weight must be a tensor"):
            f(1.0)
        with pytest.raises(RuntimeError, match="weight is on"):      # another device than the images'
            f(torch.ones(8, 16, device="meta"))
        with pytest.raises(RuntimeError, match="no CPU path"):        # a well-formed weight: the images themselves are refused
            f(torch.ones(8, 16))
        with pytest.raises(RuntimeError, match="no CPU path"):
            f(torch.ones(1, 8, 16))
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.lidar_depth_loss(plane, plane, plane > 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.lidar_depth_loss(plane, plane, plane, inv_depth=True)
    with pytest.raises(ValueError):
        loss.lidar_depth_loss(plane, plane[:4], plane)
    with pytest.raises(ValueError):
        loss.lidar_depth_loss(img, img, img)
    with pytest.raises(TypeError):
        loss.lidar_depth_loss(plane, plane.numpy(), plane)
    with pytest.raises(RuntimeError, match="lidar_mask on"):
        loss.lidar_depth_loss(plane, plane, torch.ones(8, 16, device="meta"))
