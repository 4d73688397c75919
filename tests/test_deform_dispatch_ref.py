"""CPU checks of the deformation case table (tests/deform_cases.py): the two references the GPU test leans on agree with each
other on every case, the float64 gradients exist, and the table still reaches every launch path it was built for."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import deform_oracle as do
from tests import deform_cases as dc
from tests import torch_deform_ref as tr


@pytest.mark.parametrize("case", dc.CASES, ids=dc.IDS)
def test_numpy_oracle_and_float64_restatement_agree(case):
    """oracle.deform_oracle (float32 NumPy) against tests.torch_deform_ref (float64): all five outputs to 1e-6 of the output's
    largest magnitude (observed: 4.7e-7 at the longest rows), and finite float64 gradients of every parameter."""
    raw, oa = dc.raw_inputs(case), dc.order_args(case)
    npm = dict(raw)
    npm["order_args"], npm["use_time_mask"] = oa, case.use_time_mask
    m64 = {k: torch.tensor(v, dtype=torch.float64).requires_grad_(k != "gs_time") for k, v in raw.items()}
    for t in (case.t,) + (() if case.flow_time is None else (case.flow_time,)):
        ref32, ref64 = do.get_deformed_pkg(npm, t), tr.get_deformed_pkg(m64, t, oa, case.use_time_mask)
        for key in dc.OUTPUT_KEYS:
            a, b = np.asarray(ref32[key], np.float64), ref64[key].detach().numpy()
            assert a.shape == b.shape == ((case.Ns + case.No,) + {"xyz": (3,), "rotation": (4,), "shs": (case.M, 3), "opacity": (1,), "scales": (3,)}[key])
            if a.size:
                scale = max(np.abs(b).max(), 1e-30)
                worst = np.abs(a - b).max() / scale
                print("%s %s t=%g: %.3g" % (case.id, key, t, worst))
                assert worst <= 1e-6, (case.id, key, t, worst)
    ref64 = tr.get_deformed_pkg(m64, case.t, oa, case.use_time_mask)
    ws = dc.upstream_weights(case, {k: tuple(ref64[k].shape) for k in dc.OUTPUT_KEYS})
    sum((ref64[k] * torch.tensor(ws[k])).sum() for k in dc.OUTPUT_KEYS).backward()
    for name, v in m64.items():
        if name != "gs_time" and v.numel() and v.grad is not None:
            assert torch.isfinite(v.grad).all(), (case.id, name)


def test_table_reaches_every_launch_path():
    """Every branch label the table was built for occurs in at least one case, the misaligned twins differ from their originals
    in the branches the pointers decide, and the expectations of the refusal cases follow from the mirror."""
    reached = {}
    for c in dc.CASES:
        for lab in dc.labels(c):
            reached.setdefault(lab, []).append(c.id)
    missing = [lab for lab in dc.REQUIRED_LABELS if lab not in reached]
    assert not missing, missing
    assert len(set(dc.IDS)) == len(dc.IDS) and len(dc.CASES) <= 32
    for c in dc.CASES:
        p, labs = dc.plan(c), dc.labels(c)
        assert (c.expect == "refuse") == ("refuse_fwd" in labs), c.id
        assert (c.expect == "refuse_if_grad") == ("refuse_bwd_only" in labs), c.id
        if c.expect == "ok":
            assert max(p["fwd_lds"], p["bwd_lds"]) <= dc.MAX_STAGING_LDS, c.id
    twins = [c for c in dc.CASES if c.misaligned]
    assert len(twins) == 5
    want = {"scene_generic", "xyz_staged_misaligned", "sh0_general_misaligned"}
    assert want <= set().union(*(dc.labels(c) for c in twins))
    assert any(c.rotation[4] != 0 for c in twins) and any(c.Ns == 258 for c in twins) and any(dc.get_param_num(c.shs) == 16 for c in twins)
    # the sizes and time stamps the table is to contain
    assert {1, 2, 6, 255, 258, 0} <= {c.Ns for c in dc.CASES} and {63, 64, 65, 127, 129, 0} <= {c.No for c in dc.CASES}
    assert {0.0, 1.0} <= {c.t for c in dc.CASES} and any(c.flow_time is not None for c in dc.CASES)
    assert any(c.xyz[0] and float(c.t * (c.xyz[0] - c.xyz[1])).is_integer() and 0.0 < c.t < 1.0 for c in dc.CASES)
    # the figures the long-row cases were chosen for
    by_id = {c.id: c for c in dc.CASES}
    assert dc.plan(by_id["rot52_xyz48"])["fwd_lds"] == 53504 and dc.plan(by_id["rot52_xyz48"])["fwd_B"] == 64
    assert dc.plan(by_id["rot150_ns0"])["fwd_lds"] == 153856
    assert dc.plan(by_id["xyz206_bwd_limit"])["bwd_lds"] == 160112 and dc.plan(by_id["xyz207_bwd_limit"])["bwd_lds"] == 160632
    assert dc.plan(by_id["xyz207_bwd_limit"])["fwd_lds"] == 158976


def _library_plan(case):
    """adgs_test_deform_plan on made-up addresses of the case's tensors: a tensor without elements is NULL, as adgs.deform passes it; the
    model tensors of a misaligned twin lie one float behind a 16-byte boundary, outputs and gradients are aligned (fresh allocations)."""
    import ctypes
    from adgs import _lib, deform
    lib = _lib.lib()
    raw = dc.raw_inputs(case)
    addr = iter(range(1 << 20, 1 << 30, 1 << 20))
    fake = lambda n, off=0: (next(addr) + off) if n else None
    p = deform.DeformParams()
    p.Ns, p.No, p.sh_coeffs, p.t = case.Ns, case.No, case.M, case.t
    p.use_time_mask = int(case.use_time_mask) | 4          # ADGS_DEFORM_WILL_BACKWARD
    for name in dc.RAW_NAMES:
        setattr(p, name, fake(raw[name].size, 4 if case.misaligned else 0))
    N = case.Ns + case.No
    out, grads = deform.DeformOutputs(), deform.DeformGrads()
    for key in dc.OUTPUT_KEYS:
        setattr(out, key, fake(N))
    for name in dc.RAW_NAMES:
        if name != "gs_time":
            setattr(grads, name, fake(raw[name].size))
    flow = fake(N if case.flow_time is not None else 0)
    up = [fake(N) for _ in range(4)] + [fake(N if case.flow_time is not None else 0)]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "adgs_testing.h")).read()
    fields = int(re.search(r"#define ADGS_TEST_DEFORM_PLAN_FIELDS (\d+)", hdr).group(1))
    fwd, bwd = (ctypes.c_int32 * fields)(), (ctypes.c_int32 * fields)()
    np_x, np_r = dc.get_param_num(case.xyz), dc.get_param_num(case.rotation)
    assert lib.adgs_test_deform_plan(ctypes.byref(p), np_x, np_x, np_r, ctypes.byref(out), flow, *up, ctypes.byref(grads), fwd, bwd) == 0
    names = ("B", "lds", "np_x", "stride_x", "stride_r", "xyz_rows", "scene4", "nb_rot", "nb_xyz", "nb_scene", "refused")
    assert len(names) == fields
    return dict(zip(names, fwd)), dict(zip(names, bwd))


@pytest.mark.parametrize("case", dc.CASES, ids=dc.IDS)
def test_mirror_plan_equals_the_library_plan(case):
    """The premise of the labels: `plan(case)` of the mirror is what deform.hip's plan_fwd / plan_bwd decide -- block size and dynamic LDS of
    both launches, the direct-rows and four-per-thread scene paths, and who refuses (the forward for itself: 1, for its backward: 2)."""
    fwd, bwd = _library_plan(case)
    p = dc.plan(case)
    assert (fwd["B"], fwd["lds"], bwd["B"], bwd["lds"]) == (p["fwd_B"], p["fwd_lds"], p["bwd_B"], p["bwd_lds"]), case.id
    assert fwd["xyz_rows"] == int(p["xyz_rows"]) and bwd["xyz_rows"] == 0, case.id
    assert fwd["scene4"] == bwd["scene4"] == int(p["scene4"]), case.id
    assert (fwd["refused"] == 1) == p["fwd_refused"], case.id
    assert (fwd["refused"] == 2) == (p["bwd_refused"] and not p["fwd_refused"]), case.id
    assert (bwd["refused"] == 1) == p["bwd_refused"] and bwd["refused"] in (0, 1), case.id
    for side in (fwd, bwd):
        assert (side["np_x"], side["stride_x"], side["stride_r"]) == (p["np_x"], (3 * p["np_x"]) | 1, (4 * p["np_r"]) | 1), case.id
    # the grid: the object range once per block set, the scene range in groups of four when scene4
    nb_o = lambda B: -(-case.No // B)
    nb_s = lambda B: -(-(-(-case.Ns // 4) if p["scene4"] else case.Ns) // B)
    assert (fwd["nb_rot"], fwd["nb_scene"]) == (nb_o(fwd["B"]), nb_s(fwd["B"])), case.id
    assert fwd["nb_xyz"] == (-(-3 * case.No // fwd["B"]) if p["xyz_rows"] else nb_o(fwd["B"])), case.id
    assert (bwd["nb_rot"], bwd["nb_xyz"], bwd["nb_scene"]) == (nb_o(bwd["B"]), nb_o(bwd["B"]), nb_s(bwd["B"])), case.id


def test_mirror_constants_match_the_kernel_source():
    """The constants the mirror shares with the sources, and the wording of the refusals."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = lambda name: open(os.path.join(root, "ad-gs_amd", "csrc", name)).read()
    hdr = open(os.path.join(root, "include", "adgs_deform.h")).read()
    assert int(re.search(r"constexpr size_t MAX_STAGING_LDS = (\d+) \* 1024;", csrc("kernels.h")).group(1)) * 1024 == dc.MAX_STAGING_LDS
    assert int(re.search(r"#define ADGS_FUNC_MAX_QUAT (\d+)", hdr).group(1)) == dc.MAX_QUAT
    assert csrc("deform.hip").count(dc.REFUSAL) + csrc("deform_sh.hip").count(dc.REFUSAL) >= 3
