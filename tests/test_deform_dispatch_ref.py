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


def test_mirror_constants_match_the_kernel_source():
    """The premise of the labels: the mirror uses deform.hip's own constants."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "ad-gs_amd", "csrc", "deform.hip")).read()
    hdr = open(os.path.join(root, "include", "adgs_deform.h")).read()
    assert int(re.search(r"constexpr size_t MAX_STAGING_LDS = (\d+) \* 1024;", src).group(1)) * 1024 == dc.MAX_STAGING_LDS
    assert int(re.search(r"#define ADGS_FUNC_MAX_QUAT (\d+)", hdr).group(1)) == dc.MAX_QUAT
    assert "bytes <= 48 * 1024 || B == 64" in src and "for (int B = 256; B >= 64; B >>= 1)" in src
    assert src.count(dc.REFUSAL) >= 3
