"""Every launch path of the fused deformation kernels (csrc/deform.hip) against the float64 torch restatement: the cases of
tests/deform_cases.py, each built for branches of adgs_deform_forward_flow / adgs_deform_backward_flow that the goldens and
the fuzz seeds of tests/test_gpu_deform.py do not reach -- the generic SH kernels (M != 16), sh0_rows_kernel<4, 5, 7, 8>, the
general sh0 kernel, 1 / 3 / 7 / 8 control quaternions, the launches above 48 KiB of LDS and the refusal above the cap, the
generic scene body and the staged paths chosen because of a pointer, Ns % 4 == 2 and No around the block size.

Tolerances are those of tests/test_gpu_deform.py: 1e-4 of the reference tensor's largest magnitude for the outputs, 2e-4 for
the gradients; where the float64 gradient is identically zero the kernel's is zero or None."""
import numpy as np
import pytest
import torch

from tests import deform_cases as dc
from tests import torch_deform_ref as tr
from tests.test_gpu_deform import close

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e11          # no kernel output or parameter of these cases comes near it; compared bit for bit
PAD = 3                      # floats of the buffer behind a misaligned view


class _Model:
    pass


def _build_model(case, raw, requires_grad=True):
    """The case's model on the device.  misaligned: every tensor is a contiguous view one float into its buffer, the floats
    around it hold SENTINEL (returned as {name: buffer} for the later comparison)."""
    m, bufs = _Model(), {}
    for name, v in raw.items():
        t = torch.from_numpy(np.array(v))
        if case.misaligned:
            buf = torch.full((t.numel() + 1 + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
            view = buf[1:1 + t.numel()].view(t.shape)
            view.copy_(t)
            p = view.detach()
            assert p.is_contiguous() and (p.numel() == 0 or p.data_ptr() % 16 == 4), name
            bufs[name] = buf
        else:
            p = t.cuda()
            assert p.numel() == 0 or p.data_ptr() % 16 == 0, name
        setattr(m, dc.attr_of(name), p.requires_grad_(requires_grad and name != "gs_time"))
    m.order_args, m.use_time_mask = dc.order_args(case), case.use_time_mask
    return m, bufs


def _assert_surroundings_untouched(case, raw, m, bufs, when):
    sent = torch.tensor([SENTINEL], dtype=torch.float32).view(torch.int32).item()
    for name, buf in bufs.items():
        n = raw[name].size
        bits = buf.view(torch.int32).cpu()
        assert bits[0].item() == sent, "%s: the float in front of %s changed %s" % (case.id, name, when)
        assert bool((bits[1 + n:] == sent).all()), "%s: the floats behind %s changed %s" % (case.id, name, when)
        # and the parameters themselves are inputs: bit for bit what was put there
        assert np.array_equal(bits[1:1 + n].numpy(), np.ascontiguousarray(raw[name]).reshape(-1).view(np.int32)), (case.id, name, when)


def _reference(case, raw):
    m64 = {k: torch.tensor(v, dtype=torch.float64).requires_grad_(k != "gs_time") for k, v in raw.items()}
    oa = dc.order_args(case)
    ref = tr.get_deformed_pkg(m64, case.t, oa, case.use_time_mask)
    if case.flow_time is not None:
        ref["flow_xyz"] = tr.get_deformed_pkg(m64, case.flow_time, oa, case.use_time_mask)["xyz"]
    return m64, ref


def _compare_outputs(case, pkg, ref):
    assert set(pkg) == set(ref), case.id
    for key in ref:
        assert tuple(pkg[key].shape) == tuple(ref[key].shape), (case.id, key)
        if ref[key].numel():
            got, want = pkg[key].detach().cpu().numpy(), ref[key].detach().numpy()
            print("%s %s: max |err| / max |ref| = %.3g" % (case.id, key, np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)))
            close("%s %s t=%g" % (case.id, key, case.t), got, want, tol=1e-4)


@pytest.mark.parametrize("case", [c for c in dc.CASES if c.expect == "ok"], ids=[c.id for c in dc.CASES if c.expect == "ok"])
def test_forward_and_backward_vs_float64(case):
    from adgs.deform import get_deformed_pkg
    raw = dc.raw_inputs(case)
    m, bufs = _build_model(case, raw)
    pkg = get_deformed_pkg(m, case.t, flow_time=case.flow_time)
    m64, ref = _reference(case, raw)
    _compare_outputs(case, pkg, ref)
    if case.misaligned:
        torch.cuda.synchronize()
        _assert_surroundings_untouched(case, raw, m, bufs, "in the forward")
    keys = sorted(k for k in ref if ref[k].numel())
    ws = dc.upstream_weights(case, {k: tuple(ref[k].shape) for k in keys})
    sum((pkg[k] * torch.tensor(ws[k], dtype=torch.float32).cuda()).sum() for k in keys).backward()
    sum((ref[k] * torch.tensor(ws[k])).sum() for k in keys).backward()
    for name, t64 in m64.items():
        if name == "gs_time" or t64.numel() == 0:
            continue
        got, want = getattr(m, dc.attr_of(name)).grad, t64.grad
        if want is None or float(want.abs().max()) == 0.0:
            assert got is None or float(got.abs().max()) == 0.0, (case.id, name)
        else:
            assert got is not None, (case.id, name)
            print("%s grad %s: max |err| / max |ref| = %.3g" % (case.id, name, float((got.cpu().double() - want).abs().max() / want.abs().max())))
            close("%s grad %s t=%g" % (case.id, name, case.t), got.cpu().numpy(), want.numpy(), tol=2e-4)
    if case.misaligned:
        _assert_surroundings_untouched(case, raw, m, bufs, "in the backward")


def test_rows_above_the_lds_cap_are_refused_by_the_forward():
    """Rotation rows of 156 parameters: 64 rows of stride 625 exceed MAX_STAGING_LDS.  The forward raises the library's error (it
    decides before its first launch), and the stream is still healthy afterwards."""
    from adgs.deform import get_deformed_pkg
    (case,) = [c for c in dc.CASES if c.expect == "refuse"]
    assert dc.plan(case)["fwd_lds"] > dc.MAX_STAGING_LDS
    for requires_grad in (False, True):
        m, _ = _build_model(case, dc.raw_inputs(case), requires_grad=requires_grad)
        with pytest.raises(RuntimeError, match=dc.REFUSAL):
            get_deformed_pkg(m, case.t)
        torch.cuda.synchronize()
        assert all(getattr(m, dc.attr_of(n)).grad is None for n in dc.RAW_NAMES)


@pytest.mark.parametrize("case", [c for c in dc.CASES if c.expect == "refuse_if_grad"], ids=[c.id for c in dc.CASES if c.expect == "refuse_if_grad"])
def test_forward_refuses_what_its_backward_cannot_stage(case):
    """xyz rows of 206 / 207 parameters fit the forward's LDS need (direct rows / 158 976 bytes) but not the backward's, which adds
    the two basis vectors behind the gradient rows (160 112 / 160 632 bytes, cap 159 744).  Without gradients the forward runs
    and is right; on inputs that require gradients it refuses at forward time, with the library's message, instead of failing in
    the middle of autograd."""
    from adgs.deform import get_deformed_pkg
    p = dc.plan(case)
    assert p["fwd_lds"] <= dc.MAX_STAGING_LDS < p["bwd_lds"]
    raw = dc.raw_inputs(case)
    m, _ = _build_model(case, raw, requires_grad=False)
    pkg = get_deformed_pkg(m, case.t)
    _compare_outputs(case, pkg, _reference(case, raw)[1])
    m, _ = _build_model(case, raw, requires_grad=True)
    with torch.no_grad():
        _compare_outputs(case, get_deformed_pkg(m, case.t), _reference(case, raw)[1])
    with pytest.raises(RuntimeError, match=dc.REFUSAL):
        get_deformed_pkg(m, case.t)
    torch.cuda.synchronize()
    assert all(getattr(m, dc.attr_of(n)).grad is None for n in dc.RAW_NAMES)


def test_misaligned_upstream_gradients():
    """Upstream gradients that are views one float into a buffer (a caller's own tensors; autograd's are aligned): the same
    parameter gradients as from aligned copies of them."""
    from adgs.deform import get_deformed_pkg
    case = next(c for c in dc.CASES if c.id == "b128_no129")
    raw = dc.raw_inputs(case)
    grads = []
    for misaligned in (False, True):
        m, _ = _build_model(case, raw)
        pkg = get_deformed_pkg(m, case.t, flow_time=case.flow_time)
        keys = sorted(pkg)
        ws = dc.upstream_weights(case, {k: tuple(pkg[k].shape) for k in keys})
        ups = []
        for k in keys:
            w = torch.tensor(ws[k], dtype=torch.float32)
            if misaligned:
                buf = torch.zeros(w.numel() + 1, device="cuda")
                up = buf[1:].view(w.shape)
                up.copy_(w)
                assert up.data_ptr() % 16 == 4
            else:
                up = w.cuda()
            ups.append(up)
        torch.autograd.backward([pkg[k] for k in keys], ups)
        grads.append({n: getattr(m, dc.attr_of(n)).grad for n in dc.RAW_NAMES})
    for n in dc.RAW_NAMES:
        a, b = grads[0][n], grads[1][n]
        assert (a is None) == (b is None), n
        if a is not None and n != "background_deform_param":      # that one is summed with atomics, in any order
            assert torch.equal(a, b), n
        elif a is not None:
            close(n, b.cpu().numpy(), a.cpu().numpy(), tol=1e-5)
