"""adgs._lib.call -- the one way the operators call a native entry that takes a stream -- and what adgs.loss builds on it: the call
sequence of the fused image-loss node and of the six standalone terms, the error path, the caller's stream, empty inputs."""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 33, 47          # no multiple of the SSIM tile or of 256
FUSED_FORWARD = ["adgs_l1_ssim_forward", "adgs_l1_ssim_means", "adgs_depth_loss_forward", "adgs_flow_loss_forward%s", "adgs_bce_clip_forward", "adgs_bce_clip_forward"]
FUSED_BACKWARD = ["adgs_l1_ssim_backward", "adgs_depth_loss_backward", "adgs_flow_loss_backward%s", "adgs_bce_clip_backward", "adgs_bce_clip_backward"]


@pytest.fixture
def calls(monkeypatch):
    """The symbols that go through _lib.call, in order; every call is passed on."""
    from adgs import _lib
    seen, real = [], _lib.call

    def recorder(symbol, device, *args):
        seen.append(symbol)
        return real(symbol, device, *args)

    monkeypatch.setattr(_lib, "call", recorder)
    return seen


@pytest.fixture(scope="module")
def scene():
    g = torch.Generator().manual_seed(3347)
    r = lambda *s: torch.rand(*s, generator=g)
    dev = "cuda"
    return dict(
        gt=dict(image=r(3, H, W).to(dev), depth=(r(H, W) * 0.5 + 0.01).to(dev), sem=(r(H, W) > 0.8).float().to(dev), sky=(r(H, W) > 0.7).float().to(dev),
                flow=torch.stack([r(H, W) * (W - 1), r(H, W) * (H - 1)]).to(dev), vis=(r(H, W) > 0.3).float().to(dev)),
        cam=(torch.tensor([[90.0, 0.0, W / 2.0], [0.0, 90.0, H / 2.0], [0.0, 0.0, 1.0]]), torch.eye(3), torch.tensor([0.05, -0.02, 0.1])),
        x=dict(image=r(3, H, W), depth=r(H, W) * 0.4 + 0.05, img_flow=torch.cat([r(2, H, W) * 4 - 2, r(1, H, W) * 5 + 1]), img_opacity=r(H, W) * 0.98 + 0.01,
               img_semantic=r(3, H, W)),
        w=torch.tensor([0.8, 0.2, 0.1, 0.1, 0.1, 0.05], device=dev))


@pytest.mark.parametrize("cam_on_device", [True, False])
def test_image_losses_call_sequence_is_pinned_and_equals_the_six_functions(scene, calls, cam_on_device):
    from adgs import loss
    gt = scene["gt"]
    flow_pkg = (0.4,) + tuple(t.cuda() if cam_on_device else t for t in scene["cam"]) + (gt["flow"], gt["vis"])
    suffix = "_devcam" if cam_on_device else ""

    def run(fused):
        del calls[:]
        x = {k: v.clone().cuda().requires_grad_(True) for k, v in scene["x"].items()}
        if fused:
            terms = loss.image_losses(x["image"], gt["image"], x["depth"], gt["depth"], x["img_flow"], flow_pkg, x["img_opacity"], x["img_semantic"], gt["sem"],
                                      gt["sky"], dist=0.02)
        else:
            terms = loss.l1_ssim(x["image"], gt["image"]) + (loss.get_depth_loss(x["depth"], gt["depth"]),
                                                             loss.get_flow_loss(x["img_flow"], flow_pkg, x["img_opacity"], dist=0.02),
                                                             loss.obj_loss(x["img_semantic"], gt["sem"]), loss.sky_loss(x["img_opacity"], gt["sky"]))
        n_forward = len(calls)
        (torch.stack([t.reshape(()) for t in terms]) * scene["w"]).sum().backward()
        return [t.detach().clone() for t in terms], {k: v.grad.detach().clone() for k, v in x.items()}, list(calls[:n_forward]), list(calls[n_forward:])

    t_fused, g_fused, fwd, bwd = run(True)
    assert fwd == [s % suffix if "%s" in s else s for s in FUSED_FORWARD]
    assert bwd == [s % suffix if "%s" in s else s for s in FUSED_BACKWARD]
    t_six, g_six, fwd6, bwd6 = run(False)
    assert collections.Counter(fwd6) == collections.Counter(fwd) and collections.Counter(bwd6) == collections.Counter(bwd)
    for a, b in zip(t_fused, t_six):
        assert torch.equal(a, b), (a, b)
    assert sorted(g_fused) == sorted(g_six) and len(g_fused) == 5
    for k in g_six:
        assert g_fused[k].shape == g_six[k].shape and torch.equal(g_fused[k], g_six[k]), k


def test_call_raises_with_the_symbol_it_called_and_the_native_text():
    """K = 1 neighbour: the native entry rejects the arguments before any launch."""
    from adgs import _lib, loss
    dev = torch.device("cuda", torch.cuda.current_device())
    x, idx = torch.zeros(4, 3, device=dev), torch.zeros(1, 1, dtype=torch.int64, device=dev)
    work, out = torch.zeros(loss.AUX_WORK_DOUBLES, dtype=torch.float64, device=dev), torch.empty(1, device=dev)
    with pytest.raises(RuntimeError) as err:
        _lib.call("adgs_group_var_forward", dev, 4, 1, 1, 3, 3, x.data_ptr(), idx.data_ptr(), work.data_ptr(), out.data_ptr())
    assert str(err.value).startswith("adgs_group_var_forward failed:") and "2 <= K" in str(err.value)


def test_terms_run_on_the_callers_stream():
    from adgs import loss
    g = torch.Generator().manual_seed(5)
    pred, sky = torch.rand(H, W, generator=g).cuda(), (torch.rand(H, W, generator=g) > 0.5).float().cuda()
    dev = pred.device

    def run():
        p = pred.clone().requires_grad_(True)
        val = loss.sky_loss(p, sky)
        val.backward()
        _, tok = loss._work(dev, loss.AUX_WORK_DOUBLES)
        tok.done()
        return val.detach(), p.grad, tok.arena

    v0, g0, arena0 = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        v1, g1, arena1 = run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(v0, v1) and torch.equal(g0, g1)
    assert arena0 is not None and arena1 is not None and arena1 is not arena0
    assert loss._ARENAS[(dev, side.cuda_stream, loss.AUX_WORK_DOUBLES)] is arena1


def test_empty_inputs_give_zeros_empty_gradients_and_no_launch(calls):
    """l1_ssim and sigma_loss make no native call for an empty input; get_depth_loss hands n = 0 to its two entries, which return before
    they launch anything."""
    from adgs import loss
    img = torch.zeros(3, 0, 8, device="cuda", requires_grad=True)
    l1, s = loss.l1_ssim(img, torch.zeros(3, 0, 8, device="cuda"))
    (l1 + s).backward()
    assert float(l1.detach()) == 0.0 and float(s.detach()) == 0.0 and img.grad.shape == (3, 0, 8) and calls == []
    pred = torch.zeros(0, device="cuda", requires_grad=True)
    d = loss.get_depth_loss(pred, torch.zeros(0, device="cuda"))
    d.backward()
    assert float(d.detach()) == 0.0 and pred.grad.shape == (0,) and calls == ["adgs_depth_loss_forward", "adgs_depth_loss_backward"]
    del calls[:]
    sigma = torch.zeros(0, 2, device="cuda", requires_grad=True)
    v = loss.sigma_loss(sigma, 0.1)
    v.backward()
    assert float(v.detach()) == 0.0 and sigma.grad.shape == (0, 2) and calls == []
