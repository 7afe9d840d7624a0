"""The backward of the whole metric-bins head (engine.BinsHead.backward on the HIP ops) and the head-training interface on the GPU.

Truth: float64 autograd through oracle.pf_oracle.bins_head + silog_loss on the CPU.  Comparator: the same oracle in float32 on this device
(torch's kernels).  Bar of every gradient tensor g:  max |g - g64| / max |g64|  <=  2 x (the comparator's same quantity) + f64_ref.BASE_FLOOR.
The head is the probe of tests/head_bwd_ref.py: C = 32, 128-wide embedding, 64 bins, n_attractors [16, 8, 4, 1], B = 2, x0 at (2, 3), x_blocks at
(3, 5) .. (17, 25), last at (33, 49), target uniform on (-5, 95).  It has 22 layers, so 44 parameter gradients, and 6 input gradients (7 with
the relative depth of a branch head)."""
import pytest
import torch

from tests import head_bwd_ref as R
from tests.f64_ref import BASE_FLOOR
from tests.test_head_bwd_kernels_gpu import DEV, F64, hold, normwise

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(scope="module")
def ops():
    from patchfusion_amd.hip_ops import ops
    return ops


def build_head(sd, bcfg, with_rel):
    from patchfusion_amd.engine import BinsHead
    return BinsHead(sd, "", 32, bcfg, F32, torch.device(DEV), with_rel=with_rel, min_depth=bcfg["min_depth"], max_depth=bcfg["max_depth"])


def head_step(ops, head, inp, target, bcfg):
    """forward with a context, SILog loss, backward -> (loss, depth, param grads, input grads)"""
    B, H, W, _ = inp["last"].shape
    clb = head.new_clb_buffer(ops, B, H, W)
    clb[..., :32] = inp["last"]
    if head.with_rel:
        clb[..., 32 + head.emb:] = 0.0
        clb[..., 32 + head.emb:33 + head.emb] = inp["rel"]
    ctx = {}
    depth = head.run(ops, inp["x0"], inp["x_blocks"], clb, save=ctx)
    loss, sums = ops.silog_loss_saved(depth, target, bcfg["min_depth"], bcfg["max_depth"])
    d_depth = ops.silog_loss_bwd(depth, target, sums, torch.empty_like(depth), bcfg["min_depth"], bcfg["max_depth"])
    grads, ig = head.backward(ops, ctx, d_depth)
    grads2, ig2 = head.backward(ops, ctx, d_depth)              # the same context again: identical bits
    assert all(torch.equal(grads[k], grads2[k]) for k in grads) and torch.equal(ig["x0"], ig2["x0"]) and torch.equal(ig["last"], ig2["last"])
    return loss, depth, grads, ig


def to_dev(inp):
    return {k: ([t.to(DEV) for t in v] if isinstance(v, list) else None if v is None else v.to(DEV)) for k, v in inp.items()}


@pytest.mark.parametrize("at,ak,with_rel", [("inv", "mean", False), ("exp", "sum", True)])
def test_whole_head_gradients(ops, at, ak, with_rel):
    sd, bcfg, inp, target = R.probe_head(at, ak, with_rel)
    valid = int(((target > bcfg["min_depth"]) & (target < bcfg["max_depth"])).sum())
    assert 0.7 * target.numel() < valid < 0.9 * target.numel()
    l64, d64, pg64, ig64 = R.oracle_head_grads(sd, bcfg, inp, target)
    l32, d32, pg32, ig32 = R.oracle_head_grads(sd, bcfg, inp, target, F32, DEV)
    head = build_head(sd, bcfg, with_rel)
    loss, depth, grads, ig = head_step(ops, head, to_dev(inp), target.to(DEV), bcfg)
    missed = []

    def hold_all(name, got, truth, comp):                        # every figure is printed before anything is asserted
        try:
            hold(name, got, truth, comp)
        except AssertionError as e:
            missed.append(e.args[0])

    hold_all("depth", depth, d64, d32)
    hold_all("loss", loss.reshape(1), l64.reshape(1), l32.reshape(1))
    assert set(grads) == set(pg64) and len(grads) == 44
    for k in sorted(grads):
        assert grads[k].shape == pg64[k].shape and float(pg64[k].abs().max()) > 0, k
        hold_all(k, grads[k], pg64[k], pg32[k])
    flat = lambda g: [("x0", g["x0"])] + [(f"x_blocks{i}", t) for i, t in enumerate(g["x_blocks"])] + [("last", g["last"])] + \
        ([("rel", g["rel"])] if "rel" in g else [])
    assert ("rel" in ig) == with_rel
    for (n, a), (_, t), (_, c) in zip(flat(ig), flat(ig64), flat(ig32)):
        assert float(t.abs().max()) > 0
        hold_all("d_" + n, a, t, c)
    assert not missed, missed


def test_the_saving_route_is_the_unfused_route_bit_for_bit(ops, monkeypatch):
    """with save= the head leaves the fused tail (pf_bins_tail keeps no pt): its depth is that of PF_BINS_TAIL=0; without it the fused tail runs"""
    sd, bcfg, inp, target = R.probe_head()
    inp = to_dev(inp)
    head = build_head(sd, bcfg, False)
    assert head.tail is not None
    calls = []
    real = ops.bins_tail
    monkeypatch.setattr(type(ops), "bins_tail", staticmethod(lambda *a, **k: (calls.append(1), real(*a, **k))[1]))

    def run(h, save):
        clb = h.new_clb_buffer(ops, 2, 33, 49)
        clb[..., :32] = inp["last"]
        return h.run(ops, inp["x0"], inp["x_blocks"], clb, save=save)

    fused = run(head, None)
    assert len(calls) == 1
    saved = run(head, {})
    assert len(calls) == 1
    monkeypatch.setenv("PF_BINS_TAIL", "0")
    plain_head = build_head(sd, bcfg, False)
    assert plain_head.tail is None
    assert torch.equal(saved, run(plain_head, None)) and len(calls) == 1
    assert float((fused - saved).abs().max()) <= 1e-5 * float(saved.abs().max())


def test_three_sgd_steps_follow_the_float64_oracle(ops):
    """three SGD steps (lr 1e-2) on the head's 44 tensors: forward with a context, backward, step, refresh -- and the same three steps on the
    float64 oracle (truth) and the float32 oracle on this device (comparator).  Each loss within 2 x the comparator's deviation + the floor;
    the third loss below the first."""
    sd, bcfg, inp, target = R.probe_head()
    from patchfusion_amd.engine import BinsHead
    names = BinsHead.param_names()

    def oracle_steps(dtype, device):
        cur = {k: v.clone() for k, v in sd.items()}
        losses = []
        for _ in range(3):
            loss, _, pg, _ = R.oracle_head_grads(cur, bcfg, inp, target, dtype, device)
            losses.append(float(loss))
            for k in names:
                cur[k] = (cur[k].to(device=device, dtype=dtype) - 1e-2 * pg[k]).detach()
        return losses

    l64, l32 = oracle_steps(F64, "cpu"), oracle_steps(F32, DEV)
    params = {k: torch.nn.Parameter(sd[k].to(DEV)) for k in names}
    opt = torch.optim.SGD(list(params.values()), lr=1e-2)
    head = build_head(sd, bcfg, False)
    dinp, dt = to_dev(inp), target.to(DEV)
    losses = []
    for _ in range(3):
        loss, _, grads, _ = head_step(ops, head, dinp, dt, bcfg)
        losses.append(float(loss))
        opt.zero_grad()
        for k in names:
            params[k].grad = grads[k]
        opt.step()
        head.refresh({k: p.detach() for k, p in params.items()})
    for i in range(3):
        e, base = abs(losses[i] - l64[i]) / abs(l64[i]), abs(l32[i] - l64[i]) / abs(l64[i])
        print(f"step {i}: loss hip {losses[i]:.7f} float64 {l64[i]:.7f} float32 oracle {l32[i]:.7f}: hip {e:.3e} comparator {base:.3e}")
        assert e <= 2 * base + BASE_FLOOR, (i, e, base)
    assert losses[2] < losses[0] and l64[2] < l64[0]


def test_public_interface_on_the_device(monkeypatch):
    """PatchFusion.train_forward(head_grad=...) / head_backward() / refresh_head() on the HIP ops, tiny config: head_grad=False is the path of
    forward(mode='train') bit for bit and still takes the fused tail; head_grad=True gives the depth of PF_BINS_TAIL=0 bit for bit; one SGD
    step through the interface lowers the loss and the repacked head serves the next forward."""
    from patchfusion_amd.config import make_config
    from patchfusion_amd.engine import BinsHead
    from patchfusion_amd.hip_ops import ops
    from patchfusion_amd.model import PatchFusion
    from patchfusion_amd.spec import patchfusion_spec, synthetic_state_dict
    from tests.test_train_forward_cpu import TINY, train_batch
    cfg = make_config(*TINY)
    sd = synthetic_state_dict(patchfusion_spec(cfg), 0)
    image_lr, crops, bboxs, gt = (t.to(DEV) for t in train_batch())

    def model():
        m = PatchFusion(cfg, compute_dtype="fp32").eval()
        m.load_state_dict(sd, strict=True)
        return m.to(DEV)

    m = model()
    calls = []
    real = ops.bins_tail
    monkeypatch.setattr(type(ops), "bins_tail", staticmethod(lambda *a, **k: (calls.append(1), real(*a, **k))[1]))
    l_mode, o_mode = m(mode="train", image_lr=image_lr, image_hr=None, crops_image_hr=crops, crop_depths=gt, bboxs=bboxs)
    n_fused = len(calls)
    assert n_fused == 3                                           # coarse head, fine head, fusion head
    l_plain, o_plain = m.train_forward(image_lr, crops, gt, bboxs)
    assert len(calls) == 2 * n_fused
    assert torch.equal(o_plain["depth_pred"], o_mode["depth_pred"]) and torch.equal(l_plain["total_loss"], l_mode["total_loss"])
    l_grad, o_grad = m.train_forward(image_lr, crops, gt, bboxs, head_grad=True)
    assert len(calls) == 3 * n_fused - 1                          # the fusion head alone left the fused tail
    monkeypatch.setenv("PF_BINS_TAIL", "0")
    m0 = model()
    l0, o0 = m0.train_forward(image_lr, crops, gt, bboxs)
    monkeypatch.delenv("PF_BINS_TAIL")
    assert len(calls) == 3 * n_fused - 1
    # (the branches of m0 run unfused too, and the fusion head reads their outputs: compare the fusion head's route on equal inputs instead)
    assert float((o0["depth_pred"] - o_grad["depth_pred"]).abs().max()) <= 1e-5 * float(o0["depth_pred"].abs().max())
    head = [m.get_parameter(n) for n in BinsHead.param_names()]
    opt = torch.optim.SGD(head, lr=1e-2)
    m.head_backward()
    first = [p.grad.clone() for p in head]
    m.head_backward()
    assert all(torch.equal(p.grad, g + g) for p, g in zip(head, first))
    opt.zero_grad()
    m.head_backward()
    opt.step()
    m.refresh_head()
    l_next, _ = m.train_forward(image_lr, crops, gt, bboxs)
    assert float(l_next["total_loss"]) < float(l_grad["total_loss"])
    with pytest.raises(RuntimeError, match="no context"):
        m.head_backward()
