"""The head-training interface (train_forward(head_grad=True) / head_backward() / refresh_head()) of PatchFusion and BaselinePretrain on the
CPU: the engine's backward wiring with the backward ops of tests/head_bwd_fake_ops.py (the restated formulas) against torch.autograd through
the oracle, on the tiny config of tests/test_train_forward_cpu.py.  The fake forward ops compute in float32, so the gradients agree with the
float64 autograd to float32 accuracy, not to 1e-10 (that comparison is tests/test_head_bwd_ref_cpu.py's)."""
import pytest
import torch

from oracle import pf_oracle
from patchfusion_amd.baseline import BaselinePretrain
from patchfusion_amd.config import make_config
from patchfusion_amd.engine import BinsHead
from patchfusion_amd.model import PatchFusion
from patchfusion_amd.spec import branch_spec, patchfusion_spec, synthetic_state_dict
from tests.head_bwd_fake_ops import ops as bwd_ops
from tests.test_train_forward_cpu import TINY, train_batch

FLOOR = 1e-6        # (one float32 rounding of the largest entry is 6e-8; the comparator must not decide alone when it happens to be exact)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def hold(name, got, truth, comp):
    """The engine's forward here is float32 (the fake forward ops are torch float32 on the CPU), the truth float64 autograd, the comparator
    float32 autograd through the same oracle.  This is a WIRING test, not a precision grade (tests/test_head_bwd_gpu.py grades the kernels
    at twice their comparator): a wrong buffer, a missing fan-in term, a wrong channel map or a missing accumulation changes a gradient
    by 1e-2 .. 1 of its largest entry, four to six orders above the float32 noise of the forward, while two float32 evaluations of a
    12-block ViT with different summation orders scatter by a small multiple of one another.  Bar: ten times the comparator's deviation."""
    e, base = rel(got, truth), rel(comp, truth)
    assert e <= 10 * base + FLOOR, (name, e, base)


@pytest.fixture(scope="module")
def tiny():
    cfg = make_config(*TINY)
    return cfg, synthetic_state_dict(patchfusion_spec(cfg), 0)


def fusion_model(cfg, sd, **kw):
    m = PatchFusion(cfg, compute_dtype=kw.pop("compute_dtype", "fp32"), ops=bwd_ops).eval()
    m.load_state_dict(sd, strict=True)
    return m


def oracle_fusion_head_grads(cfg, sd, batch, dtype=torch.float64):
    """autograd of the training loss w.r.t. the fusion head's parameters in `dtype`: the oracle's train_forward on leaf copies of them"""
    image_lr, crops, bboxs, gt = batch
    sdd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    names = BinsHead.param_names()
    for k in names:
        sdd[k] = sdd[k].clone().requires_grad_(True)
    # (Oracle.train_forward runs under torch.no_grad(): its undecorated body is differentiable torch)
    loss, pred = pf_oracle.Oracle.train_forward.__wrapped__(pf_oracle.Oracle(cfg, sdd), image_lr.to(dtype), crops.to(dtype), gt.to(dtype), bboxs)
    loss.backward()
    return float(loss.detach()), pred.detach(), {k: sdd[k].grad for k in names}


def test_fusion_head_gradients_land_on_the_right_parameters_and_accumulate(tiny):
    cfg, sd = tiny
    batch = train_batch()
    image_lr, crops, bboxs, gt = batch
    ref_loss, ref_pred, ref = oracle_fusion_head_grads(cfg, sd, batch)
    assert len(ref) == 44 and all(float(g.abs().max()) > 0 for g in ref.values())
    m = fusion_model(cfg, sd)
    plain, _ = m.train_forward(image_lr, crops, gt, bboxs)
    loss_dict, out = m.train_forward(image_lr, crops, gt, bboxs, head_grad=True)
    assert set(loss_dict) == {"sig_loss", "total_loss"} and set(out) == {"rgb", "depth_pred", "depth_gt"}
    assert abs(float(loss_dict["total_loss"]) - ref_loss) < 1e-4 * ref_loss and float(plain["total_loss"]) == pytest.approx(float(loss_dict["total_loss"]), rel=1e-6)
    assert rel(out["depth_pred"], ref_pred) < 2e-5
    inputs = m.head_backward()
    assert set(inputs) == {"x0", "x_blocks", "last"} and len(inputs["x_blocks"]) == 4
    assert all(torch.isfinite(t).all() and float(t.abs().max()) > 0 for t in [inputs["x0"], inputs["last"], *inputs["x_blocks"]])
    params = dict(m.named_parameters())
    with_grad = {n for n, p in params.items() if p.grad is not None}
    assert with_grad == set(ref)
    _, _, comp = oracle_fusion_head_grads(cfg, sd, batch, torch.float32)
    for n in ref:
        assert params[n].grad.shape == params[n].shape
        hold(n, params[n].grad, ref[n], comp[n])
    # the rel column of mlp.0 multiplies the fusion head's all-zero relative depth: zero gradient, like autograd's
    assert not params["conditional_log_binomial.mlp.0.weight"].grad[:, 32].any()
    first = {n: params[n].grad.clone() for n in ref}
    m.head_backward()                                             # same context again: accumulates, the same bits twice
    for n in ref:
        assert torch.equal(params[n].grad, first[n] + first[n]), n


def test_refusals(tiny):
    cfg, sd = tiny
    image_lr, crops, bboxs, gt = train_batch()
    m = fusion_model(cfg, sd)
    with pytest.raises(RuntimeError, match="no context"):
        m.head_backward()
    m.train_forward(image_lr, crops, gt, bboxs)                   # head_grad=False keeps no context
    with pytest.raises(RuntimeError, match="no context"):
        m.head_backward()
    m.train_forward(image_lr, crops, gt, bboxs, head_grad=True)
    with torch.no_grad():
        m.get_parameter("seed_projector._net.2.bias").add_(1e-3)  # a stale _version
    with pytest.raises(RuntimeError, match="changed since the forward"):
        m.head_backward()
    m16 = fusion_model(cfg, sd, compute_dtype="bf16")
    with pytest.raises(NotImplementedError, match="bf16"):
        m16.train_forward(image_lr, crops, gt, bboxs, head_grad=True)
    for kind in ("normed", "hybrid1", "hybrid2"):
        c2 = make_config(*TINY)
        c2["coarse_branch"]["bin_centers_type"] = kind
        c2["fine_branch"]["bin_centers_type"] = kind
        mb = PatchFusion(c2, compute_dtype="fp32", ops=bwd_ops).eval()
        mb.load_state_dict(synthetic_state_dict(patchfusion_spec(c2), 0), strict=True)
        with pytest.raises(NotImplementedError, match="bin_centers_type"):
            mb.train_forward(image_lr, crops, gt, bboxs, head_grad=True)


def test_sgd_step_and_refresh_head_follow_the_oracle(tiny):
    cfg, sd = tiny
    batch = train_batch()
    image_lr, crops, bboxs, gt = batch
    m = fusion_model(cfg, sd)
    head = [m.get_parameter(n) for n in BinsHead.param_names()]
    assert len(head) == 44 and all(p.requires_grad for p in head)
    assert not any(p.requires_grad for n, p in m.named_parameters() if n.startswith(("coarse_branch.", "fine_branch.")))
    opt = torch.optim.SGD(head, lr=1e-2)
    l0, _ = m.train_forward(image_lr, crops, gt, bboxs, head_grad=True)
    m.head_backward()
    opt.step()
    m.refresh_head()
    l1, out1 = m.train_forward(image_lr, crops, gt, bboxs)
    sd1 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ref_loss, ref_pred = pf_oracle.Oracle(cfg, sd1).train_forward(image_lr, crops, gt, bboxs)
    assert any(not torch.equal(sd1[k], sd[k]) for k in sd if k.startswith("seed_bin_regressor"))
    assert rel(out1["depth_pred"], ref_pred) < 2e-5 and abs(float(l1["total_loss"]) - float(ref_loss)) < 1e-4 * float(ref_loss)
    assert float(l1["total_loss"]) < float(l0["total_loss"])
    with pytest.raises(RuntimeError, match="no context"):       # refresh_head drops the context
        m.head_backward()


BRANCH = dict(midas_model_type="vits")


def test_baseline_pretrain_head_training():
    cfg = make_config(*TINY)
    bcfg = cfg["coarse_branch"]
    spec = {}
    from collections import OrderedDict
    spec = OrderedDict()
    branch_spec(spec, "coarse_branch.", bcfg)
    sd = synthetic_state_dict(spec, 0)
    m = BaselinePretrain(bcfg, cfg["fine_branch"], min_depth=cfg["min_depth"], max_depth=cfg["max_depth"], image_raw_shape=(448, 616),
                         patch_process_shape=(112, 154), patch_split_num=(2, 2), target="coarse", compute_dtype="fp32", ops=bwd_ops).eval()
    m.load_state_dict(sd, strict=True)
    assert all(p.requires_grad for p in m.parameters())           # the pretraining model trains its branch
    g = torch.Generator().manual_seed(3)
    x = torch.rand(2, 3, 112, 154, generator=g)
    gt = 0.3 + torch.rand(2, 1, 112, 154, generator=g)
    gt[:, :, :5] = 0.0
    plain, _ = m(mode="train", image_lr=x, image_hr=None, depth_gt=gt)
    loss_dict, out = m.train_forward(x, gt, head_grad=True)
    assert set(loss_dict) == {"coarse_loss", "total_loss"} and float(plain["total_loss"]) == pytest.approx(float(loss_dict["total_loss"]), rel=1e-6)
    inputs = m.head_backward()
    assert set(inputs) == {"x0", "x_blocks", "last", "rel"} and float(inputs["rel"].abs().max()) > 0
    # autograd through the oracle's branch w.r.t. the head's parameters: float64 (truth) and float32 (comparator)
    head_names = ["coarse_branch." + n for n in BinsHead.param_names()]

    def oracle(dtype):
        sdd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        for k in head_names:
            sdd[k] = sdd[k].clone().requires_grad_(True)
        depth = pf_oracle.branch_forward(sdd, "coarse_branch.", x.to(dtype), bcfg)[0]
        loss = pf_oracle.silog_loss(depth, gt.to(dtype), cfg["min_depth"], cfg["max_depth"])
        loss.backward()
        return float(loss.detach()), {k: sdd[k].grad for k in head_names}

    (loss, truth), (_, comp) = oracle(torch.float64), oracle(torch.float32)
    assert abs(loss - float(loss_dict["total_loss"])) < 1e-4 * loss
    params = dict(m.named_parameters())
    assert {n for n, p in params.items() if p.grad is not None} == set(head_names)
    for n in head_names:
        hold(n, params[n].grad, truth[n], comp[n])
    opt = torch.optim.SGD([params[n] for n in head_names], lr=1e-2)
    opt.step()
    m.refresh_head()
    l1, out1 = m.train_forward(x, gt)
    sd1 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ref = pf_oracle.branch_forward(sd1, "coarse_branch.", x, bcfg)[0]
    assert rel(out1["depth_pred"], ref) < 2e-5 and float(l1["total_loss"]) < float(loss_dict["total_loss"])
