"""BaselinePretrain (single-branch models): oracle vs the reference's own outputs (tests/golden/reference_live.npz,
made by oracle/make_golden.py live),
engine wiring (torch reference ops) vs oracle, checkpoint surface."""
import os
import random

import numpy as np
import pytest
import torch

from oracle import pf_oracle
from oracle.make_golden import stored_diff
from patchfusion_amd.baseline import BaselinePretrain
from patchfusion_amd.config import zoe_branch_config
from patchfusion_amd.spec import branch_spec, synthetic_state_dict
from tests.fake_ops import ops as fake_ops
from collections import OrderedDict

PS, RAW, SPLIT = (112, 154), (448, 616), (2, 2)


def _setup(target):
    bc = zoe_branch_config("vits", PS)
    spec = OrderedDict()
    branch_spec(spec, f"{target}_branch.", bc)
    sd = synthetic_state_dict(spec, 0)
    img = torch.rand(1, 3, *RAW, generator=torch.Generator().manual_seed(1234))
    return bc, sd, img


@pytest.mark.parametrize("target,mode", [("coarse", "m1"), ("fine", "m1"), ("fine", "r1")])
def test_engine_wiring_matches_oracle(target, mode):
    bc, sd, img = _setup(target)
    m = BaselinePretrain(bc, bc, dict(type="SILogLoss"), 1e-3, 80, RAW, PS, SPLIT, target=target, ops=fake_ops).eval()
    assert list(m.state_dict().keys()) == list(sd.keys())
    m.load_dict({k[len(target) + 8:]: v for k, v in sd.items()})          # checkpoints carry un-prefixed keys
    assert set(m.get_save_dict()) == {k[len(target) + 8:] for k in sd}
    lr = m.resizer(img)
    random.seed(5621)
    d, _ = m(mode="infer", image_lr=lr, image_hr=img, cai_mode=mode, process_num=2)
    random.seed(5621)
    o = pf_oracle.BaselineOracle(bc, PS, RAW, SPLIT, sd, target).infer(lr, img, mode, 2)
    assert d.shape == o.shape and (d - o).abs().max() < 2e-5


@pytest.mark.parametrize("target,mode", [("coarse", "m1"), ("fine", "m2"), ("fine", "r1")])
def test_oracle_matches_reference_live(golden_dir, target, mode):
    """the reference's own BaselinePretrain.forward(mode='infer') on this case (oracle/make_golden.py live)"""
    g = np.load(os.path.join(golden_dir, "reference_live.npz"))
    bc, sd, img = _setup(target)
    o = pf_oracle.BaselineOracle(bc, PS, RAW, SPLIT, sd, target)
    lr = o.resizer(img)
    random.seed(5621)
    o = o.infer(lr, img, mode, 2)
    assert stored_diff(g, f"baseline_{target}_{mode}", o) < 1e-5


def _train_batch(target):
    g = torch.Generator().manual_seed(77)
    x = torch.rand(2, 3, *PS, generator=g)
    gt = torch.rand(2, 1, 56, 77, generator=g) * 3 + 0.2                 # coarser ground-truth grid: SILogLoss resizes the prediction
    gt[0, 0, :5] = 0.0                                                   # invalid rows (below min_depth)
    return x, gt


@pytest.mark.parametrize("target", ["coarse", "fine"])
def test_train_mode_forward_value_matches_oracle(target):
    """baseline_pretrain.py:347-363 forward value (loss + prediction) through the engine wiring"""
    bc, sd, _ = _setup(target)
    m = BaselinePretrain(bc, bc, dict(type="SILogLoss"), 1e-3, 80, RAW, PS, SPLIT, target=target, ops=fake_ops).eval()
    m.load_dict({k[len(target) + 8:]: v for k, v in sd.items()})
    x, gt = _train_batch(target)
    kw = dict(image_lr=x, image_hr=None, depth_gt=gt) if target == "coarse" else dict(image_lr=x, image_hr=None, crops_image_hr=x, crop_depths=gt)
    loss, aux = m(mode="train", **kw)
    want, pred = pf_oracle.BaselineOracle(bc, PS, RAW, SPLIT, sd, target).train_forward(x, gt)
    assert set(loss) == {f"{target}_loss", "total_loss"} and loss["total_loss"] is loss[f"{target}_loss"]
    assert abs(float(loss["total_loss"]) - float(want)) <= 2e-5 * max(1.0, abs(float(want)))
    assert aux["depth_pred"].shape == pred.shape and (aux["depth_pred"] - pred).abs().max() < 2e-5
    assert aux["rgb"] is x and aux["depth_gt"] is gt


@pytest.mark.parametrize("target", ["coarse", "fine"])
def test_train_mode_oracle_matches_reference_live(golden_dir, target):
    """the reference's own BaselinePretrain.forward(mode='train') value (loss + prediction) on this batch (oracle/make_golden.py live).
    The prediction bound is 2e-5, as for the engine above: float32 rounding of this pass depends on the host CPU's conv kernels, and the
    oracle on another host sits 1.29e-5 from the stored reference (0 on the host that made it)."""
    g = np.load(os.path.join(golden_dir, "reference_live.npz"))
    loss = float(g[f"baseline_train_{target}_total_loss"])
    bc, sd, _ = _setup(target)
    x, gt = _train_batch(target)
    want, pred = pf_oracle.BaselineOracle(bc, PS, RAW, SPLIT, sd, target).train_forward(x, gt)
    assert abs(loss - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    assert stored_diff(g, f"baseline_train_{target}_depth_pred", pred) < 2e-5
