"""tests/fake_ops.py plus the backward ops of csrc/head_bwd.hip, each backed by its restatement in tests/head_bwd_ref.py (float64 inside,
written back in the buffer's dtype).  Plugged in as ``ops`` the way tests/test_train_forward_cpu.py plugs the forward's fake ops, so the
engine's backward wiring -- which buffer feeds which kernel, padding, channel maps, accumulation -- is checked on the CPU."""
import torch

from tests import head_bwd_ref as R
from tests.fake_ops import FakeOps, _as4

F64 = torch.float64


class FakeBwdOps(FakeOps):
    name = "fake+bwd"

    @staticmethod
    def conv1x1_wgrad(dy, x, dw, db=None, rows_per_block=0):
        N, K = dw.shape
        w, b = R.wgrad(_as4(dy)[..., :N].to(F64), _as4(x)[..., :K].to(F64))
        assert torch.isfinite(w).all(), "weight gradient read a never-written value"
        dw.copy_(w)
        if db is not None:
            db.copy_(b)
        return dw, db

    @staticmethod
    def resize_bwd(dy, dx, accumulate=False):
        g = R.resize_bwd(dy.to(F64), dx.shape[1], dx.shape[2])
        dx.copy_(dx.to(F64) + g if accumulate else g)
        return dx

    @staticmethod
    def attractor_bwd(A, n_attr, b_prev, d_b_new, dA, d_b_c, attractor_type="inv", kind="mean"):
        a, c = R.attractor_bwd(A[..., :n_attr].to(F64), b_prev.to(F64), d_b_new.to(F64), attractor_type, kind)
        dA[..., :n_attr] = a
        d_b_c.copy_(c)
        return dA, d_b_c

    @staticmethod
    def logbinom_depth_bwd(pt, centers, d_depth, d_pt, d_centers_up, min_temp, max_temp):
        p, c = R.logbinom_bwd(pt[..., :4].to(F64), centers.to(F64), d_depth.to(F64), min_temp, max_temp)
        d_pt[..., :4] = p
        d_centers_up.copy_(c)
        return d_pt, d_centers_up

    @staticmethod
    def act_bwd(dy, ref, act):
        d4, r4 = _as4(dy), _as4(ref)
        d4.copy_(R.act_bwd(d4.to(F64), r4[..., :d4.shape[-1]].to(F64), act))
        return dy

    @staticmethod
    def silog_loss_saved(pred, target, min_depth, max_depth, beta=0.15):
        n, s1, s2 = R.silog_sums(pred.to(F64), target.to(F64), min_depth, max_depth)
        sums = torch.tensor([n, float(s1), float(s2)], dtype=F64, device=pred.device)
        return FakeOps.silog_loss(pred, target, min_depth, max_depth, beta), sums

    @staticmethod
    def silog_loss_bwd(pred, target, sums, d_pred, min_depth, max_depth, beta=0.15, d_loss=1.0):
        n, s1, s2 = R.silog_sums(pred.to(F64), target.to(F64), min_depth, max_depth)
        assert float(sums[0]) == n and abs(float(sums[1]) - float(s1)) <= 1e-9 * max(1.0, abs(float(s1))), "the sums are not this forward's"
        d_pred.copy_(R.silog_bwd(pred.to(F64), target.to(F64), min_depth, max_depth, beta, d_loss))
        return d_pred


ops = FakeBwdOps()
