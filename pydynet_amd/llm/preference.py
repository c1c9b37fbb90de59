"""Preference optimisation (DPO) on sequence log-probabilities, stated once in float64 array arithmetic.

    margin_b = (pc_b - pr_b) - (rc_b - rr_b)
    loss     = mean_b -logsigmoid(beta * margin_b)

pc / pr: the policy's log-probabilities of the chosen / rejected row (`Llama.sequence_logprobs`: minus the sum of the row's
token losses, ignored tokens left out); rc / rr: the reference model's, computed beforehand and held fixed.  The chosen rows
are pulled one way and the rejected rows the other, so the (tokens,) upstream gradient of the lm_head + loss node differs
in sign and size from row to row -- the case core/fused/row_loss.py exists for.

`dpo_loss` is the statement (value and both gradients); `dpo_loss_tensor` is the same loss from plain tape operators.
With z = -beta * margin the loss term is softplus(z) = (z + a) / 2 + log(1 + exp(-a)), a = max(z, -z): no exponential of a
positive number, so margins of +-80 and beyond stay finite, and no `abs`, whose backward raises (as in the reference); where
z == 0 both edges of the maximum pass the gradient and cancel, which leaves the derivative 1/2 that softplus has there.
"""
import numpy as np

from ..core import tensor
from ..core.tensor import Tensor


def dpo_loss(pc, pr, rc, rr, beta=0.1):
    """(loss, dloss/dpc, dloss/dpr) in float64"""
    pc, pr, rc, rr = (np.asarray(v, np.float64).reshape(-1) for v in (pc, pr, rc, rr))
    z = -float(beta) * ((pc - pr) - (rc - rr))
    a = np.abs(z)
    loss = (np.maximum(z, 0.0) + np.log1p(np.exp(-a))).mean()
    sig = np.where(z >= 0, 1.0 / (1.0 + np.exp(-a)), np.exp(-a) / (1.0 + np.exp(-a)))      # sigmoid(z) = dsoftplus / dz
    dpc = -float(beta) * sig / z.size
    return float(loss), dpc, -dpc


def dpo_loss_tensor(pc, pr, rc, rr, beta=0.1):
    """the loss as a tape scalar from (B,) tensors pc, pr (on the tape) and rc, rr (constants: tensors or arrays)"""
    rc, rr = (v if isinstance(v, Tensor) else Tensor(np.asarray(v, pc.dtype).reshape(-1), dtype=pc.dtype, device=pc.device)
              for v in (rc, rr))
    z = ((pc - pr) - (rc - rr)) * (-float(beta))
    a = tensor.maximum(z, z * -1.0)
    return tensor.mean((z + a) * 0.5 + tensor.log(tensor.exp(a * -1.0) + 1.0))
