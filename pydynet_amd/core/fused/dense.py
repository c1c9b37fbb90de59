"""Projection, embedding and loss nodes: linear, embedding, cross_entropy, linear_cross_entropy (lm_head + loss as one node).
(One module of `pydynet_amd.core.fused`; the package docstring lists the reference chains each node replaces.)"""
from __future__ import annotations

import contextlib
import os

import numpy as np

from ... import _lib
from ...autograd import is_grad_enable
from ..tensor import Tensor, _Operator
from ._common import _hip, _L, _contig, _require_f32, _foldable, _beside, _is_leaf_f32, _Deferred, hip_f32
from . import masked_loss, row_loss, smooth_loss


class linear(_Deferred, _Operator):
    """y = x @ W (+ b) (+ residual) over the last axis of x; W is (in, out).

    `residual` (shape of y) folds the `z = x + sublayer(x)` add of a transformer block into the
    GEMM epilogue; its gradient is the upstream gradient itself.

    A projection `relu` could take over (float32 on the device, out features a multiple of 32, no residual) is
    created without running anything (`_Deferred`): `F.relu` of it becomes ONE `linear_relu` node, any other consumer
    reads `.data`, which runs the product then."""

    folds_existing = True      # backward adds the gradient x already holds inside the dX GEMM
    defer = True               # class switch: False runs every product at construction (no linear + relu fusion)
    _reshape_hook = True       # Tensor.reshape asks core/fused/chain.py about pending projections

    def __init__(self, x, weight, bias=None, residual=None):
        self.has_bias, self.has_res = bias is not None, residual is not None
        ins = [x, weight] + ([bias] if self.has_bias else []) + ([residual] if self.has_res else [])
        if type(self) is linear and self.defer and linear_relu.applicable(x, weight, bias, residual):
            self._init_deferred(ins, tuple(x.shape[:-1]) + (weight.shape[1],), np.float32)
        else:
            super().__init__(*ins)

    def _split(self, ins):
        b = ins[2] if self.has_bias else None
        r = ins[2 + self.has_bias] if self.has_res else None
        return ins[0], ins[1], b, r

    def forward_(self, *ins):
        x, w, b, r = self._split(ins)
        if self.xp is np:
            y = x.data @ w.data
            if b is not None:
                y = y + b.data
            return y + r.data if r is not None else y
        _require_f32(self, x, w, b, r)
        hp = _hip()
        fin, fout = w.shape
        x2 = x.data.reshape(-1, fin)
        out = hp.empty(x.shape[:-1] + (fout,), np.float32)
        res = _contig(r.data).reshape(-1, fout) if r is not None else None
        hp.gemm(x2, w.data, out.reshape(-1, fout), bias=b.data.reshape(-1) if b is not None else None,
                residual=res)
        return out

    def _dx(self, hp, g2, x, w, fin):
        dx = hp.empty(x.shape, np.float32)
        ex = _foldable(self, 0, x)
        mask = getattr(x, "_relu_bits", None) if type(x) is linear_relu else None
        if mask is not None and g2._strides[-1] == 1 and (ex is None or ex.is_contiguous()):
            # x = relu(pre-activation) of a linear_relu node: its bits applied in this product's store, so that node
            # receives the gradient of its PRE-activation (relu'(z) o (g W^T + what x already holds)) -- no relu pass
            wd = w.data
            # ... and the column sums of that gradient (the bias gradient of the layer below) leave the same store as one
            # partial row per 32 rows: no pass over dx for them
            xb = x.last[2] if (x.has_bias and len(x.last) > 2) else None
            parts = hp.empty(((g2.shape[0] + 31) // 32, fin), np.float32) if (xb is not None and xb.requires_grad) else None
            _L().call("pdn_linear_dx_masked_f32", g2._ptr, g2._strides[0], wd._ptr, wd._strides[0], wd._strides[1],
                      dx._ptr, fin, ex._ptr if ex is not None else None, mask._ptr,
                      parts._ptr if parts is not None else None, g2.shape[0], fin, wd.shape[1], hp.stream())
            dx._aux = ("relu_masked", mask, parts.sum(0) if parts is not None else None)
            return dx
        hp.gemm(g2, w.data.T, dx.reshape(-1, fin),                         # NT
                residual=ex.reshape(-1, fin) if ex is not None else None)
        return dx

    def backward_all(self, g):
        x, w, b, r = self._split(self.last)
        fin, fout = w.shape
        grads = [None] * len(self.last)
        if self.has_res and r.requires_grad:
            grads[2 + self.has_bias] = g
        if self.xp is np:
            g2, x2 = g.reshape(-1, fout), x.data.reshape(-1, fin)
            if x.requires_grad:
                grads[0] = (g2 @ w.data.T).reshape(x.shape)
            if w.requires_grad:
                grads[1] = x2.T @ g2
            if b is not None and b.requires_grad:
                grads[2] = g2.sum(0).reshape(b.shape)
            return grads
        hp = _hip()
        g2 = _contig(g).reshape(-1, fout)
        x2 = x.data.reshape(-1, fin)
        side = _beside(hp, fin, fout, x.requires_grad and w.requires_grad)
        if x.requires_grad and side is None:
            grads[0] = self._dx(hp, g2, x, w, fin)
        need_db = b is not None and b.requires_grad
        aux = getattr(g, "_aux", None)
        if need_db and aux is not None and aux[0] == "colsum" and aux[1].size == b.size:
            # the producer of g (fused cross entropy) already summed its columns
            if _is_leaf_f32(b):
                b.grad += aux[1].reshape(b.grad.shape)
            else:
                grads[2] = aux[1].reshape(b.shape)
            need_db = False
        # bias gradient = column sums of g: formed inside the dW GEMM (both read g once) when the
        # operands have the aligned x^T @ g layout and the leaf buffers can be accumulated into
        # (fusing costs ~25 % of the dW GEMM, a separate pass over g one read of it: the fusion only
        # pays for short contractions, fin < ~8 * MFMA rate / HBM rate ~ 192)
        fuse_db = (need_db and w.requires_grad and _is_leaf_f32(b) and x2.is_contiguous() and fin < 192
                   and fin % 4 == 0 and fout % 4 == 0 and x2.shape[0] % 4 == 0)
        if w.requires_grad:
            cs = b.grad.reshape(-1) if fuse_db else None
            dw = None if _is_leaf_f32(w) else hp.empty((fin, fout), np.float32)
            with side or contextlib.nullcontext():
                if dw is None:
                    hp.gemm(x2.T, g2, w.grad, beta=1.0, b_colsum=cs, colsum_accumulate=True)   # TN, += into the leaf
                else:
                    hp.gemm(x2.T, g2, dw, b_colsum=cs, colsum_accumulate=True)
                    grads[1] = dw
        if side is not None:
            grads[0] = self._dx(hp, g2, x, w, fin)
            side.join()
        if need_db and not fuse_db:
            grads[2] = g2.sum(0).reshape(b.shape)
        return grads


class linear_relu(linear):
    """relu(x @ W + b) as ONE node (examples/pydynet/mnist.py:70-78: Linear -> ReLU; nn/functional.py:31-32 relu =
    maximum(0., x), tensor.py:808-814: its gradient passes where out == x, i.e. pre-activation >= 0).

    Forward: the product stores max(0, x W + b) and one bit per element (pre-activation >= 0) -- the pre-activation
    never exists in HBM (`pdn_linear_relu_fwd_f32`).  Backward: a `linear` consumer applies the bits inside its
    input-gradient product (`linear._dx`), so the gradient arrives as that of the pre-activation; a gradient from any
    other consumer (or an accumulated one) gets the bits applied here (`pdn_relu_mask_bwd_f32`; applying them twice
    changes nothing)."""

    # below this many rows the plain product wins: it may split the contraction over workgroups to fill the chip (a 256-row
    # batch is 16 tiles), which the stores with bits cannot (measured: the 256-sample MLP step 0.205 -> 0.220 ms when fused)
    min_rows = 4096

    @staticmethod
    def applicable(x, weight, bias, residual=None):
        if (residual is not None or x.ndim < 1 or weight.ndim != 2 or not x.device.is_hip
                or not hip_f32(x, weight, bias)):
            return False
        rows = int(np.prod(x.shape[:-1], dtype=np.int64))
        return (rows >= linear_relu.min_rows and weight.shape[1] % 32 == 0 and x.shape[-1] == weight.shape[0]
                and (bias is None or bias.size == weight.shape[1]))

    def forward_(self, *ins):
        x, w, b, _ = self._split(ins)
        hp, L = _hip(), _L()
        fin, fout = w.shape
        x2 = _contig(x.data).reshape(-1, fin)
        out = hp.empty(x.shape[:-1] + (fout,), np.float32)
        self._relu_bits = hp.empty((x2.shape[0], fout // 32), np.float32)      # opaque 32-bit words
        wd = w.data
        L.call("pdn_linear_relu_fwd_f32", x2._ptr, x2._strides[0], wd._ptr, wd._strides[0], wd._strides[1],
               _contig(b.data).reshape(-1)._ptr if b is not None else None, out._ptr, fout, self._relu_bits._ptr,
               x2.shape[0], fout, fin, hp.stream())
        return out

    def backward_all(self, g):
        aux = getattr(g, "_aux", None)
        if not (aux is not None and aux[0] == "relu_masked" and aux[1] is self._relu_bits):
            hp = _hip()
            g = _contig(g)
            dz = hp.empty(g.shape, np.float32)
            _L().call("pdn_relu_mask_bwd_f32", g._ptr, self._relu_bits._ptr, dz._ptr, g.size // g.shape[-1], g.shape[-1],
                      hp.stream())
            g = dz
        elif len(aux) > 2 and aux[2] is not None:
            g._aux = ("colsum", aux[2])          # the producer summed the columns of this very array (see linear._dx)
        return super().backward_all(g)


class embedding(_Operator):
    """out = W[ids]; gradient = scatter-ASSIGN of the last occurrence of each id (reference
    semantics, tensor.py:937-940); `accumulate=True` opts into torch-style scatter-add."""

    accumulate = False

    def __init__(self, ids, weight):
        if isinstance(ids, Tensor):
            ids = ids.data
        self._ids = ids
        super().__init__(weight)

    def forward_(self, w):
        if self.xp is np:
            return w.data[self._ids]
        hp = _hip()
        if isinstance(self._ids, np.ndarray) or not hasattr(self._ids, "_ptr"):
            self._ids = hp.from_numpy(np.asarray(self._ids).astype(np.int64))
        return w.data[self._ids]

    def backward_all(self, g):
        w = self.last[0]
        # data parallel (distributed.DataParallel): per-row owner rank, so that the summed gradient keeps
        # the scatter-ASSIGN semantics of the concatenated batch; irrelevant for scatter-add
        owner = tag = None
        if getattr(w, "_dp_owner", None) is not None and not self.accumulate:
            owner, tag = w._dp_owner(self._ids, w.shape[0])
        if self.xp is np:
            full = np.zeros(w.shape, dtype=w.dtype)
            if self.accumulate:
                np.add.at(full, self._ids, g)
            elif owner is not None:
                ids = np.asarray(self._ids).reshape(-1)
                keep = owner[ids] == tag
                full[ids[keep]] = g.reshape(ids.size, -1)[keep]
            else:
                full[self._ids] = g
            return [full]
        hp, L = _hip(), _L()
        V, D = w.shape
        g = _contig(g)
        ids = _contig(self._ids)
        ws, wsb = hp.workspace(V * 4)
        optr, otag = (owner._ptr, tag) if owner is not None else (None, 0.0)
        if _is_leaf_f32(w):
            L.call("pdn_embedding_scatter_f32", g._ptr, ids._ptr, ids.size, w.grad._ptr, V, D,
                   2 if self.accumulate else 1, optr, otag, ws, wsb, hp.stream())
            return [None]
        full = hp.zeros(w.shape, np.float32)
        L.call("pdn_embedding_scatter_f32", g._ptr, ids._ptr, ids.size, full._ptr, V, D,
               2 if self.accumulate else 0, optr, otag, ws, wsb, hp.stream())
        return [full]


class cross_entropy(_Operator):
    """mean / sum over rows of  logsumexp(x_n) - x_n[t_n]   (integer targets).

    `ignore_index` (None: off, exactly the node above): rows whose target equals it add nothing to the loss and get a
    gradient row of exactly 0; 'mean' divides by the number of remaining rows.  The statement is core/fused/masked_loss.py.  With no
    row left the loss is 0 and every gradient is 0 -- torch returns NaN there; a replayed training step cannot look at its
    loss before the optimizer runs, and a NaN gradient would poison Adam's moments for good.  On a HIP device the count and
    its reciprocal stay on the device (`pdnl_*` entries of include/pdn_loss.h): nothing is read back, so the node can be
    captured in a `hipnp.Graph` and follows a targets buffer whose mask changes between replays.

    reduction 'none' (an extension; the statement is core/fused/row_loss.py): the node's value is the (rows,) vector of row
    losses, 0 at ignored rows, and its backward takes a (rows,) float32 gradient -- dlogits_n = (softmax - onehot) * g_n,
    exactly 0 at ignored rows whatever g_n holds (`pdnr_cross_entropy_bwd_rows_f32` of include/pdn_rowloss.h).  No count and
    no factor: normalisation is the caller's.

    `label_smoothing` eps / `z_loss` lam (extensions; both 0: off, exactly the node above; the statement is
    core/fused/smooth_loss.py): row_n = lse - (1 - eps) x_n[t_n] - eps mean(x_n) + lam lse^2 under every reduction and with or
    without `ignore_index`; 'mean' averages both terms over the same remaining rows.  On a HIP device the forward is one pass
    per row for the maximum, the sum of exponentials and the sum (`pdnz_cross_entropy_fwd_f32` of include/pdn_smoothloss.h),
    the backward `pdnz_cross_entropy_bwd_f32`; count and factor stay on the device."""

    def __init__(self, logits, targets, reduction="mean", ignore_index=None, label_smoothing=0.0, z_loss=0.0):
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("reduction must be mean, sum or none.")
        self.reduction = reduction
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self.smooth = label_smoothing != 0.0 or z_loss != 0.0         # (both 0: nothing of smooth_loss.py runs)
        self.label_smoothing, self.z_loss = smooth_loss.check_arguments(label_smoothing, z_loss) if self.smooth else (0.0, 0.0)
        self._t = targets.data if isinstance(targets, Tensor) else targets
        super().__init__(logits)

    def _forward_smooth(self, x):
        n, V = x.shape
        eps, lam = self.label_smoothing, self.z_loss
        if self.xp is np:
            t = np.asarray(self._t).reshape(-1)
            value = smooth_loss.value(x.data, t, eps, lam, self.ignore_index, self.reduction)
            return np.asarray(value).astype(x.dtype)
        _require_f32(self, x)
        hp, L = _hip(), _L()
        if not hasattr(self._t, "_ptr"):
            self._t = hp.from_numpy(np.asarray(self._t).astype(np.int64))
        self._x = _contig(x.data)
        self._t = _contig(self._t)
        loss_row = hp.empty((n,), np.float32)
        self._lse = hp.empty((n,), np.float32)
        by_rows = self.reduction == "none"
        out = None if by_rows else hp.empty((1,), np.float32)
        self._stats = None if by_rows else hp.empty((4,), np.float32)
        masked = self.ignore_index is not None
        L.call("pdnz_cross_entropy_fwd_f32", self._x._ptr, self._t._ptr, 1 if masked else 0, self.ignore_index if masked else 0,
               n, V, ("none", "sum", "mean").index(self.reduction), eps, lam, loss_row._ptr, self._lse._ptr,
               out._ptr if out is not None else None, self._stats._ptr if self._stats is not None else None,
               hp.err_flag_ptr(), hp.stream())
        return loss_row if by_rows else out.reshape(())

    def _backward_smooth(self, g):
        x = self.last[0]
        n, V = x.shape
        eps, lam = self.label_smoothing, self.z_loss
        by_rows = self.reduction == "none"
        if self.xp is np:
            t = np.asarray(self._t).reshape(-1)
            u = np.asarray(g, np.float64).reshape(-1) if by_rows else float(np.asarray(g))
            return [smooth_loss.cross_entropy(x.data, t, eps, lam, self.ignore_index, self.reduction, u)[1].astype(x.dtype)]
        hp, L = _hip(), _L()
        g = _contig(g)
        if by_rows:
            g = g.reshape(-1)
            if g.dtype != np.float32 or g.shape[0] != n:
                raise TypeError(f"cross_entropy(reduction='none'): the upstream gradient must be ({n},) float32, got {g.shape} {g.dtype}")
        dx = hp.empty((n, V), np.float32)
        masked = self.ignore_index is not None
        L.call("pdnz_cross_entropy_bwd_f32", self._x._ptr, self._t._ptr, 1 if masked else 0, self.ignore_index if masked else 0,
               self._lse._ptr, g._ptr if by_rows else None, None if by_rows else g._ptr,
               None if by_rows else self._stats._ptr, eps, lam, dx._ptr, n, V, hp.stream())
        return [dx]

    def _forward_rows(self, x):
        """reduction 'none': the rows the forward entries leave anyway (every variant of them writes loss_row and lse_row)"""
        n, V = x.shape
        if self.xp is np:
            t = np.asarray(self._t).reshape(-1)
            row_loss.check_targets(t, self.ignore_index, V)
            self._valid = row_loss.valid_rows(t, self.ignore_index)
            self._ts = np.where(self._valid, t, 0)
            m = x.data.max(-1, keepdims=True)
            self._lse = np.log(np.exp(x.data - m).sum(-1, keepdims=True)) + m
            return np.where(self._valid, self._lse[:, 0] - x.data[np.arange(n), self._ts], 0).astype(x.dtype)
        _require_f32(self, x)
        hp, L = _hip(), _L()
        if not hasattr(self._t, "_ptr"):
            self._t = hp.from_numpy(np.asarray(self._t).astype(np.int64))
        self._x = _contig(x.data)
        self._t = _contig(self._t)
        loss_row = hp.empty((n,), np.float32)
        self._lse = hp.empty((n,), np.float32)
        out = hp.empty((1,), np.float32)
        if self.ignore_index is not None:
            stats = hp.empty((4,), np.float32)
            L.call("pdnl_cross_entropy_fwd_f32", self._x._ptr, self._t._ptr, self.ignore_index, n, V, 0, loss_row._ptr,
                   self._lse._ptr, out._ptr, stats._ptr, hp.err_flag_ptr(), hp.stream())
        else:
            L.call("pdn_cross_entropy_fwd_f32", self._x._ptr, self._t._ptr, n, V, 0, loss_row._ptr, self._lse._ptr, out._ptr,
                   hp.err_flag_ptr(), hp.stream())
        return loss_row

    def _backward_rows(self, g):
        x = self.last[0]
        n, V = x.shape
        if self.xp is np:
            sm = np.exp(x.data - self._lse)
            sm[np.arange(n), self._ts] -= 1
            sm *= np.where(self._valid, np.asarray(g, x.dtype).reshape(-1), 0)[:, None]
            sm[~self._valid] = 0
            return [sm]
        hp, L = _hip(), _L()
        g = _contig(g).reshape(-1)
        if g.dtype != np.float32 or g.shape[0] != n:
            raise TypeError(f"cross_entropy(reduction='none'): the upstream gradient must be ({n},) float32, got {g.shape} {g.dtype}")
        dx = hp.empty((n, V), np.float32)
        masked = self.ignore_index is not None
        L.call("pdnr_cross_entropy_bwd_rows_f32", self._x._ptr, self._t._ptr, 1 if masked else 0,
               self.ignore_index if masked else 0, self._lse._ptr, g._ptr, dx._ptr, n, V, hp.stream())
        return [dx]

    def forward_(self, x):
        n, V = x.shape
        if self.smooth:
            return self._forward_smooth(x)
        if self.reduction == "none":
            return self._forward_rows(x)
        if self.xp is np:
            t = np.asarray(self._t)
            m = x.data.max(-1, keepdims=True)
            self._lse = np.log(np.exp(x.data - m).sum(-1, keepdims=True)) + m
            if self.ignore_index is not None:
                masked_loss.check_targets(t, self.ignore_index, V)
                self._valid = masked_loss.valid_rows(t, self.ignore_index)
                self._ts = np.where(self._valid, t, 0)
                self._factor = masked_loss.scale(t, self.ignore_index, self.reduction)[1]
                rows = np.where(self._valid, self._lse[:, 0] - x.data[np.arange(n), self._ts], 0)
                return (rows.sum() * np.asarray(self._factor, x.dtype)).astype(x.dtype)
            rows = self._lse[:, 0] - x.data[np.arange(n), t]
            return rows.mean() if self.reduction == "mean" else rows.sum()
        _require_f32(self, x)
        hp, L = _hip(), _L()
        if not hasattr(self._t, "_ptr"):
            self._t = hp.from_numpy(np.asarray(self._t).astype(np.int64))
        self._x = _contig(x.data)
        self._t = _contig(self._t)
        loss_row = hp.empty((n,), np.float32)
        self._lse = hp.empty((n,), np.float32)
        out = hp.empty((1,), np.float32)
        mean = 1 if self.reduction == "mean" else 0
        self._dx = None
        from ...autograd import is_grad_enable
        if self.ignore_index is not None:
            # the masked entries: the count and 1 / count are device scalars (`_stats`), read by the kernels themselves
            self._stats = hp.empty((4,), np.float32)
            if x.requires_grad and is_grad_enable():
                self._dx = hp.empty((n, V), np.float32)
                wsb = L.query("pdnl_cross_entropy_colsum_workspace_bytes", n, V)
                cs = hp.empty((V,), np.float32) if wsb else None
                ws, wsb = hp.workspace(wsb) if wsb else (None, 0)
                L.call("pdnl_cross_entropy_fwd_bwd_f32", self._x._ptr, self._t._ptr, self.ignore_index, n, V, mean,
                       loss_row._ptr, self._lse._ptr, out._ptr, self._stats._ptr, self._dx._ptr,
                       cs._ptr if cs is not None else None, ws, wsb, hp.err_flag_ptr(), hp.stream())
                self._dx._aux = ("colsum", cs) if cs is not None else None
            else:
                L.call("pdnl_cross_entropy_fwd_f32", self._x._ptr, self._t._ptr, self.ignore_index, n, V, mean, loss_row._ptr,
                       self._lse._ptr, out._ptr, self._stats._ptr, hp.err_flag_ptr(), hp.stream())
            return out.reshape(())
        if x.requires_grad and is_grad_enable():
            # the gradient w.r.t. the logits needs nothing computed later: write it now, while each
            # row is still in L2 (one pass over HBM for forward + backward)
            self._dx = hp.empty((n, V), np.float32)
            # column sums of dlogits (= the bias gradient of the Linear that made the logits) come
            # for free while the rows stream through; handed to that Linear via the array's `_aux`
            wsb = L.query("pdn_cross_entropy_colsum_workspace_bytes", n, V)
            cs = hp.empty((V,), np.float32) if wsb else None
            ws, wsb = hp.workspace(wsb) if wsb else (None, 0)
            L.call("pdn_cross_entropy_fwd_bwd_f32", self._x._ptr, self._t._ptr, n, V, mean,
                   1.0 / n if mean else 1.0, loss_row._ptr, self._lse._ptr, out._ptr, self._dx._ptr,
                   cs._ptr if cs is not None else None, ws, wsb, hp.err_flag_ptr(), hp.stream())
            self._dx._aux = ("colsum", cs) if cs is not None else None
        else:
            L.call("pdn_cross_entropy_fwd_f32", self._x._ptr, self._t._ptr, n, V, mean, loss_row._ptr,
                   self._lse._ptr, out._ptr, hp.err_flag_ptr(), hp.stream())
        return out.reshape(())

    def backward_all(self, g):
        if self.smooth:
            return self._backward_smooth(g)
        if self.reduction == "none":
            return self._backward_rows(g)
        x = self.last[0]
        n, V = x.shape
        scale = 1.0 / n if self.reduction == "mean" else 1.0
        if self.xp is np:
            sm = np.exp(x.data - self._lse)
            if self.ignore_index is not None:
                sm[np.arange(n), self._ts] -= 1
                sm[~self._valid] = 0
                return [sm * (g * np.asarray(self._factor, x.dtype))]
            sm[np.arange(n), np.asarray(self._t)] -= 1
            return [sm * (g * np.asarray(scale, x.dtype))]
        hp, L = _hip(), _L()
        g = _contig(g)
        if self._dx is not None:
            dx, self._dx = self._dx, None       # written in forward; apply the upstream scalar (1 -> no-op)
            L.call("pdn_scale_by_device_scalar_f32", dx._ptr, dx.size, g._ptr, hp.stream())
            aux = getattr(dx, "_aux", None)
            if aux is not None:
                L.call("pdn_scale_by_device_scalar_f32", aux[1]._ptr, aux[1].size, g._ptr, hp.stream())
            return [dx]
        dx = hp.empty((n, V), np.float32)
        if self.ignore_index is not None:
            L.call("pdnl_cross_entropy_bwd_f32", self._x._ptr, self._t._ptr, self.ignore_index, self._lse._ptr, g._ptr,
                   self._stats._ptr, dx._ptr, n, V, hp.stream())
            return [dx]
        L.call("pdn_cross_entropy_bwd_f32", self._x._ptr, self._t._ptr, self._lse._ptr, g._ptr,
               scale, dx._ptr, n, V, hp.stream())
        return [dx]


class linear_cross_entropy(_Operator):
    """loss = cross_entropy(x @ W + b, targets) as ONE tape node (llm/llama/model.py:179 feeding
    nn/functional.py:364-381): the (rows, V) gradient of the logits never exists in memory.  Forward: the
    logits GEMM and one read-only pass for the row statistics (log-sum-exp, loss).  Backward: the two products
    `dlogits @ W^T` and `x^T @ dlogits` (and the column sums for the bias) form
    dlogits = (softmax - onehot) * scale from the saved logits as they consume it (`pdn_linear_ce_backward_f32`).
    Versus linear + cross_entropy nodes: one (rows x V) write and none of its re-reads less.
    Deferred form (training step): the input-gradient product runs in the FORWARD pass (it is where the sum of exponentials
    comes from), so (i) a forward under grad mode that is never followed by `backward()` still pays that product -- wrap
    validation losses in `no_grad()` -- and (ii) dx is formed from the weights as they are at forward time: updating the
    weight IN PLACE between forward and backward leaves dx consistent with the forward pass (as the reference's tape is)
    but not with a dW computed from the new weights; `backward_all` asserts that the weight buffer is still the one
    forward read.
    `ignore_index` (None: off, exactly the node above; the contract is `cross_entropy`'s, core/fused/masked_loss.py): the products
    stay the kernels they are.  `pdnl_linear_ce_finish_f32` takes the place of the loss-from-lse launch: it leaves the count
    and 1 / count on the device, a copy of the targets with V on every ignored row and an lse of +inf there, with which both
    terms of dlogits the weight-gradient product forms are exactly 0 on those rows; under 'mean' the products run with
    gscale 1 and the upstream device scalar carries 1 / count.  `pdnl_linear_ce_backward_f32` then sets the rows of ignored
    tokens in dx to 0 (the input-gradient kernels subtract a gathered weight column whatever the row).  Nothing is folded
    into dx on this path.  On the `cpu` device the node is the NumPy statement of the same contract.
    reduction 'none' (the statement is core/fused/row_loss.py): the value is the (rows,) vector of row losses and backward
    takes a (rows,) float32 gradient u.  The products again stay the kernels they are, and take one upstream scalar; the
    per-row factor goes around them (`pdnr_linear_ce_backward_rows_f32` of include/pdn_rowloss.h): dx is the product with
    gscale 1, its rows scaled by u afterwards (ignored rows set to 0); dW = (diag(u / s) x)^T (s dz) from a scaled copy of x
    with s = max |u| as the product's device scalar; dbias, which the product can only sum unweighted, is one more pass over
    the saved logits, run only when the bias needs a gradient.  Nothing is read back, so the node replays from a
    `hipnp.Graph` over changing targets and weights.
    `label_smoothing` eps / `z_loss` lam (both 0: off, exactly the node above; the statement is core/fused/smooth_loss.py):
    the three products still stay the kernels they are and the two terms go around them (`pdnz_*` entries of
    include/pdn_smoothloss.h).  Forward: the row sums of W once (mean_v z_n = (x_n . wsum + bsum) / V, no pass over the
    logits) and a finish that takes the place of the others.  Backward: dz_n = u'_n (p - onehot) + c_n onehot - e_n with
    u' = u a, a = 1 + 2 lam lse, c = u (2 lam lse + eps), e = u eps / V: the reduction='none' backward above runs unchanged
    under the upstream vector u' (for 'mean' / 'sum' u is the upstream scalar times the device-resident factor), then
    `pdnz_linear_ce_corrections_f32` adds c_n W[:, t_n] - e_n wsum to dx rows and, per class, the c-weighted sum of its x rows
    minus sum_n e_n x_n to the columns of dW (a workgroup owns a range of classes and walks all targets in row order: no sort,
    no atomics, two runs give the same bits), the same with x_n = 1 to dbias."""

    folds_existing = True
    enabled = True
    min_rows = int(os.environ.get("PDN_LINCE_MIN_ROWS", "16384"))
    lse_epilogue = os.environ.get("PDN_NO_LSE_EPILOGUE", "0") != "1"      # row statistics in the projection's store (A/B switch)
    # statistics split over the projection (row maxima) and the input-gradient product (sum of exponentials), the latter
    # run in the forward pass of a training step (A/B switch)
    deferred_norm = os.environ.get("PDN_NO_CE_DEFERRED", "0") != "1"
    # the projection of the deferred form on split-fp16 MFMA where the library takes the shape (csrc/lm_head_split.hip).
    # The library reads PDN_LMHEAD_SPLIT=0 itself (`pdn_linear_rowmax_split_supported` then answers 0); this attribute is
    # the in-process form of the same A/B switch.
    split_forward = True
    # the same for the input-gradient product of the deferred form (csrc/lm_head_dx_split.hip; library switch
    # PDN_LMHEAD_DX_SPLIT=0, after which `pdn_linear_ce_dx_deferred_split_supported` answers 0)
    split_dx = True
    # the same for the weight gradient (csrc/lm_head_dw_split.hip; library switch PDN_LMHEAD_DW_SPLIT=0).  This product has
    # no entry of its own: `pdn_linear_ce_backward_f32` takes the split form when the workspace holds its extra region --
    # the LAST (rows / 32) * 37888 + 1152 bytes of `pdn_linear_ce_workspace_bytes` for rows >= 32768 and V >= 128
    # (include/pdn_hip.h) -- so the in-process form of the switch is to hand it the workspace without that region.
    split_dw = True

    @staticmethod
    def _dw_split_extra(rows, V):
        return (rows // 32) * 37888 + 1152 if (rows >= 32768 and V >= 128) else 0

    @staticmethod
    def applicable(x, w, b, targets, reduction="mean", ignore_index=None, label_smoothing=0.0, z_loss=0.0):
        if label_smoothing != 0.0 or z_loss != 0.0:
            smooth_loss.check_arguments(label_smoothing, z_loss)
        if not (linear_cross_entropy.enabled and x.device.is_hip and x.dtype == np.float32 and w.dtype == np.float32
                and (b is None or b.dtype == np.float32) and reduction in ("mean", "sum", "none") and w.ndim == 2):
            return False
        rows = 1
        for d in x.shape[:-1]:
            rows *= d
        t = targets.data if isinstance(targets, Tensor) else targets
        # (below 28672 tokens the row workgroups of the output-resident input-gradient kernel no longer fill the chip:
        #  it then cuts K = vocabulary into ranges over the grid, pdn_gemm_outres_plan; below `min_rows` the separate
        #  nodes on the tiled kernels are left in place)
        return (x.shape[-1] == w.shape[0] and getattr(t, "ndim", 0) == 1 and t.shape[0] == rows
                and rows >= linear_cross_entropy.min_rows
                and bool(_L().query("pdn_linear_ce_supported", rows, w.shape[1], w.shape[0])))

    def __init__(self, x, weight, bias, targets, reduction="mean", ignore_index=None, label_smoothing=0.0, z_loss=0.0):
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("reduction must be mean, sum or none.")
        self.reduction = reduction
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self.smooth = label_smoothing != 0.0 or z_loss != 0.0         # (both 0: nothing of smooth_loss.py runs)
        self.label_smoothing, self.z_loss = smooth_loss.check_arguments(label_smoothing, z_loss) if self.smooth else (0.0, 0.0)
        self.has_bias = bias is not None
        self._t = targets.data if isinstance(targets, Tensor) else targets
        super().__init__(*([x, weight] + ([bias] if self.has_bias else [])))

    def _forward_np(self, x, w, b):
        x2 = x.data.reshape(-1, w.shape[0])
        z = x2 @ w.data
        if b is not None:
            z = z + b.data.reshape(-1)
        n, V = z.shape
        t = np.asarray(self._t).reshape(-1)
        if self.smooth:
            self._saved = (x2, z, t)
            value = smooth_loss.value(z, t, self.label_smoothing, self.z_loss, self.ignore_index, self.reduction)
            return np.asarray(value).astype(z.dtype)
        if self.reduction == "none":
            row_loss.check_targets(t, self.ignore_index, V)
            valid = row_loss.valid_rows(t, self.ignore_index)
            ts, factor = np.where(valid, t, 0), 1.0
        elif self.ignore_index is None:
            valid, ts, factor = np.ones(n, bool), t, (1.0 / n if self.reduction == "mean" else 1.0)
        else:
            masked_loss.check_targets(t, self.ignore_index, V)
            valid = masked_loss.valid_rows(t, self.ignore_index)
            ts, factor = np.where(valid, t, 0), masked_loss.scale(t, self.ignore_index, self.reduction)[1]
        m = z.max(-1, keepdims=True)
        lse = np.log(np.exp(z - m).sum(-1, keepdims=True)) + m
        rows = np.where(valid, lse[:, 0] - z[np.arange(n), ts], 0)
        self._saved = (x2, z, lse, valid, ts, factor)
        if self.reduction == "none":
            return rows.astype(z.dtype)
        return (rows.sum() * np.asarray(factor, z.dtype)).astype(z.dtype)

    def _backward_np(self, g):
        x, w = self.last[0], self.last[1]
        b = self.last[2] if self.has_bias else None
        if self.smooth:
            x2, z, t = self._saved
            u = np.asarray(g, np.float64).reshape(-1) if self.reduction == "none" else float(np.asarray(g))
            d = smooth_loss.cross_entropy(z, t, self.label_smoothing, self.z_loss, self.ignore_index, self.reduction,
                                          u)[1].astype(z.dtype)
        else:
            x2, z, lse, valid, ts, factor = self._saved
            d = np.exp(z - lse)
            d[np.arange(len(ts)), ts] -= 1
            if self.reduction == "none":
                d *= np.where(valid, np.asarray(g, z.dtype).reshape(-1), 0)[:, None]      # (an ignored row's g may hold anything)
            else:
                d *= g * np.asarray(factor, z.dtype)
            d[~valid] = 0
        self._saved = None
        grads = [None] * len(self.last)
        if x.requires_grad:
            grads[0] = (d @ w.data.T).reshape(x.shape)
        if w.requires_grad:
            grads[1] = x2.T @ d
        if b is not None and b.requires_grad:
            grads[2] = d.sum(0).reshape(b.shape)
        return grads

    def forward_(self, x, w, b=None):
        if self.xp is np:
            return self._forward_np(x, w, b)
        _require_f32(self, x, w, b)
        hp, L = _hip(), _L()
        fin, V = w.shape
        x2 = _contig(x.data).reshape(-1, fin)
        n = x2.shape[0]
        masked = self.ignore_index is not None
        by_rows = self.reduction == "none"
        smooth = self.smooth
        if not hasattr(self._t, "_ptr"):
            self._t = hp.from_numpy(np.asarray(self._t).astype(np.int64))
        self._t = _contig(self._t)
        logits = hp.empty((n, V), np.float32)
        loss_row, lse, out = hp.empty((n,), np.float32), hp.empty((n,), np.float32), hp.empty((1,), np.float32)
        wd = w.data
        in_gemm = bool(wd.is_contiguous() and x2._strides[1] == 1 and L.query("pdn_linear_lse_supported", n, V, fin))
        self.deferred = bool(linear_cross_entropy.deferred_norm and wd.is_contiguous() and x2._strides[1] == 1
                             and is_grad_enable() and x.requires_grad
                             and L.query("pdn_linear_rowmax_supported", n, V, fin)
                             and L.query("pdn_linear_ce_dx_deferred_supported", n, V, fin))
        self.stats_in_gemm = bool(linear_cross_entropy.lse_epilogue and in_gemm and not self.deferred)
        self._dxu = None
        bp = b.data._ptr if b is not None else None
        mean = 1 if self.reduction == "mean" else 0
        if masked:
            # what the finish leaves for the backward: {count, 1 / count, upstream / count} and the sanitised targets
            self._stats, self._t_safe = hp.empty((4,), np.float32), hp.empty((n,), np.int64)
        elif by_rows:
            self._t_safe = hp.empty((n,), np.int64)
        if smooth:
            self._t_safe = hp.empty((n,), np.int64)
            if not masked and not by_rows:
                self._stats = hp.empty((4,), np.float32)
            # the row sums of W (and the sum of the bias) for mean_v z_n, formed once from the weights this forward reads
            self._wsum = hp.empty((fin + 1,), np.float32) if self.label_smoothing != 0.0 else None

        def finish():
            if smooth:
                wc = _contig(wd)
                if self._wsum is not None:
                    L.call("pdnz_weight_sums_f32", wc._ptr, bp, fin, V, self._wsum._ptr, hp.stream())
                L.call("pdnz_linear_ce_finish_f32", logits._ptr, V, lse._ptr, self._t._ptr, 1 if masked else 0,
                       self.ignore_index if masked else 0, x2._ptr, x2._strides[0],
                       self._wsum._ptr if self._wsum is not None else None, n, V, fin,
                       ("none", "sum", "mean").index(self.reduction), self.label_smoothing, self.z_loss, loss_row._ptr,
                       None if by_rows else out._ptr, None if by_rows else self._stats._ptr, self._t_safe._ptr,
                       hp.err_flag_ptr(), hp.stream())
            elif by_rows:
                # the masked finish without its reduction: loss_row is the node's value
                L.call("pdnr_linear_ce_finish_rows_f32", logits._ptr, V, lse._ptr, self._t._ptr, 1 if masked else 0,
                       self.ignore_index if masked else 0, n, V, loss_row._ptr, self._t_safe._ptr, hp.err_flag_ptr(),
                       hp.stream())
            elif masked:
                L.call("pdnl_linear_ce_finish_f32", logits._ptr, V, lse._ptr, self._t._ptr, self.ignore_index, n, V, mean,
                       loss_row._ptr, out._ptr, self._stats._ptr, self._t_safe._ptr, hp.err_flag_ptr(), hp.stream())
            else:
                L.call("pdn_cross_entropy_from_lse_f32", logits._ptr, V, lse._ptr, self._t._ptr, n, V, mean, loss_row._ptr,
                       out._ptr, hp.err_flag_ptr(), hp.stream())
        if self.deferred:
            # the projection leaves the row maxima; the input-gradient product -- it needs exp(logit - max) anyway, and not
            # the upstream gradient, a scalar applied in backward -- sums the exponentials as it multiplies: it runs HERE,
            # the loss follows from its log-sum-exp with one gather per row, and no pass over the logits exists
            # (few rows: both products cut the vocabulary into ranges over the grid -- `parts` vectors of maxima, a
            #  workspace of unnormalised rows and row sums)
            split = bool(linear_cross_entropy.split_forward and x2._strides[0] % 4 == 0
                         and _lib.provides("pdn_linear_rowmax_split_fwd_f32")
                         and L.query("pdn_linear_rowmax_split_supported", n, V, fin))
            if split:
                # both operands split into two fp16 planes, three f16 MFMAs per k-step: fp32 accuracy at 3/16 of the fp32
                # pipe's cycles.  The planes live in the per-stream scratch for this launch only (the next call below
                # takes the same scratch, in stream order).
                parts = L.query("pdn_linear_rowmax_split_parts", n, V, fin)
                rowmax = hp.empty((parts * n,), np.float32)
                ws, wsb = hp.workspace(L.query("pdn_linear_rowmax_split_workspace_bytes", n, V, fin))
                L.call("pdn_linear_rowmax_split_fwd_f32", x2._ptr, wd._ptr, bp, logits._ptr, rowmax._ptr, n, V, fin,
                       x2._strides[0], V, V, ws, wsb, hp.stream())
            else:
                parts = L.query("pdn_linear_rowmax_parts", n, V, fin)
                rowmax = hp.empty((parts * n,), np.float32)
                L.call("pdn_linear_rowmax_fwd_f32", x2._ptr, wd._ptr, bp, logits._ptr, rowmax._ptr, n, V, fin,
                       x2._strides[0], V, V, hp.stream())
            self._dxu = hp.empty((n, fin), np.float32)
            self._w_ptr = wd._ptr                          # (backward checks that the weight was not re-homed meanwhile)
            # the logits split on the fly, W once per call: the same three-product form as the projection above
            dx_entry = "pdn_linear_ce_dx_deferred_f32"
            if (linear_cross_entropy.split_dx and _lib.provides("pdn_linear_ce_dx_deferred_split_f32")
                    and L.query("pdn_linear_ce_dx_deferred_split_supported", n, V, fin)):
                dx_entry = "pdn_linear_ce_dx_deferred_split_f32"
            ws, wsb = hp.workspace(L.query(dx_entry.replace("_f32", "_workspace_bytes"), n, V, fin))
            # (masked: unscaled -- 1 / count is not known yet and is applied with the upstream scalar; the kernel clamps the
            #  target whose column it subtracts, and the rows of ignored tokens are set to 0 in backward)
            L.call(dx_entry, logits._ptr, rowmax._ptr, parts, self._t._ptr,
                   1.0 / n if (mean and not masked and not smooth) else 1.0, wd._ptr, self._dxu._ptr, lse._ptr, n, V, fin, ws, wsb,
                   hp.stream())
            finish()
        elif self.stats_in_gemm:
            # the projection leaves the rows' log-sum-exp itself (transposed accumulators: a lane owns a token): no
            # pass over the logits for the statistics, the loss is one gather per row
            L.call("pdn_linear_lse_fwd_f32", x2._ptr, wd._ptr, bp, logits._ptr, lse._ptr, n, V, fin, x2._strides[0], V, V,
                   hp.stream())
            finish()
        elif masked:
            # statistics by a pass over the logits (which skips the ignored rows); the finish then masks their lse
            hp.gemm(x2, wd, logits, bias=b.data.reshape(-1) if b is not None else None)
            L.call("pdnl_cross_entropy_fwd_f32", logits._ptr, self._t._ptr, self.ignore_index, n, V, mean, loss_row._ptr, lse._ptr,
                   out._ptr, self._stats._ptr, hp.err_flag_ptr(), hp.stream())
            finish()
        else:
            hp.gemm(x2, wd, logits, bias=b.data.reshape(-1) if b is not None else None)
            L.call("pdn_cross_entropy_fwd_f32", logits._ptr, self._t._ptr, n, V, mean, loss_row._ptr, lse._ptr, out._ptr,
                   hp.err_flag_ptr(), hp.stream())
            if by_rows or smooth:
                finish()
        self._saved = (x2, logits, lse)
        return loss_row if by_rows else out.reshape(())

    def backward_all(self, g):
        if self.xp is np:
            return self._backward_np(g)
        hp, L = _hip(), _L()
        x, w = self.last[0], self.last[1]
        b = self.last[2] if self.has_bias else None
        fin, V = w.shape
        masked = self.ignore_index is not None
        x2, logits, lse = self._saved
        self._saved = None
        n = x2.shape[0]
        g = _contig(g)
        by_rows = self.reduction == "none"
        if by_rows:
            g = g.reshape(-1)
            if g.dtype != np.float32 or g.shape[0] != n:
                raise TypeError(f"linear_cross_entropy(reduction='none'): the upstream gradient must be ({n},) float32, "
                                f"got {g.shape} {g.dtype}")
        smooth = self.smooth
        if smooth:
            # the row coefficients; from here on the node is the reduction='none' node under the upstream vector u'
            up, cn = hp.empty((n,), np.float32), hp.empty((n,), np.float32)
            en = hp.empty((n,), np.float32)
            L.call("pdnz_row_coefficients_f32", lse._ptr, self._t_safe._ptr, g._ptr if by_rows else None,
                   None if by_rows else g._ptr, None if by_rows else self._stats._ptr, self.label_smoothing, self.z_loss, n, V,
                   up._ptr, cn._ptr, en._ptr, hp.stream())
            g, by_rows = up, True
        grads = [None] * len(self.last)
        dx = ex = None
        dxu, self._dxu = self._dxu, None
        if dxu is not None and getattr(self, "_w_ptr", None) not in (None, w.data._ptr):
            raise RuntimeError("linear_cross_entropy: the weight's buffer was replaced between forward and backward; the "
                               "input gradient of the deferred form was formed from the forward pass's weights")
        if x.requires_grad and dxu is not None:
            if not masked and not by_rows:
                dxu *= g.reshape(())                       # formed in the forward pass, up to the upstream scalar
            grads[0] = dxu.reshape(x.shape)
        elif x.requires_grad:
            dx = hp.empty(x.shape, np.float32)
            ex = _foldable(self, 0, x) if not (masked or by_rows) else None
            grads[0] = dx
        dw, dw_beta = None, 0.0
        if w.requires_grad:
            if _is_leaf_f32(w):
                dw, dw_beta = w.grad, 1.0
            else:
                dw = grads[1] = hp.empty((fin, V), np.float32)
        db, db_beta = None, 0.0
        if b is not None and b.requires_grad:
            if _is_leaf_f32(b):
                db, db_beta = b.grad.reshape(-1), 1.0
            else:
                db = hp.empty((V,), np.float32)
                grads[2] = db.reshape(b.shape)
        if by_rows:
            # the bias gradient is a pass of its own over the logits (the product sums its columns unweighted): it is not
            # asked of the product, and it runs first, so it shares the products' scratch
            cneed = L.query("pdnr_weighted_colsum_workspace_bytes", n, V) if db is not None else 0
            need = L.query("pdn_linear_ce_workspace_bytes", n, V, fin) if dw is not None else 0
            ws, got = hp.workspace(max(need, cneed)) if max(need, cneed) else (None, 0)
            wsb = got if dw is not None else 0
            if dw is not None and not linear_cross_entropy.split_dw and need > linear_cross_entropy._dw_split_extra(n, V):
                wsb = need - linear_cross_entropy._dw_split_extra(n, V)
            xs = hp.empty((n, fin), np.float32) if dw is not None else None       # diag(u / s) x
            s_dev = hp.empty((2,), np.float32) if dw is not None else None        # {s, 1 / s}
            dxd = dxu if (x.requires_grad and dxu is not None) else None
            L.call("pdnr_linear_ce_backward_rows_f32", x2._ptr, x2._strides[0], logits._ptr, lse._ptr, self._t_safe._ptr,
                   g._ptr, w.data._ptr, dx._ptr if dx is not None else None, dxd._ptr if dxd is not None else None,
                   dw._ptr if dw is not None else None, dw_beta, db._ptr if db is not None else None, db_beta,
                   xs._ptr if xs is not None else None, s_dev._ptr if s_dev is not None else None, n, V, fin,
                   ws if wsb else None, wsb, ws if cneed else None, cneed, hp.stream())
            if smooth:
                # the target-column and the uniform term, added to what the call above left (dw_beta / db_beta are in it)
                dxc = dxd if dxd is not None else dx
                zneed = L.query("pdnz_linear_ce_corrections_workspace_bytes", n, V, fin) if self._wsum is not None else 0
                zws, zwsb = hp.workspace(zneed) if zneed else (None, 0)
                L.call("pdnz_linear_ce_corrections_f32", x2._ptr, x2._strides[0], _contig(w.data)._ptr,
                       self._wsum._ptr if self._wsum is not None else None, self._t_safe._ptr, cn._ptr,
                       en._ptr if self._wsum is not None else None, dxc._ptr if dxc is not None else None,
                       dw._ptr if dw is not None else None, db._ptr if db is not None else None, n, V, fin, zws, zwsb,
                       hp.stream())
            return grads
        need = L.query("pdn_linear_ce_workspace_bytes", n, V, fin) if (dw is not None or db is not None) else 0
        ws, wsb = hp.workspace(need) if need else (None, 0)
        if not linear_cross_entropy.split_dw and need > linear_cross_entropy._dw_split_extra(n, V):
            wsb = need - linear_cross_entropy._dw_split_extra(n, V)     # (the scratch buffer itself may be larger than asked for)
        if masked:
            dxd = dxu if (x.requires_grad and dxu is not None) else None
            L.call("pdnl_linear_ce_backward_f32", x2._ptr, x2._strides[0], logits._ptr, lse._ptr, self._t_safe._ptr,
                   self._stats._ptr, g._ptr, w.data._ptr, dx._ptr if dx is not None else None,
                   dxd._ptr if dxd is not None else None, dw._ptr if dw is not None else None, dw_beta,
                   db._ptr if db is not None else None, db_beta, n, V, fin, ws, wsb, hp.stream())
            return grads
        L.call("pdn_linear_ce_backward_f32", x2._ptr, x2._strides[0], logits._ptr, lse._ptr, self._t._ptr,
               1.0 / n if self.reduction == "mean" else 1.0, g._ptr, w.data._ptr,
               dx._ptr if dx is not None else None, ex._ptr if ex is not None else None,
               dw._ptr if dw is not None else None, dw_beta, db._ptr if db is not None else None, db_beta,
               n, V, fin, ws, wsb, hp.stream())
        return grads
