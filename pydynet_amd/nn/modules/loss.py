"""Loss layers (surface of pydynet/nn/modules/loss.py): thin modules over nn/functional.py."""
from .module import Module
from .. import functional as F


class Loss(Module):
    _criterion = None                                   # the functional form a subclass applies

    def __init__(self, reduction='mean') -> None:
        super().__init__()
        assert reduction in {'mean', 'sum'}
        self.reduction = reduction

    def forward(self, y_pred, y_true):
        return type(self)._criterion(y_pred, y_true, self.reduction)


class MSELoss(Loss):
    _criterion = staticmethod(F.mse_loss)


class NLLLoss(Loss):
    _criterion = staticmethod(F.nll_loss)


class CrossEntropyLoss(Loss):
    """`ignore_index` (an extension of the reference's module; None: off) is stored and passed on to
    F.cross_entropy_loss.  reduction 'none' (an extension, this module only): the (rows,) vector of row losses.
    `label_smoothing` in [0, 1] and `z_loss` >= 0 (extensions, both 0: off) are stored and passed on likewise; under 'mean'
    with `ignore_index` both terms are averaged over the same remaining rows."""
    _criterion = staticmethod(F.cross_entropy_loss)

    def __init__(self, reduction='mean', ignore_index=None, label_smoothing=0.0, z_loss=0.0) -> None:
        super().__init__('mean' if reduction == 'none' else reduction)
        self.reduction = reduction
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self.label_smoothing, self.z_loss = float(label_smoothing), float(z_loss)
        if not 0.0 <= self.label_smoothing <= 1.0:
            raise ValueError(f"label_smoothing must lie in [0, 1], got {label_smoothing}")
        if not self.z_loss >= 0.0:
            raise ValueError(f"z_loss must be >= 0, got {z_loss}")

    def forward(self, y_pred, y_true):
        if self.label_smoothing != 0.0 or self.z_loss != 0.0:
            return F.cross_entropy_loss(y_pred, y_true, self.reduction, self.ignore_index, self.label_smoothing, self.z_loss)
        if self.ignore_index is None and self.reduction != 'none':
            return super().forward(y_pred, y_true)
        return F.cross_entropy_loss(y_pred, y_true, self.reduction, self.ignore_index)
