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
    F.cross_entropy_loss.  reduction 'none' (an extension, this module only): the (rows,) vector of row losses."""
    _criterion = staticmethod(F.cross_entropy_loss)

    def __init__(self, reduction='mean', ignore_index=None) -> None:
        super().__init__('mean' if reduction == 'none' else reduction)
        self.reduction = reduction
        self.ignore_index = None if ignore_index is None else int(ignore_index)

    def forward(self, y_pred, y_true):
        if self.ignore_index is None and self.reduction != 'none':
            return super().forward(y_pred, y_true)
        return F.cross_entropy_loss(y_pred, y_true, self.reduction, self.ignore_index)
