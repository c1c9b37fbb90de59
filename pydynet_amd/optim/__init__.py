from .optimizer import Optimizer, SGD, Adagrad, Adadelta, Adam, AdamW
from .lr_scheduler import ExponentialLR, StepLR, MultiStepLR, CosineAnnealingLR
