"""Seeding (engine/utils/seed.py of the reference: ``set_random_seed(seed)`` before the runner is built).

One call seeds every generator the hot path can draw from -- Python, NumPy, torch CPU and every visible GPU -- and pins
``PYTHONHASHSEED`` for child processes.  Returns the seed so launch scripts can log it."""
import os
import random

import numpy
import torch

_SEEDERS = (random.seed, numpy.random.seed, torch.manual_seed)
# what a TrainLoop built after this call takes for ``deterministic`` when its config has no ``train_cfg.deterministic`` key (the counterpart of the reference's
# ``cudnn.deterministic = True`` beside its seeds, engine/utils/misc.py:60): the fixed-order forms of the training step's reductions
_DETERMINISTIC_DEFAULT = False


def deterministic_default() -> bool:
    return _DETERMINISTIC_DEFAULT


def set_random_seed(seed: int = 42, deterministic=None) -> int:
    """``deterministic``: True / False sets the default of ``TrainLoop.deterministic``; None (``set_random_seed(42)``) leaves it as it is."""
    global _DETERMINISTIC_DEFAULT
    if deterministic is not None:
        _DETERMINISTIC_DEFAULT = bool(deterministic)
    seed = int(seed)
    for seeder in _SEEDERS:
        seeder(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)          # includes the current device
    os.environ["PYTHONHASHSEED"] = str(seed)
    return seed
