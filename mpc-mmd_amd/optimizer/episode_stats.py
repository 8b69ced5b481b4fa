"""Accounting helpers both closed-loop drivers use (``optimizer/closed_loop.py`` and
``carla/closed_loop.py``).  Package-free on purpose: no relative import, so the CARLA driver, whose
own package is also named ``optimizer``, can load this file by path."""
import numpy as np


def mean_std(v):
    """(mean, sample standard deviation) of ``v``; 0.0 where there is no element, or only one."""
    v = np.asarray(v, np.float64)
    return float(v.mean()) if v.size else 0.0, float(v.std(ddof=1)) if v.size > 1 else 0.0
