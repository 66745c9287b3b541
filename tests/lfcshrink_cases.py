"""Count matrices the lfcShrink tests share (tests/test_lfcshrink_cpu.py, tests/test_gpu_lfcshrink.py)."""
from collections import OrderedDict

import numpy as np


def counts(n, x, seed):
    from deseq2_amd import simulate
    k = simulate.make_counts(n, x, seed=seed, drop_all_zero=False)["counts"]
    k[9] = 0                                                   # an all-zero gene
    return k


def spiked(seed=23):
    """two groups of 8 with spiked outliers (replaced and refitted by DESeq()); row 5 becomes all zero once its one count is
    replaced"""
    from deseq2_amd import core
    f = OrderedDict(condition=np.repeat([0, 1], 8))
    x, _ = core.standard_model_matrix(f)
    k = counts(300, x, seed)
    rng = np.random.default_rng(seed)
    for g in rng.choice(np.arange(20, 300), 12, replace=False):
        k[g, rng.integers(0, 16)] += 20000
    k[5] = 0
    k[5, 3] = 5000
    return f, x, k
