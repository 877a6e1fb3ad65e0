"""float64 references and bounds derived from them that several kernel test modules share."""
import numpy as np


def ln_ref(x, w, b, eps, dtype=np.float64):
    """two passes: mean, biased variance around it, eps inside the root"""
    x = x.astype(dtype)
    mean = x.mean(-1, keepdims=True, dtype=dtype)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True, dtype=dtype)
    return d / np.sqrt(var + dtype(eps)) * w.astype(dtype) + b.astype(dtype)


def ln_bound(x, w, b, eps, kinds=None):
    """8x the largest error of a FLOAT32 numpy restatement of the same two-pass formula against the float64 reference on the test's own
    inputs (the reference's arithmetic, not the kernel's; the factor covers another summation order and rsqrtf).  Where a test mixes
    rows of different kinds (`kinds`: one label per row) the largest error is taken per kind, so that a row of mean 100 does not widen
    the bound of the benign rows beside it.  Figures measured on a module's inputs are in the docstrings of its tests."""
    ref = ln_ref(x, w, b, eps)
    e32 = np.abs(ln_ref(x, w, b, eps, np.float32).astype(np.float64) - ref).max(-1)
    kinds = np.zeros(x.shape[0], int) if kinds is None else np.asarray(kinds)
    bound = np.empty((x.shape[0], 1))
    for kd in np.unique(kinds):
        bound[kinds == kd, 0] = 8 * e32[kinds == kd].max()
    return ref, bound
