"""Device buffers for the Python mirrors (bfv.py, tfhe.py): torch is the allocator and the copy engine, nothing more.  torch
is imported on first use, so the package stays importable without it."""
import numpy as np


def torch():
    import torch as _t

    return _t


def to_dev(x):
    """u64 words (any array-like) -> an int64 device tensor of the same shape"""
    return torch().from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64)).cuda()


def from_dev(t):
    """an int64 device tensor -> its words as a u64 numpy array"""
    return t.cpu().numpy().view(np.uint64)
