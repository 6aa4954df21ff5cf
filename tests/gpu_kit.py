"""What every GPU test file needs: arrays to the device and back, the list of items that differ, and the process-wide switches of
verification set for one block and put back after it."""
import contextlib

import numpy as np
import pytest

from ed_model import arr  # noqa: F401  (for the GPU tests)

# the threshold of the batch verification that holds outside a settings() block: None = the engine's default, 0 under always_combine
_rlc_min_outside = None


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()          # (a contiguous copy: shared fixtures are read-only arrays)


def dev_idx(idx):
    """uint32 indices as the int32 tensor the device form takes (0xFFFFFFFF travels as -1)"""
    return dev(np.ascontiguousarray(idx, dtype=np.uint32).view(np.int32))


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def bad(got, want):
    """the first items whose verdict is not the expected one"""
    return np.nonzero(np.asarray(host(got)) != want)[0][:10]


def _set_rlc_min(engine, items):
    engine.set_rlc_min_items(engine.RLC_MIN_ITEMS_DEFAULT if items is None else items)


@pytest.fixture()
def always_combine(engine):
    """small batches through the combination itself (by default calls below 5 x 2^15 items use the per-item kernels); a file
    whose every test wants it names it in pytest.mark.usefixtures"""
    global _rlc_min_outside
    _rlc_min_outside = 0
    _set_rlc_min(engine, 0)
    yield
    _rlc_min_outside = None
    _set_rlc_min(engine, None)


@contextlib.contextmanager
def settings(engine, *, offcurve=True, policy=0, cofactored=False, algo=0, rlc_min=None):
    """the five process-wide switches for one block.  On exit the equation, the policy, the off-curve mode and the algorithm go
    back to their defaults whatever the body did, so nothing leaks into the next test.  The threshold of the batch verification
    goes back to the value found on entry, not to the default: under always_combine that is 0 for the whole test, and a block
    that ends must not undo it.  (The engine has no getter for the threshold; always_combine records the value it set.)"""
    try:
        engine.set_verify_algo(algo)
        engine.set_offcurve_mode(offcurve)
        engine.set_verify_policy(policy)
        engine.set_verify_equation(cofactored)
        if rlc_min is not None:
            engine.set_rlc_min_items(rlc_min)
        yield
    finally:
        engine.set_verify_equation(False)
        engine.set_verify_policy(0)
        engine.set_offcurve_mode(True)
        engine.set_verify_algo(0)
        _set_rlc_min(engine, _rlc_min_outside)
