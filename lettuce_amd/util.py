"""Exceptions, warnings and the small numerical helpers the hot path's callers need.

Mirrors the public names of lettuce/util/utility.py:21-34 (exception/warning classes),
:37-99 (``torch_gradient``), :119-156 (``torch_jacobi``, on the engine's ``lt_jacobi`` for device
tensors) and :158-161 (``append_axes``) of the reference.  IO helpers (HDF5, datasets),
``grid_fine_to_coarse`` and moment transforms are out of scope.
"""
import inspect

import torch

from ._errors import LettuceException, LettuceWarning, InefficientCodeWarning, ExperimentalWarning
from ._native import NativeEngineError

__all__ = ["LettuceException", "LettuceWarning", "InefficientCodeWarning", "ExperimentalWarning",
           "NativeEngineError", "torch_gradient", "torch_jacobi", "append_axes", "get_subclasses"]


def get_subclasses(cls, module):
    for _, obj in inspect.getmembers(module):
        if hasattr(obj, "__bases__") and cls in obj.__bases__:
            yield obj


# central finite-difference weights on a periodic grid, keyed by order of accuracy:
# (weight, offset) pairs such that d/dx g(x) ~ sum w * g(x + offset)
_CENTRAL = {
    2: ((-1 / 2, -1), (1 / 2, 1)),
    4: ((1 / 12, -2), (-2 / 3, -1), (2 / 3, 1), (-1 / 12, 2)),
    6: ((-1 / 60, -3), (3 / 20, -2), (-3 / 4, -1), (3 / 4, 1), (-3 / 20, 2), (1 / 60, 3)),
}


def torch_gradient(f, dx=1, order=2):
    """First derivative of a periodic 2-D/3-D field along every axis; returns ``[dim, *f.shape]``.

    Same stencils, term order and final ``* 1/dx`` as lettuce/util/utility.py:37-99
    (``g(x + k)`` is ``roll(g, -k)``), so that TGV initialisation matches to rounding."""
    if f.ndim not in (2, 3):
        raise LettuceException("Invalid dimension!")
    if order not in _CENTRAL:
        raise LettuceException(f"order {order} not implemented (2, 4, 6)")
    with torch.no_grad():
        out = torch.empty((f.ndim,) + tuple(f.shape), dtype=f.dtype, device=f.device)
        scale = torch.tensor(1.0 / dx, dtype=f.dtype, device=f.device)
        for axis in range(f.ndim):
            acc = None
            for weight, offset in _CENTRAL[order]:
                term = weight * torch.roll(f, shifts=-offset, dims=axis)
                acc = term if acc is None else acc + term
            out[axis] = acc * scale
    return out


def _jacobi_engine(f, p, dim):
    """the engine's library when lt_jacobi takes these arguments, else None: contiguous fp32 / fp64 device tensors of
    one shape whose number of axes is ``dim`` (2 or 3), and a library that loads"""
    from . import _native
    if not (isinstance(f, torch.Tensor) and isinstance(p, torch.Tensor)):
        return None
    if (p.device.type != "cuda" or f.device != p.device or p.dtype not in _native.DTYPE_IDS or f.dtype != p.dtype
            or dim not in (2, 3) or p.ndim != dim or f.shape != p.shape or p.numel() == 0
            or not p.is_contiguous() or not f.is_contiguous()):
        return None
    try:
        return _native.load_library()
    except NativeEngineError:
        return None


def torch_jacobi(f, p, dx, dim, tol_abs=1e-10, max_num_steps=100000):
    """Jacobi solver for the periodic pressure-Poisson equation lap(p) = f (lettuce/util/utility.py:119-156): the
    reference's signature, stopping rule and result.

    Contiguous fp32 / fp64 device tensors with ``dim == p.ndim`` go to the engine (``lt_jacobi``: one fused sweep per
    iteration with the reference's arithmetic operation for operation, the mean squared residuum in fp64 in a fixed
    order, the stopping rule held on the device and read by the host once per batch of sweeps); everything else --
    CPU tensors, other dtypes, views, a ``dim`` that is not the field's, no library -- runs the reference's torch
    expression below, which synchronises with the device on every sweep (``error > tol_abs``)."""
    if _jacobi_engine(f, p, dim) is not None:
        from . import _native
        return _native.jacobi(f, p, dx, tol_abs, max_num_steps)[0]
    return _jacobi_expression(f, p, dx, dim, tol_abs, max_num_steps)


def _jacobi_expression(f, p, dx, dim, tol_abs, max_num_steps):
    """torch_jacobi as whole-field torch expressions, on any device"""
    if dim not in (2, 3):
        raise LettuceException("Invalid dimension!")
    taps = 2 * dim
    dx2 = dx ** 2

    def neighbours(q):
        # the reference's order: the lower neighbour along every axis, then the upper ones, added from the left
        shifted = [q.roll(shifts=shift, dims=axis) for shift in (1, -1) for axis in range(dim)]
        total = shifted[0]
        for term in shifted[1:]:
            total = total + term
        return total

    error, it = 1, 0
    while error > tol_abs and it < max_num_steps:
        it += 1
        p = (f * dx2 - neighbours(p)) * -1 / taps
        residuum = f - (neighbours(p) - taps * p) / dx2
        error = torch.mean(residuum ** 2)
    return p


def append_axes(array, n):
    """Append ``n`` singleton axes (lettuce/util/utility.py:158-161)."""
    index = (Ellipsis,) + (None,) * n
    return array[index]
