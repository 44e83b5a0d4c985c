"""Moment transforms (the counterpart of lettuce/util/moments.py): ``moment_tensor``, ``get_default_moment_transform``,
``Transform`` and its four implementations, with the reference's signatures and behaviour.  As in the reference the
module is not star-imported: ``from lettuce_amd.moments import D2Q9Lallemand``.

The matrices are data, kept here as the project's own tables: the two D2Q9 bases as integer numerators over one
denominator per entry, the Hermite basis of D3Q27 generated from the lattice (products of the Hermite polynomials 1, c,
c^2 - 1/3 of the velocity components; its inverse from the orthogonality of that basis under the lattice weights).  Every
entry is a ratio of small integers divided once, i.e. the same double as the literal of the reference's table
(lettuce_amd/csrc/mrt.hpp holds the same tables for the kernels; tests/test_mrt_kernel_host.py compares the two).  The
equilibria keep the reference's formulas as they are, oddities included.  Device tensors do not go through BLAS
(``_flow.local_contract``).
"""
import math
import warnings
from fractions import Fraction
from typing import List

import numpy as np
import torch

from ._errors import LettuceException, InefficientCodeWarning, ExperimentalWarning
from ._stencil import Stencil, D1Q3, D2Q9, D3Q27

__all__ = ["moment_tensor", "get_default_moment_transform", "Moments", "Transform", "D1Q3Transform", "D2Q9Lallemand",
           "D2Q9Dellar", "D3Q27Hermite"]


def moment_tensor(e: List[List[int]], multiindex):
    """prod_a e_qa ** multiindex_a for every velocity (lettuce/util/moments.py:34-38)"""
    if isinstance(e, torch.Tensor):
        return torch.prod(torch.pow(e, multiindex[..., None, :]), dim=-1)
    return np.prod(np.power(e, multiindex[..., None, :]), axis=-1)


def get_default_moment_transform(stencil: "Stencil", context: "Context"):
    if stencil == D1Q3 or isinstance(stencil, D1Q3):
        return D1Q3Transform(stencil, context)
    if stencil == D2Q9 or isinstance(stencil, D2Q9):
        return D2Q9Lallemand(stencil, context)
    raise LettuceException(f"No default moment transform for lattice {stencil}.")


class Moments:
    def __init__(self, lattice):
        self.rho = moment_tensor(lattice.e, lattice.convert_to_tensor(np.zeros(lattice.D)))
        self.j = moment_tensor(lattice.e, lattice.convert_to_tensor(np.eye(lattice.D)))


def _table(rows):
    """a matrix of ratios (Fraction or int) as doubles: one correctly rounded division per entry"""
    return np.array([[float(Fraction(v)) for v in row] for row in rows])


def _ratios(rows, denominator):
    """integer numerators over one denominator"""
    return _table([[Fraction(v, denominator) for v in row] for row in rows])


class Transform:
    """Base class that defines the signature for all moment (and cumulant) transforms."""

    def __init__(self, stencil: "Stencil", context: "Context", names=None):
        self.context = context
        self.names = [f"m{i}" for i in range(stencil.q)] if names is None else names
        self.stencil = stencil

    def __getitem__(self, moment_names):
        if not isinstance(moment_names, tuple):
            moment_names = [moment_names]
        return [self.names.index(name) for name in moment_names]

    def transform(self, f):
        return f

    def inverse_transform(self, m):
        return m

    def equilibrium(self, m: torch.Tensor, flow: "Flow"):
        """A very inefficient and basic implementation of the equilibrium moments: back to populations, their
        quadratic equilibrium, forward again.  (The reference's text passes the populations to ``flow.rho`` and
        ``flow.u`` behind a stray ``None`` and raises a TypeError after the warning, lettuce/util/moments.py:92-93;
        this is what it means to compute.)"""
        warnings.warn("Transform.equilibrium is a poor man's implementation of the moment equilibrium. Please consider "
                      "implementing the equilibrium moments for your transform by hand.", InefficientCodeWarning)
        f = self.inverse_transform(m)
        feq = flow.equilibrium(flow, flow.rho(f), flow.u(f))
        return self.transform(feq)

    def einsum(self, equation, fields, *args) -> torch.Tensor:
        """Einstein summation on local fields."""
        inputs, output = equation.split("->")
        inputs = inputs.split(",")
        for i, inp in enumerate(inputs):
            if len(inp) == len(fields[i].shape):
                pass
            elif len(inp) == len(fields[i].shape) - self.stencil.d:
                inputs[i] += "..."
                if not output.endswith("..."):
                    output += "..."
            else:
                assert False, "Bad dimension."
        equation = ",".join(inputs) + "->" + output
        return torch.einsum(equation, fields, *args)

    def mv(self, m, v) -> torch.Tensor:
        """matrix-vector multiplication"""
        if v.is_cuda:           # no BLAS on device tensors (see _flow.local_contract)
            from ._flow import local_contract
            return local_contract(m, v)
        return self.einsum("ij,j->i", [m, v])


class _MatrixTransform(Transform):
    """a linear transform given by the class attributes ``matrix`` and ``inverse`` (numpy), which every instance
    converts to tensors of its context"""

    def __init__(self, stencil: "Stencil", context: "Context"):
        super().__init__(stencil, context, self.names)
        self.matrix = self.context.convert_to_tensor(self.matrix)
        self.inverse = self.context.convert_to_tensor(self.inverse)

    def transform(self, f):
        return self.mv(self.matrix, f)

    def inverse_transform(self, m):
        return self.mv(self.inverse, m)


class D1Q3Transform(_MatrixTransform):
    matrix = _ratios([[1, 1, 1], [0, 1, -1], [0, 1, 1]], 1)
    inverse = _ratios([[2, 0, -2], [0, 1, 1], [0, -1, 1]], 2)
    names = ["rho", "j", "e"]
    supported_stencils = [D1Q3]


class D2Q9Dellar(_MatrixTransform):
    matrix = _ratios([[2, 2, 2, 2, 2, 2, 2, 2, 2],
                      [0, 2, 0, -2, 0, 2, -2, -2, 2],
                      [0, 0, 2, 0, -2, 2, 2, -2, -2],
                      [-3, 6, -3, 6, -3, 6, 6, 6, 6],
                      [0, 0, 0, 0, 0, 18, -18, 18, -18],
                      [-3, -3, 6, -3, 6, 6, 6, 6, 6],
                      [2, -4, -4, -4, -4, 8, 8, 8, 8],
                      [0, -4, 0, 4, 0, 8, -8, -8, 8],
                      [0, 0, -4, 0, 4, 8, 8, -8, -8]], 2)
    inverse = _ratios([[96, 0, 0, -32, 0, -32, 24, 0, 0],
                       [24, 72, 0, 16, 0, -8, -12, -18, 0],
                       [24, 0, 72, -8, 0, 16, -12, 0, -18],
                       [24, -72, 0, 16, 0, -8, -12, 18, 0],
                       [24, 0, -72, -8, 0, 16, -12, 0, 18],
                       [6, 18, 18, 4, 6, 4, 6, 9, 9],
                       [6, -18, 18, 4, -6, 4, 6, -9, 9],
                       [6, -18, -18, 4, 6, 4, 6, -9, -9],
                       [6, 18, -18, 4, -6, 4, 6, 9, -9]], 216)
    names = ["rho", "jx", "jy", "Pi_xx", "Pi_xy", "PI_yy", "N", "Jx", "Jy"]
    supported_stencils = [D2Q9]

    def equilibrium(self, m, flow: "Flow"):
        warnings.warn("I am not 100% sure if this equilibrium is correct.", ExperimentalWarning)
        meq = torch.zeros_like(m)
        rho = m[0]
        jx = m[1]
        jy = m[2]
        meq[0] = rho
        meq[1] = jx
        meq[2] = jy
        meq[3] = jx * jx / rho * 9 / 2
        meq[4] = jx * jy / rho * 9
        meq[5] = jy * jy / rho * 9 / 2
        return meq


class D2Q9Lallemand(_MatrixTransform):
    matrix = _ratios([[1, 1, 1, 1, 1, 1, 1, 1, 1],
                      [0, 1, 0, -1, 0, 1, -1, -1, 1],
                      [0, 0, 1, 0, -1, 1, 1, -1, -1],
                      [0, 1, -1, 1, -1, 0, 0, 0, 0],
                      [0, 0, 0, 0, 0, 1, -1, 1, -1],
                      [-4, -1, -1, -1, -1, 2, 2, 2, 2],
                      [0, -2, 0, 2, 0, 1, -1, -1, 1],
                      [0, 0, -2, 0, 2, 1, 1, -1, -1],
                      [4, -2, -2, -2, -2, 1, 1, 1, 1]], 1)
    inverse = _ratios([[4, 0, 0, 0, 0, -4, 0, 0, 4],
                       [4, 6, 0, 9, 0, -1, -6, 0, -2],
                       [4, 0, 6, -9, 0, -1, 0, -6, -2],
                       [4, -6, 0, 9, 0, -1, 6, 0, -2],
                       [4, 0, -6, -9, 0, -1, 0, 6, -2],
                       [4, 6, 6, 0, 9, 2, 3, 3, 1],
                       [4, -6, 6, 0, -9, 2, -3, 3, 1],
                       [4, -6, -6, 0, 9, 2, -3, -3, 1],
                       [4, 6, -6, 0, -9, 2, 3, -3, 1]], 36)
    names = ["rho", "jx", "jy", "pxx", "pxy", "e", "qx", "qy", "eps"]
    supported_stencils = [D2Q9]

    def equilibrium(self, m, flow: "Flow"):
        """From Lallemand and Luo"""
        warnings.warn("I am not 100% sure if this equilibrium is correct.", ExperimentalWarning)
        meq = torch.zeros_like(m)
        rho = m[0]
        jx = m[1]
        jy = m[2]
        c1 = -2
        alpha2 = -8
        alpha3 = 4
        gamma1 = 2 / 3
        gamma2 = 18
        gamma3 = 2 / 3
        gamma4 = -18
        meq[0] = rho
        meq[1] = jx
        meq[2] = jy
        meq[3] = 1 / 2 * gamma1 * (jx ** 2 - jy ** 2)
        meq[4] = 1 / 2 * gamma3 * (jx * jy)
        meq[5] = 1 / 4 * alpha2 * rho + 1 / 6 * gamma2 * (jx ** 2 + jy ** 2)
        meq[6] = 1 / 2 * c1 * jx
        meq[7] = 1 / 2 * c1 * jy
        meq[8] = 1 / 4 * alpha3 * rho + 1 / 6 * gamma4 * (jx ** 2 + jy ** 2)
        return meq


# the Hermite moments of D3Q27: powers of (x, y, z) per moment, in the order of the names
_HERMITE_NAMES = ["rho", "jx", "jy", "jz",
                  "Pi_xx", "Pi_xy", "PI_xz", "PI_yy", "PI_yz", "PI_zz",
                  "J_xxy", "J_xxz", "J_xyy", "J_xyz", "J_xzz", "J_yyz", "J_yzz",
                  "J_xxyy", "J_xxyz", "J_xxzz", "J_xyyz", "J_xyzz", "J_yyzz",
                  "J_xxyyz", "J_xxyzz", "J_xyyzz", "J_xyxzyz"]
_HERMITE_POWERS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1),
                   (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2),
                   (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 2, 1), (0, 1, 2),
                   (2, 2, 0), (2, 1, 1), (2, 0, 2), (1, 2, 1), (1, 1, 2), (0, 2, 2),
                   (2, 2, 1), (2, 1, 2), (1, 2, 2), (2, 2, 2)]


def _hermite(degree, c):
    """H_0 = 1, H_1 = c, H_2 = c^2 - 1/3 of a velocity component"""
    return (Fraction(1), Fraction(c), Fraction(c * c) - Fraction(1, 3))[degree]


def _hermite_tables():
    e = D3Q27().e
    weight = {0: Fraction(2, 3), 1: Fraction(1, 6), -1: Fraction(1, 6)}       # of one velocity component
    norm = (Fraction(1), Fraction(1, 3), Fraction(2, 9))                       # sum_c w(c) H_a(c)^2
    matrix = [[math.prod(_hermite(a, c) for a, c in zip(powers, v)) for v in e] for powers in _HERMITE_POWERS]
    inverse = [[math.prod(weight[c] * _hermite(a, c) / norm[a] for a, c in zip(powers, v)) for powers in _HERMITE_POWERS]
               for v in e]
    return _table(matrix), _table(inverse)


class D3Q27Hermite(_MatrixTransform):
    matrix, inverse = _hermite_tables()
    names = _HERMITE_NAMES
    supported_stencils = [D3Q27]

    def equilibrium(self, m, flow: "Flow"):
        meq = torch.zeros_like(m)
        rho = m[0]
        jx = m[1]
        jy = m[2]
        jz = m[3]
        meq[0] = rho
        meq[1] = jx
        meq[2] = jy
        meq[3] = jz
        meq[4] = jx * jx / rho
        meq[5] = jx * jy / rho
        meq[6] = jx * jz / rho
        meq[7] = jy * jy / rho
        meq[8] = jy * jz / rho
        meq[9] = jz * jz / rho
        meq[10] = jx * jx * jy / rho ** 2
        meq[11] = jx * jx * jz / rho ** 2
        meq[12] = jx * jy * jy / rho ** 2
        meq[13] = jx * jy * jz / rho ** 2
        meq[14] = jx * jz * jz / rho ** 2
        meq[15] = jy * jy * jz / rho ** 2
        meq[16] = jy * jz * jz / rho ** 2
        meq[17] = jx * jx * jy * jy / rho ** 3
        meq[18] = jx * jx * jy * jz / rho ** 3
        meq[19] = jx * jx * jz * jz / rho ** 3
        meq[20] = jx * jy * jy * jz / rho ** 3
        meq[21] = jx * jy * jz * jz / rho ** 3
        meq[22] = jy * jy * jz * jz / rho ** 3
        meq[23] = jx * jx * jy * jy * jz / rho ** 4
        meq[24] = jx * jx * jy * jz * jz / rho ** 4
        meq[25] = jx * jy * jy * jz * jz / rho ** 4
        meq[26] = jx * jy * jx * jz * jy * jz / rho ** 5
        return meq
