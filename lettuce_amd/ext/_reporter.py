"""Observables read between steps ("next" row F3) and the reporter that logs them.

API of lettuce/ext/_reporter/observable_reporter.py:17-199.  On a native context the
kinetic energy, the maximum velocity, the enstrophy and the Mass observable are device-side
wavefront/LDS reductions in fp64 (``lt_kinetic_energy``, ``lt_max_velocity``, ``lt_enstrophy``,
``lt_mass_interior``); the enstrophy uses one [d, *res] scratch field for u, the others none.
The energy spectrum is one ``torch.fft.fftn`` of the velocity field and one binning reduction on the
device (``lt_energy_spectrum``: integer bins, fp64, fixed order); neither path builds the
reference's [*res, K] wave mask, so the observable runs at the engine's grid sizes.
The force on a bounce-back body (``BoundaryForce`` and the drag and lift coefficients, which the reference snapshot
does not have) is a momentum-exchange sum over the body's surface links: ``lt_boundary_force`` reads one byte per
node and the populations of surface nodes only, in fp64 with a fixed order.
VTK / HDF5 / image writers are host-side post-processing and out of scope.
"""
import math
import sys
from abc import ABC, abstractmethod
from typing import Optional

import numpy as np
import torch

from .._errors import LettuceException
from .._native import SPECTRUM_MAX_BINS
from .._simulation import Reporter
from ..util import torch_gradient
from ._boundary import InterpolatedBounceBackBoundary

__all__ = ["Observable", "ObservableReporter", "MaximumVelocity", "IncompressibleKineticEnergy",
           "Enstrophy", "EnergySpectrum", "Mass", "BoundaryForce", "DragCoefficient", "LiftCoefficient",
           "ErrorReporter"]


class Observable(ABC):
    def __init__(self, flow: "Flow"):
        self.context = flow.context
        self.flow = flow

    @abstractmethod
    def __call__(self, f: Optional[torch.Tensor] = None):
        ...


class MaximumVelocity(Observable):
    """max |u| in physical units (observable_reporter.py:27-31); a device max-reduction on a
    native context."""

    def __call__(self, f: Optional[torch.Tensor] = None):
        plan = self.flow._engine_plan(self.flow.f)
        if plan is not None:
            return self.flow.units.convert_velocity_to_pu(plan.max_velocity_lu(self.flow.f))
        return torch.norm(self.flow.u_pu, dim=0).max()


class IncompressibleKineticEnergy(Observable):
    """E_pu = sum_x 0.5 u_lu.u_lu * (u_char_pu / u_char_lu)^2 * dx_pu^d  -- the parity metric of
    the north star (lettuce/ext/_reporter/observable_reporter.py:34-42)."""

    def __call__(self, f: Optional[torch.Tensor] = None):
        flow = self.flow
        dx = flow.units.convert_length_to_pu(1.0)
        plan = flow._engine_plan(flow.f)
        if plan is not None:
            total = plan.kinetic_energy_lu(flow.f)      # fp64 device scalar
        else:
            total = torch.sum(flow.incompressible_energy())
        kin = flow.units.convert_incompressible_energy_to_pu(total)
        kin *= dx ** flow.stencil.d
        return kin


class Enstrophy(Observable):
    """Integral of the squared vorticity; periodic domains only
    (observable_reporter.py:45-68)."""

    def __call__(self, f: Optional[torch.Tensor] = None):
        flow = self.flow
        dx = flow.units.convert_length_to_pu(1.0)
        plan = flow._engine_plan(flow.f) if flow.stencil.d >= 2 else None
        if plan is not None:
            # device reduction (lt_enstrophy): u into one scratch field, then the vorticity stencil
            total = plan.enstrophy_sum(flow.f, flow.units.convert_velocity_to_pu(1.0), 1.0 / dx)
            return (total * dx ** flow.stencil.d).to(flow.f.dtype)
        u = flow.units.convert_velocity_to_pu(flow.u())
        grad = [torch_gradient(u[a], dx=dx, order=6) for a in range(flow.stencil.d)]
        w_z = grad[0][1] - grad[1][0]
        total = torch.sum(w_z * w_z)
        if flow.stencil.d == 3:
            w_x = grad[2][1] - grad[1][2]
            w_y = grad[0][2] - grad[2][0]
            total += torch.sum(w_x * w_x + w_y * w_y)
        return total * dx ** flow.stencil.d


def spectrum_bins(resolution, device=None):
    """``(bins, K)`` of the reference's wave mask (observable_reporter.py:78-97), in integers: ``bins`` [*resolution],
    int64, holds the bin of every Fourier mode and ``K`` is the number of bins.  Index i on an axis of extent n has the
    wavenumber k = fftfreq(n, 1 / n)[i]; with m = sum_a k_a^2 the bin is 0 for m = 0 and else the n >= 1 with
    n^2 - n < m <= n^2 + n, which is the reference's n - 0.5 < |k| <= n + 0.5 squared (an integer m never ties with
    n^2 + n + 1/4).  K = isqrt(max m), the reference's int(max |k|); modes with a bin >= K belong to no bin."""
    d = len(resolution)
    m = torch.zeros([1] * d, dtype=torch.int64, device=device)
    for a, n in enumerate(resolution):
        i = torch.arange(n, dtype=torch.int64, device=device)
        k = torch.where(i < (n + 1) // 2, i, i - n)
        m = m + (k * k).reshape([-1 if b == a else 1 for b in range(d)])
    # a first guess from the floating-point root, corrected by the two integer comparisons that decide
    bins = torch.sqrt(m.to(torch.float64)).to(torch.int64)
    bins = bins + (bins * bins + bins < m).to(torch.int64)
    bins = bins - ((bins * bins - bins >= m) & (m > 0)).to(torch.int64)
    return bins, math.isqrt(int(m.max()))


class EnergySpectrum(Observable):
    """The kinetic energy spectrum (observable_reporter.py:71-137): E(n) = sum over the Fourier modes with
    n - 0.5 < |k| <= n + 0.5 of 0.5 |u_hat / norm|^2, n < K = int(max |k|).

    The reference sums ``ekin[..., None] * wavemask`` with a boolean mask [*res, K] (3.7 GB at 256^3).  Here every
    mode is binned by index instead.  On a native context: ``flow.u()``, one ``torch.fft.fftn`` over the [d, *res]
    field and ``lt_energy_spectrum`` (fp64 squares and sums in a fixed order, cast to the context dtype at the end).
    Elsewhere the same bin index with ``index_add_`` in the context dtype.  Both differ from the reference's values
    at rounding level only.  Needs the whole field: not ``slab_aware``, a slab simulation refuses it by name."""

    def __init__(self, flow: "Flow"):
        super().__init__(flow)
        self.dx = self.flow.units.convert_length_to_pu(1.0)
        self.dimensions = self.flow.resolution
        d = self.flow.stencil.d
        if d not in (2, 3) or len(self.dimensions) != d:
            raise LettuceException(f"EnergySpectrum: 2-D and 3-D flows, this one has d = {d} on {list(self.dimensions)}")
        if d == 3:
            self.norm = self.dimensions[0] * np.sqrt(2 * np.pi) / self.dx ** 2
        else:
            self.norm = self.dimensions[0] / self.dx
        self._n_bins = math.isqrt(sum((n // 2) ** 2 for n in self.dimensions))
        self.wavenumbers = torch.arange(self._n_bins)
        self._bins = None           # torch path: [nodes] int64 on the context's device, K for the modes of no bin
        self._wavemask = None

    @property
    def wavemask(self):
        """the reference's boolean mask [*res, K], kept for compatibility: built on first access, used by nothing"""
        if self._wavemask is None:
            bins, _ = spectrum_bins(self.dimensions, self.context.device)
            self._wavemask = bins[..., None] == self.wavenumbers.to(self.context.device)
        return self._wavemask

    def __call__(self, f: Optional[torch.Tensor] = None):
        return self.spectrum_from_u(self.flow.u())

    def spectrum_from_u(self, u):
        flow = self.flow
        d = flow.stencil.d
        u = flow.units.convert_velocity_to_pu(u)
        axes = tuple(range(1, d + 1))
        plan = flow._engine_plan(flow.f) if (u.is_cuda and u.dtype == self.context.dtype
                                             and list(u.shape) == [d, *self.dimensions]) else None
        if plan is not None and 1 <= self._n_bins <= SPECTRUM_MAX_BINS:
            uh = torch.fft.fftn(u, dim=axes)
            ek = plan.energy_spectrum(uh, 1.0 / float(self.norm) ** 2, self._n_bins)
            return ek.to(self.context.dtype)
        # above LT_SPECTRUM_MAX_BINS bins (a grid beyond 2000^3) the kernel's table no longer fits: the torch path
        uh = torch.fft.fftn(u, dim=axes) / self.norm
        ekin = torch.sum(0.5 * (uh.imag ** 2 + uh.real ** 2), dim=0)
        if self._bins is None or self._bins.device != ekin.device:
            bins, _ = spectrum_bins(self.dimensions, ekin.device)
            self._bins = bins.clamp(max=self._n_bins).reshape(-1)
        ek = torch.zeros(self._n_bins + 1, dtype=ekin.dtype, device=ekin.device)
        ek.index_add_(0, self._bins, ekin.reshape(-1))
        return ek[:self._n_bins]


class Mass(Observable):
    """Total mass in lattice units (observable_reporter.py:140-158)."""

    def __init__(self, flow: "Flow", no_mass_mask=None):
        super().__init__(flow)
        self.mask = no_mass_mask

    def __call__(self, f: Optional[torch.Tensor] = None):
        plan = self.flow._engine_plan(f) if (f is not None and self.flow.stencil.d >= 2) else None
        if plan is not None and (self.mask is None or list(self.mask.shape) == list(f.shape[1:])):
            return plan.mass_interior(f, self.mask).to(f.dtype)      # device reduction (lt_mass_interior)
        mass = f[..., 1:-1, 1:-1].sum()
        if self.mask is not None:
            mass -= (f * self.mask.to(dtype=torch.float)).sum()
        return mass


def momentum_exchange(stencil, f, solid):
    """The torch expression of ``BoundaryForce``: fp64 ``[d]``.  ``f`` [q, *res]; ``solid`` bool [*res] on the same
    device.  Per q one ``torch.roll`` of the mask (``roll(solid, e_q)[x] = solid[x - e_q]``), the populations on the
    links from a solid to a fluid node, summed in fp64."""
    d = stencil.d
    axes = tuple(range(d))
    total = torch.zeros(d, dtype=torch.float64, device=f.device)
    for q in range(1, stencil.q):
        e = [int(x) for x in stencil.e[q]]
        link = solid & ~torch.roll(solid, shifts=tuple(e), dims=axes)
        s = 2.0 * f[q][link].to(torch.float64).sum()
        for c in range(d):
            if e[c]:
                total[c] += e[c] * s
    return total


def link_momentum_exchange(stencil, f, links):
    """The torch expression of ``BoundaryForce`` on a body with link bounce-back: fp64 ``[d]``,

        F_c = sum over the links (r, x_s), q = opposite(r), of e_{q,c} (f_q(x_s) + f_r(x_f)),

    on post-streaming populations ``f`` [q, *res]: f_q(x_s) left the fluid along the link during the last streaming
    step, f_r(x_f) is the interpolated reflection that came back.  ``links``: the body's compact list
    (``InterpolatedBounceBackBoundary.links``) on the device of ``f``.  With every fraction 1/2 both terms are equal and
    this is ``momentum_exchange``."""
    flat = f.reshape(f.shape[0], -1)
    left = flat[links.opposite, links.node].to(torch.float64)
    back = flat[links.direction, links.xf].to(torch.float64)
    e = torch.as_tensor(np.array(stencil.e), dtype=torch.float64, device=f.device)[links.opposite]
    return (e * (left + back)[:, None]).sum(dim=0)


class BoundaryForce(Observable):
    """The force the fluid exerts on a body of full-way bounce-back nodes, per time step, in lattice units, by momentum
    exchange: ``[d]`` values in the context dtype,

        F_c = sum over solid x_s, over q >= 1 with x_s - e_q not solid, of 2 e_{q,c} f_q(x_s).

    ``flow.f`` is post-streaming: f_q(x_s) arrived from x_s - e_q and, swapped by the bounce-back rule at collision
    time, leaves again along -e_q within the same step.  Neighbours wrap periodically as streaming does, nodes of other
    boundaries count as not solid, links between two solid nodes carry nothing.  A body in a +x stream has F_0 > 0.

    ``boundary``: a ``BounceBackBoundary`` (its mask) or a bool tensor / array ``[*res]``.  Where ``Simulation`` lets a
    boundary of a higher index win on some of the body's nodes, those nodes do not bounce back: pass
    ``simulation.no_collision_mask == index`` instead.  On a native context one masked reduction on the device
    (``lt_boundary_force``: fp64, fixed order); elsewhere, and for D1Q3, one ``torch.roll`` of the mask per q and
    sums in fp64.  Needs the whole field: not ``slab_aware``, a slab simulation refuses it by name.

    Given an ``InterpolatedBounceBackBoundary`` (or ``HalfwayBounceBackBoundary``) the sum runs over that body's links
    with both populations of a link, F_c = sum e_{q,c} (f_q(x_s) + f_r(x_f)) (``link_momentum_exchange``): what left the
    fluid and what the interpolation sent back.  On a native context ``lt_link_force`` over the same list the engine
    steps with; the boundary's ``mask`` and ``fractions`` are read again whenever they were assigned."""

    def __init__(self, flow: "Flow", boundary):
        super().__init__(flow)
        self._solid = None
        self._body = boundary if isinstance(boundary, InterpolatedBounceBackBoundary) else None
        self._link_plan = None      # (body version, device, Plan holding the body's links)
        self.mask = boundary if isinstance(boundary, (torch.Tensor, np.ndarray)) else getattr(boundary, "_mask", boundary)

    @property
    def mask(self) -> torch.Tensor:
        """the solid nodes: contiguous uint8 ``[*res]`` on the context's device (assign a bool tensor / array)"""
        return self._solid

    @mask.setter
    def mask(self, value):
        if not isinstance(value, (torch.Tensor, np.ndarray)):
            raise LettuceException(f"{type(self).__name__}: a BounceBackBoundary or a bool tensor / array "
                                   f"{list(self.flow.resolution)}, got {type(value).__name__}")
        if list(value.shape) != list(self.flow.resolution):
            raise LettuceException(f"{type(self).__name__}: mask of shape {list(value.shape)} on a grid "
                                   f"{list(self.flow.resolution)}")
        solid = torch.as_tensor(value).to(self.context.device) != 0
        self._solid = solid.to(torch.uint8).contiguous()

    def force(self, f: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the force in fp64, ``[d]``, on the device of ``f``"""
        flow = self.flow
        f = flow.f if f is None else f
        d = flow.stencil.d
        if self._body is not None:
            return self._link_force(f)
        plan = flow._engine_plan(f) if (d >= 2 and self._solid.device == f.device) else None
        if plan is not None:
            return plan.boundary_force(f, self._solid)
        return momentum_exchange(flow.stencil, f, self._solid.to(f.device) != 0)

    def _link_force(self, f: torch.Tensor) -> torch.Tensor:
        """the force on a body with link bounce-back: lt_link_force on a native context, else the torch expression"""
        flow, body = self.flow, self._body
        if flow.stencil.d >= 2 and flow._engine_plan(f) is not None:
            from .._native import Plan
            key = (body._version, f.device)
            if self._link_plan is None or self._link_plan[0] != key:
                links = body.links(flow.stencil, f.dtype)
                plan = Plan(type(flow.stencil).__name__, f.dtype, "none", flow.resolution, [{"kind": "link_bounce_back"}],
                            device=f.device)
                plan.set_links(0, links.node, links.direction, links.c1, links.c2, links.second)
                self._link_plan = (key, plan)
            return self._link_plan[1].link_force(0, f)
        return link_momentum_exchange(flow.stencil, f, body._links_on_device(flow.stencil, f.dtype, f.device))

    def __call__(self, f: Optional[torch.Tensor] = None):
        return self.force(f).to(self.context.dtype)


class DragCoefficient(BoundaryForce):
    """C = F[direction] / (0.5 rho_char_lu u_char_lu^2 A_lu) of the force on ``boundary`` (``BoundaryForce``).
    ``area`` in physical units -- the frontal area in 3-D, the diameter in 2-D -- becomes
    A_lu = area * convert_length_to_lu(1)^(d - 1); the ratio is dimensionless."""

    def __init__(self, flow: "Flow", boundary, area, direction: int = 0):
        super().__init__(flow, boundary)
        self.direction = int(direction)
        if not 0 <= self.direction < flow.stencil.d:
            raise LettuceException(f"{type(self).__name__}: direction {self.direction} on a {flow.stencil.d}-D flow")
        self.area = area

    @property
    def area_lu(self) -> float:
        units = self.flow.units
        return float(self.area) * float(units.convert_length_to_lu(1.0)) ** (self.flow.stencil.d - 1)

    def __call__(self, f: Optional[torch.Tensor] = None):
        units = self.flow.units
        scale = 0.5 * float(units.characteristic_density_lu) * float(units.characteristic_velocity_lu) ** 2 * self.area_lu
        return (self.force(f)[self.direction] / scale).to(self.context.dtype)


class LiftCoefficient(DragCoefficient):
    """The same across the stream: ``direction`` defaults to 1."""

    def __init__(self, flow: "Flow", boundary, area, direction: int = 1):
        super().__init__(flow, boundary, area, direction)


class ObservableReporter(Reporter):
    """Evaluates ``observable`` every ``interval`` steps and prints ``i t_pu value...`` or
    appends it to ``out`` when that is a list (observable_reporter.py:161-199)."""
    batchable = True          # does nothing unless flow.i % interval == 0: steps in between may be fused

    def __init__(self, observable, interval=1, out=sys.stdout):
        super().__init__(interval)
        self.observable = observable
        self.out = [] if out is None else out
        self._parameter_name = type(observable).__name__
        print("steps    ", "time    ", self._parameter_name)

    def __call__(self, simulation: "Simulation"):
        if simulation.flow.i % self.interval != 0:
            return
        observed = self.observable.context.convert_to_ndarray(self.observable(simulation.flow.f))
        assert len(observed.shape) < 2
        values = [observed.item()] if observed.ndim == 0 else observed.tolist()
        entry = [simulation.flow.i, simulation.units.convert_time_to_pu(simulation.flow.i)] + values
        if isinstance(self.out, list):
            self.out.append(entry)
        else:
            print(*entry, file=self.out)


class ErrorReporter(Reporter):
    """L2 errors of u and p (physical units) against an analytic solution, e.g.
    ``flow.analytic_solution`` of the 2-D Taylor-Green vortex; used by the convergence check
    ("next" row F4; lettuce/ext/_reporter/error_reporter.py:9-48, lettuce/cli.py:128-180)."""
    batchable = True

    def __init__(self, analytical_solution, interval=1, out=sys.stdout):
        Reporter.__init__(self, interval)
        self.analytical_solution = analytical_solution
        self.out = [] if out is None else out
        if not isinstance(self.out, list):
            print("#error_u         error_p", file=self.out)

    def __call__(self, simulation: "Simulation"):
        flow = simulation.flow
        if flow.i % self.interval != 0:
            return
        p_ref, u_ref = self.analytical_solution(t=simulation.units.convert_time_to_pu(flow.i))
        p_ref = flow.context.convert_to_tensor(p_ref)
        u_ref = flow.context.convert_to_tensor(u_ref)
        p, u = flow.p_pu, flow.u_pu
        d = flow.stencil.d
        nodes = 1
        for n in p.size():
            nodes *= n
        scale = (nodes ** (1 / d)) ** (d / 2)
        err_u = (torch.norm(u - u_ref) / scale).item()
        err_p = (torch.norm(p - p_ref) / scale).item()
        if isinstance(self.out, list):
            self.out.append([err_u, err_p])
        else:
            print(err_u, err_p, file=self.out)
