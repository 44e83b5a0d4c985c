"""Forcing schemes for a body force: Guo and Shan-Chen (lettuce/ext/_force/_force.py:6-32, guo.py:7-41,
shan_chen.py:7-32).

``BGKCollision(tau, force=...)`` and ``SmagorinskyCollision(tau, C, force=...)`` evaluate them; the torch expressions
mirror the reference's.  With a uniform acceleration (one value per axis) the HIP engine has the force inside its
collide kernels (``lt_plan_set_force``), which the reference's CUDA path never had (guo.py:37-38).

An acceleration that varies in space -- Kolmogorov flow, gravity in part of a domain, a sponge -- is ``GuoField`` /
``ShanChenField``: the same two schemes with ``acceleration`` a tensor ``[d, *flow.resolution]``, on the engine as well
(``lt_plan_set_force_field``: the kernels read the tensor's device memory at every launch).  ``Guo`` and ``ShanChen``
themselves keep the reference's expressions, which append ``d`` singleton axes to the acceleration and therefore
broadcast a one-value-per-axis vector only: given a field they construct, are not ``native_available()``, and their
torch path raises on the first call, as the reference's does.
"""
from abc import ABC, abstractmethod

from ..native_desc import NativeForce
from ..util import LettuceException, append_axes

__all__ = ["Force", "Guo", "ShanChen", "GuoField", "ShanChenField"]


class Force(ABC):
    @abstractmethod
    def __init__(self, flow: "Flow", tau, acceleration):
        ...

    @abstractmethod
    def source_term(self, u):
        ...

    @abstractmethod
    def u_eq(self, flow: "Flow"):
        ...

    @property
    @abstractmethod
    def ueq_scaling_factor(self):
        ...

    @abstractmethod
    def native_available(self) -> bool:
        ...

    @abstractmethod
    def native_generator(self) -> "NativeForce":
        ...


def _uniform(acceleration, d) -> bool:
    """one value per axis: what the engine's kernels take"""
    return acceleration.dim() == 1 and acceleration.shape[0] == d


def _acceleration_values(acceleration):
    return tuple(float(a) for a in acceleration.detach().cpu().tolist())


class Guo(Force):
    """Guo, Zheng, Shi (2002): the equilibrium velocity is shifted by half the force and a source term is added
    (guo.py:14-31)."""

    def __init__(self, flow, tau, acceleration):
        self.flow = flow
        self.tau = tau
        self.acceleration = flow.context.convert_to_tensor(acceleration)

    def source_term(self, u):
        ts = self.flow.torch_stencil
        emu = append_axes(ts.e, ts.d) - u
        if u.is_cuda:       # no BLAS on device tensors (see _flow.local_contract)
            from .._flow import local_contract
            eu = local_contract(ts.e, u)
            eeu = append_axes(ts.e, ts.d) * eu[:, None, ...]
            emu_eeu = emu / (ts.cs ** 2) + eeu / (ts.cs ** 4)
            emu_eeuF = (emu_eeu * append_axes(self.acceleration, ts.d)[None, ...]).sum(dim=1)
        else:
            eu = self.flow.einsum("ib,b->i", [ts.e, u])
            eeu = self.flow.einsum("ia,i->ia", [ts.e, eu])
            emu_eeu = emu / (ts.cs ** 2) + eeu / (ts.cs ** 4)
            emu_eeuF = self.flow.einsum("ia,a->i", [emu_eeu, self.acceleration])
        weemu_eeuF = append_axes(ts.w, ts.d) * emu_eeuF
        return (1 - 1 / (2 * self.tau)) * weemu_eeuF

    def u_eq(self, flow: "Flow" = None):
        flow = self.flow if flow is None else flow
        return self.ueq_scaling_factor * append_axes(self.acceleration, flow.torch_stencil.d) / flow.rho()

    @property
    def ueq_scaling_factor(self):
        return 0.5

    def native_available(self) -> bool:
        return _uniform(self.acceleration, self.flow.stencil.d)

    def native_generator(self) -> "NativeForce":
        # read late: acceleration and tau may change between batches
        return NativeForce("guo", acceleration=lambda: _acceleration_values(self.acceleration),
                           ueq_scale=lambda: self.ueq_scaling_factor,
                           source_scale=lambda: 1 - 1 / (2 * self.tau))


class ShanChen(Force):
    """Shan, Chen (1993): the equilibrium velocity is shifted by tau times the force, no source term
    (shan_chen.py:14-25)."""

    def __init__(self, flow, tau, acceleration):
        self.tau = tau
        self.acceleration = flow.context.convert_to_tensor(acceleration)
        self._d = flow.stencil.d

    def source_term(self, u):
        return 0

    def u_eq(self, flow: "Flow"):
        return self.ueq_scaling_factor * append_axes(self.acceleration, flow.stencil.d) / flow.rho()

    @property
    def ueq_scaling_factor(self):
        return self.tau * 1

    def native_available(self) -> bool:
        return _uniform(self.acceleration, self._d)

    def native_generator(self) -> "NativeForce":
        return NativeForce("shan_chen", acceleration=lambda: _acceleration_values(self.acceleration),
                           ueq_scale=lambda: self.ueq_scaling_factor, source_scale=lambda: 0.0)


class _FieldAcceleration:
    """``acceleration`` of the field classes: a tensor ``[d, *flow.resolution]`` in the context's dtype.  It may be
    edited in place or assigned anew; an assignment is converted once and must have ``d`` components and one axis per
    axis of the grid (a wrong extent is left to ``native_available()`` and, on the torch path, to the broadcast; device
    and dtype are checked again when a native batch starts)."""

    @property
    def acceleration(self):
        return self._acceleration

    @acceleration.setter
    def acceleration(self, value):
        value = self.flow.context.convert_to_tensor(value)
        d = self.flow.stencil.d
        if value.dim() != d + 1 or value.shape[0] != d:
            raise LettuceException(f"{type(self).__name__}: the acceleration is a field [d, *resolution] = "
                                   f"{self._field_shape()}, got shape {list(value.shape)} "
                                   f"(one value per axis is Guo / ShanChen)")
        self._acceleration = value

    def _field_shape(self):
        return [self.flow.stencil.d] + [int(n) for n in self.flow.resolution]

    def native_available(self) -> bool:
        return list(self.acceleration.shape) == self._field_shape()

    def u_eq(self, flow: "Flow" = None):
        flow = self.flow if flow is None else flow
        return self.ueq_scaling_factor * self.acceleration / flow.rho()

    def _native_field(self, kind, source_scale):
        # read late: the tensor may be replaced and tau may change between batches; the kernels read its memory
        return NativeForce(kind, acceleration=None, ueq_scale=lambda: self.ueq_scaling_factor,
                           source_scale=source_scale, field=lambda: self.acceleration)


class GuoField(_FieldAcceleration, Guo):
    """Guo's scheme with an acceleration field a(x), ``[d, *flow.resolution]``:
    u* = j / rho + a(x) / (2 rho) and the source term
    (1 - 1 / (2 tau)) w_q sum_c [(e_qc - u_c) / cs^2 + (e_q . u) e_qc / cs^4] a_c(x)."""

    def __init__(self, flow, tau, acceleration):
        self.flow = flow
        self.tau = tau
        self.acceleration = acceleration

    def source_term(self, u):
        ts = self.flow.torch_stencil
        d = ts.d
        e = ts.e.to(u.dtype)
        a = self.acceleration
        # elementwise sums over the d axes: no BLAS on device tensors (see _flow.local_contract), the same on the CPU
        ua = (u * a).sum(dim=0)
        ea = sum(append_axes(e[:, c], d) * a[c][None, ...] for c in range(d))
        eu = sum(append_axes(e[:, c], d) * u[c][None, ...] for c in range(d))
        term = (ea - ua[None, ...]) / (ts.cs ** 2) + eu * ea / (ts.cs ** 4)
        return (1 - 1 / (2 * self.tau)) * append_axes(ts.w, d) * term

    def native_generator(self) -> "NativeForce":
        return self._native_field("guo", lambda: 1 - 1 / (2 * self.tau))


class ShanChenField(_FieldAcceleration, ShanChen):
    """Shan and Chen's scheme with an acceleration field a(x), ``[d, *flow.resolution]``: u* = j / rho + tau a(x) / rho,
    no source term."""

    def __init__(self, flow, tau, acceleration):
        self.flow = flow
        self.tau = tau
        self._d = flow.stencil.d
        self.acceleration = acceleration

    def native_generator(self) -> "NativeForce":
        return self._native_field("shan_chen", lambda: 0.0)
