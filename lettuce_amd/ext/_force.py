"""Forcing schemes for a body force: Guo and Shan-Chen (lettuce/ext/_force/_force.py:6-32, guo.py:7-41,
shan_chen.py:7-32).

``BGKCollision(tau, force=...)`` and ``SmagorinskyCollision(tau, C, force=...)`` evaluate them; the torch expressions
mirror the reference's.  With a uniform acceleration (one value per axis) the HIP engine has the force inside its
collide kernels (``lt_plan_set_force``), which the reference's CUDA path never had (guo.py:37-38); a per-node
acceleration field stays on the torch path.
"""
from abc import ABC, abstractmethod

from ..native_desc import NativeForce
from ..util import append_axes

__all__ = ["Force", "Guo", "ShanChen"]


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
