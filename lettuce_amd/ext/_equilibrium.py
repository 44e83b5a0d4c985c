"""Equilibrium distributions on the hot path.

``QuadraticEquilibrium`` is the default of every flow (lettuce/ext/_flows/_ext_flow.py:30).
``QuadraticEquilibriumLessMemory`` is the same arithmetic (the reference's results are bit-identical) and runs the same
kernels; ``IncompressibleQuadraticEquilibrium`` (He and Luo) has kernels of its own (``lt_plan_set_equilibrium``).  Any
other ``Equilibrium`` stays on the torch path: the engine's shortcuts step aside for it (``Flow._engine_equilibrium``).
"""
import torch

from .._flow import Equilibrium, local_contract
from ..native_desc import NativeEquilibrium

__all__ = ["QuadraticEquilibrium", "QuadraticEquilibriumLessMemory", "IncompressibleQuadraticEquilibrium"]


class QuadraticEquilibrium(Equilibrium):
    """feq_q = w_q rho ((2 e_q.u - u.u) / (2 cs^2) + (e_q.u / cs^2)^2 / 2 + 1)
    (lettuce/ext/_equilibrium/quadratic_equilibrium.py:11-25)."""

    def __call__(self, flow: "Flow", rho=None, u=None):
        engine = self.native_available()
        plan = flow._engine_plan(flow.f) if (engine and rho is None and u is None) else None
        if plan is not None:
            rho_, u_ = plan.macroscopic(flow.f)
            plan.set_equilibrium(*self.native_generator().plan_args())
            return plan.equilibrium(rho_, u_)
        rho = flow.rho() if rho is None else rho
        u = flow.u() if u is None else u
        st = flow.torch_stencil
        grid = list(flow.resolution)
        if (engine and flow.context.use_native and torch.is_tensor(rho) and list(rho.shape) == [1] + grid
                and list(u.shape) == [st.d] + grid and flow._engine_plan(flow.f) is not None):
            # whole-field feq(rho, u) on a native context: the engine's equilibrium kernel
            plan = flow._engine_plan(flow.f)
            plan.set_equilibrium(*self.native_generator().plan_args())
            return plan.equilibrium(rho.to(flow.f.dtype), u.contiguous())
        return self._torch(flow, rho, u)

    def _torch(self, flow, rho, u):
        st = flow.torch_stencil
        if u.is_cuda and u.dim() > 1:
            e_dot_u = local_contract(st.e, u)
        else:
            e_dot_u = torch.tensordot(st.e, u, dims=1)
        u_sq = (u * u).sum(dim=0) if u.is_cuda else flow.einsum("d,d->", [u, u])
        bracket = (2 * e_dot_u - u_sq) / (2 * st.cs ** 2) + 0.5 * (e_dot_u / (st.cs ** 2)) ** 2 + 1
        return flow.einsum("q,q->q", [st.w, rho * bracket])

    def native_available(self) -> bool:
        # exactly the library's classes: a subclass may override the expression and therefore does not count
        return type(self) in (QuadraticEquilibrium, QuadraticEquilibriumLessMemory, IncompressibleQuadraticEquilibrium)

    def native_generator(self) -> "NativeEquilibrium":
        return NativeEquilibrium("quadratic")


class QuadraticEquilibriumLessMemory(QuadraticEquilibrium):
    """The reference's variant that holds fewer temporaries (lettuce/ext/_equilibrium/
    quadratic_equilibrium_less_memory.py:14-30): the same operations in the same order, so the same values bit for bit
    and the same kernels.  The reference declares it not native; here it is."""


class IncompressibleQuadraticEquilibrium(QuadraticEquilibrium):
    """feq_q = w_q (rho + rho0 ((2 e_q.u - u.u) / (2 cs^2) + (e_q.u / cs^2)^2 / 2)) of He and Luo
    (lettuce/ext/_equilibrium/incompressible_quadratic_equilibrium.py:10-26).  As in the reference ``u`` stays
    ``j / rho`` and ``rho0`` is read on every call."""

    def __init__(self, rho0=1.0):
        self.rho0 = rho0

    def _torch(self, flow, rho, u):
        st = flow.torch_stencil
        if u.is_cuda and u.dim() > 1:       # no BLAS on device tensors (see _flow.local_contract)
            exu = local_contract(st.e, u)
            uxu = (u * u).sum(dim=0)
        else:
            exu = flow.einsum("qd,d->q", [st.e, u])
            uxu = flow.einsum("d,d->", [u, u])
        return flow.einsum("q,q->q", [st.w, rho + self.rho0 * ((2 * exu - uxu) / (2 * st.cs ** 2)
                                                              + 0.5 * (exu / (st.cs ** 2)) ** 2)])

    def native_generator(self) -> "NativeEquilibrium":
        return NativeEquilibrium("incompressible", rho0=lambda: self.rho0)
