"""Collision operators on the hot path: BGK, KBC (D2Q9 / D3Q27), Smagorinsky, TRT, regularised (every lattice), MRT
(D2Q9 / D3Q27) and NoCollision.

Each ``__call__`` is a pure whole-field function ``flow -> tensor`` usable outside a
``Simulation`` (the reference's tests call ``collision(flow)`` directly).  On a native context
and for the flow's grid-shaped state it is one launch of the engine's collide kernel;
otherwise the reference's torch expressions are evaluated.  BGK and Smagorinsky take a body force
(``force=Guo(...)`` / ``ShanChen(...)``, ext/_force.py), on the engine when its acceleration is uniform, and
``force=GuoField(...)`` / ``ShanChenField(...)`` with an acceleration per node, on the engine as well.
TRT and the regularised collision are on the engine for every lattice as well (one-step kernels; the plain two-step
sweep on D3Q19 fp32); neither takes a force, as in the reference.  MRT takes a moment transform of
``lettuce_amd.moments``: with D2Q9Dellar, D2Q9Lallemand or D3Q27Hermite it is on the engine (one-step kernels), with any
other transform it stays on the torch path.
"""
import warnings
from typing import AnyStr, Optional

import torch

from .._simulation import Collision
from ..native_desc import NativeCollision
from ._force import Force
from ..util import LettuceException

__all__ = ["BGKCollision", "KBCCollision", "KBCCollision2D", "KBCCollision3D", "NoCollision",
           "SmagorinskyCollision", "TRTCollision", "RegularizedCollision", "MRTCollision"]


# the collisions that evaluate flow.equilibrium (MRT relaxes towards its transform's own equilibrium moments), and those
# of them with kernels for the incompressible equilibrium (lt_plan_set_equilibrium)
FEQ_COLLISIONS = ("bgk", "kbc", "smagorinsky", "trt", "regularized")
INCOMPRESSIBLE_COLLISIONS = ("none", "bgk", "trt", "regularized")


def _engine_collide(flow, desc: NativeCollision):
    """C(flow.f) through the HIP engine, or None when flow.f is not engine-shaped.  ``desc``: the collision's own
    ``native_generator()``; its settings and its tau are read here and handed to the kind's one plan before every
    collide."""
    kind = desc.kind
    if flow._engine_plan(flow.f) is None:
        return None
    # the flow's equilibrium is a property of the plan, handed over like the other settings.  An equilibrium the engine
    # has no kernel for, or none under this collision: the torch expressions (the caller's)
    equilibrium = flow._engine_equilibrium() if kind in FEQ_COLLISIONS else ("quadratic", 1.0)
    if equilibrium is None or (equilibrium[0] != "quadratic" and kind not in INCOMPRESSIBLE_COLLISIONS):
        return None
    plans = flow.__dict__.setdefault("_collision_plans", {})
    if kind not in plans:
        from .._native import Plan
        plans[kind] = Plan(type(flow.stencil).__name__, flow.context.dtype, kind, flow.resolution,
                           device=flow.f.device)
    plan = plans[kind]
    if kind in FEQ_COLLISIONS:
        plan.set_equilibrium(*equilibrium)
    settings = desc.settings(flow)
    settings.apply(plan)
    if kind in ("bgk", "smagorinsky") and settings.force is None and settings.force_field is None:
        # the plan is shared by every collision object of this kind on the flow: one with a force may have used it last
        plan.set_force(None)
    return plan.collide(flow.f, torch.empty_like(flow.f), desc.tau(flow))


class BGKCollision(Collision):
    """f - (f - feq(rho, u)) / tau (lettuce/ext/_collision/bgk_collision.py:12-35).

    ``arithmetic`` (an attribute, not part of the reference's signature): "exact" (default) -- the HIP engine reproduces
    the reference's floating-point operations one for one.  Anything else (the former "fast") makes ``Simulation``
    raise: the engine has no such kernel."""
    arithmetic = "exact"

    def __init__(self, tau, force: Optional["Force"] = None):
        self.tau = tau
        self.force = force

    def __call__(self, flow: "Flow") -> torch.Tensor:
        if self.native_available():
            out = _engine_collide(flow, self.native_generator())
            if out is not None:
                return out
        if self.force is None:
            u = flow.u() + 0
            feq = flow.equilibrium(flow, u=u)
            return flow.f - 1.0 / self.tau * (flow.f - feq) + 0
        u = flow.u() + self.force.u_eq(flow)
        feq = flow.equilibrium(flow, u=u)
        return flow.f - 1.0 / self.tau * (flow.f - feq) + self.force.source_term(u)

    def name(self) -> AnyStr:
        if self.force is not None:
            return f"{type(self).__name__}_{type(self.force).__name__}"
        return type(self).__name__

    def native_available(self) -> bool:
        return self.force is None or (isinstance(self.force, Force) and self.force.native_available())

    def native_generator(self) -> "NativeCollision":
        return NativeCollision("bgk", tau=lambda flow: self.tau, arithmetic=getattr(self, "arithmetic", "exact"),
                               force=None if self.force is None else self.force.native_generator())


class KBCCollision(Collision):
    """Entropic multi-relaxation model of Karlin, Boesch, Chikatamarla
    (lettuce/ext/_collision/kbc_collision.py:11-166).

    As in the reference the constructor's ``tau`` is not used: on the first call tau is taken
    from ``flow.units.relaxation_parameter_lu`` (kbc_collision.py:97-99)."""

    def __init__(self, tau: float = None):
        self.tau = tau
        self.beta = None
        self._ready = False

    def _prepare(self, flow):
        if self._ready:
            return
        name = type(flow.stencil).__name__
        if flow.stencil.d == 3:
            assert name == "D3Q27", "KBC Collision is only implemented for D3Q27!"
        elif flow.stencil.d == 2:
            assert name == "D2Q9", "KBC Collision is only implemented for D2Q9!"
        else:
            raise NotImplementedError("KBC Collision is only implemented for 2d and 3d!")
        self.tau = flow.units.relaxation_parameter_lu
        self.beta = 1. / (2 * self.tau)
        self._ready = True

    # second moments of a population set, normalised by its own density
    @staticmethod
    def _moments(flow, g):
        e = flow.torch_stencil.e
        rho = torch.sum(g, dim=0)

        def m(a, b):
            coeff = e[:, a] * e[:, b]
            if g.is_cuda:       # no BLAS on device tensors (see _flow.local_contract)
                from .._flow import local_contract
                return local_contract(coeff[None, :], g)[0] / rho
            return torch.einsum("q,q...->...", coeff, g) / rho

        return rho, m

    def _shear_vector(self, flow, g):
        """s_i of kbc_collision.py:44-94; the corner populations of D3Q27 get zero."""
        rho, m = self._moments(flow, g)
        s = torch.zeros_like(g)
        if flow.stencil.d == 3:
            xx, yy, zz = m(0, 0), m(1, 1), m(2, 2)
            trace, n_xz, n_yz = xx + yy + zz, xx - zz, yy - zz
            s[0] = rho * -trace
            s[1] = s[2] = 1. / 6. * rho * (2 * n_xz - n_yz + trace)
            s[3] = s[4] = 1. / 6. * rho * (2 * n_yz - n_xz + trace)
            s[5] = s[6] = 1. / 6. * rho * (-n_xz - n_yz + trace)
            for first, (a, b) in ((7, (1, 2)), (11, (0, 2)), (15, (0, 1))):
                p = 1. / 4 * rho * m(a, b)
                s[first] = s[first + 1] = p
                s[first + 2] = s[first + 3] = -p
        else:
            xx, yy = m(0, 0), m(1, 1)
            trace, n = xx + yy, xx - yy
            s[0] = rho * -trace
            s[1] = s[3] = 1. / 2. * rho * (0.5 * (trace + n))
            s[2] = s[4] = 1. / 2. * rho * (0.5 * (trace - n))
            p = 1. / 4. * rho * m(0, 1)
            s[5] = s[7] = p
            s[6] = s[8] = -p
        return s

    def __call__(self, flow: "Flow") -> torch.Tensor:
        self._prepare(flow)
        out = _engine_collide(flow, self.native_generator())
        if out is not None:
            return out
        feq = flow.equilibrium(flow)
        delta_s = self._shear_vector(flow, flow.f) - self._shear_vector(flow, feq)
        delta_h = flow.f - feq - delta_s
        sum_s = flow.rho(delta_s * delta_h / feq)
        sum_h = flow.rho(delta_h * delta_h / feq)
        gamma = 1. / self.beta - (2 - 1. / self.beta) * sum_s / sum_h
        gamma[gamma < 1E-15] = 2.0
        gamma[torch.isnan(gamma)] = 2.0
        return flow.f - self.beta * (2 * delta_s + gamma * delta_h)

    def native_available(self) -> bool:
        return True

    def native_generator(self) -> "NativeCollision":
        def tau(flow):
            self._prepare(flow)
            return self.tau
        return NativeCollision("kbc", tau=tau)


class KBCCollision2D(KBCCollision):
    def __init__(self, tau: float = None):
        warnings.warn("KBCCollision2D is is deprecated! Use KBCCollision instead!")
        super().__init__()


class KBCCollision3D(KBCCollision):
    def __init__(self, tau: float = None):
        warnings.warn("KBCCollision3D is is deprecated! Use KBCCollision instead!")
        super().__init__()


class SmagorinskyCollision(Collision):
    """Smagorinsky large-eddy model on top of BGK (lettuce/ext/_collision/smagorinsky_collision.py:7-42): the
    relaxation time of a node grows with the second moments of its non-equilibrium populations, through two
    fixed-point iterations.  The reference's algorithm is kept as it is, including that S:S enters the eddy
    viscosity without a square root and that the contraction counts the off-diagonal components twice.

    ``tau_eff`` is ``tau`` until the torch path has run, then the per-node field of its last call (as in the
    reference); the engine's kernel keeps it in registers and does not set it."""

    def __init__(self, tau, smagorinsky_constant=0.17, force: Optional["Force"] = None):
        self.force = force
        self.tau = tau
        self.iterations = 2
        self.tau_eff = tau
        self.constant = smagorinsky_constant

    def __call__(self, flow: "Flow") -> torch.Tensor:
        if self.native_available():
            out = _engine_collide(flow, self.native_generator())
            if out is not None:
                return out
        rho = flow.rho()
        u_eq = 0 if self.force is None else self.force.u_eq(flow)
        u = flow.u() + u_eq
        feq = flow.equilibrium(flow, rho, u)
        f_neq = flow.f - feq
        if f_neq.is_cuda:       # no BLAS on device tensors (see _flow.local_contract)
            from .._flow import local_contract
            e, d = flow.torch_stencil.e, flow.stencil.d
            ee = torch.einsum("qa,qb->abq", e, e).reshape(d * d, -1)
            s_shear = local_contract(ee, f_neq).reshape([d, d] + list(f_neq.shape[1:]))
        else:
            s_shear = flow.shear_tensor(f_neq)
        s_shear /= (2.0 * rho * flow.stencil.cs ** 2)
        self.tau_eff = self.tau
        nu = (self.tau - 0.5) / 3.0
        for _ in range(self.iterations):
            s = s_shear / self.tau_eff
            s = (s * s).sum(dim=(0, 1)) if s.is_cuda else flow.einsum("ab,ab->", [s, s])
            nu_t = self.constant ** 2 * s
            nu_eff = nu + nu_t
            self.tau_eff = nu_eff * 3.0 + 0.5
        si = 0 if self.force is None else self.force.source_term(u)
        return flow.f - 1.0 / self.tau_eff * (flow.f - feq) + si

    def native_available(self) -> bool:
        return self.iterations == 2 and (
            self.force is None or (isinstance(self.force, Force) and self.force.native_available()))

    def native_generator(self) -> "NativeCollision":
        return NativeCollision("smagorinsky", tau=lambda flow: self.tau, constant=lambda flow: self.constant,
                               force=None if self.force is None else self.force.native_generator())


class TRTCollision(Collision):
    """Two relaxation times (lettuce/ext/_collision/trt_collision.py:6-27): over an opposite pair the symmetric part of
    f - feq relaxes with ``tau_plus`` (the constructor's ``tau``, which sets the viscosity), the antisymmetric part with
    ``tau_minus``.  Both attributes are read on every call, as in the reference."""

    def __init__(self, tau, tau_minus=1.0):
        self.tau_plus = tau
        self.tau_minus = tau_minus

    def __call__(self, flow: "Flow") -> torch.Tensor:
        out = _engine_collide(flow, self.native_generator())
        if out is not None:
            return out
        opposite = flow.stencil.opposite
        feq = flow.equilibrium(flow)
        f_diff_neq = (((flow.f + flow.f[opposite]) - (feq + feq[opposite])) / (2.0 * self.tau_plus))
        f_diff_neq += (((flow.f - flow.f[opposite]) - (feq - feq[opposite])) / (2.0 * self.tau_minus))
        return flow.f - f_diff_neq

    def native_available(self) -> bool:
        return True

    def native_generator(self) -> "NativeCollision":
        return NativeCollision("trt", tau=lambda flow: self.tau_plus, tau_minus=lambda flow: self.tau_minus)


class RegularizedCollision(Collision):
    """Regularised LBM of Latt and Chopard (lettuce/ext/_collision/regularized_collision.py:8-44): the non-equilibrium
    populations are rebuilt from their second moments, f = feq + (1 - 1 / tau) w_q / (2 cs^4) Q_q : Pi_neq.

    As in the reference the constructor's ``tau`` is not used: on the first call tau is taken from
    ``flow.units.relaxation_parameter_lu`` (regularized_collision.py:18-19); assignments to ``.tau`` after that are
    read on every call."""

    def __init__(self, tau: float = None):
        self.tau = tau
        self.Q_matrix = None

    def _prepare(self, flow):
        if self.Q_matrix is not None:
            return
        self.tau = flow.units.relaxation_parameter_lu
        e = flow.torch_stencil.e.to(flow.context.dtype)
        q_matrix = torch.einsum("qa,qb->qab", e, e)
        q_matrix = q_matrix - torch.eye(flow.stencil.d, device=e.device, dtype=e.dtype) * flow.torch_stencil.cs ** 2
        self.Q_matrix = q_matrix

    def __call__(self, flow: "Flow") -> torch.Tensor:
        self._prepare(flow)
        out = _engine_collide(flow, self.native_generator())
        if out is not None:
            return out
        feq = flow.equilibrium(flow)
        f_neq = flow.f - feq
        d, w = flow.stencil.d, flow.torch_stencil.w
        cs4 = flow.stencil.cs ** 4
        if f_neq.is_cuda:       # no BLAS on device tensors (see _flow.local_contract)
            from .._flow import local_contract
            e = flow.torch_stencil.e
            ee = torch.einsum("qa,qb->abq", e, e).reshape(d * d, -1)
            pi_neq = local_contract(ee, f_neq)
            pi_neq = local_contract(self.Q_matrix.reshape(-1, d * d), pi_neq)
            pi_neq = pi_neq * w.reshape([-1] + [1] * d)
        else:
            pi_neq = flow.shear_tensor(f_neq)
            pi_neq = flow.einsum("qab,ab->q", [self.Q_matrix, pi_neq])
            pi_neq = flow.einsum("q,q->q", [w, pi_neq])
        fi1 = pi_neq / (2 * cs4)
        return feq + (1. - 1. / self.tau) * fi1

    def native_available(self) -> bool:
        return True

    def native_generator(self) -> "NativeCollision":
        def tau(flow):
            self._prepare(flow)
            return self.tau
        return NativeCollision("regularized", tau=tau)


class MRTCollision(Collision):
    """Multiple relaxation times (lettuce/ext/_collision/mrt_collision.py:6-33): the moments ``transform.transform(f)``
    relax towards ``transform.equilibrium`` with one rate each, m_i <- m_i - (m_i - meq_i) / s_i.  The transform may be
    any ``lettuce_amd.moments.Transform``.  ``relaxation_parameters`` becomes a tensor of the context's dtype and is read
    on every call, as in the reference.

    On the engine for exactly the three transforms with an equilibrium of their own, each on its own lattice; a subclass
    may override the equilibrium and therefore does not count."""

    def __init__(self, transform: "Transform", relaxation_parameters: list, context: "Context"):
        self.transform = transform
        self.relaxation_parameters = context.convert_to_tensor(relaxation_parameters)

    def _native_transform(self) -> Optional[str]:
        """the engine's name of the transform, or None"""
        from ..moments import D2Q9Dellar, D2Q9Lallemand, D3Q27Hermite
        cls = type(self.transform)
        if cls not in (D2Q9Dellar, D2Q9Lallemand, D3Q27Hermite):
            return None
        if type(self.transform.stencil) not in cls.supported_stencils:
            return None
        return cls.__name__

    def _rates(self):
        """the q rates as floats: one device-to-host copy"""
        return tuple(float(s) for s in self.relaxation_parameters.tolist())

    def __call__(self, flow: "Flow") -> torch.Tensor:
        if self._native_transform() is not None:
            out = _engine_collide(flow, self.native_generator())
            if out is not None:
                return out
        m = self.transform.transform(flow.f)
        meq = self.transform.equilibrium(m, flow)
        rates = 1 / self.relaxation_parameters
        m = m - rates.reshape([-1] + [1] * flow.stencil.d) * (m - meq)
        return self.transform.inverse_transform(m)

    def native_available(self) -> bool:
        return self._native_transform() is not None

    def native_generator(self) -> "NativeCollision":
        return NativeCollision("mrt", transform=self._native_transform(), rates=lambda flow: self._rates())


class NoCollision(Collision):
    """Identity (lettuce/ext/_collision/no_collision.py:9-17); used by streaming tests."""

    def __call__(self, flow: "Flow") -> torch.Tensor:
        return flow.f

    def native_available(self) -> bool:
        return True

    def native_generator(self) -> "NativeCollision":
        return NativeCollision("none")
