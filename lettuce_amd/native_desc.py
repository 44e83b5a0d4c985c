"""Descriptors handed from the Python operators to the HIP engine.

The reference's components return *code emitters* from ``native_generator()``
(lettuce/_flow.py:21-27,45-51, lettuce/_simulation.py:21-27,119-127) because its kernel is
generated and JIT-compiled per configuration.  The engine here is prebuilt, so the same
protocol returns plain descriptors: an enum-like ``kind`` plus the scalar parameters the
kernels take.

What a collision hands to a plan before a launch, apart from ``tau``, is one value record: ``CollisionSettings``.
``NativeCollision.settings(flow)`` reads it and ``CollisionSettings.apply(engine)`` calls the plan's setters; the
steppers (``Simulation``, the slab drivers) and ``collision(flow)`` do nothing else with these values.  A new per-batch
setting (the latest: a force field, ``set_force_field``) is therefore added in three places of this file: its late-bound field in ``NativeCollision``, its line in
``settings()``, and its field and line in ``CollisionSettings`` (``calls()``).
"""
from dataclasses import dataclass, field
from typing import Any, Callable, Optional, Tuple

__all__ = ["NativeEquilibrium", "NativeCollision", "CollisionSettings", "NativeBoundary", "NativeForce", "FieldRef"]


@dataclass
class NativeEquilibrium:
    """The equilibrium of the engine's plans (``lt_plan_set_equilibrium``).  ``rho0`` is read late, per call and per
    batch like ``tau``: the reference reads ``equilibrium.rho0`` on every call
    (lettuce/ext/_equilibrium/incompressible_quadratic_equilibrium.py:22)."""
    kind: str = "quadratic"                    # 'quadratic' | 'incompressible'
    rho0: Optional[Callable[[], float]] = None         # 'incompressible': its reference density; None for 'quadratic'

    def plan_args(self) -> Tuple[str, float]:
        """the arguments of ``Plan.set_equilibrium`` now (hashable: part of the steppers' carry key)"""
        return (self.kind, 1.0 if self.rho0 is None else float(self.rho0()))


@dataclass
class NativeForce:
    """A uniform body force inside the engine's collide kernels (``lt_plan_set_force``).  The three values are read
    late, per batch, because the reference's schemes read ``force.acceleration`` and ``force.tau`` on every call
    (lettuce/ext/_force/guo.py:14-31, shan_chen.py:14-25)."""
    kind: str                                  # 'guo' | 'shan_chen'
    acceleration: Optional[Callable[[], Tuple[float, ...]]]    # lattice units, logical order x, y, z; None with a field
    ueq_scale: Callable[[], float]             # u* = j / rho + ueq_scale * a / rho
    source_scale: Callable[[], float]          # factor of the source term (0: none)
    # an acceleration that varies in space (``lt_plan_set_force_field``; GuoField, ShanChenField): the tensor
    # [d, *resolution], read late like the acceleration -- the object may be replaced between batches, and the kernels
    # read its memory at every launch, so values edited in place are seen without a call.  None: uniform
    field: Optional[Callable[[], Any]] = None

    def plan_args(self) -> Tuple[Tuple[float, ...], float, float]:
        """the arguments of ``Plan.set_force`` now (hashable: part of the steppers' carry key)"""
        return (tuple(float(a) for a in self.acceleration()), float(self.ueq_scale()), float(self.source_scale()))

    def field_args(self) -> Tuple["FieldRef", float, float]:
        """the arguments of ``Plan.set_force_field`` now, the tensor inside a ``FieldRef`` (hashable as well)"""
        return (FieldRef(self.field()), float(self.ueq_scale()), float(self.source_scale()))


class FieldRef:
    """A tensor inside a value record: compared and hashed by what the tensor IS now -- the object, its memory, its
    version counter and its shape -- so that ``CollisionSettings`` stays hashable and two records are equal exactly when
    nothing assigned or edited the field in between.  ``tensor`` is what ``Plan.set_force_field`` takes."""
    __slots__ = ("tensor", "_key")

    def __init__(self, tensor):
        self.tensor = tensor
        self._key = (id(tensor), tensor.data_ptr(), tensor._version, tuple(tensor.shape))

    def __eq__(self, other):
        return isinstance(other, FieldRef) and self._key == other._key

    def __hash__(self):
        return hash(self._key)

    def __repr__(self):
        return f"FieldRef(shape={self._key[3]}, version={self._key[2]})"


@dataclass(frozen=True)
class CollisionSettings:
    """The values a collision hands to a plan before a launch, read now: what ``Plan.set_*`` take, nothing late-bound.
    Hashable and compared by value: part of the steppers' carry key (``_kept.KeptState.key``).  ``tau`` is not among them: it is a launch argument
    of the engine, and KBC and the regularised collision fix theirs at the first read."""
    smagorinsky: Optional[float] = None        # the constant
    tau_minus: Optional[float] = None          # TRT
    mrt: Optional[Tuple[str, Tuple[float, ...]]] = None                    # the transform's name and its q rates
    force: Optional[Tuple[Tuple[float, ...], float, float]] = None         # NativeForce.plan_args()
    force_field: Optional[Tuple[FieldRef, float, float]] = None            # NativeForce.field_args()

    def calls(self):
        """(setter, its arguments) for every value that is not None, in the one order every site calls them"""
        calls = []
        if self.smagorinsky is not None:
            calls.append(("set_smagorinsky", (self.smagorinsky,)))
        if self.tau_minus is not None:
            calls.append(("set_trt", (self.tau_minus,)))
        if self.mrt is not None:
            calls.append(("set_mrt", self.mrt))
        if self.force is not None:
            calls.append(("set_force", self.force))
        if self.force_field is not None:
            ref, ueq_scale, source_scale = self.force_field
            calls.append(("set_force_field", (ref.tensor, ueq_scale, source_scale)))
        return calls

    @property
    def setters(self) -> Tuple[str, ...]:
        """the methods ``apply`` will call: a driver asks its engine for them before the first launch"""
        return tuple(name for name, _ in self.calls())

    def apply(self, engine):
        """hand the values to ``engine``: a ``lettuce_amd._native.Plan`` or anything else with these methods"""
        for name, args in self.calls():
            getattr(engine, name)(*args)


# ``kind``, ``tau`` and ``arithmetic`` say which kernels run and with which launch argument.  The fields after them are
# the per-batch settings, late-bound; they reach a plan only through settings() and CollisionSettings.apply().  A new one
# needs its field here, its line in settings(), and its field and line in CollisionSettings -- nothing in the steppers.
@dataclass
class NativeCollision:
    kind: str                                  # 'none' | 'bgk' | 'kbc' | 'smagorinsky' | 'trt' | 'regularized' | 'mrt'
    # relaxation time used for the next batch of steps; evaluated per call because the
    # reference re-reads collision.tau on every invocation
    # (lettuce/cuda_native/ext/_collision/bgk_collision.py:30)
    tau: Callable[["Flow"], float] = field(default=lambda flow: 1.0)
    # "exact": the reference's floating-point operations one for one (the default; bit-identical periodic BGK flows),
    # the only arithmetic the engine has ("fast" lost its A/B: DESIGN.md section 4)
    arithmetic: str = "exact"
    # 'smagorinsky': the constant, evaluated per batch like tau (the reference reads collision.constant on every
    # call, lettuce/ext/_collision/smagorinsky_collision.py:32); None for the other kinds
    constant: Optional[Callable[["Flow"], float]] = None
    # 'trt': tau_minus, evaluated per batch like tau (the reference reads collision.tau_minus on every call,
    # lettuce/ext/_collision/trt_collision.py:25; `tau` is its tau_plus); None for the other kinds
    tau_minus: Optional[Callable[["Flow"], float]] = None
    # 'bgk' / 'smagorinsky': the body force of the collision (uniform, or a field: NativeForce.field), or None
    force: Optional[NativeForce] = None
    # 'mrt': the class name of the moment transform ('D2Q9Dellar' | 'D2Q9Lallemand' | 'D3Q27Hermite') and its q
    # relaxation rates as a tuple of floats (hashable: part of the steppers' carry key), evaluated per batch like tau
    # (the reference reads collision.relaxation_parameters on every call, lettuce/ext/_collision/mrt_collision.py:24;
    # `tau` is not read); None for the other kinds
    transform: Optional[str] = None
    rates: Optional[Callable[["Flow"], Tuple[float, ...]]] = None

    def settings(self, flow) -> CollisionSettings:
        """the per-batch settings now: every callable is read once, in this order (the rates of MRT are one copy from
        the device)"""
        return CollisionSettings(
            smagorinsky=None if self.constant is None else float(self.constant(flow)),
            tau_minus=None if self.tau_minus is None else float(self.tau_minus(flow)),
            mrt=None if self.rates is None else (self.transform, tuple(self.rates(flow))),
            force=None if self.force is None or self.force.field is not None else self.force.plan_args(),
            force_field=None if self.force is None or self.force.field is None else self.force.field_args())


@dataclass
class NativeBoundary:
    kind: str                                  # 'bounce_back' | 'equilibrium' | 'abb_outlet' | 'pressure_outlet' |
    index: int                                 # 'link_bounce_back' (its link list goes to the plan apart: Plan.set_links)
    # engine parameters of this boundary for a given flow (dict for lettuce_amd._native.Plan)
    params: Optional[Callable[["Flow"], dict]] = None

    def plan_entry(self, flow) -> dict:
        entry = {"kind": self.kind}
        if self.params is not None:
            entry.update(self.params(flow))
        return entry
