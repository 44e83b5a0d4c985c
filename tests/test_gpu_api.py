"""GPU tests through the lettuce-style Python API with the HIP engine in the swap point --
the reference's tests/native/* restated: the same flow is stepped by the CPU oracle and by
``Simulation`` on a native context, and the populations must agree."""
import io
import os
from copy import copy

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from conftest import golden, unpack_nsm, TORCH_DT
from oracle import lettuce_oracle as orc

pytestmark = pytest.mark.gpu


def gpu(dt="f32"):
    return lt.Context(device="cuda:0", dtype=TORCH_DT[dt], use_native=True)


class Dummy(lt.ExtFlow):
    """16x16 D2Q9 flow with hand-set populations (tests/conftest.py:243-266 of the reference)."""

    def __init__(self, context, fill, boundaries=None, resolution=16):
        self._fill, self._b = fill, boundaries
        lt.ExtFlow.__init__(self, context, resolution, 1.0, 1.0)

    def make_resolution(self, resolution, stencil=None):
        return [resolution, resolution] if isinstance(resolution, int) else resolution

    def make_units(self, reynolds_number, mach_number, _):
        return lt.UnitConversion(reynolds_number=reynolds_number, mach_number=mach_number)

    def initial_pu(self):
        ...

    def initialize(self):
        self._fill(self.f)

    @property
    def boundaries(self):
        return [] if self._b is None else self._b(self)


def test_default_context_on_gpu_box_is_native():
    c = lt.Context()
    assert c.device.type == "cuda" and c.use_native and c.dtype == torch.float32


def test_native_streaming():
    def tagged(f):
        f.zero_()
        for q in range(9):
            f[q, q + 1, q + 1] = q + 1.0
    flow = Dummy(gpu(), tagged)
    sim = lt.Simulation(flow, lt.NoCollision(), [])
    assert sim._native is not None
    g = golden("native_streaming_d2q9_f32")
    np.testing.assert_array_equal(flow.f.cpu().numpy(), g["f0"])
    sim(1)
    np.testing.assert_array_equal(flow.f.cpu().numpy(), g["f1"])


def test_native_bgk_collision():
    def bump(f):
        f[:, :, :] = 1.0
        f[:, 2, 2] = 2.0
    flow = Dummy(gpu(), bump)
    lt.Simulation(flow, lt.BGKCollision(2.0), [])(1)
    assert flow.f.cpu().numpy() == pytest.approx(golden("native_bgk_d2q9_f32")["f1"])   # rel 1e-6


def test_native_bounce_back():
    class Box(lt.BounceBackBoundary):
        def make_no_collision_mask(self, shape, context):
            m = context.zero_tensor(shape, dtype=bool)
            m[0, :] = True; m[:, 0] = True; m[2:, :] = True; m[:, 2:] = True
            return m

    def one_node(f):
        f.zero_()
        f[:, 1, 1] = 1.0
    flow = Dummy(gpu(), one_node, lambda fl: [Box(torch.ones(fl.resolution))])
    sim = lt.Simulation(flow, lt.NoCollision(), [])
    g = golden("native_bounce_back_d2q9_f32")
    sim(1)
    np.testing.assert_array_equal(flow.f.cpu().numpy(), g["f1"])
    sim(1)
    np.testing.assert_array_equal(flow.f.cpu().numpy(), g["f2"])


def test_native_equilibrium_pu_with_tensor_arguments():
    class Column(lt.EquilibriumBoundaryPU):
        def make_no_collision_mask(self, shape, context):
            a = context.zero_tensor(shape, dtype=bool)
            a[:, 1] = True
            return a

        def make_no_streaming_mask(self, shape, context):
            return context.one_tensor(shape, dtype=bool)
    c = gpu("f64")

    class TGVb(lt.TaylorGreenVortex):
        extra = None

        @property
        def boundaries(self):
            return [] if self.extra is None else [self.extra]
    flow = TGVb(c, [16, 16], 1, 0.1)
    flow.extra = Column(c, mask=None, velocity=np.ones([2, 16, 16]), pressure=np.ones([16, 16]))
    g = golden("native_equilibrium_pu_d2q9_f64")
    np.testing.assert_allclose(flow.f.cpu().numpy(), g["f0"], rtol=0, atol=1e-14)
    lt.Simulation(flow, lt.NoCollision(), [])(1)
    np.testing.assert_allclose(flow.f.cpu().numpy(), g["f1"], rtol=1e-6, atol=1e-14)


def test_native_no_streaming_mask_assigned_after_construction():
    class Uniform(lt.ExtFlow):
        def make_resolution(self, resolution, stencil=None):
            return [resolution] * stencil.d

        def make_units(self, re, ma, resolution):
            return lt.UnitConversion(re, ma, characteristic_length_lu=resolution[0])

        def initial_pu(self):
            return (0.01 * np.ones([1] + self.resolution), 1.01 * np.ones([2] + self.resolution))

        @property
        def boundaries(self):
            return []
    c = gpu()
    flow = Uniform(c, 16, 1, 0.01, lt.D2Q9())
    sim = lt.Simulation(flow, lt.NoCollision(), [])
    sim.no_streaming_mask = c.zero_tensor(flow.resolution, dtype=bool)
    f0 = copy(flow.f)
    sim(64)
    assert torch.isclose(f0, flow.f).all()
    np.testing.assert_allclose(flow.f.cpu().numpy(), golden("native_no_streaming_mask_d2q9_f32")["f64"],
                               rtol=1e-6)


@pytest.mark.parametrize("name,stencil,coll,dt,n", [
    ("tgv3d_d3q19_bgk_16_f64", lt.D3Q19, "bgk", "f64", 100), ("tgv3d_d3q19_bgk_16_f32", lt.D3Q19, "bgk", "f32", 10),
    ("tgv3d_d3q27_kbc_16_f64", lt.D3Q27, "kbc", "f64", 50), ("tgv2d_d2q9_bgk_32_f64", lt.D2Q9, "bgk", "f64", 100)])
def test_taylor_green_with_reporter_batches(name, stencil, coll, dt, n):
    """Device-side TGV initialisation (F1) + batched stepping between reporter calls + the
    fp64 wave-reduced kinetic energy (F3) against the reference's decay series."""
    g = golden(name)
    res = [int(r) for r in g["resolution"]]
    flow = lt.TaylorGreenVortex(gpu(dt), res, float(g["reynolds"]), float(g["mach"]), stencil())
    tol = 1e-13 if dt == "f64" else 2e-6
    np.testing.assert_allclose(flow.f.cpu().numpy(), g["f0"], rtol=0, atol=tol)
    collision = lt.BGKCollision(flow.units.relaxation_parameter_lu) if coll == "bgk" else lt.KBCCollision()
    out = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr("sys.stdout", io.StringIO())
        rep = lt.ObservableReporter(lt.IncompressibleKineticEnergy(flow), interval=10, out=out)
    sim = lt.Simulation(flow, collision, [rep])
    sim(n)
    steps = [row[0] for row in out]
    assert steps == list(range(0, n + 1, 10))
    ref = dict(zip(g["energy_steps"].tolist(), g["energy_pu"].tolist()))
    for i, _, e in out:
        # north star: KE decay to 1e-6 relative -- fp64 observed ~1e-12; fp32 observed ~1e-7 against
        # the reference's fp32 series (its fp32-specific rounding of the cs^2 divisors is
        # reproduced in the kernel, see kernels.hpp div_cs)
        rel = 1e-9 if dt == "f64" else 1e-6
        assert e == pytest.approx(ref[i], rel=rel)
    atol = (1e-12 if dt == "f64" else 1e-5) * float(np.abs(g[f"f{n}"]).max())
    np.testing.assert_allclose(flow.f.cpu().numpy(), g[f"f{n}"], rtol=0, atol=atol)
    # the Enstrophy and Mass observables on the same state, as device reductions (row F3)
    at = g["energy_steps"].tolist().index(n)
    ens, mass = lt.Enstrophy(flow)(), lt.Mass(flow)(flow.f)
    assert ens.is_cuda and ens.dtype == flow.f.dtype and mass.is_cuda
    assert float(ens) == pytest.approx(float(g["enstrophy_pu"][at]), rel=1e-9 if dt == "f64" else 2e-5)
    assert float(mass) == pytest.approx(float(g["mass_observable"][at]), rel=1e-12 if dt == "f64" else 1e-5)


@pytest.mark.parametrize("name,stencil,coll,dt", [("obstacle2d_d2q9_bgk_f64", lt.D2Q9, "bgk", "f64"),
                                                   ("obstacle3d_d3q27_kbc_f32", lt.D3Q27, "kbc", "f32"),
                                                   ("obstacle3d_d3q27_kbc_f64", lt.D3Q27, "kbc", "f64")])
def test_obstacle_flow_end_to_end(name, stencil, coll, dt):
    """BASELINE cfg4 physics: Obstacle wires inlet + ABB outlet + bounce-back; the reference's
    own native path cannot run this flow at all."""
    g = golden(name)
    res = [int(r) for r in g["resolution"]]
    flow = lt.Obstacle(gpu(dt), res, 100, 0.1, float(g["domain_length_x"]), stencil=stencil())
    flow.mask = g["obstacle_mask"]
    flow.initialize()
    collision = lt.BGKCollision(flow.units.relaxation_parameter_lu) if coll == "bgk" else lt.KBCCollision()
    sim = lt.Simulation(flow, collision, [])
    np.testing.assert_array_equal(sim.no_collision_mask.cpu().numpy(), g["no_collision_mask"])
    np.testing.assert_array_equal(sim.no_streaming_mask.cpu().numpy(), unpack_nsm(g))
    sim(2)
    atol = (1e-11 if dt == "f64" else 1e-5) * float(np.abs(g["f2"]).max())
    np.testing.assert_allclose(flow.f.cpu().numpy(), g["f2"], rtol=0, atol=atol)
    last = 8 if "f8" in g else 10
    sim(last - 2)
    np.testing.assert_allclose(flow.f.cpu().numpy(), g[f"f{last}"], rtol=0, atol=atol)


def test_flow_modified_between_calls_restarts_from_f():
    """In-place edits of flow.f between calls must be honoured (the engine may otherwise carry
    on from its post-collision buffer)."""
    c = gpu("f64")
    flow = lt.TaylorGreenVortex(c, [16, 16], 100, 0.05, lt.D2Q9())
    sim = lt.Simulation(flow, lt.BGKCollision(0.7), [])
    ref = orc.taylor_green([16, 16], 100, 0.05, "D2Q9", torch.float64)
    ref.tau = 0.7
    sim(3); ref.step(3)
    sim(2); ref.step(2)                      # continues from f*
    np.testing.assert_allclose(flow.f.cpu().numpy(), ref.f.numpy(), rtol=0, atol=1e-13)
    flow.f[3] *= 1.01; ref.f[3] *= 1.01     # in-place edit
    sim(2); ref.step(2)
    np.testing.assert_allclose(flow.f.cpu().numpy(), ref.f.numpy(), rtol=0, atol=1e-13)
    flow.f = flow.f.clone() * 0.99; ref.f = ref.f * 0.99      # re-assignment
    sim(1); ref.step(1)
    np.testing.assert_allclose(flow.f.cpu().numpy(), ref.f.numpy(), rtol=0, atol=1e-13)


def test_flow_f_is_completed_when_somebody_looks():
    """The engine leaves a batch one streaming pass short and ``flow.f`` completes it on access (Flow.f): batches
    that nobody looks at in between cost their fused launches only, and whatever the order of looking, assigning
    and stepping, the populations are the reference's."""
    c = gpu("f64")
    g = golden("tgv2d_d2q9_bgk_32_f64")
    res = [int(r) for r in g["resolution"]]

    def fresh():
        flow = lt.TaylorGreenVortex(c, res, float(g["reynolds"]), float(g["mach"]), lt.D2Q9())
        return flow, lt.Simulation(flow, lt.BGKCollision(flow.units.relaxation_parameter_lu), [])
    flow, sim = fresh()
    sim(4)
    assert flow._pending is not None                 # not streamed yet
    sim(3); sim(3)                                   # carries on from the post-collision populations
    assert flow._pending is not None
    looked = flow.f                                  # one streaming pass, now
    assert flow._pending is None and flow.f is looked
    flow2, sim2 = fresh()
    sim2(10)
    assert torch.equal(flow2.f, looked)
    np.testing.assert_allclose(looked.cpu().numpy(), g["f10"], rtol=0, atol=1e-13)
    # looking in between changes nothing; neither does reading f_next or the moments
    flow3, sim3 = fresh()
    sim3(4); _ = flow3.rho(); sim3(3); _ = flow3.f_next; sim3(3)
    assert torch.equal(flow3.f, looked)
    # an assignment while a pass is pending replaces the state (the pending pass is dropped)
    flow4, sim4 = fresh()
    sim4(5)
    flow4.f = looked.clone()
    assert flow4._pending is None
    sim4(2); sim2(2)
    assert torch.equal(flow4.f, flow2.f)


def test_collision_callable_and_moments_use_engine():
    g = golden("operators_d3q27_f32")
    flow = lt.TaylorGreenVortex(gpu(), list(g["f"].shape[1:]), 50, 0.1, lt.D3Q27())
    flow.f = torch.tensor(g["f"], device="cuda")
    np.testing.assert_allclose(flow.rho().cpu().numpy(), g["rho"], rtol=2e-6)
    np.testing.assert_allclose(flow.u().cpu().numpy(), g["u"], rtol=0, atol=2e-7)
    np.testing.assert_allclose(lt.BGKCollision(float(g["tau"]))(flow).cpu().numpy(), g["bgk"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(lt.KBCCollision()(flow).cpu().numpy(), g["kbc"], rtol=0, atol=4e-6)
    np.testing.assert_allclose(flow.equilibrium(flow).cpu().numpy(), g["feq"], rtol=0, atol=2e-6)
    assert flow._moment_plan is not None


def test_unsupported_component_raises_on_native_context():
    class MyCollision(lt.Collision):
        def __call__(self, flow):
            return flow.f

        def native_available(self):
            return False

        def native_generator(self):
            return None
    flow = lt.TaylorGreenVortex(gpu(), [8, 8], 10, 0.05, lt.D2Q9())
    with pytest.raises(lt.LettuceException, match="MyCollision"):
        lt.Simulation(flow, MyCollision(), [])


def test_slab_driver_single_rank_on_gpu():
    """z-slab layout kernels + ghost-plane self exchange on one GPU == single-domain engine."""
    res = [32, 16, 24]
    c = gpu("f64")
    slab = lt.ZSlab(res, rank=0, world_size=1)
    flow = lt.TaylorGreenVortex(c, slab.extended_resolution, 400, 0.1, lt.D3Q19(), slab=slab)
    tau = flow.units.relaxation_parameter_lu
    sim = lt.SlabSimulation(flow, lt.BGKCollision(tau), slab)
    ref = orc.taylor_green(res, 400, 0.1, "D3Q19", torch.float64)
    np.testing.assert_allclose(sim.gather_f().cpu().numpy(), ref.f.numpy(), rtol=0, atol=1e-14)
    sim(4); sim(3)
    ref.step(7)
    np.testing.assert_allclose(sim.gather_f().cpu().numpy(), ref.f.numpy(), rtol=0, atol=1e-13)
    assert sim.kinetic_energy_pu() == pytest.approx(float(orc.kinetic_energy_pu(ref.f, ref.lat, ref.units)), rel=1e-11)
    # D3Q27 KBC fp32 through the slab kernels, wide (x % 4 == 0) and narrow paths
    for rs in ([16, 8, 6], [10, 6, 4]):
        slab = lt.ZSlab(rs, rank=0, world_size=1)
        flow = lt.TaylorGreenVortex(gpu(), slab.extended_resolution, 400, 0.1, lt.D3Q27(), slab=slab)
        sim = lt.SlabSimulation(flow, lt.KBCCollision(), slab)
        ref = orc.taylor_green(rs, 400, 0.1, "D3Q27", torch.float32, "kbc")
        sim(5); ref.step(5)
        np.testing.assert_allclose(sim.gather_f().cpu().numpy(), ref.f.numpy(), rtol=0, atol=2e-6)


def test_slab_driver_with_per_node_equilibrium_boundary_on_gpu():
    """Per-node inlet fields on the slab-layout kernels (one rank): SlabSimulation == Simulation on the whole
    grid with the same EquilibriumBoundaryPU(velocity field, pressure field)."""
    res, steps = [16, 8, 12], 6

    def setup(c, slab=None):
        torch.manual_seed(17)
        vel = 0.05 * torch.rand([3] + res, dtype=torch.float64)
        prs = 0.01 * torch.rand(res, dtype=torch.float64)
        mask = torch.zeros(res, dtype=torch.bool)
        mask[2:5, 1:4, :] = True
        if slab is not None:
            z = slab.z_indices()
            vel, prs, mask = vel[..., z], prs[..., z], mask[..., z]

        class Forced(lt.TaylorGreenVortex):
            extra = None

            @property
            def boundaries(self):
                return [] if self.extra is None else [self.extra]
        flow = Forced(c, slab.extended_resolution if slab is not None else res, 400, 0.1, lt.D3Q19(), slab=slab)
        flow.extra = lt.EquilibriumBoundaryPU(c, mask.cuda(), vel, prs)
        return flow
    c = gpu("f64")
    whole = setup(c)
    lt.Simulation(whole, lt.BGKCollision(whole.units.relaxation_parameter_lu), [])(steps)
    slab = lt.ZSlab(res, rank=0, world_size=1)
    part = setup(c, slab)
    sim = lt.SlabSimulation(part, lt.BGKCollision(part.units.relaxation_parameter_lu), slab)
    sim(steps)
    np.testing.assert_allclose(sim.gather_f().cpu().numpy(), whole.f.cpu().numpy(), rtol=0, atol=1e-14)


def test_slab_driver_with_an_outlet_along_z_on_gpu():
    """An anti-bounce-back outlet along the decomposed axis through the slab-layout kernels (one rank holds the
    whole grid, so it holds the outlet): == the reference path (non-native mirror on the CPU) of the same flow."""
    res, steps = [8, 6, 12], 6

    def channel(c, slab=None):
        zsel = slab.z_indices() if slab is not None else torch.arange(res[2])
        gz = zsel.reshape(1, 1, -1).expand(res[0], res[1], -1)
        block = torch.zeros(res, dtype=torch.bool)
        block[2:4, 1:3, 4:7] = True
        if slab is not None:
            block = block[..., zsel]

        class Channel(lt.TaylorGreenVortex):
            @property
            def boundaries(self):
                return [lt.EquilibriumBoundaryPU(self.context, (gz == 0).to(self.context.device), [0.0, 0.0, 0.05]),
                        lt.AntiBounceBackOutlet([0, 0, 1], self), lt.BounceBackBoundary(block.to(self.context.device))]
        return Channel(c, slab.extended_resolution if slab is not None else res, 100, 0.05, lt.D3Q19(), slab=slab)
    want = channel(lt.Context("cpu", torch.float64, use_native=False))
    lt.Simulation(want, lt.BGKCollision(want.units.relaxation_parameter_lu), [])(steps)
    slab = lt.ZSlab(res, rank=0, world_size=1)
    part = channel(gpu("f64"), slab)
    sim = lt.SlabSimulation(part, lt.BGKCollision(part.units.relaxation_parameter_lu), slab)
    sim(steps)
    np.testing.assert_allclose(sim.gather_f().cpu().numpy(), want.f.numpy(), rtol=0, atol=1e-13)
    whole = channel(gpu("f64"))
    lt.Simulation(whole, lt.BGKCollision(whole.units.relaxation_parameter_lu), [])(steps)
    np.testing.assert_allclose(whole.f.cpu().numpy(), want.f.numpy(), rtol=0, atol=1e-13)


def test_flow_with_two_outlets_native_equals_the_reference_path():
    """lt.Simulation on a native context with two AntiBounceBackOutlets == the non-native (reference) path of the
    mirror on the CPU, for both orders of the two outlets (str() decides the order, as in the reference)."""
    res = [10, 8, 6]

    def build(c, first):
        class OutX(lt.AntiBounceBackOutlet):
            def __str__(self):
                return "outlet-" + ("a" if first == "x" else "b")

        class OutY(lt.AntiBounceBackOutlet):
            def __str__(self):
                return "outlet-" + ("b" if first == "x" else "a")

        class TwoOutlets(lt.TaylorGreenVortex):
            made = None

            @property
            def boundaries(self):
                if self.made is None:
                    x = self.grid[0]
                    block = torch.zeros(res, dtype=torch.bool, device=self.context.device)
                    block[4:6, 3:5, 2:4] = True
                    self.made = [lt.EquilibriumBoundaryPU(self.context, torch.abs(x) < 1e-6, [0.3, 0.0, 0.0]),
                                 OutX([1, 0, 0], self), OutY([0, 1, 0], self), lt.BounceBackBoundary(block)]
                return self.made
        return TwoOutlets(c, res, 100, 0.05, lt.D3Q19())
    for first in ("x", "y"):
        want = build(lt.Context("cpu", torch.float64, use_native=False), first)
        got = build(gpu("f64"), first)
        sw = lt.Simulation(want, lt.BGKCollision(want.units.relaxation_parameter_lu), [])
        sg = lt.Simulation(got, lt.BGKCollision(got.units.relaxation_parameter_lu), [])
        for sim_ in (sw, sg):
            assert [str(b) for b in sim_.boundaries[1:] if str(b).startswith("outlet")] == ["outlet-a", "outlet-b"]
        sw(6); sg(6)
        assert sg._native.plan.kernel_name().endswith(", 1>")       # the two-outlet instantiation ran
        np.testing.assert_allclose(got.f.cpu().numpy(), want.f.numpy(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("order", ["xyz", "zyx", "yzx"])
def test_flow_with_outlets_on_all_three_axes_native_equals_the_reference_path(order):
    """lt.Simulation on a native context with AntiBounceBackOutlets on +x, +y and +z (planes meeting in a corner, where an
    outlet's neighbour was rewritten by two earlier outlets; lettuce/_simulation.py:57-86 takes any list) == the
    non-native (reference) path of the mirror on the CPU, for three orders of the outlets."""
    res = [9, 8, 7]

    def build(c):
        def named(axis):
            class Out(lt.AntiBounceBackOutlet):
                def __str__(self):
                    return f"outlet-{order.index('xyz'[axis])}"
            return Out

        class ThreeOutlets(lt.TaylorGreenVortex):
            made = None

            @property
            def boundaries(self):
                if self.made is None:
                    x = self.grid[0]
                    block = torch.zeros(res, dtype=torch.bool, device=self.context.device)
                    block[4:6, 3:5, 2:4] = True
                    outs = [named(a)([1 if k == a else 0 for k in range(3)], self) for a in range(3)]
                    self.made = ([lt.EquilibriumBoundaryPU(self.context, torch.abs(x) < 1e-6, [0.3, 0.0, 0.0])] + outs
                                 + [lt.BounceBackBoundary(block)])
                return self.made
        return ThreeOutlets(c, res, 100, 0.05, lt.D3Q27())
    want = build(lt.Context("cpu", torch.float64, use_native=False))
    got = build(gpu("f64"))
    sw = lt.Simulation(want, lt.KBCCollision(), [])
    sg = lt.Simulation(got, lt.KBCCollision(), [])
    for sim_ in (sw, sg):
        assert [str(b) for b in sim_.boundaries[1:] if str(b).startswith("outlet")] == ["outlet-0", "outlet-1", "outlet-2"]
    sw(5); sg(5)
    assert sg._native.plan.kernel_name().endswith(", 2>")           # the three-axes instantiation ran
    np.testing.assert_allclose(got.f.cpu().numpy(), want.f.numpy(), rtol=0, atol=1e-12)


def test_cfg1_simplest_tgv_energy_anchors():
    """BASELINE configs[0] = examples/00_simplest_TGV.py (D2Q9 128^2 fp64 Re 100 Ma 0.05, BGK,
    1000 steps) on the HIP engine against the reference CPU path: populations after 100 steps
    (golden) and the kinetic energies the survey recorded from the reference at steps
    0 / 100 / 500 / 1000."""
    g = golden("tgv2d_d2q9_bgk_128_f64")
    flow = lt.TaylorGreenVortex(gpu("f64"), 128, 100, 0.05, lt.D2Q9())
    assert flow.units.relaxation_parameter_lu == pytest.approx(0.610851251684408, rel=1e-14)
    out = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr("sys.stdout", io.StringIO())
        rep = lt.ObservableReporter(lt.IncompressibleKineticEnergy(flow), interval=100, out=out)
    sim = lt.Simulation(flow, lt.BGKCollision(flow.units.relaxation_parameter_lu), [rep])
    sim(100)
    np.testing.assert_allclose(flow.f.cpu().numpy(), g["f100"], rtol=0, atol=1e-12)
    sim(900)
    energy = {row[0]: row[2] for row in out}
    anchors = {0: 9.86960440108935, 100: 9.52452318761345, 500: 8.26054982612006, 1000: 6.91369866821884}
    for i, e in anchors.items():
        assert energy[i] == pytest.approx(e, rel=1e-10)
    assert float(flow.f.sum().cpu()) == pytest.approx(16384.0, rel=1e-12)      # mass


def test_convergence_order_tgv2d():
    """`lettuce convergence` (lettuce/cli.py:128-180) on the HIP engine: diffusive scaling on
    the 2-D Taylor-Green vortex gives second order in u and first order in p."""
    c = gpu("f64")
    errors = []
    for res in (16, 32, 64, 128):
        flow = lt.TaylorGreenVortex(c, [res] * 2, reynolds_number=10000, mach_number=8 / res)
        rep = lt.ErrorReporter(flow.analytic_solution, interval=1, out=None)
        sim = lt.Simulation(flow, lt.BGKCollision(flow.units.relaxation_parameter_lu), [rep])
        sim(10 * res)
        errors.append(np.mean(np.abs(rep.out), axis=0))
    order_u = np.log2(errors[-2][0] / errors[-1][0])
    order_p = np.log2(errors[-2][1] / errors[-1][1])
    # the reference accepts factor/2 within 0.1 of 2 (u) and of 1 (p)
    assert 1.8 < 2 ** order_u / 2 < 2.2, (errors, order_u)
    assert 0.8 < 2 ** order_p / 2 < 1.2, (errors, order_p)


def test_cli_convergence_command_with_its_defaults(capsys):
    """`python -m lettuce_amd convergence` as the reference's CLI runs it (double precision, 16^2 ... 256^2; the
    last grids go through the several-steps-per-launch kernel): exit code 0, i.e. orders within 0.1 of 2 and 1."""
    from lettuce_amd.cli import main
    assert main(["convergence"]) == 0
    assert "FAILED" not in capsys.readouterr().out


@pytest.mark.parametrize("transport", ["auto", "all"])
def test_bench_slab_path_on_one_gpu(tmp_path, transport):
    """`bench.py --slab` (the N > 1 code path with the rank exchanging its ghost planes with itself through RCCL) on a
    small grid.  auto: the single-step driver (timed first, its line held) and the two-step driver with the direct
    schedule; all: also the edge-launch schedule, the signalled launch and the peer-window transports.  Every candidate
    that ran ends bit-identical to the single-step reference after the warm-up probe AND after its timed batches, one
    is chosen, and the line carries the fields the driver reads."""
    import json
    import subprocess
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LT_SLAB_FORCE_P2P="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29200 + os.getpid() % 500))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--slab", "--size", "64", "--steps", "6", "--warmup", "3",
                          "--batches", "2", "--transport", transport], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    t = line["config"]["transport"]
    ran = set(t["warmup_ms_per_step"])
    expected = {"single-step/rccl", "two-step/rccl"}
    if transport == "all":
        expected |= {"two-step/rccl-edges", "two-step/rccl-signalled"}
    assert expected <= ran, t
    assert all(isinstance(v, float) for v in t["warmup_ms_per_step"].values()), t
    for name in ran - {"single-step/rccl"}:
        assert "bit-identical to single-step/rccl after the warm-up probe" in t["checks"][name], t
        assert "bit-identical after the timed batches too" in t["checks"][name], t
    # only the peer-window transports may be unavailable on a box (no symmetric memory)
    assert all(name.split("/")[1].startswith("window") for name in t["failures"]), t
    assert t["chosen"] in ran
    assert line["n_gpus"] == 1 and line["steps"] == 6 and line["value"] > 0 and line["unit"] == "MLUPS"
    assert line["repeats_per_batch"] >= 1 and len(line["batches_ms_per_step"]) == 2


def test_bench_plain_run_on_one_gpu(tmp_path):
    """`bench.py` without --full: W warm-up steps, one timed call of exactly K steps and the headline fields, none of
    the --full extras; --dump-outputs writes the populations the timed path left (whole here: 19 x 64^3 elements),
    the same in two runs with the same arguments and equal to the CPU oracle after W + K steps."""
    import json
    import subprocess
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for run in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--size", "64", "--steps", "10", "--warmup",
                              "4", "--dump-outputs", str(tmp_path / run)], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads(out.stdout.strip().splitlines()[-1])
        assert line["steps"] == 10 and line["warmup"] == 4 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "MLUPS" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["full"] is False and len(line["batches_ms_per_step"]) == 1 and line["repeats_per_batch"] == 1
        assert line["roofline"] is None and line["cpu_baseline"] is None and "other_configs" not in line
        dumps.append(np.load(tmp_path / run / "f.npy"))
    assert dumps[0].dtype == np.float32 and dumps[0].shape == (19 * 64 ** 3,)
    assert np.array_equal(dumps[0], dumps[1])
    ref = orc.taylor_green([64] * 3, 1600, 0.1, "D3Q19", torch.float32)
    ref.step(4 + 10)
    want = ref.f.numpy().reshape(-1)
    assert np.abs(dumps[0] - want).max() <= 1e-5 * np.abs(want).max()


def test_non_native_mode_on_a_gpu_device():
    """Context('cuda', use_native=False): the reference's whole-field torch expressions on device
    tensors (per-node contractions evaluated without BLAS) still match the reference vectors."""
    g = golden("obstacle3d_d3q27_kbc_f64")
    c = lt.Context("cuda:0", torch.float64, use_native=False)
    flow = lt.Obstacle(c, [int(r) for r in g["resolution"]], 100, 0.1, float(g["domain_length_x"]), stencil=lt.D3Q27())
    flow.mask = g["obstacle_mask"]
    flow.initialize()
    sim = lt.Simulation(flow, lt.KBCCollision(), [])
    assert sim._native is None
    sim(2)
    np.testing.assert_allclose(flow.f.cpu().numpy(), g["f2"], rtol=0, atol=1e-12)
    g = golden("tgv3d_d3q19_bgk_16_f64")
    flow = lt.TaylorGreenVortex(c, [16] * 3, 1600, 0.1, lt.D3Q19())
    np.testing.assert_allclose(flow.f.cpu().numpy(), g["f0"], rtol=0, atol=1e-13)
    lt.Simulation(flow, lt.BGKCollision(flow.units.relaxation_parameter_lu), [])(10)
    np.testing.assert_allclose(flow.f.cpu().numpy(), g["f10"], rtol=0, atol=1e-12)
    assert float(lt.IncompressibleKineticEnergy(flow)()) == pytest.approx(float(g["energy_pu"][1]), rel=1e-10)


# ----------------------------------------------------------------------------- full BASELINE sizes
def test_full_size_cfg4_obstacle_d3q27_kbc_properties():
    """BASELINE configs[3] size (Obstacle D3Q27 256^3, KBC, fp32, inlet + ABB outlet + sphere
    bounce-back): the fused masked kernel equals collide-then-stream at full size, the field stays
    finite, and populations with e_x = 0 on the inlet plane are exactly the inlet equilibrium."""
    c = gpu()
    flow = lt.Obstacle(c, [256, 256, 256], 100, 0.1, domain_length_x=4, stencil=lt.D3Q27())
    x, y, z = flow.grid
    flow.mask = ((x - 1) ** 2 + (y - 2) ** 2 + (z - 2) ** 2) < 0.5 ** 2
    flow.initialize()
    sim = lt.Simulation(flow, lt.KBCCollision(), [])
    plan, tau = sim._native.plan, flow.units.relaxation_parameter_lu
    sim(3)                                             # 1 collide + 2 fused + 1 stream
    f3 = flow.f.clone()
    assert torch.isfinite(f3).all()
    # same three steps as separate collide / stream passes
    flow2 = lt.Obstacle(c, [256, 256, 256], 100, 0.1, domain_length_x=4, stencil=lt.D3Q27())
    flow2.mask = flow.mask
    flow2.initialize()
    a, b = flow2.f, torch.empty_like(flow2.f)
    for _ in range(3):
        plan.collide(a, b, tau)
        plan.stream(b, a)
    torch.testing.assert_close(f3, a, rtol=0, atol=2e-6)
    inlet = lt.EquilibriumBoundaryPU(c, None, velocity=[1.0, 0.0, 0.0])._feq(flow)
    for q in (0, 3, 4, 5, 6, 7, 8, 9, 10):             # e_x = 0
        assert torch.equal(f3[q, 0], inlet[q].expand(256, 256))
    solid = flow.mask.to("cuda")
    assert int(solid.sum()) > 100_000                   # the sphere is there


def test_full_size_cfg5_slab_shear_fp64_conservation():
    """BASELINE configs[4] per-GPU size (periodic shear, D3Q19 384 x 384 x 96, fp64): BGK on a
    periodic box conserves mass and momentum to rounding over 20 steps."""
    c = gpu("f64")
    flow = lt.DoublyPeriodicShear3D(c, [384, 384, 96], 10000, 0.1)
    sim = lt.Simulation(flow, lt.BGKCollision(flow.units.relaxation_parameter_lu), [])
    plan = sim._native.plan
    m0 = float(plan.mass(flow.f).cpu())
    j0 = flow.j().sum(dim=(1, 2, 3)).cpu()
    sim(20)
    assert float(plan.mass(flow.f).cpu()) == pytest.approx(m0, rel=1e-13)
    j1 = flow.j().sum(dim=(1, 2, 3)).cpu()
    assert torch.allclose(j1, j0, rtol=0, atol=1e-9 * 384 * 384 * 96 * 0.06)
    assert torch.isfinite(flow.f).all()


def test_full_size_cfg3_slab_equals_single_domain():
    """BASELINE configs[2] per-GPU slab (512 x 512 x 64, fp32): the z-slab driver (slab-layout
    kernels, boundary planes + packed ghost exchange on the second stream) gives the same
    populations as the single-domain engine on the same periodic box."""
    res = [512, 512, 64]
    c = gpu()
    slab = lt.ZSlab(res, rank=0, world_size=1)
    fl_s = lt.TaylorGreenVortex(c, slab.extended_resolution, 1600, 0.1, lt.D3Q19(), slab=slab)
    tau = fl_s.units.relaxation_parameter_lu
    sim_s = lt.SlabSimulation(fl_s, lt.BGKCollision(tau), slab)
    fl_p = lt.TaylorGreenVortex(c, res, 1600, 0.1, lt.D3Q19())
    torch.testing.assert_close(sim_s.gather_f(), fl_p.f, rtol=0, atol=1e-6)
    sim_p = lt.Simulation(fl_p, lt.BGKCollision(tau), [])
    sim_s(6)
    sim_p(6)
    torch.testing.assert_close(sim_s.gather_f(), fl_p.f, rtol=0, atol=2e-6)
    assert sim_s.kinetic_energy_pu() == pytest.approx(float(lt.IncompressibleKineticEnergy(fl_p)()), rel=1e-6)


def test_fneq_initialisation_kernel_against_the_reference_expression_on_random_fields():
    """lt_init_fneq against the oracle's restatement of initialize_f_neq (_flow.py:309-336) on random smooth
    fields, 2-D and 3-D, fp64: rounding level."""
    from oracle import lettuce_oracle as orc
    torch.manual_seed(11)
    for stencil, res in ((lt.D2Q9, [12, 9]), (lt.D3Q19, [8, 7, 10]), (lt.D3Q27, [7, 8, 9]), (lt.D3Q15, [8, 8, 8])):
        st = stencil()
        flow = lt.TaylorGreenVortex(gpu("f64"), res if st.d == 3 else res, 100, 0.05, st, initialize_fneq=False)
        rho = 1 + 0.01 * torch.rand([1] + res, dtype=torch.float64)
        u = 0.05 * torch.rand([st.d] + res, dtype=torch.float64)
        e, w = orc.lattice_tensors(orc.LATTICES[stencil.__name__], torch.float64)
        f_eq = orc.quadratic_equilibrium(rho, u, e, w)
        flow.f = f_eq.cuda()
        from lettuce_amd._flow import initialize_f_neq
        got = initialize_f_neq(flow).cpu()
        # non-native expression of the mirror on the CPU (validated against the reference's f0 vectors)
        cpu_flow = lt.TaylorGreenVortex(lt.Context("cpu", torch.float64, use_native=False), res, 100, 0.05, stencil(),
                                        initialize_fneq=False)
        cpu_flow.f = f_eq.clone()
        want = initialize_f_neq(cpu_flow)
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=2e-16 * float(want.abs().max()) * 8)


def test_device_contraction_without_blas_at_the_slab_shape_that_faulted():
    """Regression for the round-1 fault: per-node contractions of a 512 x 512 x 70 fp32
    slab went through torch's einsum -> GEMM (19 x 9 times 9 x 18.35 M) and faulted inside the BLAS kernel.
    Device tensors do not go through BLAS any more; local_contract at that very shape against CPU einsum."""
    from lettuce_amd._flow import local_contract
    torch.manual_seed(2)
    n = 512 * 512 * 70
    m = torch.rand(19, 9)
    field = torch.rand(9, n)
    want = torch.einsum("ik,kx->ix", m, field)
    got = local_contract(m.cuda(), field.cuda().reshape(9, 512, 512, 70)).reshape(19, n).cpu()
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=2e-6)


def test_long_run_energy_decay_fp32_tracks_fp64():
    """1000 steps of TGV3D D3Q19 at 64^3 on the HIP engine: the fp32 kinetic-energy series decays
    monotonically and stays within 3e-4 of the fp64 series.  The gap is the reference's own: its
    fp32 path divides by cs^2 constants rounded to fp32 (3e-8 too large), which costs 1.1e-7 of
    kinetic energy per step (1.25e-5 per 100 steps); the kernel reproduces that
    arithmetic exactly in order to track the reference's fp32 results."""
    series = {}
    for dt in ("f64", "f32"):
        flow = lt.TaylorGreenVortex(gpu(dt), [64] * 3, 1600, 0.1, lt.D3Q19())
        out = []
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr("sys.stdout", io.StringIO())
            rep = lt.ObservableReporter(lt.IncompressibleKineticEnergy(flow), interval=100, out=out)
        lt.Simulation(flow, lt.BGKCollision(flow.units.relaxation_parameter_lu), [rep])(1000)
        series[dt] = np.array([row[2] for row in out])
        assert torch.isfinite(flow.f).all()
    assert len(series["f64"]) == 11 and (np.diff(series["f64"]) < 0).all() and (np.diff(series["f32"]) < 0).all()
    np.testing.assert_allclose(series["f32"], series["f64"], rtol=3e-4)
    drift = (series["f32"][-1] - series["f64"][-1]) / series["f64"][-1]
    assert -2.5e-4 < drift < -0.5e-4          # the reference-inherent loss, about -1.2e-4 here


def test_integration_md_ctypes_stub_steps_a_simulation():
    """The reference-side ctypes stub printed in INTEGRATION.md (section B) is executed as written
    -- only the library path is pointed at the in-tree build -- and plugged into the swap point
    `Simulation._collide_and_stream` of a non-native simulation on a GPU tensor."""
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    code = re.search(r"```python\n(# lettuce/hip_native.py.*?)```", text, re.S).group(1)
    from lettuce_amd._native import library_path
    code = code.replace('ctypes.CDLL("liblettuce_hip.so")', f'ctypes.CDLL("{library_path()}")')
    ns = {}
    exec(compile(code, "INTEGRATION.md", "exec"), ns)
    g = golden("tgv3d_d3q19_bgk_16_f32")
    c = lt.Context("cuda:0", torch.float32, use_native=False)
    flow = lt.TaylorGreenVortex(c, [16] * 3, 1600, 0.1, lt.D3Q19())
    sim = lt.Simulation(flow, lt.BGKCollision(flow.units.relaxation_parameter_lu), [])
    assert sim._native is None
    sim._collide_and_stream = ns["make_native_kernel"](sim)          # lettuce/_simulation.py:148
    sim(10)
    torch.cuda.synchronize()
    assert flow.i == 10
    np.testing.assert_allclose(flow.f.cpu().numpy(), g["f10"], rtol=0, atol=1e-5 * float(np.abs(g["f10"]).max()))


def test_engine_kernel_name_matches_the_committed_traffic_profile(monkeypatch):
    """the name bench.py looks up in profiles/traffic.json is the one the 256^3 plan reports (whether the
    table belongs to this build of the kernel sources is a separate question: its source_hash)"""
    import importlib.util
    import json
    from conftest import ROOT
    from lettuce_amd._native import Plan
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as fh:
        monkeypatch.setattr(bench, "source_hash", lambda h=json.load(fh).get("source_hash"): h)
    plan = Plan("D3Q19", torch.float32, "bgk", [256, 256, 256], [], device=torch.device("cuda:0"))
    assert bench.traffic_from_profile(plan.kernel_name()) is not None
