"""The constant-pressure equilibrium outlet (EquilibriumOutletP) on the host (CPU, no GPU needed): the mirror's torch
path against vectors produced by the reference's own CPU path (tests/golden/outlet_p_*.npz, made by
tools/gen_golden_outlet_p.py) with the boundaries in the order the reference used, the class's masks, the sort order of
the four boundary classes, and the plumbing that hands the boundary to the HIP engine (descriptor, binding, header,
lt_plan_create's checks).

Bounds: fp64 the 2e-14 of test_oracle_golden.py, fp32 1e-5 max(1, max |f|) -- for the collided field and every stepped
snapshot alike."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lettuce_amd as lt
from conftest import golden, unpack_nsm, TORCH_DT, ROOT
from outlet_p_cases import FIXTURES, SEVERAL, dtype_tag, fp32_bound, make_collision, mirror_flow


def close(got, want, dt):
    got, want = np.asarray(got), np.asarray(want)
    bound = 2e-14 if dt == "f64" else fp32_bound(want)
    err = float(np.abs(got - want).max())
    print(f"max |difference| {err:.3e} (bound {bound:.1e})")
    assert err <= bound


def cpu(dt):
    return lt.Context("cpu", TORCH_DT[dt], use_native=False)


@pytest.mark.parametrize("name", FIXTURES)
def test_torch_path_matches_the_reference(name):
    """Simulation._collide alone and f after 1, 2 and 6 steps, boundaries in the stored order"""
    g = golden(name)
    dt = dtype_tag(name)
    flow = mirror_flow(g, name, cpu(dt))
    sim = lt.Simulation(flow, make_collision(g), [])
    assert [type(b).__mro__[1].__name__ for b in sim.boundaries[1:]] == [str(k) for k in g["boundary_order"]]
    f0 = flow.f.clone()
    close(sim._collide().numpy(), g["collided"], dt)
    flow.f = f0
    for i in range(1, 7):
        sim(1)
        if i in (1, 2, 6):
            close(flow.f.numpy(), g[f"f{i}"], dt)


@pytest.mark.parametrize("name", FIXTURES)
def test_masks_are_the_references(name):
    g = golden(name)
    flow = mirror_flow(g, name, cpu(dtype_tag(name)))
    sim = lt.Simulation(flow, make_collision(g), [])
    np.testing.assert_array_equal(sim.no_collision_mask.numpy(), g["no_collision_mask"])
    np.testing.assert_array_equal(sim.no_streaming_mask.numpy().astype(np.uint8), unpack_nsm(g))
    # the class's own: its index on the whole plane, and every population with e_q . direction != 1 kept there
    q, d = flow.stencil.q, flow.stencil.d
    for b in sim.boundaries[1:]:
        if not isinstance(b, lt.EquilibriumOutletP):
            continue
        ncm = b.make_no_collision_mask(list(flow.resolution), flow.context).numpy()
        nsm = b.make_no_streaming_mask([q] + list(flow.resolution), flow.context).numpy()
        plane = tuple(b.index)
        assert ncm[plane].all() and ncm.sum() == ncm[plane].size
        kept = nsm.reshape(q, -1).any(axis=1)
        leaving = np.array(flow.stencil.e) @ np.array(b.direction) == 1
        np.testing.assert_array_equal(kept, ~leaving)
        assert kept.sum() == q - (3 if d == 2 else (1 if d == 1 else {15: 5, 19: 5, 27: 9}[q]))
        assert nsm.sum() == kept.sum() * ncm.sum()


@pytest.mark.parametrize("name", [n for n in SEVERAL if "mixed" not in n])
def test_the_order_of_several_outlets_matters(name):
    """what makes the stored order necessary: the same boundaries with the pressure outlets in reverse order give other
    populations (where the planes meet, the later outlet reads what the earlier one wrote; the -y and +y outlets of the
    "mixed" fixtures never meet)"""
    g = golden(name)
    dt = dtype_tag(name)
    kinds = [str(k) for k in g["boundary_order"]]
    where = [i for i, k in enumerate(kinds) if k == "EquilibriumOutletP"]
    swapped = dict(g)
    for key in ("boundary_direction", "rho_outlet"):
        swapped[key] = g[key].copy()
        swapped[key][where] = g[key][where[::-1]]
    flow = mirror_flow(swapped, name, cpu(dt))
    lt.Simulation(flow, make_collision(g), [])(6)
    gap = float(np.abs(flow.f.numpy() - g["f6"]).max())
    print(f"reversed order: {gap:.2e}")
    assert gap > 100 * (2e-14 if dt == "f64" else fp32_bound(g["f6"]))


def test_the_four_classes_sort_as_in_the_reference():
    """Simulation sorts by str(boundary): anti_bounce_back_outlet < bounce_back_boundary < equilibrium_boundary_pu <
    equilibrium_outlet_p in the reference's module paths, and the mirror's class names give the same"""
    context = cpu("f64")
    flow = lt.Obstacle(context, [8, 6], 100, 0.05, 2, stencil=lt.D2Q9())
    mask = torch.zeros([8, 6], dtype=torch.bool)
    made = [lt.EquilibriumOutletP([0, 1], flow, 1.01), lt.EquilibriumBoundaryPU(context, mask, [0.1, 0.0]),
            lt.BounceBackBoundary(mask), lt.AntiBounceBackOutlet([1, 0], flow)]
    names = [type(b).__name__ for b in sorted(made, key=str)]
    assert names == ["AntiBounceBackOutlet", "BounceBackBoundary", "EquilibriumBoundaryPU", "EquilibriumOutletP"]


def test_reference_signature_assertions_and_exports():
    context = cpu("f32")
    flow = lt.Obstacle(context, [8, 6], 100, 0.05, 2, stencil=lt.D2Q9())
    outlet = lt.EquilibriumOutletP([1, 0], flow)
    assert isinstance(outlet, lt.AntiBounceBackOutlet) and isinstance(outlet, lt.Boundary)
    assert lt.ext.EquilibriumOutletP is lt.EquilibriumOutletP
    assert outlet.rho_outlet.dtype == torch.float32 and float(outlet.rho_outlet) == 1.0
    assert float(lt.EquilibriumOutletP([0, -1], flow, rho_outlet=1.02).rho_outlet) == float(np.float32(1.02))
    assert outlet.native_available()
    for bad in ([1, 1], [0, 0], [2, 0], [1, 0, 0, 0]):
        with pytest.raises(AssertionError):
            lt.EquilibriumOutletP(bad, flow)
    assert "out of scope" not in lt.ext._boundary.__doc__


def test_descriptor_reads_rho_outlet_late():
    flow = lt.Obstacle(cpu("f32"), [8, 6], 100, 0.05, 2, stencil=lt.D2Q9())
    outlet = lt.EquilibriumOutletP([0, -1], flow, rho_outlet=1.02)
    desc = outlet.native_generator(3)
    assert isinstance(desc, lt.native_desc.NativeBoundary) and (desc.kind, desc.index) == ("pressure_outlet", 3)
    entry = desc.plan_entry(flow)
    assert entry == {"kind": "pressure_outlet", "axis": 1, "side": -1, "present": True,
                     "rho_outlet": float(np.float32(1.02))}
    outlet.rho_outlet.fill_(0.97)                                    # written in place: the version changes
    assert desc.plan_entry(flow)["rho_outlet"] == float(np.float32(0.97))
    outlet.rho_outlet = torch.tensor(1.5)                            # replaced
    assert desc.plan_entry(flow)["rho_outlet"] == 1.5


def test_in_place_write_covers_the_whole_plane():
    """a node of the plane that carries another boundary's index is overwritten too, and flow.f itself is written"""
    g = golden("outlet_p_block_d2q9_f64")
    flow = mirror_flow(g, "outlet_p_block_d2q9_f64", cpu("f64"))
    outlet = [b for b in flow.boundaries if isinstance(b, lt.EquilibriumOutletP)][0]
    assert g["block_mask"][-1].any() and (g["no_collision_mask"][-1] == len(flow.boundaries)).all()
    before = flow.f.clone()
    result = outlet(flow)
    assert torch.equal(result, flow.f) and not torch.equal(flow.f[:, -1], before[:, -1])
    assert torch.equal(flow.f[:, :-1], before[:, :-1])
    rho_w, u_n = outlet.rho_outlet * torch.ones_like(flow.rho()[:, -1]), flow.u()[:, -2]      # (that plane is untouched)
    feq = flow.equilibrium(flow, rho_w[..., None], u_n[..., None])[..., 0]
    assert torch.equal(flow.f[:, -1], feq)


def _desc(kind, axis, side, rho=1.0, stencil=1, dims=3, shape=(8, 6, 4), layout=0, ghosts=0):
    from lettuce_amd import _native
    d = _native._PlanDesc()
    d.abi_version = _native.LT_ABI_VERSION
    d.stencil, d.dtype, d.collision, d.layout, d.ghost_planes, d.dims = stencil, 0, 1, layout, ghosts, dims
    for a in range(3):
        d.shape[a] = shape[a] if a < dims else 1
    d.n_boundaries = 1
    d.boundaries[0].kind, d.boundaries[0].axis, d.boundaries[0].side = kind, axis, side
    d.boundaries[0].feq[0] = rho
    return d


def test_binding_header_and_plan_create(engine_library):
    """the enumerator, the binding's id, and lt_plan_create's answer to a bad axis or side -- LT_ERR_INVALID with the
    boundary's name, decided before anything touches a device"""
    from lettuce_amd import _native
    assert _native.BOUNDARY_KINDS == {"bounce_back": 1, "equilibrium": 2, "abb_outlet": 3, "pressure_outlet": 4}
    header = open(os.path.join(ROOT, "include", "lettuce_hip.h")).read()
    assert re.search(r"\bLT_BOUNDARY_PRESSURE_OUTLET\s*=\s*4\b", header)
    assert re.search(r"\bLT_BOUNDARY_ABB_OUTLET\s*=\s*3\b", header)
    assert re.search(r"#define\s+LT_ABI_VERSION\s+2\b", header)       # one enum value, no new field or function
    assert ctypes.sizeof(_native._BoundaryDesc) == 16 + 8 * _native.LT_MAX_Q + 8
    lib = ctypes.CDLL(engine_library)
    lib.lt_plan_create.restype = ctypes.c_int
    lib.lt_plan_create.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.lt_last_error.restype = ctypes.c_char_p
    for axis, side in ((3, 1), (-1, 1), (0, 0), (1, 2)):
        handle = ctypes.c_void_p()
        d = _desc(4, axis, side)
        assert lib.lt_plan_create(ctypes.byref(d), ctypes.byref(handle)) == 1      # LT_ERR_INVALID
        assert b"constant-pressure outlet" in lib.lt_last_error() and handle.value is None
    # a valid axis and side pass every check: the call succeeds, or fails only where it asks for device memory
    lib.lt_plan_destroy.argtypes = [ctypes.c_void_p]
    for axis in range(3):
        for side in (1, -1):
            handle = ctypes.c_void_p()
            d = _desc(4, axis, side, rho=1.02)
            rc = lib.lt_plan_create(ctypes.byref(d), ctypes.byref(handle))
            assert rc in (0, 3, 4) and (rc == 0 or b"outlet" not in lib.lt_last_error()), (rc, lib.lt_last_error())
            if rc == 0:
                lib.lt_plan_destroy(handle)
    handle = ctypes.c_void_p()
    d = _desc(4, 2, 1, stencil=0, dims=2, shape=(8, 6, 1))                         # D2Q9 has no z axis
    assert lib.lt_plan_create(ctypes.byref(d), ctypes.byref(handle)) == 1
    d = _desc(5, 0, 1)
    assert lib.lt_plan_create(ctypes.byref(d), ctypes.byref(handle)) == 1
    assert b"unknown boundary kind 5" in lib.lt_last_error()
    d = _desc(4, 0, 1, shape=(1, 6, 4))
    assert lib.lt_plan_create(ctypes.byref(d), ctypes.byref(handle)) == 1
    assert b">= 2 planes" in lib.lt_last_error()


@pytest.mark.gpu
def test_plan_create_accepts_the_kind_on_a_device(engine_library):
    """a valid axis and side pass the checks and the plan is made (needs device memory for the plan's tables)"""
    from lettuce_amd._native import Plan
    for axis in range(3):
        for side in (1, -1):
            plan = Plan("D3Q19", torch.float32, "bgk", [8, 6, 4],
                        [{"kind": "pressure_outlet", "axis": axis, "side": side, "rho_outlet": 1.02}])
            plan.close()


def test_slab_plane_logic_is_inherited():
    """on a z-slab the outlet along z lives on the rank that holds the plane, shifted by the halo; absent elsewhere"""
    context = cpu("f32")
    for rank, present in ((0, False), (1, True)):
        slab = lt.ZSlab([8, 6, 8], rank, 2)
        flow = lt.Obstacle(context, slab.extended_resolution, 100, 0.05, 2, stencil=lt.D3Q19(), slab=slab)
        outlet = lt.EquilibriumOutletP([0, 0, 1], flow, 1.02)
        assert outlet.present is present
        entry = outlet.native_generator(1).plan_entry(flow)
        assert entry["present"] is present and entry["axis"] == 2
        ncm = outlet.make_no_collision_mask(list(flow.resolution), context)
        assert bool(ncm.any()) is present
        if present:
            assert outlet.index[2] == slab.halo + slab.nz_local - 1 and outlet.neighbor[2] == outlet.index[2] - 1
            before = flow.f.clone()
            outlet(flow)
            assert not torch.equal(flow.f[..., outlet.index[2]], before[..., outlet.index[2]])
        else:
            before = flow.f.clone()
            assert torch.equal(outlet(flow), before)
