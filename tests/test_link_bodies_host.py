"""The assumptions of tests/test_gpu_link_bodies_vs_cpu.py about its inputs and its reference, checked without a GPU
(tests/link_body_cases.py holds both): every body's link list has links of both branches of the rule in at least 2 d
directions; no case is refused by ``native_link_list``; every reference run -- the mirror's torch path in fp64 and, for
the fp32 gate, in fp32 from the same fp32 state -- stays finite with small populations, and E_ref = max |cpu32 - cpu64| /
w_q is greater than zero (and below 1e-4), so that the gate E_gpu <= 4 E_ref is a yardstick and not a zero; the run that
part C replays graphs over stays finite too; and the CPU side of the reporter test -- the populations handed to the
reporter in both dtypes and the force of the torch expression against the exact sum over them -- holds on its own.
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import lettuce_amd as lt
import link_body_cases as cases
from conftest import TORCH_DT
from test_boundary_force_host import assert_within_bound
from test_gpu_link_bodies_vs_cpu import REPORTED, _reported
from test_gpu_link_bounce_back import exact_link_force
from test_link_bounce_back_host import STENCIL
from test_tune3_census import COLLISIONS


def test_the_table_has_every_collision_number_of_the_census():
    assert sorted({coll for coll, _ in cases.COLLISION}) == sorted(COLLISIONS) == [0, 1, 2, 3, 5, 7, 8, 9, 10, 11, 17, 21, 24, 25]
    assert {scheme for coll, scheme in cases.COLLISION if coll in (5, 7)} == {"guo", "shanchen"}
    listed = {(coll, lat) for coll, _, lat, _, _ in cases.part_a_cases()}
    assert listed == {(coll, lat.upper()) for coll, lats in COLLISIONS.items() for lat in lats if lat != "d1q3"}
    # 17 .. 25 are the mirror's operators on the incompressible equilibrium, not MRT
    flow = cases.cpu_flow("D3Q19", (6, 5, 7), torch.float64, 17)
    assert isinstance(flow.equilibrium, lt.IncompressibleQuadraticEquilibrium)
    assert isinstance(cases.mirror_operator(24, None, "D3Q19", flow), lt.TRTCollision)
    assert isinstance(cases.mirror_operator(7, "shanchen", "D3Q19", flow).force, lt.ShanChen)


@pytest.mark.parametrize("kind", cases.BODIES)
@pytest.mark.parametrize("lat,res", cases.SHAPES, ids=[cases.shape_id(*s) for s in cases.SHAPES])
def test_every_body_has_links_of_both_branches_in_2d_directions(lat, res, kind):
    boundary = cases.body(lat, res, kind)
    n, second, directions = cases.link_census(lat, res, boundary)
    print(f"{lat} {list(res)} {kind}: {n} links, {second} with d >= 1/2, {directions} directions")
    d = len(res)
    assert second >= 1 and n - second >= 1 and directions >= 2 * d
    for dt in ("f32", "f64"):                                        # alone in the plan: not refused
        listed = lt.native_link_list(boundary, 1, boundary.mask.to(torch.uint8), STENCIL[lat](), TORCH_DT[dt])
        assert len(listed[0]) == n


def _figures(what, pair, lat):
    f32, f64 = pair
    assert np.isfinite(f32).all() and np.isfinite(f64).all(), what
    e_ref = cases.weighted_error(lat, f32, f64)
    largest = float(np.abs(f64).max())
    print(f"{what}: |f|max {largest:.3f}, largest |cpu32 - cpu64| {float(np.abs(f32 - f64).max()):.3e}, E_ref {e_ref:.3e}")
    assert largest < 1.0                                             # the fp64 gate is 1e-12 max(1, |f|max): absolute here
    # fp32 has 2^-24 = 6e-8 per rounding and the populations are of the order of w_q
    assert 0 < e_ref < 1e-4, (what, e_ref)


@pytest.mark.parametrize("case", cases.part_a_cases(), ids=cases.part_a_id)
def test_part_a_references_are_finite_and_have_an_fp32_error(case):
    coll, scheme, lat, res, kind = case
    f64 = cases.reference(lat, res, "f64", coll, scheme, kind, "f64")
    for key, value in f64.items():
        assert np.isfinite(value).all() and float(np.abs(value).max()) < 1.0, (key, float(np.abs(value).max()))
    assert not np.array_equal(f64[1], f64[4])
    low, high = cases.reference(lat, res, "f32", coll, scheme, kind, "f32"), cases.reference(lat, res, "f32", coll, scheme, kind, "f64")
    for key in ("collide",) + cases.RUNS:
        _figures(f"{cases.part_a_id(case)} {key}", (low[key], high[key]), lat)


@pytest.mark.parametrize("cid", list(cases.SCENES))
def test_part_b_scenes_are_not_refused_and_their_references_hold(cid):
    _, lat, res, _, boundaries = cases.SCENES[cid]
    for dt in ("f32", "f64"):
        flow, simulation = cases.scene_simulation(cid, lt.Context("cpu", TORCH_DT[dt], use_native=False))
        assert abs(float(flow.units.relaxation_parameter_lu) - cases.SCENE_TAU) < 1e-12
        bodies = 0
        for index, boundary in enumerate(simulation.boundaries[1:], start=1):
            if not isinstance(boundary, lt.InterpolatedBounceBackBoundary):
                continue
            bodies += 1
            listed = lt.native_link_list(boundary, index, simulation.no_collision_mask, flow.stencil, TORCH_DT[dt])
            n, second, directions = cases.link_census(lat, res, boundary)
            print(f"{cid} {dt}: body of index {index} of {len(boundaries)}: {n} links, {second} with d >= 1/2, {directions} directions")
            assert len(listed[0]) == n and second >= 1 and n - second >= 1 and directions >= 2 * len(res)
            assert int((simulation.no_collision_mask == index).sum()) == 2
        assert bodies == sum(b[0] == "body" for b in boundaries) >= 1
    low, high = cases.scene_reference(cid, "f32", "f32"), cases.scene_reference(cid, "f32", "f64")
    f64 = cases.scene_reference(cid, "f64", "f64")
    for n in cases.SCENE_STEPS:
        assert np.isfinite(f64[n]).all() and float(np.abs(f64[n]).max()) < 1.0
        _figures(f"{cid} n = {n}", (low[n], high[n]), lat)


def test_part_b_has_every_kind_of_case():
    ids = list(cases.SCENES)
    kinds = {cid: [b[0] for b in cases.SCENES[cid][4]] for cid in ids}
    for letter in "abcde":
        assert any(cid.startswith(letter + "-") for cid in ids)
    a = [cid for cid in ids if cid.startswith("a-")]
    assert {kinds[cid].index("body") for cid in a} == {0, 1, 2} and all(set(kinds[cid]) == {"body", "inlet", "wall"} for cid in a)
    b = [cases.SCENES[cid] for cid in ids if cid.startswith("b-") and "-bgk-" in cid]
    for lat in ("D2Q9", "D3Q15", "D3Q19", "D3Q27"):
        d = len(cases.SMALL[lat])
        faces = {(s[2], s[4][0][0] == "body") + tuple(x for x in s[4] if x[0] == "abb")[0][1:] for s in b if s[1] == lat}
        assert faces == {(res, below, axis, side) for res in (cases.SMALL[lat], cases.ROW[lat]) for below in (True, False)
                         for axis in range(d) for side in (1, -1) if res == cases.SMALL[lat] or axis == d - 1}
        assert cases.ROW[lat][-1] == 64
    assert {cases.SCENES[cid][3] for cid in ids if cid[0] in "ab"} == {"bgk", "kbc", "trt", "guo"}
    c = [kinds[cid] for cid in ids if cid.startswith("c-")]
    assert all("pout" in k or k.count("abb") >= 2 for k in c) and any("pout" in k for k in c)
    assert {k.count("abb") for k in c} >= {1, 2, 3}
    assert all(kinds[cid].count("body") == 2 for cid in ids if cid.startswith("d-"))
    e = [cases.SCENES[cid] for cid in ids if cid.startswith("e-")]
    assert {s[1] for s in e} == {"D2Q9", "D3Q27"} and all("pout" in [b[0] for b in s[4]] for s in e)


@pytest.mark.parametrize("case", REPORTED, ids=cases.part_c_id)
def test_part_c_reporter_runs_on_the_cpu(case):
    """the CPU side of the reporter test: the populations handed to the reporter in fp32 and fp64 from the same state, and
    every force the torch expression reports against the exact sum over those populations"""
    coll, scheme, lat, res, kind, dt = case
    f0 = cases.state(lat, res, dt)
    runs = {run: _reported(case, lt.Context("cpu", TORCH_DT[run], use_native=False), f0.to(TORCH_DT[run]), 12, 3)
            for run in ("f32", "f64")}
    assert torch.equal(f0, cases.state(lat, res, dt))                # nothing stepped the state in place
    for k in range(5):
        low, high = runs["f32"][2][k].double().numpy(), runs["f64"][2][k].numpy()
        if k == 0:
            assert np.array_equal(low, f0.float().double().numpy()) and np.array_equal(high, f0.double().numpy())
        elif dt == "f32":
            _figures(f"{cases.part_c_id(case)} report {k}", (low, high), lat)
        _, _, seen, forces, boundary = runs[dt]
        exact = exact_link_force(STENCIL[lat](), seen[k], boundary.mask, boundary.fractions)
        assert_within_bound(forces[k], exact, TORCH_DT[dt], f"{cases.part_c_id(case)} report {k}")


@pytest.mark.parametrize("case", cases.PART_C, ids=cases.part_c_id)
def test_part_c_runs_stay_finite_over_the_replayed_graphs(case):
    coll, scheme, lat, res, kind, dt = case
    f = cases.long_reference(lat, res, dt, coll, scheme, kind)
    largest = float(np.abs(f).max())
    print(f"{cases.part_c_id(case)}: |f|max after {cases.GRAPH_STEPS} steps {largest:.3f}")
    assert np.isfinite(f).all() and largest < 1.0
