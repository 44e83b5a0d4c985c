"""The ring harness of slab_ring.py on the CPU stand-in: every schedule, 2 and 3 ranks, D3Q15 / D3Q19 / D3Q27 in
float64 against the single-domain oracle, and two negative controls that show the harness sees what it is for --
messages from the wrong neighbour, and a message whose near-plane and far-plane crossing blocks changed places.

The stand-in composes every entry point from the oracle's own collide and roll, so a schedule that moves the right
planes reproduces the oracle to rounding (bound 1e-13 max|f|); a control must move the result by more than 100 fp32
tolerances (1e-3 max|f|), or the GPU tests that use this harness at 1e-5 max|f| could not tell such a fault.
"""
import functools

import pytest
import torch

from oracle import lettuce_oracle as orc
from slab_cpu_engine import OracleSlabEngine
from slab_ring import SCHEDULES, SlabRing
from test_gpu_paths_vs_oracle import perturbed_state

TAU = 0.7
LATTICES = ("D3Q15", "D3Q19", "D3Q27")
NZ_LOCAL = {2: 6, 3: 5}          # planes per rank: edges of 3 planes cover the slab / edges of 2 leave one between


def _state(lat, world):
    return perturbed_state(lat, [6, 4, NZ_LOCAL[world] * world], torch.float64, 7)


@functools.lru_cache(maxsize=None)
def _oracle(lat, world, fused):
    sim = orc.OracleSimulation(orc.LATTICES[lat], _state(lat, world).clone(), "bgk", TAU)
    sim.step(fused + 1)
    return sim.f


def _ring(lat, world, schedule, fused, fault=None):
    engines = [OracleSlabEngine(lat, torch.float64, "bgk") for _ in range(world)]
    for e in engines:
        e.ghosts = 1 if schedule == "pair" else 2
    ring = SlabRing(engines, lat, schedule, edge_planes=3 if world == 2 else 2, fault=fault)
    return ring.run(_state(lat, world), TAU, fused)


@pytest.mark.parametrize("fused", [4, 5])
@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("lat", LATTICES)
def test_every_schedule_of_the_ring_reproduces_the_single_domain_oracle(lat, world, schedule, fused):
    want = _oracle(lat, world, fused)
    got = _ring(lat, world, schedule, fused)
    diff = float((got - want).abs().max())
    print(f"{lat} {world} ranks {schedule} {fused} fused steps: max |difference| {diff:.3e}")
    assert diff <= 1e-13 * float(want.abs().max())


CONTROLS = [("wrong-neighbour", 3, "direct"), ("wrong-neighbour", 3, "pair"), ("swapped-crossing-blocks", 2, "direct"),
            ("swapped-crossing-blocks", 2, "planes")]


@pytest.mark.parametrize("fault,world,schedule", CONTROLS, ids=["-".join(map(str, c)) for c in CONTROLS])
@pytest.mark.parametrize("lat", LATTICES)
def test_the_ring_sees_a_misrouted_and_a_mislaid_message(lat, fault, world, schedule):
    """negative controls: each fault is far above the tolerance the GPU tests hold the kernels to"""
    fused = 5
    want = _oracle(lat, world, fused)
    got = _ring(lat, world, schedule, fused, fault=fault)
    diff = float((got - want).abs().max()) / float(want.abs().max())
    print(f"{lat} {fault} {schedule}: max |difference| {diff:.3e} max|f|")
    assert diff > 1e-3
