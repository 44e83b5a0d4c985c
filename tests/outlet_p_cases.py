"""What the tests of the constant-pressure outlet share: the names of the fixtures tools/gen_golden_outlet_p.py wrote
(tests/golden/outlet_p_*.npz), the mirror's flow of a fixture with its boundaries in the order the reference used (among
objects of one class that order is arbitrary there and changes the result, so it is stored and replayed through
``__str__``), and the same boundaries as entries of an engine plan."""
import numpy as np
import torch

import lettuce_amd as lt
from conftest import TORCH_DT

LATTICES = {"d1q3": lt.D1Q3, "d2q9": lt.D2Q9, "d3q15": lt.D3Q15, "d3q19": lt.D3Q19, "d3q27": lt.D3Q27}
DIMS = {"d1q3": 1, "d2q9": 2, "d3q15": 3, "d3q19": 3, "d3q27": 3}

SINGLE = [f"outlet_p_{lat}_{'xyz'[axis]}{side}_r{rho}_{dt}"
          for lat in LATTICES for axis in range(DIMS[lat]) for side in "pm" for rho in (100, 102) for dt in ("f64", "f32")]
SEVERAL = ([f"outlet_p_{what}_{lat}_{dt}" for lat in ("d2q9", "d3q19") for dt in ("f64", "f32") for what in ("three", "mixed")]
           + ["outlet_p_axes_d3q27_f64", "outlet_p_axes_d3q27_f32"])
ROWS = ["outlet_p_row_d3q19_f32", "outlet_p_row_d2q9_f32", "outlet_p_row_d2q9_f64"]
OTHER = ["outlet_p_kbc_d3q27_f64", "outlet_p_smagorinsky_d3q19_f32", "outlet_p_block_d2q9_f64"]
FIXTURES = SINGLE + SEVERAL + ROWS + OTHER


def lattice_of(name):
    return [part for part in name.split("_") if part in LATTICES][0]


def dtype_tag(name):
    return name.rsplit("_", 1)[1]


def collision_kind(g):
    return str(g["collision"])


def make_collision(g):
    tau = float(g["tau"])
    return {"bgk": lt.BGKCollision, "kbc": lt.KBCCollision, "smagorinsky": lt.SmagorinskyCollision}[collision_kind(g)](tau)


def mirror_flow(g, name, context, set_f0=True):
    """the mirror's Obstacle with the fixture's boundaries; str() of the boundaries sorts them into the stored order"""
    res = [int(r) for r in g["resolution"]]
    kinds = [str(k) for k in g["boundary_order"]]
    directions = g["boundary_direction"].tolist()
    rhos = g["rho_outlet"].tolist()
    classes = {"AntiBounceBackOutlet": lt.AntiBounceBackOutlet, "BounceBackBoundary": lt.BounceBackBoundary,
               "EquilibriumBoundaryPU": lt.EquilibriumBoundaryPU, "EquilibriumOutletP": lt.EquilibriumOutletP}

    def ordered(kind, position):
        class Ordered(classes[kind]):
            def __str__(self):
                return f"boundary-{position:03d}"
        return Ordered

    class Carrier(lt.Obstacle):
        made = None

        @property
        def boundaries(self):
            if self.made is None:
                self.made = []
                for position, (kind, direction, rho) in enumerate(zip(kinds, directions, rhos)):
                    cls = ordered(kind, position)
                    if kind == "EquilibriumOutletP":
                        self.made.append(cls(direction, self, rho_outlet=rho))
                    elif kind == "AntiBounceBackOutlet":
                        self.made.append(cls(direction, self))
                    elif kind == "BounceBackBoundary":
                        self.made.append(cls(self.context.convert_to_tensor(g["block_mask"], dtype=torch.bool)))
                    else:
                        self.made.append(cls(self.context, self.context.convert_to_tensor(g["inlet_mask"], dtype=torch.bool),
                                             g["inlet_velocity_pu"].tolist()))
                self.made.reverse()                 # whatever order the flow lists them in, str() decides
            return self.made

    flow = Carrier(context, res, float(g["reynolds"]), float(g["mach"]), float(g["domain_length_x"]),
                   stencil=LATTICES[lattice_of(name)]())
    if set_f0:
        flow.f = context.convert_to_tensor(g["f0"])
    return flow


def plan_entries(g, name):
    """the boundaries of a fixture as entries of lettuce_amd._native.Plan, in the stored order"""
    context = lt.Context("cpu", TORCH_DT[dtype_tag(name)], use_native=False)
    flow = mirror_flow(g, name, context, set_f0=False)
    sim = lt.Simulation(flow, make_collision(g), [])
    assert [type(b).__mro__[1].__name__ for b in sim.boundaries[1:]] == [str(k) for k in g["boundary_order"]]
    return [b.native_generator(i).plan_entry(flow) for i, b in enumerate(sim.boundaries[1:], start=1)]


def fp32_bound(want):
    return 1e-5 * max(1.0, float(np.abs(want).max()))
