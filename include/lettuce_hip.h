/* lettuce_hip.h -- C ABI of the MI355X (gfx950) lattice-Boltzmann stream-and-collide engine.
 *
 * This is the drop-in boundary of the build: a plain-C shared library
 * (liblettuce_hip.so) with raw device pointers and sizes, no torch types.  It
 * takes the place of the module the reference JIT-generates and binds with
 * pybind11 for the same slot:
 *
 *   reference entry point  void collide_and_stream_<hash>(at::Tensor f, at::Tensor f_next
 *                              [, at::Tensor no_collision_mask, at::Tensor no_streaming_mask]
 *                              [, double tau_inv] [, at::Tensor velocityN, at::Tensor densityN ...])
 *                          lettuce/cuda_native/_template.py:58-86 (binding), :297-367 (launcher),
 *                          :175-295 (kernel), :31-44 (python invoke, f/f_next swap)
 *   reference swap point   Simulation._collide_and_stream, lettuce/_simulation.py:92-96,148,202
 *
 * All pointers named *_dev are device pointers (tensor.data_ptr()); buffers are
 * owned by the caller (lettuce/_flow.py:90,124-134) and only borrowed for the
 * call.  Engine-owned scratch (compressed masks, boundary tables, reduction
 * partials) lives in the plan and is released by lt_plan_destroy.  Every launch
 * goes to the caller's HIP stream and returns without synchronising.
 *
 * Memory layout of a population field ("f"): [q][a2][a1][a0], a0 fastest.
 *   LT_LAYOUT_REFERENCE  a0 = last logical axis: f[q][x][y][z] (3-D), f[q][x][y] (2-D)
 *                        -- exactly the reference's C-contiguous tensor (lettuce/_flow.py:90).
 *   LT_LAYOUT_SLAB       3-D only, a0 = x, a2 = z: f[q][z][y][x]; used by the multi-GPU
 *                        z-slab driver so that ghost planes are contiguous.
 * ghost_planes = g (1, or 2 for the two-step slab driver) adds g planes below and g above along
 * a2 (slab exchange); then a2 has shape_a2 + 2 g planes and no periodic wrap is applied along it.
 *
 * Error convention: every function returns LT_OK (0) or a positive LT_ERR_* code
 * and never aborts; lt_last_error() gives the message of the calling thread's
 * last failure (the reference asserts / TORCH_CHECKs: _template.py:53-56,317-323).
 */
#ifndef LETTUCE_HIP_H
#define LETTUCE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LT_ABI_VERSION 2
/* boundaries per plan: the compiled node byte has seven index bits (the reference's uint8 no_collision_mask could
 * name 255, lettuce/_simulation.py:63-86); plans with more than 15 keep the one-step kernels (the two-step kernels
 * with boundaries carry the kinds as two bits per slot in one register) */
#define LT_MAX_BOUNDARIES 127
#define LT_MAX_Q 27

enum lt_status {
  LT_OK = 0,
  LT_ERR_INVALID = 1,      /* bad argument (null pointer, shape, alignment, in == out ...) */
  LT_ERR_UNSUPPORTED = 2,  /* valid request the engine has no kernel for */
  LT_ERR_HIP = 3,          /* a HIP runtime call failed */
  LT_ERR_ALLOC = 4
};

/* lettuce/ext/_stencil/d2q9.py:8-10, d3q19.py:8-13, d3q27.py:8-12, d1q3.py:8-10, d3q15.py:8-13
 * (same velocity order) */
enum lt_stencil { LT_D2Q9 = 0, LT_D3Q19 = 1, LT_D3Q27 = 2, LT_D1Q3 = 3, LT_D3Q15 = 4 };
/* AT_DISPATCH_FLOATING_TYPES, lettuce/cuda_native/_template.py:357 */
enum lt_dtype { LT_F32 = 0, LT_F64 = 1 };
/* lettuce/ext/_collision/no_collision.py:9-17, bgk_collision.py:12-35, kbc_collision.py:11-166,
 * smagorinsky_collision.py:7-36 (every stencil; the constant: lt_plan_set_smagorinsky), trt_collision.py:6-27 (every
 * stencil; `tau` is tau_plus, tau_minus: lt_plan_set_trt), regularized_collision.py:8-44 (every stencil),
 * mrt_collision.py:6-33 (D2Q9 and D3Q27; transform and rates: lt_plan_set_mrt).  4-7 are not
 * collisions: inside the library a body force adds 4 to the plan's value (lt_plan_set_force) */
enum lt_collision {
  LT_COLLISION_NONE = 0, LT_COLLISION_BGK = 1, LT_COLLISION_KBC = 2, LT_COLLISION_SMAGORINSKY = 3,
  LT_COLLISION_TRT = 8, LT_COLLISION_REGULARIZED = 9, LT_COLLISION_MRT = 10
};
/* the moment transforms of an MRT plan (lettuce/util/moments.py:147-274, 369-579): those with an equilibrium of their own */
enum lt_mrt_transform { LT_MRT_D2Q9_DELLAR = 1, LT_MRT_D2Q9_LALLEMAND = 2, LT_MRT_D3Q27_HERMITE = 3 };
/* lettuce/ext/_boundary/bounce_back_boundary.py:10-32, equilibrium_boundary_pu.py:13-46,
 * anti_bounce_back_outlet.py:13-109 */
enum lt_boundary_kind {
  LT_BOUNDARY_BOUNCE_BACK = 1,
  LT_BOUNDARY_EQUILIBRIUM = 2,
  LT_BOUNDARY_ABB_OUTLET = 3,
  /* EquilibriumOutletP (equilibrium_outlet_p.py:12-91): every node of the outlet plane gets feq(rho_outlet, u of the
   * node next to it).  axis, side and flags as for the ABB outlet; one-step kernels only (lt_run keeps them; the
   * entry points with several steps per launch answer LT_ERR_UNSUPPORTED and name the boundary). */
  LT_BOUNDARY_PRESSURE_OUTLET = 4,
  /* Interpolated / half-way bounce-back on a list of links (no counterpart in the reference snapshot; lt_plan_set_links
   * below).  The stepping kernels leave such a node alone -- not collided, streamed -- and a sparse pass over the list
   * follows every collide-only and fused one-step launch.  2-D / 3-D plans in the reference layout without ghost planes;
   * one-step launches over the whole field only.  (6: lt_plan_create keeps answering "unknown boundary kind 5", which
   * callers have been promised.) */
  LT_BOUNDARY_LINK_BOUNCE_BACK = 6
};
enum lt_layout { LT_LAYOUT_REFERENCE = 0, LT_LAYOUT_SLAB = 1 };
/* lettuce/ext/_equilibrium/quadratic_equilibrium.py:11-25 (and quadratic_equilibrium_less_memory.py:14-30, the same
 * arithmetic), incompressible_quadratic_equilibrium.py:10-26 (lt_plan_set_equilibrium; lt_equilibrium is a function) */
enum lt_equilibrium_kind { LT_EQUILIBRIUM_QUADRATIC = 0, LT_EQUILIBRIUM_INCOMPRESSIBLE = 1 };
#define LT_BOUNDARY_ABSENT 1

/* One entry of Simulation.boundaries[1:] (lettuce/_simulation.py:57-58); entry i (0-based)
 * is the boundary whose index in no_collision_mask is i + 1. */
typedef struct lt_boundary_desc {
  int32_t kind;            /* lt_boundary_kind */
  int32_t axis;            /* ABB / pressure outlet: logical axis of `direction` (0 = x) */
  int32_t side;            /* ABB / pressure outlet: +1 or -1 */
  int32_t flags;           /* ABB / pressure outlet on a slab plan (ghost_planes > 0) whose normal is the decomposed axis:
                            * bit 0 (LT_BOUNDARY_ABSENT) = another rank holds the first / last plane of the
                            * global grid, this rank has no outlet; else 0 */
  /* EQUILIBRIUM with uniform velocity/pressure: the populations written on the masked
   * nodes, i.e. feq(rho(p_pu), u_lu(v_pu)) as the host evaluated it in the flow's dtype.
   * PRESSURE OUTLET: feq[0] is rho_outlet (rounded to the plan's dtype when it is uploaded); the struct keeps its
   * size and LT_ABI_VERSION its value.  lt_plan_update_boundary takes a new one between calls. */
  double feq[LT_MAX_Q];
  /* EQUILIBRIUM with per-node velocity/pressure: device pointer to a [q, *res] field of the
   * plan's dtype (borrowed; must outlive the plan or be re-set), or NULL. */
  const void *feq_field_dev;
} lt_boundary_desc;

typedef struct lt_plan_desc {
  int32_t abi_version;     /* LT_ABI_VERSION */
  int32_t stencil;         /* lt_stencil */
  int32_t dtype;           /* lt_dtype */
  int32_t collision;       /* lt_collision */
  int32_t layout;          /* lt_layout */
  int32_t ghost_planes;    /* 0; or 1 / 2 (LT_LAYOUT_SLAB only; 2 for the two-step slab entry points) */
  int32_t dims;            /* 1, 2 or 3; must match the stencil */
  int32_t n_boundaries;    /* 0 .. LT_MAX_BOUNDARIES */
  int64_t shape[3];        /* logical resolution (nx, ny, nz); unused trailing entries = 1.  With ghost
                              planes this is the rank-local slab WITHOUT the ghosts. */
  lt_boundary_desc boundaries[LT_MAX_BOUNDARIES];
} lt_plan_desc;

typedef struct lt_plan lt_plan;

int lt_abi_version(void);
/* 0.  (Bit 0 once meant a build with the kernels that lost their A/B; that build no longer exists.) */
int lt_build_flags(void);
const char *lt_last_error(void);

int lt_plan_create(const lt_plan_desc *desc, lt_plan **out_plan);
int lt_plan_destroy(lt_plan *plan);

/* Compile Simulation.no_collision_mask (uint8 [*res], value = boundary index,
 * lettuce/_simulation.py:73-82) and Simulation.no_streaming_mask (uint8 [q, *res], 0/1,
 * :83-86; may be NULL) into the plan's node-descriptor byte (+ a sparse per-node bit set for
 * the streaming mask).  Both NULL removes the masks.  Required before stepping a plan that
 * has boundaries.  The masks are indexed like the populations of the plan's layout: in the slab
 * layout uint8 [nz + 2][ny][nx] and [q][nz + 2][ny][nx] (ghost-plane entries are ignored). */
int lt_plan_set_masks(lt_plan *plan, const uint8_t *no_collision_mask_dev,
                      const uint8_t *no_streaming_mask_dev, void *stream);

/* Replace boundary i's parameters (e.g. inlet velocity changed between calls; the reference
 * re-reads them every step, cuda_native/ext/_boundary/equilibrium_pu.py:40-48).  The kind cannot
 * change.  The new descriptor is checked as lt_plan_create checks it (outlet axis and side); a
 * refused update leaves the plan unchanged.  When an outlet moves (axis, side or flags) the
 * admission of the masked two-step kernels is decided again for the new outlet, on the masks the
 * last lt_plan_set_masks compiled (its no-streaming bits were those of the old outlet: a plan whose
 * masks no longer match keeps the one-step kernel until lt_plan_set_masks is called with new ones),
 * and the first-use check (lt_plan_set_canary) runs again; so it does when an equilibrium boundary
 * switches between a constant feq and a per-node field. */
int lt_plan_update_boundary(lt_plan *plan, int32_t index, const lt_boundary_desc *desc,
                            void *stream);

/* out = B(C(in)): collision on nodes with no_collision_mask == 0, then the boundaries in
 * index order; no streaming (Simulation._collide, lettuce/_simulation.py:177-189).
 * in != out. */
int lt_collide(lt_plan *plan, const void *f_dev, void *f_out_dev, double tau, void *stream);

/* out = S(in): periodic streaming, destination-side no-streaming mask
 * (Simulation._stream, lettuce/_simulation.py:160-175).  in != out. */
int lt_stream(lt_plan *plan, const void *f_dev, void *f_out_dev, void *stream);

/* out = B(C(S(in))): the fused pull-scheme kernel.  `in` and `out` hold post-collision
 * populations ("f*").  in != out. */
int lt_stream_collide(lt_plan *plan, const void *fstar_dev, void *fstar_out_dev, double tau,
                      void *stream);

/* Same three operators restricted to memory planes [plane_begin, plane_end) of the slowest
 * axis a2 (ghost-plane numbering: 0 is the lower ghost).  Used by the slab driver to do the
 * two boundary planes first and the interior while the halo exchange is in flight. */
int lt_collide_planes(lt_plan *plan, const void *f_dev, void *f_out_dev, double tau,
                      int64_t plane_begin, int64_t plane_end, void *stream);
int lt_stream_planes(lt_plan *plan, const void *f_dev, void *f_out_dev,
                     int64_t plane_begin, int64_t plane_end, void *stream);
int lt_stream_collide_planes(lt_plan *plan, const void *fstar_dev, void *fstar_out_dev,
                             double tau, int64_t plane_begin, int64_t plane_end, void *stream);

/* Fused stream-collide of exactly the two planes `first` < `second` in one launch (the slab's
 * two boundary planes). */
int lt_stream_collide_plane_pair(lt_plan *plan, const void *fstar_dev, void *fstar_out_dev,
                                 double tau, int64_t first, int64_t second, void *stream);

/* As lt_stream_collide_plane_pair, and in the same launch the crossing populations of plane
 * `first` (velocity component -1 along the slowest axis) are packed into pack_first_dev and those
 * of plane `second` (+1) into pack_second_dev, in the layout of lt_slab_pack (first == second is
 * allowed: a one-plane slab). */
int lt_stream_collide_plane_pair_packed(lt_plan *plan, const void *fstar_dev, void *fstar_out_dev,
                                        double tau, int64_t first, int64_t second,
                                        void *pack_first_dev, void *pack_second_dev, void *stream);

/* Halo packing for the slab driver (no reference counterpart: the reference is single-GPU).
 * direction = +1 / -1 selects the populations whose velocity component along the slowest memory
 * axis is +1 / -1 (5 of 19 for D3Q19, 9 of 27 for D3Q27), in ascending q.
 * lt_slab_crossing reports them; lt_slab_pack copies them from memory plane `plane` of f into the
 * contiguous buffer buf[n][n1*n0] (one message per direction instead of n); lt_slab_unpack is the
 * inverse. */
int lt_slab_crossing(lt_plan *plan, int32_t direction, int32_t *q_out, int32_t *n_out);
int lt_slab_pack(lt_plan *plan, const void *f_dev, int64_t plane, int32_t direction, void *buf_dev,
                 void *stream);
int lt_slab_unpack(lt_plan *plan, void *f_dev, int64_t plane, int32_t direction, const void *buf_dev,
                   void *stream);

/* Two-step slabs (ghost_planes = 2 in the plan).  lt_stream_collide_twice_planes is
 * lt_stream_collide_twice for the output planes [begin, end) of a slab: it reads planes
 * [begin - 2, end + 2), so begin >= 2 and end <= n2 - 2.  Before the launch the ghost planes must hold,
 * on the lower side, the in-plane and upward populations of the neighbour's top plane (ghost plane 1)
 * and the upward populations of the plane below that (ghost plane 0); mirrored on the upper side.
 * lt_slab_pack_two_step gathers exactly that message for the neighbour beyond `side` (-1 lower,
 * +1 upper) from this rank's two interior planes next to the cut, as
 *   buf[n_in_plane + 2 n_crossing][n1*n0] = [in-plane of the near plane | crossing of the near
 *   plane | crossing of the far plane]           (9 + 5 + 5 = 19 blocks for D3Q19);
 * lt_slab_unpack_two_step scatters a received message into the two ghost planes beyond `side`.
 * lt_slab_crossing(plan, 0, ...) reports the in-plane populations.
 * Plans with masks (lt_plan_set_masks called) carry one more group of n_crossing blocks: the populations of
 * the near plane that move away from the cut, which a no-streaming node of the ghost plane keeps (24 blocks
 * for D3Q19); lt_slab_two_step_message_blocks reports the count.  With boundaries the two-step launches take
 * bounce-back and equilibrium nodes and one anti-bounce-back outlet whose normal is x (the contiguous axis
 * of the slab layout) opposite an inlet face of equilibrium nodes -- lt_plan_two_step_admitted returns
 * LT_ERR_UNSUPPORTED with the reason otherwise; the fused packing of the entry points below exists for
 * plans without masks only. */
int lt_stream_collide_twice_planes(lt_plan *plan, const void *f_dev, void *out_dev, double tau,
                                   int64_t begin, int64_t end, void *stream);
/* As lt_stream_collide_twice_planes, and in the same launch the halo message for the lower neighbour
 * (pack_lower_dev != NULL; begin must be the first interior plane) and / or for the upper neighbour
 * (pack_upper_dev != NULL; end must be one past the last interior plane) is written in the layout of
 * lt_slab_pack_two_step -- the buffers may be peer-mapped memory of the neighbour. */
int lt_stream_collide_twice_planes_packed(lt_plan *plan, const void *f_dev, void *out_dev, double tau,
                                          int64_t begin, int64_t end, void *pack_lower_dev,
                                          void *pack_upper_dev, void *stream);
/* The two edges of a slab in ONE launch: output planes [2, 2 + edge_planes) and
 * [n2 - 2 - edge_planes, n2 - 2), optionally writing both halo messages (both buffers or neither). */
int lt_stream_collide_twice_edges(lt_plan *plan, const void *f_dev, void *out_dev, double tau,
                                  int32_t edge_planes, void *pack_lower_dev, void *pack_upper_dev,
                                  void *stream);
/* The same edge launch fed straight from the receive buffers: wherever its pull reaches beyond a cut it reads the
 * halo message that arrived from the rank below (recv_lower_dev) / above (recv_upper_dev) -- layout of
 * lt_slab_pack_two_step -- instead of the ghost planes of f_dev, which need not be filled (no
 * lt_slab_unpack_two_step); and it writes both outgoing messages.  With lt_stream_collide_twice_planes for the
 * planes [2 + edge_planes, n2 - 2 - edge_planes), which never reads a ghost plane, a double step of a slab is two
 * launches on one stream and one exchange that starts after the first of them: no pack launch, no unpack launch,
 * no launches competing for the compute units.  Both recv pointers NULL: the ghost planes of f_dev are read (the
 * first double step after a collide pass, whose exchange ended in them).  Plans without masks. */
int lt_stream_collide_twice_edges_direct(lt_plan *plan, const void *f_dev, void *out_dev, double tau,
                                         int32_t edge_planes, const void *recv_lower_dev,
                                         const void *recv_upper_dev, void *pack_lower_dev, void *pack_upper_dev,
                                         void *stream);
/* The whole slab -- output planes [2, n2 - 2) -- in ONE launch that releases the exchange while it runs (plans
 * without masks).  The workgroups that produce the two planes next to each cut start first; each adds 1 to a
 * counter of the plan when those planes are in memory.  lt_slab_wait_edges enqueues, on ANOTHER stream, one
 * polling wave that returns when the counter has reached the value that completes the edges of the last such
 * launch -- work enqueued behind it (lt_slab_pack_two_step, the transfers, lt_slab_unpack_two_step) then runs
 * beside the rest of the sweep -- or after about one second (lt_slab_wait_timed_out then reports 1; it
 * synchronises the stream).  Replaces two edge launches + one interior launch: no planes are computed twice at
 * the lower cut, the upper edge costs its prologue only once, and three launches do not compete for the CUs. */
int lt_stream_collide_twice_slab(lt_plan *plan, const void *f_dev, void *out_dev, double tau, void *stream);
int lt_slab_wait_edges(lt_plan *plan, void *stream);
int lt_slab_wait_timed_out(lt_plan *plan, int32_t *timed_out, void *stream);
int lt_slab_two_step_message_blocks(lt_plan *plan, int32_t *blocks_out);
/* LT_OK when lt_stream_collide_twice / _planes has a kernel for this plan as it stands (lattice, dtype,
 * collision, grid extents, masks); LT_ERR_UNSUPPORTED (and the reason in lt_last_error) otherwise. */
int lt_plan_two_step_admitted(lt_plan *plan);
/* Descriptor-only query (no device, no plan): the tile of the two-step kernels for this stencil / dtype
 * (tile_width x tile_rows nodes; rows = 0: no kernel) and whether a field of these extents stays within the
 * kernels' 32-bit byte offsets (masked != 0: the whole field, q * nodes * sizeof(scalar) < 4 GiB; else one plane).
 * lt_run / lt_plan_two_step_admitted apply the same rule, so a plan beyond it keeps the one-step kernel. */
int lt_two_step_limits(const lt_plan_desc *desc, int32_t masked, int32_t *tile_width, int32_t *tile_rows,
                       int32_t *addressable);
int lt_slab_pack_two_step(lt_plan *plan, const void *f_dev, int32_t side, void *buf_dev, void *stream);
int lt_slab_unpack_two_step(lt_plan *plan, void *f_dev, int32_t side, const void *buf_dev, void *stream);

/* n whole lettuce steps (collide, boundaries, stream) starting from post-streaming
 * populations in buf_a (lettuce/_simulation.py:201-203): one collide launch, n-1 fused
 * launches, one stream launch, ping-ponging between the two buffers.  On return
 * *result_in_b tells which buffer holds the new post-streaming populations (1 = buf_b);
 * the other buffer then holds the post-collision populations of the last step, from which
 * lt_continue can carry on without the extra collide pass. */
int lt_run(lt_plan *plan, void *buf_a_dev, void *buf_b_dev, double tau, int64_t n_steps,
           void *stream, int32_t *result_in_b);
/* As lt_run, but buf_a holds post-collision populations f* of the step before (what lt_run
 * leaves in the non-result buffer): n fused launches + one stream launch. */
int lt_continue(lt_plan *plan, void *fstar_a_dev, void *buf_b_dev, double tau, int64_t n_steps,
                void *stream, int32_t *result_in_b);
/* on != 0: lt_run / lt_continue stop before their last (streaming) launch: *result_in_b then tells which
 * buffer holds the POST-COLLISION populations of the last step, the other buffer is scratch; lt_stream of
 * that buffer gives the post-streaming populations whenever somebody wants to see them, and lt_continue
 * carries on from it without them.  A caller that advances in batches and looks at the populations only
 * now and then (lettuce's Simulation with reporters every k steps) saves one pass over memory per batch. */
int lt_plan_set_deferred_stream(lt_plan *plan, int32_t on);

/* rho [*res] and u [d, *res] (either may be NULL) from post-streaming populations
 * (Flow.rho / Flow.j / Flow.u, lettuce/_flow.py:136-138,152-172). */
int lt_macroscopic(lt_plan *plan, const void *f_dev, void *rho_dev, void *u_dev, void *stream);

/* feq [q, *res] from rho [*res] and u [d, *res]
 * (QuadraticEquilibrium.__call__, lettuce/ext/_equilibrium/quadratic_equilibrium.py:11-25; the plan's equilibrium:
 * lt_plan_set_equilibrium). */
int lt_equilibrium(lt_plan *plan, const void *rho_dev, const void *u_dev, void *feq_dev,
                   void *stream);

/* *out_dev (one double, device memory) = sum over nodes of 0.5 * u.u in lattice units,
 * accumulated in fp64 with a fixed reduction order (Flow.incompressible_energy summed as in
 * IncompressibleKineticEnergy, lettuce/_flow.py:178-181,
 * lettuce/ext/_reporter/observable_reporter.py:34-42; the pu scaling stays on the host).
 * Ghost planes are excluded. */
int lt_kinetic_energy(lt_plan *plan, const void *f_dev, double *out_dev, void *stream);

/* *out_dev = sum over nodes and populations of f (total mass, fp64 accumulation). */
int lt_mass(lt_plan *plan, const void *f_dev, double *out_dev, void *stream);

/* *out_dev = max over nodes of |u| in lattice units (MaximumVelocity observable,
 * lettuce/ext/_reporter/observable_reporter.py:27-31; the pu scaling stays on the host).  The maximum
 * propagates NaN as torch.max does: if |u| of any node is NaN (a diverged run) the result is NaN, not the
 * largest finite value.  Ghost planes are excluded. */
int lt_max_velocity(lt_plan *plan, const void *f_dev, double *out_dev, void *stream);

/* Non-equilibrium initialisation (lettuce/_flow.py:309-336, Krueger et al. 2017): f_dev [q][N] =
 * feq(rho, u) - w_q Pi1:Q_q with Pi1_ab = tau rho d_b u_a / cs^2 from the 6th-order periodic central
 * differences of torch_gradient (util/utility.py:37-99, dx = 1) and Q_q,ab = e_qa e_qb - identity_cs2
 * delta_ab.  identity_cs2 is passed by the caller because the reference builds the identity in torch's
 * DEFAULT dtype (an fp32-rounded cs^2 even in an fp64 run, _flow.py:328-330).  rho_dev [N] and u_dev
 * [d][N] (lattice units, logical component order) are the moments of the equilibrium populations, as
 * Flow.rho() / Flow.u() give them; one launch, nothing else is materialised (the reference builds
 * [d][d][N] gradients, Pi1 and two [q][N] fields).  Reference layout, periodic along every axis: the
 * shifted indices wrap modulo the extent like torch.roll, for every extent >= 1 (with an extent of 1 or 2 the
 * six taps alias the same one or two nodes). */
int lt_init_fneq(lt_plan *plan, const void *rho_dev, const void *u_dev, double tau, double identity_cs2,
                 void *f_dev, void *stream);

/* Enstrophy observable (lettuce/ext/_reporter/observable_reporter.py:45-68): *out_dev = sum over nodes
 * of |curl(u_scale * u)|^2 with the 6th-order periodic central differences of torch_gradient
 * (lettuce/util/utility.py:37-99; weights -1/60, 3/20, -3/4, 3/4, -3/20, 1/60 times inv_dx), evaluated
 * per node in the working dtype as the reference's whole-field expression and accumulated in fp64
 * with a fixed reduction order; the factor dx^d stays on the host.  Two launches: u [d][N] into
 * u_scratch_dev (d * N scalars of the plan's dtype, caller-owned), then the stencil reduction over
 * it.  2-D / 3-D, reference layout, periodic domains only (as the reference).  The shifted indices wrap
 * modulo the extent like torch.roll, for every extent >= 1. */
int lt_enstrophy(lt_plan *plan, const void *f_dev, void *u_scratch_dev, double u_scale, double inv_dx,
                 double *out_dev, void *stream);

/* Mass observable (observable_reporter.py:140-158): *out_dev = sum over all populations of the nodes
 * that are not on the first / last index of the two fastest axes (the reference's f[..., 1:-1, 1:-1])
 * minus, if no_mass_mask_dev (uint8 [N], 0 / 1) is given, sum_q f over the nodes it flags (borders
 * included, as in the reference).  fp64 accumulation.  2-D / 3-D, reference layout. */
int lt_mass_interior(lt_plan *plan, const void *f_dev, const uint8_t *no_mass_mask_dev, double *out_dev,
                     void *stream);

/* The same two observables for one rank of the z-slab decomposition (plans with LT_LAYOUT_SLAB and
 * ghost planes), so that a slab reporter needs no gather (observable_reporter.py:45-68, 140-158):
 *  lt_slab_velocity   u_ext_dev [3][nz + 6][ny][nx] (nz = the rank's own planes, logical component order, lattice
 *                     units) <- u of the plan's nz + 2 g planes, written at planes [3 - g, 3 + nz + g); the caller
 *                     then fills planes [0, 3) and [nz + 3, nz + 6) with the neighbours' planes (6th-order
 *                     differences reach three planes: a velocity halo exchange, host side);
 *  lt_slab_enstrophy  *out_dev = sum over the rank's own nodes of |curl(u_scale * u)|^2, as lt_enstrophy (x and y
 *                     wrap modulo nx / ny >= 1; nothing wraps along z, where the neighbours' planes are read);
 *  lt_slab_mass_interior  *out_dev = the rank's share of lt_mass_interior: own planes only, y and the GLOBAL z index
 *                     (z_begin + local plane, of nz_global) off their first / last value; no_mass_mask_dev is uint8 per
 *                     node of the plan (ghost planes included, as f) or null.
 * The caller sums the ranks' results (all-reduce). */
int lt_slab_velocity(lt_plan *plan, const void *f_dev, void *u_ext_dev, void *stream);
int lt_slab_enstrophy(lt_plan *plan, const void *u_ext_dev, double u_scale, double inv_dx, double *out_dev,
                      void *stream);
int lt_slab_mass_interior(lt_plan *plan, const void *f_dev, const uint8_t *no_mass_mask_dev, int32_t z_begin,
                          int32_t nz_global, double *out_dev, void *stream);

/* EnergySpectrum observable (lettuce/ext/_reporter/observable_reporter.py:71-108) without its [*res, K] wave mask:
 *   out_dev[n] = scale * sum over the modes of bin n of sum_a 0.5 * (re_a^2 + im_a^2),  n < n_bins.
 * uhat_dev holds the d complex fields [d][*res] of the plan's grid, interleaved (re, im), in the plan's dtype: the full
 * transform of the velocity field (torch.view_as_real(torch.fft.fftn(u, dim = <the last d axes>))), every mode counted
 * as the reference counts it.  Index i on an axis of extent n has the integer wavenumber k = i < (n + 1) / 2 ? i : i - n
 * (np.fft.fftfreq(n, d = 1 / n), odd n too; each axis in its own extent).  With m = sum_a k_a^2 the bin of a mode is 0
 * for m = 0 and else the n >= 1 with n^2 - n < m <= n^2 + n: the reference's n - 0.5 < |k| <= n + 0.5, squared and so
 * decided in integers.  The reference has n_bins = isqrt(max m) (its int(max |k|)); modes whose bin is >= n_bins are
 * dropped, as the reference drops them.  Squares and sums are fp64 from the first operation (fp32 inputs promote
 * exactly); scale (1 / norm^2) is applied once per bin.
 * Fixed summation order, no floating-point atomics: the first launch has ceil(N / chunk) <= LT_SPECTRUM_BLOCKS
 * workgroups, each over a contiguous range of `chunk` modes (N / LT_SPECTRUM_BLOCKS rounded up to whole passes of 256,
 * 1024 modes or more) with a table of bins per wave in LDS, and writes partial_scratch_dev [workgroups][n_bins]; the second sums the
 * workgroups in index order.  Two calls on the same input give the same bits.  partial_scratch_dev is caller-owned:
 * LT_SPECTRUM_BLOCKS * n_bins doubles always suffice.  out_dev: n_bins doubles.
 * LT_ERR_UNSUPPORTED: 1-D plans, the slab layout or ghost planes, n_bins > LT_SPECTRUM_MAX_BINS (four tables of doubles
 * in 64 KiB of LDS; 768^3 has 665 bins).  LT_ERR_INVALID: a null pointer, n_bins < 1. */
#define LT_SPECTRUM_BLOCKS 1024
#define LT_SPECTRUM_MAX_BINS 2048
int lt_energy_spectrum(lt_plan *plan, const void *uhat_dev, double scale, int32_t n_bins, double *partial_scratch_dev,
                       double *out_dev, void *stream);

/* Momentum-exchange force of the fluid on a body of full-way bounce-back nodes (no counterpart in the reference
 * snapshot), per time step, in lattice units:
 *   out_dev[c] = sum over x_s with solid[x_s] of sum over q >= 1 with not solid[x_s - e_q] of 2 e_{q,c} f_q(x_s),
 * c = 0 .. d - 1 in logical axis order; out_dev[c] = 0 for d <= c < 3.  f_dev: the populations after streaming, dense
 * [q][N] in the plan's dtype (the caller's own buffer: resident populations are stored into it first).  solid_dev: one
 * byte per node [N], nonzero = solid.  f_q(x_s) arrived from x_s - e_q and, swapped at collision time, leaves again
 * along -e_q in the same step; x_s - e_q wraps periodically on every axis, as streaming wraps it (extents 1 and 2
 * included), nodes of other boundaries count as not solid, links between two solid nodes carry nothing.  A sphere in
 * a +x stream has out_dev[0] > 0.
 * A fluid node costs its one byte; a solid node the bytes of its q - 1 neighbours and, unless all of them are solid,
 * f_q of its fluid links and its own f_0 (read in place of the others and dropped).
 * fp64 from the first operation (2 f_q and the sign are exact).  Fixed summation order, no floating-point atomics: the
 * first launch has min(ceil(N / 256), LT_BOUNDARY_FORCE_BLOCKS) workgroups striding the nodes and writes
 * partial_scratch_dev [3][workgroups]; the second, one workgroup, adds them in index order and writes all three
 * outputs, exact 0.0 where nothing is solid.  Two calls on the same input give the same bits.  partial_scratch_dev is
 * caller-owned: 3 * LT_BOUNDARY_FORCE_BLOCKS doubles always suffice.  out_dev: 3 doubles.
 * LT_ERR_UNSUPPORTED: 1-D plans, the slab layout or ghost planes, a plan with a population stride (f_dev is dense).
 * LT_ERR_INVALID: a null pointer, before any HIP call. */
#define LT_BOUNDARY_FORCE_BLOCKS 1024
int lt_boundary_force(lt_plan *plan, const void *f_dev, const uint8_t *solid_dev, double *partial_scratch_dev,
                      double *out_dev, void *stream);

/* Link bounce-back (LT_BOUNDARY_LINK_BOUNCE_BACK): linear interpolated bounce-back after Bouzidi, Firdaouss and
 * Lallemand (2001), half-way bounce-back being its case d = 1/2.  A link is (r, x_s): x_s a node of the boundary, r >= 1
 * a direction whose neighbour x_f = x_s + e_r is a fluid node; q = opposite(r), x_ff = x_f + e_r; neighbours wrap
 * periodically on every axis, as streaming wraps them.  On the post-collision populations the pass writes
 *   f_r(x_s) = c1 * A + c2 * B,   A = f_q(x_f),   B = second_source ? f_r(x_f) : f_q(x_ff)
 * -- two products and one sum in the plan's dtype, each rounded on its own -- and streaming then carries the slot to
 * (r, x_f).  Only fluid nodes are read, only slots of the boundary's nodes written, every slot by one link.
 *
 * lt_plan_set_links gives boundary `boundary_index` (0-based, as for lt_plan_update_boundary) its list: n_links entries
 * in HOST memory, sorted by node, then by direction, no entry twice; nodes[i] the index of x_s within a population
 * (C order of the grid), directions[i] = r in 1 .. q - 1, c1 / c2 in the plan's dtype, second_source[i] 0 or 1.  The
 * list is copied into plan-owned device memory (the call returns when the copy is done; lt_plan_destroy frees it),
 * n_links = 0 is legal and launches nothing, a second call replaces the list.  LT_ERR_INVALID: a boundary of another
 * kind, a null array, a node or direction out of range, a list out of order.
 *
 * After lt_plan_set_links every collide-only and fused one-step launch of the plan (lt_collide, lt_stream_collide,
 * lt_run, lt_continue, the resident buffers, a captured graph) is followed, on the same stream, by the pass over each
 * list on the launch's output with its population stride; lt_stream alone gets nothing.  LT_ERR_UNSUPPORTED, each by
 * name ("... per launch with link bounce-back"): two-step and many-step launches (lt_run keeps one update per
 * launch, lt_plan_set_two_step / lt_plan_set_many_step(plan, 1) are refused), launches over a range of planes; at
 * lt_plan_create: 1-D plans, the slab layout, ghost planes.  LT_ERR_INVALID: a launch before every such boundary has
 * its list.
 *
 * lt_apply_links: the pass alone, in place on f_dev (the plan's population stride).
 * lt_link_force: the momentum-exchange force over the list of one boundary, on POST-STREAMING populations,
 *   out_dev[c] = sum over the links of e_{q,c} * (f_q(x_s) + f_r(x_f)),   c in logical axis order, 0 beyond d
 * -- f_q(x_s) left the fluid along the link, f_r(x_f) came back; for d = 1/2 both are equal and this is
 * lt_boundary_force.  fp64, fixed summation order, no atomics: min(ceil(n_links / 256), LT_LINK_FORCE_BLOCKS) workgroups
 * write partial_scratch_dev [3][workgroups] (3 * LT_LINK_FORCE_BLOCKS doubles always suffice), one workgroup adds them in
 * index order.  Two calls on the same input give the same bits; an empty list gives exact zeros. */
#define LT_LINK_FORCE_BLOCKS 1024
int lt_plan_set_links(lt_plan *plan, int32_t boundary_index, int64_t n_links, const int32_t *nodes,
                      const uint8_t *directions, const void *c1, const void *c2, const uint8_t *second_source,
                      void *stream);
int lt_apply_links(lt_plan *plan, void *f_dev, void *stream);
int lt_link_force(lt_plan *plan, int32_t boundary_index, const void *f_dev, double *partial_scratch_dev, double *out_dev,
                  void *stream);

/* Jacobi solver of the periodic pressure-Poisson equation lap(p) = rhs (lettuce/util/utility.py:119-156, torch_jacobi),
 * without a plan: the fields are dense [shape[0]][shape[1]]([shape[2]]) arrays of `dtype` in C order (the last axis
 * fastest), dims = 2 or 3, every extent >= 1 (extent 1: a node is its own neighbour, extent 2: both neighbours are the
 * same node, as torch.roll has it).  One sweep, with S the sum of the 2 dims neighbours of p in the reference's order
 * (axis 0 -, axis 1 -, [axis 2 -,] axis 0 +, axis 1 +, [axis 2 +]) and dx2 = (dtype)(dx * dx):
 *   p_next = (rhs * dx2 - S) * (-1) / (2 dims)          r = rhs - (S - (2 dims) * p) / dx2
 * operation for operation in dtype, no contraction, true divisions; the error of an iterate is mean(r^2), r widened to
 * fp64, summed in a fixed order (at most LT_JACOBI_BLOCKS workgroup partials, then one workgroup) without atomics: two
 * calls on the same input give the same bits.  Sweep s + 1 is the one that forms the error of iterate s; a one-workgroup
 * launch after it holds the error against tol_abs ON THE DEVICE and raises a done flag in work_dev, which every later
 * sweep reads first and then returns without writing.  The host enqueues `batch` sweeps at a time (0: LT_JACOBI_BATCH)
 * and reads the flag once per batch: no synchronisation per sweep.  Stopping rule, the reference's: after iteration `it`
 * when !(error_it > tol_abs) (a NaN error stops) or it == max_num_steps; max_num_steps = 0 returns p unchanged (error
 * 1, the reference's starting value).  p_dev holds the iterate `it` on return (p is ping-ponged with p_scratch_dev, a
 * buffer of p's size; rhs_dev is only read), *iterations_out = it and *error_out = error_it (either may be null).  The
 * call returns after the stream has drained.  work_dev: LT_JACOBI_WORK_BYTES caller-owned bytes, 8-byte aligned.
 * LT_ERR_INVALID, before any HIP call: a null pointer, dims outside 2-3, an extent < 1 (or more than 2^40 nodes), an
 * unknown dtype, max_num_steps < 0, batch < 0. */
#define LT_JACOBI_BLOCKS 1024
#define LT_JACOBI_BATCH 64
#define LT_JACOBI_WORK_BYTES ((LT_JACOBI_BLOCKS + 4) * 8)
int lt_jacobi(void *p_dev, void *p_scratch_dev, const void *rhs_dev, int32_t dtype, int32_t dims, const int64_t *shape,
              double dx, double tol_abs, int64_t max_num_steps, int32_t batch, void *work_dev, int64_t *iterations_out,
              double *error_out, void *stream);

/* Introspection for tests and benchmarks. */
int lt_plan_kernel_info(lt_plan *plan, int32_t *vec_width, int32_t *threads_per_block,
                        int64_t *blocks_per_launch);
/* Name of the fused kernel variant this plan launches (for matching rocprof rows). */
const char *lt_plan_kernel_name(lt_plan *plan);
/* A/B selector of the two-step kernel's workgroup order: 0 = product variant, 3 = no XCD-aware renumbering of the
 * workgroups, 4 = the round-1 renumbering (an eighth of the grid per XCD instead of an eighth of every segment
 * layer).  1, 2 and 5 named tile variants that lost their A/B and were removed (two nodes per thread in both phases,
 * two output nodes per thread, 32 x 8 tiles for the slab edge launch): LT_ERR_UNSUPPORTED.
 * 6 = the one-role schedule (every wave runs both phases of the sweep) for the sweeps that by default run with
 * separate producer and consumer waves -- D3Q19 BGK fp32, both layouts; no effect on the other kernels. */
int lt_plan_set_shift_policy(lt_plan *plan, int32_t policy);
/* out[i] = x[i] / D as the kernels' equilibrium forms it (div_cs: two or three instructions that return the IEEE
 * quotient by the constant D = 2 cs^2 (which 0) or cs^2 (which 1) rounded to dtype, the reference's divisors:
 * lettuce/ext/_equilibrium/quadratic_equilibrium.py:15-24) -- a test hook that pins the emulation on the device. */
int lt_probe_div_cs(const void *x_dev, void *out_dev, int64_t n, int32_t dtype, int32_t which, void *stream);
/* Diagnostic: dst[0:n_bytes] = src[0:n_bytes] with 16-byte accesses and the cache-policy bits of
 * lt_plan_set_tuning; max_blocks > 0 caps its grid (grid-stride loop).  bench.py uses it to
 * measure this device's copy ceiling. */
int lt_probe_copy(void *dst_dev, const void *src_dev, int64_t n_bytes, int32_t cache_policy,
                  int32_t max_blocks, void *stream);
/* hipGraph replay inside lt_run / lt_continue: the fused launches are captured 32 at a time into a
 * graph and replayed.  mode 1 = always, 0 = never, -1 = automatic, which is "never" at present:
 * on MI355X the eager launch loop was as fast or faster on small grids (3.5 vs 4.1 us per step at
 * 128^2), see DESIGN.md. */
int lt_plan_set_graph_mode(lt_plan *plan, int32_t mode);
/* Tuning knobs.  cache_policy: -1 = automatic (nontemporal accesses when the populations exceed
 * the caches), else bit 0 = nontemporal loads, bit 1 = nontemporal stores (the one-node-per-
 * thread kernels exist for 0 and 3).
 * wide != 0 asked for the 16-byte-per-lane variant of the hot kernel, which lost its A/B (8-13 % slower) and
 * was removed: LT_ERR_UNSUPPORTED. */
int lt_plan_set_tuning(lt_plan *plan, int32_t cache_policy, int32_t wide);
/* Two fused steps in one launch: out = (C S)^2 f for the whole periodic grid, the intermediate
 * state staged through LDS (one HBM read and one write of the populations per two lattice updates).
 * Bit-identical to two lt_stream_collide calls.  Exists with BGK / no collision for the 3-D lattices
 * (D3Q15 and D3Q19 in fp32 and fp64, D3Q27 in fp32) on grids whose contiguous extent is a multiple
 * of 64 (fp32) / 32 (fp64) and whose middle extent is a multiple of 8 (D3Q27: of 4), for D2Q9 (fp32 and
 * fp64) on grids whose contiguous extent is a multiple of 64, and -- D2Q9; 3-D in fp32 and D3Q15 fp64 -- for
 * plans with bounce-back / equilibrium boundaries and at most one anti-bounce-back outlet: at the last plane
 * (2-D: row) of the slowest memory axis or, in 3-D, at an end of the contiguous axis opposite a face of
 * equilibrium nodes (no-streaming bits exactly that outlet's); LT_ERR_UNSUPPORTED otherwise
 * (lt_plan_two_step_admitted tells). */
int lt_stream_collide_twice(lt_plan *plan, const void *f_dev, void *out_dev, double tau, void *stream);
/* Small 2-D grids (launch-bound): n_steps <= 8 stream-collide steps in one launch.  Every workgroup
 * keeps the neighbourhood of its 8 x 8 tile in LDS and recomputes the halo, so the launch does
 * redundant arithmetic but replaces n_steps launches; bit-identical to n_steps lt_stream_collide
 * calls.  2-D lattices, extents multiples of 8; plans with masks too (bounce-back, equilibrium and at most
 * one anti-bounce-back outlet, for which one more ring of nodes is recomputed: n_steps <= 7);
 * LT_ERR_UNSUPPORTED otherwise, 3-D plans included (a two-step 3-D variant measured slower than two launches and
 * was removed).
 * lt_plan_set_many_step: lt_run / lt_continue use it for their fused steps: -1 = automatic (2-D grids up
 * to 256 x 256 nodes, with masks up to 256 x 128; BGK / no collision, where it is bit-identical to the one-step
 * kernel; never for 3-D grids, where two steps per launch measured slower than two launches), 0 = never,
 * 1 = whenever supported. */
int lt_stream_collide_many(lt_plan *plan, const void *f_dev, void *out_dev, double tau, int32_t n_steps,
                           void *stream);
int lt_plan_set_many_step(lt_plan *plan, int32_t mode);
/* lt_run / lt_continue pair their fused steps with lt_stream_collide_twice where it exists:
 * mode -1 = automatic, 0 = never, 1 = whenever supported.  planes_per_workgroup: segment length of
 * the sweep along the slowest axis (0 = automatic). */
int lt_plan_set_two_step(lt_plan *plan, int32_t mode, int32_t planes_per_workgroup);
/* The constant C of a plan with LT_COLLISION_SMAGORINSKY (nu_t = C^2 S:S after two fixed-point iterations,
 * smagorinsky_collision.py:27-34); 0.17, the reference's default, until set.  Read at every launch, so it may change
 * between calls like tau.  LT_ERR_INVALID (plan unchanged) for a negative or non-finite value and on a plan of
 * another collision.  Two steps per launch exist for D3Q19 fp32 on periodic plans without masks: lt_run's automatic
 * mode takes them in the streaming regime as it does for BGK, lt_plan_set_two_step(plan, 1, ...) wherever the grid
 * tiles; every other plan keeps the one-step kernel (lt_plan_two_step_admitted tells why). */
int lt_plan_set_smagorinsky(lt_plan *plan, double constant);
/* tau_minus of a plan with LT_COLLISION_TRT, the relaxation time of the antisymmetric part of f - feq over an opposite
 * pair (trt_collision.py:23-25); the symmetric part relaxes with the `tau` of every call (tau_plus).  1.0, the
 * reference's default, until set.  Read at every launch, so it may change between calls like tau.  LT_ERR_INVALID (plan
 * unchanged) for a non-positive or non-finite value, on a plan of another collision and for a null plan.
 * LT_COLLISION_TRT and LT_COLLISION_REGULARIZED have every one-step kernel BGK has (masks, both layouts, packed plane
 * launches, up to three outlets) and no body force (lt_plan_set_force: LT_ERR_UNSUPPORTED, as on KBC).  Two steps per
 * launch exist for D3Q19 fp32 on periodic plans without masks (the plain sweep, both layouts), taken with
 * lt_plan_set_two_step(plan, 1, ...) only -- never by the automatic mode.  On every other plan lt_run, lt_continue and
 * lt_resident_advance keep the one-step kernel; the explicit multi-step entry points and lt_plan_two_step_admitted
 * return LT_ERR_UNSUPPORTED with a reason that names the collision. */
int lt_plan_set_trt(lt_plan *plan, double tau_minus);
/* Transform and relaxation rates of a plan with LT_COLLISION_MRT: m = M f, m_i <- m_i - (1 / relaxation[i]) (m_i -
 * meq_i(m)), f = M^-1 m, with M and meq of `transform` (lt_mrt_transform) and `count` = q rates in the order of the
 * transform's moments.  The plan rounds each rate to its scalar type and forms the reciprocal there, as the reference
 * does on every call (mrt_collision.py:18-24); the rates of the conserved moments (rho, j) are checked and not used.
 * Read at every launch, so both may change between calls.  The `tau` argument of lt_run, lt_collide and the other entry
 * points is NOT read by an MRT plan.  LT_ERR_INVALID (plan unchanged) on a plan of another collision, for a transform
 * of the other lattice, count != q, a null pointer and a rate that is not finite and > 0; a run or collide of an MRT
 * plan before the first successful call returns LT_ERR_INVALID as well.  lt_plan_create answers LT_ERR_UNSUPPORTED for
 * LT_COLLISION_MRT on a lattice other than D2Q9 / D3Q27.  MRT has every one-step kernel BGK has (masks, both layouts,
 * packed plane launches, up to three outlets, the constant-pressure outlet), no body force and no launch of several
 * steps: lt_run, lt_continue and lt_resident_advance keep one update per launch, lt_plan_set_two_step(plan, 1, ...),
 * the explicit multi-step entry points and lt_plan_two_step_admitted return LT_ERR_UNSUPPORTED with a reason that
 * names the collision. */
int lt_plan_set_mrt(lt_plan *plan, int transform, const double *relaxation, int count);
/* A uniform body force on a plan with LT_COLLISION_BGK or LT_COLLISION_SMAGORINSKY.  acceleration: `dims` values in
 * lattice units, logical order x, y, z.  A colliding node (no_collision_mask == 0) then does
 *   u*   = j / rho + (ueq_scale * a) / rho
 *   f'_q = f_q - (1 / tau_eff) (f_q - feq_q(rho, u*))
 *          + source_scale * w_q * sum_c [ (e_qc - u*_c) / cs^2 + (e_q . u*) e_qc / cs^4 ] a_c
 * with tau_eff = tau for BGK (bgk_collision.py:17-22) and, for Smagorinsky, the relaxation time formed from
 * f - feq(rho, u*) (smagorinsky_collision.py:19-36); boundary nodes are untouched.  Guo's scheme (lettuce/ext/_force/
 * guo.py:14-31) is ueq_scale = 0.5, source_scale = 1 - 1 / (2 force.tau); Shan-Chen's (shan_chen.py:14-25) is
 * ueq_scale = force.tau, source_scale = 0.  Read at every launch, so it may change between calls like tau.
 * acceleration == NULL removes the force: the plan then launches exactly what a plan that never had one launches.  A
 * zero vector is still a forced plan (its own kernels, same result up to rounding).  LT_ERR_INVALID for a non-finite
 * value, LT_ERR_UNSUPPORTED on a plan whose collision is none or KBC; a refused call leaves the plan unchanged.
 * Every one-step variant exists with the force (all lattices, dtypes, layouts, mask variants, the plane launches of a
 * slab with one ghost plane); two steps per launch exist for BGK on D3Q19 fp32, periodic plans without masks, and are
 * taken with lt_plan_set_two_step(plan, 1, ...) only -- never by the automatic mode.  On every other plan lt_run,
 * lt_continue and lt_resident_advance keep the one-step kernel; the explicit multi-step entry points and
 * lt_plan_two_step_admitted return LT_ERR_UNSUPPORTED with a reason that names the force. */
int lt_plan_set_force(lt_plan *plan, const double *acceleration /* dims values, or NULL */, double ueq_scale,
                      double source_scale);
/* The same body force with an acceleration that varies in space: `acceleration` is a DEVICE pointer to dense
 * [dims][nodes] values in the plan's dtype, lattice units, logical axis order x, y, z, the nodes in the reference's
 * order (the order of a population).  The formulas are those of lt_plan_set_force with a = a(x), the node's own value;
 * the shift ueq_scale * a(x) is formed in the plan's dtype, as the uniform call forms it on the host, so a field that
 * is constant in space gives the uniform force's populations bit for bit.  The kernels read the memory at EVERY launch:
 * it must stay allocated while the plan may launch, the caller may rewrite it between launches (ordered on the launch
 * stream), and its VALUES ARE NOT VALIDATED -- the function checks what the host can check: a non-null plan, finite
 * scales (LT_ERR_INVALID), the plan's collision (BGK and Smagorinsky; else LT_ERR_UNSUPPORTED).  acceleration == NULL
 * removes the field.  lt_plan_set_force and lt_plan_set_force_field exclude each other: the later call wins.  A changed
 * pointer is a changed setting (a captured graph is dropped).
 * The field has the one-step kernels of the reference layout (kernels' COLL 37 and 39): every lattice and dtype, fused
 * and collide-only (lt_collide takes the latter), with or without masks -- bounce-back, equilibrium boundaries (table
 * and per-node) and link bounce-back are supported; a boundary node does not read the field.  LT_ERR_UNSUPPORTED, with
 * a message that names the pair and the plan unchanged, at the call that first knows both: a slab-layout plan or ghost
 * planes; an anti-bounce-back or constant-pressure outlet in the plan; the incompressible equilibrium
 * (lt_plan_set_equilibrium refuses in turn on a plan with a field); lt_plan_set_two_step(plan, 1, ...) and
 * lt_plan_set_many_step(plan, 1) before or after it.  lt_run, lt_continue and lt_resident_advance keep one update per
 * launch; the explicit multi-step entry points and lt_plan_two_step_admitted return LT_ERR_UNSUPPORTED. */
int lt_plan_set_force_field(lt_plan *plan, const void *acceleration /* device, [dims][nodes], or NULL */,
                            double ueq_scale, double source_scale);
/* The equilibrium of the plan, lt_equilibrium_kind: LT_EQUILIBRIUM_QUADRATIC (what every plan has until this is called;
 * rho0 is not read) or LT_EQUILIBRIUM_INCOMPRESSIBLE,
 *   feq_q = w_q (rho + rho0 ((2 e_q.u - u.u) / (2 cs^2) + (e_q.u / cs^2)^2 / 2)),   u = j / rho
 * (incompressible_quadratic_equilibrium.py:14-26; rho0 is rounded to the plan's scalar type once).  Kind and rho0 are
 * read at every launch, so they may change between calls like tau: lt_collide, lt_stream_collide, lt_run, lt_continue
 * (one update per launch), lt_equilibrium and lt_init_fneq evaluate this equilibrium.  The boundaries' populations
 * (lt_boundary_desc.feq) are the caller's, whatever the kind.  A plan that never called this, or set kind 0, launches
 * exactly what it launched before.  Kind 1 has the one-step kernels of no collision, BGK (with or without
 * lt_plan_set_force), TRT and the regularised collision, every lattice and dtype, reference layout, with or without masks
 * (bounce-back, equilibrium boundaries, anti-bounce-back outlets).  Refused, with the plan unchanged:
 * LT_ERR_INVALID for an unknown kind, a non-finite rho0 and a null plan; LT_ERR_UNSUPPORTED for kind 1 on a plan with
 * KBC, Smagorinsky or MRT, on a slab-layout plan and on a plan with a constant-pressure outlet.  A kind-1 plan has no launch of several steps: lt_run, lt_continue and lt_resident_advance
 * keep one update per launch; lt_plan_set_two_step(plan, 1, ...), lt_plan_set_many_step(plan, 1), the explicit
 * multi-step entry points and lt_plan_two_step_admitted return LT_ERR_UNSUPPORTED with a reason that names the
 * equilibrium.  lt_plan_desc keeps its size and LT_ABI_VERSION its value. */
int lt_plan_set_equilibrium(lt_plan *plan, int kind, double rho0);
/* Population stride.  By default a population buffer is dense: population q starts q * nodes elements after
 * population 0 (the reference's [q, *res] tensor, lettuce/_flow.py:90).  With the q populations a power of two
 * apart (256^3 fp32: exactly 64 MiB) the q read and q write streams of a node meet in the same memory channels;
 * buffers the CALLER owns and the reference never sees -- the slab tensors of a multi-GPU rank -- may therefore
 * be padded: every population buffer handed to this plan's entry points (steps, pack / unpack, reductions,
 * lt_macroscopic) then has `stride_elements` (>= nodes incl. ghost planes, a multiple of 256 bytes) between
 * consecutive populations; 0 = dense again.  Per-node boundary fields and masks stay dense. */
int lt_plan_set_population_stride(lt_plan *plan, int64_t stride_elements);
int lt_plan_population_stride(lt_plan *plan, int64_t *stride_elements_out);
/* Resident populations: the engine's own padded ping-pong buffers for the fused steps of a periodic plan, so that
 * the caller's tensors stay the reference's plain [q, *res] (lettuce/_flow.py:90,124-134,226-236) and are touched
 * only when somebody looks:
 *   lt_resident_load     f* <- B(C(f)): one collide pass from the caller's post-streaming populations (the
 *                        reference's flow.f) into the resident buffer;
 *   lt_resident_advance  n fused stream-collide steps on the resident f* (lt_run's fused section: two updates per
 *                        launch where the kernel exists, several on small 2-D grids; lt_plan_set_fused_events and
 *                        lt_plan_last_run_info apply);
 *   lt_resident_store    out <- S(f*): the streaming pass that presents the populations in lettuce's convention;
 *                        the resident state stays valid, a later lt_resident_advance carries on from it;
 *   lt_resident_free     releases the two buffers (lt_plan_destroy does too).
 * k whole lettuce steps from flow.f are load + advance(k - 1) (+ store when flow.f is read); a batch that carries
 * on is advance(k).  lt_plan_set_resident: mode -1 = automatic (lt_resident_enabled reports 1 when the populations
 * exceed the caches), 0 = off, 1 = on; pad_elements = distance added between populations, -1 = the engine's choice.
 * lt_run / lt_continue keep working on caller-owned dense buffers whatever the mode. */
int lt_plan_set_resident(lt_plan *plan, int32_t mode, int64_t pad_elements);
int lt_resident_enabled(lt_plan *plan, int32_t *enabled_out, int64_t *stride_elements_out);
int lt_resident_load(lt_plan *plan, const void *f_dev, double tau, void *stream);
int lt_resident_advance(lt_plan *plan, double tau, int64_t n_steps, void *stream);
int lt_resident_store(lt_plan *plan, void *out_dev, void *stream);
int lt_resident_free(lt_plan *plan);
/* Measurement hooks.  With two hipEvent_t set, lt_run / lt_continue record them on the launch stream
 * around their fused launches (around the two-step launches when there are any, else around the
 * single-step ones, or around the many-step launches); null, null removes them.
 * lt_plan_last_run_info reports how many fused launches of each kind the last lt_run / lt_continue
 * issued. */
int lt_plan_set_fused_events(lt_plan *plan, void *start_event, void *stop_event);
int lt_plan_last_run_info(lt_plan *plan, int64_t *single_step_launches, int64_t *two_step_launches,
                          int64_t *many_step_launches);
/* Workgroups resident per CU for the chip-filling launches (an unused dynamic-LDS allocation caps
 * them): -1 = automatic (3, or 4 for fp32 KBC, once the populations stream from HBM and the launch
 * fills the chip several times over; no cap otherwise), 0 = no cap, 2..8 = that many. */
int lt_plan_set_residency(lt_plan *plan, int32_t workgroups_per_cu);
/* First-use check of the two-step kernels of a plan WITH masks.  Before such a plan uses a two-step kernel for the
 * first time (lt_run's pairs, lt_resident_advance, every lt_stream_collide_twice* entry point,
 * lt_plan_two_step_admitted), one double step over all its planes is held against two one-step launches: synthetic
 * populations on engine-owned scratch buffers, the plan's own masks, boundaries, tile and segment length, bit-for-bit
 * comparison on the device (four scratch fields, five launches, one synchronisation of an engine-owned stream; again
 * after lt_plan_set_masks or a change of the segment length).  If the two disagree -- hipcc has miscompiled exactly
 * this code once, see csrc/Makefile -- or the check cannot run, the plan keeps the one-step kernel: lt_run /
 * lt_continue / lt_resident_advance fall back by themselves and leave the reason in lt_last_error(); the explicit
 * two-step entry points and lt_plan_two_step_admitted return LT_ERR_UNSUPPORTED with it.  What is protected:
 * lettuce/_simulation.py:177-189 (collision, then every boundary in index order, on the nodes of its mask).
 * lt_plan_set_canary: 1 = check on first use (default), 0 = trust the kernel, 2 = report a mismatch without
 * launching (test hook).  lt_plan_canary_status: 0 = not run yet, 1 = passed, 2 = skipped, -1 = failed (then
 * *mismatches_out holds the number of differing populations, or 0 when the check could not run, and *message_out
 * the reason; the string lives as long as the plan). */
int lt_plan_set_canary(lt_plan *plan, int32_t mode);
int lt_plan_canary_status(lt_plan *plan, int32_t *status_out, int64_t *mismatches_out, const char **message_out);

/* Halo transport without compute units (slab drivers, transport "copy"; SURVEY.md 8(e): the reference has no
 * multi-GPU path, north_star asks for send/recv over xGMI overlapped with the interior).  RCCL moves a message with a
 * kernel of 64 workgroups and 20 KB of LDS each, which cannot share a compute unit with a 150 KB sweep workgroup and
 * costs the sweep beside it about 5 %; a device-to-device copy handed to a copy (SDMA) engine needs neither.
 *   lt_ipc_alloc / lt_ipc_open / lt_ipc_close / lt_ipc_free   device memory the other processes of the node can map:
 *       every rank allocates its receive window (halo messages) and, as fine-grained memory (fine_grained = 1:
 *       coherent with writers outside the running kernel), one 64-bit arrival counter per direction; it sends the
 *       64-byte handles to its two z-neighbours through the process group and opens theirs;
 *   lt_halo_copy   dst <- src on `stream`; engine 1 = without compute units (hipMemcpyDeviceToDeviceNoCU: an SDMA
 *       engine, over xGMI when dst is a neighbour's window), 0 = the runtime's choice; *engine_used reports which;
 *   lt_flag_write  *flag <- value in stream order after the copies: how 1 = stream memory operation (command
 *       processor, no kernel), 0 = a one-thread kernel storing at system scope;
 *   lt_flag_wait   one wave that returns when *flag >= at_least or, after about a second, sets *timed_out_dev and
 *       returns all the same (the driver raises at the end of the batch; nothing traps, nothing spins for ever). */
int lt_ipc_alloc(int64_t n_bytes, int32_t fine_grained, void **dev_out, void *handle_out_64_bytes);
int lt_ipc_open(const void *handle_64_bytes, void **dev_out);
int lt_ipc_close(void *mapped_dev);
int lt_ipc_free(void *dev);
int lt_halo_copy(void *dst_dev, const void *src_dev, int64_t n_bytes, int32_t engine, void *stream, int32_t *engine_used);
int lt_flag_write(uint64_t *flag_dev, uint64_t value, int32_t how, void *stream);
int lt_flag_wait(const uint64_t *flag_dev, uint64_t at_least, uint32_t *timed_out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LETTUCE_HIP_H */
