// Type-erased launch interface between api.hip (plan handling, C ABI) and the
// per-(stencil, dtype) translation units that instantiate the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace lt {

enum StepMode { kFused = 0, kCollideOnly = 1, kStreamOnly = 2, kFusedTwice = 3, kFusedMany = 4 };

// The kernels' collision number (their COLL, StepArgs::coll): lt_collision where the ABI has the operator, kCollForce
// added to BGK and Smagorinsky with a body force (5, 7), and the MRT transforms apart.  TRT and the regularised
// collision are 8 and 9, MRT 10 and 11, so that none of them carries the force bit by accident.
constexpr int kCollNone = 0, kCollBgk = 1, kCollKbc = 2, kCollSmagorinsky = 3, kCollForce = 4, kCollTrt = 8,
              kCollRegularized = 9, kCollMrt = 10, kCollMrtLallemand = 11;
// ... and kCollIncompressible added to the collisions that have kernels with the incompressible equilibrium
// (lt_plan_set_equilibrium): BGK 17, BGK with a body force 21, TRT 24, the regularised collision 25.  Without the bit:
// the quadratic equilibrium, so a zeroed StepArgs means what it meant.
constexpr int kCollIncompressible = 16;
constexpr bool coll_incompressible(int coll) { return (coll & kCollIncompressible) != 0; }
constexpr bool coll_mrt(int coll) { return coll == kCollMrt || coll == kCollMrtLallemand; }
constexpr bool coll_forced(int coll) {
  return (coll & ~kCollIncompressible) == (kCollBgk | kCollForce) || coll == (kCollSmagorinsky | kCollForce);
}
constexpr int coll_base(int coll) { return coll_forced(coll) ? coll & ~kCollForce : coll; }   // the collision under the force
// ... and kCollField added to BGK and Smagorinsky with a body force whose acceleration is a per-node field
// (lt_plan_set_force_field): 37 and 39.  A bit above every number so far (0-25), and numbers of their own rather than
// forced ones: coll_forced says "takes KParamsF", these take KParamsFF.
constexpr int kCollField = 32;
constexpr bool coll_field(int coll) {
  return coll == (kCollBgk | kCollForce | kCollField) || coll == (kCollSmagorinsky | kCollForce | kCollField);
}
constexpr int coll_field_base(int coll) { return coll & ~(kCollForce | kCollField); }   // the collision under the field

struct StepArgs {
  const void *in;
  void *out;
  int n0, n1, n2;        // memory extents (n2 incl. ghost planes)
  long long stride_in, stride_out;   // elements between consecutive populations of in / out; 0 = dense (n0*n1*n2)
  int p_begin, planes;   // a2 planes of this launch: p_begin + i * p_stride, i < planes
  int p_stride;
  int p_begin2, planes2;  // kFusedTwice: optional second range of output planes
  int wrap2;
  double tau;
  double smagorinsky;    // Smagorinsky constant (collision 3); the units square it
  double tau_minus;      // TRT (collision 8): the relaxation time of the antisymmetric part; tau is tau_plus
  // body force (coll & 4, lt_plan_set_force): acceleration in the logical order x, y, z (the units permute it to the
  // memory axes of the layout) and the two scales of the scheme
  double accel[3], ueq_scale, source_scale;
  const unsigned char *node;
  const unsigned *nsm_bits;
  const void *bt;        // BoundaryTable<T>* (device)
  int nb;
  int layout, coll, mode, masked, shift, tune;   // coll: the kernels' COLL, one of the kColl* numbers above (with a body
                                                 // force: | kCollForce)
  int strip;             // kFusedTwice on 2-D lattices: columns per workgroup (512 / 256 / 128 / 64)
  int abb_axis;          // kFusedTwice with masks: memory axis of the plan's outlet (2 without one)
  int n_abb;             // anti-bounce-back outlets of the plan
  int abb0_slot;         // one-step kernels: 1-based index of the plan's only outlet if its normal is memory axis a0, else 0
  int abb_depth;         // anti-bounce-back outlets of the plan - 1 (0: at most one; the kernels exist for 0 and 1)
  int n_pout;            // constant-pressure outlets of the plan: > 0 takes the unit's part outlets (one-step kernels only)
  int lds_bytes;         // unused dynamic LDS per workgroup (residency cap), 0 = none
  int seg_len;           // kFusedTwice: a2 planes per workgroup; kFusedMany: steps in this launch
  void *pack_lo, *pack_hi;         // fused halo packing (slab boundary launch) or null
  int pack_lo_plane, pack_hi_plane;
  unsigned long long *signal;      // kFusedTwice with both message buffers: edge workgroups first, each adds 1 here (or null)
  const void *ghost_lo, *ghost_hi; // kFusedTwice edge launch: received halo messages to read the planes beyond the cuts from (or null)
  int interior_begin, interior_end;   // first interior plane, one past the last
  hipStream_t stream;
  // MRT (coll 10, 11; lt_plan_set_mrt): the transform (lt_mrt_transform; 0: no MRT) and the relaxation rates s_i of its
  // q moments, as the caller gave them (the units form 1 / s_i in the plan's scalar type)
  int mrt_transform;
  double mrt_rates[27];
  // the incompressible equilibrium (coll & 16, lt_plan_set_equilibrium): its reference density; the units round it to
  // the plan's scalar type
  double rho0;
  // per-node body force (coll & 32, lt_plan_set_force_field): the acceleration [dims][n0 * n1 * n2] in the plan's scalar
  // type on the device, logical axis order, reference node order; null: no field.  Its two scales travel in ueq_scale
  // and source_scale above
  const void *accel_field;
};

// The auxiliary launches of a unit (aux_<tag>; AuxArgs::what).  Nothing outside csrc/ sees the numbers.
enum AuxKind {
  kAuxMacroscopic = 0,    // rho, u <- f
  kAuxEquilibrium,        // f <- feq(rho, u)
  kAuxKineticEnergy,      // sum of u.u / 2 over the interior planes
  kAuxMass,               // sum of rho over the interior planes
  kAuxMaxVelocity,        // max |u| over the interior planes (NaN wins)
  kAuxEnstrophy,          // u into the scratch field, then the vorticity stencil over it
  kAuxInteriorMass,       // the mass observable: off the faces of the two fastest axes, minus the masked nodes
  kAuxFneq,               // non-equilibrium initialisation: f <- feq(rho, u) - fneq(grad u)
  kAuxSlabEnstrophy,      // the vorticity stencil over a slab's velocity field (three neighbour planes per side)
  kAuxSlabInteriorMass,   // the mass observable over a rank's planes
  kAuxSpectrum,           // energy spectrum of d Fourier-transformed fields: part spectrum
  kAuxBoundaryForce,      // momentum-exchange force on the nodes of a mask: part boundary_force
  kAuxKinds
};
// What api.hip asks about a kind before it launches: the name its messages use; whether the kernel takes a population
// stride (the others read dense buffers only); whether it exists for whole grids only (d >= 2, reference layout, no
// ghost planes).
struct AuxTraits {
  const char *name;
  bool strided, whole_grid;
};
constexpr AuxTraits kAuxTraits[kAuxKinds] = {
    {"macroscopic moments", true, false},   {"equilibrium", false, false},        {"kinetic energy", true, false},
    {"mass", true, false},                  {"maximum velocity", true, false},    {"enstrophy", false, true},
    {"interior mass", false, true},         {"f_neq initialisation", false, true}, {"slab enstrophy", true, false},
    {"slab interior mass", true, false},    {"energy spectrum", false, true},     {"boundary force", false, true},
};

// Plan-derived fields first (api.hip, aux_args), then what the kind's entry point sets by name
struct AuxArgs {
  AuxKind what;
  int layout;
  long long N;           // nodes per population (incl. ghost planes)
  long long stride;      // elements between consecutive populations of f (the kinds with AuxTraits::strided; dense = N
                         // elsewhere)
  long long first, count;  // the interior planes' node range (kAuxKineticEnergy, kAuxMass, kAuxMaxVelocity,
                           // kAuxSlabInteriorMass); kAuxSpectrum: count = modes per workgroup
  int n0, n1, n2;        // memory extents; kAuxSlabEnstrophy: n2 = the rank's planes + 6
  double *partial;       // the plan's scratch, >= reduce_blocks doubles; kAuxSpectrum: the caller's, reduce_blocks x
                         // n_bins doubles; kAuxBoundaryForce: the caller's, 3 x reduce_blocks doubles
  int reduce_blocks;     // workgroups of the reducing launch
  int equilibrium;       // kAuxEquilibrium, kAuxFneq: lt_equilibrium_kind of the plan (0: quadratic) and, for kind 1, its rho0
  double rho0;
  hipStream_t stream;
  const void *f;         // populations; kAuxEquilibrium, kAuxFneq: the output (cast away const); kAuxSpectrum: the d
                         // transformed fields; null for kAuxSlabEnstrophy
  void *rho;             // kAuxMacroscopic: out (or null); kAuxEquilibrium, kAuxFneq: in
  void *u;               // kAuxMacroscopic: out (or null); kAuxEquilibrium, kAuxFneq: in; kAuxEnstrophy: the scratch
                         // field; kAuxSlabEnstrophy: the slab's velocity field u [3][n2][n1][n0]
  long long u_stride;    // kAuxMacroscopic: elements between the components of u (0 = N)
  double *out;           // device result: a scalar; kAuxSpectrum: n_bins doubles; kAuxBoundaryForce: 3 doubles
  double scale, inv_dx;  // kAuxEnstrophy, kAuxSlabEnstrophy: u_pu = scale * u_lu, 1 / dx_pu; kAuxFneq: tau, the identity's
                         // cs^2; kAuxSpectrum: scale of the bins
  const unsigned char *mask;   // kAuxInteriorMass, kAuxSlabInteriorMass: no-mass mask or null; kAuxBoundaryForce: the solid nodes
  int z_begin, nz_global;      // kAuxSlabInteriorMass: global index of the rank's first plane, planes of the whole grid
  int n_bins;                  // kAuxSpectrum: bins of the spectrum
};

// The link kernels of a plan with link bounce-back (link_bounce.hpp; the units' part links): one compact list of links
// in plan-owned device memory, c1 / c2 in the plan's scalar type
enum LinkKind {
  kLinkBounce = 0,       // the bounce-back pass on f, in place
  kLinkForce             // the momentum-exchange force over the list
};
struct LinkArgs {
  LinkKind what;
  void *f;               // populations [q][stride]
  long long stride;      // elements between consecutive populations of f
  const int *node;
  const unsigned char *dir;
  const void *c1, *c2;
  const unsigned char *second;
  int n_links;
  int n0, n1, n2;        // memory extents
  double *partial;       // kLinkForce: the caller's scratch of 3 x blocks doubles
  int blocks;            // kLinkForce: workgroups of the first launch (0 for an empty list)
  double *out;           // kLinkForce: 3 doubles
  hipStream_t stream;
};

// Kernel names are written into a buffer of the caller's (lt_plan_kernel_name: the plan's; a probe: a local one).
// The units' functions take a pointer to one: null launches, non-null only names the kernel the arguments select.
struct NameBuf {
  char *s;
  size_t cap;
};

typedef int (*StepFn)(const StepArgs &);
typedef int (*AuxFn)(const AuxArgs &);
typedef const char *(*NameFn)(const StepArgs &, const NameBuf &);     // the buffer, or null: no kernel

// The units: one per lattice and scalar type.                lattice, scalar, Q, D, KBC, role-wave sweep
#define LT_UNIT_d2q9_f32  D2Q9,  float,   9, 2, 1, 0
#define LT_UNIT_d2q9_f64  D2Q9,  double,  9, 2, 1, 0
#define LT_UNIT_d3q19_f32 D3Q19, float,  19, 3, 0, 1
#define LT_UNIT_d3q19_f64 D3Q19, double, 19, 3, 0, 0
#define LT_UNIT_d3q27_f32 D3Q27, float,  27, 3, 1, 0
#define LT_UNIT_d3q27_f64 D3Q27, double, 27, 3, 1, 0
#define LT_UNIT_d1q3_f32  D1Q3,  float,   3, 1, 0, 0
#define LT_UNIT_d1q3_f64  D1Q3,  double,  3, 1, 0, 0
#define LT_UNIT_d3q15_f32 D3Q15, float,  15, 3, 0, 0
#define LT_UNIT_d3q15_f64 D3Q15, double, 15, 3, 0, 0
// ... in the order of the ABI's enums: lt_stencil the slower index, lt_dtype the faster (api.hip, kUnits)
#define LT_UNITS(X)                                                                                  \
  X(d2q9_f32) X(d2q9_f64) X(d3q19_f32) X(d3q19_f64) X(d3q27_f32) X(d3q27_f64) X(d1q3_f32) X(d1q3_f64) \
  X(d3q15_f32) X(d3q15_f64)
// LT_FIELD(name, tag): a column of a unit; tag may be a macro (the build's LT_UNIT)
#define LT_FIELD(name, tag) LT_FIELD_A(name, tag)
#define LT_FIELD_A(name, tag) LT_FIELD_B(name, LT_UNIT_##tag)
#define LT_FIELD_B(name, ...) LT_FIELD_##name(__VA_ARGS__)
#define LT_FIELD_lattice(s, t, q, d, kbc, roles) s
#define LT_FIELD_scalar(s, t, q, d, kbc, roles) t
#define LT_FIELD_q(s, t, q, d, kbc, roles) q
#define LT_FIELD_d(s, t, q, d, kbc, roles) d
#define LT_FIELD_kbc(s, t, q, d, kbc, roles) kbc
#define LT_FIELD_roles(s, t, q, d, kbc, roles) roles

// What the objects of a unit export.  The parts of a unit, what each holds and which of them pass on to which are
// listed once, in the header of unit.inc (LT_PART).  Part main has the three entry points api.hip calls; declared for
// every unit, defined where the Makefile builds the part.
#define LT_DECLARE_UNIT(tag)                                   \
  int step_##tag(const StepArgs &);                            \
  int aux_##tag(const AuxArgs &);                              \
  const char *name_##tag(const StepArgs &, const NameBuf &);   \
  int forced_##tag(const StepArgs &, const NameBuf *);         \
  int relax_##tag(const StepArgs &, const NameBuf *);          \
  int outlets_##tag(const StepArgs &, const NameBuf *);        \
  int outlets2_##tag(const StepArgs &, const NameBuf *);       \
  int outlets3_##tag(const StepArgs &, const NameBuf *);       \
  int twice_##tag(const StepArgs &, const NameBuf *);          \
  int smag_##tag(const StepArgs &, const NameBuf *);           \
  int roles_##tag(const StepArgs &, const NameBuf *);          \
  int mrt_##tag(const StepArgs &, const NameBuf *);            \
  int mrt_outlets_##tag(const StepArgs &, const NameBuf *);    \
  int incompressible_##tag(const StepArgs &, const NameBuf *); \
  int incompressible_aux_##tag(const AuxArgs &);               \
  int force_field_##tag(const StepArgs &, const NameBuf *);    \
  int spectrum_##tag(const AuxArgs &);                         \
  int boundary_force_##tag(const AuxArgs &);                   \
  int links_##tag(const LinkArgs &);
LT_UNITS(LT_DECLARE_UNIT)

// returns -1 when the combination has no instantiated kernel, else the hipError_t of the launch
constexpr int kNoKernel = -1;

// The Jacobi solver's two launches (jacobi.hpp), in an object of their own (jacobi.hip) that holds no unit: one sweep from
// p_in into p_out (nullptr: the iterate is not kept) with the workgroup partials of the input iterate's squared residuum,
// and -- when finish is set -- the one-workgroup launch behind it that forms the error of iterate sweep - 1, holds it
// against tol and writes the state record.  work: the caller's kJacobiBlocks partials with the record behind them.
struct JacobiArgs {
  const void *p_in, *rhs;
  void *p_out, *work;
  int dtype, d;                // 0 float, 1 double; 2 or 3
  int n0, n1, n2;              // n2 = 1 in 2-D
  double dx2, tol;             // dx2 formed in double, cast to the dtype at the launch
  long long sweep;
  bool finish;
  hipStream_t stream;
};
int jacobi_sweep(const JacobiArgs &);          // the hipError_t of the launches
void *jacobi_state(void *work);                // where the record lies in the work buffer

}  // namespace lt
