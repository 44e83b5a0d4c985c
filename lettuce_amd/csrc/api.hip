// C ABI of the engine (include/lettuce_hip.h): plan handling, argument checks, dispatch to
// the per-(stencil, dtype) kernel units.  No kernel code here.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <type_traits>

#include "dispatch.hpp"
#include "kernels.hpp"
#include "launch_limits.hpp"
#include "lettuce_hip.h"

namespace {

// per calling thread: a caller must read lt_last_error() on the thread whose call failed (the ctypes
// binding does, right after the failing call, before anything can migrate the Python thread)
thread_local char g_error[512] = "";

int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
  return code;
}

// What a unit's launcher returned: kNoKernel is LT_ERR_UNSUPPORTED with the caller's text, a hipError_t LT_ERR_HIP
int launched(int r, const char *no_kernel_fmt, ...) {
  if (r == 0) return LT_OK;
  if (r != lt::kNoKernel) return fail(LT_ERR_HIP, "kernel launch failed: %s", hipGetErrorString((hipError_t)r));
  va_list ap;
  va_start(ap, no_kernel_fmt);
  vsnprintf(g_error, sizeof g_error, no_kernel_fmt, ap);
  va_end(ap);
  return LT_ERR_UNSUPPORTED;
}

#define LT_HIP(call)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(LT_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_));          \
  } while (0)

struct Unit {
  lt::StepFn step;
  lt::AuxFn aux;
  lt::NameFn name;
  int q, d;
  lt::UnitTile tile;     // the unit's 3-D two-step tile (launch_limits.hpp)
};

// every unit of dispatch.hpp's list, which is in the order of the ABI's enums: kUnits[2 * stencil + dtype]
#define LT_UNIT_ROW(tag) {lt::step_##tag, lt::aux_##tag, lt::name_##tag, LT_FIELD(q, tag), LT_FIELD(d, tag), \
                          lt::two_step_tile<lt::LT_FIELD(lattice, tag), LT_FIELD(scalar, tag)>()},
const Unit kUnits[] = {LT_UNITS(LT_UNIT_ROW)};
#undef LT_UNIT_ROW
static_assert(LT_D2Q9 == 0 && LT_D3Q19 == 1 && LT_D3Q27 == 2 && LT_D1Q3 == 3 && LT_D3Q15 == 4 && LT_F32 == 0 && LT_F64 == 1 &&
              sizeof kUnits == 10 * sizeof(Unit), "LT_UNITS is not in the order of lt_stencil and lt_dtype");
// has the unit a kernel for these arguments?  (its name goes into a buffer of ours)
bool has_kernel(const Unit &unit, const lt::StepArgs &a) {
  char name[192];
  return unit.name(a, lt::NameBuf{name, sizeof name}) != nullptr;
}

// the units' part links, in the order of kUnits; the 1-D units have none
typedef int (*LinkFn)(const lt::LinkArgs &);
const LinkFn kLinkUnits[] = {lt::links_d2q9_f32,  lt::links_d2q9_f64,  lt::links_d3q19_f32, lt::links_d3q19_f64,
                             lt::links_d3q27_f32, lt::links_d3q27_f64, nullptr,             nullptr,
                             lt::links_d3q15_f32, lt::links_d3q15_f64};
static_assert(sizeof kLinkUnits / sizeof kLinkUnits[0] == sizeof kUnits / sizeof kUnits[0], "a row per unit");

constexpr int kReduceBlocks = 1024;

// plain streaming copy, 16 B per lane: the device-copy ceiling the roofline fraction is quoted
// against next to the 8 TB/s spec number
typedef float probe_f4 __attribute__((ext_vector_type(4)));
template <int TUNE>
__global__ void __launch_bounds__(256) probe_copy_kernel(const probe_f4 *__restrict__ src,
                                                         probe_f4 *__restrict__ dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const probe_f4 v = (TUNE & 1) ? __builtin_nontemporal_load(src + i) : src[i];
    if (TUNE & 2) __builtin_nontemporal_store(v, dst + i); else dst[i] = v;
  }
}

// One wave: returns when *flag >= at_least (a neighbour rank's copy engine has delivered its halo message and the
// flag write that follows it in that rank's stream has landed), or after about a second, setting *timed_out -- an exit
// every launch reaches.  Relaxed polls at SYSTEM scope (the writer is another device or a copy engine), one acquire
// at the end; no LDS, one wave: it shares a CU with a 150 KB sweep workgroup.
__global__ void wait_flag_kernel(const unsigned long long *flag, unsigned long long at_least, unsigned *timed_out) {
  const long long t0 = wall_clock64();
  while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < at_least) {
    __builtin_amdgcn_s_sleep(127);
    if (wall_clock64() - t0 > 100000000ll) {           // 100 MHz: one second
      __hip_atomic_store(timed_out, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      break;
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
}
__global__ void write_flag_kernel(unsigned long long *flag, unsigned long long value) {
  __atomic_thread_fence(__ATOMIC_RELEASE);
  __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the equilibrium's exact division by its rounded constants (kernels.hpp, div_cs) on an array: the GPU-side pin of
// what tests/aux/exact_division_check.c proves on the host -- in particular that the device keeps fp32 denormals
// (x r_lo of the two-instruction form is denormal for |x / D| below ~1e-30)
template <typename T>
__global__ void __launch_bounds__(256) probe_div_cs_kernel(const T *x, T *out, long long n, int which) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = which == 0 ? lt::div_cs<0>(x[i]) : lt::div_cs<1>(x[i]);
}

// first-use check of the masked two-step kernels (run_canary): synthetic populations -- positive, near 1 / Q, a
// different value in nearly every slot -- and a bit-for-bit comparison of two population fields over a plane range
template <typename T>
__global__ void __launch_bounds__(256) canary_fill_kernel(T *f, long long stride, long long N, int Q) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N * Q; i += (long long)gridDim.x * 256) {
    const long long q = i / N, x = i - q * N;
    const unsigned h = (unsigned)(((unsigned long long)i * 2654435761ull) >> 9) & 4095u;
    f[q * stride + x] = (T)((1.0 / Q) * (1.0 + 0.2 * ((double)h / 4096.0 - 0.5)));
  }
}
template <typename U>
__global__ void __launch_bounds__(256) canary_compare_kernel(const U *a, const U *b, long long stride, long long first,
                                                             long long count, int Q, unsigned long long *mismatches) {
  unsigned long long mine = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count * Q; i += (long long)gridDim.x * 256) {
    const long long q = i / count, x = first + (i - q * count);
    mine += a[q * stride + x] != b[q * stride + x];
  }
  if (mine) atomicAdd(mismatches, mine);
}

}  // namespace

struct lt_plan {
  lt_plan_desc desc;
  Unit unit;
  int esize;                 // sizeof scalar
  int n0, n1, n2;            // memory extents incl. ghost planes
  int interior_begin, interior_end;   // a2 planes that are real nodes
  long long N;               // n0*n1*n2
  int n_cu = 0;              // compute units of the plan's device
  // What a setter may change between two launches and every launch reads, like tau.  One record: a captured graph is
  // replayed only for the Settings it was captured with (run_graph compares the whole of it), and a new setting is
  // added here -- its field, its term in operator==, and its line in fill() if it is a value the kernels take (the
  // four at the end choose the kernel and its launch instead: kernel_selector, resolve_tune, resolve_lds)
  struct Settings {
    double smagorinsky = 0.17; // Smagorinsky constant (lt_plan_set_smagorinsky); the reference's default
    double tau_minus = 1.0;    // TRT: relaxation time of the antisymmetric part (lt_plan_set_trt); the reference's default
    // MRT (lt_plan_set_mrt): the transform (lt_mrt_transform; 0 = not set yet) and the relaxation rates of its q moments
    struct Mrt { int transform = 0; double rates[27] = {}; } mrt;
    // uniform body force (lt_plan_set_force).  on: the kernels with COLL = 4 + collision
    struct Force { bool on = false; double a[3] = {0.0, 0.0, 0.0}, ueq_scale = 0.0, source_scale = 0.0; } force;
    // ... or one whose acceleration is a per-node field (lt_plan_set_force_field; the two exclude each other).  a: the
    // caller's device memory, [dims][N] in the plan's dtype; non-null: the kernels with COLL = 36 + collision.  A changed
    // pointer is a changed setting
    struct ForceField { const void *a = nullptr; double ueq_scale = 0.0, source_scale = 0.0; } field;
    // the equilibrium (lt_plan_set_equilibrium): lt_equilibrium_kind and, for the incompressible one, its rho0
    int equilibrium = LT_EQUILIBRIUM_QUADRATIC;
    double rho0 = 1.0;
    int masked = 0;            // lt_plan_set_masks
    int tune = -1;             // cache policy: -1 = automatic
    int shift = 0;             // lt_plan_set_shift_policy: workgroup order of the two-step kernel (A/B)
    int residency = -1;        // workgroups per CU of the big launches: -1 = automatic, 0 = no cap
    bool operator==(const Settings &o) const {
      return smagorinsky == o.smagorinsky && tau_minus == o.tau_minus && mrt.transform == o.mrt.transform &&
             std::equal(mrt.rates, mrt.rates + 27, o.mrt.rates) && force.on == o.force.on &&
             std::equal(force.a, force.a + 3, o.force.a) && force.ueq_scale == o.force.ueq_scale &&
             force.source_scale == o.force.source_scale && field.a == o.field.a &&
             field.ueq_scale == o.field.ueq_scale && field.source_scale == o.field.source_scale && equilibrium == o.equilibrium && rho0 == o.rho0 &&
             masked == o.masked && tune == o.tune && shift == o.shift && residency == o.residency;
    }
    void fill(lt::StepArgs &a) const {
      a.smagorinsky = smagorinsky;
      a.tau_minus = tau_minus;
      a.mrt_transform = mrt.transform;
      std::copy(mrt.rates, mrt.rates + 27, a.mrt_rates);
      std::copy(force.a, force.a + 3, a.accel);
      a.ueq_scale = force.ueq_scale; a.source_scale = force.source_scale;
      a.accel_field = field.a;
      if (field.a) { a.ueq_scale = field.ueq_scale; a.source_scale = field.source_scale; }
      a.rho0 = rho0;
    }
  } set;
  int two_step = -1;         // lt_run: pair the fused steps (lbm2_kernel): -1 = automatic, 0 / 1
  int seg_len = 0;           // planes per workgroup of the two-step kernel, 0 = automatic
  int many = -1;             // lt_run: several steps per launch on small 2-D grids: -1 = automatic, 0 / 1
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;   // lt_plan_set_fused_events
  long long last_single = 0, last_twice = 0, last_many = 0;   // fused launches of the last lt_run
  // engine-owned device scratch
  unsigned char *node = nullptr;
  unsigned *nsm_bits = nullptr;
  void *bt = nullptr;        // BoundaryTable<T>
  double *partial = nullptr;
  int n_abb = 0;             // anti-bounce-back outlets of the plan
  int n_pout = 0;            // constant-pressure outlets of the plan (one-step kernels only: multi_step_refusal)
  // link bounce-back (LT_BOUNDARY_LINK_BOUNCE_BACK): the boundaries of that kind and, per boundary of the plan, its list
  // in device memory (lt_plan_set_links; `set` also for an empty one)
  int n_link_kind = 0;
  struct Links {
    bool set = false;
    int n = 0;
    int *node = nullptr;
    unsigned char *dir = nullptr, *second = nullptr;
    void *c1 = nullptr, *c2 = nullptr;
  } links[LT_MAX_BOUNDARIES];
  int abb_depth = 0;         // how deep an outlet's neighbour must be rebuilt (lt_plan_create)
  int nsm_confined = 1;      // the no-streaming bits are exactly those of the plan's outlet (lt_plan_set_masks)
  int inlet_faces_outlet = 1;  // outlet along a0: every node of the opposite face is an equilibrium node
  unsigned *mask_flag = nullptr;   // device word written by the mask compilation
  // lt_stream_collide_twice_slab: counter the edge workgroups increment, the value it reaches when the messages
  // of the last such launch are complete, and the word wait_counter_kernel sets when it gives up
  unsigned long long *signal = nullptr;
  unsigned long long signal_target = 0;
  unsigned *signal_timed_out = nullptr;
  int defer_stream = 0;      // lt_run / lt_continue stop before their last (streaming) pass (lt_plan_set_deferred_stream)
  // distance between consecutive populations of the caller's buffers, in elements (lt_plan_set_population_stride);
  // 0 = dense (N)
  long long pop_stride = 0;
  // engine-owned padded population buffers (lt_resident_*): res[res_cur] holds the post-collision populations
  int resident = -1;         // -1 = automatic, 0 = off, 1 = on (lt_plan_set_resident)
  long long res_pad = -1;    // elements between the end of one population and the start of the next; -1 = automatic
  long long res_stride = 0;  // stride of the allocated buffers
  void *res[2] = {nullptr, nullptr};
  int res_cur = 0;
  int res_valid = 0;
  // first-use check of the masked two-step kernel (run_canary; lt_plan_set_canary / lt_plan_canary_status)
  int canary_mode = 1;       // 1 = check on first use, 0 = skip, 2 = test hook: report a mismatch without launching
  int canary = 0;            // 0 = not run for the present masks / settings, 1 = passed, 2 = skipped, -1 = failed
  long long canary_mismatches = 0;
  char canary_msg[320] = "";
  hipStream_t cstream = nullptr;
  char kernel_name[192];
  // launch-bound grids: a captured hipGraph of kGraphChunk fused steps (ping-pong returns to the
  // starting buffer), replayed on a plan-owned stream that is forked from / joined to the caller's
  int graph_mode = -1;       // -1 automatic (small grids), 0 off, 1 always
  hipStream_t gstream = nullptr;
  hipEvent_t gev_in = nullptr, gev_out = nullptr;
  hipGraphExec_t gexec = nullptr;
  struct { void *a, *b; double tau; Settings set; } gkey = {};
};

namespace {

// elements between consecutive populations of the caller's buffers
long long pop_stride_of(const lt_plan *p) { return p->pop_stride > 0 ? p->pop_stride : p->N; }

int mem_axis_of(const lt_plan *p, int logical_axis) {
  if (p->unit.d == 1) return 0;
  if (p->unit.d == 2) return logical_axis == 0 ? 1 : 0;
  return p->desc.layout == LT_LAYOUT_REFERENCE ? 2 - logical_axis : logical_axis;
}

template <typename T>
int upload_boundaries(lt_plan *p, hipStream_t stream) {
  lt::BoundaryTable<T> h;
  memset(&h, 0, sizeof h);
  const int ext[3] = {p->n0, p->n1, p->n2};
  for (int i = 0; i < p->desc.n_boundaries; ++i) {
    const lt_boundary_desc &b = p->desc.boundaries[i];
    const int s = i + 1;
    h.kind[s] = b.kind;
    if (b.kind == LT_BOUNDARY_PRESSURE_OUTLET) h.rho_outlet[s] = (T)b.feq[0];   // rounded as the reference's tensor is
    if (b.kind == LT_BOUNDARY_ABB_OUTLET || b.kind == LT_BOUNDARY_PRESSURE_OUTLET) {
      const int ax = mem_axis_of(p, b.axis);
      h.mem_axis[s] = ax;
      h.side[s] = b.side;
      // along the decomposed axis of a slab the first / last plane of the grid is the first / last
      // interior plane of the rank that holds it; the other ranks have no outlet (a plane no node has)
      const int g = ax == 2 ? p->desc.ghost_planes : 0;
      h.plane[s] = b.side > 0 ? ext[ax] - 1 - g : g;
      h.nbr[s] = h.plane[s] - b.side;
      if (g && (b.flags & LT_BOUNDARY_ABSENT)) h.plane[s] = h.nbr[s] = -1000000;
    } else if (b.kind == LT_BOUNDARY_EQUILIBRIUM) {
      for (int q = 0; q < p->unit.q; ++q) h.feq[s][q] = (T)b.feq[q];
      h.field[s] = static_cast<const T *>(b.feq_field_dev);
    }
  }
  // staged through the (pageable) host struct: synchronous w.r.t. the host, ordered on stream
  LT_HIP(hipMemcpyAsync(p->bt, &h, sizeof h, hipMemcpyHostToDevice, stream));
  LT_HIP(hipStreamSynchronize(stream));
  return LT_OK;
}

int check_boundary(const lt_plan *p, const lt_boundary_desc &b) {
  switch (b.kind) {
    case LT_BOUNDARY_BOUNCE_BACK:
    case LT_BOUNDARY_EQUILIBRIUM:
      return LT_OK;
    case LT_BOUNDARY_ABB_OUTLET:
    case LT_BOUNDARY_PRESSURE_OUTLET: {
      const char *what = b.kind == LT_BOUNDARY_ABB_OUTLET ? "anti-bounce-back outlet" : "constant-pressure outlet";
      if (b.axis < 0 || b.axis >= p->unit.d || (b.side != 1 && b.side != -1))
        return fail(LT_ERR_INVALID, "%s: axis %d side %d", what, b.axis, b.side);
      if (p->desc.shape[b.axis] < 2)
        return fail(LT_ERR_INVALID, "%s needs >= 2 planes along its axis", what);
      if (p->desc.ghost_planes && b.axis == 2 && !(b.flags & LT_BOUNDARY_ABSENT) && p->desc.shape[2] < 2)
        return fail(LT_ERR_INVALID, "an outlet along the decomposed (z) axis needs >= 2 planes on its rank");
      return LT_OK;
    }
    case LT_BOUNDARY_LINK_BOUNCE_BACK:
      if (p->unit.d < 2 || p->desc.layout != LT_LAYOUT_REFERENCE || p->desc.ghost_planes)
        return fail(LT_ERR_UNSUPPORTED, "link bounce-back: 2-D / 3-D plans in the reference layout without ghost planes "
                                        "(no 1-D plan, no slab)");
      return LT_OK;
    default:
      return fail(LT_ERR_INVALID, "unknown boundary kind %d", b.kind);
  }
}

// populations whose velocity component along logical axis `logical_axis` equals `dir`
template <class S>
lt::QList crossing_of(int logical_axis, int dir) {
  lt::QList l;
  l.n = 0;
  for (int q = 0; q < S::Q; ++q)
    if (S::E[q][logical_axis] == dir && l.n < 9) l.q[l.n++] = q;
  return l;
}

// populations whose velocity component along MEMORY axis `mem_axis` equals `dir` (the axis maps are
// involutions: mem_axis_of also takes a memory axis to its logical one)
lt::QList crossing_axis(const lt_plan *p, int mem_axis, int dir) {
  const int axis = mem_axis_of(p, mem_axis);
  switch (p->desc.stencil) {
    case LT_D1Q3: return crossing_of<lt::D1Q3>(0, dir);
    case LT_D2Q9: return crossing_of<lt::D2Q9>(axis, dir);
    case LT_D3Q15: return crossing_of<lt::D3Q15>(axis, dir);
    case LT_D3Q19: return crossing_of<lt::D3Q19>(axis, dir);
    default: return crossing_of<lt::D3Q27>(axis, dir);
  }
}
// ... along the slowest memory axis, the one the sweeps run along and the slabs are cut along
lt::QList crossing(const lt_plan *p, int dir) { return crossing_axis(p, p->unit.d == 2 ? 1 : 2, dir); }

// a pack / unpack kernel of the plan's scalar type: launch(T(), std::bool_constant<PACK>()) for the dtype and the
// direction of the copy (PACK: field -> buffer)
template <class F>
void with_dtype_and_direction(const lt_plan *p, bool do_pack, F launch) {
  if (p->desc.dtype == LT_F32) {
    if (do_pack) launch(float(), std::true_type()); else launch(float(), std::false_type());
  } else {
    if (do_pack) launch(double(), std::true_type()); else launch(double(), std::false_type());
  }
}

int pack(lt_plan *p, bool do_pack, void *f, long long plane, int dir, void *buf, void *stream) {
  if (!p || !f || !buf) return fail(LT_ERR_INVALID, "null argument");
  if (dir != 1 && dir != -1) return fail(LT_ERR_INVALID, "direction %d (must be +1 or -1)", dir);
  if (plane < 0 || plane >= p->n2) return fail(LT_ERR_INVALID, "plane %lld outside [0, %d)", plane, p->n2);
  const lt::QList ql = crossing(p, dir);
  const int plane_nodes = p->n0 * p->n1;
  const long long off = plane * plane_nodes;
  const unsigned grid = (plane_nodes + lt::kThreads - 1) / lt::kThreads;
  hipStream_t s = static_cast<hipStream_t>(stream);
  with_dtype_and_direction(p, do_pack, [&](auto scalar, auto packs) {
    using T = decltype(scalar);
    hipLaunchKernelGGL((lt::plane_pack_kernel<T, decltype(packs)::value>), dim3(grid), dim3(lt::kThreads), 0, s, (T *)f,
                       (T *)buf, pop_stride_of(p), off, plane_nodes, ql);
  });
  LT_HIP(hipGetLastError());
  return LT_OK;
}

// Nontemporal accesses pay off when the two population buffers cannot stay in the caches
// (32 MiB L2 + 256 MiB Infinity Cache); small grids keep cached stores.
int resolve_tune(const lt_plan *p) {
  if (p->set.tune == 0 || p->set.tune == 3) return p->set.tune;
  const long long bytes = 2ll * p->unit.q * p->N * p->esize;
  return bytes > (128ll << 20) ? 3 : 0;
}

// Fewer resident waves stream better: with 19-27 read and as many write streams per workgroup,
// 3 workgroups per CU (3 waves per SIMD) instead of the 8 the registers allow ran 1-4 % faster on
// MI355X (tools/occupancy_probe.py: D3Q19 fp32 -1.3..-2.7 %, D3Q27 fp32 -1..-4 %, D3Q19 fp64
// -2..-4 %; 2 per CU is 15 % slower in fp32).  fp32 KBC, the one kernel with real arithmetic, gets 4.  The cap is an unused dynamic-LDS
// allocation (160 KB per CU).  Only for launches that fill the chip several times over and stream
// from HBM; small launches (boundary planes beside the interior launch, small grids) stay uncapped.
int resolve_lds(const lt_plan *p, long long workgroups) {
  int n = p->set.residency;
  if (n < 0) {
    const long long bytes = 2ll * p->unit.q * p->N * p->esize;
    const bool kbc32 = p->desc.collision == LT_COLLISION_KBC && p->esize == 4;
    n = (bytes > (128ll << 20) && workgroups >= 8192) ? (kbc32 ? 4 : 3) : 0;
  }
  if (n <= 0 || n >= 8) return 0;
  const int per_wg = ((int)lt::kLdsBudget / n) & ~2047;   // the LDS allocator rounds up: stay below 160 KB / n
  return per_wg > 65536 ? 65536 : per_wg;
}

// ---- engine-owned padded population buffers (lt_resident_*) ----
// Distance added between consecutive populations of the engine's own buffers.  The q read streams and q write
// streams of a node advance in lockstep; with the populations a power of two apart (256^3 fp32: exactly 64 MiB)
// they meet in the same memory channels.  Measured on MI355X (tools/pad_sweep_probe.py).
// Of the pads tried on five 3-D grids and three lattices (0, 128, 320, 2112, 2368, 32832 elements, three runs
// each) 32768 + 64 elements was the best or within a per cent of the best everywhere: two-step launch -7.0 % at
// 256^3 fp32 (populations exactly 64 MiB apart when dense), -2.3 % at 512 x 512 x 64, -5.1 % at 256 x 256 x 512,
// -4.9 % at 384^3, -5.2 % at 256^3 fp64, -3.9 % for D3Q15 (profiles/r03_pad_sweep_robust.jsonl).
long long default_pad() { return 32768 + 64; }
long long resident_stride(const lt_plan *p) {
  const long long pad = p->res_pad >= 0 ? p->res_pad : default_pad();
  const long long unit = 256 / p->esize;                      // keep every population 256-byte aligned
  return (p->N + pad + unit - 1) / unit * unit;
}
bool two_step_wanted(lt_plan *p);
bool resident_wanted(const lt_plan *p) {
  if (p->desc.ghost_planes || p->unit.d < 2) return false;
  if (p->resident >= 0) return p->resident != 0;
  // automatic: 3-D plans whose fused steps run as two-step launches (which implies the streaming regime).  The
  // one-step kernels stream best from DENSE populations (padding costs them 2-4 %: 256^3 D3Q19 fp32 0.411 ->
  // 0.42-0.44 ms) and D2Q9's two-step kernel gains nothing (4096^2: -2 % .. +4 %), so those keep the caller's buffers.
  return p->unit.d == 3 && two_step_wanted(const_cast<lt_plan *>(p));
}
int resident_alloc(lt_plan *p) {
  const long long stride = resident_stride(p);
  if (p->res[0] && p->res_stride == stride) return LT_OK;
  for (void *&r : p->res) { if (r) (void)hipFree(r); r = nullptr; }
  p->res_valid = 0;
  const size_t bytes = (size_t)stride * p->unit.q * p->esize;
  for (void *&r : p->res)
    if (hipMalloc(&r, bytes) != hipSuccess) {
      for (void *&x : p->res) { if (x) (void)hipFree(x); x = nullptr; }
      return fail(LT_ERR_ALLOC, "hipMalloc of the resident population buffers (2 x %zu bytes) failed", bytes);
    }
  p->res_stride = stride;
  return LT_OK;
}

// the tile of the plan's two-step launch (launch_limits.hpp); rows = 0: no kernel
using lt::TwoStepTile;
TwoStepTile two_step_tile(const lt_plan *p) {
  return lt::two_step_tile_on(p->unit.tile, p->unit.d, p->n0, p->set.masked != 0);
}

// Can the 3-D two-step kernel of the plan's kind address the grid (launch_limits.hpp)?  Asked BEFORE a plan is put on
// the two-step path, so that lt_run falls back to the one-step kernel instead of failing at the first launch (Obstacle
// D3Q19 fp32 at 384^3 is 4.0 GiB).  distance: elements between the populations of the widest buffer in use
bool two_step_addressable(const Unit &unit, int esize, long long n0, long long n1, long long distance, bool masked,
                          int layout, int collision) {
  if (unit.d != 3) return true;
  if (!masked) return lt::plane_addressable(n0, n1, esize);
  return lt::field_addressable(unit.q, distance, esize, lt::masked_per_population(layout, collision, unit.q));
}

// planes per workgroup of the two-step kernel.  One workgroup occupies a CU (150 KB of LDS), so the
// launch runs in rounds of n_cu workgroups; a segment of L planes computes L + 2 intermediate
// planes.  Pick the divisor L of n2 with the best (L / (L + 2)) * (blocks / blocks rounded up to
// whole rounds): 128 planes = 256 workgroups at 256^3 (measured 0.3345 ms per step against 0.3412
// with 32 planes and 0.52 with 256, which leaves half the CUs idle).
// `override` > 0: the launch's own segment length in place of the plan's (lt_plan_set_two_step).
int resolve_seg_len(const lt_plan *p, int planes, int override = 0) {
  const int asked = override > 0 ? override : p->seg_len;
  if (asked >= lt::min_segment(p->set.masked != 0)) return asked;
  const TwoStepTile tile = two_step_tile(p);
  if (tile.rows == 0) return 1;                  // no kernel: the unit's launcher says so
  long long tiles = (long long)(p->n0 / tile.width) * (p->n1 / tile.rows);
  long long cus = p->n_cu > 0 ? p->n_cu : 256;
  if (p->unit.d == 2) {
    // the sweep runs along a1.  Two workgroups would fit a CU in fp32 (27 row slots of width + 2 values =
    // 55 KB), but one per CU streams better: 4096^2 fp32 0.118 ms per update with 256 workgroups of 128 rows
    // against 0.159 with 512 of 64 (tools/two_step_2d_probe.py)
    tiles = p->n0 / tile.width;
  }
  int best = 1;
  double best_score = -1.0;
  for (int len = lt::min_segment(p->set.masked != 0); len <= planes; ++len) {
    const long long segs = (planes + len - 1) / len;
    if (!p->desc.ghost_planes && planes % len) continue;   // keep whole-grid launches evenly cut
    const long long blocks = tiles * segs;
    const long long rounds = (blocks + cus - 1) / cus;
    const double score = ((double)planes / (double)(planes + 2 * segs)) *
                         ((double)blocks / (double)(rounds * cus));
    if (score > best_score) { best_score = score; best = len; }
  }
  return best;
}

// Two-step slab halo: side -1 = lower cut, +1 = upper cut.  Packing reads the two interior planes
// next to the cut, unpacking fills the two ghost planes beyond it.
int halo2(lt_plan *p, bool do_pack, void *f, int side, void *buf, void *stream) {
  if (!p || !f || !buf) return fail(LT_ERR_INVALID, "null argument");
  if (side != 1 && side != -1) return fail(LT_ERR_INVALID, "side %d (must be +1 or -1)", side);
  if (p->desc.ghost_planes != 2) return fail(LT_ERR_INVALID, "the two-step halo needs ghost_planes = 2");
  const int g = 2, n2 = p->n2;
  long long near, far;
  int dir;
  if (do_pack) {     // what the neighbour beyond `side` needs: populations staying in / leaving through the cut
    near = side < 0 ? g : n2 - g - 1;
    far = side < 0 ? g + 1 : n2 - g - 2;
    dir = side;
  } else {           // what arrived from the neighbour beyond `side`: populations entering through the cut
    near = side < 0 ? g - 1 : n2 - g;
    far = side < 0 ? g - 2 : n2 - g + 1;
    dir = -side;
  }
  const lt::QList in_plane = crossing(p, 0), cross = crossing(p, dir);
  lt::QList away = crossing(p, -dir);
  if (!p->set.masked) away.n = 0;                      // only a no-streaming node ever reads them
  const int plane_nodes = p->n0 * p->n1;
  const unsigned grid = (plane_nodes + lt::kThreads - 1) / lt::kThreads;
  hipStream_t s = static_cast<hipStream_t>(stream);
  with_dtype_and_direction(p, do_pack, [&](auto scalar, auto packs) {
    using T = decltype(scalar);
    hipLaunchKernelGGL((lt::halo2_kernel<T, decltype(packs)::value>), dim3(grid), dim3(lt::kThreads), 0, s, (T *)f,
                       (T *)buf, pop_stride_of(p), near * plane_nodes, far * plane_nodes, plane_nodes, in_plane, cross, away);
  });
  LT_HIP(hipGetLastError());
  return LT_OK;
}

// Two updates per launch on a plan with boundaries (lbm2m_kernel, twostep_masked.hpp): bounce-back and
// equilibrium nodes anywhere; at most one anti-bounce-back outlet, either at the LAST plane of the sweep axis
// (memory axis a2, side +1 -- the reference's Obstacle in the reference layout), where its neighbour's moments
// and its no-streaming bits reduce to tests on the plane index, or at an end of the rows (memory axis a0 --
// the Obstacle in the slab layout), where the neighbour is the next lane and the face opposite the outlet
// must consist of equilibrium nodes; and no-streaming bits exactly where that outlet puts them (both checked
// on the device when the masks are compiled).  Anything else keeps the one-step kernel.
// Returns the memory axis of the outlet (2 without one), or -1: not admitted.
int masked_two_step_axis(const lt_plan *p) {
  if (!p->nsm_confined) return -1;
  if (p->desc.n_boundaries > lt::kMaskedTwoStepBoundaries) return -1;
  const int sweep = p->unit.d == 2 ? 1 : 2;          // the slowest memory axis
  if (p->unit.d < 2) return -1;
  int n_abb = 0, axis = 2;
  for (int i = 0; i < p->desc.n_boundaries; ++i) {
    const lt_boundary_desc &b = p->desc.boundaries[i];
    if (b.kind != LT_BOUNDARY_ABB_OUTLET || (b.flags & LT_BOUNDARY_ABSENT)) continue;
    if (++n_abb > 1) return -1;
    const int ax = mem_axis_of(p, b.axis);
    if (ax == sweep) {
      if (b.side != 1 || (sweep == 2 ? p->n2 : p->n1) < lt::kOutletSweepMin) return -1;
      axis = 2;                                      // "at the last plane / row of the sweep"
    } else if (ax == 0 && p->unit.d == 3) {
      if (!p->inlet_faces_outlet) return -1;
      axis = 0;
    } else {
      return -1;
    }
  }
  return axis;
}
bool masked_two_step_ok(const lt_plan *p) { return masked_two_step_axis(p) >= 0; }
bool canary_ok(lt_plan *p);
// the kernels' COLL of the plan (dispatch.hpp, kColl*): its collision, | kCollForce with a body force; MRT by its
// transform (Dellar and Hermite are told apart by the lattice)
int kernel_coll(const lt_plan *p) {
  if (p->desc.collision == LT_COLLISION_MRT)
    return p->set.mrt.transform == LT_MRT_D2Q9_LALLEMAND ? lt::kCollMrtLallemand : lt::kCollMrt;
  // the incompressible equilibrium: the collisions that evaluate feq get kernels of their own (no collision does not)
  const bool incompressible = p->set.equilibrium == LT_EQUILIBRIUM_INCOMPRESSIBLE && p->desc.collision != LT_COLLISION_NONE;
  // a force field: numbers of its own (it excludes the uniform force and the incompressible equilibrium)
  if (p->set.field.a) return p->desc.collision | lt::kCollForce | lt::kCollField;
  return p->desc.collision | (p->set.force.on ? lt::kCollForce : 0) | (incompressible ? lt::kCollIncompressible : 0);
}
static_assert(lt::kCollNone == LT_COLLISION_NONE && lt::kCollBgk == LT_COLLISION_BGK && lt::kCollKbc == LT_COLLISION_KBC &&
              lt::kCollSmagorinsky == LT_COLLISION_SMAGORINSKY && lt::kCollTrt == LT_COLLISION_TRT &&
              lt::kCollRegularized == LT_COLLISION_REGULARIZED && lt::kCollMrt == LT_COLLISION_MRT,
              "the kernels' collision numbers are the ABI's where the ABI has the operator");

// Zeroed kernel arguments with the fields set that choose the kernel of a launch of `mode` on this plan (unit.inc,
// dispatch): what step() launches with, and what every question "has the unit such a kernel" / "what is its name" is
// asked with, so that the answer is about the kernel the launch will take
lt::StepArgs kernel_selector(const lt_plan *p, int mode) {
  lt::StepArgs a;
  memset(&a, 0, sizeof a);
  const bool masked = p->set.masked != 0;
  a.layout = p->desc.layout; a.coll = kernel_coll(p); a.mode = mode;
  a.masked = p->set.masked;
  a.abb_depth = p->abb_depth;
  a.abb_axis = masked ? masked_two_step_axis(p) : 2;
  a.n_abb = masked ? p->n_abb : 0;
  a.n_pout = masked ? p->n_pout : 0;
  if (masked && p->n_abb == 1 && p->n_pout == 0)
    for (int i = 0; i < p->desc.n_boundaries; ++i) {
      const lt_boundary_desc &b = p->desc.boundaries[i];
      if (b.kind == LT_BOUNDARY_ABB_OUTLET && !(b.flags & LT_BOUNDARY_ABSENT) && mem_axis_of(p, b.axis) == 0)
        a.abb0_slot = i + 1;
    }
  a.strip = p->unit.d == 2 ? two_step_tile(p).width : 0;
  a.shift = p->set.shift;                              // workgroup-order A/B variant of the two-step sweeps
  a.tune = resolve_tune(p);
  return a;
}

// ---- which plans have a launch of several steps ----
const char *const kForceMultiStep = "a body force (lt_plan_set_force) has the one-step kernels and the plain two-step sweep "
                                    "of periodic D3Q19 fp32 plans without masks only: no many-step, 2-D, masked, role-wave "
                                    "or slab two-step kernel takes it";
const char *const kForceSmagorinskyTwice = "Smagorinsky with a body force (lt_plan_set_force) does not fit the two-step "
                                           "sweep's occupancy step without scratch: it keeps the one-step kernel";
const char *const kForceFieldMultiStep = "a per-node force field (lt_plan_set_force_field) has the one-step kernels only: no "
                                         "two-step or many-step kernel takes it";
const char *const kTrtMultiStep = "the TRT collision has the one-step kernels and the plain two-step sweep of periodic D3Q19 "
                                  "fp32 plans without masks only: no many-step, 2-D, masked, role-wave, edge, packed or "
                                  "signalling two-step kernel takes it";
const char *const kRegularizedMultiStep = "the regularised collision has the one-step kernels and the plain two-step sweep "
                                          "of periodic D3Q19 fp32 plans without masks only: no many-step, 2-D, masked, "
                                          "role-wave, edge, packed or signalling two-step kernel takes it";
// (refused by name, not through the admission tests of the masked two-step kernels, which were written for the
// anti-bounce-back outlet's no-streaming bits)
const char *const kPressureOutletMultiStep = "a constant-pressure outlet (EquilibriumOutletP) has the one-step kernels only: "
                                             "no masked two-step, 2-D two-step, many-step or two-ghost-plane slab kernel "
                                             "takes it";
const char *const kMrtMultiStep = "the MRT collision has the one-step kernels only: no two-step, many-step or "
                                  "two-ghost-plane slab kernel takes it";
const char *const kIncompressibleMultiStep = "the incompressible equilibrium (lt_plan_set_equilibrium) has the one-step kernels "
                                             "only: no two-step or many-step kernel takes it";
const char *const kSmagorinskySlabs = "the Smagorinsky collision has the plain two-step sweep of periodic plans only (no "
                                      "edge, packed or signalling launches): slabs keep the one-step kernels";
// (said with "with" in front of it, like the next one: "two steps per launch with link bounce-back ...")
const char *const kLinkMultiStep = "link bounce-back (lt_plan_set_links): the pass over the links follows every one-step "
                                   "launch over the whole field; no two-step, many-step or plane-range launch takes it";
// (step() says "two steps per launch with" in front of it, the admission "two steps per launch: ")
const char *const kMaskedTwoStep = "boundaries: at most one anti-bounce-back outlet, at the last plane of the slowest memory "
                                   "axis (periodic plans only) or at an end of the contiguous axis opposite a face of "
                                   "equilibrium nodes; no-streaming bits exactly that outlet's";

// Why the plan has no launch of `mode` (kFusedTwice, kFusedMany; nullptr for any other), or nullptr: its collision and
// its kinds of boundary allow one.  The one place that keeps a collision or a boundary kind from the launches of several
// steps: step(), two_step_possible() and many_step_wanted() ask here, the first reason wins.  What depends on the grid
// -- tiling, addressing, the unit's kernels, the canary -- stays with those.
const char *multi_step_refusal(const lt_plan *p, int mode) {
  if (mode != lt::kFusedTwice && mode != lt::kFusedMany) return nullptr;
  const bool twice = mode == lt::kFusedTwice;
  if (p->n_link_kind > 0) return kLinkMultiStep;                       // the one-step kernels and the pass behind them
  // what a body force, TRT and the regularised collision have beside the one-step kernels (unit.inc, parts forced and
  // relaxations): the plain two-step sweep of periodic D3Q19 fp32 plans without masks
  const bool plain_sweep = twice && p->unit.d == 3 && !p->set.masked && !p->desc.ghost_planes && p->desc.stencil == LT_D3Q19 &&
                           p->desc.dtype == LT_F32;
  if (p->set.equilibrium == LT_EQUILIBRIUM_INCOMPRESSIBLE) return kIncompressibleMultiStep;   // (unit.inc, part incompressible)
  if (p->set.field.a) return kForceFieldMultiStep;                     // (unit.inc, part force_field)
  if (p->set.force.on) {
    if (!plain_sweep) return kForceMultiStep;
    if (!has_kernel(p->unit, kernel_selector(p, lt::kFusedTwice))) return p->desc.collision == LT_COLLISION_SMAGORINSKY ? kForceSmagorinskyTwice : kForceMultiStep;
  }
  if (p->desc.collision == LT_COLLISION_TRT && !plain_sweep) return kTrtMultiStep;
  if (p->desc.collision == LT_COLLISION_REGULARIZED && !plain_sweep) return kRegularizedMultiStep;
  if (p->n_pout > 0) return kPressureOutletMultiStep;                  // the one-step kernels only (unit.inc, part outlets)
  if (p->desc.collision == LT_COLLISION_MRT) return kMrtMultiStep;     // the one-step kernels only (unit.inc, part mrt)
  if (twice && p->desc.ghost_planes && p->desc.collision == LT_COLLISION_SMAGORINSKY) return kSmagorinskySlabs;
  // masks: their admission, and on a slab an outlet only along the rows
  if (twice && p->set.masked && (!masked_two_step_ok(p) || (p->desc.ghost_planes && p->n_abb > 0 && masked_two_step_axis(p) != 0)))
    return kMaskedTwoStep;
  return nullptr;
}

// ---- link bounce-back ----
// has every boundary of that kind its list?  (LT_OK, or the error that names the first without)
int links_ready(const lt_plan *p) {
  for (int i = 0; i < p->desc.n_boundaries; ++i)
    if (p->desc.boundaries[i].kind == LT_BOUNDARY_LINK_BOUNCE_BACK && !p->links[i].set)
      return fail(LT_ERR_INVALID, "boundary %d is link bounce-back: lt_plan_set_links must give its links first", i);
  return LT_OK;
}

lt::LinkArgs link_args(const lt_plan *p, const lt_plan::Links &l, lt::LinkKind what, void *f, long long stride, void *stream) {
  lt::LinkArgs a;
  memset(&a, 0, sizeof a);
  a.what = what; a.f = f; a.stride = stride;
  a.node = l.node; a.dir = l.dir; a.c1 = l.c1; a.c2 = l.c2; a.second = l.second; a.n_links = l.n;
  a.n0 = p->n0; a.n1 = p->n1; a.n2 = p->n2;
  a.stream = static_cast<hipStream_t>(stream);
  return a;
}

// The pass over every list of the plan, in place on the post-collision populations f (`stride` elements between its
// populations), in index order of the boundaries; an empty list launches nothing
int apply_links(const lt_plan *p, void *f, long long stride, void *stream) {
  const LinkFn fn = kLinkUnits[2 * p->desc.stencil + p->desc.dtype];
  for (int i = 0; i < p->desc.n_boundaries; ++i) {
    const lt_plan::Links &l = p->links[i];
    if (p->desc.boundaries[i].kind != LT_BOUNDARY_LINK_BOUNCE_BACK || l.n < 1) continue;
    const int r = fn ? fn(link_args(p, l, lt::kLinkBounce, f, stride, stream)) : lt::kNoKernel;
    if (const int rc = launched(r, "no link kernel for this lattice")) return rc;
  }
  return LT_OK;
}

void free_links(lt_plan::Links &l) {
  if (l.node) (void)hipFree(l.node);
  if (l.dir) (void)hipFree(l.dir);
  if (l.second) (void)hipFree(l.second);
  if (l.c1) (void)hipFree(l.c1);
  if (l.c2) (void)hipFree(l.c2);
  l = lt_plan::Links();
}

// One call of step(): what belongs to the launch and not to the plan.  Every entry point builds its own and hands it
// over; step() keeps nothing of it in the plan.
struct Launch {
  int mode;
  const void *in;
  void *out;
  double tau;
  long long begin, end;                          // a2 planes [begin, end) ...
  void *stream;
  long long stride = 1;                          // ... every stride-th of them
  void *pack_lo = nullptr, *pack_hi = nullptr;   // halo messages the launch writes (or null)
  long long begin2 = 0, end2 = 0;                // kFusedTwice: second plane range (a slab's other edge)
  int many = 1;                                  // kFusedMany: steps of the launch
  int seg_len = 0;                               // kFusedTwice: planes per workgroup; 0 = the plan's (resolve_seg_len)
  unsigned long long *signal = nullptr;          // counter the edge workgroups of the signalling slab launch add to
  const void *ghost_lo = nullptr, *ghost_hi = nullptr;   // received halo messages the direct edge launch reads
  long long stride_in = -1, stride_out = -1;     // elements between the populations of in / out; < 0: the plan's pop_stride
  bool canary = false;                           // a launch of the first-use check itself (run_canary): no check of its own
  Launch(int mode_, const void *in_, void *out_, double tau_, long long begin_, long long end_, void *stream_)
      : mode(mode_), in(in_), out(out_), tau(tau_), begin(begin_), end(end_), stream(stream_) {}
};

int step(lt_plan *p, const Launch &l) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  const int mode = l.mode;
  const long long pb = l.begin, pe = l.end, stride = l.stride;
  const double tau = l.tau;
  if (!l.in || !l.out) return fail(LT_ERR_INVALID, "null population buffer");
  if (l.in == l.out) return fail(LT_ERR_INVALID, "in-place operation is not supported (in == out)");
  if (pb < 0 || pe > p->n2 || pb > pe)
    return fail(LT_ERR_INVALID, "plane range [%lld, %lld) outside [0, %d)", pb, pe, p->n2);
  if (p->desc.ghost_planes && (pb < 1 || pe > p->n2 - 1) && mode != lt::kCollideOnly && pe > pb)
    return fail(LT_ERR_INVALID, "streaming from ghost planes: range [%lld, %lld) must stay in [1, %d)",
                pb, pe, p->n2 - 1);
  // the plan has no such launch (its two reasons about slabs and masks: behind the checks of the call's range below)
  const char *const why = multi_step_refusal(p, mode);
  const bool after_range = why == kSmagorinskySlabs || why == kMaskedTwoStep;
  const auto refuse = [&] {
    return fail(LT_ERR_UNSUPPORTED, why == kMaskedTwoStep || why == kLinkMultiStep ? "%s per launch with %s" : "%s per launch: %s",
                mode == lt::kFusedMany ? "several steps" : "two steps", why);
  };
  if (why && !after_range) return refuse();
  const bool mrt = p->desc.collision == LT_COLLISION_MRT;
  if (mrt && mode != lt::kStreamOnly && p->set.mrt.transform == 0)
    return fail(LT_ERR_INVALID, "the plan's collision is MRT: lt_plan_set_mrt must give the transform and the rates first");
  if (mode == lt::kFusedMany && (p->desc.ghost_planes || (p->set.masked && p->n_abb > 1)))
    return fail(LT_ERR_UNSUPPORTED, "several steps per launch: no slabs, at most one anti-bounce-back outlet");
  if (mode == lt::kFusedTwice) {
    if (p->desc.ghost_planes == 1)
      return fail(LT_ERR_INVALID, "two steps per launch read two planes beyond the range: the plan needs "
                                  "ghost_planes = 2");
    if (p->desc.ghost_planes == 2 && (pb < 2 || pe > p->n2 - 2) && pe > pb)
      return fail(LT_ERR_INVALID, "two-step range [%lld, %lld) must stay in [2, %d)", pb, pe, p->n2 - 2);
    if (!p->desc.ghost_planes && (pb != 0 || pe != p->n2))
      return fail(LT_ERR_INVALID, "periodic plan: the two-step launch covers all planes");
    if (why) return refuse();
    if (p->set.masked && !l.canary && !canary_ok(p)) return fail(LT_ERR_UNSUPPORTED, "%s", p->canary_msg);
  }
  if (p->desc.n_boundaries > 0 && !p->set.masked)
    return fail(LT_ERR_INVALID, "plan has boundaries but lt_plan_set_masks was not called");
  // link bounce-back: the pass follows a launch that leaves post-collision populations, over the whole field
  const bool links = p->n_link_kind > 0 && (mode == lt::kCollideOnly || mode == lt::kFused);
  if (links) {
    if (pb != 0 || pe != p->n2 || stride != 1)
      return fail(LT_ERR_UNSUPPORTED, "a range of planes per launch with %s", kLinkMultiStep);
    if (const int rc = links_ready(p)) return rc;
  }
  if (mode != lt::kStreamOnly && p->desc.collision != LT_COLLISION_NONE && !mrt && !(tau > 0.0))
    return fail(LT_ERR_INVALID, "relaxation time tau = %g", tau);
  lt::StepArgs a = kernel_selector(p, mode);
  a.in = l.in; a.out = l.out;
  a.n0 = p->n0; a.n1 = p->n1; a.n2 = p->n2;
  a.p_begin = (int)pb; a.planes = (int)((pe - pb + stride - 1) / stride); a.p_stride = (int)stride;
  a.wrap2 = p->desc.ghost_planes ? 0 : 1;
  a.tau = tau > 0.0 ? tau : 1.0;
  p->set.fill(a);
  a.node = p->node; a.nsm_bits = p->nsm_bits; a.bt = p->bt; a.nb = p->desc.n_boundaries;
  a.lds_bytes = resolve_lds(p, ((long long)a.planes * a.n1 * a.n0 + 255) / 256);
  if (mode == lt::kFusedTwice) a.seg_len = resolve_seg_len(p, p->unit.d == 2 ? p->n1 : a.planes, l.seg_len);
  if (mode == lt::kFusedMany) a.seg_len = l.many;
  a.stream = static_cast<hipStream_t>(l.stream);
  a.stride_in = l.stride_in >= 0 ? l.stride_in : p->pop_stride;
  a.stride_out = l.stride_out >= 0 ? l.stride_out : p->pop_stride;
  a.pack_lo = l.pack_lo; a.pack_hi = l.pack_hi;
  a.signal = l.signal;
  a.ghost_lo = l.ghost_lo; a.ghost_hi = l.ghost_hi;
  a.interior_begin = p->interior_begin; a.interior_end = p->interior_end;
  a.pack_lo_plane = (int)pb; a.pack_hi_plane = (int)(pb + stride * (a.planes - 1));
  if (mode == lt::kFusedTwice) {
    a.p_begin2 = (int)l.begin2;
    a.planes2 = (int)(l.end2 - l.begin2);
    if (a.planes2 > 0) a.pack_hi_plane = (int)l.end2 - 1;   // upper message: last plane of the second range
  }
  if (const int rc = launched(p->unit.step(a), "no kernel for layout %d collision %d mode %d masked %d", a.layout, a.coll,
                              a.mode, a.masked))
    return rc;
  if (links) return apply_links(p, l.out, a.stride_out > 0 ? a.stride_out : p->N, l.stream);
  return LT_OK;
}

constexpr int kGraphChunk = 32;            // fused steps per graph (even: ends in the start buffer)

// Measured on MI355X (profiles/r01_small_grid_graph.jsonl): the eager C loop of lt_run already
// runs at 3.5 us per step on 128^2 (dependent-kernel boundary ~1.5 us + kernel), and graph replay
// was slower on three of four small grids (4.1 vs 3.5 us at 128^2; 4.6 vs 5.1 us at 256^2), so
// "automatic" currently means eager; the graph path stays available with mode 1.
bool graph_wanted(const lt_plan *p, long long fused) {
  if (fused < 2 * kGraphChunk) return false;
  return p->graph_mode == 1;
}

// Replays floor(fused / kGraphChunk) chunks of fused steps starting (and ending) in `cur`; returns
// the number of steps done through the graph, or a negative status on failure.
long long run_graph(lt_plan *p, void *cur, void *other, double tau, long long fused, void *stream) {
  hipStream_t user = static_cast<hipStream_t>(stream);
  if (!p->gstream) {
    if (hipStreamCreateWithFlags(&p->gstream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&p->gev_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&p->gev_out, hipEventDisableTiming) != hipSuccess)
      return -fail(LT_ERR_HIP, "cannot create the graph stream/events");
  }
  const bool same = p->gexec && p->gkey.a == cur && p->gkey.b == other && p->gkey.tau == tau && p->gkey.set == p->set;
  if (!same) {
    if (p->gexec) { (void)hipGraphExecDestroy(p->gexec); p->gexec = nullptr; }
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(p->gstream, hipStreamCaptureModeThreadLocal) != hipSuccess)
      return -fail(LT_ERR_HIP, "hipStreamBeginCapture failed");
    void *c = cur, *o = other;
    int rc = LT_OK;
    for (int i = 0; i < kGraphChunk && rc == LT_OK; ++i) {
      rc = step(p, Launch(lt::kFused, c, o, tau, 0, p->n2, p->gstream));
      void *t = c; c = o; o = t;
    }
    const hipError_t e = hipStreamEndCapture(p->gstream, &graph);
    if (rc != LT_OK) { if (graph) (void)hipGraphDestroy(graph); return -rc; }
    if (e != hipSuccess || !graph) return -fail(LT_ERR_HIP, "hipStreamEndCapture failed");
    const hipError_t ei = hipGraphInstantiate(&p->gexec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ei != hipSuccess) { p->gexec = nullptr; return -fail(LT_ERR_HIP, "hipGraphInstantiate failed"); }
    p->gkey = {cur, other, tau, p->set};
  }
  const long long reps = fused / kGraphChunk;
  if (hipEventRecord(p->gev_in, user) != hipSuccess ||
      hipStreamWaitEvent(p->gstream, p->gev_in, 0) != hipSuccess)
    return -fail(LT_ERR_HIP, "fork to the graph stream failed");
  for (long long r = 0; r < reps; ++r)
    if (hipGraphLaunch(p->gexec, p->gstream) != hipSuccess)
      return -fail(LT_ERR_HIP, "hipGraphLaunch failed");
  if (hipEventRecord(p->gev_out, p->gstream) != hipSuccess ||
      hipStreamWaitEvent(user, p->gev_out, 0) != hipSuccess)
    return -fail(LT_ERR_HIP, "join from the graph stream failed");
  return reps * kGraphChunk;
}

// Is there a two-step launch for this plan?  Needs the kernel for this lattice / dtype / collision (asked of
// the unit by name), a grid that tiles (a0 % 64, a1 % 8) and, with masks, their admission
// (masked_two_step_axis).  why != nullptr: the reason it is not.
bool two_step_possible(lt_plan *p, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  if (const char *refused = multi_step_refusal(p, lt::kFusedTwice)) {
    *why = refused;
    return false;
  }
  if (!lt::tiles(two_step_tile(p), p->n0, p->n1)) {
    *why = "the grid does not tile (contiguous extent % 64 (fp32) / 32 (fp64), middle extent % 8 or 4)";
    return false;
  }
  // with masks the whole (padded) field is addressed with 32-bit offsets
  const long long widest = std::max({p->N, pop_stride_of(p), p->resident != 0 ? resident_stride(p) : 0ll});
  if (!two_step_addressable(p->unit, p->esize, p->n0, p->n1, widest, p->set.masked != 0, p->desc.layout, p->desc.collision)) {
    *why = p->set.masked ? "with boundaries the two-step kernel addresses with 32-bit offsets: q * nodes * sizeof(scalar) (BGK, "
                       "reference layout: nodes * sizeof(scalar)) must stay below 4 GiB"
                     : "a plane of the grid exceeds the two-step kernel's 32-bit in-plane offsets";
    return false;
  }
  if (!has_kernel(p->unit, kernel_selector(p, lt::kFusedTwice))) {
    *why = "no two-step kernel for this lattice / dtype / collision";
    return false;
  }
  // with boundaries: the kernel is held against two one-step launches once per plan and set of masks (run_canary)
  if (p->set.masked && !canary_ok(p)) {
    *why = p->canary_msg;
    return false;
  }
  return true;
}

// The plans whose two-step launch lt_run takes only when asked (lt_plan_set_two_step(plan, 1, ...)), never by itself
bool two_step_never_automatic(const lt_plan *p) {
  // KBC inside the masked two-step kernel agrees with the one-step kernel at rounding level only (hipcc contracts
  // its multiply-adds differently in the two inlining contexts): never automatic, so that the result of n steps
  // does not depend on how the caller splits them into batches
  if (p->desc.collision == LT_COLLISION_KBC) return true;
  // a body force: never automatic (the forced two-step sweep has not been measured against two one-step launches,
  // DESIGN.md section 7)
  if (p->set.force.on) return true;
  // TRT, regularised: never automatic either, for the same reason
  if (p->desc.collision == LT_COLLISION_TRT || p->desc.collision == LT_COLLISION_REGULARIZED) return true;
  // MRT has no two-step kernel
  // (Smagorinsky, D3Q19 fp32: bit-identical to two one-step launches and 0.279-0.309 against 0.409-0.475 ms per
  // update at 256^3, every sample below every sample of the one-step pair: automatic like BGK)
  return p->desc.collision == LT_COLLISION_MRT;
}

// Does lt_run pair its fused steps?  "automatic" also asks for the streaming regime (populations beyond the
// caches), where halving the HBM passes pays.
bool two_step_wanted(lt_plan *p) {
  if (p->two_step == 0 || p->desc.ghost_planes) return false;
  if (!two_step_possible(p, nullptr)) return false;
  if (p->two_step == 1) return true;
  if (two_step_never_automatic(p)) return false;
  const long long bytes = 2ll * p->unit.q * p->N * p->esize;
  return bytes > (128ll << 20);
}

// ---- first-use canary of the masked two-step kernels -----------------------------------------------------------
// The boundary dispatch of these kernels is the code hipcc has miscompiled before (Makefile header, DESIGN.md
// section 6: a register copy dropped at the join of the equilibrium branch -- wrong populations on inlet / outlet
// nodes of one instantiation, right everywhere else, and different from build to build).  The build no longer runs
// the pass at fault, but a green test on one compiler build does not protect the next one: the FIRST time a plan
// with masks is about to use a two-step kernel, one double step over all its planes is held against two one-step
// launches -- synthetic populations on scratch buffers, the plan's own masks, boundary table, tile and segment
// length, bit-for-bit comparison on the device.  A mismatch (or scratch memory that cannot be had) keeps the plan on
// the one-step kernel: two_step_possible() then says why, lt_run falls back by itself and leaves the reason in
// lt_last_error(), the explicit two-step entry points fail with it.  Run again after lt_plan_set_masks and after a
// change of the segment length or tile variant.  Costs four scratch fields and five launches, once.
// Reference semantics being protected: lettuce/_simulation.py:177-189 (collision, then the boundaries in index order).
void canary_verdict(lt_plan *p, int verdict, long long mismatches, const char *fmt, ...) {
  p->canary = verdict;
  p->canary_mismatches = mismatches;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(p->canary_msg, sizeof p->canary_msg, fmt, ap);
  va_end(ap);
  if (verdict < 0) snprintf(g_error, sizeof g_error, "%s", p->canary_msg);
}

template <typename T, typename U>
void run_canary(lt_plan *p) {
  const int g = p->desc.ghost_planes;
  if (g == 1) { canary_verdict(p, 2, 0, "no two-step launch on a plan with one ghost plane"); return; }
  if (!p->cstream && hipStreamCreateWithFlags(&p->cstream, hipStreamNonBlocking) != hipSuccess) {
    canary_verdict(p, -1, 0, "two steps per launch with boundaries: cannot create the canary's stream; the plan keeps "
                             "the one-step kernel");
    return;
  }
  const size_t bytes = (size_t)p->unit.q * p->N * p->esize;
  void *buf[4] = {nullptr, nullptr, nullptr, nullptr};
  unsigned long long *count = nullptr;
  bool ok = hipMalloc((void **)&count, sizeof *count) == hipSuccess;
  for (void *&b : buf) ok = ok && hipMalloc(&b, bytes) == hipSuccess;
  auto release = [&]() { for (void *b : buf) if (b) (void)hipFree(b); if (count) (void)hipFree(count); };
  if (!ok) {
    release();
    canary_verdict(p, -1, 0, "two steps per launch with boundaries: no memory for the first-use check (4 x %zu "
                             "bytes); the plan keeps the one-step kernel", bytes);
    return;
  }
  char saved_error[sizeof g_error];
  memcpy(saved_error, g_error, sizeof g_error);
  const double tau = 0.8;
  const long long b1 = g ? 1 : 0, e1 = g ? p->n2 - 1 : p->n2, b2 = g, e2 = p->n2 - g;
  hipLaunchKernelGGL((canary_fill_kernel<T>), dim3(1024), dim3(256), 0, p->cstream, (T *)buf[0], p->N, p->N, p->unit.q);
  if (g) for (int i = 1; i < 4; ++i) (void)hipMemsetAsync(buf[i], 0, bytes, p->cstream);   // planes a slab launch never writes
  (void)hipMemsetAsync(count, 0, sizeof *count, p->cstream);
  // the plan as the caller set it up -- masks, boundary table, tile, its own segment length -- on dense scratch buffers;
  // whichever entry point came first, these are the three launches
  const auto check_launch = [&](int mode, int from, int to, long long begin, long long end) {
    Launch l(mode, buf[from], buf[to], tau, begin, end, p->cstream);
    l.stride_in = l.stride_out = p->N;
    l.canary = true;
    return step(p, l);
  };
  int rc = check_launch(lt::kFused, 0, 1, b1, e1);
  if (rc == LT_OK) rc = check_launch(lt::kFused, 1, 2, b2, e2);
  if (rc == LT_OK) rc = check_launch(lt::kFusedTwice, 0, 3, b2, e2);
  unsigned long long bad = 0;
  hipError_t e = hipSuccess;
  if (rc == LT_OK) {
    const long long plane = (long long)p->n0 * p->n1;
    hipLaunchKernelGGL((canary_compare_kernel<U>), dim3(1024), dim3(256), 0, p->cstream, (const U *)buf[2],
                       (const U *)buf[3], p->N, plane * b2, plane * (e2 - b2), p->unit.q, count);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, count, sizeof bad, hipMemcpyDeviceToHost, p->cstream);
  }
  const hipError_t es = hipStreamSynchronize(p->cstream);
  if (e == hipSuccess) e = es;
  release();
  if (rc != LT_OK) {
    char why[sizeof g_error];
    memcpy(why, g_error, sizeof why);
    canary_verdict(p, -1, 0, "two steps per launch with boundaries: the first-use check could not run (%.160s); the "
                             "plan keeps the one-step kernel", why);
  } else if (e != hipSuccess) {
    canary_verdict(p, -1, 0, "two steps per launch with boundaries: the first-use check failed with a HIP error (%s); "
                             "the plan keeps the one-step kernel", hipGetErrorString(e));
  } else if (bad != 0) {
    canary_verdict(p, -1, (long long)bad, "two steps per launch with boundaries: the two-step kernel disagrees with two "
                   "one-step launches in %llu of %lld populations (first-use check on this plan's masks); the plan "
                   "keeps the one-step kernel", bad, (long long)p->unit.q * p->n0 * p->n1 * (e2 - b2));
  } else {
    memcpy(g_error, saved_error, sizeof g_error);
    canary_verdict(p, 1, 0, "");
  }
}

// may this plan's masked two-step kernel be used?  Runs the check if it has not been run for the present masks
bool canary_ok(lt_plan *p) {
  if (!p->set.masked) return true;
  if (p->canary == 0) {
    if (p->canary_mode == 0) canary_verdict(p, 2, 0, "");
    else if (p->canary_mode == 2)
      canary_verdict(p, -1, -1, "two steps per launch with boundaries: first-use check forced to fail "
                                "(lt_plan_set_canary(plan, 2)); the plan keeps the one-step kernel");
    else if (p->esize == 4) run_canary<float, unsigned>(p);
    else run_canary<double, unsigned long long>(p);
  }
  return p->canary > 0;
}

// steps per many-step launch (launch_limits.hpp).  3-D plans have no many-step kernel (lt_stream_collide_many:
// LT_ERR_UNSUPPORTED); their range stays the removed kernel's two
int many_max(const lt_plan *p) { return p->unit.d == 3 ? 2 : lt::many_steps_max(p->set.masked && p->n_abb > 0); }

// Several steps per launch (lbm_many_kernel): 2-D, tiles of 8 x 8, with masks at most one outlet.  Every
// workgroup recomputes a halo of K - 1 nodes around its tile (K with an outlet), so this only pays while the
// grid is launch-bound; "automatic" stops at 256 x 256 nodes, 256 x 128 with masks (measured,
// tools/small_grid_bench.py, tools/small_masked_bench.py).
// 3-D: none.  A kernel with two steps per launch for small 3-D grids (removed) measured slower than one
// launch per step on every grid (tools/small_grid_bench.py, D3Q19 fp32, us per step: 16^3 3.66 -> 4.29, 32^3 4.21 ->
// 5.79, 48^3 6.5 -> 7.9, 64^3 8.3 -> 15.4): two steps amortise one launch gap (~2 us) but the launch is a chain of two
// dependent gather -> collide phases with a barrier in between, on 1000-thread workgroups that gather 10-node rows; the
// 2-D kernel wins because it amortises EIGHT steps per launch, which the LDS does not allow in 3-D (K = 3 needs the
// 12^3 neighbourhood: 131 KB for D3Q19 fp32 and 3.4 x the arithmetic).
bool many_step_wanted(lt_plan *p) {
  if (p->many == 0 || p->desc.ghost_planes || p->unit.d != 2 || multi_step_refusal(p, lt::kFusedMany) != nullptr) return false;
  if (p->set.masked && p->n_abb > 1) return false;
  if (p->n0 % lt::kManyTile != 0 || p->n1 % lt::kManyTile != 0) return false;
  if (!has_kernel(p->unit, kernel_selector(p, lt::kFusedMany))) return false;
  if (p->many == 1) return true;
  // automatic only where the many-step kernel is bit-identical to the one-step kernel, so that the
  // result of n steps does not depend on how the caller splits them into batches (KBC agrees at
  // rounding level only)
  if (p->desc.collision == LT_COLLISION_KBC) return false;
  // with masks the launch is bound by its own latency chain (node byte, boundary values, a barrier per step) and
  // recomputes a wider ring: 128 x 64 nodes 4.2 -> 2.4 us per step, 128 x 128 4.3 -> 2.5, 256 x 128 4.5 -> 3.3,
  // 256 x 256 5.6 -> 5.7 (tools/small_masked_bench.py, fp64)
  if (p->set.masked) return p->N <= 256ll * 128ll;
  return p->N <= 256ll * 256ll;
}

// `fused` stream-collide steps starting from the post-collision populations in *cur, ping-ponging with *other (both
// pointers are updated: on return *cur holds the result): pairs of steps through the two-step kernel where it
// applies, the rest one by one; several steps per launch on small 2-D grids.  The optional events bracket the
// dominant kind of launch only.  `stride`: elements between consecutive populations of the two buffers, negative for the
// caller's own (the plan's pop_stride), which alone may go through a captured graph.
int fused_section(lt_plan *p, void *&cur, void *&other, double tau, long long fused, void *stream, long long stride = -1) {
  int rc;
  const auto advance = [&](int mode, int many = 1) {
    Launch l(mode, cur, other, tau, 0, p->n2, stream);
    l.many = many;
    l.stride_in = l.stride_out = stride;
    const int status = step(p, l);
    if (status == LT_OK) std::swap(cur, other);
    return status;
  };
  if (graph_wanted(p, fused) && stride < 0) {
    const long long done = run_graph(p, cur, other, tau, fused, stream);
    if (done < 0) return (int)-done;
    fused -= done;                       // an even number of steps: still in `cur`
  }
  hipStream_t hs = static_cast<hipStream_t>(stream);
  p->last_many = 0;
  if (many_step_wanted(p) && fused >= 2) {
    // launches of up to kManyMax steps each; the events bracket them
    if (p->ev_start) (void)hipEventRecord(p->ev_start, hs);
    while (fused > 0) {
      const int steps = fused < many_max(p) ? (int)fused : many_max(p);
      rc = advance(lt::kFusedMany, steps);
      if (rc) return rc;
      fused -= steps;
      ++p->last_many;
    }
    if (p->ev_stop) (void)hipEventRecord(p->ev_stop, hs);
    p->last_twice = 0;
    p->last_single = 0;
    return LT_OK;
  }
  const long long twice = two_step_wanted(p) ? fused / 2 : 0;
  const long long single = fused - 2 * twice;
  p->last_twice = twice; p->last_single = single;
  if (p->ev_start && twice > 0) (void)hipEventRecord(p->ev_start, hs);
  for (long long i = 0; i < twice; ++i) {
    rc = advance(lt::kFusedTwice);
    if (rc) return rc;
  }
  if (p->ev_stop && twice > 0) (void)hipEventRecord(p->ev_stop, hs);
  if (p->ev_start && twice == 0) (void)hipEventRecord(p->ev_start, hs);
  for (long long i = 0; i < single; ++i) {
    rc = advance(lt::kFused);
    if (rc) return rc;
  }
  if (p->ev_stop && twice == 0) (void)hipEventRecord(p->ev_stop, hs);
  return LT_OK;
}

int run(lt_plan *p, bool from_fstar, void *a, void *b, double tau, long long n, void *stream,
        int32_t *result_in_b) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (n < 1) return fail(LT_ERR_INVALID, "n_steps = %lld", n);
  if (!result_in_b) return fail(LT_ERR_INVALID, "null result_in_b");
  if (p->desc.ghost_planes)
    return fail(LT_ERR_UNSUPPORTED, "lt_run/lt_continue need a periodic plan (no ghost planes); "
                                    "drive slabs with the *_planes entry points");
  void *cur = a, *other = b;
  int rc;
  long long fused = n;
  if (!from_fstar) {
    rc = step(p, Launch(lt::kCollideOnly, cur, other, tau, 0, p->n2, stream));
    if (rc) return rc;
    void *t = cur; cur = other; other = t;
    fused = n - 1;
  }
  rc = fused_section(p, cur, other, tau, fused, stream);
  if (rc) return rc;
  if (p->defer_stream) {               // the caller streams when somebody wants to see the populations
    *result_in_b = (cur == b) ? 1 : 0;
    return LT_OK;
  }
  rc = step(p, Launch(lt::kStreamOnly, cur, other, tau, 0, p->n2, stream));
  if (rc) return rc;
  *result_in_b = (other == b) ? 1 : 0;
  return LT_OK;
}

// An auxiliary launch starts from the fields the plan decides: layout, N, extents, stride, the interior planes' node
// range, the plan's scratch, equilibrium, stream.  The entry point then sets what is its own by name.  (A null plan
// leaves them zero: aux() refuses it.)
lt::AuxArgs aux_args(const lt_plan *p, lt::AuxKind what, void *stream) {
  lt::AuxArgs a;
  memset(&a, 0, sizeof a);
  a.what = what;
  if (!p) return a;
  a.layout = p->desc.layout;
  a.N = p->N;
  a.stride = pop_stride_of(p);
  const long long plane = (long long)p->n0 * p->n1;
  a.first = plane * p->interior_begin;
  a.count = plane * (p->interior_end - p->interior_begin);
  a.n0 = p->n0; a.n1 = p->n1; a.n2 = p->n2;
  a.partial = p->partial; a.reduce_blocks = kReduceBlocks;
  a.equilibrium = p->set.equilibrium; a.rho0 = p->set.rho0;
  a.stream = static_cast<hipStream_t>(stream);
  return a;
}

// The refusal of the kinds that exist for whole grids only (dispatch.hpp, kAuxTraits).  The entry point of such a kind
// asks once, where its refusals always had this one: before the checks of its own arguments.  A null plan is left to
// aux().
int whole_grid_only(const lt_plan *p, lt::AuxKind what) {
  const lt::AuxTraits &kind = lt::kAuxTraits[what];
  if (p && kind.whole_grid && (p->unit.d < 2 || p->desc.layout != LT_LAYOUT_REFERENCE || p->desc.ghost_planes))
    return fail(LT_ERR_UNSUPPORTED, "%s: 2-D / 3-D grids in the reference layout without ghost planes", kind.name);
  return LT_OK;
}

// the checks every kind shares, what kAuxTraits says of the population stride, then the launch
int aux(lt_plan *p, const lt::AuxArgs &a) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  const lt::AuxTraits &kind = lt::kAuxTraits[a.what];
  if (!a.f && a.what != lt::kAuxSlabEnstrophy) return fail(LT_ERR_INVALID, "null population buffer");
  if (a.stride != a.N && !kind.strided)
    return fail(LT_ERR_UNSUPPORTED, "%s: reads dense population buffers only (the plan has a population stride of %lld)",
                kind.name, a.stride);
  return launched(p->unit.aux(a), "no %s kernel", kind.name);
}

// The admission tests of the masked two-step kernels (compile_masks_kernel) for the plan's present boundary table:
// the only no-streaming bits the two-step kernel can take are those of ONE outlet at the last plane of the slowest
// memory axis or at an end of the rows -- the populations entering through it, on every node of it
struct MaskCheck {
  int axis = -1, plane = -1, face = -1;
  unsigned expected = 0, eq_slots = 0;
  long long plane_nodes = 0;
};
MaskCheck mask_check_of(const lt_plan *p) {
  MaskCheck c;
  int outlets = 0;
  const int sweep = p->unit.d == 2 ? 1 : 2;          // the slowest memory axis: rows in 2-D, planes in 3-D
  c.plane_nodes = sweep == 1 ? (long long)p->n0 : (long long)p->n0 * p->n1;
  for (int i = 0; i < p->desc.n_boundaries; ++i) {
    const lt_boundary_desc &b = p->desc.boundaries[i];
    if (b.kind == LT_BOUNDARY_EQUILIBRIUM && i + 1 < 32) c.eq_slots |= 1u << (i + 1);   // (only read for plans the two-step kernels admit: <= 15 boundaries)
    if (b.kind != LT_BOUNDARY_ABB_OUTLET || (b.flags & LT_BOUNDARY_ABSENT)) continue;
    ++outlets;
    const int ax = mem_axis_of(p, b.axis);
    if ((ax == sweep && b.side == 1) || (ax == 0 && p->unit.d == 3)) {
      c.axis = ax == sweep ? 2 : 0;                  // compile_masks_kernel: 2 = "index / plane_nodes", 0 = a0 column
      c.plane = ax == sweep ? (sweep == 2 ? p->n2 : p->n1) - 1 - p->desc.ghost_planes : (b.side == 1 ? p->n0 - 1 : 0);
      if (ax == 0) c.face = b.side == 1 ? 0 : p->n0 - 1;
      const lt::QList in = crossing_axis(p, ax, -b.side);
      for (int k = 0; k < in.n; ++k) c.expected |= 1u << in.q[k];
    }
  }
  if (outlets != 1) { c.axis = -1; c.plane = -1; c.face = -1; c.expected = 0; }
  return c;
}

// Decides the admission of the masked two-step kernels: one launch of a mask kernel over all nodes on `hs`
// (compile_masks_kernel or recheck_masks_kernel; `lead`: its arguments in front of the MaskCheck's), whose mismatch
// bits become the plan's admission flags
template <class Kernel, class... Lead>
int decide_admission(lt_plan *p, hipStream_t hs, Kernel kernel, Lead... lead) {
  LT_HIP(hipMemsetAsync(p->mask_flag, 0, sizeof(unsigned), hs));
  const MaskCheck c = mask_check_of(p);
  const unsigned grid = (unsigned)((p->N + lt::kThreads - 1) / lt::kThreads);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(lt::kThreads), 0, hs, lead..., c.plane_nodes, p->n0, c.axis, c.plane,
                     c.expected, c.face, c.eq_slots, p->mask_flag);
  LT_HIP(hipGetLastError());
  unsigned flags = 0;
  LT_HIP(hipMemcpyAsync(&flags, p->mask_flag, sizeof flags, hipMemcpyDeviceToHost, hs));
  LT_HIP(hipStreamSynchronize(hs));
  p->nsm_confined = (flags & 1u) == 0;
  p->inlet_faces_outlet = (flags & 2u) == 0;
  return LT_OK;
}

// memory extents of a descriptor's grid, a0 the contiguous one, a slab's ghost planes included (of a `dims`-dimensional unit)
struct Extents { long long e0, e1, e2; };
Extents extents_of(const lt_plan_desc &d, int dims) {
  if (dims == 1) return {d.shape[0], 1, 1};
  if (dims == 2) return {d.shape[1], d.shape[0], 1};
  if (d.layout == LT_LAYOUT_REFERENCE) return {d.shape[2], d.shape[1], d.shape[0]};
  return {d.shape[0], d.shape[1], d.shape[2] + 2 * d.ghost_planes};
}

// the outlets' axes decide how deep an outlet's neighbour must be rebuilt (see lt_plan_create); -1: unsupported
// (outlets of both kinds: a constant-pressure outlet reads its neighbour as an anti-bounce-back outlet does, and
// rewrites its plane)
int abb_depth_of(const lt_plan_desc &d) {
  int n_abb = 0, axes = 0;
  for (int i = 0; i < d.n_boundaries; ++i)
    if (d.boundaries[i].kind == LT_BOUNDARY_ABB_OUTLET || d.boundaries[i].kind == LT_BOUNDARY_PRESSURE_OUTLET) {
      ++n_abb;
      axes |= 1 << d.boundaries[i].axis;
    }
  const int n_axes = (axes & 1) + ((axes >> 1) & 1) + ((axes >> 2) & 1);
  const int depth = n_abb <= 1 ? 0 : (n_axes <= 2 ? 1 : n_axes - 1);
  return depth > 1 && d.layout != LT_LAYOUT_REFERENCE ? -1 : depth;
}

}  // namespace

extern "C" {

int lt_abi_version(void) { return LT_ABI_VERSION; }
int lt_build_flags(void) { return 0; }
const char *lt_last_error(void) { return g_error; }

int lt_plan_create(const lt_plan_desc *d, lt_plan **out) {
  if (!d || !out) return fail(LT_ERR_INVALID, "null argument");
  *out = nullptr;
  if (d->abi_version != LT_ABI_VERSION)
    return fail(LT_ERR_INVALID, "ABI version %d, library is %d", d->abi_version, LT_ABI_VERSION);
  if (d->stencil < 0 || d->stencil > 4) return fail(LT_ERR_UNSUPPORTED, "stencil %d", d->stencil);
  if (d->dtype < 0 || d->dtype > 1) return fail(LT_ERR_UNSUPPORTED, "dtype %d (fp32/fp64 only)", d->dtype);
  if ((d->collision < 0 || d->collision > LT_COLLISION_SMAGORINSKY) && d->collision != LT_COLLISION_TRT &&
      d->collision != LT_COLLISION_REGULARIZED && d->collision != LT_COLLISION_MRT)
    return fail(LT_ERR_UNSUPPORTED, "collision %d", d->collision);
  const Unit unit = kUnits[2 * d->stencil + d->dtype];
  if (d->dims != unit.d) return fail(LT_ERR_INVALID, "stencil is %d-dimensional, dims = %d", unit.d, d->dims);
  if (d->collision == LT_COLLISION_KBC && d->stencil != LT_D2Q9 && d->stencil != LT_D3Q27)
    return fail(LT_ERR_UNSUPPORTED, "KBC collision exists for D2Q9 and D3Q27 only");
  if (d->collision == LT_COLLISION_MRT && d->stencil != LT_D2Q9 && d->stencil != LT_D3Q27)
    return fail(LT_ERR_UNSUPPORTED, "MRT collision exists for D2Q9 (Dellar, Lallemand) and D3Q27 (Hermite) only");
  if (d->layout != LT_LAYOUT_REFERENCE && d->layout != LT_LAYOUT_SLAB)
    return fail(LT_ERR_INVALID, "layout %d", d->layout);
  if (d->layout == LT_LAYOUT_SLAB && unit.d != 3) return fail(LT_ERR_UNSUPPORTED, "slab layout is 3-D only");
  if (d->ghost_planes != 0 &&
      !((d->ghost_planes == 1 || d->ghost_planes == 2) && d->layout == LT_LAYOUT_SLAB))
    return fail(LT_ERR_INVALID, "ghost_planes = %d (0, or 1 / 2 with the slab layout)", d->ghost_planes);
  if (d->n_boundaries < 0 || d->n_boundaries > LT_MAX_BOUNDARIES)
    return fail(LT_ERR_UNSUPPORTED, "%d boundaries (max %d)", d->n_boundaries, LT_MAX_BOUNDARIES);
  for (int a = 0; a < unit.d; ++a)
    if (d->shape[a] < 1) return fail(LT_ERR_INVALID, "shape[%d] = %lld", a, (long long)d->shape[a]);

  lt_plan *p = new (std::nothrow) lt_plan;
  if (!p) return fail(LT_ERR_ALLOC, "out of host memory");
  p->desc = *d;
  p->unit = unit;
  p->esize = d->dtype == LT_F32 ? 4 : 8;
  const auto [e0, e1, e2] = extents_of(*d, unit.d);
  if (e0 * e1 * e2 >= (1ll << 31)) {
    delete p;
    return fail(LT_ERR_UNSUPPORTED, "%lld nodes per rank exceed the 2^31 index range", e0 * e1 * e2);
  }
  p->n0 = (int)e0; p->n1 = (int)e1; p->n2 = (int)e2;
  p->N = e0 * e1 * e2;
  p->interior_begin = d->ghost_planes;
  p->interior_end = p->n2 - d->ghost_planes;
  {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
      p->n_cu = cus;
  }
  int n_abb = 0;
  for (int i = 0; i < d->n_boundaries; ++i) {
    const int rc = check_boundary(p, d->boundaries[i]);
    if (rc) { delete p; return rc; }
    if (d->boundaries[i].kind == LT_BOUNDARY_ABB_OUTLET) ++n_abb;
    if (d->boundaries[i].kind == LT_BOUNDARY_PRESSURE_OUTLET) ++p->n_pout;
    if (d->boundaries[i].kind == LT_BOUNDARY_LINK_BOUNCE_BACK) ++p->n_link_kind;
  }
  p->n_abb = n_abb;
  // How deep the kernels must rebuild an outlet's neighbour (neighbour_moments, DEPTH): where the planes of outlets
  // meet, an outlet's neighbour node has been rewritten by the outlets with a lower index -- and their neighbours by
  // still lower ones.  Outlets on opposite faces of one axis never meet, so the chain is as long as the number of
  // distinct AXES the outlets lie on, minus one.  Kernels exist for depth 0 (one outlet), 1 (any list of outlets on at
  // most two axes: every 2-D flow) and, in the reference layout, 2 (outlets on all three axes, whose planes meet in
  // corners) -- the reference takes any list, lettuce/_simulation.py:57-86.
  p->abb_depth = abb_depth_of(*d);
  if (p->abb_depth < 0) {
    lt_plan_destroy(p);
    return fail(LT_ERR_UNSUPPORTED, "AntiBounceBackOutlets on all three axes (their planes meet in corners, where an "
                                    "outlet's neighbour depends on two earlier outlets) exist for the reference "
                                    "layout only; on slabs outlets on one or two axes run, in any number");
  }
  const size_t bt_size = d->dtype == LT_F32 ? sizeof(lt::BoundaryTable<float>)
                                            : sizeof(lt::BoundaryTable<double>);
  if (hipMalloc(&p->bt, bt_size) != hipSuccess ||
      hipMalloc((void **)&p->partial, kReduceBlocks * sizeof(double)) != hipSuccess) {
    lt_plan_destroy(p);
    return fail(LT_ERR_ALLOC, "hipMalloc of plan scratch failed");
  }
  const int rc = d->dtype == LT_F32 ? upload_boundaries<float>(p, nullptr)
                                    : upload_boundaries<double>(p, nullptr);
  if (rc) { lt_plan_destroy(p); return rc; }
  *out = p;
  return LT_OK;
}

int lt_plan_destroy(lt_plan *p) {
  if (!p) return LT_OK;
  if (p->node) (void)hipFree(p->node);
  if (p->nsm_bits) (void)hipFree(p->nsm_bits);
  if (p->bt) (void)hipFree(p->bt);
  if (p->mask_flag) (void)hipFree(p->mask_flag);
  if (p->signal) (void)hipFree(p->signal);
  if (p->signal_timed_out) (void)hipFree(p->signal_timed_out);
  if (p->partial) (void)hipFree(p->partial);
  for (void *r : p->res) if (r) (void)hipFree(r);
  for (lt_plan::Links &l : p->links) free_links(l);
  if (p->gexec) (void)hipGraphExecDestroy(p->gexec);
  if (p->gev_in) (void)hipEventDestroy(p->gev_in);
  if (p->gev_out) (void)hipEventDestroy(p->gev_out);
  if (p->gstream) (void)hipStreamDestroy(p->gstream);
  if (p->cstream) (void)hipStreamDestroy(p->cstream);
  delete p;
  return LT_OK;
}

int lt_plan_set_masks(lt_plan *p, const uint8_t *ncm, const uint8_t *nsm, void *stream) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (!ncm && !nsm) {
    if (p->desc.n_boundaries > 0)
      return fail(LT_ERR_INVALID, "a plan with boundaries needs a no_collision_mask");
    p->set.masked = 0;
    return LT_OK;
  }
  if (!p->node) LT_HIP(hipMalloc((void **)&p->node, (size_t)p->N));
  if (nsm && !p->nsm_bits) LT_HIP(hipMalloc((void **)&p->nsm_bits, (size_t)p->N * sizeof(unsigned)));
  if (!p->mask_flag) LT_HIP(hipMalloc((void **)&p->mask_flag, sizeof(unsigned)));
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const int rc = decide_admission(p, hs, lt::compile_masks_kernel, ncm, nsm, p->unit.q, p->N, p->node,
                                  nsm ? p->nsm_bits : nullptr);
  if (rc) return rc;
  if (p->gexec) {                                    // captured with the mask pointers of its time (nsm_bits may be new)
    (void)hipGraphExecDestroy(p->gexec);
    p->gexec = nullptr;
  }
  p->set.masked = 1;
  p->canary = 0;                                     // new masks: the first-use check runs again
  return LT_OK;
}

int lt_plan_update_boundary(lt_plan *p, int32_t index, const lt_boundary_desc *b, void *stream) {
  if (!p || !b) return fail(LT_ERR_INVALID, "null argument");
  if (index < 0 || index >= p->desc.n_boundaries) return fail(LT_ERR_INVALID, "boundary index %d", index);
  const lt_boundary_desc old = p->desc.boundaries[index];
  if (b->kind != old.kind)
    return fail(LT_ERR_INVALID, "boundary %d: kind cannot change (%d -> %d)", index, old.kind, b->kind);
  // what lt_plan_create would refuse is refused here too, and leaves the plan as it was
  int rc = check_boundary(p, *b);
  if (rc) return rc;
  p->desc.boundaries[index] = *b;
  const int depth = abb_depth_of(p->desc);
  if (depth < 0) {
    p->desc.boundaries[index] = old;
    return fail(LT_ERR_UNSUPPORTED, "boundary %d: AntiBounceBackOutlets on all three axes exist for the reference "
                                    "layout only", index);
  }
  p->abb_depth = depth;
  // an outlet that moves (axis, side, present / absent) changes which kernels apply and what they compute on its plane
  const bool moved = (b->kind == LT_BOUNDARY_ABB_OUTLET || b->kind == LT_BOUNDARY_PRESSURE_OUTLET) &&
                     (b->axis != old.axis || b->side != old.side || b->flags != old.flags);
  // a constant-pressure outlet's density is read from the boundary table at every launch, like an inlet's feq; a
  // captured graph is still dropped with it, so that nothing replayed was recorded for another outlet
  const bool density = b->kind == LT_BOUNDARY_PRESSURE_OUTLET && b->feq[0] != old.feq[0];
  // an equilibrium boundary that switches between its constant feq and a per-node field takes the other branch of
  // the kernels' boundary dispatch -- the code the first-use check exists for
  const bool source = b->kind == LT_BOUNDARY_EQUILIBRIUM && (b->feq_field_dev == nullptr) != (old.feq_field_dev == nullptr);
  hipStream_t hs = static_cast<hipStream_t>(stream);
  rc = p->desc.dtype == LT_F32 ? upload_boundaries<float>(p, hs) : upload_boundaries<double>(p, hs);
  if (rc) return rc;
  if (moved || source) p->canary = 0;                // the first-use check runs again
  if ((moved || density) && p->gexec) {              // the captured launches carry the old outlet's kernel arguments
    (void)hipGraphExecDestroy(p->gexec);
    p->gexec = nullptr;
  }
  if (moved && p->set.masked) {
    // the admission of the masked two-step kernels was decided for the old outlet: decide it again on the compiled
    // masks (node bytes and no-streaming bits as lt_plan_set_masks left them) for the new one
    return decide_admission(p, hs, lt::recheck_masks_kernel, p->node, p->nsm_bits, p->N);
  }
  return LT_OK;
}

int lt_collide(lt_plan *p, const void *f, void *o, double tau, void *s) {
  return step(p, Launch(lt::kCollideOnly, f, o, tau, p ? p->interior_begin : 0, p ? p->interior_end : 0, s));
}
int lt_stream(lt_plan *p, const void *f, void *o, void *s) {
  return step(p, Launch(lt::kStreamOnly, f, o, 1.0, p ? p->interior_begin : 0, p ? p->interior_end : 0, s));
}
int lt_stream_collide(lt_plan *p, const void *f, void *o, double tau, void *s) {
  return step(p, Launch(lt::kFused, f, o, tau, p ? p->interior_begin : 0, p ? p->interior_end : 0, s));
}
int lt_collide_planes(lt_plan *p, const void *f, void *o, double tau, int64_t b, int64_t e, void *s) {
  return step(p, Launch(lt::kCollideOnly, f, o, tau, b, e, s));
}
int lt_stream_planes(lt_plan *p, const void *f, void *o, int64_t b, int64_t e, void *s) {
  return step(p, Launch(lt::kStreamOnly, f, o, 1.0, b, e, s));
}
int lt_stream_collide_planes(lt_plan *p, const void *f, void *o, double tau, int64_t b, int64_t e,
                             void *s) {
  return step(p, Launch(lt::kFused, f, o, tau, b, e, s));
}

int lt_stream_collide_plane_pair(lt_plan *p, const void *f, void *o, double tau, int64_t first,
                                 int64_t second, void *s) {
  if (second <= first) return fail(LT_ERR_INVALID, "plane pair (%lld, %lld)", (long long)first, (long long)second);
  Launch l(lt::kFused, f, o, tau, first, second + 1, s);
  l.stride = second - first;
  return step(p, l);
}

int lt_stream_collide_plane_pair_packed(lt_plan *p, const void *f, void *o, double tau,
                                        int64_t first, int64_t second, void *pack_first,
                                        void *pack_second, void *s) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (second < first) return fail(LT_ERR_INVALID, "plane pair (%lld, %lld)", (long long)first, (long long)second);
  if (!pack_first || !pack_second) return fail(LT_ERR_INVALID, "null pack buffer");
  if (p->desc.layout != LT_LAYOUT_SLAB) return fail(LT_ERR_UNSUPPORTED, "fused packing needs the slab layout");
  Launch l(lt::kFused, f, o, tau, first, second + 1, s);
  l.stride = second > first ? second - first : 1;
  l.pack_lo = pack_first; l.pack_hi = pack_second;
  return step(p, l);
}

int lt_run(lt_plan *p, void *a, void *b, double tau, int64_t n, void *s, int32_t *r) {
  return run(p, false, a, b, tau, n, s, r);
}
int lt_continue(lt_plan *p, void *a, void *b, double tau, int64_t n, void *s, int32_t *r) {
  return run(p, true, a, b, tau, n, s, r);
}

int lt_macroscopic(lt_plan *p, const void *f, void *rho, void *u, void *s) {
  if (!rho && !u) return fail(LT_ERR_INVALID, "both outputs null");
  lt::AuxArgs a = aux_args(p, lt::kAuxMacroscopic, s);
  a.f = f; a.rho = rho; a.u = u;
  return aux(p, a);
}
int lt_equilibrium(lt_plan *p, const void *rho, const void *u, void *feq, void *s) {
  if (!rho || !u) return fail(LT_ERR_INVALID, "null rho/u");
  lt::AuxArgs a = aux_args(p, lt::kAuxEquilibrium, s);
  a.f = feq; a.rho = const_cast<void *>(rho); a.u = const_cast<void *>(u);
  return aux(p, a);
}

namespace {
// the three reductions of the populations over the interior planes into one device scalar
int reduce(lt_plan *p, lt::AuxKind what, const void *f, double *out, void *s) {
  if (!out) return fail(LT_ERR_INVALID, "null output");
  lt::AuxArgs a = aux_args(p, what, s);
  a.f = f; a.out = out;
  return aux(p, a);
}
}  // namespace
int lt_kinetic_energy(lt_plan *p, const void *f, double *out, void *s) { return reduce(p, lt::kAuxKineticEnergy, f, out, s); }
int lt_mass(lt_plan *p, const void *f, double *out, void *s) { return reduce(p, lt::kAuxMass, f, out, s); }
int lt_max_velocity(lt_plan *p, const void *f, double *out, void *s) { return reduce(p, lt::kAuxMaxVelocity, f, out, s); }

int lt_init_fneq(lt_plan *p, const void *rho, const void *u, double tau, double identity_cs2, void *f, void *s) {
  if (!rho || !u) return fail(LT_ERR_INVALID, "null rho/u");
  if (const int rc = whole_grid_only(p, lt::kAuxFneq)) return rc;
  if (!(tau > 0.0)) return fail(LT_ERR_INVALID, "relaxation time tau = %g", tau);
  lt::AuxArgs a = aux_args(p, lt::kAuxFneq, s);
  a.f = f; a.rho = const_cast<void *>(rho); a.u = const_cast<void *>(u);
  a.scale = tau; a.inv_dx = identity_cs2;
  return aux(p, a);
}
int lt_enstrophy(lt_plan *p, const void *f, void *u_scratch, double u_scale, double inv_dx, double *out, void *s) {
  if (!out || !u_scratch) return fail(LT_ERR_INVALID, "null output / scratch");
  if (const int rc = whole_grid_only(p, lt::kAuxEnstrophy)) return rc;
  lt::AuxArgs a = aux_args(p, lt::kAuxEnstrophy, s);
  a.f = f; a.u = u_scratch; a.out = out;
  a.scale = u_scale; a.inv_dx = inv_dx;
  return aux(p, a);
}
int lt_mass_interior(lt_plan *p, const void *f, const uint8_t *mask, double *out, void *s) {
  if (!out) return fail(LT_ERR_INVALID, "null output");
  if (const int rc = whole_grid_only(p, lt::kAuxInteriorMass)) return rc;
  lt::AuxArgs a = aux_args(p, lt::kAuxInteriorMass, s);
  a.f = f; a.mask = mask; a.out = out;
  return aux(p, a);
}

int lt_energy_spectrum(lt_plan *p, const void *uhat, double scale, int32_t n_bins, double *partial_scratch, double *out,
                       void *s) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (!uhat || !partial_scratch || !out) return fail(LT_ERR_INVALID, "null transformed field / scratch / output");
  if (const int rc = whole_grid_only(p, lt::kAuxSpectrum)) return rc;
  if (n_bins < 1) return fail(LT_ERR_INVALID, "energy spectrum: %d bins", (int)n_bins);
  if (n_bins > LT_SPECTRUM_MAX_BINS)
    return fail(LT_ERR_UNSUPPORTED, "energy spectrum: %d bins, the kernel's table of bins per wave holds "
                                    "LT_SPECTRUM_MAX_BINS = %d", (int)n_bins, LT_SPECTRUM_MAX_BINS);
  lt::AuxArgs a = aux_args(p, lt::kAuxSpectrum, s);
  a.f = uhat; a.partial = partial_scratch; a.out = out;
  a.stride = a.N;                       // the transformed fields are dense, whatever the plan's populations are
  // fixed launch geometry: contiguous ranges of whole workgroup passes (256 modes), four passes or more, in at most
  // LT_SPECTRUM_BLOCKS workgroups
  const long long pass = 256;
  a.count = ((p->N + LT_SPECTRUM_BLOCKS - 1) / LT_SPECTRUM_BLOCKS + pass - 1) / pass * pass;
  if (a.count < 4 * pass) a.count = 4 * pass;
  a.reduce_blocks = (int)((p->N + a.count - 1) / a.count);
  a.scale = scale; a.n_bins = n_bins;
  return aux(p, a);
}

int lt_boundary_force(lt_plan *p, const void *f, const uint8_t *solid, double *partial_scratch, double *out, void *s) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (!f || !solid || !partial_scratch || !out)
    return fail(LT_ERR_INVALID, "null populations / solid mask / scratch / output");
  if (const int rc = whole_grid_only(p, lt::kAuxBoundaryForce)) return rc;
  lt::AuxArgs a = aux_args(p, lt::kAuxBoundaryForce, s);
  a.f = f; a.mask = solid; a.partial = partial_scratch; a.out = out;
  // fixed launch geometry: a node per thread and pass, at most LT_BOUNDARY_FORCE_BLOCKS workgroups of 256
  const long long blocks = (p->N + 255) / 256;
  a.reduce_blocks = (int)(blocks < LT_BOUNDARY_FORCE_BLOCKS ? blocks : LT_BOUNDARY_FORCE_BLOCKS);
  return aux(p, a);
}

int lt_plan_set_links(lt_plan *p, int32_t index, int64_t n, const int32_t *nodes, const uint8_t *directions,
                      const void *c1, const void *c2, const uint8_t *second_source, void *stream) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (index < 0 || index >= p->desc.n_boundaries) return fail(LT_ERR_INVALID, "boundary index %d", index);
  if (p->desc.boundaries[index].kind != LT_BOUNDARY_LINK_BOUNCE_BACK)
    return fail(LT_ERR_INVALID, "boundary %d is of kind %d, not link bounce-back", index, p->desc.boundaries[index].kind);
  if (n < 0 || n >= (1ll << 31)) return fail(LT_ERR_INVALID, "n_links = %lld", (long long)n);
  if (n > 0 && (!nodes || !directions || !c1 || !c2 || !second_source))
    return fail(LT_ERR_INVALID, "null nodes / directions / c1 / c2 / second_source");
  // what the kernels index with: checked here, once, so that they need no bounds of their own
  for (int64_t i = 0; i < n; ++i) {
    if (nodes[i] < 0 || nodes[i] >= p->N || directions[i] < 1 || directions[i] >= p->unit.q)
      return fail(LT_ERR_INVALID, "link %lld: node %d direction %d outside [0, %lld) x [1, %d)", (long long)i, nodes[i],
                  (int)directions[i], p->N, p->unit.q);
    if (i > 0 && (nodes[i] < nodes[i - 1] || (nodes[i] == nodes[i - 1] && directions[i] <= directions[i - 1])))
      return fail(LT_ERR_INVALID, "link %lld: the list must be sorted by node, then by direction, no link twice",
                  (long long)i);
  }
  hipStream_t hs = static_cast<hipStream_t>(stream);
  lt_plan::Links fresh;
  fresh.set = true;
  fresh.n = (int)n;
  if (n > 0) {
    const size_t count = (size_t)n, esize = (size_t)p->esize;
    if (hipMalloc((void **)&fresh.node, count * sizeof(int)) != hipSuccess ||
        hipMalloc((void **)&fresh.dir, count) != hipSuccess || hipMalloc((void **)&fresh.second, count) != hipSuccess ||
        hipMalloc(&fresh.c1, count * esize) != hipSuccess || hipMalloc(&fresh.c2, count * esize) != hipSuccess) {
      free_links(fresh);
      return fail(LT_ERR_ALLOC, "hipMalloc of %lld links failed", (long long)n);
    }
    hipError_t e = hipMemcpyAsync(fresh.node, nodes, count * sizeof(int), hipMemcpyHostToDevice, hs);
    if (e == hipSuccess) e = hipMemcpyAsync(fresh.dir, directions, count, hipMemcpyHostToDevice, hs);
    if (e == hipSuccess) e = hipMemcpyAsync(fresh.second, second_source, count, hipMemcpyHostToDevice, hs);
    if (e == hipSuccess) e = hipMemcpyAsync(fresh.c1, c1, count * esize, hipMemcpyHostToDevice, hs);
    if (e == hipSuccess) e = hipMemcpyAsync(fresh.c2, c2, count * esize, hipMemcpyHostToDevice, hs);
    const hipError_t es = hipStreamSynchronize(hs);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) {
      free_links(fresh);
      return fail(LT_ERR_HIP, "copying the links failed: %s", hipGetErrorString(e));
    }
  }
  free_links(p->links[index]);                       // (hipFree waits for the launches that still read the old list)
  p->links[index] = fresh;
  if (p->gexec) {                                    // captured with the old list's pointers and length
    (void)hipGraphExecDestroy(p->gexec);
    p->gexec = nullptr;
  }
  return LT_OK;
}

int lt_apply_links(lt_plan *p, void *f, void *stream) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (!f) return fail(LT_ERR_INVALID, "null population buffer");
  if (p->n_link_kind < 1) return fail(LT_ERR_INVALID, "the plan has no link bounce-back boundary");
  if (const int rc = links_ready(p)) return rc;
  return apply_links(p, f, pop_stride_of(p), stream);
}

int lt_link_force(lt_plan *p, int32_t index, const void *f, double *partial_scratch, double *out, void *stream) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (!f || !partial_scratch || !out) return fail(LT_ERR_INVALID, "null populations / scratch / output");
  if (index < 0 || index >= p->desc.n_boundaries) return fail(LT_ERR_INVALID, "boundary index %d", index);
  if (p->desc.boundaries[index].kind != LT_BOUNDARY_LINK_BOUNCE_BACK)
    return fail(LT_ERR_INVALID, "boundary %d is of kind %d, not link bounce-back", index, p->desc.boundaries[index].kind);
  const lt_plan::Links &l = p->links[index];
  if (!l.set) return fail(LT_ERR_INVALID, "boundary %d is link bounce-back: lt_plan_set_links must give its links first", index);
  const LinkFn fn = kLinkUnits[2 * p->desc.stencil + p->desc.dtype];
  if (!fn) return fail(LT_ERR_UNSUPPORTED, "no link kernel for this lattice");
  lt::LinkArgs a = link_args(p, l, lt::kLinkForce, const_cast<void *>(f), pop_stride_of(p), stream);
  // fixed launch geometry: a link per thread and pass, at most LT_LINK_FORCE_BLOCKS workgroups of 256
  const long long blocks = ((long long)l.n + 255) / 256;
  a.blocks = (int)(blocks < LT_LINK_FORCE_BLOCKS ? blocks : LT_LINK_FORCE_BLOCKS);
  a.partial = partial_scratch; a.out = out;
  return launched(fn(a), "no link force kernel");
}

namespace {
int slab_plan_ok(lt_plan *p, const char *who) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (p->desc.layout != LT_LAYOUT_SLAB || p->desc.ghost_planes < 1)
    return fail(LT_ERR_UNSUPPORTED, "%s: for plans in the slab layout with ghost planes (a rank's share of the "
                                    "observable); single-domain plans have lt_enstrophy / lt_mass_interior", who);
  return LT_OK;
}
}  // namespace

int lt_slab_velocity(lt_plan *p, const void *f, void *u_ext, void *s) {
  if (const int rc = slab_plan_ok(p, "lt_slab_velocity")) return rc;
  if (!u_ext) return fail(LT_ERR_INVALID, "null velocity field");
  const long long plane = (long long)p->n0 * p->n1;
  const long long owned = p->interior_end - p->interior_begin;
  // node i of the plan (its ghost planes included) is node i + (3 - g) planes of the extended field
  char *u0 = static_cast<char *>(u_ext) + (3 - p->desc.ghost_planes) * plane * p->esize;
  lt::AuxArgs a = aux_args(p, lt::kAuxMacroscopic, s);
  a.f = f; a.u = u0; a.u_stride = (owned + 6) * plane;
  return aux(p, a);
}
int lt_slab_enstrophy(lt_plan *p, const void *u_ext, double u_scale, double inv_dx, double *out, void *s) {
  if (const int rc = slab_plan_ok(p, "lt_slab_enstrophy")) return rc;
  if (!out || !u_ext) return fail(LT_ERR_INVALID, "null output / velocity field");
  lt::AuxArgs a = aux_args(p, lt::kAuxSlabEnstrophy, s);
  a.u = const_cast<void *>(u_ext); a.out = out;
  a.n2 = (p->interior_end - p->interior_begin) + 6;
  a.scale = u_scale; a.inv_dx = inv_dx;
  return aux(p, a);
}
int lt_slab_mass_interior(lt_plan *p, const void *f, const uint8_t *mask, int32_t z_begin, int32_t nz_global,
                          double *out, void *s) {
  if (const int rc = slab_plan_ok(p, "lt_slab_mass_interior")) return rc;
  if (!out) return fail(LT_ERR_INVALID, "null output");
  const int owned = p->interior_end - p->interior_begin;
  if (z_begin < 0 || nz_global < 1 || z_begin + owned > nz_global)
    return fail(LT_ERR_INVALID, "planes [%d, %d) of %d", z_begin, z_begin + owned, nz_global);
  lt::AuxArgs a = aux_args(p, lt::kAuxSlabInteriorMass, s);
  a.f = f; a.mask = mask; a.out = out;
  a.z_begin = z_begin; a.nz_global = nz_global;
  return aux(p, a);
}

int lt_plan_kernel_info(lt_plan *p, int32_t *vec, int32_t *tpb, int64_t *blocks) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (vec) *vec = 1;
  if (tpb) *tpb = lt::kThreads;
  if (blocks) {
    const long long nodes = (long long)p->n0 * p->n1 * (p->interior_end - p->interior_begin);
    *blocks = (nodes + lt::kThreads - 1) / lt::kThreads;
  }
  return LT_OK;
}

const char *lt_plan_kernel_name(lt_plan *p) {
  if (!p) return "";
  // what the fused section launches: lt_run's pairs, or a two-step slab driver on a plan with two
  // ghost planes
  int mode = (two_step_wanted(p) || p->desc.ghost_planes == 2) ? lt::kFusedTwice : lt::kFused;
  if (many_step_wanted(p)) mode = lt::kFusedMany;
  if (mode == lt::kFusedTwice && !has_kernel(p->unit, kernel_selector(p, mode))) mode = lt::kFused;
  const lt::StepArgs a = kernel_selector(p, mode);
  if (!p->unit.name(a, lt::NameBuf{p->kernel_name, sizeof p->kernel_name})) p->kernel_name[0] = 0;
  return p->kernel_name;
}

int lt_slab_crossing(lt_plan *p, int32_t direction, int32_t *q_out, int32_t *n_out) {
  if (!p || !n_out) return fail(LT_ERR_INVALID, "null argument");
  const lt::QList ql = crossing(p, direction);
  *n_out = ql.n;
  if (q_out) for (int k = 0; k < ql.n; ++k) q_out[k] = ql.q[k];
  return LT_OK;
}
int lt_slab_pack(lt_plan *p, const void *f, int64_t plane, int32_t direction, void *buf, void *s) {
  return pack(p, true, const_cast<void *>(f), plane, direction, buf, s);
}
int lt_slab_unpack(lt_plan *p, void *f, int64_t plane, int32_t direction, const void *buf, void *s) {
  return pack(p, false, f, plane, direction, const_cast<void *>(buf), s);
}

int lt_jacobi(void *p, void *p_scratch, const void *rhs, int32_t dtype, int32_t dims, const int64_t *shape, double dx,
              double tol_abs, int64_t max_num_steps, int32_t batch, void *work, int64_t *iterations_out, double *error_out,
              void *stream) {
  if (!p || !p_scratch || !rhs || !shape || !work) return fail(LT_ERR_INVALID, "jacobi: null field / scratch / shape / work buffer");
  if (dims != 2 && dims != 3) return fail(LT_ERR_INVALID, "jacobi: %d dimensions (2 or 3)", (int)dims);
  if (dtype != LT_F32 && dtype != LT_F64) return fail(LT_ERR_INVALID, "jacobi: unknown dtype %d", (int)dtype);
  long long N = 1;
  for (int a = 0; a < dims; ++a) {
    if (shape[a] < 1 || shape[a] > 0x7fffffffLL)
      return fail(LT_ERR_INVALID, "jacobi: shape[%d] = %lld (an extent is >= 1 and < 2^31)", a, (long long)shape[a]);
    N *= shape[a];
    if (N > (1LL << 40)) return fail(LT_ERR_INVALID, "jacobi: more than 2^40 nodes");
  }
  if (max_num_steps < 0) return fail(LT_ERR_INVALID, "jacobi: max_num_steps = %lld", (long long)max_num_steps);
  if (batch < 0) return fail(LT_ERR_INVALID, "jacobi: batch = %d", (int)batch);
  if (p == p_scratch || (uintptr_t)work % 8) return fail(LT_ERR_INVALID, "jacobi: scratch is the field itself, or the work buffer is not 8-byte aligned");
  if (iterations_out) *iterations_out = 0;
  if (error_out) *error_out = 1.0;                  // the reference's starting value: what max_num_steps = 0 leaves
  if (max_num_steps == 0) return LT_OK;
  const long long K = batch ? batch : LT_JACOBI_BATCH;
  hipStream_t s = static_cast<hipStream_t>(stream);
  struct Record { int32_t done, pad; int64_t iterations; double error; } record = {0, 0, 0, 1.0};
  void *state = lt::jacobi_state(work);
  LT_HIP(hipMemsetAsync(state, 0, sizeof record, s));
  lt::JacobiArgs a;
  memset(&a, 0, sizeof a);
  a.rhs = rhs; a.work = work; a.dtype = dtype; a.d = dims;
  a.n0 = (int)shape[0]; a.n1 = (int)shape[1]; a.n2 = dims == 3 ? (int)shape[2] : 1;
  a.dx2 = dx * dx; a.tol = tol_abs; a.stream = s;
  void *buf[2] = {p, p_scratch};                    // iterate k lies in buf[k % 2]
  // Sweep k reads iterate k - 1 and writes iterate k; the launch behind it forms the error of iterate k - 1 (none behind
  // sweep 1: the reference never looks at the starting field's).  Sweep max + 1 is there for the last error alone.
  const long long last = (long long)max_num_steps + 1;
  for (long long k = 1; k <= last && !record.done;) {
    for (long long end = std::min(last, k + K - 1); k <= end; ++k) {
      a.p_in = buf[(k - 1) % 2];
      a.p_out = k == last ? nullptr : buf[k % 2];
      a.sweep = k; a.finish = k >= 2;
      if (const int rc = launched(lt::jacobi_sweep(a), "no Jacobi kernel")) return rc;
    }
    LT_HIP(hipMemcpyAsync(&record, state, sizeof record, hipMemcpyDeviceToHost, s));
    LT_HIP(hipStreamSynchronize(s));
  }
  if (record.iterations % 2) {
    LT_HIP(hipMemcpyAsync(p, p_scratch, (size_t)N * (dtype == LT_F32 ? 4 : 8), hipMemcpyDeviceToDevice, s));
    LT_HIP(hipStreamSynchronize(s));
  }
  if (iterations_out) *iterations_out = record.iterations;
  if (error_out) *error_out = record.error;
  return LT_OK;
}

int lt_probe_copy(void *dst, const void *src, int64_t n_bytes, int32_t cache_policy,
                  int32_t max_blocks, void *stream) {
  if (!dst || !src || n_bytes < 16 || n_bytes % 16 != 0 || (uintptr_t)dst % 16 || (uintptr_t)src % 16)
    return fail(LT_ERR_INVALID, "probe copy needs 16-byte aligned buffers and size");
  const size_t n = (size_t)n_bytes / 16;
  size_t grid = (n + 255) / 256;
  if (max_blocks > 0 && grid > (size_t)max_blocks) grid = (size_t)max_blocks;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const probe_f4 *sp = static_cast<const probe_f4 *>(src);
  probe_f4 *dp = static_cast<probe_f4 *>(dst);
  switch (cache_policy) {
    case 0: hipLaunchKernelGGL(probe_copy_kernel<0>, dim3((unsigned)grid), dim3(256), 0, s, sp, dp, n); break;
    case 1: hipLaunchKernelGGL(probe_copy_kernel<1>, dim3((unsigned)grid), dim3(256), 0, s, sp, dp, n); break;
    case 2: hipLaunchKernelGGL(probe_copy_kernel<2>, dim3((unsigned)grid), dim3(256), 0, s, sp, dp, n); break;
    case 3: hipLaunchKernelGGL(probe_copy_kernel<3>, dim3((unsigned)grid), dim3(256), 0, s, sp, dp, n); break;
    default: return fail(LT_ERR_INVALID, "cache policy %d", cache_policy);
  }
  LT_HIP(hipGetLastError());
  return LT_OK;
}

int lt_probe_div_cs(const void *x, void *out, int64_t n, int32_t dtype, int32_t which, void *stream) {
  if (!x || !out || n < 1 || (which != 0 && which != 1) || (dtype != LT_F32 && dtype != LT_F64))
    return fail(LT_ERR_INVALID, "probe_div_cs: null buffer, n = %lld, which = %d, dtype = %d", (long long)n, which, dtype);
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == LT_F32)
    hipLaunchKernelGGL(probe_div_cs_kernel<float>, dim3(grid), dim3(256), 0, s, (const float *)x, (float *)out, (long long)n, which);
  else
    hipLaunchKernelGGL(probe_div_cs_kernel<double>, dim3(grid), dim3(256), 0, s, (const double *)x, (double *)out, (long long)n, which);
  LT_HIP(hipGetLastError());
  return LT_OK;
}

int lt_plan_set_shift_policy(lt_plan *p, int32_t policy) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (policy < 0 || policy > 6) return fail(LT_ERR_INVALID, "shift policy %d", policy);
  if (policy == 1 || policy == 2 || policy == 5)
    return fail(LT_ERR_UNSUPPORTED, "shift policy %d: its tile variant lost its A/B and was removed", policy);
  if (p->set.shift != policy) p->canary = 0;
  p->set.shift = policy;
  return LT_OK;
}

int lt_plan_set_deferred_stream(lt_plan *p, int32_t on) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  p->defer_stream = on ? 1 : 0;
  return LT_OK;
}

int lt_plan_set_population_stride(lt_plan *p, int64_t stride) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (stride != 0 && (stride < p->N || (stride * p->esize) % 256 != 0))
    return fail(LT_ERR_INVALID, "population stride %lld: 0 (dense) or >= %lld nodes and a multiple of 256 bytes",
                (long long)stride, p->N);
  p->pop_stride = stride == p->N ? 0 : stride;
  return LT_OK;
}
int lt_plan_population_stride(lt_plan *p, int64_t *stride) {
  if (!p || !stride) return fail(LT_ERR_INVALID, "null argument");
  *stride = pop_stride_of(p);
  return LT_OK;
}

// ---- engine-owned padded population buffers ----------------------------------------------------------------
int lt_plan_set_resident(lt_plan *p, int32_t mode, int64_t pad_elements) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (mode < -1 || mode > 1) return fail(LT_ERR_INVALID, "resident mode %d", mode);
  if (pad_elements < -1) return fail(LT_ERR_INVALID, "pad %lld", (long long)pad_elements);
  if (mode == 1 && (p->desc.ghost_planes || p->unit.d < 2))
    return fail(LT_ERR_UNSUPPORTED, "resident populations: periodic 2-D / 3-D plans (slab ranks own their buffers: "
                                    "lt_plan_set_population_stride)");
  p->resident = mode;
  if (pad_elements != p->res_pad) p->res_valid = 0;
  p->res_pad = pad_elements;
  return LT_OK;
}
int lt_resident_enabled(lt_plan *p, int32_t *enabled, int64_t *stride) {
  if (!p || !enabled) return fail(LT_ERR_INVALID, "null argument");
  *enabled = resident_wanted(p) ? 1 : 0;
  if (stride) *stride = resident_stride(p);
  return LT_OK;
}
int lt_resident_load(lt_plan *p, const void *f, double tau, void *stream) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (p->desc.ghost_planes) return fail(LT_ERR_UNSUPPORTED, "resident populations need a periodic plan");
  int rc = resident_alloc(p);
  if (rc) return rc;
  p->res_valid = 0;
  Launch l(lt::kCollideOnly, f, p->res[0], tau, 0, p->n2, stream);
  l.stride_out = p->res_stride;
  rc = step(p, l);
  if (rc) return rc;
  p->res_cur = 0;
  p->res_valid = 1;
  return LT_OK;
}
int lt_resident_advance(lt_plan *p, double tau, int64_t n, void *stream) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (n < 0) return fail(LT_ERR_INVALID, "n_steps = %lld", (long long)n);
  if (!p->res_valid) return fail(LT_ERR_INVALID, "no resident populations: call lt_resident_load first");
  p->last_single = p->last_twice = p->last_many = 0;
  if (n == 0) return LT_OK;
  void *cur = p->res[p->res_cur], *other = p->res[1 - p->res_cur];
  const int rc = fused_section(p, cur, other, tau, n, stream, p->res_stride);
  if (rc) { p->res_valid = 0; return rc; }
  p->res_cur = cur == p->res[0] ? 0 : 1;
  return LT_OK;
}
int lt_resident_store(lt_plan *p, void *out, void *stream) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (!p->res_valid) return fail(LT_ERR_INVALID, "no resident populations: call lt_resident_load first");
  Launch l(lt::kStreamOnly, p->res[p->res_cur], out, 1.0, 0, p->n2, stream);
  l.stride_in = p->res_stride;
  return step(p, l);
}
int lt_resident_free(lt_plan *p) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  for (void *&r : p->res) { if (r) (void)hipFree(r); r = nullptr; }
  p->res_valid = 0;
  p->res_stride = 0;
  return LT_OK;
}

int lt_plan_set_graph_mode(lt_plan *p, int32_t mode) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (mode < -1 || mode > 1) return fail(LT_ERR_INVALID, "graph mode %d", mode);
  p->graph_mode = mode;
  return LT_OK;
}

int lt_stream_collide_twice(lt_plan *p, const void *f, void *out, double tau, void *stream) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  const int g = p->desc.ghost_planes;
  return step(p, Launch(lt::kFusedTwice, f, out, tau, g, p->n2 - g, stream));
}
int lt_stream_collide_twice_planes(lt_plan *p, const void *f, void *out, double tau, int64_t begin,
                                   int64_t end, void *stream) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  return step(p, Launch(lt::kFusedTwice, f, out, tau, begin, end, stream));
}
int lt_stream_collide_twice_planes_packed(lt_plan *p, const void *f, void *out, double tau, int64_t begin,
                                          int64_t end, void *pack_lower, void *pack_upper, void *stream) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (p->desc.ghost_planes != 2) return fail(LT_ERR_INVALID, "fused two-step packing needs ghost_planes = 2");
  if (!pack_lower && !pack_upper) return fail(LT_ERR_INVALID, "null pack buffers");
  if (end - begin < 2) return fail(LT_ERR_INVALID, "the halo message reads two planes: range [%lld, %lld)",
                                   (long long)begin, (long long)end);
  if (pack_lower && begin != 2)
    return fail(LT_ERR_INVALID, "lower message: the range must start at the first interior plane");
  if (pack_upper && end != p->n2 - 2)
    return fail(LT_ERR_INVALID, "upper message: the range must end at the last interior plane");
  Launch l(lt::kFusedTwice, f, out, tau, begin, end, stream);
  l.pack_lo = pack_lower; l.pack_hi = pack_upper;
  return step(p, l);
}
namespace {
// both edges of a slab in one launch, edge_planes each (one segment per range and tile); recv_*: the received halo
// messages to read the planes beyond the cuts from, or null: the ghost planes of f
int twice_edges(lt_plan *p, const void *f, void *out, double tau, int32_t edge_planes, const void *recv_lower,
                const void *recv_upper, void *pack_lower, void *pack_upper, void *stream) {
  if (p->desc.ghost_planes != 2) return fail(LT_ERR_INVALID, "edge launch needs ghost_planes = 2");
  const long long lo = 2, hi = p->n2 - 2;
  if (edge_planes < 2 || 2ll * edge_planes > hi - lo)
    return fail(LT_ERR_INVALID, "edge_planes = %d (2 .. %lld)", edge_planes, (hi - lo) / 2);
  if ((pack_lower == nullptr) != (pack_upper == nullptr))
    return fail(LT_ERR_INVALID, "give both message buffers or neither");
  Launch l(lt::kFusedTwice, f, out, tau, lo, lo + edge_planes, stream);
  l.begin2 = hi - edge_planes; l.end2 = hi;
  l.seg_len = edge_planes;
  l.pack_lo = pack_lower; l.pack_hi = pack_upper;
  l.ghost_lo = recv_lower; l.ghost_hi = recv_upper;
  return step(p, l);
}
}  // namespace

int lt_stream_collide_twice_edges(lt_plan *p, const void *f, void *out, double tau, int32_t edge_planes,
                                  void *pack_lower, void *pack_upper, void *stream) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  return twice_edges(p, f, out, tau, edge_planes, nullptr, nullptr, pack_lower, pack_upper, stream);
}
int lt_stream_collide_twice_edges_direct(lt_plan *p, const void *f, void *out, double tau, int32_t edge_planes,
                                         const void *recv_lower, const void *recv_upper, void *pack_lower,
                                         void *pack_upper, void *stream) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (!pack_lower || !pack_upper || (recv_lower == nullptr) != (recv_upper == nullptr))
    return fail(LT_ERR_INVALID, "the direct edge launch needs both send buffers, and both received messages or "
                                "neither (then the ghost planes of f_dev are read)");
  if (p->set.masked) return fail(LT_ERR_UNSUPPORTED, "the direct edge launch exists for plans without masks");
  return twice_edges(p, f, out, tau, edge_planes, recv_lower, recv_upper, pack_lower, pack_upper, stream);
}
// The whole slab in one launch that feeds the exchange while it runs: see include/lettuce_hip.h
int lt_stream_collide_twice_slab(lt_plan *p, const void *f, void *out, double tau, void *stream) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (p->desc.ghost_planes != 2) return fail(LT_ERR_INVALID, "the two-step slab launch needs ghost_planes = 2");
  if (p->set.masked) return fail(LT_ERR_UNSUPPORTED, "the signalling slab launch exists for plans without masks");
  const long long lo = 2, hi = p->n2 - 2;
  if (hi - lo < 4) return fail(LT_ERR_INVALID, "the slab needs at least 4 interior planes");
  hipStream_t hs = static_cast<hipStream_t>(stream);
  if (!p->signal) {
    LT_HIP(hipMalloc((void **)&p->signal, sizeof(unsigned long long)));
    LT_HIP(hipMalloc((void **)&p->signal_timed_out, sizeof(unsigned)));
    LT_HIP(hipMemsetAsync(p->signal, 0, sizeof(unsigned long long), hs));
    LT_HIP(hipMemsetAsync(p->signal_timed_out, 0, sizeof(unsigned), hs));
    // once: the polling wave of ANOTHER stream must never see the counter before it is zero
    LT_HIP(hipStreamSynchronize(hs));
    p->signal_target = 0;
  }
  const TwoStepTile tile = two_step_tile(p);
  if (!lt::tiles(tile, p->n0, p->n1))
    return fail(LT_ERR_UNSUPPORTED, "two steps per launch: the grid does not tile");
  // upper edge = second range [hi - 2, hi): one short segment; first range [lo, hi - 2) in segments of at least
  // two planes
  Launch l(lt::kFusedTwice, f, out, tau, lo, hi - 2, stream);
  l.begin2 = hi - 2; l.end2 = hi;
  l.seg_len = std::max(2, resolve_seg_len(p, (int)(hi - 2 - lo)));
  l.signal = p->signal;
  const int rc = step(p, l);
  if (rc == LT_OK) p->signal_target += 2ull * (unsigned long long)((p->n0 / tile.width) * (p->n1 / tile.rows));
  return rc;
}
int lt_slab_wait_edges(lt_plan *p, void *stream) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (!p->signal) return fail(LT_ERR_INVALID, "no lt_stream_collide_twice_slab launch to wait for");
  hipLaunchKernelGGL(lt::wait_counter_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), p->signal,
                     p->signal_target, p->signal_timed_out);
  LT_HIP(hipGetLastError());
  return LT_OK;
}
int lt_slab_wait_timed_out(lt_plan *p, int32_t *timed_out, void *stream) {
  if (!p || !timed_out) return fail(LT_ERR_INVALID, "null argument");
  unsigned flag = 0;
  if (p->signal_timed_out) {
    hipStream_t hs = static_cast<hipStream_t>(stream);
    LT_HIP(hipMemcpyAsync(&flag, p->signal_timed_out, sizeof flag, hipMemcpyDeviceToHost, hs));
    LT_HIP(hipStreamSynchronize(hs));
    // reported once: the next batch starts with a clean word (the counter itself stays consistent -- every edge
    // workgroup of the launch that was waited for still adds its 1)
    if (flag) LT_HIP(hipMemsetAsync(p->signal_timed_out, 0, sizeof(unsigned), hs));
  }
  *timed_out = (int32_t)flag;
  return LT_OK;
}
int lt_plan_two_step_admitted(lt_plan *p) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  const char *why = "";
  if (!two_step_possible(p, &why)) return fail(LT_ERR_UNSUPPORTED, "two steps per launch: %s", why);
  return LT_OK;
}
int lt_two_step_limits(const lt_plan_desc *d, int32_t masked, int32_t *tile_width, int32_t *tile_rows,
                       int32_t *addressable) {
  if (!d) return fail(LT_ERR_INVALID, "null descriptor");
  if (d->stencil < 0 || d->stencil > 4) return fail(LT_ERR_UNSUPPORTED, "stencil %d", d->stencil);
  if (d->dtype < 0 || d->dtype > 1) return fail(LT_ERR_UNSUPPORTED, "dtype %d (fp32/fp64 only)", d->dtype);
  const Unit &unit = kUnits[2 * d->stencil + d->dtype];
  if (d->dims != unit.d) return fail(LT_ERR_INVALID, "stencil is %d-dimensional, dims = %d", unit.d, d->dims);
  const int esize = d->dtype == LT_F32 ? 4 : 8;
  const auto [e0, e1, e2] = extents_of(*d, unit.d);
  const TwoStepTile tile = lt::two_step_tile_on(unit.tile, unit.d, (int)e0, masked != 0);
  if (tile_width) *tile_width = tile.width;
  if (tile_rows) *tile_rows = tile.rows;
  if (addressable)
    *addressable = two_step_addressable(unit, esize, e0, e1, e0 * e1 * e2, masked != 0, d->layout, d->collision) ? 1 : 0;
  return LT_OK;
}
int lt_slab_two_step_message_blocks(lt_plan *p, int32_t *blocks) {
  if (!p || !blocks) return fail(LT_ERR_INVALID, "null argument");
  *blocks = crossing(p, 0).n + (p->set.masked ? 3 : 2) * crossing(p, 1).n;
  return LT_OK;
}
int lt_slab_pack_two_step(lt_plan *p, const void *f, int32_t side, void *buf, void *s) {
  return halo2(p, true, const_cast<void *>(f), side, buf, s);
}
int lt_slab_unpack_two_step(lt_plan *p, void *f, int32_t side, const void *buf, void *s) {
  return halo2(p, false, f, side, const_cast<void *>(buf), s);
}

int lt_plan_set_fused_events(lt_plan *p, void *start_event, void *stop_event) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if ((start_event == nullptr) != (stop_event == nullptr))
    return fail(LT_ERR_INVALID, "give both events or neither");
  p->ev_start = static_cast<hipEvent_t>(start_event);
  p->ev_stop = static_cast<hipEvent_t>(stop_event);
  return LT_OK;
}

int lt_plan_last_run_info(lt_plan *p, int64_t *single_step_launches, int64_t *two_step_launches,
                          int64_t *many_step_launches) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (single_step_launches) *single_step_launches = p->last_single;
  if (two_step_launches) *two_step_launches = p->last_twice;
  if (many_step_launches) *many_step_launches = p->last_many;
  return LT_OK;
}

int lt_stream_collide_many(lt_plan *p, const void *f, void *out, double tau, int32_t n_steps, void *stream) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (n_steps < 1 || n_steps > many_max(p))
    return fail(LT_ERR_INVALID, "n_steps = %d (1..%d per launch for this plan)", n_steps, many_max(p));
  Launch l(lt::kFusedMany, f, out, tau, 0, p->n2, stream);
  l.many = n_steps;
  return step(p, l);
}

int lt_plan_set_many_step(lt_plan *p, int32_t mode) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (mode < -1 || mode > 1) return fail(LT_ERR_INVALID, "many-step mode %d", mode);
  if (mode == 1 && p->set.equilibrium == LT_EQUILIBRIUM_INCOMPRESSIBLE)
    return fail(LT_ERR_UNSUPPORTED, "several steps per launch: %s", kIncompressibleMultiStep);
  if (mode == 1 && p->n_link_kind > 0) return fail(LT_ERR_UNSUPPORTED, "several steps per launch with %s", kLinkMultiStep);
  if (mode == 1 && p->set.field.a) return fail(LT_ERR_UNSUPPORTED, "several steps per launch: %s", kForceFieldMultiStep);
  p->many = mode;
  return LT_OK;
}

int lt_plan_set_smagorinsky(lt_plan *p, double constant) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (p->desc.collision != LT_COLLISION_SMAGORINSKY)
    return fail(LT_ERR_INVALID, "the plan's collision is %d, not Smagorinsky", p->desc.collision);
  if (!(constant >= 0.0) || !std::isfinite(constant))
    return fail(LT_ERR_INVALID, "Smagorinsky constant %g (finite and >= 0)", constant);
  p->set.smagorinsky = constant;
  return LT_OK;
}

int lt_plan_set_trt(lt_plan *p, double tau_minus) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (p->desc.collision != LT_COLLISION_TRT)
    return fail(LT_ERR_INVALID, "the plan's collision is %d, not TRT", p->desc.collision);
  if (!(tau_minus > 0.0) || !std::isfinite(tau_minus))
    return fail(LT_ERR_INVALID, "TRT relaxation time tau_minus = %g (finite and > 0)", tau_minus);
  p->set.tau_minus = tau_minus;
  return LT_OK;
}

int lt_plan_set_mrt(lt_plan *p, int transform, const double *relaxation, int count) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (p->desc.collision != LT_COLLISION_MRT)
    return fail(LT_ERR_INVALID, "the plan's collision is %d, not MRT", p->desc.collision);
  if (transform != LT_MRT_D2Q9_DELLAR && transform != LT_MRT_D2Q9_LALLEMAND && transform != LT_MRT_D3Q27_HERMITE)
    return fail(LT_ERR_INVALID, "MRT transform %d (1 Dellar, 2 Lallemand, 3 Hermite)", transform);
  if ((transform == LT_MRT_D3Q27_HERMITE) != (p->desc.stencil == LT_D3Q27))
    return fail(LT_ERR_INVALID, "MRT transform %d belongs to %s, the plan's lattice has %d velocities", transform,
                transform == LT_MRT_D3Q27_HERMITE ? "D3Q27" : "D2Q9", p->unit.q);
  if (!relaxation) return fail(LT_ERR_INVALID, "null relaxation rates");
  if (count != p->unit.q)
    return fail(LT_ERR_INVALID, "%d relaxation rates, the transform has %d moments", count, p->unit.q);
  for (int i = 0; i < count; ++i)
    if (!(relaxation[i] > 0.0) || !std::isfinite(relaxation[i]))
      return fail(LT_ERR_INVALID, "MRT relaxation rate %d = %g (finite and > 0)", i, relaxation[i]);
  p->set.mrt.transform = transform;
  std::fill(p->set.mrt.rates, p->set.mrt.rates + 27, 0.0);
  std::copy(relaxation, relaxation + count, p->set.mrt.rates);
  return LT_OK;
}

int lt_plan_set_force(lt_plan *p, const double *acceleration, double ueq_scale, double source_scale) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (p->desc.collision != LT_COLLISION_BGK && p->desc.collision != LT_COLLISION_SMAGORINSKY)
    return fail(LT_ERR_UNSUPPORTED, "a body force exists for the BGK and Smagorinsky collisions; the plan's collision "
                                    "is %d", p->desc.collision);
  lt_plan::Settings::Force f;
  if (acceleration) {
    f.on = true;
    for (int c = 0; c < p->unit.d; ++c) f.a[c] = acceleration[c];
    f.ueq_scale = ueq_scale; f.source_scale = source_scale;
    if (!std::isfinite(f.a[0]) || !std::isfinite(f.a[1]) || !std::isfinite(f.a[2]) || !std::isfinite(ueq_scale) ||
        !std::isfinite(source_scale))
      return fail(LT_ERR_INVALID, "body force: acceleration (%g, %g, %g), scales %g and %g must be finite", f.a[0],
                  f.a[1], f.a[2], ueq_scale, source_scale);
  }
  p->set.force = f;
  p->set.field = lt_plan::Settings::ForceField();      // the later call wins
  return LT_OK;
}

int lt_plan_set_force_field(lt_plan *p, const void *acceleration, double ueq_scale, double source_scale) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (p->desc.collision != LT_COLLISION_BGK && p->desc.collision != LT_COLLISION_SMAGORINSKY)
    return fail(LT_ERR_UNSUPPORTED, "a body force exists for the BGK and Smagorinsky collisions; the plan's collision "
                                    "is %d", p->desc.collision);
  if (!acceleration) {
    p->set.field = lt_plan::Settings::ForceField();
    return LT_OK;
  }
  if (!std::isfinite(ueq_scale) || !std::isfinite(source_scale))
    return fail(LT_ERR_INVALID, "force field: scales %g and %g must be finite", ueq_scale, source_scale);
  // what has no kernel with a field (unit.inc, part force_field: one-step kernels of the reference layout, no outlet)
  if (p->desc.layout != LT_LAYOUT_REFERENCE || p->desc.ghost_planes)
    return fail(LT_ERR_UNSUPPORTED, "a force field (lt_plan_set_force_field) on a slab plan: its kernels exist for the "
                                    "reference layout without ghost planes only");
  for (int i = 0; i < p->desc.n_boundaries; ++i) {
    const int kind = p->desc.boundaries[i].kind;
    if (kind == LT_BOUNDARY_ABB_OUTLET || kind == LT_BOUNDARY_PRESSURE_OUTLET)
      return fail(LT_ERR_UNSUPPORTED, "a force field (lt_plan_set_force_field) on a plan with %s (boundary %d): an outlet "
                                      "collides its neighbour node again, and no kernel does that with a field",
                  kind == LT_BOUNDARY_ABB_OUTLET ? "an anti-bounce-back outlet" : "a constant-pressure outlet", i);
  }
  if (p->set.equilibrium == LT_EQUILIBRIUM_INCOMPRESSIBLE)
    return fail(LT_ERR_UNSUPPORTED, "a force field (lt_plan_set_force_field) and the incompressible equilibrium "
                                    "(lt_plan_set_equilibrium): no kernel has the pair");
  if (p->two_step == 1) return fail(LT_ERR_UNSUPPORTED, "two steps per launch: %s", kForceFieldMultiStep);
  if (p->many == 1) return fail(LT_ERR_UNSUPPORTED, "several steps per launch: %s", kForceFieldMultiStep);
  p->set.field.a = acceleration;
  p->set.field.ueq_scale = ueq_scale;
  p->set.field.source_scale = source_scale;
  p->set.force = lt_plan::Settings::Force();           // the later call wins
  return LT_OK;
}

int lt_plan_set_equilibrium(lt_plan *p, int kind, double rho0) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (kind != LT_EQUILIBRIUM_QUADRATIC && kind != LT_EQUILIBRIUM_INCOMPRESSIBLE)
    return fail(LT_ERR_INVALID, "equilibrium kind %d (0 quadratic, 1 incompressible)", kind);
  if (!std::isfinite(rho0)) return fail(LT_ERR_INVALID, "equilibrium: rho0 = %g must be finite", rho0);
  if (kind == LT_EQUILIBRIUM_INCOMPRESSIBLE) {
    const int c = p->desc.collision;
    if (p->set.field.a)
      return fail(LT_ERR_UNSUPPORTED, "the incompressible equilibrium on a plan with a force field "
                                      "(lt_plan_set_force_field): no kernel has the pair");
    if (c == LT_COLLISION_KBC || c == LT_COLLISION_SMAGORINSKY)
      return fail(LT_ERR_UNSUPPORTED, "the incompressible equilibrium has kernels for no collision, BGK (with or without a "
                                      "body force), TRT and the regularised collision; the plan's collision is %d (%s)", c,
                  c == LT_COLLISION_KBC ? "KBC" : "Smagorinsky");
    if (c == LT_COLLISION_MRT)
      return fail(LT_ERR_UNSUPPORTED, "the incompressible equilibrium and the MRT collision: an MRT transform carries its "
                                      "own (quadratic) equilibrium moments");
    if (p->desc.layout != LT_LAYOUT_REFERENCE || p->desc.ghost_planes)
      return fail(LT_ERR_UNSUPPORTED, "the incompressible equilibrium has kernels for the reference layout only, not for "
                                      "slab plans");
    for (int i = 0; i < p->desc.n_boundaries; ++i)
      if (p->desc.boundaries[i].kind == LT_BOUNDARY_PRESSURE_OUTLET)
        return fail(LT_ERR_UNSUPPORTED, "the incompressible equilibrium on a plan with a constant-pressure outlet "
                                        "(EquilibriumOutletP): that boundary evaluates the quadratic equilibrium in the kernel");
  }
  p->set.equilibrium = kind;
  p->set.rho0 = rho0;
  return LT_OK;
}

int lt_plan_set_two_step(lt_plan *p, int32_t mode, int32_t planes_per_workgroup) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (mode < -1 || mode > 1) return fail(LT_ERR_INVALID, "two-step mode %d", mode);
  if (mode == 1 && p->desc.collision == LT_COLLISION_MRT) return fail(LT_ERR_UNSUPPORTED, "two steps per launch: %s", kMrtMultiStep);
  if (mode == 1 && p->set.equilibrium == LT_EQUILIBRIUM_INCOMPRESSIBLE)
    return fail(LT_ERR_UNSUPPORTED, "two steps per launch: %s", kIncompressibleMultiStep);
  if (mode == 1 && p->n_link_kind > 0) return fail(LT_ERR_UNSUPPORTED, "two steps per launch with %s", kLinkMultiStep);
  if (mode == 1 && p->set.field.a) return fail(LT_ERR_UNSUPPORTED, "two steps per launch: %s", kForceFieldMultiStep);
  const int sweep = p->unit.d == 2 ? p->n1 : p->n2;          // extent of the sweep axis
  if (planes_per_workgroup < 0 ||
      (planes_per_workgroup > 0 && !p->desc.ghost_planes && sweep % planes_per_workgroup != 0))
    return fail(LT_ERR_INVALID, "planes per workgroup %d does not divide %d", planes_per_workgroup, sweep);
  if (p->seg_len != planes_per_workgroup) p->canary = 0;   // another segment length takes other paths of the sweep
  p->two_step = mode;
  p->seg_len = planes_per_workgroup;
  return LT_OK;
}

// ---- halo transport without compute units (include/lettuce_hip.h) -------------------------------------------------
int lt_halo_copy(void *dst, const void *src, int64_t n_bytes, int32_t engine, void *stream, int32_t *engine_used) {
  if (!dst || !src || n_bytes <= 0) return fail(LT_ERR_INVALID, "halo copy: null buffer or %lld bytes", (long long)n_bytes);
  hipStream_t hs = static_cast<hipStream_t>(stream);
  if (engine_used) *engine_used = 0;
  if (engine == 1) {
    // device-to-device WITHOUT compute units: the runtime hands the copy to an SDMA engine (over xGMI when dst is a
    // peer's mapped buffer) instead of launching a blit kernel
    if (hipMemcpyAsync(dst, src, (size_t)n_bytes, hipMemcpyDeviceToDeviceNoCU, hs) == hipSuccess) {
      if (engine_used) *engine_used = 1;
      return LT_OK;
    }
    (void)hipGetLastError();                 // not offered for this pair of buffers: the ordinary copy below
  }
  LT_HIP(hipMemcpyAsync(dst, src, (size_t)n_bytes, hipMemcpyDeviceToDevice, hs));
  return LT_OK;
}
int lt_flag_write(uint64_t *flag, uint64_t value, int32_t how, void *stream) {
  if (!flag) return fail(LT_ERR_INVALID, "null flag");
  hipStream_t hs = static_cast<hipStream_t>(stream);
  if (how == 1) {
    // a stream memory operation: the command processor writes the word when the stream gets there (no kernel)
    if (hipStreamWriteValue64(hs, flag, value, 0) == hipSuccess) return LT_OK;
    (void)hipGetLastError();
  }
  hipLaunchKernelGGL(write_flag_kernel, dim3(1), dim3(1), 0, hs, reinterpret_cast<unsigned long long *>(flag),
                     (unsigned long long)value);
  LT_HIP(hipGetLastError());
  return LT_OK;
}
int lt_flag_wait(const uint64_t *flag, uint64_t at_least, uint32_t *timed_out, void *stream) {
  if (!flag || !timed_out) return fail(LT_ERR_INVALID, "null flag / time-out word");
  hipLaunchKernelGGL(wait_flag_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const unsigned long long *>(flag), (unsigned long long)at_least, timed_out);
  LT_HIP(hipGetLastError());
  return LT_OK;
}
// Device memory other processes of the node can map (hipIpc*): the receive windows of the copy transport
int lt_ipc_alloc(int64_t n_bytes, int32_t fine_grained, void **dev_out, void *handle_out_64_bytes) {
  if (!dev_out || !handle_out_64_bytes || n_bytes <= 0) return fail(LT_ERR_INVALID, "ipc alloc: null argument or %lld bytes", (long long)n_bytes);
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "the handle travels as 64 bytes");
  void *p = nullptr;
  // fine_grained: memory that stays coherent with writers outside the running kernel (another device's copy engine or
  // command processor) -- for the arrival counters a polling wave reads while it runs; the messages themselves are
  // read by the NEXT launch and live in ordinary (cached) device memory
  const hipError_t ea = fine_grained ? hipExtMallocWithFlags(&p, (size_t)n_bytes, hipDeviceMallocFinegrained)
                                     : hipMalloc(&p, (size_t)n_bytes);
  if (ea != hipSuccess) { (void)hipGetLastError(); return fail(LT_ERR_ALLOC, "allocation of %lld bytes (ipc window%s) failed", (long long)n_bytes, fine_grained ? ", fine-grained" : ""); }
  hipIpcMemHandle_t h;
  const hipError_t e = hipIpcGetMemHandle(&h, p);
  if (e != hipSuccess) { (void)hipFree(p); return fail(LT_ERR_HIP, "hipIpcGetMemHandle failed: %s", hipGetErrorString(e)); }
  LT_HIP(hipMemset(p, 0, (size_t)n_bytes));
  memcpy(handle_out_64_bytes, &h, sizeof h);
  *dev_out = p;
  return LT_OK;
}
int lt_ipc_open(const void *handle_64_bytes, void **dev_out) {
  if (!handle_64_bytes || !dev_out) return fail(LT_ERR_INVALID, "ipc open: null argument");
  hipIpcMemHandle_t h;
  memcpy(&h, handle_64_bytes, sizeof h);
  LT_HIP(hipIpcOpenMemHandle(dev_out, h, hipIpcMemLazyEnablePeerAccess));
  return LT_OK;
}
int lt_ipc_close(void *mapped) {
  if (!mapped) return LT_OK;
  LT_HIP(hipIpcCloseMemHandle(mapped));
  return LT_OK;
}
int lt_ipc_free(void *dev) {
  if (!dev) return LT_OK;
  LT_HIP(hipFree(dev));
  return LT_OK;
}

int lt_plan_set_canary(lt_plan *p, int32_t mode) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (mode < 0 || mode > 2) return fail(LT_ERR_INVALID, "canary mode %d (0 skip, 1 check on first use, 2 report a mismatch)", mode);
  if (mode != p->canary_mode) p->canary = 0;
  p->canary_mode = mode;
  return LT_OK;
}
int lt_plan_canary_status(lt_plan *p, int32_t *status, int64_t *mismatches, const char **message) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (status) *status = p->canary;
  if (mismatches) *mismatches = p->canary_mismatches;
  if (message) *message = p->canary_msg;
  return LT_OK;
}

int lt_plan_set_residency(lt_plan *p, int32_t workgroups_per_cu) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (workgroups_per_cu < -1 || workgroups_per_cu == 1 || workgroups_per_cu > 8)
    return fail(LT_ERR_INVALID, "workgroups per CU %d (use -1, 0 or 2..8)", workgroups_per_cu);
  p->set.residency = workgroups_per_cu;
  return LT_OK;
}

int lt_plan_set_tuning(lt_plan *p, int32_t cache_policy, int32_t wide) {
  if (!p) return fail(LT_ERR_INVALID, "null plan");
  if (cache_policy < -1 || cache_policy > 3) return fail(LT_ERR_INVALID, "cache policy %d", cache_policy);
  if (wide)
    return fail(LT_ERR_UNSUPPORTED, "the 16-byte variants of the one-step kernel lost their A/B (8-13 %% slower) and "
                                    "were removed");
  p->set.tune = cache_policy;
  return LT_OK;
}

}  // extern "C"
