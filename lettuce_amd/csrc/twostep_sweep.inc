// The body of lbm2_kernel (kernels.hpp, which includes this text into the kernel on KParams and into the one on KParamsF
// -- a body force -- and describes the sweep above them): p = the kernel's parameters, seg_len = planes per workgroup.
  constexpr bool PACK = MODE == 1;
  static_assert(MODE == 0 || LAYOUT == 1, "edge / signalling launches exist in the slab layout");
  static_assert(NPT == 1 && NPB == 1, "one intermediate and one output node per thread");
  static_assert(SCHED == 0 || (SCHED == 1 && MODE == 0), "separate producer and consumer waves: the plain sweep");
  using B = TwoStep<T, S, T0_, T1>;
  using M = MemMap<S, LAYOUT>;
  constexpr int T0 = B::T0, H0 = B::H0, NI = B::NI, NO = B::NO;
  constexpr int NU = B::template count<LAYOUT, 1>(), NC = B::template count<LAYOUT, 0>(),
                ND = B::template count<LAYOUT, -1>();
  static_assert(COLL == kCollNone || COLL == kCollBgk || COLL == kCollSmagorinsky || coll_forced(COLL) || COLL == kCollTrt ||
                    COLL == kCollRegularized,
                "two-step kernel: streaming only, BGK or Smagorinsky, the latter two also with a body force, TRT, regularised");
  static_assert(COLL == kCollNone || COLL == kCollBgk || (SCHED == 0 && MODE == 0),
                "Smagorinsky, body force, TRT, regularised: the plain one-role sweep only");
  __shared__ T lds_u[4][NU][NI];
  __shared__ T lds_c[3][NC][NI];
  __shared__ T lds_d[2][ND][NI];

  const int tid = threadIdx.x;
  const int tiles0 = p.n0 / T0, tiles1 = p.n1 / T1;
  // Workgroups go to the 8 XCDs round-robin (block b -> XCD b % 8) and every XCD has its own L2.
  // Renumber so that an XCD owns a compact patch of neighbouring tiles: the halo rows two tiles
  // share are then fetched into one L2 once instead of into two L2s.
  int b = blockIdx.x;
  const int segs_a = (p.p_end - p.p_begin + seg_len - 1) / seg_len;
  if (MODE == 2) {
    // edges first (the hardware starts workgroups in index order): upper edge = the one segment of the second
    // range, then the first segment of the first range, then the rest with the XCD-aware numbering
    // (XCD-aware within each layer of tiles)
    const int tiles = tiles0 * tiles1;
    const int layer = b / tiles, t = b - layer * tiles;
    const int tile = tiles % 8 == 0 ? (t % 8) * (tiles / 8) + t / 8 : t;
    b = (layer == 0 ? segs_a : layer - 1) * tiles + tile;
  } else if (p.nb == 0 && (tiles0 * tiles1) % 8 == 0) {
    // every XCD gets an eighth of EVERY segment layer -- a compact patch of tiles -- rather than an eighth of
    // the grid: slab launches cut their plane range into segments of unequal length (64 planes as 62 + 2: four
    // XCDs had all the long workgroups, 1.00 instead of 0.55 ms), and with equal segments it is as good or
    // better (256^3: 0.511 / 0.537 / 0.532 against 0.512 / 0.572 / 0.579 ms with 128 / 64 / 32 planes)
    const int tiles = tiles0 * tiles1;
    const int layer = b / tiles, t = b - layer * tiles;
    b = layer * tiles + (t % 8) * (tiles / 8) + t / 8;
  } else if (p.nb != 1 && gridDim.x % 8 == 0) {
    b = (b % 8) * (gridDim.x / 8) + b / 8;           // A/B (nb = 2), or tiles that do not divide by 8
  }
  const int t0 = (b % tiles0) * T0; b /= tiles0;
  const int t1 = (b % tiles1) * T1; b /= tiles1;
  // first output plane of this workgroup: segments of the first range, then of the second one
  const bool second = b >= segs_a;
  const int range_end = second ? p.p_end2 : p.p_end;
  const int s = second ? p.p_begin2 + (b - segs_a) * seg_len : p.p_begin + b * seg_len;

  const bool in_a = tid < NI, in_b = tid < NO;
  // Addresses: the plane part is uniform (scalar registers, recomputed per plane), the in-plane
  // part is a per-thread constant -- nine byte offsets for the nine (e0, e1) pairs of the lattice.
  unsigned voff[NPT][3][3];                          // [k][e1 + 1][e0 + 1], bytes within a plane
  unsigned out_off[NPB];
  int a_at[NPT];                                     // LDS index of the intermediate node
  int b_at[NPB];                                     // LDS index of the output node incl. halo offset
  static_for<NPT>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    // phase A: node (i0, i1) of the halo'd tile, global coordinates (g0, g1).  The T0 inner columns
    // of a row go to T0 consecutive threads (a wave reads one aligned 256-byte row segment per
    // population), the two halo columns of all rows to the last threads.
    const int ia = tid + k * NI;
    constexpr int inner = T0 * B::H1;
    const int i1 = ia < inner ? ia / T0 : (ia - inner) >> 1;
    const int i0 = ia < inner ? 1 + (ia - i1 * T0) : (((ia - inner) & 1) ? H0 - 1 : 0);
    a_at[k] = i1 * H0 + i0;
    int g0 = t0 + i0 - 1; g0 = g0 < 0 ? g0 + p.n0 : (g0 >= p.n0 ? g0 - p.n0 : g0);
    int g1 = t1 + i1 - 1; g1 = g1 < 0 ? g1 + p.n1 : (g1 >= p.n1 ? g1 - p.n1 : g1);
    const int g0m = g0 == 0 ? p.n0 - 1 : g0 - 1, g0p = g0 == p.n0 - 1 ? 0 : g0 + 1;
    const int g1m = g1 == 0 ? p.n1 - 1 : g1 - 1, g1p = g1 == p.n1 - 1 ? 0 : g1 + 1;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int y = a == 0 ? g1p : (a == 1 ? g1 : g1m);     // source = node - e
        const int x = c == 0 ? g0p : (c == 1 ? g0 : g0m);
        voff[k][a][c] = ((unsigned)y * (unsigned)p.n0 + (unsigned)x) * (unsigned)sizeof(T);
      }
  });
  static_for<NPB>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    // phase B: output node (j0, j1) of the tile
    const int ib = tid + k * NO;
    const int j1 = ib / T0, j0 = ib - j1 * T0;
    out_off[k] = ((unsigned)(t1 + j1) * (unsigned)p.n0 + (unsigned)(t0 + j0)) * (unsigned)sizeof(T);
    b_at[k] = (j1 + 1) * H0 + (j0 + 1);
  });
  const unsigned plane_nodes = (unsigned)p.n1 * (unsigned)p.n0;

  if constexpr (SCHED == 1) {
    // Producer waves run phase A only, consumer waves phase B only (twostep_roles.hpp: the skeleton both run, the
    // wave layout).  A SIMD then holds waves in different phases -- a consumer colliding while the producers wait
    // for their loads, producers colliding while the consumer waits for LDS -- instead of three waves that wait at
    // the same moments.  Per node the arithmetic and its order are those of SCHED 0.
    using R = RoleWaves<NI, NO>;
    constexpr int CPB = R::CPB, CT = NO / CPB;
    const int last = s + seg_len < range_end ? s + seg_len : range_end;
    auto sync = [&]() { lds_barrier(); };
    if (__builtin_amdgcn_readfirstlane(tid >> 6) < R::PW) {
      // Every lane loads (those without an intermediate node read the plane's first node): under `if (in_a)` the
      // other lanes' registers are undefined, the compiler zeroes them AFTER the loads and that write waits for them.
      if (!in_a) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int c = 0; c < 3; ++c) voff[0][a][c] = 0u;
      }
      T set0[S::Q][1], set1[S::Q][1];
      auto load = [&](int plane, auto set) {
        T (&dst)[S::Q][1] = decltype(set)::value == 0 ? set0 : set1;
        int g2 = plane, g2m = plane - 1, g2p = plane + 1;
        if (p.wrap2) {
          g2 = plane < 0 ? plane + p.n2 : (plane >= p.n2 ? plane - p.n2 : plane);
          g2m = g2 == 0 ? p.n2 - 1 : g2 - 1;
          g2p = g2 == p.n2 - 1 ? 0 : g2 + 1;
        }
        static_for<S::Q>([&](auto qc) {
          constexpr int q = decltype(qc)::value;
          constexpr int e0 = M::e(q, 0), e1 = M::e(q, 1), e2 = M::e(q, 2);
          const int z = e2 == 0 ? g2 : (e2 > 0 ? g2m : g2p);
          const T *base = p.in + ((long long)q * p.Ni + (long long)((unsigned)z * plane_nodes));
          dst[q][0] = *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + voff[0][e1 + 1][e0 + 1]);
        });
        // (the register-minimising scheduler sinks the loads behind the collide of the other set otherwise)
        __builtin_amdgcn_sched_barrier(0);
      };
      auto fill = [&](int r, int r3, auto set) {
        T (&src)[S::Q][1] = decltype(set)::value == 0 ? set0 : set1;
        collide_node<T, S, LAYOUT, 1, 0, COLL>(src, p);
        if (in_a) {
          static_for<S::Q>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            constexpr int e2 = M::e(q, 2), rank = crossing_rank<S, LAYOUT, q>();
            if constexpr (e2 > 0) lds_u[r & 3][rank][a_at[0]] = src[q][0];
            else if constexpr (e2 == 0) lds_c[r3][rank][a_at[0]] = src[q][0];
            else lds_d[r & 1][rank][a_at[0]] = src[q][0];
          });
        }
        __builtin_amdgcn_sched_barrier(0);
      };
      role_sweep(s, last, load, fill, sync, [](int, int) {}, [](int) {});
    } else {
      // consumer thread c of CT owns the output nodes c, c + CT, ... of the tile: a wave reads whole rows
      const int c = tid - R::PW * 64;
      unsigned c_off[CPB];
      int c_at[CPB];
      static_for<CPB>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        const int ib = c + k * CT;
        const int j1 = ib / T0, j0 = ib - j1 * T0;
        c_off[k] = ((unsigned)(t1 + j1) * (unsigned)p.n0 + (unsigned)(t0 + j0)) * (unsigned)sizeof(T);
        c_at[k] = (j1 + 1) * H0 + (j0 + 1);
      });
      T f[S::Q][CPB];
      auto drain = [&](int r, int r3) {
        static_for<S::Q>([&](auto qc) {
          constexpr int q = decltype(qc)::value;
          constexpr int e0 = M::e(q, 0), e1 = M::e(q, 1), e2 = M::e(q, 2), rank = crossing_rank<S, LAYOUT, q>();
          static_for<CPB>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            const int at = c_at[k] - e1 * H0 - e0;
            if constexpr (e2 > 0) f[q][k] = lds_u[(r - 1) & 3][rank][at];
            else if constexpr (e2 == 0) f[q][k] = lds_c[r3][rank][at];
            else f[q][k] = lds_d[(r + 1) & 1][rank][at];
          });
        });
      };
      auto emit = [&](int k2) {
        static_for<CPB>([&](auto kc) { collide_node<T, S, LAYOUT, CPB, decltype(kc)::value, COLL>(f, p); });
        static_for<S::Q>([&](auto qc) {
          constexpr int q = decltype(qc)::value;
          T *base = p.out + ((long long)q * p.No + (long long)((unsigned)k2 * plane_nodes));
          static_for<CPB>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            __builtin_nontemporal_store(f[q][k], reinterpret_cast<T *>(reinterpret_cast<char *>(base) + c_off[k]));
          });
        });
      };
      role_sweep(s, last, [](int, auto) {}, [](int, int, auto) {}, sync, drain, emit);
    }
    return;
  }
  T pre[S::Q][NPT];
  auto load_a = [&](int plane) {
    // periodic along a2, or a slab whose ghost planes (two per side) hold the neighbours' data
    int g2 = plane, g2m = plane - 1, g2p = plane + 1;
    if (p.wrap2) {
      g2 = plane < 0 ? plane + p.n2 : (plane >= p.n2 ? plane - p.n2 : plane);
      g2m = g2 == 0 ? p.n2 - 1 : g2 - 1;
      g2p = g2 == p.n2 - 1 ? 0 : g2 + 1;
    }
    if (in_a) {
      static_for<S::Q>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        constexpr int e0 = M::e(q, 0), e1 = M::e(q, 1), e2 = M::e(q, 2);
        const int z = e2 == 0 ? g2 : (e2 > 0 ? g2m : g2p);
        // 32-bit scalar multiply (a plane's first node index fits: N < 2^31), 64-bit scalar add
        const T *base = p.in + ((long long)q * p.Ni + (long long)((unsigned)z * plane_nodes));
        if constexpr (MODE == 1) {
          // Planes beyond a cut: the neighbour's populations as they arrived (halo2_kernel's message: in-plane
          // populations of its plane next to the cut | the crossing ones of that plane | the crossing ones of the
          // plane behind it).  The plane index is uniform, so this is scalar work; the populations moving away
          // from a cut are never pulled across it.
          constexpr int rank = crossing_rank<S, LAYOUT, q>();
          if constexpr (e2 >= 0) {
            if (p.ghost_lo != nullptr && z < p.lo)
              base = p.ghost_lo + (size_t)(e2 == 0 ? rank : (z == p.lo - 1 ? NC + rank : NC + NU + rank)) * plane_nodes;
          }
          if constexpr (e2 <= 0) {
            if (p.ghost_hi != nullptr && z >= p.hi)
              base = p.ghost_hi + (size_t)(e2 == 0 ? rank : (z == p.hi ? NC + rank : NC + ND + rank)) * plane_nodes;
          }
        }
        static_for<NPT>([&](auto kc) {
          constexpr int k = decltype(kc)::value;
          pre[q][k] = *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + voff[k][e1 + 1][e0 + 1]);
        });
      });
    }
  };
  // r = index of the plane relative to s - 1; r3 = r % 3
  auto compute_a = [&](int r, int r3) {
    if (in_a) {
      static_for<NPT>([&](auto kc) { collide_node<T, S, LAYOUT, NPT, decltype(kc)::value, COLL>(pre, p); });
      static_for<S::Q>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        constexpr int e2 = M::e(q, 2), rank = crossing_rank<S, LAYOUT, q>();
        static_for<NPT>([&](auto kc) {
          constexpr int k = decltype(kc)::value;
          if constexpr (e2 > 0) lds_u[r & 3][rank][a_at[k]] = pre[q][k];
          else if constexpr (e2 == 0) lds_c[r3][rank][a_at[k]] = pre[q][k];
          else lds_d[r & 1][rank][a_at[k]] = pre[q][k];
        });
      });
    }
  };
  T f[S::Q][NPB];
  auto read_b = [&](int r, int r3) {                 // output plane with relative index r
    if (in_b) {
      static_for<S::Q>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        constexpr int e0 = M::e(q, 0), e1 = M::e(q, 1), e2 = M::e(q, 2), rank = crossing_rank<S, LAYOUT, q>();
        static_for<NPB>([&](auto kc) {
          constexpr int k = decltype(kc)::value;
          const int at = b_at[k] - e1 * H0 - e0;
          if constexpr (e2 > 0) f[q][k] = lds_u[(r - 1) & 3][rank][at];
          else if constexpr (e2 == 0) f[q][k] = lds_c[r3][rank][at];
          else f[q][k] = lds_d[(r + 1) & 1][rank][at];
        });
      });
    }
  };
  auto collide_b = [&]() {
    if (in_b) {
      static_for<NPB>([&](auto kc) { collide_node<T, S, LAYOUT, NPB, decltype(kc)::value, COLL>(f, p); });
    }
  };
  // packing: this workgroup writes halo messages (PACK kernels; a launch that covers a whole slab runs the
  // sweep of its other workgroups without that code -- with it in the loop they took twice as long)
  // how: 0 = nontemporal stores; 1 = also the halo messages (PACK kernels); 2 = stores that are performed at
  // device scope (write-through: another XCD's kernel may read them while this launch still runs)
  auto store_b = [&](int k2, auto how) {
    constexpr int HOW = decltype(how)::value;
    constexpr bool PACKING = HOW == 1;
    if (in_b) {
      static_for<S::Q>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        T *base = p.out + ((long long)q * p.No + (long long)((unsigned)k2 * plane_nodes));
        static_for<NPB>([&](auto kc) {
          constexpr int k = decltype(kc)::value;
          T *at = reinterpret_cast<T *>(reinterpret_cast<char *>(base) + out_off[k]);
          if constexpr (HOW == 2) {
            using Bits = std::conditional_t<sizeof(T) == 4, unsigned, unsigned long long>;
            __hip_atomic_store(reinterpret_cast<Bits *>(at), __builtin_bit_cast(Bits, f[q][k]), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
          } else {
            __builtin_nontemporal_store(f[q][k], at);
          }
        });
        // Slab edge launches (PACK) also write the two-step halo message (layout of halo2_kernel: in-plane
        // populations of the plane next to the cut | its crossing populations | the crossing
        // populations of the plane behind it), possibly straight into the neighbour's memory.
        constexpr int e2 = M::e(q, 2), rank = crossing_rank<S, LAYOUT, q>();
        if constexpr (PACKING) {
        if (p.pack_lo != nullptr && e2 <= 0) {
          const int d = k2 - p.pack_lo_plane;                    // 0: near plane, 1: far plane
          if (d == 0 || (d == 1 && e2 < 0)) {
            const int slot = e2 == 0 ? rank : (d == 0 ? NC + rank : NC + ND + rank);
            T *msg = p.pack_lo + (size_t)slot * plane_nodes;
            static_for<NPB>([&](auto kc) {
              constexpr int k = decltype(kc)::value;
              *reinterpret_cast<T *>(reinterpret_cast<char *>(msg) + out_off[k]) = f[q][k];
            });
          }
        }
        if (p.pack_hi != nullptr && e2 >= 0) {
          const int d = p.pack_hi_plane - k2;
          if (d == 0 || (d == 1 && e2 > 0)) {
            const int slot = e2 == 0 ? rank : (d == 0 ? NC + rank : NC + NU + rank);
            T *msg = p.pack_hi + (size_t)slot * plane_nodes;
            static_for<NPB>([&](auto kc) {
              constexpr int k = decltype(kc)::value;
              *reinterpret_cast<T *>(reinterpret_cast<char *>(msg) + out_off[k]) = f[q][k];
            });
          }
        }
        }
      });
    }
  };

  // intermediate planes s-1 .. s+seg_len are needed (relative indices 0 .. seg_len+1)
  const int last = s + seg_len < range_end ? s + seg_len : range_end;
  if constexpr (PACK) {
    if (last - s == 2) {
      // Slab edge launch: two output planes per workgroup, i.e. four intermediate planes and no sweep to amortise a
      // serial prologue over, with all 256 workgroups of a round in lock-step (memory idle while they collide, compute
      // units idle while they load).  Straight-line schedule on two register sets with the loads of plane j + 1 in
      // flight behind the collide of plane j -- what the steady state of the sweep does.  Every thread loads (the 44
      // of 704 without an intermediate node read the plane's first node): a load under `if (in_a)` leaves the other
      // lanes' registers undefined, the compiler zeroes them AFTER the loads and that write waits for the loads.
      if (!in_a) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int c = 0; c < 3; ++c) voff[0][a][c] = 0u;
      }
      auto load_into = [&](int plane, T (&dst)[S::Q][1]) {
        const int g2 = plane, g2m = plane - 1, g2p = plane + 1;      // slab layout: no wrap along a2
        static_for<S::Q>([&](auto qc) {
          constexpr int q = decltype(qc)::value;
          constexpr int e0 = M::e(q, 0), e1 = M::e(q, 1), e2 = M::e(q, 2), rank = crossing_rank<S, LAYOUT, q>();
          const int z = e2 == 0 ? g2 : (e2 > 0 ? g2m : g2p);
          const T *base = p.in + ((long long)q * p.Ni + (long long)((unsigned)z * plane_nodes));
          if constexpr (e2 >= 0) {
            if (p.ghost_lo != nullptr && z < p.lo)
              base = p.ghost_lo + (size_t)(e2 == 0 ? rank : (z == p.lo - 1 ? NC + rank : NC + NU + rank)) * plane_nodes;
          }
          if constexpr (e2 <= 0) {
            if (p.ghost_hi != nullptr && z >= p.hi)
              base = p.ghost_hi + (size_t)(e2 == 0 ? rank : (z == p.hi ? NC + rank : NC + ND + rank)) * plane_nodes;
          }
          dst[q][0] = *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + voff[0][e1 + 1][e0 + 1]);
        });
      };
      // KEEP: which populations of the plane anybody reads -- bit 0: those moving up (the output plane above pulls
      // them), bit 1: in-plane, bit 2: moving down.  The first intermediate plane only feeds the output plane above
      // it, the last one only the plane below: 38 of the 76 post-collision populations of the four planes are needed,
      // the others are neither stored nor (dead code to the compiler) computed.
      auto collide_into_lds = [&](T (&src)[S::Q][1], int r, int r3, auto keep) {
        constexpr int KEEP = decltype(keep)::value;
        collide_node<T, S, LAYOUT, 1, 0, COLL>(src, p);
        if (in_a) {
          static_for<S::Q>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            constexpr int e2 = M::e(q, 2), rank = crossing_rank<S, LAYOUT, q>();
            if constexpr (e2 > 0) { if constexpr (KEEP & 1) lds_u[r & 3][rank][a_at[0]] = src[q][0]; }
            else if constexpr (e2 == 0) { if constexpr (KEEP & 2) lds_c[r3][rank][a_at[0]] = src[q][0]; }
            else { if constexpr (KEEP & 4) lds_d[r & 1][rank][a_at[0]] = src[q][0]; }
          });
        }
      };
      using Up = std::integral_constant<int, 1>;
      using UpIn = std::integral_constant<int, 3>;
      using InDown = std::integral_constant<int, 6>;
      using Down = std::integral_constant<int, 4>;
      // (sched_barrier: the register-minimising scheduler of this unit sinks the loads behind the collide otherwise)
      T pre2[S::Q][1];
      load_into(s - 1, pre); load_into(s, pre2);
      __builtin_amdgcn_sched_barrier(0);
      collide_into_lds(pre, 0, 0, Up{});
      __builtin_amdgcn_sched_barrier(0);
      load_into(s + 1, pre);
      __builtin_amdgcn_sched_barrier(0);
      collide_into_lds(pre2, 1, 1, UpIn{});
      __builtin_amdgcn_sched_barrier(0);
      load_into(s + 2, pre2);
      __builtin_amdgcn_sched_barrier(0);
      collide_into_lds(pre, 2, 2, InDown{});
      lds_barrier();
      read_b(1, 1);
      collide_into_lds(pre2, 3, 0, Down{});
      collide_b();
      store_b(s, std::integral_constant<int, 1>{});
      lds_barrier();
      read_b(2, 2);
      collide_b();
      store_b(s + 1, std::integral_constant<int, 1>{});
      return;
    }
  }
  load_a(s - 1); compute_a(0, 0);
  load_a(s);     compute_a(1, 1);
  load_a(s + 1); compute_a(2, 2);
  if (s + 2 <= last) load_a(s + 2);
  int r = 1, r3 = 1;                                  // output plane k has relative index k - s + 1
  auto interval = [&](int k, auto how) {
    lds_barrier();                                    // planes up to k + 1 complete; reads of k - 1 done
    read_b(r, r3);                                    // 19 LDS reads in flight ...
    if (k + 2 <= last) {
      compute_a(r + 2, r3 == 0 ? 2 : r3 - 1);         // ... behind the collide of plane k + 2; (r + 2) % 3
      if (k + 3 <= last) load_a(k + 3);
    }
    collide_b();
    store_b(k, how);
    ++r;
    r3 = r3 == 2 ? 0 : r3 + 1;
  };
  int k = s;
  using Plain = std::integral_constant<int, 0>;
  if constexpr (PACK) {
    // edge launches: every workgroup also writes the halo messages.  (This copy of the loop is slow -- 12 spilled
    // registers, message stores -- and even its presence slows the other copy: a launch over the whole slab
    // with packing first segments took 1.0 instead of 0.6 ms, so that launch does not pack.)
    for (; k < last; ++k) interval(k, std::integral_constant<int, 1>{});
  } else if constexpr (MODE == 2) {
    if (second || b == 0) {
      // Launch over the whole slab: the planes next to a cut are this workgroup's last two (upper edge) or first
      // two (lower edge).  They are stored at device scope, and once the stores have been performed the
      // workgroup counts itself done.  No release fence: at device scope that is a write-back of the XCD's
      // whole L2 -- 1024 of them made the launch take 0.99 instead of 0.66 ms.
      const int until = second ? last : (s + 2 < last ? s + 2 : last);
      for (; k < until; ++k) interval(k, std::integral_constant<int, 2>{});
      // every wave waits until ITS edge-plane stores have been acknowledged (they are write-through stores at
      // device scope, so the acknowledgement means "performed in memory"): a workgroup-scope release alone emits
      // no vmcnt wait on gfx950, and the counter below must not become visible before the planes are
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __syncthreads();
      if (tid == 0) __hip_atomic_fetch_add(p.signal, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  for (; k < last; ++k) interval(k, Plain{});
