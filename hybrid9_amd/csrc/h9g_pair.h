// h9g_pair.h -- HYDROLOGY substep with two lanes per soil column.
//
// Why: the 0.5 deg grid has 67,420 land cells, i.e. 1,054 one-lane waves
// for 1,024 SIMDs.  One wave per SIMD leaves VALU issue and LDS latency
// exposed (a lone wave64 issues at most every 4 cycles; the SIMD can take
// one every 2), and the 30 surplus waves double up on 30 SIMDs and set the
// kernel time.  Giving each column two lanes ("a pair": lanes 2k, 2k+1 of
// a wave) halves the per-lane share of the work that is independent per
// layer -- the equilibrium profile zq (HYDROLOGY.f90:517-590), hydraulic
// conductivity and matric potential (:598-639) and the specific yields
// (:937-981), i.e. 40 of the ~46 glibc-exact powf of a substep -- and
// lets 22 columns per wave x 4-wave workgroups place exactly 3 waves on
// every SIMD (767 workgroups for 768 slots at 0.5 deg).
//
// Layer split: lane h (0 = even, 1 = odd) of a pair owns layers 2t+1+h,
// t = 0..L/2-1.  A per-layer phase evaluates the reference expression for
// the lane's own layers and swaps the results with the partner lane (DPP
// quad_perm [1,0,3,2]); the tridiagonal system's interface fluxes are split
// the same way, interface 2t+1+h on lane h (H9G_FLUX_SPLIT); everything
// else (Thomas solve, drainage, ...) runs identically in both lanes.
// Every value is computed by exactly the reference expression, so the
// split changes no bit.
//
// One code path serves three builds through two policies:
//   Split2   device fast path: own layers per lane + DPP exchange;
//   SplitAll one lane computes every layer: the device exact re-run
//            (MathExact) and the host test build (tests/csrc/host_kernel.cpp).
// Stores: PairStore (device LDS, [row][lane] with the pair's layers
// interleaved over its two columns) and FlatStore (host, flat per cell).
#pragma once
#include <type_traits>

#include "h9g_step.h"
#include "h9g_expr.h"
#if !defined(__HIPCC__) && !defined(__HIP__)
#define __device__
#define __forceinline__ inline
#endif

#ifndef H9G_EXACT_HOOK
#define H9G_EXACT_HOOK(k0, ns)         // test builds: count the exact re-runs (tests/csrc/host_kernel.cpp)
#endif
#if defined(H9G_COUNT_EXACT)
__device__ unsigned long long h9g_exact_count;   // exact re-runs (lanes), measurement builds only
__device__ unsigned h9g_exact_wave[1 << 16];     // ... per wave (blockIdx * 4 + wave), pair kernel
#endif
namespace h9k {

// per-layer store fields (L entries each)
enum : int {
  PF_TS = 0, PF_HKS, PF_BSW, PF_PSI,   // soil parameters (SHARED.f90:398-429)
  PF_NINVB,                            // -one/bsw
  PF_ITS,                              // one/(ts(I)+ts(I+1))
  PF_PTE,                              // psi*ts/(one-one/bsw)
  PF_C3,                               // pte/(zi(I)-zi(I-1))
  PF_ROOTR,                            // rootr_col(1..L)
  PF_RPSI0, PF_RPSI1,                  // 1/(-psi), double (recip64) low, high word   (kRecip)
  PF_RTS0, PF_RTS1,                    // 1/theta_s, double                           (kRts)
  PF_SVH2O, PF_SVSMP,                  // day snapshot (sv_* of the store)
  PF_N
};
// per-cell fields
enum : int {
  PS_FMAX = 0, PS_MH3, PS_TSDZ1, PS_DAY,
  PS_LAI = PS_DAY + D_N,               // plant state, parked over the substeps (pair kernel)
  PS_LAIL, PS_PM, PS_PFM, PS_PLEN, PS_RDEPTH,
  PS_DR0,                              // day-constant reciprocals (kDayRecip): pairs
  PS_DRS = PS_DR0 + 4 * DRP_N,         //   (c.lo s.lo c.hi s.hi), then shared doubles (lo hi)
  PS_SVZWT = PS_DR0 + 2 * DR_N,        // day snapshot for the exact re-run (sv_* of the store)
  PS_SVWA, PS_SVRNF, PS_SVERR, PS_SVNS,
  PS_SVEVAP,                           // (the ET kernels only: EvapProf)
  PS_N
};
// sv_sc fields (SV_NS: substep of the snapshot; SV_EVAP: the evaporation sum, stored and read by the ET kernels only)
enum : int { SV_ZWT = 0, SV_WA, SV_RNF, SV_ERR, SV_NS, SV_EVAP };
// canopy/soil pairs share a row, canopy in the even column (see D_NUMC)
static_assert((PS_DAY + D_NUMC) % 2 == 0 && (PS_DAY + D_RAARAC) % 2 == 0 && (PS_DAY + D_DGRAC) % 2 == 0 &&
                  (PS_DAY + D_DRR) % 2 == 0 && (PS_DAY + D_RAC) % 2 == 0 && PS_DR0 % 2 == 0,
              "pair fields must start a row");

#ifndef H9G_EB_FAST
#define H9G_EB_FAST 1    // round 5: 182.2 -> 181.7 ms; the energy balance's quotients branch-free, runtime divisors by Markstein (hydrology_pair); 0: the exact block alone (tests)
#endif
// The one-column wave's task lanes (hydrology_pair kTask), a sum of
//   1  its powers as two task rounds, a power per lane (rounds A and B, round 7)
//   2  round C: the tridiagonal system's interface fluxes, a lane per interface
//   4  the forward sweep's quotients by mk_div from one refined reciprocal per row
// 2 and 4 need 1; 0 compiles the wave as the 11- and 22-column kernels' helper rounds.
#ifndef H9G_P1_TASKS
#define H9G_P1_TASKS 7
#endif
// The one-column kernel's second wave per column (front_year_pair): lists of at
// most H9G_PAIR1_FRONT_MAX cells run two waves per column, the front of the
// substep on a wave of its own beside the per-layer rounds.  0 builds the
// single-wave kernel only.
#ifndef H9G_P1_FRONT
#define H9G_P1_FRONT 1
#endif
// hydrology_pair's part of the substep: all of it; the front alone (everything
// up to the equilibrium profile but theta(2..L): fsat, the beta terms, rss, the
// energy balance, em1, infiltration), returning its results in FrontRes; or
// everything but the front, which takes those results from the store's
// hand-over rows behind a workgroup barrier.
// Round 10, the two-wave shape's water-table chain (recharge through the zwt
// clamps, HYDROLOGY.f90:856-1123): in a substep that starts with the water
// table in the column it reads nothing the sweep produces, so the second wave
// evaluates it too (ROLE_CHAIN, after its front) while the main wave
// (ROLE_MAINS) sweeps, and hands the new zwt, wa, rsub_top, jwt and the
// drainage loop's h2osoi_liq deltas over behind a third barrier
// (front_year_pair).  H9G_P1_SIDE=0 builds round 9's two-wave kernel.
#ifndef H9G_P1_SIDE
#define H9G_P1_SIDE 1
#endif
#if !H9G_P1_FRONT || (H9G_P1_TASKS & 3) != 3   // the chain's operands are round A's and round C's
#undef H9G_P1_SIDE
#define H9G_P1_SIDE 0
#endif
// The tridiagonal system's interface fluxes as a third pair-split phase
// (hydrology_pair, "the interface fluxes, split"): lane h of a pair evaluates
// interface 2t+1+h in slot t instead of both lanes evaluating all of them, in
// every store with kFluxSplit.  0 builds every kernel with the block that both
// lanes evaluate whole.
#ifndef H9G_FLUX_SPLIT
#define H9G_FLUX_SPLIT 1
#endif
enum : int { ROLE_ALL = 0, ROLE_FRONT = 1, ROLE_MAIN = 2, ROLE_CHAIN = 3, ROLE_MAINS = 4 };
struct FrontRes {
  float qflx_surf, tran, evg, qflx_infl;
};

template <int K>
struct FV {
  float v[K];
};

H9K_HD float sel(int h, float a, float b) { return h ? b : a; }
H9K_HD double seld(int h, double a, double b) { return h ? b : a; }

// value of the partner lane (lane ^ 1)
H9K_HD float pair_swap(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int x = __builtin_bit_cast(int, v);
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false));
#else
  return v;
#endif
}

// value of the pair's even (E = 0) or odd (E = 1) lane, in both lanes (DPP
// quad_perm [0,0,2,2] / [1,1,3,3]): one instruction instead of pair_swap
// plus a select per lane
template <int E>
H9K_HD float pair_bcast(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int x = __builtin_bit_cast(int, v);
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(x, E ? 0xF5 : 0xA0, 0xF, 0xF, true));
#else
  return v;
#endif
}

// value of lane `src` of the wave (ds_bpermute: the LDS crossbar, no LDS
// storage); the spare lanes' operands and results (hydrology_pair)
H9K_HD float lane_get(float v, int src) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src << 2, __builtin_bit_cast(int, v)));
#else
  (void)src;
  return v;
#endif
}
H9K_HD int lane_geti(int v, int src) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_ds_bpermute(src << 2, v);
#else
  (void)src;
  return v;
#endif
}

// value of the wave's lane 0, wave-uniform (v_readlane: no LDS crossbar); the
// one-column wave's starting state for its task lanes (hydrology_pair)
H9K_HD float lane0_get(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
#else
  return v;
#endif
}
H9K_HD int lane0_geti(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_readlane(v, 0);
#else
  return v;
#endif
}
// lanes of the wave where p holds (host: bit 0)
H9K_HD uint64_t lane_mask(bool p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_ballot_w64(p);
#else
  return p ? 1u : 0u;
#endif
}

// A double kept as two float fields (low word, high word).
H9K_HD double join_d(float lo, float hi) {
  return __builtin_bit_cast(double, (uint64_t)__builtin_bit_cast(uint32_t, hi) << 32 |
                                        __builtin_bit_cast(uint32_t, lo));
}
H9K_HD float lo_d(double v) { return __builtin_bit_cast(float, (uint32_t)__builtin_bit_cast(uint64_t, v)); }
H9K_HD float hi_d(double v) {
  return __builtin_bit_cast(float, (uint32_t)(__builtin_bit_cast(uint64_t, v) >> 32));
}

// ------------------------------------------------------------------ stores
// Every store has the same interface: lay/set_lay (per-layer field p of
// layer i), sc/set_sc (per-cell field k), slot/set_slot (own layer t of a
// pair lane), day/set_day, the day reciprocals day_r/set_day_r, and the
// day snapshot sv_* (q = 0: h2osoi_liq, 1: smp; k = SV_*).  kRecip,
// kRts, kDayRecip say which reciprocal fields it holds (LDS budget).
template <int L>
struct FlatStore {                     // host: one flat array per cell
  static constexpr bool kRecip = true, kRts = true, kDayRecip = true, kRtsHK = true, kSpare = false, kFront = false;
  static constexpr bool kFluxSplit = true;           // the interface fluxes by pair parity (H9G_FLUX_SPLIT): the device pair kernels' text
  static constexpr int N = PF_N * L + PS_N;
  float *b;
  const float *zt;                     // zi(0..L+1), then zi(0..L+1)/1000
  H9K_HD float zi(int i) const { return zt[i]; }
  H9K_HD float zim(int i) const { return zt[L + 2 + i]; }
  H9K_HD double rdz_t(int i) const { return join_d(zt[2 * (L + 2) + 2 * i], zt[2 * (L + 2) + 2 * i + 1]); }
  H9K_HD float lay(int p, int i) const { return b[p * L + i - 1]; }
  H9K_HD void set_lay(int p, int i, float v) const { b[p * L + i - 1] = v; }
  H9K_HD float sc(int k) const { return b[PF_N * L + k]; }
  H9K_HD void set_sc(int k, float v) const { b[PF_N * L + k] = v; }
  H9K_HD float slot(int p, int t) const { return b[p * L + 2 * t]; }   // unused (SplitAll)
  H9K_HD void set_slot(int p, int t, float v) const { b[p * L + 2 * t] = v; }
  H9K_HD void launder() {}
  H9K_HD float day(int f) const { return sc(PS_DAY + f); }
  H9K_HD void set_day(int f, float v) const { set_sc(PS_DAY + f, v); }
  H9K_HD double day_r(int k) const { return join_d(sc(PS_DRS + 2 * k), sc(PS_DRS + 2 * k + 1)); }
  H9K_HD void set_day_r(int k, double v) const {
    set_sc(PS_DRS + 2 * k, lo_d(v));
    set_sc(PS_DRS + 2 * k + 1, hi_d(v));
  }
  H9K_HD double day_rp(int j, int h) const { return join_d(sc(PS_DR0 + 4 * j + h), sc(PS_DR0 + 4 * j + 2 + h)); }
  H9K_HD void set_day_rp(int j, int h, double v) const {
    set_sc(PS_DR0 + 4 * j + h, lo_d(v));
    set_sc(PS_DR0 + 4 * j + 2 + h, hi_d(v));
  }
  H9K_HD float root(int i) const { return lay(PF_ROOTR, i); }
  H9K_HD void set_root(int i, float v) const { set_lay(PF_ROOTR, i, v); }
  H9K_HD float sv_lay(int q, int i) const { return lay(PF_SVH2O + q, i); }
  H9K_HD void sv_set_lay(int q, int i, float v) const { set_lay(PF_SVH2O + q, i, v); }
  H9K_HD float sv_sc(int k) const { return sc(PS_SVZWT + k); }
  H9K_HD void sv_set_sc(int k, float v) const { set_sc(PS_SVZWT + k, v); }
  H9K_HD void sv_sync() const {}
  H9K_HD void day_start(int) const {}
};

// Device: [row][S] LDS block per wave, S = lanes per wave.  Layer i of a
// per-layer field sits in row p*L/2 + (i-1)/2 of the pair's column
// (i-1)&1, so a lane's own layers are its own column's rows and any layer
// is a static offset from the pair's even column.  Per-cell fields are
// spread the same way over the two columns.  Both lanes of a pair store
// identical values to the same address where they both write.
//
// The day snapshot lives in global memory (L2-resident: 80 B per
// cell), in a per-workgroup block shaped like the LDS block: the byte
// offset of a value is its LDS address, so every snapshot store is
// `global_store v_lds_address, s_block + imm` with no address arithmetic.
// That leaves LDS room, within 3 workgroups per CU (75 rows per wave), for
// the reciprocal fields: 1/(-psi) at any L, 1/theta_s and the day
// reciprocals at L = 8 (75 rows; L = 10: 72 rows; the 2-wave build: all of
// them at L = 10 too, 89 rows).
// Issue priority of the waves sharing a SIMD (one from each of the CU's
// resident workgroups).  The SIMD arbitrates VALU issue by priority, then by
// wave age, so with equal priorities the oldest wave runs at its lone-wave
// rate, the youngest is starved, and the kernel ends on the youngest waves
// running alone (measured: the first-dispatched third of the waves took
// 0.82x the mean time, the last third 1.21x).
//   mode 1 (rotate): the top priority rotates over the resident rounds every
//     day, so the waves get equal issue shares (config 2: 283 -> 251 ms;
//     slowest wave 1.25 -> 1.09x the mean).  Rotating every 1, 4 or 16
//     substeps instead measured the same.
//   mode 2 (pace): each wave posts its day to a per-SIMD row in global memory
//     (keyed by the hardware XCC/SE/SH/CU/SIMD ids, tagged with the launch
//     epoch) and takes a priority equal to the number of waves on its SIMD
//     that are ahead of it, so the waves of a SIMD keep the same day and
//     finish together instead of one heavy wave finishing alone.
struct Pacer {
  unsigned *row;      // mode 2: this SIMD's 16 progress words
  unsigned epoch;     // mode 2: launch tag (20 bits)
  int me;             // mode 2: hardware wave slot (0..15)
  int mode;
  int round;          // mode 1: 0..resident-1, which of the CU's resident workgroups
  __device__ __forceinline__ static void set_prio(int p) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (p <= 0)
      __builtin_amdgcn_s_setprio(0);
    else if (p == 1)
      __builtin_amdgcn_s_setprio(1);
    else if (p == 2)
      __builtin_amdgcn_s_setprio(2);
    else
      __builtin_amdgcn_s_setprio(3);
#endif
  }
  __device__ __forceinline__ void day_start(int day, int resident) const {
#if defined(__HIP_DEVICE_COMPILE__)
    if (mode == 1) {
      set_prio((round + day) % resident);
    } else if (mode == 2) {
      const unsigned mine = (epoch << 12) | (unsigned)(day + 1);
      __hip_atomic_store(row + me, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int k = (int)(__lane_id() & 15);
      const unsigned v = __hip_atomic_load(row + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool ahead = k != me && (v >> 12) == (epoch & 0xfffffu) && (v & 0xfffu) > (unsigned)(day + 1);
      const uint64_t m = __builtin_amdgcn_ballot_w64(ahead);
      const unsigned slots = (unsigned)(m | (m >> 16) | (m >> 32) | (m >> 48)) & 0xffffu;
      set_prio(__builtin_popcount(slots));
    }
#endif
  }
};
// Key of the SIMD this wave runs on and its slot there (HW_REG_HW_ID:
// wave 3:0, simd 5:4, cu 11:8, sh 12, se 15:13; HW_REG_XCC_ID 3:0).
#define H9G_PACE_ROWS 16384
__device__ __forceinline__ void pace_key(int &row, int &slot) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);
  const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u;
  slot = (int)(hw & 15u);
  row = (int)(((((xcc * 8u + ((hw >> 13) & 7u)) * 2u + ((hw >> 12) & 1u)) * 16u + ((hw >> 8) & 15u)) * 4u) +
              ((hw >> 4) & 3u));
#else
  row = slot = 0;
#endif
}

// The L = 10 pair kernel runs 3 waves per SIMD like L = 8: without the
// per-layer double reciprocal of theta_s and the day constants' its LDS block
// fits three workgroups per CU (72 rows, 51.4 KB), and 168 VGPRs (config 5:
// 632 -> 535 ms per year against 2 waves/SIMD with every reciprocal,
// DESIGN.md §6).
template <int L>
constexpr int pair_resident() { return 3; }   // waves per SIMD (h9g.hip pair_waves)

// R = waves per SIMD the kernel is built for (its workgroups per CU): 3 (the
// default, 168 VGPRs, <= 53 KB LDS per workgroup) or 2 (round 4, L = 10:
// 256 VGPRs and 80 KB, so no spills and every reciprocal field; h9g.hip
// h9g_pair2_kernel).
// F = 1: the one-column kernel's two-wave shape (front_year_pair); its block
// ends with the hand-over rows HO_*.  F = 2: that shape with the water-table
// chain on the second wave (H9G_P1_SIDE), the rows HS_* after them.
template <int L, int S, int R = pair_resident<L>(), int F = 0>
struct PairStore {
  static constexpr int NT = L / 2;
  static constexpr bool kFront = F != 0;
  static constexpr bool kSide = F == 2;         // ... whose second wave takes the water-table chain too
  static_assert(!kFront || S == 2, "the front wave serves a one-column wave");
  // LDS fields by layer count (3 workgroups per CU: at most 75 rows).  L = 8:
  // every reciprocal (75 rows).  L = 10 (5 rows per per-layer field): 1/(-psi)
  // (~15 divisions per substep) instead of the day constants' reciprocals (~5;
  // round 3: 533.6 -> 530.3 ms for config 5), no 1/theta_s (72 rows).  At
  // R = 2 every reciprocal fits at L = 10 too (89 rows).
  // (S = 22, the 11-column wave of h9g_pair11_kernel, leaves the LDS room for
  // every reciprocal at L = 10 and 3 workgroups per CU too: 89 rows, 31.3 KB)
  static constexpr bool kRecip = true, kRts = L <= 8 || R <= 2 || S <= 22, kDayRecip = L <= 8 || R <= 2 || S <= 22;
  // s_node of the conductivity phase from the stored 1/theta_s too (round 3:
  // no longer spills in the call-free kernel)
  static constexpr bool kRtsHK = kRts;
  static constexpr int NPF = kRecip ? (kRts ? PF_SVH2O : PF_RTS0) : PF_RPSI0;   // per-layer fields in LDS
  static constexpr int NPS = kDayRecip ? PS_SVZWT : PS_DR0; // per-cell fields in LDS
  // (a one-column wave, S = 2, keeps the substep's starting theta(1..L) in
  // NT more rows, float TH0 + i - 1 of the block, for its task lanes:
  // hydrology_pair)
  static constexpr int TH0 = (NPF * NT + (NPS + 1) / 2) * S;
  // Hand-over words of the two-wave shape, floats of the block after theta:
  // main -> front (written before barrier 1): smp(1..L), h2osoi_liq(1), zwt, go
  // (0: evaluate this substep's front, else leave); front -> main (written
  // before barrier 2): the FrontRes fields.  tests/test_pair1_front_map.py
  // restates the map.
  enum : int {
    HO_SMP = TH0 + L, HO_H2O1 = HO_SMP + L, HO_ZWT, HO_GO, HO_PAD,
    HO_SURF, HO_TRAN, HO_EVG, HO_INFL, HO_END
  };
  static_assert((HO_END - TH0 - L) % 2 == 0, "whole rows");
  // The water-table chain's words (F = 2), after the front's: main -> second
  // wave, wa written before barrier 1 and the rest before barrier 2 (the two
  // single powers of round A, smp and zq of layer max(jwt, 1)); second wave ->
  // main, written before barrier 3: zwt, wa, rsub_top, the final jwt, the
  // exact-re-run flag, the STOP code and its value, and the layer and amount of
  // up to two additions to h2osoi_liq (layer 0: none).
  // tests/test_pair1_side_map.py restates the map.
  enum : int {
    HS_WA = HO_END, HS_P0, HS_PY, HS_RSMP, HS_RZQ, HS_PAD0,
    HS_ZWT, HS_WAO, HS_RSUB, HS_JWT, HS_FLAG, HS_CODE, HS_ERRV, HS_I0, HS_R0, HS_I1, HS_R1, HS_PAD1, HS_END
  };
  static_assert((HS_END - HO_END) % 2 == 0, "whole rows");
  static constexpr int ROWS =
      NPF * NT + (NPS + 1) / 2 + (S == 2 ? NT : 0) + (kFront ? ((kSide ? HS_END : HO_END) - HO_SMP) / 2 : 0);
  static constexpr int GBLOCK = 65536;                      // bytes per workgroup (>= any LDS address)
  lds_float *self, *even;
  const lds_float *zt;                 // zi(0..L+1), then zi(0..L+1)/1000 (per block)
  float *svw;                          // this workgroup's day-snapshot block (global)
  static constexpr int RESIDENT = R;                        // workgroups per CU = waves per SIMD
  Pacer pace;
  lds_float *wb;                       // the wave's block (column 0): spare lanes' stolen slots
  static constexpr int LANES = S;
  // helper lanes in the per-layer phases (hydrology_pair): not in the 3-wave
  // L = 10 build of 22-column waves, whose registers they push further into
  // scratch
  static constexpr bool kSpare = !(L >= 10 && R >= 3 && S >= 44);
  // the interface fluxes split over the pair (H9G_FLUX_SPLIT); not in the
  // one-column waves, whose round C has a lane per interface
  static constexpr bool kFluxSplit = S > 2;
  __device__ __forceinline__ void day_start(int day) const { pace.day_start(day, RESIDENT); }
  __device__ __forceinline__ float zi(int i) const { return zt[i]; }
  __device__ __forceinline__ float zim(int i) const { return zt[L + 2 + i]; }
  __device__ __forceinline__ double rdz_t(int i) const {
    return join_d(zt[2 * (L + 2) + 2 * i], zt[2 * (L + 2) + 2 * i + 1]);
  }
  __device__ __forceinline__ float lay(int p, int i) const {
    return even[(p * NT + ((i - 1) >> 1)) * S + ((i - 1) & 1)];
  }
  __device__ __forceinline__ void set_lay(int p, int i, float v) const {
    even[(p * NT + ((i - 1) >> 1)) * S + ((i - 1) & 1)] = v;
  }
  __device__ __forceinline__ float sc(int k) const { return even[(NPF * NT + (k >> 1)) * S + (k & 1)]; }
  __device__ __forceinline__ void set_sc(int k, float v) const {
    even[(NPF * NT + (k >> 1)) * S + (k & 1)] = v;
  }
  __device__ __forceinline__ float slot(int p, int t) const { return self[(p * NT + t) * S]; }
  __device__ __forceinline__ void set_slot(int p, int t, float v) const { self[(p * NT + t) * S] = v; }
  __device__ __forceinline__ void launder() {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(self), "+v"(even), "+v"(zt)::"memory");
#endif
  }
  // hand-over word k (HO_*), and the barrier of the column's two waves: what
  // either wave stored to the block before it is read by the other after it
  __device__ __forceinline__ float ho(int k) const { return wb[k]; }
  __device__ __forceinline__ void set_ho(int k, float v) const { wb[k] = v; }
  __device__ __forceinline__ void wg_sync() const {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
  }
  __device__ __forceinline__ float day(int f) const { return sc(PS_DAY + f); }
  __device__ __forceinline__ void set_day(int f, float v) const { set_sc(PS_DAY + f, v); }
  __device__ __forceinline__ double day_r(int k) const {
    return join_d(sc(PS_DRS + 2 * k), sc(PS_DRS + 2 * k + 1));
  }
  __device__ __forceinline__ void set_day_r(int k, double v) const {
    set_sc(PS_DRS + 2 * k, lo_d(v));
    set_sc(PS_DRS + 2 * k + 1, hi_d(v));
  }
  __device__ __forceinline__ double day_rp(int j, int h) const {
    return join_d(sc(PS_DR0 + 4 * j + h), sc(PS_DR0 + 4 * j + 2 + h));
  }
  __device__ __forceinline__ void set_day_rp(int j, int h, double v) const {
    set_sc(PS_DR0 + 4 * j + h, lo_d(v));
    set_sc(PS_DR0 + 4 * j + 2 + h, hi_d(v));
  }
  // per-cell field k (even) + this lane's parity: the lane's own column of
  // the row holding fields k, k+1
  __device__ __forceinline__ float sc_own(int k) const { return self[(NPF * NT + (k >> 1)) * S]; }
  __device__ __forceinline__ double day_rp_own(int j) const {
    return join_d(sc_own(PS_DR0 + 4 * j), sc_own(PS_DR0 + 4 * j + 2));
  }
  __device__ __forceinline__ float root(int i) const { return lay(PF_ROOTR, i); }
  __device__ __forceinline__ void set_root(int i, float v) const { set_lay(PF_ROOTR, i, v); }
  // snapshot: rows q*NT + t (layers), 2*NT + k/2 (scalars) of the global block
  __device__ __forceinline__ float *gl(const lds_float *p, int off) const {
    return (float *)((char *)svw + (uint32_t)(size_t)p) + off;
  }
  __device__ __forceinline__ void sv_set_slot(int q, int t, float v) const { *gl(self, (q * NT + t) * S) = v; }
  __device__ __forceinline__ float sv_lay(int q, int i) const {
    return *gl(even, (q * NT + ((i - 1) >> 1)) * S + ((i - 1) & 1));
  }
  __device__ __forceinline__ void sv_set_lay(int q, int i, float v) const {
    *gl(even, (q * NT + ((i - 1) >> 1)) * S + ((i - 1) & 1)) = v;
  }
  __device__ __forceinline__ float sv_sc(int k) const { return *gl(even, (2 * NT + (k >> 1)) * S + (k & 1)); }
  __device__ __forceinline__ void sv_set_sc(int k, float v) const {
    *gl(even, (2 * NT + (k >> 1)) * S + (k & 1)) = v;
  }
  // before reading back what the wave stored (the exact re-run)
  __device__ __forceinline__ void sv_sync() const {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
#endif
  }
};

// Device, one lane per column ("solo"): column `lane` of a [row][64] block,
// every field in the lane's own column; no reciprocal fields, no parking
// (1054 waves = 5 blocks/CU), day snapshot in LDS.  EV: one more snapshot
// field, SV_EVAP (the ET kernels).
template <int L, bool EV = false>
struct SoloStore {
  static constexpr bool kRecip = false, kRts = false, kDayRecip = false, kRtsHK = false, kSpare = false, kFront = false;
  static constexpr bool kFluxSplit = false;          // one lane per column: nothing to split
  static constexpr int NPF = PF_RPSI0 + 2;           // TS..ROOTR, SVH2O, SVSMP
  static constexpr int NPS = PS_LAI + 5 + (EV ? 1 : 0);   // FMAX..DAY, SV*
  static constexpr int ROWS = NPF * L + NPS;
  lds_float *b;
  const lds_float *zt;
  H9K_HD static constexpr int pr(int p) { return p < PF_RPSI0 ? p : p - (PF_SVH2O - PF_RPSI0); }
  H9K_HD static constexpr int kr(int k) { return k < PS_LAI ? k : k - (PS_SVZWT - PS_LAI); }
  __device__ __forceinline__ float zi(int i) const { return zt[i]; }
  __device__ __forceinline__ float zim(int i) const { return zt[L + 2 + i]; }
  __device__ __forceinline__ double rdz_t(int i) const {
    return join_d(zt[2 * (L + 2) + 2 * i], zt[2 * (L + 2) + 2 * i + 1]);
  }
  __device__ __forceinline__ float lay(int p, int i) const { return b[(pr(p) * L + i - 1) * 64]; }
  __device__ __forceinline__ void set_lay(int p, int i, float v) const { b[(pr(p) * L + i - 1) * 64] = v; }
  __device__ __forceinline__ float sc(int k) const { return b[(NPF * L + kr(k)) * 64]; }
  __device__ __forceinline__ void set_sc(int k, float v) const { b[(NPF * L + kr(k)) * 64] = v; }
  __device__ __forceinline__ float slot(int p, int t) const { return b[(pr(p) * L + 2 * t) * 64]; }
  __device__ __forceinline__ void set_slot(int p, int t, float v) const { b[(pr(p) * L + 2 * t) * 64] = v; }
  __device__ __forceinline__ void launder() {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(b), "+v"(zt)::"memory");
#endif
  }
  __device__ __forceinline__ float day(int f) const { return sc(PS_DAY + f); }
  __device__ __forceinline__ void set_day(int f, float v) const { set_sc(PS_DAY + f, v); }
  __device__ __forceinline__ double day_r(int) const { return 0.0; }
  __device__ __forceinline__ void set_day_r(int, double) const {}
  __device__ __forceinline__ double day_rp(int, int) const { return 0.0; }
  __device__ __forceinline__ void set_day_rp(int, int, double) const {}
  __device__ __forceinline__ float root(int i) const { return lay(PF_ROOTR, i); }
  __device__ __forceinline__ void set_root(int i, float v) const { set_lay(PF_ROOTR, i, v); }
  __device__ __forceinline__ float sv_lay(int q, int i) const { return lay(PF_SVH2O + q, i); }
  __device__ __forceinline__ void sv_set_lay(int q, int i, float v) const { set_lay(PF_SVH2O + q, i, v); }
  __device__ __forceinline__ float sv_sc(int k) const { return sc(PS_SVZWT + k); }
  __device__ __forceinline__ void sv_set_sc(int k, float v) const { set_sc(PS_SVZWT + k, v); }
  __device__ __forceinline__ void sv_sync() const {}
  __device__ __forceinline__ void day_start(int) const {}
};

// Phase profiler (tools: H9G_STAMPS build only).  NoProf compiles away.
// flux(evg, tran) receives the substep's qflx_evap_grnd and
// qflx_tran_veg_col (HYDROLOGY.f90:388-400); only the site path keeps them.
struct NoProf {
#if defined(H9G_ISA_PHASES) && defined(__HIP_DEVICE_COMPILE__)
  template <int K>
  __device__ __forceinline__ void markk() { asm volatile("; h9g-phase %0" ::"i"(K)); }   // tools/isa_mix.py --phases
  H9K_HD void mark(int k) {
    switch (k) {
      case 0: markk<0>(); break;
      case 1: markk<1>(); break;
      case 2: markk<2>(); break;
      case 3: markk<3>(); break;
      case 4: markk<4>(); break;
      case 5: markk<5>(); break;
      case 6: markk<6>(); break;
      default: markk<7>(); break;
    }
  }
#else
  H9K_HD void mark(int) {}
#endif
  H9K_HD void flux(float, float) {}
};
struct FluxProf {
  float evg, tran;
  H9K_HD void mark(int) {}
  H9K_HD void flux(float e, float t) { evg = e; tran = t; }
};
// The ET kernels' policy (h9g_set_evap): the year's evaporation
// sum, evap_sum = evap_sum + (qflx_evap_grnd + qflx_tran_veg_col) * dt once a
// substep (HYBRID9.f90:207-208's expression, in the form of rnf_sum's
// HYDROLOGY.f90:1282-1283), added where the substep hands the two fluxes over.
// A substep that ends in a STOP leaves the cell's rows NaN, and one that is
// re-run exactly takes the sum back from the day snapshot (SV_EVAP), so adding
// here or after the substep is the same sum.  dt: g.dt().
struct EvapProf {
  float sum, dt;
  H9K_HD void mark(int) {}
  H9K_HD void flux(float e, float t) { sum = sum + (e + t) * dt; }
};
template <class PR>
constexpr bool kEvap = std::is_same<typename std::remove_reference<PR>::type, EvapProf>::value;
#if defined(H9G_STAMPS)
H9K_HD uint64_t stamp_clock() {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_s_memtime();
#else
  return 0;
#endif
}
struct StampProf {                     // wave-uniform shader-clock deltas per phase
  uint64_t last;
  uint32_t acc[8];
  H9K_HD void mark(int k) {
    const uint64_t t = stamp_clock();
    acc[k] += (uint32_t)(t - last);
    last = t;
  }
  H9K_HD void flux(float, float) {}
};
#endif

// ---------------------------------------------------------------- policies
// One lane computes every layer.
struct SplitAll {
  static constexpr bool kSpare = false;
  H9K_HD constexpr bool act() const { return true; }
  H9K_HD SplitAll fresh() const { return *this; }
  template <class CS>
  H9K_HD float own(const CS &cs, int p, int t, int h) const { return cs.lay(p, 2 * t + 1 + h); }
  // out[2t+1+h] = fast(t, h, bad) for every layer, K outputs per layer:
  // fast is branch-free and sets bad when any of its results needs
  // glibc's/IEEE's other path; exact(t, h) (the body with in-place redos)
  // then recomputes the layer.
  template <int NT, int K, int FE = 1, class FF, class FX>
  H9K_HD void par_d(FF fast, FX exact, float *const (&out)[K]) const {
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
      for (int h = 0; h < 2; h++) {
        bool bad = false;
        FV<K> r = fast(t, h, bad);
        if (bad) r = exact(t, h);
#pragma unroll
        for (int k = 0; k < K; k++) out[k][2 * t + 1 + h] = r.v[k];
      }
      sched_fence();
    }
  }
  // r0 = f(0), r1 = f(1)
  template <int K, class F>
  H9K_HD void pick(F f, FV<K> &r0, FV<K> &r1) const {
    r0 = f(0);
    r1 = f(1);
  }
  H9K_HD bool pair_any(bool p) const { return p; }
  // per-cell field k + h of a canopy/soil pair (k even), the pair's day reciprocal
  template <class CS>
  H9K_HD float own_sc(const CS &cs, int k, int h) const { return cs.sc(k + h); }
  template <class CS>
  H9K_HD double own_day_rp(const CS &cs, int j, int h) const { return cs.day_rp(j, h); }
};

// Two lanes per column (device fast path); h = lane & 1.  The wave's lanes
// past the pairs (spare lanes, ln >= PairStore::LANES) take part only in the
// per-layer phases, where they evaluate the pairs' last slot (hydrology_pair)
// and are masked off everywhere else (act()).
struct Split2 {
  int h;
  int ln;                         // lane in the wave
  bool spare;
  static constexpr bool kSpare = true;
  H9K_HD bool act() const { return !spare; }
  H9K_HD Split2 fresh() const {   // h, opaque to the optimiser (hydrology_pair)
    Split2 r{h, ln, spare};
    opaque(r.h);
    return r;
  }
  // v of the even lane -> e, of the odd lane -> o, in both lanes: two DPP
  // broadcasts (round 3; round 2 swapped and selected per lane: one DPP
  // move and two selects, 214.5 -> 213.9 ms)
  H9K_HD void xchg(float v, float &e, float &o) const {
    e = pair_bcast<0>(v);
    o = pair_bcast<1>(v);
  }
  template <class CS>
  H9K_HD float own(const CS &cs, int p, int t, int) const { return cs.slot(p, t); }
  // The special-case checks of all NT slots deferred to one rarely-taken
  // branch after them (SplitAll::par_d).  A lane with any flag recomputes its
  // slots exactly.  A scheduling fence follows every FE slots: one slot per
  // region for the powers (wider regions spill); FE = NT for
  // slots without powers (beta), which the scheduler may interleave.
  template <int NT, int K, int FE = 1, class FF, class FX>
  H9K_HD void par_d(FF fast, FX exact, float *const (&out)[K]) const {
    FV<K> r[NT];
    bool bad = false;
#pragma unroll
    for (int t = 0; t < NT; t++) {
      r[t] = fast(t, h, bad);
      if ((t + 1) % FE == 0 || t == NT - 1) sched_fence();
    }
    if (__builtin_expect(bad, 0)) {
#pragma unroll
      for (int t = 0; t < NT; t++) r[t] = exact(t, h);
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
      for (int k = 0; k < K; k++) xchg(r[t].v[k], out[k][2 * t + 1], out[k][2 * t + 2]);
    }
  }
  // par_d that also leaves the lane's own results in r, and exchanges only the
  // outputs k with bit k of XM set (the flux phase reads the others from the
  // lane that holds them: hydrology_pair)
  template <int NT, int K, unsigned XM, int FE = 1, class FF, class FX>
  H9K_HD void par_k(FF fast, FX exact, float *const (&out)[K], FV<K> (&r)[NT]) const {
    bool bad = false;
#pragma unroll
    for (int t = 0; t < NT; t++) {
      r[t] = fast(t, h, bad);
      if ((t + 1) % FE == 0 || t == NT - 1) sched_fence();
    }
    if (__builtin_expect(bad, 0)) {
#pragma unroll
      for (int t = 0; t < NT; t++) r[t] = exact(t, h);
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
      for (int k = 0; k < K; k++)
        if ((XM >> k) & 1) xchg(r[t].v[k], out[k][2 * t + 1], out[k][2 * t + 2]);
    }
  }
  template <int K, class F>
  H9K_HD void pick(F f, FV<K> &r0, FV<K> &r1) const {
    const FV<K> r = f(h);
#pragma unroll
    for (int k = 0; k < K; k++) xchg(r.v[k], r0.v[k], r1.v[k]);
  }
  H9K_HD bool pair_any(bool p) const {
    const float f = p ? 1.0f : 0.0f;
    return (f + pair_swap(f)) != 0.0f;
  }
  template <class CS>
  H9K_HD float own_sc(const CS &cs, int k, int) const { return cs.sc_own(k); }
  template <class CS>
  H9K_HD double own_day_rp(const CS &cs, int j, int) const { return cs.day_rp_own(j); }
};

// Rollback copy of a per-layer state array (1-based v[1..L]).
template <int L, class CS>
H9K_HD void save_layers(const SplitAll &, const CS &cs, int q, const float *v) {
#pragma unroll
  for (int i = 1; i <= L; i++) cs.sv_set_lay(q, i, v[i]);
}
template <int L, class CS>
H9K_HD void save_layers(const Split2 &sp, const CS &cs, int q, const float *v) {
#pragma unroll
  for (int t = 0; t < L / 2; t++) cs.sv_set_slot(q, t, sel(sp.h, v[2 * t + 1], v[2 * t + 2]));
}

template <class CS>
H9K_HD void set_lay_d(const CS &cs, int p, int i, double v) {
  cs.set_lay(p, i, lo_d(v));
  cs.set_lay(p + 1, i, hi_d(v));
}
template <class CS>
H9K_HD double lay_d(const CS &cs, int p, int i) { return join_d(cs.lay(p, i), cs.lay(p + 1, i)); }

// x / d, from a stored double reciprocal of d when Use (MathFast::div,
// exact for normal quotients; MathExact divides), else divided.
template <bool Use, class M, class R>
H9K_HD float divr(M &m, float x, float d, R rget) {
  if constexpr (Use)
    return m.div(x, d, rget());
  else
    return x / d;
}

// divr with the check deferred (MathFast::div_d): bad |= the quotient
// needs the IEEE redo, done by divr_fix after the group.
template <bool Use, class M, class R>
H9K_HD float divr_d(M &m, float x, float d, R rget, bool &bad) {
  if constexpr (Use) {
    const float q = m.div_d(x, d, rget());
    bad |= m.div_bad(q);
    return q;
  } else {
    return x / d;
  }
}
template <bool Use, class M>
H9K_HD void divr_fix(M &m, float &q, float x, float d) {
  if constexpr (Use) m.div_fix(q, x, d);
}

// expf on glibc's main path, flagged (sp) when glibc takes another path
// (then M::expf recomputes); MathExact computes it exactly, never flagged.
template <class M>
H9K_HD float expf_fast(M &m, float x, bool &sp) {
  if constexpr (M::kExact)
    return m.expf(x);
  else
    return h9m::expf_nx(x, m.T, sp);
}

// Runs visit(k) for k = 0, 1, ... while it returns true (the reference's
// layer loops with EXIT).  The fast path (MathFast) unrolls two visits --
// the second only if some lane needs it -- and hands a third to the exact
// re-run; loops visit one layer 99.5% of the time and never three in the
// synthetic runs.  MathExact loops.
template <class M, class F>
H9K_HD void visit_layers(M &m, F visit) {
  if constexpr (M::kExact) {
    for (int k = 0;; k++)
      if (!visit(k)) break;
  } else {
    bool more = visit(0);
    if (any_lane(more)) {
      H9G_BR(BR_VISIT2);
      if (more) more = visit(1);
      m.special |= more;
    }
  }
}

// Runtime-indexable geometry table (zt_size(L) floats): zi(0..L+1), then
// zi(0..L+1)/1000 (the reference's zi(I)/1000.0, e.g. HYDROLOGY.f90:
// 499-508,998), then RN64(1/dz(I)) for I = 0..L+1 as (low, high) words
// (I = 0 unused).  A lane reads its own layers' values at a runtime index
// instead of keeping compile-time selects live in registers.
template <int L>
constexpr int zt_size() { return 4 * (L + 2); }
template <int L, class G, class T>
H9K_HD void fill_zt(const G &g, T *zt) {
#pragma unroll
  for (int i = 0; i <= L + 1; i++) {
    zt[i] = g.zi(i);
    zt[L + 2 + i] = g.zi(i) / 1000.0f;
    const double r = (i > 0 && i <= L) ? g.rdz(i) : 0.0;
    zt[2 * (L + 2) + 2 * i] = lo_d(r);
    zt[2 * (L + 2) + 2 * i + 1] = hi_d(r);
  }
}

// Parameter-only invariants (as cell_inv), into a pair/flat store.
template <int L, class G, class CS>
H9K_HD void cell_inv_pair(const G &g, const CS &cs) {
#pragma unroll
  for (int i = 1; i <= L; i++) {
    const int ip = (L < i + 1) ? L : i + 1;
    const float ts = cs.lay(PF_TS, i), tsp = cs.lay(PF_TS, ip);
    const float bsw = cs.lay(PF_BSW, i), psi = cs.lay(PF_PSI, i);
    const float e = one - one / bsw;
    cs.set_lay(PF_NINVB, i, -one / bsw);
    cs.set_lay(PF_ITS, i, one / (ts + tsp));
    const float pte = psi * ts / e;
    cs.set_lay(PF_PTE, i, pte);
    cs.set_lay(PF_C3, i, pte / (g.zi(i) - g.zi(i - 1)));
    if constexpr (CS::kRecip) set_lay_d(cs, PF_RPSI0, i, recip64(-psi));
    if constexpr (CS::kRts) set_lay_d(cs, PF_RTS0, i, recip64(ts));
  }
  float mh = cs.lay(PF_HKS, 1);
  if (cs.lay(PF_HKS, 2) < mh) mh = cs.lay(PF_HKS, 2);
  if (cs.lay(PF_HKS, 3) < mh) mh = cs.lay(PF_HKS, 3);
  cs.set_sc(PS_MH3, mh);
  cs.set_sc(PS_TSDZ1, MAXF(zero, (cs.lay(PF_TS, 1) * g.dz(1))));
}

// The task rounds of hydrology_pair: a wave that holds one column (the store's
// LANES == 2, Split2 with helper lanes), on the fast path only.
template <class M, class SP, class CS>
constexpr bool pair1_tasks() {
  if constexpr (H9G_P1_TASKS && SP::kSpare && CS::kSpare && !M::kExact)
    return CS::LANES == 2;
  else
    return false;
}

// One HYDROLOGY call (/root/reference/SOURCE/HYDROLOGY.f90:141-1283) for
// one cell; every block cites the reference lines it restates.  Returns 0
// or an H9G_ERR_* code (the reference's STOP sites) with errval set;
// Under
// Split2 the per-layer phases are split over the pair (file comment).
// The end-of-step theta(1..L) of :1233 is left to the caller (end_theta).
// ROLE (ROLE_*): the one-column kernel's two waves per column evaluate the
// front (ROLE_FRONT, results into *fr) and the rest (ROLE_MAIN) of a substep
// side by side; every other caller runs all of it.  With the chain on the
// second wave (H9G_P1_SIDE) the main wave is ROLE_MAINS: in a substep that
// starts with the water table in the column it leaves the water-table chain
// (pr.mark(4) to pr.mark(6)) to the second wave's ROLE_CHAIN call, which runs
// that text alone on the handed-over operands, posts its results in place of
// the h2osoi_liq additions and returns at pr.mark(6) (or with STOP 3); the
// main wave takes them behind barrier 3 (front_year_pair has the protocol).
template <class CS>
constexpr int main_role() {
  if constexpr (CS::kFront)
    return CS::kSide ? ROLE_MAINS : ROLE_MAIN;
  else
    return ROLE_ALL;
}
template <int L, class G, class M, class SP, class CS, class PR = NoProf, int ROLE = ROLE_ALL>
H9K_HD int hydrology_pair(const G &g, CS cs, const SP &sp0, St<L> &s, float &rnf_sum, float &errval,
                          M &m, PR &pr, FrontRes *fr = nullptr) {
  constexpr int NT = L / 2;
  constexpr bool kMain = ROLE == ROLE_MAIN || ROLE == ROLE_MAINS;   // without the front
  constexpr bool kChain = ROLE == ROLE_CHAIN;                       // the water-table chain alone
  // A STOP of the main wave between barriers 2 and 3: the wave passes barrier 3
  // on its way out, so its partner, which waits there in every substep, is
  // released and both go on to the barrier 1 that ends the year (front_done).
  // Premise: lanes 0 and 1 of the main wave take a STOP's branch together.
  // They do, because both hold the whole column and evaluate the sweep, the
  // pivots and bm(1) from the same exchanged operands (as every STOP of the
  // two-barrier shape already assumed: cell_year_pair takes lane 0's code for
  // the wave).  Lanes that parted here would pass one barrier more than the
  // partner wave, which must not happen; a change that lets the two lanes'
  // sweeps differ has to carry the code to the one barrier 3 below instead.
#define STOP_RET(c)                                  \
  {                                                  \
    if constexpr (ROLE == ROLE_MAINS) cs.wg_sync();  \
    return c;                                        \
  }
  // At L = 10 the lane parity is made opaque here, so that values that
  // depend only on it -- a lane's geometry-table offsets of its own layers,
  // one per slot -- are recomputed inside the substep (an add each) instead
  // of hoisted out of the year loop, spilled to scratch and reloaded behind
  // a vmcnt(0) in every slot (round 4: scratch ops in the L = 10 substep
  // loop 11.2 -> 6.7 per wave-substep, tools/isa_mix.py; at L = 8 nothing
  // is hoisted that way and the change would only add VALU).
  const SP sp = L >= 10 ? sp0.fresh() : sp0;
  const float dt = g.dt();
  constexpr double r1000 = 1.0 / 1000.0;
  float zim[L + 1];
#pragma unroll
  for (int i = 1; i <= L; i++) zim[i] = g.zim(i);
  float *h2o = s.h2o, *smp = s.smp;
  float theta[L + 1];
  cs.launder();
#define TS(i) cs.lay(PF_TS, i)
#define HKS(i) cs.lay(PF_HKS, i)
#define BSW(i) cs.lay(PF_BSW, i)
#define PSI(i) cs.lay(PF_PSI, i)
#define LAYF(F, i) cs.lay(F, i)
#define ROOT(i) cs.lay(PF_ROOTR, i)
#define DC(F) cs.sc(PS_DAY + F)
#define OWN(p) sp.own(cs, p, t, h)

  // :141-151
  float w0 = zero;
  if constexpr (ROLE == ROLE_FRONT) {
    // the front reads theta(1) alone: the same quotient with the same redo
    theta[1] = m.div_d(h2o[1], g.thk(1), g.rthk(1));
    m.div_fix(theta[1], h2o[1], g.thk(1));
  } else if constexpr (!kChain) {
  w0 = DC(D_FORC) * dt + s.wa;
  bool bad = false;                      // deferred checks (MathFast::div_d)
#pragma unroll
  for (int i = 1; i <= L; i++) {
    w0 = w0 + h2o[i];
    theta[i] = m.div_d(h2o[i], g.thk(i), g.rthk(i));
    bad |= m.div_bad(theta[i]);
  }
  if (__builtin_expect(bad, 0)) {
    H9G_BR(BR_THETA);
#pragma unroll
    for (int i = 1; i <= L; i++) m.div_fix(theta[i], h2o[i], g.thk(i));
  }
  }
  // :161-212
  const float hkdepth = one / 2.5f;
  const float fff = 1.0f / hkdepth;
  const float frac_h2osfc = zero;
  float qflx_surf = zero, tran = zero, evg = zero, qflx_infl = zero;
  if constexpr (!kMain && !kChain) {       // the front (the main wave: from the front wave, below)
  const float qflx_top_soil = DC(D_FORC);
  const float fsat = cs.sc(PS_FMAX) * m.expf(-0.5f * fff * s.zwt);
  qflx_surf = fsat * qflx_top_soil;
  // :269-276 (previous-step smp)
  float beta = zero;
  {
    // the terms rootr(i) * beta_i of the lane's own layers (the pair split:
    // round 3, 199.3 -> 197.3 ms), then the reference's sum over the layers
    // in order
    float rb[L + 1];
    float *const out[1] = {rb};
    auto qb_x = [&](int t, int h) __attribute__((always_inline)) {
      return sel(h, smp[2 * t + 1] - g.zc(2 * t + 1), smp[2 * t + 2] - g.zc(2 * t + 2));
    };
    auto term = [&](int t, int h, float q) __attribute__((always_inline)) {
      float b = one - q;
      b = MINC(one, b);
      b = MAXF(zero, b);
      return FV<1>{{sp.own(cs, PF_ROOTR, t, h) * b}};
    };
    sp.template par_d<NT, 1, NT>(
        [&](int t, int h, bool &bad) __attribute__((always_inline)) -> FV<1> {
          const float q = m.div_d(qb_x(t, h), -150000.0f, 1.0 / -150000.0);
          bad |= m.div_bad(q);
          return term(t, h, q);
        },
        [&](int t, int h) __attribute__((always_inline)) -> FV<1> {
          H9G_BR(BR_QB);
          return term(t, h, m.div(qb_x(t, h), -150000.0f, 1.0 / -150000.0));
        },
        out);
#pragma unroll
    for (int i = 1; i <= L; i++) beta = beta + rb[i];
  }
  // :325-331
  float rss;
  if (theta[1] <= 0.15f)
    rss = (10.0f + DC(D_LIT1000)) * m.expf(0.3563f * 100.0f * (0.15f - theta[1]));
  else
    rss = (10.0f + DC(D_LIT1000) * (1.0f - divr<CS::kRts>(m, theta[1], TS(1), [&]() { return lay_d(cs, PF_RTS0, 1); })));
  const float desatdT = DC(D_DESAT), gamma = DC(D_GAMMA);
  const float Ra = DC(D_DG) * DC(D_RAA);
  float rsc;
  bool eb_fast = false;
  if constexpr (H9G_EB_FAST && !M::kExact && CS::kDayRecip) {
    // The energy balance's chain of quotients (:283-389) branch-free: the
    // day constants' by their stored double reciprocals (MathFast::div_d),
    // the runtime divisors by mk_div (Markstein's correction of the refined
    // v_rcp_f32 reciprocal, range-flagged).  Any flag on any lane of the
    // wave re-runs the block below exactly (wave-uniform: the pair exchanges
    // values).
    bool bad = false;
    auto mdiv = [&](float x, float d) __attribute__((always_inline)) { return mk_div(x, d, bad); };
    auto ddiv = [&](float x, float d, auto rget) __attribute__((always_inline)) {
      const float q = m.div_d(x, d, rget());   // the store has the day constants' double reciprocals
      bad |= m.div_bad(q);
      return q;
    };
    // :283-295
    const bool open = (DC(D_OK) != zero) && (beta > zero);
    bool bo = bad;
    const float q_rsc = mdiv(DC(D_X), DC(D_LAI2) * beta * DC(D_PW28));
    bad = bo | (open && bad);
    float rscf = open ? q_rsc : 1.0E6f;
    rscf = MAXF(rscf, DC(D_RSCMIN));
    // :344-389
    FV<2> c2, s2;
    sp.template pick<2>(
        [&](int h) __attribute__((always_inline)) -> FV<2> {
          const float r = sel(h, rscf, rss);
          const float q = ddiv(r, sp.own_sc(cs, PS_DAY + D_RAARAC, h), [&]() { return sp.own_day_rp(cs, DRP_RAARA, h); });
          const float PM = mdiv(sp.own_sc(cs, PS_DAY + D_NUMC, h), desatdT + gamma * (one + q));
          const float R = sp.own_sc(cs, PS_DAY + D_DGRAC, h) + gamma * r;
          return FV<2>{{PM, R}};
        },
        c2, s2);
    FV<1> cc, cs1;
    sp.template pick<1>(
        [&](int h) __attribute__((always_inline)) -> FV<1> {
          const float Rh = sel(h, c2.v[1], s2.v[1]), Ro = sel(h, s2.v[1], c2.v[1]);
          return FV<1>{{mdiv(one, one + mdiv(Rh * Ra, Ro * (Rh + Ra)))}};
        },
        cc, cs1);
    const float LEf = cc.v[0] * c2.v[0] + cs1.v[0] * s2.v[0];
    const float VDD0f = DC(D_VDD) + ddiv((DC(D_A1) - DC(D_DG) * LEf) * DC(D_RAA), DC(D_RHOCP),
                                              [&]() { return cs.day_r(DR_RHOCP); });
    FV<1> ft, fe;
    sp.template pick<1>(
        [&](int h) __attribute__((always_inline)) -> FV<1> {
          const float r = sel(h, rscf, rss);
          const float d = sp.own_sc(cs, PS_DAY + D_RAC, h);
          auto rr = [&]() __attribute__((always_inline)) { return sp.own_day_rp(cs, DRP_RA, h); };
          const float LEh = mdiv(sp.own_sc(cs, PS_DAY + D_DRR, h) + ddiv(DC(D_RHOCP) * VDD0f, d, rr),
                                 desatdT + gamma * (1.0f + ddiv(r, d, rr)));
          return FV<1>{{ddiv(LEh * 1.0E3f, DC(D_RL), [&]() { return cs.day_r(DR_RL); })}};
        },
        ft, fe);
#if defined(H9G_FORCE_RERUN)   // test builds: the exact block in about one wave-substep of two
    bad |= (__builtin_bit_cast(uint32_t, theta[1]) & 15u) == 0;
#endif
    if (!__builtin_expect(any_lane(bad), 0)) {
      rsc = rscf;
      tran = ft.v[0];
      evg = fe.v[0];
      eb_fast = true;
    }
  }
  if (!eb_fast) {
  H9G_BR(BR_EBX);
  // :283-295
  if ((DC(D_OK) != zero) && (beta > zero))
    rsc = DC(D_X) / (DC(D_LAI2) * beta * DC(D_PW28));
  else
    rsc = 1.0E6f;
  rsc = MAXF(rsc, DC(D_RSCMIN));
  // :344-389.  The canopy (h = 0) and soil (h = 1) halves have the same
  // expressions on different operands: each lane of a pair evaluates one
  // (pick), reading its operands from its own column (D_NUMC comment).
  FV<2> ebc, ebs;                                       // {PM, R}: canopy, soil
  sp.template pick<2>(
      [&](int h) __attribute__((always_inline)) -> FV<2> {
        const float r = sel(h, rsc, rss);
        const float q = divr<CS::kDayRecip>(m, r, sp.own_sc(cs, PS_DAY + D_RAARAC, h),
                                            [&]() { return sp.own_day_rp(cs, DRP_RAARA, h); });
        const float PM = sp.own_sc(cs, PS_DAY + D_NUMC, h) / (desatdT + gamma * (one + q));
        const float R = sp.own_sc(cs, PS_DAY + D_DGRAC, h) + gamma * r;
        return FV<2>{{PM, R}};
      },
      ebc, ebs);
  const float PMc = ebc.v[0], Rc = ebc.v[1], PMs = ebs.v[0], Rs = ebs.v[1];
  FV<1> ccf, csf;                                       // Cc, Cs
  sp.template pick<1>(
      [&](int h) __attribute__((always_inline)) -> FV<1> {
        const float Rh = sel(h, Rc, Rs), Ro = sel(h, Rs, Rc);
        return FV<1>{{one / (one + Rh * Ra / (Ro * (Rh + Ra)))}};
      },
      ccf, csf);
  const float LE = ccf.v[0] * PMc + csf.v[0] * PMs;
  const float VDD0 = DC(D_VDD) + divr<CS::kDayRecip>(m, (DC(D_A1) - DC(D_DG) * LE) * DC(D_RAA), DC(D_RHOCP),
                                                     [&]() { return cs.day_r(DR_RHOCP); });
  FV<1> ftr, fev;                                       // tran, evg
  sp.template pick<1>(
      [&](int h) __attribute__((always_inline)) -> FV<1> {
        const float r = sel(h, rsc, rss);
        const float d = sp.own_sc(cs, PS_DAY + D_RAC, h);
        auto rr = [&]() __attribute__((always_inline)) { return sp.own_day_rp(cs, DRP_RA, h); };
        const float LEh = (sp.own_sc(cs, PS_DAY + D_DRR, h) + divr<CS::kDayRecip>(m, DC(D_RHOCP) * VDD0, d, rr)) /
                          (desatdT + gamma * (1.0f + divr<CS::kDayRecip>(m, r, d, rr)));
        return FV<1>{{divr<CS::kDayRecip>(m, LEh * 1.0E3f, DC(D_RL), [&]() { return cs.day_r(DR_RL); })}};
      },
      ftr, fev);
  tran = ftr.v[0];
  evg = fev.v[0];
  }
  // :396-400
  float em1 = m.div(g.dz(1) * (theta[1] - watmin), dt, g.rdt()) - tran * ROOT(1);
  em1 = MAXF(zero, em1);
  evg = MINF(em1, evg);
  pr.flux(evg, tran);
  // :426-478
  const float qflx_evap = evg;
  float qflx_in_soil = (one - frac_h2osfc) * (qflx_top_soil - qflx_surf);
  qflx_in_soil = qflx_in_soil - (one - frac_h2osfc) * qflx_evap;
  const float qinmax = (one - fsat) * cs.sc(PS_MH3);
  const float qflx_infl_excess = MAXF(zero, qflx_in_soil - (one - frac_h2osfc) * qinmax);
  qflx_infl = qflx_in_soil - qflx_infl_excess;
  qflx_surf = qflx_surf + qflx_infl_excess;
  }  // the front
  if constexpr (ROLE == ROLE_FRONT) {
    *fr = FrontRes{qflx_surf, tran, evg, qflx_infl};
    return 0;
  }
  // :492-508
  float zwtmm = 1000.0f * s.zwt;
  const int jwt = jwt_of<L>(s.zwt, zim);
  const bool aq = (jwt == L);
  cs.launder();
  if constexpr (!kMain && !kChain) pr.mark(1);
  if constexpr (kChain) {
    if (aq) return 0;                      // a substep that starts below the column: the main wave's own
  }

  // :517-567 equilibrium profile and :598-639 conductivity and matric
  // potential, own layers (independent phases)
  float zq[L + 2];
  float hk[L + 1], dhkdw[L + 1], dsmpdw[L + 1];
  // the single powers and the aquifer node (below); a one-column wave's task
  // rounds evaluate them with the per-layer phases and leave picks = false
  constexpr bool kTask = pair1_tasks<M, SP, CS>();
  // the interface fluxes split over the pair (below): a pair lane keeps its own
  // slots' zq (own_q) and hk, dhkdw, smp, dsmpdw (own_k) for them, and hk,
  // dhkdw and dsmpdw, which nothing else on the fast path reads, are not
  // exchanged (kOwnFlux)
  constexpr bool kFluxSplit = H9G_FLUX_SPLIT && CS::kFluxSplit && !M::kExact && !kTask && !kChain;
  constexpr bool kOwnFlux = kFluxSplit && SP::kSpare;
  FV<1> own_q[NT];
  FV<4> own_k[NT];
  FV<1> p0{{zero}}, p1{{zero}};               // lane 0's and lane 1's power
  FV<2> eA{{zero, zero}}, eS{{zero, zero}};
  bool picks = true, aq_task = false;
  // the interface fluxes (below); a one-column wave's round C evaluates them on
  // the task lanes and sets flux_done, with the recharge section's smp, zq of
  // layer max(jwt, 1) in rc_smp, rc_zq
  float c_q[L + 1], c_1[L + 1], c_2[L + 1];
  bool flux_done = false;
  float rc_smp = zero, rc_zq = zero;
  if constexpr (kChain) {                  // the second wave: what the main wave posted before barrier 2
    p0.v[0] = cs.ho(CS::HS_P0);
    p1.v[0] = cs.ho(CS::HS_PY);
    rc_smp = cs.ho(CS::HS_RSMP);
    rc_zq = cs.ho(CS::HS_RZQ);
    picks = false;
    static_assert(!kChain || (kTask && (H9G_P1_TASKS & 2)), "the chain's operands come from the task rounds");
  } else {
    float *const outq[1] = {zq};
    float *const outk[4] = {hk, dhkdw, smp, dsmpdw};
    // exact: the reference expression with every special case redone in place
    auto eq_exact = [&](int t, int h) __attribute__((always_inline)) -> FV<1> {
          H9G_BR(BR_EQX);
          const int i0 = 2 * t + 1;                           // own layer il = i0 + h
          const int il = i0 + h;
          const float zlo = cs.zi(il - 1), zhi = cs.zi(il);   // zi(i-1), zi(i): geometry table
          const float ts = OWN(PF_TS), psi = OWN(PF_PSI);
          float vol_eq;
          if (zwtmm <= zlo) {
            vol_eq = ts;
          } else {
            const float expo = one + OWN(PF_NINVB);
            auto rp = [&]() __attribute__((always_inline)) {
              return join_d(OWN(PF_RPSI0), OWN(PF_RPSI1));
            };
            // temp0 and (below the layer) tempi are independent powers:
            // both bases, then both powers, each pair checked once.  With the
            // water table inside the layer tempi is not evaluated (its base
            // is replaced by 1, whose power is exactly 1 and never special).
            const bool inl = (zwtmm < zhi) && (zwtmm > zlo);
            const float n0 = ((-psi) + zwtmm - zlo), ni = (-psi + zwtmm - zhi);
            bool bq = false;
            float b0 = divr_d<CS::kRecip>(m, n0, -psi, rp, bq);
            float bi = divr_d<CS::kRecip>(m, ni, -psi, rp, bq);
            if (__builtin_expect(bq, 0)) {
              divr_fix<CS::kRecip>(m, b0, n0, -psi);
              divr_fix<CS::kRecip>(m, bi, ni, -psi);
            }
            bi = inl ? one : bi;
            bool s0, si;
            float temp0 = m.powf_d(b0, expo, s0);
            float tpi = m.powf_d(bi, expo, si);
            if (__builtin_expect(s0 | si, 0)) {
              m.powf_fix(temp0, b0, expo, s0);
              m.powf_fix(tpi, bi, expo, si);
            }
            if (inl) {
              const float tempi = one;
              const float voleq1 = OWN(PF_PTE) / (zwtmm - zlo) * (tempi - temp0);
              vol_eq = m.div(voleq1 * (zwtmm - zlo) + ts * (zhi - zwtmm), zhi - zlo, cs.rdz_t(il));   // dz(i)
              vol_eq = MINF(ts, vol_eq);
              vol_eq = MAXF(vol_eq, zero);
            } else {
              vol_eq = vol_eq_below(OWN(PF_C3), ts, tpi, temp0);
            }
          }
          const float qv = divr<CS::kRts>(m, vol_eq, ts, [&]() { return join_d(OWN(PF_RTS0), OWN(PF_RTS1)); });
          return FV<1>{{smp_of(psi, m.powf(MAXX(qv, 0.01f), -OWN(PF_BSW)))}};
    };
    // fast: the same values branch-free (all three cases evaluated, the
    // layer's selected); bad = some quotient or power of the selected case
    // needs its other path (then eq_exact recomputes the slot).  Bases of
    // cases not taken are replaced by 1 so they raise no flag.  eq_body is
    // the slot of layer il, with O(p) the slot's value of field p and zw the
    // water table (mm): a lane's own slot (eq_fast) or, on a spare lane,
    // another pair's last slot (below).
    // inl_all: evaluate the in-layer case for every lane, branch-free (the
    // round where the pairs evaluate their last slot: round 5, 182.7 -> 181.8 ms)
    auto eq_body = [&](int il, auto O, float zw, bool &bad, bool inl_all) __attribute__((always_inline)) -> FV<1> {
          const float zlo = cs.zi(il - 1), zhi = cs.zi(il);
          const float ts = O(PF_TS), psi = O(PF_PSI);
          const bool sat = zw <= zlo;
          const bool inl = (zw < zhi) && (zw > zlo);
          const float expo = one + O(PF_NINVB);
          auto rp = [&]() __attribute__((always_inline)) { return join_d(O(PF_RPSI0), O(PF_RPSI1)); };
          const float n0 = ((-psi) + zw - zlo), ni = (-psi + zw - zhi);
          float b0 = divr_d<CS::kRecip>(m, n0, -psi, rp, bad);
          float bi = divr_d<CS::kRecip>(m, ni, -psi, rp, bad);
          b0 = sat ? one : b0;
          bi = (sat || inl) ? one : bi;
          bool s0, si;
          const float temp0 = m.powf_d(b0, expo, s0);
          const float tpi = m.powf_d(bi, expo, si);
          bad |= s0 | si;
          // water table inside the layer (:530-543): at most one layer of a
          // column, so evaluated only in a slot where some lane of the wave
          // has it (a wave-uniform branch)
          float vin = zero;
          if (inl_all || any_lane(inl)) {
          H9G_BR(BR_INL);
          vin = vol_eq_in_fast(m, [&]() { return O(PF_PTE); }, ts, temp0, zw, zlo, zhi,
                               [&]() { return cs.rdz_t(il); }, inl, bad);   // (round A below keeps a copy)
          }
          // water table below the layer (:548-558)
          const float vbl = vol_eq_below(O(PF_C3), ts, tpi, temp0);
          const float vol_eq = sat ? ts : (inl ? vin : vbl);
          const float qv = divr_d<CS::kRts>(m, vol_eq, ts, [&]() { return join_d(O(PF_RTS0), O(PF_RTS1)); }, bad);
          bool sz;
          const float z = psi * m.powf_d(MAXX(qv, 0.01f), -O(PF_BSW), sz);   // a copy of smp_of (h9g_expr.h)
          bad |= sz;
          return FV<1>{{MAXC(smpmin, z)}};
    };
    auto eq_fast = [&](int t, int h, bool &bad) __attribute__((always_inline)) -> FV<1> {
          return eq_body(2 * t + 1 + h, [&](int p) __attribute__((always_inline)) { return OWN(p); }, zwtmm, bad,
                         false);
    };
    auto hk_exact = [&](int t, int h) __attribute__((always_inline)) -> FV<4> {
          H9G_BR(BR_HKX);
          const int i0 = 2 * t + 1;
          const int ip1 = (L < i0 + 2) ? L : i0 + 2;          // ip of layer i0+1
          const float th = sel(h, theta[i0], theta[i0 + 1]);
          const float thp = sel(h, theta[i0 + 1], theta[ip1]);
          const float ts = OWN(PF_TS);
          const float tsp = sel(h, TS(i0 + 1), TS(ip1));
          float s1 = 0.5f * (th + thp) / (0.5f * (ts + tsp));
          s1 = MINC(one, s1);
          const float bsw = OWN(PF_BSW);
          const float s_node =
              sat_node(divr<CS::kRtsHK>(m, th, ts, [&]() { return join_d(OWN(PF_RTS0), OWN(PF_RTS1)); }));
          // the two powers are independent: one deferred check
          const float ek = 2.0f * bsw + 2.0f, es = -bsw;
          bool sk, ss;
          float pk = m.powf_d(s1, ek, sk);
          float ps = m.powf_d(s_node, es, ss);
          if (__builtin_expect(sk | ss, 0)) {
            m.powf_fix(pk, s1, ek, sk);
            m.powf_fix(ps, s_node, es, ss);
          }
          const float s2 = OWN(PF_HKS) * pk;                  // a copy of hk_dhk (h9g_expr.h)
          FV<4> r;
          r.v[0] = s1 * s2;
          r.v[1] = (2.0f * bsw + 3.0f) * s2 * OWN(PF_ITS);
          const float sm = smp_of(OWN(PF_PSI), ps);
          r.v[2] = sm;
          r.v[3] = dsmpdw_div(bsw, sm, s_node, ts);
          return r;
    };
    // the same, branch-free, flags deferred (par_d); hk_body as eq_body, with
    // the slot's operands theta(i), theta(ip), theta_s(ip) (ip = i + 1, at
    // most L) given
    auto hk_body = [&](auto O, float th, float thp, float tsp, bool &bad) __attribute__((always_inline)) -> FV<4> {
          const float ts = O(PF_TS);
          const float s1 = s1_mk(th + thp, ts + tsp, O(PF_ITS), bad);   // flagged for hk_exact
          const float bsw = O(PF_BSW);
          const float s_node =
              sat_node(divr_d<CS::kRtsHK>(m, th, ts, [&]() { return join_d(O(PF_RTS0), O(PF_RTS1)); }, bad));
          const float ek = 2.0f * bsw + 2.0f, es = -bsw;
          bool sk, ss;
          const float pk = m.powf_d(s1, ek, sk);
          const float ps = m.powf_d(s_node, es, ss);
          bad |= sk | ss;
          FV<4> r;
          hk_dhk(s1, pk, O(PF_HKS), bsw, O(PF_ITS), r.v[0], r.v[1]);
          r.v[2] = smp_of(O(PF_PSI), ps);
          r.v[3] = dsmpdw_fast<L>(bsw, r.v[2], s_node, ts, bad);   // flagged for hk_exact
          return r;
    };
    auto hk_fast = [&](int t, int h, bool &bad) __attribute__((always_inline)) -> FV<4> {
          const int i0 = 2 * t + 1;
          const int ip1 = (L < i0 + 2) ? L : i0 + 2;
          return hk_body([&](int p) __attribute__((always_inline)) { return OWN(p); }, sel(h, theta[i0], theta[i0 + 1]),
                         sel(h, theta[i0 + 1], theta[ip1]), sel(h, TS(i0 + 1), TS(ip1)), bad);
    };
    if constexpr (kTask) {
      // One column per wave: a power per lane.  The powers of these phases and
      // of the single-power and aquifer rounds below have two levels of
      // dependency, so they take two task rounds.  Every task is
      //   q = div_d(num, den, stored reciprocal); x = clamp/select(q);
      //   w = powf_d(x, e); flag = div_bad(q) | powf flag
      // on the operands of eq_body, hk_body and the two pick rounds:
      //   round A, lane 4(i-1)+k, layer i, kind k:
      //     0  b0^expo      (-psi + zw - zi(i-1)) / -psi, 1 where saturated
      //     1  bi^expo      (-psi + zw - zi(i)) / -psi,   1 where sat or in-layer
      //     2  s1^(2b+2)    s1 by Markstein from PF_ITS, before the round
      //     3  s_node^(-b)  theta(i) / ts
      //   lane 4L   (kind 4) the first single power: aquifer temp0 | recharge ka
      //   lane 4L+1 (kind 5) the second: specific yield of layer L | jwt+1
      //   round B, on the lane that holds its operand:
      //     kind 1  (vol_eq(i) / ts)^(-b), vol_eq from the lane's bi^expo and
      //             its neighbour's b0^expo (one DPP move)
      //     kind 4  the aquifer node's zq(L+1), from its temp0
      //     kind 5  the aquifer node's smp1 (theta(L))
      // Lanes past 4L+1 repeat the last task; kinds 0, 2 and 3 repeat kind 1's
      // expressions in round B, unread.  A task's parameters come from the
      // column's LDS block at the task's layer, theta from the rows the pair
      // lanes store it to, zwt and jwt from lane 0.  Each lane also evaluates
      // the rest of its slot's expressions (hk, dhkdw | smp, dsmpdw | zq), so
      // all of it runs once; the pair lanes then read every layer's results
      // from the lanes that hold them, and the flags by ballot.  A flagged task
      // re-runs the pair lanes' slots by eq_exact / hk_exact; a flagged single
      // or aquifer power re-runs the pick rounds below (picks).  Same
      // expressions on the same operands: no bit changes.
      constexpr int NA = 4 * L + 2;
      (void)outq;
      static_assert(NA <= 64 && CS::kRecip && CS::kRts && CS::kRtsHK, "a lane per task, every reciprocal stored");
      const bool st = sp.spare;
      const int hh = sp.h;
#if (H9G_P1_TASKS & 2)
      // round C's divisor of this lane's interface, zc(i+1) - zc(i), and its
      // reciprocal: three registers kept over the year
      float den_l = g.den(1);
      double rden_l = g.rden(1);
#pragma unroll
      for (int i = 2; i <= L - 1; i++)
        if ((sp.ln >> 2) + 1 == i) {
          den_l = g.den(i);
          rden_l = g.rden(i);
        }
      float c_qo, c_d1, c_d2;
#endif
      int ln = sp.ln;
      opaque(ln);                          // the task decode recomputed here, not kept as lane masks over the year
      if (!st) {
#pragma unroll
        for (int t = 0; t < NT; t++) cs.wb[CS::TH0 + 2 * t + hh] = sel(hh, theta[2 * t + 1], theta[2 * t + 2]);
      }
      const float zw = lane0_get(zwtmm);
      const int jwu = lane0_geti(jwt);
      const bool aqu = jwu == L;
      const int jcu = aqu ? L : jwu + 1;
      // ---- round A
      const int ta = ln < NA ? ln : NA - 1;
      const bool lay_a = ta < 4 * L;
      const int ka = lay_a ? (ta & 3) : ta - 4 * L + 4;
      const int ia = lay_a ? (ta >> 2) + 1 : jcu;
      const int ipa = ia < L ? ia + 1 : L;
      const lds_float *oa = cs.wb + (ia - 1);
      const float th = oa[CS::TH0], thp = cs.wb[CS::TH0 + ipa - 1];
      const float ts_a = oa[PF_TS * L], psi_a = oa[PF_PSI * L], bsw_a = oa[PF_BSW * L];
      const float ninv_a = oa[PF_NINVB * L], its_a = oa[PF_ITS * L], hks_a = oa[PF_HKS * L];
      const float pte_a = oa[PF_PTE * L], c3_a = oa[PF_C3 * L];
      const float tsp_a = cs.wb[PF_TS * L + ipa - 1];
      const double rpsi_a = join_d(oa[PF_RPSI0 * L], oa[PF_RPSI1 * L]);
      const double rts_a = join_d(oa[PF_RTS0 * L], oa[PF_RTS1 * L]);
      const float zlo_a = cs.zi(ia - 1), zhi_a = cs.zi(ia);
      const bool sat_a = zw <= zlo_a, inl_a = (zw < zhi_a) && (zw > zlo_a);
      bool s1bad = false;
      const float s1 = s1_mk(th + thp, ts_a + tsp_a, its_a, s1bad);
      const bool by_ts = ka == 2 || ka == 3 || (ka == 4 && !aqu);            // theta / ts, else ... / -psi
      const float nz = (-psi_a + zw) - (ka == 0 ? zlo_a : zhi_a);
      const float num_a = by_ts ? th : (ka == 5 ? zw : nz);
      const float q_a = m.div_d(num_a, by_ts ? ts_a : -psi_a, by_ts ? rts_a : rpsi_a);
      const float sn_a = sat_node(q_a);
      const bool one_a = (ka == 0 && sat_a) || (ka == 1 && (sat_a || inl_a));
      const float x_a = ka == 2 ? s1 : (by_ts ? sn_a : (ka == 5 ? one + q_a : (one_a ? one : q_a)));
      const float e_a = (ka <= 1 || (ka == 4 && aqu)) ? one + ninv_a
                        : ka == 2                     ? 2.0f * bsw_a + 2.0f
                        : ka == 3                     ? -bsw_a
                        : ka == 4                     ? 2.0f * bsw_a + 3.0f
                                                      : ninv_a;
      bool sw_a;
      const float w_a = m.powf_d(x_a, e_a, sw_a);
      bool f_a = m.div_bad(q_a) | sw_a | (ka == 2 && s1bad);
      // ---- the rest of hk_body: kind 2 holds hk, dhkdw, kind 3 smp, dsmpdw
      float o_hk, o_dhk;
      hk_dhk(x_a, w_a, hks_a, bsw_a, its_a, o_hk, o_dhk);
      const float o_sm = smp_of(psi_a, w_a);
      bool b3 = false;
      const float o_ds = dsmpdw_fast<L>(bsw_a, o_sm, x_a, ts_a, b3);
      f_a |= ka == 3 && b3;
      // ---- the rest of eq_body up to vol_eq (:530-558), on kind 1: temp0 is
      // the even neighbour's power
      const float t0 = pair_bcast<0>(w_a);
      const bool inl1 = inl_a && ka == 1;
      float vin = zero;
      if (any_lane(inl1)) {
        H9G_BR(BR_INL);
        const float d0 = zw - zlo_a;             // a copy of vol_eq_in_fast (h9g_expr.h)
        const float q1 = m.div_d(pte_a, d0, recip64(d0));
        const bool bq = m.div_bad(q1);
        const float voleq1 = q1 * (one - t0);
        vin = m.div_d(voleq1 * (zw - zlo_a) + ts_a * (zhi_a - zw), zhi_a - zlo_a, cs.rdz_t(ia));
        f_a |= inl1 && (bq | m.div_bad(vin));
        vin = MINF(ts_a, vin);
        vin = MAXF(vin, zero);
      }
      const float vbl = vol_eq_below(c3_a, ts_a, w_a, t0);
      const float vol_eq = sat_a ? ts_a : (inl_a ? vin : vbl);
      // ve of the aquifer node (:579-584), on kind 4 (its layer is L when aq)
      float ve = zero;
      if (aqu) ve = vol_clamp(vol_aq(pte_a, zw - g.zi(L), w_a), ts_a);
      const uint64_t fl_a = lane_mask(f_a);
      pr.mark(2);
      // ---- round B
      const float num_b = ka == 4 ? ve : (ka == 5 ? th : vol_eq);
      const float q_b = m.div_d(num_b, ts_a, rts_a);
      const float xm_b = MAXX(q_b, 0.01f);
      const float sn_b = sat_node_aq(q_b);
      const float x_b = ka >= 4 ? (aqu ? (ka == 4 ? xm_b : sn_b) : one) : xm_b;
      bool sw_b;
      const float w_b = m.powf_d(x_b, -bsw_a, sw_b);
      const float o_z = smp_of(psi_a, w_b);
      float o_dz = zero;
      if (aqu) o_dz = dsmpdw_div(bsw_a, o_z, x_b, ts_a);      // dsmpdw1, on kind 5
      const uint64_t fl_b = lane_mask((m.div_bad(q_b) | sw_b) && (ka == 1 || (ka >= 4 && aqu)));
      // ---- flags (wave-uniform): the pair lanes' exact re-runs
      constexpr uint64_t ALL_A = (1ull << (4 * L)) - 1;
      const bool bad_eq = (((fl_a & 0x3333333333333333ull) | (fl_b & 0x2222222222222222ull)) & ALL_A) != 0;
      const bool bad_hk = (fl_a & 0xCCCCCCCCCCCCCCCCull & ALL_A) != 0;
      const bool bad_pk = ((fl_a >> (4 * L)) & 3) != 0 || (aqu && ((fl_b >> (4 * L)) & 3) != 0);
      int vz = 0;
      opaque(vz);
      bool slow = true;                    // the pair lanes evaluate the fluxes themselves
#if (H9G_P1_TASKS & 2)
      // ---- round C: the tridiagonal's interface fluxes (flux3_f below, the
      // same expressions on the same operands), interface i on the kind-2 lane
      // of layer i, which holds hk(i), dhkdw(i): smp, dsmpdw of layers i and
      // i+1 from their kind-3 lanes, zq of both from their kind-1 lanes.  The
      // aquifer interface (i = L, read only when aqu) takes smp1, dsmpdw1
      // from lane 4L+1 and zq(L+1) from lane 4L.
      {
        const bool top = ia == L;
        const float n_sm = ka == 5 ? o_z : o_sm, n_ds = ka == 5 ? o_dz : o_ds;
        const int sn = top ? 4 * L + 1 : ln + 5, zn = top ? 4 * L : ln + 3;
        const float sm_i = lane_get(o_sm, (ln + 1) & 63), ds_i = lane_get(o_ds, (ln + 1) & 63);
        const float sm_n = lane_get(n_sm, sn & 63), ds_n = lane_get(n_ds, sn & 63);
        const float zq_i = lane_get(o_z, (ln + 63) & 63), zq_n = lane_get(o_z, zn & 63);
        float den_c = den_l;
        double rden_c = rden_l;
        if (aqu) {
          const float zcA_c = 0.5f * (zw + g.zc(L));
          const float dA = zcA_c - g.zc(L);
          const double rA = recip64(dA);
          den_c = top ? dA : den_c;
          rden_c = top ? rA : rden_c;
        }
        const float num = flux_num(sm_n, sm_i, zq_n, zq_i);
        c_qo = m.div_d(flux_q(o_hk, num), den_c, rden_c);
        c_d1 = m.div_d(flux_d1(o_hk, num, ds_i, o_dhk), den_c, rden_c);
        c_d2 = m.div_d(flux_d2(o_hk, num, ds_n, o_dhk), den_c, rden_c);
        bool f_c = (m.div_bad(c_qo) | m.div_bad(c_d1) | m.div_bad(c_d2)) && ka == 2 && (!top || aqu);
#if defined(H9G_FORCE_RERUN)   // test builds: the pair lanes' flux block in about one wave-substep of two
        f_c |= (__builtin_bit_cast(uint32_t, zw) & 1u) == 0;
#endif
        slow = bad_eq | bad_hk | bad_pk | (lane_mask(f_c) != 0);
      }
      // ---- the pair lanes read every interface's fluxes and every layer's
      // smp (the state, and the next substep's beta), from the lanes that hold
      // them (the index kept in a VGPR: the values stay out of the scalar
      // registers); the recharge section's smp, zq of layer max(jwt, 1)
#pragma unroll
      for (int i = 1; i <= L; i++) {
        const int lb = 4 * (i - 1);
        smp[i] = lane_get(o_sm, vz + lb + 3);
        if (i < L) {
          c_q[i] = lane_get(c_qo, vz + lb + 2);
          c_1[i] = lane_get(c_d1, vz + lb + 2);
          c_2[i] = lane_get(c_d2, vz + lb + 2);
        }
      }
      c_q[L] = c_1[L] = c_2[L] = zero;
      if (aqu) {
        c_q[L] = lane_get(c_qo, vz + 4 * L - 2);
        c_1[L] = lane_get(c_d1, vz + 4 * L - 2);
        c_2[L] = lane_get(c_d2, vz + 4 * L - 2);
      }
      {
        const int lm = 4 * ((jwu > 1 ? jwu : 1) - 1);
        rc_smp = lane_get(o_sm, vz + lm + 3);
        rc_zq = lane_get(o_z, vz + lm + 1);
      }
#endif
      p0.v[0] = lane_get(w_a, vz + 4 * L);
      p1.v[0] = lane_get(w_a, vz + 4 * L + 1);
      // ---- a flagged wave-substep: every layer's results to the pair lanes,
      // which run their own flux block below (a uniform branch, all lanes
      // still here)
      if (__builtin_expect(slow, 0)) {
#pragma unroll
        for (int i = 1; i <= L; i++) {
          const int lb = 4 * (i - 1);
          zq[i] = lane_get(o_z, vz + lb + 1);
          hk[i] = lane_get(o_hk, vz + lb + 2);
          dhkdw[i] = lane_get(o_dhk, vz + lb + 2);
          smp[i] = lane_get(o_sm, vz + lb + 3);
          dsmpdw[i] = lane_get(o_ds, vz + lb + 3);
        }
        if (aqu) {
          eA.v[0] = lane_get(o_z, vz + 4 * L);
          eS.v[0] = lane_get(o_z, vz + 4 * L + 1);
          eS.v[1] = lane_get(o_dz, vz + 4 * L + 1);
        }
      }
      if (st) return 0;                    // the helper lanes' part ends here
      flux_done = !slow;
      if (__builtin_expect(bad_eq, 0)) {
#pragma unroll
        for (int t = 0; t < NT; t++) {
          const FV<1> r = eq_exact(t, hh);
          sp.xchg(r.v[0], zq[2 * t + 1], zq[2 * t + 2]);
        }
      }
      if (__builtin_expect(bad_hk, 0)) {
#pragma unroll
        for (int t = 0; t < NT; t++) {
          const FV<4> r = hk_exact(t, hh);
#pragma unroll
          for (int kk = 0; kk < 4; kk++) sp.xchg(r.v[kk], outk[kk][2 * t + 1], outk[kk][2 * t + 2]);
        }
      }
#if (H9G_P1_TASKS & 2)
      if (__builtin_expect(slow, 0)) {     // the recharge section's operands from the (exact) arrays
#pragma unroll
        for (int i = 1; i <= L; i++)
          if (i == (jwt > 1 ? jwt : 1)) { rc_smp = smp[i]; rc_zq = zq[i]; }
      }
#endif
      aq_task = aqu;
      picks = bad_pk;
    } else if constexpr (SP::kSpare && CS::kSpare && !M::kExact) {
      // Helper lanes (round 4: "spare lanes"; round 5: any number of slots).
      // A wave's C pairs use S = 2C of its 64 lanes; the other H = 64 - S
      // lanes help in these two phases.  The phases take R = ceil(NT S / 64)
      // rounds instead of NT: in round q every pair lane evaluates its own
      // slot U + q (U = NT - R), and the helpers evaluate the first U slots of
      // all pair lanes, task tau = u S + k (slot u of pair lane k) on helper
      // S + tau % H in round tau / H, with k's operands by ds_bpermute
      // (fetched before the rounds) and its parameters from k's LDS column.
      // After the rounds pair lane k takes each helper result, and the flags
      // of that evaluation, from its helper.  The same expressions on the
      // same operands: no bit changes.  A flag on either side re-runs the
      // pair lane's slots exactly, as in par_d.
      //   L = 8,  C = 22: R = 3, U = 1 (round 4's spare lanes: NT - 1 rounds)
      //   L = 10, C = 11: R = 2, U = 3 (h9g_pair11_kernel, small L = 10 shards)
      // The helpers take the FIRST U slots (round 5): the water table lies in
      // layers L-1 or L in most columns, and the equilibrium profile's
      // in-layer case (a wave-uniform branch of ~20 VALU on the round's
      // critical path, :530-543) then runs in the one round where the pairs
      // evaluate their last slot, not in every round that holds a helper's
      // last slot of some pair (branch counts: 1.77 of 3 rounds with the
      // helpers on the last slot; config 2: 186.5 -> 183.7 ms).
      constexpr int S = CS::LANES, H = 64 - S;
      constexpr int R = (NT * S + 63) / 64, U = NT - R, TOT = U * S;
      static_assert(U >= 1 && TOT <= R * H, "the helpers cover the first U slots in R rounds");
      const bool st = sp.spare;
      const int hh = sp.h;
      // helper: its task in round q (idle helpers repeat the last task)
      auto tau_q = [&](int q) __attribute__((always_inline)) {
        const int t = q * H + (st ? sp.ln - S : 0);
        return t < TOT ? t : TOT - 1;
      };
      // pair lane: the helper lane of its slot u, and the round it ran in
      auto src_u = [&](int u) __attribute__((always_inline)) { return S + (u * S + sp.ln) % H; };
      auto qo_u = [&](int u) __attribute__((always_inline)) { return (u * S + sp.ln) / H; };
      // rounds that hold tasks of slot u, and slots that round q holds
      auto qlo = [](int u) constexpr { return (u * S) / H; };
      auto qhi = [](int u) constexpr { return ((u * S + S - 1) / H) < R - 1 ? (u * S + S - 1) / H : R - 1; };
      auto ulo = [](int q) constexpr { return (q * H) / S < U - 1 ? (q * H) / S : U - 1; };
      auto uhi = [](int q) constexpr { return (q * H + H - 1) / S < U - 1 ? (q * H + H - 1) / S : U - 1; };
      // a helper result of every round -> pair lane's slot u.  A ds_bpermute
      // must run in converged control flow: a lane reads only what active
      // lanes provide (a helpers-only fetch under `st ?` read zeros).
      auto back = [&](const float (&v)[R], int u) __attribute__((always_inline)) {
        const int src = src_u(u), qo = qo_u(u);
        float x = lane_get(v[qlo(u)], src);
#pragma unroll
        for (int q = qlo(u) + 1; q <= qhi(u); q++) {
          const float g = lane_get(v[q], src);
          x = qo == q ? g : x;
        }
        return x;
      };
      auto flags_back = [&](int fl) __attribute__((always_inline)) {
        bool any = false;
#pragma unroll
        for (int u = 0; u < U; u++) any |= ((lane_geti(fl, src_u(u)) >> qo_u(u)) & 1) != 0;
        return any;
      };
      {
        float zwk[R];
#pragma unroll
        for (int q = 0; q < R; q++) zwk[q] = lane_get(zwtmm, tau_q(q) % S);
        FV<1> r[NT];
        float rv[R];
        int fl = 0;
#pragma unroll
        for (int q = 0; q < R; q++) {
          const int tau = tau_q(q), k = tau % S, u = tau / S;
          const int t = U + q;
          const lds_float *o = st ? cs.wb + k + u * S : cs.self + t * S;
          bool b = false;
          r[t] = eq_body(st ? 2 * u + 1 + (k & 1) : 2 * t + 1 + hh,
                         [&](int p) __attribute__((always_inline)) { return o[p * NT * S]; },
                         st ? zwk[q] : zwtmm, b, U + q == NT - 1);
          rv[q] = r[t].v[0];
          fl |= (b ? 1 : 0) << q;
        }
#pragma unroll
        for (int u = 0; u < U; u++) r[u].v[0] = back(rv, u);
        const bool bad = !st & ((fl != 0) | flags_back(fl));
        if (__builtin_expect(bad, 0)) {
#pragma unroll
          for (int t = 0; t < NT; t++) r[t] = eq_exact(t, hh);
        }
#pragma unroll
        for (int t = 0; t < NT; t++) {
          sp.xchg(r[t].v[0], zq[2 * t + 1], zq[2 * t + 2]);
          if constexpr (kOwnFlux) own_q[t] = r[t];
        }
      }
      pr.mark(2);
      {
        // this lane's operands of its helper slots u (theta(i), theta(ip),
        // ip = i + 1 <= L as u <= NT - 2), and each helper's of its tasks
        float thu[U], thpu[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          thu[u] = sel(hh, theta[2 * u + 1], theta[2 * u + 2]);
          thpu[u] = sel(hh, theta[2 * u + 2], theta[2 * u + 3]);
        }
        float thk[R], thpk[R];
#pragma unroll
        for (int q = 0; q < R; q++) {
          const int tau = tau_q(q), k = tau % S, u = tau / S;
          float a = lane_get(thu[ulo(q)], k), b = lane_get(thpu[ulo(q)], k);
#pragma unroll
          for (int w = ulo(q) + 1; w <= uhi(q); w++) {
            const float ga = lane_get(thu[w], k), gb = lane_get(thpu[w], k);
            a = u == w ? ga : a;
            b = u == w ? gb : b;
          }
          thk[q] = a;
          thpk[q] = b;
        }
        const lds_float *pe = cs.even + PF_TS * NT * S + (hh ? S : 1);           // TS(i + 1), TS(ip) of own slots
        FV<4> r[NT];
        float rv[4][R];
        int fl = 0;
#pragma unroll
        for (int q = 0; q < R; q++) {
          const int tau = tau_q(q), k = tau % S, u = tau / S;
          const int t = U + q;
          const lds_float *o = st ? cs.wb + k + u * S : cs.self + t * S;
          // TS(ip) of the slot: layer 2t+2 (odd column, row t) for the even
          // lane, 2t+3 (even column, row t+1) for the odd one; TS(L) (odd
          // column, row NT-1) in the last slot
          const lds_float *pt_h = cs.wb + ((k & 1) ? (k & ~1) + S : (k | 1)) + (PF_TS * NT + u) * S;
          const lds_float *pt_own = t == NT - 1 ? cs.even + 1 + (PF_TS * NT + NT - 1) * S : pe + t * S;
          const lds_float *pt = st ? pt_h : pt_own;
          bool b = false;
          r[t] = hk_body([&](int p) __attribute__((always_inline)) { return o[p * NT * S]; },
                         st ? thk[q] : sel(hh, theta[2 * t + 1], theta[2 * t + 2]),
                         st ? thpk[q] : sel(hh, theta[2 * t + 2], theta[2 * t + 3 <= L ? 2 * t + 3 : L]), *pt, b);
#pragma unroll
          for (int kk = 0; kk < 4; kk++) rv[kk][q] = r[t].v[kk];
          fl |= (b ? 1 : 0) << q;
        }
#pragma unroll
        for (int kk = 0; kk < 4; kk++)
#pragma unroll
          for (int u = 0; u < U; u++) r[u].v[kk] = back(rv[kk], u);
        const bool bad = !st & ((fl != 0) | flags_back(fl));
        if (__builtin_expect(bad, 0)) {
#pragma unroll
          for (int t = 0; t < NT; t++) r[t] = hk_exact(t, hh);
        }
#pragma unroll
        for (int t = 0; t < NT; t++) {
#pragma unroll
          for (int kk = 0; kk < 4; kk++)
            if (!kOwnFlux || kk == 2) sp.xchg(r[t].v[kk], outk[kk][2 * t + 1], outk[kk][2 * t + 2]);
          if constexpr (kOwnFlux) own_k[t] = r[t];
        }
      }
    } else if constexpr (kOwnFlux) {
      sp.template par_k<NT, 1, 1u>(eq_fast, eq_exact, outq, own_q);
      pr.mark(2);
      sp.template par_k<NT, 4, 4u>(hk_fast, hk_exact, outk, own_k);
    } else {
      // (round 3: the two phases' slots interleaved in one region, twice the
      // independent powers per region, spilled 225 VGPRs: 214.5 vs 208.9 ms)
      sp.template par_d<NT, 1>(eq_fast, eq_exact, outq);
      pr.mark(2);
      sp.template par_d<NT, 4>(hk_fast, hk_exact, outk);
    }
  }
  if constexpr (SP::kSpare) {
    if (!sp.act()) return 0;             // spare lanes: only the per-layer phases above
  }
  // First round of single powers, one per lane, chosen by where the lane's
  // water table is (jwt = L: below the column), with the lane's operands:
  //   below:  lane 0 temp0 of the aquifer node (:579-580), lane 1 the
  //           specific-yield power of layer L at this zwtmm (:937-940);
  //   inside: lane 0 the recharge conductivity's power (:874-877), lane 1
  //           the specific-yield power of layer jwt+1 (:963-981), both of
  //           the recharge section below, which reads only this substep's
  //           starting theta and zwt.
  // A wave holding columns of both kinds evaluates one round here instead of
  // one per kind (round 3).  The second aquifer round (zq(L+1) and smp1 of the
  // aquifer row, :581-590, :737-741) is read only by lanes below the column:
  // a wave with none skips it (wave-uniform); the deepening loop's rare
  // fall-through below the column evaluates s_y(L) itself for a lane inside.
  bool any_aq_v;
  if constexpr (kTask)
    any_aq_v = aq_task;                       // one column: uniform
  else
    any_aq_v = any_lane(aq);
  const bool any_aq = any_aq_v;
  if (!kTask || __builtin_expect(picks, 0)) {   // (a one-column wave: only when a task round flagged one of them)
  const int jc = aq ? L : jwt + 1;            // the layer whose -psi divides
  float s1c = one, bsw_c = zero;              // recharge operands of layer jwt+1 (:866-873)
  if (any_lane(!aq)) {
    float th_j = zero;
#pragma unroll
    for (int i = 1; i <= L; i++)
      if (i == jc) th_j = theta[i];
    s1c = sat_node(divr<CS::kRts>(m, th_j, cs.lay(PF_TS, jc), [&]() { return lay_d(cs, PF_RTS0, jc); }));
    bsw_c = cs.lay(PF_BSW, jc);
  }
  sp.template pick<1>(
      [&](int h) __attribute__((always_inline)) -> FV<1> {
        const float npsi = -cs.lay(PF_PSI, jc);
        const float num = (aq && h == 0) ? (-PSI(L) + zwtmm - g.zi(L)) : zwtmm;
        bool sq = false, sw = false;
        float q = divr_d<CS::kRecip>(m, num, npsi, [&]() { return lay_d(cs, PF_RPSI0, jc); }, sq);
        const float ninv = cs.lay(PF_NINVB, jc);
        const float e = h ? ninv : (aq ? one + ninv : 2.0f * bsw_c + 3.0f);
        float w = m.powf_d(h ? one + q : (aq ? q : s1c), e, sw);
        if (__builtin_expect(sq | sw, 0)) {                  // one deferred check
          H9G_BR(BR_RECH);
          divr_fix<CS::kRecip>(m, q, num, npsi);
          w = m.powf(h ? one + q : (aq ? q : s1c), e);
        }
        return FV<1>{{w}};
      },
      p0, p1);
  const FV<1> pA = p0;
  if (any_aq) {
  H9G_BR(BR_ANYAQ);
  {
    const float d0 = aq ? (zwtmm - g.zi(L)) : one;
    const float ve = vol_clamp(vol_aq(LAYF(PF_PTE, L), d0, pA.v[0]), TS(L));
    sp.template pick<2>(
        [&](int h) __attribute__((always_inline)) -> FV<2> {
          // the quotient's and the power's checks deferred to one branch
          // (round 2's d878d3e, backed out after a GPU fault that the calls
          // of the then out-of-line redo caused: DESIGN.md §3)
          const float xn = sel(h, ve, theta[L]);
          auto xof = [&](float q2) __attribute__((always_inline)) {
            const float sn = sat_node_aq(q2);
            const float x = sel(h, MAXX(q2, 0.01f), sn);
            return aq ? x : one;
          };
          bool sq = false, sw = false;
          float q2 = divr_d<CS::kRts>(m, xn, TS(L), [&]() { return lay_d(cs, PF_RTS0, L); }, sq);
          float x = xof(q2);
          float pw = m.powf_d(x, -BSW(L), sw);
          if (__builtin_expect(sq | sw, 0)) {
            H9G_BR(BR_AQS);
            divr_fix<CS::kRts>(m, q2, xn, TS(L));
            x = xof(q2);
            pw = m.powf(x, -BSW(L));
          }
          const float z = smp_of(PSI(L), pw);
          return FV<2>{{z, dsmpdw_div(BSW(L), z, x, TS(L))}};
        },
        eA, eS);
  }
  }  // any_aq
  }  // picks
  const FV<1> pY = p1;
  zq[L + 1] = aq ? eA.v[0] : zero;
  const float smp1 = eS.v[0], dsmpdw1 = eS.v[1];
  cs.launder();
  pr.mark(3);
  if constexpr (kMain) {
    // barrier 2 (front_year_pair): the front wave's results of this substep,
    // first read by the rows below.  Lanes 0 and 1 are here on every path (the
    // helper lanes have returned); every STOP of this function lies below.
    // Stamps: p1 is the wait here, the front wave's time that was not covered.
    if constexpr (ROLE == ROLE_MAINS) {    // the chain's operands that only this wave holds
      cs.set_ho(CS::HS_P0, p0.v[0]);
      cs.set_ho(CS::HS_PY, p1.v[0]);
      cs.set_ho(CS::HS_RSMP, rc_smp);
      cs.set_ho(CS::HS_RZQ, rc_zq);
    }
    cs.wg_sync();
    qflx_surf = cs.ho(CS::HO_SURF);
    tran = cs.ho(CS::HO_TRAN);
    evg = cs.ho(CS::HO_EVG);
    qflx_infl = cs.ho(CS::HO_INFL);
    pr.flux(evg, tran);                  // (the front, skipped here, holds the other roles' call)
    pr.mark(1);
  }
  // :645-650 aquifer node geometry
  const float zcA = 0.5f * (zwtmm + g.zc(L));
  const float dzA = (jwt < L) ? g.dz(L) : zwtmm - g.zc(L);
  cs.launder();
  // Tridiagonal system rows 1..L+1 (:661-799), each row eliminated as soon
  // as it is assembled (Thomas forward sweep, :806-831).  The flux terms
  // of interface k are the reference's qout/dqodw1/dqodw2 of row k and,
  // bit for bit the same expressions, qin/dqidw0/dqidw1 of row k+1; they
  // are evaluated once.
  float dwat2[L + 2], GAM[L + 2];
  float BET = zero;
  double rbet = 0.0;
  int zero_pivot = 0;
  // Row i also evaluates the next row's GAM(i+1) = c(i) / BET(i) (the
  // reference's :827 of row i+1): it is independent of dwat2(i), so the two
  // quotients share one deferred check.
  auto row = [&](int i, float am, float bm, float cm, float rm) __attribute__((always_inline)) {
    float x;
    if (i == 1) {
      BET = bm;
      x = rm;
    } else {
      BET = row_bet(am, bm, GAM[i]);
      if (BET == 0.0f && !zero_pivot) zero_pivot = i;
      x = row_x(am, rm, dwat2[i - 1]);
    }
    rbet = recip64(BET);
    dwat2[i] = m.div_d(x, BET, rbet);
    bool bad = m.div_bad(dwat2[i]);
    if (i <= L) {
      GAM[i + 1] = m.div_d(cm, BET, rbet);
      bad |= m.div_bad(GAM[i + 1]);
    }
    if (__builtin_expect(bad, 0)) {
      m.div_fix(dwat2[i], x, BET);
      if (i <= L) m.div_fix(GAM[i + 1], cm, BET);
    }
  };
  // Fast path (MathFast): every interface flux first (branch-free, one
  // deferred check, then the layer arrays die), then the forward sweep,
  // branch-free with its checks deferred to its end.  The two shapes of
  // rows L, L+1 (water table in the column or below it) are one set of
  // expressions with selected operands (a zero operand only where the
  // reference writes one too: x - 0, x + 0).  A flagged quotient, a zero
  // pivot or bm(1) = 0 re-runs the sweep exactly on the (exact) fluxes,
  // raising the reference's STOPs.  Measured: 234.3 -> 230.1 ms (config 2);
  // keeping the layer arrays live for a whole-block redo instead spilled
  // 55 VGPRs and measured 238.9 ms.
  bool tri_ok = kChain;                  // (the chain alone: no system)
  if constexpr (kChain) dwat2[L + 1] = zero;
  if constexpr (!M::kExact && !kChain) {
    bool bad = false, zp = false;
    float qo[L + 1], d1[L + 1], d2[L + 1];
    auto flux3_f = [&](float hki, float num, float dsi, float dsn, float dhk, float den, double rden, int k,
                       bool &b) __attribute__((always_inline)) {
      qo[k] = m.div_d(flux_q(hki, num), den, rden);
      d1[k] = m.div_d(flux_d1(hki, num, dsi, dhk), den, rden);
      d2[k] = m.div_d(flux_d2(hki, num, dsn, dhk), den, rden);
      b |= m.div_bad(qo[k]) | m.div_bad(d1[k]) | m.div_bad(d2[k]);
    };
    if constexpr (kTask && (H9G_P1_TASKS & 2)) {   // a one-column wave: round C's, unless a flag sent it here
#pragma unroll
      for (int i = 1; i <= L; i++) {
        qo[i] = c_q[i];
        d1[i] = c_1[i];
        d2[i] = c_2[i];
      }
    }
    if constexpr (kFluxSplit) {
      // ---- the interface fluxes, split (H9G_FLUX_SPLIT): a third pair-split
      // phase.  Lane h evaluates in slot t interface i = 2t+1+h, between its
      // own layer i and the partner's layer i+1: the even lane 1, 3, .., L-1,
      // the odd lane 2, 4, .., L-2 and in its last slot the aquifer interface
      // L.  flux3_f's expressions on flux3_f's operands, so no bit changes:
      //   hk, dhkdw, smp, dsmpdw, zq of layer i: the lane's own slot results,
      //     kept from the two phases above (own_k, own_q);
      //   smp, zq of layer i+1: from the exchanged arrays, which the state,
      //     beta and the recharge read anyway, by a select on the parity
      //     (smp1, zq(L+1) for the aquifer interface);
      //   dsmpdw of layer i+1: the partner's slot t (even lane) or t+1 (odd
      //     lane), by one select of what to send and one pair_swap per slot --
      //     2 NT + 1 instructions against 3 NT for two broadcasts and a select
      //     -- and dsmpdw1 for the aquifer interface;
      //   den, rden: g.den, g.rden of the two candidate layers selected on the
      //     parity (three selects per slot; constants, no LDS read); the aquifer
      //     interface's zcA - zc(L) and its reciprocal under the wave-uniform
      //     any_aq as before.  Without any_aq the odd lane's last slot runs on
      //     a divisor of 1, raises no flag and yields the zeros of flux3_f's
      //     caller; its flag counts only for a lane with aq.
      // The moves run here, in converged flow (the spare lanes have returned:
      // both lanes of every pair are active); a flagged lane redoes its own
      // slots by div_fix on the operands it holds, before the exchange (par_d).
      // One lane for every layer (SplitAll) runs both parities on the arrays.
      float *const outf[3] = {qo, d1, d2};
      float denA = one;
      double rdenA = 1.0;
      if (any_aq) {
        denA = zcA - g.zc(L);
        rdenA = recip64(denA);
      }
      float ds_n[NT];
      if constexpr (kOwnFlux) {
#pragma unroll
        for (int t = 0; t < NT - 1; t++) ds_n[t] = pair_swap(sel(sp.h, own_k[t + 1].v[3], own_k[t].v[3]));
        ds_n[NT - 1] = sel(sp.h, pair_swap(own_k[NT - 1].v[3]), dsmpdw1);
      }
#if defined(H9G_FORCE_RERUN)
      // test builds: the flag in about one wave-substep of two, in turn on the
      // even lanes, the odd lanes and both (each shape of the lane-local redo)
      const uint32_t f_u = __builtin_bit_cast(uint32_t, lane_get(zwtmm, 0));
      const int f_shape = (f_u & 1u) ? 0 : 1 + (int)((f_u >> 1) % 3u);
#endif
      auto fx_ops = [&](int t, int h, float (&x)[3], float &den, double &rden) __attribute__((always_inline)) {
        const bool last = t == NT - 1;
        const int i0 = 2 * t + 1;
        float hki, dhk, smi, dsi, zqi, dsn;
        if constexpr (kOwnFlux) {
          hki = own_k[t].v[0];
          dhk = own_k[t].v[1];
          smi = own_k[t].v[2];
          dsi = own_k[t].v[3];
          zqi = own_q[t].v[0];
          dsn = ds_n[t];
        } else {
          hki = sel(h, hk[i0], hk[i0 + 1]);
          dhk = sel(h, dhkdw[i0], dhkdw[i0 + 1]);
          smi = sel(h, smp[i0], smp[i0 + 1]);
          dsi = sel(h, dsmpdw[i0], dsmpdw[i0 + 1]);
          zqi = sel(h, zq[i0], zq[i0 + 1]);
          dsn = sel(h, dsmpdw[i0 + 1], last ? dsmpdw1 : dsmpdw[last ? L : i0 + 2]);
        }
        const float smn = sel(h, smp[i0 + 1], last ? smp1 : smp[last ? L : i0 + 2]);
        const float zqn = sel(h, zq[i0 + 1], zq[i0 + 2]);
        den = sel(h, g.den(i0), last ? denA : g.den(last ? i0 : i0 + 1));
        rden = seld(h, g.rden(i0), last ? rdenA : g.rden(last ? i0 : i0 + 1));
        const float num = flux_num(smn, smi, zqn, zqi);
        x[0] = flux_q(hki, num);
        x[1] = flux_d1(hki, num, dsi, dhk);
        x[2] = flux_d2(hki, num, dsn, dhk);
      };
      auto fx_fast = [&](int t, int h, bool &fbad) __attribute__((always_inline)) -> FV<3> {
        float x[3], den;
        double rden;
        fx_ops(t, h, x, den, rden);
        FV<3> r;
        bool b = false;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          r.v[k] = m.div_d(x[k], den, rden);
          b |= m.div_bad(r.v[k]);
        }
        if (t == NT - 1) {
          b = b && (!h || aq);
#pragma unroll
          for (int k = 0; k < 3; k++) r.v[k] = (h && !any_aq) ? zero : r.v[k];
        }
        fbad |= b;
#if defined(H9G_FORCE_RERUN)
        fbad |= f_shape == 3 || f_shape == 1 + h;
#endif
        return r;
      };
      auto fx_exact = [&](int t, int h) __attribute__((always_inline)) -> FV<3> {
        if (t == 0) H9G_BR(BR_TRIFLUX);
        float x[3], den;
        double rden;
        fx_ops(t, h, x, den, rden);
        FV<3> r;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          r.v[k] = m.div_d(x[k], den, rden);
          m.div_fix(r.v[k], x[k], den);
          if (t == NT - 1) r.v[k] = (h && !any_aq) ? zero : r.v[k];
        }
        return r;
      };
      sp.template par_d<NT, 3, NT>(fx_fast, fx_exact, outf);
    } else
    if (!kTask || __builtin_expect(!flux_done, 0)) {
#pragma unroll
    for (int i = 1; i <= L - 1; i++)
      flux3_f(hk[i], flux_num(smp[i + 1], smp[i], zq[i + 1], zq[i]), dsmpdw[i], dsmpdw[i + 1], dhkdw[i], g.den(i),
              g.rden(i), i, bad);
    qo[L] = d1[L] = d2[L] = zero;
    if (any_aq) {                      // aquifer interface (used when aq)
      const float den = zcA - g.zc(L);
      bool ba = false;
      flux3_f(hk[L], flux_num(smp1, smp[L], zq[L + 1], zq[L]), dsmpdw[L], dsmpdw1, dhkdw[L], den, recip64(den), L, ba);
      bad |= aq && ba;
    }
    // fluxes made exact here, so the layer arrays die before the sweep
    if (__builtin_expect(bad, 0)) {
      H9G_BR(BR_TRIFLUX);
#pragma unroll
      for (int i = 1; i <= L; i++) {
        const bool a = i == L;
        const float num = a ? flux_num(smp1, smp[L], zq[L + 1], zq[L]) : flux_num(smp[i + 1], smp[i], zq[i + 1], zq[i]);
        const float dsn = a ? dsmpdw1 : dsmpdw[i < L ? i + 1 : L];
        const float den = a ? zcA - g.zc(L) : g.den(i);
        m.div_fix(qo[i], flux_q(hk[i], num), den);
        m.div_fix(d1[i], flux_d1(hk[i], num, dsmpdw[i], dhkdw[i]), den);
        m.div_fix(d2[i], flux_d2(hk[i], num, dsn, dhkdw[i]), den);
      }
      bad = false;
    }
    }  // !flux_done
    auto row_f = [&](int i, float am, float bm, float cm, float rm) __attribute__((always_inline)) {
      float x;
      if (i == 1) {
        BET = bm;
        x = rm;
      } else {
        BET = row_bet(am, bm, GAM[i]);
        zp |= BET == 0.0f;
        x = row_x(am, rm, dwat2[i - 1]);
      }
      if constexpr (kTask && (H9G_P1_TASKS & 4)) {
        // a lone wave waits on every row's chain: both quotients by Markstein's
        // correction from one refined reciprocal of BET (mk_div), six dependent
        // f32 operations for recip64's and div_d's eight in f64.  The +0
        // operands of rows L and L+1 with the water table in the column pass
        // (mk_div_z); a range flag re-runs the exact sweep like div_bad.
        dwat2[i] = i == L + 1 ? mk_div_z(x, BET, bad) : mk_div(x, BET, bad);
        if (i <= L) GAM[i + 1] = i == L ? mk_div_z(cm, BET, bad) : mk_div(cm, BET, bad);
      } else {
      const double rb = recip64(BET);
      dwat2[i] = m.div_d(x, BET, rb);
      bad |= m.div_bad(dwat2[i]);
      if (i <= L) {
        GAM[i + 1] = m.div_d(cm, BET, rb);
        bad |= m.div_bad(GAM[i + 1]);
      }
      }
    };
    auto dzdt = [&](float dz) __attribute__((always_inline)) {
      const float q = m.div_d(dz, dt, g.rdt());
      bad |= m.div_bad(q);
      return q;
    };
    const float bm1 = dzdt(g.dz(1)) + d1[1];
    row_f(1, zero, bm1, d2[1], qflx_infl - qo[1] - tran * ROOT(1));
#pragma unroll
    for (int i = 2; i <= L - 1; i++)
      row_f(i, -d1[i - 1], dzdt(g.dz(i)) - d2[i - 1] + d1[i], d2[i], qo[i - 1] - qo[i] - tran * ROOT(i));
    row_f(L, -d1[L - 1], dzdt(g.dz(L)) - d2[L - 1] + (aq ? d1[L] : zero), aq ? d2[L] : zero,
          qo[L - 1] - (aq ? qo[L] : zero) - tran * ROOT(L));
    const float qA = dzdt(dzA);
    const float bmA = qA - d2[L] + zero;   // (rows L, L+1: stated again by the exact sweep and the exact path)
    const float rmA = qo[L] - zero;
    row_f(L + 1, aq ? -d1[L] : zero, aq ? bmA : qA, zero, aq ? rmA : zero);
    if (__builtin_expect(bad | zp | (bm1 == 0.0f), 0)) {  // the exact sweep on the (exact) fluxes
      H9G_BR(BR_TRISWEEP);
      BET = zero;
      zero_pivot = 0;
      const float bm1x = m.div(g.dz(1), dt, g.rdt()) + d1[1];
      if (bm1x == 0.0f) { errval = bm1x; STOP_RET(1); }             // :806-812
      row(1, zero, bm1x, d2[1], qflx_infl - qo[1] - tran * ROOT(1));
#pragma unroll
      for (int i = 2; i <= L - 1; i++)
        row(i, -d1[i - 1], m.div(g.dz(i), dt, g.rdt()) - d2[i - 1] + d1[i], d2[i], qo[i - 1] - qo[i] - tran * ROOT(i));
      if (!aq) {
        row(L, -d1[L - 1], m.div(g.dz(L), dt, g.rdt()) - d2[L - 1] + zero, zero, qo[L - 1] - zero - tran * ROOT(L));
        row(L + 1, zero, m.div(dzA, dt, g.rdt()), zero, zero);
      } else {
        row(L, -d1[L - 1], m.div(g.dz(L), dt, g.rdt()) - d2[L - 1] + d1[L], d2[L], qo[L - 1] - qo[L] - tran * ROOT(L));
        row(L + 1, -d1[L], m.div(dzA, dt, g.rdt()) - d2[L] + zero, zero, qo[L] - zero);
      }
      if (zero_pivot) { errval = (float)zero_pivot; STOP_RET(2); }   // :818-825
    }
    tri_ok = true;
  }
  if (!tri_ok) {
  // qout, dqodw1, dqodw2 of one interface: independent quotients, one check.
  auto flux3 = [&](float hki, float num, float dsi, float dsn, float dhk, float den, double rden, float &qo,
                   float &d1, float &d2) __attribute__((always_inline)) {
    const float x0 = flux_q(hki, num), x1 = flux_d1(hki, num, dsi, dhk), x2 = flux_d2(hki, num, dsn, dhk);
    qo = m.div_d(x0, den, rden);
    d1 = m.div_d(x1, den, rden);
    d2 = m.div_d(x2, den, rden);
    if (__builtin_expect(m.div_bad(qo) | m.div_bad(d1) | m.div_bad(d2), 0)) {
      m.div_fix(qo, x0, den);
      m.div_fix(d1, x1, den);
      m.div_fix(d2, x2, den);
    }
  };
  float q_prev, dq0_prev, dq1_prev;      // interface i-1
  {
    const float den = g.den(1);
    const double rden = g.rden(1);
    // num, here and in the two blocks below: flux_num (h9g_expr.h) with dzq first, as the reference has it
    const float dzq = (zq[2] - zq[1]);
    const float num = (smp[2] - smp[1]) - dzq;
    float qout, dqodw1, dqodw2;
    flux3(hk[1], num, dsmpdw[1], dsmpdw[2], dhkdw[1], den, rden, qout, dqodw1, dqodw2);
    const float bm1 = m.div(g.dz(1), dt, g.rdt()) + dqodw1;
    if (bm1 == 0.0f) { errval = bm1; STOP_RET(1); }                 // :806-812
    row(1, zero, bm1, dqodw2, qflx_infl - qout - tran * ROOT(1));
    q_prev = qout; dq0_prev = dqodw1; dq1_prev = dqodw2;
  }
#pragma unroll
  for (int i = 2; i <= L - 1; i++) {
    const float den = g.den(i);
    const double rden = g.rden(i);
    const float dzq = zq[i + 1] - zq[i];
    const float num = (smp[i + 1] - smp[i]) - dzq;
    float qout, dqodw1, dqodw2;
    flux3(hk[i], num, dsmpdw[i], dsmpdw[i + 1], dhkdw[i], den, rden, qout, dqodw1, dqodw2);
    row(i, -dq0_prev, m.div(g.dz(i), dt, g.rdt()) - dq1_prev + dqodw1, dqodw2,
        q_prev - qout - tran * ROOT(i));
    q_prev = qout; dq0_prev = dqodw1; dq1_prev = dqodw2;
  }
  {
    constexpr int i = L;
    if (i > jwt) {                 // water table inside the column
      const float qout = zero, dqodw1 = zero;
      row(i, -dq0_prev, m.div(g.dz(i), dt, g.rdt()) - dq1_prev + dqodw1, zero,
          q_prev - qout - tran * ROOT(i));
      row(i + 1, zero, m.div(dzA, dt, g.rdt()), zero, zero);
    } else {                       // below: aquifer row (smp1, dsmpdw1 from the pair split)
      const float den = zcA - g.zc(i);
      const double rden = recip64(den);
      const float dzq = zq[i + 1] - zq[i];
      const float num = smp1 - smp[i] - dzq;
      float qout, dqodw1, dqodw2;
      flux3(hk[i], num, dsmpdw[i], dsmpdw1, dhkdw[i], den, rden, qout, dqodw1, dqodw2);
      row(i, -dq0_prev, m.div(g.dz(i), dt, g.rdt()) - dq1_prev + dqodw1, dqodw2,
          q_prev - qout - tran * ROOT(i));
      const float qout1 = zero, dqodw1b = zero;
      row(i + 1, -dqodw1, m.div(dzA, dt, g.rdt()) - dqodw2 + dqodw1b, zero, qout - qout1);
    }
  }
  if (zero_pivot) { errval = (float)zero_pivot; STOP_RET(2); }       // :818-825
  }  // !tri_ok
  if constexpr (!kChain) {
#pragma unroll
  for (int i = L; i >= 1; i--) dwat2[i] = dwat2[i] - GAM[i + 1] * dwat2[i + 1];
  // :845-850
#pragma unroll
  for (int i = 1; i <= L; i++) h2o[i] = h2o[i] + dwat2[i] * g.dz(i);
  }
  cs.launder();
  pr.mark(4);
  // The water-table chain, :856-1123: from here to pr.mark(6).  Its results
  // besides the state: rsub_top and the final jwt (read by the sections after
  // it) and additions to h2osoi_liq of up to two layers (add_h2o).  The main
  // wave of a column whose second wave takes the chain (ROLE_MAINS) runs it
  // only for a substep that starts below the column, whose recharge is the
  // sweep's: the branches of a water table in the column do not exist there
  // (kOwn; no block around the text: a scope of its own moved the 22-column
  // kernel's code), and in a substep that is the second wave's it passes over
  // the powers of the baseflow section and takes everything from the
  // hand-over rows below.  The second wave (kChain) posts the additions
  // instead of adding.
  constexpr bool kOwn = ROLE != ROLE_MAINS;
  float rsub_top;
  int jwt3;
  // h2o(I) = h2o(I) + v, I at runtime: a select per layer (opaque, so it is
  // not folded back into an indexed store that would demote h2o to scratch)
  auto add_h2o = [&](int i, float v) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 1; j <= L; j++) {
      int hit = (j == i);
      opaque(hit);
      h2o[j] = hit ? h2o[j] + v : h2o[j];
    }
  };
  // The specific yield s_y(I) = max(ts(I) (1 - (1 + zwtmm/(-psi(I)))^(-1/b(I))),
  // 0.02) (:963-965, :979-981, :1077-1080), for a layer i at runtime.
  auto s_y_base = [&](int i, float zmm) __attribute__((always_inline)) -> float {
    return one + divr<CS::kRecip>(m, zmm, -cs.lay(PF_PSI, i), [&]() { return lay_d(cs, PF_RPSI0, i); });
  };
  auto s_y_of = [&](int i, float pw) __attribute__((always_inline)) -> float {
    return MAXX(cs.lay(PF_TS, i) * (one - pw), 0.02f);
  };
  auto s_y_at = [&](int i, float zmm) __attribute__((always_inline)) -> float {
    return s_y_of(i, m.powf(s_y_base(i, zmm), cs.lay(PF_NINVB, i)));
  };
  // :856-904 recharge.  With the water table in the column, the power of
  // the recharge conductivity ka (:874-877) and the power of the first
  // layer the water-table loops below visit, s_y(jwt+1) at this zwtmm, are
  // independent: one lane of the pair evaluates each.
  float qcharge, sy_first = zero;
  if (kOwn && jwt < L) {
    H9G_BR(BR_JWTCOL);
    // operands of layer jwt+1 (and jwt): the parameters by runtime-indexed
    // store reads, the register arrays by selects
    const int j1 = jwt + 1;
    const float hks_j = cs.lay(PF_HKS, j1);
    float smp_m = zero, zq_m = zero, zc_j = zero;
    if constexpr (kTask && (H9G_P1_TASKS & 2)) {   // from round C's lane reads (or its fallback)
      smp_m = rc_smp;
      zq_m = rc_zq;
#pragma unroll
      for (int i = 1; i <= L; i++)
        if (i == jwt) zc_j = g.zc(i);
    } else {
#pragma unroll
    for (int i = 1; i <= L; i++) {
      if (i == (jwt > 1 ? jwt : 1)) { smp_m = smp[i]; zq_m = zq[i]; }
      if (i == jwt) zc_j = g.zc(i);
    }
    }
    const float wh_zwt = zero;
    // the two powers came from the first round above (p0, p1)
    sy_first = s_y_of(jwt + 1, p1.v[0]);
    const float ka = hks_j * p0.v[0];
    const float smp1m = MAXC(smpmin, smp_m);
    const float wh = smp1m - zq_m;
    if (jwt == 0)
      qcharge = -ka * (wh_zwt - wh) / (zwtmm + one);
    else
      qcharge = -ka * (wh_zwt - wh) / ((zwtmm - zc_j) * 2.0f);
    qcharge = MAXC(-10.0f / dt, qcharge);
    qcharge = MINC(10.0f / dt, qcharge);
  } else {
    qcharge = m.div(dwat2[L + 1] * dzA, dt, g.rdt());
  }
  // :923-1009 water table from recharge.  s_y(I) is evaluated for exactly
  // the layers the loops visit (usually one), at a runtime layer index (the
  // first visit's from the pick above); rous = s_y(L) of the pre-update
  // zwtmm came from the pair split of the equilibrium profile.
  float rous = MAXX(TS(L) * (one - pY.v[0]), 0.02f);
  // x / 1000 in the water-table loops, which run only for a substep that
  // started with the water table in the column (a day snapshot exists): a
  // quotient that needs the IEEE division (subnormal) asks for the exact
  // re-run of the substep instead of a redo branch in place (round 5: -0.45%)
  auto wdiv = [&](float x) __attribute__((always_inline)) {
    if constexpr (!M::kExact) {
      const float q = m.div_d(x, 1000.0f, r1000);
      m.special |= m.div_bad(q);
      return q;
    } else {
      return m.div(x, 1000.0f, r1000);
    }
  };
  int jwt2 = jwt;
  if (jwt == L) {
    s.wa = s.wa + qcharge * dt;
    s.zwt = s.zwt - m.div(qcharge * dt, 1000.0f, r1000) / rous;
  } else if (kOwn) {
    float qcharge_tot = qcharge * dt;
    if (qcharge_tot > zero) {          // rising: I = jwt+1 .. 1
      visit_layers(m, [&](int k) __attribute__((always_inline)) -> bool {
        const int i = jwt + 1 - k;
        const float s_y = k == 0 ? sy_first : s_y_at(i, zwtmm);
        float qcl = MINF(qcharge_tot, s_y * (zwtmm - cs.zi(i - 1)));
        qcl = MAXF(qcl, zero);
        if (s_y > zero) s.zwt = s.zwt - wdiv(qcl / s_y);
        qcharge_tot = qcharge_tot - qcl;
        return !(qcharge_tot <= zero || i == 1);
      });
    } else {                            // deepening: I = jwt+1 .. L
      visit_layers(m, [&](int k) __attribute__((always_inline)) -> bool {
        const int i = jwt + 1 + k;
        const float s_y = k == 0 ? sy_first : s_y_at(i, zwtmm);
        float qcl = MAXF(qcharge_tot, -s_y * (cs.zi(i) - zwtmm));
        qcl = MINF(qcl, zero);
        qcharge_tot = qcharge_tot - qcl;
        if (qcharge_tot >= zero) {
          s.zwt = s.zwt - wdiv(qcl / s_y);
          return false;
        }
        s.zwt = cs.zim(i);
        return i != L;
      });
      if (qcharge_tot > zero) {
        if (!aq) rous = s_y_at(L, zwtmm);    // this lane's first round was the recharge's
        s.zwt = s.zwt - wdiv(qcharge_tot) / rous;
      }
    }
    jwt2 = jwt_of<L>(s.zwt, zim);
  }
  cs.launder();
  pr.mark(5);
  // :1015-1035 baseflow; s_y(L) for the new zwtmm (:1077-1080) on one lane
  // of the pair, the drainage loop's first layer s_y(jwt2+1) on the other
  zwtmm = 1000.0f * s.zwt;
  // rsub_top's exponential and the pair's power are independent: both
  // branch-free, one deferred check (before the pair exchange).
  const int jd = jwt2 < L ? jwt2 + 1 : L;
  FV<1> pR, pD;
  sp.template pick<1>(
      [&](int h) __attribute__((always_inline)) -> FV<1> {
        const int i = h ? jd : L;
        if constexpr (!kOwn) {           // (the second wave's substep)
          if (!aq) {
            rsub_top = zero;
            return FV<1>{{zero}};
          }
        }
        bool se = false, sq = false, sw = false;
        float ex = expf_fast(m, -fff * s.zwt, se);
        const float nb = -cs.lay(PF_PSI, i);
        float q = divr_d<CS::kRecip>(m, zwtmm, nb, [&]() { return lay_d(cs, PF_RPSI0, i); }, sq);
        float w = m.powf_d(one + q, cs.lay(PF_NINVB, i), sw);
        if (__builtin_expect(se | sq | sw, 0)) {
          H9G_BR(BR_BASE);
          if (se) ex = m.expf(-fff * s.zwt);
          divr_fix<CS::kRecip>(m, q, zwtmm, nb);
          w = m.powf(one + q, cs.lay(PF_NINVB, i));
        }
        rsub_top = 5.5E-3f * ex;
        return FV<1>{{w}};
      },
      pR, pD);
  rous = s_y_of(L, pR.v[0]);
  const float sy_drain = s_y_of(jd, pD.v[0]);
  // :1048-1118
  jwt3 = jwt2;
  if (jwt2 == L) {
    s.wa = s.wa - rsub_top * dt;
    s.zwt = s.zwt + m.div(rsub_top * dt, 1000.0f, r1000) / rous;
    if constexpr (kChain) {              // (the same sum, by add_h2o on the main wave)
      cs.set_ho(CS::HS_I0, (float)L);
      cs.set_ho(CS::HS_R0, MAXF(0.0f, (s.wa - 5000.0f)));
    } else {
    h2o[L] = h2o[L] + MAXF(0.0f, (s.wa - 5000.0f));
    }
    s.wa = MINF(s.wa, 5000.0f);
  } else if (kOwn) {
    float rsub_top_tot = -rsub_top * dt;
    if (rsub_top_tot > zero) { errval = rsub_top_tot; STOP_RET(3); }
    visit_layers(m, [&](int k) __attribute__((always_inline)) -> bool {   // I = jwt+1 .. L
      const int i = jwt2 + 1 + k;
      const float s_y = k == 0 ? sy_drain : s_y_at(i, zwtmm);
      float rstl = MAXF(rsub_top_tot, -(s_y * (cs.zi(i) - zwtmm)));
      rstl = MINF(rstl, zero);
      if constexpr (kChain) {           // h2o(I) = h2o(I) + rstl, on the main wave
        cs.set_ho(CS::HS_I0 + 2 * k, (float)i);
        cs.set_ho(CS::HS_R0 + 2 * k, rstl);
      } else {
#pragma unroll
      for (int j = 1; j <= L; j++) {    // h2o(I) = h2o(I) + rstl, I at runtime: a select per
        int hit = (j == i);             // layer (opaque, so it is not folded back into an
        opaque(hit);                    // indexed store that would demote h2o to scratch)
        h2o[j] = hit ? h2o[j] + rstl : h2o[j];
      }
      }
      rsub_top_tot = rsub_top_tot - rstl;
      if (rsub_top_tot >= zero) {
        s.zwt = s.zwt - wdiv(rstl / s_y);
        return false;
      }
      s.zwt = cs.zim(i);
      return i != L;
    });
    s.zwt = s.zwt - wdiv(rsub_top_tot) / rous;
    s.wa = s.wa + rsub_top_tot;
    jwt3 = jwt_of<L>(s.zwt, zim);
  }
  // :1122-1123
  s.zwt = MAXF(0.0f, s.zwt);
  s.zwt = MINC(80.0f, s.zwt);
  if constexpr (kChain) {                // the second wave's call ends here (front_year_pair posts the state)
    cs.set_ho(CS::HS_RSUB, rsub_top);
    cs.set_ho(CS::HS_JWT, (float)jwt3);
    pr.mark(6);
    return 0;
  }
  if constexpr (ROLE == ROLE_MAINS) {
    // barrier 3 (front_year_pair): the second wave's chain of this substep.
    // Lanes 0 and 1 are here on every path but a STOP's, which passes the
    // barrier where it returns (STOP_RET).  Stamps: with the chain on the
    // second wave p5 is the wait here and p6 the taking over.
    cs.wg_sync();
    if (!aq) {
      pr.mark(5);
      s.zwt = cs.ho(CS::HS_ZWT);
      s.wa = cs.ho(CS::HS_WAO);
      rsub_top = cs.ho(CS::HS_RSUB);
      jwt3 = (int)cs.ho(CS::HS_JWT);
      const int scode = (int)cs.ho(CS::HS_CODE);
      if (__builtin_expect(scode != 0, 0)) {   // the chain's STOP 3 (:1048), where the reference raises it
        errval = cs.ho(CS::HS_ERRV);
        return scode;
      }
      m.special |= cs.ho(CS::HS_FLAG) != zero;
      const int i0 = (int)cs.ho(CS::HS_I0), i1 = (int)cs.ho(CS::HS_I1);
      if (i0) add_h2o(i0, cs.ho(CS::HS_R0));
      if (i1) add_h2o(i1, cs.ho(CS::HS_R1));
    }
  }
  cs.launder();
  pr.mark(6);
  // :1131-1137 saturation excess, bottom-up bucket
#pragma unroll
  for (int i = L; i >= 2; i--) {
    const float cap = MAXF(0.01f, TS(i)) * g.dz(i);
    const float xsi = MAXF(h2o[i] - cap, zero);
    h2o[i] = MINF(cap, h2o[i]);
    h2o[i - 1] = h2o[i - 1] + xsi;
  }
  // :1144-1152
  const float xs1 = MAXF(MAXF(h2o[1], zero) - cs.sc(PS_TSDZ1), zero);
  h2o[1] = MINF(cs.sc(PS_TSDZ1), h2o[1]);
  float qflx_rsub_sat = m.div_d(xs1, dt, g.rdt());   // checked with the watmin section's branch
  // :1161-1211 watmin.  With no layer below watmin every xs is zero and
  // every update below is an identity (x + 0 would change only x = -0, and
  // -0 < watmin), so a lane with no layer below watmin skips the section:
  // one rarely-taken branch instead of one per layer.
  bool low = false;
#pragma unroll
  for (int i = 1; i <= L; i++) low |= h2o[i] < watmin;
  if (__builtin_expect(low | m.div_bad(qflx_rsub_sat), 0)) {
  H9G_BR(BR_WATMIN);
  m.div_fix(qflx_rsub_sat, xs1, dt);
  // :1161-1174 watmin top-down
#pragma unroll
  for (int i = 1; i <= L - 1; i++) {
    float xs = zero;
    if (h2o[i] < watmin) {
      xs = watmin - h2o[i];
      if (i == jwt3) s.zwt = s.zwt + m.div(xs / MAXF(0.01f, TS(i)), 1000.0f, r1000);
    }
    h2o[i] = h2o[i] + xs;
    h2o[i + 1] = h2o[i + 1] - xs;
  }
  // :1180-1211 bottom layer from above
  float xs = zero;
  if (h2o[L] < watmin) {
    xs = watmin - h2o[L];
    bool active = true;
#pragma unroll
    for (int j = L - 1; j >= 1; j--) {
      if (active) {
        const float avail = MAXF(h2o[j] - watmin - xs, zero);
        if (avail >= xs) {
          h2o[L] = h2o[L] + xs;
          h2o[j] = h2o[j] - xs;
          xs = zero;
          active = false;
        } else {
          h2o[L] = h2o[L] + avail;
          h2o[j] = h2o[j] - avail;
          xs = xs - avail;
        }
      }
    }
  }
  h2o[L] = h2o[L] + xs;
  rsub_top = rsub_top - m.div(xs, dt, g.rdt());
  }  // low
  // :1221-1236.  The end-of-step theta (:1233) is read only by the daily
  // sums after the day's last substep (the next substep recomputes theta
  // from h2osoi_liq, :141-151), so cell_year_pair evaluates it once a day.
  float w1 = ((1.0f - frac_h2osfc) * (qflx_surf + evg + tran) + rsub_top + qflx_rsub_sat) * dt + s.wa;
#pragma unroll
  for (int i = 1; i <= L; i++) w1 = w1 + h2o[i];
  pr.mark(7);
  // :1244
  if (absf(w1 - w0) > 0.1f) { errval = w1 - w0; return 4; }
  // :1282-1283
  rnf_sum = rnf_sum + qflx_surf * dt;
  rnf_sum = rnf_sum + rsub_top * dt;
  return 0;
#undef TS
#undef HKS
#undef BSW
#undef PSI
#undef LAYF
#undef ROOT
#undef DC
#undef OWN
#undef STOP_RET
}

// The day snapshot (sv_* of the store): the state at the start of substep
// SV_NS of the current day -- h2osoi_liq, smp, zwt, wa and the runoff sum.
// cell_year_pair writes it at most once a day, before the day's first
// substep with the water table in the column; the exact re-run below
// advances it.  Round 2 rewrote it before every substep (11 stores per lane
// per substep, 4.5 GB per config-2 launch written back from L2) although
// only the rare re-run reads it.
template <int L, class SP, class CS>
H9K_HD void save_day(const SP &sp, const CS &cs, const St<L> &s, float rnf_sum, int ns) {
  save_layers<L>(sp, cs, 0, s.h2o);
  save_layers<L>(sp, cs, 1, s.smp);
  cs.sv_set_sc(SV_ZWT, s.zwt);
  cs.sv_set_sc(SV_WA, s.wa);
  cs.sv_set_sc(SV_RNF, rnf_sum);
  cs.sv_set_sc(SV_NS, (float)ns);
}

// Exact re-run (rare path, out of line): from the snapshot (the state at
// the start of substep SV_NS of the day) through substep ns, one lane
// computing every layer with the full glibc special-case logic.  The fast
// path's substeps before ns are bit-identical to these, so replaying them
// reproduces its state exactly.  The snapshot then holds the state after ns.
// EV (the ET kernels): the evaporation sum too, from SV_EVAP and back.
template <int L, class G, class CS, bool EV = false>
H9K_RARE int substep_exact_pair(const G *g, CS cs, const uint64_t *e2, const double *l2, int ns) {
  cs.sv_sync();
  St<L> s;
#pragma unroll
  for (int i = 1; i <= L; i++) {
    s.h2o[i] = cs.sv_lay(0, i);
    s.smp[i] = cs.sv_lay(1, i);
  }
  s.zwt = cs.sv_sc(SV_ZWT);
  s.wa = cs.sv_sc(SV_WA);
  float rnf = cs.sv_sc(SV_RNF), errval = zero;
  MathExact me{{e2, l2}};
  const SplitAll sa;
  typename std::conditional<EV, EvapProf, NoProf>::type np;
  if constexpr (EV) np = EvapProf{cs.sv_sc(SV_EVAP), g->dt()};
  int code = 0;
  H9G_EXACT_HOOK((int)cs.sv_sc(SV_NS), ns);
  for (int k = (int)cs.sv_sc(SV_NS); k <= ns && !code; k++)
    code = hydrology_pair<L, G, MathExact, SplitAll, CS, decltype(np)>(*g, cs, sa, s, rnf, errval, me, np);
  cs.launder();
#pragma unroll
  for (int i = 1; i <= L; i++) {
    cs.sv_set_lay(0, i, s.h2o[i]);
    cs.sv_set_lay(1, i, s.smp[i]);
  }
  cs.sv_set_sc(SV_ZWT, s.zwt);
  cs.sv_set_sc(SV_WA, s.wa);
  cs.sv_set_sc(SV_RNF, rnf);
  cs.sv_set_sc(SV_ERR, errval);
  cs.sv_set_sc(SV_NS, (float)(ns + 1));
  if constexpr (EV) cs.sv_set_sc(SV_EVAP, np.sum);
  cs.sv_sync();
  return code;
}

// Substep ns of the day on the fast path.  A pair re-runs (exactly, from the
// day snapshot) if either of its lanes needs a third water-table layer visit.
// `snapped`: the day snapshot was taken today, at or before this substep.
// Only a substep that starts with the water table in the column (jwt < L)
// can ask for the re-run -- the rising/deepening loops run only for jwt < L
// and the drainage loop only for jwt2 < L, where HYDROLOGY.f90 recomputes
// jwt2 only in the jwt < L branch (:995-1005), so a substep starting below
// the column keeps jwt2 = L -- and cell_year_pair snapshots before the
// first such substep of the day.  A request without a snapshot would replay
// another day's (or, after the yearly re-sort, another cell's) block: it is
// reported as H9G_ERR_NOSNAP instead (never raised by a correct
// build, tests/test_kernel_host.py forces it).
template <int L, class G, class SP, class CS, class PR>
H9K_HD int substep_pair(const G &g, CS cs, const SP &sp, St<L> &s, float &rnf_sum, float &errval,
                        const h9m::Tabs &T, PR &pr, int ns, bool snapped) {
  pr.mark(0);
  H9G_BR(BR_SUBSTEP);
#if defined(H9G_ISA_MARK) && defined(__HIP_DEVICE_COMPILE__)
  asm volatile("; h9g-substep");     // tools/isa_mix.py: once per substep
#endif
  MathFast mf{T, false};
#if defined(H9G_FORCE_RERUN)
  const bool in_column = s.zwt <= g.zim(L);   // the substeps that may re-run (cell_year_pair)
#elif defined(H9G_FORCE_RERUN_ANY)
  const bool in_column = true;                // test builds: also below the column (-> H9G_ERR_NOSNAP)
#endif
  // (the two-wave shape's main wave: without the front, which its front wave evaluates)
  int code = hydrology_pair<L, G, MathFast, SP, CS, PR, main_role<CS>()>(g, cs, sp, s, rnf_sum, errval, mf, pr);
#if defined(H9G_FORCE_RERUN)
  // test builds: also re-run every H9G_FORCE_RERUN-th substep of a day that
  // could (the exact replay from the day snapshot must reproduce the fast
  // path's state)
  if (sp.act() && in_column && ns % H9G_FORCE_RERUN == H9G_FORCE_RERUN - 1) mf.special = true;
#elif defined(H9G_FORCE_RERUN_ANY)
  if (sp.act() && in_column && ns % H9G_FORCE_RERUN_ANY == H9G_FORCE_RERUN_ANY - 1) mf.special = true;
#endif
  if (__builtin_expect(sp.pair_any(mf.special), 0)) {
    H9G_BR(BR_RERUN);
    if (!snapped) {                          // no snapshot of today to replay from
      errval = (float)ns;
      return H9G_ERR_NOSNAP_K;
    }
#if defined(H9G_COUNT_EXACT) && defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(&h9g_exact_count, 1ull);      // measurement builds only
    atomicAdd(&h9g_exact_wave[(blockIdx.x * 4 + (threadIdx.x >> 6)) & 0xffff], 1u);
#endif
    cs.launder();
    code = substep_exact_pair<L, G, CS, kEvap<PR>>(&g, cs, T.exp2, T.log2, ns);
    cs.launder();
#pragma unroll
    for (int i = 1; i <= L; i++) {
      s.h2o[i] = cs.sv_lay(0, i);
      s.smp[i] = cs.sv_lay(1, i);
    }
    s.zwt = cs.sv_sc(SV_ZWT);
    s.wa = cs.sv_sc(SV_WA);
    rnf_sum = cs.sv_sc(SV_RNF);
    errval = cs.sv_sc(SV_ERR);
    if constexpr (kEvap<PR>) pr.sum = cs.sv_sc(SV_EVAP);
  }
  return code;
}

// Monthly output: what cell_year_pair does at the end of a
// day besides the reference's sums.  The month (0..11) that ends with day d1
// (1-based) of a year of nt days in the calendar of INIT.f90:844-859, or -1.
// From nt alone: the two groups of a launch run different calendar years.
H9K_HD int month_end(int d1, int nt) {
  if (d1 == 31) return 0;
  switch (d1 - (nt == 366 ? 1 : 0)) {      // from February on
    case 59: return 1;
    case 90: return 2;
    case 120: return 3;
    case 151: return 4;
    case 181: return 5;
    case 212: return 6;
    case 243: return 7;
    case 273: return 8;
    case 304: return 9;
    case 334: return 10;
    case 365: return 11;
    default: return -1;
  }
}
// NoMonths: nothing (every kernel but the monthly ones).
struct NoMonths {
  template <int L>
  H9K_HD void day_end(int, int, const gbl_float *, size_t, float) const {}
};
// Months: at a month's last day, the year's 12 + L running sums as they
// stand -- after GROW and the day's additions, undivided (the form `raw`
// gives the day-1 probe) -- into the cell's monthly rows: value k of month
// m at M[(m * (12 + L) + k) * stride].  rnf_sum comes from its register; row
// evap is the reference's zero (it never accumulates evap_sum); the others
// are read back from the annual rows A, which the day has just stored.  The
// sums are not reset: the year's sums stay the reference's, and a month's
// mean is the difference of two snapshots (h9g.h).  Called by active lanes
// only, once a day, outside the substep loop; the test is wave-uniform.
struct Months {
  gbl_float *M;
  size_t stride;
  template <int L>
  H9K_HD void day_end(int day, int nt, const gbl_float *A, size_t as, float rnf_sum) const {
    const int m = month_end(day + 1, nt);
    if (m < 0) return;
    gbl_float *o = M + (size_t)m * (12 + L) * stride;
    float v[12 + L];
#pragma unroll
    for (int k = 0; k < 12 + L; k++) v[k] = k == 2 ? rnf_sum : k == 3 ? zero : A[k * as];
#pragma unroll
    for (int k = 0; k < 12 + L; k++) o[k * stride] = v[k];
  }
};

// MonthsEt: the ET kernels' (EvapProf), with row evap the evaporation sum as
// it stands, like rnf_sum.  M may be null (ET without monthly recording: one
// kernel serves both): nothing is stored then, by a wave-uniform test.
struct MonthsEt {
  gbl_float *M;
  size_t stride;
  template <int L>
  H9K_HD void day_end(int day, int nt, const gbl_float *A, size_t as, float rnf_sum, float evap_sum) const {
    if (!M) return;
    const int m = month_end(day + 1, nt);
    if (m < 0) return;
    gbl_float *o = M + (size_t)m * (12 + L) * stride;
    float v[12 + L];
#pragma unroll
    for (int k = 0; k < 12 + L; k++) v[k] = k == 2 ? rnf_sum : k == 3 ? evap_sum : A[k * as];
#pragma unroll
    for (int k = 0; k < 12 + L; k++) o[k * stride] = v[k];
  }
};

// DaysEt: the day kernels' (h9g_set_days; DESIGN.md §7 "Day records"), with
// EvapProf.  Its month-end part is MonthsEt's (M0 may be null).  Its day part:
// the H9G_NDAYREC values a day leaves -- after the day's last substep, GROW
// and the day's additions -- into the cell's day rows, value r of day d at
// D[(d * 7 + r) * stride]: rnf_sum and evap_sum as they stand (cumulative and
// never reset, as the month-end snapshots), the column's liquid water
// h2osoi_liq(1) + ... + h2osoi_liq(L) added in that order, the day's addend to
// theta_sum(1) (HYDROLOGY.f90:1233), zwt, wa and the LAI GROW left.  D0 may be
// null (the cell order's day-1 probes): nothing is stored then, by a
// wave-uniform test.  stop(): the days a cell that reaches a STOP on day
// `day` does not complete are NaN -- the year's buffer is reused from year to
// year, so the cell's earlier values there must go.
// M0, D0 and A0 are the launch's bases of the monthly, day and annual rows,
// the same for every lane: the cell's own rows lie as far from M0 and D0 as
// its annual rows A from A0, and that offset is taken from A at the day's end,
// so that no per-lane pointer of the policy's is live over the substep loop.
struct DaysEt {
  gbl_float *M0;
  size_t stride;
  gbl_float *D0;
  const gbl_float *A0;
  enum { NREC = 7 };
  template <int L>
  H9K_HD void day_end(int day, int nt, const gbl_float *A, size_t as, float rnf_sum, float evap_sum,
                      const St<L> &s, float theta1) const {
    if (D0) {
      float w = s.h2o[1];
#pragma unroll
      for (int i = 2; i <= L; i++) w = w + s.h2o[i];
      gbl_float *o = D0 + (A - A0) + (size_t)day * NREC * stride;
      o[0] = rnf_sum;
      o[stride] = evap_sum;
      o[2 * stride] = w;
      o[3 * stride] = theta1;
      o[4 * stride] = s.zwt;
      o[5 * stride] = s.wa;
      o[6 * stride] = s.LAI;
    }
    MonthsEt{M0 ? M0 + (A - A0) : nullptr, stride}.template day_end<L>(day, nt, A, as, rnf_sum, evap_sum);
  }
  H9K_HD void stop(int day, int nt, const gbl_float *A) const {
    if (!D0) return;
    gbl_float *o = D0 + (A - A0);
    const float nan = __builtin_nanf("");
    for (size_t k = (size_t)day * NREC; k < (size_t)nt * NREC; k++) o[k * stride] = nan;
  }
};
template <class MO>
constexpr bool kDays = std::is_same<MO, DaysEt>::value;

// The one-column kernel's two waves per column (PairStore kFront; h9g.hip
// h9g_pair1f_kernel: a workgroup is one column's main wave and front wave).
//
// A lone wave issues in order, so the front of the substep (hydrology_pair up
// to the equilibrium profile: about a fifth of the substep, on lanes 0 and 1)
// costs its own length whatever the rest of the SIMDs do.  It reads only the
// previous substep's smp, h2osoi_liq(1), zwt, the day constants and the parked
// plant state; the per-layer rounds A, B and C read none of its results.  So a
// second wave evaluates it while the main wave runs theta and the rounds.
//
// Protocol: two workgroup barriers per substep, one buffer, no spinning.
//   main wave (cell_year_pair)            front wave (front_year_pair)
//     front_post: smp, h2o(1), zwt,
//       go = 0 -> hand-over rows
//     barrier 1 ------------------------- barrier 1
//     theta, rounds A, B, C                 go != 0: leave
//                                           the front from the rows posted
//                                           FrontRes -> hand-over rows
//     barrier 2 ------------------------- barrier 2
//     FrontRes -> registers, p4..p7         (waits at the next barrier 1)
//   at every exit of the year loop:
//     front_done: go = 1, barrier 1 ----- barrier 1, go != 0: leave
// The day constants, the parked plant state and rootr are the block's own
// fields: the main wave writes them (day_consts, GROW) only between a
// barrier 2 and the next barrier 1, when the front wave reads nothing.
// One buffer is enough: the main wave rewrites the posted state after
// barrier 2, when the front wave has read it, and the front wave rewrites
// FrontRes after the next barrier 1, which the main wave reaches only after
// its reads of them have completed (wg_sync waits for the wave's LDS traffic).
//
// Why no wave waits at a barrier its partner does not reach:
//  - The main wave's sequence is (barrier 1, barrier 2) per substep, then one
//    barrier 1 with go = 1; the front wave's is barrier 1, then (barrier 2,
//    barrier 1) for as long as go = 0.  The front wave has no trip counts of
//    its own: it follows go, so the two sequences match whatever ends the year.
//  - Barrier 2 lies on the one path of hydrology_pair<ROLE_MAIN> that lanes 0
//    and 1 take in every substep: no return of the function precedes it except
//    the helper lanes' (lanes of the same wave, which stays).  Every STOP code
//    of the function, H9G_ERR_NOSNAP_K and a STOP of the exact re-run (which
//    evaluates its own front, ROLE_ALL, and holds no barrier) arise after it and
//    leave through cell_year_pair's `code`.
//  - cell_year_pair makes `code` wave-uniform (lane 0's) before it tests it, so
//    the helper lanes leave the year loop with lanes 0 and 1 instead of running
//    the year on alone, barriers included, as they harmlessly do in the
//    single-wave kernel.  Both its exits -- a code, the year's end -- pass
//    front_done once.
//  - pair_body's early returns (slot past the list, non-land cell, stopped
//    cell) are decided by both waves from the same global values before the
//    first barrier 1; then neither wave reaches any.
//
// Round 10 (PairStore kSide, H9G_P1_SIDE): three barriers per substep, the
// water-table chain (hydrology_pair, pr.mark(4) to pr.mark(6)) on the second
// wave beside the main wave's tridiagonal sweep.  Both waves decide from the
// posted zwt whose chain a substep's is: the second wave's when the substep
// starts with the water table in the column (jwt < L), else the main wave's
// as before (the recharge is then the sweep's dwat2(L+1)).
//   main wave                             second wave
//     front_post (and wa), go = 0
//     barrier 1 ------------------------- barrier 1
//     theta, rounds A, B, C                 go != 0: leave
//     the two single powers, smp and        the front, FrontRes -> rows
//       zq of layer max(jwt, 1) -> rows
//     barrier 2 ------------------------- barrier 2
//     FrontRes -> registers                 jwt < L: the chain from the rows
//     the sweep, h2o += dwat2 dz              posted; zwt, wa, rsub_top, jwt,
//     jwt = L: the chain                      flag, STOP 3 and its value, the
//                                             h2o additions -> rows
//     barrier 3 ------------------------- barrier 3
//     jwt < L: the rows -> registers,       (waits at the next barrier 1)
//       STOP 3, h2o additions in order
//     saturation excess .. balance
//   at every exit of the year loop: front_done, as above.
// Each interval's words: the HS_* rows the main wave writes (wa before barrier
// 1, the rest before barrier 2) are read by the second wave only between
// barriers 2 and 3; those the second wave writes there are read by the main
// wave only between barrier 3 and the next barrier 1.  The chain reads the
// block's parameter fields and the geometry table besides, which nobody
// writes during the year.
// Why still no wave waits at a barrier its partner does not reach:
//  - The main wave's sequence is (barrier 1, 2, 3) per substep, then one
//    barrier 1 with go = 1; the second wave's is barrier 1, then (barrier 2,
//    3, 1) for as long as go = 0.  Neither count depends on jwt: the second
//    wave's chain call returns at once for jwt = L and it goes to barrier 3,
//    and the main wave passes barrier 3 after its own chain.
//  - The main wave's returns between barriers 2 and 3 are the sweep's STOPs 1
//    and 2 (and, formally, its own chain's STOP 3, never reached with jwt = L):
//    each passes barrier 3 on its way out (STOP_RET) and carries its code to
//    cell_year_pair, which then passes front_done.  The second wave may have
//    raised STOP 3 in the same substep: the main wave never reads those rows.
//  - The second wave's STOP 3 does not end its loop: it posts the code and its
//    value and goes to barrier 3; the main wave returns it after barrier 3.
//  - H9G_ERR_NOSNAP_K and the exact re-run (ROLE_ALL, no barrier) stay behind
//    hydrology_pair's return, after barrier 3.  The second wave's flag for the
//    re-run (a third layer visit, a subnormal quotient) travels in HS_FLAG.
template <int L, class SP, class CS>
H9K_HD void front_post(const SP &sp, const CS &cs, const St<L> &s) {
#pragma unroll
  for (int t = 0; t < L / 2; t++) cs.set_ho(CS::HO_SMP + 2 * t + sp.h, sel(sp.h, s.smp[2 * t + 1], s.smp[2 * t + 2]));
  cs.set_ho(CS::HO_H2O1, s.h2o[1]);
  cs.set_ho(CS::HO_ZWT, s.zwt);
  cs.set_ho(CS::HO_GO, zero);
  if constexpr (CS::kSide) cs.set_ho(CS::HS_WA, s.wa);
}
template <class CS>
H9K_HD void front_done(const CS &cs) {
  cs.set_ho(CS::HO_GO, one);
  cs.wg_sync();
}
// The front wave's year: lanes 0 and 1 as the canopy and soil halves, as in the
// main wave; no state, no stores but FrontRes.  pr: p0 its wait at barrier 1,
// p1 the front.
template <int L, class G, class SP, class CS, class PR = NoProf>
H9K_HD void front_year_pair(const G &g, CS cs, const SP &sp, const h9m::Tabs &T, PR &&pr = PR()) {
  if (sp.spare) return;
  St<L> s{};
  float rnf_sum = zero, errval = zero;
  for (;;) {
    cs.wg_sync();                                      // barrier 1
    cs.launder();
    if (lane0_get(cs.ho(CS::HO_GO)) != zero) break;
    pr.mark(0);
#pragma unroll
    for (int i = 1; i <= L; i++) s.smp[i] = cs.ho(CS::HO_SMP + i - 1);
    s.h2o[1] = cs.ho(CS::HO_H2O1);
    s.zwt = cs.ho(CS::HO_ZWT);
    MathFast mf{T, false};
    FrontRes fr;
    hydrology_pair<L, G, MathFast, SP, CS, PR, ROLE_FRONT>(g, cs, sp, s, rnf_sum, errval, mf, pr, &fr);
    pr.mark(1);
    cs.set_ho(CS::HO_SURF, fr.qflx_surf);
    cs.set_ho(CS::HO_TRAN, fr.tran);
    cs.set_ho(CS::HO_EVG, fr.evg);
    cs.set_ho(CS::HO_INFL, fr.qflx_infl);
    cs.wg_sync();                                      // barrier 2
    if constexpr (CS::kSide) {
      // the water-table chain of a substep that starts with the water table in
      // the column (the call returns at once for one that starts below it);
      // pr: p5, p6 the chain, p7 the wait at barrier 3
      cs.launder();
      s.wa = cs.ho(CS::HS_WA);
      cs.set_ho(CS::HS_I0, zero);
      cs.set_ho(CS::HS_I1, zero);
      MathFast mc{T, false};
      const int code = hydrology_pair<L, G, MathFast, SP, CS, PR, ROLE_CHAIN>(g, cs, sp, s, rnf_sum, errval, mc, pr);
      cs.set_ho(CS::HS_ZWT, s.zwt);
      cs.set_ho(CS::HS_WAO, s.wa);
      cs.set_ho(CS::HS_FLAG, mc.special ? one : zero);
      cs.set_ho(CS::HS_CODE, (float)code);
      cs.set_ho(CS::HS_ERRV, errval);
      cs.wg_sync();                                    // barrier 3
      pr.mark(7);
    }
  }
}

// One calendar year for one cell (HYBRID9.f90:150-290), as cell_year.
// Park = keep the plant state in the store over the substeps (register
// relief for the 168-VGPR pair kernel).  MO: NoMonths or Months.  The ET
// kernels: PR = EvapProf (the year's evaporation sum, from zero) and
// MO = MonthsEt; row evap is then that sum, divided like row rnf, and the day
// snapshot carries it (SV_EVAP).  With any other PR row evap is the
// reference's +0 and none of those statements exists.
template <int L, class G, class SP, class CS, bool Park = true, class PR = NoProf, class MO = NoMonths>
H9K_HD int cell_year_pair(const G &g, CS cs, const SP &sp, St<L> &s, const gbl_float *forc, size_t fday,
                          size_t fvar, int nt, int nisurf, int grow_on, gbl_float *acc, size_t astride,
                          int &eday, int &estep, float &errval, const h9m::Tabs &T, int raw = 0,
                          PR &&pr = PR(), MO mo = MO()) {
  enum { A_NPP = 0, A_PM, A_RNF, A_EVAP, A_TAS, A_RLDS, A_RSDS, A_HUSS, A_PS, A_PR, A_RHS,
         A_THETA, A_H2O = 11 + L };
  gbl_float *A = acc;
  const size_t as = astride;
  float rnf_sum = zero;
  // spare lanes (Split2) run only the substeps' per-layer phases: everything
  // here that stores is behind act()
  const bool act = sp.act();
  if (act) {
#pragma unroll
    for (int k = 0; k < 12 + L; k++) A[k * as] = zero;
  }
  // plant state parked in the store over the substeps (read by day_consts
  // and GROW only, once a day)
  auto park = [&]() __attribute__((always_inline)) {
    if constexpr (Park) {
      if (!act) return;
      cs.set_sc(PS_LAI, s.LAI);
      cs.set_sc(PS_LAIL, s.LAI_litter);
      cs.set_sc(PS_PM, s.pm);
      cs.set_sc(PS_PFM, s.pfm);
      cs.set_sc(PS_PLEN, s.plen);
      cs.set_sc(PS_RDEPTH, s.rdepth);
    }
  };
  park();
  float npp = zero;
  int code = 0;
  MathExact me{T};
  s.naq = 0;
  for (int day = 0; day < nt; day++) {
    cs.day_start(day);
    H9G_BR(BR_DAY);
#if defined(H9G_DUMP_AQ) && defined(__HIP_DEVICE_COMPILE__)
    if (act && h9g_aq_bits && s.zwt > g.zim(L)) {   // spare lanes hold a mirrored cell's stale zwt
      const size_t c = (size_t)((const float *)acc - h9g_aq_base);
      atomicOr(&h9g_aq_bits[c * 12 + day / 32], 1u << (day & 31));
    }
#endif
    cs.launder();
    opaque(A);
    const gbl_float *f = forc + (size_t)day * fday;
    opaque(f);
    if (act) {
      float fv[7];             // tas rlds rsds huss ps pr rhs
#pragma unroll
      for (int k = 0; k < 7; k++) fv[k] = ld_stream(f + k * fvar);
      const Day d = make_day(fv[0], fv[1], fv[2], fv[3], fv[4], fv[5], fv[6]);   // :168-184
      if constexpr (Park)
        day_consts(d, cs.sc(PS_LAI), cs.sc(PS_LAIL), cs, me);
      else
        day_consts(d, s.LAI, s.LAI_litter, cs, me);
      // :235-241, the forcing's running sums: they depend on the forcing
      // only, so they are added here, once the day's forcing is loaded, and
      // the forcing is read once a day (the reference adds them after the
      // substeps: the same values in the same order; a cell that STOPs has
      // NaN annual means either way)
      float a7[7];
#pragma unroll
      for (int k = 0; k < 7; k++) a7[k] = A[(A_TAS + k) * as];
#pragma unroll
      for (int k = 0; k < 7; k++) A[(A_TAS + k) * as] = a7[k] + fv[k];
    }
    bool snapped = false;
    for (int ns = 0; ns < nisurf; ns++) {                            // :193-211
      // the day snapshot, taken before the first substep of the day whose
      // water table is in the column (jwt < L): only such a substep visits
      // layers (:923-1118), so only it can need the exact re-run
      const bool in_column = s.zwt <= g.zim(L);
      s.naq += in_column ? 0 : 1;
      if (act && !snapped && in_column) {
        H9G_BR(BR_SNAP);
        save_day<L>(sp, cs, s, rnf_sum, ns);
        if constexpr (kEvap<PR>) cs.sv_set_sc(SV_EVAP, pr.sum);
        snapped = true;
      }
      if constexpr (CS::kFront) {            // the substep's state to the front wave (front_year_pair)
        if (act) front_post<L>(sp, cs, s);
        cs.wg_sync();                        // barrier 1
      }
      code = substep_pair<L, G, SP, CS>(g, cs, sp, s, rnf_sum, errval, T, pr, ns, snapped);
      if constexpr (CS::kFront) code = lane0_geti(code);   // the helper lanes leave with the pair
      if (code) { eday = day; estep = ns; break; }
    }
    cs.launder();
    if constexpr (Park) {
      s.LAI = cs.sc(PS_LAI);
      s.LAI_litter = cs.sc(PS_LAIL);
      s.pm = cs.sc(PS_PM);
      s.pfm = cs.sc(PS_PFM);
      s.plen = cs.sc(PS_PLEN);
      s.rdepth = cs.sc(PS_RDEPTH);
    }
    if (code) {
      if constexpr (CS::kFront) front_done(cs);
      if constexpr (kDays<MO>)
        if (act) mo.stop(day, nt, A);
      return code;
    }
    if (!act) continue;
    opaque(A);
    if (grow_on) {
      opaque(f);               // tas again (not kept live over the substeps)
      grow_day<L, G, MathExact>(g, ld_stream(f), s, cs, npp, me);       // :217
      park();
    }
    // :242-254.  All running sums are loaded before any is stored, so the
    // loads issue back to back (the compiler cannot prove the strided
    // fields distinct)
    auto later = [](int k) { return k != A_RNF && k != A_EVAP && (k < A_TAS || k > A_RHS); };
    float a[12 + L];
#pragma unroll
    for (int k = 0; k < 12 + L; k++)
      if (later(k)) a[k] = A[k * as];
    a[A_PM] = a[A_PM] + s.pm;
    a[A_NPP] = a[A_NPP] + npp;
    float h2o_sum = a[A_H2O];
#pragma unroll
    for (int i = 1; i <= L; i++) {
      const float theta = MAXF(s.h2o[i], 1.0E-6f) / g.thk(i);       // HYDROLOGY.f90:1233
      a[A_THETA + i - 1] = a[A_THETA + i - 1] + theta;
      h2o_sum = h2o_sum + s.h2o[i];
    }
    a[A_H2O] = h2o_sum;
#pragma unroll
    for (int k = 0; k < 12 + L; k++)
      if (later(k)) A[k * as] = a[k];
    if constexpr (kDays<MO>)
      mo.template day_end<L>(day, nt, A, as, rnf_sum, pr.sum, s, MAXF(s.h2o[1], 1.0E-6f) / g.thk(1));
    else if constexpr (kEvap<PR>)
      mo.template day_end<L>(day, nt, A, as, rnf_sum, pr.sum);
    else
      mo.template day_end<L>(day, nt, A, as, rnf_sum);
  }
  if constexpr (CS::kFront) front_done(cs);   // the year's end: the front wave leaves
  // :263-290
  if (!act) return 0;
  opaque(A);
  if (raw) {                   // the cell order's day-1 probe: the running sums themselves
    A[A_RNF * as] = rnf_sum;
    if constexpr (kEvap<PR>) A[A_EVAP * as] = pr.sum;
    return 0;
  }
  A[A_PM * as] = A[A_PM * as] / (float)nt;
  A[A_RNF * as] = rnf_sum / (float)(nt * nisurf);
  if constexpr (kEvap<PR>)
    A[A_EVAP * as] = pr.sum / (float)(nt * nisurf);
  else
    A[A_EVAP * as] = zero / (float)(nt * nisurf);
#pragma unroll
  for (int k = A_TAS; k <= A_H2O; k++) A[k * as] = A[k * as] / (float)nt;
  return 0;
}

// LCLIM single-site days for one cell (HYBRID9.f90:353-478): per-substep
// forcing, the day-of-year LAI schedule, no GROW.  Every substep runs the
// exact path (MathExact, one lane for all layers): this is the one-site
// evaluation tool, not the grid path.  Layouts (n = cells, [row][cell]):
//   sub   (nday*nisurf, 5, n): tak (degC), rh, Rnet, PAR, ppt (mm per substep)  :428-439
//   daily (nday, 2, n): huss, ps                                                 :377-378
//   lai   (nday, 3, n): LAI, a, b -- LAI = LAI, LAI_litter = LAI_litter + a - b,
//         NaN = no change (the schedule of :380-417)
//   out   (nday, 11, n): evap_day, evap_grnd_day, theta(1:4), theta_ma(1), LAI,
//         LAI_litter, w_i, fT                                                    :464-469
// w_i and fT are GROW's and GROW never runs here: they are 0.
template <int L, class G, class CS>
H9K_HD int cell_site(const G &g, CS cs, St<L> &s, float h2o_ma1, const float *sub, const float *daily,
                     const float *lai, float *out, size_t n, int nday, int nisurf, int &eday, int &estep,
                     float &errval, const h9m::Tabs &T) {
  MathExact me{T};
  const SplitAll sp;
  FluxProf fx{zero, zero};
  float rnf_sum = zero;
  const float dt = g.dt();
  const float theta_ma1 = h2o_ma1 / g.thk(1);                         // HYDROLOGY.f90:149
  for (int day = 0; day < nday; day++) {
    const float *l = lai + (size_t)day * 3 * n;
    if (l[0] == l[0]) s.LAI = l[0];
    if (l[n] == l[n]) s.LAI_litter = s.LAI_litter + l[n] - l[2 * n];
    const float *dd = daily + (size_t)day * 2 * n;
    float evap_day = zero, evap_grnd_day = zero;
    for (int ns = 0; ns < nisurf; ns++) {
      const float *v = sub + ((size_t)day * nisurf + ns) * 5 * n;
      Day d;
      d.tak = v[0] + tf;
      d.rh = v[n];
      d.Rnet = v[2 * n];
      d.PAR = v[3 * n];
      d.forc_rain = v[4 * n] / dt;
      d.lamb = ((2503.0f - 2.386f * (d.tak - tf))) * 1.0E3f;        // :445
      d.huss = dd[0];
      d.ps = dd[n];
      day_consts(d, s.LAI, s.LAI_litter, cs, me);
      const int code = hydrology_pair<L, G, MathExact, SplitAll, CS, FluxProf>(g, cs, sp, s, rnf_sum, errval,
                                                                            me, fx);
      if (code) { eday = day; estep = ns; return code; }
      evap_day = evap_day + (fx.evg + fx.tran) * dt;                  // :457-458
      evap_grnd_day = evap_grnd_day + fx.evg * dt;
    }
    float *o = out + (size_t)day * 11 * n;
    o[0] = evap_day;
    o[n] = evap_grnd_day;
#pragma unroll
    for (int i = 1; i <= 4; i++) o[(1 + i) * n] = MAXF(s.h2o[i], 1.0E-6f) / g.thk(i);   // :1233
    o[6 * n] = theta_ma1;
    o[7 * n] = s.LAI;
    o[8 * n] = s.LAI_litter;
    o[9 * n] = zero;
    o[10 * n] = zero;
  }
  return 0;
}

// The daily diagnostics line of the reference's INTERACTIVE mode
// (HYBRID9.f90:221-229) for one grid cell: a shadow run of the cell's years
// from a copy of its start state, beside the year kernels and not inside
// them.  Every kernel computes the reference's bits, so this run follows the
// trajectory the year kernel takes.  As cell_site it runs every substep on
// the exact path with one lane for all layers (the fast path's exact re-run
// restores state from the day snapshot and does not carry the fluxes), but
// on the PGF day forcing and with GROW, as cell_year_pair: make_day,
// day_consts, nisurf substeps, grow_day when grow_on.  It reads only:
// no state, annual mean or STOP record is stored.
//   yrs   the consecutive calendar years: forcing base (7 variables fvar
//         apart, days fday apart, this cell at `cell`) and days
//   out   (total days, 11, n): evap_day, evap_grnd_day, theta(1:4),
//         theta_ma(1), LAI, LAI_litter (after GROW), w_i, fT (as GROW computed
//         them that day, GROW.f90:55-71; 0 when grow_on = 0)             :223-228
// A cell that reaches a reference STOP has NaN from that day on (the
// reference ends before writing the day's line); returns its code.
struct FocusYear {
  const float *forc;
  int nt;
};

template <int L, class G, class CS>
H9K_HD int cell_focus(const G &g, CS cs, St<L> &s, float h2o_ma1, const FocusYear *yrs, int nyears, size_t cell,
                      size_t fday, size_t fvar, int nisurf, int grow_on, float *out, size_t n,
                      const h9m::Tabs &T) {
  MathExact me{T};
  const SplitAll sp;
  FluxProf fx{zero, zero};
  float rnf_sum = zero, errval = zero, npp = zero;
  const float dt = g.dt();
  const float theta_ma1 = h2o_ma1 / g.thk(1);                         // HYDROLOGY.f90:149
  const float nan = __builtin_nanf("");
  gbl_float *o = (gbl_float *)out;
  int code = 0;
  for (int y = 0; y < nyears; y++) {
    const gbl_float *forc = (const gbl_float *)yrs[y].forc + cell;
    const int nt = yrs[y].nt;
    for (int day = 0; day < nt; day++, o += 11 * n) {
      float evap_day = zero, evap_grnd_day = zero, w_i = zero, fT = zero;
      if (!code) {
        const gbl_float *f = forc + (size_t)day * fday;
        float fv[7];             // tas rlds rsds huss ps pr rhs
#pragma unroll
        for (int k = 0; k < 7; k++) fv[k] = ld_stream(f + k * fvar);
        const Day d = make_day(fv[0], fv[1], fv[2], fv[3], fv[4], fv[5], fv[6]);   // :168-184
        day_consts(d, s.LAI, s.LAI_litter, cs, me);
        for (int ns = 0; ns < nisurf && !code; ns++) {                  // :193-211
          code = hydrology_pair<L, G, MathExact, SplitAll, CS, FluxProf>(g, cs, sp, s, rnf_sum, errval, me, fx);
          evap_day = evap_day + (fx.evg + fx.tran) * dt;                // :207-209
          evap_grnd_day = evap_grnd_day + fx.evg * dt;
        }
        if (!code && grow_on) {
          grow_drivers<L>(fv[0], s, cs, w_i, fT);
          grow_day<L, G, MathExact>(g, fv[0], s, cs, npp, me);          // :217
        }
      }
      if (code) {
#pragma unroll
        for (int r = 0; r < 11; r++) o[r * n] = nan;
        continue;
      }
      o[0] = evap_day;
      o[n] = evap_grnd_day;
#pragma unroll
      for (int i = 1; i <= 4; i++) o[(1 + i) * n] = MAXF(s.h2o[i], 1.0E-6f) / g.thk(i);   // :1233
      o[6 * n] = theta_ma1;
      o[7 * n] = s.LAI;
      o[8 * n] = s.LAI_litter;
      o[9 * n] = w_i;
      o[10 * n] = fT;
    }
  }
  return code;
}

}  // namespace h9k
