// h9g.hip -- MI355X (gfx950) implementation of the HYBRID9 per-cell
// time-stepping hot path behind the C-ABI of include/h9g.h.
//
// Kernel design:
//   * h9g_pair_kernel<L, G> (default): one launch runs one calendar year --
//     all days x NISURF substeps of HYDROLOGY plus the daily GROW -- for
//     every cell, time innermost as in the reference.  Two lanes per soil
//     column: the per-layer phases (equilibrium profile, conductivity and
//     matric potential; ~40 of the ~46 glibc-exact powf of a substep) are
//     split over the pair and exchanged by DPP, the rest runs in both
//     lanes.  22 columns per wave, 4 waves per workgroup: 3 waves on every
//     SIMD at 0.5 deg (767 workgroups, 768 slots).  The column's water
//     state lives in VGPRs, its read-mostly data (soil parameters and
//     their invariants, rootr, the day's constants) in the pair's two
//     columns of an LDS block, the day snapshot of the exact re-run in an
//     L2-resident global block.  HBM traffic per
//     cell-day is the 7 forcing values (coalesced, cell-fastest) plus the
//     annual sums (L2-resident): the SHARED-state contract of each substep
//     (376 B at L=8) never leaves the CU.
//   * h9g_solo_kernel<L, G> (at L = 10 chosen by column count, alone or
//     followed by the pair kernel on the remainder, l10_kind;
//     H9G_KERNEL=solo|pair|mixed overrides): one lane per column, the same
//     code with one lane doing every layer.
//   * glibc-exact expf/powf (h9_math.h) read their 32+16-entry tables from
//     LDS (per-lane indices, no scalar-cache serialisation).
//   * no MFMA: nothing here is GEMM-shaped.
//   * h9g_diag_kernel: deterministic FP64 reduction of global diagnostics
//     (the payload of the cross-GPU all-reduce).
// The year kernels, the table of their launch shapes and their launch are
// h9g_year.h, instantiated in h9g_plain.hip, h9g_mon.hip and h9g_et.hip; the
// other geometry-templated kernels are h9g_cols.hip.  This file is the host
// runtime's core (h9g_ctx.h): the context's lifetime and configuration,
// parameters, state, forcing and prefetch, the year launch with its
// permutation and diagnostics kernels, h9g_run_year, the daily diagnostics,
// the recorded outputs (RecStream: months and day records, one code path:
// rec_begin, rec_get), statistics and errors.  The ordered mode is h9g_ord.hip, spin-up
// h9g_spin.hip; the soil build, synthetic inputs and self-tests are
// h9g_aux.hip.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "h9g_ctx.h"
#include "h9g_io.h"

static_assert(H9G_ERR_NOSNAP_K == H9G_ERR_NOSNAP, "kernel and ABI error codes");
static_assert(H9G_NDAILY == DAILY_ROWS, "the daily line of the ABI and of h9g_rows.h");

// The year's forcing in the year kernel's slot order (round 4, VERDICT r03
// #5): dst[v][d][s] = src[v][d][perm[s]].  With the cells re-ordered each
// year (h9g_sort_kernel), a wave's daily forcing loads by cell id scattered
// over its XCD's range, so the non-temporal loads of neighbouring lanes hit
// different lines: 4.45 GB fetched per config-2 launch for 0.69 GB of
// forcing (pmc_r03i.json).  One gather per year makes every wave's daily
// loads contiguous again.  XCD-aware like the year kernel: the launch range
// [c0, cend) is cut into the year kernel's workgroups of cpb slots, dealt to
// the XCDs as xcd_vwg deals them, and block L (XCD L % 8) copies PF_ROWS
// rows of one workgroup of XCD L % 8 -- so it reads only cells of its own
// XCD's range, which the sort never leaves.
#define H9G_PF_ROWS 32
// Source rows have stride n (a forcing slot, variables fvar apart); the
// slot-ordered copy has stride ds (variables dvar apart).
__global__ void __launch_bounds__(256) h9g_perm_forcing_kernel(int c0, int cend, int cpb, int nt, int n, size_t fvar,
                                                               size_t ds, size_t dvar, const int *__restrict__ perm,
                                                               const float *__restrict__ src, float *__restrict__ dst) {
  const unsigned nb = (unsigned)((cend - c0 + cpb - 1) / cpb), x = blockIdx.x % H9G_NXCD, j = blockIdx.x / H9G_NXCD;
  const unsigned q = nb / H9G_NXCD, r = nb % H9G_NXCD, cnt = q + (x < r ? 1u : 0u);
  const unsigned rows = 7u * (unsigned)nt, rgroups = (rows + H9G_PF_ROWS - 1) / H9G_PF_ROWS;
  if (cnt == 0 || j >= cnt * rgroups) return;
  const unsigned v = x * q + (x < r ? x : r) + j % cnt, r0 = (j / cnt) * H9G_PF_ROWS;
  for (unsigned t = threadIdx.x; t < (unsigned)cpb * H9G_PF_ROWS; t += blockDim.x) {
    const int s = c0 + (int)(v * (unsigned)cpb + t % (unsigned)cpb);
    const unsigned row = r0 + t / (unsigned)cpb;
    if (s >= cend || row >= rows) continue;
    const size_t v = row / (unsigned)nt, d = row % (unsigned)nt;
    dst[v * dvar + d * ds + s] = src[v * fvar + d * (size_t)n + perm[s]];
  }
}
static unsigned perm_forcing_blocks(int c0, int cend, int cpb, int nt) {
  const unsigned nb = (unsigned)((cend - c0 + cpb - 1) / cpb);
  const unsigned cmax = nb / H9G_NXCD + (nb % H9G_NXCD ? 1u : 0u);
  return H9G_NXCD * cmax * ((7u * (unsigned)nt + H9G_PF_ROWS - 1) / H9G_PF_ROWS);
}

// The annual sums of a sorted year kernel (slot order, rows of stride ss)
// back to cell order (rows of stride n): the m slots from s0 of the launch.
__global__ void __launch_bounds__(256) h9g_unperm_annual_kernel(int m, int n, int rows, int s0, size_t ss,
                                                                const int *__restrict__ perm,
                                                                const float *__restrict__ src, float *__restrict__ dst) {
  const int s = s0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= s0 + m) return;
  const int c = perm[s];
  for (int r = blockIdx.y; r < rows; r += gridDim.y) dst[(size_t)r * n + c] = src[(size_t)r * ss + s];
}

// dst[r][j] = st[r][sel[j]] for every state row; the smp rows from `guess`
// (L rows of n) instead where given (the cell order: the smp a cell's first
// substep of the decade reads is its predecessor's, h9g_chain_kernel).
__global__ void __launch_bounds__(256) h9g_focus_gather_kernel(int nsel, int n, int srows, int L,
                                                               const int *__restrict__ sel,
                                                               const float *__restrict__ st,
                                                               const float *__restrict__ guess,
                                                               float *__restrict__ dst) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nsel) return;
  const int c = sel[j];
  H9K_COPY_CELL(dst, nsel, j, st, n, c, srows);
  if (guess)
    for (int i = 0; i < L; i++) dst[(size_t)(smp_row(L, 0) + i) * nsel + j] = guess[(size_t)i * n + c];
}

// deterministic FP64 diagnostics: one block, fixed strided order + tree
__global__ void __launch_bounds__(1024) h9g_diag_kernel(int ncell, int L, const float *__restrict__ annual,
                                                        const float *__restrict__ st,
                                                        const int *__restrict__ err, double *__restrict__ out) {
  __shared__ double red[1024];
  double acc[H9G_NDIAG];
  for (int k = 0; k < H9G_NDIAG; k++) acc[k] = 0.0;
  const size_t n = ncell;
  const size_t o8 = (size_t)scalar_row(L, 0) * n;
  for (int c = threadIdx.x; c < ncell; c += blockDim.x) {
    const float rnf = annual[2 * n + c];
    if (err[c] != 0) { acc[11] += 1.0; continue; }
    if (rnf != rnf) continue;                    // non-soil cell
    acc[0] += 1.0;
    acc[1] += (double)rnf;
    acc[2] += (double)annual[(size_t)(11 + L) * n + c];
    acc[3] += (double)st[o8 + SC_ZWT * n + c];
    acc[4] += (double)st[o8 + SC_WA * n + c];
    acc[5] += (double)annual[0 * n + c];
    acc[6] += (double)annual[1 * n + c];
    acc[7] += (double)st[o8 + SC_LAI * n + c];
    acc[8] += (double)annual[11 * n + c];
    acc[9] += (double)annual[4 * n + c];
    acc[10] += (double)annual[9 * n + c];
  }
  for (int k = 0; k < H9G_NDIAG; k++) {
    red[threadIdx.x] = acc[k];
    __syncthreads();
    for (int w = blockDim.x / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[k] = red[0];
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// What h9g_kernel_name reports for a year of `cells` cells on `kind`:
// "h9g_pair_kernel<8,GeoC<8,48>>"; the mixed kind: its solo kernel + its pair
// kernel.  (hybrid9_amd kind_id reads the prefix.)
static std::string year_kernel_name(const h9g_ctx *ctx, int kind, size_t cells) {
  const GeoKind gk = geo_kind(ctx->cfg);
  const std::string L = std::to_string(ctx->L);
  const std::string targs = "<" + L + "," + (gk == GEO_R ? "GeoR" : "GeoC<" + L + "," + std::to_string((int)gk) + ">") + ">";
  auto name = [&](int k) {
    const ShapeInfo si = shape_info(year_shape(k, cells));
    return (ctx->rec[REC_DAY].on ? si.day_name : ctx->evap ? si.et_name : si.name) + targs;
  };
  return kind == K_MIXED ? name(K_SOLO) + "+" + name(K_PAIR) : name(kind);
}

extern "C" {

int h9g_abi_version(void) { return H9G_ABI_VERSION; }

int h9g_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int h9g_state_size(int nlayers) { return state_rows(nlayers); }

void h9g_destroy(h9g_ctx *ctx) {
  if (!ctx) return;
  for (auto &t : ctx->prefetch)
    if (t.joinable()) t.join();
  (void)hipSetDevice(ctx->device);
  if (ctx->sc) hipStreamSynchronize(ctx->sc);
  if (ctx->sx) hipStreamSynchronize(ctx->sx);
  (void)hipFree(ctx->d_par);
  (void)hipFree(ctx->d_st);
  (void)hipFree(ctx->d_forc);
  (void)hipFree(ctx->d_ann);
  (void)hipFree(ctx->d_err);
  (void)hipFree(ctx->d_sv);
  (void)hipFree(ctx->d_errflag);
  (void)hipFree(ctx->d_diag);
  (void)hipFree(ctx->d_gid);
  (void)hipFree(ctx->d_lat);
  (void)hipFree(ctx->d_stamps);
  (void)hipFree(ctx->d_slow);
  (void)hipFree(ctx->d_perm);
  (void)hipFree(ctx->d_perm2);
  (void)hipFree(ctx->d_forc_s);
  (void)hipFree(ctx->d_ann_s);
  for (RecStream &s : ctx->rec)
    for (float *p : {s.d_year, s.d_year_s, s.d_ret}) (void)hipFree(p);
  (void)hipFree(ctx->d_hist);
  (void)hipFree(ctx->d_aqbits);
  (void)hipFree(ctx->d_pace);
  (void)hipFree(ctx->d_dsel);
  (void)hipFree(ctx->d_dst);
  (void)hipFree(ctx->d_daily);
  (void)hipFree(ctx->d_fyrs);
  ord_free(ctx);
  spin_free(ctx);
  stat_free(ctx);
  quant_free(ctx);
  for (auto e : ctx->ev_copied) hipEventDestroy(e);
  for (auto e : ctx->ev_consumed) hipEventDestroy(e);
  for (int i = 0; i < NEVT; i++) {
    (void)hipEventDestroy(ctx->ev0[i]);
    (void)hipEventDestroy(ctx->ev1[i]);
  }
  if (ctx->ev_ext) (void)hipEventDestroy(ctx->ev_ext);
  if (ctx->ev_diag) (void)hipEventDestroy(ctx->ev_diag);
  for (auto p : ctx->h_pin) (void)hipHostFree(p);
  if (ctx->sc) hipStreamDestroy(ctx->sc);
  if (ctx->sx) hipStreamDestroy(ctx->sx);
  delete ctx;
}

// Kernel for L = 10 (pair, solo or both).  They are bit-identical
// and differ in how n columns quantise into rounds of resident waves: the
// solo kernel (1-wave blocks, 1 wave/SIMD) packs 64 columns per wave, the
// pair kernel (88-column blocks, 3 waves/SIMD since round 3, pair_resident)
// 22; K_MIXED runs the whole solo rounds and the pair kernel on the rest.
// Round 3 measured every strong-scaling shard of the config-5 grid
// (tools/l10_shards.py, profiles/r03e_l10_shards.txt, ms per year, pair /
// solo / mixed): 270,000 cells 537.7 / 618.6 / 538.1; 135,000 274.5 / 373.2 /
// 274.4; 67,500 130.1 / 246.5 / 130.4; 33,750 107.9 / 134.1 / 108.1.  The
// pair kernel is within noise of the best everywhere, so it is the choice;
// round 2's rounds model picked solo at 33,750 cells (24% slower there).
// Solo and mixed stay selectable (H9G_KERNEL) and are tested.  *n_solo:
// the whole solo rounds (K_MIXED only).
// Round 4 adds the pair kernel built for 2 waves per SIMD (K_PAIR2, 256
// VGPRs: no spills, every reciprocal): where the shard's pair workgroups fit
// one round of 2 per CU it is the faster one (33,750 cells: 98.1 vs 100.9 ms
// per year), and wherever they do not it needs an extra round (270,000 cells:
// 601.5 vs 505.8 ms), profiles/r04*_l10_shards.txt.
static Kind l10_kind(size_t n, int ncu, size_t *n_solo) {
  const size_t solo_round = (size_t)4 * ncu * H9G_YBLOCK;
  *n_solo = (n / solo_round) * solo_round;
  return shape_blocks(S_PAIR2, n) <= (size_t)shape_info(S_PAIR2).waves * ncu ? K_PAIR2 : K_PAIR;
}

// Device bytes a context of this configuration allocates: h9g_create's
// arrays plus what the first h9g_run_year / h9g_soil_layer allocate lazily
// (the pair kernel's per-workgroup day-snapshot blocks, the pacing rows, the
// soil build's slow-cell flags).
// Not counted: the daily diagnostics of a selection (h9g_set_daily), whose
// size depends on the call -- years x max_days x 11 x nsel floats for the
// lines, allocated by the run that records them and kept until the context is
// destroyed, plus the nsel gathered state rows (H9G_ENOMEM if they do not fit).
// Device bytes of the ordered mode's buffers for decades of up to ny years
// (h9g_config_bytes counts them with ny = 10).
static size_t ord_bytes(size_t n, size_t L, size_t ny) {
  const size_t srows = state_rows((int)L), rows = annual_rows((int)L);
  return 2 * (sizeof(float) * (srows + L + ny * (rows + srows)) * n + sizeof(int) * (STOP_ROWS + STOP_ROWS * ny + 1) * n +
              sizeof(int) * 5 * (n + 1)) +
         sizeof(float) * srows * n + sizeof(int) * (STOP_ROWS * n + n + 1) +
         // the day-1 probe (OrdBufs): old inputs, two runs' state, sums and STOP rows, list, flags
         sizeof(float) * (L + 2 * srows + 2 * rows) * n + sizeof(int) * (2 * STOP_ROWS * n + 2 * (n + 1));
}

size_t h9g_config_bytes(const h9g_config *cfg) {
  if (!cfg || cfg->ncell <= 0 || cfg->nlayers < 1 || cfg->max_days < 1 || cfg->nslots < 1) return 0;
  const size_t n = (size_t)cfg->ncell, L = (size_t)cfg->nlayers;
  const size_t ios = 2 * round_up(n, H9G_PCPW) + 64;
  // the largest launch's day-snapshot blocks: the 11-column kernel's over
  // every cell, or the one-column kernel's over H9G_PAIR1_MAX listed cells
  // (a workgroup per cell up to H9G_PAIR1_FRONT_MAX)
  const size_t blocks = std::max(shape_blocks(S_PAIR11, ios),
                                 std::max((size_t)1024 / H9G_PWAVES, (size_t)H9G_PAIR1_FRONT_MAX));
  // + the slot-ordered copies of a forcing slot and of the annual sums
  // (h9g_run_year, allocated on first use), the ordered mode's decade
  // buffers (h9g_run_ordered, decades of up to 10 years)
  const size_t prows = par_rows(cfg->nlayers), srows = state_rows(cfg->nlayers), arows = annual_rows(cfg->nlayers);
  return sizeof(float) * (prows + srows + 7 * (size_t)cfg->max_days * (size_t)cfg->nslots + arows + 1) * n +
         sizeof(float) * (7 * (size_t)cfg->max_days + arows) * ios + sizeof(int) * 2 * ios +
         sizeof(int) * (STOP_ROWS + 2) * n + sizeof(int64_t) * n + sizeof(double) * H9G_NDIAG + sizeof(int) +
         blocks * PairStore<8, H9G_PLANES>::GBLOCK + sizeof(unsigned) * 16 * (size_t)H9G_PACE_ROWS +
         ord_bytes(n, L, 10);
}

// Free HBM h9g_create leaves beyond h9g_config_bytes (HIP runtime, RCCL
// buffers, allocation granularity), so that a configuration that passes the
// check at create time does not fail later inside h9g_run_year.
#define H9G_HEADROOM ((size_t)256 << 20)

static thread_local char g_create_reason[256];

static int config_fail(char *reason, int len, const char *msg) {
  if (reason && len > 0) snprintf(reason, (size_t)len, "%s", msg);
  return H9G_EINVAL;
}

// Host-only validation of a configuration (no GPU needed): 0 or H9G_EINVAL
// with a readable reason.  The slot count is bounded by memory, which
// h9g_create checks against the device's free HBM.
int h9g_config_check(const h9g_config *cfg, char *reason, int reason_len) {
  if (reason && reason_len > 0) reason[0] = 0;
  if (!cfg) return config_fail(reason, reason_len, "cfg is NULL");
  if (cfg->ncell <= 0) return config_fail(reason, reason_len, "ncell must be > 0");
  if (!(cfg->nlayers == 8 || cfg->nlayers == 10))
    return config_fail(reason, reason_len, "nlayers must be 8 or 10");
  if (cfg->nisurf < 1) return config_fail(reason, reason_len, "nisurf must be >= 1");
  if (cfg->max_days < 366) return config_fail(reason, reason_len, "max_days must be >= 366");
  if (cfg->nslots < 1 || cfg->nslots > H9G_MAX_SLOTS)
    return config_fail(reason, reason_len, "nslots must be in [1, H9G_MAX_SLOTS]");
  if ((size_t)cfg->ncell * 7 * (size_t)cfg->max_days > (size_t)INT32_MAX * 4)
    return config_fail(reason, reason_len, "ncell * max_days too large for one slot");
  for (int i = 1; i <= cfg->nlayers + 1; i++)
    if (!(cfg->zi[i] > cfg->zi[i - 1])) return config_fail(reason, reason_len, "zi must increase strictly");
  return 0;
}

const char *h9g_create_error(void) { return g_create_reason; }

h9g_ctx *h9g_create(const h9g_config *cfg, int device) {
  g_create_reason[0] = 0;
  if (h9g_config_check(cfg, g_create_reason, sizeof g_create_reason)) return nullptr;
  if (hipSetDevice(device) != hipSuccess) {
    snprintf(g_create_reason, sizeof g_create_reason, "hipSetDevice(%d) failed: no gfx950 GPU visible?", device);
    return nullptr;
  }
  {
    size_t free_b = 0, total_b = 0;
    const size_t need = h9g_config_bytes(cfg);
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need + H9G_HEADROOM > free_b) {
      snprintf(g_create_reason, sizeof g_create_reason,
               "needs %.2f GB of device memory + %.2f GB headroom, %.2f GB free (reduce nslots=%d)", need / 1e9,
               H9G_HEADROOM / 1e9, free_b / 1e9, cfg->nslots);
      return nullptr;
    }
  }
  h9g_ctx *ctx = new h9g_ctx();
  ctx->cfg = *cfg;
  ctx->device = device;
  ctx->L = cfg->nlayers;
  ctx->n = (size_t)cfg->ncell;
  const size_t n = ctx->n;
  const int L = ctx->L;
  ctx->ios = 2 * round_up(n, H9G_PCPW) + 64;
  ctx->rec[REC_MON].year_rows = (size_t)H9G_NMONTHS * annual_rows(L);
  ctx->rec[REC_DAY].year_rows = (size_t)cfg->max_days * H9G_NDAYREC;
  ctx->rec[REC_DAY].day_rows = H9G_NDAYREC;
  bool ok = hipStreamCreateWithFlags(&ctx->sc, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithFlags(&ctx->sx, hipStreamNonBlocking) == hipSuccess &&
            hipMalloc(&ctx->d_par, sizeof(float) * par_rows(L) * n) == hipSuccess &&
            hipMalloc(&ctx->d_st, sizeof(float) * state_rows(L) * n) == hipSuccess &&
            hipMalloc(&ctx->d_forc, sizeof(float) * 7 * (size_t)cfg->max_days * n * cfg->nslots) == hipSuccess &&
            hipMalloc(&ctx->d_ann, sizeof(float) * annual_rows(L) * n) == hipSuccess &&
            hipMalloc(&ctx->d_err, sizeof(int) * STOP_ROWS * n) == hipSuccess &&
            hipMalloc(&ctx->d_errflag, sizeof(int)) == hipSuccess &&
            hipMalloc(&ctx->d_diag, sizeof(double) * H9G_NDIAG) == hipSuccess &&
            hipMalloc(&ctx->d_gid, sizeof(int64_t) * n) == hipSuccess &&
            hipMalloc(&ctx->d_lat, sizeof(float) * n) == hipSuccess &&
            hipMalloc(&ctx->d_perm, sizeof(int) * ctx->ios) == hipSuccess &&
            hipMalloc(&ctx->d_perm2, sizeof(int) * ctx->ios) == hipSuccess &&
            hipMalloc(&ctx->d_hist, sizeof(int) * n) == hipSuccess;
  if (ok) {
    ok = hipMemset(ctx->d_err, 0, sizeof(int) * STOP_ROWS * n) == hipSuccess &&
         hipMemset(ctx->d_errflag, 0, sizeof(int)) == hipSuccess &&
         hipMemset(ctx->d_diag, 0, sizeof(double) * H9G_NDIAG) == hipSuccess &&
         hipMemset(ctx->d_ann, 0xff, sizeof(float) * annual_rows(L) * n) == hipSuccess &&
         hipMemset(ctx->d_hist, 0xff, sizeof(int) * n) == hipSuccess;
  }
  ctx->slot_days.assign(cfg->nslots, 0);
  ctx->h_pin.assign(cfg->nslots, nullptr);
  ctx->prefetch.resize(cfg->nslots);
  ctx->prefetch_rc.assign(cfg->nslots, 0);
  ctx->ev_copied.resize(cfg->nslots);
  ctx->ev_consumed.resize(cfg->nslots);
  for (int s = 0; ok && s < cfg->nslots; s++)
    ok = hipEventCreateWithFlags(&ctx->ev_copied[s], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&ctx->ev_consumed[s], hipEventDisableTiming) == hipSuccess;
  for (int i = 0; ok && i < NEVT; i++)
    ok = hipEventCreate(&ctx->ev0[i]) == hipSuccess && hipEventCreate(&ctx->ev1[i]) == hipSuccess;
  if (ok)
    ok = hipEventCreateWithFlags(&ctx->ev_ext, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&ctx->ev_diag, hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    snprintf(g_create_reason, sizeof g_create_reason, "device allocation failed (ncell=%d, nslots=%d)",
             cfg->ncell, cfg->nslots);
    fprintf(stderr, "h9g_create: %s\n", g_create_reason);
    h9g_destroy(ctx);
    return nullptr;
  }
  // default: the pair kernel at L = 8; at L = 10 the kernel that needs less
  // time for this many columns (l10_kind)
  if (const char *se = getenv("H9G_SORT")) ctx->sort = atoi(se) != 0;
  if (const char *se = getenv("H9G_PRIO")) ctx->prio_mode = atoi(se);
  if (getenv("H9G_NO_PROBE")) ctx->ord_probe = 0;
  ctx->no_pair1 = getenv("H9G_NO_PAIR1") != nullptr;
  ctx->no_pair11 = getenv("H9G_NO_PAIR11") != nullptr;
  ctx->no_exclude = getenv("H9G_NO_EXCLUDE") != nullptr;
  ctx->no_ride = getenv("H9G_NO_RIDE") != nullptr;
  const char *kenv = getenv("H9G_KERNEL");
  int ncu = 256;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu < 1)
    ncu = 256;
  ctx->ncu = ncu;
  // The XCD-aware orders (xcd_vwg, h9g_sort_kernel, h9g_perm_forcing_kernel)
  // assume H9G_NXCD = 8 XCDs dealt round-robin, i.e. the MI355X in SPX mode
  // (256 CUs).  Results never depend on it (every mapping is a permutation);
  // only the per-XCD L2 locality does.  Say so once if the device differs
  // (a CPX partition has one XCD of 32 CUs).
  if (ncu != 32 * H9G_NXCD) {
    static bool said = false;
    if (!said) {
      fprintf(stderr, "h9g: device %d has %d CUs, not %d: XCD-aware cell orders assume %d XCDs (SPX); results are "
                      "unaffected, L2 locality may not hold\n", device, ncu, 32 * H9G_NXCD, H9G_NXCD);
      said = true;
    }
  }
  // H9G_KERNEL names a kind (pair2: L = 10 only); else the pair kernel at L = 8 and l10_kind's choice at L = 10
  Kind forced = K_NSTAT;
  for (int k = K_PAIR; kenv && k < K_PROBE; k++)
    if (strcmp(kenv, kind_info(k).env) == 0 && (k != K_PAIR2 || L == 10)) forced = (Kind)k;
  if (forced == K_MIXED) {
    // forced split (tests): H9G_SPLIT cells on the solo kernel, else the model's
    ctx->kind = K_MIXED;
    size_t ns = 0;
    (void)l10_kind(n, ncu, &ns);
    if (const char *sp = getenv("H9G_SPLIT")) ns = (size_t)strtoull(sp, nullptr, 10);
    ctx->n_solo = std::min(ns, n);
  } else if (forced != K_NSTAT)
    ctx->kind = forced;
  else if (L == 8)
    ctx->kind = K_PAIR;
  else
    ctx->kind = l10_kind(n, ncu, &ctx->n_solo);
  ctx->kname = year_kernel_name(ctx, ctx->kind, ctx->n);
  return ctx;
}

// (L, ncell) layer-fastest host arrays -> device rows
int h9g_set_params(h9g_ctx *ctx, const float *theta_s, const float *hksat, const float *bsw,
                   const float *psi_s, const float *fmax) {
  if (!ctx || !theta_s || !hksat || !bsw || !psi_s || !fmax) return H9G_EINVAL;
  const size_t n = ctx->n;
  const int L = ctx->L;
  std::vector<float> rows(par_rows(L) * n);
  const float *src[4] = {theta_s, hksat, bsw, psi_s};
  for (int k = 0; k < 4; k++)
    for (size_t c = 0; c < n; c++)
      for (int i = 0; i < L; i++) rows[(size_t)par_row(L, k, i) * n + c] = src[k][c * L + i];
  memcpy(&rows[(size_t)fmax_row(L) * n], fmax, sizeof(float) * n);
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(ctx->d_par, rows.data(), sizeof(float) * rows.size(), hipMemcpyHostToDevice, ctx->sc));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  ctx->params_set = 1;
  return 0;
}

// device rows -> (L, ncell) layer-fastest host arrays (h9g_set_params layout)
int h9g_get_params(h9g_ctx *ctx, float *theta_s, float *hksat, float *bsw, float *psi_s, float *fmax) {
  if (!ctx || !theta_s || !hksat || !bsw || !psi_s || !fmax) return H9G_EINVAL;
  const size_t n = ctx->n;
  const int L = ctx->L;
  std::vector<float> rows(par_rows(L) * n);
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  HIPCHK(hipMemcpy(rows.data(), ctx->d_par, sizeof(float) * rows.size(), hipMemcpyDeviceToHost));
  float *dst[4] = {theta_s, hksat, bsw, psi_s};
  for (int k = 0; k < 4; k++)
    for (size_t c = 0; c < n; c++)
      for (int i = 0; i < L; i++) dst[k][c * L + i] = rows[(size_t)par_row(L, k, i) * n + c];
  memcpy(fmax, &rows[(size_t)fmax_row(L) * n], sizeof(float) * n);
  return 0;
}

int h9g_init_state(h9g_ctx *ctx) {
  if (!ctx) return H9G_EINVAL;
  if (!ctx->params_set) return H9G_ESTATE;
  HIPCHK(hipSetDevice(ctx->device));
  const int n = (int)ctx->n;
  if (int rc = h9g_init_launch(&ctx->cfg, ctx->sc, n, ctx->d_par, ctx->d_st)) return rc;
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(ctx->d_err, 0, sizeof(int) * STOP_ROWS * ctx->n, ctx->sc));
  HIPCHK(hipMemsetAsync(ctx->d_errflag, 0, sizeof(int), ctx->sc));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  HIPCHK(hipMemsetAsync(ctx->d_hist, 0xff, sizeof(int) * ctx->n, ctx->sc));   // a new state has no last year
  ctx->hist_nsub = 0;
  ctx->state_set = 1;
  ctx->last_err = h9g_error{};
  return 0;
}

// packed (field-major, width-fastest) <-> device rows: h9g_rows.h
int h9g_set_state(h9g_ctx *ctx, const float *packed) {
  if (!ctx || !packed) return H9G_EINVAL;
  const size_t n = ctx->n;
  std::vector<float> rows((size_t)h9g_state_size(ctx->L) * n);
  state_rows_from_packed(ctx->L, n, packed, rows.data());
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpyAsync(ctx->d_st, rows.data(), sizeof(float) * rows.size(), hipMemcpyHostToDevice, ctx->sc));
  HIPCHK(hipMemsetAsync(ctx->d_err, 0, sizeof(int) * STOP_ROWS * n, ctx->sc));
  HIPCHK(hipMemsetAsync(ctx->d_errflag, 0, sizeof(int), ctx->sc));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  HIPCHK(hipMemsetAsync(ctx->d_hist, 0xff, sizeof(int) * ctx->n, ctx->sc));   // a new state has no last year
  ctx->hist_nsub = 0;
  ctx->state_set = 1;
  ctx->last_err = h9g_error{};
  return 0;
}

int h9g_get_state(h9g_ctx *ctx, float *packed) {
  if (!ctx || !packed) return H9G_EINVAL;
  const size_t n = ctx->n;
  std::vector<float> rows((size_t)h9g_state_size(ctx->L) * n);
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  HIPCHK(hipMemcpy(rows.data(), ctx->d_st, sizeof(float) * rows.size(), hipMemcpyDeviceToHost));
  state_packed_from_rows(ctx->L, n, rows.data(), packed);
  return 0;
}

float *h9g_forcing_slot(h9g_ctx *ctx, int slot) {
  if (!ctx || slot < 0 || slot >= ctx->cfg.nslots) return nullptr;
  return ctx->d_forc + (size_t)slot * 7 * ctx->cfg.max_days * ctx->n;
}

void *h9g_host_alloc(size_t bytes) {
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
  return p;
}

void h9g_host_free(void *p) {
  if (p) (void)hipHostFree(p);
}

// (7, nday, ncell) -> slot (7, max_days, ncell)
static int push_impl(h9g_ctx *ctx, int slot, int nday, const float *src, hipMemcpyKind kind, bool async) {
  if (!ctx || !src || slot < 0 || slot >= ctx->cfg.nslots || nday < 1 || nday > ctx->cfg.max_days)
    return H9G_EINVAL;
  HIPCHK(hipSetDevice(ctx->device));
  float *dst = h9g_forcing_slot(ctx, slot);
  const size_t n = ctx->n;
  HIPCHK(hipStreamWaitEvent(ctx->sx, ctx->ev_consumed[slot], 0));
  HIPCHK(hipMemcpy2DAsync(dst, sizeof(float) * ctx->cfg.max_days * n, src, sizeof(float) * nday * n,
                          sizeof(float) * nday * n, 7, kind, ctx->sx));
  HIPCHK(hipEventRecord(ctx->ev_copied[slot], ctx->sx));
  if (!async) HIPCHK(hipStreamSynchronize(ctx->sx));
  ctx->slot_days[slot] = nday;
  return 0;
}

int h9g_push_forcing(h9g_ctx *ctx, int slot, int nday, const float *forcing, int async) {
  return push_impl(ctx, slot, nday, forcing, hipMemcpyHostToDevice, async != 0);
}

int h9g_push_forcing_device(h9g_ctx *ctx, int slot, int nday, const float *dev_forcing) {
  return push_impl(ctx, slot, nday, dev_forcing, hipMemcpyDeviceToDevice, true);
}

// Join the NetCDF prefetch thread of a slot (its copy is queued when it ends).
int join_prefetch(h9g_ctx *ctx, int slot) {
  if (ctx->prefetch[slot].joinable()) ctx->prefetch[slot].join();
  const int rc = ctx->prefetch_rc[slot];
  ctx->prefetch_rc[slot] = 0;
  return rc;
}

// Lists of at most this many cells (the cell-order re-runs' tails) run on
// h9g_pair1_kernel: every workgroup resident at one wave per SIMD.
#define H9G_PAIR1_MAX 1024
// Pacer mode of a pair launch of `blocks` workgroups (h9g_pair.h Pacer): pace
// when all of them are resident at once (one round), else rotate -- a wave of
// a later round starts hundreds of days behind the waves it shares a SIMD with.
// (The solo kernel does not pace: its launches carry the mode the pair kernel's would.)
static int pace_mode(const h9g_ctx *ctx, Shape shape, size_t blocks) {
  if (ctx->prio_mode >= 0) return ctx->prio_mode;
  return blocks <= (size_t)ctx->ncu * shape_info(shape_info(shape).pair ? shape : S_PAIR).waves ? 2 : 1;
}

// Whether a year launch of `base` cells on the context's kernel can carry k
// more cells in a second group for free: a pair kernel kind (not the mixed
// one, whose year is two launches), and the extra waves fit the launch's last
// round of resident workgroups.
bool g2_fits(const h9g_ctx *ctx, size_t base, size_t k) {
  const ShapeInfo si = shape_info(year_shape(ctx->kind, base));
  if (k == 0 || !ctx->sort || ctx->kind == K_MIXED || !si.second_group) return false;
#if defined(H9G_DUMP_AQ)
  return false;
#endif
  const size_t C = (size_t)si.wave_cols, per = (size_t)si.block_cells();
  if (round_up(base, C) + k > ctx->ios) return false;
  const size_t slots = (size_t)ctx->ncu * si.waves;
  const size_t b1 = (base + per - 1) / per, b2 = (round_up(base, C) + k + per - 1) / per;
  return (b2 + slots - 1) / slots == (b1 + slots - 1) / slots;
}

// Fold the finished launches' HIP-event timings into the totals and the
// per-kernel-kind counts (synchronises the compute stream).
int fold_events(h9g_ctx *ctx) {
  HIPCHK(hipStreamSynchronize(ctx->sc));
  for (int i = 0; i < ctx->nev; i++) {
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev0[i], ctx->ev1[i]));
    ctx->total_ms += ms;
    ctx->last_ms = ms;
    const int k = ctx->ev_kind[i];
    ctx->kstat[k][0] += 1.0;
    ctx->kstat[k][1] += (double)ctx->ev_cells[i];
    ctx->kstat[k][2] += ms;
  }
  ctx->nev = 0;
  return 0;
}

// The kernel of a list launch of m cells (the cell order's re-runs): the
// one-column kernel up to H9G_PAIR1_MAX cells (lone waves, one per SIMD);
// at L = 8 the 11-column kernel up to H9G_PAIR11_LIST cells, where its
// waves still fit about one round; else the context's pair kernel (the
// pair kernel for the mixed kind), never solo rounds.  Round 6,
// tools/list_sweep.py (config 2 / config 3, ms per year): 1,000 cells pair
// 132.7 / 67.7, pair11 119.7 / 61.3, pair1 97.4 / 50.2; 10,000 cells pair
// 132.5 / 67.9, pair11 120.0 / 62.3; 20,000 cells 133.6 / 68.5 against
// 136.3 / 70.3.
#define H9G_PAIR11_LIST 16384
static Kind list_kind(const h9g_ctx *ctx, int m) {
  if (ctx->kind == K_SOLO) return K_SOLO;
  if (m <= H9G_PAIR1_MAX && !ctx->no_pair1) return K_PAIR1;
  if (ctx->L == 8 && ctx->kind == K_PAIR && m <= H9G_PAIR11_LIST && !ctx->no_pair11) return K_PAIR11;
  return shape_info(kind_info(ctx->kind).shape).kind;
}

// The launch ranges of an every-cell year on the context's kernel: cells
// [c0, cend) in workgroups of `shape`.  One range, or for the mixed kind
// [0, n_solo) in solo blocks and [n_solo, n) in pair blocks.
struct LaunchRange {
  int c0, cend;
  Shape shape;
  int cpb() const { return shape_info(shape).block_cells(); }
};
static int year_ranges(const h9g_ctx *ctx, LaunchRange r[2]) {
  const int n = (int)ctx->n, ns = (int)ctx->n_solo;
  int k = 0;
  if (ctx->kind != K_MIXED) {
    r[k++] = {0, n, year_shape(ctx->kind, ctx->n)};
  } else {
    if (ns > 0) r[k++] = {0, ns, S_SOLO};
    if (ns < n) r[k++] = {ns, n, S_PAIR};
  }
  return k;
}

// The year kernel of `shape` over a's slots [c0, cend); mixed: the mixed
// kind's year, year_ranges' two launches (neither with a second group).
// mon: the base of the launch's monthly rows; then the shape's monthly kernel.
// An ET context (h9g_set_evap): the shape's ET kernel, with mon or without.
// day: the base of the launch's day rows (h9g_set_days); then the shape's day
// kernel, with mon or without.
static int launch_year(h9g_ctx *ctx, Shape shape, bool mixed, KArgs a, float *mon, float *day) {
  if (mixed) {
    LaunchRange r[2];
    const int nr = year_ranges(ctx, r);
    for (int i = 0; i < nr; i++) {
      a.c0 = r[i].c0;
      a.cend = a.bend = a.split = r[i].cend;
      if (int rc = launch_year(ctx, r[i].shape, false, a, mon, day)) return rc;
    }
    return 0;
  }
  if (int rc = day         ? h9g_day_launch(shape, &ctx->cfg, ctx->sc, a, mon, day)
               : ctx->evap ? h9g_et_launch(shape, &ctx->cfg, ctx->sc, a, mon)
               : mon       ? h9g_mon_launch(shape, &ctx->cfg, ctx->sc, a, mon)
                           : h9g_plain_launch(shape, &ctx->cfg, ctx->sc, a))
    return rc;
  HIPCHK(hipGetLastError());
  return 0;
}

// h9g_sort_kernel over slots [c0, cend) in workgroups of cpb cells, of the
// cells `list` (null: the slots' own numbers) with state st and STOP rows err.
static int sort_slots(h9g_ctx *ctx, int c0, int cend, int cpb, const float *st, const int *err, const int *list) {
  return h9g_sort_launch(&ctx->cfg, ctx->sc, (int)ctx->n, c0, cend, cpb, st, err, ctx->d_hist, ctx->hist_nsub,
                         ctx->d_perm, list);
}

// h9g_diag_kernel over the context's cells, state and last annual means.
int diag_launch(h9g_ctx *ctx) {
  h9g_diag_kernel<<<1, 1024, 0, ctx->sc>>>((int)ctx->n, ctx->L, ctx->d_ann, ctx->d_st, ctx->d_err, ctx->d_diag);
  HIPCHK(hipGetLastError());
  return 0;
}

int run_year_impl(h9g_ctx *ctx, const YearSpec &ys) {
  const int *d_list = ys.d_list;
  const int m = ys.m;
  if (!ctx || ys.slot < 0 || ys.slot >= ctx->cfg.nslots || ys.jyear < 1861 || ys.jyear > 2299) return H9G_EINVAL;
  if (d_list && (m < 1 || (size_t)m > ctx->n || !ys.ann_dst)) return H9G_EINVAL;
  if (ys.bulk && (!d_list || ys.st || ctx->kind == K_SOLO || ctx->kind == K_MIXED)) return H9G_EINVAL;
  if (ys.probe && (!d_list || ys.bulk || !ys.st || ys.k2 > 0 || ys.ndays < 1)) return H9G_EINVAL;
  const bool two = ys.k2 > 0;
  if (two && ((d_list && !ys.bulk) || !ys.h2 || !ys.st2 || !ys.err2 || !ys.ann2 || ys.slot2 < 0 ||
              ys.slot2 >= ctx->cfg.nslots || ys.jyear2 < 1861 || ys.jyear2 > 2299 ||
              !g2_fits(ctx, d_list ? (size_t)m : ctx->n, (size_t)ys.k2)))
    return H9G_EINVAL;
  if (!ctx->params_set || !ctx->state_set) return H9G_ESTATE;
  bool rec[REC_N];   // what the launch records (a probe nothing: with days on it runs on the ET kernels)
  for (int w = 0; w < REC_N; w++) {
    rec[w] = ctx->rec[w].on && !ys.probe;
    if (rec[w] && ((d_list && !ys.rec_dst[w]) || (two && !ys.rec2[w]))) return H9G_EINVAL;
  }
#if defined(H9G_DUMP_AQ)
  if (d_list || ys.st) return H9G_EINVAL;   // (the record is indexed by the annual array's cell)
#endif
  if (const int prc = join_prefetch(ctx, ys.slot)) return prc;
  if (two)
    if (const int prc = join_prefetch(ctx, ys.slot2)) return prc;
  const int nt = ys.probe ? std::min(ys.ndays, days_in_year(ys.jyear)) : days_in_year(ys.jyear);
  const int nt2 = two ? days_in_year(ys.jyear2) : nt;
  if (ctx->slot_days[ys.slot] < nt || (two && ctx->slot_days[ys.slot2] < nt2)) return H9G_EINVAL;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamWaitEvent(ctx->sc, ctx->ev_copied[ys.slot], 0));
  if (two) HIPCHK(hipStreamWaitEvent(ctx->sc, ctx->ev_copied[ys.slot2], 0));
  const int n = (int)ctx->n;
  const size_t ios = ctx->ios;
  for (int w = 0; w < REC_N; w++) {
    RecStream &s = ctx->rec[w];
    if (!rec[w] || s.d_year) continue;      // NaN until a year writes it, as d_ann
    if (int r = rec_malloc(&s.d_year, s.year_floats(ctx->n))) return r;
    HIPCHK(hipMemsetAsync(s.d_year, 0xff, sizeof(float) * s.year_floats(ctx->n), ctx->sc));
  }
  KArgs a;
  a.ncell = n;
  a.c0 = 0;
  a.cend = d_list ? m : n;
  a.nt = nt;
  a.nisurf = ctx->cfg.nisurf;
  a.grow_on = ctx->cfg.grow_on;
  a.fvar = (size_t)ctx->cfg.max_days * ctx->n;
  a.par = ctx->d_par;
  a.st = ys.st ? ys.st : ctx->d_st;
  a.forc = h9g_forcing_slot(ctx, ys.slot);
  a.annual = ctx->d_ann;
  a.err = ys.err ? ys.err : ctx->d_err;
  a.err_flag = ctx->d_errflag;
  a.stamps = nullptr;
  a.sv = nullptr;
  a.perm = nullptr;
  a.sorted_io = 0;
  a.hist = ys.st ? nullptr : ctx->d_hist;   // sort history: the context's own cells only
  a.bend = a.split = a.cend;
  a.nt2 = nt;
  a.st2 = a.st;
  a.err2 = a.err;
  a.iostride = ios;
  a.raw = ys.probe ? 1 : 0;
  const Kind kind = d_list && !ys.bulk ? list_kind(ctx, m) : ctx->kind;
  const size_t ncells = d_list ? (size_t)m : ctx->n;
  // the launch's shape (the mixed kind: its pair part's), decided here once
  // (the one-column kernel carries no second group: ncells is the launch)
  const Shape shape = year_shape(kind, ncells);
  const ShapeInfo si = shape_info(shape);
  // slot-ordered forcing and annual sums (row stride ios: the cells plus a
  // second group's slack)
  if (d_list || ctx->sort) {
    if (!ctx->d_forc_s) HIPCHK(hipMalloc(&ctx->d_forc_s, sizeof(float) * 7 * (size_t)ctx->cfg.max_days * ios));
    if (!ctx->d_ann_s) HIPCHK(hipMalloc(&ctx->d_ann_s, sizeof(float) * annual_rows(ctx->L) * ios));
    for (int w = 0; w < REC_N; w++)
      if (rec[w] && !ctx->rec[w].d_year_s)
        if (int r = rec_malloc(&ctx->rec[w].d_year_s, ctx->rec[w].year_rows * ios)) return r;
  }
  const size_t dvar = (size_t)ctx->cfg.max_days * ios;
  // the second group from the first whole wave after the first group's
  // cells: its slots of d_perm (in h9g_sort_kernel's order over its own
  // state), then its year's forcing into them
  const int pcpb = si.block_cells();
  auto second_group = [&](int base) -> int {
    const int split = (int)round_up((size_t)base, (size_t)si.wave_cols);
    HIPCHK(hipMemcpyAsync(ctx->d_perm2 + split, ys.h2, sizeof(int) * ys.k2, hipMemcpyHostToDevice, ctx->sc));
    if (int rc = sort_slots(ctx, split, split + ys.k2, pcpb, ys.st2, ys.err2, ctx->d_perm2)) return rc;
    h9g_perm_forcing_kernel<<<perm_forcing_blocks(split, split + ys.k2, pcpb, nt2), 256, 0, ctx->sc>>>(
        split, split + ys.k2, pcpb, nt2, n, a.fvar, ios, dvar, ctx->d_perm, h9g_forcing_slot(ctx, ys.slot2),
        ctx->d_forc_s);
    HIPCHK(hipGetLastError());
    a.split = split;
    a.cend = split + ys.k2;
    a.nt2 = nt2;
    a.st2 = ys.st2;
    a.err2 = ys.err2;
    return 0;
  };
  if (d_list) {
    a.perm = d_list;
    if (ctx->sort && kind != K_PAIR1) {
      // the list in h9g_sort_kernel's order (its waves' columns take the
      // same branches), into d_perm, free between every-cell launches
      if (int rc = sort_slots(ctx, 0, m, pcpb, a.st, a.err, d_list)) return rc;
      a.perm = ctx->d_perm;
    }
    h9g_perm_forcing_kernel<<<perm_forcing_blocks(0, m, pcpb, nt), 256, 0, ctx->sc>>>(
        0, m, pcpb, nt, n, a.fvar, ios, dvar, a.perm, a.forc, ctx->d_forc_s);
    HIPCHK(hipGetLastError());
    if (two)
      if (int r = second_group(m)) return r;
    a.forc = ctx->d_forc_s;
    a.annual = ctx->d_ann_s;
    a.sorted_io = 1;
  } else if (ctx->sort) {             // per launch range and its workgroup size (h9g_sort_kernel)
    LaunchRange r[2];
    const int nr = year_ranges(ctx, r);
    for (int i = 0; i < nr; i++)
      if (int rc = sort_slots(ctx, r[i].c0, r[i].cend, r[i].cpb(), ctx->d_st, ctx->d_err, nullptr)) return rc;
    HIPCHK(hipGetLastError());
    a.perm = ctx->d_perm;
#if !defined(H9G_DUMP_AQ)                 // (that record is indexed by the annual array's cell)
    // forcing and annual sums in slot order for the year kernel, per launch
    // range with its workgroup size, as the sort above
    for (int i = 0; i < nr; i++)
      h9g_perm_forcing_kernel<<<perm_forcing_blocks(r[i].c0, r[i].cend, r[i].cpb(), nt), 256, 0, ctx->sc>>>(
          r[i].c0, r[i].cend, r[i].cpb(), nt, n, a.fvar, ios, dvar, ctx->d_perm, a.forc, ctx->d_forc_s);
    HIPCHK(hipGetLastError());
    if (two)
      if (int rc = second_group(n)) return rc;
    a.forc = ctx->d_forc_s;
    a.annual = ctx->d_ann_s;
    a.sorted_io = 1;
#endif
  }
  if (a.sorted_io) a.fvar = dvar;
  // the recorded rows, addressed as a.annual
  float *rec_a[REC_N];
  for (int w = 0; w < REC_N; w++)
    rec_a[w] = !rec[w] ? nullptr : a.sorted_io ? ctx->rec[w].d_year_s : ctx->rec[w].d_year;
  // workgroups of the launch (the pair part's, for the mixed kind)
  const size_t blocks = shape_blocks(shape, kind == K_MIXED ? ctx->n - ctx->n_solo : (size_t)a.cend);
  if (si.pair) {
    // the pair kernels' day-snapshot blocks, one per workgroup of the launch
    const size_t need = std::max<size_t>(blocks, 1) * PairStore<8, H9G_PLANES>::GBLOCK;
    if (ctx->sv_bytes < need) {
      (void)hipFree(ctx->d_sv);
      ctx->d_sv = nullptr;
      ctx->sv_bytes = 0;
      HIPCHK(hipMalloc(&ctx->d_sv, need));
      ctx->sv_bytes = need;
    }
    a.sv = ctx->d_sv;
    if (!ctx->d_pace) {
      const size_t pb = sizeof(unsigned) * 16 * H9G_PACE_ROWS;
      HIPCHK(hipMalloc(&ctx->d_pace, pb));
      HIPCHK(hipMemsetAsync(ctx->d_pace, 0, pb, ctx->sc));
    }
  }
  a.pace = ctx->d_pace;
  a.epoch = ++ctx->epoch;
  a.prio_mode = pace_mode(ctx, shape, blocks);
#if defined(H9G_STAMPS)
  {  // one record of 8 words per wave of the launch
    const size_t words = (size_t)8 * H9G_PWAVES * (blocks + 1);
    if (ctx->stamp_words < words) {
      (void)hipFree(ctx->d_stamps);
      ctx->d_stamps = nullptr;
      HIPCHK(hipMalloc(&ctx->d_stamps, sizeof(unsigned) * words));
      ctx->stamp_words = words;
    }
    HIPCHK(hipMemsetAsync(ctx->d_stamps, 0, sizeof(unsigned) * words, ctx->sc));
    a.stamps = ctx->d_stamps;
    ctx->stamp_shape = shape;
    ctx->stamp_blocks = blocks;
  }
#endif
  if (ctx->nev >= NEVT)   // fold finished timings before reusing events
    if (int r = fold_events(ctx)) return r;
#if defined(H9G_DUMP_AQ)
  // the last year's record to $H9G_AQ_DUMP: year, n, then n x 12 words
  if (const char *path = getenv("H9G_AQ_DUMP"); path && ctx->d_aqbits && ctx->ran) {
    std::vector<unsigned> bits(12 * ctx->n);
    HIPCHK(hipStreamSynchronize(ctx->sc));
    HIPCHK(hipMemcpy(bits.data(), ctx->d_aqbits, sizeof(unsigned) * bits.size(), hipMemcpyDeviceToHost));
    if (FILE *f = fopen(path, "ab")) {
      const int hdr[2] = {ctx->last_year, (int)ctx->n};
      fwrite(hdr, sizeof(int), 2, f);
      fwrite(bits.data(), sizeof(unsigned), bits.size(), f);
      fclose(f);
    }
  }
  if (!ctx->d_aqbits) HIPCHK(hipMalloc(&ctx->d_aqbits, sizeof(unsigned) * 12 * ctx->n));
  HIPCHK(hipMemsetAsync(ctx->d_aqbits, 0, sizeof(unsigned) * 12 * ctx->n, ctx->sc));
  if (int r = h9g_aq_set(ctx->d_aqbits, ctx->d_ann, ctx->sc)) return r;
#endif
  const int e = ctx->nev++;
  ctx->ev_kind[e] = ys.probe ? K_PROBE : kind;
  ctx->ev_cells[e] = (int64_t)ncells + (two ? ys.k2 : 0);
  HIPCHK(hipEventRecord(ctx->ev0[e], ctx->sc));
  if (int r = launch_year(ctx, shape, kind == K_MIXED, a, rec_a[REC_MON], rec_a[REC_DAY])) return r;
  // a one-column context's name is the kernel its last year ran on (the
  // launch record of the shape; until a year runs, h9g_create's)
  if (kind == K_PAIR1 && ctx->kind == K_PAIR1) ctx->kname = year_kernel_name(ctx, kind, ncells);
  HIPCHK(hipEventRecord(ctx->ev1[e], ctx->sc));
  HIPCHK(hipEventRecord(ctx->ev_consumed[ys.slot], ctx->sc));
  if (two) HIPCHK(hipEventRecord(ctx->ev_consumed[ys.slot2], ctx->sc));
  if (a.sorted_io) {
    const unsigned rows = (unsigned)annual_rows(ctx->L);
    // nrows rows of the launch's first group, or of its second (the k2 slots from a.split), back to cell order
    auto unperm = [&](bool second, size_t nrows, const float *src, float *dst) {
      const size_t cells = second ? (size_t)ys.k2 : ncells;
      h9g_unperm_annual_kernel<<<dim3((unsigned)((cells + 255) / 256), rows), 256, 0, ctx->sc>>>(
          (int)cells, n, (int)nrows, second ? a.split : 0, ios, a.perm, src, dst);
    };
    unperm(false, rows, ctx->d_ann_s, d_list ? ys.ann_dst : ctx->d_ann);
    if (two) unperm(true, rows, ctx->d_ann_s, ys.ann2);
    for (int w = 0; w < REC_N; w++) {     // each group the rows of its own year
      const RecStream &s = ctx->rec[w];
      if (!rec[w]) continue;
      unperm(false, s.rows_written(nt), s.d_year_s, d_list ? ys.rec_dst[w] : s.d_year);
      if (two) unperm(true, s.rows_written(nt2), s.d_year_s, ys.rec2[w]);
    }
    HIPCHK(hipGetLastError());
  }
  if (!d_list || ys.bulk)
    if (int r = diag_launch(ctx)) return r;
  if (!ys.st) {
    ctx->last_year = ys.jyear;
    ctx->hist_nsub = nt * ctx->cfg.nisurf;
  }
  ctx->ran = 1;
  return 0;
}

// ---------------------------------------------------------------------------
// Daily diagnostics of selected cells (h9g_set_daily, h9g_get_daily)
// ---------------------------------------------------------------------------
// The year kernels store nothing per day.  The selected cells are run once
// more by h9g_focus_kernel from a gathered copy of their start state, on the
// compute stream before the year kernel (h9g_run_year) or after the decade's
// fixed point has settled (the cell order).  With no selection none of this
// runs: no launch, allocation or synchronisation.

// Room for the lines of years jyear0 .. jyear0+nyears-1; nothing recorded yet.
int daily_begin(h9g_ctx *ctx, int jyear0, int nyears) {
  ctx->daily_nt.clear();
  size_t days = 0;
  for (int y = 0; y < nyears; y++) days += (size_t)days_in_year(jyear0 + y);
  const size_t need = days * H9G_NDAILY * ctx->daily_sel.size();
  if (ctx->daily_cap < need || ctx->fyrs_cap < (size_t)nyears) HIPCHK(hipStreamSynchronize(ctx->sc));
  if (ctx->daily_cap < need) {
    (void)hipFree(ctx->d_daily);
    ctx->d_daily = nullptr;
    ctx->daily_cap = 0;
    if (hipMalloc(&ctx->d_daily, sizeof(float) * need) != hipSuccess) {
      (void)hipGetLastError();
      return H9G_ENOMEM;
    }
    ctx->daily_cap = need;
  }
  if (ctx->fyrs_cap < (size_t)nyears) {
    (void)hipFree(ctx->d_fyrs);
    ctx->d_fyrs = nullptr;
    ctx->fyrs_cap = 0;
    if (hipMalloc(&ctx->d_fyrs, sizeof(FocusYear) * (size_t)nyears) != hipSuccess) {
      (void)hipGetLastError();
      return H9G_ENOMEM;
    }
    ctx->fyrs_cap = (size_t)nyears;
  }
  ctx->h_fyrs.resize(std::max(ctx->h_fyrs.size(), (size_t)nyears));
  return 0;
}

// The selected cells over years jyear0 .. jyear0+ny-1 (forcing in slots[0..ny),
// already waited for on the compute stream) from the state rows st (stride
// ncell), smp from guess where given, STOP records err; appended to the lines
// recorded since daily_begin.
int daily_launch(h9g_ctx *ctx, const float *st, const float *guess, const int *err, const int32_t *slots, int jyear0,
                 int ny) {
  const int nsel = (int)ctx->daily_sel.size(), n = (int)ctx->n, L = ctx->L;
  const size_t k0 = ctx->daily_nt.size();
  size_t day0 = 0, days = 0;
  for (int nt : ctx->daily_nt) day0 += (size_t)nt;
  if (k0 + (size_t)ny > ctx->fyrs_cap || k0 + (size_t)ny > ctx->h_fyrs.size()) return H9G_ESTATE;
  for (int y = 0; y < ny; y++) {
    const int nt = days_in_year(jyear0 + y);
    if (slots[y] < 0 || slots[y] >= ctx->cfg.nslots || ctx->slot_days[slots[y]] < nt) return H9G_EINVAL;
    ctx->h_fyrs[k0 + y].forc = h9g_forcing_slot(ctx, slots[y]);
    ctx->h_fyrs[k0 + y].nt = nt;
    days += (size_t)nt;
  }
  if ((day0 + days) * H9G_NDAILY * (size_t)nsel > ctx->daily_cap) return H9G_ESTATE;
  HIPCHK(hipMemcpyAsync(ctx->d_fyrs + k0, ctx->h_fyrs.data() + k0, sizeof(FocusYear) * (size_t)ny,
                        hipMemcpyHostToDevice, ctx->sc));
  h9g_focus_gather_kernel<<<(unsigned)((nsel + 255) / 256), 256, 0, ctx->sc>>>(nsel, n, h9g_state_size(L), L, ctx->d_dsel,
                                                                              st, guess, ctx->d_dst);
  HIPCHK(hipGetLastError());
  FocusArgs a;
  a.ncell = n;
  a.nsel = nsel;
  a.nyears = ny;
  a.nisurf = ctx->cfg.nisurf;
  a.grow_on = ctx->cfg.grow_on;
  a.fvar = (size_t)ctx->cfg.max_days * ctx->n;
  a.par = ctx->d_par;
  a.st = ctx->d_dst;
  a.sel = ctx->d_dsel;
  a.err = err;
  a.yrs = ctx->d_fyrs + k0;
  a.out = ctx->d_daily + day0 * H9G_NDAILY * (size_t)nsel;
  if (int rc = h9g_focus_launch(&ctx->cfg, ctx->sc, a)) return rc;
  HIPCHK(hipGetLastError());
  for (int y = 0; y < ny; y++) ctx->daily_nt.push_back(days_in_year(jyear0 + y));
  return 0;
}

// h9g_run_year's shadow run: the selected cells from the context's state as
// the year kernel is about to find it.
static int daily_year(h9g_ctx *ctx, int slot, int jyear) {
  if (slot < 0 || slot >= ctx->cfg.nslots || jyear < 1861 || jyear > 2299) return H9G_EINVAL;
  if (!ctx->params_set || !ctx->state_set) return H9G_ESTATE;
  if (const int prc = join_prefetch(ctx, slot)) return prc;
  HIPCHK(hipSetDevice(ctx->device));
  if (int r = daily_begin(ctx, jyear, 1)) return r;
  HIPCHK(hipStreamWaitEvent(ctx->sc, ctx->ev_copied[slot], 0));
  const int32_t s = slot;
  return daily_launch(ctx, ctx->d_st, nullptr, ctx->d_err, &s, jyear, 1);
}

int h9g_set_daily(h9g_ctx *ctx, int nsel, const int32_t *cells) {
  if (!ctx || nsel < 0 || (nsel > 0 && !cells) || (size_t)nsel > ctx->n) return H9G_EINVAL;
  for (int j = 0; j < nsel; j++)
    if (cells[j] < 0 || (size_t)cells[j] >= ctx->n || (j > 0 && cells[j] <= cells[j - 1])) return H9G_EINVAL;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  (void)hipFree(ctx->d_dsel);
  (void)hipFree(ctx->d_dst);
  ctx->d_dsel = nullptr;
  ctx->d_dst = nullptr;
  ctx->daily_sel.clear();
  ctx->daily_nt.clear();
  if (nsel == 0) return 0;
  if (hipMalloc(&ctx->d_dsel, sizeof(int) * (size_t)nsel) != hipSuccess ||
      hipMalloc(&ctx->d_dst, sizeof(float) * (size_t)h9g_state_size(ctx->L) * (size_t)nsel) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(ctx->d_dsel);
    ctx->d_dsel = nullptr;
    return H9G_ENOMEM;
  }
  HIPCHK(hipMemcpy(ctx->d_dsel, cells, sizeof(int) * (size_t)nsel, hipMemcpyHostToDevice));
  ctx->daily_sel.assign(cells, cells + nsel);
  return 0;
}

int h9g_get_daily(h9g_ctx *ctx, int k, float *out) {
  if (!ctx || !out) return H9G_EINVAL;
  if (ctx->daily_sel.empty() || ctx->daily_nt.empty()) return H9G_ESTATE;
  if (k < 0 || (size_t)k >= ctx->daily_nt.size()) return H9G_EINVAL;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  size_t day0 = 0;
  for (int y = 0; y < k; y++) day0 += (size_t)ctx->daily_nt[(size_t)y];
  const size_t row = (size_t)H9G_NDAILY * ctx->daily_sel.size();
  HIPCHK(hipMemcpy(out, ctx->d_daily + day0 * row, sizeof(float) * (size_t)ctx->daily_nt[(size_t)k] * row,
                   hipMemcpyDeviceToHost));
  return 0;
}

int h9g_run_year(h9g_ctx *ctx, int slot, int jyear) {
  if (ctx && !ctx->daily_sel.empty())
    if (int r = daily_year(ctx, slot, jyear)) return r;
  YearSpec ys;
  ys.slot = slot;
  ys.jyear = jyear;
  if (ctx)
    for (RecStream &s : ctx->rec) s.nt.clear();
  const int r = run_year_impl(ctx, ys);
  if (r == 0)
    for (RecStream &s : ctx->rec)
      if (s.on) {
        s.nt.assign(1, days_in_year(jyear));
        s.in_ret = false;
      }
  return r;
}

int h9g_set_monthly(h9g_ctx *ctx, int on) {
  if (!ctx) return H9G_EINVAL;
#if defined(H9G_STAMPS)
  if (on) return H9G_EINVAL;   // (the phase-stamp measurement build profiles the year kernels proper)
#endif
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  ctx->rec[REC_MON].on = on ? 1 : 0;
  ctx->rec[REC_MON].nt.clear();
  return 0;
}

// The context's name follows (h9g_kernel_name: the ET kernels').  The day-1
// probes of the cell order then run the ET kernels too: their rows are the
// running sums (KArgs::raw), so h9g_probe_cmp_kernel compares the first
// day's evaporation with the other rows.
int h9g_set_evap(h9g_ctx *ctx, int on) {
  if (!ctx) return H9G_EINVAL;
#if defined(H9G_STAMPS)
  if (on) return H9G_EINVAL;   // (as h9g_set_monthly)
#endif
  if (!on && ctx->rec[REC_DAY].on) return H9G_ESTATE;  // day recording rides on the ET sum (h9g_set_days)
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  if (ctx->evap != (on ? 1 : 0)) {
    ctx->evap = on ? 1 : 0;
    // (a one-column context's name is the shape of its last year: renamed in place)
    const std::string from = on ? "_kernel" : "_et_kernel", to = on ? "_et_kernel" : "_kernel";
    for (size_t p = 0; (p = ctx->kname.find(from, p)) != std::string::npos; p += to.size())
      ctx->kname.replace(p, from.size(), to);
  }
  return 0;
}

// Year k of what the last call recorded of stream `which`: the rows that year wrote.
static int rec_get(h9g_ctx *ctx, int which, int k, float *out) {
  if (!ctx || !out) return H9G_EINVAL;
  const RecStream &s = ctx->rec[which];
  if (s.nt.empty()) return H9G_ESTATE;
  if (k < 0 || (size_t)k >= s.nt.size()) return H9G_EINVAL;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  HIPCHK(hipMemcpy(out, s.in_ret ? s.ret_year(ctx->n, k) : s.d_year,
                   sizeof(float) * s.rows_written(s.nt[(size_t)k]) * ctx->n, hipMemcpyDeviceToHost));
  return 0;
}

int h9g_get_monthly(h9g_ctx *ctx, int k, float *out) { return rec_get(ctx, REC_MON, k, out); }

// Day records (include/h9g.h): needs ET recording on.  The context's name
// follows (h9g_kernel_name: the day kernels').
int h9g_set_days(h9g_ctx *ctx, int on) {
  if (!ctx) return H9G_EINVAL;
#if defined(H9G_STAMPS)
  if (on) return H9G_EINVAL;   // (as h9g_set_monthly)
#endif
  if (on && !ctx->evap) return H9G_ESTATE;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  RecStream &s = ctx->rec[REC_DAY];
  if (s.on != (on ? 1 : 0)) {
    s.on = on ? 1 : 0;
    const std::string from = on ? "_et_kernel" : "_day_kernel", to = on ? "_day_kernel" : "_et_kernel";
    for (size_t p = 0; (p = ctx->kname.find(from, p)) != std::string::npos; p += to.size())
      ctx->kname.replace(p, from.size(), to);
  }
  s.nt.clear();
  return 0;
}

int h9g_get_days(h9g_ctx *ctx, int k, float *out) { return rec_get(ctx, REC_DAY, k, out); }

// An ordered call of `nyears` years begins: room for them in the retained
// buffer of every recording that is on; none recorded yet.
int rec_begin(h9g_ctx *ctx, int nyears) {
  for (RecStream &s : ctx->rec) {
    if (!s.on) continue;
    s.nt.clear();
    s.base = 0;
    if (s.ret_cap >= (size_t)nyears) continue;
    HIPCHK(hipStreamSynchronize(ctx->sc));
    (void)hipFree(s.d_ret);
    s.ret_cap = 0;
    if (int r = rec_malloc(&s.d_ret, (size_t)nyears * s.year_floats(ctx->n))) return r;
    s.ret_cap = (size_t)nyears;
  }
  return 0;
}

int h9g_launch_stats(h9g_ctx *ctx, double *out, int n, int reset) {
  if (!ctx || !out || n < 1) return H9G_EINVAL;
  if (int r = fold_events(ctx)) return r;
  int m = 0;
  for (int k = K_PAIR; k <= K_PROBE; k++)
    for (int j = 0; j < 3 && m < n; j++) out[m++] = ctx->kstat[k][j];
  if (reset)
    for (auto &row : ctx->kstat) row[0] = row[1] = row[2] = 0.0;
  return m;
}

#if defined(H9G_STAMPS)
// The last stamped launch's record (ctx->d_stamps, 8 phase cycle sums per wave): the phases' means and the
// waves' load balance, to stderr.
static int stamps_report(h9g_ctx *ctx) {
  if (ctx->d_stamps && (ctx->kind == K_PAIR || ctx->kind == K_PAIR11 || ctx->kind == K_PAIR1)) {   // mean shader cycles per wave and substep, by phase
    const size_t cw = (size_t)shape_info(kind_info(ctx->kind).shape).wave_cols, nw = (ctx->n + cw - 1) / cw;
    std::vector<unsigned> st(8 * nw);
    HIPCHK(hipMemcpy(st.data(), ctx->d_stamps, sizeof(unsigned) * 8 * nw, hipMemcpyDeviceToHost));
    double sum[8] = {0}, tot = 0;
    for (size_t w = 0; w < nw; w++)
      for (int k = 0; k < 8; k++) sum[k] += st[8 * w + k];
    const double steps = (double)nw * days_in_year(ctx->last_year) * ctx->cfg.nisurf;
    fprintf(stderr, "h9g stamps (cycles/wave/substep):");
    for (int k = 0; k < 8; k++) { fprintf(stderr, " p%d=%.0f", k, sum[k] / steps); tot += sum[k]; }
    fprintf(stderr, " total=%.0f\n", tot / steps);
    if (shape_info(ctx->stamp_shape).front()) {
      // the two-wave shape, by the launch's own record: p1 above is the main
      // wave's wait at barrier 2; the front waves' records follow the grid's
      // main waves' (pair_body: one main wave per workgroup)
      std::vector<unsigned> fs(8 * nw);
      HIPCHK(hipMemcpy(fs.data(), ctx->d_stamps + 8 * ctx->stamp_blocks, sizeof(unsigned) * 8 * nw, hipMemcpyDeviceToHost));
      // Means over every substep, of both kinds together.  The labels hold for a
      // substep that starts with the water table in the column: marks 3 and 4 of
      // the chain call follow barrier 2, 5 and 6 are the chain, 7 the wait at
      // barrier 3.  In a substep that starts below it the call returns before
      // mark 3, so everything from the front's end to barrier 3 (the wait at
      // barrier 2, the main wave's sweep and its own chain) falls into slot 7.
      // So "chain" is the share of in-column substeps times the chain's length,
      // and "wait at barrier 3" grows with the share of the other kind.
      double w = 0, f = 0, w2 = 0, ch = 0, w3 = 0;
      for (size_t k = 0; k < nw; k++) {
        w += fs[8 * k];
        f += fs[8 * k + 1];
        w2 += fs[8 * k + 3] + fs[8 * k + 4];     // (H9G_P1_SIDE: the chain call's marks 3 and 4 follow barrier 2)
        ch += fs[8 * k + 5] + fs[8 * k + 6];
        w3 += fs[8 * k + 7];
      }
      fprintf(stderr, "h9g stamps, front waves (cycles/wave/substep): wait at barrier 1=%.0f front=%.0f", w / steps,
              f / steps);
      if (ch > 0)                                // the water-table chain on the second wave
        fprintf(stderr, " wait at barrier 2=%.0f chain=%.0f wait at barrier 3=%.0f", w2 / steps, ch / steps, w3 / steps);
      fprintf(stderr, "\n");
    }
    // load balance: per-wave totals (the kernel lasts as long as its slowest wave)
    std::vector<double> wt(nw, 0.0);
    for (size_t w = 0; w < nw; w++)
      for (int k = 0; k < 8; k++) wt[w] += st[8 * w + k];
    std::vector<double> ws(wt);
    std::sort(ws.begin(), ws.end());
    const double mean = tot / nw;
    fprintf(stderr, "h9g wave totals / mean: min %.3f p50 %.3f p90 %.3f p99 %.3f max %.3f\n", ws[0] / mean,
            ws[nw / 2] / mean, ws[nw * 9 / 10] / mean, ws[nw * 99 / 100] / mean, ws[nw - 1] / mean);
    // by blockIdx % 8 (workgroups are dealt round-robin to the 8 XCDs) and by wave in block (SIMD)
    double bx[8] = {0}, nx[8] = {0}, bs[4] = {0}, ns[4] = {0};
    for (size_t w = 0; w < nw; w++) {
      const size_t b = w / 4;
      bx[b % 8] += wt[w];
      nx[b % 8] += 1;
      bs[w % 4] += wt[w];
      ns[w % 4] += 1;
    }
    {  // phases of the slowest tenth of the waves against the fastest half
      const double cut90 = ws[nw * 9 / 10], cut50 = ws[nw / 2];
      double hi[8] = {0}, lo[8] = {0}, nh = 0, nl = 0;
      for (size_t w = 0; w < nw; w++) {
        if (wt[w] >= cut90) { nh++; for (int k = 0; k < 8; k++) hi[k] += st[8 * w + k]; }
        if (wt[w] <= cut50) { nl++; for (int k = 0; k < 8; k++) lo[k] += st[8 * w + k]; }
      }
      const double sub = (double)days_in_year(ctx->last_year) * ctx->cfg.nisurf;
      fprintf(stderr, "h9g slowest 10%% / fastest 50%% waves by phase (cycles/substep):");
      for (int k = 0; k < 8; k++) fprintf(stderr, " p%d %.0f/%.0f", k, hi[k] / nh / sub, lo[k] / nl / sub);
      fprintf(stderr, "\n");
    }
    {
      fprintf(stderr, "h9g mean wave total by slot decile:");
      for (int d = 0; d < 10; d++) {
        double a = 0, c = 0;
        for (size_t w = nw * d / 10; w < nw * (d + 1) / 10; w++) { a += wt[w]; c++; }
        fprintf(stderr, " %.3f", a / c / mean);
      }
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "h9g mean wave total by block%%8:");
    for (int k = 0; k < 8; k++) fprintf(stderr, " %.3f", bx[k] / nx[k] / mean);
    fprintf(stderr, "  by wave-in-block:");
    for (int k = 0; k < 4; k++) fprintf(stderr, " %.3f", bs[k] / ns[k] / mean);
    fprintf(stderr, "\n");
  }
  return 0;
}
#endif

int h9g_sync(h9g_ctx *ctx) {
  if (!ctx) return H9G_EINVAL;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->sx));
  if (int r = fold_events(ctx)) return r;
#if defined(H9G_STAMPS)
  if (int r = stamps_report(ctx)) return r;
#endif
#if defined(H9G_COUNT_EXACT)
  if (int r = h9g_exact_report()) return r;
#endif
#if defined(H9G_COUNT_BRANCH)
  if (int r = h9g_branch_report()) return r;
#endif
  int flag = 0;
  HIPCHK(hipMemcpy(&flag, ctx->d_errflag, sizeof(int), hipMemcpyDeviceToHost));
  if (!flag) return 0;
  if (ctx->last_err.code == 0) {
    const size_t n = ctx->n;
    std::vector<int> e(STOP_ROWS * n);
    HIPCHK(hipMemcpy(e.data(), ctx->d_err, sizeof(int) * STOP_ROWS * n, hipMemcpyDeviceToHost));
    for (size_t c = 0; c < n; c++) {
      if (e[c]) {        // lowest cell index first, as the reference's cell-outer loop
        ctx->last_err.code = e[c];
        ctx->last_err.cell = (int)c;
        ctx->last_err.year = ctx->last_year;
        ctx->last_err.day = e[n + c];
        ctx->last_err.substep = e[2 * n + c];
        ctx->last_err.value = __builtin_bit_cast(float, e[3 * n + c]);
        break;
      }
    }
  }
  return ctx->last_err.code;
}

int h9g_run_site(h9g_ctx *ctx, int nday, const float *sub, const float *daily, const float *lai, float *diag) {
  if (!ctx || nday <= 0 || !sub || !daily || !lai || !diag) return H9G_EINVAL;
  if (!ctx->params_set || !ctx->state_set) return H9G_ESTATE;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  const size_t n = ctx->n, ns = (size_t)ctx->cfg.nisurf;
  const size_t nsub = (size_t)nday * ns * 5 * n, nd = (size_t)nday * 2 * n, nl = (size_t)nday * 3 * n;
  const size_t nout = (size_t)nday * DAILY_ROWS * n;
  float *buf = nullptr;
  HIPCHK(hipMalloc(&buf, sizeof(float) * (nsub + nd + nl + nout)));
  SiteArgs a;
  a.ncell = (int)n;
  a.nday = nday;
  a.nisurf = ctx->cfg.nisurf;
  a.par = ctx->d_par;
  a.st = ctx->d_st;
  a.sub = buf;
  a.daily = buf + nsub;
  a.lai = buf + nsub + nd;
  a.out = buf + nsub + nd + nl;
  a.err = ctx->d_err;
  a.err_flag = ctx->d_errflag;
  int rc = 0;
  hipError_t e = hipMemcpy(buf, sub, sizeof(float) * nsub, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(buf + nsub, daily, sizeof(float) * nd, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(buf + nsub + nd, lai, sizeof(float) * nl, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    rc = h9g_site_launch(&ctx->cfg, ctx->sc, a);
    if (rc) {
      (void)hipFree(buf);
      return rc;
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->sc);
  if (e == hipSuccess) e = hipMemcpy(diag, a.out, sizeof(float) * nout, hipMemcpyDeviceToHost);
  (void)hipFree(buf);
  if (e != hipSuccess) {
    fprintf(stderr, "h9g: h9g_run_site failed: %s\n", hipGetErrorString(e));
    return H9G_EHIP;
  }
  ctx->last_year = 0;      // error records of a site run: day counts from the start of the run
  ctx->ran = 1;
  rc = h9g_sync(ctx);
  return rc;
}

// Per-cell STOP records of the runs since the last state (re)set: 4 rows of
// ncell int32 -- code (0 = none), day, substep, bits of the float value.
int h9g_get_errors(h9g_ctx *ctx, int32_t *rec) {
  if (!ctx || !rec) return H9G_EINVAL;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  HIPCHK(hipMemcpy(rec, ctx->d_err, sizeof(int32_t) * STOP_ROWS * ctx->n, hipMemcpyDeviceToHost));
  return 0;
}

int h9g_last_error(h9g_ctx *ctx, h9g_error *err) {
  if (!ctx || !err) return H9G_EINVAL;
  *err = ctx->last_err;
  return 0;
}

int h9g_get_annual(h9g_ctx *ctx, float *annual) {
  if (!ctx || !annual) return H9G_EINVAL;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  HIPCHK(hipMemcpy(annual, ctx->d_ann, sizeof(float) * annual_rows(ctx->L) * ctx->n, hipMemcpyDeviceToHost));
  return 0;
}

int h9g_get_diagnostics(h9g_ctx *ctx, double *host_out, double *dev_out) {
  if (!ctx) return H9G_EINVAL;
  HIPCHK(hipSetDevice(ctx->device));
  if (dev_out)
    HIPCHK(hipMemcpyAsync(dev_out, ctx->d_diag, sizeof(double) * H9G_NDIAG, hipMemcpyDeviceToDevice, ctx->sc));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  if (host_out) HIPCHK(hipMemcpy(host_out, ctx->d_diag, sizeof(double) * H9G_NDIAG, hipMemcpyDeviceToHost));
  return 0;
}

// Stream-ordered diagnostics hand-off for a cross-GPU all-reduce with no
// host synchronisation: the copy into dev_out waits for the work already
// queued on `stream` (e.g. last year's all-reduce still reading dev_out),
// and `stream` waits for the copy.  The next h9g_run_year queues behind it
// on the compute stream, so year k+1 runs while year k's all-reduce does.
int h9g_get_diagnostics_async(h9g_ctx *ctx, double *dev_out, void *stream) {
  if (!ctx || !dev_out) return H9G_EINVAL;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipEventRecord(ctx->ev_ext, s));
  HIPCHK(hipStreamWaitEvent(ctx->sc, ctx->ev_ext, 0));
  HIPCHK(hipMemcpyAsync(dev_out, ctx->d_diag, sizeof(double) * H9G_NDIAG, hipMemcpyDeviceToDevice, ctx->sc));
  HIPCHK(hipEventRecord(ctx->ev_diag, ctx->sc));
  HIPCHK(hipStreamWaitEvent(s, ctx->ev_diag, 0));
  return 0;
}

int h9g_set_cells(h9g_ctx *ctx, const int64_t *gid, const float *lat) {
  if (!ctx || !gid || !lat) return H9G_EINVAL;
  ctx->h_gid.assign(gid, gid + ctx->n);
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipMemcpy(ctx->d_gid, gid, sizeof(int64_t) * ctx->n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->d_lat, lat, sizeof(float) * ctx->n, hipMemcpyHostToDevice));
  return 0;
}

// Async PGF prefetch (READ_PGF.f90 on a host thread): days [t0, t0+nt) of
// the 7 NetCDF files are gathered for the context's cells (h9g_set_cells)
// into the slot's pinned staging buffer by the reader's thread pool, and
// copied into the slot on the copy stream in 8 day groups, each as soon as
// the pool has filled it (round 4: the copy overlaps the rest of the read
// instead of following it).  h9g_run_year on that slot joins the thread
// first, so the read of year y+1 overlaps the kernel of year y.
int h9g_nc_forcing_prefetch(h9g_ctx *ctx, int slot, const char *const *paths, int nx, int ny, int t0, int nt) {
  if (!ctx || slot < 0 || slot >= ctx->cfg.nslots || !paths || nt < 1 || nt > ctx->cfg.max_days || t0 < 0)
    return H9G_EINVAL;
  if (ctx->h_gid.size() != ctx->n) return H9G_ESTATE;
  for (int k = 0; k < H9G_NFORCING; k++)
    if (!paths[k]) return H9G_EINVAL;
  if (const int prc = join_prefetch(ctx, slot)) return prc;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t n = ctx->n;
  if (!ctx->h_pin[slot])
    HIPCHK(hipHostMalloc(&ctx->h_pin[slot], sizeof(float) * 7 * (size_t)ctx->cfg.max_days * n, hipHostMallocDefault));
  // the staging buffer may still feed the slot's previous copy
  HIPCHK(hipEventSynchronize(ctx->ev_copied[slot]));
  std::vector<std::string> p(paths, paths + H9G_NFORCING);
  ctx->slot_days[slot] = nt;
  ctx->prefetch[slot] = std::thread([ctx, slot, p, nx, ny, t0, nt]() {
    const char *pp[H9G_NFORCING];
    for (int k = 0; k < H9G_NFORCING; k++) pp[k] = p[k].c_str();
    if (hipSetDevice(ctx->device) != hipSuccess ||
        hipStreamWaitEvent(ctx->sx, ctx->ev_consumed[slot], 0) != hipSuccess) {
      ctx->prefetch_rc[slot] = H9G_EHIP;
      return;
    }
    const size_t n = ctx->n;
    float *dst = h9g_forcing_slot(ctx, slot), *src = ctx->h_pin[slot];
    std::atomic<int> hip_rc{0};
    std::mutex q;                      // one enqueuer at a time on the copy stream
    int rc = h9g_nc_read_groups(pp, nx, ny, (int)n, ctx->h_gid.data(), t0, nt, src, 8, [&](int d0, int d1) {
      std::lock_guard<std::mutex> g(q);
      // days [d0, d1) of the 7 variables: staging (7, nt, n) -> slot (7, max_days, n)
      if (hipSetDevice(ctx->device) != hipSuccess ||
          hipMemcpy2DAsync(dst + (size_t)d0 * n, sizeof(float) * ctx->cfg.max_days * n, src + (size_t)d0 * n,
                           sizeof(float) * nt * n, sizeof(float) * (size_t)(d1 - d0) * n, 7, hipMemcpyHostToDevice,
                           ctx->sx) != hipSuccess)
        hip_rc = H9G_EHIP;
    });
    if (rc == 0 && hip_rc) rc = hip_rc;
    if (rc == 0 && hipEventRecord(ctx->ev_copied[slot], ctx->sx) != hipSuccess) rc = H9G_EHIP;
    ctx->prefetch_rc[slot] = rc;
  });
  return 0;
}

float h9g_last_kernel_ms(h9g_ctx *ctx) { return ctx ? ctx->last_ms : 0.0f; }

double h9g_total_kernel_ms(h9g_ctx *ctx, int reset) {
  if (!ctx) return 0.0;
  const double t = ctx->total_ms;
  if (reset) ctx->total_ms = 0.0;
  return t;
}

const char *h9g_kernel_name(h9g_ctx *ctx) { return ctx ? ctx->kname.c_str() : ""; }

// (h9g_build_id is defined in h9g_io.cpp, the translation unit that is
// recompiled with every build.)

}  // extern "C"
