// h9g_aux.hip -- what stands beside the time stepping: the soil parameter
// build (h9g_soil_layer, h9g_soil_fmax), the synthetic inputs on the device
// and on the host (h9g_synth_*, h9g_land_cells), and the self-tests of the
// math, the division and the pacing ids, with their small kernels.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "h9g_ctx.h"
#include "h9g_synth.h"

static const uint64_t h_exp2tab[32] = H9M_EXP2F_TAB_INIT;
static const double h_log2tab[32] = H9M_POWF_LOG2_TAB_INIT;

template <int L>
__global__ void __launch_bounds__(H9G_BLOCK) h9g_synth_params_kernel(int ncell, const int64_t *__restrict__ gid,
                                                                     uint64_t seed, float *__restrict__ par) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncell) return;
  const size_t n = ncell;
  const uint64_t g = (uint64_t)gid[c];
#pragma unroll
  for (int l = 0; l < L; l++) {
    float ts, hk, b, ps;
    h9s::params(seed, g, l, &ts, &hk, &b, &ps);
    par[(size_t)par_row(L, PF_TS, l) * n + c] = ts;
    par[(size_t)par_row(L, PF_HKS, l) * n + c] = hk;
    par[(size_t)par_row(L, PF_BSW, l) * n + c] = b;
    par[(size_t)par_row(L, PF_PSI, l) * n + c] = ps;
  }
  par[(size_t)fmax_row(L) * n + c] = h9s::fmax_param(seed, g);
}

__global__ void __launch_bounds__(H9G_BLOCK) h9g_synth_forcing_kernel(int ncell, int nday, int day0,
                                                                      const int64_t *__restrict__ gid,
                                                                      const float *__restrict__ lat, uint64_t seed,
                                                                      size_t fvar, float *__restrict__ forc) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int d = blockIdx.y;
  if (c >= ncell || d >= nday) return;
  float v[7];
  h9s::forcing(seed, (uint64_t)gid[c], lat[c], (int64_t)day0 + d, v);
#pragma unroll
  for (int k = 0; k < 7; k++) forc[k * fvar + (size_t)d * ncell + c] = v[k];
}

// ---------------------------------------------------------------------------
// Soil parameter build, INIT.f90:575-631: each 0.5 deg
// cell of the context averages its 60x60 block of 30" pixels whose
// theta_s >= 0, then converts units.  The reference sums sequentially
// (x1 outer, y1 inner).  h9g_soil_kernel reads the block coalesced (a wave
// per pixel row) and reduces in a tree; that equals the sequential sum
// bit for bit whenever every contributing value is an integer of
// magnitude <= 4096 (the BNU fields are stored as scaled integers): all
// partial sums are then exact floats below 2^24.  Any other block is
// flagged and summed in the reference's order by h9g_soil_seq_kernel.
// ---------------------------------------------------------------------------
#define H9G_SWAVES 4
struct SoilOut {
  __device__ __forceinline__ static void store(float *par, int L, int layer, size_t n, int c, int v,
                                                float sum, int j) {
    float m = sum;
    if (j > 0) m = m / (float)j;                                  // INIT.f90:593-598
    float out;
    if (v == 0) out = m / 1.0E3f;                                 // theta_s      :613
    else if (v == 1) out = 10.0f * m / 86400.0f;                  // hksat        :614
    else if (v == 2) out = 1.0f / MAXF(m / 1.0E3f, 1.0E-8f);      // bsw          :615,624,628
    else out = 10.0f * m;                                         // psi_s        :616
    par[(size_t)par_row(L, v, layer) * n + c] = out;
  }
};

__device__ __forceinline__ bool small_int(float v) { return v == __builtin_truncf(v) && __builtin_fabsf(v) <= 4096.0f; }

__global__ void __launch_bounds__(64 * H9G_SWAVES) h9g_soil_kernel(int nx, int ncell, const int64_t *__restrict__ gid,
                                                                  const float *__restrict__ ts,
                                                                  const float *__restrict__ ks,
                                                                  const float *__restrict__ lm,
                                                                  const float *__restrict__ ps, size_t pitch, int L,
                                                                  int layer, float *__restrict__ par,
                                                                  int *__restrict__ slow) {
  __shared__ float red[H9G_SWAVES][5];
  __shared__ int red_ok[H9G_SWAVES];
  const int c = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g = gid[c];
  const int x = (int)(g % nx), y = (int)(g / nx);
  const size_t base = (size_t)y * 60 * pitch + (size_t)x * 60 + lane;
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f, sj = 0.0f;
  bool ok = true;
  if (lane < 60) {
#pragma unroll 5
    for (int r = wave; r < 60; r += H9G_SWAVES) {                 // one pixel row per wave
      const size_t i = base + (size_t)r * pitch;
      const float a = ts[i];
      if (a >= 0.0f) {                                            // :584
        const float b = ks[i], d = lm[i], e = ps[i];
        s0 += a; s1 += b; s2 += d; s3 += e; sj += 1.0f;
        ok = ok && small_int(a) && small_int(b) && small_int(d) && small_int(e);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                              // wave tree (exact: see above)
    s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o);
    s3 += __shfl_xor(s3, o); sj += __shfl_xor(sj, o);
  }
  const bool wok = __builtin_amdgcn_ballot_w64(!ok) == 0;
  if (lane == 0) {
    red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; red[wave][3] = s3; red[wave][4] = sj;
    red_ok[wave] = wok;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int v = threadIdx.x;
    bool all = true;
    float sum = 0.0f, cnt = 0.0f;
    for (int w = 0; w < H9G_SWAVES; w++) {
      all = all && red_ok[w];
      sum += red[w][v];
      cnt += red[w][4];
    }
    if (!all) {
      if (v == 0) slow[c] = 1;
    } else {
      SoilOut::store(par, L, layer, (size_t)ncell, c, v, sum, (int)cnt);
    }
  }
}

// The reference's order for the flagged blocks: thread (cell, variable).
__global__ void h9g_soil_seq_kernel(int nx, int ncell, const int64_t *__restrict__ gid, const float *__restrict__ ts,
                                    const float *__restrict__ ks, const float *__restrict__ lm,
                                    const float *__restrict__ ps, size_t pitch, int L, int layer,
                                    float *__restrict__ par, const int *__restrict__ slow) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int c = t >> 2, v = t & 3;
  if (c >= ncell || !slow[c]) return;
  const float *src = v == 0 ? ts : (v == 1 ? ks : (v == 2 ? lm : ps));
  const int64_t g = gid[c];
  const int x = (int)(g % nx), y = (int)(g / nx);
  float sum = 0.0f;
  int j = 0;
  for (int x1 = x * 60; x1 < x * 60 + 60; x1++)                  // :582-592, x1 outer
    for (int y1 = y * 60; y1 < y * 60 + 60; y1++) {
      const size_t i = (size_t)y1 * pitch + x1;
      if (ts[i] >= 0.0f) {
        sum = sum + src[i];
        j = j + 1;
      }
    }
  SoilOut::store(par, L, layer, (size_t)ncell, c, v, sum, j);
}

// Probe of the hardware ids pace_key decodes (h9g_pair.h): the
// pair kernel's launch shape and LDS footprint (dynamic LDS of the same size,
// so the same workgroups per CU), each wave's lane 0 arriving at a bounded
// barrier (s_sleep, at most `spin` shader cycles) and then recording
// HW_REG_HW_ID, HW_REG_XCC_ID and whether every wave had arrived, i.e. was
// resident at once.  out: 3 words per wave (blockIdx * waves + wave).
__global__ void __launch_bounds__(64 * H9G_PWAVES) h9g_pace_probe_kernel(unsigned *out, unsigned *arrive,
                                                                         unsigned total, long long spin) {
  extern __shared__ float pad[];
  if (threadIdx.x & 63) return;
  pad[threadIdx.x] = 0.0f;
  const unsigned w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const long long t0 = clock64();
  unsigned seen = 0;
  while ((seen = __hip_atomic_load(arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < total &&
         clock64() - t0 < spin)
    __builtin_amdgcn_s_sleep(2);
  out[3 * w + 0] = __builtin_amdgcn_s_getreg((31 << 11) | 4);           // HW_REG_HW_ID
  out[3 * w + 1] = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u;     // HW_REG_XCC_ID
  out[3 * w + 2] = seen >= total ? 1u : 0u;
}

// MathFast's division path with a device-computed reciprocal (recip64).
__global__ void h9g_div_kernel(int n, const float *x, const float *d, float *out, int *flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  MathFast mf{{nullptr, nullptr}, false};
  out[i] = mf.div(x[i], d[i], recip64(d[i]));
  flag[i] = (mf.special || mf.redone) ? 1 : 0;     // 1: the quotient was redone as x / d
}

__global__ void h9g_math_kernel(int n, const float *x, const float *y, float *out) {
  __shared__ uint64_t s_e2[32];
  __shared__ double s_l2[32];
  load_tabs(s_e2, s_l2);
  const h9m::Tabs T = {s_e2, s_l2};
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = y ? h9m::powf(x[i], y[i], T) : h9m::expf(x[i], T);
}

// The year kernels' math (MathFast: glibc's main path, the rest redone in
// place); flag = 1 where it was redone.
__global__ void h9g_math_fast_kernel(int n, const float *x, const float *y, float *out, int *flag) {
  __shared__ uint64_t s_e2[32];
  __shared__ double s_l2[32];
  load_tabs(s_e2, s_l2);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  MathFast mf{{s_e2, s_l2}, false};
  out[i] = y ? mf.powf(x[i], y[i]) : mf.expf(x[i]);
  flag[i] = mf.redone ? 1 : 0;
}

extern "C" {

int h9g_synth_params(h9g_ctx *ctx, uint64_t seed) {
  if (!ctx) return H9G_EINVAL;
  HIPCHK(hipSetDevice(ctx->device));
  const int n = (int)ctx->n;
  if (ctx->L == 8)
    h9g_synth_params_kernel<8><<<nblocks(n), H9G_BLOCK, 0, ctx->sc>>>(n, ctx->d_gid, seed, ctx->d_par);
  else
    h9g_synth_params_kernel<10><<<nblocks(n), H9G_BLOCK, 0, ctx->sc>>>(n, ctx->d_gid, seed, ctx->d_par);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->sc));
  ctx->params_set = 1;
  return 0;
}

int h9g_synth_forcing(h9g_ctx *ctx, int slot, uint64_t seed, int day0, int nday) {
  if (!ctx || slot < 0 || slot >= ctx->cfg.nslots || nday < 1 || nday > ctx->cfg.max_days || day0 < 0)
    return H9G_EINVAL;
  HIPCHK(hipSetDevice(ctx->device));
  HIPCHK(hipStreamWaitEvent(ctx->sx, ctx->ev_consumed[slot], 0));
  dim3 grid(nblocks(ctx->n), (unsigned)nday);
  h9g_synth_forcing_kernel<<<grid, H9G_BLOCK, 0, ctx->sx>>>((int)ctx->n, nday, day0, ctx->d_gid, ctx->d_lat, seed,
                                                           (size_t)ctx->cfg.max_days * ctx->n,
                                                           h9g_forcing_slot(ctx, slot));
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->ev_copied[slot], ctx->sx));
  ctx->slot_days[slot] = nday;
  return 0;
}

// INIT.f90:575-631 for one soil layer (0-based) of the context's cells
// (h9g_set_cells).  ts, ks, lm, ps: the layer's 30" fields, (ny*60) rows of
// nx*60 values (row 0 north), device pointers if on_device else host
// (copied through a device staging buffer).  Writes the theta_s, hksat,
// bsw, psi_s rows of the parameters.
int h9g_soil_layer(h9g_ctx *ctx, int layer, const float *ts, const float *ks, const float *lm, const float *ps,
                   int nx, int ny, int on_device) {
  if (!ctx || layer < 0 || layer >= ctx->L || !ts || !ks || !lm || !ps || nx <= 0 || ny <= 0) return H9G_EINVAL;
  if (ctx->h_gid.size() != ctx->n) return H9G_ESTATE;
  for (auto g : ctx->h_gid)
    if (g < 0 || g >= (int64_t)nx * ny) return H9G_EINVAL;
  HIPCHK(hipSetDevice(ctx->device));
  const size_t pitch = (size_t)nx * 60, npix = pitch * (size_t)ny * 60;
  const float *src[4] = {ts, ks, lm, ps};
  float *stage = nullptr;
  if (!on_device) {
    HIPCHK(hipMalloc(&stage, sizeof(float) * 4 * npix));
    for (int k = 0; k < 4; k++) {
      HIPCHK(hipMemcpyAsync(stage + k * npix, src[k], sizeof(float) * npix, hipMemcpyHostToDevice, ctx->sc));
      src[k] = stage + k * npix;
    }
  }
  if (!ctx->d_slow) HIPCHK(hipMalloc(&ctx->d_slow, sizeof(int) * ctx->n));
  HIPCHK(hipMemsetAsync(ctx->d_slow, 0, sizeof(int) * ctx->n, ctx->sc));
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0));
  HIPCHK(hipEventCreate(&e1));
  HIPCHK(hipEventRecord(e0, ctx->sc));
  const int n = (int)ctx->n;
  h9g_soil_kernel<<<n, 64 * H9G_SWAVES, 0, ctx->sc>>>(nx, n, ctx->d_gid, src[0], src[1], src[2], src[3], pitch,
                                                      ctx->L, layer, ctx->d_par, ctx->d_slow);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(e1, ctx->sc));
  h9g_soil_seq_kernel<<<(4 * n + 255) / 256, 256, 0, ctx->sc>>>(nx, n, ctx->d_gid, src[0], src[1], src[2], src[3],
                                                               pitch, ctx->L, layer, ctx->d_par, ctx->d_slow);
  HIPCHK(hipGetLastError());
  std::vector<int> slow(ctx->n);
  HIPCHK(hipMemcpyAsync(slow.data(), ctx->d_slow, sizeof(int) * ctx->n, hipMemcpyDeviceToHost, ctx->sc));
  HIPCHK(hipStreamSynchronize(ctx->sc));
  HIPCHK(hipEventElapsedTime(&ctx->soil_ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (stage) HIPCHK(hipFree(stage));
  ctx->soil_slow = 0;
  for (int v : slow) ctx->soil_slow += v != 0;
  ctx->soil_layers |= 1u << layer;
  return 0;
}

// INIT.f90:661-680 after every layer is built: Fmax of the soiled cells
// (soil_tex > 0, /= 13, SUM(theta_s) > trunc) from the 0.5 deg integer field
// (-9999 -> 3809), NaN elsewhere.  soil_tex, fmax: host (ny, nx) grids.
// The parameters are then complete (h9g_init_state may follow).
int h9g_soil_fmax(h9g_ctx *ctx, const int32_t *soil_tex, const int32_t *fmax, int nx, int ny) {
  if (!ctx || !soil_tex || !fmax || nx <= 0 || ny <= 0) return H9G_EINVAL;
  if (ctx->h_gid.size() != ctx->n || ctx->soil_layers != (1u << ctx->L) - 1) return H9G_ESTATE;
  const size_t n = ctx->n;
  const int L = ctx->L;
  HIPCHK(hipSetDevice(ctx->device));
  std::vector<float> ts((size_t)L * n), fm(n);
  HIPCHK(hipStreamSynchronize(ctx->sc));
  HIPCHK(hipMemcpy(ts.data(), ctx->d_par, sizeof(float) * L * n, hipMemcpyDeviceToHost));
  for (size_t c = 0; c < n; c++) {
    const int64_t g = ctx->h_gid[c];
    if (g < 0 || g >= (int64_t)nx * ny) return H9G_EINVAL;
    float sum = 0.0f;
    for (int i = 0; i < L; i++) sum = sum + ts[(size_t)i * n + c];
    const int tex = soil_tex[g];
    if (tex > 0 && tex != 13 && sum > 1.0E-8f) {
      int v = fmax[g];
      if (v == -9999) v = 3809;
      fm[c] = (float)v / 10000.0f;
    } else {
      fm[c] = __builtin_nanf("");
    }
  }
  HIPCHK(hipMemcpy(ctx->d_par + (size_t)fmax_row(L) * n, fm.data(), sizeof(float) * n, hipMemcpyHostToDevice));
  ctx->params_set = 1;
  return 0;
}

// Device time of the last h9g_soil_layer's block-average kernel, and the
// number of its cells that took the reference-order path.
float h9g_last_soil_ms(h9g_ctx *ctx) { return ctx ? ctx->soil_ms : 0.0f; }
int h9g_last_soil_slow(h9g_ctx *ctx) { return ctx ? ctx->soil_slow : -1; }

int h9g_math_selftest(int device, int n, const float *x, const float *y, float *out) {
  if (n <= 0 || !x || !out) return H9G_EINVAL;
  HIPCHK(hipSetDevice(device));
  float *dx = nullptr, *dy = nullptr, *dout = nullptr;
  HIPCHK(hipMalloc(&dx, sizeof(float) * n));
  HIPCHK(hipMalloc(&dout, sizeof(float) * n));
  HIPCHK(hipMemcpy(dx, x, sizeof(float) * n, hipMemcpyHostToDevice));
  if (y) {
    HIPCHK(hipMalloc(&dy, sizeof(float) * n));
    HIPCHK(hipMemcpy(dy, y, sizeof(float) * n, hipMemcpyHostToDevice));
  }
  h9g_math_kernel<<<(n + 255) / 256, 256>>>(n, dx, dy, dout);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dout, sizeof(float) * n, hipMemcpyDeviceToHost));
  (void)hipFree(dx);
  (void)hipFree(dy);
  (void)hipFree(dout);
  return 0;
}

int h9g_math_fast_selftest(int device, int n, const float *x, const float *y, float *out, int *flag) {
  if (n <= 0 || !x || !out || !flag) return H9G_EINVAL;
  HIPCHK(hipSetDevice(device));
  float *dx = nullptr, *dy = nullptr, *dout = nullptr;
  int *dflag = nullptr;
  HIPCHK(hipMalloc(&dx, sizeof(float) * n));
  HIPCHK(hipMalloc(&dout, sizeof(float) * n));
  HIPCHK(hipMalloc(&dflag, sizeof(int) * n));
  if (y) HIPCHK(hipMalloc(&dy, sizeof(float) * n));
  HIPCHK(hipMemcpy(dx, x, sizeof(float) * n, hipMemcpyHostToDevice));
  if (y) HIPCHK(hipMemcpy(dy, y, sizeof(float) * n, hipMemcpyHostToDevice));
  h9g_math_fast_kernel<<<(n + 255) / 256, 256>>>(n, dx, dy, dout, dflag);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dout, sizeof(float) * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(flag, dflag, sizeof(int) * n, hipMemcpyDeviceToHost));
  (void)hipFree(dx);
  (void)hipFree(dy);
  (void)hipFree(dout);
  (void)hipFree(dflag);
  return 0;
}

int h9g_pace_probe(int device, int nblocks, unsigned *out) {
  if (nblocks <= 0 || !out) return H9G_EINVAL;
  HIPCHK(hipSetDevice(device));
  const size_t nw = (size_t)nblocks * H9G_PWAVES;
  unsigned *dout = nullptr, *darr = nullptr;
  HIPCHK(hipMalloc(&dout, sizeof(unsigned) * 3 * nw));
  HIPCHK(hipMalloc(&darr, sizeof(unsigned)));
  HIPCHK(hipMemset(darr, 0, sizeof(unsigned)));
  const size_t lds = sizeof(float) * (size_t)PairStore<8, H9G_PLANES>::ROWS * H9G_PLANES * H9G_PWAVES +
                     sizeof(uint64_t) * 32 + sizeof(double) * 32 + sizeof(float) * zt_size<8>();
  h9g_pace_probe_kernel<<<nblocks, 64 * H9G_PWAVES, lds>>>(dout, darr, (unsigned)nw, 1ll << 29);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dout, sizeof(unsigned) * 3 * nw, hipMemcpyDeviceToHost));
  (void)hipFree(dout);
  (void)hipFree(darr);
  return 0;
}

int h9g_div_selftest(int device, int n, const float *x, const float *d, float *out, int *flag) {
  if (n <= 0 || !x || !d || !out || !flag) return H9G_EINVAL;
  HIPCHK(hipSetDevice(device));
  float *dx = nullptr, *dd = nullptr, *dout = nullptr;
  int *dflag = nullptr;
  HIPCHK(hipMalloc(&dx, sizeof(float) * n));
  HIPCHK(hipMalloc(&dd, sizeof(float) * n));
  HIPCHK(hipMalloc(&dout, sizeof(float) * n));
  HIPCHK(hipMalloc(&dflag, sizeof(int) * n));
  HIPCHK(hipMemcpy(dx, x, sizeof(float) * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dd, d, sizeof(float) * n, hipMemcpyHostToDevice));
  h9g_div_kernel<<<(n + 255) / 256, 256>>>(n, dx, dd, dout, dflag);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dout, sizeof(float) * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(flag, dflag, sizeof(int) * n, hipMemcpyDeviceToHost));
  (void)hipFree(dx);
  (void)hipFree(dd);
  (void)hipFree(dout);
  (void)hipFree(dflag);
  return 0;
}

// Host build of the synthetic generator (CPU tests pin it to synth.py).
int h9g_synth_host(uint64_t seed, int nlayers, int ncell, const int64_t *gid, const float *lat, int day0,
                   int nday, float *params_out, float *forcing_out) {
  if (ncell < 0 || nlayers < 1 || nlayers > H9G_LMAX) return H9G_EINVAL;
  const size_t n = ncell;
  const int L = nlayers;
  if (params_out) {
    for (size_t c = 0; c < n; c++) {
      for (int l = 0; l < L; l++) {
        float ts, hk, b, ps;
        h9s::params(seed, (uint64_t)gid[c], l, &ts, &hk, &b, &ps);
        params_out[0 * n * L + c * L + l] = ts;
        params_out[1 * n * L + c * L + l] = hk;
        params_out[2 * n * L + c * L + l] = b;
        params_out[3 * n * L + c * L + l] = ps;
      }
      params_out[4 * n * L + c] = h9s::fmax_param(seed, (uint64_t)gid[c]);
    }
  }
  if (forcing_out) {
    for (int d = 0; d < nday; d++)
      for (size_t c = 0; c < n; c++) {
        float v[7];
        h9s::forcing(seed, (uint64_t)gid[c], lat[c], (int64_t)day0 + d, v);
        for (int k = 0; k < 7; k++) forcing_out[(size_t)k * nday * n + (size_t)d * n + c] = v[k];
      }
  }
  return 0;
}

int h9g_land_cells(int nx, int ny, int nland, uint64_t seed, int64_t *gid, float *lat) {
  if (nx <= 0 || ny <= 0 || nland <= 0 || nland > nx * ny || !gid || !lat) return H9G_EINVAL;
  const int64_t ng = (int64_t)nx * ny;
  std::vector<double> score(ng);
  for (int64_t g = 0; g < ng; g++) {
    const double iy = (double)(g / nx);
    const double la = 90.0 - (iy + 0.5) * (180.0 / ny);
    double c = (la + 10.0) / 70.0;
    c = c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
    const double w = la < -60.0 ? 0.15 : (la > 80.0 ? 0.2 : 0.45 + 0.35 * c);
    score[g] = (double)h9s::u01(seed, 1, (uint64_t)g) * w;
  }
  std::vector<int64_t> idx(ng);
  for (int64_t g = 0; g < ng; g++) idx[g] = g;
  std::nth_element(idx.begin(), idx.begin() + nland, idx.end(), [&](int64_t a, int64_t b) {
    return score[a] > score[b] || (score[a] == score[b] && a < b);
  });
  std::sort(idx.begin(), idx.begin() + nland);
  const float dlat = (float)(180.0 / ny);
  for (int i = 0; i < nland; i++) {
    gid[i] = idx[i];
    lat[i] = (90.0f - dlat * 0.5f) - (float)(idx[i] / nx) * dlat;
  }
  return 0;
}

// Host build of the device math, for CPU checks of the shipped object.
float h9g_host_expf(float x) {
  const h9m::Tabs T = {h_exp2tab, h_log2tab};
  return h9m::expf(x, T);
}
float h9g_host_powf(float x, float y) {
  const h9m::Tabs T = {h_exp2tab, h_log2tab};
  return h9m::powf(x, y, T);
}

}  // extern "C"
