// h9g_rows.h -- the row layout of the per-cell arrays, and the code that
// reads and writes a cell through it.  Host and device (the product library
// and the host test builds of tests/csrc share it).
//
// Every per-cell array is rows of one value per cell: value r of cell c is
// base[r * stride + c], stride being the cells of the array (the context's
// ncell, or the selection's nsel for a gathered copy).
//
//   state, 4L+9 rows   h2o (h2osoi_liq) at 0, h2o_ma (h2osoi_liq_ma) at L,
//                      smp at 2L, rootr (rootr_col, L+1 rows: the last is
//                      rootr_col(Nlevgrnd) = 0) at 3L, then from 4L+1
//                      zwt wa LAI LAI_litter pm pfm plen rdepth
//   parameters, 4L+1   theta_s hksat bsw psi_s (L rows each), then fmax
//   STOP record, 4     code, day, substep, the value's bits
//   annual means, 12+L the 11 scalars, theta(1..L), theta_total
//   daily line, 11     (include/h9g.h H9G_NDAILY)
//
// The packed form of the ABI and of the oracle (include/h9g.h, h9g_set_state;
// oracle/refcase.py state_fields) holds the same fields in the same order,
// each as (cell, width) with the width fastest: transpose_packed goes from
// one to the other.
#pragma once
#include <stddef.h>
#include "h9g_pair.h"

namespace h9k {

H9K_HD constexpr int h2o_ma_row(int L, int i) { return L + i; }
H9K_HD constexpr int smp_row(int L, int i) { return 2 * L + i; }
H9K_HD constexpr int rootr_row(int L, int i) { return 3 * L + i; }      // i = 0 .. L
H9K_HD constexpr int scalar_row(int L, int k) { return 4 * L + 1 + k; } // k = SC_*
H9K_HD constexpr int state_rows(int L) { return 4 * L + 9; }
H9K_HD constexpr int par_row(int L, int p, int i) { return p * L + i; } // p = PF_TS .. PF_PSI
H9K_HD constexpr int fmax_row(int L) { return 4 * L; }
H9K_HD constexpr int par_rows(int L) { return 4 * L + 1; }
H9K_HD constexpr int annual_rows(int L) { return 12 + L; }
constexpr int STOP_ROWS = 4, DAILY_ROWS = 11;
// the state's scalars in row order; the site path stores the first SC_SITE
enum : int { SC_ZWT = 0, SC_WA, SC_LAI, SC_LAIL, SC_PM, SC_PFM, SC_PLEN, SC_RDEPTH, SC_N, SC_SITE = SC_LAIL + 1 };
constexpr int STATE_FIELDS = 4 + SC_N, PAR_FIELDS = 5;

template <int L>
struct Rows {
  enum : int {
    H2O = 0, H2O_MA = h2o_ma_row(L, 0), SMP = smp_row(L, 0), ROOTR = rootr_row(L, 0),
    SCALARS = scalar_row(L, 0), STATE = state_rows(L), FMAX = fmax_row(L), PAR = par_rows(L),
    ANNUAL = annual_rows(L)
  };
};

// ---- one cell: base pointer st (par), row stride n, column c ----------------
// These are macros, not functions.  The year kernels' machine code is tuned
// and measured; with the same statements in inlined functions the compiler
// ordered their loads and stores differently and allocated other registers
// (profiles/rows_refactor_ab.txt), and the small kernels' register counts
// moved too.  Expanded in place this is the text all of them were compiled
// from.  n and c are the callers' ints, widened where they index.

// parameters, h2o, smp and rootr into a store whose lane holds every layer
// (cs.set_lay) and s; the pair kernel loads by half-pair itself (pair_body)
#define H9K_LOAD_LANE(L, cs, s, par, pn, pc, st, n, c)                                     \
  _Pragma("unroll") for (int p_ = PF_TS; p_ <= PF_PSI; p_++)                               \
    _Pragma("unroll") for (int i_ = 1; i_ <= L; i_++)                                      \
      (cs).set_lay(p_, i_, (par)[(size_t)par_row(L, p_, i_ - 1) * (pn) + (pc)]);           \
  (cs).set_sc(PS_FMAX, (par)[(size_t)Rows<L>::FMAX * (pn) + (pc)]);                        \
  _Pragma("unroll") for (int i_ = 1; i_ <= L; i_++) {                                      \
    (s).h2o[i_] = (st)[(size_t)(Rows<L>::H2O + i_ - 1) * (n) + (c)];                       \
    (s).smp[i_] = (st)[(size_t)(Rows<L>::SMP + i_ - 1) * (n) + (c)];                       \
    (cs).set_lay(PF_ROOTR, i_, (st)[(size_t)(Rows<L>::ROOTR + i_ - 1) * (n) + (c)]);       \
  }
#define H9K_LOAD_SCALARS(L, s, st, n, c)                                                   \
  {                                                                                        \
    const size_t o8_ = (size_t)Rows<L>::SCALARS * (n) + (c);                               \
    (s).zwt = (st)[o8_ + SC_ZWT * (size_t)(n)];                                            \
    (s).wa = (st)[o8_ + SC_WA * (size_t)(n)];                                              \
    (s).LAI = (st)[o8_ + SC_LAI * (size_t)(n)];                                            \
    (s).LAI_litter = (st)[o8_ + SC_LAIL * (size_t)(n)];                                    \
    (s).pm = (st)[o8_ + SC_PM * (size_t)(n)];                                              \
    (s).pfm = (st)[o8_ + SC_PFM * (size_t)(n)];                                            \
    (s).plen = (st)[o8_ + SC_PLEN * (size_t)(n)];                                          \
    (s).rdepth = (st)[o8_ + SC_RDEPTH * (size_t)(n)];                                      \
  }
// h2o, smp and the first `nsc` scalars back (SC_N, or SC_SITE: the site path
// keeps pm pfm plen rdepth); with `grow` the store's rootr rows too
#define H9K_STORE_CELL(L, s, cs, st, n, c, grow, nsc)                                      \
  {                                                                                        \
    const size_t ow_ = (size_t)Rows<L>::SCALARS * (n) + (c);                               \
    _Pragma("unroll") for (int i_ = 1; i_ <= L; i_++) {                                    \
      (st)[(size_t)(Rows<L>::H2O + i_ - 1) * (n) + (c)] = (s).h2o[i_];                     \
      (st)[(size_t)(Rows<L>::SMP + i_ - 1) * (n) + (c)] = (s).smp[i_];                     \
      if (grow) (st)[(size_t)(Rows<L>::ROOTR + i_ - 1) * (n) + (c)] = (cs).lay(PF_ROOTR, i_); \
    }                                                                                      \
    if (grow) (st)[(size_t)(Rows<L>::ROOTR + L) * (n) + (c)] = zero; /* rootr_col(Nlevgrnd) */ \
    (st)[ow_ + SC_ZWT * (size_t)(n)] = (s).zwt;                                            \
    (st)[ow_ + SC_WA * (size_t)(n)] = (s).wa;                                              \
    (st)[ow_ + SC_LAI * (size_t)(n)] = (s).LAI;                                            \
    (st)[ow_ + SC_LAIL * (size_t)(n)] = (s).LAI_litter;                                    \
    if ((nsc) > SC_SITE) {                                                                 \
      (st)[ow_ + SC_PM * (size_t)(n)] = (s).pm;                                            \
      (st)[ow_ + SC_PFM * (size_t)(n)] = (s).pfm;                                          \
      (st)[ow_ + SC_PLEN * (size_t)(n)] = (s).plen;                                        \
      (st)[ow_ + SC_RDEPTH * (size_t)(n)] = (s).rdepth;                                    \
    }                                                                                      \
  }
// Soil mask (HYBRID9.f90:122-123): SUM(theta_s) > trunc.  A cell without
// soil, or with a STOP record from before the run, does not run and its
// output rows are NaN (nan_rows).  Declares `float sum`.
constexpr float SOIL_TRUNC = 1.0E-8f;
#define H9K_TS_SUM(L, cs, sum) \
  float sum = zero;            \
  _Pragma("unroll") for (int i_ = 1; i_ <= L; i_++) sum = sum + (cs).lay(PF_TS, i_);
// whole cells: `rows` rows (state_rows(L), STOP_ROWS, annual_rows(L)) copied,
// or compared bit for bit into `same`
#define H9K_COPY_CELL(dst, dn, dc, src, sn, sc, rows) \
  for (int r_ = 0; r_ < (rows); r_++) (dst)[(size_t)r_ * (dn) + (dc)] = (src)[(size_t)r_ * (sn) + (sc)]
#define H9K_SAME_CELL(same, a, b, n, c, rows) \
  for (int r_ = 0; r_ < (rows); r_++) same &= row_bits((a)[(size_t)r_ * (n) + (c)]) == row_bits((b)[(size_t)r_ * (n) + (c)])
H9K_HD unsigned row_bits(float v) { return __builtin_bit_cast(unsigned, v); }
H9K_HD unsigned row_bits(int v) { return (unsigned)v; }

H9K_HD void nan_rows(float *base, int rows, size_t n, int c) {
#pragma unroll
  for (int r = 0; r < rows; r++) base[(size_t)r * n + c] = __builtin_nanf("");
}

// the cell's STOP record, and the launch's flag
H9K_HD void stop_write(int *err, int n, int c, int code, int day, int step, float value, int *flag) {
  err[0 * (size_t)n + c] = code;
  err[1 * (size_t)n + c] = day;
  err[2 * (size_t)n + c] = step;
  err[3 * (size_t)n + c] = __builtin_bit_cast(int, value);
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(flag, 1);
#else
  __atomic_fetch_or(flag, 1, __ATOMIC_RELAXED);
#endif
}

// ---- packed <-> rows (host) -------------------------------------------------
// nf fields of widths w[], each packed as (n, w[k]) with the width fastest.
inline void transpose_packed(float *packed, float *rows, size_t n, const int *w, int nf, bool to_rows) {
  size_t off = 0, row = 0;
  for (int k = 0; k < nf; k++) {
    for (size_t c = 0; c < n; c++)
      for (int i = 0; i < w[k]; i++) {
        float &p = packed[off + c * w[k] + i], &r = rows[(row + i) * n + c];
        (to_rows ? r : p) = to_rows ? p : r;
      }
    off += n * w[k];
    row += w[k];
  }
}
inline void state_rows_from_packed(int L, size_t n, const float *packed, float *rows) {
  const int w[STATE_FIELDS] = {L, L, L, L + 1, 1, 1, 1, 1, 1, 1, 1, 1};
  transpose_packed(const_cast<float *>(packed), rows, n, w, STATE_FIELDS, true);
}
inline void state_packed_from_rows(int L, size_t n, const float *rows, float *packed) {
  const int w[STATE_FIELDS] = {L, L, L, L + 1, 1, 1, 1, 1, 1, 1, 1, 1};
  transpose_packed(packed, const_cast<float *>(rows), n, w, STATE_FIELDS, false);
}
inline void par_rows_from_packed(int L, size_t n, const float *packed, float *rows) {
  const int w[PAR_FIELDS] = {L, L, L, L, 1};
  transpose_packed(const_cast<float *>(packed), rows, n, w, PAR_FIELDS, true);
}

}  // namespace h9k
