// TEST INFRASTRUCTURE ONLY: the row layout header (hybrid9_amd/csrc/h9g_rows.h)
// on the host, for tests/test_rows.py: its packed <-> rows transposition and
// a load-then-store round trip of every cell through St<L> and a FlatStore<L>.
// Never linked into the product library.
#include <stdint.h>
#include <string.h>
#include "../../hybrid9_amd/csrc/h9g_geo.h"
#include "../../hybrid9_amd/csrc/h9g_step.h"
#include "../../hybrid9_amd/csrc/h9g_pair.h"
#include "../../hybrid9_amd/csrc/h9g_rows.h"

using namespace h9k;

extern "C" int h9k_rows_state_size(int L) { return state_rows(L); }
extern "C" void h9k_rows_unpack(int L, int n, const float *packed, float *rows) {
  state_rows_from_packed(L, n, packed, rows);
}
extern "C" void h9k_rows_pack(int L, int n, const float *rows, float *packed) {
  state_packed_from_rows(L, n, rows, packed);
}
extern "C" void h9k_rows_unpack_params(int L, int n, const float *packed, float *rows) {
  par_rows_from_packed(L, n, packed, rows);
}

// Every cell of par (parameter rows of n) and st (state rows of n) loaded,
// then stored: the state into st_out (its first `nscalars` scalars; the
// rootr rows with `rootr`), the store's parameter fields into par_out.  The
// caller pre-fills both outputs: what is not stored keeps its value.
template <int L>
static void roundtrip(int n, const float *par, const float *st, float *par_out, float *st_out, int nscalars,
                      int rootr) {
  for (int c = 0; c < n; c++) {
    float store[FlatStore<L>::N], zt[zt_size<L>()];
    FlatStore<L> cs{store, zt};
    St<L> s;
    H9K_LOAD_LANE(L, cs, s, par, n, c, st, n, c)
    H9K_LOAD_SCALARS(L, s, st, n, c)
    H9K_STORE_CELL(L, s, cs, st_out, n, c, rootr, nscalars)
    for (int p = PF_TS; p <= PF_PSI; p++)
      for (int i = 1; i <= L; i++) par_out[(size_t)par_row(L, p, i - 1) * n + c] = cs.lay(p, i);
    par_out[(size_t)fmax_row(L) * n + c] = cs.sc(PS_FMAX);
  }
}

extern "C" int h9k_rows_roundtrip(int L, int n, const float *par, const float *st, float *par_out, float *st_out,
                                  int nscalars, int rootr) {
  if (L == 8)
    roundtrip<8>(n, par, st, par_out, st_out, nscalars, rootr);
  else if (L == 10)
    roundtrip<10>(n, par, st, par_out, st_out, nscalars, rootr);
  else
    return -1;
  return 0;
}
