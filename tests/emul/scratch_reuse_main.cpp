// scratch_reuse_main.cpp -- a stand-alone driver for `make asan` (not run by pytest): the emulation
// sources linked straight into this executable with -fsanitize=address,undefined.  Through the C ABI
// it runs a 5-member core for 16 years, grows, shrinks and reuses the verbs' host-side bookkeeping
// of their scratch (1, 9, 2 metric specifications; score; a pair metric; a series; a per-member
// mix), has the core lay out its device memory anew, does the same again and destroys the core.
// Exit status 0 and no sanitizer report is the result.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/hector_amd.h"

#define CK(call)                                                                  \
  do {                                                                            \
    if ((call) != 0) {                                                            \
      std::fprintf(stderr, "%s:%d: %s\n  %s\n", __FILE__, __LINE__, #call, hx_last_error()); \
      std::exit(1);                                                               \
    }                                                                             \
  } while (0)

namespace {
const int N = 5, Y0 = 1745, Y1 = 1760;

void metrics(hx_core *c, int nspecs) {
  std::vector<hx_metric> specs((size_t)nspecs);
  for (int i = 0; i < nspecs; ++i) {
    hx_metric &m = specs[(size_t)i];
    m.op = i % HX_MET_NOPS; m.year0 = Y0 + i % 4; m.year1 = Y1 - i % 3;
    m.base_year0 = i % 2 ? Y0 : 1; m.base_year1 = i % 2 ? Y0 + 2 + i % 3 : 0;   // odd ones: a reference period
    m.reserved = 0; m.threshold = 0.01 * i;
  }
  std::vector<double> out((size_t)nspecs * N);
  CK(hx_member_metrics(c, "global_tas", specs.data(), nspecs, out.data()));
}

void verbs(hx_core *c, int round) {
  metrics(c, 1); metrics(c, 9); metrics(c, 2);
  const int years[3] = {1750, 1755, 1760};
  const double obs[3] = {0.0, 0.05, 0.1}, sigma[3] = {0.1, 0.1, 0.2};
  double chi2[N];
  int used = 0;
  CK(hx_member_score(c, "global_tas", years, obs, sigma, 3, Y0, Y0 + 4, chi2, &used));
  hx_pair_metric pm = {HX_PMET_SLOPE, Y0, Y1, 1, 0, 1, 0, 0, 0.0};
  double slope[N];
  CK(hx_member_pair_metrics(c, "global_tas", "CO2_concentration", nullptr, 0, 0, &pm, 1, slope));
  hx_series_op op = {};
  op.op = HX_SER_COPY;
  CK(hx_series_define(c, round ? "tas_again" : "tas_copy", "global_tas", &op));
  // a per-member mix of two shared year-vectors over three years, applied by the next run
  const int my[3] = {1750, 1751, 1752};
  const double basis[2 * 3] = {4.0, 4.1, 4.2, 5.0, 5.1, 5.2};
  double coeff[2 * N];
  for (int m = 0; m < N; ++m) { coeff[m] = 0.2 * m; coeff[N + m] = 1.0 - 0.2 * m; }
  CK(hx_setvar_dated_mix(c, "ffi_emissions", my, 3, basis, 2, coeff, nullptr));
  CK(hx_run(c, Y1));
  CK(hx_sync(c));
  metrics(c, 2);
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <scenario>\n", argv[0]); return 2; }
  hx_core *c = nullptr;
  CK(hx_newcore(argv[1], N, 0, &c));
  double S[N];
  for (int m = 0; m < N; ++m) S[m] = 2.5 + 0.25 * m;
  CK(hx_setvar(c, "S", S, N, "degC"));
  const char *outs[] = {"global_tas", "CO2_concentration"};
  CK(hx_set_outputs(c, 2, outs));
  CK(hx_run(c, Y1));
  CK(hx_sync(c));
  verbs(c, 0);
  // a different list of outputs: the next run lays the device memory out anew (free_device)
  const char *more[] = {"global_tas", "CO2_concentration", "RF_tot"};
  CK(hx_set_outputs(c, 3, more));
  CK(hx_run(c, Y1));
  CK(hx_sync(c));
  verbs(c, 1);
  CK(hx_shutdown(c));
  std::puts("scratch_reuse: ok");
  return 0;
}
