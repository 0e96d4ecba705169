// TEST INFRASTRUCTURE ONLY: driver of `make asan` -- every entry point of the device-math probe
// (host build) over in-contract inputs, in one executable with the sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
const char *devmath_backend();
int devmath_exp(const double *x, int n, int table, double *out);
int devmath_exp1(const double *x, int n, double *out);
int devmath_log(const double *x, int n, int table, double *out);
int devmath_log1(const double *x, int n, int table, double *out);
int devmath_sqrt(const double *x, int n, double *out);
int devmath_frozen(const double *d, int n, double *out);
int devmath_div(const double *a, const double *b, int n, double *out);
int devmath_pow13(const double *x, int n, double *out);
int devmath_pow15(const double *x, int n, double *out);
int devmath_chem_fit(const double *TcH, const double *TcL, int n, double *out);
int devmath_chem_formula(const double *TcH, const double *TcL, int n, int table, double *out);
}

static uint64_t state = 0x9e3779b97f4a7c15ull;
static double uniform(double lo, double hi) {
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return lo + (hi - lo) * ((double)(state >> 11) * 0x1p-53);
}

static int failures = 0;
// (want0: the first output as libm has it, to tol relative -- tol < 0: to -tol absolute; NaN: not compared)
static void check(const char *what, int rc, const std::vector<double> &out, double want0, double tol) {
  bool finite = true;
  for (double v : out) finite = finite && std::isfinite(v);
  const bool near = std::isnan(want0) || (tol < 0 ? std::fabs(out[0] - want0) <= -tol
                                                  : std::fabs(out[0] / want0 - 1.0) <= tol);
  if (rc != 0 || !finite || !near) {
    std::printf("devmath: %s: rc %d, finite %d, first %.17g (want %.17g)\n", what, rc, (int)finite, out[0], want0);
    ++failures;
  }
}

int main() {
  const int n = 197;   // three full wavefronts and a partial one
  std::vector<double> x(n), y(n), out;
  auto fill = [&](std::vector<double> &v, double lo, double hi) { for (double &e : v) e = uniform(lo, hi); };

  for (int table = 0; table < 2; ++table) {
    fill(x, -700.0, 700.0);
    out.assign((size_t)50 * n, 0.0);
    check("exp", devmath_exp(x.data(), n, table, out.data()), out, std::exp(x[0]), 1e-15);
    fill(x, -700.0, 700.0);
    for (double &e : x) e = std::exp(e);
    out.assign((size_t)8 * n, 0.0);
    check("log", devmath_log(x.data(), n, table, out.data()), out, std::log(x[0]), 1e-15);
    out.assign(n, 0.0);
    check("log1", devmath_log1(x.data(), n, table, out.data()), out, std::log(x[0]), 1e-15);
    fill(x, -2.0, 45.0); fill(y, -2.0, 45.0);
    out.assign((size_t)12 * n, 0.0);
    check("chem_formula", devmath_chem_formula(x.data(), y.data(), n, table, out.data()), out, NAN, 0.0);
  }
  fill(x, -745.0, 700.0);
  out.assign(n, 0.0);
  check("exp1", devmath_exp1(x.data(), n, out.data()), out, std::exp(x[0]), 1e-15);
  fill(x, 1.0, 4.0);
  out.assign(n, 0.0);
  check("sqrt", devmath_sqrt(x.data(), n, out.data()), out, std::sqrt(x[0]), 1e-15);
  fill(x, -27.0, 27.0);
  out.assign((size_t)5 * n, 0.0);
  check("frozen", devmath_frozen(x.data(), n, out.data()), out, 1.0 - std::erfc(-x[0]) / 2.0, -1e-14);
  fill(x, -10.0, 10.0); fill(y, 1.0, 2.0);
  out.assign((size_t)4 * n, 0.0);
  check("div", devmath_div(x.data(), y.data(), n, out.data()), out, 1.0 / y[0], 1e-15);
  fill(x, 1.0, 1e6);
  out.assign(n, 0.0);
  check("pow13", devmath_pow13(x.data(), n, out.data()), out, std::pow(x[0], -1.0 / 3.0), 1e-15);
  fill(x, 3.2e-4, 1.0);
  out.assign(n, 0.0);
  check("pow15", devmath_pow15(x.data(), n, out.data()), out, std::pow(x[0], -0.2), 1e-15);
  fill(x, -1.4, 14.6); fill(y, 17.9, 33.9);
  out.assign((size_t)12 * n, 0.0);
  check("chem_fit", devmath_chem_fit(x.data(), y.data(), n, out.data()), out, NAN, 0.0);

  if (failures) return 1;
  std::printf("devmath: ok\n");
  return 0;
}
