// ensemble_post.cpp -- EnsembleCore's post-processing verbs (see ensemble_core.hpp): what is done with
// a finished ensemble on the device.  They read results only: no prepare(), no spinup, the core is not
// dirtied.  First the verbs whose kernels are lane-local, the checks and the resolver of "a per-member
// variable" -- built everywhere --, then the cooperative verbs, which the host-emulation build
// replaces by refusals.
#include "ensemble_core.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

// The host-emulation build has no device object: the lane-local kernels and their launchers are
// compiled here, the one place that may define them.  That build does not compile this file on its
// own: ensemble_core.cpp includes it at its end.
#ifdef HX_HOST_EMULATION
#include "hx_dev_post.h"
#endif

namespace hx {

namespace {
void check_nprobs(const char *fn, int nprobs) {
  if (nprobs < 1 || nprobs > HXQ_MAXP) throw std::runtime_error(std::string(fn) + ": nprobs must lie in 1..16");
}
#ifdef HX_HOST_EMULATION
[[noreturn]] void refuse(const char *fn, bool why = true) {
  throw std::runtime_error(std::string(fn) + " is not available in the host-emulation build" +
                           (why ? " (its kernels are cooperative: LDS atomics and cross-lane operations)" : ""));
}
#endif
}  // namespace

// ---- member scores (hx_dev_post.h) ---------------------------------------------------------------

int EnsembleCore::member_score(const std::string &capability, const int *years, const double *obs,
                               const double *sigma, int n, int base_year0, int base_year1,
                               double *out_host) {
  if (n < 1 || !years || !obs || !out_host)
    throw std::runtime_error("hx_member_score: n < 1 or a null argument");
  const PostSource ps = post_source(capability, "hx_member_score");
  if (ps.v >= 0 && !d_out_[ps.v])
    throw std::runtime_error("variable " + capability + " was not enabled with set_outputs()");
  const int last = scen_.start + ps.last_iy;   // (the source's own valid range: the current date for a recorded output)
  const bool has_base = base_year0 <= base_year1;
  std::vector<int> iy((size_t)n);
  int used = 0;
  for (int i = 0; i < n; ++i) {
    if (years[i] < scen_.start || years[i] > last)
      throw std::runtime_error("hx_member_score: dates must lie between startDate and the current date");
    iy[(size_t)i] = years[i] - scen_.start;
    if (obs[i] == obs[i]) ++used;
  }
  if (has_base && (base_year0 < scen_.start || base_year1 > last))
    throw std::runtime_error("hx_member_score: the reference period must lie between startDate and the current date");
  if (!d_lane_of_member_) throw std::runtime_error("hx_member_score: run the core first");
  sync();
  const size_t nn = (size_t)n, doubles = 2 * nn + (size_t)npad_ + (size_t)n_;
  const size_t bytes = sizeof(double) * doubles + sizeof(int) * nn;
  d_score_.reserve(bytes, *this, "hipMalloc score");
  double *d_obs = d_score_.as<double>(), *d_sig = d_obs + nn, *d_lane = d_sig + nn, *d_mem = d_lane + npad_;
  int *d_iy = reinterpret_cast<int *>(d_mem + n_);
  check(hipMemcpyAsync(d_obs, obs, sizeof(double) * nn, hipMemcpyHostToDevice, stream_), "score obs");
  if (sigma)
    check(hipMemcpyAsync(d_sig, sigma, sizeof(double) * nn, hipMemcpyHostToDevice, stream_), "score sigma");
  check(hipMemcpyAsync(d_iy, iy.data(), sizeof(int) * nn, hipMemcpyHostToDevice, stream_), "score years");
  check(hx_launch_score(ps.block, n_, npad_, d_iy, d_obs, sigma ? d_sig : nullptr, n,
                        has_base ? base_year0 - scen_.start : 1, has_base ? base_year1 - scen_.start : 0,
                        d_lane, stream_), "score kernel");
  check(hx_launch_gather(d_lane, d_lane_of_member_, d_mem, n_, npad_, 1, stream_), "score gather");
  check(hipMemcpyAsync(out_host, d_mem, sizeof(double) * (size_t)n_, hipMemcpyDeviceToHost, stream_), "score fetch");
  check(hipStreamSynchronize(stream_), "score sync");
  return used;
}

int hxq_host_start(const unsigned long long *st, unsigned long long *pre) {
  *pre = 0;
  if (st[3] == 0) return 0;
  const unsigned long long kmin = ~st[0], diff = kmin ^ st[1];
  if (!diff) { *pre = kmin; return 0; }
  int lo = 0;
  while (lo < 64 && (diff >> lo)) ++lo;
  if (lo < 64) *pre = (kmin >> lo) << lo;
  return lo;
}
unsigned long long hxq_host_target(double p, unsigned long long W) {
  const double t = std::ceil(p * (double)W);
  return t < 1.0 ? 1ull : (unsigned long long)t;
}
void hxq_host_pick(int lo, const unsigned long long *hist, unsigned long long *prefix,
                   unsigned long long *rem) {
  const int shift = lo >= 8 ? lo - 8 : 0;
  unsigned long long cum = 0, bin = 255;
  for (unsigned long long b = 0; b < 256; ++b) {
    if (cum + hist[b] >= *rem) { bin = b; break; }
    cum += hist[b];
  }
  *prefix = (*prefix & ~(255ull << shift)) | (bin << shift);
  *rem -= cum;
}
double hxq_key_to_double(unsigned long long key) {
  const unsigned long long b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  double x;
  std::memcpy(&x, &b, sizeof x);
  return x;
}

const double *EnsembleCore::q_check(const std::string &capability, int year0, int year1, int nprobs,
                                    const char *fn) {
  const std::string f(fn);
  check_nprobs(fn, nprobs);
  const PostSource ps = post_source(capability, fn);
  const int v = ps.v;
  const bool is_q = f == "hx_ensemble_quantiles";   // (its messages stay as they were)
  if (v >= 0 && (is_q ? !d_out_[v] : !out_enabled_[v]))
    throw std::runtime_error((is_q ? std::string() : f + ": ") + "variable " + capability +
                             " was not enabled with set_outputs()");
  if (year0 < scen_.start || year1 > scen_.start + ps.last_iy || year1 < year0)
    throw std::runtime_error(f + ": dates must lie between startDate and the current date");
  if (!d_lane_of_member_ || !ps.block) throw std::runtime_error(f + ": run the core first");
  if (const char *e = std::getenv("HECTOR_AMD_POST_AB")) post_flags_ = std::atoi(e);
  return ps.block;
}

// ---- per-member metrics, their quantiles, and bin probabilities ----------------------------------

int EnsembleCore::metric_check(const std::string &capability, const hx_metric *specs, int nspecs,
                               const char *fn, const double **src) {
  const std::string f(fn);
  if (nspecs < 1 || nspecs > HX_MET_MAX_SPECS || !specs)
    throw std::runtime_error(f + ": nspecs must lie in 1..32");
  const PostSource ps = post_source(capability, fn);
  const int v = ps.v;
  if (v >= 0 && !out_enabled_[v])
    throw std::runtime_error(f + ": variable " + capability + " was not enabled with set_outputs()");
  const int last = scen_.start + ps.last_iy;   // (the source's own valid range)
  for (int i = 0; i < nspecs; ++i) {
    const hx_metric &m = specs[i];
    const std::string which = " (specification " + std::to_string(i) + ")";
    if (m.op < 0 || m.op >= HX_MET_NOPS) throw std::runtime_error(f + ": unknown op" + which);
    if (m.year1 < m.year0) throw std::runtime_error(f + ": year1 < year0" + which);
    if (m.year0 < scen_.start || m.year1 > last)
      throw std::runtime_error(f + ": the window must lie between startDate and the current date" + which);
    if (m.base_year0 <= m.base_year1 && (m.base_year0 < scen_.start || m.base_year1 > last))
      throw std::runtime_error(f + ": the reference period must lie between startDate and the current date" + which);
    if ((m.op == HX_MET_FIRST_GE || m.op == HX_MET_COUNT_GE) && !(m.threshold == m.threshold))
      throw std::runtime_error(f + ": the threshold is NaN" + which);
  }
  if (!d_lane_of_member_ || !ps.block) throw std::runtime_error(f + ": run the core first");
  *src = ps.block;
  return v;
}

namespace {
// the ascending union of [lo, hi] ranges, padded to a multiple of HXM_BATCH, appended to rows
void append_rows(const std::vector<std::pair<int, int>> &ranges, std::vector<int> &rows, int *first, int *count) {
  std::vector<int> u;
  for (const auto &r : ranges) for (int y = r.first; y <= r.second; ++y) u.push_back(y);
  std::sort(u.begin(), u.end());
  u.erase(std::unique(u.begin(), u.end()), u.end());
  while (!u.empty() && u.size() % HXM_BATCH) u.push_back(u.back() | HXM_PAD);
  for (size_t i = 0; i < u.size(); ++i) if (i && (u[i] & HXM_PAD)) u[i] = (u[i - 1] & (HXM_PAD - 1)) | HXM_PAD;
  *first = (int)rows.size(); *count = (int)u.size();
  rows.insert(rows.end(), u.begin(), u.end());
}
}  // namespace

// the specifications, four to a group in the caller's order, into the device's records and row
// lists; the kernel is queued on stream_ and d_met_ [nspecs rounded up to groups][npad_] returned
const double *EnsembleCore::metric_block(const double *src, const hx_metric *specs, int nspecs) {
  const int ngroups = (nspecs + HXM_GROUP - 1) / HXM_GROUP;
  std::vector<HxMetGroup> groups((size_t)ngroups);
  std::vector<int> rows;
  for (int gi = 0; gi < ngroups; ++gi) {
    HxMetGroup &g = groups[(size_t)gi];
    std::memset(&g, 0, sizeof g);
    std::vector<std::pair<int, int>> bases, windows;
    for (int j = 0; j < HXM_GROUP && gi * HXM_GROUP + j < nspecs; ++j) {
      const hx_metric &m = specs[gi * HXM_GROUP + j];
      HxMetSpec &d = g.s[g.nspec++];
      d.op = m.op; d.iy0 = m.year0 - scen_.start; d.iy1 = m.year1 - scen_.start; d.base = -1;
      d.thr = m.threshold; d.mid = 0.5 * (double)(m.year0 + m.year1);
      windows.emplace_back(d.iy0, d.iy1);
      if (m.base_year0 <= m.base_year1) {
        const std::pair<int, int> b(m.base_year0 - scen_.start, m.base_year1 - scen_.start);
        size_t k = 0;
        while (k < bases.size() && bases[k] != b) ++k;
        if (k == bases.size()) { bases.push_back(b); g.b0[k] = b.first; g.b1[k] = b.second; }
        d.base = (int)k;
      }
    }
    g.nbase = (int)bases.size();
    append_rows(bases, rows, &g.brow0, &g.nbrow);
    append_rows(windows, rows, &g.wrow0, &g.nwrow);
  }
  const size_t gbytes = sizeof(HxMetGroup) * groups.size(), rbytes = sizeof(int) * rows.size();
  d_metplan_.reserve(gbytes + rbytes, *this, "hipMalloc metric plan");
  const size_t words = (size_t)ngroups * HXM_GROUP * (size_t)npad_;
  d_met_.reserve(words, *this, "hipMalloc metric block");
  // (stream order: an earlier call's kernel has finished with the plan before this copy lands)
  check(hipMemcpyAsync(d_metplan_.get(), groups.data(), gbytes, hipMemcpyHostToDevice, stream_), "metric groups");
  check(hipMemcpyAsync(d_metplan_.get() + gbytes, rows.data(), rbytes, hipMemcpyHostToDevice, stream_), "metric rows");
  check(hipStreamSynchronize(stream_), "metric plan");   // groups / rows are this call's locals
  check(hx_launch_metric(src, n_, npad_, d_metplan_.get(), ngroups,
                         reinterpret_cast<const int *>(d_metplan_.get() + gbytes), scen_.start, d_met_.get(), stream_),
        "metric kernel");
  return d_met_.get();
}

void EnsembleCore::member_metrics(const std::string &capability, const hx_metric *specs, int nspecs,
                                  double *out_host, const char *fn) {
  const double *src = nullptr;
  metric_check(capability, specs, nspecs, fn, &src);
  if (!out_host) throw std::runtime_error(std::string(fn) + ": null argument");
  sync();
  const double *blk = metric_block(src, specs, nspecs);
  // member order through the score scratch: [nspecs][n_]
  const size_t bytes = sizeof(double) * (size_t)nspecs * (size_t)n_;
  d_score_.reserve(bytes, *this, "hipMalloc score");
  double *d_mem = d_score_.as<double>();
  check(hx_launch_gather(blk, d_lane_of_member_, d_mem, n_, npad_, nspecs, stream_), "metric gather");
  check(hipMemcpyAsync(out_host, d_mem, bytes, hipMemcpyDeviceToHost, stream_), "metric fetch");
  check(hipStreamSynchronize(stream_), "metric sync");
}

// ---- pair metrics: two series of the same member (hx_member_pair_metrics and its siblings) --------

void EnsembleCore::pair_metric_check(const std::string &cap_a, const PairCall &pc, const char *fn,
                                     const double **src_a, const double **src_b) {
  const std::string f(fn);
  if (pc.nspecs < 1 || pc.nspecs > HX_PMET_MAX_SPECS || !pc.specs)
    throw std::runtime_error(f + ": nspecs must lie in 1..32");
  if ((pc.cap_b != nullptr) == (pc.b_vec != nullptr))
    throw std::runtime_error(f + ": operand b is exactly one of cap_b (a per-member variable) and b_vec (a "
                             "per-year vector): " + (pc.cap_b ? "both were given" : "neither was given"));
  if (pc.b_vec) {
    if (pc.b_year1 < pc.b_year0) throw std::runtime_error(f + ": b_year1 < b_year0");
    for (int y = pc.b_year0; y <= pc.b_year1; ++y)
      if (!std::isfinite(pc.b_vec[y - pc.b_year0]))
        throw std::runtime_error(f + ": b_vec is not finite in " + std::to_string(y));
  }
  auto operand = [&](const std::string &cap) {
    const PostSource ps = post_source(cap, fn);
    if (ps.v >= 0 && !out_enabled_[ps.v])
      throw std::runtime_error(f + ": variable " + cap + " was not enabled with set_outputs()");
    return ps;
  };
  PostSource pa = operand(cap_a), pb{nullptr, 0, -1};
  if (pc.cap_b) {
    pb = operand(pc.cap_b);
    pa = operand(cap_a);   // (two derived blocks are kept: b's has not displaced a's)
  }
  // the years where both operands hold values
  const int a_last = scen_.start + pa.last_iy;
  const int b_first = pc.b_vec ? pc.b_year0 : scen_.start;
  const int b_last = pc.b_vec ? pc.b_year1 : scen_.start + pb.last_iy;
  const int first = std::max(scen_.start, b_first), last = std::min(a_last, b_last);
  const std::string range = pc.b_vec ? "startDate, the current date and b_year0..b_year1"
                                     : "startDate and the current date";
  for (int i = 0; i < pc.nspecs; ++i) {
    const hx_pair_metric &m = pc.specs[i];
    const std::string which = " (specification " + std::to_string(i) + ")";
    if (m.op < 0 || m.op >= HX_PMET_NOPS) throw std::runtime_error(f + ": unknown op" + which);
    if (m.year1 < m.year0) throw std::runtime_error(f + ": year1 < year0" + which);
    if (m.year0 < first || m.year1 > last)
      throw std::runtime_error(f + ": the window must lie between " + range + which);
    if (m.base_a0 <= m.base_a1 && (m.base_a0 < scen_.start || m.base_a1 > a_last))
      throw std::runtime_error(f + ": the reference period of a must lie between startDate and the current date" +
                               which);
    if (m.base_b0 <= m.base_b1 && (m.base_b0 < b_first || m.base_b0 < scen_.start || m.base_b1 > b_last))
      throw std::runtime_error(f + ": the reference period of b must lie between " + range + which);
    if ((m.op == HX_PMET_AT_FIRST_GE || m.op == HX_PMET_MEAN_WHERE_GE) && !(m.threshold == m.threshold))
      throw std::runtime_error(f + ": the threshold is NaN" + which);
  }
  if (!d_lane_of_member_ || !pa.block || (pc.cap_b && !pb.block)) throw std::runtime_error(f + ": run the core first");
  *src_a = pa.block;
  *src_b = pb.block;
}

// the specifications (and the vector operand, indexed from b_year0) into the metric plan scratch; the
// kernel is queued on stream_ and d_met_ [nspecs][npad_] returned
const double *EnsembleCore::pair_metric_block(const double *src_a, const double *src_b, const PairCall &pc) {
  const int nspecs = pc.nspecs;
  std::vector<HxPairSpec> recs((size_t)nspecs);
  for (int i = 0; i < nspecs; ++i) {
    const hx_pair_metric &m = pc.specs[i];
    HxPairSpec &d = recs[(size_t)i];
    d.op = m.op; d.iy0 = m.year0 - scen_.start; d.iy1 = m.year1 - scen_.start; d.pad = 0; d.thr = m.threshold;
    d.a0 = 1; d.a1 = 0; d.b0 = 1; d.b1 = 0;
    if (m.base_a0 <= m.base_a1) { d.a0 = m.base_a0 - scen_.start; d.a1 = m.base_a1 - scen_.start; }
    if (m.base_b0 <= m.base_b1) { d.b0 = m.base_b0 - scen_.start; d.b1 = m.base_b1 - scen_.start; }
  }
  const size_t sbytes = sizeof(HxPairSpec) * recs.size();
  const size_t vbytes = pc.b_vec ? sizeof(double) * (size_t)(pc.b_year1 - pc.b_year0 + 1) : 0;
  d_metplan_.reserve(sbytes + vbytes, *this, "hipMalloc pair-metric plan");
  const size_t words = (size_t)nspecs * (size_t)npad_;
  d_met_.reserve(words, *this, "hipMalloc pair-metric block");
  // (stream order: an earlier call's kernel has finished with the plan before this copy lands)
  check(hipMemcpyAsync(d_metplan_.get(), recs.data(), sbytes, hipMemcpyHostToDevice, stream_), "pair-metric specifications");
  if (vbytes)
    check(hipMemcpyAsync(d_metplan_.get() + sbytes, pc.b_vec, vbytes, hipMemcpyHostToDevice, stream_), "pair-metric vector");
  check(hipStreamSynchronize(stream_), "pair-metric plan");   // recs is this call's local, b_vec the caller's
  check(hx_launch_pair_metric(src_a, src_b, vbytes ? reinterpret_cast<const double *>(d_metplan_.get() + sbytes) : nullptr,
                              pc.b_year0 - scen_.start, n_, npad_, d_metplan_.get(), nspecs, d_met_.get(), stream_),
        "pair-metric kernel");
  return d_met_.get();
}

void EnsembleCore::member_pair_metrics(const std::string &cap_a, const PairCall &pc, double *out_host,
                                       size_t row_pitch) {
  const char *fn = "hx_member_pair_metrics";
  const double *sa = nullptr, *sb = nullptr;
  pair_metric_check(cap_a, pc, fn, &sa, &sb);
  if (!out_host) throw std::runtime_error(std::string(fn) + ": null argument");
  sync();
  const double *blk = pair_metric_block(sa, sb, pc);
  // member order through the score scratch: [nspecs][n_]
  const size_t row = sizeof(double) * (size_t)n_, bytes = row * (size_t)pc.nspecs;
  d_score_.reserve(bytes, *this, "hipMalloc score");
  double *d_mem = d_score_.as<double>();
  check(hx_launch_gather(blk, d_lane_of_member_, d_mem, n_, npad_, pc.nspecs, stream_), "pair-metric gather");
  check(hipMemcpy2DAsync(out_host, sizeof(double) * (row_pitch ? row_pitch : (size_t)n_), d_mem, row, row,
                         (size_t)pc.nspecs, hipMemcpyDeviceToHost, stream_), "pair-metric fetch");
  check(hipStreamSynchronize(stream_), "pair-metric sync");
}

// ---- the checks of the cooperative verbs that check before they run (or, in the host-emulation
// build, before they refuse) ----------------------------------------------------------------------

const double *EnsembleCore::rows_check(const RowSource &rs, const Groups &g, int nprobs, const double **src_b) {
#ifdef HX_HOST_EMULATION
  if (!rs.pair && !g.ngroups) refuse(rs.fn);
#endif
  const double *src = nullptr, *sb = nullptr;
  if (!rs.specs && !rs.pair) {
    src = q_check(rs.capability, rs.year0, rs.year1, nprobs, rs.fn);
  } else {
    if (rs.pair) pair_metric_check(rs.capability, *rs.pair, rs.fn, &src, &sb);
    else metric_check(rs.capability, rs.specs, rs.nspecs, rs.fn, &src);
    check_nprobs(rs.fn, nprobs);
    if (const char *e = std::getenv("HECTOR_AMD_POST_AB")) post_flags_ = std::atoi(e);
  }
#ifdef HX_HOST_EMULATION
  refuse(rs.fn);
#endif
  if (src_b) *src_b = sb;
  return src;
}

// the variable of a verb over listed years resolved, years[n] and the reference period held to its range
EnsembleCore::PostSource EnsembleCore::listed_source(const std::string &f, const std::string &capability,
                                                     const int *years, int n, int base_year0, int base_year1) {
  const PostSource ps = post_source(capability, f.c_str());
  if (ps.v >= 0 && !d_out_[ps.v])
    throw std::runtime_error(f + ": variable " + capability + " was not enabled with set_outputs()");
  const int last = scen_.start + ps.last_iy;
  for (int i = 0; i < n; ++i)
    if (years[i] < scen_.start || years[i] > last)
      throw std::runtime_error(f + ": dates must lie between startDate and the current date");
  if (base_year0 <= base_year1 && (base_year0 < scen_.start || base_year1 > last))
    throw std::runtime_error(f + ": the reference period must lie between startDate and the current date");
  if (!d_lane_of_member_ || !ps.block) throw std::runtime_error(f + ": run the core first");
  return ps;
}

EnsembleCore::PostSource EnsembleCore::whitened_check(const std::string &capability, const int *years,
                                                      const double *obs, const double *whiten, int n,
                                                      int base_year0, int base_year1, const double *out_host) {
  const std::string f = "hx_member_score_whitened";
  if (!years || !obs || !whiten || !out_host) throw std::runtime_error(f + ": null argument");
  if (n < 1 || n > HX_SCORE_WHITENED_MAX) throw std::runtime_error(f + ": n must lie in 1..256");
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(obs[i]))
      throw std::runtime_error(f + ": an observation is NaN or infinite (there is no skipping: drop the "
                                   "year and factorise the remaining covariance)");
  for (int i = 0; i < n; ++i)
    for (int k = 0; k <= i; ++k)
      if (!std::isfinite(whiten[(size_t)i * n + k]))
        throw std::runtime_error(f + ": an entry of whiten on or below the diagonal is NaN or infinite");
  return listed_source(f, capability, years, n, base_year0, base_year1);
}

EnsembleCore::PostSource EnsembleCore::project_check(const std::string &capability, const int *years,
                                                     const double *center, const double *basis, int n, int m,
                                                     int base_year0, int base_year1, const double *out_host) {
  const std::string f = "hx_member_project";
  if (!years || !basis || !out_host) throw std::runtime_error(f + ": null argument");
  if (n < 1 || n > HX_PROJECT_MAX_YEARS) throw std::runtime_error(f + ": n must lie in 1..1024");
  if (m < 1 || m > HX_PROJECT_MAX_OUT) throw std::runtime_error(f + ": m must lie in 1..64");
  if (center)
    for (int i = 0; i < n; ++i)
      if (!std::isfinite(center[i]))
        throw std::runtime_error(f + ": an entry of center is NaN or infinite (there is no skipping)");
  for (size_t i = 0; i < (size_t)m * (size_t)n; ++i)
    if (!std::isfinite(basis[i])) throw std::runtime_error(f + ": an entry of basis is NaN or infinite");
  return listed_source(f, capability, years, n, base_year0, base_year1);
}

// ---- the resolver of the verbs, and series (hx_series_define in hector_amd.h) ----------------------

namespace {
// whole-surface values: area-weighted low / high latitude (ocean_component.cpp:466-503)
const char *const kCombos[][3] = {{"pH", "LL_pH", "HL_pH"}, {"PCO2", "LL_PCO2", "HL_PCO2"},
                                  {"DIC", "LL_DIC", "HL_DIC"}, {"CO3", "LL_CO3", "HL_CO3"},
                                  {"ML_ocean_c", "LL_ocean_c", "HL_ocean_c"}};
const char *const *combo_of(const std::string &name) {
  for (auto &c : kCombos) if (name == c[0]) return c;
  return nullptr;
}
}  // namespace

int EnsembleCore::find_series(const std::string &name) const {
  for (size_t i = 0; i < series_.size(); ++i) if (series_[i].name == name) return (int)i;
  return -1;
}

void EnsembleCore::free_series() {
  for (Series &s : series_) if (s.block) (void)hipFree(s.block);
  series_.clear();
  if (d_ser_vec_) (void)hipFree(d_ser_vec_);
  if (d_ser_perm_) (void)hipFree(d_ser_perm_);
  if (d_expr_) (void)hipFree(d_expr_);
  d_ser_vec_ = nullptr; d_ser_perm_ = nullptr; d_expr_ = nullptr; d_expr_words_ = 0;
}

void EnsembleCore::free_derived_cache() {
  for (DerivedBlock &b : derived_cache_) {
    if (b.block) (void)hipFree(b.block);
    b.block = nullptr; b.name.clear(); b.epoch = 0; b.used = 0;
  }
  if (d_ps_tmp_) (void)hipFree(d_ps_tmp_);
  d_ps_tmp_ = nullptr;
}

// A series is stored in the lane order of its definition (or of its last use).  If the core has
// reordered its lanes since -- assign_lanes() through a changed sorting switch, a newly varying
// parameter or the measured-cost calibration -- the block is permuted on the device, once, before it
// is read: new lane l holds member member_of_lane_[l], whose row sat in the old lane
// lane_of_member[that member].
void EnsembleCore::series_to_current_lanes(Series &s) {
  if (s.lane_of_member == lane_of_member_) return;
  const size_t np = (size_t)npad_, ns = (size_t)scen_.ns();
  std::vector<int> src_lane(np);
  for (size_t l = 0; l < np; ++l) src_lane[l] = s.lane_of_member[(size_t)member_of_lane_[l]];
  if (!d_ser_perm_) check(hipMalloc(&d_ser_perm_, sizeof(int) * np), "hipMalloc series lane map");
  double *dst = nullptr;
  if (hipMalloc(&dst, sizeof(double) * ns * np) != hipSuccess || !dst) {
    (void)hipGetLastError();
    throw std::runtime_error("series " + s.name + ": no device memory to move it to the core's new lane "
                             "order (" + std::to_string((sizeof(double) * ns * np) >> 20) + " MiB)");
  }
  try {
    check(hipMemcpy(d_ser_perm_, src_lane.data(), sizeof(int) * np, hipMemcpyHostToDevice), "series lane map");
    check(hx_launch_series_permute(s.block, d_ser_perm_, npad_, (int)ns, dst, stream_), "series permute kernel");
    check(hipStreamSynchronize(stream_), "series permute");
  } catch (...) { (void)hipFree(dst); throw; }
  (void)hipFree(s.block);
  s.block = dst;
  s.lane_of_member = lane_of_member_;
}

// The kept block of a derived diagnostic (not the slr family: d_slr_ holds it whole) or of a
// whole-surface combination, rows 0..last_iy_, computed on stream_.  Two blocks, the one used longest
// ago is given up; a block stands while out_epoch_ does (no run, reset or new layout since).
const double *EnsembleCore::derived_block(const std::string &capability) {
  for (DerivedBlock &b : derived_cache_)
    if (b.block && b.epoch == out_epoch_ && b.name == capability) { b.used = ++derived_clock_; return b.block; }
  DerivedBlock *slot = nullptr;
  for (DerivedBlock &b : derived_cache_) if (b.name == capability) slot = &b;
  if (!slot) for (DerivedBlock &b : derived_cache_) if (!b.block && !slot) slot = &b;
  if (!slot) slot = derived_cache_[0].used <= derived_cache_[1].used ? &derived_cache_[0] : &derived_cache_[1];
  const size_t np = (size_t)npad_, ns = (size_t)scen_.ns();
  slot->name.clear(); slot->epoch = 0;
  if (!slot->block) check(hipMalloc(&slot->block, sizeof(double) * ns * np), "hipMalloc derived block");
  const int ny = last_iy_ + 1;
  if (const char *const *c = combo_of(capability)) {
    // the order fetchvars() uses on the host: part_low * ll + part_high * hl; ML_ocean_c: ll + hl
    const double *part[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; ++k) {
      const std::string name = c[1 + k];
      if (derived_kind(name) >= 0) {
        if (!d_ps_tmp_) check(hipMalloc(&d_ps_tmp_, sizeof(double) * 2 * ns * np), "hipMalloc combination parts");
        compute_derived(name, 0, ny, d_ps_tmp_ + (size_t)k * ns * np);
        part[k] = d_ps_tmp_ + (size_t)k * ns * np;
      } else {
        const int v = out_index(name);
        if (!d_out_[v])
          throw std::runtime_error("variable " + capability + " needs " + name + ": enable it (or " +
                                   capability + ") with set_outputs()");
        part[k] = d_out_[v];
      }
    }
    const bool sum = capability == "ML_ocean_c";
    const double part_high = 0.15, part_low = 1 - 0.15;
    check(hx_launch_series_ew(sum ? HX_SER_ADD : HXS_COMBINE, part[0], part[1], nullptr, nullptr, npad_, (int)ns,
                              0, last_iy_, part_low, part_high, slot->block, stream_), "combination kernel");
  } else {
    compute_derived(capability, 0, ny, slot->block);
  }
  slot->name = capability; slot->epoch = out_epoch_; slot->used = ++derived_clock_;
  return slot->block;
}

EnsembleCore::PostSource EnsembleCore::post_source(const std::string &capability, const char *fn) {
  const std::string f(fn);
  const int si = find_series(capability);
  if (si >= 0) {
    Series &s = series_[(size_t)si];
    series_to_current_lanes(s);
    return {s.block, s.valid_iy, -1};
  }
  const int dk = derived_kind(capability);   // 0: a diagnostic computed into a block, 1 + i: block i of d_slr_
  if (dk >= 0 || combo_of(capability)) {
    check_component_enabled(capability);
    if (!d_lane_of_member_) throw std::runtime_error(f + ": run the core first");
    if (dk > 0) {
      compute_derived(capability, 0, 0, nullptr);   // d_slr_ up to date
      const size_t np = (size_t)npad_, ns = (size_t)scen_.ns();
      return {d_slr_ + (size_t)(dk - 1) * ns * np, last_iy_, -1};
    }
    return {derived_block(capability), last_iy_, -1};
  }
  int v = -1;
  try {
    v = out_index(capability);
  } catch (const std::runtime_error &e) {
    bool host = false;
    try { host = host_output(capability); } catch (...) {}
    if (host)
      throw std::runtime_error(f + ": variable " + capability + " is the same for every member (fetchvars "
                               "answers it on the host); the per-member verbs take recorded outputs, "
                               "derived diagnostics and series");
    // (the verbs whose messages carried no function name keep them as they were)
    if (f == "hx_ensemble_quantiles" || f == "hx_member_score" || f == "stats" || f == "hx_device_var") throw;
    throw std::runtime_error(f + ": " + e.what());
  }
  return {d_out_[v], last_iy_, v};
}

void EnsembleCore::series_list(std::vector<std::string> *names, std::vector<int> *valid_to) const {
  if (names) names->clear();
  if (valid_to) valid_to->clear();
  for (const Series &s : series_) {
    if (names) names->push_back(s.name);
    if (valid_to) valid_to->push_back(scen_.start + s.valid_iy);
  }
}

void EnsembleCore::series_drop(const std::string &name) {
  const int si = find_series(name);
  if (si < 0) throw std::runtime_error("hx_series_drop: no series named '" + name + "'");
  sync();
  (void)hipFree(series_[(size_t)si].block);
  series_.erase(series_.begin() + si);
}

// a new series' name, or the one it replaces, by the rules of hx_series_define (f: the function named)
int EnsembleCore::series_name_check(const std::string &f, const std::string &name) {
  {  // [A-Za-z_][A-Za-z0-9_]{0,62}
    bool ok = !name.empty() && name.size() <= 63;
    for (size_t i = 0; ok && i < name.size(); ++i) {
      const char c = name[i];
      const bool alpha = (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || c == '_';
      ok = alpha || (i > 0 && c >= '0' && c <= '9');
    }
    if (!ok) throw std::runtime_error(f + ": bad series name '" + name + "' (a letter or _, then up to 62 "
                                      "letters, digits or _)");
  }
  const int existing = find_series(name);
  if (existing < 0) {  // a name the core already answers
    bool answered = derived_kind(name) >= 0 || combo_of(name) || recorded_name(name) ||
                    name == "ocean_timesteps" || name == "N2O_concentration";
    if (!answered) { try { answered = host_output(name); } catch (...) {} }
    if (answered)
      throw std::runtime_error(f + ": '" + name + "' is a variable of the core; a series needs a name of its own");
    if ((int)series_.size() >= HX_SER_MAX)
      throw std::runtime_error(f + ": the core holds " + std::to_string(HX_SER_MAX) + " series already "
                               "(hx_series_drop frees one)");
  }
  return existing;
}

void EnsembleCore::series_define(const std::string &name, const std::string &a_name, const hx_series_op &op) {
  const std::string f = "hx_series_define";
  const int existing = series_name_check(f, name);
  if (op.op < 0 || op.op >= HX_SER_NOPS) throw std::runtime_error(f + ": unknown op " + std::to_string(op.op));
  const bool binary = op.op >= HX_SER_ADD && op.op <= HX_SER_DIV;
  const int ns = scen_.ns();
  if (binary) {
    if (op.b_kind == HX_SER_B_VAR) { if (!op.b) throw std::runtime_error(f + ": operand b is null"); }
    else if (op.b_kind == HX_SER_B_VECTOR) {
      if (!op.b_values || op.b_n < 1) throw std::runtime_error(f + ": the vector operand b is empty");
    } else if (op.b_kind != HX_SER_B_SCALAR)
      throw std::runtime_error(f + ": this op needs an operand b (a variable, a scalar or a per-year vector)");
  }
  if (op.op == HX_SER_RUNMEAN) {
    if (op.width < 1) throw std::runtime_error(f + ": width < 1");
    if (op.width > ns) throw std::runtime_error(f + ": width exceeds the " + std::to_string(ns) + " years of the core");
    if (op.align != HX_SER_TRAILING && op.align != HX_SER_CENTRED) throw std::runtime_error(f + ": unknown align");
  }
  if (op.op == HX_SER_DELTA && (op.lag < 1 || op.lag >= ns))
    throw std::runtime_error(f + ": lag must lie in 1.." + std::to_string(ns - 1));
  if (!d_lane_of_member_ || lane_of_member_.empty()) throw std::runtime_error(f + ": run the core first");
  sync();
  auto operand = [&](const std::string &cap) {
    const PostSource ps = post_source(cap, "hx_series_define");
    if (ps.v >= 0 && !out_enabled_[ps.v])
      throw std::runtime_error(f + ": variable " + cap + " was not enabled with set_outputs()");
    if (!ps.block) throw std::runtime_error(f + ": run the core first");
    return ps;
  };
  const PostSource pa = operand(a_name);
  PostSource pb{nullptr, pa.last_iy, -1};
  if (binary && op.b_kind == HX_SER_B_VAR) pb = operand(op.b);
  // (both operands are in the current lane order now: resolving b does not move a's block -- a
  //  series is permuted at most once per lane order, and a derived a keeps its cache slot: b takes
  //  the other one)
  const int valid = std::min(pa.last_iy, pb.last_iy);
  const int last = scen_.start + pa.last_iy;
  if (op.op == HX_SER_ANOMALY && (op.year1 < op.year0 || op.year0 < scen_.start || op.year1 > last))
    throw std::runtime_error(f + ": the reference period must lie between startDate and " + std::to_string(last) +
                             ", the end of " + a_name);
  if (op.op == HX_SER_CUMSUM && (op.year0 < scen_.start || op.year0 > last))
    throw std::runtime_error(f + ": year0 must lie between startDate and " + std::to_string(last) +
                             ", the end of " + a_name);
  const size_t np = (size_t)npad_;
  if (!d_ser_vec_) check(hipMalloc(&d_ser_vec_, sizeof(double) * ((size_t)ns + np)), "hipMalloc series operand");
  double *d_bvec = d_ser_vec_, *d_base = d_ser_vec_ + ns;
  if (binary && op.b_kind != HX_SER_B_VAR) {
    std::vector<double> bv((size_t)ns, op.b_kind == HX_SER_B_SCALAR ? op.b_scalar : std::nan(""));
    if (op.b_kind == HX_SER_B_VECTOR)
      for (int i = 0; i < op.b_n; ++i) {
        const long long iy = (long long)op.b_first_year + i - scen_.start;
        if (iy >= 0 && iy < ns) bv[(size_t)iy] = op.b_values[i];
      }
    check(hipMemcpy(d_bvec, bv.data(), sizeof(double) * (size_t)ns, hipMemcpyHostToDevice), "series operand");
  }
  double *z = nullptr;
  if (hipMalloc(&z, sizeof(double) * (size_t)ns * np) != hipSuccess || !z) {
    (void)hipGetLastError();
    throw std::runtime_error(f + ": no device memory for the block of series " + name + " (" +
                             std::to_string((sizeof(double) * (size_t)ns * np) >> 20) + " MiB)");
  }
  try {
    switch (op.op) {
      case HX_SER_COPY:
        check(hx_launch_series_ew(HX_SER_COPY, pa.block, nullptr, nullptr, nullptr, npad_, ns, 0, valid, 0.0, 0.0,
                                  z, stream_), "series kernel");
        break;
      case HX_SER_ADD: case HX_SER_SUB: case HX_SER_MUL: case HX_SER_DIV:
        check(hx_launch_series_ew(op.op, pa.block, pb.block, pb.block ? nullptr : d_bvec, nullptr, npad_, ns, 0,
                                  valid, 0.0, 0.0, z, stream_), "series kernel");
        break;
      case HX_SER_ANOMALY:
        check(hx_launch_series_base(pa.block, npad_, op.year0 - scen_.start, op.year1 - scen_.start, d_base,
                                    stream_), "series base kernel");
        check(hx_launch_series_ew(HXS_ANOM_APPLY, pa.block, nullptr, nullptr, d_base, npad_, ns, 0, valid, 0.0,
                                  0.0, z, stream_), "series kernel");
        break;
      case HX_SER_CUMSUM:
        check(hx_launch_series_cumsum(pa.block, npad_, ns, op.year0 - scen_.start, valid, z, stream_),
              "series cumsum kernel");
        break;
      case HX_SER_RUNMEAN:
        check(hx_launch_series_runmean(pa.block, npad_, ns, op.width,
                                       op.align == HX_SER_CENTRED ? (op.width - 1) / 2 : op.width - 1, valid, z,
                                       stream_), "series running-mean kernel");
        break;
      default:  // HX_SER_DELTA: a itself `lag` rows earlier (rows below `lag` are never loaded)
        check(hx_launch_series_ew(HX_SER_SUB, pa.block, pa.block - (size_t)op.lag * np, nullptr, nullptr, npad_,
                                  ns, op.lag, valid, 0.0, 0.0, z, stream_), "series kernel");
        break;
    }
    check(hipStreamSynchronize(stream_), "series sync");   // (the old block of a replaced series is freed below)
  } catch (...) { (void)hipFree(z); throw; }
  Series s;
  s.name = name; s.block = z; s.valid_iy = valid; s.lane_of_member = lane_of_member_;
  if (existing >= 0) {
    (void)hipFree(series_[(size_t)existing].block);
    series_[(size_t)existing] = std::move(s);
  } else {
    series_.push_back(std::move(s));
  }
}

// hx_series_eval: the program is checked and translated before anything is resolved or allocated (a
// refused call changes nothing); the distinct (name, lag) operands the VAR instructions use become
// the kernel's operand table, and every instruction carries the stack depth in front of it.
void EnsembleCore::series_eval(const std::string &name, const hx_expr &ex) {
  const std::string f = "hx_series_eval";
  const int existing = series_name_check(f, name);
  const int ns = scen_.ns();
  auto refuse = [&](const std::string &what) { throw std::runtime_error(f + ": " + what); };
  if (ex.reserved[0] || ex.reserved[1]) refuse("a reserved field of hx_expr is not 0");
  if (ex.nins < 1 || ex.nins > HX_EX_MAX_INS)
    refuse("nins must lie in 1.." + std::to_string(HX_EX_MAX_INS) + " (HX_EX_MAX_INS)");
  if (!ex.ins || (ex.nvars > 0 && !ex.vars) || (ex.nmem > 0 && !ex.members) || (ex.nvec > 0 && !ex.yearvecs))
    refuse("null argument");
  if (ex.nvars < 0 || ex.nvars > HX_EX_MAX_INS || ex.nmem < 0 || ex.nvec < 0) refuse("a negative or oversized table count");
  if (ex.nmem > HX_EX_MAX_MEMBERS)
    refuse("more than " + std::to_string(HX_EX_MAX_MEMBERS) + " member vectors (HX_EX_MAX_MEMBERS)");
  if (ex.nvec > HX_EX_MAX_YEARVECS)
    refuse("more than " + std::to_string(HX_EX_MAX_YEARVECS) + " year vectors (HX_EX_MAX_YEARVECS)");
  for (int k = 0; k < ex.nvars; ++k) {
    if (!ex.vars[k].name) refuse("null argument (the name of vars[" + std::to_string(k) + "])");
    if (ex.vars[k].reserved) refuse("a reserved field of vars[" + std::to_string(k) + "] is not 0");
    if (ex.vars[k].lag < 0 || ex.vars[k].lag >= ns)
      refuse("the lag of " + std::string(ex.vars[k].name) + " must lie in 0.." + std::to_string(ns - 1) +
             ", the years of the core");
  }
  for (int k = 0; k < ex.nmem; ++k)
    if (!ex.members[k]) refuse("member vector " + std::to_string(k) + " is a null pointer");
  for (int k = 0; k < ex.nvec; ++k)
    if (!ex.yearvecs[k].values || ex.yearvecs[k].n < 1) refuse("year vector " + std::to_string(k) + " is empty");
  HxExprProg prog;
  std::memset(&prog, 0, sizeof prog);
  std::vector<int> distinct;   // indices into ex.vars, one per distinct (name, lag) a VAR instruction uses
  int depth = 0, top = 0;
  for (int i = 0; i < ex.nins; ++i) {
    const hx_expr_ins &in = ex.ins[i];
    const std::string at = "instruction " + std::to_string(i);
    if (in.op < 0 || in.op >= HX_EX_NOPS) refuse(at + ": unknown op " + std::to_string(in.op));
    int arg = 0;
    const int pops = in.op <= HX_EX_YEAR ? 0 : in.op <= HX_EX_EXP ? 1 : in.op == HX_EX_WHERE ? 3 : 2;
    if (in.op <= HX_EX_YEARVEC) {
      const int count = in.op == HX_EX_VAR ? ex.nvars : in.op == HX_EX_MEMBER ? ex.nmem : ex.nvec;
      const char *table = in.op == HX_EX_VAR ? "vars" : in.op == HX_EX_MEMBER ? "members" : "yearvecs";
      if (in.arg < 0 || in.arg >= count)
        refuse(at + ": arg " + std::to_string(in.arg) + " is outside the table " + table + " of " +
               std::to_string(count));
      arg = in.arg;
      if (in.op == HX_EX_VAR) {
        size_t k = 0;
        for (; k < distinct.size(); ++k) {
          const hx_expr_var &v = ex.vars[distinct[k]];
          if (v.lag == ex.vars[in.arg].lag && std::strcmp(v.name, ex.vars[in.arg].name) == 0) break;
        }
        if (k == distinct.size()) {
          if ((int)distinct.size() == HX_EX_MAX_VARS)
            refuse("more than " + std::to_string(HX_EX_MAX_VARS) + " distinct (name, lag) operands (HX_EX_MAX_VARS)");
          distinct.push_back(in.arg);
        }
        arg = (int)k;
      }
    }
    if (depth < pops) refuse(at + ": stack underflow (the op takes " + std::to_string(pops) + " values, the stack holds " +
                             std::to_string(depth) + ")");
    prog.ins[i] = (unsigned)in.op | (unsigned)arg << 8 | (unsigned)depth << 16;
    prog.cval[i] = in.op == HX_EX_CONST ? in.value : 0.0;
    depth += 1 - pops;
    if (depth > HX_EX_MAX_STACK)
      refuse(at + ": the stack would hold more than " + std::to_string(HX_EX_MAX_STACK) + " values (HX_EX_MAX_STACK)");
    top = std::max(top, depth);
  }
  if (depth != 1)
    refuse("the program ends with " + std::to_string(depth) + " values on the stack; it must end with exactly one");
  if (distinct.empty()) refuse("the program has no VAR: a series needs a per-member variable");
  // the core keeps two blocks of derived diagnostics / combinations, the one used longest ago is given
  // up for a third: an expression that names more than two has each copied into a block of its own
  // as it is resolved, freed when the call returns
  std::vector<std::string> kept;
  for (int k : distinct) {
    const std::string cap = ex.vars[k].name;
    if (find_series(cap) >= 0 || !(derived_kind(cap) == 0 || combo_of(cap))) continue;
    if (std::find(kept.begin(), kept.end(), cap) == kept.end()) kept.push_back(cap);
  }
  struct Temps {
    std::vector<std::pair<std::string, double *>> blocks;
    ~Temps() { for (auto &b : blocks) (void)hipFree(b.second); }
  } temps;
  if (!d_lane_of_member_ || lane_of_member_.empty()) refuse("run the core first");
  sync();
  int valid = ns - 1;
  for (size_t k = 0; k < distinct.size(); ++k) {
    const std::string cap = ex.vars[distinct[k]].name;
    const PostSource ps = post_source(cap, "hx_series_eval");
    if (ps.v >= 0 && !out_enabled_[ps.v]) refuse("variable " + cap + " was not enabled with set_outputs()");
    if (!ps.block) refuse("run the core first");
    prog.var[k] = ps.block;
    if (kept.size() > 2 && std::find(kept.begin(), kept.end(), cap) != kept.end()) {
      const double *own = nullptr;
      for (auto &b : temps.blocks) if (b.first == cap) own = b.second;
      if (!own) {
        double *t = nullptr;
        if (hipMalloc(&t, sizeof(double) * (size_t)ns * (size_t)npad_) != hipSuccess || !t) {
          (void)hipGetLastError();
          refuse("no device memory for a copy of " + cap + " (" +
                 std::to_string((sizeof(double) * (size_t)ns * (size_t)npad_) >> 20) + " MiB)");
        }
        temps.blocks.emplace_back(cap, t);
        check(hx_launch_series_ew(HX_SER_COPY, ps.block, nullptr, nullptr, nullptr, npad_, ns, 0, ps.last_iy, 0.0, 0.0,
                                  t, stream_), "series kernel");
        check(hipStreamSynchronize(stream_), "series sync");
        own = t;
      }
      prog.var[k] = own;
    }
    prog.lag[k] = ex.vars[distinct[k]].lag;
    valid = std::min(valid, ps.last_iy);
  }
  // (a series among the operands is permuted at most once per lane order and the derived ones keep
  //  their two cache slots: resolving one operand does not move another's block)
  prog.nins = ex.nins; prog.nvar = (int)distinct.size(); prog.nmem = ex.nmem;
  // the record, the member vectors in lane order and the year vectors over the core's years: one copy
  const size_t np = (size_t)npad_, head = (sizeof(HxExprProg) + 7) / 8;
  const size_t words = head + (size_t)ex.nmem * np + (size_t)ex.nvec * (size_t)ns;
  if (words > d_expr_words_) {
    if (d_expr_) (void)hipFree(d_expr_);
    d_expr_ = nullptr; d_expr_words_ = 0;
    check(hipMalloc(&d_expr_, sizeof(double) * words), "hipMalloc expression operands");
    d_expr_words_ = words;
  }
  std::vector<double> stage(words, 0.0);
  for (int k = 0; k < ex.nmem; ++k) {
    double *row = stage.data() + head + (size_t)k * np;
    for (int m = 0; m < n_; ++m) row[(size_t)lane_of_member_[(size_t)m]] = ex.members[k][m];
    prog.mem[k] = d_expr_ + head + (size_t)k * np;
  }
  for (int k = 0; k < ex.nvec; ++k) {
    double *row = stage.data() + head + (size_t)ex.nmem * np + (size_t)k * (size_t)ns;
    for (int y = 0; y < ns; ++y) row[y] = std::nan("");
    for (int i = 0; i < ex.yearvecs[k].n; ++i) {
      const long long iy = (long long)ex.yearvecs[k].first_year + i - scen_.start;
      if (iy >= 0 && iy < ns) row[(size_t)iy] = ex.yearvecs[k].values[i];
    }
    prog.vec[k] = d_expr_ + head + (size_t)ex.nmem * np + (size_t)k * (size_t)ns;
  }
  std::memcpy(stage.data(), &prog, sizeof prog);
  check(hipMemcpy(d_expr_, stage.data(), sizeof(double) * words, hipMemcpyHostToDevice), "expression operands");
  double *z = nullptr;
  if (hipMalloc(&z, sizeof(double) * (size_t)ns * np) != hipSuccess || !z) {
    (void)hipGetLastError();
    throw std::runtime_error(f + ": no device memory for the block of series " + name + " (" +
                             std::to_string((sizeof(double) * (size_t)ns * np) >> 20) + " MiB)");
  }
  try {
    check(hx_launch_series_expr((const HxExprProg *)d_expr_, prog.nvar, prog.nmem, top, npad_, ns, scen_.start,
                                valid, z, stream_), "series expression kernel");
    check(hipStreamSynchronize(stream_), "series sync");
  } catch (...) { (void)hipFree(z); throw; }
  Series s;
  s.name = name; s.block = z; s.valid_iy = valid; s.lane_of_member = lane_of_member_;
  if (existing >= 0) {
    (void)hipFree(series_[(size_t)existing].block);
    series_[(size_t)existing] = std::move(s);
  } else {
    series_.push_back(std::move(s));
  }
}

// ==== the cooperative verbs =========================================================================
// Their kernels exchange data between lanes (LDS atomics, cross-lane operations), which the
// host-emulation build, one lane at a time, cannot run: it has the refusals at the end instead.
#ifndef HX_HOST_EMULATION

// ---- what the summary verbs share: the rows of a source, weights and labels in lane order, the
// rows' records ------------------------------------------------------------------------------------

EnsembleCore::Rows EnsembleCore::rows(const RowSource &rs, const Groups &g, int nprobs) {
  const double *sb = nullptr, *src = rows_check(rs, g, nprobs, &sb);
  sync();
  if (rs.pair) return {pair_metric_block(src, sb, *rs.pair), 0, rs.pair->nspecs};
  if (rs.specs) return {metric_block(src, rs.specs, rs.nspecs), 0, rs.nspecs};
  return {src, rs.year0 - scen_.start, rs.year1 - rs.year0 + 1};
}

const unsigned long long *EnsembleCore::lane_weights(const unsigned long long *q) {
  if (!q) return nullptr;
  if (!d_q_) check(hipMalloc(&d_q_, 8 * (size_t)npad_), "hipMalloc weights");
  std::vector<unsigned long long> ql((size_t)npad_, 0ull);
  for (int m = 0; m < n_; ++m) ql[(size_t)lane_of_member_[(size_t)m]] = q[m];
  check(hipMemcpy(d_q_, ql.data(), 8 * (size_t)npad_, hipMemcpyHostToDevice), "weights");
  return d_q_;
}

int *EnsembleCore::group_labels() {
  if (!d_glab_) check(hipMalloc(&d_glab_, sizeof(int) * ((size_t)npad_ + (size_t)n_)), "hipMalloc group labels");
  check(hipMemsetAsync(d_glab_, 0xff, sizeof(int) * (size_t)npad_, stream_), "group labels");   // -1: in no group
  return d_glab_;
}

void EnsembleCore::upload_labels(const int *labels) {
  int *d_mem = group_labels() + npad_;
  check(hipMemcpyAsync(d_mem, labels, sizeof(int) * (size_t)n_, hipMemcpyHostToDevice, stream_), "group labels");
  check(hx_launch_grp_prepare(d_mem, n_, npad_, d_lane_of_member_, d_glab_, stream_), "group label kernel");
}

// The grouped kernels fill the (group, row) records and sums from one read of every row; the init,
// pick and reduce kernels run over them unchanged.
void EnsembleCore::minmax(const Rows &r, int ngroups, const unsigned long long *dq, unsigned long long *st) {
  check(hipMemsetAsync(st, 0, 8 * 4 * (size_t)std::max(ngroups, 1) * (size_t)r.nrows, stream_), "row records");
  check(ngroups ? hx_launch_gq_minmax(r.block, n_, npad_, r.iy0, r.nrows, dq, d_glab_, ngroups, st, stream_)
                : hx_launch_q_minmax(r.block, n_, npad_, r.iy0, r.nrows, dq, st, stream_), "min/max kernel");
}

// ---- weighted quantiles (hx_ensemble_quantiles) ---------------------------------------------------

namespace {
// d_qstate_ in 8-byte words: [ny][4] row records, [ny][np] prefix, [ny][np] rem, [HXQ_MAXP] probs, [ny] lo (int)
struct QState {
  unsigned long long *st, *prefix, *rem;
  double *probs;
  int *lo;
  size_t words;
  QState(unsigned long long *base, int ny, int np) {
    const size_t y = (size_t)ny, yp = y * (size_t)np;
    st = base; prefix = st + 4 * y; rem = prefix + yp;
    probs = reinterpret_cast<double *>(rem + yp);
    lo = reinterpret_cast<int *>(rem + yp + HXQ_MAXP);
    words = 4 * y + 2 * yp + HXQ_MAXP + (y + 1) / 2;
  }
};
}  // namespace

int EnsembleCore::q_start(const RowSource &rs, const Groups &g, const unsigned long long *q, int np) {
  const Rows r = rows(rs, g, np);
  const int nrows = std::max(g.ngroups, 1) * r.nrows;
  if (g.ngroups) upload_labels(g.labels);
  d_qstate_.reserve(QState(nullptr, nrows, np).words, *this, "hipMalloc quantile state");
  d_qhist_.reserve((size_t)nrows * (size_t)np * 256, *this, "hipMalloc quantile histograms");
  minmax(r, g.ngroups, lane_weights(q), QState(d_qstate_.get(), nrows, np).st);
  q_src_ = r.block; q_iy0_ = r.iy0; q_ny_ = r.nrows; q_np_ = np; q_weighted_ = q != nullptr; q_groups_ = g.ngroups;
  return nrows;
}

void EnsembleCore::q_hist(const int *lo, const unsigned long long *prefix) {
  const unsigned long long *dq = q_weighted_ ? d_q_ : nullptr;
  check(q_groups_ ? hx_launch_gq_hist(q_src_, n_, npad_, q_iy0_, q_ny_, dq, d_glab_, q_groups_, lo, prefix, q_np_,
                                      d_qhist_.get(), stream_)
                  : hx_launch_q_hist(q_src_, n_, npad_, q_iy0_, q_ny_, dq, lo, prefix, q_np_,
                                     (post_flags_ & 2) ? 1 : 0, d_qhist_.get(), stream_),
        "quantile histogram kernel");
}

void EnsembleCore::quantiles(const RowSource &rs, const Groups &g, const unsigned long long *q,
                             const double *probs, int nprobs, double *out_host, long long *n_part) {
  const int ny = q_start(rs, g, q, nprobs), np = nprobs;
  QState s(d_qstate_.get(), ny, np);
  const size_t yp = (size_t)ny * (size_t)np;
  check(hipMemsetAsync(d_qhist_.get(), 0, 8 * yp * 256, stream_), "quantile histograms");
  check(hipMemcpyAsync(s.probs, probs, sizeof(double) * (size_t)np, hipMemcpyHostToDevice, stream_), "quantile probs");
  check(hx_launch_q_init(s.st, ny, s.probs, np, (post_flags_ & 1) ? 0 : 1, s.lo, s.prefix, s.rem, stream_),
        "quantile init kernel");
  // eight 8-bit digits at most; a row whose select has finished makes its workgroups return at once
  // (grouped: when every group of its row has finished)
  for (int pass = 0; pass < 8; ++pass) {
    q_hist(s.lo, s.prefix);
    check(hx_launch_q_pick(ny, s.lo, s.prefix, s.rem, np, d_qhist_.get(), stream_), "quantile pick kernel");
  }
  std::vector<unsigned long long> h((size_t)4 * ny + yp);   // row records, then prefixes: adjacent
  check(hipMemcpyAsync(h.data(), s.st, 8 * h.size(), hipMemcpyDeviceToHost, stream_), "quantile fetch");
  check(hipStreamSynchronize(stream_), "quantile sync");
  for (int y = 0; y < ny; ++y) {
    const unsigned long long cnt = h[(size_t)4 * y + 3];
    if (n_part) n_part[y] = (long long)cnt;
    for (int j = 0; j < np; ++j)
      out_host[(size_t)y * np + j] = cnt ? hxq_key_to_double(h[(size_t)4 * ny + (size_t)y * np + j]) : std::nan("");
  }
}

void EnsembleCore::q_begin(const RowSource &rs, const Groups &g, const unsigned long long *q, int nprobs,
                           unsigned long long *st_host) {
  const int ny = q_start(rs, g, q, nprobs);
  check(hipMemcpyAsync(st_host, QState(d_qstate_.get(), ny, nprobs).st, 8 * 4 * (size_t)ny, hipMemcpyDeviceToHost,
                       stream_), "quantile fetch");
  check(hipStreamSynchronize(stream_), "quantile sync");
}

void EnsembleCore::q_pass(const int *lo, const unsigned long long *prefix, unsigned long long *hist_host) {
  if (!q_src_) throw std::runtime_error("quantile pass without q_begin");
  const int rows = std::max(q_groups_, 1) * q_ny_;
  QState s(d_qstate_.get(), rows, q_np_);
  const size_t yp = (size_t)rows * (size_t)q_np_;
  check(hipMemcpyAsync(s.lo, lo, sizeof(int) * (size_t)rows, hipMemcpyHostToDevice, stream_), "quantile lo");
  check(hipMemcpyAsync(s.prefix, prefix, 8 * yp, hipMemcpyHostToDevice, stream_), "quantile prefix");
  check(hipMemsetAsync(d_qhist_.get(), 0, 8 * yp * 256, stream_), "quantile histograms");
  q_hist(s.lo, s.prefix);
  check(hipMemcpyAsync(hist_host, d_qhist_.get(), 8 * yp * 256, hipMemcpyDeviceToHost, stream_), "quantile fetch");
  check(hipStreamSynchronize(stream_), "quantile sync");
}

// ---- weighted bin probabilities (hx_ensemble_probabilities) ----------------------------------------

void EnsembleCore::bin_sums(const RowSource &rs, const Groups &g, const unsigned long long *q, const double *edges,
                            int nedges, unsigned long long *sums_host) {
  const Rows r = rows(rs, g, 1);
  if (g.ngroups) upload_labels(g.labels);
  const unsigned long long *dq = lane_weights(q);
  const size_t words = 32 + (size_t)std::max(g.ngroups, 1) * (size_t)r.nrows * (size_t)(nedges + 2);
  d_bin_.reserve(words, *this, "hipMalloc bin sums");
  double *d_edges = reinterpret_cast<double *>(d_bin_.get());
  unsigned long long *d_sums = d_bin_.get() + 32;
  check(hipMemcpyAsync(d_edges, edges, sizeof(double) * (size_t)nedges, hipMemcpyHostToDevice, stream_), "bin edges");
  check(hipMemsetAsync(d_sums, 0, 8 * (words - 32), stream_), "bin sums");
  check(g.ngroups ? hx_launch_gbin(r.block, n_, npad_, r.iy0, r.nrows, dq, d_glab_, g.ngroups, d_edges, nedges,
                                   d_sums, stream_)
                  : hx_launch_bin(r.block, n_, npad_, r.iy0, r.nrows, dq, d_edges, nedges, d_sums, stream_),
        "bin kernel");
  check(hipMemcpyAsync(sums_host, d_sums, 8 * (words - 32), hipMemcpyDeviceToHost, stream_), "bin fetch");
  check(hipStreamSynchronize(stream_), "bin sync");
}

// ---- weighted moments and cross moments with predictors (hx_ensemble_moments) ----------------------

namespace {
// d_mom_ in 8-byte words: the call's weights and predictors in member order and in lane order, the
// groups' predictor shifts, the rows' records and shifts, the chunks' partial sums and the sums; for
// a grouped call (ngroups > 0, ny = ngroups * nrows) the labels in member order behind them, two to
// a word
struct MomBuf {
  unsigned long long *q_mem, *q_lane, *st;
  double *pred_mem, *c, *qd_lane, *e_lane, *shift, *part, *out;
  int *lab_mem;
  size_t words, lane_words;
  MomBuf(unsigned long long *base, int n, int npad, int npred, int ny, int nchunks, int ngroups) {
    const size_t N = (size_t)n, P = (size_t)npad, K = (size_t)npred, Y = (size_t)ny;
    const size_t nc = 2 + 3 * K, G = (size_t)std::max(ngroups, 1);
    q_lane = base;                                             // [npad]  } zeroed before the prepare
    qd_lane = reinterpret_cast<double *>(q_lane + P);          // [npad]  } kernel: padding lanes
    e_lane = qd_lane + P;                                      // [npred][npad] } take no part
    lane_words = (2 + K) * P;
    q_mem = base + lane_words;                                 // [n]
    pred_mem = reinterpret_cast<double *>(q_mem + N);          // [npred][n]
    c = pred_mem + K * N;                                      // [G][8]
    st = reinterpret_cast<unsigned long long *>(c + 8 * G);    // [ny][4]
    shift = reinterpret_cast<double *>(st + 4 * Y);            // [ny]
    part = shift + Y;                                          // [ny][nchunks][nc]
    out = part + Y * (size_t)nchunks * nc;                     // [ny][nc]
    lab_mem = reinterpret_cast<int *>(out + Y * nc);           // [n], grouped only
    words = lane_words + N + K * N + 8 * G + 5 * Y + Y * (size_t)nchunks * nc + Y * nc + (ngroups ? (N + 1) / 2 : 0);
  }
};
}  // namespace

void EnsembleCore::mom_begin(const RowSource &rs, const Groups &g, const unsigned long long *q, const double *pred,
                             int npred, const double *c, unsigned long long *st_host) {
  const Rows r = rows(rs, g, 1);
  const int G = g.ngroups, ny = std::max(G, 1) * r.nrows, nchunks = hx_mom_chunks(n_);
  d_mom_.reserve(MomBuf(nullptr, n_, npad_, npred, ny, nchunks, G).words, *this, "hipMalloc moments");
  MomBuf b(d_mom_.get(), n_, npad_, npred, ny, nchunks, G);
  const size_t N = (size_t)n_;
  check(hipMemsetAsync(b.q_lane, 0, 8 * b.lane_words, stream_), "moments lanes");
  check(hipMemcpyAsync(b.q_mem, q, 8 * N, hipMemcpyHostToDevice, stream_), "moments weights");
  if (npred)
    check(hipMemcpyAsync(b.pred_mem, pred, 8 * N * (size_t)npred, hipMemcpyHostToDevice, stream_),
          "moments predictors");
  check(hipMemcpyAsync(b.c, c, 8 * 8 * (size_t)std::max(G, 1), hipMemcpyHostToDevice, stream_),
        "moments predictor shifts");
  if (G) {   // (the prepare kernel brings the labels to lane order with the weights)
    check(hipMemcpyAsync(b.lab_mem, g.labels, sizeof(int) * N, hipMemcpyHostToDevice, stream_), "group labels");
    check(hx_launch_gmom_prepare(b.q_mem, b.pred_mem, b.lab_mem, npred, n_, npad_, d_lane_of_member_, b.c, b.q_lane,
                                 b.qd_lane, b.e_lane, group_labels(), stream_), "grouped moments prepare kernel");
  } else {
    check(hx_launch_mom_prepare(b.q_mem, b.pred_mem, npred, n_, npad_, d_lane_of_member_, b.c, b.q_lane,
                                b.qd_lane, b.e_lane, stream_), "moments prepare kernel");
  }
  minmax(r, G, b.q_lane, b.st);
  check(hipMemcpyAsync(st_host, b.st, 8 * 4 * (size_t)ny, hipMemcpyDeviceToHost, stream_), "moments fetch");
  check(hipStreamSynchronize(stream_), "moments sync");   // (q, pred, c and the labels are the caller's until here)
  mom_src_ = r.block; mom_iy0_ = r.iy0; mom_ny_ = r.nrows; mom_npred_ = npred; mom_groups_ = G;
}

// the sum pass over the block mom_begin prepared: shift_host[rows] (the smallest participating value
// of every row over ALL shards) -> sums_host[rows][2 + 3 npred] of this core's members
void EnsembleCore::mom_finish(const double *shift_host, double *sums_host) {
  if (!mom_src_) throw std::runtime_error("moment sums without mom_begin");
  const int nrows = mom_ny_, npred = mom_npred_, G = mom_groups_, ny = std::max(G, 1) * nrows;
  MomBuf b(d_mom_.get(), n_, npad_, npred, ny, hx_mom_chunks(n_), G);
  const size_t nc = 2 + 3 * (size_t)npred;
  check(hipMemcpyAsync(b.shift, shift_host, 8 * (size_t)ny, hipMemcpyHostToDevice, stream_), "moments shifts");
  check(G ? hx_launch_gmoments(mom_src_, n_, npad_, mom_iy0_, nrows, b.qd_lane, b.e_lane, d_glab_, G, npred, b.shift,
                               b.part, b.out, stream_)
          : hx_launch_moments(mom_src_, n_, npad_, mom_iy0_, nrows, b.qd_lane, b.e_lane, npred, b.shift, b.part,
                              b.out, stream_), "moments kernel");
  check(hipMemcpyAsync(sums_host, b.out, 8 * (size_t)ny * nc, hipMemcpyDeviceToHost, stream_), "moments fetch");
  check(hipStreamSynchronize(stream_), "moments sync");
  mom_src_ = nullptr;
}

// ---- Sobol sums from a Saltelli design (hx_ensemble_sobol, hx_metric_sobol) -----------------------

namespace {
// d_sobol_ in 8-byte words: the rows' records, shifts, counts and sums, the chunks' partial sums, the
// group-major lane table, the groups' flags (the caller's use; in use and every lane valid) and the
// rows' participation bytes
struct SobBuf {
  unsigned long long *st;
  double *shift, *out, *part;
  long long *npart;
  int *tab;
  unsigned char *use, *flag, *on;
  size_t words;
  SobBuf(unsigned long long *base, int k, int nb, int ny, int nchunks) {
    const size_t K = (size_t)k, NB = (size_t)nb, Y = (size_t)ny, nc = 4 + 4 * K;
    const size_t gw = (NB + 7) / 8;                            // words of one byte per group
    st = base;                                                 // [ny][2]
    shift = reinterpret_cast<double *>(st + 2 * Y);            // [ny]
    npart = reinterpret_cast<long long *>(shift + Y);          // [ny]
    out = reinterpret_cast<double *>(npart + Y);               // [ny][nc]
    part = out + Y * nc;                                       // [ny][nchunks][nc]
    unsigned long long *w = reinterpret_cast<unsigned long long *>(part + Y * (size_t)nchunks * nc);
    tab = reinterpret_cast<int *>(w);                          // [k + 2][nb]
    w += ((K + 2) * NB + 1) / 2;
    use = reinterpret_cast<unsigned char *>(w);                // [nb]
    flag = reinterpret_cast<unsigned char *>(w + gw);          // [nb]
    on = reinterpret_cast<unsigned char *>(w + 2 * gw);        // [ny][nb]
    words = 4 * Y + Y * nc + Y * (size_t)nchunks * nc + ((K + 2) * NB + 1) / 2 + 2 * gw + (Y * NB + 7) / 8;
  }
};
}  // namespace

void EnsembleCore::sobol_begin(const RowSource &rs, int k, int n_base, const unsigned char *use) {
  const std::string f(rs.fn);
  if (k < 1 || k > HX_SOBOL_MAX_FACTORS) throw std::runtime_error(f + ": k must lie in 1..16");
  if (n_base < 1 || (long long)n_base * (long long)(k + 2) > (long long)n_)
    throw std::runtime_error(f + ": n_base * (k + 2) must lie in 1..n_members");
  const Rows r = rows(rs, Groups{nullptr, 0}, 1);
  const double *src = r.block;
  const int iy0 = r.iy0, ny = r.nrows;
  const int nchunks = hx_sobol_chunks(n_base);
  const size_t words = SobBuf(nullptr, k, n_base, ny, nchunks).words;
  d_sobol_.reserve(words, *this, "hipMalloc sobol");
  SobBuf b(d_sobol_.get(), k, n_base, ny, nchunks);
  check(hipMemsetAsync(b.st, 0, 8 * 2 * (size_t)ny, stream_), "sobol state");
  if (use) check(hipMemcpyAsync(b.use, use, (size_t)n_base, hipMemcpyHostToDevice, stream_), "sobol use");
  check(hx_launch_sobol_prepare(d_lane_of_member_, npad_, k, n_base, use ? b.use : nullptr, b.tab, b.flag, stream_),
        "sobol prepare kernel");
  check(hx_launch_sobol_part(src, npad_, iy0, ny, b.tab, n_base, k, b.flag, b.st, b.on, stream_),
        "sobol participation kernel");
  check(hipStreamSynchronize(stream_), "sobol sync");   // (use is the caller's until here)
  sob_src_ = src; sob_iy0_ = iy0; sob_ny_ = ny; sob_k_ = k; sob_nb_ = n_base;
}

// the sum pass over the block sobol_begin prepared -> shift_host[ny], sums_host[ny][4 + 4 k], n_part_host[ny]
void EnsembleCore::sobol_finish(double *shift_host, double *sums_host, long long *n_part_host) {
  if (!sob_src_) throw std::runtime_error("sobol sums without sobol_begin");
  const int ny = sob_ny_, k = sob_k_, nb = sob_nb_;
  SobBuf b(d_sobol_.get(), k, nb, ny, hx_sobol_chunks(nb));
  const size_t nc = 4 + 4 * (size_t)k;
  check(hx_launch_sobol_sums(sob_src_, npad_, sob_iy0_, ny, b.tab, nb, k, b.st, b.on, b.part, b.out, b.shift,
                             b.npart, stream_), "sobol kernel");
  check(hipMemcpyAsync(sums_host, b.out, 8 * (size_t)ny * nc, hipMemcpyDeviceToHost, stream_), "sobol fetch");
  check(hipMemcpyAsync(shift_host, b.shift, 8 * (size_t)ny, hipMemcpyDeviceToHost, stream_), "sobol fetch");
  check(hipMemcpyAsync(n_part_host, b.npart, 8 * (size_t)ny, hipMemcpyDeviceToHost, stream_), "sobol fetch");
  check(hipStreamSynchronize(stream_), "sobol sync");
  sob_src_ = nullptr;
}

// ---- score against observations with correlated errors (hx_member_score_whitened) ----------------

void EnsembleCore::member_score_whitened(const std::string &capability, const int *years, const double *obs,
                                         const double *whiten, int n, int base_year0, int base_year1,
                                         double *out_host) {
  const PostSource ps = whitened_check(capability, years, obs, whiten, n, base_year0, base_year1, out_host);
  const bool has_base = base_year0 <= base_year1;
  sync();
  const int np = hx_sw_padded(n);
  const size_t NP = (size_t)np, NL = NP + 8, P = (size_t)npad_;   // (the lists: padded by two steps of the kernel)
  // [wf NP^2][obs NL][base npad][chi2 npad][chi2 in member order n_] doubles, then the rows [NL] ints
  const size_t doubles = NP * NP + NL + 2 * P + (size_t)n_;
  const size_t bytes = sizeof(double) * doubles + sizeof(int) * NL;
  d_whiten_.reserve(bytes, *this, "hipMalloc whitened score");
  double *d_wf = d_whiten_.as<double>(), *d_obs = d_wf + NP * NP, *d_base = d_obs + NL, *d_lane = d_base + P, *d_mem = d_lane + P;
  int *d_iy = reinterpret_cast<int *>(d_mem + n_);
  // one upload: W in fragment order (zeros above the diagonal and in the padding), the observations
  // and, behind the device-only part, the rows -- both padded with a valid row / 0.0 (never consumed)
  std::vector<double> h(NP * NP + NL, 0.0);
  hx_sw_pack(whiten, n, h.data());
  std::vector<int> iy(NL, years[n - 1] - scen_.start);
  for (int i = 0; i < n; ++i) {
    h[NP * NP + (size_t)i] = obs[i];
    iy[(size_t)i] = years[i] - scen_.start;
  }
  check(hipMemcpyAsync(d_wf, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, stream_), "whitened score W");
  check(hipMemcpyAsync(d_iy, iy.data(), sizeof(int) * NL, hipMemcpyHostToDevice, stream_), "whitened score years");
  if (has_base)
    check(hx_launch_series_base(ps.block, npad_, base_year0 - scen_.start, base_year1 - scen_.start, d_base,
                                stream_), "whitened score base kernel");
  check(hx_launch_score_whiten(ps.block, n_, npad_, d_iy, d_obs, d_wf, n, has_base ? d_base : nullptr, d_lane,
                               stream_), "whitened score kernel");
  check(hx_launch_gather(d_lane, d_lane_of_member_, d_mem, n_, npad_, 1, stream_), "whitened score gather");
  check(hipMemcpyAsync(out_host, d_mem, sizeof(double) * (size_t)n_, hipMemcpyDeviceToHost, stream_),
        "whitened score fetch");
  check(hipStreamSynchronize(stream_), "whitened score sync");   // (h and iy are pageable: copied by now)
}

// ---- projection onto a caller's basis (hx_member_project) -------------------------------------------

void EnsembleCore::member_project(const std::string &capability, const int *years, const double *center,
                                  const double *basis, int n, int m, int base_year0, int base_year1,
                                  double *out_host, size_t row_pitch) {
  const PostSource ps = project_check(capability, years, center, basis, n, m, base_year0, base_year1, out_host);
  const bool has_base = base_year0 <= base_year1;
  sync();
  const int nt = (m + 15) / 16;
  const size_t NB = (size_t)hx_project_steps(n) * (size_t)nt * 64;   // the basis in fragment order
  const size_t NL = 4 * (size_t)hx_project_steps(n) + 8;             // (the lists: padded by two steps of the kernel)
  const size_t P = (size_t)npad_, M = (size_t)m;
  // [bf NB][center NL][base npad][out m x npad][out in member order m x n_] doubles, then the rows [NL] ints
  const size_t doubles = NB + NL + P + M * P + M * (size_t)n_;
  const size_t bytes = sizeof(double) * doubles + sizeof(int) * NL;
  d_project_.reserve(bytes, *this, "hipMalloc project");
  double *d_bf = d_project_.as<double>(), *d_center = d_bf + NB, *d_base = d_center + NL, *d_lane = d_base + P, *d_mem = d_lane + M * P;
  int *d_iy = reinterpret_cast<int *>(d_mem + M * (size_t)n_);
  // one upload: the basis in fragment order (zeros in the padding) and the centre, and one of the rows
  // -- both lists padded with 0.0 / a valid row (never consumed)
  std::vector<double> h(NB + NL, 0.0);
  hx_project_pack(basis, n, m, h.data());
  std::vector<int> iy(NL, years[n - 1] - scen_.start);
  for (int i = 0; i < n; ++i) {
    if (center) h[NB + (size_t)i] = center[i];
    iy[(size_t)i] = years[i] - scen_.start;
  }
  check(hipMemcpyAsync(d_bf, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, stream_), "project basis");
  check(hipMemcpyAsync(d_iy, iy.data(), sizeof(int) * NL, hipMemcpyHostToDevice, stream_), "project years");
  if (has_base)
    check(hx_launch_series_base(ps.block, npad_, base_year0 - scen_.start, base_year1 - scen_.start, d_base,
                                stream_), "project base kernel");
  check(hx_launch_project(ps.block, n_, npad_, d_iy, d_center, d_bf, n, m, has_base ? d_base : nullptr, d_lane,
                          stream_), "project kernel");
  check(hx_launch_gather(d_lane, d_lane_of_member_, d_mem, n_, npad_, m, stream_), "project gather");
  if (row_pitch)
    check(hipMemcpy2DAsync(out_host, sizeof(double) * row_pitch, d_mem, sizeof(double) * (size_t)n_,
                           sizeof(double) * (size_t)n_, M, hipMemcpyDeviceToHost, stream_), "project fetch");
  else
    check(hipMemcpyAsync(out_host, d_mem, sizeof(double) * M * (size_t)n_, hipMemcpyDeviceToHost, stream_),
          "project fetch");
  check(hipStreamSynchronize(stream_), "project sync");   // (h and iy are pageable: copied by now)
}

// ---- year-by-year co-moments of two windows (hx_ensemble_comoments) --------------------------------

namespace {
// d_comom_ in 8-byte words.  R = na + nb rows (na in the symmetric call: B is A).  The partials of
// the Gram kernel are bounded: hx_co_chunks() grows the member chunk until chunks x na x nb stays
// within 8 Mi doubles (64 MiB), whatever the windows; the rest is 2 npad + n + 8 R + na nb words
// and the row sums' partials, 2 R hx_mom_chunks(n).
struct CoBuf {
  unsigned long long *q_lane, *q_mem, *st;
  double *qd_lane, *shift, *mpart, *mout, *gpart, *cross;
  size_t words, lane_words;
  CoBuf(unsigned long long *base, int n, int npad, int na, int nb, int rows, int mchunks, int gchunks) {
    const size_t N = (size_t)n, P = (size_t)npad, R = (size_t)rows, C = (size_t)na * (size_t)nb;
    q_lane = base;                                              // [npad] } zeroed before the prepare
    qd_lane = reinterpret_cast<double *>(q_lane + P);           // [npad] } kernel: padding lanes 0
    lane_words = 2 * P;
    q_mem = base + lane_words;                                  // [n]
    st = q_mem + N;                                             // [R][4]
    shift = reinterpret_cast<double *>(st + 4 * R);             // [R]
    mpart = shift + R;                                          // [R][mchunks][2]
    mout = mpart + 2 * R * (size_t)mchunks;                     // [R][2]
    cross = mout + 2 * R;                                       // [na][nb]
    gpart = cross + C;                                          // [gchunks][na][nb]
    words = lane_words + N + 7 * R + 2 * R * (size_t)mchunks + C + C * (size_t)gchunks;
  }
};
}  // namespace

// The windows' capabilities and dates against this core, before anything is sized from them.
void EnsembleCore::comom_check(const std::string &cap_a, int a0, int a1, const std::string *cap_b, int b0,
                               int b1) {
  const char *fn = "hx_ensemble_comoments";
  (void)q_check(cap_a, a0, a1, 1, fn);
  if (cap_b) (void)q_check(*cap_b, b0, b1, 1, fn);
}

// Validates both windows (nothing is changed by a refused call), brings q[n_] to lane order, zeroes
// it where a value of either window is NaN, and reduces {~min key, max key, sum q, count} of every
// row -- A's na rows, then B's nb unless cap_b is nullptr -- into st_host[rows][4].
void EnsembleCore::comom_begin(const std::string &cap_a, int a0, int a1, const std::string *cap_b, int b0,
                               int b1, const unsigned long long *q, unsigned long long *st_host) {
  const char *fn = "hx_ensemble_comoments";
  const double *sa = q_check(cap_a, a0, a1, 1, fn), *sb = sa;
  if (cap_b) {
    sb = q_check(*cap_b, b0, b1, 1, fn);
    sa = q_check(cap_a, a0, a1, 1, fn);   // (two derived blocks are kept: B's has not displaced A's)
  }
  if (npad_ % 32) throw std::runtime_error(std::string(fn) + ": the lane count is not a multiple of 32");
  sync();
  const bool sym = cap_b == nullptr;
  const int na = a1 - a0 + 1, nb = sym ? na : b1 - b0 + 1, rows = sym ? na : na + nb;
  const int ia0 = a0 - scen_.start, ib0 = sym ? ia0 : b0 - scen_.start;
  const int mchunks = hx_mom_chunks(n_), gchunks = hx_co_chunks(n_, na, nb);
  const size_t words = CoBuf(nullptr, n_, npad_, na, nb, rows, mchunks, gchunks).words;
  d_comom_.reserve(words, *this, "hipMalloc co-moments");
  CoBuf b(d_comom_.get(), n_, npad_, na, nb, rows, mchunks, gchunks);
  check(hipMemsetAsync(b.q_lane, 0, 8 * b.lane_words, stream_), "co-moments lanes");
  check(hipMemsetAsync(b.st, 0, 8 * 4 * (size_t)rows, stream_), "co-moments state");
  check(hipMemcpyAsync(b.q_mem, q, 8 * (size_t)n_, hipMemcpyHostToDevice, stream_), "co-moments weights");
  check(hx_launch_mom_prepare(b.q_mem, nullptr, 0, n_, npad_, d_lane_of_member_, nullptr, b.q_lane, b.qd_lane,
                              nullptr, stream_), "co-moments prepare kernel");
  check(hx_launch_co_mask(sa, ia0, na, sb, ib0, sym ? 0 : nb, npad_, b.q_lane, b.qd_lane, stream_),
        "co-moments mask kernel");
  check(hx_launch_q_minmax(sa, n_, npad_, ia0, na, b.q_lane, b.st, stream_), "co-moments min kernel");
  if (!sym)
    check(hx_launch_q_minmax(sb, n_, npad_, ib0, nb, b.q_lane, b.st + 4 * (size_t)na, stream_),
          "co-moments min kernel");
  check(hipMemcpyAsync(st_host, b.st, 8 * 4 * (size_t)rows, hipMemcpyDeviceToHost, stream_), "co-moments fetch");
  check(hipStreamSynchronize(stream_), "co-moments sync");   // (q is the caller's until here)
  co_a_ = sa; co_b_ = sb; co_ia0_ = ia0; co_ib0_ = ib0; co_na_ = na; co_nb_ = nb; co_sym_ = sym;
}

// the sums of this core's members about shift_host[rows] (the rows' smallest participating values
// over ALL shards): sums_host[rows][2] and cross_host[na][nb]
void EnsembleCore::comom_finish(const double *shift_host, double *sums_host, double *cross_host) {
  if (!co_a_) throw std::runtime_error("co-moment sums without comom_begin");
  const int na = co_na_, nb = co_nb_, rows = co_sym_ ? na : na + nb;
  CoBuf b(d_comom_.get(), n_, npad_, na, nb, rows, hx_mom_chunks(n_), hx_co_chunks(n_, na, nb));
  const size_t C = (size_t)na * (size_t)nb;
  check(hipMemcpyAsync(b.shift, shift_host, 8 * (size_t)rows, hipMemcpyHostToDevice, stream_), "co-moments shifts");
  check(hx_launch_moments(co_a_, n_, npad_, co_ia0_, na, b.qd_lane, nullptr, 0, b.shift, b.mpart, b.mout,
                          stream_), "co-moments row sums");
  if (!co_sym_)
    check(hx_launch_moments(co_b_, n_, npad_, co_ib0_, nb, b.qd_lane, nullptr, 0, b.shift + na,
                            b.mpart + 2 * (size_t)na * (size_t)hx_mom_chunks(n_), b.mout + 2 * (size_t)na,
                            stream_), "co-moments row sums");
  check(hx_launch_co_gram(co_a_, co_ia0_, na, co_b_, co_ib0_, nb, n_, npad_, co_sym_ ? 1 : 0, b.qd_lane, b.shift,
                          co_sym_ ? b.shift : b.shift + na, b.gpart, b.cross, stream_), "co-moments Gram kernel");
  check(hipMemcpyAsync(sums_host, b.mout, 8 * 2 * (size_t)rows, hipMemcpyDeviceToHost, stream_), "co-moments fetch");
  check(hipMemcpyAsync(cross_host, b.cross, 8 * C, hipMemcpyDeviceToHost, stream_), "co-moments fetch");
  check(hipStreamSynchronize(stream_), "co-moments sync");
  co_a_ = nullptr;
}

// ---- member ranks and the CRPS (hx_series_rank, hx_metric_ranks, hx_ensemble_crps) ----------------

namespace {
// d_rank_ in 8-byte words: the rows' records [nrows][4], the observations [nrows], the row list
// [nrows] (int), then the sort's buffers for one batch of `per` rows: the rows are split into equal
// batches that keep those buffers under hx_rank_scratch_bytes() (one row, if a row alone is more)
struct RankBuf {
  unsigned long long *res, *sort;
  double *obs;
  int *rows;
  int per;
  size_t words;
  RankBuf(unsigned long long *base, int n, int nrows) {
    const size_t R = (size_t)nrows, rw = hx_rank_row_words(n);
    const size_t most = std::max<size_t>(1, hx_rank_scratch_bytes() / 8 / rw);
    const size_t nb = (R + most - 1) / most;
    per = (int)((R + nb - 1) / nb);
    res = base;
    obs = reinterpret_cast<double *>(res + 4 * R);
    rows = reinterpret_cast<int *>(res + 5 * R);
    sort = res + 5 * R + (R + 1) / 2;
    words = 5 * R + (R + 1) / 2 + (size_t)per * rw;
  }
};
}  // namespace

std::vector<unsigned long long> EnsembleCore::rank_rows(const char *fn, const double *src, int row0,
                                                        const int *rows, int nrows, const unsigned long long *q,
                                                        int mode, const double *obs, double *dst, int dst_row0) {
  std::vector<unsigned long long> rec;
  const size_t words = RankBuf(nullptr, n_, nrows).words;
  if (d_rank_.grow(words) != hipSuccess) {   // (this one words its own failure)
    (void)hipGetLastError();
    throw std::runtime_error(std::string(fn) + ": no device memory for the scratch of the sort (" +
                             std::to_string((8 * words) >> 20) + " MiB)");
  }
  RankBuf b(d_rank_.get(), n_, nrows);
  const unsigned long long *dq = lane_weights(q);   // (the sort never reads the padding lanes)
  if (rows) check(hipMemcpy(b.rows, rows, sizeof(int) * (size_t)nrows, hipMemcpyHostToDevice), "rank rows");
  if (obs) check(hipMemcpy(b.obs, obs, sizeof(double) * (size_t)nrows, hipMemcpyHostToDevice), "rank observations");
  for (int r0 = 0; r0 < nrows; r0 += b.per) {   // (stream order: a batch has finished with the buffers before the next)
    const int nr = std::min(b.per, nrows - r0);
    check(hx_launch_rank(src, n_, npad_, row0 + r0, rows ? b.rows + r0 : nullptr, nr, dq, mode,
                         obs ? b.obs + r0 : nullptr, b.sort, dst, dst_row0 + r0, b.res + 4 * (size_t)r0, stream_),
          "rank kernel");
  }
  if (mode == 2) {
    rec.resize(4 * (size_t)nrows);
    check(hipMemcpyAsync(rec.data(), b.res, 8 * rec.size(), hipMemcpyDeviceToHost, stream_), "rank fetch");
  }
  check(hipStreamSynchronize(stream_), "rank sync");
  return rec;
}

void EnsembleCore::series_rank(const std::string &name, const std::string &capability, int year0, int year1,
                               const unsigned long long *q, int kind) {
  const char *fn = "hx_series_rank";
  const std::string f(fn);
  const int existing = series_name_check(f, name);
  if (kind != HX_RANK_PIT && kind != HX_RANK_NUMERATOR)
    throw std::runtime_error(f + ": unknown kind " + std::to_string(kind) + " (HX_RANK_PIT or HX_RANK_NUMERATOR)");
  const double *src = q_check(capability, year0, year1, 1, fn);
  if (lane_of_member_.empty()) throw std::runtime_error(f + ": run the core first");
  sync();
  const size_t bytes = sizeof(double) * (size_t)scen_.ns() * (size_t)npad_;
  double *z = nullptr;
  if (hipMalloc(&z, bytes) != hipSuccess || !z) {
    (void)hipGetLastError();
    throw std::runtime_error(f + ": no device memory for the block of series " + name + " (" +
                             std::to_string(bytes >> 20) + " MiB)");
  }
  const int iy0 = year0 - scen_.start, ny = year1 - year0 + 1;
  try {
    check(hipMemsetAsync(z, 0xff, bytes, stream_), "rank series fill");   // every double a NaN
    (void)rank_rows(fn, src, iy0, nullptr, ny, q, kind, nullptr, z, iy0);
  } catch (...) { (void)hipFree(z); throw; }
  Series s;
  s.name = name; s.block = z; s.valid_iy = year1 - scen_.start; s.lane_of_member = lane_of_member_;
  if (existing >= 0) {
    (void)hipFree(series_[(size_t)existing].block);
    series_[(size_t)existing] = std::move(s);
  } else {
    series_.push_back(std::move(s));
  }
}

void EnsembleCore::metric_ranks(const std::string &capability, const hx_metric *specs, int nspecs,
                                const unsigned long long *q, int kind, double *out_host) {
  const char *fn = "hx_metric_ranks";
  const std::string f(fn);
  const double *src = nullptr;
  metric_check(capability, specs, nspecs, fn, &src);
  if (kind != HX_RANK_PIT && kind != HX_RANK_NUMERATOR)
    throw std::runtime_error(f + ": unknown kind " + std::to_string(kind) + " (HX_RANK_PIT or HX_RANK_NUMERATOR)");
  if (!out_host) throw std::runtime_error(f + ": null argument");
  sync();
  const double *blk = metric_block(src, specs, nspecs);
  // the ranks in lane order [nspecs][npad_], then in member order [nspecs][n_], in the score scratch
  const size_t lane_bytes = sizeof(double) * (size_t)nspecs * (size_t)npad_;
  const size_t mem_bytes = sizeof(double) * (size_t)nspecs * (size_t)n_;
  d_score_.reserve(lane_bytes + mem_bytes, *this, "hipMalloc score");
  double *d_lane = d_score_.as<double>(), *d_mem = d_lane + (size_t)nspecs * (size_t)npad_;
  check(hipMemsetAsync(d_lane, 0xff, lane_bytes, stream_), "metric rank fill");
  (void)rank_rows(fn, blk, 0, nullptr, nspecs, q, kind, nullptr, d_lane, 0);
  check(hx_launch_gather(d_lane, d_lane_of_member_, d_mem, n_, npad_, nspecs, stream_), "metric rank gather");
  check(hipMemcpyAsync(out_host, d_mem, mem_bytes, hipMemcpyDeviceToHost, stream_), "metric rank fetch");
  check(hipStreamSynchronize(stream_), "metric rank sync");
}

void EnsembleCore::crps(const std::string &capability, const int *years, const double *obs, int nyears,
                        const unsigned long long *q, double *crps_host, double *pit_host,
                        long long *n_part_host) {
  const char *fn = "hx_ensemble_crps";
  const std::string f(fn);
  if (nyears < 1 || !years || !obs || !crps_host) throw std::runtime_error(f + ": nyears < 1");
  const int y0 = *std::min_element(years, years + nyears), y1 = *std::max_element(years, years + nyears);
  const double *src = q_check(capability, y0, y1, 1, fn);
  sync();
  std::vector<int> rows((size_t)nyears);
  for (int i = 0; i < nyears; ++i) rows[(size_t)i] = years[i] - scen_.start;
  const std::vector<unsigned long long> rec = rank_rows(fn, src, 0, rows.data(), nyears, q, 2, obs, nullptr, 0);
  for (int i = 0; i < nyears; ++i) {
    std::memcpy(&crps_host[i], &rec[4 * (size_t)i], 8);
    if (pit_host) std::memcpy(&pit_host[i], &rec[4 * (size_t)i + 1], 8);
    if (n_part_host) n_part_host[i] = (long long)rec[4 * (size_t)i + 2];
  }
}


#else   // HX_HOST_EMULATION: the same entry points refuse, each where it refused before.  The summary
        // verbs over a RowSource refuse in rows_check: at once, or behind the checks of a pair or grouped
        // call.  The helpers only the verbs reach (rows, q_start, minmax, rank_rows and their like) are
        // not built.

namespace {
using Str = const std::string &;
using U64 = unsigned long long;
}  // namespace

void EnsembleCore::quantiles(const RowSource &rs, const Groups &g, const U64 *, const double *, int nprobs, double *, long long *) { rows_check(rs, g, nprobs); }
void EnsembleCore::q_begin(const RowSource &rs, const Groups &g, const U64 *, int nprobs, U64 *) { rows_check(rs, g, nprobs); }
void EnsembleCore::q_pass(const int *, const U64 *, U64 *) { refuse("hx_ensemble_quantiles", false); }
void EnsembleCore::bin_sums(const RowSource &rs, const Groups &g, const U64 *, const double *, int, U64 *) { rows_check(rs, g, 1); }
void EnsembleCore::mom_begin(const RowSource &rs, const Groups &g, const U64 *, const double *, int, const double *, U64 *) { rows_check(rs, g, 1); }
void EnsembleCore::mom_finish(const double *, double *) { refuse("hx_ensemble_moments"); }
void EnsembleCore::sobol_begin(const RowSource &rs, int, int, const unsigned char *) { refuse(rs.fn); }
void EnsembleCore::sobol_finish(double *, double *, long long *) { refuse("hx_ensemble_sobol"); }
void EnsembleCore::comom_check(Str, int, int, const std::string *, int, int) { refuse("hx_ensemble_comoments"); }
void EnsembleCore::comom_begin(Str, int, int, const std::string *, int, int, const U64 *, U64 *) { refuse("hx_ensemble_comoments"); }
void EnsembleCore::comom_finish(const double *, double *, double *) { refuse("hx_ensemble_comoments"); }
void EnsembleCore::series_rank(Str, Str, int, int, const U64 *, int) { refuse("hx_series_rank"); }
void EnsembleCore::metric_ranks(Str, const hx_metric *, int, const U64 *, int, double *) { refuse("hx_metric_ranks"); }
void EnsembleCore::crps(Str, const int *, const double *, int, const U64 *, double *, double *, long long *) { refuse("hx_ensemble_crps"); }

// ... and those that check their arguments first
void EnsembleCore::member_score_whitened(Str capability, const int *years, const double *obs, const double *whiten, int n,
                                         int base_year0, int base_year1, double *out_host) {
  whitened_check(capability, years, obs, whiten, n, base_year0, base_year1, out_host);
  refuse("hx_member_score_whitened");
}
void EnsembleCore::member_project(Str capability, const int *years, const double *center, const double *basis, int n, int m,
                                  int base_year0, int base_year1, double *out_host, size_t) {
  project_check(capability, years, center, basis, n, m, base_year0, base_year1, out_host);
  refuse("hx_member_project");
}

#endif  // HX_HOST_EMULATION

}  // namespace hx
