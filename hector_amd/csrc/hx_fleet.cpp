// hx_fleet.cpp -- see hx_fleet.hpp.
#include "hx_fleet.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <thread>

#ifndef HX_HOST_EMULATION
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: the library is loaded at first use
#endif

namespace hx {

namespace {

void hip_ck(hipError_t e, const char *what) {
  if (e != hipSuccess)
    throw std::runtime_error(std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
}

#ifndef HX_HOST_EMULATION
// The RCCL entry points the fleet uses, bound once per process.  The copy that is already
// loaded wins (PyTorch-ROCm brings its own librccl.so whose SONAME is librccl.so.1, too): two
// RCCLs in one process would each bring their own topology state and kernels.
struct Rccl {
  void *handle = nullptr;
  std::string origin;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclCommAbort) CommAbort = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclGetVersion) GetVersion = nullptr;
};

Rccl &rccl() {
  static Rccl r;
  if (r.handle) return r;
  std::vector<std::pair<std::string, int>> tries;
  if (const char *p = std::getenv("HECTOR_AMD_RCCL")) tries.push_back({p, RTLD_NOW | RTLD_LOCAL});
  tries.push_back({"librccl.so.1", RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD});
  tries.push_back({"librccl.so", RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD});
  tries.push_back({"librccl.so.1", RTLD_NOW | RTLD_LOCAL});
  tries.push_back({"/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL});
  std::string errs;
  for (auto &t : tries) {
    void *h = dlopen(t.first.c_str(), t.second);
    if (h) { r.handle = h; r.origin = t.first + ((t.second & RTLD_NOLOAD) ? " (already loaded)" : ""); break; }
    if (!(t.second & RTLD_NOLOAD)) { const char *e = dlerror(); errs += std::string(" [") + (e ? e : "?") + "]"; }
  }
  if (!r.handle)
    throw std::runtime_error("hector_amd: RCCL (librccl.so.1) could not be loaded for the multi-GPU "
                             "collective:" + errs + " -- set HECTOR_AMD_RCCL to its path");
  auto sym = [&](const char *name) {
    void *p = dlsym(r.handle, name);
    if (!p) throw std::runtime_error(std::string("hector_amd: RCCL symbol missing: ") + name);
    return p;
  };
  r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
  r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
  r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
  r.CommAbort = reinterpret_cast<decltype(r.CommAbort)>(sym("ncclCommAbort"));
  r.AllGather = reinterpret_cast<decltype(r.AllGather)>(sym("ncclAllGather"));
  r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(sym("ncclGroupStart"));
  r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(sym("ncclGroupEnd"));
  r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
  r.GetVersion = reinterpret_cast<decltype(r.GetVersion)>(sym("ncclGetVersion"));
  return r;
}

void nccl_ck(ncclResult_t e, const char *what) {
  if (e != ncclSuccess)
    throw std::runtime_error(std::string("RCCL error in ") + what + ": " + rccl().GetErrorString(e));
}
// ncclGroupStart ... ncclGroupEnd around the per-shard calls of one process.  The group is ALWAYS
// closed: an exception between the two would otherwise leave RCCL's thread-local group open, and
// the library shares the process's RCCL with the host (PyTorch's copy when there is one) -- its
// next collective would be queued into our dangling group and never run.  end() is the checked
// close of the normal path (the calls' results -- communicator handles, queued kernels -- exist
// only after it); the destructor closes what an unwinding exception left open, result ignored.
struct RcclGroup {
  Rccl &r;
  bool open = false;
  RcclGroup(Rccl &rc, bool grouped) : r(rc) {
    if (grouped) { nccl_ck(r.GroupStart(), "ncclGroupStart"); open = true; }
  }
  void end() {
    if (!open) return;
    open = false;
    nccl_ck(r.GroupEnd(), "ncclGroupEnd");
  }
  ~RcclGroup() { if (open) (void)r.GroupEnd(); }
  RcclGroup(const RcclGroup &) = delete;
  RcclGroup &operator=(const RcclGroup &) = delete;
};
#endif

bool rehearsal_allowed() {
#ifdef HX_HOST_EMULATION
  return true;
#else
  const char *e = std::getenv("HECTOR_AMD_FLEET_REHEARSAL");
  return e && std::atoi(e) != 0;
#endif
}

}  // namespace

Fleet::Fleet(const std::string &scenario, int n_members, const int *devices, int n_devices) : n_(n_members) {
  if (n_devices < 1 || !devices) throw std::runtime_error("hx_newcore_devices: empty device list");
  if (n_members < n_devices)
    throw std::runtime_error("hx_newcore_devices: fewer members than devices");
  for (int a = 0; a < n_devices; ++a)
    for (int b = a + 1; b < n_devices; ++b)
      if (devices[a] == devices[b]) duplicates_ = true;
  if (duplicates_ && !rehearsal_allowed())
    throw std::runtime_error(
        "hx_newcore_devices: a device appears twice in the list.  RCCL needs one rank per GPU; for a "
        "rehearsal of the sharded path on a box with fewer GPUs set HECTOR_AMD_FLEET_REHEARSAL=1 "
        "(the statistics are then exchanged by device copies, not by RCCL)");
  // contiguous member blocks, the remainder spread over the first shards
  const int base = n_members / n_devices, rem = n_members % n_devices;
  int off = 0;
  shards_.resize((size_t)n_devices);
  for (int s = 0; s < n_devices; ++s) {
    Shard &sh = shards_[(size_t)s];
    sh.device = devices[s];
    sh.offset = off;
    sh.count = base + (s < rem ? 1 : 0);
    off += sh.count;
    sh.core.reset(new EnsembleCore(scenario, sh.count, sh.device));
  }
}

Fleet::~Fleet() {
  free_stats_buffers();
#ifndef HX_HOST_EMULATION
  for (Shard &s : shards_)
    if (s.comm) { (void)hipSetDevice(s.device); (void)rccl().CommDestroy((ncclComm_t)s.comm); s.comm = nullptr; }
#endif
  for (Shard &s : shards_) { (void)hipSetDevice(s.device); s.core.reset(); }
}

void Fleet::use(const Shard &s) const { hip_ck(hipSetDevice(s.device), "hipSetDevice"); }

EnsembleCore &Fleet::shard(int s) {
  if (s < 0 || s >= n_shards()) throw std::runtime_error("bad shard index");
  use(shards_[(size_t)s]);
  return *shards_[(size_t)s].core;
}

int Fleet::shard_of_member(int member) const {
  if (member < 0 || member >= n_) throw std::runtime_error("bad member index");
  for (int s = n_shards() - 1; s >= 0; --s)
    if (member >= shards_[(size_t)s].offset) return s;
  return 0;
}

void Fleet::check_poison() const {
  if (!poisoned_.empty()) throw std::runtime_error(poisoned_);
}
void Fleet::poison(size_t shard, const char *call, const char *why) {
  poisoned_ = "hector_amd: this sharded core is inconsistent and refuses further calls: " +
              std::string(call) + " failed on shard " + std::to_string(shard) + " of " +
              std::to_string(shards_.size()) + " (" + why + ") after it had been applied to the "
              "shards before it; shut the core down and create it again";
}

// a routed call, shard after shard; a failure after the first shard leaves the shards different.
// HX_EACH_DO(label, statements on Shard &s): the one place that holds the poison protocol; HX_EACH(call)
// is the common case, the same call on every shard's core.
#define HX_EACH_DO(label_, ...)                                                     \
  {                                                                                \
    check_poison();                                                                \
    size_t k_ = 0;                                                                 \
    try {                                                                          \
      for (; k_ < shards_.size(); ++k_) { Shard &s = shards_[k_]; use(s); __VA_ARGS__; } \
    } catch (const std::exception &e_) {                                           \
      if (k_ > 0) poison(k_, label_, e_.what());                                   \
      throw;                                                                       \
    }                                                                              \
  }
#define HX_EACH(call) HX_EACH_DO(#call, s.core->call)

// The verbs that do real host work or wait for a device -- run() (lane order, parameter upload,
// spinup), reset(), sync(), fetchvars() -- take the shards side by side, one host thread per
// shard: done one after the other, GPU k would start k x (host preparation + spinup) late, and
// eight device-to-host copies would share one PCIe link's worth of time.  The first error in shard
// order is the call's error.  (The host-emulation build runs a "kernel" on the calling thread with
// its LDS in globals: shards stay sequential there.)
template <class F>
void Fleet::each_parallel(F &&fn) {
  check_poison();
#ifndef HX_HOST_EMULATION
  if (shards_.size() > 1 && !std::getenv("HECTOR_AMD_FLEET_SEQUENTIAL")) {
    std::vector<std::exception_ptr> err(shards_.size());
    std::vector<std::thread> th;
    auto body = [&](size_t k) {
      try { use(shards_[k]); fn(shards_[k]); } catch (...) { err[k] = std::current_exception(); }
    };
    size_t started = 1;
    try {
      for (; started < shards_.size(); ++started) th.emplace_back(body, started);
    } catch (...) {  // no more threads to be had: the remaining shards on this one
    }
    body(0);
    for (size_t k = started; k < shards_.size(); ++k) body(k);
    for (std::thread &t : th) t.join();
    size_t failed = 0, first = shards_.size();
    for (size_t k = 0; k < err.size(); ++k) if (err[k]) { ++failed; if (first == shards_.size()) first = k; }
    if (failed) {
      if (failed < shards_.size()) {   // some shards went through, some did not
        try { std::rethrow_exception(err[first]); }
        catch (const std::exception &e) { poison(first, "a parallel call (run / reset / sync / fetchvars)", e.what()); }
        catch (...) { poison(first, "a parallel call", "unknown error"); }
      }
      std::rethrow_exception(err[first]);
    }
    return;
  }
#endif
  {
    size_t k = 0;
    try {
      for (; k < shards_.size(); ++k) { use(shards_[k]); fn(shards_[k]); }
    } catch (const std::exception &e) {
      if (k > 0) poison(k, "a sharded call (run / reset / sync / fetchvars)", e.what());
      throw;
    }
  }
}

void Fleet::setvar(const std::string &cap, const double *values, int nvalues, const char *units) {
  if (shards_.size() == 1) { shards_[0].core->setvar(cap, values, nvalues, units); return; }
  if (nvalues != 1 && nvalues != n_)
    throw std::runtime_error("setvar: expected 1 or n_members values");
  check_poison();
  size_t k = 0;
  try {
    for (; k < shards_.size(); ++k) {
      Shard &s = shards_[k];
      use(s);
      if (nvalues == 1) s.core->setvar(cap, values, 1, units);
      else s.core->setvar(cap, values + s.offset, s.count, units);
    }
  } catch (const std::exception &e) {
    if (k > 0) poison(k, "setvar", e.what());
    throw;
  }
}
void Fleet::getvar(const std::string &cap, double *out) {
  for (Shard &s : shards_) { use(s); s.core->getvar(cap, out + s.offset); }
}
void Fleet::split_biome(const std::vector<std::string> &names, const double *fveg, const double *fdet,
                        const double *fsoil, const double *fpf, const double *fnpp) {
  HX_EACH(split_biome(names, fveg, fdet, fsoil, fpf, fnpp))
}
void Fleet::split_biome_of(const std::string &old_biome, const std::vector<std::string> &names,
                           const double *fveg, const double *fdet, const double *fsoil,
                           const double *fpf, const double *fnpp) {
  HX_EACH(split_biome_of(old_biome, names, fveg, fdet, fsoil, fpf, fnpp))
}
void Fleet::create_biome(const std::string &b) { HX_EACH(create_biome(b)) }
void Fleet::delete_biome(const std::string &b) { HX_EACH(delete_biome(b)) }
void Fleet::rename_biome(const std::string &a, const std::string &b) { HX_EACH(rename_biome(a, b)) }
void Fleet::set_outputs(const std::vector<std::string> &caps) { HX_EACH(set_outputs(caps)) }
void Fleet::set_member_sorting(bool on) { HX_EACH(set_member_sorting(on)) }
void Fleet::set_lane_calibration(bool on) { HX_EACH(set_lane_calibration(on)) }
void Fleet::set_cost_model(bool on) { HX_EACH(set_cost_model(on)) }
bool Fleet::lanes_calibrated() const {
  for (const Shard &s : shards_) if (!s.core->lanes_calibrated()) return false;
  return true;
}
void Fleet::enable_history(bool on) { HX_EACH(enable_history(on)) }
void Fleet::enable_spinup_record(bool on) { HX_EACH(enable_spinup_record(on)) }
void Fleet::enable_slcf_mixes(bool on) { HX_EACH(enable_slcf_mixes(on)) }
void Fleet::enable_member_forcing(bool on) {
  if (!on && shards_.size() > 1) {   // every shard first: a refused call changes nothing
    static const char *const order[7] = {"delta_co2", "delta_ch4", "delta_n2o", "rho_bc", "rho_oc", "rho_so2", "rho_nh3"};
    std::string names;
    for (const char *k : order)
      for (Shard &s : shards_) {
        const auto held = s.core->member_forcing_names();
        if (std::find(held.begin(), held.end(), k) == held.end()) continue;
        names += (names.empty() ? "" : ", ") + std::string(k);
        break;
      }
    if (!names.empty())
      throw std::runtime_error("hx_enable_member_forcing: " + names + " differs between members: set "
                               "one value for the whole core first (hx_setvar with one value)");
  }
  HX_EACH(enable_member_forcing(on))
}
int Fleet::spinup_record(int member, double *values, int max_steps) {
  Shard &s = shards_[(size_t)shard_of_member(member)];
  use(s);
  return s.core->spinup_record(member - s.offset, values, max_steps);
}
void Fleet::set_pair_kernel_limit(int m) { HX_EACH(set_pair_kernel_limit(m)) }
void Fleet::set_prewarm(int ms) { HX_EACH(set_prewarm(ms)) }
bool Fleet::last_run_prewarmed() const { return shards_.front().core->last_run_prewarmed(); }
void Fleet::set_two_wave_from(int m) { HX_EACH(set_two_wave_from(m)) }   // (members of a shard)
void Fleet::setvar_dated(const std::string &cap, const int *years, const double *values, int n,
                         const char *units) {
  HX_EACH(setvar_dated(cap, years, values, n, units))
}
void Fleet::setvar_dated_members(const std::string &cap, const int *years, const double *values,
                                 int nyears, const char *units) {
  if (shards_.size() == 1) { shards_[0].core->setvar_dated_members(cap, years, values, nyears, units); return; }
  std::vector<double> part;
  for (Shard &s : shards_) {  // values[i * n_members + member] -> this shard's [i][count]
    use(s);
    part.resize((size_t)nyears * (size_t)s.count);
    for (int i = 0; i < nyears; ++i)
      std::memcpy(part.data() + (size_t)i * s.count, values + (size_t)i * n_ + s.offset,
                  sizeof(double) * (size_t)s.count);
    s.core->setvar_dated_members(cap, years, part.data(), nyears, units);
  }
}
void Fleet::setvar_dated_mix(const std::string &cap, const int *years, int nyears, const double *basis,
                             int nbasis, const double *coeff, const char *units) {
  if (shards_.size() == 1) { shards_[0].core->setvar_dated_mix(cap, years, nyears, basis, nbasis, coeff, units); return; }
  // every shard validates its own part: all of them first, so that a refused call changes nothing
  std::vector<std::vector<double>> part(shards_.size());
  for (size_t j = 0; j < shards_.size(); ++j) {  // coeff[k * n_members + member] -> this shard's [k][count]
    Shard &s = shards_[j];
    if (nbasis > 0 && nbasis <= HX_MIX_MAX_BASIS && coeff) {
      part[j].resize((size_t)nbasis * (size_t)s.count);
      for (int k = 0; k < nbasis; ++k)
        std::memcpy(part[j].data() + (size_t)k * s.count, coeff + (size_t)k * n_ + s.offset,
                    sizeof(double) * (size_t)s.count);
    }
    use(s);
    s.core->check_dated_mix(cap, years, nyears, basis, nbasis, part[j].empty() ? nullptr : part[j].data(), units);
  }
  for (size_t j = 0; j < shards_.size(); ++j) {
    use(shards_[j]);
    shards_[j].core->setvar_dated_mix(cap, years, nyears, basis, nbasis,
                                      part[j].empty() ? nullptr : part[j].data(), units);
  }
}
int Fleet::setvar_scenario_mix(const std::vector<std::string> &paths, const double *coeff) {
  if (!coeff) throw std::runtime_error("hx_setvar_scenario_mix: null coeff");
  use(shards_[0]);
  const auto plan = shards_[0].core->plan_scenario_mix(paths);   // (every shard holds the same scenario)
  const int y0 = start_date(), ns = end_date() - y0 + 1, K = (int)paths.size();
  for (size_t j = 0; j < (size_t)K * (size_t)n_; ++j)
    if (!std::isfinite(coeff[j])) throw std::runtime_error("hx_setvar_scenario_mix: a coefficient is not finite");
  std::vector<int> years((size_t)ns);
  for (int i = 0; i < ns; ++i) years[(size_t)i] = y0 + i;
  // every check of every mix first (its own shard's slice of one coefficient row suffices for the
  // shape; the values were checked above), then the mixes: nothing can be refused half way
  for (const auto &p : plan)
    for (Shard &s : shards_) {
      use(s);
      s.core->check_dated_mix(p.capability, years.data(), ns, p.basis.data(), K, coeff, nullptr);
    }
  for (const auto &p : plan) setvar_dated_mix(p.capability, years.data(), ns, p.basis.data(), K, coeff, nullptr);
  return (int)plan.size();
}
void Fleet::lane_of_member(int *out) {
  for (Shard &s : shards_) { use(s); s.core->lane_of_member(out + s.offset); }
}
void Fleet::reset(double date) { each_parallel([&](Shard &s) { s.core->reset(date); }); }
void Fleet::run(double runtodate) { each_parallel([&](Shard &s) { s.core->run(runtodate); }); }
void Fleet::sync() { each_parallel([&](Shard &s) { s.core->sync(); }); }

void Fleet::fetchvars(const std::string &cap, int year0, int year1, double *out_host) {
  if (shards_.size() == 1) { shards_[0].core->fetchvars(cap, year0, year1, out_host); return; }
  const int ny = year1 - year0 + 1;
  if (ny < 1) throw std::runtime_error("fetchvars: year1 < year0");
  // every shard copies its block of members straight into its columns of out_host
  each_parallel([&](Shard &s) { s.core->fetchvars(cap, year0, year1, out_host + s.offset, (size_t)n_); });
}

const double *Fleet::device_var(const std::string &cap, int *npad, int shard_index) {
  if (shard_index < 0) {
    if (shards_.size() > 1)
      throw std::runtime_error("hx_device_var: this core spans several GPUs -- ask for one shard's "
                               "array with hx_device_var_shard");
    shard_index = 0;
  }
  return shard(shard_index).device_var(cap, npad);
}

void Fleet::stats_device(const std::string &cap, int year0, int year1, double *d_stats) {
  if (shards_.size() == 1 && !comm_ready_) { shards_[0].core->stats_device(cap, year0, year1, d_stats); return; }
  ensemble_stats({cap}, year0, year1, nullptr, d_stats);
}

void Fleet::status(unsigned *out) { for (Shard &s : shards_) { use(s); s.core->status(out + s.offset); } }

int Fleet::member_score(const std::string &cap, const int *years, const double *obs, const double *sigma,
                        int n, int base_year0, int base_year1, double *out) {
  check_poison();
  int used = 0;
  for (Shard &s : shards_) {
    use(s);
    used = s.core->member_score(cap, years, obs, sigma, n, base_year0, base_year1, out + s.offset);
  }
  return used;
}

void Fleet::member_score_whitened(const std::string &cap, const int *years, const double *obs,
                                  const double *whiten, int n, int base_year0, int base_year1, double *out) {
  check_poison();
  for (Shard &s : shards_) {
    use(s);
    s.core->member_score_whitened(cap, years, obs, whiten, n, base_year0, base_year1, out + s.offset);
  }
}

void Fleet::member_project(const std::string &cap, const int *years, const double *center, const double *basis,
                           int n, int m, int base_year0, int base_year1, double *out) {
  check_poison();
  for (Shard &s : shards_) {   // every shard copies its members straight into its columns of out[m][n_]
    use(s);
    s.core->member_project(cap, years, center, basis, n, m, base_year0, base_year1, out + s.offset, (size_t)n_);
  }
}

void Fleet::quantise_weights(const double *weights, const char *fn, std::vector<unsigned long long> &q) const {
  // integer weights: q = rint(w / wmax * 2^32), wmax over ALL shards
  q.clear();
  if (!weights) return;
  const std::string f(fn);
  double wmax = 0.0;
  for (int m = 0; m < n_; ++m) {
    const double w = weights[m];
    if (!(w >= 0.0) || std::isinf(w))
      throw std::runtime_error(f + ": a weight is negative, NaN or infinite");
    wmax = std::max(wmax, w);
  }
  if (!(wmax > 0.0)) throw std::runtime_error(f + ": the weights are all zero");
  q.resize((size_t)n_);
  unsigned long long total = 0;
  for (int m = 0; m < n_; ++m) {
    q[(size_t)m] = (unsigned long long)std::rint(weights[m] / wmax * 4294967296.0);
    total += q[(size_t)m];
  }
  if (total > (1ull << 52))
    throw std::runtime_error(f + ": more than 2^20 weighted members");
}

void Fleet::refuse_processes(const char *fn, const char *what) const {
  if (comm_ready_ && world_ > n_shards())
    throw std::runtime_error(std::string(fn) + ": this core joined a communicator of several "
                             "processes (hx_comm_init_rank with n_procs > 1); " + what +
                             " over processes are not supported");
}

static void check_probs(const double *probs, int nprobs, const char *fn) {
  const std::string f(fn);
  if (nprobs < 1 || nprobs > 16 || !probs)
    throw std::runtime_error(f + ": nprobs must lie in 1..16");
  for (int j = 0; j < nprobs; ++j)
    if (!(probs[j] >= 0.0 && probs[j] <= 1.0))
      throw std::runtime_error(f + ": a probability outside [0, 1]");
}

// nspecs of a metric or pair source held to its range -> the rows of the source.  A year window may
// still be empty: "year1 < year0" is refused behind the weights.
static int source_rows(const RowSource &rs) {
  if (!rs.specs && !rs.pair) return rs.year1 - rs.year0 + 1;
  const int nspecs = rs.pair ? rs.pair->nspecs : rs.nspecs;
  if (nspecs < 1 || nspecs > HX_MET_MAX_SPECS || (rs.pair && !rs.pair->specs))
    throw std::runtime_error(std::string(rs.fn) + ": nspecs must lie in 1..32");
  return nspecs;
}

// a shard's four-word row records {~min key, max key, sum q, count} into the totals
static void fold_records(std::vector<unsigned long long> &st, const std::vector<unsigned long long> &part) {
  for (size_t y = 0; y < st.size() / 4; ++y) {
    if (!part[4 * y + 3]) continue;
    st[4 * y] = std::max(st[4 * y], part[4 * y]);
    st[4 * y + 1] = std::max(st[4 * y + 1], part[4 * y + 1]);
    st[4 * y + 2] += part[4 * y + 2];
    st[4 * y + 3] += part[4 * y + 3];
  }
}

// the labels of a grouped call: -1 .. ngroups-1, one of them >= 0 (an ungrouped call passes)
void Fleet::check_groups(const char *fn, const Groups &g) const {
  if (!g.labels && !g.ngroups) return;
  const std::string f(fn);
  if (!g.labels) throw std::runtime_error(f + ": labels is NULL");
  if (g.ngroups < 1 || g.ngroups > HX_GROUP_MAX) throw std::runtime_error(f + ": ngroups must lie in 1..16");
  bool any = false;
  for (int m = 0; m < n_; ++m) {
    if (g.labels[m] < -1 || g.labels[m] >= g.ngroups)
      throw std::runtime_error(f + ": label " + std::to_string(g.labels[m]) + " of member " + std::to_string(m) +
                               " lies outside -1.." + std::to_string(g.ngroups - 1));
    any = any || g.labels[m] >= 0;
  }
  if (!any) throw std::runtime_error(f + ": no member has a label >= 0");
}

void Fleet::quantiles(const RowSource &rs, const Groups &g, const double *weights, const double *probs,
                      int nprobs, double *out, long long *n_part) {
  check_poison();
  const int nrows = source_rows(rs);
  check_probs(probs, nprobs, rs.fn);
  check_groups(rs.fn, g);
  refuse_processes(rs.fn, "quantiles");
  std::vector<unsigned long long> q;
  quantise_weights(weights, rs.fn, q);
  const unsigned long long *qp = weights ? q.data() : nullptr;
  if (shards_.size() == 1) {   // (an empty year window: the core's own date check speaks)
    use(shards_[0]);
    shards_[0].core->quantiles(rs, g, qp, probs, nprobs, out, n_part);
    return;
  }
  if (nrows < 1) throw std::runtime_error(std::string(rs.fn) + ": year1 < year0");
  select_rows(std::max(g.ngroups, 1) * nrows, qp, probs, nprobs, out, n_part,
              [&](Shard &s, const unsigned long long *qs, unsigned long long *part) {
                s.core->q_begin(rs, of_shard(g, s), qs, nprobs, part);
              });
}

void Fleet::member_pair_metrics(const std::string &cap_a, const PairCall &pc, double *out) {
  check_poison();
  for (Shard &s : shards_) {   // every shard copies its members straight into its columns of out[nspecs][n_]
    use(s);
    s.core->member_pair_metrics(cap_a, pc, out + s.offset, (size_t)n_);
  }
}

void Fleet::select_rows(int ny, const unsigned long long *qp, const double *probs, int np, double *out,
                        long long *n_part,
                        const std::function<void(Shard &, const unsigned long long *, unsigned long long *)> &begin) {
  const size_t Y = (size_t)ny, YP = Y * (size_t)np;
  std::vector<unsigned long long> st(4 * Y, 0ull), part(4 * Y);
  for (Shard &s : shards_) {
    use(s);
    begin(s, qp ? qp + s.offset : nullptr, part.data());
    fold_records(st, part);
  }
  std::vector<int> lo(Y);
  std::vector<unsigned long long> prefix(YP), rem(YP), hist(YP * 256), hpart(YP * 256);
  bool open = false;
  for (size_t y = 0; y < Y; ++y) {
    unsigned long long pre;
    lo[y] = hxq_host_start(&st[4 * y], &pre);
    open = open || lo[y] > 0;
    for (int j = 0; j < np; ++j) {
      prefix[y * np + j] = pre;
      rem[y * np + j] = hxq_host_target(probs[j], st[4 * y + 2]);
    }
  }
  while (open) {
    std::fill(hist.begin(), hist.end(), 0ull);
    for (Shard &s : shards_) {
      use(s);
      s.core->q_pass(lo.data(), prefix.data(), hpart.data());
      for (size_t i = 0; i < hist.size(); ++i) hist[i] += hpart[i];
    }
    open = false;
    for (size_t y = 0; y < Y; ++y) {
      if (lo[y] == 0) continue;
      int owner[16];   // the first probability with the same prefix holds the histogram
      for (int j = 0; j < np; ++j) {
        owner[j] = j;
        for (int k = 0; k < j; ++k) if (prefix[y * np + k] == prefix[y * np + j]) { owner[j] = k; break; }
      }
      for (int j = 0; j < np; ++j)
        hxq_host_pick(lo[y], &hist[(y * np + (size_t)owner[j]) * 256], &prefix[y * np + j], &rem[y * np + j]);
      lo[y] = lo[y] >= 8 ? lo[y] - 8 : 0;
      open = open || lo[y] > 0;
    }
  }
  for (size_t y = 0; y < Y; ++y) {
    if (n_part) n_part[y] = (long long)st[4 * y + 3];
    for (int j = 0; j < np; ++j)
      out[y * np + j] = st[4 * y + 3] ? hxq_key_to_double(prefix[y * np + j]) : std::nan("");
  }
}

void Fleet::member_metrics(const std::string &cap, const hx_metric *specs, int nspecs, double *out) {
  check_poison();
  if (shards_.size() == 1) {
    use(shards_[0]);
    shards_[0].core->member_metrics(cap, specs, nspecs, out);
    return;
  }
  if (nspecs < 1 || nspecs > HX_MET_MAX_SPECS || !specs)
    throw std::runtime_error("hx_member_metrics: nspecs must lie in 1..32");
  std::vector<double> part;
  for (Shard &s : shards_) {   // a shard returns [nspecs][its members]; out is [nspecs][n_]
    use(s);
    part.resize((size_t)nspecs * (size_t)s.count);
    s.core->member_metrics(cap, specs, nspecs, part.data());
    for (int k = 0; k < nspecs; ++k)
      std::copy(part.begin() + (size_t)k * s.count, part.begin() + (size_t)(k + 1) * s.count,
                out + (size_t)k * n_ + s.offset);
  }
}

void Fleet::probabilities(const RowSource &rs, const Groups &g, const double *weights, const double *edges,
                          int nedges, double *prob, unsigned long long *sums, long long *n_part) {
  check_poison();
  const char *fn = rs.fn;
  const std::string f(fn);
  const int nrows = source_rows(rs);
  if (nedges < 1 || nedges > HX_BIN_MAX_EDGES || !edges)
    throw std::runtime_error(f + ": nedges must lie in 1..31");
  for (int k = 0; k < nedges; ++k) {
    if (!std::isfinite(edges[k])) throw std::runtime_error(f + ": an edge is not finite");
    if (k && !(edges[k] > edges[k - 1])) throw std::runtime_error(f + ": the edges are not strictly ascending");
  }
  check_groups(fn, g);
  refuse_processes(fn, "probabilities");
  std::vector<unsigned long long> q;
  quantise_weights(weights, fn, q);
  const unsigned long long *qp = weights ? q.data() : nullptr;
  if (nrows < 1) throw std::runtime_error(f + ": year1 < year0");
  const size_t stride = (size_t)nedges + 2, R = (size_t)std::max(g.ngroups, 1) * (size_t)nrows;
  std::vector<unsigned long long> tot(R * stride, 0ull), part(R * stride);
  for (Shard &s : shards_) {
    use(s);
    s.core->bin_sums(rs, of_shard(g, s), qp ? qp + s.offset : nullptr, edges, nedges, part.data());
    for (size_t i = 0; i < tot.size(); ++i) tot[i] += part[i];
  }
  const size_t B = (size_t)nedges + 1;
  for (size_t r = 0; r < R; ++r) {
    const unsigned long long *t = &tot[r * stride];
    unsigned long long W = 0;
    for (size_t b = 0; b < B; ++b) W += t[b];
    if (n_part) n_part[r] = (long long)t[B];
    for (size_t b = 0; b < B; ++b) {
      if (sums) sums[r * B + b] = t[b];
      prob[r * B + b] = t[B] ? (double)t[b] / (double)W : std::nan("");
    }
  }
}

void Fleet::moments(const RowSource &rs, const Groups &g, const double *weights, const double *predictors,
                    int npred, double *shift, double *pshift, double *sums, unsigned long long *wsum,
                    long long *n_part) {
  check_poison();
  const char *fn = rs.fn;
  const std::string f(fn);
  const int nrows = source_rows(rs);
  if (npred < 0 || npred > HX_MOM_MAX_PRED)
    throw std::runtime_error(f + ": npred must lie in 0..8");
  if (npred > 0 && !predictors)
    throw std::runtime_error(f + ": predictors is NULL with npred > 0");
  check_groups(fn, g);
  refuse_processes(fn, "moments");
  std::vector<unsigned long long> q;
  quantise_weights(weights, fn, q);
  if (!weights) q.assign((size_t)n_, 1ull);
  if (nrows < 1) throw std::runtime_error(f + ": year1 < year0");
  // the call's effective weights, and every group's predictor shifts over the members they leave it
  // (an ungrouped call: one group of every member)
  const size_t N = (size_t)n_, K = (size_t)npred, G = (size_t)std::max(g.ngroups, 1), R = G * (size_t)nrows;
  const size_t nc = 2 + 3 * K;
  // (predictor by predictor: the loops stream through one array each)
  for (size_t k = 0; k < K; ++k)
    for (size_t m = 0; m < N; ++m)
      if (!std::isfinite(predictors[k * N + m])) q[m] = 0;
  if (g.ngroups)
    for (size_t m = 0; m < N; ++m)
      if (g.labels[m] < 0) q[m] = 0;
  std::vector<double> c(G * HX_MOM_MAX_PRED, std::nan(""));
  for (size_t k = 0; k < K; ++k)
    for (size_t m = 0; m < N; ++m) {
      if (!q[m]) continue;   // (among them every label -1)
      double &ck = c[(g.ngroups ? (size_t)g.labels[m] : 0) * HX_MOM_MAX_PRED + k];
      if (!(ck <= predictors[k * N + m])) ck = predictors[k * N + m];
    }
  // 1. every shard's minimum, W and count of every row; the minimum over the shards is the shift
  std::vector<unsigned long long> st(4 * R, 0ull), part(4 * R);
  std::vector<double> pred;
  for (Shard &s : shards_) {
    use(s);
    pred.resize(K * (size_t)s.count);
    for (size_t k = 0; k < K; ++k)
      std::copy(predictors + k * N + (size_t)s.offset, predictors + k * N + (size_t)(s.offset + s.count),
                pred.begin() + k * (size_t)s.count);
    s.core->mom_begin(rs, of_shard(g, s), q.data() + s.offset, pred.data(), npred, c.data(), part.data());
    fold_records(st, part);
  }
  for (size_t y = 0; y < R; ++y) {
    shift[y] = st[4 * y + 3] ? hxq_key_to_double(~st[4 * y]) : std::nan("");
    if (wsum) wsum[y] = st[4 * y + 2];
    if (n_part) n_part[y] = (long long)st[4 * y + 3];
  }
  if (pshift)
    for (size_t gi = 0; gi < G; ++gi)
      for (size_t k = 0; k < K; ++k) pshift[gi * K + k] = c[gi * HX_MOM_MAX_PRED + k];
  // 2. every shard's sums about those shifts, added in ascending shard order
  std::fill(sums, sums + R * nc, 0.0);
  std::vector<double> sp(R * nc);
  for (Shard &s : shards_) {
    use(s);
    s.core->mom_finish(shift, sp.data());
    for (size_t i = 0; i < R * nc; ++i) sums[i] += sp[i];
  }
}

void Fleet::sobol(const RowSource &rs, int k, int n_base, const unsigned char *use_group, double *shift,
                  double *sums, long long *n_part) {
  check_poison();
  const char *fn = rs.fn;
  const std::string f(fn);
  source_rows(rs);   // (nspecs held to its range; a window's years are held by rows_check below)
  if (k < 1 || k > HX_SOBOL_MAX_FACTORS)
    throw std::runtime_error(f + ": k must lie in 1..16");
  if (n_base < 1) throw std::runtime_error(f + ": n_base must be at least 1");
  if ((long long)n_base * (long long)(k + 2) > (long long)n_)
    throw std::runtime_error(f + ": n_base * (k + 2) = " + std::to_string((long long)n_base * (k + 2)) +
                             " exceeds the " + std::to_string(n_) + " members of the core");
  refuse_processes(fn, "Sobol sums");
  // the first shard answers for capability, dates and a core that has not run (the host-emulation
  // build refuses by name there); k and n_base were held to the whole core above
  Shard &s = shards_.front();
  use(s);
  s.core->rows_check(rs, Groups{nullptr, 0}, 1);
  if (shards_.size() > 1)
    throw std::runtime_error(f + ": this core has several shards (" + std::to_string(shards_.size()) +
                             "): the members of a group lie on different GPUs under the fleet's split, "
                             "which the Sobol verbs do not serve");
  s.core->sobol_begin(rs, k, n_base, use_group);
  s.core->sobol_finish(shift, sums, n_part);
}

void Fleet::comoments(const std::string &cap_a, int a0, int a1, const char *cap_b, int b0, int b1,
                      const double *weights, double *shift_a, double *sums_a, double *shift_b, double *sums_b,
                      double *cross, unsigned long long *wsum, long long *n_part) {
  check_poison();
  const char *fn = "hx_ensemble_comoments";
  refuse_processes(fn, "co-moments");
  std::vector<unsigned long long> q;
  quantise_weights(weights, fn, q);
  if (!weights) q.assign((size_t)n_, 1ull);
  const bool sym = cap_b == nullptr;
  const std::string sb = sym ? std::string() : std::string(cap_b);
  // (the windows are held to the scenario's rows before anything is sized from them)
  use(shards_.front());
  shards_.front().core->comom_check(cap_a, a0, a1, sym ? nullptr : &sb, b0, b1);
  const size_t na = (size_t)(a1 - a0 + 1), nb = sym ? na : (size_t)(b1 - b0 + 1), R = sym ? na : na + nb;
  // 1. every shard's mask, and the minimum, W and count of every row; the minimum over the shards is
  //    the shift.  (Complete cases: W and the count are those of any row.)
  std::vector<unsigned long long> st(4 * R, 0ull), part(4 * R);
  for (Shard &s : shards_) {
    use(s);
    s.core->comom_begin(cap_a, a0, a1, sym ? nullptr : &sb, b0, b1, q.data() + s.offset, part.data());
    fold_records(st, part);
  }
  std::vector<double> shift(R);
  for (size_t y = 0; y < R; ++y) shift[y] = st[4 * y + 3] ? hxq_key_to_double(~st[4 * y]) : std::nan("");
  // 2. every shard's sums about the common shifts, added in ascending shard order
  std::vector<double> sums(2 * R, 0.0), sp(2 * R), cp(na * nb);
  std::fill(cross, cross + na * nb, 0.0);
  for (Shard &s : shards_) {
    use(s);
    s.core->comom_finish(shift.data(), sp.data(), cp.data());
    for (size_t i = 0; i < 2 * R; ++i) sums[i] += sp[i];
    for (size_t i = 0; i < na * nb; ++i) cross[i] += cp[i];
  }
  if (sym) for (size_t a = 0; a < na; ++a) sums[2 * a + 1] = cross[a * nb + a];
  std::copy(shift.begin(), shift.begin() + na, shift_a);
  std::copy(sums.begin(), sums.begin() + 2 * na, sums_a);
  if (shift_b) std::copy(shift.begin() + (sym ? 0 : na), shift.begin() + (sym ? na : R), shift_b);
  if (sums_b) std::copy(sums.begin() + (sym ? 0 : 2 * na), sums.begin() + (sym ? 2 * na : 2 * R), sums_b);
  if (wsum) *wsum = st[2];
  if (n_part) *n_part = (long long)st[3];
}

void Fleet::series_define(const std::string &name, const std::string &a, const hx_series_op &op) {
  HX_EACH(series_define(name, a, op))
}
void Fleet::series_eval(const std::string &name, const hx_expr &ex) {
  // every shard takes its slice of the member vectors (a table the program cannot use is the shard's
  // to refuse: nothing is read from it here)
  const bool sliced = ex.members && ex.nmem > 0 && ex.nmem <= HX_EX_MAX_MEMBERS;
  const double *mem[HX_EX_MAX_MEMBERS];
  hx_expr part = ex;
  HX_EACH_DO("series_eval(name, expr)", {
    if (sliced) {
      for (int i = 0; i < ex.nmem; ++i) mem[i] = ex.members[i] ? ex.members[i] + s.offset : nullptr;
      part.members = mem;
    }
    s.core->series_eval(name, part);
  })
}
void Fleet::series_drop(const std::string &name) { HX_EACH(series_drop(name)) }

// The three rank verbs share their refusals: the first shard answers for the capability, the dates or
// specifications and a core that has not run (the host-emulation build refuses by name there), then
// a core of several shards is refused -- the sort needs the whole row on one GPU
EnsembleCore &Fleet::rank_shard(const char *fn, const std::string &cap, int year0, int year1,
                                const hx_metric *specs, int nspecs) {
  refuse_processes(fn, "ranks");
  Shard &s = shards_.front();
  use(s);
  s.core->rows_check(RowSource{fn, cap, year0, year1, specs, nspecs, nullptr}, Groups{nullptr, 0}, 1);
  if (shards_.size() > 1)
    throw std::runtime_error(std::string(fn) + ": this core has several shards (" +
                             std::to_string(shards_.size()) + "): a rank needs the whole row of members on "
                             "one GPU, which the rank verbs do not serve");
  return *s.core;
}

static void check_rank_kind(const char *fn, int kind) {
  if (kind != HX_RANK_PIT && kind != HX_RANK_NUMERATOR)
    throw std::runtime_error(std::string(fn) + ": unknown kind " + std::to_string(kind) +
                             " (HX_RANK_PIT or HX_RANK_NUMERATOR)");
}

void Fleet::series_rank(const std::string &name, const std::string &cap, int year0, int year1,
                        const double *weights, int kind) {
  check_poison();
  const char *fn = "hx_series_rank";
  check_rank_kind(fn, kind);
  std::vector<unsigned long long> q;
  quantise_weights(weights, fn, q);
  rank_shard(fn, cap, year0, year1, nullptr, 0).series_rank(name, cap, year0, year1, weights ? q.data() : nullptr,
                                                            kind);
}

void Fleet::metric_ranks(const std::string &cap, const hx_metric *specs, int nspecs, const double *weights,
                         int kind, double *out) {
  check_poison();
  const char *fn = "hx_metric_ranks";
  if (nspecs < 1 || nspecs > HX_MET_MAX_SPECS || !specs)
    throw std::runtime_error(std::string(fn) + ": nspecs must lie in 1..32");
  check_rank_kind(fn, kind);
  std::vector<unsigned long long> q;
  quantise_weights(weights, fn, q);
  rank_shard(fn, cap, 0, 0, specs, nspecs).metric_ranks(cap, specs, nspecs, weights ? q.data() : nullptr, kind, out);
}

void Fleet::crps(const std::string &cap, const int *years, const double *obs, int nyears, const double *weights,
                 double *crps_out, double *pit_obs, long long *n_part) {
  check_poison();
  const char *fn = "hx_ensemble_crps";
  if (nyears < 1) throw std::runtime_error(std::string(fn) + ": nyears < 1");
  std::vector<unsigned long long> q;
  quantise_weights(weights, fn, q);
  const int y0 = *std::min_element(years, years + nyears), y1 = *std::max_element(years, years + nyears);
  rank_shard(fn, cap, y0, y1, nullptr, 0).crps(cap, years, obs, nyears, weights ? q.data() : nullptr, crps_out,
                                               pit_obs, n_part);
}

void Fleet::state_row(int row, double *out) {
  for (Shard &s : shards_) { use(s); s.core->state_row(row, out + s.offset); }
}
int Fleet::spinup_steps(int member) {
  Shard &s = shards_[(size_t)shard_of_member(member)];
  use(s);
  return s.core->spinup_steps(member - s.offset);
}
void Fleet::tracking_data(int member, int year0, int year1, double *values, double *fractions,
                          unsigned long long *source_masks) {
  Shard &s = shards_[(size_t)shard_of_member(member)];
  use(s);
  s.core->tracking_data(member - s.offset, year0, year1, values, fractions, source_masks);
}
int Fleet::wave_clock(int shard_index, long long *ticks, int cap) {
  Shard &s = shards_[(size_t)shard_index];
  use(s);
  return s.core->wave_clock(ticks, cap);
}
int Fleet::wave_epilogue_clock(int shard_index, long long *ticks, int cap) {
  Shard &s = shards_[(size_t)shard_index];
  use(s);
  return s.core->wave_epilogue_clock(ticks, cap);
}
double Fleet::last_run_kernel_ms() {
  double ms = 0;
  for (Shard &s : shards_) { use(s); s.core->sync(); ms = std::max(ms, s.core->last_run_kernel_ms()); }
  return ms;
}
double Fleet::last_spinup_ms() {
  double ms = 0;
  for (Shard &s : shards_) ms = std::max(ms, s.core->last_spinup_ms());
  return ms;
}

// ---- the collective ----------------------------------------------------------------------------

void Fleet::unique_id(char *id_out) {
#ifndef HX_HOST_EMULATION
  ncclUniqueId id;
  nccl_ck(rccl().GetUniqueId(&id), "ncclGetUniqueId");
  static_assert(sizeof(id.internal) == 128, "ncclUniqueId is 128 bytes");
  std::memcpy(id_out, id.internal, sizeof(id.internal));
#else
  (void)id_out;
  throw std::runtime_error("the host-emulation build has no RCCL");
#endif
}

const char *Fleet::comm_backend() const {
  if (!comm_ready_) return "none";
  if (duplicates_) return "device-copies (rehearsal: a device is listed twice)";
#ifndef HX_HOST_EMULATION
  static thread_local std::string s;
  int v = 0;
  (void)rccl().GetVersion(&v);
  s = "rccl " + std::to_string(v) + " via " + rccl().origin;
  return s.c_str();
#else
  return "none";
#endif
}

void Fleet::comm_init_rank(int n_procs, int proc_rank, const char *id_bytes) {
  if (comm_ready_) throw std::runtime_error("hx_comm_init_rank: this core already has a communicator");
  if (n_procs < 1 || proc_rank < 0 || proc_rank >= n_procs || !id_bytes)
    throw std::runtime_error("hx_comm_init_rank: bad arguments");
  if (duplicates_) {
    if (n_procs != 1)
      throw std::runtime_error("hx_comm_init_rank: a rehearsal core (duplicate devices) cannot join "
                               "other processes");
    world_ = n_shards(); first_rank_ = 0; comm_ready_ = true;
    return;
  }
#ifndef HX_HOST_EMULATION
  Rccl &r = rccl();
  ncclUniqueId id;
  std::memcpy(id.internal, id_bytes, sizeof(id.internal));
  const int L = n_shards();
  world_ = n_procs * L;
  first_rank_ = proc_rank * L;
  // (inside a group ncclCommInitRank writes the handle when the group ends: the slots it writes to
  // must outlive the calls, hence one array for all shards)
  std::vector<ncclComm_t> comms((size_t)L, nullptr);
  try {
    {
      RcclGroup group(r, L > 1);
      for (int s = 0; s < L; ++s) {
        hip_ck(hipSetDevice(shards_[(size_t)s].device), "hipSetDevice");
        nccl_ck(r.CommInitRank(&comms[(size_t)s], world_, id, first_rank_ + s), "ncclCommInitRank");
      }
      group.end();
    }
    for (int s = 0; s < L; ++s)
      if (!comms[(size_t)s]) throw std::runtime_error("ncclCommInitRank returned no communicator");
    for (int s = 0; s < L; ++s) shards_[(size_t)s].comm = comms[(size_t)s];
    free_stats_buffers();  // sized for the old world
  } catch (...) {
    // communicators that did come to life are torn down, not leaked (abort: their peers may never
    // have arrived, a destroy could wait for them)
    for (int s = 0; s < L; ++s)
      if (comms[(size_t)s]) { (void)hipSetDevice(shards_[(size_t)s].device); (void)r.CommAbort(comms[(size_t)s]); }
    for (Shard &s : shards_) s.comm = nullptr;
    world_ = 1; first_rank_ = 0;
    throw;
  }
  comm_ready_ = true;
#else
  throw std::runtime_error("the host-emulation build has no RCCL");
#endif
}

void Fleet::ensure_comm() {
  if (comm_ready_ || shards_.size() == 1) return;
  if (duplicates_) { world_ = n_shards(); first_rank_ = 0; comm_ready_ = true; return; }
  char id[128];
  unique_id(id);  // one process owns every rank: what ncclCommInitAll does
  comm_init_rank(1, 0, id);
}

void Fleet::free_stats_buffers() {
  for (Shard &s : shards_) {
    if (!s.d_local && !s.d_slots && !s.d_result) continue;
    (void)hipSetDevice(s.device);
    if (s.d_local) (void)hipFree(s.d_local);
    if (s.d_slots) (void)hipFree(s.d_slots);
    if (s.d_result) (void)hipFree(s.d_result);
    s.d_local = s.d_slots = s.d_result = nullptr;
  }
  stats_cap_ = 0;
}

void Fleet::ensure_stats_buffers(size_t blk) {
  if (blk <= stats_cap_) return;
  free_stats_buffers();
  for (Shard &s : shards_) {
    use(s);
    hip_ck(hipMalloc(&s.d_local, sizeof(double) * blk), "hipMalloc stats block");
    hip_ck(hipMalloc(&s.d_slots, sizeof(double) * blk * (size_t)world_), "hipMalloc stats slots");
    hip_ck(hipMalloc(&s.d_result, sizeof(double) * blk), "hipMalloc stats result");
  }
  stats_cap_ = blk;
}

void Fleet::ensemble_stats(const std::vector<std::string> &caps, int year0, int year1,
                           double *out_host, double *d_out) {
  if (caps.empty()) throw std::runtime_error("ensemble_stats: no variables");
  const int ny = year1 - year0 + 1;
  if (ny < 1) throw std::runtime_error("ensemble_stats: year1 < year0");
  ensure_comm();
  const int world = comm_ready_ ? world_ : 1;
  const size_t nv = caps.size(), rows = nv * (size_t)ny, blk = rows * 5;
  ensure_stats_buffers(blk);
  // One rank: its own block is the result (folding one slot copies it, bit for bit) -- reduced
  // straight into the caller's device buffer, no slot copy, no combine, no result copy.
  if (world == 1) {
    Shard &s = shards_[0];
    use(s);
    double *dst = d_out ? d_out : s.d_local;
    s.core->stats_async(caps, year0, year1, dst);
    if (out_host)
      hip_ck(hipMemcpyAsync(out_host, dst, sizeof(double) * blk, hipMemcpyDeviceToHost, s.core->stream()),
             "stats result to host");
    hip_ck(hipStreamSynchronize(s.core->stream()), "stats sync");
    return;
  }
  // 1. every shard reduces its own members on its own GPU, on its own stream
  for (Shard &s : shards_) {
    use(s);
    s.core->stats_async(caps, year0, year1, s.d_local);
  }
  // 2. the one collective: every rank receives every rank's block
  if (duplicates_) {
    for (Shard &s : shards_) { use(s); hip_ck(hipStreamSynchronize(s.core->stream()), "stats sync"); }
    for (Shard &dst : shards_) {
      use(dst);
      for (size_t r = 0; r < shards_.size(); ++r)
        hip_ck(hipMemcpyAsync(dst.d_slots + r * blk, shards_[r].d_local, sizeof(double) * blk,
                              hipMemcpyDeviceToDevice, dst.core->stream()), "stats exchange");
    }
  } else {
#ifndef HX_HOST_EMULATION
    Rccl &r = rccl();
    RcclGroup group(r, shards_.size() > 1);
    for (Shard &s : shards_) {
      use(s);
      nccl_ck(r.AllGather(s.d_local, s.d_slots, blk, ncclDouble, (ncclComm_t)s.comm, s.core->stream()),
              "ncclAllGather");
    }
    group.end();
#endif
  }
  // 3. combined in rank order on every rank: bit-identical everywhere
  for (Shard &s : shards_) {
    use(s);
    hip_ck(hx_launch_combine_stats(s.d_slots, world, (int)rows, s.d_result, s.core->stream()),
           "combine statistics");
  }
  Shard &s0 = shards_[0];
  use(s0);
  if (d_out)
    hip_ck(hipMemcpyAsync(d_out, s0.d_result, sizeof(double) * blk, hipMemcpyDeviceToDevice,
                          s0.core->stream()), "stats result");
  if (out_host)
    hip_ck(hipMemcpyAsync(out_host, s0.d_result, sizeof(double) * blk, hipMemcpyDeviceToHost,
                          s0.core->stream()), "stats result to host");
  for (Shard &s : shards_) { use(s); hip_ck(hipStreamSynchronize(s.core->stream()), "stats sync"); }
}

}  // namespace hx
