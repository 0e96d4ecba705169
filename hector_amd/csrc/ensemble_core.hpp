// ensemble_core.hpp -- host runtime for an N-member Hector ensemble on one GPU.
//
// Mirrors the reference's Core for the year-loop path (inst/include/core.hpp:37-114,
// src/core.cpp:302-549): init from an INI/scenario, setData through capability
// strings (incl. "<biome>.<var>"), prepareToRun (incl. spinup), run(runToDate)
// callable repeatedly with increasing dates, reset(date), getData -- except that
// every parameter and every result carries a member axis.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/hector_amd.h"   // hx_metric
#include "hx_layout.h"
#include "hx_post_abi.h"
#include "hx_scenario.hpp"

namespace hx {

// The process-wide registry of lane-cost models (ensemble_core.cpp, fit_cost_model) to / from a
// text file: -> number of models written / read, -1 if the file cannot be opened.
int hx_cost_models_export_file(const char *path);
int hx_cost_models_load_file(const char *path);

// The operands b and the specifications of a pair-metric call (hx_member_pair_metrics in
// hector_amd.h): exactly one of cap_b and b_vec[b_year0..b_year1] is set.
struct PairCall {
  const char *cap_b;
  const double *b_vec;
  int b_year0, b_year1;
  const hx_pair_metric *specs;
  int nspecs;
};

// The rows a summary verb works on.  fn is the ABI function named in every message.  specs and pair
// null: the years year0..year1 of capability; else its nspecs metrics, or the pair->nspecs pair
// metrics with capability as operand a.
struct RowSource {
  const char *fn;
  std::string capability;
  int year0, year1;
  const hx_metric *specs;
  int nspecs;
  const PairCall *pair;
};

// The groups of a grouped summary (hx_group_* in hector_amd.h): labels[n_] in member order,
// -1 .. ngroups-1 (checked by the fleet, whose shards take labels + offset); ngroups == 0: ungrouped.
// Every state and result array of a grouped call is group-major, (group, row) at g * nrows + row, so
// that hx_fleet.cpp combines shards over ngroups * nrows rows exactly as it does over rows.
struct Groups {
  const int *labels;
  int ngroups;
};

// How a mix of a dated input is evaluated: not at all, into the variable's table
// (hx_mseries_mix_kernel), by the gas pre-pass (hx_gas_mix_kernel) or by the aerosol / precursor
// pre-pass (hx_slcf_mix_kernel; taken only behind hx_enable_slcf_mixes)
enum MixFamily { MIX_NONE, MIX_TABLE, MIX_GAS, MIX_SLCF };
// A dated input as EnsembleCore::find_dated describes it; name empty = no such input
struct DatedInput {
  std::string name, sections[2];     // the one or two INI sections that hold the series
  std::string units;
  double dflt = 0.0;                 // the value where the scenario has no series
  int row = -1, lag = 0;             // HXM_* row of its per-member table (-1: none) and that table's lag
  MixFamily mix = MIX_NONE;
  int slcf = -1;                     // MIX_SLCF: the input's index in hx_slcf_mix_kernel, 0..6
  bool halocarbon = false;           // resolved from the scenario's halocarbons, not a row of the table
  explicit operator bool() const { return !name.empty(); }
};

class EnsembleCore {
 public:
  EnsembleCore(const std::string &scenario_path, int n_members, int device);
  ~EnsembleCore();
  EnsembleCore(const EnsembleCore &) = delete;
  EnsembleCore &operator=(const EnsembleCore &) = delete;

  int n_members() const { return n_; }
  int n_biomes() const { return B_; }
  int start_date() const { return scen_.start; }
  int end_date() const { return scen_.end; }
  int last_date() const { return scen_.start + last_iy_; }
  const std::vector<std::string> &biomes() const { return biome_names_; }

  // SETDATA for a model parameter: nvalues == 1 (all members) or n_members.
  // capability = reference capability string (component_data.hpp), optionally
  // "<biome>.<capability>".  units: "" / nullptr skips the check, otherwise it
  // must equal the reference's unit string for that variable (unitval.cpp).
  // Marks the core dirty from date 0 (spinup reruns if a spinup-relevant
  // parameter changed), like R/messages.R:107-140.
  void setvar(const std::string &capability, const double *values, int nvalues,
              const char *units);
  // current value of a parameter for every member (GETDATA without date)
  void getvar(const std::string &capability, double *out) const;

  // split_biome (R/biome.R:61-130): replace the single biome by n new ones,
  // pools and npp_flux0 partitioned by the given fractions (nullptr = equal),
  // other parameters copied; forces a re-spinup.
  void split_biome(const std::vector<std::string> &names, const double *fveg,
                   const double *fdet, const double *fsoil, const double *fpf,
                   const double *fnpp);
  void split_biome_of(const std::string &old_biome, const std::vector<std::string> &names,
                      const double *fveg, const double *fdet, const double *fsoil,
                      const double *fpf, const double *fnpp);
  // create_biome_impl / delete_biome_impl / rename_biome (src/rcpp_hector.cpp; SimpleNbox::
  // createBiome, deleteBiome, renameBiome): at most HX_BDYN biomes (1..HX_MAXB run unrolled
  // kernels, more the looped ones)
  void create_biome(const std::string &biome);
  void delete_biome(const std::string &biome);
  void rename_biome(const std::string &oldname, const std::string &newname);
  int biome_index(const std::string &biome) const;

  // which output variables are recorded per year (capability strings);
  // sst and land_tas are always recorded (the model needs their history).
  void set_outputs(const std::vector<std::string> &capabilities);
  // lane assignment: sort members by their perturbed parameters so that the lanes of a
  // wavefront follow similar solver schedules (default on; results do not depend on it)
  void set_member_sorting(bool on);
  // Lane order by MEASURED cost: the run kernel adds up what every member's solver did (dopri5
  // steps, stashes); after a run that covered startDate..endDate, the next reset(startDate)
  // reorders the lanes by it, costliest wavefronts first (they are dispatched first, so an
  // ensemble of more wavefronts than SIMDs ends on cheap ones), and spins up again.  Only for
  // ensembles of more wavefronts than the GPU has SIMDs (otherwise the launch lasts as long as
  // its costliest wavefront under any order).  Results do not depend on the order.  Default on; a parameter change falls back to the parameter key
  // until the next complete run.
  void set_lane_calibration(bool on) { calibrate_lanes_ = on; }
  bool lanes_calibrated() const { return !lane_cost_.empty(); }
  // what the lanes of the last upload are ordered by: 0 the parameter key, 1 this core's measured
  // cost, 2 the cost a model predicts that was fitted to an earlier core's measurements (same
  // scenario table, biome count and varying rows, this process; ensemble_core.cpp: fit_cost_model)
  int lane_order_source() const { return lane_order_source_; }
  void set_cost_model(bool on) { cost_model_ = on; }
  // the chip's clocks kept up while prepare() uploads and spins up after an idle gap, so that the
  // run kernel behind it does not start at ramping clocks (ensemble_core.cpp: prewarm_begin);
  // ms: the most the busy loop may last on the device's own clock, 0 = off
  void set_prewarm(int ms) { prewarm_ms_ = ms < 0 ? 0 : (ms > 200 ? 200 : ms); }
  int prewarm_ms() const { return prewarm_ms_; }
  bool last_run_prewarmed() const { return last_run_prewarmed_; }
  // keep every year's component state in HBM (272 B per member-year for one biome) so that
  // reset(date) can go back to any computed year, like the reference's tseries records
  void enable_history(bool on);
  // keep what the reference's output stream sees after every spinup step (its "spinup = 1" rows,
  // csv_outputstream_visitor.cpp:86-95): the carbon-cycle variables, max_spinup x 21 x 8 B per member
  void enable_spinup_record(bool on);
  // Let the mix verb, mix_capabilities() and plan_scenario_mix() take the aerosol and ozone / OH
  // precursor emissions as well (SO2, BC, OC, NH3, NOX, CO, NMVOC: hx_enable_slcf_mixes).  Off by
  // default, and free until such a mix is set; refused while one is.
  void enable_slcf_mixes(bool on);
  bool slcf_mixes_enabled() const { return slcf_on_; }
  // Let setvar take n_members values for the forcing efficacies delta_co2, delta_ch4, delta_n2o,
  // rho_bc, rho_oc, rho_so2, rho_nh3 (hx_enable_member_forcing).  Off by default; switching it off
  // is refused while one of them differs between members.
  void enable_member_forcing(bool on);
  bool member_forcing_enabled() const { return forcing_on_; }
  std::vector<std::string> member_forcing_names() const;   // those that differ between members now
  static const std::vector<std::string> &spinup_record_vars();
  // values[step * nvars + v] for steps 1..spinup_steps(member); returns the step count
  int spinup_record(int member, double *values, int max_steps);
  // SETDATA with dates for a scenario input series (emissions, SV, RF_albedo...): the same
  // new values for every member.  Like R/messages.R:107-140 the core becomes dirty from
  // min(year) - 1; the next run() resets there (needs the history) or to startDate.
  void setvar_dated(const std::string &capability, const int *years, const double *values,
                    int n, const char *units);
  void lane_of_member(int *out);
  // SETDATA with dates and a different value for every member (ffi_emissions, luc_emissions,
  // daccs_uptake, luc_uptake, CH4_emissions): values[i * n_members + member] for years[i] --
  // the reference's pattern of re-running a period with new emissions per run
  // (vignettes/ex_hector_apply.Rmd), for all members at once.
  void setvar_dated_members(const std::string &capability, const int *years, const double *values,
                            int nyears, const char *units);
  // The same as a mix of nbasis shared year-vectors (hx_setvar_dated_mix in hector_amd.h):
  // basis[k * nyears + i], coeff[k * n_members + member].  Kept as that recipe; prepare() expands
  // it into the device table.  nbasis == 0 removes the variable's mix.
  void setvar_dated_mix(const std::string &capability, const int *years, int nyears, const double *basis,
                        int nbasis, const double *coeff, const char *units);
  // every check of setvar_dated_mix, changing nothing (throws what it would throw)
  void check_dated_mix(const std::string &capability, const int *years, int nyears, const double *basis,
                       int nbasis, const double *coeff, const char *units) const;
  // the names setvar_dated_mix accepts for this core (the halocarbons are the scenario's)
  std::vector<std::string> mix_capabilities() const;
  // Whole scenarios as mixes (hx_setvar_scenario_mix): every dated input series in which one of
  // the scenarios differs from this core's, as {capability, basis[nscen][ns]} over
  // startDate..endDate.  Throws, naming section and key, if the scenarios cannot be members of
  // this core (dates, halocarbons, a scalar, an unmixable or missing series).  Changes nothing.
  struct ScenarioSeries { std::string capability; std::vector<double> basis; };
  std::vector<ScenarioSeries> plan_scenario_mix(const std::vector<std::string> &paths) const;
  static const char *const *output_capabilities(int *count);

  void reset(double date);      // Core::reset: date < startDate => redo spinup
  void run(double runtodate);   // Core::run; < 0 => endDate.  Asynchronous.
  void sync();                  // wait for the stream
  // GETDATA with dates: out[(year - year0) * n + member]
  void fetchvars(const std::string &capability, int year0, int year1, double *out_host,
                 size_t row_pitch = 0);
  bool host_output(const std::string &capability);
  // Carbon tracking (Core::trackingDate, get_tracking_data): origins of every pool's carbon from
  // `year` on.  year <= 0 or beyond endDate switches it off.
  void set_tracking_date(int year);
  int tracking_date() const { return tracking_year_; }
  std::vector<std::string> tracking_pools() const;
  // values[ny][TP], fractions[ny][TP][TP], source_masks[ny][TP] (bit s: source s is in the pool's
  // map; optional) of one member for year0..year1 (>= the tracking date)
  void tracking_data(int member, int year0, int year1, double *values, double *fractions,
                     unsigned long long *source_masks = nullptr);
  std::string run_name() const;
  void var_info(const std::string &capability, std::string *component, std::string *units) const;
  const std::vector<std::string> &halocarbon_names() const { return halo_names_; }
  // device pointer to the [ns][npad] array of an output variable
  const double *device_var(const std::string &capability, int *npad);
  // per-year ensemble statistics {count,sum,sumsq,min,max} into a DEVICE buffer
  // of (year1-year0+1)*5 doubles (caller-owned, e.g. a torch tensor for RCCL)
  void stats_device(const std::string &capability, int year0, int year1, double *d_stats);
  // the same, queued on the core's stream without waiting (the fleet's collective follows it)
  void stats_async(const std::string &capability, int year0, int year1, double *d_stats);
  // ... of several variables, d_stats[v][year][5]: those the run kernel left per-wavefront partials
  // for (stats_partials_var) share one combine launch, the others take hx_stats_kernel each
  void stats_async(const std::vector<std::string> &capabilities, int year0, int year1, double *d_stats);
  // ---- post-processing on the device (ensemble_post.cpp, hx_dev_post.h); both read results only: no prepare(), no
  // prewarm loop, no spinup, the core is not dirtied.  Scratch is allocated on first use.
  // chi2[member] of a recorded output against obs (hx_member_score in hector_amd.h): out_host[n_]
  // in member order; -> the number of observations that counted
  int member_score(const std::string &capability, const int *years, const double *obs,
                   const double *sigma, int n, int base_year0, int base_year1, double *out_host);
  // chi2[member] = |W r|^2 against obs with correlated errors (hx_member_score_whitened in
  // hector_amd.h): whiten[n x n] row-major, only k <= i read; out_host[n_] in member order
  void member_score_whitened(const std::string &capability, const int *years, const double *obs,
                             const double *whiten, int n, int base_year0, int base_year1, double *out_host);
  // out[j][member] = sum_k basis[j * n + k] r_k (hx_member_project in hector_amd.h): basis[m x n]
  // row-major, center nullptr = zeros; out_host row j at out_host + j * row_pitch (0: n_), member order
  void member_project(const std::string &capability, const int *years, const double *center,
                      const double *basis, int n, int m, int base_year0, int base_year1, double *out_host,
                      size_t row_pitch = 0);
  // per-member metrics (hx_member_metrics): out_host[nspecs][n_] in member order.  fn: the ABI
  // function on whose behalf the specifications are checked (it is named in every message)
  void member_metrics(const std::string &capability, const hx_metric *specs, int nspecs,
                      double *out_host, const char *fn = "hx_member_metrics");
  // per-member pair metrics (hx_member_pair_metrics): two operands of a member, PairCall above;
  // out_host row s at out_host + s * row_pitch (0: n_), member order
  void member_pair_metrics(const std::string &cap_a, const PairCall &pc, double *out_host, size_t row_pitch = 0);
  // ---- the summary verbs over a RowSource, per group if Groups says so.  rows below counts
  // max(ngroups, 1) * nrows, group-major; q[n_] are integer weights in member order.
  // Every check of a source, and nothing else: capability, dates or specifications, nprobs (1 for a
  // verb without probabilities), a core that has not run -> the block the rows are read in or computed
  // from (*src_b: operand b of a pair call).  A year window tests nprobs before it resolves the
  // capability, the metric and pair sources after their specifications.  The host-emulation build
  // refuses by rs.fn here: at once, or for a pair or grouped call behind the checks.
  const double *rows_check(const RowSource &rs, const Groups &g, int nprobs, const double **src_b = nullptr);
  // weighted quantiles (hx_ensemble_quantiles, hx_metric_quantiles, hx_pair_metric_quantiles,
  // hx_group_quantiles): the whole select on this core's GPU.  q nullptr: every member 1;
  // out_host[rows][nprobs], n_part[rows] (may be nullptr)
  void quantiles(const RowSource &rs, const Groups &g, const unsigned long long *q, const double *probs,
                 int nprobs, double *out_host, long long *n_part);
  // ... and its steps for a core of several shards (hx_fleet.cpp adds the shards' integer
  // histograms): q_begin validates, uploads q and reduces {~min key, max key, sum q, count} of
  // every row into st_host[rows][4]; q_pass fills hist_host[rows][nprobs][256] for the select state
  // lo[rows], prefix[rows][nprobs] (hxq_* below)
  void q_begin(const RowSource &rs, const Groups &g, const unsigned long long *q, int nprobs,
               unsigned long long *st_host);
  void q_pass(const int *lo, const unsigned long long *prefix, unsigned long long *hist_host);
  // weighted bin sums (hx_ensemble_probabilities and its metric, pair and group forms): this core's
  // integer sums_host[rows][nedges + 2] = the nedges + 1 bins, then the members that took part.  The
  // edges are checked by the fleet (1..31, finite, strictly ascending)
  void bin_sums(const RowSource &rs, const Groups &g, const unsigned long long *q, const double *edges,
                int nedges, unsigned long long *sums_host);
  // weighted moments (hx_ensemble_moments and its forms), in the two steps hx_fleet.cpp drives for
  // one shard or several.  mom_begin validates, brings q[n_] (effective integer weights: 0 where a
  // predictor is not finite or the label is -1) and pred[npred][n_] (member order) to lane order with
  // the predictor shifts c[max(ngroups, 1)][8] subtracted, and reduces {~min key, max key, sum q,
  // count} of every row into st_host[rows][4]; mom_finish takes the rows' shifts over ALL shards,
  // shift_host[rows], and returns this core's sums_host[rows][2 + 3 npred]
  void mom_begin(const RowSource &rs, const Groups &g, const unsigned long long *q, const double *pred,
                 int npred, const double *c, unsigned long long *st_host);
  void mom_finish(const double *shift_host, double *sums_host);
  // year-by-year co-moments (hx_ensemble_comoments), in the same two steps.  comom_begin validates
  // both windows (cap_b == nullptr: the symmetric call, B is A), brings q[n_] to lane order, zeroes
  // it where any value of either window is NaN (complete cases) and reduces the rows' records into
  // st_host[na (+ nb)][4]; comom_finish takes the rows' shifts over ALL shards and returns this
  // core's sums_host[na (+ nb)][2] and cross_host[na][nb].  No prepare(), no spinup, not dirtied.
  // comom_check is the validation alone: the caller sizes its buffers from windows that passed it.
  void comom_check(const std::string &cap_a, int a0, int a1, const std::string *cap_b, int b0, int b1);
  void comom_begin(const std::string &cap_a, int a0, int a1, const std::string *cap_b, int b0, int b1,
                   const unsigned long long *q, unsigned long long *st_host);
  void comom_finish(const double *shift_host, double *sums_host, double *cross_host);
  // Sobol sums of a Saltelli design (hx_ensemble_sobol; rs.specs != nullptr: hx_metric_sobol over the
  // metric block), one shard only: a group's k + 2 consecutive members must all live on this core.
  // rows_check is the validation alone; sobol_begin validates, turns the lane order into the
  // group-major lane table with use[n_base] (nullptr: every group) and reduces every row's
  // participation, min key and count on the device; sobol_finish runs the sum pass and returns
  // shift_host[rows], sums_host[rows][4 + 4 k] and n_part_host[rows].  No prepare(), no spinup, not
  // dirtied.
  void sobol_begin(const RowSource &rs, int k, int n_base, const unsigned char *use);
  void sobol_finish(double *shift_host, double *sums_host, long long *n_part_host);
  // ---- held and derived per-member series (hx_series_define in hector_amd.h) ----------------------
  void series_define(const std::string &name, const std::string &a, const hx_series_op &op);
  // hx_series_eval: a series from a whole postfix expression in one launch; ex.members point at THIS
  // core's n_members() doubles (the fleet hands every shard its slice)
  void series_eval(const std::string &name, const hx_expr &ex);
  void series_drop(const std::string &name);
  void series_list(std::vector<std::string> *names, std::vector<int> *valid_to) const;
  // ---- member ranks and the CRPS (hx_series_rank / hx_metric_ranks / hx_ensemble_crps) ------------
  // One shard only: the sort needs the whole row on this core.  q[n_] integer weights in member order
  // (nullptr: every member 1); kind: HX_RANK_*.  rows_check is the validation of capability and
  // dates or specifications alone.  No prepare(), no spinup, not dirtied.
  void series_rank(const std::string &name, const std::string &capability, int year0, int year1,
                   const unsigned long long *q, int kind);
  void metric_ranks(const std::string &capability, const hx_metric *specs, int nspecs,
                    const unsigned long long *q, int kind, double *out_host);
  void crps(const std::string &capability, const int *years, const double *obs, int nyears,
            const unsigned long long *q, double *crps_host, double *pit_host, long long *n_part_host);
  int device() const { return device_; }
  void status(unsigned *out_host);
  void state_row(int row, double *out_host);
  int spinup_steps(int member);

  double last_run_kernel_ms() const { return run_ms_; }
  // "output=0" in a component's section: the output stream leaves its rows out (core.cpp:257-262)
  bool component_output_enabled(const std::string &section) const { return scen_.scalar(section, "output", 1.0) > 0; }
  void set_pair_kernel_limit(int max_members) { pair_max_members_ = max_members < 0 ? 0 : max_members; }
  // Ensembles of at least min_members take the one-biome kernel built for two resident
  // wavefronts per SIMD (hx_run_kernel<HX_B1W2>): < 0 the default -- more wavefronts than the
  // device has SIMDs --, 0 never
  void set_two_wave_from(int min_members) { two_wave_from_ = min_members; }
  int wave_clock(long long *ticks, int cap);   // [wavefront][start, end] of the last launch, 100 MHz ticks
  // ticks a wavefront of the last launch spent in the statistics epilogue behind its year loop
  // (hx_wave_partials); -> wavefronts written, 0 if the launch wrote no partials
  int wave_epilogue_clock(long long *ticks, int cap);
  const char *last_run_kernel() const { return last_run_pair_ ? "pair" : last_run_w2_ ? "run2" : "run"; }
  // which instantiation family the last run() asked for (the CON template argument of
  // hx_run_kernel): 0 plain, -2 plain + diagnostics, -1 extended, 1 extended with the NBP
  // machinery, 2 carbon tracking
  int last_run_variant() const { return last_run_con_; }
  // 1: the last run took the solver's retries inside the step loop (the faithful path), 0: at the
  // head of the segment (HxConst::faithful_retries as that launch saw it)
  int last_run_retries() const { return last_run_faithful_; }
  double last_spinup_ms() const { return spin_ms_; }
  hipStream_t stream() const { return stream_; }

 private:
  struct ParamRef { int row; bool per_biome; const char *units; bool affects_spinup; };
  int resolve_param(const std::string &capability, const ParamRef **ref) const;
  int out_index(const std::string &capability) const;
  void build_shared();
  void alloc_device();
  void free_device();
  void upload_params();
  void prepare();  // upload + spinup when dirty
  HxBuffers buffers() const;
  void check(hipError_t e, const char *what) const;
  // A grow-only scratch buffer on the device, sized in elements of T.  reserve() frees and allocates
  // anew only when count exceeds the capacity: the old contents are gone then, nothing is waited for
  // and nothing rounded up.  No destructor: free_device() releases every one of them while the
  // device is still there.
  template <class T> class Scratch {
   public:
    T *get() const { return p_; }
    template <class U> U *as() const { return reinterpret_cast<U *>(p_); }   // a buffer of mixed parts
    size_t capacity() const { return cap_; }
    hipError_t grow(size_t count) {   // reserve() for the caller that words the failure itself
      if (count <= cap_) return hipSuccess;
      release();
      const hipError_t e = hipMalloc(&p_, sizeof(T) * count);
      if (e == hipSuccess) cap_ = count; else p_ = nullptr;
      return e;
    }
    T *reserve(size_t count, const EnsembleCore &core, const char *what) {
      core.check(grow(count), what);
      return p_;
    }
    void release() {
      if (p_) (void)hipFree(p_);
      p_ = nullptr; cap_ = 0;
    }
   private:
    T *p_ = nullptr;
    size_t cap_ = 0;
  };

  Scenario scen_;
  int n_, npad_, B_, device_;
  std::vector<std::string> biome_names_;
  std::vector<std::vector<double>> params_;  // [row][npad]
  std::vector<bool> row_uniform_;
  std::vector<int> member_of_lane_, lane_of_member_;  // lane <-> member (size npad / n)
  bool sort_members_ = true, calibrate_lanes_ = true;
  std::vector<double> lane_cost_;  // [n_] measured cost per member (empty: parameter key)
  double *d_cost_ = nullptr;
  long long *d_wave_clk_ = nullptr;   // HxBuffers::wave_clk
  // Per-wavefront partial statistics of CO2_concentration and global_tas (HxBuffers::wpart),
  // allocated with the outputs of a one-biome core.  wpart_on_ / wpart_skip_: what the kernel
  // arguments on the device say.  Rows wpart_lo_ .. wpart_hi_ of the output blocks were written
  // together with their partials and by nothing else since (hi < lo: none): a launch of another
  // kernel flavour cuts the range at its first row, a new layout or spinup empties it.
  double *d_wpart_ = nullptr;
  bool wpart_on_ = false, last_run_wpart_ = false;
  int wpart_skip_ = 0, wpart_row0_ = 0, wpart_row1_ = -1, wpart_lo_ = 0, wpart_hi_ = -1;
  int stats_partials_var(const double *block, int iy0, int iy1) const;   // 0 / 1, or -1: hx_stats_kernel
  int partials_skip_waves() const;
  double *d_bscratch_ = nullptr;  // [nbiome][npad] f_new_thaw of the seven- and eight-biome kernels
  int cost_from_iy_ = -1;         // d_cost_ covers the years cost_from_iy_+1..last_iy_ (-1: nothing)
  void maybe_calibrate_lanes();
  uint64_t cost_model_key(const std::vector<int> &varying) const;
  void fit_cost_model(const std::vector<double> &member_cost);
  bool predict_cost(const std::vector<int> &varying, std::vector<double> &out) const;
  int lane_order_source_ = 0;
  bool cost_model_ = true, cost_fitted_ = false;
  void assign_lanes();
  bool params_dirty_ = true, need_spinup_ = true, layout_dirty_ = true, ker_per_member_ = false;
  // What the device holds of the parameter table: the rows set since the last upload and the lane
  // order of that upload (upload_params() sends only what moved).
  std::vector<char> row_dirty_;
  bool rows_all_dirty_ = true, order_changed_ = true;
  std::vector<int> uploaded_order_;
  // The post-spinup snapshot on the device belongs to the current spinup inputs (a shared spinup
  // is then not repeated when only parameters it does not see were set: prepare()).
  bool spin_valid_ = false;
  int last_iy_ = 0;
  HxConst kc_{};
  std::vector<double> member_series_[HXM_N];  // host [ns][n_], member order; empty = shared
  // tas_constrain / RF_tot_constrain interpolate between the dates they were given at
  // (temperature_component.cpp:112, forcing_component.cpp:112): per-member POINTS, year -> [n_]
  // (NaN = none for that member), from which the dense member series is rebuilt
  std::map<int, std::vector<double>> member_points_[HXM_N];
  void densify_member_constraint(int k, const std::string &capability);
  double *d_mseries_[HXM_N] = {};
  bool mseries_dirty_ = false;
  void upload_member_series();
  // the one lookup of a dated input: a row of kDatedInputs (ensemble_core.cpp), or the scenario's
  // <gas>_emissions / <gas>_constrain
  DatedInput find_dated(const std::string &capability) const;
  // A variable's mix (setvar_dated_mix): the recipe, never the n_ x years table.  It overlays
  // member_series_[row] if that exists, else the scenario's shared series, in `years`.
  struct MemberMix {
    MixFamily family = MIX_NONE;       // the descriptor's
    int nbasis = 0;
    std::vector<int> years;            // [ny], as given
    std::vector<double> basis, coeff;  // [nbasis][ny], [nbasis][n_] in member order
    bool covers(int year) const;
    // year index (from `start`) -> column of the recipe, -1: not covered
    std::vector<int> cover_map(int start, int ns) const;
    // the definition's bits in year column i: every member (out[n_]), one member
    void year_values(size_t i, double *out) const;
    double member_value(size_t i, size_t member) const;
  };
  // Every mix of the core by capability, whatever its family.  Nothing that reaches the device or
  // a message iterates this map: the pre-passes fill their slots in their own order.
  std::map<std::string, MemberMix> mixes_;
  const MemberMix *mix_of(const std::string &capability) const;
  bool any_mix(MixFamily family) const;
  // the gas pre-pass runs: a gas parameter or an input of it differs between members
  bool gas_prepass() const { return !gas_member_.empty() || any_mix(MIX_GAS); }
  // throws "<fn>: <capability> has a mix that covers <year>: remove the mix first ..."
  void refuse_covered(const char *fn, const std::string &capability, const int *years, int n) const;
  // inputs changed from `year` on: the next run() goes back to year - 1 (R/messages.R:125-133)
  void reset_from(int year);
  Scratch<char> d_mix_;                // scratch of the mix kernel: lane map, rows, basis, coefficients
  void build_mix_table(const DatedInput &d, const MemberMix &mx, bool dense);
  // The recipe block of a pre-pass (hx_gas_mix_kernel, hx_slcf_mix_kernel): pack_recipes appends
  // to the caller's doubles the coefficient blocks of the slots that hold a mix and their bases
  // dense in years; upload_recipes puts the four parts into one fresh allocation.
  struct RecipePack {
    std::vector<long long> coff;       // [nblk] offset of a block's coefficients in the doubles
    std::vector<int> rec;              // [slots][2]: nbasis (0: no mix), block
    std::vector<int> ints;             // cover [nblk][ns] | member_of_lane [npad]
    size_t nblk = 0, o_basis = 0;      // basis [nblk][HX_MIX_MAX_BASIS][ns] at dbl[o_basis]
  };
  struct RecipeBlock { double *dbl; long long *coff; int *rec, *cover, *member_of_lane; };
  RecipePack pack_recipes(const std::vector<const MemberMix *> &slot, std::vector<double> &dbl) const;
  RecipeBlock upload_recipes(char **block, const std::vector<double> &dbl, const RecipePack &p,
                             const char *what);
  void upload_args();
  bool component_disabled(const std::string &section) const;  // "enabled=0" in the INI section
  void check_component_enabled(const std::string &capability) const;
  // N2O / halocarbon parameters that differ between members: capability -> [n_] (member order)
  std::map<std::string, std::vector<double>> gas_member_;
  double *d_gas_par_ = nullptr, *d_gas_ser_ = nullptr;
  // Mixes of the inputs the gas pre-pass reads (N2O_emissions, RF_albedo, <gas>_emissions) have no
  // HXM_* row of their own and never a table: the pre-pass evaluates them where it needs the value
  // (hx_gas_mix_kernel).
  char *d_gas_mix_ = nullptr;          // that kernel's recipe block (coefficients, basis, cover, lane map)
  // ... and those of the aerosol / precursor inputs (hx_enable_slcf_mixes) are evaluated by
  // hx_slcf_mix_kernel into the HXM_OH_B .. HXM_RF_AERO rows
  char *d_slcf_mix_ = nullptr;
  bool slcf_on_ = false, slcf_dirty_ = false;
  // Forcing efficacies that differ between members (hx_enable_member_forcing): capability -> [n_]
  // in member order.  The four rho_* go to hx_slcf_mix_kernel, which writes the HXM_RF_AERO row
  // with them; the three delta_* are the HXM_EFFICACY rows the extended run kernels read.
  std::map<std::string, std::vector<double>> forcing_member_;
  bool forcing_on_ = false, eff_dirty_ = false;
  bool rho_member() const;     // one of rho_bc, rho_oc, rho_so2, rho_nh3 differs between members
  bool delta_member() const;   // ... of delta_co2, delta_ch4, delta_n2o, and the run uses them
  bool slcf_prepass() const { return any_mix(MIX_SLCF) || rho_member(); }
  void upload_efficacies();
  void run_slcf_kernel();
  void run_gas_kernel();  // fills the per-member N2O and halocarbon-forcing series
  bool gas_dirty_ = false;
  int member_con_mask_ = 0;  // HXC_* bits that only per-member constraint series contribute
  void init_from_scenario();
  std::vector<std::string> halo_names_;
  std::vector<std::vector<double>> halo_conc_;  // [gas][ns] halocarbon concentrations, pptv
  std::vector<double> shared_, ker_;
  bool out_enabled_[HXO_NVAR];
  // device
  double *d_params_ = nullptr, *d_state_ = nullptr, *d_shared_ = nullptr, *d_ker_ = nullptr;
  double *d_out_[HXO_NVAR];
  unsigned *d_status_ = nullptr;
  int *d_spin_steps_ = nullptr;
  HxArgs *d_args_ = nullptr;
  double *d_uparams_ = nullptr;
  int tracking_year_ = 0;  // 0 = off
  double *d_track_out_f_ = nullptr, *d_track_out_v_ = nullptr;
  // SimpleNbox::run starts tracking when runToDate == trackingDate (simpleNbox-runtime.cpp:215-220):
  // a date at or before startDate, or past endDate, never engages
  int trk_iy() const {
    return (tracking_year_ > scen_.start && tracking_year_ <= scen_.end) ? tracking_year_ - scen_.start : -1;
  }
  double *d_derived_ = nullptr, *d_dpart_ = nullptr, *d_hist_ = nullptr;
  unsigned *d_hist_status_ = nullptr;  // [ns][npad] status bits of every year (with d_hist_)
  void remap_biome_outputs(const std::vector<int> &old_of_new);
  bool history_ = false, shared_dirty_ = false;
  bool spin_record_ = false, spin_uniform_ = false;
  double *d_spin_rec_ = nullptr;
  int hist_valid_to_ = 0;   // history slabs 1..hist_valid_to_ are valid
  int dirty_from_iy_ = -1;  // pending auto-reset target (R wrapper's reset_date)
  int *d_lane_of_member_ = nullptr;
  Scratch<double> d_gather_, d_diag_;   // fetchvars: [ny][n_] in member order, [ny][npad_] of a derived diagnostic
  double *d_slr_ = nullptr;
  int slr_valid_to_ = -1;
  void check_parameters() const;
  bool fetch_host(const std::string &capability, int year0, int year1, double *out_host);
  void compute_derived(const std::string &capability, int iy0, int ny, double *dst);
  // ---- the scratch of the verbs (ensemble_post.cpp).  The three that hold doubles with a list of
  // ints behind them are sized in bytes.
  // member_score: [obs n][sigma n][chi2 npad][chi2 in member order n_] doubles + years; shared with the
  // metric, pair-metric and rank verbs, which bring their block to member order through it
  Scratch<unsigned char> d_score_;
  // member_score_whitened: [W in fragment order np^2][obs np][base npad][chi2 npad][chi2 in member order
  // n_] doubles + rows np
  Scratch<unsigned char> d_whiten_;
  // member_project: [basis in fragment order][center][base npad][out m x npad][out in member order
  // m x n_] doubles + rows
  Scratch<unsigned char> d_project_;
  unsigned long long *d_q_ = nullptr;         // integer weights in lane order [npad]
  Scratch<unsigned long long> d_qstate_;      // per year {HxQYear, lo}, per (year, prob) {prefix, rem}, probs
  Scratch<unsigned long long> d_qhist_;       // [ny][nprobs][256]
  // The block the select's first step (q_begin, or quantiles itself) prepared for its histogram
  // passes: d_out_[v], a series, a derived block or d_met_.  It is not owned, and between q_begin and
  // q_pass it may point into the metric block: a metric or pair-metric call that regrows d_met_ in
  // between leaves it dangling, as it always has (the fleet drives q_begin and q_pass back to back).
  // free_device() resets it.
  const double *q_src_ = nullptr;
  int q_iy0_ = 0, q_ny_ = 0, q_np_ = 0;
  bool q_weighted_ = false;
  int post_flags_ = 0;                        // HECTOR_AMD_POST_AB (measurements): 1 no prefix skip, 2 with wave aggregation
  const double *q_check(const std::string &capability, int year0, int year1, int nprobs,
                        const char *fn);      // -> the source block
  // rows_check, then sync(), then the metric or pair kernel queued on stream_ -> the rows iy0 ..
  // iy0 + nrows - 1 of a [rows][npad_] block in lane order
  struct Rows { const double *block; int iy0, nrows; };
  Rows rows(const RowSource &rs, const Groups &g, int nprobs);
  // q[n_] in member order -> d_q_ in lane order (padding lanes 0), which it returns; nullptr stays
  const unsigned long long *lane_weights(const unsigned long long *q);
  int *group_labels();                        // d_glab_ allocated, its lane part set to -1 on stream_
  void upload_labels(const int *labels);      // member order -> d_glab_ in lane order
  // {~min key, max key, sum q, count} of every row of r, per group if ngroups, into st (zeroed here)
  void minmax(const Rows &r, int ngroups, const unsigned long long *dq, unsigned long long *st);
  // the select's scratch, q and the rows' records for rs; q_src_ and its companions set -> rows
  int q_start(const RowSource &rs, const Groups &g, const unsigned long long *q, int np);
  void q_hist(const int *lo, const unsigned long long *prefix);   // one histogram pass over q_src_
  // scratch of the metric kernel: group records + row lists, and the block [nspecs][npad_] (lane order)
  Scratch<unsigned char> d_metplan_;
  Scratch<double> d_met_;
  Scratch<unsigned long long> d_bin_;         // [32 edges as doubles][rows][nedges + 2]
  Scratch<unsigned long long> d_mom_;         // scratch of the moment verbs (MomBuf in ensemble_post.cpp)
  const double *mom_src_ = nullptr;           // the block mom_begin prepared for mom_finish
  int mom_iy0_ = 0, mom_ny_ = 0, mom_npred_ = 0;
  // the grouped summaries: labels [npad_] in lane order, then [n_] in member order as uploaded
  int *d_glab_ = nullptr;
  int q_groups_ = 0, mom_groups_ = 0;         // 0: q_pass / the moment scratch belong to an ungrouped call
  Scratch<unsigned long long> d_comom_;       // scratch of hx_ensemble_comoments (CoBuf in ensemble_post.cpp)
  const double *co_a_ = nullptr, *co_b_ = nullptr;   // the windows comom_begin prepared for comom_finish
  int co_ia0_ = 0, co_ib0_ = 0, co_na_ = 0, co_nb_ = 0;
  bool co_sym_ = false;
  Scratch<unsigned long long> d_sobol_;       // scratch of the Sobol verbs (SobBuf in ensemble_post.cpp)
  const double *sob_src_ = nullptr;           // the block sobol_begin prepared for sobol_finish
  int sob_iy0_ = 0, sob_ny_ = 0, sob_k_ = 0, sob_nb_ = 0;
  int metric_check(const std::string &capability, const hx_metric *specs, int nspecs, const char *fn,
                   const double **src);
  const double *metric_block(const double *src, const hx_metric *specs, int nspecs);   // -> d_met_, queued on stream_
  // both operands of a pair call resolved and its specifications checked against the range where both
  // are valid (fn is named in every message); *src_b stays nullptr for a vector b
  void pair_metric_check(const std::string &cap_a, const PairCall &pc, const char *fn, const double **src_a,
                         const double **src_b);
  // the pair kernel queued on stream_ -> d_met_ [nspecs][npad_] in lane order, laid out like metric_block's
  const double *pair_metric_block(const double *src_a, const double *src_b, const PairCall &pc);
  // ---- "a per-member variable on the device": the one resolver of the verbs -----------------------
  // block: [ns][npad_] in the CURRENT lane order, rows 0..last_iy hold values; v: the index of a
  // recorded output (its block may still be null: the callers keep their own messages for that), -1
  // for a derived diagnostic, a whole-surface combination or a series
  struct PostSource { const double *block; int last_iy; int v; };
  // fn: the ABI function on whose behalf it is resolved (named in the messages of the new cases).
  // Derived diagnostics and combinations are computed on stream_ into a block kept in derived_cache_.
  PostSource post_source(const std::string &capability, const char *fn);
  // ensemble_core.cpp's tables by name, for the resolver: a derived diagnostic (-1: none, 0: computed
  // into a block by hx_diag_kernel, 1 + i: block i of the slr family in d_slr_), a recorded output
  static int derived_kind(const std::string &name);
  static bool recorded_name(const std::string &name);
  // every check of the whitened score and of the projection -> the variable; both hold years[n] and the
  // reference period to the variable's range through listed_source (f: the ABI function named)
  PostSource listed_source(const std::string &f, const std::string &capability, const int *years, int n,
                           int base_year0, int base_year1);
  PostSource whitened_check(const std::string &capability, const int *years, const double *obs,
                            const double *whiten, int n, int base_year0, int base_year1, const double *out_host);
  PostSource project_check(const std::string &capability, const int *years, const double *center,
                           const double *basis, int n, int m, int base_year0, int base_year1,
                           const double *out_host);
  struct Series {
    std::string name;
    double *block = nullptr;             // [ns][npad_], lane order `lane_of_member`
    int valid_iy = 0;
    std::vector<int> lane_of_member;     // the lane order the block is stored in
  };
  std::vector<Series> series_;
  int find_series(const std::string &name) const;
  // the rules of hx_series_define for a new or replaced name, fn named in the messages -> the index of
  // the series it replaces, -1 for a new one
  int series_name_check(const std::string &fn, const std::string &name);
  // scratch of the rank verbs (RankBuf in ensemble_post.cpp) and the sort of `nrows` rows of a block in
  // lane order: rows == nullptr the rows row0.., else rows[i]; mode HX_RANK_* writes dst rows
  // dst_row0.., mode 2 (the CRPS against obs[i]) fills the records it returns (4 words a row:
  // crps, pit, n_part, 0).  Queued on stream_ and waited for.
  Scratch<unsigned long long> d_rank_;
  std::vector<unsigned long long> rank_rows(const char *fn, const double *src, int row0, const int *rows,
                                            int nrows, const unsigned long long *q, int mode, const double *obs,
                                            double *dst, int dst_row0);
  void series_to_current_lanes(Series &s);   // permutes the block on the device if the lanes have moved
  void free_series();
  // the kept blocks of derived diagnostics / combinations: valid while out_epoch_ stands
  struct DerivedBlock { std::string name; double *block = nullptr; unsigned long long epoch = 0, used = 0; };
  DerivedBlock derived_cache_[2];
  unsigned long long out_epoch_ = 1, derived_clock_ = 0;   // out_epoch_: bumped whenever recorded rows may change
  double *d_ps_tmp_ = nullptr;               // [ns][npad_]: the high-latitude part of a combination
  double *d_ser_vec_ = nullptr;              // [ns] a per-year operand + [npad_] ANOMALY's bases
  int *d_ser_perm_ = nullptr;                // [npad_] source lanes of a permutation
  double *d_expr_ = nullptr;                 // hx_series_eval: HxExprProg, member vectors [npad_], year vectors [ns]
  size_t d_expr_words_ = 0;
  void free_derived_cache();
  const double *derived_block(const std::string &capability);
  hipStream_t stream_ = nullptr;
  hipStream_t aux_stream_ = nullptr;          // the prewarm loop's (non-blocking)
  unsigned char *d_prewarm_ = nullptr;        // its stop flag (+ a sink)
  int prewarm_ms_ = 50;
  bool prewarm_on_ = false, last_run_prewarmed_ = false;
  double last_gpu_activity_s_ = -1.0;         // host clock of the last launch / wait of this core
  void prewarm_begin();
  void prewarm_end();
  hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
  bool run_timed_ = false;
  int pair_max_members_ = 32768;  // ensembles up to this size use the two-wavefront kernel (0: never)
  bool last_run_pair_ = false;
  int two_wave_from_ = -1;        // see set_two_wave_from()
  bool pair_costly_with_cheap_ = true;   // lane order by measured cost: see assign_lanes()
  int key_order_mode_ = 0;               // HECTOR_AMD_KEY_ORDER (experiments, see assign_lanes)
  bool last_run_w2_ = false;
  int last_run_con_ = 0;
  int last_run_faithful_ = 1;
  bool two_wave_expected() const;   // run() will take hx_run_kernel<HX_B1W2> (see assign_lanes)
  int simds_ = 1024;              // SIMDs of this core's device (4 per compute unit)
  mutable double run_ms_ = 0, spin_ms_ = 0;
};

}  // namespace hx
