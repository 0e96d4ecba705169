/*
 * hector_amd.h -- C ABI of libhector_amd.so: an MI355X-native ensemble
 * integrator for Hector's coupled carbon-cycle / climate year loop.
 *
 * Each entry point names the reference interface it replaces (file:line in
 * JGCRI/hector v3.5.0).  The reference drives ONE member through
 *   Core::mkcore/getcore/delcore   inst/include/core.hpp:105-109, src/core.cpp:813-857
 *   Core::init + INIToCoreReader   src/rcpp_hector.cpp:31-86 (newcore_impl)
 *   Core::sendMessage(SETDATA/GETDATA, capability, message_data)
 *                                  src/core.cpp:716-778, src/rcpp_hector.cpp:282-356
 *   Core::run / Core::reset / Core::shutDown
 *                                  src/core.cpp:448-549, src/rcpp_hector.cpp:88-181
 * This library keeps those verbs and the capability strings of
 * inst/include/component_data.hpp, and adds a member axis: every parameter is a
 * vector over members and every result is [year][member].
 *
 * Conventions: plain C types only; every function returns 0 on success and a
 * non-zero code on failure, with the message available from hx_last_error()
 * (the reference throws h_exception; nothing is thrown across this ABI).
 * Per-member MODEL errors (mass balance, >8 solver retries, negative pool...)
 * do not fail a call: they set bits in the member's status word (hx_status).
 * A core is bound to one GPU (hx_newcore) or to a list of GPUs (hx_newcore_devices: contiguous
 * member blocks, one per GPU, no exchange during integration); there is no CPU execution
 * path -- hx_newcore fails if no HIP device is present.  Not thread-safe per handle (like Core).
 */
#ifndef HECTOR_AMD_H
#define HECTOR_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hx_core hx_core; /* opaque; replaces the int index of Core::mkcore */

/* "hip" for the product library.  (A test-only host-emulation build reports
 * "host-emulation"; the Python loader refuses it outside tests.) */
const char *hx_backend(void);
/* "built with HIP x.y.z (<compiler>), gfx950; runtime <hipRuntimeGetVersion>, driver
 * <hipDriverGetVersion>": the toolchain pairing behind a run's figures.  hx_backend()'s first call
 * warns on stderr when the runtime's major version is not the build's. */
const char *hx_build_info(void);
const char *hx_last_error(void);

/* newcore(inifile, ...)  R/hector.R:81-87, src/rcpp_hector.cpp:31-86.
 * `scenario` is a Hector INI file (csv: tables resolved like the reference) or
 * a dense scenario pack (.hxs).  Creates an n_members ensemble on GPU `device`,
 * all members at the INI's parameter values; one biome "global", or the biomes the INI
 * defines with "<biome>.<variable>" keys (at most 32; carbon tracking: 24). */
int hx_newcore(const char *scenario, int n_members, int device, hx_core **out);

/* The same ensemble over SEVERAL GPUs of the node.  The reference keeps many
 * independent cores in one process through its registry (Core::mkcore / getcore / delcore,
 * inst/include/core.hpp:105-109, src/core.cpp:813-857) and the host loops over them; here the
 * handle is that registry: shard s is an n_members / n_devices block of consecutive members on
 * devices[s] (the remainder goes to the first shards), every call of this header is routed to the
 * shards -- per-member arguments sliced, results returned in member order -- and hx_run queues
 * the kernels of every GPU before it returns.  Nothing is exchanged while the model runs; the one
 * collective is hx_ensemble_stats.  Each device may appear once (RCCL needs one rank per GPU;
 * HECTOR_AMD_FLEET_REHEARSAL=1 admits duplicates on a smaller box and exchanges the statistics
 * with device copies instead). */
int hx_newcore_devices(const char *scenario, int n_members, const int *devices, int n_devices,
                       hx_core **out);
/* devices[n_shards], offsets[n_shards + 1] (offsets[s] = first member of shard s); NULL = skip */
int hx_shards(hx_core *core, int *n_shards, int *devices, int *offsets);

/* Per-year ensemble statistics {count, sum, sum of squares, min, max} of nvars recorded outputs
 * over EVERY member on every GPU (and every process that joined the communicator):
 * [nvars][year1 - year0 + 1][5] doubles into host memory out_host and / or device memory d_out
 * (on the first shard's GPU); either may be NULL.  Every GPU reduces its own members
 * (wavefront shuffles), ONE ncclAllGather over RCCL / xGMI hands every rank all blocks (44 KB per
 * rank and variable), and every rank folds them in rank order -- the result is bit-identical on
 * all ranks.  The north star's "RCCL gather of Tgav / CO2 stats"; the reference has no
 * counterpart (its hosts aggregate fetchvars() data frames in R).  A one-GPU core that joined
 * no communicator does no collective.  Returns when the result is in place. */
int hx_ensemble_stats(hx_core *core, int nvars, const char *const *capabilities, int year0,
                      int year1, double *out_host, double *d_out);
/* One process per GPU (MPI / torchrun style hosts): ONE process calls hx_comm_unique_id and
 * hands the 128 bytes to the others by its own means; every process then joins with its
 * process rank.  The communicator has n_procs * n_shards ranks, this core's shards are ranks
 * proc_rank * n_shards + s, and hx_ensemble_stats reduces over all of them.  A core made by
 * hx_newcore_devices that never calls this gets a communicator of its own shards at the first
 * hx_ensemble_stats.  RCCL is loaded when first needed (librccl.so.1 -- the copy already in the
 * process if there is one; HECTOR_AMD_RCCL overrides the path). */
int hx_comm_unique_id(char *id128);
int hx_comm_init_rank(hx_core *core, int n_procs, int proc_rank, const char *id128);
/* world: ranks of the communicator (0 = none yet); backend: "rccl <version> via <library>" */
int hx_comm_info(hx_core *core, int *world, int *first_rank, const char **backend);

/* shutdown(core)  src/rcpp_hector.cpp:88-101 (Core::shutDown + delcore) */
int hx_shutdown(hx_core *core);

/* setvar(core, NA, var, values, unit)  R/messages.R:107-140 ->
 * sendmessage(SETDATA)  src/rcpp_hector.cpp:282-356 -> Core::setData.
 * capability: component_data.hpp string, optionally "<biome>.<capability>".
 * nvalues is 1 (every member) or n_members.  units: NULL/"" = unchecked, else it
 * must match the reference's unit string (e.g. "degC" for S).  Like the R
 * wrapper this invalidates results from date 0 (the next run respins if needed).
 * Parameters of the member-independent components (delta_co2, rho_bc, M0, Tsoil, Tstrat ...)
 * take one value for the whole core -- except those of the N2O and halocarbon components
 * (N0, TN2O0, UC_N2O: src/n2o_component.cpp:95-130; tau_<gas> = the INI key "tau" of
 * [<gas>_halocarbon], rho_<gas>, delta_<gas>: src/halocarbon_component.cpp:118-150), which the
 * reference perturbs per run: with one value per member their recurrences run per member on
 * the device ahead of the year loop (16 B per member-year of HBM) -- and, after
 * hx_enable_member_forcing (below), the forcing efficacies delta_co2, delta_ch4, delta_n2o, rho_bc,
 * rho_oc, rho_so2, rho_nh3 (src/forcing_component.cpp).  M0, Tsoil, Tstrat, TOH0 and PO3 stay
 * core-wide: they sit inside the CH4 / OH recurrence and in the CH4 initial state. */
int hx_setvar(hx_core *core, const char *capability, const double *values, int nvalues,
              const char *units);
/* setvar(core, dates, var, values, unit) for a scenario INPUT series (emissions, SV,
 * RF_albedo, RF_misc ...) or a constraint (CO2_constrain, NBP_constrain, tas_constrain,
 * RF_tot_constrain, CH4_constrain, N2O_constrain, <gas>_constrain; NaN removes a date);
 * R/messages.R:107-140 with dates: the same new values for every member.  Marks the core dirty from min(year)-1: the next hx_run first resets there (if the
 * state history is enabled, else to startDate), like run() does for a core that is not clean
 * (src/rcpp_hector.cpp:160-166). */
int hx_setvar_dated(hx_core *core, const char *capability, const int *years, const double *values,
                    int n, const char *units);
/* The same with a different value for every member -- the reference's "re-run a period with new
 * emissions per run" pattern (vignettes/ex_hector_apply.Rmd; one reset/setvar/run per run
 * there), for all members in one run: values[i * n_members + member] is the value of
 * years[i].  ffi_emissions, luc_emissions, daccs_uptake, luc_uptake, CH4_emissions, and the
 * constraints CO2_constrain, NBP_constrain, tas_constrain, RF_tot_constrain, CH4_constrain
 * (NaN = no constraint for that member and year; a CH4 constraint at startDate is core-wide)
 * -- 8 B per member-year of HBM each, once used. */
int hx_setvar_dated_members(hx_core *core, const char *capability, const int *years,
                            const double *values, int nyears, const char *units);
/* A different series for every member given as what it usually is: a MIX of a few shared
 * year-vectors -- a scenario scaled per member, a blend of two scenarios with a per-member weight,
 * a common pulse of per-member size.  basis[k * nyears + i] is vector k in years[i],
 * coeff[k * n_members + member] the member's weight of it, nbasis <= HX_MIX_MAX_BASIS.
 * DEFINITION.  In every years[i] the variable of member m is
 *     s = coeff[0][m] * basis[0][i];   for k = 1 .. nbasis-1:  s = s + (coeff[k][m] * basis[k][i])
 * each product rounded before it is added, in ascending k, in IEEE double without fused
 * multiply-add: numpy reproduces it bit for bit under any lane order, kernel flavour or shard
 * layout, and hx_fetchvars returns these bits ([year][member], member order; the other years hold
 * the underlying value).  A variable has at most one mix.  It OVERLAYS, in the years it lists, the
 * series beneath it: the per-member table of hx_setvar_dated_members if there is one, else the
 * scenario's shared series.  A second call replaces the whole mix (years only the old one listed
 * go back to the series beneath); nbasis = 0 removes it (years, basis, coeff are not read), and a
 * variable without a per-member table is shared again.  While a mix exists, hx_setvar_dated and
 * hx_setvar_dated_members of that variable are refused in a year it covers (remove the mix
 * first); in the other years they work as without one.  Marks the core dirty from min(year)-1
 * over the years of the new and of the replaced mix, like hx_setvar_dated_members.
 * COST.  The host keeps the recipe, nbasis x (n_members + nyears) doubles, never a table of
 * n_members x n_years.  The next hx_run uploads it and expands it on the device into the 8 B per
 * member-year table the run kernels read (one store-bound kernel); new coefficients for the same
 * years cost nbasis x n_members doubles of upload and that kernel again.
 * NAMES.  ffi_emissions, daccs_uptake, luc_emissions, luc_uptake, CH4_emissions -- the run kernels
 * read their table -- and the inputs of the N2O and halocarbon components and the albedo forcing:
 * N2O_emissions ("Tg N"), RF_albedo ("W/m2") and <gas>_emissions ("Gg") of every halocarbon the
 * scenario holds (hx_mix_capabilities lists them for a core).  These three kinds never have a table
 * of emissions, on the host or on the device: hx_setvar_dated_members keeps refusing them, so their
 * mix overlays the scenario's shared series, and a lane-per-member pre-pass ahead of the year loop
 * evaluates the definition where the N2O and halocarbon recurrences read the value and writes the
 * two rows the run kernels take (N2O; halocarbon + albedo + misc forcing: 16 B per member-year, as
 * for per-member N0 or tau_<gas>).  N2O_concentration, RF_N2O, <gas>_concentration, RF_<gas> and
 * RF_albedo are then per member.  The aerosol emissions (SO2, BC, OC, NH3) and the ozone / OH
 * precursors (NOX, CO, NMVOC) can be mixed after hx_enable_slcf_mixes (below); SV, RF_misc, CH4N
 * and N2O_natural_emissions cannot.
 * ERRORS (every message names the function; a refused call changes nothing): a capability other
 * than ffi_emissions, daccs_uptake, luc_emissions, luc_uptake, CH4_emissions and the names above (the
 * constraint series, with NaN = none and interpolated points, are no linear mix); units that do not match
 * (rule of hx_setvar_dated_members); nbasis outside 0..HX_MIX_MAX_BASIS; nyears < 1; a year
 * outside startDate..endDate or listed twice; a basis value or coefficient that is not finite;
 * NULL years, basis or coeff with nbasis > 0. */
#define HX_MIX_MAX_BASIS 8
int hx_setvar_dated_mix(hx_core *core, const char *capability, const int *years, int nyears,
                        const double *basis, int nbasis, const double *coeff, const char *units);
/* The names hx_setvar_dated_mix accepts for THIS core: the list holds the scenario's halocarbons.
 * The strings live until the next call on this thread. */
int hx_mix_capabilities(hx_core *core, const char *const **names, int *count);
/* Whole scenarios as members of one core: scenarios[nscen] are scenario files (pack or INI),
 * coeff[k * n_members + member] the member's weight of scenario k, 1 <= nscen <= HX_MIX_MAX_BASIS.
 * The library reads each file with its own scenario reader, finds every dated input series in which
 * one of them differs from the core's (bit for bit), and sets for each ONE mix over
 * startDate..endDate whose basis is the scenarios' series and whose coefficients are coeff
 * (*nseries, may be NULL: how many).  With one-hot coefficients a member's inputs are its scenario's
 * own bits: 1.0 * x + (0.0 * y) + ... is exact for finite values.  Cost: that of the mixes.
 * ERRORS (the message names the function and the section and key at fault; a refused call changes
 * nothing): nscen outside 1..HX_MIX_MAX_BASIS; startDate or endDate that differ; a different list of
 * halocarbons; ANY scalar that differs or is missing on one side (core.run_name, a label, excepted):
 * the members share one parameter table and one spinup; a series that differs and cannot be a mix
 * -- a constraint, SV, RF_misc, CH4N, N2O_natural_emissions, and, unless hx_enable_slcf_mixes is on,
 * the aerosol and ozone / OH precursor emissions, so that the shipped SSPs, which differ in
 * so2.SO2_emissions among others, are then refused against each other -- or that is missing on one
 * side; a coefficient that is not finite. */
int hx_setvar_scenario_mix(hx_core *core, const char *const *scenarios, int nscen, const double *coeff,
                           int *nseries);
/* The short-lived climate forcer inputs as mixes: with on != 0, hx_setvar_dated_mix,
 * hx_mix_capabilities (after the halocarbons) and hx_setvar_scenario_mix also take SO2_emissions
 * ("Gg S"), BC_emissions, OC_emissions, NH3_emissions ("Tg"), NOX_emissions ("Tg N"), CO_emissions
 * ("Tg CO") and NMVOC_emissions ("Tg NMVOC") -- with the always-mixable names everything the shipped
 * SSPs differ in, so hx_setvar_scenario_mix puts them into ONE core.  A precursor name stands for the
 * series of both the OH and the ozone section, as in hx_setvar_dated; a scenario file whose two
 * series differ is refused, naming both.  Like the gas inputs these never have a table of emissions:
 * the host keeps the recipe, and a lane-per-member pre-pass (hx_slcf_mix_kernel) writes the finished
 * terms the year loop adds -- six rows for the precursors (the three OH-lifetime terms, relative to
 * the MEMBER's own emissions at startDate when the mix covers it, and the three ozone terms), one
 * for the aerosols (BC + OC + SO2 + NH3 + aerosol-cloud term for aero_scalar = 1) -- 8 B per
 * member-year and row, each group only while one of its inputs is a mix.  hx_fetchvars returns the
 * seven inputs with the definition's bits and RF_BC, RF_OC, RF_SO2, RF_NH3, RF_aci per member.  A new
 * coefficient marks the core dirty from the earliest year of the mix; for a precursor mix that covers
 * startDate from startDate.  Off by default: every message and list is then what it was before this
 * switch existed, and it costs nothing until such a mix is set.  on == 0 while such a mix exists is
 * refused, naming it (remove the mix first).  hx_setvar_dated_members keeps refusing the names. */
int hx_enable_slcf_mixes(hx_core *core, int on);
/* The forcing efficacies per member: with on != 0, hx_setvar of delta_co2, delta_ch4, delta_n2o
 * ("(unitless)"), rho_bc, rho_oc, rho_nh3 ("W/m2/Tg") and rho_so2 ("W/m2/Gg") accepts n_members
 * values (units checked as before) and hx_getvar returns them -- a forcing-uncertainty ensemble in
 * which CO2, CH4 and N2O forcing scale independently and every aerosol species has its own efficacy,
 * in one launch.  One value, or n_members equal values, puts the name back on the shared path (the
 * rule of N0, tau_<gas> ...); a core of several shards splits the vectors like every other
 * per-member parameter.  Invalidation is what hx_setvar of these names always did.
 * rho_*: the lane-per-member pre-pass that serves the aerosol mixes (hx_slcf_mix_kernel) writes
 * the finished aerosol row with the member's own efficacies -- (((rho_bc*BC + rho_oc*OC) +
 * rho_so2*SO2) + rho_nh3*NH3) + aerosol-cloud term, unfused, as the host writes the shared column
 * -- and the extended run kernels take it; hx_enable_slcf_mixes is not needed.  8 B per member-year
 * for the row, whatever the number of per-member rho_*, only while one differs or an aerosol input
 * is a mix.  hx_fetchvars of RF_BC, RF_OC, RF_SO2, RF_NH3 answers per member.
 * delta_*: three values per lane, 24 B per member, uploaded with the parameters; the extended run
 * kernels read them where the core-wide ones are used -- (sarf*delta)+sarf for CO2, (delta*sarf)+sarf
 * for CH4 and N2O -- and the derived RF_CH4 / RF_N2O follow.  The reference's range check (-1..1,
 * ForcingComponent::prepareToRun) holds for every member: hx_run fails naming the first member at
 * fault.  With [CH4] or [N2O] disabled the forcing component leaves the three gases out: the
 * members' values are kept and returned, the run uses the shared -1 for every member.
 * A core that holds such values runs the extended instantiations of the run kernels (one- and
 * two-wave, 2-4 and looped biomes, carbon tracking) or, where the small-ensemble pair kernel would
 * serve it, that kernel's instantiation with the constraint code; the plain instantiations are
 * unchanged.  Off by default: every message and list is then what it was before this switch existed.  on == 0 while one of the seven differs between members is
 * refused, naming it; a refused call changes nothing.
 * Out of scope: M0, Tsoil, Tstrat, TOH0, PO3 (see hx_setvar). */
int hx_enable_member_forcing(hx_core *core, int on);
/* Keep every year's component state in HBM so hx_reset can return to any computed date --
 * what the reference's per-component tseries records provide (src/simpleNbox.cpp:708-840,
 * src/ocean_component.cpp:767-846).  272 B per member-year (one biome); default off. */
int hx_enable_history(hx_core *core, int on);

/* The spinup as the reference's output stream sees it: CSVOutputStreamVisitor is visited after
 * every spinup step with spinup = 1 (src/core.cpp:402-408, src/csv_outputstream_visitor.cpp:86-95,
 * the year column holds the step number).  hx_enable_spinup_record(core, 1) before the first run
 * keeps the carbon-cycle variables of those rows -- the ones that move during the spinup: NBP, NPP,
 * RH, rh_det, rh_soil, atmos_co2, atmos_c_residual, the land pools, earth_c, the ocean boxes'
 * carbon and the air-sea / HL->DO fluxes -- at max_spinup x 21 x 8 B of HBM per member.
 * hx_spinup_record: *names / *nvars = the capability names (values == NULL: only that);
 * values[(step-1) * nvars + v] for steps 1 .. *steps of `member`.  hector-amd writes them as the
 * spinup = 1 rows of outputstream_<run_name>.csv. */
int hx_enable_spinup_record(hx_core *core, int on);
int hx_spinup_record(hx_core *core, int member, const char *const **names, int *nvars, double *values,
                     int max_steps, int *steps);
/* fetchvars(core, NA, var) for parameters: GETDATA without a date. out[n_members] */
int hx_getvar(hx_core *core, const char *capability, double *out);

/* split_biome(core, "global", names, fveg_c, ...)  R/biome.R:61-130.
 * names: n_biomes C strings.  Fraction arrays may be NULL (equal split / same as fveg). */
int hx_split_biome(hx_core *core, int n_biomes, const char *const *names, const double *fveg,
                   const double *fdet, const double *fsoil, const double *fpf,
                   const double *fnpp);

/* split_biome(core, old_biome, new_biomes, ...) for a core that already has several biomes:
 * the new biomes are appended to the biome list, old_biome is deleted (R/biome.R:61-130). */
int hx_split_biome_of(hx_core *core, const char *old_biome, int n_biomes,
                      const char *const *names, const double *fveg, const double *fdet,
                      const double *fsoil, const double *fpf, const double *fnpp);

/* create_biome_impl / delete_biome_impl / rename_biome  (src/rcpp_hector.cpp:359-400;
 * SimpleNbox::createBiome / deleteBiome / renameBiome, src/simpleNbox.cpp:864-1060).  A created
 * biome has empty pools and npp_flux0 = 0 and the other parameters of the most recent biome
 * (set them with hx_setvar("<biome>.veg_c", ...), like R's create_biome does); at most 32 biomes
 * (1-8 run fully unrolled kernels, 9-32 kernels that loop over the biomes).
 * All three invalidate the run (spinup again), like any parameter change. */
int hx_create_biome(hx_core *core, const char *biome);
int hx_delete_biome(hx_core *core, const char *biome);
int hx_rename_biome(hx_core *core, const char *oldname, const char *newname);

/* get_biome_list(core)  R/biome.R:8-16: "global", the names given to hx_split_biome, or the
 * biomes an INI file defines with "<biome>.<variable>" keys in [simpleNbox]
 * (src/simpleNbox.cpp:190-330).  Per-biome parameters are "<biome>.beta" ..., per-biome pools
 * "<biome>.veg_c", ".detritus_c", ".soil_c", ".permafrost_c", ".thawedp_c" are outputs. */
int hx_biomes(hx_core *core, const char *const **names, int *count);

/* Select which per-year outputs are recorded (capability strings such as
 * "CO2_concentration", "global_tas", "RF_tot"...).  sst and land_tas are always
 * recorded.  The reference records everything always (tseries in every
 * component); here it is opt-in because each variable costs 8 B/member-year. */
int hx_set_outputs(hx_core *core, int nvars, const char *const *capabilities);
int hx_output_capabilities(const char *const **names, int *count);
/* Names of the scenario's halocarbon components ("CF4", "HFC23" ...; one
 * HalocarbonComponent each in the reference, src/core.cpp:120-175): "<name>_concentration",
 * "<name>_emissions", "RF_<name>" and "<name>_constrain" are fetchvars / setvar capabilities. */
int hx_halocarbons(hx_core *core, const char *const **names, int *count);

/* Internal lane assignment: by default members are mapped to GPU lanes sorted by their
 * perturbed parameters (wavefronts then follow similar solver schedules); every result is
 * returned in the caller's member order either way and does not depend on this switch.
 * hx_device_var exposes the raw lane-ordered arrays; hx_lane_of_member maps them. */
int hx_set_member_sorting(hx_core *core, int on);
/* The order is refined by MEASURED cost: the run kernel adds up every member's dopri5 steps and
 * stashes, and the first hx_reset(startDate) after a run that covered startDate..endDate reorders
 * the lanes by it -- wavefronts of members that really walk the same schedule, the costliest
 * dispatched first, so that an ensemble of more wavefronts than SIMDs does not end on its most
 * expensive ones; where two wavefronts share a SIMD (hx_set_two_wave_from) the second batch in
 * ascending cost, so that the costliest shares with the cheapest -- and spins up again (once; a parameter change falls back to the parameter
 * key until the next complete run).  Only ensembles of more wavefronts than the GPU has SIMDs
 * (65 536 members on an MI355X) are reordered: a smaller one lasts as long as its costliest
 * wavefront under any order.  Default on; results do not depend on it.
 * Cost to know about: that one hx_reset(startDate) uploads the reordered rows and, unless the
 * spinup is shared by all members, integrates the spinup again before it returns (it BLOCKS for
 * hx_last_spinup_ms, which then reports that spinup; 0 when the shared spinup was reused), and a
 * hx_setvar afterwards falls back to the parameter key -- a calibration loop that changes
 * parameters every iteration (setvar / reset / run) gains nothing from it and should switch it
 * off with hx_set_lane_calibration(core, 0).
 * hx_lanes_calibrated: 1 once the measured order is in use. */
int hx_set_lane_calibration(hx_core *core, int on);
int hx_lanes_calibrated(hx_core *core, int *yes);
/* A one-shot run has no measured costs of its own.  After a complete run every core fits
 * cost ~ quadratic in its varying parameter rows (standardised) to what it measured and files the
 * model under its scenario table, biome count and varying rows, process-wide; a LATER core with
 * the same key (the larger ensemble of the same study, the next iteration of a calibration loop
 * after hx_setvar) orders its lanes by the predicted cost from its first run on -- where the
 * order matters, more wavefronts than SIMDs.  hx_lane_order_source: what the lanes of the last
 * upload are ordered by -- 0 the parameter key, 1 this core's measured cost, 2 the model's
 * prediction.  hx_set_cost_model(core, 0) / HECTOR_AMD_COST_MODEL=0: neither fit nor use one.
 * Results do not depend on the order.  No counterpart in the reference. */
int hx_lane_order_source(hx_core *core, int *source);
int hx_set_cost_model(hx_core *core, int on);
/* The registry as a file, so that a fresh process -- a genuine one-shot run -- starts with models:
 * hx_cost_models_export writes every model the process holds (text, one record per model),
 * hx_cost_models_load adds a file's models to the registry (count: how many).  Without either
 * call the library reads $HECTOR_AMD_COST_MODELS, else <its directory>/../data/cost_models.txt
 * -- the models shipped with the scenarios (tools/make_cost_models.py) -- once, before the first
 * lookup.  A model is keyed on the scenario's per-year table, the biome count, the varying rows,
 * the values of the uniform rows and the constraint mask; it only orders lanes.  No counterpart
 * in the reference. */
int hx_cost_models_export(const char *path, int *count);
int hx_cost_models_load(const char *path, int *count);
int hx_lane_of_member(hx_core *core, int *out /* n_members */);

/* reset(core, date)  src/rcpp_hector.cpp:103-151 -> Core::reset src/core.cpp:511-549.
 * date < startDate (e.g. 0): rerun the spinup on the next run; date == startDate:
 * back to the post-spinup state; any other computed date if hx_enable_history is on. */
int hx_reset(hx_core *core, double date);

/* run(core, runtodate)  src/rcpp_hector.cpp:153-181 -> Core::run src/core.cpp:448-509.
 * runtodate < 0: run to endDate.  Callable repeatedly with increasing dates.
 * hx_run returns after the GPU work is queued; hx_sync waits for it.
 * Prepares the core first (parameter upload, spinup) if anything changed. */
int hx_run(hx_core *core, double runtodate);
int hx_sync(hx_core *core);

/* fetchvars(core, dates, var)  R/messages.R:46-88: GETDATA per (variable, year).
 * out[(year - year0) * n_members + member], host memory. */
int hx_fetchvars(hx_core *core, const char *capability, int year0, int year1, double *out);
/* Same data without leaving the GPU: device pointer to the variable's
 * [n_years_total][npad] array (row = year - startDate, npad >= n_members), columns in
 * LANE order (see hx_lane_of_member). */
int hx_device_var(hx_core *core, const char *capability, const double **d_ptr, int *npad);
/* ... of one shard of a multi-GPU core (memory of that shard's GPU, npad of that shard) */
int hx_device_var_shard(hx_core *core, int shard, const char *capability, const double **d_ptr,
                        int *npad);
/* Per-year ensemble statistics {count, sum, sum of squares, min, max} of one
 * variable into a caller-owned DEVICE buffer of (year1-year0+1)*5 doubles --
 * the sufficient statistics that a multi-GPU job all-reduces over RCCL.  The kernel runs on the
 * core's stream (hx_stream) and has finished when the call returns; work the caller queued on
 * d_stats on another stream (e.g. a fill) must have completed before the call.  On a core that
 * spans several GPUs or joined a communicator this is hx_ensemble_stats for one variable (d_stats
 * on the first shard's GPU). */
int hx_stats_device(hx_core *core, const char *capability, int year0, int year1,
                    double *d_stats);

/* Misfit of every member against an observed record, on the device; no counterpart in the
 * reference (its hosts score fetchvars() data frames in R).
 *   chi2[member] = sum_i r_i^2,  r_i = ((x(years[i], member) - base(member)) - obs[i]) / sigma[i]
 * x: a RECORDED output (hx_set_outputs), years inside startDate..current date, in any order.
 * obs[i] NaN: that year is skipped.  sigma NULL: no division.
 * base_year0 <= base_year1: base = the member's own mean of x over those years (an anomaly relative
 * to a reference period); base_year0 > base_year1: base is not subtracted.
 * Evaluated per member in exactly this order, in IEEE double, without fused multiply-add:
 *   s = 0.0; for y = base_year0..base_year1: s = s + x_y;  base = s / count;
 *   chi = 0.0; for i = 0..n-1 with obs_i not NaN: r = ((x_i - base) - obs_i) / sigma_i;
 *   chi = chi + (r * r)  -- the product rounded before the sum
 * (no baseline: r = (x_i - obs_i) / sigma_i), so numpy reproduces it bit for bit and the result
 * does not depend on lane order, kernel flavour or shard layout.
 * out[n_members] in the caller's member order; *n_used (may be NULL) = years that counted.
 * Cost: one kernel, one lane per member, n (+ reference period) coalesced row reads, and
 * n_members doubles back to the host; returns when they are there.  The core is not prepared, spun
 * up or dirtied.  Errors: an unrecorded capability, dates outside startDate..current date, n < 1. */
int hx_member_score(hx_core *core, const char *capability, const int *years, const double *obs,
                    const double *sigma, int n, int base_year0, int base_year1,
                    double *out, int *n_used);

/* Misfit of every member against an observed record whose errors are CORRELATED, on the device: the
 * generalised chi-square r^T C^-1 r for an error covariance C = L L^T, given as the whitening matrix
 * W = L^-1 (lower-triangular, n x n, row-major: whiten[i * n + k]); no counterpart in the reference.
 *   r_k = (x(years[k], member) - base(member)) - obs[k]      (no baseline: r_k = x - obs[k])
 *   y_i = sum_{k <= i} whiten[i * n + k] * r_k,    chi2[member] = sum_i y_i^2
 * x, years (any order, repeats allowed; W refers to the order given) and base as in hx_member_score:
 * base is the sequential sum s = 0.0; s = s + x_y over base_year0..base_year1 and ONE division;
 * base_year0 > base_year1: no baseline.  r is two IEEE subtractions, nothing is fused into them.
 * ONLY the entries with k <= i are read: the upper triangle of whiten may hold anything, NaN included.
 * 1 <= n <= HX_SCORE_WHITENED_MAX.  There is NO skipping: a NaN or infinite obs is an error (dropping
 * a year changes the factorisation, which is the caller's to redo), and so is a non-finite whiten
 * entry at k <= i.  A member whose x is NaN in a scored year or in the reference period gets NaN (an
 * infinite x: NaN or infinity); no other member is affected.
 * The ORDER of the sums and the use of fused multiply-adds are NOT part of the definition (the
 * contraction runs on the fp64 matrix pipe).  The error bound is: with s_i = sum_{k <= i}
 * |whiten[i * n + k] * r_k| and the r_k as above,
 *   |chi2 - sum_i y_i^2 evaluated exactly| <= (3 n + 8) 2^-53 sum_i s_i^2
 * (each y_i within n 2^-53 s_i of its exact value, |y_i| <= s_i, and the squares and their n additions
 * of non-negative terms add (n + 1) 2^-53), whatever the order.  Every member's sums are formed in ONE
 * fixed order: the result for a member is bit-identical from call to call and depends neither on lane
 * order, kernel flavour or shard layout, nor on which other members exist.
 * out[n_members] in the caller's member order.  Cost: one read of the n (+ reference period) rows,
 * about n^2 n_members flops on the matrix pipe, an n x n upload and n_members doubles back to the
 * host; returns when they are there.  The core is not prepared, spun up or dirtied; a core of several
 * shards or in a communicator of several processes scores shard by shard (nothing crosses members).
 * The host-emulation build refuses the call after the argument checks.  Errors: a null argument, n
 * outside 1..HX_SCORE_WHITENED_MAX, a non-finite obs or whiten entry, dates or a reference period
 * outside startDate..current date, an unrecorded capability, a core that has not run. */
#define HX_SCORE_WHITENED_MAX 256
int hx_member_score_whitened(hx_core *core, const char *capability, const int *years, const double *obs,
                             const double *whiten, int n, int base_year0, int base_year1, double *out);

/* Projection of every member's trajectory onto a caller's basis, on the device: a dense m x n matrix
 * (row-major: basis[j * n + k]) applied to every member's residuals -- principal-component scores,
 * the update of an ensemble smoother, any fixed linear functional; no counterpart in the reference.
 *   r_k = (x(years[k], member) - base(member)) - center[k]      (no baseline: r_k = x - center[k])
 *   out[j * n_members + member] = sum_{k < n} basis[j * n + k] * r_k,    j < m
 * x, years (any order, repeats allowed; basis refers to the order given) and base as in
 * hx_member_score: base is the sequential sum s = 0.0; s = s + x_y over base_year0..base_year1 and ONE
 * division; base_year0 > base_year1: no baseline.  r is two IEEE subtractions, nothing is fused into
 * them.  center == NULL means zeros: the second subtraction is then - 0.0.
 * 1 <= n <= HX_PROJECT_MAX_YEARS and 1 <= m <= HX_PROJECT_MAX_OUT.  There is NO skipping: a NaN or
 * infinite center or basis entry is an error.  A member whose x is NaN in any year read or in the
 * reference period gets NaN in ALL m outputs -- a zero coefficient does not mask it (an infinite x:
 * NaN or infinity); no other member is affected.
 * The ORDER of the sum and the use of fused multiply-adds are NOT part of the definition (the
 * contraction runs on the fp64 matrix pipe).  The error bound is: with s_j = sum_k
 * |basis[j * n + k] * r_k| and the r_k as above,
 *   |out_j - sum_k basis[j * n + k] * r_k evaluated exactly| <= (n + 2) 2^-53 s_j
 * (a dot product of length n in any order, fused or not, is within (n + 1) 2^-53 s_j of exact while
 * n 2^-53 << 1; one more for slack).  Every (output, member) sum is formed in ONE fixed order: the
 * result is bit-identical from call to call and depends neither on lane order, member sorting, kernel
 * flavour or shard layout, nor on which other members exist, nor on which other rows basis has or at
 * which position row j stands.
 * out[m * n_members], row j in the caller's member order.  Cost: one read of the n (+ reference
 * period) rows, 2 n m n_members flops on the matrix pipe, an n x m upload and m x n_members doubles
 * back to the host; returns when they are there.  The core is not prepared, spun up or dirtied; a
 * core of several shards or in a communicator of several processes projects shard by shard (nothing
 * crosses members).  The host-emulation build refuses the call after the argument checks.  Errors: a
 * null argument (center excepted), n outside 1..HX_PROJECT_MAX_YEARS, m outside 1..HX_PROJECT_MAX_OUT,
 * a non-finite center or basis entry, dates or a reference period outside startDate..current date,
 * an unrecorded capability, a core that has not run. */
#define HX_PROJECT_MAX_OUT   64
#define HX_PROJECT_MAX_YEARS 1024
int hx_member_project(hx_core *core, const char *capability, const int *years, const double *center,
                      const double *basis, int n, int m, int base_year0, int base_year1, double *out);

/* Per-year weighted quantiles over the whole ensemble, on the device; no counterpart in the
 * reference.  out[(year - year0) * nprobs + j] = the probs[j]-quantile of x(year, .) over the members
 * that take part, weighted by weights[n_members] (member order; NULL = every member weight 1);
 * n_part[year - year0] (may be NULL) = members that took part.  1 <= nprobs <= 16, 0 <= probs <= 1.
 * Definition: the weighted inverted CDF (Hyndman-Fan type 1, numpy's method="inverted_cdf").  The
 * weights are made integers once, q_m = (uint64) rint(w_m / wmax * 2^32) with wmax the largest
 * weight of the WHOLE ensemble (NULL weights: q_m = 1); a member takes part in a year if q_m > 0 and
 * its value that year is not NaN; with the participating values sorted ascending and W = sum q, the
 * answer for p is the value of the first member in that order whose running sum of q reaches
 * t = max(1, ceil(p * (double) W)).  Every sum is an exact integer, the result is a value some
 * member has, bit-identical under any lane order or shard split; a year in which nobody takes
 * part gives NaN and n_part = 0.
 * Cost: an exact most-significant-digit radix select on the order-preserving 64-bit image of the
 * doubles, begun at the highest bit in which the year's min and max differ: one read of the
 * year's row for min / max and one per 8-bit digit (at most 8) for ALL probabilities together;
 * nprobs (+ 4) x n_years values back to the host; returns when they are there.  A core of several
 * shards adds the shards' integer histograms on the host after every digit (the same bits as one
 * core); a core that joined a communicator of several processes is refused.  The core is not
 * prepared, spun up or dirtied.  Errors: an unrecorded capability, dates outside startDate..current
 * date, nprobs outside 1..16, a probability outside [0, 1], a negative, NaN or infinite weight,
 * weights that are all zero.  Not available in the host-emulation build of the test suite. */
int hx_ensemble_quantiles(hx_core *core, const char *capability, int year0, int year1,
                          const double *weights, const double *probs, int nprobs,
                          double *out, long long *n_part);

/* ---- A number per member, its weighted distribution, and outcome classes ----------------------
 * The metric_calc / prob_calc step of a perturbed-parameter workflow, on the device; no counterpart
 * in the reference (its hosts do this in R on fetchvars() data frames).
 *
 * A metric specification reduces the window year0..year1 of ONE recorded output to one double per
 * member.  base_year0 <= base_year1: the member's own mean over that reference period is subtracted
 * first; base_year0 > base_year1: nothing is subtracted.  threshold: the two _GE operations only. */
typedef struct {
  int op, year0, year1, base_year0, base_year1, reserved;
  double threshold;
} hx_metric;
#define HX_MET_MEAN 0        /* mean of a over the window */
#define HX_MET_MIN 1         /* smallest a */
#define HX_MET_MAX 2         /* largest a */
#define HX_MET_YEAR_OF_MIN 3 /* the first year that holds the smallest a */
#define HX_MET_YEAR_OF_MAX 4 /* the first year that holds the largest a */
#define HX_MET_FIRST_GE 5    /* the first year with a >= threshold; NaN if there is none */
#define HX_MET_COUNT_GE 6    /* the number of years with a >= threshold */
#define HX_MET_SLOPE 7       /* ordinary least-squares trend of a, per year */
#define HX_MET_NOPS 8
#define HX_MET_MAX_SPECS 32
#define HX_BIN_MAX_EDGES 31

/* out[s * n_members + member] = metric s of every member, in the caller's member order;
 * 1 <= nspecs <= 32, all on the one recorded output `capability`.
 * Evaluated per member in exactly this order, in IEEE double, without fused multiply-add, so that
 * numpy reproduces it bit for bit under any lane order, kernel flavour or shard layout:
 *   base:  s = 0.0; for y = base_year0..base_year1: s = s + x_y;  base = s / count
 *   a_y = x_y - base (with a reference period), a_y = x_y (without); y ascends from year0 to year1
 *   MEAN:  s = 0.0; s = s + a_y;  result s / count
 *   MIN / MAX:  m = a_year0; a later a_y replaces m on strict < / > (the first occurrence is kept)
 *   YEAR_OF_MIN / YEAR_OF_MAX:  the year of that first occurrence, as a double
 *   FIRST_GE:  the first year with a_y >= threshold, as a double; NaN if there is none
 *   COUNT_GE:  the number of years with a_y >= threshold, as a double
 *   SLOPE:  t_y = (double) y - 0.5 * (double) (year0 + year1)  (exact);
 *           num = 0.0; num = num + (t_y * a_y)  -- the product rounded before the sum;
 *           den = 0.0; den = den + (t_y * t_y);  result num / den  (a one-year window: NaN)
 *   NaN rule: if any x_y of the window or of the reference period is NaN, the result is NaN.
 * Cost: one kernel, one lane per member; specifications are handled four at a time, and the four
 * of a group read every row of the union of their reference periods once and every row of the
 * union of their windows once (sixteen rows of a lane in flight at a time); nspecs x n_members
 * doubles back to the host; returns when they are there.  A core of several shards routes the call
 * to every shard.  The core is not prepared, spun up or dirtied.
 * Errors (every message names the function): an unrecorded capability ("not enabled"), nspecs
 * outside 1..32, an unknown op, year1 < year0, a window or reference period outside
 * startDate..current date, a NaN threshold for FIRST_GE / COUNT_GE, a core that has not run. */
int hx_member_metrics(hx_core *core, const char *capability, const hx_metric *specs, int nspecs,
                      double *out);

/* The weighted quantiles of every metric over the ensemble: out[s * nprobs + j], n_part[s] (may be
 * NULL) = members that took part.  Definition, weights, limits and errors of hx_ensemble_quantiles,
 * with the members' metric values (as hx_member_metrics defines them) in place of a year's row; a
 * member whose metric is NaN does not take part.  The metric block is computed on the device and
 * selected there: it never reaches the host.  A core of several shards adds the shards' integer
 * histograms on the host; a communicator of several processes is refused.  Not available in the
 * host-emulation build of the test suite. */
int hx_metric_quantiles(hx_core *core, const char *capability, const hx_metric *specs, int nspecs,
                        const double *weights, const double *probs, int nprobs, double *out,
                        long long *n_part);

/* Weighted probabilities of outcome classes, per recorded year.  edges[nedges]: finite, strictly
 * ascending, 1 <= nedges <= 31.  The bin of x is the number of edges <= x (numpy's
 * searchsorted(edges, x, side="right")): bin 0 is x < edges[0], bin nedges is x >= edges[nedges-1];
 * a value equal to an edge lies in the upper bin.  A member takes part exactly as in
 * hx_ensemble_quantiles (q_m > 0 with the same integer weights q, value not NaN).
 *   sums[(year - year0) * (nedges + 1) + b] = Q_b, the integer sum of q over the members in bin b
 *   prob[same index] = (double) Q_b / (double) W,  W = sum_b Q_b
 *   n_part[year - year0] = members that took part;  nobody: prob NaN, sums 0, n_part 0.
 * sums and n_part may be NULL.  Every sum is an exact integer: the result does not depend on lane
 * order or shard split.  Cost: ONE read of every row (a select needs up to nine); a core of several
 * shards adds the shards' sums on the host; a communicator of several processes is refused.  The
 * core is not prepared, spun up or dirtied.  Errors: those of hx_ensemble_quantiles for capability,
 * dates and weights; nedges outside 1..31; edges not finite or not strictly ascending.  Not
 * available in the host-emulation build of the test suite. */
int hx_ensemble_probabilities(hx_core *core, const char *capability, int year0, int year1,
                              const double *weights, const double *edges, int nedges, double *prob,
                              unsigned long long *sums, long long *n_part);

/* The same over metrics: row s is metric s of every member (computed and binned on the device);
 * prob[s * (nedges + 1) + b], sums likewise, n_part[s]. */
int hx_metric_probabilities(hx_core *core, const char *capability, const hx_metric *specs,
                            int nspecs, const double *weights, const double *edges, int nedges,
                            double *prob, unsigned long long *sums, long long *n_part);

/* Weighted moments of every recorded year over the ensemble, and its cross moments with up to 8
 * per-member predictors (parameters, metrics): what a weighted mean, variance, correlation or
 * regression of an output against the members' parameters needs, year by year, without the
 * trajectories leaving the device.  No counterpart in the reference.
 *   weights[n_members] (member order) or NULL; predictors[k * n_members + m], 0 <= npred <= 8.
 * The weights become the integers q exactly as in hx_ensemble_quantiles (wmax over the WHOLE
 * ensemble; NULL: q_m = 1).  A member takes part in a row if q_m > 0, its value x in that row is not
 * NaN, and every one of its predictor values is finite (so a NaN metric used as a predictor removes
 * the member, as a NaN value does).
 * Shifts: c_y = the smallest participating x of the row (an exact value some member has); c_k = the
 * smallest of predictor k over the members with q_m > 0 and all predictors finite.  d = x - c_y and
 * e_k = p_k - c_k are each ONE IEEE subtraction -- that rounding is part of the definition -- and
 * both are >= 0.  Over the participants of the row:
 *   W = sum q (exact integer)      A = sum q d        B = sum q d d
 *   C_k = sum q e_k                D_k = sum q e_k e_k        E_k = sum q d e_k
 *   shift[y] = c_y;  wsum[y] = W;  n_part[y] = participants (wsum, n_part may be NULL);
 *   sums[y * (2 + 3 npred) + ...] = A, B, then C_k, D_k, E_k for k = 0 .. npred - 1.
 * A row in which nobody takes part: shift NaN, sums 0, W 0, n_part 0.  Every term is >= 0, so a sum
 * in any order is within (n_part + 8) 2^-53 of the exact one, relatively, and the statistics below
 * are conditioned by the spread of the row and not by its magnitude.  In double:
 *   mean = c_y + A/W        var = B/W - (A/W)^2   (the population variance)
 *   pmean_k = c_k + C_k/W   pvar_k = D_k/W - (C_k/W)^2
 *   cov_k = E_k/W - (A/W)(C_k/W)    corr_k = cov_k / sqrt(var pvar_k)    slope_k = cov_k / pvar_k
 * (corr and slope are undefined where a variance is 0; c_k is not returned: it is the smallest
 * predictor value over the members named above.)  W and the sums scale with the quantisation: NULL
 * weights give q_m = 1, weights of all ones q_m = 2^32, so W and every sum of the second call are
 * exactly 2^32 times those of the first; only the statistics above do not depend on the scale of
 * the weights (those two calls give them bit for bit).
 * Reproducibility: W, n_part and c_y are exact under any lane order or shard split.  The floating
 * sums are NOT bit-identical across lane orders or shard splits, unlike the integer verbs above; they
 * ARE bit-identical from call to call for the same core, lane order and shard layout: no floating
 * atomics, a fixed reduction tree inside a workgroup, workgroup partials added in ascending chunk
 * order, shards added on the host in ascending shard order.
 * Cost: the predictors and weights go to lane order (one lane-local kernel), one read of every row
 * for the minimum and one for all sums; 2 + 3 npred (+ 4) values a row back to the host.  A
 * communicator of several processes is refused.  The core is not prepared, spun up or dirtied.
 * Errors (every message names the function; a refused call changes nothing): those of
 * hx_ensemble_quantiles for capability, dates and weights; npred outside 0..8; predictors NULL with
 * npred > 0; a core that has not run.  Not available in the host-emulation build of the test suite. */
#define HX_MOM_MAX_PRED 8
int hx_ensemble_moments(hx_core *core, const char *capability, int year0, int year1,
                        const double *weights, const double *predictors, int npred, double *shift,
                        double *sums, unsigned long long *wsum, long long *n_part);

/* The same over metrics: row s is metric s of every member (as hx_member_metrics defines it,
 * computed on the device); shift[s], sums[s * (2 + 3 npred) + ...], wsum[s], n_part[s]. */
int hx_metric_moments(hx_core *core, const char *capability, const hx_metric *specs, int nspecs,
                      const double *weights, const double *predictors, int npred, double *shift,
                      double *sums, unsigned long long *wsum, long long *n_part);

/* ---- Grouped summaries: quantiles, classes and moments per class of member, in one call ----------
 * An ensemble is rarely one population: several scenarios in one launch (hx_setvar_dated_mix),
 * blocks of a design, members binned by a parameter.  labels[n_members] (member order) gives every
 * member its group 0 .. ngroups-1, or -1 for "in no group"; 1 <= ngroups <= HX_GROUP_MAX.  No
 * counterpart in the reference.
 * Rows: specs == NULL: the years year0..year1 of `capability` (nspecs is not read); specs != NULL:
 * the nspecs metrics of every member as hx_member_metrics defines them (year0 / year1 are not read).
 * Every output is group-major: row r of group g stands at index g * nrows + r.
 * Weights: they become the integers q ONCE, exactly as in hx_ensemble_quantiles -- wmax is the
 * largest weight of the WHOLE ensemble whatever the labels, NULL gives q_m = 1 -- so that the groups'
 * W add up to the W of the ungrouped call over the labelled members.
 * Definition: the result for group g is what the ungrouped verb computes from the weights q^g, where
 * q^g_m = q_m if labels[m] == g and 0 otherwise: the same participation rule with W_g and n_part per
 * (group, row), the rank target t = max(1, ceil(p * (double) W_g)), the bins of
 * hx_ensemble_probabilities, the shifts c_{y,g} (the smallest participating value of the row in the
 * group), the predictor shifts c_{k,g} (the smallest of predictor k over the group's members with
 * q_m > 0 and all predictors finite) and the sums A, B, C_k, D_k, E_k of hx_ensemble_moments.  A
 * group nobody takes part in for a row -- an empty group, all its members NaN, all its weights
 * quantised to 0 -- gives NaN quantiles, probabilities and shift, zero sums, W 0 and n_part 0; a group
 * without a member that has q_m > 0 and finite predictors gives NaN predictor shifts.
 *   hx_group_quantiles:      out[(g * nrows + r) * nprobs + j], n_part[g * nrows + r] (may be NULL);
 *                            1 <= nprobs <= 16.
 *   hx_group_probabilities:  prob[(g * nrows + r) * (nedges + 1) + b], sums likewise (may be NULL),
 *                            n_part[g * nrows + r] (may be NULL): with one row, the contingency table
 *                            of (group x class).
 *   hx_group_moments:        shift[g * nrows + r], sums[(g * nrows + r) * (2 + 3 npred) + ...],
 *                            wsum and n_part[g * nrows + r] (may be NULL), pshift[g * npred + k] (may be
 *                            NULL): the predictor shifts, which differ per group; 0 <= npred <= 8.
 * Reproducibility: quantiles, bin sums, W, n_part and the shifts are exact integers or values some
 * member has, bit-identical under any lane order or shard split.  The floating sums are bit-identical
 * from call to call for one core, lane order and shard layout (no floating atomics, fixed trees,
 * partials added in ascending order), and every one is within (n_part + 8) 2^-53 of the exact sum of
 * its group, relatively.
 * Cost: the labels go to lane order once per call; every pass reads a row ONCE whatever ngroups is
 * (one pass for min / max / W, one per 8-bit digit of the select while any group of the row is open,
 * one for the bins, two for the moments), against ngroups times that for masked calls.  A core of
 * several shards combines the shards' integer histograms, sums and minima on the host over the
 * (group, row) pairs; a communicator of several processes is refused.  The core is not prepared, spun
 * up or dirtied.
 * Errors (every message names the function; a refused call changes nothing): those of the ungrouped
 * verb; labels NULL; ngroups outside 1..16; a label below -1 or >= ngroups; no member with a label
 * >= 0.  The host-emulation build of the test suite refuses each function after the argument checks. */
#define HX_GROUP_MAX 16
int hx_group_quantiles(hx_core *core, const char *capability, int year0, int year1, const hx_metric *specs,
                       int nspecs, const int *labels, int ngroups, const double *weights, const double *probs,
                       int nprobs, double *out, long long *n_part);
int hx_group_probabilities(hx_core *core, const char *capability, int year0, int year1, const hx_metric *specs,
                           int nspecs, const int *labels, int ngroups, const double *weights,
                           const double *edges, int nedges, double *prob, unsigned long long *sums,
                           long long *n_part);
int hx_group_moments(hx_core *core, const char *capability, int year0, int year1, const hx_metric *specs,
                     int nspecs, const int *labels, int ngroups, const double *weights,
                     const double *predictors, int npred, double *shift, double *pshift, double *sums,
                     unsigned long long *wsum, long long *n_part);

/* Variance-based (Sobol) sensitivity sums of every recorded year from a Saltelli design: what the
 * first-order and total indices of an output with respect to k factors need, year by year, without
 * the trajectories leaving the device.  No counterpart in the reference.
 * The design (hector_amd.ensemble.saltelli lays it out) is n_base groups of k + 2 CONSECUTIVE members:
 * member j(k+2) ran the parameters A_j, member j(k+2)+1 ran B_j, and member j(k+2)+2+i ran A_j with
 * factor i taken from B_j.  1 <= k <= 16, n_base >= 1, n_base (k + 2) <= n_members; members past
 * n_base (k + 2) are ignored.  use[n_base] or NULL.
 * Group j, row y: x_A, x_B and x_i (i < k) are the row's values of those members.  A group takes
 * part in a row if use is NULL or use[j] != 0, and none of its k + 2 values is NaN: a NaN anywhere
 * removes the whole group from that row.
 * Shift: c_y = the smallest x_A or x_B over the participating groups (an exact value some member
 * has).  Every difference below is ONE IEEE subtraction -- that rounding is part of the definition
 * -- and everything else is products of the differences, so every term is >= 0.  Over the
 * participating groups of the row:
 *   dA = x_A - c_y;  dB = x_B - c_y
 *   SA1 = sum dA     SA2 = sum dA dA     SB1 = sum dB     SB2 = sum dB dB
 *   e = x_A - x_i;  t = e e;   T_i = sum t     TT_i = sum t t
 *   g = x_B - x_i;  u = g g;   F_i = sum u     FF_i = sum u u
 *   shift[y] = c_y;  n_part[y] = participating groups;
 *   sums[y * (4 + 4 k) + ...] = SA1, SA2, SB1, SB2, then T_i, TT_i, F_i, FF_i for i = 0 .. k - 1.
 * A row in which no group takes part: shift NaN, sums 0, n_part 0.  Every sum, in any order, is
 * within (n_part + 8) 2^-53 of the exact sum of the terms as defined, relatively.  In double, with
 * n = n_part[y]:
 *   m = (SA1 + SB1) / (2 n)      mean = c_y + m
 *   V = (SA2 + SB2) / (2 n) - m m      (the population variance of the 2 n pooled A and B values)
 *   total_i = T_i / (2 n V)            (Jansen's estimator of the total index)
 *   first_i = 1 - F_i / (2 n V)        (Jansen's form of the first-order index)
 *   total_se_i = sqrt((TT_i / n - (T_i / n)^2) / n) / (2 V);  first_se_i the same from F_i, FF_i
 * The two standard errors are those of the numerators T_i / (2 n) and F_i / (2 n) with V taken as
 * known: the sampling error of V itself is not in them.  Where V == 0 or n == 0 the indices and
 * their standard errors are undefined.
 * Reproducibility: n_part and c_y are exact under any lane order.  The floating sums are NOT
 * bit-identical across lane orders; they ARE bit-identical from call to call for the same core and
 * lane order: no floating atomics, a fixed reduction tree inside a workgroup, workgroup partials
 * added in ascending chunk order.
 * Cost: one lane-local kernel turns the lane order into a group-major lane table; one pass of
 * gathered 8-byte loads over every row for participation, the minimum and the count, and one for
 * all sums (k > 8: two, A and B re-read from the cache); 4 + 4 k (+ 2) values a row back to the host.
 * The core is not prepared, spun up or dirtied.
 * Errors (every message names the function; a refused call changes nothing): those of
 * hx_ensemble_moments for capability and dates; k outside 1..16; n_base < 1 or n_base (k + 2) >
 * n_members; a core that has not run; a core of several shards (a group's members lie on different
 * GPUs under the fleet's split: not served); a communicator of several processes.  Not available in
 * the host-emulation build of the test suite. */
#define HX_SOBOL_MAX_FACTORS 16
int hx_ensemble_sobol(hx_core *core, const char *capability, int year0, int year1, int k, int n_base,
                      const unsigned char *use, double *shift, double *sums, long long *n_part);

/* The same over metrics: row s is metric s of every member (as hx_member_metrics defines it,
 * computed on the device; the metric block does not reach the host), 1 <= nspecs <= 32; shift[s],
 * sums[s * (4 + 4 k) + ...], n_part[s]. */
int hx_metric_sobol(hx_core *core, const char *capability, const hx_metric *specs, int nspecs, int k,
                    int n_base, const unsigned char *use, double *shift, double *sums, long long *n_part);

/* ---- Two series of the same member: regress or sample one output on another ----------------------
 * A pair-metric specification reduces the window year0..year1 of TWO series of a member, a (reported
 * / dependent) and b (condition / independent), to one double per member: TCRE (the slope of
 * global_tas on cumulative emissions), the CO2 concentration in the year a member crosses 1.5 K, the
 * airborne fraction, a Gregory regression of heat flux on temperature, the pH while warming is above
 * 2 K, the concentration at peak warming.  No counterpart in the reference (its hosts do this in R on
 * fetchvars() data frames of two variables).
 * base_a0 <= base_a1: a's own mean over that reference period is subtracted from a first; base_a0 >
 * base_a1: nothing is subtracted.  base_b0, base_b1: the same for b, with b's own reference period.
 * threshold: the two _GE operations only. */
typedef struct {
  int op, year0, year1;
  int base_a0, base_a1;      /* reference period of a; base_a0 > base_a1: none */
  int base_b0, base_b1;      /* reference period of b; likewise */
  int reserved;
  double threshold;
} hx_pair_metric;
#define HX_PMET_SLOPE 0          /* ordinary least-squares slope of a on b */
#define HX_PMET_INTERCEPT 1      /* its intercept */
#define HX_PMET_R2 2             /* its coefficient of determination */
#define HX_PMET_AT_FIRST_GE 3    /* a in the first year with b >= threshold; NaN if there is none */
#define HX_PMET_AT_MAX 4         /* a in the first year that holds the largest b */
#define HX_PMET_AT_MIN 5         /* a in the first year that holds the smallest b */
#define HX_PMET_MEAN_WHERE_GE 6  /* mean of a over the years with b >= threshold; NaN if there is none */
#define HX_PMET_END_RATIO 7      /* (a_year1 - a_year0) / (b_year1 - b_year0) */
#define HX_PMET_NOPS 8
#define HX_PMET_MAX_SPECS 32

/* out[s * n_members + member] = pair metric s of every member, in the caller's member order;
 * 1 <= nspecs <= 32, all on the one pair of operands.
 * cap_a: a per-member variable on the device like every other verb's `capability` (a recorded output,
 * a derived diagnostic, a held / derived series).  b is EXACTLY ONE of (both or neither is an error)
 *   - cap_b: a per-member variable, resolved the same way as cap_a (b_vec NULL; b_year0, b_year1 are
 *     ignored), or
 *   - b_vec: a caller's per-year vector, b_y = b_vec[y - b_year0] for b_year0..b_year1, the same for
 *     every member (cumulative emissions, the year itself), with cap_b NULL.  Every window and every
 *     reference period of b must lie inside b_year0..b_year1; a non-finite entry is an error that names
 *     the year.
 * Evaluated per member in exactly this order, in IEEE double, without fused multiply-add, so that
 * numpy reproduces every result bit for bit under any lane order, kernel flavour or shard layout
 * (xa_y, xb_y: the operands' values in year y):
 *   base:  s = 0.0; for y = base_a0..base_a1: s = s + xa_y;  base_a = s / count
 *   a_y = xa_y - base_a (with a reference period), a_y = xa_y (without); b_y likewise with b's own
 *   reference period; y ascends from year0 to year1, n = year1 - year0 + 1
 *   SLOPE, INTERCEPT, R2: two ascending passes.
 *     pass 1:  sa = 0.0; sa = sa + a_y;  sb = 0.0; sb = sb + b_y;  ma = sa / n;  mb = sb / n
 *     pass 2:  da = a_y - ma;  db = b_y - mb;  sab = sab + (db * da);  sbb = sbb + (db * db);
 *              saa = saa + (da * da)  -- every product rounded before its sum
 *     SLOPE = sab / sbb;  INTERCEPT = ma - (SLOPE * mb);  R2 = (sab * sab) / (sbb * saa)
 *     Degenerate windows are whatever IEEE gives: a constant b or a one-year window is 0 / 0 = NaN;
 *     there is no special case and no sqrt.
 *   AT_FIRST_GE:  a_y of the first year with b_y >= threshold; NaN if there is none
 *   AT_MAX / AT_MIN:  a_y of the first year that holds the largest / smallest b_y: a later year
 *     replaces an earlier one only on strict > / <
 *   MEAN_WHERE_GE:  s = 0.0; s = s + a_y over the years with b_y >= threshold, ascending, divided by
 *     their count as a double; none: 0 / 0 = NaN
 *   END_RATIO:  (a_year1 - a_year0) / (b_year1 - b_year0); reads only the two end rows and the
 *     reference periods
 *   NaN rule: a NaN of a or b in any row the specification reads (window and reference periods; for
 *   END_RATIO the two end rows and the reference periods) makes the result NaN.
 * Cost: one kernel, one lane per member, one specification per workgroup row (no grouping: a second
 * specification re-reads its rows from L2); the reference rows, then one pass over the window (two
 * for SLOPE / INTERCEPT / R2, none for END_RATIO) with eight rows of each operand of a lane in
 * flight; nspecs x n_members doubles back to the host; returns when they are there.  A core of
 * several shards or in a communicator of several processes runs shard by shard (nothing crosses
 * members).  The core is not prepared, spun up or dirtied.
 * Errors (every message names the function; a refused call changes nothing): a null argument, an
 * unrecorded capability ("not enabled"), nspecs outside 1..32, an unknown op, year1 < year0, a
 * window or reference period outside the range where both operands are valid (startDate..current
 * date, a series' own end, b_year0..b_year1 of the vector), a NaN threshold for AT_FIRST_GE /
 * MEAN_WHERE_GE, both or neither of cap_b / b_vec, a non-finite b_vec entry, a core that has not
 * run. */
int hx_member_pair_metrics(hx_core *core, const char *cap_a, const char *cap_b, const double *b_vec,
                           int b_year0, int b_year1, const hx_pair_metric *specs, int nspecs,
                           double *out);

/* The weighted quantiles, outcome-class probabilities and moments of every pair metric over the
 * ensemble: the leading arguments of hx_member_pair_metrics, then those of hx_metric_quantiles /
 * hx_metric_probabilities / hx_metric_moments, whose definitions, weights, limits and errors hold
 * with the members' pair-metric values in place of the metric values; a member whose pair metric is
 * NaN does not take part.  The block is computed on the device and reduced there: it never reaches
 * the host.  A core of several shards is combined exactly as for the hx_metric_* functions; a
 * communicator of several processes is refused.  Not available in the host-emulation build of the
 * test suite (refused after the argument checks). */
int hx_pair_metric_quantiles(hx_core *core, const char *cap_a, const char *cap_b, const double *b_vec,
                             int b_year0, int b_year1, const hx_pair_metric *specs, int nspecs,
                             const double *weights, const double *probs, int nprobs, double *out,
                             long long *n_part);
int hx_pair_metric_probabilities(hx_core *core, const char *cap_a, const char *cap_b, const double *b_vec,
                                 int b_year0, int b_year1, const hx_pair_metric *specs, int nspecs,
                                 const double *weights, const double *edges, int nedges, double *prob,
                                 unsigned long long *sums, long long *n_part);
int hx_pair_metric_moments(hx_core *core, const char *cap_a, const char *cap_b, const double *b_vec,
                           int b_year0, int b_year1, const hx_pair_metric *specs, int nspecs,
                           const double *weights, const double *predictors, int npred, double *shift,
                           double *sums, unsigned long long *wsum, long long *n_part);

/* Year-by-year co-moments of two windows of rows over the ensemble: what a full year x year
 * covariance or correlation matrix needs -- an emergent constraint as a map over (observed year,
 * projected year), the EOFs / PCA of the trajectories, the auto-covariance of a residual -- without
 * the trajectories leaving the device.  No counterpart in the reference.
 *   Window A: the rows a_year0..a_year1 of cap_a (na rows); window B: b_year0..b_year1 of cap_b (nb).
 *   cap_a and cap_b are per-member variables on the device like every other verb's `capability`.
 *   cap_b NULL is the SYMMETRIC call: B is A (b_year0, b_year1 are ignored; shift_b, sums_b may be
 *   NULL and receive A's values if they are not).
 *   weights[n_members] (member order) or NULL.
 * The weights become the integers q exactly as in hx_ensemble_quantiles (wmax over the WHOLE
 * ensemble; NULL: q_m = 1).  Participation is by COMPLETE CASES: a member takes part in the call if
 * q_m > 0 and none of its values in the na rows of A and the nb rows of B is NaN.  The call has
 * therefore ONE W = sum q (an exact integer) and ONE n_part.  This differs from
 * hx_ensemble_moments, where participation is per row: a covariance matrix whose entries are taken
 * over differing member sets need not be positive semi-definite.
 * Shifts: c_a = the smallest participating value of row a of A, c_b likewise of B (exact values
 * some member has).  d_a = x_a - c_a and d_b = x_b - c_b are each ONE IEEE subtraction -- that
 * rounding is part of the definition -- and both are >= 0.  Over the participants:
 *   sums_a[a * 2 + ...] = S_a = sum q d_a,  T_a = sum q d_a d_a;   sums_b[b * 2 + ...] likewise
 *   cross[a * nb + b] = sum (q d_a) d_b
 *   shift_a[a] = c_a;  shift_b[b] = c_b;  *wsum = W;  *n_part = participants (may be NULL).
 * Every term is >= 0, so every sum, in any order and with fused multiply-adds, is within
 * (n_part + 8) 2^-53 of the exact one, relatively.  In double:
 *   mean_a = c_a + S_a/W        var_a = T_a/W - (S_a/W)^2   (the population variance)
 *   cov[a][b] = cross[a][b]/W - (S_a/W)(S_b/W)
 *   corr[a][b] = cov[a][b] / sqrt(var_a var_b)      slope[a][b] = cov[a][b] / var_b
 * (corr and slope are undefined where a variance is 0.)
 * The symmetric call computes only the blocks of the matrix on or above the diagonal and mirrors
 * them -- towards half of the contraction's work as the matrix grows (36 of 64 quadrants of 32 x 32
 * for 251 rows), as EOFs want it: cross is then EXACTLY symmetric, and sums_a[a * 2 + 1] is
 * set to cross[a * na + a].
 * Nobody takes part: the shifts are NaN, the sums and cross are 0, W and n_part are 0.
 * Reproducibility: W, n_part and the shifts are exact under any lane order or shard split.  The
 * floating sums are NOT bit-identical across lane orders or shard splits; they ARE bit-identical
 * from call to call for the same core, lane order and shard layout: no floating atomics, a fixed
 * reduction tree, the member chunks' partials added in ascending chunk order, shards added on the
 * host in ascending shard order.
 * Cost: one lane-local read of every row of both windows for the participation mask, one for the
 * minima, one for the rows' own sums, and the contraction over the members on the fp64 matrix pipe
 * (v_mfma_f64_16x16x4_f64): 2 na nb n flops, each row re-read once per 64 rows of the other window.
 * na + nb is limited by the scenario's rows only.  A communicator of several processes is refused.
 * The core is not prepared, spun up or dirtied.
 * Errors (every message names the function; a refused call changes nothing): those of
 * hx_ensemble_quantiles for capability, dates and weights, for either window; a core that has not
 * run.  Not available in the host-emulation build of the test suite.
 * Out of scope: a metric x metric variant, and per-entry (pairwise) participation. */
int hx_ensemble_comoments(hx_core *core, const char *cap_a, int a_year0, int a_year1,
                          const char *cap_b, int b_year0, int b_year1, const double *weights,
                          double *shift_a, double *sums_a, double *shift_b, double *sums_b,
                          double *cross, unsigned long long *wsum, long long *n_part);

/* ---- Held and derived per-member series -----------------------------------------------------------
 * What the six verbs above, hx_fetchvars, hx_stats_device / hx_ensemble_stats and hx_device_var call
 * `capability` is "a per-member variable on the device", one of
 *   - a RECORDED output (hx_set_outputs), valid to the current date: exactly as before;
 *   - a diagnostic the core derives on the device from recorded outputs -- slr, sl_rc, slr_no_ice,
 *     sl_rc_no_ice, HL_/LL_sst, _DIC, _CO3, _Revelle, _OmegaAr, _OmegaCa, ocean_tas, RF_N2O, RF_CH4,
 *     RF_H2O_strat, RF_O3_trop -- or a whole-surface combination pH, PCO2, DIC, CO3
 *     ((0.85 * LL) + (0.15 * HL), each product rounded) or ML_ocean_c (LL + HL): computed for
 *     startDate..current date into a block the core keeps until the next run or reset; the outputs it
 *     is derived from must be recorded ("needs ...: enable it ...");
 *   - a SERIES, below: valid to the date it was defined at, NaN behind it.
 * Dates are checked against the variable's own valid range.  A variable that is the same for every
 * member (scenario inputs, the shared gas cycles: hx_fetchvars answers them on the host) is refused by
 * the per-member verbs with a message that says so.  (hx_fetchvars of a diagnostic keeps computing just
 * the rows asked for; hx_device_var of one returns the kept block.)
 *
 * A series is a named [years][members] block of doubles that belongs to the core, filled ONCE by
 * hx_series_define from its operands as they are at the call (the core's pending work is waited for
 * first).  It is a snapshot: later hx_reset, hx_run, hx_setvar, hx_set_outputs do not touch it, and
 * when the core reorders its lanes the block is permuted on the device, so a series always means
 * "member m's trajectory".  At most HX_SER_MAX series per core; hx_shutdown frees them.
 * Names match [A-Za-z_][A-Za-z0-9_]{0,62} and must not be a name the core already answers (recorded,
 * derived, combination, host-answered; a "<biome>.<pool>" cannot match the pattern).  Defining an
 * existing series replaces it; the operands may name it (everything is read before the new block
 * takes the name).
 *
 * a: any per-member variable as above, valid for startDate..end_a.  The operation (one per call;
 * compose by name), per member, y ascending from startDate, in IEEE double without fused
 * multiply-add, so that numpy reproduces every result bit for bit:
 *   COPY              z_y = a_y
 *   ADD SUB MUL DIV   z_y = a_y op b_y.  b (b_kind): HX_SER_B_VAR a per-member variable `b` (the result
 *                     is valid to min(end_a, end_b)); HX_SER_B_SCALAR b_y = b_scalar;
 *                     HX_SER_B_VECTOR b_y = b_values[y - b_first_year] for b_n years, NaN outside them
 *   ANOMALY           s = 0.0; for y = year0..year1: s = s + a_y;  base = s / count;  z_y = a_y - base
 *                     (hx_member_score's baseline)
 *   CUMSUM            NaN before year0;  z_year0 = a_year0;  z_y = z_(y-1) + a_y  (numpy's cumsum)
 *   RUNMEAN           the window is y-width+1 .. y (align HX_SER_TRAILING) or y-(width-1)/2 .. y+width/2
 *                     (HX_SER_CENTRED, integer division);  s = 0.0; s = s + a_k for k ascending over the
 *                     window -- a fresh sum for every y --;  z_y = s / width;  NaN where the window
 *                     leaves startDate..end_a
 *   DELTA             z_y = a_y - a_(y-lag);  NaN for the first `lag` years
 * Rows behind the valid end hold NaN; a NaN in an operand propagates by IEEE arithmetic, and the
 * verbs' NaN rules then leave that member or year out.
 * Cost: one kernel (ANOMALY two), one lane per member, rows read coalesced; the elementwise
 * operations are a stream with 16 rows of each operand in flight per lane, CUMSUM walks the years of a
 * lane, RUNMEAN re-reads the window per year.  Nothing reaches the host.  A core of several shards
 * forwards the call to every shard; nothing crosses shards or processes.
 * Errors (every message names hx_series_define; a refused call changes nothing): a bad name, a name
 * the core already answers, a 17th series, an unknown op / b_kind / align, width < 1 or beyond the
 * number of years, lag < 1, a reference period or year0 outside startDate..end_a, an operand that is
 * unknown, not recorded, answered on the host, or dropped, a core that has not run, no device memory
 * for the block. */
#define HX_SER_COPY 0
#define HX_SER_ADD 1
#define HX_SER_SUB 2
#define HX_SER_MUL 3
#define HX_SER_DIV 4
#define HX_SER_ANOMALY 5
#define HX_SER_CUMSUM 6
#define HX_SER_RUNMEAN 7
#define HX_SER_DELTA 8
#define HX_SER_NOPS 9
#define HX_SER_B_NONE 0
#define HX_SER_B_VAR 1
#define HX_SER_B_SCALAR 2
#define HX_SER_B_VECTOR 3
#define HX_SER_TRAILING 0
#define HX_SER_CENTRED 1
#define HX_SER_MAX 16
typedef struct {
  int op;               /* HX_SER_* */
  int year0, year1;     /* ANOMALY: the reference period; CUMSUM: year0 = the first year */
  int width, align;     /* RUNMEAN */
  int lag;              /* DELTA */
  int b_kind;           /* ADD SUB MUL DIV: HX_SER_B_* */
  int b_first_year, b_n; /* HX_SER_B_VECTOR */
  int reserved;
  double b_scalar;      /* HX_SER_B_SCALAR */
  const char *b;        /* HX_SER_B_VAR */
  const double *b_values; /* HX_SER_B_VECTOR: b_n values from b_first_year on */
} hx_series_op;
int hx_series_define(hx_core *core, const char *name, const char *a, const hx_series_op *op);
/* Frees a series; an unknown name is an error that names hx_series_drop. */
int hx_series_drop(hx_core *core, const char *name);
/* The series of the core in the order they were first defined: names[i], valid_to[i] (the last year
 * that holds values); either may be NULL.  The arrays stay valid until the next call on this thread. */
int hx_series_list(hx_core *core, const char *const **names, const int **valid_to, int *count);

/* ---- A series from a whole expression, in one pass ------------------------------------------------
 * hx_series_eval defines the series `name` from a postfix program over per-member variables, evaluated
 * per element (member, year) in ONE kernel: every distinct operand row is read once, the result is
 * written once, nothing reaches the host.  All rules of hx_series_define hold unchanged, through the
 * same checks and the same store: names, "a name the core already answers", the 17th series, replacing
 * a series that its own expression names, lane reordering, "run the core first", forwarding to every
 * shard, the no-device-memory message.  An element depends on its own lane's operands only, so the
 * block is bit-identical across lane orders, kernel flavours and shard splits.
 *
 * The operand tables of hx_expr:
 *   vars[nvars]      capability names as for every verb (recorded, derived diagnostic, combination,
 *                    series), each with a lag >= 0 in years.  A (name, lag) pair that occurs twice is ONE
 *                    operand; at most HX_EX_MAX_VARS distinct pairs (nvars itself may reach
 *                    HX_EX_MAX_INS).  The core keeps two blocks of derived diagnostics outside the slr
 *                    family or combinations: an expression that names more than two has each copied
 *                    into a block of its own for the call (a block of memory and a copy apiece).
 *   members[nmem]    pointers to n_members doubles in MEMBER order (a parameter, a weight): the library
 *                    permutes them to lane order, a shard takes its slice.  At most HX_EX_MAX_MEMBERS.
 *   yearvecs[nvec]   first_year, n, values: one value a year for every member, NaN outside the span (as
 *                    HX_SER_B_VECTOR).  At most HX_EX_MAX_YEARVECS.
 *   ins[nins]        {op, arg, value}, 1..HX_EX_MAX_INS instructions; the evaluation stack holds at most
 *                    HX_EX_MAX_STACK values and the program must end with exactly one.
 * Instructions, in program order, in IEEE double with contraction off (no fused multiply-add anywhere),
 * so that numpy reproduces every result but LOG and EXP bit for bit (pops -> pushes):
 *   VAR k              -> the value of operand vars[arg] in year y - lag; NaN if that year is before
 *                      startDate (such a row is not loaded)
 *   MEMBER k           -> members[arg][member]
 *   YEARVEC k          -> yearvecs[arg] in year y, NaN outside the span
 *   CONST              -> value
 *   YEAR               -> (double) calendar year
 *   NEG ABS            a -> -a, fabs(a): sign-bit operations (-0.0 and NaN payloads as numpy)
 *   ADD SUB MUL DIV    a b -> a op b, correctly rounded
 *   SQRT               a -> sqrt(a), correctly rounded
 *   LOG EXP            a -> natural log / exp of the device's math library (the host-emulation build:
 *                      libm): within 1 ulp on the host; measured 0.80 (exp) and 0.50 (log) ulp on the
 *                      MI355X (the bound a conforming device library must keep is 3); log(0) = -inf, log(<0) = NaN,
 *                      exp(-inf) = 0, inf / NaN as libm -- exact on both
 *   MIN MAX            a b -> (a < b || a != a) ? a : b  and  (a > b || a != a) ? a : b: numpy's scalar
 *                      definition -- NaN from either side propagates, at +-0 ties the second operand
 *   LT LE GT GE EQ NE  a b -> NaN if either operand is NaN, else 1.0 or 0.0
 *   WHERE              c a b -> NaN if c is NaN; a if c != 0; otherwise b.  The branch not taken does not
 *                      matter, NaN included.
 *   IFNAN              a b -> b if a is NaN, else a
 * At least one VAR is required.  The series is valid to the smallest valid end over its VAR operands;
 * rows behind that are NaN.
 * Cost: one kernel, one lane per member, rows read coalesced; a lane takes a batch of rows of every
 * operand into registers, all loads in flight, and runs the program once over the batch -- the program
 * is read through scalar loads and decoded once per batch, its stack lives in registers.  One host to
 * device copy of the program record, the member vectors and the year vectors.  A core of several shards
 * forwards the call to every shard.
 * Errors (every message names hx_series_eval; a refused call changes nothing): a null argument, nins
 * outside 1..HX_EX_MAX_INS, an unknown op, an arg outside its table, stack underflow, a depth above
 * HX_EX_MAX_STACK, a program that does not end with exactly one value, more than HX_EX_MAX_VARS distinct
 * (name, lag) pairs, more than HX_EX_MAX_MEMBERS / HX_EX_MAX_YEARVECS of the other tables, no VAR,
 * lag < 0 or >= the core's years, an empty year vector, a null member pointer, a reserved field that is
 * not 0, and every refusal of hx_series_define for a name, an operand (unknown, not recorded, answered
 * on the host, not enabled), a core that has not run and device memory. */
#define HX_EX_VAR 0
#define HX_EX_MEMBER 1
#define HX_EX_YEARVEC 2
#define HX_EX_CONST 3
#define HX_EX_YEAR 4
#define HX_EX_NEG 5
#define HX_EX_ABS 6
#define HX_EX_SQRT 7
#define HX_EX_LOG 8
#define HX_EX_EXP 9
#define HX_EX_ADD 10
#define HX_EX_SUB 11
#define HX_EX_MUL 12
#define HX_EX_DIV 13
#define HX_EX_MIN 14
#define HX_EX_MAX 15
#define HX_EX_LT 16
#define HX_EX_LE 17
#define HX_EX_GT 18
#define HX_EX_GE 19
#define HX_EX_EQ 20
#define HX_EX_NE 21
#define HX_EX_WHERE 22
#define HX_EX_IFNAN 23
#define HX_EX_NOPS 24
#define HX_EX_MAX_INS 64
#define HX_EX_MAX_VARS 8
#define HX_EX_MAX_MEMBERS 8
#define HX_EX_MAX_YEARVECS 8
#define HX_EX_MAX_STACK 8
typedef struct { const char *name; int lag; int reserved; } hx_expr_var;
typedef struct { int first_year, n; const double *values; } hx_expr_yearvec;
typedef struct { int op, arg; double value; } hx_expr_ins;   /* arg: VAR MEMBER YEARVEC; value: CONST */
typedef struct {
  int nvars, nmem, nvec, nins;
  const hx_expr_var *vars;
  const double *const *members;
  const hx_expr_yearvec *yearvecs;
  const hx_expr_ins *ins;
  int reserved[2];
} hx_expr;
int hx_series_eval(hx_core *core, const char *name, const hx_expr *expr);

/* ---- Member ranks within a year's row, and the CRPS of a row against an observation --------------
 * Every member's weighted mid-rank within its year (its mid-PIT), and the continuous ranked
 * probability score of the ensemble against an observed record, by a sort of every row on the
 * device.  No counterpart in the reference.  capability: a per-member variable on the device as for
 * the other verbs (recorded, derived or a series), so the CRPS of an anomaly is hx_series_define
 * (ANOMALY) first and then hx_ensemble_crps of that series.
 * Weights: quantised exactly as for hx_ensemble_quantiles, q_m = rint(w_m / wmax * 2^32), NULL: every
 * q_m = 1; the same weights are refused.  Values are compared as IEEE doubles after x + 0.0, so -0.0
 * and +0.0 tie.
 * Mid-PIT of a member.  For a row, the members whose value is not NaN take part.  W = sum q over
 * them (a q of 0 adds nothing, but such a member still gets a rank).  For member i:
 *   L_i = sum of q_j with x_j < x_i;   E_i = sum of q_j with x_j == x_i (q_i included);
 *   N_i = 2 L_i + E_i      an exact integer <= 2 W <= 2^53
 *   HX_RANK_PIT:        z_i = (double) N_i / (double) (2 W)   one correctly rounded division, in (0, 1]
 *   HX_RANK_NUMERATOR:  z_i = (double) N_i    (NULL weights: the average rank of the member, as
 *                       scipy.stats.rankdata gives it, is (N_i + 1) / 2)
 * A NaN value gives NaN; W = 0 gives NaN for the whole row.  The result does not depend on lane
 * order, kernel flavour or how ties are stored: numpy reproduces it bit for bit
 * (hector_amd.ensemble.midpit).
 * CRPS of a row against an observation y.  The members with q > 0 and a value that is not NaN take
 * part (n_part of them); v_1 < ... < v_m are their distinct values, C_k the running sum of q up to and
 * including v_k, W = C_m, F_k = (double) C_k / (double) W and G_k = (double) (W - C_k) / (double) W (the
 * integer difference: 1 - F is never formed in floating point).  The result is the sum of these
 * non-negative terms, each evaluated in double without fused multiply-add:
 *   v_1 - y  if y < v_1;      y - v_m  if y > v_m;      and for k = 1 .. m-1:
 *   y <= v_k:       (v_(k+1) - v_k) * (G_k * G_k)
 *   y >= v_(k+1):   (v_(k+1) - v_k) * (F_k * F_k)
 *   otherwise the two terms  (y - v_k) * (F_k * F_k)  and  (v_(k+1) - y) * (G_k * G_k)
 * The order of the additions is not fixed; no term is negative, so every result lies within
 * (m + 8) 2^-53, relatively, of the exact sum (four roundings a term, m - 1 additions), as long as
 * the result is a normal double: below 2^-1022 a term or a result is a multiple of 2^-1074.  It equals the
 * energy form sum p |x - y| - 1/2 sum sum p p' |x - x'| with p = q / W.  pit_obs is the mid-PIT of
 * the observation itself, (2 sum q[x < y] + sum q[x == y]) / (2 W), exact as above.  A NaN observation,
 * or a year in which nobody takes part: crps NaN, pit_obs NaN, n_part 0.  With an infinite
 * participating value the result is whatever IEEE arithmetic gives for the formula (inf or NaN).
 * Reproducibility: ranks, pit_obs and n_part are exact; the CRPS is bit-identical from call to call
 * and across lane orders (the terms are added in the order of the sorted values by a fixed tree).
 * Cost: one workgroup per row sorts the row's (key, lane) pairs by a least-significant-digit radix
 * sort, 8 bits a pass, and only the passes below the highest bit in which the row's smallest and
 * largest key differ (a row of equal values runs none, a typical temperature row seven); two more
 * sweeps over the sorted row give the ranks, one the CRPS.  Scratch: 24 bytes a member and row; rows are
 * processed in batches so that it stays under HX_RANK_SCRATCH_MIB MiB (or one row, if that is more).
 * hx_series_rank defines (or replaces) the series `name`: rows year0..year1 hold the ranks of
 * `capability`, every other row NaN, valid_to = year1; all rules of hx_series_define for names, the
 * 16-series limit and lane reordering hold.  With the rank as a series the other verbs do the rest:
 * hx_ensemble_moments of it against ranked predictors is the Spearman correlation,
 * hx_ensemble_probabilities of it a rank histogram.  hx_metric_ranks is the same for a metric block
 * (as hx_member_metrics defines it): out[s * n_members + member], member order, back on the host.
 * hx_ensemble_crps: crps[i], pit_obs[i], n_part[i] (either of the last two may be NULL) for the year
 * years[i] and the observation obs[i]; the years need not be ascending, contiguous or distinct.
 * Errors (every message names its function; a refused call changes nothing): those of
 * hx_ensemble_quantiles for capability, dates and weights; those of hx_series_define for the name;
 * those of hx_member_metrics for the specifications; an unknown kind; nyears < 1; a core that has not
 * run; a core of several shards (a rank needs the whole row on one GPU: not served); a communicator
 * of several processes; no device memory for the scratch or the block.  Not available in the
 * host-emulation build of the test suite. */
#define HX_RANK_PIT 0
#define HX_RANK_NUMERATOR 1
#define HX_RANK_SCRATCH_MIB 512
int hx_series_rank(hx_core *core, const char *name, const char *capability, int year0, int year1,
                   const double *weights, int kind);
int hx_metric_ranks(hx_core *core, const char *capability, const hx_metric *specs, int nspecs,
                    const double *weights, int kind, double *out);
int hx_ensemble_crps(hx_core *core, const char *capability, const int *years, const double *obs,
                     int nyears, const double *weights, double *crps, double *pit_obs, long long *n_part);

/* per-member model-error bitmask (HX_ERR_* below), host array of n_members */
int hx_status(hx_core *core, unsigned *out);
int hx_spinup_steps(hx_core *core, int member, int *steps);

/* Diagnostic: one row of the per-member state table (hx_layout.h HxStateRow /
 * HxBiomeState numbering) at the current date, host array of n_members.  The
 * reference exposes the same quantities as undated GETDATA (e.g. ocean box
 * carbon, max timestep: src/ocean_component.cpp:422-512). */
int hx_state_row(hx_core *core, int row, double *out);

/* Carbon tracking: get_tracking_data(core)  R/hector.R -> Core::getTrackingData
 * (src/core.cpp:199-209, src/csv_tracking_visitor.cpp): where the carbon of every pool
 * originated, from Core::trackingDate on.  Switch it on with
 * hx_setvar(core, "trackingDate", &year, 1, NULL) before running.  Pools (hx_tracking_pools):
 * atmos_c, earth_c, [<biome>.]veg_c/detritus_c/soil_c/permafrost_c/thawedp_c, and the ocean
 * boxes HL, LL, intermediate, deep.  hx_tracking_data: for one member and year0..year1,
 * values[(y-year0)*TP + pool] (Pg C), fractions[((y-year0)*TP + pool)*TP + source] and, if
 * source_masks is not NULL, source_masks[((y-year0)*TP + pool)*W + s/64] with bit s%64 set where
 * source s is in the pool's map (the rows CSVFluxPoolVisitor::print_pool writes); W = (TP+63)/64
 * words per pool: 1 up to 11 biomes (TP = 6 + 5 biomes <= 64), 2 from 12 biomes on.  A [core]
 * trackingDate in the INI switches tracking on as well; hector-amd then writes
 * tracking_<run_name>.csv.  Any biome count (1-16).  Costs TP*TP*8 B per member-year of HBM
 * (968 B for one biome, 59 KB for sixteen; a record that does not fit is refused with the
 * numbers); not combinable with a CO2 or NBP constraint. */
int hx_tracking_pools(hx_core *core, const char *const **names, int *count);
int hx_tracking_data(hx_core *core, int member, int year0, int year1, double *values,
                     double *fractions, unsigned long long *source_masks);

/* getunits(var)  R/units.R (unit strings of src/unitval.cpp:30-165) and the component that owns
 * the variable (IModelComponent::getComponentName, as printed by the output stream): for
 * parameters, inputs, constraints and outputs.  The strings stay valid until the next call on
 * this thread. */
int hx_var_info(hx_core *core, const char *capability, const char **component, const char **units);
/* Core::getRun_name (src/core.cpp:215-220): the INI's [core] run_name, "" if none */
int hx_run_name(hx_core *core, const char **name);
/* Unit vectors for function-level parity tests (no core needed).
 * hx_unit_csys: oceancsys::ocean_csys_run (src/ocean_csys.cpp:166-366) for n independent
 *   (T degC, box carbon Pg C, alkalinity mol/kg) triples in a box of `volume` m3;
 *   out[4*i..] = {pCO2 uatm, pH, Tr, status bits}.
 * hx_unit_doeclim_kernel: TemperatureComponent::prepareToRun's Ker[ns]
 *   (src/temperature_component.cpp:303-371) for one diffusivity (cm2/s). */
int hx_unit_csys(int device, int n, const double *Tc, const double *carbon, const double *alk,
                 double volume, double *out);
int hx_unit_doeclim_kernel(int device, double diff, int ns, double *out);

/* core metadata: startDate, endDate, current date, members, biomes */
int hx_dates(hx_core *core, int *start, int *end, int *current);
int hx_sizes(hx_core *core, int *n_members, int *n_biomes);

/* HIP-event time of the last run / spinup launch on the core's stream, ms */
int hx_last_run_ms(hx_core *core, double *ms);
int hx_last_spinup_ms(hx_core *core, double *ms);
/* the core's hipStream_t, as void* */
int hx_stream(hx_core *core, void **stream);
int hx_stream_shard(hx_core *core, int shard, void **stream);

/* Small ensembles -- too few 64-member wavefronts to occupy the GPU's 1 024 SIMDs, BASELINE
 * configs[1] -- are run by a kernel that gives every 64 members TWO wavefronts (ocean / climate and
 * land, hx_dev_pair.h): same model, same decisions, ~20 % shorter launch.  It serves
 * ensembles of one to four biomes without an NBP constraint, a land-ocean warming ratio, per-member series
 * (scenario-wide CO2 / tas / RF_tot / CH4 constraints -- concentration-driven runs -- are served,
 * with shared diffusivity) or diagnostics beyond CO2,
 * tas, RF_tot, RF_CO2, SST, land tas, timesteps, the carbon pools (atmos_co2, ocean_c, veg_c,
 * detritus_c, soil_c, permafrost_c, thawedp_c, earth_c), NBP, NPP, RH and its parts, f_frozen,
 * ocean_uptake, heatflux, gmst, HL_pH, LL_pH and the
 * CH4 / O3 concentrations (any scalar parameter may differ between members, diffusivity included);
 * everything else takes the one-wavefront kernels.
 * hx_set_pair_kernel_limit: ensembles of up to max_members use it (default 32 768 = one workgroup
 * per two SIMDs; 0 = never; the environment variable HECTOR_AMD_PAIR_MAX_MEMBERS sets the default of
 * new cores).  hx_last_run_kernel: "run" or "pair", whichever the last hx_run took. */
int hx_set_pair_kernel_limit(hx_core *core, int max_members);
/* Large ensembles -- more wavefronts of 64 members than the GPU has SIMDs (65 536 members on an
 * MI355X), e.g. BASELINE configs[3]'s 131 072 members per GPU -- are run by a flavour of the
 * one-biome kernel compiled for TWO resident wavefronts per SIMD (at most 256 registers and 20 KB
 * of LDS a wavefront; hx_dev_member.h, HX_B1W2): the second wavefront issues into the slots a
 * dependent fp64 chain of the first leaves empty.  Same model code, same decisions; it serves what
 * the one-biome kernels serve -- shared or per-member diffusivity, heat flux, and the extended kernel's
 * constraints, land-ocean warming ratio and diagnostics -- except carbon tracking.
 * hx_set_two_wave_from: ensembles of at least min_members members use it (< 0: the default, one
 * more wavefront than the device has SIMDs; 0: never; the environment variable
 * HECTOR_AMD_TWO_WAVE_FROM sets the default of new cores).  hx_last_run_kernel then says "run2".
 * With the default (< 0) an ensemble whose members differ in ocean heat diffusivity stays on the
 * one-wavefront kernel, which is the faster one for it (131 072 such members 13.5 against 14.3 ms). */
int hx_set_two_wave_from(hx_core *core, int min_members);
/* A run kernel launched after an idle gap -- the first run of a fresh core, behind 10-15 ms of
 * upload and spinup -- executes at ramping clocks (+6 % at 65 536 members, +11-15 % at 131 072:
 * profiles/r06_prewarm_curve.txt).  While hx_run's preparation uploads and spins up after such a
 * gap, a busy loop of three small wavefronts a SIMD keeps the chip's clocks up; hx_run stops it right
 * ahead of the run kernel, and it stops by itself after `ms` milliseconds of the device's own
 * clock (default 50; 0: off; HECTOR_AMD_PREWARM_MS sets the default of new cores).
 * hx_last_run_prewarmed: whether the last hx_run's kernel was launched behind it.  Results do
 * not depend on it.  No counterpart in the reference. */
int hx_set_prewarm(hx_core *core, int ms);
int hx_last_run_prewarmed(hx_core *core, int *yes);

/* Core::outputEnabled (src/core.cpp:257-262, 688-695): 0 if the scenario's section of that component
 * says output=0 -- the output stream visitor then leaves the component's rows out
 * (src/csv_outputstream_visitor.cpp, every visit()); hector-amd's stream does the same. */
int hx_component_output(hx_core *core, const char *component, int *enabled);
int hx_last_run_kernel(hx_core *core, const char **name);
/* Which family of run-kernel instantiations the last hx_run asked for: 0 the plain kernel;
 * -2 the plain kernel plus the diagnostics the reference's output stream writes (NPP, RH and its
 * parts, the ocean boxes' carbon / pCO2 / uptake, gmst ...: csv_outputstream_visitor.cpp:126-365)
 * when no constraint, land-ocean warming ratio or per-member series exists anywhere; -1 the
 * extended kernel (those too: temperature_component.cpp:510-525,586-625, forcing_component.cpp:
 * 498-505, ch4_component.cpp:156-157, simpleNbox-runtime.cpp:567-603); 1 the extended kernel with
 * the NBP constraint's machinery (simpleNbox-runtime.cpp:343-383); 2 carbon tracking. */
int hx_last_run_variant(hx_core *core, int *variant);
/* Where the last hx_run took the carbon-cycle solver's retries: *faithful = 1 inside the step loop,
 * as the reference does (carbon-cycle-solver.cpp:266-276), the steps a retry discards executed and
 * counted -- what a run that records "solver_steps" gets, or any run under
 * HECTOR_AMD_FAITHFUL_RETRIES=1; 0 at the head of the segment, before its first step (the default
 * otherwise; the results are the same bit for bit).  Under HECTOR_AMD_FAITHFUL_RETRIES=0 a run
 * that records "solver_steps" answers 0 too: that output then counts the executed steps, not the
 * reference's -- a test setting, and this is how to tell.  A run with an NBP constraint
 * always answers 1.  (The kernels that always take the retries inside the loop -- five and more
 * biomes, carbon tracking -- ignore the setting.) */
int hx_last_run_retries(hx_core *core, int *faithful);
/* When every wavefront of the last hx_run's year-loop launch started and ended: ticks[2 w] and
 * ticks[2 w + 1] for wavefront w of shard `shard` (64 members in lane order; the small-ensemble
 * kernel has two wavefronts per 64 members), in ticks of the device's constant 100 MHz clock
 * relative to the earliest start; *n_waves = wavefronts written (at most cap; 0 before a run).
 * The launch lasts as long as its last wavefront: this is the launch's tail, wavefront by
 * wavefront -- what bench.py reports as roofline.wave_time and what decides whether another lane
 * order or more resident wavefronts can shorten a launch.  No counterpart in the reference
 * (src/core.cpp:483-504 runs one member). */
int hx_wave_clock(hx_core *core, int shard, long long *ticks, int cap, int *n_waves);
/* ticks[w]: what wavefront w of shard `shard`'s last year-loop launch spent behind its year loop
 * reducing its own CO2_concentration and global_tas rows to per-wavefront partial statistics (what
 * hx_stats_device and hx_ensemble_stats fold instead of reading the rows again), same clock;
 * 0 for a wavefront that left it out.  *n_waves = 0 when the launch wrote no partials (any kernel
 * but the plain one-biome run kernel, or HECTOR_AMD_STATS_PARTIALS=0). */
int hx_wave_epilogue_clock(hx_core *core, int shard, long long *ticks, int cap, int *n_waves);

#define HX_ERR_MASS 1u     /* mass not conserved        simpleNbox-runtime.cpp:553-563 */
#define HX_ERR_RETRIES 2u  /* solver retries exhausted  carbon-cycle-solver.cpp:242-294 */
#define HX_ERR_NEGPOOL 4u  /* negative pool             fluxpool.hpp:100-102 */
#define HX_ERR_SPINUP 8u   /* did not spin up           core.cpp:394-420 */
#define HX_ERR_SINGULAR 16u /* DOECLIM matrix singular  temperature_component.cpp:84-86 */
#define HX_ERR_ROOT 32u    /* carbonate root not found  ocean_csys.cpp:134-156 */
#define HX_ERR_STEPFAIL 64u /* >500 rejected ODE steps  (odeint failed_step_checker), or more than
                             * 20 000 accepted ones in a year (step size collapsed) */
/* A member with a flag is not integrated any further -- the reference throws at that point. */

#ifdef __cplusplus
}
#endif
#endif
