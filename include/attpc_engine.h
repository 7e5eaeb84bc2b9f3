/*
 * attpc_engine.h -- C ABI of the MI355X-native AT-TPC Monte-Carlo hot path.
 *
 * The reference (ATTPC/attpc_engine, pure Python) has no FFI layer; its operator
 * boundary for the hot path is a set of Python call signatures.  Each entry point
 * below names the reference interface it replaces (paths relative to the
 * reference's src/attpc_engine/).  The Python package `attpc_engine_amd` binds
 * these symbols with ctypes (attpc_engine_amd/_abi.py) and re-exposes the
 * reference's own class/function names on top.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary; every call returns an int32
 *     status (ATTPC_OK == 0); attpc_last_error(ctx) gives a ctx-owned string.
 *   - the caller owns every host buffer; the library owns device memory, freed in
 *     attpc_ctx_destroy.  A ctx is single-threaded; distinct ctxs (one per GPU,
 *     one per process in the multi-GPU bench) are independent.
 *   - all floating point is IEEE binary64 ("f64"), charges are int64.
 *   - random numbers: Philox4x32-10, key = seed, counter = (global event id, draw index, domain); the
 *     time-bucket jitter of a cloud point is Philox2x32-7 with counter = (event[31:0],
 *     event[39:32] << 24 | tb << 14 | pad) and key word = seed[31:0] ^ rotl(seed[63:32], 13) ^ 0x100
 *     -- every draw a pure function of (seed, global event id, ...): results do not depend on
 *     batch / chunk / GPU count.
 *   - seeds are any u64.  A call's event ids first_event .. first_event + n_events - 1 must all lie in
 *     [0, 2^64): a range that would wrap past 2^64 is ATTPC_E_INVALID (attpc_kin_run, attpc_det_run,
 *     attpc_sim_run, their _spyral, _traces, _trace_rows and _summary forms, attpc_det_tracks, attpc_det_scatter,
 *     attpc_sim_hint_next, attpc_traces_at, attpc_trace_rows_at, and the _traces_packed forms).
 *     Ids 2^40 apart share their jitter streams (the jitter counter holds event[39:0]) and nothing else.
 */
#ifndef ATTPC_ENGINE_H
#define ATTPC_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ATTPC_ABI_VERSION 3
#define ATTPC_API __attribute__((visibility("default")))

/* status codes */
#define ATTPC_OK 0
#define ATTPC_E_INVALID 1       /* bad argument / descriptor                                */
#define ATTPC_E_NODEVICE 2      /* no HIP device                                            */
#define ATTPC_E_HIP 3           /* a HIP runtime call failed (see attpc_last_error)         */
#define ATTPC_E_CAPACITY 4      /* caller buffer too small; required size in stats          */
#define ATTPC_E_NOTCONFIGURED 5 /* run called before the matching configure                 */
#define ATTPC_E_DATALOSS 6      /* the run finished but stats.n_failed or stats.n_inconsistent is
                                   not 0: part of an event's charge is missing from the cloud     */

#define ATTPC_MAX_STEPS 8    /* 1 Reaction + up to 7 Decays                                 */
#define ATTPC_MAX_ROWS (4 + 2 * (ATTPC_MAX_STEPS - 1)) /* nuclei (rows) per event           */
#define ATTPC_MAX_SPECIES 16
#define ATTPC_MAX_SIM 8      /* max simulated nuclei per event (len(indices))               */

/* stopping-power table: nodes on a "binade" grid, E = 2^e (1 + m/32) MeV,
 * e in [ATTPC_DEDX_EMIN, ATTPC_DEDX_EMAX), m in [0,32); one extra closing node. */
#define ATTPC_DEDX_EMIN (-30)
#define ATTPC_DEDX_EMAX 14
#define ATTPC_DEDX_SUB 32
#define ATTPC_DEDX_NODES ((ATTPC_DEDX_EMAX - ATTPC_DEDX_EMIN) * ATTPC_DEDX_SUB + 1)

#define ATTPC_NUM_TB 512        /* detector/constants.py:23                                 */
#define ATTPC_TIME_SAMPLES 10001 /* detector/solver.py:16  TIME_STEPS                       */
#define ATTPC_MESH_STEPS 10     /* detector/transporter.py:8  STEPS                         */
#define ATTPC_LONG_STEPS 5      /* time slices of the longitudinal-diffusion extension       */

/* excitation sampler kinds -- kinematics/excitation.py */
#define ATTPC_EX_GAUSSIAN 0 /* p0 = centroid, p1 = sigma (= FWHM/2.355)         :32-80      */
#define ATTPC_EX_UNIFORM 1  /* p0 = min, p1 = max                               :83-128     */
#define ATTPC_EX_TABLE 2    /* inverse-CDF table: x[table_len], cdf[table_len]; value=x-p0.
                               ExcitationBreitWigner (:131-188) is configured this way
                               (x = total energy, p0 = rest mass).                          */
/* polar sampler kinds -- kinematics/angle.py */
#define ATTPC_POLAR_UNIFORM 0   /* uniform in cos(theta) in [cos_min, cos_max]  :35-80      */
#define ATTPC_POLAR_ARBITRARY 1 /* choice(angles, p) + U*bin_width              :83-152     */

typedef struct attpc_excitation_desc {
  int32_t kind;
  int32_t table_len;
  double p0, p1, p2;
  const double* table_x;   /* [table_len] (ATTPC_EX_TABLE) */
  const double* table_cdf; /* [table_len], nondecreasing, last == 1 */
} attpc_excitation_desc;

typedef struct attpc_polar_desc {
  int32_t kind;
  int32_t table_len;
  double cos_min, cos_max;
  double bin_width;
  const double* angles; /* [table_len] lower bin edges, radians */
  const double* cdf;    /* [table_len] cumulative probabilities (numpy choice semantics) */
} attpc_polar_desc;

/* replaces KinematicsPipeline.__init__ state, kinematics/pipeline.py:125-185 */
typedef struct attpc_kin_desc {
  int32_t n_steps;      /* 1 + number of decays */
  int32_t sample_limit; /* event_sample_limit, pipeline.py:132 */
  double beam_energy;   /* MeV */
  /* nuclear masses (MeV) in result-row order: target, projectile, ejectile, residual,
     then (residual_1, residual_2) per decay -- pipeline.py:398-406 */
  double masses[ATTPC_MAX_ROWS];
  attpc_excitation_desc excitation[ATTPC_MAX_STEPS];
  attpc_polar_desc polar[ATTPC_MAX_STEPS];
  /* KinematicsTargetMaterial, pipeline.py:16-36 / :245-264 */
  int32_t has_target;
  int32_t eloss_len;   /* nodes of the beam energy-loss table */
  double rho_sigma;    /* m */
  double z_min, z_max; /* m */
  const double* eloss; /* [eloss_len] energy loss (MeV) of the projectile at beam_energy after
                          path z_min + i (z_max - z_min)/(eloss_len - 1) */
} attpc_kin_desc;

typedef struct attpc_species_desc {
  int32_t Z;
  int32_t A;
  double mass;        /* ground-state nuclear mass, MeV (solver.py:273) */
  const double* dedx; /* [ATTPC_DEDX_NODES] MeV/(g/cm^2) on the binade grid */
} attpc_species_desc;

/* replaces Config / DetectorParams / ElectronicsParams, detector/parameters.py:10-174 */
typedef struct attpc_det_desc {
  double length;   /* m */
  double efield;   /* V/m */
  double bfield;   /* T */
  double density;  /* g/cm^3, target.density (solver.py:65) */
  double diffusion;   /* V */
  double fano_factor;
  double w_value;  /* eV */
  int64_t mpgd_gain;
  int32_t micromegas_edge; /* time buckets */
  int32_t windows_edge;
  /* pad look-up at whole-millimetre pitch (transporter.py:78-120 floors to mm first).
     pad_lut[ix * lut_n + iy] for floor(x_mm) = lut_lo + ix; -1 = no pad.  Beam pads
     (detector/beam_pads.py) must already be folded to -1 by the caller. */
  const int16_t* pad_lut;
  int32_t lut_n;
  int32_t lut_lo;
  int32_t n_species;
  int32_t ode_substeps; /* RK4 sub-steps per 1e-10 s output sample; 0 -> default (1) */
  attpc_species_desc species[ATTPC_MAX_SPECIES];
  /* EXTENSION (not in the reference, which has no longitudinal diffusion -- docs/user_guide/
     detector/index.md:130-133): > 0 spreads every sample over ATTPC_LONG_STEPS time slices,
     linspace(t - 3 sigma_l, t + 3 sigma_l), sigma_l = sqrt(2 D_l dv t / E) / dv time buckets,
     slice s carrying the fraction long_weights[s] (1-D Gaussian pdf x slice pitch) of each
     pixel: electrons = int(pdf h^2 * (long_weights[s] * n)).  0 = reference behaviour. */
  double longitudinal_diffusion; /* V */
  double long_weights[5];
  /* EXTENSION (north star: "stochastic per-electron diffusion instead of the deterministic 10x10
     mesh"): != 0 moves every primary electron k of an entry (sample x slice) by its own Gaussian
     step, x = x0 + sigma_t N_x, y = y0 + sigma_t N_y (Box-Muller on the Philox pair with index k in
     domain 0x200 + entry number), and adds int(w_slice * gain) electrons to the pad it lands on.
     0 = the reference's mesh. */
  int32_t mc_diffusion;
  int32_t reserved_ext;
  /* EXTENSION (BASELINE configs[4] "0.1 mm dE/dx step"; the reference grid is fixed in time,
     detector/solver.py:16,285-303): > 0 records a track sample -- and creates its electrons from the
     energy lost since the previous sample, solver.py:338-346 -- every `path_step` metres of arc length:
     sample k+1 follows sample k after the time min(path_step / v_k, 1e-10 s) (v_k = speed at sample k;
     never coarser than the reference grid, so the end of the range is integrated as in the default
     mode), each interval integrated with ode_substeps RK4 steps; recording ends with the reference's
     1 us window or after ATTPC_TIME_SAMPLES samples.  0 = the reference's 1e-10 s grid. */
  double path_step; /* m */
} attpc_det_desc;

/* which rows of an event are simulated, detector/simulator.py:96-101,157-158 */
typedef struct attpc_event_layout {
  int32_t n_rows;                          /* nuclei per event (rows of the kinematics result) */
  int32_t n_sim;                           /* len(indices) */
  int32_t indices[ATTPC_MAX_SIM];          /* rows to simulate, in order */
  int32_t species_of_row[ATTPC_MAX_ROWS];  /* index into det_desc.species, -1 => skip (Z == 0) */
} attpc_event_layout;

/* Host output buffers for a run (any pointer may be NULL => that output stays on the device). */
typedef struct attpc_cloud_out {
  int64_t capacity;   /* rows available in points/labels */
  int64_t* offsets;   /* [n_events + 1] CSR offsets into points/labels */
  double* points;     /* [capacity, 3] rows (pad, time bucket, electrons) -- simulator.py:40-46 */
  int64_t* labels;    /* [capacity] row index of the nucleus that last touched the point */
  int64_t* event_points; /* [n_events] or NULL: cloud rows of every event BEFORE any threshold
                            (simulator.py:204-205 decides "empty event" on this count) */
} attpc_cloud_out;

typedef struct attpc_run_stats {
  uint64_t n_events;
  uint64_t n_points;          /* cloud rows produced */
  uint64_t n_track_samples;   /* track samples with >= 1 electron (scatter work items) */
  uint64_t n_sample_limit;    /* events that hit event_sample_limit */
  uint64_t n_lds_overflow;    /* windows redone with a smaller time-bucket range (LDS table too full) */
  uint64_t n_failed;          /* events that lost a time bucket (more than 65 536 lone buckets in one launch);
                                 must be 0 -- the run then returns ATTPC_E_DATALOSS */
  uint64_t charge_checksum;   /* sum of all charges mod 2^64 */
  uint64_t key_checksum;      /* sum over points of (event*2^24 + tb*2^14 + pad) mod 2^64 */
  double ms_kinematics;       /* device time of each kernel family (HIP events on the ctx stream) */
  double ms_tracks;
  double ms_scatter;
  uint32_t launches_kinematics;
  uint32_t launches_tracks;
  uint32_t launches_scatter;
  uint32_t n_inconsistent;    /* self-check: flushed windows whose occupied-slot count differed from the
                                 number of claimed keys; must be 0 */
  uint64_t n_lone_buckets;    /* time buckets that alone exceeded the LDS table and went through the
                                 direct-mapped table of lone_bucket_kernel (complete, just slower) */
  uint64_t n_buffer_growths;  /* device buffers (re)allocated during this run; 0 once the sizes have settled */
  uint64_t n_tracks_capped;   /* path-length dE/dx step only: tracks that reached ATTPC_TIME_SAMPLES samples before the
                                 end of the 1 us recording window and were cut there (about 1 m of arc length at a
                                 0.1 mm step); always 0 on the reference's time grid, whose 10 001st sample IS 1 us */
  uint64_t device_bytes;      /* device memory the context holds at the end of the run (buffers it allocated) */
} attpc_run_stats;

typedef struct attpc_ctx attpc_ctx;

ATTPC_API int32_t attpc_version(void);
ATTPC_API int32_t attpc_device_count(void);
/* device >= 0: that HIP device.  There is no CPU fallback: without a device -> ATTPC_E_NODEVICE. */
ATTPC_API int32_t attpc_ctx_create(int32_t device, attpc_ctx** out);
ATTPC_API int32_t attpc_ctx_destroy(attpc_ctx* ctx);
ATTPC_API const char* attpc_last_error(const attpc_ctx* ctx);
/* events processed per internal chunk (device working set scales with it); 0 -> default */
ATTPC_API int32_t attpc_set_chunk_events(attpc_ctx* ctx, int32_t chunk_events);
ATTPC_API int32_t attpc_sync(attpc_ctx* ctx);
/* Tuning / test switches of a context (no environment variables are read by the library):
 *   "scatter_variant"  0 = automatic, 1 = always the two-workgroups-per-CU build, 2 = always the
 *                      one-workgroup build of the scatter kernel, 3 = always the build with u64 sums per table
 *                      slot (the automatic choice switches to it when u32 sums -- 4.3e9 electrons per pad and
 *                      time bucket -- turn out too small for the detector at hand)
 *   "tiny_buffers"     != 0: the next buffers are allocated far too small (exercises the
 *                      grow-and-rerun path in tests)
 *   "compact_transfer" 2 (default): delivered clouds cross PCIe as 8-byte records (attpc_unpack_rows8: the host
 *                      regenerates the time-bucket jitter), 1: as 16-byte records (attpc_unpack_rows), into
 *                      library-owned pinned staging, and are expanded into the caller's arrays by host threads; a chunk
 *                      with a row that does not fit the record falls back to the next wider form;
 *                      0: rows are copied in the reference's dtypes (32 bytes) straight into the caller's arrays.
 *                      Spyral rows: != 0 = 24-byte records (attpc_unpack_spyral_rows)
 *   "unpack_threads"   host threads of that expansion; 0 (default) = min(32, the CPUs the process may use: affinity
 *                      mask and control-group quota honoured, half of them on a machine with 64 or more)
 *   "deliver_chunk_events"  events per chunk when clouds are delivered (default 8192: a chunk's copy hides the next
 *                      chunk's scatter and assembly; the first chunk's device work and the last chunk's expansion
 *                      stand alone, so smaller chunks shorten a short call)
 *   "serial_tracks"    1: kinematics + track integration of the next batch run on the scatter stream, behind the
 *                      current batch's scatter launches; 0: beside them on a low-priority stream; -1 (default):
 *                      behind on the reference's time grid (beside is 3 % slower there: both kernels are issue
 *                      bound), beside with the path-length dE/dx step (12 % faster there)
 *   "track_species_major"  1 (default): the track kernel takes its tracks nucleus by nucleus, lightest species first
 *                      (its lanes then run dry on the short tracks of the heavy ions); 0: event by event.  Scheduling
 *                      only: results do not depend on it
 *   "first_batch_chunks"  > 0: the first track batch of a call spans at most this many scatter chunks (experiment)
 *   "scatter_merge"    -1 (default) = automatic, 0 = never, 1 = always use the scatter kernel's merge variant, which adds
 *                      up the pixel charges of consecutive track samples that fall on the same pad in the same time
 *                      bucket before the table sees them (same results; automatic = with the path-length dE/dx step,
 *                      attpc_det_desc.path_step > 0, where samples are far closer than a pad)
 *   "trace_pack_workgroups"  workgroups (of four waves, one row a wave) the trace pack kernels are launched with at
 *                      most; 0 (default) = 8 per compute unit.  Scheduling only: results do not depend on it
 *   "track_workgroups"  0..65536, workgroups (of four waves) the track kernel is launched with at most; 0 (default) =
 *                      as many as the tracks need, up to "track_blocks_per_cu" per compute unit.  A test hook: with one
 *                      workgroup a few hundred tracks make every lane take several tracks, and every wave several
 *                      batches of track ids and pools of arena blocks.  Scheduling only: results do not depend on it
 *   "chunk_events"     as attpc_set_chunk_events
 *   "reaction_spectra_only"  != 0: a trace-row call in which the reaction reconstruction runs ("reaction
 *                      reconstruction" below) copies none of its stages' records to the host -- estimates, fits, pid,
 *                      reaction, clusters, joins stay in the chunk buffers, no pinned room is made for them, and the
 *                      attpc_*_last readers of those records answer ATTPC_E_NOTCONFIGURED for that call -- so that only
 *                      the spectra (attpc_reaction_spectra_last) cross the link, whatever the number of events.  The
 *                      spectra do not depend on it.  A call without the reaction reconstruction ignores it.  Default 0 */
ATTPC_API int32_t attpc_set_option(attpc_ctx* ctx, const char* name, int64_t value);
/* Page-locked host memory for output buffers (point clouds are PCIe bound on their way to the host:
 * copies into pinned memory run at the link rate, copies into pageable memory at a fraction of it).
 * Plain memory otherwise: the caller reads/writes it freely and returns it with attpc_host_free. */
ATTPC_API int32_t attpc_host_alloc(attpc_ctx* ctx, uint64_t bytes, void** out);
ATTPC_API int32_t attpc_host_free(attpc_ctx* ctx, void* ptr);
/* The 16-byte transfer record of a cloud row and its expansion (host only, no device, no context):
 *   bytes 0..7   f64  time bucket + jitter (column 1 of the row, as it is)
 *   bytes 8..15  u64  electrons (bits 0..44) | pad << 45 (14 bits) | label << 59 (5 bits)
 * -> points[r] = (pad, time bucket, electrons) as f64, labels[r] as i64 (detector/simulator.py:40-46). */
ATTPC_API int32_t attpc_unpack_rows(const void* packed, int64_t n_rows, double* points, int64_t* labels, int32_t n_threads);
/* The 8-byte transfer record of a cloud row ("compact_transfer" 2, the default) and its expansion, host only.  The
 * jitter of a cloud point is a pure function of (seed, global event id, time bucket, pad) -- Philox2x32-7, see the
 * conventions at the top -- so it does not cross the link: the host regenerates it.
 *   u64  electrons (bits 0..35) | time bucket << 36 (9 bits) | pad << 45 (14 bits) | label << 59 (5 bits)
 * packed [n_rows] holds the rows of events first_event .. first_event + n_events - 1 in event order, offsets
 * [n_events + 1] their CSR offsets (offsets[n_events] - offsets[0] == n_rows)
 * -> points[r] = (pad, time bucket + jitter, electrons) as f64, labels[r] as i64: bit-identical to the rows the device
 * writes (detector/simulator.py:40-46, :108). */
ATTPC_API int32_t attpc_unpack_rows8(const void* packed, int64_t n_rows, const int64_t* offsets, int64_t n_events,
                                     uint64_t seed, uint64_t first_event, double* points, int64_t* labels, int32_t n_threads);
/* The 24-byte transfer record of a Spyral row (attpc_sim_run_spyral with "compact_transfer") and its expansion
 * to the 8 columns of convert_to_spyral (detector/writer.py:61-112), host only:
 *   bytes 0..7 f64 time bucket + jitter, 8..15 u64 electrons | pad << 45 | label << 59, 16..23 f64 clipped integral
 * -> x, y = pad_centers[pad], z = (windows_edge - tb) / (windows_edge - micromegas_edge) * length * 1000,
 *    amplitude = min(r_max * electrons, 4095) with r_max the largest response sample, integral, pad, tb,
 *    pad_sizes[pad]; labels[r] as i64. */
ATTPC_API int32_t attpc_unpack_spyral_rows(const void* packed, int64_t n_rows, const double* pad_centers,
                                           const double* pad_sizes, int32_t n_pads, double r_max, int32_t windows_edge,
                                           int32_t micromegas_edge, double length, double* rows, int64_t* labels,
                                           int32_t n_threads);

/* KinematicsPipeline(...) state -> device.  kinematics/pipeline.py:125-185 */
ATTPC_API int32_t attpc_kin_configure(attpc_ctx* ctx, const attpc_kin_desc* desc);
/* n x KinematicsPipeline.run(), kinematics/pipeline.py:285-388 (sample :232-283,
 * Reaction/Decay.calculate reaction.py:103-178,252-303).
 * p4 [n, n_rows, 4] (px,py,pz,E MeV), vertex [n,3] m, status [n] (0 ok, 1 sample limit),
 * attempts [n]; each may be NULL. */
ATTPC_API int32_t attpc_kin_run(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                      double* p4, double* vertex, int32_t* status, uint32_t* attempts);

/* Deterministic map "sampled parameters -> 4-vectors" for n parameter sets, using the
 * configured masses / n_steps: Reaction.calculate + is_excitation_allowed
 * (kinematics/reaction.py:70-178) followed by Decay.* (:230-303) per decay.
 * beam_energy [n]; ex, polar, azim [n, n_steps]; p4 [n, n_rows, 4];
 * status [n]: 0 ok, k+1 = step k not energetically allowed (rows from step k on are NaN),
 * -1 = reaction allowed but below the non-relativistic threshold formula of
 * Reaction.calculate (reaction.py:136-143, where the reference raises ValueError),
 * -2 = both not allowed and below that threshold. */
ATTPC_API int32_t attpc_kin_calculate(attpc_ctx* ctx, uint64_t n, const double* beam_energy,
                            const double* ex, const double* polar, const double* azim,
                            double* p4, int32_t* status);

/* Decay.is_excitation_allowed + Decay.calculate for explicit parent 4-vectors
 * (kinematics/reaction.py:230-303): parent [n,4]; ex, polar, azim [n];
 * out [n,2,4] = residual_1, residual_2; status [n]: 0 ok, 1 not allowed (rows NaN). */
ATTPC_API int32_t attpc_decay_calculate(attpc_ctx* ctx, uint64_t n, const double* parent, double mass_1,
                              double mass_2, const double* ex, const double* polar,
                              const double* azim, double* out, int32_t* status);

/* Config(...) + nuclei table -> device.  detector/parameters.py:145-174 */
ATTPC_API int32_t attpc_det_configure(attpc_ctx* ctx, const attpc_det_desc* desc);
/* n x simulate(), detector/simulator.py:52-115 (generate_point_cloud solver.py:350-413,
 * transport_track transporter.py:252-317, dict_to_points simulator.py:19-49).
 * p4/vertex are host arrays as produced by attpc_kin_run (or read from a kinematics file). */
ATTPC_API int32_t attpc_det_run(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                      const attpc_event_layout* layout, const double* p4, const double* vertex,
                      attpc_cloud_out* out, attpc_run_stats* stats);

/* Fused kinematics + detector: run_kinematics_pipeline + run_simulation without the
 * file in between (kinematics/pipeline.py:429-495, detector/simulator.py:118-210);
 * kinematics never leaves HBM.  out == NULL keeps the clouds device-resident
 * (chunk buffers are overwritten; stats carry counts and checksums). */
ATTPC_API int32_t attpc_sim_run(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                      const attpc_event_layout* layout, double* p4, double* vertex,
                      int32_t* kin_status, attpc_cloud_out* out, attpc_run_stats* stats);

/* Announces the attpc_sim_run / attpc_sim_run_spyral call AFTER the next one: "when the run I am about to start has
 * queued its last track batch, go on with the kinematics + tracks of events first_event .. of this seed".  The next
 * run then queues that first batch (up to 8 scatter chunks) on its low-priority stream behind its own last scatter
 * launches, and the call that was announced finds it under way instead of starting with track integration that has
 * nothing to run beside (about 5 % of a 1e6-event call of the headline workload).  Purely a scheduling hint: a call
 * for other events, another entry point or a configure call lets the batch finish and drops it; results never depend
 * on it.  n_events == 0 or layout == NULL withdraws the announcement.  The reference has no counterpart (its loop is
 * one event at a time, detector/simulator.py:183-208). */
ATTPC_API int32_t attpc_sim_hint_next(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                      const attpc_event_layout* layout);

/* Diagnostics used by the parity tests: one track per (event, simulated nucleus) of a
 * det_run-style input.  samples [n_tracks, ATTPC_TIME_SAMPLES, 4] rows (x m, y m,
 * time bucket, electrons*gain) of the samples with >= 1 electron; counts [n_tracks];
 * n_steps [n_tracks] = number of recorded ODE samples (rows of the reference's track).  A track whose count or
 * arena block lies outside the track buffers (a track the kernel never ran) is ATTPC_E_DATALOSS, not a copy. */
ATTPC_API int32_t attpc_det_tracks(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                         const attpc_event_layout* layout, const double* p4,
                         const double* vertex, int64_t max_samples_per_track, double* samples,
                         int32_t* counts, int32_t* n_steps);

/* Diagnostics used by the parity tests: the pad-plane scatter alone -- transport_track
 * (detector/transporter.py:252-317: transverse_transport :172-249, point_transport :123-169,
 * position_to_index :78-120) per simulated nucleus into the event's shared dictionary, then
 * dict_to_points + jitter + 0 <= tb < 512 mask (detector/simulator.py:19-49, :93-113) -- for EXPLICIT
 * track samples, so that reference-generated transport fixtures reach the HIP kernel directly.
 * samples [sum(counts), 4] rows (x m, y m, time bucket, electrons already multiplied by the gain),
 * concatenated track by track, track = event * n_sim + position in layout->indices;
 * counts [n_events * n_sim] (each <= 10112).  layout->species_of_row is ignored. */
ATTPC_API int32_t attpc_det_scatter(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                          const attpc_event_layout* layout, const double* samples, const int32_t* counts,
                          attpc_cloud_out* out, attpc_run_stats* stats);

/* GET response + Spyral row conversion, detector/response.py:8-57, detector/writer.py:61-112:
 * rows [n,8] = x_mm, y_mm, z_mm, amplitude, integral, pad, tb, pad_scale. */
ATTPC_API int32_t attpc_spyral_rows(attpc_ctx* ctx, int64_t n_points, const double* points,
                          const double* response /*[512]*/, const double* pad_centers /*[npads,2]*/,
                          const double* pad_sizes /*[npads]*/, int32_t n_pads, int32_t windows_edge,
                          int32_t micromegas_edge, double length, double* rows);

/* Electronics / geometry the Spyral conversion needs: get_response(config) (detector/response.py:8-32),
 * Config.pad_centers / pad_sizes (detector/parameters.py:207-261), adc_threshold, time-bucket edges. */
typedef struct attpc_spyral_desc {
  const double* response;    /* [ATTPC_NUM_TB] ADC counts per electron and time bucket */
  const double* pad_centers; /* [n_pads, 2] mm */
  const double* pad_sizes;   /* [n_pads] */
  int32_t n_pads;
  int32_t windows_edge;
  int32_t micromegas_edge;
  int32_t reserved;
  double length;             /* m */
  double adc_threshold;      /* rows with amplitude <= threshold are dropped (writer.py:232-234) */
} attpc_spyral_desc;

ATTPC_API int32_t attpc_spyral_configure(attpc_ctx* ctx, const attpc_spyral_desc* desc);

/* attpc_sim_run followed, on the device and before anything crosses PCIe, by what SpyralWriter.write
 * does per event (detector/writer.py:194-238): convert_to_spyral (rows of 8: x_mm, y_mm, z_mm,
 * amplitude, integral, pad, tb, pad_scale), the ADC-threshold cut (:232-234) and the sort by z
 * (:236-238).  out->points receives rows of EIGHT doubles here (capacity counts rows), the rows of
 * every event in ascending z, ready for the writer. */
ATTPC_API int32_t attpc_sim_run_spyral(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                       const attpc_event_layout* layout, double* p4, double* vertex,
                                       int32_t* kin_status, attpc_cloud_out* out, attpc_run_stats* stats);

/* attpc_det_run followed, on the device, by the same per-event work of SpyralWriter.write as in
 * attpc_sim_run_spyral: the file-driven flow run_simulation(config, kinematics file, SpyralWriter)
 * (detector/simulator.py:183-208 -> detector/writer.py:194-255) with kinematics read from a file (host arrays
 * p4 [n, n_rows, 4], vertex [n, 3]) instead of generated on the device.  out->points receives rows of EIGHT doubles,
 * every event's rows thresholded and in ascending z; out->event_points the cloud rows of every event before the
 * threshold (simulator.py:204-205 decides "empty event" on those). */
ATTPC_API int32_t attpc_det_run_spyral(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                       const attpc_event_layout* layout, const double* p4, const double* vertex,
                                       attpc_cloud_out* out, attpc_run_stats* stats);

/* ---- digitised GET pad traces (EXTENSION: the reference stops at point clouds, docs/user_guide/detector/index.md
 * "Why Point clouds") ----
 * The contract, for one event's cloud rows (pad p, jittered time bucket tau, electrons q, label l) as attpc_sim_run
 * produces them, a response R[512] (default get_response(config), detector/response.py:8-32), an ADC threshold thr and
 * an integer offset >= 0:
 *   - t = floor(tau): the GET digitises whole buckets, the jitter plays no part.  Rows of one event have distinct (pad, t).
 *   - for every pad p hit in the event and j in 0..511
 *       A_p[j] = sum over the rows r of pad p with 0 <= j + offset - t_r < 512, in ascending t_r, of q_r * R[j + offset - t_r]
 *     in f64 from +0.0, every product rounded and then added (no fused multiply-add); R is indexed by sample number,
 *     as the reference's apply_response indexes its linspace(0, 512, 512) array.
 *   - trace_p[j] = (int16) rint(min(A_p[j], 4095.0)), rint rounding half to even: the SUMMED signal saturates (pile-up on
 *     one pad saturates as the electronics would; unlike the Spyral row's per-point clip, response.py:35-57).
 *   - a pad row is kept iff max_j trace_p[j] > thr (strict, as writer.py:232); thr < 0 keeps every hit pad, all-zero
 *     traces included.
 *   - a kept row carries pad (i32), samples[512] (i16) and label (i64): the label of the pad's row with the largest q, the
 *     smallest t on a tie.  Rows of an event come out in ascending pad, events in id order with CSR offsets.
 *   - offset = 0 is the causal response (response sample k lands at bucket t + k); offset = argmax(R) puts the peak on the
 *     arrival bucket.
 * attpc_run_stats keeps its cloud meaning in every trace entry point (the counts and checksums attpc_sim_run reports for
 * the same ids).  The id-range rules at the top apply; a pending attpc_sim_hint_next is dropped. */
#define ATTPC_NUM_PADS 10240

typedef struct attpc_trace_desc {
  const double* response; /* [ATTPC_NUM_TB] ADC counts per electron by sample number */
  double adc_threshold;   /* rows with max sample <= threshold are dropped; < 0 keeps every hit pad */
  int32_t offset;         /* >= 0; sample j reads R[j + offset - t] */
  int32_t reserved;
} attpc_trace_desc;

ATTPC_API int32_t attpc_trace_configure(attpc_ctx* ctx, const attpc_trace_desc* desc);

/* Host output buffers of a trace run; any array may be NULL (that output then stays on the device). */
typedef struct attpc_trace_out {
  int64_t capacity;        /* rows available in pads / samples / labels */
  int64_t* offsets;        /* [n_events + 1] CSR offsets of the kept rows */
  int32_t* pads;           /* [capacity] */
  int16_t* samples;        /* [capacity, ATTPC_NUM_TB] */
  int64_t* labels;         /* [capacity] */
  int64_t* event_points;   /* [n_events]: cloud rows of every event before the suppression (simulator.py:204-205) */
  int64_t n_rows;          /* written: kept rows of the call (the capacity needed on ATTPC_E_CAPACITY) */
  uint64_t sample_checksum; /* written: sum over rows, j of trace[j] * (j + 1) mod 2^64 */
  uint64_t pad_checksum;   /* written: sum over rows of (event * 2^14 + pad) mod 2^64; event = the global event id
                              (attpc_traces: the index of the event in the call) */
} attpc_trace_out;

/* attpc_sim_run, then the traces of every event on the device before anything crosses PCIe. */
ATTPC_API int32_t attpc_sim_run_traces(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                       const attpc_event_layout* layout, double* p4, double* vertex,
                                       int32_t* kin_status, attpc_trace_out* out, attpc_run_stats* stats);
/* attpc_det_run (kinematics from host p4 [n, n_rows, 4] / vertex [n, 3], the file-driven flow), then the traces. */
ATTPC_API int32_t attpc_det_run_traces(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                       const attpc_event_layout* layout, const double* p4, const double* vertex,
                                       attpc_trace_out* out, attpc_run_stats* stats);
/* Traces of any host cloud: offsets [n_events + 1] (nondecreasing), points [rows, 3] (pad, tau, electrons), labels
 * [rows].  Every row needs an integer pad in [0, ATTPC_NUM_PADS), 0 <= tau < 512, finite electrons >= 0 and a (pad, t)
 * of its own within the event, else ATTPC_E_INVALID.  = attpc_traces_at(ctx, 0, 0, ...). */
ATTPC_API int32_t attpc_traces(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* points,
                               const int64_t* labels, attpc_trace_out* out);

/* ---- electronic noise and per-pad pedestals of the traces (opt-in; off, every trace output is the contract above) ----
 * Notation: s_p[j] = rint(min(A_p[j], 4095)), the noiseless sample above (an integer in [0, 4095]); e the global event
 * id; seed the run's 64-bit seed.
 *   - noise table: n_levels in 0..ATTPC_MAX_NOISE_LEVELS, an integer min_level with |min_level| <= 4095 and
 *     cdf[n_levels - 1], non-decreasing u32.  n_levels = 0 is no noise (n = 0).
 *   - draw of sample j of pad p:
 *       out = Philox4x32-10(counter = (e[31:0], e[63:32], p * 128 + 2 * (j mod 64) + (j div 256), 0x80000000 | stream),
 *                           key = (seed[31:0], seed[63:32])),   u = out[(j div 64) mod 4]
 *     (the lane holding samples j = lane + 64 s needs two Philox calls per pad).  The domain 0x80000000 | stream is
 *     disjoint from every other draw's (0, 1 + row, 0x200 + entry, and the jitter's own generator); stream < 2^31
 *     draws another noise realisation on the same physics.
 *   - noise value n_p[j] = min_level + #{k : cdf[k] <= u}  (numpy.searchsorted(cdf, u, side="right")).
 *   - sample trace_p[j] = min(max(s_p[j] + ped_p + n_p[j], 0), 4095); ped_p the pad's pedestal, an int16 in [0, 4095],
 *     0 without a pedestal array.  Everything after s_p is integer arithmetic.
 *   - a pad row is kept iff max_j (trace_p[j] - ped_p) > thr (strict; thr < 0 keeps every hit pad).
 *   - unchanged: only pads with at least one cloud row get a trace (noise-only pads are read out only in the readout modes
 *     of attpc_trace_configure_readout below), the label rule,
 *     row and event order, the CSR offsets, and the definitions of sample_checksum and pad_checksum (taken over the
 *     noisy samples).
 * With n_levels = 0 and no pedestals the result is the noiseless contract exactly (s_p[j] is already in [0, 4095]).
 * attpc_sim_run_traces and attpc_det_run_traces key the noise on the run's seed and the global event ids. */
#define ATTPC_MAX_NOISE_LEVELS 512

typedef struct attpc_trace_noise_desc {
  const uint32_t* cdf;       /* [n_levels - 1] */
  int32_t n_levels;
  int32_t min_level;
  const int16_t* pedestals;  /* [ATTPC_NUM_PADS], NULL = zeros */
  uint32_t stream;
  int32_t reserved;
} attpc_trace_noise_desc;

/* desc == NULL turns noise and pedestals off.  Independent of attpc_trace_configure: neither call resets the other.
 * ATTPC_E_INVALID for a decreasing cdf, more than ATTPC_MAX_NOISE_LEVELS levels, |min_level| > 4095, a pedestal
 * outside [0, 4095] or stream >= 2^31. */
ATTPC_API int32_t attpc_trace_configure_noise(attpc_ctx* ctx, const attpc_trace_noise_desc* desc);
/* attpc_traces with the noise keyed on (seed, first_event + i) for the i-th event of the call; the pad checksum counts
 * events from first_event.  The id-range rules at the top apply. */
ATTPC_API int32_t attpc_traces_at(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, int64_t n_events,
                                  const int64_t* offsets, const double* points, const int64_t* labels,
                                  attpc_trace_out* out);

/* ---- readout of noise-only pads: partial (zero-suppressed) and full readout of the GET electronics (opt-in; the
 * default ATTPC_READOUT_HIT is every trace contract above exactly) ----
 * A readout mode and a readout set S, a subset of 0 .. ATTPC_NUM_PADS - 1: the pads that have an electronics channel.
 * Notation as in the noise contract (s_p, ped_p, n_p, thr); without noise n_p = 0 and ped_p = 0.
 *   - ATTPC_READOUT_HIT: the contracts above; S is ignored.
 *   - ATTPC_READOUT_PARTIAL: every pad of S is a candidate in every event.  A pad of S with cloud rows keeps its s_p; a
 *     pad of S without rows is noise-only, s_p[j] = 0.  Both get trace_p[j] = min(max(s_p[j] + ped_p + n_p[j], 0), 4095)
 *     with the same (seed, e, p, j) draw, and a pad is kept iff max_j (trace_p[j] - ped_p) > thr (strict, as above).
 *     Cloud rows on pads outside S are dropped (a dead channel).
 *   - ATTPC_READOUT_FULL: every pad of S is kept; every event has exactly |S| rows.  The traces are those of PARTIAL.
 *   - both: noise-only rows carry label -1.  Rows come in ascending pad within an event, hit and noise-only rows
 *     interleaved; events in id order with CSR offsets.  sample_checksum and pad_checksum keep their definitions over
 *     every kept row; event_points and attpc_run_stats keep their meaning.  An event with no cloud rows still gets its
 *     noise-only rows -- a host cloud's empty events in attpc_traces_at too, so a call on empty events in full readout
 *     is a simulated pedestal run.  Callers that follow the reference's empty-event rule (simulator.py:204-205) skip
 *     the events with event_points == 0, as run_simulation and run_fused do.
 *   - decision rule (a consequence of the above, what the kernels evaluate): with N = max_j n_j, a noise-only pad of
 *     PARTIAL is kept iff 4095 - ped_p > thr and (-ped_p > thr or N > thr).  N > thr iff some u_j >= cdf[c - 1], where
 *     c = floor(thr) + 1 - min_level; c <= 0 makes it always true; c > n_levels - 1, or no noise table (N = 0 then:
 *     c = floor(thr) + 1 against the one level 0), makes it false.  So for thr >= 0 a noise-only pad is kept iff
 *     4095 - ped_p > thr and some u_j >= cdf[c - 1]: one u32 compare per sample, no table search; with thr >= 0 and
 *     c > n_levels - 1 (the default threshold 40 with gaussian_noise_table(5), whose levels end at +-40) no noise-only
 *     pad is ever kept.  For thr < 0 every pad of S with ped_p < -thr is kept, and any other one with a draw N > thr
 *     (with a table that has levels >= 0, all but never-seen draws).
 * Device storage of a readout chunk: 3 x 1 280 B of bitmaps per event beside the trace outputs.  Every readout run
 * sizes its trace chunks for |S| kept rows per event (about 4 GiB of samples a chunk) until it has seen its own rate
 * (FULL: always |S|); attpc_traces_at takes its events in chunks of the same size, so a pedestal run of any number of
 * events holds at most two chunks of outputs on the device.  A run whose events have nothing to scatter (a layout
 * without simulated nuclei) still gets the noise-only rows of every event. */
#define ATTPC_READOUT_HIT 0
#define ATTPC_READOUT_PARTIAL 1
#define ATTPC_READOUT_FULL 2

typedef struct attpc_trace_readout_desc {
  int32_t mode;              /* ATTPC_READOUT_* */
  int32_t reserved;
  const uint8_t* channels;   /* [ATTPC_NUM_PADS], nonzero = in S; NULL = all pads */
} attpc_trace_readout_desc;

/* desc == NULL restores ATTPC_READOUT_HIT.  Independent of attpc_trace_configure and attpc_trace_configure_noise: no
 * call resets another.  ATTPC_E_INVALID for an unknown mode.  Enables the readout in attpc_sim_run_traces,
 * attpc_det_run_traces, attpc_traces_at and attpc_traces. */
ATTPC_API int32_t attpc_trace_configure_readout(attpc_ctx* ctx, const attpc_trace_readout_desc* desc);

/* ---- trace rows: peaks of the kept pad traces as Spyral rows, on the device (opt-in: without a call of the entry
 * points below every output of every other entry point is what it is without this section) ----
 * The first phase of Spyral's analysis (baseline, peak finding, point per peak), run on the chunk's traces in HBM
 * behind the trace write pass, before anything crosses PCIe.
 * Input: the kept trace rows of an event exactly as the trace contracts above define them -- hit, partial or full
 * readout, with or without noise and pedestals, kept by the adc_threshold rule of attpc_trace_configure.  Every trace
 * mode therefore composes with this stage as it is.
 * Parameters (attpc_peak_desc, all f64): separation >= 1, prominence >= 0, 0 <= min_width <= max_width, rel_height in
 * (0, 1], threshold.
 * For a kept row of pad p in event e (global id) with samples trace[0..511]:
 *   1. y[j] = trace[j] - ped_p, an integer (ped_p = 0 without pedestals).  The baseline is the configured pedestal
 *      -- unless attpc_trace_configure_baseline has turned the Fourier baseline on, which replaces this step (below).
 *   2. Candidates: the strict local maxima of y, a flat top counted once at (first + last) div 2, never sample 0 or
 *      511 (scipy.signal.find_peaks(y) without a condition).
 *   3. Separation: a candidate closer than ceil(separation) samples to a kept candidate of higher priority is dropped;
 *      priority = height y[k], and of two candidates of equal height the LATER one has priority.  Processed from the
 *      highest priority down (scipy's `distance` rule with its tie made definite).
 *   4. Prominence of each survivor on the whole of y: walk left from the peak while y[i] <= y[peak], keeping the
 *      minimum (updated only by a strictly lower sample: of equal minima the one nearest the peak is the base), stop
 *      at a higher sample or the edge; the same to the right; prominence = y[peak] - max(left_min, right_min);
 *      kept iff prominence >= desc.prominence (scipy.signal.peak_prominences).
 *   5. Width at h = (double)y[peak] - (double)prominence * rel_height (the product rounded, then subtracted): walk
 *      left from the peak while i > left_base && h < y[i], then left_ip = i + (h - y[i]) / (y[i+1] - y[i]) if
 *      y[i] < h, else i; mirrored for right_ip; kept iff min_width <= right_ip - left_ip <= max_width
 *      (scipy.signal.peak_widths; f64, one rounding per operation).
 *   6. A surviving peak k is a point iff y[k] > threshold (strict).  amplitude = y[k]; integral = the sum of |y[j]|
 *      over j = floor(left_ip) .. ceil(right_ip) - 1; centroid = (double)k + u with u the Philox2x32-7 jitter
 *      generator of the conventions at the top on counter (e[31:0], e[39:32] << 24 | k << 14 | p) and key word
 *      seed[31:0] ^ rotl(seed[63:32], 13) ^ 0x300: a stream of its own beside the cloud's (0x100) and, like every
 *      draw, a pure function of (seed, global event id, pad, sample).
 *   7. Row of 8 f64 in the layout of convert_to_spyral (detector/writer.py:97-110): pad_centers[p] (x, y),
 *      z = (windows_edge - centroid) / (windows_edge - micromegas_edge) * length * 1000.0 evaluated left to right
 *      with every operation rounded, amplitude, integral, p, centroid, pad_sizes[p]; label (i64) = the trace row's
 *      label (-1 for a noise-only row).  Geometry and edges are those of attpc_spyral_configure (its response and
 *      threshold play no part); windows_edge != micromegas_edge and n_pads >= ATTPC_NUM_PADS, else ATTPC_E_INVALID.
 *   8. An event's rows come in ascending z, i.e. descending centroid, equal centroids in ascending pad; events in id
 *      order with CSR offsets.  event_points keeps its meaning (cloud rows before any suppression).
 * With offset = argmax(R) in attpc_trace_configure a lone arrival at bucket t peaks at sample t, so its point's z is
 * the arrival's z; with offset = 0 every point sits argmax(R) buckets late.
 * By default the baseline is not fitted: the analysis is handed every pad's true pedestal.  Spyral has to estimate
 * it, with a Fourier low-pass filter that takes part of a wide pulse for baseline; attpc_trace_configure_baseline
 * (below) runs that estimate in place of step 1.  Spyral's later phases (clustering, fitting) are not part of this;
 * its estimation phase on the labelled rows is "track estimates of the trace rows" at the end of this file.
 * Results of a call: rows of EIGHT doubles in out->points (capacity counts rows), out->labels, out->offsets,
 * out->event_points; any of them may be NULL, and with points and labels both NULL the capacity does not bind: the
 * rows stay on the device.  stats->n_points is the number of rows of the call (as attpc_sim_run_spyral reports its
 * rows; the capacity needed on ATTPC_E_CAPACITY), every other field of stats keeps its cloud meaning.
 * attpc_trace_rows_last gives the rows and the row checksum of the context's last trace-row call:
 *   row_checksum = sum over the rows of (event * 2^23 + pad * 2^9 + k) mod 2^64, event the global event id. */
typedef struct attpc_peak_desc {
  double separation;  /* >= 1: candidates closer than ceil(separation) samples to a higher one are dropped */
  double prominence;  /* >= 0 */
  double min_width;   /* 0 <= min_width <= max_width, in samples at rel_height */
  double max_width;
  double rel_height;  /* in (0, 1] */
  double threshold;   /* points have amplitude > threshold */
} attpc_peak_desc;

/* desc == NULL turns the stage off (the trace-row entry points then answer ATTPC_E_NOTCONFIGURED).  Independent of
 * attpc_trace_configure, attpc_trace_configure_noise and attpc_trace_configure_readout: no call resets another.
 * ATTPC_E_INVALID for a parameter outside the ranges above (NaN included). */
ATTPC_API int32_t attpc_trace_configure_peaks(attpc_ctx* ctx, const attpc_peak_desc* desc);
/* attpc_sim_run_traces, then the rows of every event's traces.  ATTPC_E_INVALID without attpc_spyral_configure or
 * attpc_trace_configure. */
ATTPC_API int32_t attpc_sim_run_trace_rows(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                           const attpc_event_layout* layout, double* p4, double* vertex,
                                           int32_t* kin_status, attpc_cloud_out* out, attpc_run_stats* stats);
/* attpc_det_run_traces (kinematics from host arrays), then the rows. */
ATTPC_API int32_t attpc_det_run_trace_rows(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                           const attpc_event_layout* layout, const double* p4, const double* vertex,
                                           attpc_cloud_out* out, attpc_run_stats* stats);
/* attpc_traces_at (any host cloud; its rules for the rows), then the rows of its traces.  out->event_points receives
 * the cloud rows of every event as given. */
ATTPC_API int32_t attpc_trace_rows_at(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, int64_t n_events,
                                      const int64_t* offsets, const double* points, const int64_t* labels,
                                      attpc_cloud_out* out);
/* Rows and row checksum of the context's last trace-row call (either pointer may be NULL). */
ATTPC_API int32_t attpc_trace_rows_last(attpc_ctx* ctx, int64_t* n_rows, uint64_t* row_checksum);

/* ---- Fourier baseline of the trace rows (opt-in: off by default, and with it off every output of every entry point
 * is bit for bit what it is without this section) ----
 * Replaces Spyral's preprocess_traces / GetParameters.baseline_window_scale (the reference stops at point clouds and
 * has no counterpart: parity is unpinned there).  With the stage on it replaces step 1 of the trace-row contract
 * above.  For a kept trace row with samples trace[0..511] (int16, 0..4095) and scale = window_scale:
 *   a. Edges: x[j] = trace[j], then x[0] = x[1] and x[511] = x[510] (Spyral's edge fix).  It is part of x from here
 *      on, in the result as well.
 *   b. Peak mask, in integers: S = sum x, Q = sum x^2, d_j = 512 x[j] - S.  Sample j is masked iff d_j > 0 and
 *      4 d_j^2 > 9 (512 Q - S^2): x - mean > 1.5 std with the population std, made exact (everything fits i64).
 *   c. Replacement: if any sample is masked, m = (double)(sum of the unmasked x) / (double)(their number), one
 *      rounding (the unmasked set is never empty); b[j] = m if j is masked, else (double)x[j].
 *   d. Filter: F[k] = sinc(w_k / scale) with w_k = k for k < 256 and k - 512 otherwise, sinc(t) = sin(pi t) / (pi t),
 *      sinc(0) = 1 -- ifftshift(sinc(arange(-256, 256) / scale)) -- built on the host when the stage is configured;
 *      baseline = Re(IDFT_512(DFT_512(b) * F)) in f64.
 *   e. Result: y[j] = clamp(x[j] - (int)rint(baseline[j]), -4095, 4095) as int16 (the clamp keeps the priority key of
 *      step 3, (height + 4096) << 9, inside its domain; |y| could pass 4095 by about 1.6 % at scale 20 in theory, no
 *      realistic row does).
 *   f. Steps 2 to 8 of the trace-row contract run on this y.  Pedestals are NOT subtracted: the analysis does not
 *      know them.  What keeps a trace row is unchanged: that rule is the hardware's zero suppression and still uses
 *      the pedestal.
 *   g. Purity: the y of a row and its f64 baseline are functions of that row's 512 samples and of scale alone, bit
 *      for bit whatever rows share the launch, chunk or call: every row has a transform of its own (two rows are
 *      never packed into the real and imaginary part of one), and within one build of the library the transform has
 *      one fixed order of operations.
 *   h. Exactness: steps a to c and e are exact.  Step d is floating point (fused multiply-adds allowed), so two
 *      implementations may differ where baseline[j] lies within 1e-6 of a half-integer: there y may differ by 1, and
 *      nowhere else.  (A forward-error bound for two 512-point f64 transforms of data below 4095 is about 1e-9.)
 * tests/baseline_reference.py restates a to e in numpy.  The stage costs 1 KiB of device memory per kept trace row of
 * a chunk while it is on. */
typedef struct attpc_baseline_desc {
  double window_scale;  /* finite and > 0; Spyral's default is 20 */
} attpc_baseline_desc;

/* desc == NULL turns the stage off (the default).  Independent of every other configure call: no call resets another.
 * ATTPC_E_INVALID unless window_scale is finite and > 0.  Takes effect in attpc_sim_run_trace_rows,
 * attpc_det_run_trace_rows and attpc_trace_rows_at; no other entry point's output changes. */
ATTPC_API int32_t attpc_trace_configure_baseline(attpc_ctx* ctx, const attpc_baseline_desc* desc);
/* The stage alone on any host rows, in the manner of attpc_spyral_rows / attpc_traces: samples [n_rows][512] ->
 * y [n_rows][512] and, unless NULL, baseline [n_rows][512] (f64, step d).  The same kernel as the fused path; needs no
 * other configuration and leaves the configured stage as it is.  n_rows = 0 is ATTPC_OK; ATTPC_E_INVALID for a sample
 * outside 0..4095 or a window_scale that is not finite and > 0.  Any n_rows: the rows go through the device in bounded
 * chunks. */
ATTPC_API int32_t attpc_trace_baseline(attpc_ctx* ctx, int64_t n_rows, const int16_t* samples, double window_scale,
                                       int16_t* y, double* baseline);

/* ---- multiplicity trigger on the pad traces (opt-in: off by default, and with it off every output of every entry
 * point is bit for bit what it is without this section and no buffer of the stage is allocated) ----
 * Would the electronics have triggered on this event, and when?  The AT-TPC's GET electronics run self-triggered on pad
 * multiplicity: every channel has a discriminator, every CoBo integrates the multiplicity of its channels over a
 * sliding window and compares it with a threshold, and MuTanT requires a number of CoBos.  This stage evaluates that on
 * the chunk's traces in HBM behind the trace write pass and leaves one 32-byte record per event.  The reference has no
 * counterpart (parity is unpinned there, as for the traces themselves); tests/trigger_reference.py restates it in numpy.
 * Input: the kept trace rows of event e exactly as the trace contracts above define them -- pad p, trace_p[0..511] --
 * and the pad's pedestal ped_p (0 without pedestals), whatever the readout mode, the noise or a configured Fourier
 * baseline: the discriminator sits on the raw channel above its own pedestal, the baseline stage plays no part.
 * y_p[j] = trace_p[j] - ped_p, an integer.
 * Parameters (attpc_trigger_desc): threshold in 0..4095, window W in 1..512, group_multiplicity Mg >= 1, min_groups in
 * 1..ATTPC_MAX_TRIGGER_GROUPS, groups [ATTPC_NUM_PADS] (NULL: every pad in group 0; a value below
 * ATTPC_MAX_TRIGGER_GROUPS is the pad's trigger group, its CoBo; 255: the pad takes no part; anything else is
 * ATTPC_E_INVALID), gate (0 / 1, below).  The map from pads to CoBos is the caller's: the library has no table of it.
 *   hit_p[j]  = y_p[j] > threshold (strict; time over threshold)
 *   m_g[j]    = the number of kept rows of the event on pads of group g with hit_p[j]
 *   s_g[j]    = sum of m_g[i] over i = max(0, j - W + 1) .. j
 *   group g asserts at j iff s_g[j] >= Mg;  A[j] = the number of asserting groups
 *   the event fires iff some j has A[j] >= min_groups
 * Record (attpc_trigger_record, one per event): fired; sample = the first j with A[j] >= min_groups, else -1; groups =
 * bit g set iff group g asserts at any sample; n_rows = kept trace rows of the event, excluded pads included;
 * n_hit_pads = rows on participating pads with at least one hit; peak_group_sum = max over g, j of s_g[j] (with
 * min_groups = 1 an event fires iff this is >= Mg: one run gives the efficiency curve over Mg); peak_sum = max over j
 * of the sum over g of s_g[j]; peak_sample = the first j attaining peak_sum, -1 when that is 0.  An event without kept
 * rows gets zeros and -1s.  Every sum is at most 10240 * 512 and fits int32; every field is a count, sum, minimum or
 * maximum of integers and a pure function of (seed, global event id), independent of chunking and GPU count.
 * Only kept rows can hit.  With threshold >= the adc_threshold of attpc_trace_configure, in partial or full readout,
 * the kept rows contain every channel of the readout set that can hit: the result is that of all its channels.  In hit
 * mode noise-only pads do not exist, so they cannot contribute.
 * Gate (trace rows only): with gate = 1 attpc_*_run_trace_rows and attpc_trace_rows_at produce no rows for an event
 * that did not fire -- the peak passes skip its trace rows; offsets keep one entry per event (an unfired event is an
 * empty range), event_points and the cloud statistics keep their meaning, row_checksum and n_rows cover the rows
 * produced.  The trace entry points (attpc_*_run_traces, attpc_traces_at) deliver all rows whatever gate says:
 * dropping the rows of unfired events before the copy is out of scope (the packed entry points, "packed pad traces"
 * below, make every row cheaper to copy instead; they too deliver all rows). */
#define ATTPC_MAX_TRIGGER_GROUPS 16
typedef struct attpc_trigger_desc {
  int32_t threshold;           /* 0..4095: discriminator level above the pedestal */
  int32_t window;              /* W in 1..512 samples */
  int32_t group_multiplicity;  /* Mg >= 1 */
  int32_t min_groups;          /* 1..ATTPC_MAX_TRIGGER_GROUPS */
  const uint8_t* groups;       /* [ATTPC_NUM_PADS] or NULL (host memory, copied by the call) */
  int32_t gate;                /* 0 / 1 */
  int32_t reserved;            /* 0 */
} attpc_trigger_desc;

typedef struct attpc_trigger_record {
  int32_t fired;
  int32_t sample;
  uint32_t groups;
  int32_t n_rows;
  int32_t n_hit_pads;
  int32_t peak_group_sum;
  int32_t peak_sum;
  int32_t peak_sample;
} attpc_trigger_record;

/* desc == NULL turns the stage off (the default).  Independent of every other configure call: no call resets another.
 * ATTPC_E_INVALID for anything outside the ranges above.  Takes effect in the six trace and trace-row entry points
 * (attpc_sim_run_traces, attpc_det_run_traces, attpc_traces_at and their *_trace_rows counterparts). */
ATTPC_API int32_t attpc_trace_configure_trigger(attpc_ctx* ctx, const attpc_trigger_desc* desc);
/* Records first .. first + count - 1 of the context's last trace or trace-row call, in the call's event order (a call
 * repeated after ATTPC_E_CAPACITY overwrites them).  ATTPC_E_NOTCONFIGURED if no trigger was configured for that
 * call, ATTPC_E_INVALID for a range outside it. */
ATTPC_API int32_t attpc_trigger_last(attpc_ctx* ctx, int64_t first, int64_t count, attpc_trigger_record* out);
/* The stage alone on any host rows in CSR form, through the same kernel (what attpc_trace_baseline is to the baseline
 * stage): offsets [n_events + 1], pads [rows], samples [rows][512], pedestals [ATTPC_NUM_PADS] or NULL -> out
 * [n_events].  Needs no other configuration and leaves the configured stage as it is; desc->gate plays no part.
 * ATTPC_E_INVALID for a pad outside 0..10239, a sample outside 0..4095, a pedestal outside 0..4095, decreasing
 * offsets or a desc out of range. */
ATTPC_API int32_t attpc_trigger_rows(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const int32_t* pads,
                                     const int16_t* samples, const int16_t* pedestals, const attpc_trigger_desc* desc,
                                     attpc_trigger_record* out);

/* ---- micromegas gain of the traces (opt-in: off by default, and with it off every output of every entry point is bit
 * for bit what it is without this section and no buffer of the stage is allocated) ----
 * Without this stage a cloud row of q electrons lands on its pad as exactly q * R[...]: one gain for every electron and
 * every pad.  The stage puts the detector's own amplitude response between the assembled cloud and the trace kernels:
 * the avalanche statistics of the micromegas (a Polya-distributed single-electron gain) and pad-to-pad gain differences
 * (what Spyral's gain-match file corrects).  The reference stops at point clouds and has no counterpart (parity is
 * unpinned there, as for the traces themselves); tests/gain_reference.py restates the stage in numpy.
 * Settings (attpc_trace_gain_desc):
 *   - rel_variance f in [0, 1]: the relative variance of the single-electron gain, 1 / (1 + theta) for a Polya
 *     parameter theta >= 0; a bucket of q electrons then has a relative amplitude spread of sqrt(f / q).  f = 0: pad
 *     gains only.
 *   - pad_gain [ATTPC_NUM_PADS], finite and >= 0; NULL = 1.0 everywhere.
 *   - stream < 2^30 draws another realisation on the same physics.
 *   - quantiles Z[0 .. ATTPC_GAIN_KNOTS - 1], finite and non-decreasing doubles: the inverse CDF of the standardised
 *     fluctuation (mean 0, variance 1) at equally spaced knots.  Required when f > 0, ignored when f = 0.
 * Gained charge of a cloud row of event e (global id), pad p, t = floor(tau) and electrons q:
 *   - q == 0: q' = 0.  Otherwise
 *       u  = word 0 of Philox4x32-10(counter = (e[31:0], e[63:32], p * 512 + t, 0x40000000 | stream),
 *                                   key = (seed[31:0], seed[63:32]))
 *       i  = u >> 20,  w = (double)(u & 0xFFFFF) * 2^-20
 *       z  = Z[i] + (Z[i + 1] - Z[i]) * w
 *       r  = c / q, with c = f / 9.0 computed once on the host in f64
 *       s  = sqrt(r)
 *       x  = max((1.0 - r) + z * s, 0.0)         (a NaN, which only a subnormal q can produce, counts as 0)
 *       q' = ((q * x) * x) * x
 *     the Wilson-Hilferty form of Gamma(shape q / f, scale f), the sum of q Polya gains of mean 1.  With f = 0 no draw
 *     is made and x = 1: q' = q exactly.
 *   - q'' = q' * pad_gain[p].
 *   - every operation above is rounded once (no fused multiply-add); / and sqrt are the correctly rounded f64
 *     operations.
 * Effect: the trace contract holds with q'' in place of q_r in A_p[j].  The label rule still uses the cloud's own q.
 * Rows of one event have distinct (pad, t), so every row has a counter of its own; the domain 0x40000000 | stream is
 * disjoint from every other draw's (0, 1 + row, 0x200 + entry, the noise's 0x80000000 | stream, and the jitter
 * generators).  q'' is a pure function of (seed, global event id, pad, t, q): it does not depend on chunking, GPU
 * count or what shares the launch.
 * Unchanged: every cloud output, attpc_run_stats, event_points, the cloud-based Spyral rows, and the row order.
 * Device storage: 8 B per cloud row of a chunk while the stage is on. */
#define ATTPC_GAIN_KNOTS 4097

typedef struct attpc_trace_gain_desc {
  double rel_variance;      /* f in [0, 1] */
  const double* pad_gain;   /* [ATTPC_NUM_PADS], NULL = 1.0 everywhere */
  const double* quantiles;  /* [ATTPC_GAIN_KNOTS]; may be NULL when rel_variance == 0 */
  uint32_t stream;          /* < 2^30 */
  int32_t reserved;
} attpc_trace_gain_desc;

/* desc == NULL turns the stage off (the default); so does rel_variance == 0 without a pad_gain.  Independent of the
 * other attpc_trace_configure_* calls: no call resets another.  ATTPC_E_INVALID for rel_variance outside [0, 1] or not
 * finite, a negative or non-finite pad gain, a decreasing or non-finite table, a missing table with rel_variance > 0,
 * or stream >= 2^30.  With the stage on it acts in attpc_sim_run_traces, attpc_det_run_traces, attpc_traces_at,
 * attpc_traces and the trace-row entry points (attpc_*_run_trace_rows, attpc_trace_rows_at); through their traces it
 * reaches the Fourier baseline and the trigger. */
ATTPC_API int32_t attpc_trace_configure_gain(attpc_ctx* ctx, const attpc_trace_gain_desc* desc);
/* The stage alone on any host cloud, through the same kernel: offsets [n_events + 1], points [rows, 3] (pad, tau,
 * electrons) -> gained [rows] (q'' of every row; event i of the call is the global event first_event + i).  The rows
 * are validated as attpc_traces validates them.  With the stage off gained is the cloud's own charge.  The id-range
 * rules at the top apply. */
ATTPC_API int32_t attpc_gain_rows(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, int64_t n_events,
                                  const int64_t* offsets, const double* points, double* gained);

/* ---- common-mode noise of the traces (opt-in: off by default, and with it off every output of every entry point is
 * bit for bit what it is without this section and no buffer of the stage is allocated) ----
 * The noise above is independent from pad to pad.  On the GET electronics a share of the noise is coherent: every
 * channel of a chip or board moves together.  The stage adds one further draw per (event, group, sample) to every pad of
 * the group; the pad -> group map is the caller's (the project holds no hardware map).  The reference stops at point
 * clouds and has no counterpart; tests/common_mode_reference.py restates the stage in numpy.
 * Notation as in the noise contract (s_p, ped_p, n_p, thr, e, seed).
 * Settings (attpc_trace_common_desc):
 *   - groups [ATTPC_NUM_PADS] uint8: a value g < 255 is the pad's group, 255 means the pad has no common-mode term;
 *     NULL puts every pad in group 0.  n_groups = 1 + max g over the pads with g < 255 (a map of 255 alone: the stage
 *     is off).
 *   - a noise table of its own -- cdf [n_levels - 1] u32, n_levels, min_level -- under the rules of
 *     attpc_trace_noise_desc: at most ATTPC_MAX_NOISE_LEVELS levels, |min_level| <= 4095, a non-decreasing cdf;
 *     n_levels = 0 turns the stage off.
 *   - stream < 2^29 draws another realisation on the same physics.
 * Draw of sample j of group g in event e:
 *       out = Philox4x32-10(counter = (e[31:0], e[63:32], g * 128 + 2 * (j mod 64) + (j div 256), 0x20000000 | stream),
 *                           key = (seed[31:0], seed[63:32])),   u = out[(j div 64) mod 4]
 *       c_g[j] = min_level + #{k : cdf[k] <= u}
 *     the pad noise's layout with g in place of p.  The domain 0x20000000 | stream is disjoint from every other draw's
 *     (0, 1 + row, 0x200 + entry -- all below 2^19 --, the gain's 0x40000000 | stream, the noise's 0x80000000 | stream,
 *     and the jitter generators).
 * Sample of a pad with group g != 255:
 *       trace_p[j] = min(max(s_p[j] + ped_p + n_p[j] + c_g[j], 0), 4095)
 *     A pad of group 255 keeps the formula of the noise contract.  n_p = 0 and ped_p = 0 when no pad noise is configured:
 *     the stage does not need attpc_trace_configure_noise.  A row is kept iff max_j (trace_p[j] - ped_p) > thr, as before,
 *     in hit mode and for every candidate of ATTPC_READOUT_PARTIAL; ATTPC_READOUT_FULL keeps every pad of S.  Everything
 *     is integer arithmetic, and c_g[j] is a pure function of (seed, global event id, group, sample): chunking, GPU count
 *     and what shares a launch play no part.
 * Unchanged: labels, row order, offsets, the definitions of sample_checksum and pad_checksum (over the samples with
 *     the term), event_points, attpc_run_stats, every cloud output and the cloud-based Spyral rows.  The trace rows, the
 *     Fourier baseline and the trigger see the stage through the traces.
 * Decision rule for a noise-only pad of PARTIAL with group g != 255 (a consequence of the above, s_p = 0):
 *   - 4095 - ped_p <= thr: the pad is never kept;
 *   - -ped_p > thr: the pad is always kept (its samples never go below 0);
 *   - otherwise the pad is kept iff some j has n_p[j] + c_g[j] > thr (the clamps cannot change the verdict then:
 *     thr >= -ped_p and thr < 4095 - ped_p).
 *   The one-compare cutoff of the readout contract holds for pads of group 255 only.  No noise-only pad at all is kept,
 *   and the scan is skipped, iff thr >= 0, the pad table alone never crosses (c > n_levels - 1 there) and the largest
 *   pad level plus the largest common-mode level is <= thr (0 for the pad level without a pad table).
 * Device storage: 1 KiB per (event, group) of a chunk, int16 in the trace kernels' lane order (lane l of a wave holds
 * samples l + 64 s, s = 0 .. 7, as 16 contiguous bytes), in a grow-only buffer of the chunk's assembly set, allocated
 * only while the stage is on. */
typedef struct attpc_trace_common_desc {
  const uint8_t* groups;     /* [ATTPC_NUM_PADS], 255 = no common-mode term; NULL = every pad in group 0 */
  const uint32_t* cdf;       /* [n_levels - 1] */
  int32_t n_levels;          /* 0 = the stage off */
  int32_t min_level;
  uint32_t stream;           /* < 2^29 */
  int32_t reserved;
} attpc_trace_common_desc;

/* desc == NULL turns the stage off (the default); so do n_levels == 0 and a map of 255 alone.  Independent of the other
 * attpc_trace_configure_* calls: no call resets another.  ATTPC_E_INVALID for a decreasing cdf, more than
 * ATTPC_MAX_NOISE_LEVELS levels, |min_level| > 4095, a table of several levels without a cdf, or stream >= 2^29.  With
 * the stage on it acts wherever the pad noise does: attpc_sim_run_traces, attpc_det_run_traces, attpc_traces_at,
 * attpc_traces and the trace-row entry points. */
ATTPC_API int32_t attpc_trace_configure_common_mode(attpc_ctx* ctx, const attpc_trace_common_desc* desc);
/* The stage alone, through the same kernel: out [n_events][n_groups][512] int16 in sample order, c_g[j] of the global
 * events first_event .. first_event + n_events - 1.  ATTPC_E_NOTCONFIGURED with the stage off.  The id-range rules at
 * the top apply. */
ATTPC_API int32_t attpc_common_mode_rows(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, int64_t n_events,
                                         int16_t* out);

/* ---- packed pad traces (opt-in: without a call of the entry points below every output, kernel and instruction
 * stream of every other entry point is what it is without this section) ----
 * A kept pad row crosses PCIe as 512 int16 samples (1 KiB), most of them pedestal plus a few counts of noise.  The
 * packed entry points deliver the same rows as losslessly packed records instead: a per-block frame-of-reference code
 * with bit planes, made on the device from the samples the trace write pass left in HBM (csrc/trace_pack.hip), before
 * anything crosses the link.  The encoding of a row is unique, so the device is tested byte for byte against the
 * numpy restatement in tests/trace_pack_reference.py.  The reference has no counterpart (it stops at point clouds).
 *
 * Format ATTPC_TRACE_PACK_FORMAT = "for64-bitplane-v1".  A row is 512 samples s[j] in 0 .. 4095 (every trace
 * configuration clamps to that range).  Block b (0 .. 7) holds samples 64 b .. 64 b + 63.  For each block
 *     w_b = bit_length(maximum - minimum), in 0 .. 12,     base_b = min(the minimum of the block, 4096 - 2^w_b).
 * The base is the block's minimum -- except where minimum + 2^w - 1 would pass 4095 (minimum 290, maximum 4095: w = 12),
 * where it is the largest base whose w bits stay inside 0 .. 4095; s - base_b still needs exactly w_b bits.  So the
 * header alone bounds every sample a record can hold, and a decoder checks nothing else to stay inside 12 bits.
 * The record of a row is, in this order,
 *   - 8 little-endian u16 headers h_b = base_b | w_b << 12 (16 bytes);
 *   - then, for b ascending and k = 0 .. w_b - 1 ascending, one little-endian u64 plane word whose bit i is bit k of
 *     s[64 b + i] - base_b.
 * A row takes 16 + 8 sum_b w_b bytes: 16 (a constant row) to 784 (ATTPC_TRACE_PACK_MAX_ROW_BYTES), always a multiple
 * of 8.  row_start is an int64 array [R + 1] of byte offsets into one byte array: record r is bytes row_start[r] ..
 * row_start[r + 1]; row_start[0] = 0 and the offsets are absolute within a call, across its chunks.
 * The encoders (device and host) emit exactly that base and the minimal width: the bytes are unique.  The decoder
 * accepts any w <= 12 with base + 2^w - 1 <= 4095.
 *
 * Device cost: per chunk of a run two kernels behind the trace write pass (record sizes; records), a scan between
 * them, and one host round trip for the chunk's bytes (they size the record buffer and the caller's row_start, and
 * answer the capacity); 28 bytes of scratch per kept row and the records themselves beside the samples. */
#define ATTPC_TRACE_PACK_FORMAT "for64-bitplane-v1"
#define ATTPC_TRACE_PACK_MAX_ROW_BYTES 784

/* attpc_trace_out with the samples replaced by their records; any array may be NULL (that output stays on the device;
 * with all of them NULL the run still reports n_rows, n_bytes and the checksums: the packed size of a run at the
 * device-resident rate). */
typedef struct attpc_trace_packed_out {
  int64_t capacity;          /* rows pads / labels hold; row_start holds capacity + 1 entries */
  int64_t* offsets;          /* [n_events + 1] CSR offsets of the events' rows */
  int32_t* pads;             /* [capacity] */
  int64_t* row_start;        /* [capacity + 1] byte offsets of the rows' records in bytes */
  uint8_t* bytes;            /* [byte_capacity] the records */
  int64_t byte_capacity;
  int64_t* labels;           /* [capacity] */
  int64_t* event_points;     /* [n_events] */
  int64_t n_rows;            /* written: kept rows of the call */
  int64_t n_bytes;           /* written: bytes of their records */
  uint64_t sample_checksum;  /* written: as in attpc_trace_out, taken over the samples */
  uint64_t pad_checksum;     /* written: as in attpc_trace_out */
} attpc_trace_packed_out;

/* attpc_sim_run_traces, attpc_det_run_traces and attpc_traces_at with that out struct: the same events, rows, pads,
 * labels, offsets, event_points, checksums, stats and trigger records (attpc_trigger_last), and the same id-range
 * rules.  ATTPC_E_CAPACITY when the rows pass capacity (any row array wanted) or the bytes pass byte_capacity (bytes
 * wanted): n_rows and n_bytes then hold what the whole call needs, and the row arrays are unspecified. */
ATTPC_API int32_t attpc_sim_run_traces_packed(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                              const attpc_event_layout* layout, double* p4, double* vertex,
                                              int32_t* kin_status, attpc_trace_packed_out* out, attpc_run_stats* stats);
ATTPC_API int32_t attpc_det_run_traces_packed(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                              const attpc_event_layout* layout, const double* p4, const double* vertex,
                                              attpc_trace_packed_out* out, attpc_run_stats* stats);
ATTPC_API int32_t attpc_traces_packed_at(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, int64_t n_events,
                                         const int64_t* offsets, const double* points, const int64_t* labels,
                                         attpc_trace_packed_out* out);
/* The stage alone on any host rows, through the same two kernels: samples [n_rows][512] -> row_start [n_rows + 1]
 * (may be NULL), bytes [byte_capacity] (may be NULL: sizes only) and *n_bytes (may be NULL) = the bytes all rows take.
 * ATTPC_E_INVALID for a sample outside 0 .. 4095; ATTPC_E_CAPACITY (with *n_bytes and row_start written) when bytes
 * is given and too small. */
ATTPC_API int32_t attpc_trace_pack(attpc_ctx* ctx, int64_t n_rows, const int16_t* samples, int64_t* row_start,
                                   uint8_t* bytes, int64_t byte_capacity, int64_t* n_bytes);
/* The same encoder and the decoder on the host: no context, no GPU (csrc/trace_pack_host.cpp).  attpc_trace_pack_host
 * takes and answers what attpc_trace_pack does.  attpc_trace_unpack: records row_start[r] .. row_start[r + 1] of bytes
 * [n_bytes], r < n_rows (row_start[0] need not be 0: any run of consecutive rows of a call decodes alone) -> samples
 * [n_rows][512], over n_threads host threads (the rule of attpc_unpack_rows; 0 = automatic).  ATTPC_E_INVALID, with no
 * read or write outside what it was given, for: offsets that decrease or are no multiples of 8, a span past n_bytes
 * or below 0, a width above 12, base + 2^w - 1 above 4095, a record whose header-implied size differs from its span
 * (samples of a refused call are unspecified). */
ATTPC_API int32_t attpc_trace_pack_host(int64_t n_rows, const int16_t* samples, int64_t* row_start, uint8_t* bytes,
                                        int64_t byte_capacity, int64_t* n_bytes);
ATTPC_API int32_t attpc_trace_unpack(const uint8_t* bytes, int64_t n_bytes, const int64_t* row_start, int64_t n_rows,
                                     int16_t* samples, int32_t n_threads);

/* ---- event and track summaries of a device-resident run (opt-in: without a call of the entry points below every
 * output of every other entry point is what it is without this section) ----
 * A summary run is a device-resident run (attpc_sim_run with out == NULL: same chunks, no event-ordered copy of the
 * cloud) that reduces every chunk's cloud and track samples, in place and right behind its scatter, to one fixed-size
 * record per event and one per (event, simulated nucleus): a few hundred bytes per event cross the link instead of
 * the cloud.
 * Settings (attpc_summary_desc): min_electrons >= 0 -- a cloud row is KEPT iff its electrons q >= min_electrons (0
 * keeps every row) -- and pad_centers [n_pads, 2] (mm), n_pads >= ATTPC_NUM_PADS: the geometry of rho2_max, a copy of
 * the mode's own.
 * For the event with global id e, over its cloud rows (pad p, tau, q, label l) exactly as attpc_sim_run / attpc_det_run
 * produce them for the same seed and id (every extension included), t = floor(tau):
 *   - event record: n_points = all rows (what event_points reports); n_kept = kept rows; n_pads = distinct pads among
 *     the kept rows; tb_min / tb_max = smallest / largest t over the kept rows, -1 / -1 without one; charge = sum of q
 *     over ALL rows (whole numbers: the event's share of charge_checksum).
 *   - track record, one per event and position s of layout->indices ([n_events][n_sim]), over the rows with
 *     l == indices[s]: the same six fields, and rho2_max = max over the kept rows of x * x + y * y with
 *     (x, y) = pad_centers[p], each product rounded and then added (no fused multiply-add), -1.0 without a kept row.
 *     A cloud row carries the label of the nucleus that touched its (pad, time bucket) cell LAST
 *     (detector/simulator.py:40-47): a cell shared by two tracks counts, charge and all, for the later one.
 *     The track part: n_steps = ODE samples recorded for the track and n_samples = track samples with >= 1 electron
 *     (n_steps / counts of attpc_det_tracks); electrons = sum of the samples' fourth column (electrons x gain: what
 *     the track put into the gas, before the pad plane lost any of it); end_x, end_y, end_tb = columns 0..2 of the
 *     last sample with >= 1 electron (m, m, time bucket), NaN with n_samples == 0.
 *   - a position whose species is skipped (species_of_row == -1) has an all-empty record.  A row that occurs twice in
 *     indices: the cloud part of its label goes to the first position that holds it, later positions get the empty
 *     cloud part; the track part is per position either way.
 * Every field is a count, an integer sum, a minimum or a maximum: a pure function of (seed, global event id) that does
 * not depend on chunking, on how a call's id range is split, on the scatter build or on the order in which workgroups
 * run.  attpc_run_stats keeps its cloud meaning (what attpc_sim_run reports for the same ids); the id-range rules at
 * the top apply; a pending attpc_sim_hint_next is dropped.  The sizes are known: there is no capacity. */
typedef struct attpc_event_summary {
  uint32_t n_points;
  uint32_t n_kept;
  uint32_t n_pads;
  int32_t tb_min;
  int32_t tb_max;
  int32_t reserved;   /* 0 */
  int64_t charge;
} attpc_event_summary;  /* 32 bytes */

typedef struct attpc_track_summary {
  uint32_t n_points;
  uint32_t n_kept;
  uint32_t n_pads;
  int32_t tb_min;
  int32_t tb_max;
  int32_t reserved;   /* 0 */
  int64_t charge;
  double rho2_max;    /* mm^2 */
  int32_t n_steps;
  int32_t n_samples;
  int64_t electrons;
  double end_x;       /* m */
  double end_y;       /* m */
  double end_tb;      /* time bucket */
} attpc_track_summary;  /* 80 bytes */

typedef struct attpc_summary_desc {
  int64_t min_electrons;     /* >= 0 */
  const double* pad_centers; /* [n_pads, 2] mm */
  int32_t n_pads;            /* >= ATTPC_NUM_PADS */
  int32_t reserved;
} attpc_summary_desc;

/* Host output of a summary call; either array may be NULL. */
typedef struct attpc_summary_out {
  attpc_event_summary* events; /* [n_events] */
  attpc_track_summary* tracks; /* [n_events * n_sim] */
} attpc_summary_out;

/* desc == NULL turns the mode off (the entry points below then answer ATTPC_E_NOTCONFIGURED).  Independent of
 * attpc_spyral_configure, the attpc_trace_configure* calls and the peak stage: no call resets another.
 * ATTPC_E_INVALID for min_electrons < 0, n_pads < ATTPC_NUM_PADS or pad_centers == NULL. */
ATTPC_API int32_t attpc_summary_configure(attpc_ctx* ctx, const attpc_summary_desc* desc);
/* attpc_sim_run with out == NULL, plus the records of every event and track. */
ATTPC_API int32_t attpc_sim_run_summary(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                        const attpc_event_layout* layout, double* p4, double* vertex,
                                        int32_t* kin_status, attpc_summary_out* out, attpc_run_stats* stats);
/* The same with kinematics from host arrays p4 [n, n_rows, 4] / vertex [n, 3] (the file-driven flow). */
ATTPC_API int32_t attpc_det_run_summary(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                        const attpc_event_layout* layout, const double* p4, const double* vertex,
                                        attpc_summary_out* out, attpc_run_stats* stats);
/* The cloud part for any host cloud in CSR form, through the kernel of the fused path: offsets [n_events + 1]
 * (nondecreasing), points [rows, 3] (pad, tau, electrons), labels [rows].  Every row needs an integer pad in
 * [0, ATTPC_NUM_PADS), 0 <= tau < 512 and finite electrons >= 0, else ATTPC_E_INVALID; distinct (pad, t) is neither
 * required nor checked.  Rows whose label is not in layout->indices count for the event record only.  The track part of
 * every record is the empty one (n_steps = n_samples = 0, electrons = 0, ends NaN).  Needs attpc_summary_configure
 * only (layout->species_of_row is ignored). */
ATTPC_API int32_t attpc_cloud_summary(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* points,
                                      const int64_t* labels, const attpc_event_layout* layout, attpc_summary_out* out);

/* ---- selected delivery: only the events that pass a selection on their summary records are delivered (opt-in and
 * additive under ABI version 3: without a call of the entry points below every output of every other entry point is
 * what it is without this section) ----
 * A selected run is the delivered run attpc_sim_run / attpc_det_run (kind ATTPC_SELECT_CLOUD) or attpc_sim_run_spyral /
 * attpc_det_run_spyral (kind ATTPC_SELECT_SPYRAL) that, behind every chunk's scatter and before its assembly, reduces
 * the chunk to the records of the section above and evaluates a predicate on them: the rows of an event that fails it
 * are not put in event order, not converted and not copied.
 * The predicate, passed = f(event record E, track records T[0 .. n_sim), desc), on exactly the records
 * attpc_sim_run_summary produces for the same seed, global event id, min_electrons and pad centres:
 *   - event cuts, each an inclusive range [lo, hi]: E.n_kept; E.n_pads; the time-bucket span E.tb_max - E.tb_min + 1
 *     (0 when E.n_kept == 0); E.charge.
 *   - track cuts, on every position s of layout->indices whose bit s is set in track_mask: T[s].n_kept; T[s].n_pads;
 *     T[s].n_samples; T[s].rho2_max (mm^2; the record's -1.0 for "no kept row" compares as -1.0); T[s].end_tb; and
 *     end_rho2 = fl(fl(end_x * end_x) + fl(end_y * end_y)) in m^2: both products rounded, then added (no fused
 *     multiply-add), as for rho2_max.  A masked position passes iff all of its evaluated cuts hold.
 *   - the event passes iff its event cuts hold and at least min_tracks masked positions pass: popcount(track_mask) asks
 *     for all of them, 1 for any, 0 for no track cut at all.
 *   - a range whose two bounds are both at their open values (0 / UINT32_MAX, INT64_MIN / INT64_MAX, -inf / +inf) is
 *     NOT evaluated: an absent cut lets a NaN end point through.  An evaluated range is lo <= v && v <= hi, false for
 *     NaN.
 * f is a pure function of the records and desc, so passed does not depend on chunking, on how a call's id range is
 * split, on the scatter build or on the number of GPUs, as the records do not. */
typedef struct attpc_select_desc {
  uint32_t n_kept_lo, n_kept_hi;             /* event cuts */
  uint32_t n_pads_lo, n_pads_hi;
  uint32_t tb_span_lo, tb_span_hi;
  int64_t charge_lo, charge_hi;
  uint32_t track_mask;                       /* bit s: position s of layout->indices is cut on; bits >= ATTPC_MAX_SIM
                                                are ATTPC_E_INVALID */
  uint32_t min_tracks;                       /* <= popcount(track_mask) */
  uint32_t track_n_kept_lo, track_n_kept_hi; /* track cuts */
  uint32_t track_n_pads_lo, track_n_pads_hi;
  uint32_t track_n_samples_lo, track_n_samples_hi;
  double track_rho2_max_lo, track_rho2_max_hi; /* mm^2 */
  double track_end_tb_lo, track_end_tb_hi;     /* time bucket */
  double track_end_rho2_lo, track_end_rho2_hi; /* m^2 */
} attpc_select_desc;  /* 120 bytes */

#define ATTPC_SELECT_CLOUD 0   /* rows as attpc_sim_run delivers them: points [capacity, 3] */
#define ATTPC_SELECT_SPYRAL 1  /* rows as attpc_sim_run_spyral delivers them: points [capacity, 8] */

/* Host output of a selected run.  offsets has n_events + 1 entries whatever passed: a rejected event is an empty
 * range, so position e is global id first_event + e as in every other run.  event_points[e] keeps its meaning (the
 * cloud rows of event e before selection and threshold).  events / tracks: the records of ALL events (either may be
 * NULL).  capacity binds the SELECTED rows, and only when points and labels are both given: with either NULL nothing of
 * the rows is copied and everything else (offsets, passed, records, n_passed, n_rows) is still produced -- what a
 * selection would deliver.  ATTPC_E_CAPACITY: n_rows says what is needed (stats.n_points is the cloud's). */
typedef struct attpc_select_out {
  int32_t kind;          /* in: ATTPC_SELECT_CLOUD / ATTPC_SELECT_SPYRAL */
  int32_t reserved;      /* 0 */
  int64_t capacity;      /* in: rows available in points / labels */
  int64_t* offsets;      /* [n_events + 1] or NULL */
  double* points;        /* [capacity, 3 or 8] or NULL */
  int64_t* labels;       /* [capacity] or NULL */
  int64_t* event_points; /* [n_events] or NULL */
  uint8_t* passed;       /* [n_events] or NULL: 1 = the event passed */
  attpc_event_summary* events; /* [n_events] or NULL */
  attpc_track_summary* tracks; /* [n_events * n_sim] or NULL */
  int64_t n_passed;      /* out: events that passed */
  int64_t n_rows;        /* out: rows of the passed events (Spyral kind: those above the threshold) */
} attpc_select_out;

/* desc == NULL turns the mode off.  Independent of every other *_configure: no call resets another.  ATTPC_E_INVALID
 * for lo > hi in any range, a NaN bound, min_tracks > popcount(track_mask) or mask bits at or above ATTPC_MAX_SIM. */
ATTPC_API int32_t attpc_select_configure(attpc_ctx* ctx, const attpc_select_desc* desc);
/* attpc_sim_run / attpc_sim_run_spyral (out->kind) of the events that pass.  Needs attpc_summary_configure and
 * attpc_select_configure, the Spyral kind attpc_spyral_configure as well (else ATTPC_E_NOTCONFIGURED); a mask bit at or
 * above layout->n_sim is ATTPC_E_INVALID.  attpc_run_stats keeps its cloud meaning over ALL events (n_points: every
 * cloud row, in either kind), the kinematics outputs cover all events; a pending attpc_sim_hint_next is dropped. */
ATTPC_API int32_t attpc_sim_run_selected(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                         const attpc_event_layout* layout, double* p4, double* vertex,
                                         int32_t* kin_status, attpc_select_out* out, attpc_run_stats* stats);
/* The same with kinematics from host arrays p4 [n, n_rows, 4] / vertex [n, 3] (the file-driven flow). */
ATTPC_API int32_t attpc_det_run_selected(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                         const attpc_event_layout* layout, const double* p4, const double* vertex,
                                         attpc_select_out* out, attpc_run_stats* stats);
/* The predicate on any host cloud through the same kernels: attpc_cloud_summary (same arguments, same checks; out may
 * be NULL) followed by the selection.  The track part of the records is the empty one (n_samples = 0, ends NaN), so a
 * present cut on an end point rejects and an absent one passes.  passed [n_events].  A mask bit at or above
 * layout->n_sim is ATTPC_E_INVALID. */
ATTPC_API int32_t attpc_cloud_select(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* points,
                                     const int64_t* labels, const attpc_event_layout* layout, attpc_summary_out* out,
                                     uint8_t* passed);

/* ---- run maps: pad and time-bucket hit maps summed over the events of a device-resident run (opt-in and additive
 * under ABI version 3: without a call of the entry points below every output of every other entry point is what it is
 * without this section) ----
 * A maps run is the summary run of the section above that also reads every chunk's rows once more, in place and behind
 * the chunk's summary kernels (and the selection on their records), into a few maps of the detector: how often every pad
 * fires, how much charge it collects and where in the drift window the kept charge sits, over all events or over those
 * an acceptance cut keeps.  The result is 172 KiB per call whatever its length.
 * Settings (attpc_maps_desc):
 *   - track_mask: bit s < ATTPC_MAX_SIM -- rows labelled layout->indices[s] contribute; bit ATTPC_MAX_SIM -- rows whose
 *     label is in no position of layout->indices contribute.  The label -> position rule is the summary's: a label that
 *     occurs twice in indices belongs to its first position (the bit of a later one names no row, nor does a bit at or
 *     above layout->n_sim).  The full mask is (2 << ATTPC_MAX_SIM) - 1.
 *   - selected: 0 -- every event contributes; 1 -- only the events that pass the configured selection
 *     (attpc_select_configure: the predicate of "selected delivery", on the same records).
 * min_electrons is that of attpc_summary_configure: KEPT means what it means there.
 * For a call over the global ids [first, first + n): E = the events that contribute; a row COUNTS iff it belongs to an
 * event of E, is kept (q >= min_electrons) and its position's bit is set; t = floor(tau).  Then
 *   pad_events[p] = events of E with at least one counted row on pad p      pad_charge[p] = sum of q over those rows
 *   tb_events[t]  = events of E with a counted row in time bucket t         tb_rows[t]    = counted rows in bucket t
 *   tb_charge[t]  = sum of q over the counted rows in bucket t
 *   n_events = |E| (an event with nothing to scatter is in E if it passes)  n_hit = events of E with a counted row
 * Every term is an integer, so:
 *   - maps(A u B) = maps(A) + maps(B), field by field, for disjoint id ranges A and B (what shards of a run add up);
 *   - the maps do not depend on chunking, on the scatter build, on buffer growth (a chunk that is scattered again counts
 *     once) or on the order in which workgroups run;
 *   - with the full mask and selected = 0: sum(pad_events) = sum(events[].n_pads), sum(tb_rows) = sum(events[].n_kept);
 *   - at min_electrons = 0 as well: sum(pad_charge) = sum(tb_charge) = sum(events[].charge).
 * One call makes one plane: maps per position take one call per mask. */
typedef struct attpc_maps_desc {
  uint32_t track_mask; /* != 0, no bit above ATTPC_MAX_SIM */
  uint32_t selected;   /* 0 / 1 */
} attpc_maps_desc;

/* Host output of a maps call.  Any array may be NULL; n_events and n_hit are filled whatever arrays are given. */
typedef struct attpc_maps_out {
  uint64_t* pad_events; /* [ATTPC_NUM_PADS] */
  int64_t* pad_charge;  /* [ATTPC_NUM_PADS] */
  uint64_t* tb_events;  /* [ATTPC_NUM_TB] */
  uint64_t* tb_rows;    /* [ATTPC_NUM_TB] */
  int64_t* tb_charge;   /* [ATTPC_NUM_TB] */
  uint64_t n_events;    /* out */
  uint64_t n_hit;       /* out */
} attpc_maps_out;

/* desc == NULL turns the mode off (the entry points below then answer ATTPC_E_NOTCONFIGURED).  Independent of every
 * other *_configure: no call resets another.  ATTPC_E_INVALID for an empty mask, mask bits above ATTPC_MAX_SIM or
 * selected > 1. */
ATTPC_API int32_t attpc_maps_configure(attpc_ctx* ctx, const attpc_maps_desc* desc);
/* attpc_sim_run_summary plus the maps.  records (may be NULL, as may its arrays): the records of ALL events, as
 * attpc_sim_run_summary gives them; passed [n_events] (may be NULL): 1 = the event is in E (all ones with
 * selected = 0).  Needs attpc_summary_configure and attpc_maps_configure, with selected attpc_select_configure as well
 * (else ATTPC_E_NOTCONFIGURED; a selection mask bit at or above layout->n_sim is then ATTPC_E_INVALID).  A maps run is
 * the resident run: attpc_run_stats keeps its cloud meaning, the id-range rules at the top apply, a pending
 * attpc_sim_hint_next is dropped.  The sizes are known: there is no capacity. */
ATTPC_API int32_t attpc_sim_run_maps(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                     const attpc_event_layout* layout, double* p4, double* vertex, int32_t* kin_status,
                                     attpc_summary_out* records, uint8_t* passed, attpc_maps_out* maps,
                                     attpc_run_stats* stats);
/* The same with kinematics from host arrays p4 [n, n_rows, 4] / vertex [n, 3] (the file-driven flow). */
ATTPC_API int32_t attpc_det_run_maps(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                     const attpc_event_layout* layout, const double* p4, const double* vertex,
                                     attpc_summary_out* records, uint8_t* passed, attpc_maps_out* maps,
                                     attpc_run_stats* stats);
/* The maps of any host cloud through the same kernel, one segment per event: the arguments and checks of
 * attpc_cloud_select (records and passed may be NULL), at most 2^32 - 1 rows. */
ATTPC_API int32_t attpc_cloud_maps(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* points,
                                   const int64_t* labels, const attpc_event_layout* layout, attpc_summary_out* records,
                                   uint8_t* passed, attpc_maps_out* maps);

/* ---- track estimates of the trace rows (opt-in: off by default, and with it off every output, kernel and buffer of
 * every entry point is what it is without this section; the entry points are additions under ABI version 3) ----
 * What Spyral's estimation phase computes for every cluster, made on the device for every simulated nucleus of every
 * event from the event's trace rows, right behind the kernel that writes them: a circle in the pad plane (radius ->
 * B rho), the polar angle from z against the path in the pad plane, the vertex and dE/dx.  Clustering is not needed:
 * a trace row carries the label of the nucleus that made it.  One 128-byte record (attpc_track_estimate) per event and
 * position of layout->indices crosses PCIe, beside the p4 / vertex of the same call, which are the truth.
 * The formulae follow Spyral's estimate_physics in STRUCTURE -- the start at the beam axis, a circle on the first part
 * of the trajectory, the polar angle from z against the cumulated pad-plane distance of consecutive points (zig-zag
 * included), B rho = B R / sin(theta), dE/dx = charge over that length -- but THIS CONTRACT, not Spyral's source, is
 * what the device is tested against (tests/estimate_reference.py restates it in numpy), and the circle is the
 * algebraic (Kasa) least-squares fit in closed form, not Spyral's iterative one ("geometric circle fit" below refines
 * it by an iterative least-squares fit of the geometric distances, opt-in).
 * A "unit" is the quantisation step of the coordinates, 1/16 mm.
 * Settings (attpc_estimate_desc): beam_region_radius in mm, finite and >= 0; min_points >= 3; magnetic_field in T, not
 * NaN; reserved = 0.
 * For event e and position s of layout->indices take the event's trace rows in their delivered order (ascending z)
 * whose label equals indices[s].  A label that occurs twice in indices goes to its FIRST position, as in the summaries;
 * a later position gets the empty record.  Rows of label -1 and of any other label take no part.
 *   1. Quantise.  X = rint(16 x), Y = rint(16 y), Z = rint(16 z) (columns 0, 1, 2 of the row; the product is exact,
 *      rint rounds half to even), I = rint(integral) (column 4): integers.  A row is OUT OF RANGE if any of x, y, z,
 *      integral is not finite, or |x| > 320 mm, |y| > 320 mm, |z| > 8192 mm or |integral| >= 2^31; such a row is not
 *      used and sets the status bit RANGE.  A row is USED iff it is in range and X^2 + Y^2 >= Rb^2 with
 *      Rb = rint(16 beam_region_radius) -- an integer comparison (Rb^2 as a 64-bit integer, Rb clamped to 2^31 - 1).
 *      n_rows = rows of the label, n_used = used rows.
 *   2. Few points.  n_used < min_points: status FEW (EMPTY instead if n_rows == 0), plus RANGE if it was set;
 *      n_fit = 0, direction = 0, charge = 0, arc = 0 and every f64 field NaN.  Nothing else is computed.
 *   3. Direction.  direction = +1 if X^2 + Y^2 of the first used row <= that of the last used row (a tie is +1);
 *      otherwise direction = -1 and the used rows are taken in reverse order.  The end nearer the beam axis is the start.
 *   4. Fit segment: the first m = min(max((n_used + 1) div 2, min_points), 2048) used rows in that order; n_fit = m.
 *      A cut at 2048 sets the status bit CAPPED.
 *   5. Moment sums.  Row 0 of the segment gives (X0, Y0, Z0).  For segment rows i = 0 .. m - 1: u = X - X0,
 *      v = Y - Y0, w = Z - Z0; d_0 = 0 and d_i = rint(sqrt((double)(dX^2 + dY^2))) with (dX, dY) the step from segment
 *      row i - 1 (the radicand is an exact integer below 2^53, the square root correctly rounded, the result an
 *      integer again); S_i = S_(i-1) + d_i.  The 64-bit integer sums over the segment:
 *        Su, Sv, Suu, Suv, Svv, Suuu, Suvv, Svvv, Svuu (of u, v, u u, u v, ..., v u u), SS, Sw, SSS, SSw (of S, w,
 *        S S, S w) and SI (of I).
 *      Bounds: |X|, |Y| <= 5120, so |u|, |v| <= 10240 and d <= 14482; |Z| <= 131072, so |w| <= 262144;
 *      S <= 2047 * 14482 < 3e7.  With m <= 2048: |Suuu| <= 2048 * 10240^3 < 2.2e15, SSS <= 2048 * 9e14 < 1.8e18,
 *      |SSw| <= 2048 * 3e7 * 262144 < 1.7e16, |SI| <= 2^42 -- all inside 2^63 = 9.2e18.  No sum can overflow, so the
 *      sums are exact and independent of any order of summation.
 *   6. Closed form, in f64: the sums and m, X0, Y0, Z0 converted to double (one rounding each), then exactly the
 *      operations below, each rounded once, left to right as C evaluates the expression, no fused multiply-add
 *      (#pragma clang fp contract(off)); only + - * / and sqrt.  Trigonometric functions stay on the host.
 *        A = m Suu - Su Su;  B = m Suv - Su Sv;  C = m Svv - Sv Sv
 *        D = (m (Suvv + Suuu) - Su (Suu + Svv)) / 2;  E = (m (Svuu + Svvv) - Sv (Suu + Svv)) / 2
 *        den = A C - B B;  uc = (D C - B E) / den;  vc = (A E - B D) / den
 *        r2 = (Suu + Svv - 2 uc Su - 2 vc Sv) / m + uc uc + vc vc
 *      den == 0 or not r2 > 0: status NO_CIRCLE; cx, cy, radius, vx, vy, vz and brho are NaN.  Otherwise
 *        cx = (X0 + uc) / 16;  cy = (Y0 + vc) / 16;  radius = sqrt(r2) / 16                       (mm)
 *      Vertex in the plane, the circle's point nearest the z axis: c = sqrt(cx cx + cy cy);
 *        vx = cx (1 - radius / c);  vy = cy (1 - radius / c)
 *      c == 0: status ON_AXIS; vx, vy, vz are NaN.
 *      Slope of z against the path: sden = m SSS - SS SS; sden == 0: status NO_SLOPE; slope, vz and brho are NaN.  Else
 *        slope = b = (m SSw - SS Sw) / sden     (signed along the direction of travel: a backward track has b < 0)
 *      Vertex z, the regression's value at S = 0 carried back by the chord from segment row 0 to the vertex:
 *        a0 = (Sw - b SS) / m;  gx = X0 - 16 vx;  gy = Y0 - 16 vy;  chord0 = sqrt(gx gx + gy gy)
 *        vz = (Z0 + a0 - b chord0) / 16
 *      x_mean = (X0 + Su / m) / 16, y_mean = (Y0 + Sv / m) / 16 (the host takes the azimuth from the chord vertex ->
 *      segment mean); arc = S_(m-1) (int64, units); charge = SI (int64);
 *        dedx = charge / (arc / 16), NaN at arc == 0
 *        brho = magnetic_field radius 1e-3 sqrt(1 + b b)  (T m: B R / sin(theta) with cot(theta) = b)
 * An event that a trigger gate left without rows has EMPTY records.  Every field is a pure function of the event's
 * rows, hence of (seed, global event id): independent of chunking, shards and scatter build. */
#define ATTPC_EST_EMPTY 1      /* no row of the label (or a later position of a label given twice) */
#define ATTPC_EST_FEW 2        /* n_used < min_points */
#define ATTPC_EST_RANGE 4      /* a row of the label was out of range and not used */
#define ATTPC_EST_CAPPED 8     /* the fit segment was cut at 2048 rows */
#define ATTPC_EST_NO_CIRCLE 16
#define ATTPC_EST_ON_AXIS 32
#define ATTPC_EST_NO_SLOPE 64
#define ATTPC_EST_MAX_FIT 2048

typedef struct attpc_estimate_desc {
  double beam_region_radius;  /* mm, finite and >= 0; Spyral's default is 25 */
  double magnetic_field;      /* T */
  int32_t min_points;         /* >= 3; Spyral's default is 30 */
  int32_t reserved;           /* 0 */
} attpc_estimate_desc;

typedef struct attpc_track_estimate {
  int32_t n_rows;
  int32_t n_used;
  int32_t n_fit;
  int32_t status;     /* ATTPC_EST_* bits */
  int32_t direction;  /* +1, -1, or 0 without a fit */
  int32_t reserved;   /* 0; with the geometric circle fit on: its evaluations */
  int64_t charge;
  int64_t arc;
  double cx, cy, radius;
  double vx, vy, vz;
  double slope;
  double x_mean, y_mean;
  double dedx;
  double brho;
} attpc_track_estimate;  /* 128 bytes */

/* desc == NULL turns the stage off (the default).  Independent of every other configure call: no call resets another.
 * ATTPC_E_INVALID outside the ranges above, NaN included.  Takes effect in attpc_sim_run_trace_rows and
 * attpc_det_run_trace_rows: every chunk's records are made right behind the kernel that writes its rows, on the same
 * stream, and copied to pinned host memory in the call's event order -- also when the rows stay on the device (points
 * and labels NULL).  attpc_trace_rows_at takes no layout, so it makes no records (attpc_estimates_last then answers
 * ATTPC_E_NOTCONFIGURED); attpc_rows_estimate on its rows gives them. */
ATTPC_API int32_t attpc_trace_configure_estimates(attpc_ctx* ctx, const attpc_estimate_desc* desc);
/* Records [count][layout->n_sim] of events first .. first + count - 1 of the context's last trace-row call, in the
 * call's event order (a call repeated after ATTPC_E_CAPACITY overwrites them).  ATTPC_E_NOTCONFIGURED if the stage was
 * off for that call, ATTPC_E_INVALID for a range outside it.  A trace or trace-row call that is refused at its start
 * leaves nothing to read: every attpc_*_last reader of the records that call would have replaced (for a trace call
 * attpc_trigger_last alone) answers ATTPC_E_NOTCONFIGURED until the next such call that succeeds. */
ATTPC_API int32_t attpc_estimates_last(attpc_ctx* ctx, int64_t first, int64_t count, attpc_track_estimate* out);
/* The stage alone on any host rows in CSR form, through the same kernel (what attpc_trigger_rows is to the trigger):
 * offsets [n_events + 1], rows [R][8] as the trace-row and Spyral-row entry points deliver them, labels [R] -> out
 * [n_events][layout->n_sim]; of the layout only n_sim and indices are read.  Needs no other configure call and leaves
 * the configured stage as it is.  ATTPC_E_INVALID for decreasing offsets, n_sim outside 0 .. ATTPC_MAX_SIM or a desc
 * out of range. */
ATTPC_API int32_t attpc_rows_estimate(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows,
                                      const int64_t* labels, const attpc_event_layout* layout,
                                      const attpc_estimate_desc* desc, attpc_track_estimate* out);

/* ---- thinned track points (opt-in: off by default, and with it off every output, kernel and buffer of every entry
 * point is what it is without this section; the entry points are additions under ABI version 3) ----
 * A track lights several neighbouring pads at every z, so its labelled trace rows form a band, not a line: the
 * cumulated pad-plane distance of the estimates zig-zags across it and their unweighted circle shrinks.  Thinning
 * reduces every track's rows to ONE charge-weighted centroid per z bin, on the device and in exact integer arithmetic,
 * in front of the estimates.  tests/thin_reference.py restates this contract in numpy.  A "unit" is 1/16 mm, as above.
 * Settings (attpc_thin_desc): z_step in mm, finite, 1/16 <= z_step <= 512; reserved = pad = 0.
 * H = rint(16 z_step), an integer in 1 .. 8192.
 * For event e and position s of layout->indices the event's rows in their delivered order whose label equals
 * indices[s] take part.  A label given twice goes to its FIRST position only; label -1 and labels that are not in
 * indices take no part.
 *   1. Quantise exactly as step 1 of the estimates (the same code): X, Y, Z, I.  A row that is out of range there is
 *      DROPPED and counted in n_dropped.
 *   2. bin = floor(Z / H) (floor also for negative Z: -1 / H is bin -1), weight w = max(I, 1).
 *   3. A POINT is a maximal run of consecutive participating rows (the dropped ones taken out) of equal bin.  Delivered
 *      rows are in ascending z, so a bin's rows are one run; the rule is on consecutive rows and assumes no order:
 *      unsorted rows simply make more points.  A run is cut after 4096 rows: if the next participating row has the same
 *      bin it starts a new point (a SPLIT), the point in front of it has column 7 = 1, and every point that ends or
 *      begins at a split counts once in n_split (a bin of 4097 rows: 2, of 8193 rows: 3).  A run of exactly 4096 rows
 *      that a change of bin ends is no split.
 *   4. Sums of a point, 64-bit integers: W = sum w, Sx = sum w X, Sy = sum w Y, Sz = sum w Z, SI = sum I, n = rows;
 *      amplitude = fmax over column 3 of its rows, NaN ignored (NaN if every one is).
 *   5. Bounds: w < 2^31, |X|, |Y| <= 5120, |Z| <= 2^17 and n <= 4096, so |Sz| < 2^31 2^17 2^12 = 2^60 (|Sx|, |Sy| less),
 *      |2 Sz + W| < 2^62 and 0 < W < 2^43, |SI| < 2^43.  Nothing can overflow: the sums are exact and independent of the
 *      order of summation.
 *   6. Centroid, integers only: C(S) = floor_div(2 S + W, 2 W) -- S / W to the nearest integer, a tie upwards, floor
 *      semantics for a negative numerator.  The point is (C(Sx), C(Sy), C(Sz), SI); |C(Sx)| <= 5120, |C(Sz)| <= 2^17.
 * Point row [8]: x = C(Sx) / 16, y = C(Sy) / 16, z = C(Sz) / 16 (exact), amplitude, SI, n, bin, 1 if a split closed it
 * else 0.  Such rows are valid input of attpc_rows_estimate as they are (quantising them gives C(Sx), C(Sy), C(Sz) and
 * SI back; a point with |SI| >= 2^31 is out of range by the rule there), and the fused stage is DEFINED by that:
 * with thinning and the estimates both on, the records of attpc_estimates_last are exactly the records the estimate
 * contract gives on the event's point rows with their labels -- n_rows counts the label's points, n_used the used
 * points, min_points counts points -- with ATTPC_EST_RANGE OR-ed in if thinning dropped a row of the label. */
typedef struct attpc_thin_desc {
  double z_step;     /* mm, 1/16 .. 512 */
  int32_t reserved;  /* 0 */
  int32_t pad;       /* 0 */
} attpc_thin_desc;

typedef struct attpc_thin_info {
  int32_t n_rows;     /* rows of the label, dropped ones included */
  int32_t n_points;
  int32_t n_dropped;
  int32_t n_split;
} attpc_thin_info;  /* 16 bytes */

#define ATTPC_THIN_MAX_RUN 4096

/* desc == NULL turns the stage off (the default).  Independent of every other configure call.  ATTPC_E_INVALID outside
 * the ranges above, NaN included.  Takes effect only in the trace-row calls in which the estimates are on: every chunk's
 * rows are then thinned right behind the kernel that writes them and the estimates are made of the points.  Alone it is
 * inert: no kernel, no buffer.  The trace rows, labels, offsets and checksums of the call do not change. */
ATTPC_API int32_t attpc_trace_configure_thinning(attpc_ctx* ctx, const attpc_thin_desc* desc);
/* The stage alone on any host rows in CSR form, through the same kernel: offsets [n_events + 1], rows [R][8], labels
 * [R] -> point_offsets [n_events + 1], points [P][8], point_labels [P] (= indices[s]) and info [n_events][n_sim].  Per
 * event the points come position-major (s ascending) and in run order inside a position.  P <= R always, so capacity
 * = R cannot fail; capacity < P gives ATTPC_E_CAPACITY with *needed = P (point_offsets and info are complete then, the
 * points are not).  Needs no other configure call and leaves the configured stage as it is.  ATTPC_E_INVALID as
 * attpc_rows_estimate. */
ATTPC_API int32_t attpc_rows_thin(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows,
                                  const int64_t* labels, const attpc_event_layout* layout, const attpc_thin_desc* desc,
                                  int64_t capacity, int64_t* point_offsets, double* points, int64_t* point_labels,
                                  attpc_thin_info* info, int64_t* needed);

/* ---- geometric circle fit (opt-in: off by default, and with it off every output, kernel and buffer of every entry
 * point is what it is without this section; the entry points are additions under ABI version 3) ----
 * The Kasa circle of step 6 of the estimates minimises an algebraic distance, which pulls the radius low on a short
 * noisy arc.  With this stage on, the (cx, cy, radius) of step 6 are refined by a least-squares fit of the GEOMETRIC
 * distances of the fit segment's points to the circle (Levenberg-Marquardt, started from the Kasa circle), and all that
 * step 6 derives from the circle (vx, vy, vz, brho) is made from the refined circle by the same formulae.  Unweighted;
 * Spyral's ODE fit it is not.  tests/circle_reference.py restates this contract in numpy; csrc/circle_host.hpp is its
 * arithmetic, shared by the kernel and the host.  A "unit" is 1/16 mm, as above.
 * Settings (attpc_circle_desc): tolerance in units, finite and > 0 (default 2^-7); max_evaluations in 2 .. 64 (default
 * 32); reserved = 0.
 * When: only if step 6 found a Kasa circle (den != 0 and r2 > 0).  NO_CIRCLE stays NO_CIRCLE, nothing is refined and
 * reserved stays 0.  The start is p = (a, b, R) = (uc, vc, sqrt(r2)) of step 6: units, relative to (X0, Y0).
 * All arithmetic is f64, one rounding per operation, no fused multiply-add, only + - * / and sqrt, as step 6.
 *   One EVALUATION at p = (a, b, R).  For segment rank i = 0 .. m - 1 with the integers u_i, v_i of step 5:
 *       dx = u - a;  dy = v - b;  r = sqrt(dx dx + dy dy);  U = dx / r;  V = dy / r  (r == 0: U = V = 0);  g = r - R
 *     and the nine sums F = sum g g, SUU = sum U U, SUV = sum U V, SVV = sum V V, SU = sum U, SV = sum V,
 *     SgU = sum g U, SgV = sum g V, Sg = sum g.
 *     The ORDER OF SUMMATION is part of the contract (these sums are not integers): rank i belongs to lane i mod 64; a
 *     lane adds its terms in ascending i onto +0.0 (a lane without a term holds +0.0); the 64 lane values are then
 *     combined by s[lane] <- s[lane] + s[lane xor off] for off = 32, 16, 8, 4, 2, 1, all lanes at once.  Addition is
 *     commutative, so every lane ends with the same bits: that value is the sum.
 *   The STEP at p with the sums of p and the damping lambda, by this one elimination (M = double(m)):
 *       m00 = SUU + lambda SUU;  m11 = SVV + lambda SVV;  m22 = M + lambda M
 *       l10 = SUV / m00;  l20 = SU / m00
 *       a11 = m11 - l10 SUV;  a12 = SV - l10 SU;  b1 = SgV - l10 SgU
 *       a22 = m22 - l20 SU;   b2 = Sg - l20 SgU
 *       l21 = a12 / a11;  c22 = a22 - l21 a12;  c2 = b2 - l21 b1
 *       d2 = c2 / c22;  d1 = (b1 - a12 d2) / a11;  d0 = (SgU - SUV d1 - SU d2) / m00
 *     -- (N + lambda diag N) d = (SgU, SgV, Sg) with N = [[SUU, SUV, SU], [SUV, SVV, SV], [SU, SV, M]], no pivoting.
 *   ITERATION.  lambda = 2^-10; evaluate at the start (evaluation 1).  Then repeat:
 *       if the evaluations made == max_evaluations: stop with the status bit NOT_CONVERGED
 *       d = the step at p;  p' = (a + d0, b + d1, R + d2);  evaluate at p'
 *       accepted = F' <= F and R' > 0   (a NaN anywhere fails one of the two comparisons: rejected)
 *       accepted: p = p' with its sums, lambda = 0.04 lambda, and if max(|d0|, |d1|, |d2|) <= tolerance stop, converged
 *       rejected: lambda = 10 lambda
 *     So a converged fit has made 2 .. max_evaluations evaluations, and the p of the record is the last accepted one
 *     (the start if none was).
 * Record: reserved = the evaluations made (>= 1 where the refinement ran, 0 everywhere else -- also in every record
 * made with the stage off); status gets ATTPC_EST_NOT_CONVERGED where the iteration stopped unconverged;
 *   cx = (X0 + a) / 16;  cy = (Y0 + b) / 16;  radius = R / 16
 * and c, vx, vy, ON_AXIS, chord0, vz and brho follow from these as in step 6.  slope, x_mean, y_mean, dedx, charge, arc
 * and the counts do not depend on the circle.  (A fit that makes no accepted step leaves exactly the Kasa record, plus
 * reserved and the bit.)
 * A record stays a pure function of the event's rows; with thinning on, the fused records are still DEFINED as this
 * contract on the event's point rows. */
#define ATTPC_EST_NOT_CONVERGED 128  /* the geometric circle fit spent max_evaluations evaluations */
#define ATTPC_CIRCLE_MIN_EVALUATIONS 2
#define ATTPC_CIRCLE_MAX_EVALUATIONS 64

typedef struct attpc_circle_desc {
  double tolerance;         /* units (1/16 mm), finite and > 0; default 2^-7 = 0.0078125 */
  int32_t max_evaluations;  /* 2 .. 64; default 32 */
  int32_t reserved;         /* 0 */
} attpc_circle_desc;

/* desc == NULL turns the stage off (the default).  Independent of every other configure call.  ATTPC_E_INVALID outside
 * the ranges above, NaN included.  Takes effect only in the trace-row calls in which the estimates are on, with or
 * without thinning: the estimate kernel that runs is then its refining instantiation.  Alone it is inert: no kernel, no
 * buffer.  The trace rows, labels, offsets and checksums of the call do not change. */
ATTPC_API int32_t attpc_trace_configure_circle(attpc_ctx* ctx, const attpc_circle_desc* desc);
/* attpc_rows_estimate with the geometric circle fit of `circle` (not NULL), through the refining kernel.  Errors as
 * attpc_rows_estimate, and ATTPC_E_INVALID for a circle desc out of range. */
ATTPC_API int32_t attpc_rows_estimate_circle(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows,
                                             const int64_t* labels, const attpc_event_layout* layout,
                                             const attpc_estimate_desc* desc, const attpc_circle_desc* circle,
                                             attpc_track_estimate* out);

/* ---- helix slope (opt-in: off by default, and with it off every output, kernel and buffer of every entry point is what
 * it is without this section; the entry points are additions under ABI version 3) ----
 * The slope of step 6 is the regression of z against the cumulated pad-plane distance between consecutive points.
 * Every bit of lateral scatter lengthens that zig-zag path, so cot(theta) comes out low and the polar angle is pulled
 * towards pi/2, most for stiff forward tracks.  With this stage on, a point's progress is its TURNING ANGLE about the
 * centre of the record's circle instead -- the radial scatter drops out of the path -- and slope, vz and brho are made
 * from the regression of z against that angle.  tests/helix_reference.py restates this contract in numpy;
 * csrc/helix_host.hpp is its arithmetic, shared by the kernel and the host.  A "unit" is 1/16 mm, as above.
 * Settings (attpc_helix_desc): regressor 0 = auto, 1 = z against the path, 2 = the path against z; reserved = 0.
 * When: only in a record that has a circle (no NO_CIRCLE; Kasa or refined, an unconverged refined one included), on the
 * circle the record carries: centre (a, b) and radius R in units relative to (X0, Y0).  A NO_CIRCLE record gets
 * NO_HELIX too and is otherwise unchanged; EMPTY and FEW records are untouched and get no NO_HELIX.
 *   1. Turning angle.  For segment rank i = 0 .. m - 1 with the integers u_i, v_i, w_i of step 5, in f64:
 *        px = u - a;  py = v - b;  p0 = (-a, -b), rank 0's;  cr = p0x py - p0y px;  dt = p0x px + p0y py
 *        phi_q = (int) rint(65536 atan2w(cr, dt)), an integer in -205887 .. 205887
 *      atan2w(y, x) is WRITTEN arithmetic: + - * / only, one rounding per operation, no fused multiply-add:
 *        ax = |x|;  ay = |y|;  hi = the larger, lo = the smaller;  hi == 0: the result is 0;  t = lo / hi
 *        t > 0.41421356237309503: r = (t - 1) / (t + 1), base = pi/4;  otherwise r = t, base = 0;  z = r r
 *        p = c_19;  p = p z + c_k for k = 18 .. 0, c_k = (-1)^k / (2 k + 1) as f64 (the 20 Taylor coefficients)
 *        at = base + r p;  if ay > ax: at = pi/2 - at;  then if x < 0: at = pi - at;  then if y < 0: at = -at
 *      with pi = 3.141592653589793, pi/2 = 1.5707963267948966, pi/4 = 0.7853981633974483 and plain comparisons (-0.0 is
 *      not negative).  |r| < 0.4143, so the truncation is below 5e-18; against the C library the result differs by at
 *      most 4.44e-16 (2 ulp of pi, observed on 3e6 inputs) and rint(65536 .) of the two never.  An angle that is not a
 *      number (a circle so large that the products overflow) gives NO_HELIX.
 *   2. Unwrap, integers only.  K_0 = 0; for i >= 1 with D = phi_q_i - phi_q_(i-1): j_i = -1 if D > 205887, +1 if
 *      D < -205887, else 0; K_i = K_(i-1) + j_i; PHI_i = phi_q_i + 411775 K_i  (411775 = rint(2 pi 65536),
 *      205887 = rint(pi 65536)).  Any |PHI_i| >= 2^24 (about 40 turns): NO_HELIX.
 *   3. Sums, 64-bit integers: SP = sum PHI, SPP = sum PHI PHI, SPw = sum PHI w, Sww = sum w w; Sw and m are step 5's.
 *      Bounds: |PHI| < 2^24, |w| <= 2^18 and m <= 2^11, so SPP < 2^11 2^48 = 2^59, |SPw| < 2^11 2^24 2^18 = 2^53 and
 *      Sww <= 2^11 2^36 = 2^47 -- inside 2^63 (in a record past the cap the sums are not used; an implementation lets
 *      such an angle add nothing).  Nothing can overflow: the sums are exact and independent of any order of summation.
 *   4. Closed form, f64: the sums converted once each, then exactly these operations, left to right, no fused
 *      multiply-add, + - * / and sqrt only.  M = (double) m.
 *        vp = M SPP - SP SP;  vw = M Sww - Sw Sw;  cv = M SPw - SP Sw
 *      vp == 0 (no angular spread; a first point at the centre ends here): NO_HELIX.
 *      B ("the path against z") holds with regressor 2; with regressor 0 iff vw 4294967296.0 >= vp R R and cv != 0 (the
 *      regressor is the coordinate with the larger spread); not with regressor 1.
 *        q = vw / cv with B (cv == 0: NO_HELIX), else q = cv / vp;  q not finite: NO_HELIX
 *        sg = +1 if SP >= 0 else -1;  slope = b = (sg 65536.0 q) / R   (dz/ds along the direction of travel: a backward
 *                                                                        track has b < 0, as in step 6)
 *        a0 = (Sw - q SP) / M;  pv = (-(X0 + a), -(Y0 + b_centre))
 *        Pv = rint(65536 atan2w(p0x pvy - p0y pvx, p0x pvx + p0y pvy))  (a double, not unwrapped)
 *        vz = (Z0 + a0 + q Pv) / 16   (NaN with ON_AXIS, as in step 6)
 *        brho = magnetic_field radius 1e-3 sqrt(1 + b b)
 * With NO_HELIX the record is exactly the one the stage-off contract gives, plus the bit.  Otherwise only slope, vz,
 * brho and the status change: a NO_SLOPE bit of step 6 is cleared.  The counts, arc, charge, dedx, the circle, vx, vy,
 * x_mean, y_mean and reserved do not change.  A record stays a pure function of the event's rows; with thinning on, the
 * fused records are still DEFINED as this contract on the event's point rows. */
#define ATTPC_EST_NO_HELIX 256   /* the stage was on and could not run; the record is step 6's */
#define ATTPC_HELIX_AUTO 0
#define ATTPC_HELIX_Z_ON_PATH 1
#define ATTPC_HELIX_PATH_ON_Z 2

typedef struct attpc_helix_desc {
  int32_t regressor;  /* 0 = auto, 1 = z against the path, 2 = the path against z */
  int32_t reserved;   /* 0 */
} attpc_helix_desc;

/* desc == NULL turns the stage off (the default).  Independent of every other configure call.  ATTPC_E_INVALID for a
 * regressor outside 0 .. 2 or a non-zero reserved.  Takes effect only in the trace-row calls in which the estimates are
 * on, on raw rows and on thinned points, behind the Kasa circle and behind the geometric circle fit: the estimate kernel
 * that runs is then its instantiation with one more pass.  Alone it is inert: no kernel, no buffer.  The trace rows,
 * labels, offsets and checksums of the call do not change. */
ATTPC_API int32_t attpc_trace_configure_helix(attpc_ctx* ctx, const attpc_helix_desc* desc);
/* attpc_rows_estimate_circle with the helix slope of `helix` (not NULL) behind the circle; `circle` may be NULL: the
 * Kasa circle then.  Errors as attpc_rows_estimate_circle, and ATTPC_E_INVALID for a helix desc out of range. */
ATTPC_API int32_t attpc_rows_estimate_helix(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows,
                                            const int64_t* labels, const attpc_event_layout* layout,
                                            const attpc_estimate_desc* desc, const attpc_circle_desc* circle,
                                            const attpc_helix_desc* helix, attpc_track_estimate* out);

/* ---- track straggling (opt-in: off by default, and with it off every output, kernel and buffer of every entry point
 * is what it is without this section; the entry point is an addition under ABI version 3) ----
 * The track integrator solves a deterministic equation of motion, so two particles of one momentum follow one path.
 * This stage adds multiple Coulomb scattering and energy-loss straggling to every recorded sample of every track.
 * tests/straggle_reference.py restates this contract in numpy; csrc/straggle_host.hpp is its arithmetic, shared by
 * the kernel and the host, + - * / and sqrt only with every operation rounded (no fused multiply-add).
 *
 * The model, and what it is not: first order, Gaussian per step.  No single-scattering tail, no Landau tail; Bohr's
 * variance is too large at low velocity.  The two scales exist so that a user can fit the lateral and the range
 * straggling of their own SRIM or LISE tables.
 *
 * Where: after the RK4 sub-steps of recorded sample k (1 .. 10 000) have been accepted and before the electrons of
 * that sample are made.  g = gamma beta after the step, m and Z the species' mass [MeV] and charge number.
 * Step length: ds = c * sqrt(gv2 / (1 + gv2)) * h_sample, gv2 = |gamma beta|^2 of the state at the PREVIOUS recorded
 * sample (after that sample's own kick), h_sample = 1e-10 s on the time grid and the path-length mode's own step
 * otherwise.
 * Angular kick (Rossi-Greisen, without Highland's logarithm: the variances of consecutive steps add and the result
 * does not depend on the step length), skipped if angular_scale == 0:
 *   theta0 = angular_scale * (13.6 MeV * |Z| / (beta p)) * sqrt(ds / X0), p = m |g|, beta = |g| / sqrt(1 + |g|^2)
 *   u = g / |g|;  sign = copysign(1, u_z), a = -1 / (sign + u_z), b = u_x u_y a (Duff et al., JCGT 6(1), 2017)
 *   e1 = (1 + sign u_x^2 a, sign b, -sign u_x),  e2 = (b, sign + u_y^2 a, -u_y)
 *   d = u + theta0 n1 e1 + theta0 n2 e2;  the new direction is d / |d|  (else: u)
 * Energy fluctuation (Bohr, Gaussian), skipped if energy_scale == 0:
 *   KE = m |g|^2 / (gamma + 1)   (= m (gamma - 1)),  gamma^2 = 1 + |g|^2
 *   Omega^2 = energy_scale^2 * K * Z^2 * n_e * ds * gamma^2 * (1 - beta^2 / 2),  K = 4 pi (r_e m_e c^2)^2 =
 *             2.605634303273153e-29 MeV^2 m^2 (CODATA)
 *   KE' = max(KE - Omega n3, KE_LIMIT);  |g'|^2 = (KE' / m) (KE' / m + 2)   (else: |g'| = |g|)
 *   Unclamped on the high side on purpose: a step may "lose" a negative amount, the mean loss stays the table's.
 * g' = |g'| * direction.  A skipped part uses no draw and keeps the direction u / the magnitude |g| bit for bit; with
 * both scales 0 the stage is off.  Then the event functions and the sample's electrons are those of g' (the electrons
 * come from |KE(g') - KE(previous sample)| as always).  A sample whose energy was clamped sits AT the limit: its "ke"
 * event function is exactly 0, and the next step ends the track through the ordinary "ke" event.
 * Random numbers: (n1, n2) are the Box-Muller (cos, sin) normals of the Philox pair (seed, event, 2 k, D), n3 the cos
 * normal of the pair (seed, event, 2 k + 1, D), D = 0x10000000 + stream * 32 + row of the nucleus (row < 32).  A track
 * is a pure function of (seed, global event id, row, stream): chunking, lanes and the number of GPUs do not enter. */
typedef struct {
  double angular_scale;     /* >= 0; 0 = no angular kick */
  double energy_scale;      /* >= 0; 0 = no energy fluctuation */
  double radiation_length;  /* X0 of the gas at its density, m, > 0 */
  double electron_density;  /* electrons per m^3, > 0 */
  uint32_t stream;          /* < 2^16 */
} attpc_straggle_desc;

/* desc == NULL turns the stage off (the default).  ATTPC_E_INVALID for a value that is not finite, a negative scale,
 * X0 or n_e <= 0 or stream >= 2^16.  The descriptor is kept on the context, independent of every other configure call
 * (attpc_det_configure does not drop it), and every entry point that integrates tracks uses it: attpc_det_tracks,
 * attpc_det_run* and attpc_sim_run* in all their forms, and the batch attpc_sim_hint_next starts early.  With both
 * scales 0 the kernels that run are those of the stage off. */
ATTPC_API int32_t attpc_det_configure_straggling(attpc_ctx* ctx, const attpc_straggle_desc* desc);

/* ---- drift distortion (opt-in: off by default, and with it off every output, kernel and buffer of every entry point
 * is what it is without this section; the entry points are additions under ABI version 3) ----
 * The engine's drift field is ideal: an electron made at (x, y, z) lands at (x, y) on the pad plane at time bucket
 * (length - z) / dv + micromegas_edge.  A real field cage and space charge give E a radial component; with B parallel
 * to E the drifting electrons are pushed radially and, through E x B, azimuthally, and they arrive at a shifted time.
 * This stage moves every kept track record (x m, y m, time bucket, electrons x gain) by a map of those three shifts
 * over (creation radius, ideal drift time), before anything reads the records.  tests/distortion_reference.py restates
 * this contract in numpy; csrc/distort_host.hpp is its arithmetic, shared by the kernel and the host.
 *
 * The map.  Node (i, j) stands for creation radius rho = i * rho_step and ideal drift tau = tb - tb_origin =
 * j * tau_step.  Every table value is finite, |radial| and |azimuthal| <= 1 m, |time| <= 1024 time buckets: the caps
 * keep a shifted record inside what the scatter is built to take.
 *
 * One record (x, y, tb, q), in f64, every operation rounded once in the written order (no fused multiply-add), + - * /
 * and sqrt only:
 *  1. rho = sqrt(x * x + y * y), tau = tb - tb_origin.  A record whose x, y or tb is not finite keeps its bits.
 *  2. a = rho / rho_step clamped to [0, n_rho - 1] by plain comparisons; i = min((int) floor(a), n_rho - 2),
 *     fr = a - i.  b = tau / tau_step, clamped to [0, n_tau - 1], gives j and fs the same way.  Outside the grid the
 *     edge value holds.
 *  3. for each table T: lo = T[i][j] + fs * (T[i][j+1] - T[i][j]), hi = T[i+1][j] + fs * (T[i+1][j+1] - T[i+1][j]),
 *     v = lo + fr * (hi - lo): dr, da, dt (a NULL table gives 0).
 *  4. ux = x / rho, uy = y / rho (rho == 0: both 0 -- no direction, no shift in the plane);
 *     x' = (x + dr * ux) - da * uy,  y' = (y + dr * uy) + da * ux,  tb' = tb + dt,  q' = q bit for bit.
 * A record is a pure function of itself and the map: no random draw, no dependence on event id, chunking or shard.
 *
 * Who sees it.  Every entry point that integrates tracks: attpc_sim_run* and attpc_det_run* in all their forms (the
 * batch attpc_sim_hint_next starts early included) and attpc_det_tracks, which returns the shifted records.
 * attpc_det_scatter takes records as given and does not apply it.  The shift is applied exactly once per track batch,
 * however often the batch is scattered (chunks, a launch repeated with larger buffers, a call repeated after
 * ATTPC_E_CAPACITY).  The diffusion widths of a record are those of its shifted arrival time, as for any record, and a
 * record shifted out of the time buckets 0 .. 511 is dropped by the scatter like any other.  The end point of a track
 * summary (end_x, end_y, end_tb) and a selection on it are those of the shifted, apparent record; counts, n_steps,
 * n_track_samples and whether the arena overflowed do not change. */
typedef struct attpc_distort_desc {
  double rho_step;          /* m, finite, > 0 */
  double tau_step;          /* time buckets, finite, > 0 */
  double tb_origin;         /* the time bucket of drift distance 0 (the config's micromegas_edge), finite */
  int32_t n_rho, n_tau;     /* 2 .. 256 each */
  const double* radial;     /* [n_rho][n_tau] m, + = outward;                 NULL = zeros */
  const double* azimuthal;  /* [n_rho][n_tau] m of arc, + = counter-clockwise; NULL = zeros */
  const double* time;       /* [n_rho][n_tau] time buckets, + = later;        NULL = zeros */
} attpc_distort_desc;

/* desc == NULL turns the stage off (the default), and so does a desc whose three tables are all NULL or all zero: no
 * kernel is launched then.  ATTPC_E_INVALID for anything the section above rules out, a NaN in any field included.
 * The library copies the tables to the device and owns the copies.  The map is kept on the context, independent of
 * every other configure call (attpc_det_configure does not drop it); the call drops a track batch queued ahead. */
ATTPC_API int32_t attpc_det_configure_distortion(attpc_ctx* ctx, const attpc_distort_desc* desc);

/* The stage alone: out[k] = the shifted record of samples[k] ([n][4] each: x, y, tb, q), by the same kernel on the
 * array presented as chains of arena blocks.  Any n >= 0 (n == 0: nothing is read or written); desc as above and not
 * NULL (an all-zero map copies the records).  Needs no other configure call and leaves the configured stage as it is.
 * out may be samples. */
ATTPC_API int32_t attpc_samples_distort(attpc_ctx* ctx, int64_t n, const double* samples, const attpc_distort_desc* desc,
                                        double* out);

/* ---- drift correction (opt-in: off by default, and with it off every output, kernel and buffer of every entry point
 * is what it is without this section; the entry points are additions under ABI version 3) ----
 * The way back from the drift distortion, on the trace rows: every row of a chunk is taken from its apparent place
 * (x, y, time) to where its electrons were made, by fixed-point iteration on the forward map of the section above, and
 * the rows of every event are sorted again, because a map with a time table changes z and with it the order that the
 * thinning and the estimates rely on.  The stage sits between the kernel that writes a chunk's trace rows and everything
 * that reads them: thinning, estimates, delivery.  tests/undistort_reference.py restates this contract in numpy;
 * csrc/undistort_host.hpp is the arithmetic of one row, shared by the kernel and the host.
 *
 * Settings (attpc_undistort_desc): map, an attpc_distort_desc under the rules of attpc_det_configure_distortion -- the
 * caller's correction map, which need not be the map the tracks were distorted with; windows_edge > micromegas_edge;
 * length in m, finite and > 0; iterations in 1 .. 64; tolerance_xy in m and tolerance_tb in time buckets, each finite
 * and >= 0.
 *
 * One row (8 doubles), in f64, every operation rounded once in the written order (no fused multiply-add), + - * / and
 * sqrt only:
 *  1. Observed point: sx = row[0] / 1000.0, sy = row[1] / 1000.0, st = row[6] (the centroid in time buckets, which is
 *     exact; the time is not taken back from z).
 *  2. A row whose row[0], row[1] or row[6] is not finite keeps all its bits and is SKIPPED (n_skipped).
 *  3. Estimate (x, y, t) = (sx, sy, st).  `iterations` times: (fx, fy, ft) = the shifted record of (x, y, t) by the map
 *     (steps 1 .. 4 of "drift distortion"); dx = fx - sx, dy = fy - sy, dt = ft - st; x = x - dx, y = y - dy,
 *     t = t - dt.
 *  4. The row is UNCONVERGED iff on the last repetition |dx| > tolerance_xy or |dy| > tolerance_xy or
 *     |dt| > tolerance_tb.  (The estimate cannot run away: x - dx is sx minus a shift, and a shift is at most 1 m.)
 *  5. Output row: [0] = x * 1000.0, [1] = y * 1000.0, [2] = ((windows_edge - t) / (windows_edge - micromegas_edge))
 *     * length * 1000.0 with the division correctly rounded -- the expression of the trace rows' own z, so that a map
 *     that shifts nothing gives z back bit for bit.  Columns 3 .. 7 keep their bits; column 6 stays the observed time.
 *  6. Order: within an event the output rows stand in descending corrected t (ascending corrected z), equal t in input
 *     order (stable), the skipped rows behind every corrected row in input order.  Labels move with their rows, the
 *     offsets do not change.  n_moved counts the rows whose position changed.
 * Rows and counts are pure functions of the input rows and the settings: no random draw, no dependence on event id,
 * chunking or shard. */
typedef struct attpc_undistort_desc {
  attpc_distort_desc map;
  int32_t windows_edge;
  int32_t micromegas_edge;  /* < windows_edge */
  double length;            /* m, finite, > 0 */
  int32_t iterations;       /* 1 .. 64 (four bytes of padding follow) */
  double tolerance_xy;      /* m, finite, >= 0 */
  double tolerance_tb;      /* time buckets, finite, >= 0 */
} attpc_undistort_desc;

typedef struct attpc_undistort_info {
  int64_t n_rows;         /* rows seen, skipped ones included */
  int64_t n_skipped;
  int64_t n_unconverged;
  int64_t n_moved;
} attpc_undistort_info;  /* 32 bytes */

/* desc == NULL turns the stage off (the default), and so does a desc whose map shifts nothing: no kernel is launched
 * and no buffer is held then.  ATTPC_E_INVALID for anything the section above rules out, a NaN in any field included.
 * The library copies the tables to the device and owns the copies.  Independent of every other configure call.  With
 * the stage on attpc_sim_run_trace_rows, attpc_det_run_trace_rows and attpc_trace_rows_at deliver the corrected,
 * re-sorted rows and labels, and the thinning and the estimates read them; offsets, event_points and the row checksum
 * (whose terms are event, pad and sample) do not change.  It costs a second row and label buffer per chunk set, 72
 * bytes of device memory per row. */
ATTPC_API int32_t attpc_trace_configure_correction(attpc_ctx* ctx, const attpc_undistort_desc* desc);
/* The counts of the context's last trace-row call, every event counted exactly once however the call was chunked;
 * ATTPC_E_NOTCONFIGURED if the stage was off for it (or there was none). */
ATTPC_API int32_t attpc_correction_last(attpc_ctx* ctx, attpc_undistort_info* info);
/* The stage alone on any host rows in CSR form, through the same kernel: offsets [n_events + 1], rows [R][8], labels
 * [R] or NULL -> out_rows [R][8], out_labels [R] (NULL with labels NULL), order [R] or NULL (order[k] = the input row
 * of output row k; all five arrays are indexed by the row numbers of offsets) and *info.  desc not NULL; a map that shifts nothing runs like any other
 * (the rows come back bit for bit, sorted by column 6).  Needs no other configure call and leaves the configured stage
 * as it is.  Rows of attpc_*_run_spyral are valid input as well.  An event holds fewer than 2^31 rows. */
ATTPC_API int32_t attpc_rows_undistort(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows,
                                       const int64_t* labels, const attpc_undistort_desc* desc, double* out_rows,
                                       int64_t* out_labels, int64_t* order, attpc_undistort_info* info);

/* ---- track fit (opt-in: off by default, and with it off every output, kernel and buffer of every entry point is what
 * it is without this section; inert while the track estimates are off; the entry points are additions under ABI
 * version 3) ----
 * Every stage above fits a circle and a straight line, a model in which the particle loses no energy.  The track fit
 * is Spyral's solver phase on the device: for every (event, position) it takes the estimate record as a start and fits
 * the momentum and the vertex of a trial track, integrated through the gas with the species' stopping-power table, to
 * the label's points.  One 128-byte record (attpc_track_fit) per event and position, beside the estimate record.
 * THIS CONTRACT is what the device is tested against; tests/fit_reference.py restates it in numpy, and
 * csrc/fit_host.hpp is its arithmetic, the same code on the device and on the host.  Everything is f64, each operation
 * rounded once, left to right as C evaluates the expression, no fused multiply-add; only + - * / and sqrt.
 *
 * Settings (attpc_fit_desc): time_step in s, tolerance_momentum (relative), tolerance_position in m, all finite and
 * > 0; max_steps 1 .. 10000; max_evaluations 2 .. 32.
 *
 * Parameters.  q = (gx, gy, gz, x0, y0, z0): g = gamma beta at the vertex, the vertex in metres.
 *
 * Species.  The position's nucleus is species_of_row[indices[s]] of the layout, with the context's mass m (MeV), charge
 * number Z, stopping-power table and the fields, density and length of its detector:
 *   mkg = m * 1.7826619216278976e-30;  qm = Z * 1.602176634e-19 / mkg;  c = 299792458
 *   qb = qm * (-B) / c;  qe = qm * (-E) / c;  drag = 1.6021766339999998e-13 * density * 100 / mkg / c
 * Right-hand side of the state s = (x, y, z, gx, gy, gz), that of the track kernel with sqrt and / for rsqrt:
 *   gv2 = gx gx + gy gy + gz gz;  gv = sqrt(gv2);  gamma = sqrt(1 + gv2);  ke = m (gamma - 1);  vs = c / gamma
 *   v = (gx vs, gy vs, gz vs);  dec = dedx(ke) * drag / gv
 *   ds = (vx, vy, vz, qb vy - dec gx, (-qb) vx - dec gy, qe - dec gz)
 * dedx(ke) reads the table as the track kernel does (exponent -> binade, top five mantissa bits -> node i, the low 47
 * bits / 2^47 -> t; lo + t * (hi - lo); table[0] below 2^-30 MeV or for a NaN, the last node from 2^14 MeV).
 * Step of length h = time_step, classical RK4: k1 = f(s), k2 = f(s + (0.5 h) k1), k3 = f(s + (0.5 h) k2),
 * k4 = f(s + h k3), s' = s + (h / 6) * (((k1 + 2 k2) + 2 k3) + k4), component by component.
 *
 * End of a trial.  Sample 0 is the vertex, sample n the state after n steps.  The trial ends at the first sample for
 * which, tested in this order: a component of s is not finite (end = 4); ke <= 1e-6 MeV (end = 1, stopped);
 * z < 0, z > length or x x + y y >= 0.292 * 0.292 (end = 2, left); n >= max_steps (end = 3, step cap).
 *
 * Data.  The USED rows of the label (step 1 of the track estimates, the same code; with thinning on the label's
 * thinned points), all of them, in delivered order: n_used.  n_points = min(n_used, 2048); data point j is used row
 * j for n_used <= 2048 and used row floor(j n_used / 2048) otherwise, which sets CAPPED.  Metres: x = (double)X /
 * 16000.0, and so y and z.
 *
 * Residuals of a trial.  sg = +1 for gz >= 0 at the vertex, else -1; the cursor c = 0, 1, .. stands for data point c
 * (sg = +1) or n_points - 1 - c (sg = -1).  (i) While sg z_c < sg z_vertex: r_c = vertex - point (three components),
 * next c.  (ii) After every step from sample p to sample s, with d = s - p: while sg z_c <= sg z_s:
 * w = 0 if dz == 0, else (z_c - z_p) / dz; r_c = ((x_p + w dx) - x_c, (y_p + w dy) - y_c, 0), the point counts as
 * inside, next c.  A tie in z therefore goes to the first bracket that reaches it, and an empty bracket (dz == 0) gives
 * sample p.  The end test follows (ii).  (iii) Every point left when the trial has ended: r_c = last sample - point
 * (three components).  path = the sum over the steps of sqrt((dx dx + dy dy) + dz dz), in step order.
 *
 * Evaluation at q: seven trials, trial 0 at q and trial k at q + delta_(k-1) e_(k-1), with delta = 2^-16 |g_start| for
 * the momentum components and 2^-16 m for the vertex, fixed for the whole fit (|v| = sqrt((v0 v0 + v1 v1) + v2 v2)).
 * Per point J_k = (r^(k+1) - r^(0)) / delta_k component by component, dot(a, b) = (a0 b0 + a1 b1) + a2 b2, and the 28
 * sums f = sum dot(r0, r0), (J^T r)_k = sum dot(J_k, r0), N_kl = sum dot(J_k, J_l) for k <= l.
 * ORDER OF SUMMATION: eight accumulators starting at 0, point i to accumulator i mod 8 in ascending i; then
 * a_l <- a_l + a_(l xor 4), a_l <- a_l + a_(l xor 2), a_l <- a_l + a_(l xor 1) on all eight at once; the sum is a_0.
 *
 * Step: A = N (symmetric), A_kk = N_kk + lambda N_kk, b = -(J^T r).  For p = 0 .. 5: a pivot A_pp that is not > 0 ->
 * SINGULAR; for r > p: l = A_rp / A_pp, A_rc = A_rc - l A_pc for c = p .. 5, b_r = b_r - l b_p.  Back substitution for
 * p = 5 .. 0: v = b_p; v = v - A_pc d_c for c = p + 1 .. 5 ascending; d_p = v / A_pp.
 *
 * Iteration (Levenberg-Marquardt with the constants of the geometric circle fit): lambda = 2^-10; evaluate the start;
 * while evaluations < max_evaluations: solve the step (SINGULAR ends the fit with the kept q), evaluate q + d; the
 * trial is ACCEPTED iff f(q + d) <= f(q) and every component of q + d is finite: q <- q + d with its sums,
 * lambda <- 0.04 lambda, and the fit has converged if |d_g| <= tolerance_momentum |g| (the new g) and
 * |d_x| <= tolerance_position; otherwise lambda <- 10 lambda and the step is solved again from the kept sums.
 * Neither converged nor singular: NOT_CONVERGED.
 *
 * Start from the estimate record e (rows of Z mass units as above):
 *   |g| = 299.792458 * Z * e.brho / m;  b = e.slope;  w = sqrt(1 + b b);  st = 1 / w;  ct = b / w
 *   n = ((e.vx - e.cx) / e.radius, (e.vy - e.cy) / e.radius);  t = (-ny, nx), negated if
 *   tx (e.x_mean - e.vx) + ty (e.y_mean - e.vy) < 0;  q = (|g| st tx, |g| st ty, |g| ct, e.vx / 1000, e.vy / 1000,
 *   e.vz / 1000).
 * e.status with EMPTY or FEW -> the same bit here; a start value that is not finite, or a position without a species
 * (Z = 0) -> NO_START.  In all three cases n_points = min(e.n_used, 2048), evaluations, n_inside, steps and end are 0 and
 * every f64 field is NaN (the reserved ones are 0).
 *
 * Record: f, lambda, g, the vertex in mm (x0 * 1000.0), n_inside, steps, end and path of trial 0 of the kept q,
 * ke = m (sqrt(1 + |g| |g|) - 1) in MeV, brho = |g| m / (299.792458 * Z) in T m; STEP_CAP iff end == 3.
 * A label given twice goes to its first position (the later one is EMPTY through its estimate).  A record is a pure
 * function of the event's rows, the estimate record, the species' table and the settings. */
#define ATTPC_FIT_EMPTY 1
#define ATTPC_FIT_FEW 2
#define ATTPC_FIT_CAPPED 8          /* more than 2048 used rows: every floor(j n_used / 2048)-th was taken */
#define ATTPC_FIT_NO_START 16
#define ATTPC_FIT_SINGULAR 32
#define ATTPC_FIT_STEP_CAP 64       /* the final trial ended at sample max_steps */
#define ATTPC_FIT_NOT_CONVERGED 128
#define ATTPC_FIT_MAX_POINTS 2048
#define ATTPC_FIT_MAX_STEPS 10000
#define ATTPC_FIT_MIN_EVALUATIONS 2
#define ATTPC_FIT_MAX_EVALUATIONS 32
#define ATTPC_FIT_END_STOPPED 1
#define ATTPC_FIT_END_LEFT 2
#define ATTPC_FIT_END_STEP_CAP 3
#define ATTPC_FIT_END_NOT_FINITE 4

typedef struct attpc_fit_desc {
  double time_step;           /* s; 1e-10 is the grid of the track kernel */
  double tolerance_momentum;  /* relative to |g| */
  double tolerance_position;  /* m */
  int32_t max_steps;          /* 1 .. 10000 */
  int32_t max_evaluations;    /* 2 .. 32 */
} attpc_fit_desc;  /* 32 bytes */

typedef struct attpc_track_fit {
  int32_t status;       /* ATTPC_FIT_* bits */
  int32_t evaluations;
  int32_t n_points;
  int32_t n_inside;
  int32_t steps;
  int32_t end;          /* ATTPC_FIT_END_* of the final trial */
  double f;             /* m^2 */
  double lambda;
  double g[3];
  double vertex[3];     /* mm */
  double ke;            /* MeV */
  double brho;          /* T m */
  double path;          /* m; the range of a stopped track */
  double reserved[2];   /* 0 */
} attpc_track_fit;  /* 128 bytes */

/* desc == NULL turns the stage off (the default).  ATTPC_E_INVALID outside the ranges above, NaN included.
 * Independent of every other configure call.  With the track estimates on, attpc_sim_run_trace_rows and
 * attpc_det_run_trace_rows launch the fit behind every chunk's estimate kernel on the same stream, on what the
 * estimates read (corrected rows, thinned points or raw rows), also when the rows stay on the device.  It holds 3 MiB
 * of device memory per resident wave for the trials' residuals, 1024 waves at the most. */
ATTPC_API int32_t attpc_trace_configure_fit(attpc_ctx* ctx, const attpc_fit_desc* desc);
/* Records [count][layout->n_sim] of the context's last trace-row call, as attpc_estimates_last. */
ATTPC_API int32_t attpc_fits_last(attpc_ctx* ctx, int64_t first, int64_t count, attpc_track_fit* out);
/* The stage alone on any host rows in CSR form, through the same kernel: estimates_in [n_events][n_sim] are the
 * records of attpc_rows_estimate* on the same rows with estimate_desc; start [n_events][n_sim][6] or NULL replaces
 * the start from the estimates (EMPTY and FEW still come from them).  The context needs a configured detector
 * (ATTPC_E_NOTCONFIGURED without one); indices and species_of_row of the layout are read. */
ATTPC_API int32_t attpc_rows_fit(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows,
                                 const int64_t* labels, const attpc_event_layout* layout,
                                 const attpc_estimate_desc* estimate_desc, const attpc_track_estimate* estimates_in,
                                 const double* start, const attpc_fit_desc* fit_desc, attpc_track_fit* out);

/* ---- clustering (opt-in: off by default, and with it off every output, kernel and buffer of every entry point is
 * what it is without this section; the entry points are additions under ABI version 3) ----
 * Every stage above selects "the rows of a track" by the truth label the simulation gave the row.  This stage splits an
 * event's rows into tracks without it: it sits behind the drift correction (when that is on) and in front of the
 * thinning, the estimates, the circle fit, the helix slope and the track fit, reads a chunk's rows where they lie and
 * writes one CLUSTER LABEL per row, which those stages then read in place of the truth label.  The delivered labels
 * stay the truth labels; the cluster labels and the records below are additional outputs.
 *
 * The algorithm is DBSCAN with every tie made definite.  It is NOT Spyral's sequence of HDBSCAN, cluster joining by
 * circle overlap and outlier-factor cleanup, and nothing here has been compared against Spyral.  The arithmetic is
 * integer throughout, so a result is a pure function of the event's rows and the settings: no dependence on event id,
 * chunking, shard or the order in which the device happens to work.  tests/cluster_reference.py restates this contract
 * in numpy by brute force; csrc/cluster_host.hpp holds the metric and a plain sequential form, shared with the host.
 *
 * Settings (attpc_cluster_desc): eps_xy and eps_z, the linking lengths in mm, each finite and in 1/16 .. 64, as
 * Exy = rint(16 eps_xy) and Ez = rint(16 eps_z), integers in 1 .. 1024; min_samples >= 1, the neighbours a core row
 * needs, itself included; min_cluster_size >= 1, the rows a cluster needs to survive; max_rows in 1 .. 65535, the rows
 * of an event above which it is not clustered; match, ATTPC_CLUSTER_MATCH_TRUTH or ATTPC_CLUSTER_MATCH_RANK; the
 * reserved words 0.
 *
 * One event, on its n rows in delivered order, row index i = 0 .. n-1 (rows [n][8] in ascending z, truth labels [n]):
 *  1. Quantise: estimate_quantise of "track estimates" on columns 0, 1, 2 and 4 -- the same code -- gives X, Y, Z in
 *     units of 1/16 mm.  A row out of its range (a NaN, or the skipped rows the drift correction leaves behind the
 *     others) is noise and counts in n_range.  The in-range rows stand in nondecreasing Z.
 *  2. Metric: d(i, j) = (dX^2 + dY^2) Ez^2 + dZ^2 Exy^2 in int64.  j is a NEIGHBOUR of i iff |dZ| <= Ez and
 *     d <= Exy^2 Ez^2 (an ellipsoid with the half axes eps_xy, eps_xy, eps_z, its surface included); i is its own
 *     neighbour.  Bounds: |dX|, |dY| <= 10 240 and Ez^2 <= 2^20 give (dX^2 + dY^2) Ez^2 < 2^48, |dZ| <= Ez gives
 *     dZ^2 Exy^2 <= 2^40, so d < 2^49 and the threshold is <= 2^40: nothing overflows 64 bits.
 *  3. Core: row i is CORE iff it has at least min_samples neighbours.
 *  4. Cluster: a connected component of the core rows under "is a neighbour of"; its id is the lowest row index among
 *     its core rows.
 *  5. Border: an in-range row that is not core and has a core neighbour joins the cluster of the core neighbour with
 *     the smallest d, ties to the lowest row index.  Every other row is noise.
 *  6. Size cut: a cluster of fewer than min_cluster_size rows (core and border) is dissolved into noise (n_small).
 *  7. Rank: the surviving clusters by rows descending, ties by id ascending.
 *  8. Labels, values of layout->indices or -1 (what thinning, estimates and fit then match against):
 *     MATCH_RANK: the cluster of rank k < n_sim gets indices[k], every other -1.  This is the label-free mode; with
 *       the track fit on, a slot's species is then the position's, not the particle's.  n_split = n_fake = 0.
 *     MATCH_TRUTH: a row VOTES for the lowest position s < n_sim with indices[s] == its truth label (a row whose label
 *       is negative or not among indices votes for nobody).  A cluster's MAJORITY is the position with the most votes,
 *       ties to the lower s; without a vote it has none (-1).  For every position the best-ranked cluster with that
 *       majority gets indices[s]; every other cluster gets -1 and counts in n_split if it had a majority, in n_fake
 *       (made of noise) if it had none.  This stands in for the particle-identification gate an analysis applies, and
 *       it makes estimates[e, s] and fits[e, s] directly comparable with those of the truth-labelled run.
 *     The majority is formed in both modes (the records carry it).
 *  9. Cap: an event of more than max_rows rows is not clustered: every row gets -1 and status carries CAPPED.
 * An event whose components the device could not settle within the bound every one of its loops has (a defect, never
 * seen) is labelled -1 throughout with INTERNAL in status.  In both cases the record holds n_rows, n_noise = n_rows,
 * truth_rows and status, every other field 0, and the event has no cluster records.
 *
 * attpc_cluster_event: n_rows; n_range (step 1); n_core and n_border, the core and border rows of the surviving
 * clusters; n_noise = n_rows - n_core - n_border; n_clusters, the surviving clusters; n_small (step 6); n_split and
 * n_fake (step 8); status; truth_rows[s], the event's rows that vote for position s (all rows, in range or not),
 * saturating at 65535 -- which only a CAPPED event can reach.
 * attpc_cluster_record [n_events][ATTPC_MAX_SIM], the clusters of rank 0 .. 7: rows; core_rows; first_row, the id;
 * majority, the position or -1; majority_rows, its votes (0 without one); label, what step 8 gave (or -1); z_min and
 * z_max of its rows in units.  An unused slot is zero with first_row = -1.  Every field is a count, a minimum or a
 * maximum: nothing depends on an order of accumulation. */
#define ATTPC_CLUSTER_MATCH_TRUTH 0
#define ATTPC_CLUSTER_MATCH_RANK 1
#define ATTPC_CLUSTER_CAPPED 1    /* status: more than max_rows rows */
#define ATTPC_CLUSTER_INTERNAL 2  /* status: a loop of the kernel met its bound */
#define ATTPC_CLUSTER_DEFAULT_MAX_ROWS 16384

typedef struct attpc_cluster_desc {
  double eps_xy;             /* mm, 1/16 .. 64 */
  double eps_z;              /* mm, 1/16 .. 64 */
  int32_t min_samples;       /* >= 1 */
  int32_t min_cluster_size;  /* >= 1 */
  int32_t max_rows;          /* 1 .. 65535 */
  int32_t match;             /* ATTPC_CLUSTER_MATCH_* */
  int32_t reserved[2];       /* 0 */
} attpc_cluster_desc;  /* 40 bytes */

typedef struct attpc_cluster_event {
  int32_t n_rows;
  int32_t n_range;
  int32_t n_core;
  int32_t n_border;
  int32_t n_noise;
  int32_t n_clusters;
  int32_t n_small;
  int32_t n_split;
  int32_t n_fake;
  int32_t status;       /* ATTPC_CLUSTER_CAPPED, ATTPC_CLUSTER_INTERNAL */
  int32_t reserved[2];  /* 0 */
  uint16_t truth_rows[ATTPC_MAX_SIM];
} attpc_cluster_event;  /* 64 bytes */

typedef struct attpc_cluster_record {
  int32_t rows;
  int32_t core_rows;
  int32_t first_row;      /* the id; -1: the slot is unused */
  int32_t majority;       /* position, -1: none */
  int32_t majority_rows;
  int32_t label;          /* a value of layout->indices, or -1 */
  int32_t z_min;          /* units of 1/16 mm */
  int32_t z_max;
} attpc_cluster_record;  /* 32 bytes */

/* desc == NULL turns the stage off (the default): no kernel is launched and no buffer is held then.  ATTPC_E_INVALID
 * for anything the section above rules out, a NaN included.  Independent of every other configure call.  With the
 * stage on attpc_sim_run_trace_rows and attpc_det_run_trace_rows cluster every chunk behind the drift correction, also
 * when the rows stay on the device, and the thinning, the estimates and the fit match the cluster labels; rows, truth
 * labels, offsets and checksums are delivered as without it.  The stage needs a layout, so attpc_trace_rows_at does not
 * run it.  Behind a trigger gate an event that did not fire has no rows and a record of zeros.  It holds 108 bytes of
 * device memory per row of a chunk. */
ATTPC_API int32_t attpc_trace_configure_clustering(attpc_ctx* ctx, const attpc_cluster_desc* desc);
/* The records of events first .. first + count - 1 of the context's last trace-row call: events [count] and records
 * [count][ATTPC_MAX_SIM], either may be NULL.  ATTPC_E_NOTCONFIGURED if the stage was off for that call (or it had no
 * layout), ATTPC_E_INVALID for a range outside it. */
ATTPC_API int32_t attpc_clusters_last(attpc_ctx* ctx, int64_t first, int64_t count, attpc_cluster_event* events,
                                      attpc_cluster_record* records);
/* The cluster labels of rows first_row .. first_row + count - 1 of that call, indexed as its delivered rows are, from a
 * buffer the context owns.  It is filled only when the call fetched the rows themselves: ATTPC_E_NOTCONFIGURED
 * otherwise, ATTPC_E_INVALID for a range outside the delivered rows. */
ATTPC_API int32_t attpc_cluster_labels_last(attpc_ctx* ctx, int64_t first_row, int64_t count, int64_t* out);
/* The stage alone on any host rows in CSR form, through the same kernel: offsets [n_events + 1], rows [R][8], labels
 * [R] the truth labels or NULL (then nobody votes) -> out_labels [R], events [n_events] and records
 * [n_events][ATTPC_MAX_SIM] (each of the three may be NULL).  n_sim and indices of the layout are read.  The in-range
 * rows of every event must stand in nondecreasing Z, which is checked on the host: ATTPC_E_INVALID otherwise.  Needs no
 * other configure call and leaves the configured stage as it is.  An event holds fewer than 2^31 rows. */
ATTPC_API int32_t attpc_rows_cluster(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows,
                                     const int64_t* labels, const attpc_event_layout* layout,
                                     const attpc_cluster_desc* desc, int64_t* out_labels, attpc_cluster_event* events,
                                     attpc_cluster_record* records);

/* ---- cluster joining (opt-in: off by default, and with it off every output, kernel and buffer of every entry point is
 * what it is without this section; the entry points are additions under ABI version 3) ----
 * The clustering above breaks a track into pieces where its rows lie farther apart than the linking lengths (n_split).
 * This stage joins clusters whose circles in the pad plane overlap, which is what Spyral does between its clustering and
 * its estimation.  It does nothing unless the clustering is on; it sits between step 6 (size cut) and step 7 (rank) of
 * the clustering contract, so with it on steps 7 to 9 run on the JOINED clusters and every stage behind the clustering
 * (thinning, estimates, circle fit, helix slope, track fit) reads the joined labels.
 *
 * The contract is Spyral's in structure, with every tie made definite.  It is NOT Spyral's code, Spyral ITERATES the
 * joining with refitted circles and this stage does NOT (one round: a joined cluster's circle is not fitted again), and
 * nothing here has been compared against Spyral.  tests/join_reference.py restates this contract in numpy;
 * csrc/join_host.hpp holds the circle, the overlap predicate, the merge and a plain sequential form, shared with the
 * host.
 *
 * Settings (attpc_join_desc): overlap_ratio, f64 in (0, 1]; min_radius in mm, 1/16 .. 5000; radius_ratio, 0 (no
 * condition) or >= 1; max_clusters in 2 .. 64; the reserved words 0.  A NaN is refused.  The defaults (0.5, 10 mm, 0,
 * 32) are a starting point, not a tuning.
 *
 * One event, behind step 6:
 *  6a. Candidates: the surviving clusters of step 6 in ascending id, K of them.  An event of more than max_clusters
 *      candidates is not joined: its labels, cluster event and cluster records are exactly those of the stage off, its
 *      join event holds n_candidates and JOIN_CAPPED with every other field 0, and its join records are unused.  An
 *      event the clustering did not cluster (CAPPED, INTERNAL, or no rows at all) is not joined either: its join event
 *      is zeros plus JOIN_NOT_CLUSTERED, its join records are unused.
 *  6b. Circle of a candidate: over all its rows, core and border, u = X - X_id and v = Y - Y_id in units of 1/16 mm,
 *      (X_id, Y_id) the cluster's id row, so |u|, |v| <= 10 240.  The sums of u, v, u^2, v^2, uv, u (u^2 + v^2) and
 *      v (u^2 + v^2) are exact in int64: a cluster has at most 65 535 rows, and 65 535 * 10 240 * 2 * 10 240^2 < 2^57.
 *      The Kasa circle follows from them in f64 by estimate_kasa of "track estimates" -- the same code, its two cubic
 *      sums of each axis given as one -- and is moved to absolute mm: a = (X_id + uc) / 16, b = (Y_id + vc) / 16,
 *      R = sqrt(r2) / 16.  A candidate has NO CIRCLE and takes no part if it has fewer than 3 rows, a zero determinant,
 *      r2 <= 0 or a non-finite a, b or R (which covers a determinant that is not finite).  A candidate with
 *      R < min_radius has a circle but takes no part.
 *  6c. Overlap of two candidates that take part, Rs <= Rl their radii (on a tie the lower id is "s"),
 *      d = sqrt(da^2 + db^2) the distance of their centres:
 *        d >= Rs + Rl:  A = 0;      d <= Rl - Rs:  A = pi Rs^2;     otherwise
 *        A = Rs^2 acos(cs) + Rl^2 acos(cl) - sqrt(k) / 2,  cs = (d^2 + Rs^2 - Rl^2) / (2 d Rs),
 *        cl = (d^2 + Rl^2 - Rs^2) / (2 d Rl),  k = (-d + Rs + Rl)(d + Rs - Rl)(d - Rs + Rl)(d + Rs + Rl) clamped at 0,
 *        acos(c) = atan2w(sqrt(max(0, 1 - c^2)), c) with the written arctangent of "helix slope", the same code, and
 *        pi its f64 constant 3.141592653589793.
 *      The pair is JOINED iff A >= overlap_ratio * (pi * Rs^2) and (radius_ratio == 0 or Rl <= radius_ratio * Rs).
 *      Every operation is one f64 rounding in the written order (no contraction).
 *  6d. Join: the joined clusters are the connected components of the candidates under "is joined with" (transitive, one
 *      round).  A component's id is its lowest member id; its rows, core rows and votes are the members' sums, its z
 *      extent their minimum and maximum.  A candidate that takes no part is a component of its own.
 *  7 to 9 run on the components: rank by (rows descending, id ascending), the majority from the summed votes,
 *      MATCH_TRUTH and MATCH_RANK as before.  n_clusters counts components, n_split and n_fake are counted on
 *      components; n_core, n_border, n_noise, n_small and n_range do not change.  The cluster records describe
 *      components.  attpc_cluster_event and attpc_cluster_record keep their layouts and their reserved words (0).
 *
 * attpc_join_event, one per event: n_candidates (K); n_circles, the candidates with a circle; n_taking_part; n_pairs,
 * the pairs joined in 6c; n_joined = candidates - components; status.
 * attpc_join_record [n_events][ATTPC_MAX_SIM], one per ranked component, beside its cluster record: parts, the members
 * it has; first_row, its id; a, b, radius in mm, the circle of its lowest-id member that has one, NaN if none has.  An
 * unused slot is zero with first_row = -1. */
#define ATTPC_JOIN_CAPPED 1         /* status: more than max_clusters candidates, not joined */
#define ATTPC_JOIN_NOT_CLUSTERED 2  /* status: the clustering did not cluster the event */
#define ATTPC_JOIN_MAX_CLUSTERS 64

typedef struct attpc_join_desc {
  double overlap_ratio;   /* (0, 1] */
  double min_radius;      /* mm, 1/16 .. 5000 */
  double radius_ratio;    /* 0: no condition, or >= 1 */
  int32_t max_clusters;   /* 2 .. 64 */
  int32_t reserved[3];    /* 0 */
} attpc_join_desc;  /* 40 bytes */

typedef struct attpc_join_event {
  int32_t n_candidates;
  int32_t n_circles;
  int32_t n_taking_part;
  int32_t n_pairs;
  int32_t n_joined;
  int32_t status;       /* ATTPC_JOIN_CAPPED, ATTPC_JOIN_NOT_CLUSTERED */
  int32_t reserved[2];  /* 0 */
} attpc_join_event;  /* 32 bytes */

typedef struct attpc_join_record {
  int32_t parts;        /* the members of the component */
  int32_t first_row;    /* the id; -1: the slot is unused */
  double a, b, radius;  /* mm; NaN: no member has a circle */
} attpc_join_record;  /* 32 bytes */

/* desc == NULL turns the stage off (the default): no kernel is launched and no buffer is held then.  ATTPC_E_INVALID
 * for anything the section above rules out, a NaN included; refused for nothing else: it is independent of every other
 * configure call, and without the clustering it does nothing.  With both on, every chunk of
 * attpc_sim_run_trace_rows and attpc_det_run_trace_rows is joined right behind its clustering, also when the rows stay
 * on the device.  Behind a trigger gate an event that did not fire has no rows: a join event of zeros plus
 * JOIN_NOT_CLUSTERED and unused join records. */
ATTPC_API int32_t attpc_trace_configure_cluster_join(attpc_ctx* ctx, const attpc_join_desc* desc);
/* The join records of events first .. first + count - 1 of the context's last trace-row call: events [count] and
 * records [count][ATTPC_MAX_SIM], either may be NULL.  ATTPC_E_NOTCONFIGURED if this stage or the clustering was off
 * for that call (or it had no layout), ATTPC_E_INVALID for a range outside it. */
ATTPC_API int32_t attpc_joins_last(attpc_ctx* ctx, int64_t first, int64_t count, attpc_join_event* events,
                                   attpc_join_record* records);
/* attpc_rows_cluster with the joining behind it, through the same kernels: join_desc must not be NULL; join_events
 * [n_events] and join_records [n_events][ATTPC_MAX_SIM] may be NULL like the other outputs. */
ATTPC_API int32_t attpc_rows_cluster_join(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows,
                                          const int64_t* labels, const attpc_event_layout* layout,
                                          const attpc_cluster_desc* desc, const attpc_join_desc* join_desc,
                                          int64_t* out_labels, attpc_cluster_event* events, attpc_cluster_record* records,
                                          attpc_join_event* join_events, attpc_join_record* join_records);

/* ---- particle identification (opt-in: off by default, and with it off every output, kernel and buffer of every entry
 * point is what it is without this section; inert while the track estimates are off; the entry points are additions
 * under ABI version 3) ----
 * With the clustering in MATCH_RANK, slot k of an event is its k-th largest cluster and the track fit integrates its
 * trials with the stopping-power table of POSITION k, whatever the particle.  This stage decides per (event, slot)
 * which position's species the track is, or none: a polygon gate per position in the plane of the estimate record's
 * dE/dx against B rho, which is the one tool an analysis of data has (Spyral's particle ID is such a gate).  It sits
 * behind the estimate kernel and in front of the track fit; the fit of a slot then uses the species of the position the
 * slot was assigned and skips the slots no gate holds.  The estimates' dedx and brho are strongly biased; a gate is
 * drawn on the biased quantities themselves.  tests/pid_reference.py restates this contract in numpy;
 * csrc/pid_host.hpp holds the desc check, the edge rule, the inside test, the assignment walk and a plain sequential
 * form, shared with the host.  Gates are not read from Spyral's files, and nothing here has been compared against
 * Spyral.
 *
 * Gates (attpc_pid_desc): one per layout position p < ATTPC_MAX_SIM.  n_vertices[p] is 0 (no gate: the position is
 * never assigned) or 3 .. ATTPC_PID_MAX_VERTICES; vertices[p][v] = (x, y) in f64, finite: x is B rho in T m, y is
 * dE/dx in the units of attpc_track_estimate.dedx; the vertices behind n_vertices[p] are not read.  mode is
 * ATTPC_PID_ANY or ATTPC_PID_OWN; reserved is 0.  Anything else, a NaN vertex included, is ATTPC_E_INVALID.
 *
 * Inside.  A record's point is (x, y) = (brho, dedx).  It is tested only if both are finite and > 0; otherwise the
 * slot's status is NO_ESTIMATE (position and species -1, held 0).  The test is the crossing number with one written
 * rule per edge from (x0, y0) = vertex v to (x1, y1) = vertex v + 1, the closing edge from the last vertex to the first
 * included: the edge COUNTS iff
 *   (y0 > y) != (y1 > y)   and   d != 0   and   (d > 0) == (y1 > y0),
 *   d = (x1 - x0) * (y - y0) - (x - x0) * (y1 - y0),
 * every difference and product rounded once in f64, nothing contracted into a fused multiply-add.  The point is inside
 * iff the count is odd.  A horizontal edge never counts; a point on an edge (d == 0) does not count that edge, so a
 * point on an edge or a vertex has a definite answer (tests/pid_cases.py pins which).  No division, no transcendental.
 *
 * Assignment per event.  held[k] is the bit mask of the positions p < n_sim whose gate holds slot k's point; in mode
 * OWN only bit k is tested.  The slots are walked in ascending k (with the clustering on this is rank order, the
 * largest cluster first): slot k takes the LOWEST position in held[k] that no earlier slot took.
 *
 * attpc_pid_record per (event, slot): position (-1: none); species, the detector species of that position
 * (species_of_row[indices[position]] of the call's layout where the context's detector has it with Z > 0 and a mass,
 * the index of the table the fit then reads; -1 if there is none, and always -1 from attpc_estimates_pid, which has no
 * layout); held; status, the bits
 *   NO_ESTIMATE  the point was not tested;
 *   NONE         no gate holds it (held == 0);
 *   TAKEN        gates hold it, but all their positions are taken (position -1);
 *   AMBIGUOUS    more than one gate holds it (set beside an assignment, which is still made, or beside TAKEN).
 * A record is a pure function of the event's estimate records and the gates, whatever the chunking.
 *
 * Fit.  With this stage on, the fit of slot k uses the nucleus of position pid.position in every place where "track
 * fit" says "the position's nucleus"; everything else it reads (rows, cluster labels, thinned points, the estimate
 * record as the start) stays slot k's.  A slot with position < 0 is not fitted: its record is the record without a fit
 * of "track fit" (n_points = min(n_used, 2048), the integers 0, every f64 NaN) with status ATTPC_FIT_NO_PID alone. */
#define ATTPC_PID_ANY 0
#define ATTPC_PID_OWN 1
#define ATTPC_PID_MAX_VERTICES 32
#define ATTPC_PID_NO_ESTIMATE 1
#define ATTPC_PID_NONE 2
#define ATTPC_PID_TAKEN 4
#define ATTPC_PID_AMBIGUOUS 8
#define ATTPC_FIT_NO_PID 256        /* attpc_track_fit.status: the particle identification gave the slot no position */

typedef struct attpc_pid_desc {
  int32_t n_vertices[ATTPC_MAX_SIM];  /* 0, or 3 .. 32 */
  int32_t mode;                       /* ATTPC_PID_ANY, ATTPC_PID_OWN */
  int32_t reserved;                   /* 0 */
  double vertices[ATTPC_MAX_SIM][ATTPC_PID_MAX_VERTICES][2];  /* (B rho in T m, dE/dx) */
} attpc_pid_desc;  /* 4136 bytes */

typedef struct attpc_pid_record {
  int32_t position;  /* -1: none */
  int32_t species;   /* -1: none */
  int32_t held;      /* bit p: the gate of position p holds the point */
  int32_t status;    /* ATTPC_PID_* bits */
} attpc_pid_record;  /* 16 bytes */

/* desc == NULL turns the stage off (the default): no kernel is launched and no buffer is held then.  ATTPC_E_INVALID
 * for anything the section above rules out; refused for nothing else: it is independent of every other configure call,
 * and without the track estimates it does nothing.  With both on, attpc_sim_run_trace_rows and attpc_det_run_trace_rows
 * launch the stage behind every chunk's estimate kernel and in front of its track fit on the same stream, also when the
 * rows stay on the device, with the fit off as well.  It holds 4 KiB of device memory for the gates. */
ATTPC_API int32_t attpc_trace_configure_pid(attpc_ctx* ctx, const attpc_pid_desc* desc);
/* Records [count][layout->n_sim] of the context's last trace-row call, as attpc_estimates_last.
 * ATTPC_E_NOTCONFIGURED if this stage or the estimates were off for that call. */
ATTPC_API int32_t attpc_pid_last(attpc_ctx* ctx, int64_t first, int64_t count, attpc_pid_record* out);
/* The stage alone on any host estimate records [n_events][n_sim], through the same kernel: n_sim in
 * 0 .. ATTPC_MAX_SIM, desc not NULL, out [n_events][n_sim]; only brho and dedx of a record are read.  Needs no other
 * configure call and leaves the configured stage as it is. */
ATTPC_API int32_t attpc_estimates_pid(attpc_ctx* ctx, int64_t n_events, int32_t n_sim,
                                      const attpc_track_estimate* estimates, const attpc_pid_desc* desc,
                                      attpc_pid_record* out);
/* attpc_rows_fit with the records of this stage, through the same instantiation of the fit kernel as the fused path:
 * pid [n_events][n_sim], of which position is read (ATTPC_E_INVALID outside -1 .. n_sim - 1). */
ATTPC_API int32_t attpc_rows_fit_pid(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows,
                                     const int64_t* labels, const attpc_event_layout* layout,
                                     const attpc_estimate_desc* estimate_desc, const attpc_track_estimate* estimates_in,
                                     const double* start, const attpc_fit_desc* fit_desc, const attpc_pid_record* pid,
                                     attpc_track_fit* out);

/* ---- reaction reconstruction (opt-in: off by default, and with it off every output, kernel and buffer of every entry
 * point is what it is without this section; inert while its source -- the track estimates, and for the fit source the
 * track fit -- is off; the entry points are additions under ABI version 3) ----
 * The chain above ends at a fitted momentum and vertex per track.  This stage takes it to the observable the simulation
 * is run for: per event the excitation energy Ex of the unobserved partner (missing mass) and the centre-of-mass angle
 * theta_cm of the ejectile of the two-body first step, from ONE observed track, next to the same two numbers made by
 * the same code from the event's truth 4-vector and truth vertex -- and, over the call, the spectra that give the
 * resolution and the efficiency in (Ex, theta_cm).  It is not a row of the trace-row chain: it needs the reaction, which
 * that chain does not know, so it is configured on the context like the summary, the selection and the maps.
 * tests/reaction_reference.py restates this contract in numpy; csrc/reaction_host.hpp holds it as one piece of code for
 * the device and the host.
 *
 * Settings (attpc_reaction_desc, self-contained: the configured kinematics are not read).  masses[0 .. 3]: target,
 * projectile, ejectile, residual in MeV, finite and > 0.  beam_energy (MeV, > 0), has_target (0 or 1); with a target
 * z_min < z_max (m) and eloss [eloss_len], 2 .. ATTPC_REACTION_MAX_ELOSS finite nodes, the projectile's energy loss as
 * attpc_kin_desc.eloss; without one eloss_len is 0.  observed_row is 2 (the ejectile is observed) or 3 (the residual),
 * charge >= 1 the charge number of that nucleus, track the layout position whose track is read, source
 * ATTPC_REACTION_FROM_FIT or ATTPC_REACTION_FROM_ESTIMATE.  Bins: n_ex in 1 .. 256 from ex_lo to ex_hi (finite, lo < hi),
 * n_theta in 1 .. 180 from 0 to PI = 3.141592653589793; ex_inv_width and theta_inv_width are computed ONCE, by the
 * caller, as (double)n_ex / (ex_hi - ex_lo) and (double)n_theta / PI, and are refused if they are anything else.
 * reserved is 0.  Anything else, a NaN included, is ATTPC_E_INVALID.
 *
 * Arithmetic: f64 only, every operation rounded once in the order written, nothing contracted into a fused
 * multiply-add; + - * / and sqrt, floor in the two places named, and atan2w = the written arctangent of "helix slope".
 *
 * Beam energy at a vertex z (m).  Without a target T_b = beam_energy.  With one
 *   t = (z - z_min) / (z_max - z_min) * (double)(eloss_len - 1),
 *   i = floor(t) held to 0 .. eloss_len - 2 (a t that is not >= 0 gives 0),   f = t - (double)i,
 *   T_b = beam_energy - (eloss[i] + f * (eloss[i + 1] - eloss[i])):
 * the look-up of the kinematics kernel, linear in the table and extrapolating beyond both ends.
 *
 * Momentum of the observed nucleus, MeV/c, with m_e = masses[observed_row] and m_r = masses[5 - observed_row].
 *   From a fit record f:       (px, py, pz) = (m_e * g[0], m_e * g[1], m_e * g[2]),   z = vertex[2] / 1000.
 *   From an estimate record e: pmag = 299.792458 * (double)charge * brho,   w = sqrt(1 + slope * slope),
 *                              st = 1 / w,  ct = slope / w  (as the start of the track fit makes them),
 *                              (px, py, pz) = (pmag * st, 0, pmag * ct),   z = vz / 1000.
 *   From the truth:            (px, py, pz) of the event's p4 row observed_row,   z = the truth vertex z.
 *
 * Value(T_b, px, py, pz), m_t = masses[0], m_p = masses[1]:
 *   E   = (T_b + m_p) + m_t                     pb2 = T_b * (T_b + 2 * m_p)          pb = sqrt(pb2)
 *   pt2 = px * px + py * py                     p2  = pt2 + pz * pz                  E_e = sqrt(p2 + m_e * m_e)
 *   dE  = E - E_e                               M2  = dE * dE - ((pb2 + p2) - (2 * pb) * pz)
 *   Ex  = sqrt(M2) - m_r
 *   beta = pb / E                               gamma = E / sqrt(E * E - pb2)        pt = sqrt(pt2)
 *   th  = atan2w(pt, gamma * (pz - beta * E_e))
 *   theta_cm = th for observed_row 2, PI - th for observed_row 3
 * theta_cm is the EJECTILE's polar angle in the centre-of-mass frame in both cases, as Reaction.calculate of the
 * reference defines it.  The value is physical iff M2 > 0 and Ex and theta_cm are finite; otherwise both are NaN.
 * The cancellation is in M2: |delta Ex| is of the order of 2^-53 E^2 / m_r (DESIGN section 6 has the measured
 * constant).
 *
 * Slot.  With the particle identification on (the call made pid records): the FIRST slot s with pid[s].position ==
 * track; none: no slot.  Otherwise slot = track.
 *
 * attpc_reaction_record per event (64 bytes): status, slot (-1: none), beam_ke, ex, theta_cm from the source record,
 * truth_beam_ke, truth_ex, truth_theta_cm from the truth, reserved 0.  status bits:
 *   NO_TRACK        no slot; or its fit record has EMPTY, FEW, NO_START or NO_PID (its estimate record: EMPTY or FEW);
 *                   or px, py, pz or z is not finite.  beam_ke, ex and theta_cm are NaN.
 *   OUTSIDE_TARGET  with a target, z is not in z_min .. z_max (both ends inside).  The value is still computed.
 *   UNPHYSICAL      the value of the source record is not physical; ex and theta_cm are NaN, beam_ke stays.
 *   NO_TRUTH        the kinematics status is not 0, or the value of the truth is not physical.  The three truth fields
 *                   are NaN.  (Host kinematics without a status, attpc_det_run_trace_rows, count as status 0.)
 *
 * Spectra of a call: u64 cells, reaction_cells = 3 n_ex n_theta + n_ex n_ex + 3 of them, in this order:
 *   truth               [n_ex][n_theta]  every event without NO_TRUTH, at the truth values;
 *   truth_reconstructed [n_ex][n_theta]  those of `truth` whose status is 0, at the truth values (their ratio is the
 *                                        efficiency);
 *   reconstructed       [n_ex][n_theta]  status 0, at the reconstructed values;
 *   ex_response         [n_ex truth][n_ex reconstructed]  status 0;
 *   outside [3]         the events of truth / reconstructed / ex_response one of whose two values is outside its bins.
 * Bin of v in n bins from lo: outside iff not (v >= lo and v < hi) -- below lo, at or above hi, NaN --, otherwise
 * floor((v - lo) * inv_width), and n - 1 where that product rounds up to n.  Every term is an integer: the spectra of
 * disjoint id ranges add, and the chunking of a call cannot change them. */
#define ATTPC_REACTION_FROM_FIT 0
#define ATTPC_REACTION_FROM_ESTIMATE 1
#define ATTPC_REACTION_NO_TRACK 1
#define ATTPC_REACTION_OUTSIDE_TARGET 2
#define ATTPC_REACTION_UNPHYSICAL 4
#define ATTPC_REACTION_NO_TRUTH 8
#define ATTPC_REACTION_MAX_EX 256
#define ATTPC_REACTION_MAX_THETA 180
#define ATTPC_REACTION_MAX_ELOSS 65536

typedef struct attpc_reaction_desc {
  double masses[4];        /* MeV: target, projectile, ejectile, residual */
  double beam_energy;      /* MeV */
  double z_min, z_max;     /* m */
  double ex_lo, ex_hi;     /* MeV */
  double ex_inv_width;     /* (double)n_ex / (ex_hi - ex_lo) */
  double theta_inv_width;  /* (double)n_theta / 3.141592653589793 */
  const double* eloss;     /* [eloss_len], host memory; copied by the call */
  int32_t eloss_len;
  int32_t has_target;
  int32_t charge;          /* Z of the observed nucleus */
  int32_t track;           /* layout position */
  int32_t observed_row;    /* 2 or 3 */
  int32_t source;          /* ATTPC_REACTION_FROM_* */
  int32_t n_ex, n_theta;
  int64_t reserved;        /* 0 */
} attpc_reaction_desc;  /* 136 bytes */

typedef struct attpc_reaction_record {
  int32_t status;  /* ATTPC_REACTION_* bits */
  int32_t slot;    /* -1: none */
  double beam_ke, ex, theta_cm;
  double truth_beam_ke, truth_ex, truth_theta_cm;
  double reserved; /* 0 */
} attpc_reaction_record;  /* 64 bytes */

/* desc == NULL turns the stage off (the default): no kernel is launched and no buffer is held then.  ATTPC_E_INVALID
 * for anything the section above rules out.  Independent of every other configure call.  With the stage and its source
 * on, attpc_sim_run_trace_rows and attpc_det_run_trace_rows launch reaction_kernel behind the last of every chunk's
 * estimate, pid and fit kernels on the same stream, also when the rows stay on the device; such a call is refused with
 * ATTPC_E_INVALID if track is not a position of its layout, if the layout has fewer than 4 rows, or if
 * layout->indices[track] is not observed_row (the track of one nucleus would be read with the mass and the truth row of
 * another).  With the option "reaction_spectra_only" (attpc_set_option) such a call copies no record to the host.  It holds the table
 * and the spectra's cells on the device (8 bytes per cell). */
ATTPC_API int32_t attpc_reaction_configure(attpc_ctx* ctx, const attpc_reaction_desc* desc);
/* Records [count] of the context's last trace-row call, as attpc_fits_last.  ATTPC_E_NOTCONFIGURED if this stage or
 * its source was off for that call. */
ATTPC_API int32_t attpc_reaction_last(attpc_ctx* ctx, int64_t first, int64_t count, attpc_reaction_record* out);
/* The spectra of that call: n_cells must be the reaction_cells of the configured bins. */
ATTPC_API int32_t attpc_reaction_spectra_last(attpc_ctx* ctx, int64_t n_cells, uint64_t* cells);
/* The stage alone on host arrays, through the same kernel: fits (source fit) or estimates (source estimate)
 * [n_events][n_sim], the other may be NULL; pid [n_events][n_sim] or NULL; p4 [n_events][n_rows][4] with n_rows in
 * 4 .. ATTPC_MAX_ROWS, vertex [n_events][3] in m, kin_status [n_events] or NULL (all 0).  n_sim in 1 .. ATTPC_MAX_SIM
 * (without pid: > track).  records [n_events] and cells [n_cells] (overwritten, not added to) are the outputs.  Needs
 * no other configure call and leaves the configured stage as it is. */
ATTPC_API int32_t attpc_reaction_records(attpc_ctx* ctx, int64_t n_events, int32_t n_sim, int32_t n_rows,
                                         const attpc_reaction_desc* desc, const attpc_track_fit* fits,
                                         const attpc_track_estimate* estimates, const attpc_pid_record* pid,
                                         const double* p4, const double* vertex, const int32_t* kin_status,
                                         attpc_reaction_record* records, int64_t n_cells, uint64_t* cells);

/* ---- fit hypotheses (opt-in: off by default, and with it off every output, kernel and buffer of every entry point is
 * what it is without this section; inert while the track estimates or the track fit are off; the entry points are
 * additions under ABI version 3) ----
 * The particle identification above gates on the two most biased numbers of the chain.  The track fit itself holds the
 * quantity that separates species: a trial integrated with the wrong stopping-power table cannot have the curvature and
 * the range of the data at once, and a data point beyond the trial's end costs its full distance ("track fit",
 * Residuals (iii)).  This stage fits every slot once per candidate species and gives every slot the position of the
 * lowest f.  It is not a row of the trace-row chain: it is configured on the context, like the reaction reconstruction.
 * tests/hypothesis_reference.py restates this contract in numpy; csrc/hypothesis_host.hpp holds the candidate test, the
 * fitted test, the walk and the record as one piece of code for the device and the host.
 *
 * Hypotheses.  Two positions p, p' < n_sim of the call's layout are the same hypothesis iff they have the same detector
 * species (species_of_row[indices[p]], where the context's detector has it with Z > 0 and a mass: the species of
 * attpc_pid_record); a position without one is no candidate.  The H <= ATTPC_MAX_SIM hypotheses are numbered in the
 * order of their first position.  The host works them out once per call.
 *
 * Candidates of slot k: tried[k] = candidates (the settings' bit mask of positions) AND the positions p < n_sim with a
 * species AND, if the call makes pid records, pid.held of the slot.  With the particle identification on the gates only
 * narrow the choice, and the fit decides among what they hold.
 *
 * Fits.  For every (slot k, hypothesis h) with a position of h in tried[k]: the record "track fit" defines with "the
 * position's nucleus" replaced by the species of h; everything else it reads (rows, cluster labels, thinned points, the
 * estimate record as the start, a given start) is slot k's.  It is byte for byte the record of attpc_rows_fit_pid with
 * pid.position of the slot forced to a position of h.  Every other (slot, hypothesis) pair is not integrated: its
 * record is the record without a fit with ATTPC_FIT_NO_PID alone, as "particle identification" defines it.
 *
 * Selection per event.  Position p of tried[k] is FITTED for slot k iff the record of (k, hypothesis of p) has none of
 * EMPTY, FEW, NO_START and its f is finite; fitted[k] is their bit mask, f[p] the f of that record (NaN for p outside
 * tried[k]).  The slots are walked in ascending k (with the clustering on this is rank order): slot k takes the fitted
 * position with the lowest f that no earlier slot took; f is compared with < only and the positions are tested in
 * ascending order, so a tie goes to the lowest position -- two positions of one species go to two slots in position
 * order.  Comparisons and copies only: no arithmetic on f.
 *
 * attpc_fit_hypothesis per (event, slot), 96 bytes: position (-1: none); species, the detector species of that position
 * (-1: none); tried; fitted; status; reserved 0; f[ATTPC_MAX_SIM]; f_next, the lowest f among the fitted positions of a
 * species other than the chosen one (taken or not), NaN if there is none or no position was chosen -- a caller cuts on
 * f_next / f[position] on the host.  status bits:
 *   NO_CANDIDATE  tried == 0;
 *   NO_FIT        fitted == 0 (set beside NO_CANDIDATE too);
 *   TAKEN         there are fitted positions, but all of them are taken (position -1);
 *   DISPLACED     a position was assigned whose f is greater than the lowest f of the fitted positions: the best one
 *                 was taken.  (A free position of the same f as the taken best one is not a displacement.)
 *
 * Outputs.  fits[e][k] (attpc_fits_last) is a copy of the record of (k, hypothesis of the chosen position); for a slot
 * without a position it is the record without a fit with ATTPC_FIT_NO_PID alone.  The pid records stay what the gates
 * made them.  With this stage on, the "Slot" rule of the reaction reconstruction reads this stage's position where it
 * read pid.position.  A record is a pure function of the event's rows, its estimate records, the tables, the settings
 * and, with the particle identification on, the gates, whatever the chunking. */
#define ATTPC_HYP_NO_CANDIDATE 1
#define ATTPC_HYP_NO_FIT 2
#define ATTPC_HYP_TAKEN 4
#define ATTPC_HYP_DISPLACED 8

typedef struct attpc_hypothesis_desc {
  int32_t candidates;  /* bit p: position p may be chosen; not 0, no bit at or above ATTPC_MAX_SIM */
  int32_t reserved;    /* 0 */
} attpc_hypothesis_desc;  /* 8 bytes */

typedef struct attpc_fit_hypothesis {
  int32_t position;  /* -1: none */
  int32_t species;   /* -1: none */
  int32_t tried;     /* bit p: position p was a candidate */
  int32_t fitted;    /* bit p: ... and its species' fit can be compared */
  int32_t status;    /* ATTPC_HYP_* bits */
  int32_t reserved;  /* 0 */
  double f[ATTPC_MAX_SIM];  /* by position; NaN outside tried */
  double f_next;
} attpc_fit_hypothesis;  /* 96 bytes */

/* desc == NULL turns the stage off (the default): no kernel is launched and no buffer is held then.  ATTPC_E_INVALID
 * for a candidates mask of 0, for bits at or above ATTPC_MAX_SIM and for a reserved field that is not 0.  Independent of
 * every other configure call; without the track estimates and the track fit it does nothing.  With all three on,
 * attpc_sim_run_trace_rows and attpc_det_run_trace_rows launch, in the place of every chunk's fit kernel, its
 * instantiation over (track, hypothesis) pairs -- item = track * H + h, eight lanes per item, [events][n_sim][H]
 * records in a buffer of the chunk -- and behind it hypothesis_selection_kernel, a lane per event, in front of
 * reaction_kernel on the same stream, also when the rows stay on the device. */
ATTPC_API int32_t attpc_trace_configure_hypotheses(attpc_ctx* ctx, const attpc_hypothesis_desc* desc);
/* Records [count][layout->n_sim] of the context's last trace-row call, as attpc_fits_last.  ATTPC_E_NOTCONFIGURED if
 * this stage, the track fit or the estimates were off for that call. */
ATTPC_API int32_t attpc_hypotheses_last(attpc_ctx* ctx, int64_t first, int64_t count, attpc_fit_hypothesis* out);
/* The fit records of every hypothesis of that call, [count][layout->n_sim][H], and H itself (n_hypotheses, may be NULL;
 * written also when count is 0); out holds count * n_sim * ATTPC_MAX_SIM records at the most.  For tests and studies. */
ATTPC_API int32_t attpc_hypothesis_fits_last(attpc_ctx* ctx, int64_t first, int64_t count, int32_t* n_hypotheses,
                                             attpc_track_fit* out);
/* attpc_rows_fit_pid with this stage, through the same two kernels as the fused path: desc not NULL; pid
 * [n_events][n_sim] or NULL (of which held is read); records [n_events][n_sim], fits [n_events][n_sim], all_fits
 * [n_events][n_sim][H] with room for ATTPC_MAX_SIM hypotheses per slot, or NULL: not wanted; n_hypotheses (H) and
 * species [ATTPC_MAX_SIM] (the detector species of hypothesis h, -1 behind H) may be NULL. */
ATTPC_API int32_t attpc_rows_fit_hypotheses(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows,
                                            const int64_t* labels, const attpc_event_layout* layout,
                                            const attpc_estimate_desc* estimate_desc,
                                            const attpc_track_estimate* estimates_in, const double* start,
                                            const attpc_fit_desc* fit_desc, const attpc_hypothesis_desc* desc,
                                            const attpc_pid_record* pid, attpc_fit_hypothesis* records,
                                            attpc_track_fit* fits, attpc_track_fit* all_fits, int32_t* n_hypotheses,
                                            int32_t* species);

#ifdef __cplusplus
}
#endif
#endif /* ATTPC_ENGINE_H */
