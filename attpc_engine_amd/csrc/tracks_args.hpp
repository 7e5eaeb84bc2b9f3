// tracks_args.hpp -- kernel argument blocks and host launch wrappers (one per kernel file).
#pragma once
#include "common.hpp"
#include "cluster_host.hpp"  // (behind the HIP runtime header)
#include "distort_host.hpp"
#include "hypothesis_host.hpp"
#include "join_host.hpp"
#include "undistort_host.hpp"
#include "unpack_host.hpp"

namespace attpc {

struct TrackArgs {
  DetDev det;
  attpc_event_layout layout;
  TrackBuffers buf;
  const double* p4;           // [n_events][n_rows][4]
  const double* vertex;       // [n_events][3]
  const int32_t* kin_status;  // [n_events] or nullptr; != 0 -> event has no tracks
  uint64_t seed;
  uint64_t first_event;       // global id of chunk-local event 0
  uint32_t n_events;
  uint32_t n_tracks;          // n_events * n_sim
  // Order in which the tracks are handed to the lanes: all events' nucleus sim_order[0] first, then sim_order[1], ...
  // (the host puts the species with the longest tracks first: the lanes run dry on short tracks at the kernel's end).
  // sim_order[0] == 0xff: event by event, as the tables are laid out.
  uint8_t sim_order[ATTPC_MAX_SIM];
};

struct ScatterArgs {
  DetDev det;
  attpc_event_layout layout;
  TrackBuffers trk;
  CloudBuffers out;
  uint64_t seed;
  uint64_t first_event;
  uint32_t n_events;
  uint32_t event0;     // first event of this launch within the track batch (track ids start at event0 * n_sim)
  uint32_t batch;      // events a workgroup takes per visit to the event counter
  uint32_t row_block;  // output rows a workgroup reserves at a time (1: exactly what each window needs)
  // merge variant of the kernel (scatter.hip, scatter_kernel<false, true>; path-length dE/dx step): per workgroup two
  // lists of merge_cap 8-byte entries {arena record, time bucket | nucleus << 10 | slice << 13}, the event's entries
  // in list order and sorted by time bucket; merge_cap >= the entries an event can have.  nullptr: the default kernel
  uint2* merge_scratch;
  uint32_t merge_cap;
};

void launch_kin_run(hipStream_t s, const attpc_kin_desc& d, uint64_t seed, uint64_t first_event, uint32_t n,
                    double* p4, double* vertex, int32_t* status, uint32_t* attempts);
void launch_kin_calculate(hipStream_t s, const attpc_kin_desc& d, uint32_t n, const double* beam, const double* ex,
                          const double* th, const double* ph, double* p4, int32_t* status);
void launch_decay_calculate(hipStream_t s, uint32_t n, const double* parent, double m1, double m2, const double* ex,
                            const double* th, const double* ph, double* out, int32_t* status);
// straggle (attpc_det_configure_straggling; nullptr or both scales 0: the kernels of the stage off): the track
// straggling, track_kernel<*, true> with an argument block of its own (tracks.hip)
void launch_track_kernel(uint32_t blocks, size_t lds_bytes, hipStream_t s, const TrackArgs& a,
                         const attpc_straggle_desc* straggle = nullptr);
// drift distortion of a track batch's records (distort.hip; attpc_det_configure_distortion, the contract is in
// include/attpc_engine.h): every record below counts[t] of tracks 0 .. n_tracks - 1 is shifted in place by `map`
struct DistortArgs {
  DistortMap map;       // the tables on the device
  TrackBuffers buf;     // ctrl[TRK_NEXT_DISTORT] zero before the launch; ctrl[TRK_OVERFLOW] != 0: nothing is touched
  uint32_t n_tracks;
};
// persistent waves, four per workgroup, each taking four tracks at a time: `workgroups` = distort_workgroups(n_tracks,
// limit) > 0
inline uint32_t distort_workgroups(uint32_t n_tracks, uint32_t limit) {
  const uint32_t want = (n_tracks + 15u) / 16u;
  return want < limit ? (want ? want : 1u) : (limit ? limit : 1u);
}
void launch_distort(uint32_t workgroups, hipStream_t s, const DistortArgs& a);
// scatter.hip compiled as it is / through scatter_small.hip (workgroups per CU: 1 / 2)
void launch_scatter_kernel_big(uint32_t n_workgroups, hipStream_t s, const ScatterArgs& a);
void launch_scatter_kernel_small(uint32_t n_workgroups, hipStream_t s, const ScatterArgs& a);
void launch_scatter_kernel_wide(uint32_t n_workgroups, hipStream_t s, const ScatterArgs& a);  // scatter_wide.hip: u64 sums
// lone.hip: the time buckets scatter_kernel recorded in out.lone_list (normally none: exits at once)
void launch_lone_bucket_kernel(uint32_t n_workgroups, hipStream_t s, const ScatterArgs& a);

// response + threshold + Spyral rows on device (spyral.hip)
struct SpyralDev {
  const double* response;      // [512]
  const double* sorted_desc;   // [512] response sorted descending
  const double* tail;          // [513] tail[k] = sum of all but the k largest samples (spyral_integral.hpp)
  const double* pad_centers;   // [n_pads][2]
  const double* pad_sizes;     // [n_pads]
  int32_t n_pads;
  double r_max;
  double window_edge, mm_edge, length, threshold;
};
// plain row conversion of `n` cloud points, nothing dropped or sorted (attpc_spyral_rows): rows [n][8]
void launch_spyral_rows_kernel(hipStream_t s, int64_t n, const double* points, const double* response, const double* centers,
                               const double* sizes, int32_t n_pads, double window_edge, double mm_edge, double length, double* rows);
void launch_spyral_count(hipStream_t s, const SpyralDev& sp, uint32_t n_events, const int64_t* event_start,
                         const double* points, uint32_t* kept);
// rows of every event sorted by z (writer.py:236-238); sort_scratch: one u32 + one f64 per cloud row of the chunk
// (SpyralPacked: the 24-byte transfer record of a Spyral row, unpack_host.hpp)
// packed != nullptr: write SpyralPacked records (and raise *pack_flag for a row that does not fit) instead of rows / labels
void launch_spyral_write(hipStream_t s, const SpyralDev& sp, uint32_t n_events, const int64_t* event_start,
                         const int64_t* kept_start, const double* points, const int64_t* labels, double* rows,
                         int64_t* out_labels, uint32_t* sort_idx, double* sort_key, SpyralPacked* packed, int64_t* pack_flag);

// digitised pad traces on device (traces.hip; the contract is in include/attpc_engine.h)
struct TraceDev {
  const double* response;  // [512]
  double threshold;
  int32_t offset;
  const double* gained;    // [rows] the chunk's gained charges q'' (gain.hip), or nullptr: the cloud's own charges
};
// a cloud row the traces can place: pad and time bucket in range
__device__ __forceinline__ bool trace_row_ok(double padf, double tb) {
  return padf >= 0.0 && padf < (double)ATTPC_NUM_PADS && tb >= 0.0 && tb < (double)ATTPC_NUM_TB;
}
// per-event working lists in global memory, ranges of the event's own cloud rows (rows lo .. hi of the chunk)
struct TraceScratch {
  uint32_t* row;        // [rows] the event's row numbers grouped by pad, pads ascending
  uint32_t* hit;        // [rows] k-th hit pad of the event
  uint32_t* hit_start;  // [rows] first entry of that pad's group in `row`
  int32_t* rank;        // [rows] rank of that pad among the event's kept pads, -1 = dropped
  uint32_t* info;       // [2 * events] hit pads, rows placed
};
// electronic noise and pedestals of the traces (attpc_trace_configure_noise); the noise of event e of a launch is keyed
// on (seed, first_event + e)
struct TraceNoiseDev {
  const uint32_t* cdf;        // [n_levels - 1], padded to ATTPC_MAX_NOISE_LEVELS
  const uint16_t* guide;      // [256]: #{k : cdf[k] <= b << 24}, where the search for u with u >> 24 == b starts
  const int16_t* pedestals;   // [ATTPC_NUM_PADS] or nullptr (zeros)
  int32_t n_levels;           // 0 = no noise draw (pedestals only)
  int32_t min_level;
  uint32_t domain;            // DOMAIN_TRACE_NOISE | stream
};
// readout of noise-only pads (attpc_trace_configure_readout, PARTIAL / FULL)
constexpr int TR_MAP_WORDS = ATTPC_NUM_PADS / 32;  // words of a per-event pad bitmap
constexpr int32_t TRACE_CUT_DRAW = 0;    // a noise-only pad of PARTIAL is kept iff some u_j >= cut
constexpr int32_t TRACE_CUT_ALWAYS = 1;  // ... always (c <= 0)
constexpr int32_t TRACE_CUT_NEVER = 2;   // ... never (c > n_levels - 1, or no noise table)
struct TraceReadoutDev {
  const uint32_t* channels;  // [TR_MAP_WORDS] bit p % 32 of word p / 32: pad p is in the readout set S
  int32_t full;              // ATTPC_READOUT_FULL: every pad of S is kept
  int32_t cut_kind;          // TRACE_CUT_* (the pedestal terms of the decision rule come on top)
  uint32_t cut;              // cdf[c - 1] (TRACE_CUT_DRAW)
};
// per-event bitmaps of a chunk in readout ([events][TR_MAP_WORDS] each): the noise-only kept pads, every kept pad, and
// the number of kept pads below each word
struct TraceMaps {
  uint32_t* noise;
  uint32_t* kept;
  uint32_t* before;
};
// common-mode noise of the traces (attpc_trace_configure_common_mode): what the sample-producing kernels read
struct CommonDev {
  const int16_t* values;  // [events of the launch][n_groups][512], a group's 512 values in lane order: sample l + 64 s
                          // at 8 l + s (common_mode_kernel writes them, add_common reads 16 B per lane)
  const uint8_t* groups;  // [ATTPC_NUM_PADS] on the device: the pad's group, 255 = no common-mode term; nullptr = group 0
  int32_t n_groups;       // 1 + the highest group of the map
  int32_t top;            // largest pad-noise level + largest common-mode level: no sum n_p[j] + c_g[j] is above it
};
// values of events first_event .. first_event + n_events - 1, one wave per (event, group); `table`: the stage's own
// noise table (cdf padded, guide, n_levels > 0, min_level, domain = DOMAIN_TRACE_COMMON | stream)
void launch_common_mode(hipStream_t s, const TraceNoiseDev& table, uint64_t seed, uint32_t n_events, uint64_t first_event,
                        uint32_t n_groups, int16_t* values);
// kept[e]: kept pad rows of event e (the count pass works out every trace, keeps the ranks in scratch).
// noise == nullptr: the noiseless kernels; ro == nullptr: hit-mode readout; common == nullptr: no common-mode term
// (with it the kernels with noise run, `noise` may then be a table-less, pedestal-less TraceNoiseDev or nullptr)
void launch_trace_count(hipStream_t s, const TraceDev& tr, const TraceNoiseDev* noise, uint64_t seed, uint32_t n_events,
                        uint64_t first_event, const int64_t* event_start, const double* points, const int64_t* labels,
                        TraceScratch sc, uint32_t* kept, const TraceReadoutDev* ro, const CommonDev* common = nullptr);
// behind the count pass with ro: the noise-only verdicts of every event (empty ones included), kept[e] and the hit pads'
// ranks over the union of kept pads, the maps of the noise write
void launch_trace_scan(hipStream_t s, const TraceDev& tr, const TraceNoiseDev* noise, const TraceReadoutDev& ro,
                       uint64_t seed, uint32_t n_events, uint64_t first_event, const int64_t* event_start, TraceScratch sc,
                       uint32_t* kept, TraceMaps maps, const CommonDev* common = nullptr);
// the noise-only rows (label -1) at kept_start[e] + rank; the checksums as launch_trace_write
void launch_trace_noise_write(hipStream_t s, const TraceNoiseDev* noise, uint64_t seed, uint32_t n_events,
                              uint64_t first_event, TraceMaps maps, const int64_t* kept_start, int32_t* pads,
                              int16_t* samples, int64_t* out_labels, unsigned long long* sums,
                              const CommonDev* common = nullptr);
// the kept rows at kept_start[e] + rank; sums[0] += sample checksum, sums[1] += pad checksum (event = first_event + e)
void launch_trace_write(hipStream_t s, const TraceDev& tr, const TraceNoiseDev* noise, uint64_t seed, uint32_t n_events,
                        uint64_t first_event, const int64_t* event_start, const double* points, const int64_t* labels,
                        TraceScratch sc, const int64_t* kept_start, int32_t* pads, int16_t* samples, int64_t* out_labels,
                        unsigned long long* sums, const CommonDev* common = nullptr);

// micromegas gain of the traces (gain.hip; attpc_trace_configure_gain, the contract is in include/attpc_engine.h)
struct GainDev {
  const double* quantiles;  // [ATTPC_GAIN_KNOTS] inverse CDF of the standardised fluctuation, or nullptr: no draw (f = 0)
  const double* pad_gain;   // [ATTPC_NUM_PADS] or nullptr (1.0 everywhere)
  double c;                 // rel_variance / 9.0
  uint32_t domain;          // DOMAIN_TRACE_GAIN | stream
};
// gained[r] = q'' of row r of the event-ordered cloud (event e of the launch = global id first_event + e); rows out of
// the traces' range get 0.  One workgroup per event.
void launch_gain(hipStream_t s, const GainDev& g, uint64_t seed, uint32_t n_events, uint64_t first_event,
                 const int64_t* event_start, const double* points, double* gained);

// peaks of the kept trace rows -> Spyral rows (peaks.hip; attpc_trace_configure_peaks, the contract is in
// include/attpc_engine.h).  The geometry is SpyralDev's.
struct PeakDev {
  int32_t distance;  // ceil(separation), at most ATTPC_NUM_TB
  double prominence, min_width, max_width, rel_height, threshold;
};
// per kept trace row (pads / samples as the trace write pass left them; pedestals nullptr = zeros): maps [rows][64],
// bit s of byte l = sample 8 l + s is a point; counts [rows] their number.  row_pass [rows] (the trigger's gate,
// trigger.hip): a row whose byte is 0 has no points; nullptr = every row
void launch_peak_count(hipStream_t s, const PeakDev& pk, const int16_t* pedestals, uint32_t n_rows, const int32_t* pads,
                       const int16_t* samples, uint8_t* maps, uint32_t* counts, const uint8_t* row_pass = nullptr);
// row_start [n_rows + 1] = exclusive scan of counts [n_rows], n_rows > 0; block_sums [peak_scan_blocks(n_rows)] and
// block_start [peak_scan_blocks(n_rows) + 1]: scratch
uint32_t peak_scan_blocks(uint32_t n_rows);
void launch_peak_scan(hipStream_t s, const uint32_t* counts, uint32_t n_rows, int64_t* row_start, uint32_t* block_sums,
                      int64_t* block_start);
// ev_start[e] = row_start[kept_start[e]], e = 0 .. n_events
void launch_peak_event_start(hipStream_t s, uint32_t n_events, const int64_t* kept_start, const int64_t* row_start,
                             int64_t* ev_start);
// records [points]: (trace row, sample, amplitude, integral) of every point, at row_start[row] in ascending sample
void launch_peak_write(hipStream_t s, const PeakDev& pk, const int16_t* pedestals, uint32_t n_rows, const int32_t* pads,
                       const int16_t* samples, const uint8_t* maps, const int64_t* row_start, uint4* records,
                       const uint8_t* row_pass = nullptr);
// rows [points][8] / out_labels in the contract's order per event (ev_start: CSR offsets of the events' points);
// centroid / sort_idx / sort_key: scratch of one entry per point; sums[0] += the row checksum (event = first_event + e)
void launch_peak_rows(hipStream_t s, const SpyralDev& sp, uint64_t seed, uint32_t n_events, uint64_t first_event,
                      const int64_t* ev_start, const uint4* records, const int32_t* pads, const int64_t* labels,
                      double* centroid, uint32_t* sort_idx, double* sort_key, double* rows, int64_t* out_labels,
                      unsigned long long* sums);

// Fourier baseline removal of trace rows (baseline.hip; the contract is in include/attpc_engine.h): samples / y
// [n_rows][512] int16, twiddle [512] (cos, sin) of 2 pi j / 512, filter [512] = F / 512 in the transform's order
// (entry 64 k2 + 8 k0 + k1 is F[k0 + 8 k1 + 64 k2]), baseline [n_rows][512] f64 or nullptr
void launch_baseline(hipStream_t s, uint32_t n_rows, const int16_t* samples, const double2* twiddle, const double* filter,
                     int16_t* y, double* baseline);

// multiplicity trigger on the kept trace rows (trigger.hip; attpc_trace_configure_trigger, the contract is in
// include/attpc_engine.h)
struct TriggerDev {
  int32_t threshold, window, group_multiplicity, min_groups;
  int32_t n_groups;       // 1 + the highest group of the map (1 without a map): what the kernel clears and scans
  const uint8_t* groups;  // [ATTPC_NUM_PADS] on the device, or nullptr = every pad in group 0
};
struct TriggerArgs {
  TriggerDev tg;
  const int16_t* pedestals;       // [ATTPC_NUM_PADS] or nullptr = zeros
  const int64_t* kept_start;      // [n_events + 1] CSR offsets of the events' rows
  const int32_t* pads;            // [rows]
  const int16_t* samples;         // [rows][512]
  attpc_trigger_record* records;  // [n_events]
  uint8_t* row_pass;              // [rows] fired of the row's event (the gate of the peak passes), or nullptr
};
// one workgroup per event, empty events included
void launch_trigger(hipStream_t s, uint32_t n_events, const TriggerArgs& a);

// one thinned track point (thin.hip writes them, estimate.hip reads them)
struct ThinPoint {  // what the estimator reads first, then what attpc_rows_thin delivers
  int32_t X, Y, Z;   // C(Sx), C(Sy), C(Sz) in units
  int32_t n;
  int64_t si;
  double amplitude;
  int32_t bin;
  int32_t split;
};  // 40 bytes

// track estimates of the trace rows (estimate.hip; attpc_trace_configure_estimates, the contract is in
// include/attpc_engine.h)
struct EstimateArgs {
  const int64_t* ev_start;          // [n_events + 1] CSR offsets of the events' rows
  const double* rows;               // [rows][8] Spyral rows, every event in its delivered order
  const int64_t* labels;            // [rows]
  attpc_track_estimate* records;    // [n_events][n_sim]
  int64_t slot_label[ATTPC_MAX_SIM];  // the label of position s, -1: none (a later position of a label given twice)
  int32_t n_sim;
  int32_t min_points;
  int64_t rb2;                      // Rb^2 in units^2
  double magnetic_field;
  // the estimates of thinned points (launch_point_estimates) read these in the place of rows and labels
  const ThinPoint* points;            // [rows] the regions thin_kernel filled
  const attpc_thin_info* thin_info;   // [n_events][n_sim]
  // the geometric circle fit (launch_circle_estimates) reads these
  double circle_tolerance;            // units
  int32_t circle_max_evaluations;     // 2 .. 64
  // the helix slope (launch_helix_estimates) reads this
  int32_t helix_regressor;            // 0 .. 2
};
// one workgroup per event, empty events included (n_events > 0, n_sim > 0)
void launch_estimates(hipStream_t s, uint32_t n_events, const EstimateArgs& a);
// the same on the thinned points of every (event, position): a.points and a.thin_info as launch_thin left them
void launch_point_estimates(hipStream_t s, uint32_t n_events, const EstimateArgs& a);
// launch_estimates (points = false) or launch_point_estimates (points = true) with the geometric circle fit behind the
// Kasa circle (attpc_trace_configure_circle, "geometric circle fit" in the header): a.circle_* are set
void launch_circle_estimates(hipStream_t s, uint32_t n_events, const EstimateArgs& a, bool points);
// any of the four with the helix slope behind the circle (attpc_trace_configure_helix, "helix slope" in the header):
// a.helix_regressor is set, and with `circle` a.circle_* are
void launch_helix_estimates(hipStream_t s, uint32_t n_events, const EstimateArgs& a, bool points, bool circle);

// thinned track points (thin.hip; attpc_trace_configure_thinning, the contract is in include/attpc_engine.h)
struct ThinArgs {
  const int64_t* ev_start;          // [n_events + 1] CSR offsets of the events' rows
  const double* rows;               // [rows][8]
  const int64_t* labels;            // [rows]
  ThinPoint* points;                // [rows]: the region of (e, s) starts at ev_start[e] + the rows of the labels of the
                                    // positions below s and holds info[e][s].n_points points
  attpc_thin_info* info;            // [n_events][n_sim]
  int64_t slot_label[ATTPC_MAX_SIM];  // as EstimateArgs
  int32_t n_sim;
  int32_t step;                     // H in units
};
// one workgroup per event, empty events included (n_events > 0, n_sim > 0)
void launch_thin(hipStream_t s, uint32_t n_events, const ThinArgs& a);

// track fit (fit.hip; attpc_trace_configure_fit, the contract is in include/attpc_engine.h)
struct FitPosition {                // the nucleus of position s (FitSpecies of fit_host.hpp)
  double mass, charge, qm_b, qm_e, drag;
  int32_t table;                    // its table in dedx, -1: the position has no species
  int32_t pad;
};
struct FitArgs {
  const int64_t* ev_start;          // as EstimateArgs: the rows ...
  const double* rows;
  const int64_t* labels;
  const ThinPoint* points;          // ... or, if not nullptr, the thinned points
  const attpc_thin_info* thin_info;
  const attpc_track_estimate* estimates;  // [n_events][n_sim]
  const double* start;              // [n_events][n_sim][6] or nullptr
  attpc_track_fit* records;         // [n_events][n_sim]
  double* scratch;                  // [workgroups][8 tracks][8][ATTPC_FIT_MAX_POINTS][3]
  const double* dedx;               // [n_species][ATTPC_DEDX_NODES]
  int64_t slot_label[ATTPC_MAX_SIM];
  FitPosition position[ATTPC_MAX_SIM];
  attpc_fit_desc d;
  double length;                    // m
  int64_t rb2;
  uint32_t n_events;
  int32_t n_sim;
};
struct FitPidArgs : FitArgs {       // fit_kernel<true>: behind the particle identification (pid.hip), the nucleus of
  const attpc_pid_record* pid;      // slot s is that of position pid[e][s].position; [n_events][n_sim]
};
struct FitHypArgs : FitArgs {       // fit_kernel<false, true>: the fit hypotheses (hypothesis_host.hpp).  Its work items
  const attpc_pid_record* pid;      // are (track, hypothesis) pairs, item = track * hyp.n + h: slot s is fitted as the
  HypLayout hyp;                    // nucleus of position hyp.first[h] if a position of h is a candidate of the slot
};                                  // (pid: [n_events][n_sim] or nullptr); records is [n_events][n_sim][hyp.n]
constexpr uint32_t FIT_MAX_WORKGROUPS = 1024;
constexpr size_t FIT_SCRATCH_PER_WORKGROUP = (size_t)8 * 8 * ATTPC_FIT_MAX_POINTS * 3 * sizeof(double);
// the workgroups (one wave of eight items each) for n_events * n_sim tracks of n_hyp items each (1: an item is a
// track); a.scratch holds that many regions
uint32_t fit_workgroups(uint32_t n_events, int32_t n_sim, int32_t n_hyp = 1);
// fit_kernel<false>, or with `pid` fit_kernel<true> (FitPidArgs)
void launch_fit(hipStream_t s, const FitArgs& a, const attpc_pid_record* pid = nullptr);
// fit_kernel<false, true> (FitHypArgs): `hyp` with n >= 1, `pid` or nullptr
void launch_fit_hypotheses(hipStream_t s, const FitArgs& a, const HypLayout& hyp, const attpc_pid_record* pid);
// hypothesis_selection_kernel (hypothesis.hip), a lane per event, behind launch_fit_hypotheses on the same stream
void launch_hypothesis_select(hipStream_t s, const HypothesisArgs& a);

// particle identification (pid.hip; attpc_trace_configure_pid, the contract is in include/attpc_engine.h)
struct PidGates {                   // the gates of an attpc_pid_desc as the device holds them
  double vertices[ATTPC_MAX_SIM * ATTPC_PID_MAX_VERTICES * 2];
  int32_t n_vertices[ATTPC_MAX_SIM];
};
struct PidArgs {
  const attpc_track_estimate* estimates;  // [n_events][n_sim]
  const PidGates* gates;
  attpc_pid_record* records;        // [n_events][n_sim]
  int32_t species[ATTPC_MAX_SIM];   // the detector species of every position, -1: none
  uint32_t n_events;                // > 0
  int32_t n_sim;                    // 1 .. ATTPC_MAX_SIM
  int32_t mode;                     // ATTPC_PID_ANY, ATTPC_PID_OWN
};
constexpr uint32_t PID_MAX_WORKGROUPS = 2048;
// the workgroups (one wave each) for n_events events
uint32_t pid_workgroups(uint32_t n_events);
void launch_pid(hipStream_t s, const PidArgs& a);

// drift correction of trace rows (undistort.hip; attpc_trace_configure_correction, the contract is in
// include/attpc_engine.h)
struct UndistortArgs {
  UndistortSettings s;              // the map's tables on the device
  const int64_t* ev_start;          // [n_events + 1] CSR offsets of the events' rows
  const double* rows;               // [rows][8]
  const int64_t* labels;            // [rows] or nullptr
  double* xyt;                      // [rows][3] scratch: the corrected x, y (m) and t of every row (t NaN: skipped)
  uint32_t* sort_idx;               // [rows] and
  double* sort_key;                 // [rows]: the sort's scratch
  double* out_rows;                 // [rows][8]
  int64_t* out_labels;              // [rows] or nullptr
  int64_t* order;                   // [rows] or nullptr: order_base + the input row of every output row
  int64_t order_base;
  unsigned long long* counts;       // [4] += n_rows, n_skipped, n_unconverged, n_moved
};
// one workgroup per event, empty events included (n_events > 0)
void launch_undistort(hipStream_t s, uint32_t n_events, const UndistortArgs& a);

// clustering of trace rows (cluster.hip; attpc_trace_configure_clustering, the contract is in include/attpc_engine.h)
// cluster_join_kernel (cluster_join.hip) reads this scratch as cluster_kernel left it -- cx, cy, cz, orig, core, comp
// and the per-root counts, votes and extent -- and reuses w_lo: it must be launched right behind cluster_kernel on the
// same stream with nothing else in between that touches the scratch, which is what keeps it alive.
constexpr size_t CLUSTER_SCRATCH_WORDS = 25;  // 32-bit words of scratch per row (cluster.hip lists them)
struct ClusterArgs {
  ClusterSettings s;
  const int64_t* ev_start;          // [n_events + 1] CSR offsets of the events' rows
  const double* rows;               // [rows][8]
  const int64_t* labels;            // [rows] the truth labels, or nullptr: nobody votes
  int32_t* scratch;                 // [rows][CLUSTER_SCRATCH_WORDS]
  int64_t* out_labels;              // [rows] the cluster labels
  attpc_cluster_event* events;      // [n_events] or nullptr
  attpc_cluster_record* records;    // [n_events][ATTPC_MAX_SIM] or nullptr
};
// one workgroup per event, empty events included (n_events > 0)
void launch_cluster(hipStream_t s, uint32_t n_events, const ClusterArgs& a);

// cluster joining (cluster_join.hip; attpc_trace_configure_cluster_join, the contract is in include/attpc_engine.h)
struct ClusterJoinArgs {
  ClusterArgs c;                    // what cluster_kernel was launched with just before; c.events is not nullptr
  JoinSettings j;
  attpc_join_event* join_events;    // [n_events] or nullptr
  attpc_join_record* join_records;  // [n_events][ATTPC_MAX_SIM] or nullptr
};
// one workgroup per event, right behind launch_cluster on the same stream (n_events > 0)
void launch_cluster_join(hipStream_t s, uint32_t n_events, const ClusterJoinArgs& a);

// packed pad traces (trace_pack.hip; the format "for64-bitplane-v1" is in include/attpc_engine.h).  samples
// [n_rows][512] as the trace write pass left them, n_rows > 0; `workgroups` = trace_pack_workgroups(n_rows, limit).
// size pass: headers [n_rows] (the eight u16 headers of every row) and sizes [n_rows] (bytes of its record)
uint32_t trace_pack_workgroups(uint32_t n_rows, uint32_t limit);
void launch_trace_pack_size(hipStream_t s, uint32_t workgroups, uint32_t n_rows, const int16_t* samples, uint4* headers,
                            uint32_t* sizes);
// write pass: row_start [n_rows + 1] = the exclusive scan of sizes on entry (relative to `bytes`), + base on return
void launch_trace_pack_write(hipStream_t s, uint32_t workgroups, uint32_t n_rows, const int16_t* samples, const uint4* headers,
                             int64_t* row_start, int64_t base, unsigned char* bytes);

// event and track summaries of a scattered chunk (summary.hip; attpc_summary_configure, the contract is in
// include/attpc_engine.h).  The rows are read in place through the launch's segment list.
struct SummaryArgs {
  ChunkView chunk;                 // the chunk's cloud as the scatter left it
  uint32_t n_events;               // events of the chunk
  uint32_t event0;                 // first event of the chunk within the track batch (tracks, records)
  uint32_t* seg_count;             // [n_events] segments of every event, zero before summary_count_kernel
  uint32_t* seg_rank;              // [seg_capacity] place of a segment among its event's
  const int64_t* seg_start;        // [n_events + 1] exclusive scan of seg_count
  uint32_t* seg_list;              // [seg_capacity] segment numbers grouped by event
  TrackBuffers trk;                // trk.counts == nullptr: no tracks (attpc_cloud_summary), empty track parts
  int32_t n_sim;
  uint64_t slot_nibbles[2];        // 4 bits per label (16 labels a word): its first position in layout->indices, 15 = none
  double min_electrons;
  const double* pad_centers;       // [>= ATTPC_NUM_PADS][2]
  attpc_event_summary* events;     // [batch events] or nullptr
  attpc_track_summary* tracks;     // [batch events][n_sim] or nullptr
};
// seg_count / seg_rank of the launch's segments (seg_count zeroed by the caller on the same stream)
void launch_summary_count(hipStream_t s, const SummaryArgs& a, uint32_t n_workgroups);
// seg_list from seg_start and seg_rank
void launch_summary_fill(hipStream_t s, const SummaryArgs& a, uint32_t n_workgroups);
// the records of events event0 .. event0 + n_events - 1, plain stores: a repeated chunk overwrites them
void launch_summary_events(hipStream_t s, const SummaryArgs& a, uint32_t n_workgroups);

// selected delivery (select.hip; attpc_select_configure, the contract is in include/attpc_engine.h): the predicate on a
// chunk's records, and the gather that leaves out the segments of the events that failed it.
// The contract's predicate itself, for the device (select_kernel) and for the host (a batch with nothing to scatter).
// A range whose bounds are both open is not evaluated; an evaluated one is lo <= v && v <= hi (false for NaN).
__host__ __device__ inline bool select_in_u32(uint32_t lo, uint32_t hi, int64_t v) {
  return (lo == 0u && hi == 0xffffffffu) || ((int64_t)lo <= v && v <= (int64_t)hi);
}
__host__ __device__ inline bool select_in_f64(double lo, double hi, double v) {
  return (lo == -__builtin_inf() && hi == __builtin_inf()) || (lo <= v && v <= hi);
}
__host__ __device__ inline bool select_passes(const attpc_select_desc& d, const attpc_event_summary& ev,
                                              const attpc_track_summary* tracks, int n_sim) {
#pragma clang fp contract(off)
  const int64_t span = ev.n_kept ? (int64_t)ev.tb_max - (int64_t)ev.tb_min + 1 : 0;
  bool ok = select_in_u32(d.n_kept_lo, d.n_kept_hi, (int64_t)ev.n_kept) &&
            select_in_u32(d.n_pads_lo, d.n_pads_hi, (int64_t)ev.n_pads) &&
            select_in_u32(d.tb_span_lo, d.tb_span_hi, span);
  const bool charge_open = d.charge_lo == INT64_MIN && d.charge_hi == INT64_MAX;
  ok = ok && (charge_open || (d.charge_lo <= ev.charge && ev.charge <= d.charge_hi));
  uint32_t good = 0u;
  for (int s = 0; s < n_sim && tracks != nullptr; ++s) {
    if (!((d.track_mask >> s) & 1u)) continue;
    const attpc_track_summary& t = tracks[s];
    const double xx = t.end_x * t.end_x, yy = t.end_y * t.end_y;  // each product rounded, then added
    const double end_rho2 = xx + yy;
    const bool pass = select_in_u32(d.track_n_kept_lo, d.track_n_kept_hi, (int64_t)t.n_kept) &&
                      select_in_u32(d.track_n_pads_lo, d.track_n_pads_hi, (int64_t)t.n_pads) &&
                      select_in_u32(d.track_n_samples_lo, d.track_n_samples_hi, (int64_t)t.n_samples) &&
                      select_in_f64(d.track_rho2_max_lo, d.track_rho2_max_hi, t.rho2_max) &&
                      select_in_f64(d.track_end_tb_lo, d.track_end_tb_hi, t.end_tb) &&
                      select_in_f64(d.track_end_rho2_lo, d.track_end_rho2_hi, end_rho2);
    good += pass ? 1u : 0u;
  }
  return ok && good >= d.min_tracks;
}

struct SelectArgs {
  attpc_select_desc desc;
  const unsigned long long* ctrl;     // the scatter launch's control words (ScatterWord)
  const attpc_event_summary* events;  // [batch events]
  const attpc_track_summary* tracks;  // [batch events][n_sim] or nullptr (n_sim == 0)
  int32_t n_sim;
  uint32_t n_events;                  // events of the chunk
  uint32_t event0;                    // first event of the chunk within the batch (records, passed)
  const uint32_t* ev_rows;            // [n_events] cloud rows of the chunk's events, or nullptr
  uint8_t* passed;                    // [batch events]
  uint32_t* sel_rows;                 // [n_events] passed ? ev_rows : 0, or nullptr
};
// passed and sel_rows of events event0 .. event0 + n_events - 1, one lane per event
void launch_select(hipStream_t s, const SelectArgs& a);

// run maps (maps.hip; attpc_maps_configure, the contract is in include/attpc_engine.h).  A map on the device is one
// array of MAPS_CELLS u64 cells, the fields of attpc_maps_out one behind the other (the charges as two's complement):
constexpr int MAPS_PAD_EVENTS = 0;
constexpr int MAPS_PAD_CHARGE = MAPS_PAD_EVENTS + ATTPC_NUM_PADS;
constexpr int MAPS_TB_EVENTS = MAPS_PAD_CHARGE + ATTPC_NUM_PADS;
constexpr int MAPS_TB_ROWS = MAPS_TB_EVENTS + ATTPC_NUM_TB;
constexpr int MAPS_TB_CHARGE = MAPS_TB_ROWS + ATTPC_NUM_TB;
constexpr int MAPS_N_HIT = MAPS_TB_CHARGE + ATTPC_NUM_TB;
constexpr int MAPS_CELLS = MAPS_N_HIT + 1;  // 22 017 cells, 172 KiB
struct MapsArgs {
  ChunkView chunk;                 // the chunk's cloud as the scatter left it
  uint32_t n_events;               // events of the chunk
  uint32_t event0;                 // first event of the chunk within the batch (passed)
  const int64_t* seg_start;        // [n_events + 1] and
  const uint32_t* seg_list;        // [seg_capacity]: the segments grouped by event, as the chunk's summary left them
  const uint8_t* passed;           // [batch events] of the selection, or nullptr: every event contributes
  int32_t n_sim;
  uint32_t track_mask;             // bit s: rows of position s count; bit ATTPC_MAX_SIM: rows whose label has no position
  uint64_t slot_nibbles[2];        // as SummaryArgs
  double min_electrons;
  unsigned long long* map;         // [MAPS_CELLS] the chunk's map, zero before the launch
};
// adds the chunk's events (n_events > 0) to a.map (global u64 atomics); max_workgroups: the compute units.  false:
// nothing was launched, the chunk has too many events for the workgroups' u32 cells
bool launch_maps_events(hipStream_t s, const MapsArgs& a, uint32_t max_workgroups);
// total[i] += map[i]
void launch_maps_fold(hipStream_t s, const unsigned long long* map, unsigned long long* total);

// assembly of a scattered chunk and the small kernels of the host pipeline (assemble.hip)
// out[i] = sum of in[0..i), i = 0 .. n.  ctrl (may be null): the scatter launch that produced the counts; all 0 if it overflowed
void launch_exclusive_scan(hipStream_t s, const uint32_t* in, uint32_t n, int64_t* out, const unsigned long long* ctrl);
struct GatherArgs {
  ChunkView chunk;
  int64_t out_capacity;            // rows of out_points / out_labels
  uint32_t n_events;
  uint32_t event0;                 // first event of the chunk within the batch (passed)
  const uint8_t* passed;           // [batch events] (gather_selected_kernel only)
  const int64_t* ev_start;         // [n_events + 1] CSR offsets of the event-ordered arrays
  double* out_points;
  int64_t* out_labels;
};
// segment s to rows ev_start[event] + ev_offset of the event-ordered arrays; `selected`: not those of events that failed
void launch_gather(hipStream_t s, const GatherArgs& a, bool selected, uint32_t n_workgroups);
// the event-ordered cloud as transfer records (PackedRow, or PackedRow8 when `tight`); flag[0] / [1]: a row does not fit
void launch_pack_rows_kernel(hipStream_t s, uint32_t n_workgroups, const int64_t* ev_start, uint32_t n_events,
                             const double* points, const int64_t* labels, PackedRow* packed, int64_t* flag, int tight);
void launch_count_status(hipStream_t s, const int32_t* status, uint32_t n, uint32_t* counter);  // *counter += #{status[i] != 0}

}  // namespace attpc
