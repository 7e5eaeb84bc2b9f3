// abi.hip -- host side of the C ABI (include/attpc_engine.h): context, configuration upload, the
// launch pipeline kinematics -> tracks -> scatter (-> Spyral rows) and output assembly.
//
// HBM layout (N rows/event, S simulated nuclei/event):
//   two TRACK SETS, each for one track batch of B events (up to 8 scatter chunks, T = B*S tracks):
//     p4 f64[B][N][4], vertex f64[B][3], status i32[B], attempts u32[B]          kinematics
//     arena f64[blocks][128][4]  (x, y, time bucket, electrons)                   track samples
//     block_table i32[T][79], counts i32[T], n_steps i32[T]                       track index
//   one CLOUD of one scatter chunk of C events:
//     points f64[cap][3], labels i64[cap], segments {event,count,offset,ev_offset}[..], ev_rows u32[C]
//   two ASSEMBLY SETS (only when clouds are delivered to the host): the chunk's cloud in event order
//     (CSR) or its Spyral rows, filled on the device while the previous chunk's set crosses PCIe.
// Buffers grow on demand and are reused (device-resident mode overwrites the cloud chunk by chunk).
//
// Streams: S (scatter, lone buckets, assembly), T (kinematics + tracks of the NEXT batch, low
// priority: it fills the compute units the persistent scatter workgroups leave at the end of each
// launch), C (device-to-host copies).  The host does not wait per launch: control words of every
// launch are copied to pinned host memory behind it and read once per batch (device-resident) or per
// chunk (delivered clouds, where the copy needs the row total anyway).  A launch whose buffers
// turned out too small is repeated with larger ones (results are deterministic, so a re-run is exact).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "tracks_args.hpp"
#include "trace_pack_host.hpp"
#include "unpack_host.hpp"
#include "spyral_integral.hpp"  // (behind the HIP runtime header)
#include "circle_host.hpp"
#include "fit_host.hpp"
#include "pid_host.hpp"
#include "reaction_host.hpp"
#include "helix_host.hpp"
#include "estimate_host.hpp"
#include "thin_host.hpp"
#include "straggle_host.hpp"
#include "host_args.hpp"

namespace {

using namespace attpc;

constexpr int MAX_SLOTS = 8;           // scatter chunks per track batch
constexpr uint32_t LONE_CAPACITY = 65536;
constexpr int64_t CLOUD_BUDGET_BYTES = 24ll << 30;  // points + labels of one chunk
constexpr int64_t DELIVER_CHUNK_ROWS = 96ll << 20;  // cloud rows of a chunk whose cloud is delivered (3 GB: ~60 ms of PCIe)
constexpr int64_t TRACE_CHUNK_ROWS = 4ll << 20;     // kept pad rows of a chunk of a trace run (4 GiB of samples)
                                                    // (readout modes too: their first chunk is sized by |S| per event)
constexpr uint64_t ARENA_BUDGET_BYTES = 24ull << 30;
constexpr int64_t CHUNK_ROWS = 1 << 20, CHUNK_EVENTS = 65536;  // a chunk of an operator on host rows: whole events up to these (at least one)

struct DevBuf {  // grow-only device buffer (ensure()), freed with its owner
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p), std::swap(bytes, o.bytes); return *this; }  // (o frees ours)
  ~DevBuf() { if (p) (void)hipFree(p); }
};

template <typename T>
struct Pinned {  // page-locked host array of the library, grow-only (ensure_pinned), freed with its owner
  T* p = nullptr;
  size_t n = 0;
  Pinned() = default;
  Pinned(const Pinned&) = delete;
  Pinned& operator=(const Pinned&) = delete;
  ~Pinned() { if (p) (void)hipHostFree(p); }
  T& operator[](size_t i) const { return p[i]; }
};

// The records a stage leaves per event of a trace or trace-row call, for its attpc_*_last: the call's pinned array
// [events][per] in its event order, and which call it answers for (begin_records, chunk_room, copy_chunk, records_last;
// a chunk's records on the device are a DevBuf of its AsmSet: two chunks are in flight).
template <typename T>
struct CallRecords {
  Pinned<T> h;
  size_t per = 0;        // records per event of that call
  int64_t events = -1;   // its events; -1: the call in progress, or the last one, did not make the stream
  bool to_host = false;  // its records are copied to `h` (a spectra-only call keeps them on the device)
  bool made() const { return events >= 0; }
  void off() { events = -1; }
};

struct DevAllocs {  // the device allocations of one configure call (upload()): freed on clear() and with their owner
  std::vector<void*> ptrs;
  DevAllocs() = default;
  DevAllocs(const DevAllocs&) = delete;
  DevAllocs& operator=(const DevAllocs&) = delete;
  ~DevAllocs() { clear(); }
  void clear() { for (void* p : ptrs) (void)hipFree(p); ptrs.clear(); }
};

struct TrackSet {  // kinematics + tracks of one track batch
  DevBuf p4, vertex, status, attempts, arena, block_table, counts, n_steps, ctrl;
  size_t arena_blocks = 0;
  Pinned<uint32_t> h_ctrl;  // [TRK_WORDS]
  hipEvent_t done = nullptr, k0 = nullptr, k1 = nullptr, t0 = nullptr, t1 = nullptr;
  bool timed_kin = false;
};

struct AsmSet {  // one chunk's cloud in event order, or its Spyral rows, or its pad traces
  DevBuf ev_start, points, labels, kept, kept_start, sp_rows, sp_labels;
  DevBuf tr_scratch, tr_info, tr_pads, tr_samples, tr_labels;  // pad traces (traces.hip)
  DevBuf tr_maps;     // readout of noise-only pads: TraceMaps, 3 x TR_MAP_WORDS words per event
  DevBuf tr_gained;   // micromegas gain on (gain.hip): the gained charge of every cloud row of the chunk, f64 [rows]
  DevBuf tr_common;   // common-mode noise on: the values of every (event, group) of the chunk, 1 KiB each (CommonDev)
  size_t tr_cap = 0;  // kept pad rows the trace outputs are kept at (grown with headroom)
  hipEvent_t traced = nullptr;  // the chunk's traces are written (the copies on C wait for it)
  hipEvent_t counted = nullptr; // trace rows: the chunk's points per event are in h_pk_start (the host waits for it)
  // trace rows (peaks.hip): the point map and count of every kept trace row, the scanned offsets of the trace rows and
  // of the events, the points' records and centroids; the rows themselves go to sp_rows / sp_labels
  DevBuf pk_maps, pk_counts, pk_row_start, pk_block_sums, pk_block_start, pk_ev_start, pk_records, pk_centroid;
  size_t pk_cap = 0;           // points the point-sized buffers are kept at (grown with headroom)
  DevBuf pk_y;                 // Fourier baseline on (baseline.hip): the y rows the peak kernels read, int16 [traces][512]
  DevBuf tg_records;           // trigger on (trigger.hip): the chunk's records, attpc_trigger_record [events]
  DevBuf tg_row_pass;          // ... with its gate, trace rows: fired of every kept trace row's event, uint8 [traces]
  DevBuf fit_records;          // track fit on (fit.hip): the chunk's records, attpc_track_fit [events][n_sim]
  DevBuf pid_records;          // particle identification on (pid.hip): the chunk's records, attpc_pid_record [events][n_sim]
  DevBuf hyp_records;          // fit hypotheses on (hypothesis.hip): the chunk's records, attpc_fit_hypothesis [events][n_sim],
  DevBuf hyp_fits;             // ... the fits of every hypothesis, attpc_track_fit [events][n_sim][H],
  DevBuf hyp_assigned;         // ... and, for the reaction reconstruction, the positions as attpc_pid_record [events][n_sim]
  DevBuf rx_records;           // reaction reconstruction on (reaction.hip): the chunk's records, attpc_reaction_record [events]
  DevBuf est_records;          // track estimates on (estimate.hip): the chunk's records, attpc_track_estimate [events][n_sim]
  DevBuf thin_points;          // ... of thinned points (thin.hip): one ThinPoint per trace row (pk_cap)
  DevBuf thin_info;            // ... and the attpc_thin_info of every (event, position)
  DevBuf uc_rows, uc_labels;   // drift correction on (undistort.hip): the chunk's corrected, re-sorted rows and labels (pk_cap)
  DevBuf cl_labels;            // clustering on (cluster.hip): the chunk's cluster labels (pk_cap),
  DevBuf cl_events, cl_records;  // ... its attpc_cluster_event [events] and attpc_cluster_record [events][ATTPC_MAX_SIM]
  DevBuf jn_events, jn_records;  // cluster joining on (cluster_join.hip): attpc_join_event [events], attpc_join_record [events][ATTPC_MAX_SIM]
  Pinned<int64_t> h_pk_start;  // CSR offsets of the chunk's points by event (n + 1 entries)
  // packed traces (trace_pack.hip): the headers and record sizes of every kept trace row, their scanned byte offsets
  // (tp_block_*: the scan's scratch) and the records; the chunk's bytes in pinned memory (the host waits on `counted`)
  DevBuf tp_headers, tp_sizes, tp_row_start, tp_block_sums, tp_block_start, tp_bytes;
  Pinned<int64_t> h_tp_total;  // [1]
  size_t row_cap = 0;  // rows the row-sized buffers of the set are kept at (grown with headroom: a launch's row
                       // capacity follows the observed rows per event and moves by fractions of a percent)
  Pinned<int64_t> h_start;     // CSR offsets of the chunk (n + 1 entries)
  Pinned<uint32_t> h_ev_rows;  // cloud rows of every event before any threshold
  Pinned<int64_t> h_total;     // [2]: [0] != 0: a row of the chunk does not fit the 16-byte transfer record
  hipEvent_t ready = nullptr, copied = nullptr;
  // compact transfer: the chunk's rows as 16-byte records, device and (pinned, library-owned) host side, and the
  // expansion into the caller's arrays that is still to be done once the copy has arrived
  DevBuf packed;
  Pinned<char> h_packed;
  uint64_t unpack_ticket = 0;  // number of the expansion job that last used h_packed (0: none)
};

struct UnpackJob {  // one chunk's records in pinned staging -> the caller's arrays, once `copied` has fired
  hipEvent_t copied = nullptr;
  const void* src = nullptr;
  int64_t rows = 0;
  double* points = nullptr;   // [rows, 3] cloud rows, or [rows, 8] Spyral rows when `spyral`
  int64_t* labels = nullptr;
  bool spyral = false;
  // 8-byte cloud records: what the host needs to regenerate the jitter (the job's own copy of the chunk's CSR
  // offsets: the set's pinned copy is overwritten by the chunk after next while this job may still run)
  bool tight = false;
  uint64_t seed = 0, first_event = 0;
  std::vector<int64_t> offsets;
};

// What a trace-row call settles at its start (begin_trace_row_call) for the stages behind its rows, and the truth of
// the track batch in progress that the reaction reconstruction reads.  No buffers: the streams hold those.
struct TraceRowCall {
  int32_t n_sim = 0;                             // positions of the call's layout (0: it has none)
  int64_t est_slot_label[ATTPC_MAX_SIM] = {};    // their labels (EstimateArgs)
  FitPosition fit_position[ATTPC_MAX_SIM] = {};  // their nuclei
  int32_t pid_species[ATTPC_MAX_SIM] = {};       // their species
  HypLayout hyp{};                               // the fit hypotheses of the layout (n == 0: the stage does not run)
  ClusterSettings cluster{};                     // the clustering's settings with the call's layout
  JoinSettings join{};                           // the joining's
  int64_t cluster_rows = -1;       // the delivered rows whose cluster labels are in h_cl_labels so far (-1: it fetches none)
  const double *rx_p4 = nullptr, *rx_vertex = nullptr;  // the truth of the track batch in progress on the device: p4
                                   // [events][rx_n_rows][4], vertex [events][3],
  const int32_t* rx_status = nullptr;  // the kinematics status [events] (nullptr: host kinematics, all 0);
  uint64_t rx_batch_first = 0;     // the batch's first event in the call's order
  int32_t rx_n_rows = 0;
};

}  // namespace

struct attpc_ctx {
  int device = 0;
  int n_cus = 256;                 // compute units
  hipStream_t stream = nullptr;    // S
  hipStream_t stream_t = nullptr;  // T (== stream when the option "serial_tracks" is on)
  hipStream_t stream_t_own = nullptr;  // the low-priority stream the context created
  hipStream_t stream_c = nullptr;  // C
  std::string error;
  int32_t chunk_events = 65536;
  int opt_variant = 0;             // 0 auto, 1 small, 2 big, 3 wide (u64 sums)
  bool opt_tiny = false;
  bool opt_spectra_only = false;   // option "reaction_spectra_only": a trace-row call with the reaction reconstruction copies no records to the host
  int opt_compact = 2;             // delivered clouds cross PCIe as 8-byte (2) / 16-byte (1) records and are expanded
                                   // by host threads, or in the reference's dtypes (0)
  int opt_unpack_threads = 0;      // 0: min(32, half of the hardware threads)
  int opt_deliver_chunk = 8192;    // events per chunk when clouds are delivered (the pipeline's fill and drain time)
  int opt_merge = -1;              // scatter kernel's merge variant: -1 automatic (path-length dE/dx step), 0 never, 1 always
  int opt_first_batch_chunks = 0;  // > 0: the first track batch of a call spans at most this many scatter chunks
  int opt_track_species_major = 1; // tracks handed out nucleus by nucleus, lightest species first (0: event by event)
  int opt_track_blocks_per_cu = 8; // track_kernel workgroups (256 threads) launched per CU at most
  int opt_serial_tracks = -1;      // -1 automatic (see pick_track_stream), 0 beside the scatter launches, 1 behind them
  int opt_trace_pack_workgroups = 0;  // workgroups of the trace pack kernels at most; 0: 8 per CU
  int opt_track_workgroups = 0;    // > 0: track_kernel workgroups at most (test hook: few waves, many tracks per lane)

  bool kin_ready = false;
  attpc_kin_desc kin{};            // device pointers inside
  DevAllocs kin_allocs;

  bool det_ready = false;
  DetDev det{};
  DevAllocs det_allocs;
  bool straggle_on = false;        // attpc_det_configure_straggling (kept over attpc_det_configure)
  attpc_straggle_desc straggle{};
  bool distort_on = false;         // attpc_det_configure_distortion (kept over attpc_det_configure)
  DistortMap distort{};            // the tables on the device
  DevAllocs distort_allocs;

  TrackSet tset[2];
  // cloud of one chunk
  DevBuf points, labels, segments, ev_rows, lone_list, lone_chg, lone_mask, out_ctrl, merge_scratch;
  Pinned<unsigned long long> h_out_ctrl;  // [MAX_SLOTS][CTRL_WORDS]
  hipEvent_t s0[MAX_SLOTS] = {}, s1[MAX_SLOTS] = {};
  int64_t cloud_capacity = 0, seg_capacity = 0;
  AsmSet aset[2];
  DevBuf sort_idx, sort_key;
  // running estimates that size the next launches (reset by configure)
  double rows_per_event = 0.0;     // observed cloud rows per event, 0 = unknown
  double segs_per_event = 0.0;
  double blocks_per_track = 0.0;   // observed arena blocks per track
  bool prefer_big = false;         // sticky: the small scatter variant met too many lone buckets
  bool prefer_wide = false;        // sticky: u32 sums per table slot are not enough for this detector (scatter_wide.hip)
  bool slot_wide[MAX_SLOTS] = {};        // per control-word slot: the launch queued last used the wide build
  bool lone_ready = false;         // lone_bucket_kernel's tables are allocated AND their zeroing has been queued
  uint64_t n_growths = 0;          // device buffers (re)allocated so far (a steady workload stops growing)
  uint64_t device_bytes = 0;       // bytes of the grow-only device buffers (ensure()) held right now
  int64_t launch_row_cap = 0;      // row capacity given to the scatter launch queued last (<= cloud_capacity)
  uint32_t max_batch_events = 0;   // largest track batch so far: both track sets are sized for it (the set that
                                   // first meets the shorter last batch of a call would otherwise grow in the next call)

  // attpc_sim_hint_next: the call after the one that comes next.  `hint_*` is what the caller announced; once the
  // run it was given to has queued that call's first track batch (behind its own last scatter launches) `pre_valid`
  // says which track set holds it.
  bool hint_valid = false, pre_valid = false;
  uint64_t hint_seed = 0, hint_first = 0, hint_n = 0;
  attpc_event_layout hint_lay{};
  int pre_set = 0;
  uint64_t pre_seed = 0, pre_first = 0;
  uint32_t pre_nb = 0;
  attpc_event_layout pre_lay{};

  bool spyral_ready = false;
  SpyralDev spyral{};
  bool trace_ready = false;
  TraceDev trace{};
  DevAllocs trace_allocs;
  bool noise_on = false;           // attpc_trace_configure_noise: noise and / or pedestals on (the NOISE kernels)
  TraceNoiseDev noise{};
  DevAllocs noise_allocs;
  std::vector<uint32_t> noise_cdf;  // host copy of the noise cdf [n_levels - 1] (the readout's cutoff)
  bool gain_on = false;            // attpc_trace_configure_gain
  GainDev gain{};
  DevAllocs gain_allocs;
  bool common_on = false;          // attpc_trace_configure_common_mode
  TraceNoiseDev common_table{};    // the stage's own noise table (no pedestals), domain DOMAIN_TRACE_COMMON | stream
  const uint8_t* common_groups = nullptr;  // [ATTPC_NUM_PADS] on the device, or nullptr = every pad in group 0
  int32_t common_n_groups = 0;     // 1 + the highest group of the map
  DevAllocs common_allocs;
  int32_t readout_mode = ATTPC_READOUT_HIT;  // attpc_trace_configure_readout
  int64_t readout_pads = 0;        // |S|
  const uint32_t* readout_channels = nullptr;  // [TR_MAP_WORDS] bitmap of S on the device
  DevAllocs readout_allocs;
  DevBuf trace_sums;               // [2] sample / pad checksums of the trace run in progress
  bool peaks_on = false;           // attpc_trace_configure_peaks
  PeakDev peaks{};
  DevBuf peak_sums;                // [1] row checksum of the trace-row run in progress
  bool baseline_on = false;        // attpc_trace_configure_baseline
  DevBuf bl_twiddle;               // [512] (cos, sin) of 2 pi j / 512, uploaded once (baseline.hip)
  DevBuf bl_filter;                // [512] the configured filter in the transform's order
  DevBuf bl_op_filter;             // [512] the filter of attpc_trace_baseline's last call,
  double bl_op_scale = 0.0;        // and its window scale (0: none yet): a call with the same scale uploads nothing
  bool trigger_on = false;         // attpc_trace_configure_trigger
  TriggerDev trigger{};
  bool trigger_gate = false;
  DevBuf tg_groups;                // [ATTPC_NUM_PADS] the configured group map (trigger.groups points here, or is nullptr)
  DevBuf tg_op_groups;             // [ATTPC_NUM_PADS] the map of attpc_trigger_rows' last call
  CallRecords<attpc_trigger_record> tg_records;  // of the last trace or trace-row call, [events]
  bool estimates_on = false;       // attpc_trace_configure_estimates
  attpc_estimate_desc estimates{};
  TraceRowCall call;               // the trace-row call in progress, or the last one
  CallRecords<attpc_track_estimate> est_records;  // of the last trace-row call, [events][n_sim], as are the streams below
  bool thinning_on = false;        // attpc_trace_configure_thinning (inert while the estimates are off)
  attpc_thin_desc thinning{};
  bool circle_on = false;          // attpc_trace_configure_circle (inert while the estimates are off)
  attpc_circle_desc circle{};
  bool helix_on = false;           // attpc_trace_configure_helix (inert while the estimates are off)
  attpc_helix_desc helix{};
  bool fit_on = false;             // attpc_trace_configure_fit (inert while the estimates are off)
  attpc_fit_desc fit{};
  CallRecords<attpc_track_fit> fit_records;  // [events][n_sim]
  DevBuf fit_scratch;              // the trials' residuals (FitArgs::scratch), shared by the chunks: they run in stream order
  bool pid_on = false;             // attpc_trace_configure_pid (inert while the estimates are off)
  attpc_pid_desc pid{};
  DevBuf pid_gates;                // the gates on the device (PidGates), filled by the configure call
  CallRecords<attpc_pid_record> pid_records;  // [events][n_sim]
  bool hyp_on = false;             // attpc_trace_configure_hypotheses (inert while the estimates or the fit are off)
  attpc_hypothesis_desc hyp{};
  CallRecords<attpc_fit_hypothesis> hyp_records;  // [events][n_sim]
  CallRecords<attpc_track_fit> hyp_fits;          // [events][n_sim * H]
  bool reaction_on = false;        // attpc_reaction_configure (inert while its source is off)
  attpc_reaction_desc reaction{};  // (eloss: nullptr, the table is in rx_eloss)
  DevBuf rx_eloss;                 // the table on the device, filled by the configure call
  DevBuf rx_cells;                 // the spectra of the trace-row call in progress, u64 [reaction_cells]
  CallRecords<attpc_reaction_record> rx_records;  // [events] (made and not to_host: the call left its spectra alone)
  std::vector<uint64_t> h_rx_cells;          // its spectra
  bool summary_on = false;         // attpc_summary_configure
  double summary_min = 0.0;        // min_electrons (kept: q >= it)
  const double* summary_centers = nullptr;  // [n_pads][2] on the device, the mode's own copy
  DevAllocs summary_allocs;
  // summaries of a batch (summary.hip): the records, and per chunk the segments grouped by event
  DevBuf sm_events, sm_tracks, sm_seg_count, sm_seg_rank, sm_seg_start, sm_seg_list, sm_host_segs, sm_host_ctrl;
  bool select_on = false;          // attpc_select_configure
  attpc_select_desc select{};
  // selected delivery (select.hip): passed of a batch's events, the selected rows of a chunk's events, and passed of
  // a call's events on the host (counted there, then copied to the caller's array if there is one)
  DevBuf sel_passed, sel_rows;
  std::vector<uint8_t> sel_host;
  bool maps_on = false;            // attpc_maps_configure
  attpc_maps_desc maps{};
  // run maps (maps.hip): one map per control-word slot [MAX_SLOTS][MAPS_CELLS], the chunk in that slot's own, and the
  // totals of the call in progress [MAPS_CELLS]
  DevBuf mp_slots, mp_total;
  bool correction_on = false;      // attpc_trace_configure_correction
  UndistortSettings correction{};  // the map's tables on the device
  DevAllocs correction_allocs;
  DevBuf uc_xyt;                   // [rows][3] the corrected points of the chunk being corrected (undistort.hip's scratch)
  DevBuf uc_sums;                  // [4] the counts of the trace-row run in progress
  bool correction_call = false;    // attpc_correction_last: the stage was on for the last trace-row call, and its counts
  attpc_undistort_info last_correction{};
  bool cluster_on = false;         // attpc_trace_configure_clustering
  attpc_cluster_desc cluster{};
  DevBuf cl_scratch;               // [rows][CLUSTER_SCRATCH_WORDS] the per-row state of the chunk being clustered (cluster.hip)
  CallRecords<attpc_cluster_event> cl_events;     // [events]
  CallRecords<attpc_cluster_record> cl_records;   // [events][ATTPC_MAX_SIM]
  Pinned<int64_t> h_cl_labels;     // attpc_cluster_labels_last: the cluster labels of the call's delivered rows (call.cluster_rows)
  bool join_on = false;            // attpc_trace_configure_cluster_join
  attpc_join_desc join{};
  CallRecords<attpc_join_event> jn_events;     // [events]
  CallRecords<attpc_join_record> jn_records;   // [events][ATTPC_MAX_SIM]
  int64_t last_rows = 0;           // attpc_trace_rows_last: rows and row checksum of the last trace-row call
  uint64_t last_row_checksum = 0;
  double trace_rows_per_event = 0.0;  // observed kept pad rows per event (bounds the chunks of a trace run)
  DevAllocs spyral_allocs;
  std::vector<double> h_pad_centers, h_pad_sizes;  // host copies: the expansion of compact Spyral records needs them
  DevBuf scratch[8];
  std::vector<void*> host_allocs;  // attpc_host_alloc

  // expansion of compact transfer records: one helper thread takes the jobs in order (it waits for the copy,
  // then fans the rows out over worker threads), so that the thread driving the GPU never stands in a memcpy
  // while the copy engine waits for its next order
  std::thread unpacker;
  std::mutex unpack_mutex;
  std::condition_variable unpack_cv;
  std::deque<UnpackJob> unpack_jobs;
  uint64_t unpack_submitted = 0, unpack_done = 0;
  bool unpack_stop = false, unpack_failed = false;

  ~attpc_ctx() {  // (attpc_ctx_destroy has stopped everything first; the DevBuf / Pinned / DevAllocs members free themselves)
    for (void* p : host_allocs) (void)hipHostFree(p);
  }
};

namespace {

int32_t fail(attpc_ctx* ctx, int32_t code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (ctx) ctx->error = buf;
  return code;
}

#define HIP_TRY(ctx, call)                                                                     \
  do {                                                                                         \
    hipError_t err__ = (call);                                                                 \
    if (err__ != hipSuccess)                                                                   \
      return fail(ctx, ATTPC_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(err__), \
                  __FILE__, __LINE__);                                                         \
  } while (0)

// grow-only device buffer; the caller makes sure nothing in flight uses it when it has to grow
int32_t ensure(attpc_ctx* ctx, DevBuf& b, size_t bytes) {
  if (bytes <= b.bytes) return ATTPC_OK;
  ctx->n_growths++;
#ifdef ATTPC_DEBUG_GROWTH  // (diagnostic builds only, tools/build_variant.sh: which buffer is re-allocated, and when)
  fprintf(stderr, "[attpc grow] buffer at +%zu of the context: %zu -> %zu bytes\n",
          (size_t)(reinterpret_cast<const char*>(&b) - reinterpret_cast<const char*>(ctx)), b.bytes, bytes);
#endif
  if (b.p) HIP_TRY(ctx, hipFree(b.p));
  ctx->device_bytes -= b.bytes;
  b.p = nullptr;
  b.bytes = 0;
  HIP_TRY(ctx, hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  ctx->device_bytes += bytes;
  return ATTPC_OK;
}

// ... given back (a stage turned off): nothing in flight uses it
void release(attpc_ctx* ctx, DevBuf& b) {
  ctx->device_bytes -= b.bytes;
  b = DevBuf{};
}

// Staging of an operator on host arrays: scratch slot `k` as `n` elements of T, grow-only like ensure() -- the byte count
// is formed here and nowhere else.  `rc` is the operator's status: a call does nothing once it is set and sets it when it
// fails, so an operator names its buffers one after the other and looks at rc once before the launch.
template <typename T>
T* stage(attpc_ctx* ctx, int k, size_t n, int32_t& rc) {
  if (!rc) rc = ensure(ctx, ctx->scratch[k], n * sizeof(T));
  return rc ? nullptr : static_cast<T*>(ctx->scratch[k].p);
}

// ... filled with host[0 .. n) by a copy on S (`room` > n: the elements the slot holds at least, also for a chunk without rows)
template <typename T>
const T* stage_in(attpc_ctx* ctx, int k, const T* host, size_t n, int32_t& rc, size_t room = 0) {
  T* dev = stage<T>(ctx, k, std::max(n, room), rc);
  if (!rc && n)
    rc = [&]() -> int32_t {
      HIP_TRY(ctx, hipMemcpyAsync(dev, host, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
      return ATTPC_OK;
    }();
  return dev;
}

// n elements of a staged result back to the host, by a copy on S
template <typename T>
int32_t stage_out(attpc_ctx* ctx, T* host, const T* dev, size_t n) {
  HIP_TRY(ctx, hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
  return ATTPC_OK;
}

// What a stage behind the trace rows reads of a chunk of events: their CSR starts and the rows and labels these name.
struct ChunkRows {
  const int64_t* ev_start;  // [events + 1]
  const double* rows;       // [rows][8]
  const int64_t* labels;    // [rows], or nullptr: none
  template <typename Args>
  void into(Args& a) const { a.ev_start = ev_start; a.rows = rows; a.labels = labels; }
};

// Events e0 .. e1 of a host-row operator staged as its next chunk: their starts in scratch slot 2 (also left in
// `start`), their rows in slot 0 and their labels in slot 1, each slot with room for one row at least.  Labels that are
// nullptr: with `optional_labels` the operator works without them and reads nullptr; otherwise it has refused a call
// with rows and no labels, so no chunk has a row, and the slot is there all the same.
inline ChunkRows stage_rows(attpc_ctx* ctx, const int64_t* offsets, int64_t e0, int64_t e1, const double* rows,
                            const int64_t* labels, std::vector<int64_t>* start, int32_t& rc, bool optional_labels = false) {
  const size_t n_rows = (size_t)(offsets[e1] - offsets[e0]);
  chunk_starts(offsets, e0, e1, start);
  ChunkRows in{};
  in.ev_start = stage_in(ctx, 2, start->data(), (size_t)(e1 - e0) + 1, rc);
  in.rows = stage_in(ctx, 0, n_rows ? rows + offsets[e0] * 8 : nullptr, n_rows * 8, rc, 8);
  if (labels || !optional_labels) in.labels = stage_in(ctx, 1, n_rows ? labels + offsets[e0] : nullptr, n_rows, rc, 1);
  return in;
}

// grow-only pinned host array: at least `n` elements, re-allocated at `alloc` (with headroom, if larger) when it grows;
// the caller makes sure no copy in flight uses it then
template <typename T>
int32_t ensure_pinned(attpc_ctx* ctx, Pinned<T>& b, size_t n, size_t alloc = 0) {
  if (n <= b.n) return ATTPC_OK;
  if (b.p) HIP_TRY(ctx, hipHostFree(b.p));
  b.p = nullptr;
  b.n = 0;
  alloc = std::max(alloc, n);
  HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void**>(&b.p), alloc * sizeof(T), hipHostMallocDefault));
  b.n = alloc;
  return ATTPC_OK;
}

template <typename T>
int32_t upload(attpc_ctx* ctx, DevAllocs& owner, const T* host, size_t n, const T** dev) {
  void* p = nullptr;
  HIP_TRY(ctx, hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
  owner.ptrs.push_back(p);
  if (n) HIP_TRY(ctx, hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
  *dev = static_cast<const T*>(p);
  return ATTPC_OK;
}

// The tables of baseline.hip.  filter: F[k] = sinc(w_k / scale), w_k = k below 256 and k - 512 from there on, divided by
// 512 (the inverse transform's factor: exact) and in the order the kernel's lanes hold the spectrum.
void baseline_filter(double scale, double* filter) {
  const long double pi = 3.14159265358979323846264338327950288L;
  for (int k = 0; k < ATTPC_NUM_TB; ++k) {
    const long double t = (long double)(k < ATTPC_NUM_TB / 2 ? k : k - ATTPC_NUM_TB) / (long double)scale;
    const long double f = t == 0.0L ? 1.0L : std::sin(pi * t) / (pi * t);
    const int k0 = k & 7, k1 = (k >> 3) & 7, k2 = k >> 6;
    filter[64 * k2 + 8 * k0 + k1] = (double)f / (double)ATTPC_NUM_TB;
  }
}

// twiddle / filter on the device: the former once per context, the latter `scale`'s into `buf`
int32_t upload_baseline_tables(attpc_ctx* ctx, DevBuf& buf, double scale) {
  int32_t rc;
  if (!ctx->bl_twiddle.p) {
    const long double pi = 3.14159265358979323846264338327950288L;
    std::vector<double> tw(2 * ATTPC_NUM_TB);
    for (int j = 0; j < ATTPC_NUM_TB; ++j) {
      tw[2 * j] = (double)std::cos(2.0L * pi * (long double)j / (long double)ATTPC_NUM_TB);
      tw[2 * j + 1] = (double)std::sin(2.0L * pi * (long double)j / (long double)ATTPC_NUM_TB);
    }
    if ((rc = ensure(ctx, ctx->bl_twiddle, tw.size() * sizeof(double)))) return rc;
    HIP_TRY(ctx, hipMemcpy(ctx->bl_twiddle.p, tw.data(), tw.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  std::vector<double> filter(ATTPC_NUM_TB);
  baseline_filter(scale, filter.data());
  if ((rc = ensure(ctx, buf, filter.size() * sizeof(double)))) return rc;
  HIP_TRY(ctx, hipMemcpy(buf.p, filter.data(), filter.size() * sizeof(double), hipMemcpyHostToDevice));
  return ATTPC_OK;
}

int32_t sync_all(attpc_ctx* ctx) {
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream_t));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream_c));
  return ATTPC_OK;
}

// how a configure call opens: its device selected and nothing in flight on any stream
int32_t begin_configure(attpc_ctx* ctx) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return sync_all(ctx);
}

// ATTPC_E_INVALID for what a check of host_args.hpp found (a refusal without a text leaves the last error as it was)
int32_t refuse(attpc_ctx* ctx, const ArgError& bad) {
  return bad.text.empty() ? ATTPC_E_INVALID : fail(ctx, ATTPC_E_INVALID, "%s", bad.text.c_str());
}

// attpc_trace_configure_* of a stage that is a flag and a descriptor of the context (`on`, `stored`): `d` checked by
// `desc_error` (its refusals start with `what`), nothing in flight, then stored; nullptr turns the stage off.
template <typename Desc>
int32_t configure_desc(attpc_ctx* ctx, const Desc* d, const char* (*desc_error)(const Desc&), const char* what,
                       bool attpc_ctx::*on, Desc attpc_ctx::*stored) {
  if (!ctx) return ATTPC_E_INVALID;
  if (d)
    if (const char* bad = desc_error(*d)) return fail(ctx, ATTPC_E_INVALID, "%s: %s", what, bad);
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  ctx->*on = d != nullptr;
  if (d) ctx->*stored = *d;
  return ATTPC_OK;
}

// ATTPC_E_INVALID under the name `func` for a number of track positions outside 0 .. ATTPC_MAX_SIM
int32_t n_sim_range(attpc_ctx* ctx, const char* func, int32_t n_sim) {
  if (n_sim >= 0 && n_sim <= ATTPC_MAX_SIM) return ATTPC_OK;
  return fail(ctx, ATTPC_E_INVALID, "%s: n_sim %d outside 0 .. %d", func, n_sim, ATTPC_MAX_SIM);
}

// attpc_*_last under the name `func`: records first .. first + count of a call of `events` events, `per_event` of them
// per event, from the call's pinned array `src` to `dst` (nullptr: refused if `required`, else not wanted)
template <typename Record>
int32_t copy_last(attpc_ctx* ctx, const char* func, int64_t first, int64_t count, int64_t events, size_t per_event,
                  const Record* src, Record* dst, bool required = true) {
  if (const ArgError bad = records_range_error(func, first, count, events)) return refuse(ctx, bad);
  if (count == 0 || per_event == 0) return ATTPC_OK;
  if (!dst) return required ? ATTPC_E_INVALID : ATTPC_OK;
  std::memcpy(dst, src + (size_t)first * per_event, (size_t)count * per_event * sizeof(Record));
  return ATTPC_OK;
}

// The start of a call of `n` events that makes the stream `r`, `per` records per event: pinned room for them (none if
// they stay on the device), then the stream is the call's.  Nothing of an earlier call is in flight.
template <typename T>
int32_t begin_records(attpc_ctx* ctx, CallRecords<T>& r, uint64_t n, size_t per, bool to_host = true) {
  r.off();
  const int32_t rc = ensure_pinned(ctx, r.h, to_host ? std::max<size_t>((size_t)n * per, 1) : 0);
  if (rc) return rc;
  r.per = per;
  r.events = (int64_t)n;
  r.to_host = to_host;
  return ATTPC_OK;
}

// Room for the records of a chunk of `n` events of the stream in `dev`, the set's buffer for them (`rc` as stage()).
template <typename T>
T* chunk_room(attpc_ctx* ctx, const CallRecords<T>& r, DevBuf& dev, uint32_t n, int32_t& rc) {
  if (!rc) rc = ensure(ctx, dev, (size_t)n * r.per * sizeof(T));
  return rc ? nullptr : static_cast<T*>(dev.p);
}

// ... and their copy to events first_local .. of the call's pinned array, on C (the caller has made C wait for them):
// nothing if the call does not make the stream or keeps it on the device.
template <typename T>
int32_t copy_chunk(attpc_ctx* ctx, const CallRecords<T>& r, const DevBuf& dev, uint64_t first_local, uint32_t n) {
  if (!r.made() || !r.to_host || !n || !r.per) return ATTPC_OK;
  HIP_TRY(ctx, hipMemcpyAsync(r.h.p + (size_t)first_local * r.per, dev.p, (size_t)n * r.per * sizeof(T), hipMemcpyDeviceToHost,
                              ctx->stream_c));
  return ATTPC_OK;
}

// attpc_*_last under the name `func`: records first .. first + count of the stream to `out` (copy_last), or
// ATTPC_E_NOTCONFIGURED with `why` if the last call did not make the stream or kept it on the device.
template <typename T>
int32_t records_last(attpc_ctx* ctx, const CallRecords<T>& r, const char* func, const char* why, int64_t first, int64_t count,
                     T* out, bool required = true) {
  if (!r.made() || !r.to_host) return fail(ctx, ATTPC_E_NOTCONFIGURED, "%s: %s", func, why);
  return copy_last(ctx, func, first, count, r.events, r.per, r.h.p, out, required);
}

// A first track batch queued ahead for a call that does not come (another entry point, other events, a new
// configuration): let it finish and forget it.
int32_t drop_prefetch(attpc_ctx* ctx) {
  ctx->hint_valid = false;
  if (!ctx->pre_valid) return ATTPC_OK;
  ctx->pre_valid = false;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream_t));
  return ATTPC_OK;
}

bool same_layout(const attpc_event_layout& a, const attpc_event_layout& b) {
  if (a.n_rows != b.n_rows || a.n_sim != b.n_sim) return false;
  for (int i = 0; i < a.n_sim; ++i)
    if (a.indices[i] != b.indices[i]) return false;
  for (int i = 0; i < a.n_rows; ++i)
    if (a.species_of_row[i] != b.species_of_row[i]) return false;
  return true;
}

// Where the kinematics + tracks of the NEXT batch run while the current one is scattered: on the scatter stream itself,
// behind its launches (serial), or beside them on the low-priority stream.  Both kernels are bound by instruction issue;
// beside the default scatter kernel the track kernel (170 VGPRs, 2 waves per SIMD) displaces co-resident scatter
// workgroups and costs more than it hides (headline: 171.6 ms per step beside, 166.5 behind) -- beside the merge variant
// of the path-length step, where track integration is a quarter of the device time and the scatter kernel leaves more
// idle issue slots, it pays (configs[4]: 1.80e5 events/s beside, 1.61e5 behind).  Nothing may be in flight when it changes.
void pick_track_stream(attpc_ctx* ctx) {
  const bool serial = ctx->opt_serial_tracks >= 0 ? ctx->opt_serial_tracks != 0 : !(ctx->det_ready && ctx->det.path_step > 0.0);
  ctx->stream_t = serial ? ctx->stream : ctx->stream_t_own;
}

// event ids first_event .. first_event + n_events - 1 must all lie in [0, 2^64) (include/attpc_engine.h): a range that
// wraps would silently reuse the streams of events 0, 1, ...
int32_t validate_id_range(attpc_ctx* ctx, uint64_t first_event, uint64_t n_events) {
  if (n_events != 0 && n_events - 1 > ~0ull - first_event)
    return fail(ctx, ATTPC_E_INVALID, "event ids %llu + %llu events pass 2^64", (unsigned long long)first_event,
                (unsigned long long)n_events);
  return ATTPC_OK;
}

int32_t validate_layout(attpc_ctx* ctx, const attpc_event_layout* lay, bool with_species) {
  if (!lay || lay->n_rows < 1 || lay->n_rows > ATTPC_MAX_ROWS || lay->n_sim < 0 || lay->n_sim > ATTPC_MAX_SIM)
    return fail(ctx, ATTPC_E_INVALID, "bad event layout");
  for (int i = 0; i < lay->n_sim; ++i) {
    const int row = lay->indices[i];
    if (row < 0 || row >= lay->n_rows) return fail(ctx, ATTPC_E_INVALID, "indices[%d]=%d out of range", i, row);
    const int sp = lay->species_of_row[row];
    if (with_species && sp >= ctx->det.n_species) return fail(ctx, ATTPC_E_INVALID, "species_of_row[%d]=%d out of range", row, sp);
  }
  return ATTPC_OK;
}

// momentum rows per event of the configured kinematics
int kin_rows(const attpc_ctx* ctx) { return 4 + 2 * (ctx->kin.n_steps - 1); }

struct ChunkResult {
  unsigned long long rows = 0, reserved = 0, segs = 0, charge = 0, keys = 0, failed = 0, retried = 0, samples = 0,
                     mismatch = 0, lone = 0, danger = 0;
  bool overflow = false;
  float ms_scatter = 0;
};

// ------------------------------------------------------------------ tracks ----
int32_t ensure_kin_buffers(attpc_ctx* ctx, TrackSet& ts, uint32_t n, int n_rows) {
  int32_t rc;
  ctx->max_batch_events = std::max(ctx->max_batch_events, n);
  n = ctx->max_batch_events;
  if ((rc = ensure(ctx, ts.p4, (size_t)n * n_rows * 4 * sizeof(double)))) return rc;
  if ((rc = ensure(ctx, ts.vertex, (size_t)n * 3 * sizeof(double)))) return rc;
  if ((rc = ensure(ctx, ts.status, (size_t)n * sizeof(int32_t)))) return rc;
  if ((rc = ensure(ctx, ts.attempts, (size_t)n * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, ts.ctrl, TRK_WORDS * sizeof(uint32_t)))) return rc;
  return ATTPC_OK;
}

TrackBuffers track_buffers(const TrackSet& ts) {  // the device view of a track set
  return TrackBuffers{static_cast<double*>(ts.arena.p), static_cast<int32_t*>(ts.block_table.p), static_cast<int32_t*>(ts.counts.p),
                      static_cast<int32_t*>(ts.n_steps.p), static_cast<uint32_t*>(ts.ctrl.p),
                      (uint32_t)std::min<size_t>(ts.arena_blocks, 0xFFFFFFFFu)};
}

struct TrackLaunch {  // what launch_tracks queued, for finish_tracks
  attpc_event_layout lay{};
  uint64_t seed = 0, first_event = 0;
  uint32_t n = 0;
  bool use_status = false;
};

// Queue the track integration of a BATCH of `n` events whose kinematics are (being) written to the
// set's p4 / vertex (/ status) on stream T.  A batch spans several scatter chunks: the track kernel
// hands tracks to lanes dynamically, and with fewer tracks than a few times the 200 k lanes of the
// chip the launch is one generation of tracks whose length is set by its longest member.
int32_t launch_tracks(attpc_ctx* ctx, TrackSet& ts, const TrackLaunch& tl) {
  const uint32_t n_tracks = tl.n * (uint32_t)tl.lay.n_sim;
  int32_t rc;
  if ((rc = ensure(ctx, ts.ctrl, TRK_WORDS * sizeof(uint32_t)))) return rc;
  HIP_TRY(ctx, hipMemsetAsync(ts.ctrl.p, 0, TRK_WORDS * sizeof(uint32_t), ctx->stream_t));
  if (n_tracks) {
    ctx->max_batch_events = std::max(ctx->max_batch_events, tl.n);
    const size_t alloc_tracks = (size_t)ctx->max_batch_events * (size_t)tl.lay.n_sim;
    if ((rc = ensure(ctx, ts.block_table, alloc_tracks * MAX_BLOCKS_PER_TRACK * sizeof(int32_t)))) return rc;
    if ((rc = ensure(ctx, ts.counts, alloc_tracks * sizeof(int32_t)))) return rc;
    if ((rc = ensure(ctx, ts.n_steps, alloc_tracks * sizeof(int32_t)))) return rc;
    const size_t lds = (size_t)ctx->det.n_species * ATTPC_DEDX_NODES * sizeof(double);
    const uint32_t waves_needed = (n_tracks + 63) / 64;
    uint32_t blocks = std::min<uint32_t>((waves_needed + 3) / 4, (uint32_t)ctx->n_cus * (uint32_t)ctx->opt_track_blocks_per_cu);
    if (ctx->opt_track_workgroups > 0) blocks = std::min<uint32_t>(blocks, (uint32_t)ctx->opt_track_workgroups);
    // every wave reserves arena blocks 64 at a time: that slack comes on top of what the samples need
    // keep the arena while it covers the observed need with 3 % to spare, grow it by 25 % when it does not:
    // the need per track moves by fractions of a percent from batch to batch, and re-allocating tens of GB
    // for each such step costs more than the kernels (a too small arena is caught and the batch repeated)
    const size_t pools = (size_t)blocks * 4 * 64 + 1024;
    const double bpt = ctx->blocks_per_track;
    const size_t need_blocks = bpt > 0.0 ? (size_t)((double)n_tracks * (bpt * 1.03 + 0.05)) + pools : (size_t)n_tracks * 3 + pools;
    size_t want_blocks = ts.arena_blocks;
    if (need_blocks > ts.arena_blocks)
      want_blocks = bpt > 0.0 ? (size_t)((double)n_tracks * (bpt * 1.25 + 0.25)) + pools : need_blocks;
    if (ctx->opt_tiny && ts.arena_blocks == 0) want_blocks = 4;  // test hook: grow-and-rerun path
    if ((rc = ensure(ctx, ts.arena, want_blocks * ARENA_BLK * 4 * sizeof(double)))) return rc;
    ts.arena_blocks = want_blocks;
    TrackArgs ta;
    ta.det = ctx->det;
    ta.layout = tl.lay;
    ta.buf = track_buffers(ts);
    ta.p4 = static_cast<const double*>(ts.p4.p);
    ta.vertex = static_cast<const double*>(ts.vertex.p);
    ta.kin_status = tl.use_status ? static_cast<const int32_t*>(ts.status.p) : nullptr;
    ta.seed = tl.seed;
    ta.first_event = tl.first_event;
    ta.n_events = tl.n;
    ta.n_tracks = n_tracks;
    {  // lightest species first (they travel farthest): the kernel's last tracks are then the short ones
      int order[ATTPC_MAX_SIM];
      const int n_sim = tl.lay.n_sim;
      for (int i = 0; i < n_sim; ++i) order[i] = i;
      auto weight = [&](int isim) -> double {
        const int sp = tl.lay.species_of_row[tl.lay.indices[isim]];
        return sp < 0 ? 1.0e30 : (double)ctx->det.Z[sp] * 1.0e6 + ctx->det.mass[sp];  // by charge, then by mass
      };
      std::stable_sort(order, order + n_sim, [&](int x, int y) { return weight(x) < weight(y); });
      for (int i = 0; i < ATTPC_MAX_SIM; ++i) ta.sim_order[i] = (uint8_t)(i < n_sim ? order[i] : 0);
      if (!ctx->opt_track_species_major || n_sim <= 1) ta.sim_order[0] = 0xffu;
    }
    HIP_TRY(ctx, hipEventRecord(ts.t0, ctx->stream_t));
    launch_track_kernel(blocks, lds, ctx->stream_t, ta, ctx->straggle_on ? &ctx->straggle : nullptr);
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->distort_on) {
      // the drift distortion of the batch's records, in place and here only: once per run of the track kernel,
      // however often the batch is scattered; a batch run again for a larger arena passes here again
      uint32_t limit = (uint32_t)ctx->n_cus * (uint32_t)ctx->opt_track_blocks_per_cu;
      if (ctx->opt_track_workgroups > 0) limit = std::min<uint32_t>(limit, (uint32_t)ctx->opt_track_workgroups);
      launch_distort(distort_workgroups(n_tracks, limit), ctx->stream_t, DistortArgs{ctx->distort, ta.buf, n_tracks});
      HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipEventRecord(ts.t1, ctx->stream_t));
  }
  if (tl.use_status && tl.n) {  // events that hit event_sample_limit
    launch_count_status(ctx->stream_t, static_cast<const int32_t*>(ts.status.p), tl.n, static_cast<uint32_t*>(ts.ctrl.p) + TRK_AT_LIMIT);
    HIP_TRY(ctx, hipGetLastError());
  }
  HIP_TRY(ctx, hipMemcpyAsync(ts.h_ctrl.p, ts.ctrl.p, TRK_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream_t));
  HIP_TRY(ctx, hipEventRecord(ts.done, ctx->stream_t));
  return ATTPC_OK;
}

// Wait for the batch queued by launch_tracks; a batch whose arena was too small is run again with a
// larger one.  ms / n_limit accumulate.
int32_t finish_tracks(attpc_ctx* ctx, TrackSet& ts, const TrackLaunch& tl, TrackBuffers* out, double* ms_tracks,
                      uint64_t* n_limit, uint64_t* n_capped = nullptr) {
  const uint32_t n_tracks = tl.n * (uint32_t)tl.lay.n_sim;
  for (int attempt = 0; attempt < 8; ++attempt) {
    HIP_TRY(ctx, hipEventSynchronize(ts.done));
    if (n_tracks) {
      float ms_t = 0;
      HIP_TRY(ctx, hipEventElapsedTime(&ms_t, ts.t0, ts.t1));
      *ms_tracks += ms_t;  // timings of discarded attempts stay counted: they were spent
    }
    if (ts.h_ctrl[TRK_OVERFLOW] == 0) {  // no sample was refused
      if (n_tracks) ctx->blocks_per_track = (double)ts.h_ctrl[TRK_NEXT_BLOCK] / (double)n_tracks;
      if (n_limit) *n_limit += ts.h_ctrl[TRK_AT_LIMIT];
      if (n_capped) *n_capped += ts.h_ctrl[TRK_CAPPED];
      *out = track_buffers(ts);
      return ATTPC_OK;
    }
    // arena exhausted (the block counter kept counting): grow and run the batch again
    const size_t want = std::max<size_t>((size_t)ts.h_ctrl[TRK_NEXT_BLOCK] + (size_t)ts.h_ctrl[TRK_NEXT_BLOCK] / 8 + 1024, ts.arena_blocks * 2);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream_t));
    ts.arena_blocks = std::max(ts.arena_blocks, want);
    int32_t rc = launch_tracks(ctx, ts, tl);
    if (rc) return rc;
  }
  return fail(ctx, ATTPC_E_HIP, "track arena did not fit after repeated growth");
}

// events per track batch: up to MAX_SLOTS scatter chunks, bounded so that the sample arena stays below
// ARENA_BUDGET_BYTES (with the observed blocks per track once a batch has run)
uint64_t track_batch_events(const attpc_ctx* ctx, const attpc_event_layout& lay, uint64_t chunk) {
  const double per_track = ctx->blocks_per_track > 0.0 ? ctx->blocks_per_track * 1.15 + 0.25 : 3.0;
  const double bytes_per_event = (double)std::max(1, lay.n_sim) * per_track * ARENA_BLK * 4 * sizeof(double);
  const uint64_t by_memory = (uint64_t)((double)ARENA_BUDGET_BYTES / bytes_per_event);
  const uint64_t chunks = std::max<uint64_t>(1, std::min<uint64_t>(MAX_SLOTS, by_memory / std::max<uint64_t>(1, chunk)));
  return std::max<uint64_t>(1, std::min<uint64_t>(chunk * chunks, std::max<uint64_t>(by_memory, 1)));
}

// events of the next scatter chunk: a small pilot while the cloud size per event is unknown, then the
// configured chunk bounded by the cloud budget
uint32_t next_chunk_events(const attpc_ctx* ctx, uint64_t remaining) {
  uint64_t n = (uint64_t)std::max(1, ctx->chunk_events);
  if (ctx->rows_per_event <= 0.0) n = std::min<uint64_t>(n, 4096);
  else n = std::min<uint64_t>(n, std::max<uint64_t>(256, (uint64_t)((double)CLOUD_BUDGET_BYTES / (ctx->rows_per_event * 1.15 * 32.0 + 1.0))));
  return (uint32_t)std::min<uint64_t>(n, remaining);
}

// ------------------------------------------------------------------ scatter ----
struct ScatterPlan {  // launch geometry of one chunk
  bool use_small = false;
  bool use_wide = false;  // u64 sums per table slot (scatter_wide.hip), one workgroup per CU like the big build
  uint32_t wgs = 0, batch = 1, row_block = 1;
  int64_t need_rows = 0, need_segs = 0;  // the launch should fit in this much
  int64_t grow_rows = 0, grow_segs = 0;  // what to allocate when the buffers are smaller than that
};

ScatterPlan plan_scatter(const attpc_ctx* ctx, uint32_t n) {
  ScatterPlan p;
  // Kernel variant: "small" (two 512-thread workgroups with 6144-slot tables per CU) is ~6 % faster
  // for detectors with the usual diffusion; "big" (one 1024-thread workgroup, 12288 slots) holds twice
  // as many keys per time bucket.  Small is used when a sample is expected to touch at most 40 pads at
  // the far end of the drift (default detector: 28; the same estimate as key_estimate() in scatter.hip)
  // and no extension is on.  A time bucket that fits neither table goes through lone_bucket_kernel; a
  // context whose small launches meet many of those switches to big for good (prefer_big).
  const double spread = (6.0 / 4.9e-3) * (6.0 / 4.9e-3) * 2.0 * ctx->det.diffusion * ctx->det.dv / ctx->det.efield;
  const double far_keys = (1.0 + std::sqrt(spread * (ATTPC_NUM_TB - 1))) * (1.0 + std::sqrt(spread * (ATTPC_NUM_TB - 1)));
  p.use_small = far_keys <= 40.0 && !ctx->det.mc_diffusion && !(ctx->det.longitudinal_diffusion > 0.0) && !ctx->prefer_big;
  if (ctx->opt_variant == 1) p.use_small = true;
  if (ctx->opt_variant == 2) p.use_small = false;
  // u32 sums per slot hold what the AT-TPC makes (largest key of the headline workload: 1.1e9 electrons); a launch in
  // which many windows had to be given to lone_bucket_kernel (read_scatter) switches the context to the u64 build
  p.use_wide = ctx->opt_variant == 3 || (ctx->prefer_wide && ctx->opt_variant == 0);
  if (p.use_wide) p.use_small = false;
#ifndef ATTPC_SC_SMALL_WGS
#define ATTPC_SC_SMALL_WGS 2  // workgroups per CU of the small variant (scatter_small.hip)
#endif
  // persistent workgroups that take `batch` events per visit to the event counter and reserve output
  // rows `row_block` at a time (small launches: exact reservations, so that short runs waste no rows)
  p.wgs = std::min<uint32_t>((uint32_t)ctx->n_cus * (p.use_small ? (uint32_t)ATTPC_SC_SMALL_WGS : 1u), n);
  p.batch = n / p.wgs >= 64u ? 2u : 1u;  // the request for the next batch is hidden (scatter.hip)
  const double per_event = ctx->rows_per_event > 0.0 ? ctx->rows_per_event * 1.10 : 16384.0;
  const int64_t est_rows = (int64_t)((double)n * per_event) + 4096;
  p.row_block = est_rows / ((int64_t)p.wgs * 16) >= 16384 ? (uint32_t)std::min<int64_t>(est_rows / ((int64_t)p.wgs * 16), 1 << 18) : 1u;
  const int64_t hole_rows = p.row_block > 1u ? (int64_t)p.wgs * p.row_block + est_rows / 16 : 0;
  // keep the buffers while they cover the estimate with 3 % to spare, grow them by 25 % when they do not:
  // rows per event move by fractions of a percent from chunk to chunk, and re-allocating tens of GB for each
  // such step costs more than the kernels (a too small buffer is caught and the launch repeated)
  const double known = ctx->rows_per_event > 0.0 ? ctx->rows_per_event : 16384.0;
  p.need_rows = (int64_t)((double)n * known * 1.03) + hole_rows + 65536;
  p.grow_rows = (int64_t)((double)n * known * 1.25) + hole_rows + 65536;
  const double segs = ctx->segs_per_event > 0.0 ? ctx->segs_per_event : 5.0;
  p.need_segs = (int64_t)((double)n * (segs * 1.05 + 0.5)) + 4096 + (int64_t)p.wgs * 16;
  // (24 bytes a segment: when the list has to grow it is sized for a full chunk at once -- a call's chunks are not all
  //  of one length, and the next call's would re-allocate it inside a caller's timed region)
  p.grow_segs = (int64_t)((double)std::max<uint32_t>(n, (uint32_t)std::max(1, ctx->chunk_events)) * (segs * 1.5 + 1.0)) + 4096 + (int64_t)p.wgs * 16;
  if (ctx->opt_tiny && ctx->cloud_capacity == 0) {
    p.need_rows = p.grow_rows = 64;  // test hook: start with buffers that are certainly too small
    p.need_segs = p.grow_segs = 2;
  }
  return p;
}

// the device control words of slot `slot`, and the chunk its launch scattered as the kernels behind it read it
unsigned long long* slot_words(const attpc_ctx* ctx, int slot) {
  return static_cast<unsigned long long*>(ctx->out_ctrl.p) + (size_t)slot * CTRL_WORDS;
}
ChunkView chunk_view(const attpc_ctx* ctx, int slot) {
  return ChunkView{static_cast<const double*>(ctx->points.p), static_cast<const int64_t*>(ctx->labels.p),
                   static_cast<const Segment*>(ctx->segments.p), slot_words(ctx, slot), ctx->seg_capacity, ctx->cloud_capacity};
}

// Queue the scatter of the `n` events starting at event `e0` of a track batch (global id
// `first_event` = batch first + e0) on stream S, control words in slot `slot`.  `grow` may enlarge the
// cloud (the caller guarantees S is idle then).
int32_t enqueue_scatter(attpc_ctx* ctx, int slot, const attpc_event_layout& lay, const TrackBuffers& trk, uint64_t seed,
                        uint64_t first_event, uint32_t e0, uint32_t n, int64_t min_rows, int64_t min_segs) {
  int32_t rc;
  const ScatterPlan p = plan_scatter(ctx, n);
  int64_t want_rows = ctx->cloud_capacity, want_segs = ctx->seg_capacity;
  if (std::max(p.need_rows, min_rows) > ctx->cloud_capacity) want_rows = std::max(p.grow_rows, min_rows);
  if (std::max(p.need_segs, min_segs) > ctx->seg_capacity) want_segs = std::max(p.grow_segs, min_segs);
  // merge variant (scatter.hip): track samples far closer than a pad, i.e. the path-length dE/dx step; every
  // workgroup sorts its event's entries into two lists of its own in global memory
  const bool merge = !ctx->det.mc_diffusion && (ctx->opt_merge == 1 || (ctx->opt_merge < 0 && ctx->det.path_step > 0.0));
  const size_t merge_cap = (size_t)std::max(1, lay.n_sim) * MAX_BLOCKS_PER_TRACK * ARENA_BLK *
                           (ctx->det.longitudinal_diffusion > 0.0 ? ATTPC_LONG_STEPS : 1);
  const size_t merge_bytes = merge ? (size_t)p.wgs * 2 * merge_cap * sizeof(uint2) : 0;
  if (want_rows > ctx->cloud_capacity || want_segs > ctx->seg_capacity || (size_t)n * sizeof(uint32_t) > ctx->ev_rows.bytes ||
      merge_bytes > ctx->merge_scratch.bytes) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // nothing in flight may use the old buffers
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream_c));
    if ((rc = ensure(ctx, ctx->merge_scratch, merge_bytes))) return rc;
    if ((rc = ensure(ctx, ctx->points, (size_t)want_rows * 3 * sizeof(double)))) return rc;
    if ((rc = ensure(ctx, ctx->labels, (size_t)want_rows * sizeof(int64_t)))) return rc;
    if ((rc = ensure(ctx, ctx->segments, (size_t)want_segs * sizeof(Segment)))) return rc;
    if ((rc = ensure(ctx, ctx->ev_rows, (size_t)std::max<uint32_t>(n, (uint32_t)std::max(1, ctx->chunk_events)) * sizeof(uint32_t)))) return rc;
    ctx->cloud_capacity = want_rows;
    ctx->seg_capacity = want_segs;
    // test hook: poison the segment list, so that a consumer of slots a launch did not write (one that ran
    // out of capacity) cannot go unnoticed on freshly allocated, zero-filled memory
    if (ctx->opt_tiny) HIP_TRY(ctx, hipMemsetAsync(ctx->segments.p, 0x7f, ctx->segments.bytes, ctx->stream));
  }
  unsigned long long* d_ctrl = slot_words(ctx, slot);
  HIP_TRY(ctx, hipMemsetAsync(d_ctrl, 0, CTRL_WORDS * sizeof(unsigned long long), ctx->stream));
  ScatterArgs sa;
  sa.det = ctx->det;
  sa.layout = lay;
  sa.trk = trk;
  sa.out.points = static_cast<double*>(ctx->points.p);
  sa.out.labels = static_cast<int64_t*>(ctx->labels.p);
  sa.out.segments = static_cast<Segment*>(ctx->segments.p);
  sa.out.ctrl = d_ctrl;
  sa.out.ev_rows = static_cast<uint32_t*>(ctx->ev_rows.p);
  sa.out.lone_list = static_cast<LoneBucket*>(ctx->lone_list.p);
  sa.out.lone_capacity = LONE_CAPACITY;
  sa.out.lone_chg = static_cast<unsigned long long*>(ctx->lone_chg.p);
  sa.out.lone_mask = static_cast<uint32_t*>(ctx->lone_mask.p);
  // The launch may use what its plan asked for (or what a repeated launch was found to need), not the whole
  // buffer: whoever assembles its cloud sizes the event-ordered copy, the Spyral rows and the transfer records by
  // this number, and a device-resident run of large chunks may have left a buffer of many times that size.
  ctx->launch_row_cap = std::min<int64_t>(ctx->cloud_capacity, std::max<int64_t>(p.grow_rows, min_rows));
  sa.out.capacity = ctx->launch_row_cap;
  sa.out.seg_capacity = ctx->seg_capacity;
  sa.seed = seed;
  sa.first_event = first_event;
  sa.n_events = n;
  sa.event0 = e0;
  sa.batch = p.batch;
  sa.row_block = p.row_block;
  sa.merge_scratch = merge ? static_cast<uint2*>(ctx->merge_scratch.p) : nullptr;
  sa.merge_cap = (uint32_t)merge_cap;
  HIP_TRY(ctx, hipEventRecord(ctx->s0[slot], ctx->stream));
  ctx->slot_wide[slot] = p.use_wide;
  if (p.use_wide) launch_scatter_kernel_wide(p.wgs, ctx->stream, sa);
  else if (p.use_small) launch_scatter_kernel_small(p.wgs, ctx->stream, sa);
  else launch_scatter_kernel_big(p.wgs, ctx->stream, sa);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->s1[slot], ctx->stream));
  launch_lone_bucket_kernel((uint32_t)LONE_WORKGROUPS, ctx->stream, sa);  // exits at once without lone buckets
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_out_ctrl.p + (size_t)slot * CTRL_WORDS, d_ctrl, CTRL_WORDS * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost, ctx->stream));
#ifdef ATTPC_PHASE_TIMERS
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const unsigned long long* octrl = ctx->h_out_ctrl.p + (size_t)slot * CTRL_WORDS;
  const unsigned long long* ph = octrl + CTRL_PHASE;  // the CTRL_PHASE_WORDS phase words, numbered as PHASE_MARK / PHASE_COUNT do
  fprintf(stderr, "[attpc phase cycles] init %llu hist %llu select %llu stage %llu items %llu insert-calls %llu insert-trips %llu flushcount %llu flushwrite %llu (events %u)\n",
          ph[0], ph[1], ph[2], ph[3], ph[4], ph[5] >> 32, ph[5] & 0xffffffffull, ph[6], ph[7], n);
  fprintf(stderr, "[attpc rows-phase cycles] gathers %llu runs %llu scan+queue %llu drain %llu\n", ph[8], ph[9], ph[10], ph[11]);
  fprintf(stderr, "[attpc rounds] rows-rounds %llu staged %llu busiest-wave passes %llu\n", ph[12], ph[13], ph[14]);
  fprintf(stderr, "[attpc flush cycles] to-barrier %llu to-compacted %llu atomics-wait %llu segment %llu select %llu barrier %llu\n", ph[19], ph[15], ph[16], ph[17], ph[18], ph[6]);
  fprintf(stderr, "[attpc ctrl] rows %llu segments %llu failed %llu retried %llu samples %llu\n", octrl[CTRL_ROW_CURSOR], octrl[CTRL_SEG_CURSOR],
          octrl[CTRL_FAILED], octrl[CTRL_RETRIED], octrl[CTRL_SAMPLES]);
  fprintf(stderr, "[attpc per-wave wait at the window's last barrier]");
  for (int w = 0; w < CTRL_WAVE_WORDS; ++w) fprintf(stderr, " %llu", octrl[CTRL_WAVE_WAIT + w]);
  fprintf(stderr, "\n[attpc staging, even waves]");
  for (int w = 0; w < CTRL_STAGING_WORDS; ++w) fprintf(stderr, " %llu", octrl[CTRL_STAGING + w]);
  fprintf(stderr, "\n");
#endif
  return ATTPC_OK;
}

// Read the control words of slot `slot` (its copy has completed).  Updates the context's size
// estimates; r->overflow says the launch has to be repeated with at least min_rows / min_segs.
void read_scatter(attpc_ctx* ctx, int slot, uint32_t n, ChunkResult* r, int64_t* min_rows, int64_t* min_segs) {
  const unsigned long long* o = ctx->h_out_ctrl.p + (size_t)slot * CTRL_WORDS;
  float ms = 0;
  if (hipEventElapsedTime(&ms, ctx->s0[slot], ctx->s1[slot]) == hipSuccess) r->ms_scatter += ms;
  r->overflow = o[CTRL_OVERFLOW] != 0;
  r->reserved = o[CTRL_ROW_CURSOR];
  r->segs = o[CTRL_SEG_CURSOR];
  r->danger = o[CTRL_DANGER];
  // Windows whose u32 sums could have wrapped were done again by lone_bucket_kernel, one time bucket at a time: exact,
  // but meant for the odd window.  Where they are many (more than one per 64 events), or the list of lone buckets ran
  // over because of them, this detector needs u64 sums: the context switches to the wide build for good and this
  // launch is repeated with it (results do not depend on the build).
  if (!ctx->slot_wide[slot] && ctx->opt_variant == 0 && r->danger && (r->danger * 64ull > (unsigned long long)n || o[CTRL_FAILED] != 0)) {
    ctx->prefer_wide = true;
    r->overflow = true;
    *min_rows = std::max<int64_t>(*min_rows, ctx->launch_row_cap);
    *min_segs = std::max<int64_t>(*min_segs, ctx->seg_capacity);
    return;
  }
  if (r->overflow) {  // cloud / segment capacity exceeded (the cursors kept counting)
    *min_rows = (int64_t)(r->reserved + r->reserved / 8) + 65536;
    *min_segs = (int64_t)(r->segs + r->segs / 8) + 4096;
    return;
  }
  r->rows = o[CTRL_ROWS];  // rows written; r->reserved is the reservation cursor (holes included)
  r->charge = o[CTRL_CHARGE_SUM];
  r->keys = o[CTRL_KEY_SUM];
  r->failed = o[CTRL_FAILED];
  r->retried = o[CTRL_RETRIED];
  r->samples = o[CTRL_SAMPLES];
  r->mismatch = o[CTRL_MISMATCH];
  r->lone = std::min<unsigned long long>(o[CTRL_LONE], LONE_CAPACITY);
  if (n) {
    ctx->rows_per_event = std::max((double)r->rows / (double)n, 1.0e-3);  // > 0 = known
    ctx->segs_per_event = (double)r->segs / (double)n;
    if (r->lone * 100ull > (unsigned long long)n) ctx->prefer_big = true;  // > 1 % of the events: the small table is too small here
  }
}

void accumulate(attpc_run_stats* st, const ChunkResult& r) {
  st->n_points += r.rows;
  st->n_track_samples += r.samples;
  st->n_failed += r.failed;
  st->n_lds_overflow += r.retried;
  st->charge_checksum += r.charge;
  st->key_checksum += r.keys;
  st->ms_scatter += r.ms_scatter;
  st->launches_scatter += 1;
  st->n_inconsistent += (uint32_t)r.mismatch;
  st->n_lone_buckets += r.lone;
}

// ------------------------------------------------------------------ assembly (delivered clouds) ----
// What a run delivers: clouds (attpc_sim_run / attpc_det_run), Spyral rows (_spyral) or pad traces (_traces).
// trace_rows: the traces as in `traces`, kept on the device, and their peaks as Spyral rows (_trace_rows).
// summary: a device-resident run whose chunks are reduced to event and track records behind their scatter (_summary).
enum class OutMode { cloud, spyral, traces, trace_rows, summary };
// the modes whose chunks go through the trace kernels
bool makes_traces(OutMode mode) { return mode == OutMode::traces || mode == OutMode::trace_rows; }

// A run's output: the mode, the caller's output struct of that mode (neither: a device-resident run of clouds), and
// how far the delivery into it has come.
struct RunOut {
  OutMode mode = OutMode::cloud;
  attpc_cloud_out* cloud = nullptr;  // cloud, spyral, trace_rows
  attpc_trace_out* trace = nullptr;  // traces
  int64_t rows = 0;                  // row cursor: rows of the chunks delivered so far
  attpc_trace_packed_out* tpacked = nullptr;  // traces, packed: `trace` then holds its row arrays and no samples
  int64_t bytes = 0;                 // ... and their byte cursor: packed bytes of the chunks so far
  bool over = false;                 // ... more than the caller's capacity
  attpc_summary_out* summary = nullptr;  // summary (a resident run: neither cloud nor trace)
  attpc_select_out* select = nullptr;    // a selected run: cloud and summary are views of it (mode cloud or spyral)
  attpc_maps_out* maps = nullptr;        // a maps run: the summary run that also accumulates the run maps (maps.hip)
  uint8_t* maps_passed = nullptr;        // ... its caller's passed [n_events], or nullptr
  bool maps_selected = false;            // ... only the events that pass the configured selection contribute
  // the configured selection is evaluated on the records of every chunk (passed of the call in ctx->sel_host)
  bool predicate() const { return select || maps_selected; }
  bool resident() const { return !cloud && !trace; }
  int64_t* offsets() const { return cloud ? cloud->offsets : trace ? trace->offsets : nullptr; }
  int64_t* event_points() const { return cloud ? cloud->event_points : trace ? trace->event_points : nullptr; }
  int64_t capacity() const { return cloud ? cloud->capacity : trace->capacity; }
  // the capacity binds clouds always, traces when any of their row arrays is wanted
  // (trace rows: when their rows or labels are)
  bool bounded() const {
    if (select) return cloud->points && cloud->labels;  // (nothing of the rows is copied otherwise)
    if (mode == OutMode::trace_rows) return cloud->points || cloud->labels;
    if (tpacked && (tpacked->row_start || tpacked->bytes)) return true;
    return cloud || (trace && (trace->pads || trace->samples || trace->labels));
  }
};

// The event-ordered cloud of a chunk of `n` events and `cap` rows in `as`, and the pinned copies of its CSR offsets and
// rows per event (exact size).
int32_t ensure_asm_cloud(attpc_ctx* ctx, AsmSet& as, uint32_t n, size_t cap) {
  int32_t rc;
  if ((rc = ensure(ctx, as.ev_start, ((size_t)n + 1) * sizeof(int64_t)))) return rc;
  if ((rc = ensure(ctx, as.points, cap * 3 * sizeof(double)))) return rc;
  if ((rc = ensure(ctx, as.labels, cap * sizeof(int64_t)))) return rc;
  if ((rc = ensure_pinned(ctx, as.h_start, (size_t)n + 1))) return rc;
  return ensure_pinned(ctx, as.h_ev_rows, (size_t)n + 1);
}

TraceScratch trace_scratch(AsmSet& as, size_t cap) {
  TraceScratch sc;
  uint32_t* base = static_cast<uint32_t*>(as.tr_scratch.p);
  sc.row = base;
  sc.hit = base + cap;
  sc.hit_start = base + 2 * cap;
  sc.rank = reinterpret_cast<int32_t*>(base + 3 * cap);
  sc.info = static_cast<uint32_t*>(as.tr_info.p);
  return sc;
}

// The trace settings of the chunk in `as`: with the micromegas gain on, its charges come from as.tr_gained
// (enqueue_trace_count fills it in front of the count pass; the write pass reads the same array).
TraceDev trace_dev(const attpc_ctx* ctx, const AsmSet& as) {
  TraceDev tr = ctx->trace;
  tr.gained = ctx->gain_on ? static_cast<const double*>(as.tr_gained.p) : nullptr;
  return tr;
}

// The noise of the trace kernels: nullptr = the noiseless kernels.
const TraceNoiseDev* trace_noise(const attpc_ctx* ctx) { return ctx->noise_on ? &ctx->noise : nullptr; }

// The largest level of a noise table (0 without one: the one level 0).
int32_t top_level(const TraceNoiseDev& t) { return t.n_levels > 0 ? t.min_level + t.n_levels - 1 : 0; }

// The common-mode noise of the trace kernels for the chunk in `as` (its values in as.tr_common, which
// enqueue_trace_count fills in front of the count pass): nullptr = the kernels without the term.
const CommonDev* trace_common(const attpc_ctx* ctx, const AsmSet& as, CommonDev& cm) {
  if (!ctx->common_on) return nullptr;
  cm = CommonDev{static_cast<const int16_t*>(as.tr_common.p), ctx->common_groups, ctx->common_n_groups,
                 top_level(ctx->noise) + top_level(ctx->common_table)};
  return &cm;
}
// Events of a chunk whose common-mode values fill 1 GiB (at least one).
uint32_t common_chunk_events(const attpc_ctx* ctx) {
  return (uint32_t)std::max<int64_t>(1, (1ll << 20) / std::max(ctx->common_n_groups, 1));
}

// The readout of the trace kernels (ro.channels == nullptr: hit mode) with the cutoff of the decision rule for the
// configured threshold and noise table: c = floor(thr) + 1 - min_level; c <= 0 always, c > n_levels - 1 never (no
// table: the one level 0), else u_j >= cdf[c - 1].
TraceReadoutDev trace_readout(const attpc_ctx* ctx) {
  TraceReadoutDev ro{};
  if (ctx->readout_mode == ATTPC_READOUT_HIT) return ro;
  ro.channels = ctx->readout_channels;
  ro.full = ctx->readout_mode == ATTPC_READOUT_FULL ? 1 : 0;
  const bool table = ctx->noise_on && ctx->noise.n_levels > 0;
  const int64_t n_levels = table ? ctx->noise.n_levels : 1, min_level = table ? ctx->noise.min_level : 0;
  const double thr = std::min(std::max(ctx->trace.threshold, -16384.0), 16384.0);  // levels lie in -4095 .. 4606
  const int64_t c = (int64_t)std::floor(thr) + 1 - min_level;
  if (c <= 0) ro.cut_kind = TRACE_CUT_ALWAYS;
  else if (c > n_levels - 1) ro.cut_kind = TRACE_CUT_NEVER;
  else {
    ro.cut_kind = TRACE_CUT_DRAW;
    ro.cut = ctx->noise_cdf[(size_t)(c - 1)];
  }
  return ro;
}

// Does a readout run need the scan and the noise-only write?  Not in hit mode, nor in PARTIAL when the decision rule
// keeps no noise-only pad: thr >= 0 and a cutoff above the pad table -- and, with the common-mode noise on, the largest
// pad level plus the largest common-mode level <= thr.  The count pass's ranks are then the union's.
bool readout_scan(const attpc_ctx* ctx, const TraceReadoutDev& ro) {
  if (!ro.channels) return false;
  if (ro.full || !(ro.cut_kind == TRACE_CUT_NEVER && ctx->trace.threshold >= 0.0)) return true;
  return ctx->common_on && (double)(top_level(ctx->noise) + top_level(ctx->common_table)) > ctx->trace.threshold;
}

TraceMaps trace_maps(AsmSet& as, uint32_t n) {
  uint32_t* base = static_cast<uint32_t*>(as.tr_maps.p);
  const size_t words = (size_t)n * TR_MAP_WORDS;
  return TraceMaps{base, base + words, base + 2 * words};
}

// Trace count pass of the n events whose event-ordered cloud is in `as` (ev_start / points / labels, `cap` rows at
// most; global ids first_event .. first_event + n - 1), the scan of the kept rows and the copy of their CSR offsets to
// as.h_start, on S.
int32_t enqueue_trace_count(attpc_ctx* ctx, AsmSet& as, uint32_t n, size_t cap, uint64_t seed, uint64_t first_event) {
  int32_t rc;
  if ((rc = ensure(ctx, as.kept, std::max<size_t>(n, 1) * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, as.kept_start, ((size_t)n + 1) * sizeof(int64_t)))) return rc;
  if ((rc = ensure(ctx, as.tr_scratch, std::max<size_t>(cap, 1) * 4 * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, as.tr_info, std::max<size_t>(n, 1) * 2 * sizeof(uint32_t)))) return rc;
  if (ctx->gain_on && (rc = ensure(ctx, as.tr_gained, std::max<size_t>(cap, 1) * sizeof(double)))) return rc;
  if (ctx->common_on && n &&
      (rc = ensure(ctx, as.tr_common, (size_t)n * (size_t)ctx->common_n_groups * ATTPC_NUM_TB * sizeof(int16_t))))
    return rc;
  const TraceReadoutDev ro = trace_readout(ctx);
  CommonDev cm_store{};
  const CommonDev* cm = trace_common(ctx, as, cm_store);
  if (n) {
    if (cm) {  // the common-mode values of the chunk's events and groups, in front of the count pass
      launch_common_mode(ctx->stream, ctx->common_table, seed, n, first_event, (uint32_t)ctx->common_n_groups,
                         static_cast<int16_t*>(as.tr_common.p));
      HIP_TRY(ctx, hipGetLastError());
    }
    if (ctx->gain_on) {  // the gained charges of the chunk's rows, in front of the count pass
      launch_gain(ctx->stream, ctx->gain, seed, n, first_event, static_cast<const int64_t*>(as.ev_start.p),
                  static_cast<const double*>(as.points.p), static_cast<double*>(as.tr_gained.p));
      HIP_TRY(ctx, hipGetLastError());
    }
    const TraceScratch sc = trace_scratch(as, as.tr_scratch.bytes / (4 * sizeof(uint32_t)));
    launch_trace_count(ctx->stream, trace_dev(ctx, as), trace_noise(ctx), seed, n, first_event, static_cast<const int64_t*>(as.ev_start.p),
                       static_cast<const double*>(as.points.p), static_cast<const int64_t*>(as.labels.p), sc,
                       static_cast<uint32_t*>(as.kept.p), ro.channels ? &ro : nullptr, cm);
    HIP_TRY(ctx, hipGetLastError());
    if (readout_scan(ctx, ro)) {
      if ((rc = ensure(ctx, as.tr_maps, (size_t)n * 3 * TR_MAP_WORDS * sizeof(uint32_t)))) return rc;
      launch_trace_scan(ctx->stream, ctx->trace, trace_noise(ctx), ro, seed, n, first_event,
                        static_cast<const int64_t*>(as.ev_start.p), sc, static_cast<uint32_t*>(as.kept.p), trace_maps(as, n), cm);
      HIP_TRY(ctx, hipGetLastError());
    }
  }
  launch_exclusive_scan(ctx->stream, static_cast<const uint32_t*>(as.kept.p), n, static_cast<int64_t*>(as.kept_start.p), nullptr);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(as.h_start.p, as.kept_start.p, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  return ATTPC_OK;
}

// The counted chunk in `as` has `total` kept rows (as.h_start[n], read by the host): size the trace outputs, queue the
// write pass on S (checksums into ctx->trace_sums) and record as.traced behind it.
int32_t enqueue_trace_write(attpc_ctx* ctx, AsmSet& as, uint32_t n, int64_t total, uint64_t seed, uint64_t first_event) {
  int32_t rc;
  if (total > 0) {
    CommonDev cm_store{};
    const CommonDev* cm = trace_common(ctx, as, cm_store);
    if ((size_t)total > as.tr_cap) as.tr_cap = (size_t)total + (size_t)total / 8;
    if ((rc = ensure(ctx, as.tr_pads, as.tr_cap * sizeof(int32_t)))) return rc;
    if ((rc = ensure(ctx, as.tr_samples, as.tr_cap * ATTPC_NUM_TB * sizeof(int16_t)))) return rc;
    if ((rc = ensure(ctx, as.tr_labels, as.tr_cap * sizeof(int64_t)))) return rc;
    launch_trace_write(ctx->stream, trace_dev(ctx, as), trace_noise(ctx), seed, n, first_event, static_cast<const int64_t*>(as.ev_start.p),
                       static_cast<const double*>(as.points.p), static_cast<const int64_t*>(as.labels.p),
                       trace_scratch(as, as.tr_scratch.bytes / (4 * sizeof(uint32_t))),
                       static_cast<const int64_t*>(as.kept_start.p), static_cast<int32_t*>(as.tr_pads.p),
                       static_cast<int16_t*>(as.tr_samples.p), static_cast<int64_t*>(as.tr_labels.p),
                       static_cast<unsigned long long*>(ctx->trace_sums.p), cm);
    HIP_TRY(ctx, hipGetLastError());
    if (readout_scan(ctx, trace_readout(ctx))) {  // the noise-only rows between them
      launch_trace_noise_write(ctx->stream, trace_noise(ctx), seed, n, first_event, trace_maps(as, n),
                               static_cast<const int64_t*>(as.kept_start.p), static_cast<int32_t*>(as.tr_pads.p),
                               static_cast<int16_t*>(as.tr_samples.p), static_cast<int64_t*>(as.tr_labels.p),
                               static_cast<unsigned long long*>(ctx->trace_sums.p), cm);
      HIP_TRY(ctx, hipGetLastError());
    }
  }
  HIP_TRY(ctx, hipEventRecord(as.traced, ctx->stream));
  return ATTPC_OK;
}

// The start of a trace or trace-row call of `n` events: room for its trigger records (attpc_trigger_last), if a trigger
// is configured.  Nothing of an earlier call is in flight.
int32_t begin_trigger_call(attpc_ctx* ctx, uint64_t n) {
  ctx->tg_records.off();
  return ctx->trigger_on ? begin_records(ctx, ctx->tg_records, n, 1) : ATTPC_OK;
}

// The positions of `lay` as the estimate kernel takes them: the label of every position, -1 for a later position of a
// label given twice (and for an index that is no label).
void estimate_positions(const attpc_event_layout& lay, int64_t slot_label[ATTPC_MAX_SIM]) {
  for (int s = 0; s < ATTPC_MAX_SIM; ++s) {
    slot_label[s] = s < lay.n_sim && lay.indices[s] >= 0 ? (int64_t)lay.indices[s] : -1;
    for (int t = 0; t < s && t < lay.n_sim; ++t)
      if (lay.indices[t] == lay.indices[s]) slot_label[s] = -1;
  }
}

// The kernel's settings from a checked desc.
void estimate_settings(const attpc_estimate_desc& d, EstimateArgs* a) {
  const int64_t rb = estimate_beam_units(d.beam_region_radius);
  a->rb2 = rb * rb;
  a->min_points = d.min_points;
  a->magnetic_field = d.magnetic_field;
}

// The refining kernel's settings from a checked desc.
void circle_settings(const attpc_circle_desc& d, EstimateArgs* a) {
  a->circle_tolerance = d.tolerance;
  a->circle_max_evaluations = d.max_evaluations;
}

// The nuclei of the layout's positions for the track fit, from the configured detector.
void fit_positions(const DetDev& det, const attpc_event_layout& lay, FitPosition position[ATTPC_MAX_SIM]) {
  for (int s = 0; s < ATTPC_MAX_SIM; ++s) {
    FitPosition& p = position[s];
    p = FitPosition{0.0, 0.0, 0.0, 0.0, 0.0, -1, 0};
    if (s >= lay.n_sim || lay.indices[s] < 0 || lay.indices[s] >= lay.n_rows) continue;
    const int sp = lay.species_of_row[lay.indices[s]];
    if (sp < 0 || sp >= det.n_species || det.Z[sp] <= 0 || !(det.mass[sp] > 0.0)) continue;
    const FitSpecies f = fit_species(det.mass[sp], det.Z[sp], det.bfield, det.efield, det.density);
    p = FitPosition{f.mass, f.charge, f.qm_b, f.qm_e, f.drag, sp, 0};
  }
}

// The track fit of `n` events behind their estimates on S: the arguments the estimates had, their records, and room
// for the trials.
// With `hyp` (n >= 1) the launch is the instantiation over (track, hypothesis) pairs: records is [n][n_sim][hyp->n], pid
// may be nullptr.
int32_t enqueue_fit(attpc_ctx* ctx, const EstimateArgs& e, uint32_t n, const attpc_fit_desc& d, const FitPosition* position,
                    const double* start, const attpc_pid_record* pid, attpc_track_fit* records, const HypLayout* hyp = nullptr) {
  const uint32_t workgroups = fit_workgroups(n, e.n_sim, hyp ? hyp->n : 1);
  const int32_t rc = ensure(ctx, ctx->fit_scratch, (size_t)workgroups * FIT_SCRATCH_PER_WORKGROUP);
  if (rc) return rc;
  FitArgs a{};
  a.ev_start = e.ev_start;
  a.rows = e.rows;
  a.labels = e.labels;
  a.points = e.points;
  a.thin_info = e.thin_info;
  a.estimates = e.records;
  a.start = start;
  a.records = records;
  a.scratch = static_cast<double*>(ctx->fit_scratch.p);
  a.dedx = ctx->det.dedx;
  std::memcpy(a.slot_label, e.slot_label, sizeof a.slot_label);
  std::memcpy(a.position, position, sizeof a.position);
  a.d = d;
  a.length = ctx->det.length;
  a.rb2 = e.rb2;
  a.n_events = n;
  a.n_sim = e.n_sim;
  if (hyp) launch_fit_hypotheses(ctx->stream, a, *hyp, pid);
  else launch_fit(ctx->stream, a, pid);
  HIP_TRY(ctx, hipGetLastError());
  return ATTPC_OK;
}

// The selection of the fit hypotheses of `n` > 0 events behind their fits (enqueue_fit with `hyp`) on S.
int32_t enqueue_hypothesis_select(attpc_ctx* ctx, const HypLayout& hyp, uint32_t n, int32_t n_sim, const attpc_track_fit* all,
                                  const attpc_pid_record* pid, const attpc_track_estimate* estimates,
                                  attpc_fit_hypothesis* records, attpc_track_fit* fits, attpc_pid_record* assigned) {
  HypothesisArgs a{};
  a.l = hyp;
  a.all = all;
  a.pid = pid;
  a.estimates = estimates;
  a.records = records;
  a.fits = fits;
  a.assigned = assigned;
  a.n_events = n;
  a.n_sim = n_sim;
  launch_hypothesis_select(ctx->stream, a);
  HIP_TRY(ctx, hipGetLastError());
  return ATTPC_OK;
}

// The gates of a checked desc on the device, in `buf`.
int32_t upload_pid_gates(attpc_ctx* ctx, DevBuf& buf, const attpc_pid_desc& d) {
  PidGates g{};
  std::memcpy(g.vertices, d.vertices, sizeof g.vertices);
  std::memcpy(g.n_vertices, d.n_vertices, sizeof g.n_vertices);
  const int32_t rc = ensure(ctx, buf, sizeof g);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpy(buf.p, &g, sizeof g, hipMemcpyHostToDevice));
  return ATTPC_OK;
}

// The particle identification of `n` > 0 events of n_sim > 0 positions on S: their estimate records against the gates
// in `gates` (upload_pid_gates).
int32_t enqueue_pid(attpc_ctx* ctx, const attpc_track_estimate* estimates, uint32_t n, int32_t n_sim, const DevBuf& gates,
                    int32_t mode, const int32_t* species, attpc_pid_record* records) {
  PidArgs a{};
  a.estimates = estimates;
  a.gates = static_cast<const PidGates*>(gates.p);
  a.records = records;
  for (int s = 0; s < ATTPC_MAX_SIM; ++s) a.species[s] = species ? species[s] : -1;
  a.n_events = n;
  a.n_sim = n_sim;
  a.mode = mode;
  launch_pid(ctx->stream, a);
  HIP_TRY(ctx, hipGetLastError());
  return ATTPC_OK;
}

// The table of a checked desc on the device, in `buf` (nothing without a target).
int32_t upload_reaction_eloss(attpc_ctx* ctx, DevBuf& buf, const attpc_reaction_desc& d) {
  if (!d.has_target) return ATTPC_OK;
  const int32_t rc = ensure(ctx, buf, (size_t)d.eloss_len * sizeof(double));
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpy(buf.p, d.eloss, (size_t)d.eloss_len * sizeof(double), hipMemcpyHostToDevice));
  return ATTPC_OK;
}

// The reaction reconstruction of `n` > 0 events on S: the source records and the truth of `a` (everything but the
// settings filled in by the caller) with the settings `d`, whose table is in `eloss` (upload_reaction_eloss).
int32_t enqueue_reaction(attpc_ctx* ctx, ReactionArgs a, const attpc_reaction_desc& d, const DevBuf& eloss) {
  a.c = reaction_params(d);
  a.eloss = d.has_target ? static_cast<const double*>(eloss.p) : nullptr;
  if (d.source == ATTPC_REACTION_FROM_FIT) a.estimates = nullptr; else a.fits = nullptr;
  launch_reaction(ctx->stream, a);
  HIP_TRY(ctx, hipGetLastError());
  return ATTPC_OK;
}

// The streams of a trace-row call turned off: none answers for any call.
void trace_row_records_off(attpc_ctx* ctx) {
  auto off = [](auto&... r) { (r.off(), ...); };
  off(ctx->est_records, ctx->fit_records, ctx->pid_records, ctx->hyp_records, ctx->hyp_fits, ctx->rx_records, ctx->cl_events, ctx->cl_records, ctx->jn_events, ctx->jn_records);
}

// The start of a trace-row call of `n` events with the layout `lay` (nullptr: the call has none, makes no records and
// is not clustered) that fetches `row_capacity` rows (-1: none): every stream of an earlier call off and a fresh call
// state, then what the call cannot do refused, then the streams of the stages that are on -- with their pinned room --
// and what these stages read of the layout.  Nothing of an earlier call is in flight.
int32_t begin_trace_row_call(attpc_ctx* ctx, uint64_t n, const attpc_event_layout* lay, int64_t row_capacity) {
  trace_row_records_off(ctx);
  TraceRowCall& call = ctx->call = TraceRowCall{};
  if (!lay) return ATTPC_OK;
  call.n_sim = lay->n_sim;
  // (the fit, the identification and the reconstruction do nothing without the estimates, the reconstruction nothing
  //  without its source; what it cannot read is refused before the call has any stream)
  const bool reaction = ctx->estimates_on && ctx->reaction_on && (ctx->reaction.source == ATTPC_REACTION_FROM_ESTIMATE || ctx->fit_on);
  if (reaction && (ctx->reaction.track >= lay->n_sim || lay->n_rows < 4))
    return fail(ctx, ATTPC_E_INVALID, "reaction: track %d and rows 0 .. 3 need a layout of more than %d positions and %d rows",
                ctx->reaction.track, lay->n_sim, lay->n_rows);
  if (reaction && lay->indices[ctx->reaction.track] != ctx->reaction.observed_row)
    return fail(ctx, ATTPC_E_INVALID, "reaction: position %d of the layout is row %d, observed_row is %d", ctx->reaction.track,
                lay->indices[ctx->reaction.track], ctx->reaction.observed_row);
  // a spectra-only call (option reaction_spectra_only) keeps every record on the device: no pinned room, no copy
  const bool to_host = !(reaction && ctx->opt_spectra_only);
  const size_t n_sim = (size_t)lay->n_sim;
  int32_t rc;
  if (ctx->estimates_on) {
    if ((rc = begin_records(ctx, ctx->est_records, n, n_sim, to_host))) return rc;
    estimate_positions(*lay, call.est_slot_label);
    if (ctx->fit_on || ctx->pid_on) {
      fit_positions(ctx->det, *lay, call.fit_position);
      for (int s = 0; s < ATTPC_MAX_SIM; ++s) call.pid_species[s] = call.fit_position[s].table;
    }
    if (ctx->fit_on && (rc = begin_records(ctx, ctx->fit_records, n, n_sim, to_host))) return rc;
    if (ctx->pid_on && (rc = begin_records(ctx, ctx->pid_records, n, n_sim, to_host))) return rc;
    if (ctx->fit_on && ctx->hyp_on) {
      call.hyp = hypothesis_layout(call.pid_species, lay->n_sim, ctx->hyp.candidates);
      if ((rc = begin_records(ctx, ctx->hyp_records, n, n_sim, to_host))) return rc;
      if ((rc = begin_records(ctx, ctx->hyp_fits, n, n_sim * (size_t)call.hyp.n, to_host))) return rc;
    }
  }
  if (reaction) {
    if ((rc = begin_records(ctx, ctx->rx_records, n, 1, to_host))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->rx_cells.p, 0, ctx->rx_cells.bytes, ctx->stream));
    call.rx_n_rows = lay->n_rows;
  }
  if (!ctx->cluster_on) return ATTPC_OK;  // (the joining does nothing without the clustering)
  if ((rc = begin_records(ctx, ctx->cl_events, n, 1, to_host))) return rc;
  if ((rc = begin_records(ctx, ctx->cl_records, n, ATTPC_MAX_SIM, to_host))) return rc;
  call.cluster = cluster_settings(ctx->cluster, *lay);
  if (ctx->join_on) {
    if ((rc = begin_records(ctx, ctx->jn_events, n, 1, to_host))) return rc;
    if ((rc = begin_records(ctx, ctx->jn_records, n, ATTPC_MAX_SIM, to_host))) return rc;
    call.join = join_settings(ctx->join);
  }
  if (row_capacity >= 0) {
    if ((rc = ensure_pinned(ctx, ctx->h_cl_labels, std::max<size_t>((size_t)row_capacity, 1)))) return rc;
    call.cluster_rows = 0;
  }
  return ATTPC_OK;
}

// The start of a trace (`rows` false) or trace-row call: begin_trace_row_call and begin_trigger_call.  A call that
// either refuses leaves every stream it would have reset turned off.
int32_t begin_record_streams(attpc_ctx* ctx, bool rows, uint64_t n, const attpc_event_layout* lay, int64_t row_capacity) {
  int32_t rc = rows ? begin_trace_row_call(ctx, n, lay, row_capacity) : ATTPC_OK;
  if (!rc) rc = begin_trigger_call(ctx, n);
  if (rc) ctx->tg_records.off();
  if (rc && rows) trace_row_records_off(ctx);
  return rc;
}

// What the reconstruction stages and the delivery read of the chunk in `as`: the starts of its events and its rows and
// truth labels, the corrected ones with the drift correction on (rows and labels nullptr: no event of it has a row).
ChunkRows chunk_rows(const attpc_ctx* ctx, const AsmSet& as) {
  const bool corrected = ctx->correction_on;
  return {static_cast<const int64_t*>(as.pk_ev_start.p), static_cast<const double*>(corrected ? as.uc_rows.p : as.sp_rows.p),
          static_cast<const int64_t*>(corrected ? as.uc_labels.p : as.sp_labels.p)};
}

// The estimate kernel of n events of `a`: of raw rows or of `thinned` points, with the geometric `circle` fit, with the
// `helix` slope.
void launch_estimate_kernel(hipStream_t stream, uint32_t n, const EstimateArgs& a, bool thinned, bool circle, bool helix) {
  if (helix)
    launch_helix_estimates(stream, n, a, thinned, circle);
  else if (circle)
    launch_circle_estimates(stream, n, a, thinned);
  else if (thinned)
    launch_point_estimates(stream, n, a);
  else
    launch_estimates(stream, n, a);
}

// The track estimates of the chunk in `as` (n events, rows written: directly behind launch_peak_rows) on S, as.traced
// recorded again behind them, and the copy of the records to events first_local .. of the call's pinned array on C.
// With thinning on the rows are thinned first (thin.hip) and the estimates are those of the points; with the geometric
// circle fit on the estimate kernel is its refining instantiation, with the helix slope on the one with its third pass.
int32_t enqueue_estimates(attpc_ctx* ctx, AsmSet& as, uint32_t n, uint64_t first_local) {
  const TraceRowCall& call = ctx->call;
  const size_t n_sim = (size_t)call.n_sim;
  if (!n || !n_sim) return ATTPC_OK;
  int32_t rc = ATTPC_OK;
  EstimateArgs a{};
  a.records = chunk_room(ctx, ctx->est_records, as.est_records, n, rc);
  if (rc) return rc;
  if (ctx->thinning_on) {  // (a point per trace row is room enough: pk_cap is what sp_rows holds)
    if ((rc = ensure(ctx, as.thin_points, std::max<size_t>(as.pk_cap, 1) * sizeof(ThinPoint)))) return rc;
    if ((rc = ensure(ctx, as.thin_info, (size_t)n * n_sim * sizeof(attpc_thin_info)))) return rc;
  }
  estimate_settings(ctx->estimates, &a);
  chunk_rows(ctx, as).into(a);
  if (ctx->cl_events.made()) a.labels = static_cast<const int64_t*>(as.cl_labels.p);  // (clustering on: its labels)
  std::memcpy(a.slot_label, call.est_slot_label, sizeof a.slot_label);
  a.n_sim = (int32_t)n_sim;
  if (ctx->thinning_on) {
    ThinArgs t{};
    t.ev_start = a.ev_start;
    t.rows = a.rows;
    t.labels = a.labels;
    t.points = static_cast<ThinPoint*>(as.thin_points.p);
    t.info = static_cast<attpc_thin_info*>(as.thin_info.p);
    std::memcpy(t.slot_label, a.slot_label, sizeof t.slot_label);
    t.n_sim = a.n_sim;
    t.step = thin_step_units(ctx->thinning.z_step);
    launch_thin(ctx->stream, n, t);
    HIP_TRY(ctx, hipGetLastError());
    a.points = t.points;
    a.thin_info = t.info;
  }
  if (ctx->circle_on) circle_settings(ctx->circle, &a);
  if (ctx->helix_on) a.helix_regressor = ctx->helix.regressor;
  launch_estimate_kernel(ctx->stream, n, a, ctx->thinning_on, ctx->circle_on, ctx->helix_on);
  HIP_TRY(ctx, hipGetLastError());
  const attpc_pid_record* pid = nullptr;
  if (ctx->pid_records.made()) {
    attpc_pid_record* records = chunk_room(ctx, ctx->pid_records, as.pid_records, n, rc);
    if (rc || (rc = enqueue_pid(ctx, a.records, n, a.n_sim, ctx->pid_gates, ctx->pid.mode, call.pid_species, records))) return rc;
    pid = records;
  }
  if (ctx->fit_records.made()) {
    attpc_track_fit* records = chunk_room(ctx, ctx->fit_records, as.fit_records, n, rc);
    if (ctx->hyp_records.made()) {  // fit hypotheses: in the place of the plain or pid fit launch, never beside it
      const bool any = call.hyp.n > 0;  // (no position of the layout has a species: nothing to integrate, nothing is read)
      attpc_track_fit* all = any ? chunk_room(ctx, ctx->hyp_fits, as.hyp_fits, n, rc) : nullptr;
      attpc_fit_hypothesis* chosen = chunk_room(ctx, ctx->hyp_records, as.hyp_records, n, rc);
      if (!rc && ctx->rx_records.made()) rc = ensure(ctx, as.hyp_assigned, (size_t)n * n_sim * sizeof(attpc_pid_record));
      attpc_pid_record* assigned = ctx->rx_records.made() ? static_cast<attpc_pid_record*>(as.hyp_assigned.p) : nullptr;
      if (rc || (any && (rc = enqueue_fit(ctx, a, n, ctx->fit, call.fit_position, nullptr, pid, all, &call.hyp)))) return rc;
      if ((rc = enqueue_hypothesis_select(ctx, call.hyp, n, a.n_sim, all, pid, a.records, chosen, records, assigned))) return rc;
      if (assigned) pid = assigned;  // (what the reaction reconstruction's slot rule reads)
    } else if (rc || (rc = enqueue_fit(ctx, a, n, ctx->fit, call.fit_position, nullptr, pid, records))) return rc;
  }
  if (ctx->rx_records.made()) {  // behind the last of the estimate, pid, fit and hypothesis kernels
    const size_t b = (size_t)(first_local - call.rx_batch_first);  // the chunk's first event in its track batch
    ReactionArgs r{};
    r.fits = static_cast<const attpc_track_fit*>(as.fit_records.p);
    r.estimates = a.records;
    r.pid = pid;
    r.p4 = call.rx_p4 + b * (size_t)call.rx_n_rows * 4;
    r.vertex = call.rx_vertex + b * 3;
    r.kin_status = call.rx_status ? call.rx_status + b : nullptr;
    r.records = chunk_room(ctx, ctx->rx_records, as.rx_records, n, rc);
    r.cells = static_cast<unsigned long long*>(ctx->rx_cells.p);
    r.n_events = n;
    r.n_sim = a.n_sim;
    r.n_rows = call.rx_n_rows;
    if (rc || (rc = enqueue_reaction(ctx, r, ctx->reaction, ctx->rx_eloss))) return rc;
  }
  HIP_TRY(ctx, hipEventRecord(as.traced, ctx->stream));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream_c, as.traced, 0));
  if ((rc = copy_chunk(ctx, ctx->rx_records, as.rx_records, first_local, n))) return rc;
  if ((rc = copy_chunk(ctx, ctx->fit_records, as.fit_records, first_local, n))) return rc;
  if ((rc = copy_chunk(ctx, ctx->pid_records, as.pid_records, first_local, n))) return rc;
  if ((rc = copy_chunk(ctx, ctx->hyp_records, as.hyp_records, first_local, n))) return rc;
  if ((rc = copy_chunk(ctx, ctx->hyp_fits, as.hyp_fits, first_local, n))) return rc;
  return copy_chunk(ctx, ctx->est_records, as.est_records, first_local, n);
}

// The drift correction of the chunk in `as` (n events, rows written: directly behind launch_peak_rows, which is done
// with the sort scratch on the same stream) on S: as.sp_rows / as.sp_labels -> as.uc_rows / as.uc_labels, the rows and
// labels every later stage and the delivery read.  The counts go to ctx->uc_sums; a chunk is delivered once, so every
// event counts once.
int32_t enqueue_correction(attpc_ctx* ctx, AsmSet& as, uint32_t n) {
  int32_t rc;
  if ((rc = ensure(ctx, as.uc_rows, as.pk_cap * 8 * sizeof(double)))) return rc;
  if ((rc = ensure(ctx, as.uc_labels, as.pk_cap * sizeof(int64_t)))) return rc;
  if ((rc = ensure(ctx, ctx->uc_xyt, as.pk_cap * 3 * sizeof(double)))) return rc;
  UndistortArgs a{};
  a.s = ctx->correction;
  a.ev_start = static_cast<const int64_t*>(as.pk_ev_start.p);
  a.rows = static_cast<const double*>(as.sp_rows.p);
  a.labels = static_cast<const int64_t*>(as.sp_labels.p);
  a.xyt = static_cast<double*>(ctx->uc_xyt.p);
  a.sort_idx = static_cast<uint32_t*>(ctx->sort_idx.p);
  a.sort_key = static_cast<double*>(ctx->sort_key.p);
  a.out_rows = static_cast<double*>(as.uc_rows.p);
  a.out_labels = static_cast<int64_t*>(as.uc_labels.p);
  a.counts = static_cast<unsigned long long*>(ctx->uc_sums.p);
  launch_undistort(ctx->stream, n, a);
  HIP_TRY(ctx, hipGetLastError());
  return ATTPC_OK;
}

// The clustering of the chunk in `as` (n events; rows written, and corrected if the drift correction is on) on S: the
// rows and truth labels every later stage would read -> as.cl_labels, the labels the thinning, the estimates and the
// fit read instead, and the chunk's records.
int32_t enqueue_clustering(attpc_ctx* ctx, AsmSet& as, uint32_t n) {
  if (!n) return ATTPC_OK;
  const size_t cap = std::max<size_t>(as.pk_cap, 1);
  int32_t rc;
  if ((rc = ensure(ctx, as.cl_labels, cap * sizeof(int64_t)))) return rc;
  ClusterArgs a{};
  a.events = chunk_room(ctx, ctx->cl_events, as.cl_events, n, rc);
  a.records = chunk_room(ctx, ctx->cl_records, as.cl_records, n, rc);
  if (rc || (rc = ensure(ctx, ctx->cl_scratch, cap * CLUSTER_SCRATCH_WORDS * sizeof(int32_t)))) return rc;
  a.s = ctx->call.cluster;
  chunk_rows(ctx, as).into(a);
  a.scratch = static_cast<int32_t*>(ctx->cl_scratch.p);
  a.out_labels = static_cast<int64_t*>(as.cl_labels.p);
  launch_cluster(ctx->stream, n, a);
  HIP_TRY(ctx, hipGetLastError());
  if (ctx->jn_events.made()) {  // right behind the clustering on S: it reads the scratch that kernel left
    ClusterJoinArgs j{};
    j.c = a;
    j.j = ctx->call.join;
    j.join_events = chunk_room(ctx, ctx->jn_events, as.jn_events, n, rc);
    j.join_records = chunk_room(ctx, ctx->jn_records, as.jn_records, n, rc);
    if (rc) return rc;
    launch_cluster_join(ctx->stream, n, j);
    HIP_TRY(ctx, hipGetLastError());
  }
  return ATTPC_OK;
}

// The trigger of the chunk in `as` (n events, `total` kept rows, written: directly behind enqueue_trace_write) on S --
// with `gate` the pass byte of every kept row too --, as.traced recorded again behind it, and the copy of the records
// to events first_local .. of the call's pinned array on C.
int32_t enqueue_trigger(attpc_ctx* ctx, AsmSet& as, uint32_t n, int64_t total, uint64_t first_local, bool gate) {
  if (!n) return ATTPC_OK;
  int32_t rc = ATTPC_OK;
  TriggerArgs a{};
  a.records = chunk_room(ctx, ctx->tg_records, as.tg_records, n, rc);
  if (rc) return rc;
  if (gate && (rc = ensure(ctx, as.tg_row_pass, std::max<size_t>(as.tr_cap, (size_t)std::max<int64_t>(total, 1))))) return rc;
  a.tg = ctx->trigger;
  a.pedestals = ctx->noise_on ? ctx->noise.pedestals : nullptr;
  a.kept_start = static_cast<const int64_t*>(as.kept_start.p);
  a.pads = static_cast<const int32_t*>(as.tr_pads.p);
  a.samples = static_cast<const int16_t*>(as.tr_samples.p);
  a.row_pass = gate ? static_cast<uint8_t*>(as.tg_row_pass.p) : nullptr;
  launch_trigger(ctx->stream, n, a);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(as.traced, ctx->stream));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream_c, as.traced, 0));
  return copy_chunk(ctx, ctx->tg_records, as.tg_records, first_local, n);
}

// Queue the copies of the written traces of `as` (rows base .. base + total of the caller's arrays; any array may be
// NULL) on C behind as.traced, then record as.copied.
int32_t copy_traces(attpc_ctx* ctx, AsmSet& as, int64_t total, int64_t base, const attpc_trace_out* out, bool fits) {
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream_c, as.traced, 0));
  if (total > 0 && fits) {
    if (out->pads)
      HIP_TRY(ctx, hipMemcpyAsync(out->pads + base, as.tr_pads.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream_c));
    if (out->samples)
      HIP_TRY(ctx, hipMemcpyAsync(out->samples + base * ATTPC_NUM_TB, as.tr_samples.p, (size_t)total * ATTPC_NUM_TB * sizeof(int16_t),
                                  hipMemcpyDeviceToHost, ctx->stream_c));
    if (out->labels)
      HIP_TRY(ctx, hipMemcpyAsync(out->labels + base, as.tr_labels.p, (size_t)total * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream_c));
  }
  HIP_TRY(ctx, hipEventRecord(as.copied, ctx->stream_c));
  return ATTPC_OK;
}

// Packed traces, first half: the size pass over `rows` (> 0) trace rows at `samples` on the device, the scan of the
// record sizes into as.tp_row_start (relative to the chunk) and the copy of their total to as.h_tp_total, on S;
// as.counted is recorded behind it.
int32_t enqueue_trace_pack_size(attpc_ctx* ctx, AsmSet& as, int64_t rows, const int16_t* samples) {
  int32_t rc;
  const size_t cap = std::max(as.tr_cap, (size_t)rows);
  const uint32_t blocks = peak_scan_blocks((uint32_t)rows);
  if ((rc = ensure(ctx, as.tp_headers, cap * sizeof(uint4)))) return rc;
  if ((rc = ensure(ctx, as.tp_sizes, cap * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, as.tp_row_start, (cap + 1) * sizeof(int64_t)))) return rc;
  if ((rc = ensure(ctx, as.tp_block_sums, (size_t)blocks * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, as.tp_block_start, ((size_t)blocks + 1) * sizeof(int64_t)))) return rc;
  if ((rc = ensure_pinned(ctx, as.h_tp_total, 1))) return rc;
  const uint32_t limit = ctx->opt_trace_pack_workgroups > 0 ? (uint32_t)ctx->opt_trace_pack_workgroups : (uint32_t)ctx->n_cus * 8u;
  launch_trace_pack_size(ctx->stream, trace_pack_workgroups((uint32_t)rows, limit), (uint32_t)rows, samples,
                         static_cast<uint4*>(as.tp_headers.p), static_cast<uint32_t*>(as.tp_sizes.p));
  HIP_TRY(ctx, hipGetLastError());
  launch_peak_scan(ctx->stream, static_cast<const uint32_t*>(as.tp_sizes.p), (uint32_t)rows, static_cast<int64_t*>(as.tp_row_start.p),
                   static_cast<uint32_t*>(as.tp_block_sums.p), static_cast<int64_t*>(as.tp_block_start.p));
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(as.h_tp_total.p, static_cast<const int64_t*>(as.tp_row_start.p) + rows, sizeof(int64_t),
                              hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(as.counted, ctx->stream));
  return ATTPC_OK;
}

// ... second half, once the host knows the chunk's `total` bytes: the records into as.tp_bytes on S; as.tp_row_start
// then holds the offsets + `base` (the bytes of the call's chunks before this one).
int32_t enqueue_trace_pack_write(attpc_ctx* ctx, AsmSet& as, int64_t rows, const int16_t* samples, int64_t total, int64_t base) {
  int32_t rc;
  if ((size_t)total > as.tp_bytes.bytes && (rc = ensure(ctx, as.tp_bytes, (size_t)total + (size_t)total / 8))) return rc;
  const uint32_t limit = ctx->opt_trace_pack_workgroups > 0 ? (uint32_t)ctx->opt_trace_pack_workgroups : (uint32_t)ctx->n_cus * 8u;
  launch_trace_pack_write(ctx->stream, trace_pack_workgroups((uint32_t)rows, limit), (uint32_t)rows, samples,
                          static_cast<const uint4*>(as.tp_headers.p), static_cast<int64_t*>(as.tp_row_start.p), base,
                          static_cast<unsigned char*>(as.tp_bytes.p));
  HIP_TRY(ctx, hipGetLastError());
  return ATTPC_OK;
}

// deliver() of packed traces: the chunk's `total` rows are written (as.traced is recorded behind them, and behind the
// trigger).  Queue the size pass and the scan on S and wait for the chunk's bytes alone (an event of its own: the one
// host round trip of the stage, as in deliver_trace_rows -- the bytes size the record buffer, rebase the next chunk's
// row_start and answer the capacity); then the write pass, and on C the copies of row_start, bytes, pads and labels.
int32_t deliver_packed_traces(attpc_ctx* ctx, RunOut& o, AsmSet& as, int64_t total, int64_t base, bool fits) {
  attpc_trace_packed_out* out = o.tpacked;
  const int16_t* samples = static_cast<const int16_t*>(as.tr_samples.p);
  const int64_t byte_base = o.bytes;
  int64_t chunk_bytes = 0;
  int32_t rc;
  if (total > 0) {
    if ((rc = enqueue_trace_pack_size(ctx, as, total, samples))) return rc;
    HIP_TRY(ctx, hipEventSynchronize(as.counted));
    chunk_bytes = as.h_tp_total[0];
    if ((rc = enqueue_trace_pack_write(ctx, as, total, samples, chunk_bytes, byte_base))) return rc;
    HIP_TRY(ctx, hipEventRecord(as.traced, ctx->stream));
  }
  o.bytes = byte_base + chunk_bytes;
  if (out->bytes && o.bytes > out->byte_capacity) fits = false;
  if (!fits) o.over = true;
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream_c, as.traced, 0));
  if (total > 0 && fits) {
    if (out->row_start)  // (entry `base` is the chunk before's last, or the 0 the entry point wrote)
      HIP_TRY(ctx, hipMemcpyAsync(out->row_start + base + 1, static_cast<const int64_t*>(as.tp_row_start.p) + 1,
                                  (size_t)total * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream_c));
    if (out->bytes)
      HIP_TRY(ctx, hipMemcpyAsync(out->bytes + byte_base, as.tp_bytes.p, (size_t)chunk_bytes, hipMemcpyDeviceToHost, ctx->stream_c));
  }
  return copy_traces(ctx, as, total, base, o.trace, fits);  // pads and labels (no samples: NULL there)
}

// The flags pack_rows_kernel / launch_spyral_write leave behind the transfer records (of `record` bytes) of `as`.
int64_t* packed_flag(const AsmSet& as, size_t record) {
  return reinterpret_cast<int64_t*>(static_cast<char*>(as.packed.p) + as.row_cap * record);
}

// pack_rows_kernel on S: the event-ordered cloud of `as` into its transfer records (8-byte ones when `tight`).
int32_t launch_pack_rows(attpc_ctx* ctx, AsmSet& as, uint32_t n, int tight) {
  launch_pack_rows_kernel(ctx->stream, (uint32_t)ctx->n_cus * 8u, static_cast<const int64_t*>(as.ev_start.p), n,
                          static_cast<const double*>(as.points.p), static_cast<const int64_t*>(as.labels.p),
                          static_cast<PackedRow*>(as.packed.p), packed_flag(as, sizeof(PackedRow)), tight);
  HIP_TRY(ctx, hipGetLastError());
  return ATTPC_OK;
}

// The Spyral write pass on S: the event-ordered cloud of `as` as converted, thresholded, z-sorted rows into
// sp_rows / sp_labels, or into records (`packed`, with their flag) when those are given.
int32_t launch_spyral_rows(attpc_ctx* ctx, AsmSet& as, uint32_t n, SpyralPacked* packed, int64_t* flag) {
  launch_spyral_write(ctx->stream, ctx->spyral, n, static_cast<const int64_t*>(as.ev_start.p),
                      static_cast<const int64_t*>(as.kept_start.p), static_cast<const double*>(as.points.p),
                      static_cast<const int64_t*>(as.labels.p), static_cast<double*>(as.sp_rows.p),
                      static_cast<int64_t*>(as.sp_labels.p), static_cast<uint32_t*>(ctx->sort_idx.p),
                      static_cast<double*>(ctx->sort_key.p), packed, flag);
  HIP_TRY(ctx, hipGetLastError());
  return ATTPC_OK;
}

// Assembly tail of clouds: the CSR offsets to pinned memory, and for a compact transfer the rows packed into records.
int32_t assemble_cloud(attpc_ctx* ctx, AsmSet& as, uint32_t n) {
  HIP_TRY(ctx, hipMemcpyAsync(as.h_start.p, as.ev_start.p, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  if (!ctx->opt_compact) return ATTPC_OK;
  int32_t rc;
  if ((rc = ensure(ctx, as.packed, as.row_cap * sizeof(PackedRow) + 2 * sizeof(int64_t)))) return rc;
  int64_t* d_flag = packed_flag(as, sizeof(PackedRow));
  HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, 2 * sizeof(int64_t), ctx->stream));
  if ((rc = launch_pack_rows(ctx, as, n, ctx->opt_compact == 2 ? 1 : 0))) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(as.h_total.p, d_flag, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  return ATTPC_OK;
}

// Assembly tail of Spyral rows: the kept-row counts, their scan, the converted, thresholded, z-sorted rows (or their
// records), and the CSR offsets of the kept rows to pinned memory.
int32_t assemble_spyral(attpc_ctx* ctx, AsmSet& as, uint32_t n) {
  const size_t cap = as.row_cap;
  int32_t rc;
  if ((rc = ensure(ctx, as.kept, (size_t)n * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, as.kept_start, ((size_t)n + 1) * sizeof(int64_t)))) return rc;
  if ((rc = ensure(ctx, as.sp_rows, cap * 8 * sizeof(double)))) return rc;
  if ((rc = ensure(ctx, as.sp_labels, cap * sizeof(int64_t)))) return rc;
  if ((rc = ensure(ctx, ctx->sort_idx, cap * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, ctx->sort_key, cap * sizeof(double)))) return rc;
  launch_spyral_count(ctx->stream, ctx->spyral, n, static_cast<const int64_t*>(as.ev_start.p),
                      static_cast<const double*>(as.points.p), static_cast<uint32_t*>(as.kept.p));
  HIP_TRY(ctx, hipGetLastError());
  launch_exclusive_scan(ctx->stream, static_cast<const uint32_t*>(as.kept.p), n, static_cast<int64_t*>(as.kept_start.p), nullptr);
  HIP_TRY(ctx, hipGetLastError());
  SpyralPacked* d_packed = nullptr;
  int64_t* d_flag = nullptr;
  if (ctx->opt_compact) {  // 24-byte records instead of rows of 8 doubles + label; the flag sits behind them
    if ((rc = ensure(ctx, as.packed, cap * sizeof(SpyralPacked) + 2 * sizeof(int64_t)))) return rc;
    d_packed = static_cast<SpyralPacked*>(as.packed.p);
    d_flag = packed_flag(as, sizeof(SpyralPacked));
    HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, 2 * sizeof(int64_t), ctx->stream));
  }
  if ((rc = launch_spyral_rows(ctx, as, n, d_packed, d_flag))) return rc;
  if (ctx->opt_compact) HIP_TRY(ctx, hipMemcpyAsync(as.h_total.p, d_flag, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(as.h_start.p, as.kept_start.p, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  return ATTPC_OK;
}

// Queue, behind the scatter of slot `slot` on S, the assembly of its cloud into `as`: CSR offsets by a device scan of
// the per-event row counts, rows gathered into event order, the row counts copied to pinned memory, then the tail of
// the mode (assemble_cloud, assemble_spyral, or for traces the count pass and the scan of the kept pad rows -- the
// write pass follows once the host knows their number, deliver); as.ready is recorded at the end.  `seed` /
// `first_global`: the run's seed and the chunk's first global event id (the noise of the traces).
// `selected`: the chunk (events e0 .. of its batch) went through enqueue_select -- the offsets come from sel_rows and the
// gather skips the segments of the events that did not pass (select.hip).
int32_t enqueue_assembly(attpc_ctx* ctx, int slot, AsmSet& as, uint32_t n, OutMode mode, uint64_t seed, uint64_t first_global,
                         bool selected = false, uint32_t e0 = 0) {
  int32_t rc;
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, as.copied, 0));  // the set's previous contents have left
  // rows of the scatter launch queued just before (same stream, same slot), kept with 12 % headroom
  if ((size_t)ctx->launch_row_cap > as.row_cap) as.row_cap = (size_t)ctx->launch_row_cap + (size_t)ctx->launch_row_cap / 8;
  if ((rc = ensure_asm_cloud(ctx, as, n, as.row_cap))) return rc;
  GatherArgs g{};
  g.chunk = chunk_view(ctx, slot);
  g.out_capacity = (int64_t)as.row_cap;
  g.n_events = n;
  g.event0 = e0;
  g.passed = selected ? static_cast<const uint8_t*>(ctx->sel_passed.p) : nullptr;
  g.ev_start = static_cast<const int64_t*>(as.ev_start.p);
  g.out_points = static_cast<double*>(as.points.p);
  g.out_labels = static_cast<int64_t*>(as.labels.p);
  launch_exclusive_scan(ctx->stream, static_cast<const uint32_t*>(selected ? ctx->sel_rows.p : ctx->ev_rows.p), n,
                        static_cast<int64_t*>(as.ev_start.p), g.chunk.ctrl);
  HIP_TRY(ctx, hipGetLastError());
  launch_gather(ctx->stream, g, selected, 4096);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(as.h_ev_rows.p, ctx->ev_rows.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (makes_traces(mode)) rc = enqueue_trace_count(ctx, as, n, as.row_cap, seed, first_global);
  else if (mode == OutMode::spyral) rc = assemble_spyral(ctx, as, n);
  else rc = assemble_cloud(ctx, as, n);
  if (rc) return rc;
  HIP_TRY(ctx, hipEventRecord(as.ready, ctx->stream));
  return ATTPC_OK;
}

void unpacker_main(attpc_ctx* ctx) {
  (void)hipSetDevice(ctx->device);
  for (;;) {
    UnpackJob job;
    {
      std::unique_lock<std::mutex> lock(ctx->unpack_mutex);
      ctx->unpack_cv.wait(lock, [&] { return ctx->unpack_stop || !ctx->unpack_jobs.empty(); });
      if (ctx->unpack_jobs.empty()) return;  // stop requested and nothing left
      job = ctx->unpack_jobs.front();
      ctx->unpack_jobs.pop_front();
    }
    const bool ok = hipEventSynchronize(job.copied) == hipSuccess;
    if (ok && job.spyral) {
      SpyralHostTables t;
      t.centers = ctx->h_pad_centers.data();
      t.sizes = ctx->h_pad_sizes.data();
      t.n_pads = ctx->spyral.n_pads;
      t.r_max = ctx->spyral.r_max;
      t.window_edge = ctx->spyral.window_edge;
      t.mm_edge = ctx->spyral.mm_edge;
      t.length = ctx->spyral.length;
      unpack_spyral_rows(static_cast<const SpyralPacked*>(job.src), job.rows, t, job.points, job.labels, ctx->opt_unpack_threads);
    } else if (ok && job.tight) {
      unpack_rows8(static_cast<const unsigned long long*>(job.src), job.rows, job.offsets.data(), (int64_t)job.offsets.size() - 1,
                   job.seed, job.first_event, job.points, job.labels, ctx->opt_unpack_threads);
    } else if (ok) {
      unpack_rows(static_cast<const PackedRow*>(job.src), job.rows, job.points, job.labels, ctx->opt_unpack_threads);
    }
    {
      std::lock_guard<std::mutex> lock(ctx->unpack_mutex);
      ctx->unpack_done++;
      if (!ok) ctx->unpack_failed = true;
    }
    ctx->unpack_cv.notify_all();
  }
}

uint64_t submit_unpack(attpc_ctx* ctx, const UnpackJob& job) {
  uint64_t ticket;
  {
    std::lock_guard<std::mutex> lock(ctx->unpack_mutex);
    if (!ctx->unpacker.joinable()) ctx->unpacker = std::thread(unpacker_main, ctx);
    ctx->unpack_jobs.push_back(job);
    ticket = ++ctx->unpack_submitted;
  }
  ctx->unpack_cv.notify_all();
  return ticket;
}

int32_t wait_unpacked(attpc_ctx* ctx, uint64_t ticket);

// Every run entry point holds one of these: whatever way the call ends, no expansion job may outlive it (the
// jobs write into the caller's arrays).
struct UnpackDrain {
  attpc_ctx* ctx;
  explicit UnpackDrain(attpc_ctx* c) : ctx(c) {}
  ~UnpackDrain() {
    std::unique_lock<std::mutex> lock(ctx->unpack_mutex);
    ctx->unpack_cv.wait(lock, [&] { return ctx->unpack_done >= ctx->unpack_submitted; });
  }
};

// Queue the copy of the chunk's cloud or Spyral rows in `as` (`total` rows, to rows base .. of the caller's arrays) on
// C -- as compact records that the unpacker thread expands, or as they are -- and record as.copied.  `fits`: the rows
// fit the caller's capacity (else nothing is copied).
int32_t copy_rows(attpc_ctx* ctx, AsmSet& as, uint32_t n, const RunOut& o, int64_t base, int64_t total, bool fits,
                  uint64_t seed, uint64_t chunk_first_global) {
  const bool spyral = o.mode == OutMode::spyral;
  attpc_cloud_out* out = o.cloud;
  if (!fits || !out->points || !out->labels) {
    HIP_TRY(ctx, hipEventRecord(as.copied, ctx->stream_c));
    return ATTPC_OK;
  }
  const bool compact = ctx->opt_compact && as.h_total[0] == 0;  // [0]: a row of the chunk does not fit the record
  const bool tight = compact && !spyral && ctx->opt_compact == 2 && as.h_total[1] == 0;  // [1]: ... the 8-byte record
  int32_t rc;
  if (total > 0 && compact && !spyral && ctx->opt_compact == 2 && !tight) {
    // the pack kernel wrote 8-byte records and one of them does not hold its row: pack again, 16 bytes per row (rare)
    if ((rc = launch_pack_rows(ctx, as, n, 0))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (total > 0 && spyral && ctx->opt_compact && !compact) {
    // the write kernel produced records only: produce the rows themselves for the plain copy below (rare)
    if ((rc = launch_spyral_rows(ctx, as, n, nullptr, nullptr))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (total > 0 && compact) {
    const size_t bytes = (size_t)total * (spyral ? sizeof(SpyralPacked) : (tight ? sizeof(unsigned long long) : sizeof(PackedRow)));
    // the staging's previous occupant (two chunks back) must have been expanded; it grows with 25 % headroom
    if ((rc = wait_unpacked(ctx, as.unpack_ticket))) return rc;
    if ((rc = ensure_pinned(ctx, as.h_packed, bytes, bytes + bytes / 4))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(as.h_packed.p, as.packed.p, bytes, hipMemcpyDeviceToHost, ctx->stream_c));
    HIP_TRY(ctx, hipEventRecord(as.copied, ctx->stream_c));
    UnpackJob job;
    job.copied = as.copied;
    job.src = as.h_packed.p;
    job.rows = total;
    job.points = out->points + base * (spyral ? 8 : 3);
    job.labels = out->labels + base;
    job.spyral = spyral;
    if (tight) {
      job.tight = true;
      job.seed = seed;
      job.first_event = chunk_first_global;
      job.offsets.assign(as.h_start.p, as.h_start.p + n + 1);
    }
    as.unpack_ticket = submit_unpack(ctx, job);
    return ATTPC_OK;
  } else if (total > 0) {
    const size_t width = spyral ? 8 : 3;
    HIP_TRY(ctx, hipMemcpyAsync(out->points + base * width, spyral ? as.sp_rows.p : as.points.p, (size_t)total * width * sizeof(double),
                                hipMemcpyDeviceToHost, ctx->stream_c));
    HIP_TRY(ctx, hipMemcpyAsync(out->labels + base, spyral ? as.sp_labels.p : as.labels.p, (size_t)total * sizeof(int64_t),
                                hipMemcpyDeviceToHost, ctx->stream_c));
  }
  HIP_TRY(ctx, hipEventRecord(as.copied, ctx->stream_c));
  return ATTPC_OK;
}

// The chunk of `n` events in `as` is assembled and its offsets are in as.h_start (as.ready has fired; its events are
// first_local .. of the call, first_global .. globally): write its offsets and event_points into the caller's arrays,
// move the row cursor past it and queue its copy on C (traces: behind their write pass on S).  A chunk beyond the
// caller's capacity sets o.over and is not copied.
int32_t deliver_trace_rows(attpc_ctx* ctx, RunOut& o, AsmSet& as, uint32_t n, uint64_t first_local, uint64_t seed,
                           uint64_t first_global);

// The row cursor of `o` past the chunk of `n` events in `as` whose CSR offsets are `start` [n + 1]: its offsets and
// event_points into the caller's arrays; false, and o.over, if the caller's capacity does not hold its rows.
bool advance_rows(RunOut& o, const AsmSet& as, const Pinned<int64_t>& start, uint32_t n, uint64_t first_local) {
  if (int64_t* offsets = o.offsets())
    for (uint32_t i = 0; i <= n; ++i) offsets[first_local + i] = o.rows + start[i];
  if (int64_t* event_points = o.event_points())
    for (uint32_t i = 0; i < n; ++i) event_points[first_local + i] = (int64_t)as.h_ev_rows[i];
  o.rows += start[n];
  const bool fits = !o.bounded() || o.rows <= o.capacity();
  if (!fits) o.over = true;
  return fits;
}

int32_t deliver(attpc_ctx* ctx, RunOut& o, AsmSet& as, uint32_t n, uint64_t first_local, uint64_t seed, uint64_t first_global) {
  if (o.mode == OutMode::trace_rows) return deliver_trace_rows(ctx, o, as, n, first_local, seed, first_global);
  const int64_t base = o.rows, total = as.h_start[n];
  const bool fits = advance_rows(o, as, as.h_start, n, first_local);
  if (o.mode != OutMode::traces) return copy_rows(ctx, as, n, o, base, total, fits, seed, first_global);
  if (n) ctx->trace_rows_per_event = std::max((double)total / (double)n, 1.0e-3);
  int32_t rc;
  if ((rc = enqueue_trace_write(ctx, as, n, total, seed, first_global))) return rc;
  if (ctx->tg_records.made() && (rc = enqueue_trigger(ctx, as, n, total, first_local, false))) return rc;
  if (o.tpacked) return deliver_packed_traces(ctx, o, as, total, base, fits);
  return copy_traces(ctx, as, total, base, o.trace, fits);
}

// deliver() of trace rows: the chunk's traces are counted (as.h_start) but not written.  Queue on S their write pass and
// behind it the peak count pass, the scans of the points per trace row and per event and the copy of the latter to
// pinned memory; wait for that copy alone (an event: the one host round trip of the stage -- the number of points
// sizes what follows and the caller's offsets need it -- does not drain what else is queued on S); then queue the record pass and the per-event sort into rows, and their copy on C.
int32_t deliver_trace_rows(attpc_ctx* ctx, RunOut& o, AsmSet& as, uint32_t n, uint64_t first_local, uint64_t seed,
                           uint64_t first_global) {
  const int64_t base = o.rows, traces = as.h_start[n];
  if (n) ctx->trace_rows_per_event = std::max((double)traces / (double)n, 1.0e-3);
  int32_t rc;
  if ((rc = enqueue_trace_write(ctx, as, n, traces, seed, first_global))) return rc;
  const bool gated = ctx->tg_records.made() && ctx->trigger_gate;
  if (ctx->tg_records.made() && (rc = enqueue_trigger(ctx, as, n, traces, first_local, gated))) return rc;
  const uint8_t* row_pass = gated ? static_cast<const uint8_t*>(as.tg_row_pass.p) : nullptr;
  const size_t tr = (size_t)std::max<int64_t>(traces, 1);
  if ((rc = ensure(ctx, as.pk_maps, tr * 64))) return rc;
  if ((rc = ensure(ctx, as.pk_counts, tr * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(ctx, as.pk_row_start, (tr + 1) * sizeof(int64_t)))) return rc;
  if ((rc = ensure(ctx, as.pk_ev_start, ((size_t)n + 1) * sizeof(int64_t)))) return rc;
  if ((rc = ensure_pinned(ctx, as.h_pk_start, (size_t)n + 1))) return rc;
  const int16_t* pedestals = ctx->noise_on ? ctx->noise.pedestals : nullptr;
  const int32_t* d_pads = static_cast<const int32_t*>(as.tr_pads.p);
  const int16_t* d_samples = static_cast<const int16_t*>(as.tr_samples.p);
  if (ctx->baseline_on) {  // step 1 of the contract is the fitted baseline: the peak kernels read y rows, no pedestal
    if ((rc = ensure(ctx, as.pk_y, tr * ATTPC_NUM_TB * sizeof(int16_t)))) return rc;
    if (traces > 0) {
      launch_baseline(ctx->stream, (uint32_t)traces, d_samples, static_cast<const double2*>(ctx->bl_twiddle.p),
                      static_cast<const double*>(ctx->bl_filter.p), static_cast<int16_t*>(as.pk_y.p), nullptr);
      HIP_TRY(ctx, hipGetLastError());
    }
    d_samples = static_cast<const int16_t*>(as.pk_y.p);
    pedestals = nullptr;
  }
  if (traces > 0) {
    launch_peak_count(ctx->stream, ctx->peaks, pedestals, (uint32_t)traces, d_pads, d_samples,
                      static_cast<uint8_t*>(as.pk_maps.p), static_cast<uint32_t*>(as.pk_counts.p), row_pass);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (traces > 0) {
    const size_t blocks = peak_scan_blocks((uint32_t)traces);
    if ((rc = ensure(ctx, as.pk_block_sums, blocks * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(ctx, as.pk_block_start, (blocks + 1) * sizeof(int64_t)))) return rc;
    launch_peak_scan(ctx->stream, static_cast<const uint32_t*>(as.pk_counts.p), (uint32_t)traces,
                     static_cast<int64_t*>(as.pk_row_start.p), static_cast<uint32_t*>(as.pk_block_sums.p),
                     static_cast<int64_t*>(as.pk_block_start.p));
  } else {
    HIP_TRY(ctx, hipMemsetAsync(as.pk_row_start.p, 0, sizeof(int64_t), ctx->stream));
  }
  HIP_TRY(ctx, hipGetLastError());
  launch_peak_event_start(ctx->stream, n, static_cast<const int64_t*>(as.kept_start.p),
                          static_cast<const int64_t*>(as.pk_row_start.p), static_cast<int64_t*>(as.pk_ev_start.p));
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(as.h_pk_start.p, as.pk_ev_start.p, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(as.counted, ctx->stream));
  HIP_TRY(ctx, hipEventSynchronize(as.counted));
  const int64_t total = as.h_pk_start[n];
  const bool fits = advance_rows(o, as, as.h_pk_start, n, first_local);
  if (total > 0) {
    if ((size_t)total > as.pk_cap) as.pk_cap = (size_t)total + (size_t)total / 8;
    if ((rc = ensure(ctx, as.pk_records, as.pk_cap * sizeof(uint4)))) return rc;
    if ((rc = ensure(ctx, as.pk_centroid, as.pk_cap * sizeof(double)))) return rc;
    if ((rc = ensure(ctx, ctx->sort_idx, as.pk_cap * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(ctx, ctx->sort_key, as.pk_cap * sizeof(double)))) return rc;
    if ((rc = ensure(ctx, as.sp_rows, as.pk_cap * 8 * sizeof(double)))) return rc;
    if ((rc = ensure(ctx, as.sp_labels, as.pk_cap * sizeof(int64_t)))) return rc;
    launch_peak_write(ctx->stream, ctx->peaks, pedestals, (uint32_t)traces, d_pads, d_samples,
                      static_cast<const uint8_t*>(as.pk_maps.p), static_cast<const int64_t*>(as.pk_row_start.p),
                      static_cast<uint4*>(as.pk_records.p), row_pass);
    HIP_TRY(ctx, hipGetLastError());
    launch_peak_rows(ctx->stream, ctx->spyral, seed, n, first_global, static_cast<const int64_t*>(as.pk_ev_start.p),
                     static_cast<const uint4*>(as.pk_records.p), d_pads, static_cast<const int64_t*>(as.tr_labels.p),
                     static_cast<double*>(as.pk_centroid.p), static_cast<uint32_t*>(ctx->sort_idx.p),
                     static_cast<double*>(ctx->sort_key.p), static_cast<double*>(as.sp_rows.p),
                     static_cast<int64_t*>(as.sp_labels.p), static_cast<unsigned long long*>(ctx->peak_sums.p));
    HIP_TRY(ctx, hipGetLastError());
    if (ctx->correction_on && (rc = enqueue_correction(ctx, as, n))) return rc;
  }
  const bool clustered = ctx->cl_events.made() && n > 0;
  if (clustered && (rc = enqueue_clustering(ctx, as, n))) return rc;  // (an event without rows has a record too)
  HIP_TRY(ctx, hipEventRecord(as.traced, ctx->stream));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream_c, as.traced, 0));
  if ((rc = copy_chunk(ctx, ctx->cl_events, as.cl_events, first_local, n))) return rc;
  if ((rc = copy_chunk(ctx, ctx->cl_records, as.cl_records, first_local, n))) return rc;
  if ((rc = copy_chunk(ctx, ctx->jn_events, as.jn_events, first_local, n))) return rc;
  if ((rc = copy_chunk(ctx, ctx->jn_records, as.jn_records, first_local, n))) return rc;
  if (clustered && ctx->cl_events.to_host && ctx->call.cluster_rows >= 0 && fits && o.cloud->points) {
    if (total > 0)
      HIP_TRY(ctx, hipMemcpyAsync(ctx->h_cl_labels.p + base, as.cl_labels.p, (size_t)total * sizeof(int64_t),
                                  hipMemcpyDeviceToHost, ctx->stream_c));
    ctx->call.cluster_rows = base + total;
  }
  if (total > 0 && fits) {
    const ChunkRows made = chunk_rows(ctx, as);
    if (o.cloud->points)
      HIP_TRY(ctx, hipMemcpyAsync(o.cloud->points + base * 8, made.rows, (size_t)total * 8 * sizeof(double), hipMemcpyDeviceToHost,
                                  ctx->stream_c));
    if (o.cloud->labels)
      HIP_TRY(ctx, hipMemcpyAsync(o.cloud->labels + base, made.labels, (size_t)total * sizeof(int64_t), hipMemcpyDeviceToHost,
                                  ctx->stream_c));
  }
  if (ctx->est_records.made() && (rc = enqueue_estimates(ctx, as, n, first_local))) return rc;
  HIP_TRY(ctx, hipEventRecord(as.copied, ctx->stream_c));
  return ATTPC_OK;
}

// The traces of n host-side events (attpc_traces_at; a run's batch with nothing to scatter in a readout mode) on
// assembly set 0, delivered into o as events first_local .. of the call, global ids first_event ..: `offsets` [n + 1]
// their rows in points / labels (nullptr: n events without rows).  In a readout mode a chunk holds at most
// TRACE_CHUNK_ROWS / |S| events, so the device output stays bounded whatever n is; in hit mode the n events are one
// chunk (their kept rows are bounded by the rows given).
int32_t trace_host_events(attpc_ctx* ctx, RunOut& o, uint64_t first_local, uint32_t n, const int64_t* offsets,
                          const double* points, const int64_t* labels, uint64_t seed, uint64_t first_event) {
  AsmSet& as = ctx->aset[0];
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // the set's previous contents have left
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream_c));
  uint32_t step = ctx->readout_mode != ATTPC_READOUT_HIT && ctx->readout_pads > 0
                      ? (uint32_t)std::max<int64_t>(1, TRACE_CHUNK_ROWS / ctx->readout_pads)
                      : std::max<uint32_t>(n, 1);
  if (ctx->common_on) step = std::min(step, common_chunk_events(ctx));  // 1 KiB of values per (event, group)
  uint32_t e0 = 0;
  do {
    const uint32_t m = std::min(step, n - e0);
    const int64_t lo = offsets ? offsets[e0] : 0, rows = offsets ? offsets[e0 + m] - lo : 0;
    const size_t cap = (size_t)std::max<int64_t>(rows, 1);
    int32_t rc;
    if ((rc = ensure_asm_cloud(ctx, as, m, cap))) return rc;
    std::vector<int64_t> start((size_t)m + 1, 0);
    if (offsets) chunk_starts(offsets, e0, e0 + m, &start);
    HIP_TRY(ctx, hipMemcpyAsync(as.ev_start.p, start.data(), start.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    if (rows > 0) {
      HIP_TRY(ctx, hipMemcpyAsync(as.points.p, points + 3 * lo, (size_t)rows * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(ctx, hipMemcpyAsync(as.labels.p, labels + lo, (size_t)rows * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    }
    if ((rc = enqueue_trace_count(ctx, as, m, cap, seed, first_event + e0))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the copies above read pageable memory: nothing of it stays in flight)
    for (uint32_t e = 0; e < m; ++e) as.h_ev_rows[e] = (uint32_t)(start[e + 1] - start[e]);  // event_points: the caller's
    if ((rc = deliver(ctx, o, as, m, first_local + e0, seed, first_event + e0))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream_c));  // the next chunk overwrites the set
    e0 += m;
  } while (e0 < n);
  return ATTPC_OK;
}

// Wait until expansion job `ticket` (and every earlier one) is done: the staging it read is free again and its
// rows are in the caller's arrays.
int32_t wait_unpacked(attpc_ctx* ctx, uint64_t ticket) {
  std::unique_lock<std::mutex> lock(ctx->unpack_mutex);
  ctx->unpack_cv.wait(lock, [&] { return ctx->unpack_done >= ticket || ctx->unpack_failed; });
  if (ctx->unpack_failed) return fail(ctx, ATTPC_E_HIP, "waiting for a device-to-host copy failed in the expansion thread");
  return ATTPC_OK;
}

// ------------------------------------------------------------------ summaries (summary.hip) ----
// ensure() for a buffer that launches already queued on S may use: S is drained before it is re-allocated
int32_t ensure_idle(attpc_ctx* ctx, DevBuf& b, size_t bytes) {
  if (bytes <= b.bytes) return ATTPC_OK;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return ensure(ctx, b, bytes);
}

attpc_event_summary empty_event_summary() {
  attpc_event_summary r{};
  r.tb_min = r.tb_max = -1;
  return r;
}

// 4 bits per label, 16 labels a word: the first position of layout->indices that holds the label, 15 = none
void label_positions(const attpc_event_layout& lay, uint64_t nibbles[2]) {
  nibbles[0] = nibbles[1] = ~0ull;
  for (int label = 0; label < ATTPC_MAX_ROWS; ++label)
    for (int s = 0; s < lay.n_sim; ++s)
      if (lay.indices[s] == label) {
        uint64_t& word = nibbles[label / 16];
        word = (word & ~(15ull << (4 * (label % 16)))) | ((uint64_t)s << (4 * (label % 16)));
        break;
      }
}

// The records of `n` events of a batch (its events e0 ..), queued on S behind the launch that wrote the cloud
// `chunk`.  trk == nullptr: no tracks, the empty track parts.
int32_t enqueue_summary(attpc_ctx* ctx, const ChunkView& chunk, const attpc_event_layout& lay, const TrackBuffers* trk,
                        uint32_t e0, uint32_t n) {
  int32_t rc;
  if (n == 0) return ATTPC_OK;
  const size_t n_alloc = std::max<size_t>(n, (size_t)std::max(1, ctx->chunk_events));
  if ((rc = ensure_idle(ctx, ctx->sm_seg_count, n_alloc * sizeof(uint32_t)))) return rc;
  if ((rc = ensure_idle(ctx, ctx->sm_seg_start, (n_alloc + 1) * sizeof(int64_t)))) return rc;
  if ((rc = ensure_idle(ctx, ctx->sm_seg_rank, (size_t)std::max<int64_t>(chunk.seg_capacity, 1) * sizeof(uint32_t)))) return rc;
  if ((rc = ensure_idle(ctx, ctx->sm_seg_list, (size_t)std::max<int64_t>(chunk.seg_capacity, 1) * sizeof(uint32_t)))) return rc;
  SummaryArgs a{};
  a.chunk = chunk;
  a.n_events = n;
  a.event0 = e0;
  a.seg_count = static_cast<uint32_t*>(ctx->sm_seg_count.p);
  a.seg_rank = static_cast<uint32_t*>(ctx->sm_seg_rank.p);
  a.seg_start = static_cast<const int64_t*>(ctx->sm_seg_start.p);
  a.seg_list = static_cast<uint32_t*>(ctx->sm_seg_list.p);
  if (trk) a.trk = *trk;
  a.n_sim = lay.n_sim;
  label_positions(lay, a.slot_nibbles);
  a.min_electrons = ctx->summary_min;
  a.pad_centers = ctx->summary_centers;
  a.events = static_cast<attpc_event_summary*>(ctx->sm_events.p);
  a.tracks = lay.n_sim ? static_cast<attpc_track_summary*>(ctx->sm_tracks.p) : nullptr;
  HIP_TRY(ctx, hipMemsetAsync(ctx->sm_seg_count.p, 0, (size_t)n * sizeof(uint32_t), ctx->stream));
  const uint32_t seg_wgs = (uint32_t)std::min<int64_t>((int64_t)ctx->n_cus * 4, (std::max<int64_t>(chunk.seg_capacity, 1) + 255) / 256);
  launch_summary_count(ctx->stream, a, seg_wgs);
  HIP_TRY(ctx, hipGetLastError());
  launch_exclusive_scan(ctx->stream, static_cast<const uint32_t*>(ctx->sm_seg_count.p), n, static_cast<int64_t*>(ctx->sm_seg_start.p), chunk.ctrl);
  HIP_TRY(ctx, hipGetLastError());
  launch_summary_fill(ctx->stream, a, seg_wgs);
  HIP_TRY(ctx, hipGetLastError());
  launch_summary_events(ctx->stream, a, std::min<uint32_t>(n, (uint32_t)ctx->n_cus * 8u));
  HIP_TRY(ctx, hipGetLastError());
  return ATTPC_OK;
}

// the record buffers of a batch of nb events
int32_t ensure_summary_records(attpc_ctx* ctx, uint32_t nb, int n_sim) {
  int32_t rc;
  if ((rc = ensure_idle(ctx, ctx->sm_events, std::max<size_t>(nb, 1) * sizeof(attpc_event_summary)))) return rc;
  return ensure_idle(ctx, ctx->sm_tracks, std::max<size_t>((size_t)nb * (size_t)std::max(n_sim, 1), 1) * sizeof(attpc_track_summary));
}

// The settled records of a batch (on the device) to the caller's arrays, as events first_local .. of the call (queued on S).
int32_t copy_summary(attpc_ctx* ctx, const attpc_summary_out* out, uint64_t first_local, uint32_t nb, int n_sim) {
  if (out->events && nb)
    HIP_TRY(ctx, hipMemcpyAsync(out->events + first_local, ctx->sm_events.p, (size_t)nb * sizeof(attpc_event_summary),
                                hipMemcpyDeviceToHost, ctx->stream));
  if (out->tracks && nb && n_sim)
    HIP_TRY(ctx, hipMemcpyAsync(out->tracks + first_local * (uint64_t)n_sim, ctx->sm_tracks.p,
                                (size_t)nb * (size_t)n_sim * sizeof(attpc_track_summary), hipMemcpyDeviceToHost, ctx->stream));
  return ATTPC_OK;
}

// ------------------------------------------------------------------ selected delivery (select.hip) ----
// The predicate on the records of `n` events of a batch (its events e0 ..), queued on S behind their summary kernels:
// passed of the batch's events, and with `ev_rows` (the chunk's rows per event) the selected rows in ctx->sel_rows.
int32_t enqueue_select(attpc_ctx* ctx, const unsigned long long* d_ctrl, int n_sim, uint32_t e0, uint32_t n, const uint32_t* ev_rows) {
  if (n == 0) return ATTPC_OK;
  int32_t rc;
  if ((rc = ensure_idle(ctx, ctx->sel_rows, std::max<size_t>(n, (size_t)std::max(1, ctx->chunk_events)) * sizeof(uint32_t)))) return rc;
  SelectArgs a{};
  a.desc = ctx->select;
  a.ctrl = d_ctrl;
  a.events = static_cast<const attpc_event_summary*>(ctx->sm_events.p);
  a.tracks = n_sim ? static_cast<const attpc_track_summary*>(ctx->sm_tracks.p) : nullptr;
  a.n_sim = n_sim;
  a.n_events = n;
  a.event0 = e0;
  a.ev_rows = ev_rows;
  a.passed = static_cast<uint8_t*>(ctx->sel_passed.p);
  a.sel_rows = ev_rows ? static_cast<uint32_t*>(ctx->sel_rows.p) : nullptr;
  launch_select(ctx->stream, a);
  HIP_TRY(ctx, hipGetLastError());
  return ATTPC_OK;
}

// mask bits of the configured selection at or above a call's n_sim
int32_t validate_select_mask(attpc_ctx* ctx, const char* name, int n_sim) {
  if (ctx->select.track_mask >> n_sim)
    return fail(ctx, ATTPC_E_INVALID, "%s: track_mask 0x%x names positions at or above n_sim = %d", name, ctx->select.track_mask, n_sim);
  return ATTPC_OK;
}

// ------------------------------------------------------------------ run maps (maps.hip) ----
unsigned long long* slot_map(attpc_ctx* ctx, int slot) {
  return static_cast<unsigned long long*>(ctx->mp_slots.p) + (size_t)slot * MAPS_CELLS;
}

// The map buffers, and the totals of the call that begins at zero (queued on S).
int32_t begin_maps_call(attpc_ctx* ctx) {
  int32_t rc;
  if ((rc = ensure_idle(ctx, ctx->mp_slots, (size_t)MAX_SLOTS * MAPS_CELLS * sizeof(unsigned long long)))) return rc;
  if ((rc = ensure_idle(ctx, ctx->mp_total, (size_t)MAPS_CELLS * sizeof(unsigned long long)))) return rc;
  HIP_TRY(ctx, hipMemsetAsync(ctx->mp_total.p, 0, (size_t)MAPS_CELLS * sizeof(unsigned long long), ctx->stream));
  return ATTPC_OK;
}

// The map of `n` events of a batch (its events e0 ..) into the map of `slot`, queued on S directly behind the chunk's
// enqueue_summary (whose seg_start / seg_list it reads) and, with `selected`, its enqueue_select (passed).  The memset
// in front makes a repeated chunk start from nothing.
int32_t enqueue_maps(attpc_ctx* ctx, const ChunkView& chunk, int slot, const attpc_event_layout& lay, uint32_t e0, uint32_t n,
                     bool selected) {
  if (n == 0) return ATTPC_OK;
  MapsArgs a{};
  a.chunk = chunk;
  a.n_events = n;
  a.event0 = e0;
  a.seg_start = static_cast<const int64_t*>(ctx->sm_seg_start.p);
  a.seg_list = static_cast<const uint32_t*>(ctx->sm_seg_list.p);
  a.passed = selected ? static_cast<const uint8_t*>(ctx->sel_passed.p) : nullptr;
  a.n_sim = lay.n_sim;
  a.track_mask = ctx->maps.track_mask;
  label_positions(lay, a.slot_nibbles);
  a.min_electrons = ctx->summary_min;
  a.map = slot_map(ctx, slot);
  HIP_TRY(ctx, hipMemsetAsync(a.map, 0, (size_t)MAPS_CELLS * sizeof(unsigned long long), ctx->stream));
  if (!launch_maps_events(ctx->stream, a, (uint32_t)ctx->n_cus))
    return fail(ctx, ATTPC_E_INVALID, "run maps: a chunk of %u events is too long for the %d workgroups' 32-bit cells", n, ctx->n_cus);
  HIP_TRY(ctx, hipGetLastError());
  return ATTPC_OK;
}

// The accepted chunk of `slot`: its map into the call's totals (queued on S).
int32_t enqueue_maps_fold(attpc_ctx* ctx, int slot) {
  launch_maps_fold(ctx->stream, slot_map(ctx, slot), static_cast<unsigned long long*>(ctx->mp_total.p));
  HIP_TRY(ctx, hipGetLastError());
  return ATTPC_OK;
}

// The end of a maps call: the totals into the caller's attpc_maps_out.  `passed` [n_events] of the selection, or nullptr
// (every event contributed).
int32_t read_maps_total(attpc_ctx* ctx, attpc_maps_out* out, uint64_t n_events, const uint8_t* passed, uint8_t* passed_out) {
  std::vector<unsigned long long> h(MAPS_CELLS);
  HIP_TRY(ctx, hipMemcpyAsync(h.data(), ctx->mp_total.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (out->pad_events) std::memcpy(out->pad_events, h.data() + MAPS_PAD_EVENTS, ATTPC_NUM_PADS * sizeof(uint64_t));
  if (out->pad_charge) std::memcpy(out->pad_charge, h.data() + MAPS_PAD_CHARGE, ATTPC_NUM_PADS * sizeof(int64_t));
  if (out->tb_events) std::memcpy(out->tb_events, h.data() + MAPS_TB_EVENTS, ATTPC_NUM_TB * sizeof(uint64_t));
  if (out->tb_rows) std::memcpy(out->tb_rows, h.data() + MAPS_TB_ROWS, ATTPC_NUM_TB * sizeof(uint64_t));
  if (out->tb_charge) std::memcpy(out->tb_charge, h.data() + MAPS_TB_CHARGE, ATTPC_NUM_TB * sizeof(int64_t));
  out->n_hit = h[MAPS_N_HIT];
  uint64_t n_in = n_events;
  if (passed) {
    n_in = 0;
    for (uint64_t e = 0; e < n_events; ++e) n_in += passed[e];
  }
  out->n_events = n_in;
  if (passed_out && n_events) {
    if (passed) std::memcpy(passed_out, passed, (size_t)n_events);
    else std::memset(passed_out, 1, (size_t)n_events);
  }
  return ATTPC_OK;
}

int32_t read_maps(attpc_ctx* ctx, const RunOut& o, uint64_t n_events) {
  return read_maps_total(ctx, o.maps, n_events, o.maps_selected ? ctx->sel_host.data() : nullptr, o.maps_passed);
}

// ------------------------------------------------------------------ the run loop ----
struct RunSource {   // where a batch's kinematics come from
  bool from_kernel = false;        // attpc_sim_run: kin_run_kernel on T
  const double* h_p4 = nullptr;    // attpc_det_run: host arrays
  const double* h_vertex = nullptr;
};

struct RunSink {     // optional host copies of the kinematics (attpc_sim_run)
  double* p4 = nullptr;
  double* vertex = nullptr;
  int32_t* status = nullptr;
};

int32_t queue_batch(attpc_ctx* ctx, TrackSet& ts, TrackLaunch& tl, const attpc_event_layout& lay, const RunSource& src,
                    uint64_t seed, uint64_t first_event, uint64_t b0, uint32_t nb, int n_rows) {
  int32_t rc;
  if ((rc = ensure_kin_buffers(ctx, ts, nb, n_rows))) return rc;
  ts.timed_kin = false;
  if (src.from_kernel) {
    HIP_TRY(ctx, hipEventRecord(ts.k0, ctx->stream_t));
    launch_kin_run(ctx->stream_t, ctx->kin, seed, first_event + b0, nb, static_cast<double*>(ts.p4.p),
                   static_cast<double*>(ts.vertex.p), static_cast<int32_t*>(ts.status.p), static_cast<uint32_t*>(ts.attempts.p));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ts.k1, ctx->stream_t));
    ts.timed_kin = true;
  } else {
    HIP_TRY(ctx, hipMemcpyAsync(ts.p4.p, src.h_p4 + b0 * n_rows * 4, (size_t)nb * n_rows * 4 * sizeof(double), hipMemcpyHostToDevice, ctx->stream_t));
    HIP_TRY(ctx, hipMemcpyAsync(ts.vertex.p, src.h_vertex + b0 * 3, (size_t)nb * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream_t));
  }
  tl.lay = lay;
  tl.seed = seed;
  tl.first_event = first_event + b0;
  tl.n = nb;
  tl.use_status = src.from_kernel;
  return launch_tracks(ctx, ts, tl);
}

// Scatter (and deliver) the chunks of one finished track batch.
// `queue_next` is called once, right after the first launches of this batch are queued on S: it queues the
// next batch's kinematics + tracks on the low-priority stream T, BEHIND scatter work, so that the track
// workgroups only take the compute units the persistent scatter workgroups leave.
template <typename QueueNext>
int32_t run_batch_chunks(attpc_ctx* ctx, const attpc_event_layout& lay, const TrackBuffers& trk, uint64_t seed,
                         uint64_t batch_first_global, uint64_t batch_first_local, uint32_t nb, RunOut& o,
                         attpc_run_stats* st, QueueNext queue_next) {
  int32_t rc;
  bool next_queued = false;
  auto queue_next_once = [&]() -> int32_t {
    if (next_queued) return ATTPC_OK;
    next_queued = true;
    return queue_next();
  };
  if (lay.n_sim == 0 || nb == 0) {  // nothing to scatter: empty clouds
    if ((rc = queue_next_once())) return rc;
    if (makes_traces(o.mode) && ctx->readout_mode != ATTPC_READOUT_HIT && nb)  // their noise-only rows
      return trace_host_events(ctx, o, batch_first_local, nb, nullptr, nullptr, nullptr, seed, batch_first_global);
    if (o.summary && o.summary->events) std::fill(o.summary->events + batch_first_local, o.summary->events + batch_first_local + nb, empty_event_summary());
    if (o.predicate() && nb) {  // the predicate on the empty records (n_sim == 0: no position to cut on)
      const uint8_t pass = select_passes(ctx->select, empty_event_summary(), nullptr, 0) ? 1 : 0;
      std::fill(ctx->sel_host.begin() + batch_first_local, ctx->sel_host.begin() + batch_first_local + nb, pass);
    }
    if (int64_t* offsets = o.offsets()) std::fill(offsets + batch_first_local, offsets + batch_first_local + nb + 1, o.rows);
    if (int64_t* event_points = o.event_points()) std::fill(event_points + batch_first_local, event_points + batch_first_local + nb, 0);
    return ATTPC_OK;
  }
  if ((rc = ensure(ctx, ctx->out_ctrl, (size_t)MAX_SLOTS * CTRL_WORDS * sizeof(unsigned long long)))) return rc;
  if ((rc = ensure(ctx, ctx->lone_list, (size_t)LONE_CAPACITY * sizeof(LoneBucket)))) return rc;
  if (!ctx->lone_ready) {  // lone_bucket_kernel's tables: zero once, the kernel leaves them zero.  The flag is set
                           // only when both allocations and both memsets went through (a call that failed half-way
                           // is repeated from the start by the next run)
    if ((rc = ensure(ctx, ctx->lone_chg, (size_t)LONE_WORKGROUPS * LONE_PADS * sizeof(unsigned long long)))) return rc;
    if ((rc = ensure(ctx, ctx->lone_mask, (size_t)LONE_WORKGROUPS * (LONE_PADS / 4) * sizeof(uint32_t)))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->lone_chg.p, 0, ctx->lone_chg.bytes, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->lone_mask.p, 0, ctx->lone_mask.bytes, ctx->stream));
    ctx->lone_ready = true;
  }
  struct Chunk { uint32_t e0, n; int slot; };
  // summary mode: the records of chunk c, queued directly behind its scatter (the next chunk overwrites the cloud)
  auto summarise = [&](const Chunk& c) -> int32_t {
    if (!o.summary) return ATTPC_OK;
    int32_t rc2;
    if ((rc2 = enqueue_summary(ctx, chunk_view(ctx, c.slot), lay, &trk, c.e0, c.n)) || !o.maps) return rc2;
    // a maps run: the chunk's map directly behind its records (the next chunk overwrites the segment lists as well)
    if (o.maps_selected && (rc2 = enqueue_select(ctx, slot_words(ctx, c.slot), lay.n_sim, c.e0, c.n, nullptr))) return rc2;
    return enqueue_maps(ctx, chunk_view(ctx, c.slot), c.slot, lay, c.e0, c.n, o.maps_selected);
  };
  if (o.summary && (rc = ensure_summary_records(ctx, nb, lay.n_sim))) return rc;
  if (o.predicate() && (rc = ensure_idle(ctx, ctx->sel_passed, std::max<size_t>(nb, 1)))) return rc;
  // The assembly of chunk c into `as`; a selected chunk first gets its records and the predicate on them, where its rows
  // lie, and only the rows of the events that pass are put in event order.
  auto assemble = [&](const Chunk& c, AsmSet& as) -> int32_t {
    int32_t rc2;
    if (o.select) {
      if ((rc2 = summarise(c))) return rc2;
      if ((rc2 = enqueue_select(ctx, slot_words(ctx, c.slot), lay.n_sim, c.e0, c.n, static_cast<const uint32_t*>(ctx->ev_rows.p)))) return rc2;
    }
    return enqueue_assembly(ctx, c.slot, as, c.n, o.mode, seed, batch_first_global + c.e0, o.select != nullptr, c.e0);
  };
  // The scatter of chunk c (and its assembly into `as`, when delivered) has completed: read its control words, and
  // while the launch ran out of room, queue it again with larger buffers (and the assembly behind it) and read again.
  auto settle = [&](const Chunk& c, AsmSet* as) -> int32_t {
    ChunkResult r;
    int64_t min_rows = 0, min_segs = 0;
    read_scatter(ctx, c.slot, c.n, &r, &min_rows, &min_segs);
    for (int attempt = 0; r.overflow && attempt < 8; ++attempt) {  // too small: run this chunk again
      int32_t rc2;
      if ((rc2 = enqueue_scatter(ctx, c.slot, lay, trk, seed, batch_first_global + c.e0, c.e0, c.n, min_rows, min_segs))) return rc2;
      if (as) {
        if ((rc2 = assemble(c, *as))) return rc2;  // (a repeated chunk overwrites its records, passed and selected rows)
        HIP_TRY(ctx, hipEventSynchronize(as->ready));
      } else {
        if ((rc2 = summarise(c))) return rc2;  // (a repeated chunk overwrites its records)
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      }
      read_scatter(ctx, c.slot, c.n, &r, &min_rows, &min_segs);
    }
    if (r.overflow) return fail(ctx, ATTPC_E_HIP, "point cloud did not fit after repeated buffer growth");
    accumulate(st, r);
    // the chunk is accepted: only now does its map count (a repetition zeroed and filled it again); the fold runs on S
    // before the slot's next chunk zeroes the map
    return o.maps ? enqueue_maps_fold(ctx, c.slot) : ATTPC_OK;
  };
  if (o.resident()) {
    // device resident: queue up to MAX_SLOTS chunks back to back, read their control words once
    uint32_t e0 = 0;
    while (e0 < nb) {
      std::vector<Chunk> group;
      while (e0 < nb && (int)group.size() < MAX_SLOTS) {
        const uint32_t n = next_chunk_events(ctx, nb - e0);
        const Chunk c{e0, n, (int)group.size()};
        if ((rc = enqueue_scatter(ctx, c.slot, lay, trk, seed, batch_first_global + e0, e0, n, 0, 0))) return rc;
        if ((rc = summarise(c))) return rc;
        group.push_back(c);
        e0 += n;
        if (ctx->rows_per_event <= 0.0) break;  // pilot chunk: size the rest from what it produced
      }
      if ((rc = queue_next_once())) return rc;
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      for (const Chunk& c : group)
        if ((rc = settle(c, nullptr))) return rc;
    }
    // every chunk of the batch has settled: its records (and passed) are final
    if (o.maps_selected)
      HIP_TRY(ctx, hipMemcpyAsync(ctx->sel_host.data() + batch_first_local, ctx->sel_passed.p, nb, hipMemcpyDeviceToHost, ctx->stream));
    return o.summary ? copy_summary(ctx, o.summary, batch_first_local, nb, lay.n_sim) : ATTPC_OK;
  }
  // delivered clouds: chunk c+1 is scattered and assembled while chunk c crosses PCIe
  Chunk prev{0, 0, -1};
  int prev_set = 0;
  uint32_t e0 = 0;
  int seq = 0;
  auto complete = [&](const Chunk& c, int set) -> int32_t {
    AsmSet& as = ctx->aset[set];
    HIP_TRY(ctx, hipEventSynchronize(as.ready));
    int32_t rc2 = settle(c, &as);
    return rc2 ? rc2 : deliver(ctx, o, as, c.n, batch_first_local + c.e0, seed, batch_first_global + c.e0);
  };
  while (e0 < nb) {
    const bool pilot = ctx->rows_per_event <= 0.0;  // only ever true with nothing in flight
    // delivered clouds are PCIe bound: small chunks, so that the copy of one hides the scatter and
    // assembly of the next from the first chunk on
    // ... and bounded in rows as well: the assembly sets, the Spyral sort scratch and the pinned staging all scale
    // with the chunk's cloud (configs[4] has 54 k points per event: 8192 such events would be 100 GB of them)
    uint32_t n = std::min<uint32_t>(next_chunk_events(ctx, nb - e0), (uint32_t)ctx->opt_deliver_chunk);
    if (ctx->rows_per_event > 0.0)
      n = std::min<uint32_t>(n, (uint32_t)std::max(256.0, (double)DELIVER_CHUNK_ROWS / ctx->rows_per_event));
    if (makes_traces(o.mode) && ctx->readout_mode != ATTPC_READOUT_HIT) {  // the first chunk too: |S| rows per event
      const double rows = ctx->readout_mode == ATTPC_READOUT_FULL || ctx->trace_rows_per_event <= 0.0
                              ? (double)ctx->readout_pads : ctx->trace_rows_per_event;
      if (rows > 0.0) n = std::min<uint32_t>(n, (uint32_t)std::max(1.0, (double)TRACE_CHUNK_ROWS / rows));
    } else if (makes_traces(o.mode) && ctx->trace_rows_per_event > 0.0)  // 1 KiB of samples per kept pad row
      n = std::min<uint32_t>(n, (uint32_t)std::max(256.0, (double)TRACE_CHUNK_ROWS / ctx->trace_rows_per_event));
    if (makes_traces(o.mode) && ctx->common_on) n = std::min(n, common_chunk_events(ctx));
    const Chunk c{e0, n, seq % MAX_SLOTS};
    const int set = seq & 1;
    // an overflow of the chunk in flight is repaired inside complete(); queue this one behind it
    if ((rc = enqueue_scatter(ctx, c.slot, lay, trk, seed, batch_first_global + e0, e0, n, 0, 0))) return rc;
    if ((rc = assemble(c, ctx->aset[set]))) return rc;
    if ((rc = queue_next_once())) return rc;
    if (prev.slot >= 0 && (rc = complete(prev, prev_set))) return rc;
    prev = c;
    prev_set = set;
    e0 += n;
    seq++;
    if (pilot) {  // size the following chunks from the pilot
      if ((rc = complete(prev, prev_set))) return rc;
      prev.slot = -1;
    }
  }
  if (prev.slot >= 0 && (rc = complete(prev, prev_set))) return rc;
  if ((rc = wait_unpacked(ctx, ctx->unpack_submitted))) return rc;  // every row is in the caller's arrays
  if (o.select) {  // every chunk of the batch has settled: its records and passed are final
    if ((rc = copy_summary(ctx, o.summary, batch_first_local, nb, lay.n_sim))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->sel_host.data() + batch_first_local, ctx->sel_passed.p, nb, hipMemcpyDeviceToHost, ctx->stream));
  }
  return queue_next_once();
}

// The trace checksums of a run, and for trace rows their row checksum, start at zero (queued on S).
int32_t reset_trace_sums(attpc_ctx* ctx, OutMode mode) {
  int32_t rc;
  if ((rc = ensure(ctx, ctx->trace_sums, 2 * sizeof(unsigned long long)))) return rc;
  HIP_TRY(ctx, hipMemsetAsync(ctx->trace_sums.p, 0, 2 * sizeof(unsigned long long), ctx->stream));
  if (mode != OutMode::trace_rows) return ATTPC_OK;
  if ((rc = ensure(ctx, ctx->peak_sums, sizeof(unsigned long long)))) return rc;
  HIP_TRY(ctx, hipMemsetAsync(ctx->peak_sums.p, 0, sizeof(unsigned long long), ctx->stream));
  ctx->correction_call = false;
  if (!ctx->correction_on) return ATTPC_OK;
  if ((rc = ensure(ctx, ctx->uc_sums, 4 * sizeof(unsigned long long)))) return rc;
  HIP_TRY(ctx, hipMemsetAsync(ctx->uc_sums.p, 0, 4 * sizeof(unsigned long long), ctx->stream));
  return ATTPC_OK;
}

// The end of a trace-row run whose copies have all arrived: its rows and row checksum for attpc_trace_rows_last.
int32_t read_peak_sums(attpc_ctx* ctx, const RunOut& o) {
  unsigned long long sum = 0ull;
  HIP_TRY(ctx, hipMemcpyAsync(&sum, ctx->peak_sums.p, sizeof sum, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  ctx->last_rows = o.rows;
  ctx->last_row_checksum = sum;
  if (ctx->correction_on) {  // the counts of the drift correction, read like the checksum: once, when the call has ended
    unsigned long long counts[4] = {0ull, 0ull, 0ull, 0ull};
    HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->uc_sums.p, sizeof counts, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->last_correction = attpc_undistort_info{(int64_t)counts[0], (int64_t)counts[1], (int64_t)counts[2], (int64_t)counts[3]};
    ctx->correction_call = true;
  }
  return ATTPC_OK;
}

// The end of a trace run whose copies have all arrived: its kept rows and checksums into the caller's attpc_trace_out.
int32_t read_trace_sums(attpc_ctx* ctx, const RunOut& o) {
  unsigned long long sums[2] = {0ull, 0ull};
  HIP_TRY(ctx, hipMemcpyAsync(sums, ctx->trace_sums.p, sizeof sums, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  o.trace->n_rows = o.rows;
  o.trace->sample_checksum = sums[0];
  o.trace->pad_checksum = sums[1];
  if (o.tpacked) o.tpacked->n_bytes = o.bytes;
  return ATTPC_OK;
}

// The end of a run: its statistics to the caller, then the verdicts on the capacity and on lost charge.
int32_t run_status(attpc_ctx* ctx, const attpc_run_stats& st, attpc_run_stats* stats, const RunOut& o) {
  if (stats) *stats = st;
  if (o.over && o.tpacked)
    return fail(ctx, ATTPC_E_CAPACITY, "packed traces need %lld rows and %lld bytes, capacity %lld rows and %lld bytes",
                (long long)o.rows, (long long)o.bytes, (long long)o.capacity(), (long long)o.tpacked->byte_capacity);
  if (o.over)
    return fail(ctx, ATTPC_E_CAPACITY, "%s %lld rows, capacity %lld",
                o.mode == OutMode::traces ? "traces need" : o.mode == OutMode::trace_rows ? "trace rows need" : "cloud needs",
                (long long)o.rows, (long long)o.capacity());
  if (st.n_failed || st.n_inconsistent)
    return fail(ctx, ATTPC_E_DATALOSS, "%llu events lost a time bucket (n_failed), %u table self-check failures (n_inconsistent) in %llu events",
                (unsigned long long)st.n_failed, st.n_inconsistent, (unsigned long long)st.n_events);
  return ATTPC_OK;
}

int32_t run_events(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events, const attpc_event_layout& lay,
                   const RunSource& src, const RunSink& sink, RunOut o, attpc_run_stats* stats) {
  int32_t rc;
  if ((rc = validate_id_range(ctx, first_event, n_events))) return rc;
  if (makes_traces(o.mode) && (rc = reset_trace_sums(ctx, o.mode))) return rc;
  if (makes_traces(o.mode) && (rc = begin_record_streams(ctx, o.mode == OutMode::trace_rows, n_events, &lay,
                                                          o.cloud && o.cloud->points ? o.cloud->capacity : -1)))
    return rc;
  // a readout run sizes its trace chunks for |S| rows per event until it has seen its own rate: the rate of an earlier
  // run says nothing once the threshold, the noise or the workload has changed (hit mode keeps the context's rate)
  if (makes_traces(o.mode) && ctx->readout_mode != ATTPC_READOUT_HIT) ctx->trace_rows_per_event = 0.0;
  UnpackDrain drain(ctx);
  attpc_run_stats st{};
  st.n_events = n_events;
  const uint64_t growths_before = ctx->n_growths;
  const int n_rows = lay.n_rows;
  if (int64_t* offsets = o.offsets()) offsets[0] = 0;
  if (o.predicate()) ctx->sel_host.assign((size_t)n_events, 0);
  if (o.maps && (rc = begin_maps_call(ctx))) return rc;
  // batches of up to MAX_SLOTS chunks (a small pilot batch while the arena need per track is unknown),
  // each integrated on T while the previous batch is scattered on S
  uint64_t b0 = 0;
  // the call starts on the track set with the larger buffers: a context's first call leaves set 0 sized for its pilot
  // batch and set 1 for a full one, and a later call of one batch per call would grow set 0 (arena and all) to the
  // same size for nothing
  int cur = ctx->tset[1].p4.bytes > ctx->tset[0].p4.bytes ? 1 : 0;
  TrackLaunch tl[2];
  auto batch_size = [&](uint64_t at) -> uint32_t {
    const uint64_t chunk = (uint64_t)std::max(1, ctx->chunk_events);
    uint64_t want = track_batch_events(ctx, lay, chunk);
    if (ctx->blocks_per_track <= 0.0) {
      want = std::min<uint64_t>(want, std::min<uint64_t>(chunk, 16384));  // pilot: sizes the arena
    } else {
      // the per-batch buffers -- the sample arena: tens of GB -- are sized for the largest batch a call of this length
      // has, not for what is left of THIS call behind its pilot batch: the next call of the same length would grow
      // them all again (8 re-allocations inside a caller's timed region)
      ctx->max_batch_events = std::max<uint32_t>(ctx->max_batch_events, (uint32_t)std::min<uint64_t>(want, n_events));
      // the first batch of a call is integrated with nothing to run beside: a shorter one (opt_first_batch_chunks
      // scatter chunks) leaves less of the call's track time exposed
      if (at == 0 && ctx->opt_first_batch_chunks > 0) want = std::min<uint64_t>(want, chunk * (uint64_t)ctx->opt_first_batch_chunks);
    }
    return (uint32_t)std::min<uint64_t>(want, n_events - at);
  };
  // the caller's announcement of the call AFTER this one (attpc_sim_hint_next) belongs to this run alone
  const bool hinted = ctx->hint_valid && src.from_kernel;
  const uint64_t hint_seed = ctx->hint_seed, hint_first = ctx->hint_first, hint_n = ctx->hint_n;
  const attpc_event_layout hint_lay = ctx->hint_lay;
  ctx->hint_valid = false;
  uint32_t nb = n_events ? batch_size(0) : 0;
  if (ctx->pre_valid && src.from_kernel && nb && ctx->pre_seed == seed && ctx->pre_first == first_event &&
      ctx->pre_nb <= n_events && same_layout(ctx->pre_lay, lay)) {
    // the previous run queued this call's first track batch behind its own last scatter launches: take it over
    ctx->pre_valid = false;
    cur = ctx->pre_set;
    nb = ctx->pre_nb;
    tl[cur].lay = lay;
    tl[cur].seed = seed;
    tl[cur].first_event = first_event;
    tl[cur].n = nb;
    tl[cur].use_status = true;
  } else {
    if ((rc = drop_prefetch(ctx))) return rc;
    if (nb && (rc = queue_batch(ctx, ctx->tset[cur], tl[cur], lay, src, seed, first_event, 0, nb, n_rows))) return rc;
  }
  while (nb) {
    TrackSet& ts = ctx->tset[cur];
    TrackBuffers trk;
    if ((rc = finish_tracks(ctx, ts, tl[cur], &trk, &st.ms_tracks, &st.n_sample_limit, &st.n_tracks_capped))) return rc;
    st.launches_tracks += 1;
    if (ts.timed_kin) {
      float ms_k = 0;
      HIP_TRY(ctx, hipEventElapsedTime(&ms_k, ts.k0, ts.k1));
      st.ms_kinematics += ms_k;
      st.launches_kinematics += 1;
    }
    // the next batch goes to the other set: the scatter chunks of the batch before this one have all
    // been read, so that set is free
    const uint64_t next_b0 = b0 + nb;
    uint32_t next_nb = 0;
    auto queue_next = [&]() -> int32_t {
      if (next_b0 >= n_events) {
        // the last batch of this call: the other track set is free, and the caller said what comes next -- that call's
        // first kinematics + track batch goes onto the low-priority stream now, behind this call's last scatter
        // launches, instead of standing alone at the head of the next call
        if (!hinted || hint_n == 0) return ATTPC_OK;
        const uint64_t chunk = (uint64_t)std::max(1, ctx->chunk_events);
        const uint32_t pre_nb = (uint32_t)std::min<uint64_t>(track_batch_events(ctx, hint_lay, chunk), hint_n);
        TrackLaunch pre_tl;
        int32_t rcq = queue_batch(ctx, ctx->tset[cur ^ 1], pre_tl, hint_lay, src, hint_seed, hint_first, 0, pre_nb, hint_lay.n_rows);
        if (rcq) return rcq;
        ctx->pre_valid = true;
        ctx->pre_set = cur ^ 1;
        ctx->pre_seed = hint_seed;
        ctx->pre_first = hint_first;
        ctx->pre_nb = pre_nb;
        ctx->pre_lay = hint_lay;
        return ATTPC_OK;
      }
      next_nb = batch_size(next_b0);
      return queue_batch(ctx, ctx->tset[cur ^ 1], tl[cur ^ 1], lay, src, seed, first_event, next_b0, next_nb, n_rows);
    };
    if (sink.status) HIP_TRY(ctx, hipMemcpyAsync(sink.status + b0, ts.status.p, (size_t)nb * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (sink.p4) HIP_TRY(ctx, hipMemcpyAsync(sink.p4 + b0 * n_rows * 4, ts.p4.p, (size_t)nb * n_rows * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (sink.vertex) HIP_TRY(ctx, hipMemcpyAsync(sink.vertex + b0 * 3, ts.vertex.p, (size_t)nb * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->rx_records.made()) {  // the truth of this batch, for the reaction reconstruction behind its chunks
      ctx->call.rx_p4 = static_cast<const double*>(ts.p4.p);
      ctx->call.rx_vertex = static_cast<const double*>(ts.vertex.p);
      ctx->call.rx_status = src.from_kernel ? static_cast<const int32_t*>(ts.status.p) : nullptr;
      ctx->call.rx_batch_first = b0;
    }
    if ((rc = run_batch_chunks(ctx, lay, trk, seed, first_event + b0, b0, nb, o, &st, queue_next))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // this set's readers are done before it is refilled
    b0 = next_b0;
    nb = next_nb;
    cur ^= 1;
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream_c));
  if (o.select) {  // (st keeps its cloud meaning over all events)
    int64_t n_passed = 0;
    for (uint8_t p : ctx->sel_host) n_passed += p;
    if (o.select->passed && n_events) std::memcpy(o.select->passed, ctx->sel_host.data(), (size_t)n_events);
    o.select->n_passed = n_passed;
    o.select->n_rows = o.rows;
  } else if (o.mode == OutMode::spyral) st.n_points = (uint64_t)o.rows;  // rows that survive the threshold
  if (o.maps && (rc = read_maps(ctx, o, n_events))) return rc;
  if (o.mode == OutMode::traces && (rc = read_trace_sums(ctx, o))) return rc;  // (the cloud's meaning stays in st)
  if (o.mode == OutMode::trace_rows) {
    st.n_points = (uint64_t)o.rows;  // the rows of the call, as in the Spyral mode
    if ((rc = read_peak_sums(ctx, o))) return rc;
    if (ctx->rx_records.made()) {  // the spectra of the call, read like the checksum: once, when the call has ended
      ctx->h_rx_cells.resize(ctx->rx_cells.bytes / sizeof(uint64_t));
      HIP_TRY(ctx, hipMemcpyAsync(ctx->h_rx_cells.data(), ctx->rx_cells.p, ctx->rx_cells.bytes, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
  }
  st.n_buffer_growths = ctx->n_growths - growths_before;
  st.device_bytes = ctx->device_bytes;
  return run_status(ctx, st, stats, o);
}

// What a trace-row call needs beside the detector: the trace settings, the Spyral geometry and the peak parameters.
int32_t trace_rows_ready(attpc_ctx* ctx, const char* name) {
  if (!ctx->trace_ready) return fail(ctx, ATTPC_E_INVALID, "%s: attpc_trace_configure has not been called", name);
  if (!ctx->spyral_ready) return fail(ctx, ATTPC_E_INVALID, "%s: attpc_spyral_configure has not been called (the geometry of the rows)", name);
  if (ctx->spyral.n_pads < ATTPC_NUM_PADS)
    return fail(ctx, ATTPC_E_INVALID, "%s: the Spyral geometry has %d pads, the traces name pads up to %d", name, ctx->spyral.n_pads,
                ATTPC_NUM_PADS - 1);
  if (ctx->spyral.window_edge == ctx->spyral.mm_edge) return fail(ctx, ATTPC_E_INVALID, "%s: windows_edge == micromegas_edge", name);
  if (!ctx->peaks_on) return fail(ctx, ATTPC_E_NOTCONFIGURED, "%s: attpc_trace_configure_peaks has not been called", name);
  return ATTPC_OK;
}

// The eight run entry points (attpc_det_run*, attpc_sim_run*; `name`) after their checks: the kinematics come from the
// host (src.h_p4 / h_vertex) or from the kinematics kernel (src.from_kernel), the output is `o`.
int32_t run_entry(const char* name, attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                  const attpc_event_layout* layout, const RunSource& src, const RunSink& sink, RunOut o, attpc_run_stats* stats) {
  if (!ctx || (!src.from_kernel && (!src.h_p4 || !src.h_vertex))) return ATTPC_E_INVALID;
  if (o.mode == OutMode::traces && !o.trace) return fail(ctx, ATTPC_E_INVALID, "%s needs an attpc_trace_out", name);
  if ((o.mode == OutMode::spyral || o.mode == OutMode::trace_rows) && !o.cloud) return fail(ctx, ATTPC_E_INVALID, "%s needs output buffers", name);
  if (src.from_kernel && !ctx->kin_ready) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_kin_configure has not been called");
  if (!ctx->det_ready) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_det_configure has not been called");
  if (o.mode == OutMode::spyral && !ctx->spyral_ready) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_spyral_configure has not been called");
  if (o.mode == OutMode::traces && !ctx->trace_ready) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_trace_configure has not been called");
  if (o.mode == OutMode::trace_rows) {
    const int32_t rc0 = trace_rows_ready(ctx, name);
    if (rc0) return rc0;
  }
  if (o.mode == OutMode::summary) {
    if (!o.summary) return fail(ctx, ATTPC_E_INVALID, "%s needs an attpc_summary_out", name);
    if (!ctx->summary_on) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_summary_configure has not been called");
  }
  if (o.maps && !ctx->maps_on) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_maps_configure has not been called");
  if (o.maps) o.maps_selected = ctx->maps.selected != 0;
  if (o.predicate()) {
    if (!ctx->summary_on) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_summary_configure has not been called");
    if (!ctx->select_on) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_select_configure has not been called");
    if (n_events > (uint64_t)INT64_MAX) return fail(ctx, ATTPC_E_INVALID, "%s: too many events", name);
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc = validate_layout(ctx, layout, true);
  if (rc) return rc;
  if (o.predicate() && (rc = validate_select_mask(ctx, name, layout->n_sim))) return rc;
  if (src.from_kernel && layout->n_rows != kin_rows(ctx))
    return fail(ctx, ATTPC_E_INVALID, "layout.n_rows=%d but the pipeline has %d rows", layout->n_rows, kin_rows(ctx));
  if ((makes_traces(o.mode) || o.mode == OutMode::summary || o.select) && (rc = drop_prefetch(ctx))) return rc;  // a trace, summary or selected call is never the announced one
  return run_events(ctx, seed, first_event, n_events, *layout, src, sink, o, stats);
}

}  // namespace

extern "C" {

int32_t attpc_version(void) { return ATTPC_ABI_VERSION; }

int32_t attpc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int32_t attpc_ctx_create(int32_t device, attpc_ctx** out) {
  if (!out) return ATTPC_E_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return ATTPC_E_NODEVICE;
  if (hipSetDevice(device) != hipSuccess) return ATTPC_E_HIP;
  attpc_ctx* ctx = new attpc_ctx();
  ctx->device = device;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) ctx->n_cus = cus;
  }
  bool ok = true;
  int prio_low = 0, prio_high = 0;
  if (hipDeviceGetStreamPriorityRange(&prio_low, &prio_high) != hipSuccess) prio_low = prio_high = 0;
  ok = ok && hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, prio_high) == hipSuccess;
  ok = ok && hipStreamCreateWithPriority(&ctx->stream_t_own, hipStreamNonBlocking, prio_low) == hipSuccess;
  pick_track_stream(ctx);
  ok = ok && hipStreamCreateWithPriority(&ctx->stream_c, hipStreamNonBlocking, prio_high) == hipSuccess;
  auto make_event = [&](hipEvent_t* e) { ok = ok && hipEventCreate(e) == hipSuccess; };
  for (TrackSet& ts : ctx->tset) {
    make_event(&ts.done); make_event(&ts.k0); make_event(&ts.k1); make_event(&ts.t0); make_event(&ts.t1);
    ok = ok && ensure_pinned(ctx, ts.h_ctrl, TRK_WORDS) == ATTPC_OK;
  }
  for (int i = 0; i < MAX_SLOTS; ++i) { make_event(&ctx->s0[i]); make_event(&ctx->s1[i]); }
  for (AsmSet& as : ctx->aset) {
    make_event(&as.ready); make_event(&as.copied); make_event(&as.traced); make_event(&as.counted);
    ok = ok && ensure_pinned(ctx, as.h_total, 2) == ATTPC_OK;
  }
  ok = ok && ensure_pinned(ctx, ctx->h_out_ctrl, (size_t)MAX_SLOTS * CTRL_WORDS) == ATTPC_OK;
  if (!ok) {
    attpc_ctx_destroy(ctx);
    return ATTPC_E_HIP;
  }
  *out = ctx;
  return ATTPC_OK;
}

int32_t attpc_ctx_destroy(attpc_ctx* ctx) {
  if (!ctx) return ATTPC_OK;
  (void)hipSetDevice(ctx->device);
  {
    std::lock_guard<std::mutex> lock(ctx->unpack_mutex);
    ctx->unpack_stop = true;
  }
  ctx->unpack_cv.notify_all();
  if (ctx->unpacker.joinable()) ctx->unpacker.join();
  if (ctx->stream_t_own) (void)hipStreamSynchronize(ctx->stream_t_own);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->stream_c) (void)hipStreamSynchronize(ctx->stream_c);
  auto destroy = [](std::initializer_list<hipEvent_t> events) {
    for (hipEvent_t e : events)
      if (e) (void)hipEventDestroy(e);
  };
  for (TrackSet& ts : ctx->tset) destroy({ts.done, ts.k0, ts.k1, ts.t0, ts.t1});
  for (AsmSet& as : ctx->aset) destroy({as.ready, as.copied, as.traced, as.counted});
  for (int i = 0; i < MAX_SLOTS; ++i) destroy({ctx->s0[i], ctx->s1[i]});
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->stream_t_own) (void)hipStreamDestroy(ctx->stream_t_own);
  if (ctx->stream_c) (void)hipStreamDestroy(ctx->stream_c);
  delete ctx;  // (frees the buffers)
  return ATTPC_OK;
}

const char* attpc_last_error(const attpc_ctx* ctx) { return ctx ? ctx->error.c_str() : "null context"; }

int32_t attpc_set_chunk_events(attpc_ctx* ctx, int32_t chunk_events) {
  if (!ctx) return ATTPC_E_INVALID;
  ctx->chunk_events = chunk_events > 0 ? chunk_events : 65536;
  return ATTPC_OK;
}

int32_t attpc_set_option(attpc_ctx* ctx, const char* name, int64_t value) {
  if (!ctx || !name) return ATTPC_E_INVALID;
  const std::string key(name);
  if (key == "scatter_variant") {
    if (value < 0 || value > 3) return fail(ctx, ATTPC_E_INVALID, "scatter_variant must be 0, 1, 2 or 3");
    ctx->opt_variant = (int)value;
  } else if (key == "reaction_spectra_only") {
    // != 0: a trace-row call in which the reaction reconstruction runs copies no stage records to the host (estimates,
    // fits, pid, reaction, clusters, joins): attpc_*_last answer ATTPC_E_NOTCONFIGURED for it, the spectra are read as ever
    ctx->opt_spectra_only = value != 0;
  } else if (key == "tiny_buffers") {
    ctx->opt_tiny = value != 0;
  } else if (key == "compact_transfer") {
    if (value < 0 || value > 2) return fail(ctx, ATTPC_E_INVALID, "compact_transfer must be 0, 1 or 2");
    ctx->opt_compact = (int)value;
  } else if (key == "deliver_chunk_events") {
    if (value < 64 || value > (1 << 20)) return fail(ctx, ATTPC_E_INVALID, "deliver_chunk_events must be 64..1048576");
    ctx->opt_deliver_chunk = (int)value;
  } else if (key == "unpack_threads") {
    if (value < 0 || value > 1024) return fail(ctx, ATTPC_E_INVALID, "unpack_threads must be 0..1024");
    ctx->opt_unpack_threads = (int)value;
  } else if (key == "serial_tracks") {
    // != 0: kinematics + track integration of the next batch are queued on the scatter stream, behind the current
    // batch's scatter launches, instead of beside them on the low-priority stream
    int32_t rcs = drop_prefetch(ctx);
    if (rcs) return rcs;
    if ((rcs = sync_all(ctx))) return rcs;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream_t_own));
    if (value < -1 || value > 1) return fail(ctx, ATTPC_E_INVALID, "serial_tracks must be -1, 0 or 1");
    ctx->opt_serial_tracks = (int)value;
    pick_track_stream(ctx);
  } else if (key == "track_blocks_per_cu") {
    if (value < 1 || value > 64) return fail(ctx, ATTPC_E_INVALID, "track_blocks_per_cu must be 1..64");
    ctx->opt_track_blocks_per_cu = (int)value;
  } else if (key == "track_species_major") {
    ctx->opt_track_species_major = value != 0;
  } else if (key == "first_batch_chunks") {
    if (value < 0 || value > MAX_SLOTS) return fail(ctx, ATTPC_E_INVALID, "first_batch_chunks must be 0..8");
    ctx->opt_first_batch_chunks = (int)value;
  } else if (key == "scatter_merge") {
    if (value < -1 || value > 1) return fail(ctx, ATTPC_E_INVALID, "scatter_merge must be -1, 0 or 1");
    ctx->opt_merge = (int)value;
  } else if (key == "trace_pack_workgroups") {
    if (value < 0 || value > 65536) return fail(ctx, ATTPC_E_INVALID, "trace_pack_workgroups must be 0..65536");
    ctx->opt_trace_pack_workgroups = (int)value;
  } else if (key == "track_workgroups") {
    if (value < 0 || value > 65536) return fail(ctx, ATTPC_E_INVALID, "track_workgroups must be 0..65536");
    ctx->opt_track_workgroups = (int)value;
  } else if (key == "chunk_events") {
    return attpc_set_chunk_events(ctx, (int32_t)value);
  } else {
    return fail(ctx, ATTPC_E_INVALID, "unknown option '%s'", name);
  }
  return ATTPC_OK;
}

int32_t attpc_host_alloc(attpc_ctx* ctx, uint64_t bytes, void** out) {
  if (!ctx || !out) return ATTPC_E_INVALID;
  *out = nullptr;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  void* p = nullptr;
  HIP_TRY(ctx, hipHostMalloc(&p, std::max<uint64_t>(bytes, 1), hipHostMallocDefault));
  ctx->host_allocs.push_back(p);
  *out = p;
  return ATTPC_OK;
}

int32_t attpc_host_free(attpc_ctx* ctx, void* ptr) {
  if (!ctx) return ATTPC_E_INVALID;
  if (!ptr) return ATTPC_OK;
  auto it = std::find(ctx->host_allocs.begin(), ctx->host_allocs.end(), ptr);
  if (it == ctx->host_allocs.end()) return fail(ctx, ATTPC_E_INVALID, "attpc_host_free: not an attpc_host_alloc pointer of this context");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream_c));
  HIP_TRY(ctx, hipHostFree(ptr));
  ctx->host_allocs.erase(it);
  return ATTPC_OK;
}

int32_t attpc_unpack_rows(const void* packed, int64_t n_rows, double* points, int64_t* labels, int32_t n_threads) {
  if (n_rows < 0 || (n_rows > 0 && (!packed || !points || !labels))) return ATTPC_E_INVALID;
  unpack_rows(static_cast<const PackedRow*>(packed), n_rows, points, labels, n_threads);
  return ATTPC_OK;
}

int32_t attpc_unpack_rows8(const void* packed, int64_t n_rows, const int64_t* offsets, int64_t n_events, uint64_t seed,
                           uint64_t first_event, double* points, int64_t* labels, int32_t n_threads) {
  if (n_rows < 0 || n_events < 0 || !offsets || (n_rows > 0 && (!packed || !points || !labels))) return ATTPC_E_INVALID;
  if (offsets[n_events] != offsets[0] + n_rows) return ATTPC_E_INVALID;
  unpack_rows8(static_cast<const unsigned long long*>(packed), n_rows, offsets, n_events, seed, first_event, points, labels, n_threads);
  return ATTPC_OK;
}

int32_t attpc_unpack_spyral_rows(const void* packed, int64_t n_rows, const double* pad_centers, const double* pad_sizes,
                                 int32_t n_pads, double r_max, int32_t windows_edge, int32_t micromegas_edge, double length,
                                 double* rows, int64_t* labels, int32_t n_threads) {
  if (n_rows < 0 || n_pads < 1 || (n_rows > 0 && (!packed || !pad_centers || !pad_sizes || !rows || !labels))) return ATTPC_E_INVALID;
  SpyralHostTables t;
  t.centers = pad_centers;
  t.sizes = pad_sizes;
  t.n_pads = n_pads;
  t.r_max = r_max;
  t.window_edge = (double)windows_edge;
  t.mm_edge = (double)micromegas_edge;
  t.length = length;
  unpack_spyral_rows(static_cast<const SpyralPacked*>(packed), n_rows, t, rows, labels, n_threads);
  return ATTPC_OK;
}

int32_t attpc_sync(attpc_ctx* ctx) {
  if (!ctx) return ATTPC_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return sync_all(ctx);
}

int32_t attpc_kin_configure(attpc_ctx* ctx, const attpc_kin_desc* d) {
  if (!ctx || !d) return ATTPC_E_INVALID;
  if (d->n_steps < 1 || d->n_steps > ATTPC_MAX_STEPS) return fail(ctx, ATTPC_E_INVALID, "n_steps=%d", d->n_steps);
  if (d->sample_limit < 1) return fail(ctx, ATTPC_E_INVALID, "sample_limit=%d", d->sample_limit);
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  { int32_t rc0 = drop_prefetch(ctx); if (rc0) return rc0; }  // (nothing is in flight: it only forgets the batch)
  ctx->kin_allocs.clear();
  ctx->kin_ready = false;
  ctx->rows_per_event = ctx->segs_per_event = ctx->blocks_per_track = 0.0;  // another workload: size estimates start over
  attpc_kin_desc k = *d;
  int32_t rc;
  for (int s = 0; s < d->n_steps; ++s) {
    attpc_excitation_desc& e = k.excitation[s];
    if (e.kind == ATTPC_EX_TABLE) {
      if (e.table_len < 2 || !e.table_x || !e.table_cdf) return fail(ctx, ATTPC_E_INVALID, "excitation %d: bad table", s);
      if ((rc = upload(ctx, ctx->kin_allocs, d->excitation[s].table_x, (size_t)e.table_len, &e.table_x))) return rc;
      if ((rc = upload(ctx, ctx->kin_allocs, d->excitation[s].table_cdf, (size_t)e.table_len, &e.table_cdf))) return rc;
    } else if (e.kind != ATTPC_EX_GAUSSIAN && e.kind != ATTPC_EX_UNIFORM) {
      return fail(ctx, ATTPC_E_INVALID, "excitation %d: unknown kind %d", s, e.kind);
    } else {
      e.table_x = e.table_cdf = nullptr;
    }
    attpc_polar_desc& p = k.polar[s];
    if (p.kind == ATTPC_POLAR_ARBITRARY) {
      if (p.table_len < 1 || !p.angles || !p.cdf) return fail(ctx, ATTPC_E_INVALID, "polar %d: bad table", s);
      if ((rc = upload(ctx, ctx->kin_allocs, d->polar[s].angles, (size_t)p.table_len, &p.angles))) return rc;
      if ((rc = upload(ctx, ctx->kin_allocs, d->polar[s].cdf, (size_t)p.table_len, &p.cdf))) return rc;
    } else if (p.kind != ATTPC_POLAR_UNIFORM) {
      return fail(ctx, ATTPC_E_INVALID, "polar %d: unknown kind %d", s, p.kind);
    } else {
      p.angles = p.cdf = nullptr;
    }
  }
  if (k.has_target) {
    if (k.eloss_len < 1 || !d->eloss) return fail(ctx, ATTPC_E_INVALID, "target without energy-loss table");
    if ((rc = upload(ctx, ctx->kin_allocs, d->eloss, (size_t)k.eloss_len, &k.eloss))) return rc;
  } else {
    k.eloss = nullptr;
    k.eloss_len = 0;
  }
  ctx->kin = k;
  ctx->kin_ready = true;
  return ATTPC_OK;
}

int32_t attpc_kin_run(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events, double* p4,
                      double* vertex, int32_t* status, uint32_t* attempts) {
  if (!ctx) return ATTPC_E_INVALID;
  if (!ctx->kin_ready) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_kin_configure has not been called");
  if (validate_id_range(ctx, first_event, n_events)) return ATTPC_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int n_rows = kin_rows(ctx);
  // buffers of its own (ctx->scratch): the track sets are sized by the largest track batch met so far
  // (max_batch_events), and a kinematics-only call of 4 chunks per launch must not set that mark for every later
  // detector run; and nothing a failed earlier run may have left queued on any stream is overtaken
  int32_t rc = sync_all(ctx);
  if (rc) return rc;
  const uint64_t chunk = (uint64_t)std::max(1, ctx->chunk_events) * 4;
  const size_t cap = (size_t)std::min<uint64_t>(chunk, std::max<uint64_t>(n_events, 1));
  double* d_p4 = stage<double>(ctx, 4, cap * n_rows * 4, rc);
  double* d_vertex = stage<double>(ctx, 5, cap * 3, rc);
  int32_t* d_status = stage<int32_t>(ctx, 6, cap, rc);
  uint32_t* d_attempts = stage<uint32_t>(ctx, 7, cap, rc);
  if (rc) return rc;
  for (uint64_t done = 0; done < n_events; done += chunk) {
    const uint32_t n = (uint32_t)std::min<uint64_t>(chunk, n_events - done);
    launch_kin_run(ctx->stream, ctx->kin, seed, first_event + done, n, d_p4, d_vertex, d_status, d_attempts);
    HIP_TRY(ctx, hipGetLastError());
    if (p4 && (rc = stage_out(ctx, p4 + done * n_rows * 4, d_p4, (size_t)n * n_rows * 4))) return rc;
    if (vertex && (rc = stage_out(ctx, vertex + done * 3, d_vertex, (size_t)n * 3))) return rc;
    if (status && (rc = stage_out(ctx, status + done, d_status, (size_t)n))) return rc;
    if (attempts && (rc = stage_out(ctx, attempts + done, d_attempts, (size_t)n))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return ATTPC_OK;
}

int32_t attpc_kin_calculate(attpc_ctx* ctx, uint64_t n, const double* beam_energy, const double* ex,
                            const double* polar, const double* azim, double* p4, int32_t* status) {
  if (!ctx || !beam_energy || !ex || !polar || !azim || !p4 || !status) return ATTPC_E_INVALID;
  if (!ctx->kin_ready) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_kin_configure has not been called");
  if (n == 0) return ATTPC_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int ns = ctx->kin.n_steps, n_rows = kin_rows(ctx);
  int32_t rc = ATTPC_OK;
  const double* d_beam = stage_in(ctx, 0, beam_energy, n, rc);
  const double* d_ex = stage_in(ctx, 1, ex, n * ns, rc);
  const double* d_polar = stage_in(ctx, 2, polar, n * ns, rc);
  const double* d_azim = stage_in(ctx, 3, azim, n * ns, rc);
  double* d_p4 = stage<double>(ctx, 4, n * n_rows * 4, rc);
  int32_t* d_status = stage<int32_t>(ctx, 5, n, rc);
  if (rc) return rc;
  launch_kin_calculate(ctx->stream, ctx->kin, (uint32_t)n, d_beam, d_ex, d_polar, d_azim, d_p4, d_status);
  HIP_TRY(ctx, hipGetLastError());
  if ((rc = stage_out(ctx, p4, d_p4, n * n_rows * 4))) return rc;
  if ((rc = stage_out(ctx, status, d_status, n))) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return ATTPC_OK;
}

int32_t attpc_decay_calculate(attpc_ctx* ctx, uint64_t n, const double* parent, double mass_1, double mass_2,
                              const double* ex, const double* polar, const double* azim, double* out,
                              int32_t* status) {
  if (!ctx || !parent || !ex || !polar || !azim || !out || !status) return ATTPC_E_INVALID;
  if (n == 0) return ATTPC_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc = ATTPC_OK;
  const double* d_parent = stage_in(ctx, 0, parent, n * 4, rc);
  const double* d_ex = stage_in(ctx, 1, ex, n, rc);
  const double* d_polar = stage_in(ctx, 2, polar, n, rc);
  const double* d_azim = stage_in(ctx, 3, azim, n, rc);
  double* d_out = stage<double>(ctx, 4, n * 8, rc);
  int32_t* d_status = stage<int32_t>(ctx, 5, n, rc);
  if (rc) return rc;
  launch_decay_calculate(ctx->stream, (uint32_t)n, d_parent, mass_1, mass_2, d_ex, d_polar, d_azim, d_out, d_status);
  HIP_TRY(ctx, hipGetLastError());
  if ((rc = stage_out(ctx, out, d_out, n * 8))) return rc;
  if ((rc = stage_out(ctx, status, d_status, n))) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return ATTPC_OK;
}

int32_t attpc_det_configure(attpc_ctx* ctx, const attpc_det_desc* d) {
  if (!ctx || !d) return ATTPC_E_INVALID;
  if (d->n_species < 1 || d->n_species > ATTPC_MAX_SPECIES) return fail(ctx, ATTPC_E_INVALID, "n_species=%d", d->n_species);
  if ((size_t)d->n_species * ATTPC_DEDX_NODES * sizeof(double) > 150 * 1024)
    return fail(ctx, ATTPC_E_INVALID, "stopping-power tables of %d species do not fit LDS (max 13)", d->n_species);
  if (!d->pad_lut || d->lut_n < 1) return fail(ctx, ATTPC_E_INVALID, "missing pad look-up table");
  // (the limit is also what scatter.hip's lut_offsets() rests on: it multiplies an index <= lut_n by the byte pitch
  //  2 (lut_n + 1) as two 16-bit factors -- v_mad_u32_u16 -- which holds up to lut_n = 32 766; do not raise it past that)
  static_assert(2 * (32000 + 1) < 65536, "the LUT's byte pitch is a 16-bit factor in scatter.hip");
  if (d->lut_n > 32000) return fail(ctx, ATTPC_E_INVALID, "pad look-up table larger than 32000 x 32000 (indices are staged as 16 bit)");
  if (d->windows_edge <= d->micromegas_edge) return fail(ctx, ATTPC_E_INVALID, "windows_edge <= micromegas_edge");
  if (!(d->length > 0.0) || !(d->w_value > 0.0)) return fail(ctx, ATTPC_E_INVALID, "length and w_value must be > 0");
  {  // the scatter key packs the pad into 14 bits (tb << 14 | pad): ids outside [-1, 16383] would corrupt the
     // time bucket bits; the reference only treats -1 as "no pad" (transporter.py:162,237)
    const size_t cells = (size_t)d->lut_n * (size_t)d->lut_n;
    for (size_t i = 0; i < cells; ++i)
      if (d->pad_lut[i] < -1 || d->pad_lut[i] >= LONE_PADS)
        return fail(ctx, ATTPC_E_INVALID, "pad look-up table holds pad id %d at cell %zu: ids must be in [-1, %d]", (int)d->pad_lut[i], i, LONE_PADS - 1);
  }
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  { int32_t rc0 = drop_prefetch(ctx); if (rc0) return rc0; }  // (nothing is in flight: it only forgets the batch)
  ctx->det_allocs.clear();
  ctx->det_ready = false;
  ctx->rows_per_event = ctx->segs_per_event = ctx->blocks_per_track = 0.0;  // size estimates start over
  ctx->prefer_big = false;
  ctx->prefer_wide = false;
  DetDev dv{};
  dv.length = d->length; dv.efield = d->efield; dv.bfield = d->bfield; dv.density = d->density;
  dv.diffusion = d->diffusion; dv.fano_factor = d->fano_factor; dv.w_value = d->w_value;
  dv.dv = d->length / (double)(d->windows_edge - d->micromegas_edge);  // parameters.py:172-174
  dv.inv_dv = 1.0 / dv.dv;
  dv.mm_edge = (double)d->micromegas_edge;
  dv.mpgd_gain = d->mpgd_gain;
  dv.lut_n = d->lut_n; dv.lut_lo = d->lut_lo;
  dv.n_species = d->n_species; dv.ode_substeps = d->ode_substeps > 0 ? d->ode_substeps : 1;
  dv.longitudinal_diffusion = d->longitudinal_diffusion > 0.0 ? d->longitudinal_diffusion : 0.0;
  for (int s = 0; s < ATTPC_LONG_STEPS; ++s) dv.long_weights[s] = d->long_weights[s];
  dv.mc_diffusion = d->mc_diffusion != 0 ? 1 : 0;
  dv.mpgd_gain32 = (int32_t)d->mpgd_gain;
  if (!(d->path_step >= 0.0) || !(d->path_step < 1.0e300)) return fail(ctx, ATTPC_E_INVALID, "path_step must be >= 0 and finite");
  dv.path_step = d->path_step;
  if (dv.mc_diffusion && (d->mpgd_gain < 1 || d->mpgd_gain > 0x7fffffff)) return fail(ctx, ATTPC_E_INVALID, "mc_diffusion needs 1 <= mpgd_gain < 2^31");
  int32_t rc;
  {  // device copy: [x][y] as given, padded with one extra row and column of -1 (index lut_n = "off
     // the pad plane").  The scatter kernel's lanes are mesh lines of constant y that step through x
     // together, so one gather instruction reads neighbouring y of the same x row -- 1-2 cache lines
     // per sample instead of one per lane.
    const size_t n = (size_t)d->lut_n, pitch = n + 1;
    std::vector<int16_t> lut_t(pitch * pitch, (int16_t)-1);
    for (size_t ix = 0; ix < n; ++ix)
      for (size_t iy = 0; iy < n; ++iy) lut_t[ix * pitch + iy] = d->pad_lut[ix * n + iy];
    if ((rc = upload(ctx, ctx->det_allocs, lut_t.data(), pitch * pitch, &dv.pad_lut))) return rc;
  }
  std::vector<double> tabs((size_t)d->n_species * ATTPC_DEDX_NODES);
  for (int s = 0; s < d->n_species; ++s) {
    if (!d->species[s].dedx) return fail(ctx, ATTPC_E_INVALID, "species %d: missing dE/dx table", s);
    if (!(d->species[s].mass > 0.0)) return fail(ctx, ATTPC_E_INVALID, "species %d: mass must be > 0", s);
    std::memcpy(tabs.data() + (size_t)s * ATTPC_DEDX_NODES, d->species[s].dedx, ATTPC_DEDX_NODES * sizeof(double));
    dv.mass[s] = d->species[s].mass;
    dv.Z[s] = d->species[s].Z;
  }
  if ((rc = upload(ctx, ctx->det_allocs, tabs.data(), tabs.size(), &dv.dedx))) return rc;
  ctx->det = dv;
  ctx->det_ready = true;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream_t_own));  // (sync_all above covered stream_t, whichever it was)
  pick_track_stream(ctx);
  return ATTPC_OK;
}

// ---- track straggling (tracks.hip, straggle_host.hpp; the contract is in include/attpc_engine.h) ----
int32_t attpc_det_configure_straggling(attpc_ctx* ctx, const attpc_straggle_desc* d) {
  if (!ctx) return ATTPC_E_INVALID;
  if (d) {
    const char* wrong = straggle_desc_error(*d);
    if (wrong) return fail(ctx, ATTPC_E_INVALID, "attpc_det_configure_straggling: %s", wrong);
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // (a track batch queued ahead of the next call was integrated under the old settings)
  { int32_t rc0 = drop_prefetch(ctx); if (rc0) return rc0; }
  ctx->straggle_on = d != nullptr;
  ctx->straggle = d ? *d : attpc_straggle_desc{};
  return ATTPC_OK;
}

// ---- drift distortion (distort.hip, distort_host.hpp; the contract is in include/attpc_engine.h) ----
// the tables of a checked desc on the device, owned by `owner` (a NULL table stays NULL: zeros)
static int32_t upload_distort_map(attpc_ctx* ctx, DevAllocs& owner, const attpc_distort_desc& d, DistortMap* map) {
  const size_t nodes = (size_t)d.n_rho * (size_t)d.n_tau;
  DistortMap m{d.rho_step, d.tau_step, d.tb_origin, d.n_rho, d.n_tau, nullptr, nullptr, nullptr};
  int32_t rc;
  if (d.radial && (rc = upload(ctx, owner, d.radial, nodes, &m.radial))) return rc;
  if (d.azimuthal && (rc = upload(ctx, owner, d.azimuthal, nodes, &m.azimuthal))) return rc;
  if (d.time && (rc = upload(ctx, owner, d.time, nodes, &m.time))) return rc;
  *map = m;
  return ATTPC_OK;
}

int32_t attpc_det_configure_distortion(attpc_ctx* ctx, const attpc_distort_desc* d) {
  if (!ctx) return ATTPC_E_INVALID;
  if (d) {
    const char* wrong = distort_desc_error(*d);
    if (wrong) return fail(ctx, ATTPC_E_INVALID, "attpc_det_configure_distortion: %s", wrong);
  }
  // nothing in flight may read the old tables (and a track batch queued ahead was made under the old map)
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  { int32_t rc0 = drop_prefetch(ctx); if (rc0) return rc0; }
  ctx->distort_on = false;
  ctx->distort = DistortMap{};
  ctx->distort_allocs.clear();
  if (!d || distort_desc_is_off(*d)) return ATTPC_OK;
  int32_t rc = upload_distort_map(ctx, ctx->distort_allocs, *d, &ctx->distort);
  if (rc) {
    ctx->distort_allocs.clear();
    return rc;
  }
  ctx->distort_on = true;
  return ATTPC_OK;
}

int32_t attpc_samples_distort(attpc_ctx* ctx, int64_t n, const double* samples, const attpc_distort_desc* d, double* out) {
  if (!ctx || !d || n < 0 || n > ((int64_t)1 << 36) || (n > 0 && (!samples || !out))) return ATTPC_E_INVALID;
  const char* wrong = distort_desc_error(*d);
  if (wrong) return fail(ctx, ATTPC_E_INVALID, "attpc_samples_distort: %s", wrong);
  if (n == 0) return ATTPC_OK;
  if (distort_desc_is_off(*d)) {
    if (out != samples) std::memcpy(out, samples, (size_t)n * 4 * sizeof(double));
    return ATTPC_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // the array as chains of consecutive arena blocks: "tracks" of MAX_BLOCKS_PER_TRACK blocks, the last one shorter
  constexpr int64_t CHAIN = (int64_t)MAX_BLOCKS_PER_TRACK * ARENA_BLK;
  const size_t n_blocks = (size_t)((n + ARENA_BLK - 1) / ARENA_BLK);
  const uint32_t n_tracks = (uint32_t)((n + CHAIN - 1) / CHAIN);
  std::vector<int32_t> table((size_t)n_tracks * MAX_BLOCKS_PER_TRACK, -1), counts(n_tracks);
  for (size_t b = 0; b < n_blocks; ++b) table[b] = (int32_t)b;
  for (uint32_t t = 0; t < n_tracks; ++t) counts[t] = (int32_t)std::min<int64_t>(CHAIN, n - (int64_t)t * CHAIN);
  DevAllocs tables;  // this call's own copy of the map, freed when it returns
  DistortArgs a{};
  int32_t rc = upload_distort_map(ctx, tables, *d, &a.map);
  // (the arena's tail past record n is read by the kernel's whole-block loads and never stored)
  double* d_arena = stage<double>(ctx, 0, n_blocks * ARENA_BLK * 4, rc);
  const int32_t* d_table = stage_in(ctx, 1, table.data(), table.size(), rc);
  const int32_t* d_counts = stage_in(ctx, 2, counts.data(), counts.size(), rc);
  uint32_t* d_ctrl = stage<uint32_t>(ctx, 3, TRK_WORDS, rc);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(d_arena, samples, (size_t)n * 4 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(d_ctrl, 0, TRK_WORDS * sizeof(uint32_t), ctx->stream));
  a.buf = TrackBuffers{d_arena, const_cast<int32_t*>(d_table), const_cast<int32_t*>(d_counts), nullptr, d_ctrl,
                       (uint32_t)std::min<size_t>(n_blocks, 0xFFFFFFFFu)};
  a.n_tracks = n_tracks;
  uint32_t limit = (uint32_t)ctx->n_cus * (uint32_t)ctx->opt_track_blocks_per_cu;
  if (ctx->opt_track_workgroups > 0) limit = std::min<uint32_t>(limit, (uint32_t)ctx->opt_track_workgroups);
  launch_distort(distort_workgroups(n_tracks, limit), ctx->stream, a);
  HIP_TRY(ctx, hipGetLastError());
  if ((rc = stage_out(ctx, out, d_arena, (size_t)n * 4))) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (before `tables` and the host vectors go)
  return ATTPC_OK;
}

// ---- drift correction (undistort.hip, undistort_host.hpp; the contract is in include/attpc_engine.h) ----
int32_t attpc_trace_configure_correction(attpc_ctx* ctx, const attpc_undistort_desc* d) {
  if (!ctx) return ATTPC_E_INVALID;
  if (d)
    if (const char* wrong = undistort_desc_error(*d)) return fail(ctx, ATTPC_E_INVALID, "attpc_trace_configure_correction: %s", wrong);
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }  // nothing in flight may read the old tables
  ctx->correction_on = false;
  ctx->correction = UndistortSettings{};
  ctx->correction_allocs.clear();
  if (!d || distort_desc_is_off(d->map)) return ATTPC_OK;
  DistortMap map{};
  const int32_t rc = upload_distort_map(ctx, ctx->correction_allocs, d->map, &map);
  if (rc) {
    ctx->correction_allocs.clear();
    return rc;
  }
  ctx->correction = undistort_settings(*d, map);
  ctx->correction_on = true;
  return ATTPC_OK;
}

int32_t attpc_correction_last(attpc_ctx* ctx, attpc_undistort_info* info) {
  if (!ctx || !info) return ATTPC_E_INVALID;
  if (!ctx->correction_call)
    return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_correction_last: the drift correction was off for the last trace-row call");
  *info = ctx->last_correction;
  return ATTPC_OK;
}

int32_t attpc_rows_undistort(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows, const int64_t* labels,
                             const attpc_undistort_desc* d, double* out_rows, int64_t* out_labels, int64_t* order,
                             attpc_undistort_info* info) {
  if (!ctx || !d || !info || n_events < 0) return ATTPC_E_INVALID;
  if (const char* wrong = undistort_desc_error(*d)) return fail(ctx, ATTPC_E_INVALID, "attpc_rows_undistort: %s", wrong);
  if (const ArgError bad = csr_error(__func__, n_events, offsets)) return refuse(ctx, bad);
  if (n_events > 0 && offsets[n_events] > offsets[0] && (!rows || !out_rows)) return ATTPC_E_INVALID;
  if ((labels == nullptr) != (out_labels == nullptr)) return ATTPC_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc;
  if ((rc = sync_all(ctx))) return rc;
  *info = attpc_undistort_info{};
  if (n_events == 0) return ATTPC_OK;
  DevAllocs tables;  // this call's own copy of the map, freed when it returns
  DistortMap map{};
  if ((rc = upload_distort_map(ctx, tables, d->map, &map))) return rc;
  UndistortArgs a{};
  a.s = undistort_settings(*d, map);
  unsigned long long* d_counts = stage<unsigned long long>(ctx, 6, 4, rc);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, 4 * sizeof(unsigned long long), ctx->stream));
  a.counts = d_counts;
  std::vector<int64_t> start;
  for (int64_t e0 = 0, e1; e0 < n_events; e0 = e1) {
    e1 = chunk_end(offsets, n_events, e0, CHUNK_ROWS, CHUNK_EVENTS);
    const size_t m = (size_t)(e1 - e0), n_rows = (size_t)(offsets[e1] - offsets[e0]), cap = std::max<size_t>(n_rows, 1);
    if (!n_rows) continue;  // (empty events: nothing to count)
    stage_rows(ctx, offsets, e0, e1, rows, labels, &start, rc, true).into(a);
    a.out_rows = stage<double>(ctx, 3, cap * 8, rc);
    a.out_labels = labels ? stage<int64_t>(ctx, 4, cap, rc) : nullptr;
    a.order = order ? stage<int64_t>(ctx, 5, cap, rc) : nullptr;
    a.order_base = offsets[e0];
    if (!rc) rc = ensure(ctx, ctx->uc_xyt, cap * 3 * sizeof(double));
    if (!rc) rc = ensure(ctx, ctx->sort_idx, cap * sizeof(uint32_t));
    if (!rc) rc = ensure(ctx, ctx->sort_key, cap * sizeof(double));
    if (rc) return rc;
    a.xyt = static_cast<double*>(ctx->uc_xyt.p);
    a.sort_idx = static_cast<uint32_t*>(ctx->sort_idx.p);
    a.sort_key = static_cast<double*>(ctx->sort_key.p);
    launch_undistort(ctx->stream, (uint32_t)m, a);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = stage_out(ctx, out_rows + offsets[e0] * 8, a.out_rows, n_rows * 8))) return rc;
    if (labels && (rc = stage_out(ctx, out_labels + offsets[e0], a.out_labels, n_rows))) return rc;
    if (order && (rc = stage_out(ctx, order + offsets[e0], a.order, n_rows))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (before the staging is filled again)
  }
  unsigned long long counts[4] = {0ull, 0ull, 0ull, 0ull};
  HIP_TRY(ctx, hipMemcpyAsync(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (before `tables` and the host vector go)
  *info = attpc_undistort_info{(int64_t)counts[0], (int64_t)counts[1], (int64_t)counts[2], (int64_t)counts[3]};
  return ATTPC_OK;
}

int32_t attpc_det_run(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                      const attpc_event_layout* layout, const double* p4, const double* vertex,
                      attpc_cloud_out* out, attpc_run_stats* stats) {
  return run_entry(__func__, ctx, seed, first_event, n_events, layout, RunSource{false, p4, vertex}, RunSink{},
                   RunOut{OutMode::cloud, out}, stats);
}

int32_t attpc_det_run_spyral(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                             const attpc_event_layout* layout, const double* p4, const double* vertex,
                             attpc_cloud_out* out, attpc_run_stats* stats) {
  return run_entry(__func__, ctx, seed, first_event, n_events, layout, RunSource{false, p4, vertex}, RunSink{},
                   RunOut{OutMode::spyral, out}, stats);
}

int32_t attpc_sim_run(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                      const attpc_event_layout* layout, double* p4, double* vertex, int32_t* kin_status,
                      attpc_cloud_out* out, attpc_run_stats* stats) {
  return run_entry(__func__, ctx, seed, first_event, n_events, layout, RunSource{true}, RunSink{p4, vertex, kin_status},
                   RunOut{OutMode::cloud, out}, stats);
}

int32_t attpc_sim_run_spyral(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                             const attpc_event_layout* layout, double* p4, double* vertex, int32_t* kin_status,
                             attpc_cloud_out* out, attpc_run_stats* stats) {
  return run_entry(__func__, ctx, seed, first_event, n_events, layout, RunSource{true}, RunSink{p4, vertex, kin_status},
                   RunOut{OutMode::spyral, out}, stats);
}

// ---- digitised pad traces (traces.hip; the contract is in include/attpc_engine.h) ----
int32_t attpc_trace_configure(attpc_ctx* ctx, const attpc_trace_desc* d) {
  if (!ctx || !d || !d->response) return ATTPC_E_INVALID;
  if (d->offset < 0 || d->offset >= ATTPC_NUM_TB) return fail(ctx, ATTPC_E_INVALID, "trace offset %d outside 0..511", d->offset);
  if (std::isnan(d->adc_threshold)) return fail(ctx, ATTPC_E_INVALID, "trace threshold is NaN");
  for (int j = 0; j < ATTPC_NUM_TB; ++j)
    if (!(d->response[j] >= 0.0) || std::isinf(d->response[j]))
      return fail(ctx, ATTPC_E_INVALID, "response[%d] = %g: the trace response must be finite and >= 0", j, d->response[j]);
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  ctx->trace_allocs.clear();
  ctx->trace_ready = false;
  TraceDev tr{};
  int32_t rc;
  if ((rc = upload(ctx, ctx->trace_allocs, d->response, (size_t)ATTPC_NUM_TB, &tr.response))) return rc;
  tr.threshold = d->adc_threshold;
  tr.offset = d->offset;
  ctx->trace = tr;
  ctx->trace_ready = true;
  return ATTPC_OK;
}

int32_t attpc_trace_configure_noise(attpc_ctx* ctx, const attpc_trace_noise_desc* d) {
  if (!ctx) return ATTPC_E_INVALID;
  if (d) {
    if (d->n_levels < 0 || d->n_levels > ATTPC_MAX_NOISE_LEVELS)
      return fail(ctx, ATTPC_E_INVALID, "noise table of %d levels: 0 .. %d", d->n_levels, ATTPC_MAX_NOISE_LEVELS);
    if (d->min_level < -4095 || d->min_level > 4095)
      return fail(ctx, ATTPC_E_INVALID, "noise min_level %d outside -4095 .. 4095", d->min_level);
    if (d->n_levels > 1 && !d->cdf) return fail(ctx, ATTPC_E_INVALID, "noise table of %d levels without a cdf", d->n_levels);
    for (int k = 1; k < d->n_levels - 1; ++k)
      if (d->cdf[k] < d->cdf[k - 1]) return fail(ctx, ATTPC_E_INVALID, "noise cdf decreases at entry %d", k);
    if (d->pedestals)
      for (int p = 0; p < ATTPC_NUM_PADS; ++p)
        if (d->pedestals[p] < 0 || d->pedestals[p] > 4095)
          return fail(ctx, ATTPC_E_INVALID, "pedestal of pad %d is %d, outside 0 .. 4095", p, (int)d->pedestals[p]);
    if (d->stream >= 0x80000000u) return fail(ctx, ATTPC_E_INVALID, "noise stream %u >= 2^31", d->stream);
  }
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  ctx->noise_allocs.clear();
  ctx->noise_on = false;
  ctx->noise = TraceNoiseDev{};
  ctx->noise_cdf.clear();
  if (!d || (d->n_levels == 0 && !d->pedestals)) return ATTPC_OK;  // the noiseless contract
  const NoiseTable table = noise_table(d->n_levels, d->cdf);
  ctx->noise_cdf.assign(table.cdf.begin(), table.cdf.begin() + std::max(d->n_levels - 1, 0));
  TraceNoiseDev nz{};
  int32_t rc;
  if ((rc = upload(ctx, ctx->noise_allocs, table.cdf.data(), table.cdf.size(), &nz.cdf))) return rc;
  if ((rc = upload(ctx, ctx->noise_allocs, table.guide.data(), table.guide.size(), &nz.guide))) return rc;
  if (d->pedestals && (rc = upload(ctx, ctx->noise_allocs, d->pedestals, (size_t)ATTPC_NUM_PADS, &nz.pedestals))) return rc;
  nz.n_levels = d->n_levels;
  nz.min_level = d->min_level;
  nz.domain = DOMAIN_TRACE_NOISE | d->stream;
  ctx->noise = nz;
  ctx->noise_on = true;
  return ATTPC_OK;
}

int32_t attpc_trace_configure_readout(attpc_ctx* ctx, const attpc_trace_readout_desc* d) {
  if (!ctx) return ATTPC_E_INVALID;
  if (d && d->mode != ATTPC_READOUT_HIT && d->mode != ATTPC_READOUT_PARTIAL && d->mode != ATTPC_READOUT_FULL)
    return fail(ctx, ATTPC_E_INVALID, "trace readout mode %d: 0 (hit), 1 (partial) or 2 (full)", d->mode);
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  ctx->readout_allocs.clear();
  ctx->readout_mode = ATTPC_READOUT_HIT;
  ctx->readout_pads = 0;
  ctx->readout_channels = nullptr;
  ctx->trace_rows_per_event = 0.0;  // the kept rows of another readout say nothing about this one
  if (!d || d->mode == ATTPC_READOUT_HIT) return ATTPC_OK;
  std::vector<uint32_t> words(TR_MAP_WORDS, 0u);
  int64_t count = 0;
  for (int p = 0; p < ATTPC_NUM_PADS; ++p)
    if (!d->channels || d->channels[p]) {
      words[p >> 5] |= 1u << (p & 31);
      ++count;
    }
  int32_t rc;
  if ((rc = upload(ctx, ctx->readout_allocs, words.data(), words.size(), &ctx->readout_channels))) return rc;
  ctx->readout_pads = count;
  ctx->readout_mode = d->mode;
  return ATTPC_OK;
}

int32_t attpc_sim_run_traces(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                             const attpc_event_layout* layout, double* p4, double* vertex, int32_t* kin_status,
                             attpc_trace_out* out, attpc_run_stats* stats) {
  return run_entry(__func__, ctx, seed, first_event, n_events, layout, RunSource{true}, RunSink{p4, vertex, kin_status},
                   RunOut{OutMode::traces, nullptr, out}, stats);
}

int32_t attpc_det_run_traces(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                             const attpc_event_layout* layout, const double* p4, const double* vertex,
                             attpc_trace_out* out, attpc_run_stats* stats) {
  return run_entry(__func__, ctx, seed, first_event, n_events, layout, RunSource{false, p4, vertex}, RunSink{},
                   RunOut{OutMode::traces, nullptr, out}, stats);
}

int32_t attpc_traces(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* points, const int64_t* labels,
                     attpc_trace_out* out) {
  return attpc_traces_at(ctx, 0, 0, n_events, offsets, points, labels, out);
}

namespace {
// The checks of a host cloud in CSR form (attpc_traces_at, attpc_trace_rows_at, attpc_gain_rows; `what` names the entry
// point): n_events, offsets and the contract's rows -- integer pad in range, 0 <= tau < 512, finite electrons >= 0, a
// (pad, t) of their own within the event.
int32_t check_host_cloud(attpc_ctx* ctx, const char* what, int64_t n_events, const int64_t* offsets, const double* points,
                         bool has_labels) {
  if (const ArgError bad = csr_error(what, n_events, offsets, CSR_CLOUD)) return refuse(ctx, bad);
  const int64_t rows = n_events ? offsets[n_events] - offsets[0] : 0;
  if (rows > 0 && (!points || !has_labels)) return ATTPC_E_INVALID;
  if (rows > (int64_t)UINT32_MAX) return fail(ctx, ATTPC_E_INVALID, "%s takes fewer than 2^32 rows per call", what);
  if (const ArgError bad = cloud_rows_error(n_events, offsets, points, true)) return refuse(ctx, bad);
  return ATTPC_OK;
}

// attpc_traces_at and attpc_trace_rows_at: the checks of the host cloud, then its events through trace_host_events
// into `o`.
int32_t host_cloud_run(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, int64_t n_events, const int64_t* offsets,
                       const double* points, const int64_t* labels, RunOut& o) {
  if (const ArgError bad = csr_count_error("attpc_traces", n_events, offsets)) return refuse(ctx, bad);
  if (validate_id_range(ctx, first_event, (uint64_t)n_events)) return ATTPC_E_INVALID;
  if (!ctx->trace_ready) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_trace_configure has not been called");
  const uint32_t n = (uint32_t)n_events;
  if (int32_t bad = check_host_cloud(ctx, "attpc_traces", n_events, offsets, points, labels != nullptr)) return bad;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc;
  if ((rc = drop_prefetch(ctx))) return rc;
  if ((rc = sync_all(ctx))) return rc;
  if ((rc = reset_trace_sums(ctx, o.mode))) return rc;
  if ((rc = begin_record_streams(ctx, o.mode == OutMode::trace_rows, n, nullptr, -1))) return rc;  // (no layout: the trigger's records alone)
  const double keep = ctx->trace_rows_per_event;  // a host cloud says nothing about the configured workload
  rc = trace_host_events(ctx, o, 0, n, offsets, points, labels, seed, first_event);
  ctx->trace_rows_per_event = keep;
  return rc;
}
}  // namespace

int32_t attpc_traces_at(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, int64_t n_events, const int64_t* offsets,
                        const double* points, const int64_t* labels, attpc_trace_out* out) {
  if (!ctx || !out) return ATTPC_E_INVALID;
  RunOut o{OutMode::traces, nullptr, out};
  int32_t rc;
  if ((rc = host_cloud_run(ctx, seed, first_event, n_events, offsets, points, labels, o))) return rc;
  if ((rc = read_trace_sums(ctx, o))) return rc;
  return run_status(ctx, attpc_run_stats{}, nullptr, o);
}

// ---- packed pad traces (trace_pack.hip, trace_pack_host.cpp; the contract is in include/attpc_engine.h) ----
namespace {
// The row arrays of an attpc_trace_packed_out as the attpc_trace_out the run loop fills (no samples), and the way back.
struct PackedView {
  attpc_trace_out t{};
  explicit PackedView(attpc_trace_packed_out* p) {
    t.capacity = p->capacity;
    t.offsets = p->offsets;
    t.pads = p->pads;
    t.labels = p->labels;
    t.event_points = p->event_points;
    p->n_rows = p->n_bytes = 0;
    if (p->row_start) p->row_start[0] = 0;
  }
  RunOut run(attpc_trace_packed_out* p) {
    RunOut o{OutMode::traces, nullptr, &t};
    o.tpacked = p;
    return o;
  }
  int32_t finish(attpc_trace_packed_out* p, int32_t rc) {
    p->n_rows = t.n_rows;
    p->sample_checksum = t.sample_checksum;
    p->pad_checksum = t.pad_checksum;
    return rc;
  }
};
bool bad_packed_out(const attpc_trace_packed_out* out) { return !out || out->byte_capacity < 0; }
}  // namespace

int32_t attpc_sim_run_traces_packed(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                    const attpc_event_layout* layout, double* p4, double* vertex, int32_t* kin_status,
                                    attpc_trace_packed_out* out, attpc_run_stats* stats) {
  if (!ctx) return ATTPC_E_INVALID;
  if (bad_packed_out(out)) return fail(ctx, ATTPC_E_INVALID, "%s needs an attpc_trace_packed_out", __func__);
  PackedView view(out);
  return view.finish(out, run_entry(__func__, ctx, seed, first_event, n_events, layout, RunSource{true},
                                    RunSink{p4, vertex, kin_status}, view.run(out), stats));
}

int32_t attpc_det_run_traces_packed(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                    const attpc_event_layout* layout, const double* p4, const double* vertex,
                                    attpc_trace_packed_out* out, attpc_run_stats* stats) {
  if (!ctx) return ATTPC_E_INVALID;
  if (bad_packed_out(out)) return fail(ctx, ATTPC_E_INVALID, "%s needs an attpc_trace_packed_out", __func__);
  PackedView view(out);
  return view.finish(out, run_entry(__func__, ctx, seed, first_event, n_events, layout, RunSource{false, p4, vertex}, RunSink{},
                                    view.run(out), stats));
}

int32_t attpc_traces_packed_at(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, int64_t n_events, const int64_t* offsets,
                               const double* points, const int64_t* labels, attpc_trace_packed_out* out) {
  if (!ctx || bad_packed_out(out)) return ATTPC_E_INVALID;
  PackedView view(out);
  RunOut o = view.run(out);
  int32_t rc;
  if ((rc = host_cloud_run(ctx, seed, first_event, n_events, offsets, points, labels, o))) return rc;
  if ((rc = read_trace_sums(ctx, o))) return rc;
  return view.finish(out, run_status(ctx, attpc_run_stats{}, nullptr, o));
}

int32_t attpc_trace_pack(attpc_ctx* ctx, int64_t n_rows, const int16_t* samples, int64_t* row_start, uint8_t* bytes,
                         int64_t byte_capacity, int64_t* n_bytes) {
  if (!ctx || n_rows < 0 || byte_capacity < 0) return ATTPC_E_INVALID;
  if (n_bytes) *n_bytes = 0;
  if (row_start) row_start[0] = 0;
  if (n_rows == 0) return ATTPC_OK;
  if (!samples) return ATTPC_E_INVALID;
  if (const ArgError bad = sample_error(samples, 0, n_rows)) return refuse(ctx, bad);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc;
  if ((rc = drop_prefetch(ctx))) return rc;
  if ((rc = sync_all(ctx))) return rc;
  AsmSet& as = ctx->aset[0];
  constexpr int64_t CHUNK = 16384;  // rows: 16 MiB of samples on the device
  int64_t total = 0;
  for (int64_t first = 0; first < n_rows; first += CHUNK) {
    const int64_t n = std::min(CHUNK, n_rows - first);  // (the first chunk is the largest: the slot grows once)
    const int16_t* d_samples = stage_in(ctx, 0, samples + first * ATTPC_NUM_TB, (size_t)n * ATTPC_NUM_TB, rc);
    if (rc) return rc;
    if ((rc = enqueue_trace_pack_size(ctx, as, n, d_samples))) return rc;
    HIP_TRY(ctx, hipEventSynchronize(as.counted));
    const int64_t chunk_bytes = as.h_tp_total[0];
    if ((rc = enqueue_trace_pack_write(ctx, as, n, d_samples, chunk_bytes, total))) return rc;
    if (row_start)
      HIP_TRY(ctx, hipMemcpyAsync(row_start + first + 1, static_cast<const int64_t*>(as.tp_row_start.p) + 1, (size_t)n * sizeof(int64_t),
                                  hipMemcpyDeviceToHost, ctx->stream));
    if (bytes && total + chunk_bytes <= byte_capacity)
      HIP_TRY(ctx, hipMemcpyAsync(bytes + total, as.tp_bytes.p, (size_t)chunk_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    total += chunk_bytes;
  }
  if (n_bytes) *n_bytes = total;
  if (bytes && total > byte_capacity)
    return fail(ctx, ATTPC_E_CAPACITY, "packed rows need %lld bytes, capacity %lld", (long long)total, (long long)byte_capacity);
  return ATTPC_OK;
}

int32_t attpc_trace_pack_host(int64_t n_rows, const int16_t* samples, int64_t* row_start, uint8_t* bytes, int64_t byte_capacity,
                              int64_t* n_bytes) {
  return trace_pack_host(n_rows, samples, row_start, bytes, byte_capacity, n_bytes);
}

int32_t attpc_trace_unpack(const uint8_t* bytes, int64_t n_bytes, const int64_t* row_start, int64_t n_rows, int16_t* samples,
                           int32_t n_threads) {
  return trace_unpack_host(bytes, n_bytes, row_start, n_rows, samples, n_threads);
}

// ---- micromegas gain of the traces (gain.hip; the contract is in include/attpc_engine.h) ----
int32_t attpc_trace_configure_gain(attpc_ctx* ctx, const attpc_trace_gain_desc* d) {
  if (!ctx) return ATTPC_E_INVALID;
  if (d) {
    if (!(d->rel_variance >= 0.0 && d->rel_variance <= 1.0))
      return fail(ctx, ATTPC_E_INVALID, "gain rel_variance %g: 0 .. 1", d->rel_variance);
    if (d->pad_gain)
      for (int p = 0; p < ATTPC_NUM_PADS; ++p)
        if (!(d->pad_gain[p] >= 0.0) || std::isinf(d->pad_gain[p]))
          return fail(ctx, ATTPC_E_INVALID, "gain of pad %d is %g: finite and >= 0", p, d->pad_gain[p]);
    if (d->rel_variance > 0.0) {
      if (!d->quantiles) return fail(ctx, ATTPC_E_INVALID, "gain rel_variance %g without a quantile table", d->rel_variance);
      for (int k = 0; k < ATTPC_GAIN_KNOTS; ++k) {
        if (!std::isfinite(d->quantiles[k])) return fail(ctx, ATTPC_E_INVALID, "gain quantile %d is not finite", k);
        if (k && d->quantiles[k] < d->quantiles[k - 1]) return fail(ctx, ATTPC_E_INVALID, "gain quantiles decrease at entry %d", k);
      }
    }
    if (d->stream >= 0x40000000u) return fail(ctx, ATTPC_E_INVALID, "gain stream %u >= 2^30", d->stream);
  }
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  ctx->gain_allocs.clear();
  ctx->gain_on = false;
  ctx->gain = GainDev{};
  if (!d || (d->rel_variance == 0.0 && !d->pad_gain)) return ATTPC_OK;  // q'' = q: the contract without the stage
  GainDev g{};
  int32_t rc;
  if (d->rel_variance > 0.0 && (rc = upload(ctx, ctx->gain_allocs, d->quantiles, (size_t)ATTPC_GAIN_KNOTS, &g.quantiles))) return rc;
  if (d->pad_gain && (rc = upload(ctx, ctx->gain_allocs, d->pad_gain, (size_t)ATTPC_NUM_PADS, &g.pad_gain))) return rc;
  g.c = d->rel_variance / 9.0;
  g.domain = DOMAIN_TRACE_GAIN | d->stream;
  ctx->gain = g;
  ctx->gain_on = true;
  return ATTPC_OK;
}

int32_t attpc_gain_rows(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, int64_t n_events, const int64_t* offsets,
                        const double* points, double* gained) {
  if (!ctx) return ATTPC_E_INVALID;
  if (int32_t bad = check_host_cloud(ctx, "attpc_gain_rows", n_events, offsets, points, true)) return bad;
  if (validate_id_range(ctx, first_event, (uint64_t)n_events)) return ATTPC_E_INVALID;
  const int64_t all = n_events ? offsets[n_events] - offsets[0] : 0;
  if (all == 0) return ATTPC_OK;
  if (!gained) return ATTPC_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc;
  if ((rc = sync_all(ctx))) return rc;
  // chunks of whole events: about 4 Mi rows (96 MiB of points) and at most 1 Mi events, one event at the least
  constexpr int64_t CHUNK_ROWS = 4ll << 20, CHUNK_EVENTS = 1ll << 20;
  std::vector<int64_t> start;
  for (int64_t e0 = 0, e1; e0 < n_events; e0 = e1) {
    e1 = chunk_end(offsets, n_events, e0, CHUNK_ROWS, CHUNK_EVENTS);
    const int64_t lo = offsets[e0], rows = offsets[e1] - lo, m = e1 - e0;
    if (rows > 0) {
      chunk_starts(offsets, e0, e1, &start);
      const int64_t* d_start = stage_in(ctx, 0, start.data(), start.size(), rc);
      const double* d_points = stage_in(ctx, 1, points + 3 * lo, (size_t)rows * 3, rc);
      double* d_gained = stage<double>(ctx, 2, (size_t)rows, rc);
      if (rc) return rc;
      launch_gain(ctx->stream, ctx->gain, seed, (uint32_t)m, first_event + (uint64_t)e0, d_start, d_points, d_gained);
      HIP_TRY(ctx, hipGetLastError());
      if ((rc = stage_out(ctx, gained + lo, d_gained, (size_t)rows))) return rc;
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
  }
  return ATTPC_OK;
}

// ---- common-mode noise of the traces (traces.hip; the contract is in include/attpc_engine.h) ----
int32_t attpc_trace_configure_common_mode(attpc_ctx* ctx, const attpc_trace_common_desc* d) {
  if (!ctx) return ATTPC_E_INVALID;
  int n_groups = 0;
  if (d) {
    if (d->n_levels < 0 || d->n_levels > ATTPC_MAX_NOISE_LEVELS)
      return fail(ctx, ATTPC_E_INVALID, "common-mode table of %d levels: 0 .. %d", d->n_levels, ATTPC_MAX_NOISE_LEVELS);
    if (d->min_level < -4095 || d->min_level > 4095)
      return fail(ctx, ATTPC_E_INVALID, "common-mode min_level %d outside -4095 .. 4095", d->min_level);
    if (d->n_levels > 1 && !d->cdf) return fail(ctx, ATTPC_E_INVALID, "common-mode table of %d levels without a cdf", d->n_levels);
    for (int k = 1; k < d->n_levels - 1; ++k)
      if (d->cdf[k] < d->cdf[k - 1]) return fail(ctx, ATTPC_E_INVALID, "common-mode cdf decreases at entry %d", k);
    if (d->stream >= 0x20000000u) return fail(ctx, ATTPC_E_INVALID, "common-mode stream %u >= 2^29", d->stream);
    n_groups = d->groups ? 0 : 1;
    if (d->groups)
      for (int p = 0; p < ATTPC_NUM_PADS; ++p)
        if (d->groups[p] != 255) n_groups = std::max(n_groups, (int)d->groups[p] + 1);
  }
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  ctx->common_allocs.clear();
  ctx->common_on = false;
  ctx->common_table = TraceNoiseDev{};
  ctx->common_groups = nullptr;
  ctx->common_n_groups = 0;
  if (!d || d->n_levels == 0 || n_groups == 0) return ATTPC_OK;  // the contract without the stage
  const NoiseTable table = noise_table(d->n_levels, d->cdf);
  TraceNoiseDev t{};
  const uint8_t* groups = nullptr;
  int32_t rc;
  if ((rc = upload(ctx, ctx->common_allocs, table.cdf.data(), table.cdf.size(), &t.cdf))) return rc;
  if ((rc = upload(ctx, ctx->common_allocs, table.guide.data(), table.guide.size(), &t.guide))) return rc;
  if (d->groups && (rc = upload(ctx, ctx->common_allocs, d->groups, (size_t)ATTPC_NUM_PADS, &groups))) return rc;
  t.n_levels = d->n_levels;
  t.min_level = d->min_level;
  t.domain = DOMAIN_TRACE_COMMON | d->stream;
  ctx->common_table = t;
  ctx->common_groups = groups;
  ctx->common_n_groups = n_groups;
  ctx->common_on = true;
  return ATTPC_OK;
}

int32_t attpc_common_mode_rows(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, int64_t n_events, int16_t* out) {
  if (!ctx || n_events < 0) return ATTPC_E_INVALID;
  if (n_events > (int64_t)INT32_MAX) return fail(ctx, ATTPC_E_INVALID, "attpc_common_mode_rows takes at most 2^31 - 1 events per call");
  if (validate_id_range(ctx, first_event, (uint64_t)n_events)) return ATTPC_E_INVALID;
  if (!ctx->common_on) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_trace_configure_common_mode has not turned the stage on");
  if (n_events == 0) return ATTPC_OK;
  if (!out) return ATTPC_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc;
  if ((rc = sync_all(ctx))) return rc;
  const size_t per_event = (size_t)ctx->common_n_groups * ATTPC_NUM_TB;  // values
  const int64_t step = (int64_t)common_chunk_events(ctx);
  std::vector<int16_t> lanes;
  for (int64_t e0 = 0; e0 < n_events; e0 += step) {
    const int64_t m = std::min(step, n_events - e0);
    const size_t count = (size_t)m * per_event;
    int16_t* d_lanes = stage<int16_t>(ctx, 0, count, rc);
    if (rc) return rc;
    launch_common_mode(ctx->stream, ctx->common_table, seed, (uint32_t)m, first_event + (uint64_t)e0,
                       (uint32_t)ctx->common_n_groups, d_lanes);
    HIP_TRY(ctx, hipGetLastError());
    lanes.resize(count);
    if ((rc = stage_out(ctx, lanes.data(), d_lanes, count))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // the device keeps a group's values in lane order (sample l + 64 s at 8 l + s): sample order for the caller
    int16_t* dst = out + (size_t)e0 * per_event;
    for (size_t item = 0; item < (size_t)m * (size_t)ctx->common_n_groups; ++item)
      for (int l = 0; l < 64; ++l)
        for (int k = 0; k < 8; ++k) dst[item * ATTPC_NUM_TB + l + 64 * k] = lanes[item * ATTPC_NUM_TB + 8 * l + k];
  }
  return ATTPC_OK;
}

// ---- event and track summaries (summary.hip; the contract is in include/attpc_engine.h) ----
int32_t attpc_summary_configure(attpc_ctx* ctx, const attpc_summary_desc* d) {
  if (!ctx) return ATTPC_E_INVALID;
  if (d) {
    if (d->min_electrons < 0) return fail(ctx, ATTPC_E_INVALID, "summary min_electrons %lld < 0", (long long)d->min_electrons);
    if (d->n_pads < ATTPC_NUM_PADS) return fail(ctx, ATTPC_E_INVALID, "summary geometry of %d pads, the clouds name pads up to %d", d->n_pads, ATTPC_NUM_PADS - 1);
    if (!d->pad_centers) return fail(ctx, ATTPC_E_INVALID, "summary geometry without pad centres");
  }
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  ctx->summary_allocs.clear();
  ctx->summary_on = false;
  ctx->summary_centers = nullptr;
  if (!d) return ATTPC_OK;
  int32_t rc;
  if ((rc = upload(ctx, ctx->summary_allocs, d->pad_centers, (size_t)d->n_pads * 2, &ctx->summary_centers))) return rc;
  ctx->summary_min = (double)d->min_electrons;
  ctx->summary_on = true;
  return ATTPC_OK;
}

int32_t attpc_sim_run_summary(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                              const attpc_event_layout* layout, double* p4, double* vertex, int32_t* kin_status,
                              attpc_summary_out* out, attpc_run_stats* stats) {
  RunOut o{OutMode::summary};
  o.summary = out;
  return run_entry(__func__, ctx, seed, first_event, n_events, layout, RunSource{true}, RunSink{p4, vertex, kin_status}, o, stats);
}

int32_t attpc_det_run_summary(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                              const attpc_event_layout* layout, const double* p4, const double* vertex,
                              attpc_summary_out* out, attpc_run_stats* stats) {
  RunOut o{OutMode::summary};
  o.summary = out;
  return run_entry(__func__, ctx, seed, first_event, n_events, layout, RunSource{false, p4, vertex}, RunSink{}, o, stats);
}

namespace {
// attpc_cloud_summary, and with `passed` attpc_cloud_select: the records of a host cloud (to `out`, if given), then the
// configured selection on them.  With `maps` attpc_cloud_maps: the selection only if the maps ask for it (`passed` is
// then who contributed), and the cloud's maps behind it.
int32_t host_cloud_records(const char* name, attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* points,
                           const int64_t* labels, const attpc_event_layout* layout, const attpc_summary_out* out, uint8_t* passed,
                           attpc_maps_out* maps = nullptr) {
  if (const ArgError bad = csr_count_error(name, n_events, offsets)) return refuse(ctx, bad);
  if (!ctx->summary_on) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_summary_configure has not been called");
  if (maps && !ctx->maps_on) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_maps_configure has not been called");
  const bool predicate = maps ? ctx->maps.selected != 0 : passed != nullptr;
  if (predicate && !ctx->select_on) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_select_configure has not been called");
  int32_t rc;
  if ((rc = validate_layout(ctx, layout, false))) return rc;
  if (predicate && (rc = validate_select_mask(ctx, name, layout->n_sim))) return rc;
  const uint32_t n = (uint32_t)n_events;
  if (const ArgError bad = csr_error(name, n_events, offsets)) return refuse(ctx, bad);
  const int64_t first = n ? offsets[0] : 0;
  const int64_t rows = n ? offsets[n] - first : 0;
  if (rows > 0 && (!points || !labels)) return ATTPC_E_INVALID;
  if (const ArgError bad = cloud_rows_error(n_events, offsets, points, false)) return refuse(ctx, bad);  // the contract's rows
  if (maps) {
    // (one workgroup may meet every row: the 32-bit cells of maps_event_kernel)
    if (rows > (int64_t)UINT32_MAX) return fail(ctx, ATTPC_E_INVALID, "%s takes at most 2^32 - 1 rows per call", name);
    maps->n_events = maps->n_hit = 0;
    if (n == 0) {  // the maps of no event
      if (maps->pad_events) std::fill(maps->pad_events, maps->pad_events + ATTPC_NUM_PADS, 0ull);
      if (maps->pad_charge) std::fill(maps->pad_charge, maps->pad_charge + ATTPC_NUM_PADS, 0ll);
      if (maps->tb_events) std::fill(maps->tb_events, maps->tb_events + ATTPC_NUM_TB, 0ull);
      if (maps->tb_rows) std::fill(maps->tb_rows, maps->tb_rows + ATTPC_NUM_TB, 0ull);
      if (maps->tb_charge) std::fill(maps->tb_charge, maps->tb_charge + ATTPC_NUM_TB, 0ll);
    }
  }
  if (n == 0) return ATTPC_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if ((rc = drop_prefetch(ctx))) return rc;
  if ((rc = sync_all(ctx))) return rc;
  // the cloud on the device as the kernels of the fused path find it: rows in place, one segment per event
  AsmSet& as = ctx->aset[0];
  const size_t cap = (size_t)std::max<int64_t>(rows, 1);
  if ((rc = ensure(ctx, as.points, cap * 3 * sizeof(double)))) return rc;
  if ((rc = ensure(ctx, as.labels, cap * sizeof(int64_t)))) return rc;
  if ((rc = ensure(ctx, ctx->sm_host_segs, (size_t)n * sizeof(Segment)))) return rc;
  if ((rc = ensure(ctx, ctx->sm_host_ctrl, CTRL_WORDS * sizeof(unsigned long long)))) return rc;
  if ((rc = ensure_summary_records(ctx, n, layout->n_sim))) return rc;
  std::vector<Segment> segs(n);
  for (uint32_t e = 0; e < n; ++e) segs[e] = Segment{(int32_t)e, (int32_t)(offsets[e + 1] - offsets[e]), offsets[e] - first, 0};
  unsigned long long words[CTRL_WORDS] = {};  // of a launch that wrote these rows and segments and did not run out of room
  words[CTRL_ROW_CURSOR] = (unsigned long long)rows, words[CTRL_SEG_CURSOR] = (unsigned long long)n;
  HIP_TRY(ctx, hipMemcpy(ctx->sm_host_segs.p, segs.data(), segs.size() * sizeof(Segment), hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(ctx->sm_host_ctrl.p, words, sizeof words, hipMemcpyHostToDevice));
  if (rows > 0) {
    HIP_TRY(ctx, hipMemcpy(as.points.p, points + 3 * first, (size_t)rows * 3 * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(as.labels.p, labels + first, (size_t)rows * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  const ChunkView chunk{static_cast<const double*>(as.points.p), static_cast<const int64_t*>(as.labels.p),
                        static_cast<const Segment*>(ctx->sm_host_segs.p), static_cast<const unsigned long long*>(ctx->sm_host_ctrl.p),
                        (int64_t)n, rows};
  if ((rc = enqueue_summary(ctx, chunk, *layout, nullptr, 0, n))) return rc;
  if (out && (rc = copy_summary(ctx, out, 0, n, layout->n_sim))) return rc;
  if (predicate) {
    if ((rc = ensure_idle(ctx, ctx->sel_passed, n))) return rc;
    if ((rc = enqueue_select(ctx, chunk.ctrl, layout->n_sim, 0, n, nullptr))) return rc;
    if (passed) HIP_TRY(ctx, hipMemcpyAsync(passed, ctx->sel_passed.p, n, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (maps) {  // the cloud as one accepted chunk of slot 0
    std::vector<uint8_t> in(predicate ? n : 0);
    if (predicate) HIP_TRY(ctx, hipMemcpyAsync(in.data(), ctx->sel_passed.p, n, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = begin_maps_call(ctx))) return rc;
    if ((rc = enqueue_maps(ctx, chunk, 0, *layout, 0, n, predicate))) return rc;
    if ((rc = enqueue_maps_fold(ctx, 0))) return rc;
    return read_maps_total(ctx, maps, n, predicate ? in.data() : nullptr, passed);
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return ATTPC_OK;
}
}  // namespace

int32_t attpc_cloud_summary(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* points,
                            const int64_t* labels, const attpc_event_layout* layout, attpc_summary_out* out) {
  if (!ctx || !out) return ATTPC_E_INVALID;
  return host_cloud_records(__func__, ctx, n_events, offsets, points, labels, layout, out, nullptr);
}

// ---- selected delivery (select.hip; the contract is in include/attpc_engine.h) ----
int32_t attpc_select_configure(attpc_ctx* ctx, const attpc_select_desc* d) {
  if (!ctx) return ATTPC_E_INVALID;
  if (d) {
    const struct { const char* name; double lo, hi; } f64[] = {{"track_rho2_max", d->track_rho2_max_lo, d->track_rho2_max_hi},
                                                               {"track_end_tb", d->track_end_tb_lo, d->track_end_tb_hi},
                                                               {"track_end_rho2", d->track_end_rho2_lo, d->track_end_rho2_hi}};
    for (const auto& r : f64)
      if (std::isnan(r.lo) || std::isnan(r.hi) || r.lo > r.hi) return fail(ctx, ATTPC_E_INVALID, "selection: %s range [%g, %g]", r.name, r.lo, r.hi);
    const struct { const char* name; uint32_t lo, hi; } u32[] = {
        {"n_kept", d->n_kept_lo, d->n_kept_hi}, {"n_pads", d->n_pads_lo, d->n_pads_hi}, {"tb_span", d->tb_span_lo, d->tb_span_hi},
        {"track_n_kept", d->track_n_kept_lo, d->track_n_kept_hi}, {"track_n_pads", d->track_n_pads_lo, d->track_n_pads_hi},
        {"track_n_samples", d->track_n_samples_lo, d->track_n_samples_hi}};
    for (const auto& r : u32)
      if (r.lo > r.hi) return fail(ctx, ATTPC_E_INVALID, "selection: %s range [%u, %u]", r.name, r.lo, r.hi);
    if (d->charge_lo > d->charge_hi) return fail(ctx, ATTPC_E_INVALID, "selection: charge range [%lld, %lld]", (long long)d->charge_lo, (long long)d->charge_hi);
    if (d->track_mask >> ATTPC_MAX_SIM) return fail(ctx, ATTPC_E_INVALID, "selection: track_mask 0x%x has bits at or above %d", d->track_mask, ATTPC_MAX_SIM);
    if (d->min_tracks > (uint32_t)__builtin_popcount(d->track_mask))
      return fail(ctx, ATTPC_E_INVALID, "selection: min_tracks %u above the %d masked positions", d->min_tracks, __builtin_popcount(d->track_mask));
  }
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  ctx->select_on = d != nullptr;
  if (d) ctx->select = *d;
  return ATTPC_OK;
}

namespace {
// The two selected entry points: `out` seen as the cloud output of its kind and as a summary output.
int32_t run_selected(const char* name, attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                     const attpc_event_layout* layout, const RunSource& src, const RunSink& sink, attpc_select_out* out,
                     attpc_run_stats* stats) {
  if (!ctx) return ATTPC_E_INVALID;
  if (!out) return fail(ctx, ATTPC_E_INVALID, "%s needs an attpc_select_out", name);
  if (out->kind != ATTPC_SELECT_CLOUD && out->kind != ATTPC_SELECT_SPYRAL) return fail(ctx, ATTPC_E_INVALID, "%s: kind %d", name, out->kind);
  out->n_passed = out->n_rows = 0;
  attpc_cloud_out cloud{out->capacity, out->offsets, out->points, out->labels, out->event_points};
  attpc_summary_out records{out->events, out->tracks};
  RunOut o{out->kind == ATTPC_SELECT_SPYRAL ? OutMode::spyral : OutMode::cloud, &cloud};
  o.summary = &records;
  o.select = out;
  return run_entry(name, ctx, seed, first_event, n_events, layout, src, sink, o, stats);
}
}  // namespace

int32_t attpc_sim_run_selected(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                               const attpc_event_layout* layout, double* p4, double* vertex, int32_t* kin_status,
                               attpc_select_out* out, attpc_run_stats* stats) {
  return run_selected(__func__, ctx, seed, first_event, n_events, layout, RunSource{true}, RunSink{p4, vertex, kin_status}, out, stats);
}

int32_t attpc_det_run_selected(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                               const attpc_event_layout* layout, const double* p4, const double* vertex,
                               attpc_select_out* out, attpc_run_stats* stats) {
  return run_selected(__func__, ctx, seed, first_event, n_events, layout, RunSource{false, p4, vertex}, RunSink{}, out, stats);
}

int32_t attpc_cloud_select(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* points,
                           const int64_t* labels, const attpc_event_layout* layout, attpc_summary_out* out, uint8_t* passed) {
  if (!ctx || !passed) return ATTPC_E_INVALID;
  return host_cloud_records(__func__, ctx, n_events, offsets, points, labels, layout, out, passed);
}

// ---- run maps (maps.hip; the contract is in include/attpc_engine.h) ----
int32_t attpc_maps_configure(attpc_ctx* ctx, const attpc_maps_desc* d) {
  if (!ctx) return ATTPC_E_INVALID;
  if (d) {
    if (d->track_mask == 0u) return fail(ctx, ATTPC_E_INVALID, "run maps: empty track_mask");
    if (d->track_mask >> (ATTPC_MAX_SIM + 1)) return fail(ctx, ATTPC_E_INVALID, "run maps: track_mask 0x%x has bits above %d", d->track_mask, ATTPC_MAX_SIM);
    if (d->selected > 1u) return fail(ctx, ATTPC_E_INVALID, "run maps: selected %u", d->selected);
  }
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  ctx->maps_on = d != nullptr;
  if (d) ctx->maps = *d;
  return ATTPC_OK;
}

namespace {
// The two maps entry points: the summary run with the maps on top.
int32_t run_maps(const char* name, attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                 const attpc_event_layout* layout, const RunSource& src, const RunSink& sink, attpc_summary_out* records,
                 uint8_t* passed, attpc_maps_out* maps, attpc_run_stats* stats) {
  if (!ctx) return ATTPC_E_INVALID;
  if (!maps) return fail(ctx, ATTPC_E_INVALID, "%s needs an attpc_maps_out", name);
  maps->n_events = maps->n_hit = 0;
  attpc_summary_out none{nullptr, nullptr};
  RunOut o{OutMode::summary};
  o.summary = records ? records : &none;
  o.maps = maps;
  o.maps_passed = passed;
  return run_entry(name, ctx, seed, first_event, n_events, layout, src, sink, o, stats);
}
}  // namespace

int32_t attpc_sim_run_maps(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                           const attpc_event_layout* layout, double* p4, double* vertex, int32_t* kin_status,
                           attpc_summary_out* records, uint8_t* passed, attpc_maps_out* maps, attpc_run_stats* stats) {
  return run_maps(__func__, ctx, seed, first_event, n_events, layout, RunSource{true}, RunSink{p4, vertex, kin_status}, records,
                  passed, maps, stats);
}

int32_t attpc_det_run_maps(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                           const attpc_event_layout* layout, const double* p4, const double* vertex,
                           attpc_summary_out* records, uint8_t* passed, attpc_maps_out* maps, attpc_run_stats* stats) {
  return run_maps(__func__, ctx, seed, first_event, n_events, layout, RunSource{false, p4, vertex}, RunSink{}, records, passed,
                  maps, stats);
}

int32_t attpc_cloud_maps(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* points,
                         const int64_t* labels, const attpc_event_layout* layout, attpc_summary_out* records,
                         uint8_t* passed, attpc_maps_out* maps) {
  if (!ctx || !maps) return ATTPC_E_INVALID;
  return host_cloud_records(__func__, ctx, n_events, offsets, points, labels, layout, records, passed, maps);
}

// ---- trace rows (peaks.hip; the contract is in include/attpc_engine.h) ----
int32_t attpc_trace_configure_peaks(attpc_ctx* ctx, const attpc_peak_desc* d) {
  if (!ctx) return ATTPC_E_INVALID;
  if (d) {
    if (!(d->separation >= 1.0)) return fail(ctx, ATTPC_E_INVALID, "peak separation %g: >= 1", d->separation);
    if (!(d->prominence >= 0.0)) return fail(ctx, ATTPC_E_INVALID, "peak prominence %g: >= 0", d->prominence);
    if (!(d->min_width >= 0.0 && d->max_width >= d->min_width))
      return fail(ctx, ATTPC_E_INVALID, "peak widths %g .. %g: 0 <= min_width <= max_width", d->min_width, d->max_width);
    if (!(d->rel_height > 0.0 && d->rel_height <= 1.0)) return fail(ctx, ATTPC_E_INVALID, "peak rel_height %g: in (0, 1]", d->rel_height);
    if (std::isnan(d->threshold)) return fail(ctx, ATTPC_E_INVALID, "peak threshold is NaN");
  }
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  ctx->peaks_on = false;
  if (!d) return ATTPC_OK;
  PeakDev pk{};
  pk.distance = (int32_t)std::min(std::ceil(d->separation), (double)ATTPC_NUM_TB);  // (512 samples apart: one candidate a row)
  pk.prominence = d->prominence;
  pk.min_width = d->min_width;
  pk.max_width = d->max_width;
  pk.rel_height = d->rel_height;
  pk.threshold = d->threshold;
  ctx->peaks = pk;
  ctx->peaks_on = true;
  return ATTPC_OK;
}

// ---- Fourier baseline of the trace rows (baseline.hip; the contract is in include/attpc_engine.h) ----
int32_t attpc_trace_configure_baseline(attpc_ctx* ctx, const attpc_baseline_desc* d) {
  if (!ctx) return ATTPC_E_INVALID;
  if (d && !(std::isfinite(d->window_scale) && d->window_scale > 0.0))
    return fail(ctx, ATTPC_E_INVALID, "baseline window_scale %g: finite and > 0", d->window_scale);
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  ctx->baseline_on = false;
  if (!d) return ATTPC_OK;
  int32_t rc;
  if ((rc = upload_baseline_tables(ctx, ctx->bl_filter, d->window_scale))) return rc;
  ctx->baseline_on = true;
  return ATTPC_OK;
}

int32_t attpc_trace_baseline(attpc_ctx* ctx, int64_t n_rows, const int16_t* samples, double window_scale, int16_t* y,
                             double* baseline) {
  if (!ctx || n_rows < 0) return ATTPC_E_INVALID;
  if (!(std::isfinite(window_scale) && window_scale > 0.0))
    return fail(ctx, ATTPC_E_INVALID, "baseline window_scale %g: finite and > 0", window_scale);
  if (n_rows == 0) return ATTPC_OK;
  if (!samples || !y) return ATTPC_E_INVALID;
  if (const ArgError bad = sample_error(samples, 0, n_rows)) return refuse(ctx, bad);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc;
  if ((rc = sync_all(ctx))) return rc;
  if (ctx->bl_op_scale != window_scale) {
    ctx->bl_op_scale = 0.0;
    if ((rc = upload_baseline_tables(ctx, ctx->bl_op_filter, window_scale))) return rc;
    ctx->bl_op_scale = window_scale;
  }
  constexpr int64_t CHUNK = 16384;  // rows: 16 MiB of samples, 16 MiB of y and 64 MiB of baseline on the device
  for (int64_t first = 0; first < n_rows; first += CHUNK) {
    const size_t n = (size_t)std::min(CHUNK, n_rows - first) * ATTPC_NUM_TB;  // samples (the first chunk is the largest)
    const int16_t* d_samples = stage_in(ctx, 0, samples + first * ATTPC_NUM_TB, n, rc);
    int16_t* d_y = stage<int16_t>(ctx, 1, n, rc);
    double* d_baseline = baseline ? stage<double>(ctx, 2, n, rc) : nullptr;
    if (rc) return rc;
    launch_baseline(ctx->stream, (uint32_t)(n / ATTPC_NUM_TB), d_samples, static_cast<const double2*>(ctx->bl_twiddle.p),
                    static_cast<const double*>(ctx->bl_op_filter.p), d_y, d_baseline);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = stage_out(ctx, y + first * ATTPC_NUM_TB, d_y, n))) return rc;
    if (baseline && (rc = stage_out(ctx, baseline + first * ATTPC_NUM_TB, d_baseline, n))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return ATTPC_OK;
}

// ---- multiplicity trigger on the pad traces (trigger.hip; the contract is in include/attpc_engine.h) ----
namespace {
// The checks of an attpc_trigger_desc, and its group map on the device in `buf`: the kernel's parameters in *tg.
int32_t upload_trigger(attpc_ctx* ctx, const attpc_trigger_desc* d, DevBuf& buf, TriggerDev* tg) {
  if (d->threshold < 0 || d->threshold > 4095) return fail(ctx, ATTPC_E_INVALID, "trigger threshold %d: 0 .. 4095", d->threshold);
  if (d->window < 1 || d->window > ATTPC_NUM_TB) return fail(ctx, ATTPC_E_INVALID, "trigger window %d: 1 .. %d", d->window, ATTPC_NUM_TB);
  if (d->group_multiplicity < 1) return fail(ctx, ATTPC_E_INVALID, "trigger group_multiplicity %d: >= 1", d->group_multiplicity);
  if (d->min_groups < 1 || d->min_groups > ATTPC_MAX_TRIGGER_GROUPS)
    return fail(ctx, ATTPC_E_INVALID, "trigger min_groups %d: 1 .. %d", d->min_groups, ATTPC_MAX_TRIGGER_GROUPS);
  if (d->gate != 0 && d->gate != 1) return fail(ctx, ATTPC_E_INVALID, "trigger gate %d: 0 or 1", d->gate);
  if (d->reserved != 0) return fail(ctx, ATTPC_E_INVALID, "trigger reserved %d: 0", d->reserved);
  int n_groups = 1;
  if (d->groups)
    for (int p = 0; p < ATTPC_NUM_PADS; ++p) {
      const int g = d->groups[p];
      if (g >= ATTPC_MAX_TRIGGER_GROUPS && g != 255)
        return fail(ctx, ATTPC_E_INVALID, "trigger group %d of pad %d: below %d, or 255", g, p, ATTPC_MAX_TRIGGER_GROUPS);
      if (g != 255) n_groups = std::max(n_groups, g + 1);
    }
  int32_t rc = begin_configure(ctx);
  if (rc) return rc;
  if (d->groups) {
    if ((rc = ensure(ctx, buf, ATTPC_NUM_PADS))) return rc;
    HIP_TRY(ctx, hipMemcpy(buf.p, d->groups, ATTPC_NUM_PADS, hipMemcpyHostToDevice));
  }
  *tg = TriggerDev{d->threshold, d->window, d->group_multiplicity, d->min_groups, n_groups,
                   d->groups ? static_cast<const uint8_t*>(buf.p) : nullptr};
  return ATTPC_OK;
}
}  // namespace

int32_t attpc_trace_configure_trigger(attpc_ctx* ctx, const attpc_trigger_desc* d) {
  if (!ctx) return ATTPC_E_INVALID;
  if (!d) {
    { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
    ctx->trigger_on = false;
    return ATTPC_OK;
  }
  TriggerDev tg{};
  const int32_t rc = upload_trigger(ctx, d, ctx->tg_groups, &tg);  // (a refused desc leaves the configured one as it is:
  if (rc) return rc;                                               //  the checks come before the upload)
  ctx->trigger = tg;
  ctx->trigger_gate = d->gate != 0;
  ctx->trigger_on = true;
  return ATTPC_OK;
}

int32_t attpc_trigger_last(attpc_ctx* ctx, int64_t first, int64_t count, attpc_trigger_record* out) {
  if (!ctx) return ATTPC_E_INVALID;
  return records_last(ctx, ctx->tg_records, __func__, "no trigger was configured for the last trace call", first, count, out);
}

int32_t attpc_trigger_rows(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const int32_t* pads, const int16_t* samples,
                           const int16_t* pedestals, const attpc_trigger_desc* d, attpc_trigger_record* out) {
  if (!ctx || n_events < 0 || !d) return ATTPC_E_INVALID;
  if (n_events > 0 && !out) return ATTPC_E_INVALID;
  if (const ArgError bad = csr_error(__func__, n_events, offsets)) return refuse(ctx, bad);
  const int64_t r0 = n_events ? offsets[0] : 0, r1 = n_events ? offsets[n_events] : 0;
  if (r1 > r0 && (!pads || !samples)) return ATTPC_E_INVALID;
  for (int64_t r = r0; r < r1; ++r)
    if (pads[r] < 0 || pads[r] >= ATTPC_NUM_PADS)
      return fail(ctx, ATTPC_E_INVALID, "row %lld: pad %d outside 0 .. %d", (long long)r, pads[r], ATTPC_NUM_PADS - 1);
  if (const ArgError bad = sample_error(samples, r0, r1)) return refuse(ctx, bad);
  if (pedestals)
    for (int p = 0; p < ATTPC_NUM_PADS; ++p)
      if (pedestals[p] < 0 || pedestals[p] > 4095)
        return fail(ctx, ATTPC_E_INVALID, "pedestal %d of pad %d: 0 .. 4095", (int)pedestals[p], p);
  TriggerArgs a{};
  int32_t rc;
  if ((rc = upload_trigger(ctx, d, ctx->tg_op_groups, &a.tg))) return rc;  // (checks, device, sync_all)
  if (n_events == 0) return ATTPC_OK;
  if (pedestals) {  // (a blocking copy, as it has always been: the slot is not one of the chunks')
    int16_t* d_pedestals = stage<int16_t>(ctx, 4, ATTPC_NUM_PADS, rc);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpy(d_pedestals, pedestals, ATTPC_NUM_PADS * sizeof(int16_t), hipMemcpyHostToDevice));
    a.pedestals = d_pedestals;
  }
  constexpr int64_t CHUNK_ROWS = 16384, CHUNK_EVENTS = 65536;  // a chunk: whole events up to these (at least one event)
  std::vector<int64_t> start;
  for (int64_t e0 = 0, e1; e0 < n_events; e0 = e1) {
    e1 = chunk_end(offsets, n_events, e0, CHUNK_ROWS, CHUNK_EVENTS);
    const size_t m = (size_t)(e1 - e0), rows = (size_t)(offsets[e1] - offsets[e0]);
    chunk_starts(offsets, e0, e1, &start);
    a.kept_start = stage_in(ctx, 2, start.data(), m + 1, rc);
    a.samples = stage_in(ctx, 0, rows ? samples + offsets[e0] * ATTPC_NUM_TB : nullptr, rows * ATTPC_NUM_TB, rc, ATTPC_NUM_TB);
    a.pads = stage_in(ctx, 1, rows ? pads + offsets[e0] : nullptr, rows, rc, 1);
    a.records = stage<attpc_trigger_record>(ctx, 3, m, rc);
    if (rc) return rc;
    a.row_pass = nullptr;
    launch_trigger(ctx->stream, (uint32_t)m, a);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = stage_out(ctx, out + e0, a.records, m))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return ATTPC_OK;
}

// ---- track estimates of the trace rows (estimate.hip; the contract is in include/attpc_engine.h) ----
int32_t attpc_trace_configure_estimates(attpc_ctx* ctx, const attpc_estimate_desc* d) {
  return configure_desc(ctx, d, estimate_desc_error, "estimates", &attpc_ctx::estimates_on, &attpc_ctx::estimates);
}

int32_t attpc_estimates_last(attpc_ctx* ctx, int64_t first, int64_t count, attpc_track_estimate* out) {
  if (!ctx) return ATTPC_E_INVALID;
  return records_last(ctx, ctx->est_records, __func__, "the last trace-row call made no track estimates, or kept them on the device",
                      first, count, out);
}

namespace {
// attpc_rows_estimate (circle == nullptr), attpc_rows_estimate_circle and attpc_rows_estimate_helix (helix != nullptr)
// under the name `func`
int32_t rows_estimate(attpc_ctx* ctx, const char* func, int64_t n_events, const int64_t* offsets, const double* rows,
                      const int64_t* labels, const attpc_event_layout* layout, const attpc_estimate_desc* d,
                      const attpc_circle_desc* circle, attpc_track_estimate* out, const attpc_helix_desc* helix = nullptr) {
  if (!ctx || n_events < 0 || !d || !layout) return ATTPC_E_INVALID;
  if (const int32_t bad = n_sim_range(ctx, func, layout->n_sim)) return bad;
  if (const char* bad = estimate_desc_error(*d)) return fail(ctx, ATTPC_E_INVALID, "estimates: %s", bad);
  if (circle)
    if (const char* bad = circle_desc_error(*circle)) return fail(ctx, ATTPC_E_INVALID, "circle: %s", bad);
  if (helix)
    if (const char* bad = helix_desc_error(*helix)) return fail(ctx, ATTPC_E_INVALID, "helix: %s", bad);
  const size_t n_sim = (size_t)layout->n_sim;
  if (n_events > 0 && n_sim && !out) return ATTPC_E_INVALID;
  if (const ArgError bad = csr_error(func, n_events, offsets)) return refuse(ctx, bad);
  if (n_events > 0 && offsets[n_events] > offsets[0] && (!rows || !labels)) return ATTPC_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc;
  if ((rc = sync_all(ctx))) return rc;
  if (n_events == 0 || n_sim == 0) return ATTPC_OK;
  EstimateArgs a{};
  estimate_settings(*d, &a);
  estimate_positions(*layout, a.slot_label);
  a.n_sim = (int32_t)n_sim;
  if (circle) circle_settings(*circle, &a);
  if (helix) a.helix_regressor = helix->regressor;
  std::vector<int64_t> start;
  for (int64_t e0 = 0, e1; e0 < n_events; e0 = e1) {
    e1 = chunk_end(offsets, n_events, e0, CHUNK_ROWS, CHUNK_EVENTS);
    const size_t m = (size_t)(e1 - e0);
    stage_rows(ctx, offsets, e0, e1, rows, labels, &start, rc).into(a);
    a.records = stage<attpc_track_estimate>(ctx, 3, m * n_sim, rc);
    if (rc) return rc;
    launch_estimate_kernel(ctx->stream, (uint32_t)m, a, false, circle != nullptr, helix != nullptr);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = stage_out(ctx, out + (size_t)e0 * n_sim, a.records, m * n_sim))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return ATTPC_OK;
}
}  // namespace

int32_t attpc_rows_estimate(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows, const int64_t* labels,
                            const attpc_event_layout* layout, const attpc_estimate_desc* d, attpc_track_estimate* out) {
  return rows_estimate(ctx, __func__, n_events, offsets, rows, labels, layout, d, nullptr, out);
}

// ---- geometric circle fit (estimate.hip; the contract is in include/attpc_engine.h) ----
int32_t attpc_trace_configure_circle(attpc_ctx* ctx, const attpc_circle_desc* d) {
  return configure_desc(ctx, d, circle_desc_error, "circle", &attpc_ctx::circle_on, &attpc_ctx::circle);
}

int32_t attpc_rows_estimate_circle(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows,
                                   const int64_t* labels, const attpc_event_layout* layout, const attpc_estimate_desc* d,
                                   const attpc_circle_desc* circle, attpc_track_estimate* out) {
  if (!circle) return ATTPC_E_INVALID;
  return rows_estimate(ctx, __func__, n_events, offsets, rows, labels, layout, d, circle, out);
}

// ---- helix slope (estimate.hip; the contract is in include/attpc_engine.h) ----
int32_t attpc_trace_configure_helix(attpc_ctx* ctx, const attpc_helix_desc* d) {
  return configure_desc(ctx, d, helix_desc_error, "helix", &attpc_ctx::helix_on, &attpc_ctx::helix);
}

int32_t attpc_rows_estimate_helix(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows,
                                  const int64_t* labels, const attpc_event_layout* layout, const attpc_estimate_desc* d,
                                  const attpc_circle_desc* circle, const attpc_helix_desc* helix, attpc_track_estimate* out) {
  if (!helix) return ATTPC_E_INVALID;
  return rows_estimate(ctx, __func__, n_events, offsets, rows, labels, layout, d, circle, out, helix);
}

// ---- clustering (cluster.hip, cluster_host.hpp; the contract is in include/attpc_engine.h) ----
int32_t attpc_trace_configure_clustering(attpc_ctx* ctx, const attpc_cluster_desc* d) {
  return configure_desc(ctx, d, cluster_desc_error, "clustering", &attpc_ctx::cluster_on, &attpc_ctx::cluster);
}

int32_t attpc_clusters_last(attpc_ctx* ctx, int64_t first, int64_t count, attpc_cluster_event* events,
                            attpc_cluster_record* records) {
  if (!ctx) return ATTPC_E_INVALID;
  const char* why = "the clustering was off for the last trace-row call";
  if (const int32_t rc = records_last(ctx, ctx->cl_events, __func__, why, first, count, events, false)) return rc;
  return records_last(ctx, ctx->cl_records, __func__, why, first, count, records, false);
}

int32_t attpc_cluster_labels_last(attpc_ctx* ctx, int64_t first_row, int64_t count, int64_t* out) {
  if (!ctx) return ATTPC_E_INVALID;
  if (!ctx->cl_events.made() || ctx->call.cluster_rows < 0)
    return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_cluster_labels_last: the last trace-row call made no cluster labels or did not fetch its rows");
  const int64_t rows = ctx->call.cluster_rows;
  if (first_row < 0 || count < 0 || first_row > rows || count > rows - first_row)
    return fail(ctx, ATTPC_E_INVALID, "attpc_cluster_labels_last: rows %lld .. + %lld of %lld", (long long)first_row, (long long)count, (long long)rows);
  if (count == 0) return ATTPC_OK;
  if (!out) return ATTPC_E_INVALID;
  std::memcpy(out, ctx->h_cl_labels.p + (size_t)first_row, (size_t)count * sizeof(int64_t));
  return ATTPC_OK;
}

namespace {

// attpc_rows_cluster (jd == nullptr) and attpc_rows_cluster_join
int32_t rows_cluster(attpc_ctx* ctx, const char* func, int64_t n_events, const int64_t* offsets, const double* rows,
                     const int64_t* labels, const attpc_event_layout* layout, const attpc_cluster_desc* d,
                     const attpc_join_desc* jd, int64_t* out_labels, attpc_cluster_event* events, attpc_cluster_record* records,
                     attpc_join_event* join_events, attpc_join_record* join_records) {
  if (!ctx || n_events < 0 || !d || !layout) return ATTPC_E_INVALID;
  if (const char* bad = cluster_layout_error(*layout)) return fail(ctx, ATTPC_E_INVALID, "%s: %s", func, bad);
  if (const char* bad = cluster_desc_error(*d)) return fail(ctx, ATTPC_E_INVALID, "clustering: %s", bad);
  if (jd)
    if (const char* bad = join_desc_error(*jd)) return fail(ctx, ATTPC_E_INVALID, "cluster joining: %s", bad);
  if (const ArgError bad = csr_error(func, n_events, offsets)) return refuse(ctx, bad);
  if (n_events > 0 && offsets[n_events] > offsets[0] && !rows) return ATTPC_E_INVALID;
  for (int64_t e = 0; e < n_events; ++e)
    if (offsets[e + 1] > offsets[e] && !cluster_rows_sorted(offsets[e + 1] - offsets[e], rows + offsets[e] * 8))
      return fail(ctx, ATTPC_E_INVALID, "%s: the in-range rows of event %lld are not in nondecreasing z", func, (long long)e);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc;
  if ((rc = sync_all(ctx))) return rc;
  if (n_events == 0) return ATTPC_OK;
  ClusterArgs a{};
  a.s = cluster_settings(*d, *layout);
  std::vector<int64_t> start;
  for (int64_t e0 = 0, e1; e0 < n_events; e0 = e1) {
    e1 = chunk_end(offsets, n_events, e0, CHUNK_ROWS, CHUNK_EVENTS);
    const size_t m = (size_t)(e1 - e0), n_rows = (size_t)(offsets[e1] - offsets[e0]), cap = std::max<size_t>(n_rows, 1);
    stage_rows(ctx, offsets, e0, e1, rows, labels, &start, rc, true).into(a);
    a.out_labels = stage<int64_t>(ctx, 3, cap, rc);
    a.events = stage<attpc_cluster_event>(ctx, 4, m, rc);
    a.records = stage<attpc_cluster_record>(ctx, 5, m * ATTPC_MAX_SIM, rc);
    if (!rc) rc = ensure(ctx, ctx->cl_scratch, cap * CLUSTER_SCRATCH_WORDS * sizeof(int32_t));
    if (rc) return rc;
    a.scratch = static_cast<int32_t*>(ctx->cl_scratch.p);
    launch_cluster(ctx->stream, (uint32_t)m, a);
    HIP_TRY(ctx, hipGetLastError());
    if (jd) {
      ClusterJoinArgs j{};
      j.c = a;
      j.j = join_settings(*jd);
      j.join_events = stage<attpc_join_event>(ctx, 6, m, rc);
      j.join_records = stage<attpc_join_record>(ctx, 7, m * ATTPC_MAX_SIM, rc);
      if (rc) return rc;
      launch_cluster_join(ctx->stream, (uint32_t)m, j);
      HIP_TRY(ctx, hipGetLastError());
      if (join_events && (rc = stage_out(ctx, join_events + e0, j.join_events, m))) return rc;
      if (join_records && (rc = stage_out(ctx, join_records + (size_t)e0 * ATTPC_MAX_SIM, j.join_records, m * ATTPC_MAX_SIM))) return rc;
    }
    if (out_labels && n_rows && (rc = stage_out(ctx, out_labels + offsets[e0], a.out_labels, n_rows))) return rc;
    if (events && (rc = stage_out(ctx, events + e0, a.events, m))) return rc;
    if (records && (rc = stage_out(ctx, records + (size_t)e0 * ATTPC_MAX_SIM, a.records, m * ATTPC_MAX_SIM))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (before the staging is filled again)
  }
  return ATTPC_OK;
}

}  // namespace

int32_t attpc_rows_cluster(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows, const int64_t* labels,
                           const attpc_event_layout* layout, const attpc_cluster_desc* d, int64_t* out_labels,
                           attpc_cluster_event* events, attpc_cluster_record* records) {
  return rows_cluster(ctx, __func__, n_events, offsets, rows, labels, layout, d, nullptr, out_labels, events, records, nullptr, nullptr);
}

// ---- cluster joining (cluster_join.hip, join_host.hpp; the contract is in include/attpc_engine.h) ----
int32_t attpc_trace_configure_cluster_join(attpc_ctx* ctx, const attpc_join_desc* d) {
  return configure_desc(ctx, d, join_desc_error, "cluster joining", &attpc_ctx::join_on, &attpc_ctx::join);
}

int32_t attpc_joins_last(attpc_ctx* ctx, int64_t first, int64_t count, attpc_join_event* events, attpc_join_record* records) {
  if (!ctx) return ATTPC_E_INVALID;
  const char* why = "the cluster joining or the clustering was off for the last trace-row call";
  if (const int32_t rc = records_last(ctx, ctx->jn_events, __func__, why, first, count, events, false)) return rc;
  return records_last(ctx, ctx->jn_records, __func__, why, first, count, records, false);
}

int32_t attpc_rows_cluster_join(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows, const int64_t* labels,
                                const attpc_event_layout* layout, const attpc_cluster_desc* d, const attpc_join_desc* jd,
                                int64_t* out_labels, attpc_cluster_event* events, attpc_cluster_record* records,
                                attpc_join_event* join_events, attpc_join_record* join_records) {
  if (!jd) return ATTPC_E_INVALID;
  return rows_cluster(ctx, __func__, n_events, offsets, rows, labels, layout, d, jd, out_labels, events, records, join_events,
                      join_records);
}

// ---- track fit (fit.hip; the contract is in include/attpc_engine.h) ----
int32_t attpc_trace_configure_fit(attpc_ctx* ctx, const attpc_fit_desc* d) {
  return configure_desc(ctx, d, fit_desc_error, "fit", &attpc_ctx::fit_on, &attpc_ctx::fit);
}

int32_t attpc_fits_last(attpc_ctx* ctx, int64_t first, int64_t count, attpc_track_fit* out) {
  if (!ctx) return ATTPC_E_INVALID;
  return records_last(ctx, ctx->fit_records, __func__, "the last trace-row call made no track fits", first, count, out);
}

namespace {

struct RowsFitHypotheses {  // what attpc_rows_fit_hypotheses has beyond attpc_rows_fit_pid
  const attpc_hypothesis_desc* desc;
  attpc_fit_hypothesis* records;  // [n_events][n_sim]
  attpc_track_fit* all;           // [n_events][n_sim][H], or nullptr
  int32_t* n;                     // H, or nullptr
  int32_t* species;               // [ATTPC_MAX_SIM], or nullptr
};

// attpc_rows_fit (pid == nullptr), attpc_rows_fit_pid and, with `hyp`, attpc_rows_fit_hypotheses (pid optional)
int32_t rows_fit(attpc_ctx* ctx, const char* func, int64_t n_events, const int64_t* offsets, const double* rows,
                 const int64_t* labels, const attpc_event_layout* layout, const attpc_estimate_desc* ed,
                 const attpc_track_estimate* estimates_in, const double* start, const attpc_fit_desc* fd,
                 const attpc_pid_record* pid, bool with_pid, attpc_track_fit* out, const RowsFitHypotheses* hyp = nullptr) {
  if (!ctx || n_events < 0 || !ed || !fd || !layout || (hyp && !hyp->desc)) return ATTPC_E_INVALID;
  if (const int32_t bad = n_sim_range(ctx, func, layout->n_sim)) return bad;
  if (layout->n_rows < 0 || layout->n_rows > ATTPC_MAX_ROWS)
    return fail(ctx, ATTPC_E_INVALID, "%s: n_rows %d outside 0 .. %d", func, layout->n_rows, ATTPC_MAX_ROWS);
  if (const char* bad = estimate_desc_error(*ed)) return fail(ctx, ATTPC_E_INVALID, "estimates: %s", bad);
  if (const char* bad = fit_desc_error(*fd)) return fail(ctx, ATTPC_E_INVALID, "fit: %s", bad);
  if (hyp)
    if (const char* bad = hypothesis_desc_error(*hyp->desc)) return fail(ctx, ATTPC_E_INVALID, "hypotheses: %s", bad);
  if (!ctx->det_ready) return fail(ctx, ATTPC_E_NOTCONFIGURED, "%s: no detector is configured", func);
  const size_t n_sim = (size_t)layout->n_sim;
  if (n_events > 0 && n_sim && (!out || !estimates_in || (with_pid && !pid) || (hyp && !hyp->records))) return ATTPC_E_INVALID;
  if (const ArgError bad = csr_error(func, n_events, offsets)) return refuse(ctx, bad);
  if (n_events > 0 && offsets[n_events] > offsets[0] && (!rows || !labels)) return ATTPC_E_INVALID;
  if (with_pid && !hyp)  // (the hypotheses read held, not position)
    for (size_t i = 0; i < (size_t)n_events * n_sim; ++i)
      if (pid[i].position < -1 || pid[i].position >= layout->n_sim)
        return fail(ctx, ATTPC_E_INVALID, "%s: pid[%zu].position %d outside -1 .. %d", func, i, pid[i].position, layout->n_sim - 1);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc;
  if ((rc = sync_all(ctx))) return rc;
  FitPosition position[ATTPC_MAX_SIM];
  fit_positions(ctx->det, *layout, position);
  HypLayout hl{};
  if (hyp) {
    int32_t species[ATTPC_MAX_SIM];
    for (int s = 0; s < ATTPC_MAX_SIM; ++s) species[s] = position[s].table;
    hl = hypothesis_layout(species, layout->n_sim, hyp->desc->candidates);
    if (hyp->n) *hyp->n = hl.n;
    for (int h = 0; h < ATTPC_MAX_SIM && hyp->species; ++h) hyp->species[h] = h < hl.n ? hl.species[hl.first[h]] : -1;
  }
  if (n_events == 0 || n_sim == 0) return ATTPC_OK;
  EstimateArgs a{};
  estimate_settings(*ed, &a);
  estimate_positions(*layout, a.slot_label);
  a.n_sim = (int32_t)n_sim;
  std::vector<int64_t> first;
  for (int64_t e0 = 0, e1; e0 < n_events; e0 = e1) {
    e1 = chunk_end(offsets, n_events, e0, CHUNK_ROWS, CHUNK_EVENTS);
    const size_t m = (size_t)(e1 - e0);
    stage_rows(ctx, offsets, e0, e1, rows, labels, &first, rc).into(a);
    a.records = const_cast<attpc_track_estimate*>(stage_in(ctx, 3, estimates_in + (size_t)e0 * n_sim, m * n_sim, rc));
    const double* d_start = start ? stage_in(ctx, 4, start + (size_t)e0 * n_sim * 6, m * n_sim * 6, rc) : nullptr;
    attpc_track_fit* d_out = stage<attpc_track_fit>(ctx, 5, m * n_sim, rc);
    const attpc_pid_record* d_pid = with_pid ? stage_in(ctx, 6, pid + (size_t)e0 * n_sim, m * n_sim, rc) : nullptr;
    // (hypotheses: the fits of every hypothesis and, behind them, the chosen records share slot 7)
    const size_t n_all = hyp ? m * n_sim * (size_t)hl.n : 0;
    char* d_hyp = hyp ? stage<char>(ctx, 7, n_all * sizeof(attpc_track_fit) + m * n_sim * sizeof(attpc_fit_hypothesis), rc) : nullptr;
    if (rc) return rc;
    if (hyp) {
      attpc_track_fit* d_all = reinterpret_cast<attpc_track_fit*>(d_hyp);
      attpc_fit_hypothesis* d_records = reinterpret_cast<attpc_fit_hypothesis*>(d_hyp + n_all * sizeof(attpc_track_fit));
      if (hl.n > 0 && (rc = enqueue_fit(ctx, a, (uint32_t)m, *fd, position, d_start, d_pid, d_all, &hl))) return rc;
      if ((rc = enqueue_hypothesis_select(ctx, hl, (uint32_t)m, a.n_sim, d_all, d_pid, a.records, d_records, d_out, nullptr))) return rc;
      if ((rc = stage_out(ctx, hyp->records + (size_t)e0 * n_sim, d_records, m * n_sim))) return rc;
      if (hyp->all && n_all && (rc = stage_out(ctx, hyp->all + (size_t)e0 * n_sim * (size_t)hl.n, d_all, n_all))) return rc;
    } else if ((rc = enqueue_fit(ctx, a, (uint32_t)m, *fd, position, d_start, d_pid, d_out))) return rc;
    if ((rc = stage_out(ctx, out + (size_t)e0 * n_sim, d_out, m * n_sim))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return ATTPC_OK;
}

}  // namespace

int32_t attpc_rows_fit(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows, const int64_t* labels,
                       const attpc_event_layout* layout, const attpc_estimate_desc* ed, const attpc_track_estimate* estimates_in,
                       const double* start, const attpc_fit_desc* fd, attpc_track_fit* out) {
  return rows_fit(ctx, __func__, n_events, offsets, rows, labels, layout, ed, estimates_in, start, fd, nullptr, false, out);
}

// ---- particle identification (pid.hip; the contract is in include/attpc_engine.h) ----
int32_t attpc_rows_fit_pid(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows, const int64_t* labels,
                           const attpc_event_layout* layout, const attpc_estimate_desc* ed,
                           const attpc_track_estimate* estimates_in, const double* start, const attpc_fit_desc* fd,
                           const attpc_pid_record* pid, attpc_track_fit* out) {
  return rows_fit(ctx, __func__, n_events, offsets, rows, labels, layout, ed, estimates_in, start, fd, pid, true, out);
}

// ---- fit hypotheses (fit.hip, hypothesis.hip; the contract is in include/attpc_engine.h) ----
int32_t attpc_trace_configure_hypotheses(attpc_ctx* ctx, const attpc_hypothesis_desc* d) {
  return configure_desc(ctx, d, hypothesis_desc_error, "hypotheses", &attpc_ctx::hyp_on, &attpc_ctx::hyp);
}

int32_t attpc_hypotheses_last(attpc_ctx* ctx, int64_t first, int64_t count, attpc_fit_hypothesis* out) {
  if (!ctx) return ATTPC_E_INVALID;
  return records_last(ctx, ctx->hyp_records, __func__, "the last trace-row call made no fit hypotheses", first, count, out);
}

int32_t attpc_hypothesis_fits_last(attpc_ctx* ctx, int64_t first, int64_t count, int32_t* n_hypotheses, attpc_track_fit* out) {
  if (!ctx) return ATTPC_E_INVALID;
  if (ctx->hyp_fits.made() && ctx->hyp_fits.to_host && n_hypotheses) *n_hypotheses = ctx->call.hyp.n;
  return records_last(ctx, ctx->hyp_fits, __func__, "the last trace-row call made no fit hypotheses", first, count, out);
}

int32_t attpc_rows_fit_hypotheses(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows,
                                  const int64_t* labels, const attpc_event_layout* layout, const attpc_estimate_desc* ed,
                                  const attpc_track_estimate* estimates_in, const double* start, const attpc_fit_desc* fd,
                                  const attpc_hypothesis_desc* d, const attpc_pid_record* pid, attpc_fit_hypothesis* records,
                                  attpc_track_fit* fits, attpc_track_fit* all_fits, int32_t* n_hypotheses, int32_t* species) {
  const RowsFitHypotheses hyp{d, records, all_fits, n_hypotheses, species};
  return rows_fit(ctx, __func__, n_events, offsets, rows, labels, layout, ed, estimates_in, start, fd, pid, pid != nullptr, fits, &hyp);
}

int32_t attpc_trace_configure_pid(attpc_ctx* ctx, const attpc_pid_desc* d) {
  if (!ctx) return ATTPC_E_INVALID;
  if (d)
    if (const char* bad = pid_desc_error(*d)) return fail(ctx, ATTPC_E_INVALID, "pid: %s", bad);
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  ctx->pid_on = false;
  if (!d) {  // (off: the gates' buffer goes too)
    release(ctx, ctx->pid_gates);
    return ATTPC_OK;
  }
  const int32_t rc = upload_pid_gates(ctx, ctx->pid_gates, *d);
  if (rc) return rc;
  ctx->pid = *d;
  ctx->pid_on = true;
  return ATTPC_OK;
}

int32_t attpc_pid_last(attpc_ctx* ctx, int64_t first, int64_t count, attpc_pid_record* out) {
  if (!ctx) return ATTPC_E_INVALID;
  return records_last(ctx, ctx->pid_records, __func__, "the last trace-row call made no particle identification", first, count, out);
}

int32_t attpc_estimates_pid(attpc_ctx* ctx, int64_t n_events, int32_t n_sim, const attpc_track_estimate* estimates,
                            const attpc_pid_desc* d, attpc_pid_record* out) {
  if (!ctx || n_events < 0 || !d) return ATTPC_E_INVALID;
  if (const int32_t bad = n_sim_range(ctx, __func__, n_sim)) return bad;
  if (const char* bad = pid_desc_error(*d)) return fail(ctx, ATTPC_E_INVALID, "pid: %s", bad);
  if (n_events > 0 && n_sim && (!estimates || !out)) return ATTPC_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc;
  if ((rc = sync_all(ctx))) return rc;
  if (n_events == 0 || n_sim == 0) return ATTPC_OK;
  if ((rc = upload_pid_gates(ctx, ctx->scratch[2], *d))) return rc;
  constexpr int64_t CHUNK_EVENTS = 1 << 20;
  for (int64_t e0 = 0; e0 < n_events; e0 += CHUNK_EVENTS) {
    const size_t m = (size_t)std::min<int64_t>(CHUNK_EVENTS, n_events - e0);
    const attpc_track_estimate* d_est = stage_in(ctx, 0, estimates + (size_t)e0 * (size_t)n_sim, m * (size_t)n_sim, rc);
    attpc_pid_record* d_out = stage<attpc_pid_record>(ctx, 1, m * (size_t)n_sim, rc);
    if (rc) return rc;
    if ((rc = enqueue_pid(ctx, d_est, (uint32_t)m, n_sim, ctx->scratch[2], d->mode, nullptr, d_out))) return rc;
    if ((rc = stage_out(ctx, out + (size_t)e0 * (size_t)n_sim, d_out, m * (size_t)n_sim))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  return ATTPC_OK;
}

// ---- reaction reconstruction (reaction.hip; the contract is in include/attpc_engine.h) ----
int32_t attpc_reaction_configure(attpc_ctx* ctx, const attpc_reaction_desc* d) {
  if (!ctx) return ATTPC_E_INVALID;
  if (d)
    if (const char* bad = reaction_desc_error(*d)) return fail(ctx, ATTPC_E_INVALID, "reaction: %s", bad);
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  ctx->reaction_on = false;
  ctx->rx_records.off();
  release(ctx, ctx->rx_eloss);  // (off, or other bins: the buffers go)
  release(ctx, ctx->rx_cells);
  if (!d) return ATTPC_OK;
  int32_t rc;
  if ((rc = upload_reaction_eloss(ctx, ctx->rx_eloss, *d))) return rc;
  if ((rc = ensure(ctx, ctx->rx_cells, (size_t)reaction_cells(d->n_ex, d->n_theta) * sizeof(uint64_t)))) return rc;
  ctx->reaction = *d;
  ctx->reaction.eloss = nullptr;
  ctx->reaction_on = true;
  return ATTPC_OK;
}

int32_t attpc_reaction_last(attpc_ctx* ctx, int64_t first, int64_t count, attpc_reaction_record* out) {
  if (!ctx) return ATTPC_E_INVALID;
  return records_last(ctx, ctx->rx_records, __func__, "the last trace-row call made no reaction reconstruction", first, count, out);
}

int32_t attpc_reaction_spectra_last(attpc_ctx* ctx, int64_t n_cells, uint64_t* cells) {
  if (!ctx) return ATTPC_E_INVALID;
  if (!ctx->rx_records.made())
    return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_reaction_spectra_last: the last trace-row call made no reaction reconstruction");
  if (n_cells != (int64_t)ctx->h_rx_cells.size() || !cells)
    return fail(ctx, ATTPC_E_INVALID, "%s: %lld cells, the spectra have %zu", __func__, (long long)n_cells, ctx->h_rx_cells.size());
  std::memcpy(cells, ctx->h_rx_cells.data(), ctx->h_rx_cells.size() * sizeof(uint64_t));
  return ATTPC_OK;
}

int32_t attpc_reaction_records(attpc_ctx* ctx, int64_t n_events, int32_t n_sim, int32_t n_rows, const attpc_reaction_desc* d,
                               const attpc_track_fit* fits, const attpc_track_estimate* estimates, const attpc_pid_record* pid,
                               const double* p4, const double* vertex, const int32_t* kin_status,
                               attpc_reaction_record* records, int64_t n_cells, uint64_t* cells) {
  if (!ctx || n_events < 0 || !d) return ATTPC_E_INVALID;
  if (const char* bad = reaction_desc_error(*d)) return fail(ctx, ATTPC_E_INVALID, "reaction: %s", bad);
  if (n_sim < 1 || n_sim > ATTPC_MAX_SIM) return fail(ctx, ATTPC_E_INVALID, "%s: n_sim %d outside 1 .. %d", __func__, n_sim, ATTPC_MAX_SIM);
  if (n_rows < 4 || n_rows > ATTPC_MAX_ROWS) return fail(ctx, ATTPC_E_INVALID, "%s: n_rows %d outside 4 .. %d", __func__, n_rows, ATTPC_MAX_ROWS);
  if (!pid && d->track >= n_sim) return fail(ctx, ATTPC_E_INVALID, "%s: track %d with n_sim %d", __func__, d->track, n_sim);
  if (n_cells != reaction_cells(d->n_ex, d->n_theta) || !cells)
    return fail(ctx, ATTPC_E_INVALID, "%s: %lld cells, the bins have %lld", __func__, (long long)n_cells,
                (long long)reaction_cells(d->n_ex, d->n_theta));
  const bool from_fit = d->source == ATTPC_REACTION_FROM_FIT;
  if (n_events > 0 && (!(from_fit ? (const void*)fits : (const void*)estimates) || !p4 || !vertex || !records)) return ATTPC_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc;
  if ((rc = sync_all(ctx))) return rc;
  uint64_t* d_cells = stage<uint64_t>(ctx, 6, (size_t)n_cells, rc);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemsetAsync(d_cells, 0, (size_t)n_cells * sizeof(uint64_t), ctx->stream));
  if ((rc = upload_reaction_eloss(ctx, ctx->scratch[7], *d))) return rc;
  constexpr int64_t CHUNK_EVENTS = 1 << 20;
  for (int64_t e0 = 0; e0 < n_events; e0 += CHUNK_EVENTS) {
    const size_t m = (size_t)std::min<int64_t>(CHUNK_EVENTS, n_events - e0), per = (size_t)n_sim;
    ReactionArgs a{};
    if (from_fit) a.fits = stage_in(ctx, 0, fits + (size_t)e0 * per, m * per, rc);
    else a.estimates = stage_in(ctx, 0, estimates + (size_t)e0 * per, m * per, rc);
    a.pid = pid ? stage_in(ctx, 1, pid + (size_t)e0 * per, m * per, rc) : nullptr;
    a.p4 = stage_in(ctx, 2, p4 + (size_t)e0 * (size_t)n_rows * 4, m * (size_t)n_rows * 4, rc);
    a.vertex = stage_in(ctx, 3, vertex + (size_t)e0 * 3, m * 3, rc);
    a.kin_status = kin_status ? stage_in(ctx, 4, kin_status + e0, m, rc) : nullptr;
    a.records = stage<attpc_reaction_record>(ctx, 5, m, rc);
    if (rc) return rc;
    a.cells = reinterpret_cast<unsigned long long*>(d_cells);
    a.n_events = (uint32_t)m;
    a.n_sim = n_sim;
    a.n_rows = n_rows;
    if ((rc = enqueue_reaction(ctx, a, *d, ctx->scratch[7]))) return rc;
    if ((rc = stage_out(ctx, records + e0, a.records, m))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  if ((rc = stage_out(ctx, cells, d_cells, (size_t)n_cells))) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return ATTPC_OK;
}

// ---- thinned track points (thin.hip; the contract is in include/attpc_engine.h) ----
int32_t attpc_trace_configure_thinning(attpc_ctx* ctx, const attpc_thin_desc* d) {
  return configure_desc(ctx, d, thin_desc_error, "thinning", &attpc_ctx::thinning_on, &attpc_ctx::thinning);
}

int32_t attpc_rows_thin(attpc_ctx* ctx, int64_t n_events, const int64_t* offsets, const double* rows, const int64_t* labels,
                        const attpc_event_layout* layout, const attpc_thin_desc* d, int64_t capacity, int64_t* point_offsets,
                        double* points, int64_t* point_labels, attpc_thin_info* info, int64_t* needed) {
  if (!ctx || n_events < 0 || !d || !layout || capacity < 0 || !needed) return ATTPC_E_INVALID;
  if (const int32_t bad = n_sim_range(ctx, __func__, layout->n_sim)) return bad;
  if (const char* bad = thin_desc_error(*d)) return fail(ctx, ATTPC_E_INVALID, "thinning: %s", bad);
  const size_t n_sim = (size_t)layout->n_sim;
  if (!point_offsets || (n_events > 0 && n_sim && !info)) return ATTPC_E_INVALID;
  if (const ArgError bad = csr_error(__func__, n_events, offsets)) return refuse(ctx, bad);
  if (n_events > 0 && offsets[n_events] > offsets[0] && (!rows || !labels)) return ATTPC_E_INVALID;
  if (capacity > 0 && (!points || !point_labels)) return ATTPC_E_INVALID;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc;
  if ((rc = sync_all(ctx))) return rc;
  *needed = 0;
  point_offsets[0] = 0;
  if (n_events == 0) return ATTPC_OK;
  if (n_sim == 0) {
    std::fill(point_offsets, point_offsets + n_events + 1, (int64_t)0);
    return ATTPC_OK;
  }
  ThinArgs a{};
  estimate_positions(*layout, a.slot_label);
  a.n_sim = (int32_t)n_sim;
  a.step = thin_step_units(d->z_step);
  std::vector<int64_t> start;
  std::vector<ThinPoint> sparse;  // the chunk's point buffer: the regions of its (event, position)s
  int64_t total = 0;              // points so far
  for (int64_t e0 = 0, e1; e0 < n_events; e0 = e1) {
    e1 = chunk_end(offsets, n_events, e0, CHUNK_ROWS, CHUNK_EVENTS);
    const size_t m = (size_t)(e1 - e0), n_rows = (size_t)(offsets[e1] - offsets[e0]), cap = std::max<size_t>(n_rows, 1);
    stage_rows(ctx, offsets, e0, e1, rows, labels, &start, rc).into(a);
    a.points = stage<ThinPoint>(ctx, 3, cap, rc);
    a.info = stage<attpc_thin_info>(ctx, 4, m * n_sim, rc);
    if (rc) return rc;
    launch_thin(ctx->stream, (uint32_t)m, a);
    HIP_TRY(ctx, hipGetLastError());
    sparse.resize(cap);
    attpc_thin_info* chunk_info = info + (size_t)e0 * n_sim;
    if ((rc = stage_out(ctx, chunk_info, a.info, m * n_sim))) return rc;
    if (n_rows && (rc = stage_out(ctx, sparse.data(), a.points, n_rows))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // the regions -> CSR, position-major per event
    for (size_t e = 0; e < m; ++e) {
      int64_t region = start[e];
      for (size_t s = 0; s < n_sim; ++s) {
        const attpc_thin_info& i = chunk_info[e * n_sim + s];
        for (int32_t k = 0; k < i.n_points; ++k, ++total) {
          if (total >= capacity) continue;
          const ThinPoint& p = sparse[(size_t)region + (size_t)k];
          double* row = points + total * 8;
          row[0] = (double)p.X / 16.0;
          row[1] = (double)p.Y / 16.0;
          row[2] = (double)p.Z / 16.0;
          row[3] = p.amplitude;
          row[4] = (double)p.si;
          row[5] = (double)p.n;
          row[6] = (double)p.bin;
          row[7] = (double)p.split;
          point_labels[total] = layout->indices[s];
        }
        region += i.n_rows;
      }
      point_offsets[e0 + (int64_t)e + 1] = total;
    }
  }
  *needed = total;
  if (total > capacity)
    return fail(ctx, ATTPC_E_CAPACITY, "attpc_rows_thin: %lld points, capacity %lld", (long long)total, (long long)capacity);
  return ATTPC_OK;
}

int32_t attpc_sim_run_trace_rows(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                 const attpc_event_layout* layout, double* p4, double* vertex, int32_t* kin_status,
                                 attpc_cloud_out* out, attpc_run_stats* stats) {
  return run_entry(__func__, ctx, seed, first_event, n_events, layout, RunSource{true}, RunSink{p4, vertex, kin_status},
                   RunOut{OutMode::trace_rows, out}, stats);
}

int32_t attpc_det_run_trace_rows(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                                 const attpc_event_layout* layout, const double* p4, const double* vertex,
                                 attpc_cloud_out* out, attpc_run_stats* stats) {
  return run_entry(__func__, ctx, seed, first_event, n_events, layout, RunSource{false, p4, vertex}, RunSink{},
                   RunOut{OutMode::trace_rows, out}, stats);
}

int32_t attpc_trace_rows_at(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, int64_t n_events, const int64_t* offsets,
                            const double* points, const int64_t* labels, attpc_cloud_out* out) {
  if (!ctx || !out) return ATTPC_E_INVALID;
  int32_t rc;
  if ((rc = trace_rows_ready(ctx, __func__))) return rc;
  RunOut o{OutMode::trace_rows, out};
  if (out->offsets) out->offsets[0] = 0;
  if ((rc = host_cloud_run(ctx, seed, first_event, n_events, offsets, points, labels, o))) return rc;
  if ((rc = read_peak_sums(ctx, o))) return rc;
  return run_status(ctx, attpc_run_stats{}, nullptr, o);
}

int32_t attpc_trace_rows_last(attpc_ctx* ctx, int64_t* n_rows, uint64_t* row_checksum) {
  if (!ctx) return ATTPC_E_INVALID;
  if (n_rows) *n_rows = ctx->last_rows;
  if (row_checksum) *row_checksum = ctx->last_row_checksum;
  return ATTPC_OK;
}

int32_t attpc_sim_hint_next(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                            const attpc_event_layout* layout) {
  if (!ctx) return ATTPC_E_INVALID;
  ctx->hint_valid = false;
  if (!layout || n_events == 0) return ATTPC_OK;  // "nothing known about the next call"
  if (!ctx->kin_ready || !ctx->det_ready) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_sim_hint_next before the configure calls");
  int32_t rc = validate_id_range(ctx, first_event, n_events);
  if (rc) return rc;
  if ((rc = validate_layout(ctx, layout, true))) return rc;
  if (layout->n_rows != kin_rows(ctx)) return fail(ctx, ATTPC_E_INVALID, "layout.n_rows does not match the pipeline");
  ctx->hint_valid = true;
  ctx->hint_seed = seed;
  ctx->hint_first = first_event;
  ctx->hint_n = n_events;
  ctx->hint_lay = *layout;
  return ATTPC_OK;
}

int32_t attpc_spyral_configure(attpc_ctx* ctx, const attpc_spyral_desc* d) {
  if (!ctx || !d || !d->response || !d->pad_centers || !d->pad_sizes || d->n_pads < 1) return ATTPC_E_INVALID;
  if (d->windows_edge <= d->micromegas_edge) return fail(ctx, ATTPC_E_INVALID, "windows_edge <= micromegas_edge");
  { int32_t rc0 = begin_configure(ctx); if (rc0) return rc0; }
  ctx->spyral_allocs.clear();
  ctx->spyral_ready = false;
  SpyralDev sp{};
  static_assert(SPYRAL_SAMPLES == ATTPC_NUM_TB, "spyral_integral.hpp: one table entry per response sample");
  std::vector<double> sorted(ATTPC_NUM_TB), tail(ATTPC_NUM_TB + 1);
  spyral_integral_tables(d->response, sorted.data(), tail.data());
  int32_t rc;
  if ((rc = upload(ctx, ctx->spyral_allocs, d->response, (size_t)ATTPC_NUM_TB, &sp.response))) return rc;
  if ((rc = upload(ctx, ctx->spyral_allocs, sorted.data(), sorted.size(), &sp.sorted_desc))) return rc;
  if ((rc = upload(ctx, ctx->spyral_allocs, tail.data(), tail.size(), &sp.tail))) return rc;
  if ((rc = upload(ctx, ctx->spyral_allocs, d->pad_centers, (size_t)d->n_pads * 2, &sp.pad_centers))) return rc;
  if ((rc = upload(ctx, ctx->spyral_allocs, d->pad_sizes, (size_t)d->n_pads, &sp.pad_sizes))) return rc;
  ctx->h_pad_centers.assign(d->pad_centers, d->pad_centers + (size_t)d->n_pads * 2);
  ctx->h_pad_sizes.assign(d->pad_sizes, d->pad_sizes + (size_t)d->n_pads);
  sp.n_pads = d->n_pads;
  sp.r_max = sorted[0];
  sp.window_edge = (double)d->windows_edge;
  sp.mm_edge = (double)d->micromegas_edge;
  sp.length = d->length;
  sp.threshold = d->adc_threshold;
  ctx->spyral = sp;
  ctx->spyral_ready = true;
  return ATTPC_OK;
}

int32_t attpc_det_tracks(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                         const attpc_event_layout* layout, const double* p4, const double* vertex,
                         int64_t max_samples_per_track, double* samples, int32_t* counts, int32_t* n_steps) {
  if (!ctx || !p4 || !vertex || !counts || !n_steps) return ATTPC_E_INVALID;
  if (!ctx->det_ready) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_det_configure has not been called");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc = validate_layout(ctx, layout, true);
  if (rc) return rc;
  if ((rc = validate_id_range(ctx, first_event, n_events))) return rc;
  if (n_events > (uint64_t)ctx->chunk_events) return fail(ctx, ATTPC_E_INVALID, "attpc_det_tracks handles at most one chunk");
  if ((rc = drop_prefetch(ctx))) return rc;
  const uint32_t n = (uint32_t)n_events;
  TrackSet& ts = ctx->tset[0];
  TrackLaunch tl;
  RunSource src;
  src.h_p4 = p4;
  src.h_vertex = vertex;
  if ((rc = queue_batch(ctx, ts, tl, *layout, src, seed, first_event, 0, n, layout->n_rows))) return rc;
  TrackBuffers trk;
  double ms = 0;
  if ((rc = finish_tracks(ctx, ts, tl, &trk, &ms, nullptr))) return rc;
  const uint32_t n_tracks = n * (uint32_t)layout->n_sim;
  if (n_tracks == 0) return ATTPC_OK;
  std::vector<int32_t> table((size_t)n_tracks * MAX_BLOCKS_PER_TRACK);
  HIP_TRY(ctx, hipMemcpy(table.data(), ts.block_table.p, table.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(counts, ts.counts.p, (size_t)n_tracks * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(n_steps, ts.n_steps.p, (size_t)n_tracks * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (samples) {
    // TRK_NEXT_BLOCK counts reserved blocks (waves reserve pools), all below arena_blocks after a good run
    std::vector<double> arena(std::min<size_t>(ts.h_ctrl[TRK_NEXT_BLOCK], ts.arena_blocks) * ARENA_BLK * 4);
    if (!arena.empty()) HIP_TRY(ctx, hipMemcpy(arena.data(), ts.arena.p, arena.size() * sizeof(double), hipMemcpyDeviceToHost));
    const size_t n_blocks = arena.size() / ((size_t)ARENA_BLK * 4);
    for (uint32_t t = 0; t < n_tracks; ++t) {
      // a track the kernel never ran leaves whatever its count and block entries held: an error, not a read past the copy
      if (counts[t] < 0 || counts[t] > MAX_BLOCKS_PER_TRACK * ARENA_BLK)
        return fail(ctx, ATTPC_E_DATALOSS, "attpc_det_tracks: track %u has %d samples (0..%d)", t, counts[t], MAX_BLOCKS_PER_TRACK * ARENA_BLK);
      const int64_t c = std::min<int64_t>(counts[t], max_samples_per_track);
      for (int64_t s = 0; s < c; ++s) {
        const int32_t blk = table[(size_t)t * MAX_BLOCKS_PER_TRACK + s / ARENA_BLK];
        if (blk < 0 || (size_t)blk >= n_blocks)
          return fail(ctx, ATTPC_E_DATALOSS, "attpc_det_tracks: track %u names arena block %d of %zu", t, blk, n_blocks);
        std::memcpy(samples + ((size_t)t * max_samples_per_track + s) * 4,
                    arena.data() + ((size_t)blk * ARENA_BLK + (s % ARENA_BLK)) * 4, 4 * sizeof(double));
      }
    }
  }
  return ATTPC_OK;
}

int32_t attpc_det_scatter(attpc_ctx* ctx, uint64_t seed, uint64_t first_event, uint64_t n_events,
                          const attpc_event_layout* layout, const double* samples, const int32_t* counts,
                          attpc_cloud_out* out, attpc_run_stats* stats) {
  if (!ctx || !counts || !layout) return ATTPC_E_INVALID;
  if (!ctx->det_ready) return fail(ctx, ATTPC_E_NOTCONFIGURED, "attpc_det_configure has not been called");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc = validate_layout(ctx, layout, false);
  if (rc) return rc;
  if ((rc = validate_id_range(ctx, first_event, n_events))) return rc;
  if (n_events > (uint64_t)ctx->chunk_events) return fail(ctx, ATTPC_E_INVALID, "attpc_det_scatter handles at most one chunk");
  if ((rc = drop_prefetch(ctx))) return rc;
  const uint32_t n = (uint32_t)n_events;
  const uint32_t n_tracks = n * (uint32_t)layout->n_sim;
  // pack the samples into arena blocks, one chain of consecutive blocks per track
  std::vector<int32_t> table((size_t)n_tracks * MAX_BLOCKS_PER_TRACK, 0);
  size_t total_samples = 0, n_blocks = 0;
  for (uint32_t t = 0; t < n_tracks; ++t) {
    if (counts[t] < 0 || counts[t] > MAX_BLOCKS_PER_TRACK * ARENA_BLK)
      return fail(ctx, ATTPC_E_INVALID, "counts[%u]=%d: a track holds 0..%d samples", t, counts[t], MAX_BLOCKS_PER_TRACK * ARENA_BLK);
    total_samples += (size_t)counts[t];
    n_blocks += ((size_t)counts[t] + ARENA_BLK - 1) / ARENA_BLK;
  }
  if (total_samples && !samples) return ATTPC_E_INVALID;
  std::vector<double> arena(std::max<size_t>(n_blocks, 1) * ARENA_BLK * 4, 0.0);
  size_t blk = 0, src_row = 0;
  for (uint32_t t = 0; t < n_tracks; ++t) {
    const size_t nb = ((size_t)counts[t] + ARENA_BLK - 1) / ARENA_BLK;
    for (size_t b = 0; b < nb; ++b) table[(size_t)t * MAX_BLOCKS_PER_TRACK + b] = (int32_t)(blk + b);
    if (counts[t]) std::memcpy(arena.data() + blk * ARENA_BLK * 4, samples + src_row * 4, (size_t)counts[t] * 4 * sizeof(double));
    blk += nb;
    src_row += (size_t)counts[t];
  }
  if ((rc = sync_all(ctx))) return rc;
  TrackSet& ts = ctx->tset[0];
  if ((rc = ensure(ctx, ts.arena, arena.size() * sizeof(double)))) return rc;
  ts.arena_blocks = std::max(ts.arena_blocks, arena.size() / ((size_t)ARENA_BLK * 4));
  if ((rc = ensure(ctx, ts.block_table, std::max<size_t>(table.size(), 1) * sizeof(int32_t)))) return rc;
  if ((rc = ensure(ctx, ts.counts, std::max<size_t>(n_tracks, 1) * sizeof(int32_t)))) return rc;
  HIP_TRY(ctx, hipMemcpy(ts.arena.p, arena.data(), arena.size() * sizeof(double), hipMemcpyHostToDevice));
  if (n_tracks) {
    HIP_TRY(ctx, hipMemcpy(ts.block_table.p, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ts.counts.p, counts, (size_t)n_tracks * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  const TrackBuffers trk = track_buffers(ts);  // (the scatter reads arena, block_table and counts only)
  UnpackDrain drain(ctx);
  attpc_run_stats st{};
  st.n_events = n_events;
  RunOut o{OutMode::cloud, out};
  if (int64_t* offsets = o.offsets()) offsets[0] = 0;
  const double keep_rows = ctx->rows_per_event, keep_segs = ctx->segs_per_event;
  ctx->rows_per_event = ctx->segs_per_event = 0.0;  // explicit samples say nothing about the configured workload
  rc = run_batch_chunks(ctx, *layout, trk, seed, first_event, 0, n, o, &st, []() -> int32_t { return ATTPC_OK; });
  ctx->rows_per_event = keep_rows;
  ctx->segs_per_event = keep_segs;
  if (rc) return rc;
  if ((rc = sync_all(ctx))) return rc;
  return run_status(ctx, st, stats, o);
}

}  // extern "C"

// ---- response + Spyral rows ("next" row 1; spyral_rows_kernel of spyral.hip) ----
extern "C" int32_t attpc_spyral_rows(attpc_ctx* ctx, int64_t n_points, const double* points, const double* response,
                                     const double* pad_centers, const double* pad_sizes, int32_t n_pads,
                                     int32_t windows_edge, int32_t micromegas_edge, double length, double* rows) {
  if (!ctx || !points || !response || !pad_centers || !pad_sizes || !rows || n_pads < 1) return ATTPC_E_INVALID;
  if (n_points <= 0) return ATTPC_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int32_t rc = ATTPC_OK;
  const size_t n = (size_t)n_points;
  const double* d_points = stage_in(ctx, 0, points, n * 3, rc);
  const double* d_response = stage_in(ctx, 1, response, (size_t)ATTPC_NUM_TB, rc);
  const double* d_centers = stage_in(ctx, 2, pad_centers, (size_t)n_pads * 2, rc);
  const double* d_sizes = stage_in(ctx, 3, pad_sizes, (size_t)n_pads, rc);
  double* d_rows = stage<double>(ctx, 4, n * 8, rc);
  if (rc) return rc;
  attpc::launch_spyral_rows_kernel(ctx->stream, n_points, d_points, d_response, d_centers, d_sizes, n_pads, (double)windows_edge,
                                   (double)micromegas_edge, length, d_rows);
  HIP_TRY(ctx, hipGetLastError());
  if ((rc = stage_out(ctx, rows, d_rows, n * 8))) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return ATTPC_OK;
}
