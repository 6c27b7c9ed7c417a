// dtrl_engine.h -- batch engine: owns the device slabs, the per-env ground windows and the frame loop.
// The backend interface isolates the HIP runtime (dtrl_backend_hip.hip) from the engine logic so that the same logic can
// be unit-tested on a CPU-only box against the lane-loop build of the kernel math (tests/emul/, tests only).
#pragma once
#include "dtrl_host.h"
#include "dtrl_kernel.h"
#include "dtrl_terrain_dev.h"
#include <string>
#include <vector>

namespace dtrl {

// scratch of the packed tuple drain (device memory): order [cap], hist [n_envs + 1], meta [4], carry staging rows [cap][W] / flags [cap] / env [cap]
struct PackScratch { int32_t* order = nullptr; int32_t* hist = nullptr; int32_t* meta = nullptr; float* rows = nullptr; uint32_t* flags = nullptr; int32_t* env = nullptr; };

// ---- env snapshots (include/dtrl.h: dtrl_snapshot_save ...) ----
// One per-env record family of a snapshot: env e's record is `bytes` bytes at slab + e * bytes (records are contiguous in every slab) and sits at byte `off`
// (a multiple of 8) of the env's slice of a snapshot payload. `bytes` is a multiple of 4 (the fp32 library's policy-state rows); everything else is 8-aligned.
struct SnapRec { char* slab = nullptr; uint32_t bytes = 0, off = 0, host = 0, pad_ = 0; };   // host: the slab is page-locked HOST memory (the status array of host terrain mode)
constexpr int kSnapRecs = 12;   // (most in use: 9 -- external policy mode with -terrain_gen= device)
// what moves with an env, and how a payload slice is laid out. gr_rec >= 0 (host terrain mode): rec[gr_rec] is the GroundRec slab, and an env whose regenerated
// record is still waiting in page-locked memory (stage_slot[e] > 0) is READ from gr_stage[stage_slot[e] - 1], the record that will be in force at its next launch
struct SnapPlan { SnapRec rec[kSnapRecs]; int32_t n_rec = 0, gr_rec = -1; uint32_t env_bytes = 0; const GroundRec* gr_stage = nullptr; const int32_t* stage_slot = nullptr; };

// ---- policy slots (include/dtrl.h: dtrl_slots_create ...) ----
// One record per slot of the device-visible slot table: where the slot's net lives and how it explores. kSlotLaunchPolicy: the five policy pointers are NOT
// taken from the record but from the launch's own DevBuffers (slot 0 and every alias of it: slot 0's weights change buffers with a hand-over while launches are
// in flight, and a launch argument cannot change under a running kernel); kSlotLaunchExplore: the same for the exploration settings and RunParams (slot 0:
// dtrl_set_explore acts at any time). Everything else in the table is only ever rewritten while every stream is idle.
enum SlotFlags { kSlotLaunchPolicy = 1, kSlotLaunchExplore = 2 };
constexpr int kMaxSlots = 32;
struct SlotRec {
	const float* weights;
	const real* in_off; const real* in_scale; const real* out_off; const real* out_scale;
	real exp_rate, exp_temp, exp_base_rate;
	int32_t enable_exp, flags;
};
static_assert(sizeof(SlotRec) % 8 == 0, "slot records are read as 64-bit words");
DTRL_HD_INLINE void slot_patch(const SlotRec& r, RunParams& rp, DevBuffers& buf)
{
	if (!(r.flags & kSlotLaunchPolicy)) { buf.weights = r.weights; buf.in_off = r.in_off; buf.in_scale = r.in_scale; buf.out_off = r.out_off; buf.out_scale = r.out_scale; }
	if (!(r.flags & kSlotLaunchExplore)) { rp.enable_exp = r.enable_exp; rp.exp_rate = r.exp_rate; rp.exp_temp = r.exp_temp; rp.exp_base_rate = r.exp_base_rate; }
}
// what a launch over envs of several keys is given, a key being the env's policy slot or its model variant (the two exclude each other): the per-env key array
// (indexed by local env id) as the kernels read it (device memory) and as the host loops read it, and what the per-key default needs to split a launch list:
// the list in host-readable form (nullptr: it exists on the device only and is read back; ignored when the launch has no list) and `part`, HostStaging()
// memory for the launch's n_envs entries regrouped by key. Policy slots add the slot table in both forms, model variants the table of complete DevModel
// records (device memory; record 0 is a copy of the batch's own model); the other family's pointers stay null.
struct EnvKeyView {
	int32_t n_keys = 0;
	const int32_t* env_key_dev = nullptr; const int32_t* env_key_host = nullptr;
	bool keys_on_device = false;   // a variant redraw on device terrain moves env_key_dev while frames run: the per-key default reads the listed envs' keys from there
	const int32_t* env_list_host = nullptr;
	int32_t* part = nullptr;
	const SlotRec* slots_dev = nullptr; const SlotRec* slots_host = nullptr;
	const DevModel* models_dev = nullptr;
};
// per-slot totals of dtrl_slot_stats (Backend::SlotReduce): envs in the slot, and over them the sums dtrl_eval_stats takes over the batch
struct SlotSums { int64_t n_envs, episodes, cycles, resets; double dist_sum; };   // dist_sum = sum of avg_dist * num_episodes

// which TerrainCfg the terrain work of an env runs under, and the ladder's rule in front of it (Backend::TerrainBoundary). All null: the batch's own *buf.tcfg
struct TerrainRule { const TerrainCfg* table = nullptr; int32_t* env_terrain = nullptr; LadderRec* ladder = nullptr; LadderCfg lc{}; };

class Backend {
public:
	virtual ~Backend() {}
	// A launch over envs of several keys: env e runs slot keys.env_key[e]'s record patched over rp / buf (slot_patch), or under the model keys.models_dev[keys.env_key[e]]
	// (gm is then record 0). The default is one Launch per non-empty key over that key's part of the launch list, list order kept inside a key (what the lane-loop
	// check build runs, and DTRL_SLOTS_FALLBACK=1 / DTRL_VARIANTS_FALLBACK=1 on HIP; it waits for the selected stream before it reuses keys.part). The HIP backend
	// overrides it with ONE launch of the family's kernels (dtrl_backend_hip_slots.hip, dtrl_backend_hip_variants.hip).
	virtual bool LaunchKeyed(const DevModel* gm, const RunParams& rp, const DevBuffers& buf, const EnvKeyView& keys, int n_envs, int n_steps, real dt, bool frame_end);
	// sums[s] for s < n_slots (<= kMaxSlots) over the envs e < n_envs with env_slot[e] == slot_base + s (an env outside the window counts nowhere: the per-variant
	// statistics take a table of any size in windows of kMaxSlots); st / env_slot are device memory, sums host memory. Synchronised. The default is a
	// host loop over a D2H of the records; the HIP backend reduces on the device (two launches, fixed summation order: the same bytes from call to call)
	virtual bool SlotReduce(const EnvState* st, const int32_t* env_slot, int n_envs, int n_slots, SlotSums* sums, int slot_base);
	// Snapshot transport. ids / src_ids / dst_ids live in HostStaging() memory (host- and device-addressable), payload is device memory laid out [n][env_bytes].
	// Queued on the selected stream and synchronised. The defaults are built from D2D (one copy per record and env); the HIP backend overrides them with
	// one kernel launch each (one wavefront per listed env, every record copied as consecutive 64-bit words).
	//   SnapGather   payload slice i  <- env ids[i]          (save)
	//   SnapScatter  env ids[i]       <- payload slice i     (restore; ids are distinct)
	//   SnapCopy     env dst_ids[i]   <- env src_ids[i]      (clone; dst ids are distinct and NO env is both read and written: the engine stages overlapping lists)
	virtual bool SnapGather(const SnapPlan& p, char* payload, const int32_t* ids, int n);
	virtual bool SnapScatter(const SnapPlan& p, const char* payload, const int32_t* ids, int n);
	virtual bool SnapCopy(const SnapPlan& p, const int32_t* src_ids, const int32_t* dst_ids, int n);
	// External policy mode (include/dtrl.h dtrl_pending_actions* / dtrl_supply_actions*). Queued on the selected stream and synchronised. ids / states / the row
	// arrays are device memory, meta is HostStaging() memory. The defaults are host loops over D2H / H2D (what the lane-loop check build runs); the HIP backend
	// overrides them with its kernels (a scan-based compaction + one wavefront per env / per row).
	//   ExtCollect  ids[0 .. m) = the awaiting envs in ascending env id (m = min(#awaiting, cap)), states row i = env ids[i]'s S policy-state values as float
	//               (f32) or double; meta = {m, #awaiting, #ready, 0}. states may be null (counts and ids only)
	//   ExtSupply   row i -> env ids[i]'s slab record, awaiting -> ready; a row whose id or label (0 .. n_labels - 1) is out of range or whose env is not awaiting is skipped and counted in *rejected
	//               (host memory). apply = false: count only, write nothing
	virtual bool ExtCollect(const DevBuffers& buf, int n_envs, int cap, int32_t* ids, void* states, bool f32, int32_t* meta);
	virtual bool ExtSupply(const DevBuffers& buf, int n_envs, int n_opt, int n_labels, const int32_t* ids, int n, const int32_t* action_ids, const void* params, bool f32, const uint32_t* flags, bool apply, int32_t* rejected);
	virtual double ExtLaunchMs(int which) { (void)which; return -1.0; }   // device time of the collection (0) / scatter (1) launches since the last call (HIP events)
	virtual double SnapLaunchMs() { return -1.0; }   // device time of the snapshot launches since the last call (HIP events; -1: this backend launches nothing)
	virtual bool Init(int device_id, std::string& err) = 0;
	// -reserve_cus= k (before Init): keep k compute units per XCD out of the frame launches (HIP backend; see dtrl_side_stream in include/dtrl.h)
	virtual void SetReserveCus(int) {}
	// k = 0, 1: a stream (hipStream_t) whose kernels start on the reserved units while frame launches are in flight; nullptr without a reservation
	virtual void* SideStream(int) { return nullptr; }
	virtual double SideStreamDelayUs(int) { return -1.0; }
	virtual void* Alloc(size_t bytes) = 0;   // zero-filled
	virtual void Free(void* p) = 0;
	virtual bool H2D(void* dst, const void* src, size_t n) = 0;
	// stream-ordered upload without a host sync; src must come from HostStaging() and stay untouched until the next Sync()/D2H()
	virtual bool H2DAsync(void* dst, const void* src, size_t n) = 0;
	// stream-ordered download into HostStaging() memory without a host sync (valid after SyncSelected())
	virtual bool D2HAsync(void* dst, const void* src, size_t n) = 0;
	virtual void* HostStaging(size_t bytes) = 0;   // page-locked host memory the device can address directly through the same pointer (coherent; plain malloc in the test backend)
	virtual bool SyncSelected() = 0;               // wait for the selected stream
	virtual void FreeHostStaging(void* p) = 0;
	virtual bool D2H(void* dst, const void* src, size_t n) = 0;
	virtual bool D2D(void* dst, const void* src, size_t n) = 0;   // device-to-device on the selected stream, synchronised before returning
	// dst[i] = idx[i] >= 0 ? src[idx[i]] : 0 for i < n, all device pointers (policy hand-over without a host round trip); synchronised
	virtual bool GatherF32(float* dst, const float* src, const int32_t* idx, size_t n) = 0;
	// the same on a stream of the caller's (a hipStream_t; nullptr = the selected stream), synchronised: work the caller has queued there comes first
	virtual bool GatherF32On(void* stream, float* dst, const float* src, const int32_t* idx, size_t n) { (void)stream; return GatherF32(dst, src, idx, n); }
	// ---- the per-env rules of the frame boundary (dtrl_terrain_dev.h), each over an EnvSpan and queued on the selected stream ----
	// Every default is a host loop over the span's envs with per-env D2H / H2D of what the rule reads and writes, synchronised -- what the lane-loop check build
	// runs, and DTRL_TERRAINS_FALLBACK=1 / DTRL_VARIANTS_FALLBACK=1 / DTRL_PUSH_FALLBACK=1 / DTRL_PERTURB_FALLBACK=1 / DTRL_EPISODE_FALLBACK=1 / DTRL_TRACE_FALLBACK=1 / DTRL_EPISODE_LOG_FALLBACK=1 on HIP; the HIP backend overrides each with ONE
	// launch of its kernel. All per-env arrays are device memory under the local env id, and are written back only where the rule changed them.
	// the span as a host vector (a list is read back: the copy waits for the selected stream)
	bool SpanList(const EnvSpan& span, std::vector<int32_t>& list);
	// -terrain_gen= device: the terrain work (tg_env_boundary); mode 0 = after a frame, 1 = (re)initialise, 2 = re-seed + initialise. `rule` says under which
	// TerrainCfg env e is built: *buf.tcfg (no table), table[env_terrain[e]] (terrain sets, include/dtrl.h dtrl_terrains_create ...), or -- with ladder records
	// (dtrl_terrain_ladder) -- table[its new level] after tg_ladder_step has moved env_terrain[e] and ladder[e] in front of the terrain work, in the same launch
	virtual bool TerrainBoundary(const DevBuffers& buf, const EnvSpan& span, int mode, const TerrainRule& rule);
	// where the default above sends the rule-less case (the batch's own terrain): a backend whose host addresses device memory runs tg_env_boundary in place (the
	// lane-loop check build); else the same host loop (TerrainBoundaryLoop: the body of both defaults). The engine calls the entry above only.
	virtual bool TerrainBoundary(const DevBuffers& buf, int e0, int n, int mode, const int32_t* env_list);
	bool TerrainBoundaryLoop(const DevBuffers& buf, const EnvSpan& span, int mode, const TerrainRule& rule);
	// Variant redraw (include/dtrl.h dtrl_variant_redraw; var_redraw_step): an env with status[e].need_reset & 1 whose variant is inside [cfg.lo, cfg.hi] draws;
	// env_model[e] and recs[e] move. cfg.cum is device memory too.
	virtual bool VariantRedraw(const EnvStatus* status, const EnvSpan& span, int32_t* env_model, RedrawRec* recs, const RedrawCfg& cfg);
	// Variant rescale (include/dtrl.h dtrl_variant_rescale; rescale_step): an env at an episode start -- status[e].need_reset & 1, or every env of the span with
	// status == nullptr (the listed form, dtrl_reset) -- whose key env_model[e] is its private one, key_base + e, has the mass and motor scalars of its private
	// record models[key_base + e] rewritten from the base scalars (device memory, one record) and its own draws; recs[e].episodes counts. Nothing else of the
	// record, and no other env's record, is touched. The default waits for the selected stream first.
	virtual bool VariantRescale(const EnvStatus* status, const EnvSpan& span, const int32_t* env_model, DevModel* models, int key_base, RescaleRec* recs, const ModelScalarsD* base, const RescaleCfg& cfg);
	// Push schedule (include/dtrl.h dtrl_push_schedule; push_step). status != nullptr: an env with status[e].need_reset != 0 starts an episode (its wait is drawn
	// afresh), any other counts down and is pushed at 0; status == nullptr: every env of the span starts (creation of the schedule, dtrl_reset, a terrain
	// restart). recs[e] and the seven slot fields of st[e] move; an env of scale[e] == 0 is not touched. The default waits for the selected stream first.
	virtual bool PushSchedule(const EnvStatus* status, const EnvSpan& span, EnvState* st, PushRec* recs, const double* scale, const PushCfg& cfg);
	// Episode limit (include/dtrl.h dtrl_episode_limit; episode_limit_step, episode_end). status != nullptr: every env of the span with on[e] != 0 counts the
	// boundary; one that fell has its episode recorded, one that reached its frame limit or the distance has need_reset written into status[e] and st[e] (with the
	// poli_eval episode bookkeeping frame_end() does for a fall), so that everything queued behind sees an env whose episode ended. status == nullptr: every env of
	// the span starts an episode (the limit is set, dtrl_reset, a terrain restart). recs[e] moves; an env with on[e] == 0 is not touched. The default waits for the
	// selected stream first (the lane-loop check build, DTRL_EPISODE_FALLBACK=1 on HIP); the HIP backend overrides it with one launch of dtrl_episode_limit.
	virtual bool EpisodeLimit(EnvStatus* status, const EnvSpan& span, EnvState* st, EpisodeRec* recs, const uint8_t* on, const EpisodeCfg& cfg);
	// Frame trace (include/dtrl.h dtrl_trace; trace_due / trace_value / trace_int). list[0 .. n) (device memory) are the traced indices t of one env group: each
	// of them whose env completed a frame writes one row -- the env's state and status record and its three keys as they stand -- into slot written[t] % frames of
	// its ring, then written[t] += 1. Reads state only; the ring and the counters are all it writes. The default waits for the selected stream first (the lane-loop
	// check build, DTRL_TRACE_FALLBACK=1 on HIP); the HIP backend overrides it with one launch of dtrl_trace_record, one wavefront per listed index.
	virtual bool TraceRecord(const EnvState* st, const EnvStatus* status, const TraceView& tv, const int32_t* list, int n);
	// The rings in chronological order: for i < n, with t = list[i] (memory host and device address: HostStaging()) and c = min(written[t], frames, max_rows),
	// counts[i] = c (HostStaging() memory) and rows r < c of slice i of vals_out [n][row_stride][W] / ints_out [n][row_stride][kTraceInts] = the env's last c rows,
	// oldest first; rows beyond c are not touched. The destination is memory the device addresses: device memory, or with dst_host HostStaging() memory (which the
	// default writes with plain stores). Queued on the selected stream and synchronised. Same default / override split, behind the same knob (dtrl_trace_gather).
	virtual bool TraceGather(const TraceView& tv, const int32_t* list, int n, int max_rows, int row_stride, double* vals_out, int32_t* ints_out, int32_t* counts, bool dst_host);
	// Episode log (include/dtrl.h dtrl_episode_log; log_count / log_row / log_start). status != nullptr: a frame boundary of the contiguous span [e0, e0 + n) of one
	// env group (no list) -- every env that completed a frame counts it in v.recs[e], and every one whose status record has need_reset != 0 appends a row to the
	// group's ring v.ring (page-locked host memory, `capacity` rows) in ascending env id behind v.cursor[0] rows written so far, at most the last `capacity` rows of
	// the boundary being stored; then the cursor words move: cursor[2] (the reservation) = cursor[0] + the boundary's rows in FRONT of the first row, and behind the
	// rows cursor[1] (the group's boundary counter) += 1, then cursor[0] += the boundary's rows. status == nullptr: the listed envs start an episode without a row. Reads state, status, the limit's records, the keys and the rescale's counters;
	// writes v.recs, the ring and the cursor pair alone. The default waits for the selected stream first (the lane-loop check build,
	// DTRL_EPISODE_LOG_FALLBACK=1 on HIP) and leaves the same bytes; the HIP backend overrides it with one launch of dtrl_episode_log (one workgroup) / dtrl_episode_log_start.
	virtual bool EpisodeLog(const EnvState* st, const EnvStatus* status, const EnvSpan& span, const LogView& v);
	// dtrl_add_perturb: rows[0 .. n) (device memory, at most one row per env: the row names its env, so there is no span) into the perturbation slots of
	// st[rows[i].env] (perturb_write_slot). The default copies each env's whole EnvState down, edits the seven fields and copies it back.
	virtual bool PerturbScatter(EnvState* st, const PerturbRow* rows, int n);
	// order[e0 .. e0 + n) = the envs e0 .. e0 + n - 1 sorted by status[].cost, costliest first (launch order of the group's next frame), on the selected stream
	virtual bool OrderByCost(const EnvStatus* status, int e0, int n, int32_t* order) = 0;
	// pending tuples -> block [block_rows + 1][W + 2] (header row + rows sorted by env id, flag word and global env id as the two extra columns); rows
	// beyond block_rows are carried (moved to the front of the ring, in order), drained / lost-to-a-full-ring totals accumulated in tuple_count[1], [2];
	// device pointers; queued on the selected stream and synchronised. n_envs = number of local envs (tuple_env values are < n_envs).
	virtual bool PackTuples(const DevBuffers& buf, float* block, int block_rows, int64_t env_id_base, int n_envs, const PackScratch& sc) = 0;
	// MarkFrame: remember the point behind everything queued so far on env group `group`'s stream under (group, slot); WaitFrames: the selected stream
	// waits (on the device, not the host) for the marks of `slot` of groups 0 .. n_groups - 1. Lets the tuple drain follow the frame that wrote its ring
	// when the host never synchronised with that frame (-terrain_gen= device). No-ops on a synchronous backend.
	virtual bool MarkFrame(int group, int slot) = 0;
	virtual bool WaitFrames(int slot, int n_groups) = 0;
	// MarkWeightReader: env group `group`'s latest launch reads weight buffer `wbuf` (0 / 1: the double-buffered policy hand-over) -- remember the point behind it;
	// WaitWeightReaders: `stream` (nullptr = the selected stream) waits on the device for every group's latest reader of `wbuf`, so that a gather INTO that
	// buffer cannot overtake a frame kernel still reading it (dtrl_step_poll relaunches, -terrain_gen= device frames the host never waited for). No-ops on a
	// synchronous backend.
	// the gather WITHOUT a host wait, on a stream of the caller's (required): src must stay unchanged until the work queued on that stream has passed this
	// point. Records the "policy ready" point behind it; WaitPolicyReady makes env group `group`'s stream wait for it on the device (the next frame launch
	// of a group must not start before the weights it will read are complete); SyncPolicyReady waits for it on the host. The synchronous test backend
	// performs the gather at once.
	virtual bool GatherF32Async(void* stream, float* dst, const float* src, const int32_t* idx, size_t n) { (void)stream; return GatherF32(dst, src, idx, n); }
	virtual bool WaitPolicyReady(int group) { (void)group; return true; }
	virtual bool SyncPolicyReady() { return true; }
	virtual bool MarkWeightReader(int group, int wbuf) { (void)group; (void)wbuf; return true; }
	virtual bool WaitWeightReaders(void* stream, int wbuf, int n_groups) { (void)stream; (void)wbuf; (void)n_groups; return true; }
	virtual bool Launch(const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end) = 0;
	virtual bool Sync() = 0;                 // all streams
	// work queues: H2D / H2DAsync / D2H / Launch act on the selected stream (0 by default); D2H and H2D synchronise only that stream
	virtual int NumStreams() const = 0;
	virtual void SelectStream(int sid) = 0;
	virtual bool StreamIdle(int sid) = 0;    // everything queued on the stream has completed
	virtual void KernelTime(double* avg_ms, int64_t* launches) = 0;
	virtual const char* Name() const = 0;
	const std::string& error() const { return err_; }
protected:
	std::string err_;
};
Backend* MakeBackend();   // resolved at link time: HIP in libdtrl.so, the lane-loop test backend under tests/emul/

// Header of an exported snapshot blob (dtrl_snapshot_export): [SnapHeader][int32 slot ids, padded to 8 bytes][device payload n x env_bytes][host payload n x host_bytes].
// dtrl_snapshot_import / dtrl_snapshot_restore compare every field up to `terrain_mode` with the batch and refuse a mismatch by name.
constexpr uint64_t kSnapMagic = 0x31504e534c525444ULL;   // "DTRLSNP1"
constexpr uint32_t kSnapVersion = 1;
struct SnapHeader {
	uint64_t magic;
	uint32_t version, header_bytes;
	uint32_t sizeof_real, sizeof_env_state, sizeof_ground_rec, sizeof_ground_gen, sizeof_env_status, sizeof_ground_host;
	int32_t char_type, ctrl_type, L, D, S, A, nn_out;
	int32_t terrain_mode;                      // 0 = host generator (GroundWindow records in the host payload), 1 = -terrain_gen= device (GroundGen in the device payload)
	uint32_t env_bytes, host_bytes;            // per env: device payload, host payload
	int32_t n_envs;
	int32_t policy_mode;                       // 0 = internal, 1 = -policy_mode= external (the device payload then ends with the env's ExtAction record); was padding: older blobs read as internal
};
static_assert(sizeof(SnapHeader) % 8 == 0, "the payload behind the header is copied as 64-bit words");
class Engine;
struct Snapshot {
	SnapHeader hdr{};
	std::vector<int32_t> ids;     // the slots the envs were saved from
	char* payload = nullptr;      // device memory [n][env_bytes], owned by `owner`'s backend
	std::vector<char> host;       // [n][host_bytes]: the host generator's windows (host terrain mode)
	Engine* owner = nullptr;      // the batch that holds the payload; nullptr once that batch is gone
};

class Engine {
public:
	Engine() {}
	// external policy mode (include/dtrl.h)
	bool external() const { return cfg_.external_policy; }
	int PendingActions(int32_t* env_ids, void* states, int cap, int* out_n, bool device);
	int SupplyActions(const int32_t* env_ids, int n, const int32_t* action_ids, const void* params, const uint32_t* flags, bool device, int* rejected);
	int ExtStats(int64_t* awaiting, int64_t* ready, int64_t* env_steps_total, int64_t* env_frames_total);
	int ExtEnvInfo(const int32_t* env_ids, int n, int32_t* park, int32_t* steps_left);
	double ExtLaunchMs(int which) { return be_ ? be_->ExtLaunchMs(which) : -1.0; }
	// env snapshots (include/dtrl.h)
	int SnapshotSave(const int32_t* env_ids, int n, Snapshot** out);
	int SnapshotRestore(const Snapshot* s, const int32_t* env_ids, int n);
	int CloneEnvs(const int32_t* src_ids, const int32_t* dst_ids, int n);
	int SnapshotExport(const Snapshot* s, void* buf, size_t cap, size_t* bytes);
	int SnapshotImport(const void* blob, size_t bytes, Snapshot** out);
	void SnapshotRelease(Snapshot* s);
	double SnapLaunchMs() { return be_ ? be_->SnapLaunchMs() : -1.0; }
	// policy slots (include/dtrl.h)
	int SlotsCreate(int n_slots);
	int SlotSetPolicy(int slot, const float* w, size_t n, const double* io, const double* is, const double* oo, const double* os, bool device);
	int SlotAlias(int slot, int src_slot);
	int SlotSetExplore(int slot, int enable, double rate, double temp, double base_rate);
	int AssignSlots(const int32_t* env_ids, int n, const int32_t* slots) { return KeysAssign(slot_keys_, "dtrl_assign_slots", env_ids, n, slots); }
	int GetSlots(const int32_t* env_ids, int n, int32_t* slots_out) { return KeysGet(slot_keys_, "dtrl_get_slots", env_ids, n, slots_out); }
	// (the one asymmetry of the two families: dtrl_slot_stats WAITS for a frame in flight, dtrl_variant_stats REFUSES one -- DESIGN 6d)
	int SlotStats(int slot, int64_t* n_envs, double* avg_dist, int64_t* episodes, int64_t* cycles, int64_t* resets) { return KeysStats(slot_keys_, "dtrl_slot_stats", true, slot, n_envs, avg_dist, episodes, cycles, resets); }
	// model variants (include/dtrl.h)
	int VariantsCreate(int n_variants);
	int VariantLoad(int v, const char* character_file, const char* text, size_t bytes);   // text == nullptr: the file, resolved like -character_file=
	int AssignVariants(const int32_t* env_ids, int n, const int32_t* variants);
	int GetVariants(const int32_t* env_ids, int n, int32_t* variants_out);
	// variant redraw (include/dtrl.h)
	int VariantRedraw(int lo, int hi, uint64_t seed, const double* weights);
	int VariantRedrawInfo(const int32_t* env_ids, int n, int32_t* lo, int32_t* hi, int32_t* variant, int32_t* draws);
	// variant rescale (include/dtrl.h)
	int VariantRescale(int base, const int32_t* env_ids, int n, uint64_t seed, const double* lo4, const double* hi4, uint32_t per_link, bool remove);
	int VariantRescaleInfo(const int32_t* env_ids, int n, int32_t* base, uint64_t* seed, double* lo4, double* hi4, uint32_t* per_link, int32_t* key, int32_t* episodes, double* factors);
	int VariantScalars(int env, double* out6L, double* total_mass);
	int VariantStats(int v, int64_t* n_envs, double* avg_dist, int64_t* episodes, int64_t* cycles, int64_t* resets) { return KeysStats(variant_keys_, "dtrl_variant_stats", false, v, n_envs, avg_dist, episodes, cycles, resets); }
	int num_variants() const { return static_cast<int>(var_models_.size()); }
	// terrain sets (include/dtrl.h)
	int TerrainsCreate(int n_terrains);
	int TerrainSetFile(int t, const char* terrain_file, double lerp);
	int TerrainSetParams(int t, const char* type_name, const double* params40);
	int TerrainInfo(int t, char* type_out, int type_cap, double* params40_out, int* filled_out);
	int AssignTerrains(const int32_t* env_ids, int n, const int32_t* terrains, bool restart);
	int GetTerrains(const int32_t* env_ids, int n, int32_t* terrains_out);
	// terrain ladder (include/dtrl.h)
	int TerrainLadder(int lo, int hi, double up_dist, double down_dist, int at_top);
	int LadderInfo(const int32_t* env_ids, int n, double* mark_x_out, int32_t* ups_out, int32_t* downs_out);
	int TerrainStats(int t, int64_t* n_envs, double* avg_dist, int64_t* episodes, int64_t* cycles, int64_t* resets) { return KeysStats(terrain_keys_, "dtrl_terrain_stats", false, t, n_envs, avg_dist, episodes, cycles, resets); }
	int num_terrains() const { return terrain_keys_.n_keys(); }
	// the model env e (local id, in range) runs under: what host-side readers of per-env geometry use (dtrl_get_link_states, AddPerturb). With a redraw on device
	// terrain the caller brings the host keys up to date first (VariantKeysCurrent, once per call, behind a wait for the streams)
	int VariantKeysCurrent() { return KeysRefresh(variant_keys_); }
	// (an env under its private record of the variant rescale: the rescale's base -- geometry is not scaled)
	const DevModel& ModelOf(int e) const { return var_models_.empty() ? cfg_.model : var_models_[PublicKey(variant_keys_.env_key[e])]; }
	~Engine();
	int Create(const char* const* argv, int argc, int num_envs, int device_id);
	int Reset(const int32_t* env_ids, int n, const uint64_t* seeds);
	int Step(double dt);
	int StepBegin(double dt);
	int StepEnd();
	int StepUpdates(int n);
	int RunFrames(int frames, double dt);
	int SetPolicy(const float* w, size_t n, const double* io, const double* is, const double* oo, const double* os);
	int LoadScaleFile(const char* path);
	int WriteScaleFile(const char* path);
	int SetExplore(int enable, double rate, double temp, double base_rate);
	int SetTerrainLerp(double lerp);
	int DrainTuples(float* rows, uint32_t* flags, int32_t* env_ids, int cap, int* out_n, bool device_dst = false);
	int TupleStats(int64_t* pending, int64_t* drained, int64_t* dropped, int32_t* capacity);
	int GetDistLog(double* dist, int32_t* env_ids, int cap, int* out_n);
	int ResetAvgDist();
	int SetPolicyDevice(const float* w_dev, size_t n, const double* io_dev, const double* is_dev, const double* oo_dev, const double* os_dev, void* stream = nullptr);
	int SetPolicyDeviceAsync(const float* w_dev, size_t n, void* stream);
	int GetStates(const int32_t* env_ids, int n, std::vector<EnvState>& out);
	int SetPoseVel(const int32_t* env_ids, int n, const double* q, const double* qd);
	int GetContactCache(const int32_t* env_ids, int n, int32_t* count, int32_t* ids, double* lambda);
	int SetContactCache(const int32_t* env_ids, int n, const int32_t* count, const int32_t* ids, const double* lambda);
	int CommandAction(const int32_t* env_ids, int n, const int32_t* action_ids);
	void ApplyPendingPolicy();
	void* SideStream(int k, double* delay_us) { void* s = be_ ? be_->SideStream(k) : nullptr; if (delay_us) *delay_us = be_ ? be_->SideStreamDelayUs(k) : -1.0; return s; }
	int AddPerturb(const int32_t* env_ids, int n, const int32_t* link, const double* local_pos, const double* force, const double* duration);
	// push schedule (include/dtrl.h)
	int PushSchedule(int min_wait, int max_wait, uint64_t seed, double min_force, double max_force, double min_dur, double max_dur);
	int PushScale(const int32_t* env_ids, int n, const double* scales);
	int PushInfo(const int32_t* env_ids, int n, int32_t* wait, int32_t* pushes, int32_t* last_link, double* last_force, double* last_dur);
	// episode limit (include/dtrl.h)
	int EpisodeLimit(int min_frames, int max_frames, double max_dist, uint64_t seed);
	int EpisodeLimitEnvs(const int32_t* env_ids, int n, const uint8_t* on);
	int EpisodeInfo(const int32_t* env_ids, int n, int32_t* frames, int32_t* limit, int64_t* by_fall, int64_t* by_limit, int32_t* last_frames, double* last_dist, int32_t* last_cause);
	// frame trace (include/dtrl.h)
	int Trace(const int32_t* env_ids, int n, int frames);
	int TraceInfo(int32_t* n_traced, int32_t* frames, int32_t* width, int32_t* env_ids_out, int64_t* rows_written_out);
	int TraceRead(const int32_t* env_ids, int n, int max_rows, double* vals, int32_t* ints, int32_t* counts, bool device);
	// episode log (include/dtrl.h)
	int EpisodeLog(int capacity);
	int EpisodeLogInfo(int32_t* capacity, int32_t* n_groups, int64_t* written, int64_t* lost);
	int EpisodeLogDrain(void* out /* [max_rows] LogRow */, int max_rows, int32_t* n_out, int64_t* lost);
	int VariantRescaleFactors(const int32_t* env_ids, const int32_t* draws, int n, double* factors);
	int ApplyRandForce(const int32_t* env_ids, int n, uint64_t seed);
	int GetPoliState(const int32_t* env_ids, int n, double* s);
	int GetPolicyOutput(const int32_t* env_ids, int n, double* y);
	int GroundWindowRec(int env, int32_t* w2, double* min_x2, double* max_x2, float* h0, float* h1, int cap, int64_t* num_builds);
	int DrainTuplesPacked(float* block_dev, int block_rows, int* out_n);
	int SetTuplePipelining(bool on);
	int StepEndBegin(double dt);
	int StepPoll(double dt, int* relaunched);
	int SampleGround(int env, int n, const double* x, double* h, int32_t* seg, int32_t* oi, int32_t* oj);
	int EvalStats(double* avg_dist, int64_t* episodes, int64_t* cycles, int64_t* resets);
	int KernelTime(double* avg_ms, int64_t* launches);
	int ProfileSections(unsigned long long* out, int cap);
	int ProfileEnv(int section, unsigned long long* out, int cap);   // summed s_memtime ticks per kernel section (DTRL_PROFILE builds)

	const ScenarioConfig& cfg() const { return cfg_; }
	int num_envs() const { return n_; }
	int S() const { return S_; }
	int A() const { return A_; }
	const std::string& error() const { return err_; }
	void set_error(const std::string& e) { err_ = e; }

private:
	int Fail(int code, const std::string& msg) { err_ = msg; return code; }
	int HostFrameWork(int group);
	int FoldTupleTotals();
	int DeviceFrameWork(int group);   // -terrain_gen= device: the same frame-boundary work queued as device kernels, no host sync
	int DrainDeviceDistLog();
	int UploadTerrainCfg(const double* params);
	TerrainCfg MakeTerrainCfg(int type, const double* params) const;   // the scene constants of a TerrainCfg are the batch's
	// -terrain_gen= device: the boundary work of every caller, under the rule in force -- the batch's own terrain, once terrains exist the env's table entry, with a
	// ladder its rule in front of that (which moves the device keys and records: the host copies go stale)
	bool Boundary(const EnvSpan& span, int mode)
	{
		TerrainRule r;
		if (!terrain_keys_.filled.empty()) { r.table = d_terrain_table_; r.env_terrain = terrain_keys_.d_env_key; }
		if (ladder_on_) { r.ladder = ladder_.dev; r.lc = ladder_cfg_; terrain_keys_.stale = true; }
		return be_->TerrainBoundary(buf_, span, mode, r);
	}
	// The one place an env list is laid out for the device: `ids` into the id staging at `off`, uploaded on the selected stream unless the device reads the staging
	// itself (zero_copy_). Returns the list as the device reads it -- what every listed launch and rule of the call is handed -- or nullptr with the error set
	const int32_t* StageIds(const std::vector<int32_t>& ids, int off = 0);
	int ApplyResets(const std::vector<int32_t>& ids, int group, const int32_t* staged = nullptr);   // the reset launch; staged: StageIds(ids) of a user reset (group < 0)
	// The per-env rules of the frame boundary, each queued where it is in force (else nothing) on the selected stream; false: the backend's error. status: the
	// span's envs whose episode ended act (a frame boundary), or nullptr: every env of the span starts an episode (the listed form and the rule's creation).
	bool EpisodeQueue(EnvStatus* status, const EnvSpan& span) { return !episode_on_ || be_->EpisodeLimit(status, span, buf_.st, episode_.dev, episode_flag_.dev, episode_cfg_); }
	bool RedrawQueue(const EnvSpan& span) { if (!redraw_on_) return true; variant_keys_.stale = true; return be_->VariantRedraw(buf_.status, span, variant_keys_.d_env_key, redraw_.dev, redraw_cfg_); }   // (device terrain)
	bool RescaleQueue(const EnvStatus* status, const EnvSpan& span) { return !rescale_on_ || be_->VariantRescale(status, span, variant_keys_.d_env_key, d_var_models_, static_cast<int>(var_models_.size()), rescale_.dev, d_rescale_base_, rescale_cfg_); }
	bool PushQueue(const EnvStatus* status, const EnvSpan& span) { return !push_on_ || be_->PushSchedule(status, span, buf_.st, push_.dev, push_scale_.dev, push_cfg_); }
	// THE ORDER OF THE RULES, at a frame boundary and at a listed episode start alike:
	//   episode limit, trace, log | terrain work (with the ladder) | redraw, rescale, push | reset launch                  a frame boundary of a group's span
	//                               terrain work (with the ladder) | redraw, rescale | reset launch | push, episode, log   the listed envs start an episode
	// The limit comes first: for every other rule an env it ended is an env whose episode ended. The trace comes right behind it and in front of everything that moves
	// a key or resets an env: a row holds the state its frame ended in, the need_reset every later rule sees and the keys the frame ran under; a listed episode start
	// writes no row. The episode log comes behind the trace and, like it, in front of everything that moves a key or redraws a scale: a row shows the cause the limit
	// recorded, the keys and the draw the episode ran under; its listed form (the running episode is abandoned without a row) comes behind the reset launch. Redraw and rescale come in front of the reset launch, which runs
	// reset_env under the new model, the rescale behind the redraw (which acts on keys below V only). At a boundary the push comes in front of the reset launch (an
	// env that fell draws a new wait and is not pushed; the launch clears nothing the rule wrote); the listed starts of push and limit come behind it.
	bool TraceQueue(int group);   // (dtrl_engine.cpp) the group's traced envs write their rows; a group without one queues nothing
	bool LogQueue(const EnvStatus* status, const EnvSpan& span, int group);   // (dtrl_engine.cpp) the group's ended episodes append their rows (status == nullptr: the listed form; group: whose ring)
	bool RulesBehindFrame(int group) { const Group& g = groups_[group]; const EnvSpan span{g.e0, g.n, nullptr}; return EpisodeQueue(buf_.status, span) && TraceQueue(group) && LogQueue(buf_.status, span, group); }   // behind a group's frame launch, in front of everything that reads its status
	bool RulesBeforeResets(const EnvSpan& span) { return (!cfg_.device_terrain || RedrawQueue(span)) && RescaleQueue(buf_.status, span) && PushQueue(buf_.status, span); }   // (host terrain: the host status loop has run the redraw)
	// "These envs start an episode now" (dtrl_reset: draw_models; a terrain restart: not), synchronised: the list staged once, with -terrain_gen= device the listed envs'
	// terrain work under terrain_mode (Boundary: 1 = initialise, 2 = re-seed + initialise), then the second line above
	int StartEpisodes(const std::vector<int32_t>& ids, bool draw_models, int terrain_mode);
	int LaunchGroup(int group, int n_steps, double dt_step, bool frame_end);
	// env groups: contiguous env ranges, each with its own stream, launch order and staging slices. Envs are independent, so a group
	// starts its next frame as soon as ITS host work is done instead of waiting for the slowest wavefront of the whole batch
	struct Group { int e0 = 0, n = 0; };
	std::vector<Group> groups_;
	int32_t* d_env_list_ = nullptr;
	int32_t* d_order_ = nullptr;         // launch order of the full-batch frame launches (costliest env first)
	std::vector<int32_t> reset_ids_;
	bool UploadGround(int env);
	bool FetchGroundRec(int env);
	int EnvIndex(const int32_t* env_ids, int i) const { return env_ids ? env_ids[i] : i; }
	// the env list of a per-env getter or setter: DTRL_ERR_ARG unless n is 0 .. num_envs (and `required`, the call's array `name`, is there when n > 0) and every id
	// is in range. w: the call's prefix "dtrl_xxx: "; tail: what a refused setter adds ("; nothing changed")
	int CheckEnvList(const std::string& w, const int32_t* env_ids, int n, const char* tail = "", const char* name = nullptr, const void* required = nullptr);
	int DevOk(bool ok);   // DTRL_OK, or DTRL_ERR_DEVICE with the backend's error text

	ScenarioConfig cfg_;
	Backend* be_ = nullptr;
	int n_ = 0, S_ = 0, A_ = 0, W_ = 0;
	bool policy_set_ = false;
	std::vector<char> early_; bool early_any_ = false;   // env groups dtrl_step_poll has relaunched ahead of the next dtrl_step_end_begin
	float* weights_alt_ = nullptr; const float* weights_buf0_ = nullptr; bool policy_flip_pending_ = false;
	std::vector<char> policy_wait_;   // per env group: its next launch waits (on the device) for the asynchronous hand-over's gather   // SetPolicyDevice during a frame: gathered here, switched in with the next launch
	bool step_pending_ = false;
	DevModel* d_model_ = nullptr;
	DevBuffers buf_{};
	std::vector<void*> allocs_;
	std::vector<GroundWindow> grounds_;
	EnvStatus* status_ = nullptr;   // page-locked; in host terrain mode the frame kernel writes it directly (zero_copy_), else the per-frame read-back lands here
	int32_t* stage_slot_ = nullptr;  // page-locked [n]: slot + 1 of the env's regenerated terrain record in pin_recs_, 0 = none (cleared by the env's wavefront)
	bool zero_copy_ = false;        // host terrain mode: status, launch order, reset lists and terrain records cross the boundary without a copy (dtrl_engine.cpp Init)
	GroundRec tmp_rec_;
	TerrainCfg* d_tcfg_ = nullptr;
	PackScratch pack_;                  // allocated by the first packed drain
	static constexpr int kDistRingCap = 1 << 20;
	bool D2HReal(double* dst, const real* src, size_t n);
	std::vector<double> in_off_, in_scale_, out_off_, out_scale_;   // host copies of the policy normalisers (identity until set)
	int UploadNormalizers();
	void BuildRelayoutMap(std::vector<int32_t>& map) const;
	std::vector<int32_t> relayout_;
	// page-locked staging for the per-frame uploads (terrain records, launch order, reset list): the copies are queued on the
	// stream without a host sync; the arena is recycled after the next frame's status read-back (a stream sync)
	char* pin_drain_ = nullptr; size_t pin_drain_bytes_ = 0;   // page-locked staging of dtrl_drain_tuples (count word + rows + flags + env ids)
	GroundRec* pin_recs_ = nullptr;
	int32_t* pin_order_ = nullptr; int32_t* pin_ids_ = nullptr;
	std::vector<int32_t> bucket_;
	std::vector<std::pair<int32_t, double>> dist_log_;   // (env, distance) of every recorded poli_eval episode, in completion order
	int64_t tuples_drained_ = 0, tuples_dropped_ = 0;
	// tuple pipelining (dtrl_set_tuple_pipelining): two tuple rings; every dtrl_step_begin switches the ring the kernels write, so the frame that
	// has just ended can be drained on its own stream while the next frame already runs
	struct TupleRing { float* rows = nullptr; uint32_t* flags = nullptr; int32_t* env = nullptr; int32_t* count = nullptr; };
	TupleRing ring_[2];
	std::vector<void*> host_allocs_;   // page-locked ring storage (-tuple_ring= host)
	bool AllocRing(TupleRing& r);
	bool RingRead(void* dst, const void* src, size_t n);
	bool RingWrite(void* dst, const void* src, size_t n);
	int wr_ring_ = 0;
	bool tuple_pipelining_ = false;
	void UseRing(DevBuffers& b, int r) const { b.tuple_rows = ring_[r].rows; b.tuple_flags = ring_[r].flags; b.tuple_env = ring_[r].env; b.tuple_count = ring_[r].count; }
	int DrainRing() const { return (tuple_pipelining_ && step_pending_) ? (wr_ring_ ^ 1) : wr_ring_; }   // the ring no kernel is writing
	int DrainFail(); bool drain_order_error_ = false;
	bool DrainSync();   // make the drain ring's contents final: all streams, or -- while a pipelined frame runs -- only the drain stream
	int PendingTuples(int32_t* stored, int32_t* overflow);
	std::vector<int32_t> work_;
	// snapshots
	int RequireIdle(const std::string& refusal, bool drain = true);   // DTRL_ERR_ARG (`refusal`) while a frame is in flight; else, with `drain`, waits for every stream
	int SnapReady(const char* what);                       // RequireIdle, and the id staging exists
	SnapPlan MakeSnapPlan() const;
	SnapHeader MakeSnapHeader(int n) const;
	int CheckSnapHeader(const SnapHeader& h, const char* what);
	int CheckSlots(const int32_t* ids, int n, const char* what);   // in range and distinct
	Snapshot* NewSnapshot(int n);
	int32_t* snap_ids_ = nullptr;                          // page-locked [2 n]: the env lists the transport kernels read
	char* snap_scratch_ = nullptr;                         // device [n][env_bytes]: staging of a clone whose lists overlap (allocated on first use)
	std::vector<Snapshot*> snapshots_;                     // live snapshots whose payload this batch holds
	// external policy mode: scratch of the hand-over calls
	int ExtRefuse(const char* what);                       // DTRL_ERR_ARG unless the batch is in external mode and no step is pending
	int32_t* ext_meta_ = nullptr;                          // page-locked {m, awaiting, ready, 0}
	int32_t* d_ext_ids_ = nullptr;                         // device [n]
	double* d_ext_states_ = nullptr;                       // device [n][S] (host call)
	int32_t* d_ext_action_ids_ = nullptr; uint32_t* d_ext_flags_ = nullptr; double* d_ext_params_ = nullptr;   // device [n], [n], [n][n_opt]: the rows of a host call
	// Per-env keys: what policy slots, model variants and terrain sets share (slots and variants exclude each other; terrains combine with either). A key is a slot, a variant or a terrain number; every env starts under
	// key 0. The family's table and the per-env array are read by launches in flight and are therefore rewritten only by calls that have refused a frame in flight and
	// waited for every stream (KeysIdle). The three texts are the family's own words in the refusals (they differ in more than the noun).
	// WHO OWNS THE KEYS. The host array is the truth and the device array its copy (KeysAssign uploads it) -- also under a frame-boundary rule that moves keys
	// (terrain ladder, variant redraw) in host terrain mode, where HostFrameWork runs the rule and uploads the group's slice. With such a rule and -terrain_gen=
	// device the rule's kernel moves the DEVICE keys and the rule's device records (`recs`) while frames run (on_device): whoever queues such a launch sets `stale`,
	// and every call that reads or uploads the keys or the records first waits for every stream and brings both host copies up to date (KeysCurrent, or KeysRefresh
	// behind a wait of the caller's own), which clears it.
	struct RecsBase { virtual ~RecsBase() {} virtual bool Pull(Backend& be) = 0; };
	struct EnvAssignment {
		const char* noun; const char* none_text; const char* empty_text;
		std::vector<char> filled;                // per key: it may be assigned. Empty: the family was not created, every launch is Backend::Launch as it always was
		std::vector<int32_t> env_key;            // host form of the per-env array
		int32_t* d_env_key = nullptr; int32_t* part = nullptr;   // device array [n], page-locked [2 n] (the scratch of the per-key default's list split)
		bool on_device = false, stale = false; RecsBase* recs = nullptr;   // a rule moves the keys on the device / has been queued since the last refresh / its records
		int n_keys() const { return static_cast<int>(filled.size()); }
		EnvKeyView View(const int32_t* list_host, int part_off) const { EnvKeyView v; v.n_keys = n_keys(); v.env_key_dev = d_env_key; v.env_key_host = env_key.data(); v.keys_on_device = on_device; v.env_list_host = list_host; v.part = part + part_off; return v; }
	};
	// The per-env records of a frame-boundary rule: a device array [count] and a host form, which is the truth without a device array (a rule the host runs),
	// its copy with one, or only the staging of Pull / Push (records that live on the device alone)
	template <class Rec> struct RuleRecs : RecsBase {
		std::vector<Rec> host; Rec* dev = nullptr; size_t count = 0;
		bool Alloc(Backend& be, size_t n, std::vector<void*>& owner)   // once; zero-filled
		{
			if (dev) return true;
			dev = static_cast<Rec*>(be.Alloc(sizeof(Rec) * n));
			if (dev) { owner.push_back(dev); count = n; }
			return dev != nullptr;
		}
		bool Pull(Backend& be) override { if (!dev) return true; host.resize(count); return be.D2H(host.data(), dev, sizeof(Rec) * count); }   // host <- device, all of it
		bool Push(Backend& be) { return !dev || be.H2D(dev, host.data(), sizeof(Rec) * host.size()); }                                         // device <- host, as far as the host form goes
	};
	template <class Rec> int RecsAlloc(RuleRecs<Rec>& r, size_t n);   // (dtrl_engine.cpp) the device array, once
	template <class Rec> int RecsAlloc(RuleRecs<Rec>& r, size_t n, const Rec& fill);   // the same, and on that first call the host form filled with `fill` and pushed
	// The opening of a rule's info and per-env settings calls, in this order: refuse a frame in flight and wait for every stream (RequireIdle; with `keys` the
	// family's KeysIdle), refuse with `no_rule` (nullptr: the rule is there), bring the keys and records a device rule moves up to date (KeysRefresh, with `keys`),
	// check the env list, and pull `recs` (nullptr: nothing)
	struct EnvListArg { const int32_t* ids; int n; const char* tail = ""; const char* name = nullptr; const void* required = nullptr; };   // (CheckEnvList's arguments)
	int RuleCallBegin(const char* what, EnvAssignment* keys, const char* no_rule, const EnvListArg& list, RecsBase* recs);
	int KeysRefresh(EnvAssignment& a);       // on_device and stale: host keys and the rule's records <- device (call with the streams idle); else nothing
	// KeysIdle + KeysRefresh for an assignment whose keys move on the device; else nothing (`always`: KeysIdle even so -- the ladder's calls, in either terrain mode)
	int KeysCurrent(EnvAssignment& a, const char* what, bool always = false);
	void* KeysAllocate(EnvAssignment& a, size_t table_bytes);   // the family's device table (returned; nullptr: failed, error set), the per-env array and the scratch
	// DTRL_ERR_ARG without keys / key out of range / frame in flight, else every stream idle. wait_in_flight (dtrl_slot_stats alone): a frame in flight is waited for
	int KeysIdle(const EnvAssignment& a, const char* what, int key, bool wait_in_flight = false);
	int KeysAssign(EnvAssignment& a, const char* what, const int32_t* env_ids, int n, const int32_t* keys);   // all or nothing
	int KeysGet(const EnvAssignment& a, const char* what, const int32_t* env_ids, int n, int32_t* keys_out);
	int KeysStats(const EnvAssignment& a, const char* what, bool wait_in_flight, int key, int64_t* n_envs, double* avg_dist, int64_t* episodes, int64_t* cycles, int64_t* resets);
	// policy slots. Slot 0 is the batch's policy (buf_'s five pointers, cfg_.run's exploration); a slot >= 1 owns storage (weights) or is an alias (alias >= 0) or is empty
	struct SlotHost { float* weights = nullptr; real* norm[4] = {nullptr, nullptr, nullptr, nullptr}; int alias = -1; int enable_exp = 0; double rate = 0, temp = 1, base_rate = 0; };
	EnvAssignment slot_keys_{"slot", "the batch has no policy slots (call dtrl_slots_create first)", "is empty (it has neither a policy nor an alias)"};
	std::vector<SlotHost> slots_;            // empty: no slots
	std::vector<SlotRec> slot_table_; SlotRec* d_slot_table_ = nullptr;   // the table: host form, device memory [n_slots]
	int SlotRoot(int slot) const { while (slots_[slot].alias >= 0) slot = slots_[slot].alias; return slot; }
	int UploadSlotTable();
	// every frame-kernel launch of the batch: Backend::Launch, or -- once slots or variants exist -- Backend::LaunchKeyed. list_host: b.env_list in host-readable
	// form or nullptr; part_off: offset of the launch's scratch inside the family's `part`
	bool LaunchEnvs(const DevBuffers& b, int n_envs, int n_steps, real dt, bool frame_end, const int32_t* list_host, int part_off);
	// model variants. Variant 0 is the batch's own model; a variant >= 1 is empty until dtrl_variant_load_* fills it
	ArgParser args_;                         // the creation arguments (command line + arg file): a variant is loaded through them with another character description
	EnvAssignment variant_keys_{"variant", "the batch has no model variants (call dtrl_variants_create first)", "is empty (no dtrl_variant_load_* has filled it)"};
	std::vector<DevModel> var_models_; DevModel* d_var_models_ = nullptr;   // the table: host form (empty: no variants), device memory [n_variants]
	// terrain sets. Terrain 0 is the batch's terrain (cfg_.terrain_type / terrain_param_sets at terrain_lerp_: what dtrl_set_terrain_lerp moves); a terrain >= 1 is
	// empty until dtrl_terrain_set_* fills it. No frame launch reads the table: the consumers are the frame-boundary paths (host: each env's GroundWindow carries its
	// terrain's type and parameters; device: Backend::TerrainBoundary), so terrains combine with slots, variants and external policy mode
	struct TerrainSource { std::vector<std::vector<double>> sets; double lerp = 0; };   // where a terrain's parameters came from (a file's sets; empty: given directly)
	EnvAssignment terrain_keys_{"terrain", "the batch has no terrain sets (call dtrl_terrains_create first)", "is empty (no dtrl_terrain_set_file / dtrl_terrain_set_params has filled it)"};
	std::vector<TerrainCfg> terrain_table_; TerrainCfg* d_terrain_table_ = nullptr;   // the table: host form (empty: no terrains), device memory [n_terrains]
	std::vector<TerrainSource> terrain_src_;
	double terrain_lerp_ = 0;                // terrain 0's lerp in force
	int TerrainFill(const char* what, int t, int type, const double* params);   // table entry t (>= 1) in both forms, and the windows of the envs under it
	// terrain ladder and variant redraw: settings and per-env records are batch state, like the assignment whose keys the rule moves (see EnvAssignment for who owns
	// keys and records when). The records' host form is kept when the rule is replaced or removed.
	bool ladder_on_ = false;
	LadderCfg ladder_cfg_{};
	RuleRecs<LadderRec> ladder_;             // device array with -terrain_gen= device (allocated by the first ladder)
	int RootX(int e, double* x);             // env e's current root x (q[0] of its state record; call with the streams idle)
	bool redraw_on_ = false;
	RedrawCfg redraw_cfg_{};                 // (cum: the DEVICE table)
	RuleRecs<RedrawRec> redraw_;             // device array with -terrain_gen= device (allocated by the first redraw)
	RuleRecs<double> redraw_cum_;            // the cumulative table: host form [hi - lo + 1], device [n_variants]
	int RedrawListed(const std::vector<int32_t>& ids);
	// variant rescale: settings, counters and the per-env private records are batch state. The private records are records V .. V + num_envs - 1 of the device
	// table (V = n_variants; the table is grown once, by the first dtrl_variant_rescale, with the streams idle); env e's private key is V + e. The host table
	// var_models_ keeps its V records: a private key stands for the rescale's base wherever the host reads a model (PublicKey). The DEVICE counters and records are
	// the truth in both terrain modes: the rule runs in Backend::VariantRescale on the group's stream at every frame boundary, between the group's frame launch and
	// its reset launch, and nothing else writes a record while launches run -- stream order is the whole timing rule.
	bool rescale_on_ = false, rescale_table_ = false;   // (rescale_table_: the device table holds the private records)
	int rescale_base_ = 0;
	RescaleCfg rescale_cfg_{};
	RuleRecs<RescaleRec> rescale_;           // device [n] (allocated by the first dtrl_variant_rescale)
	std::vector<ModelScalarsD> var_scalars_; // per variant: the character file's doubles (empty: no variants)
	ModelScalarsD* d_rescale_base_ = nullptr;   // device: the base's copy
	int32_t PublicKey(int32_t k) const { return k >= static_cast<int32_t>(var_models_.size()) ? rescale_base_ : k; }
	// push schedule: settings, per-env records and per-env scales are batch state. The DEVICE records and scales are the truth in both terrain modes (the host form
	// is staging): the rule runs in Backend::PushSchedule on the group's stream at every frame boundary, and the calls that read the records wait for queued work
	bool push_on_ = false;
	PushCfg push_cfg_{};
	RuleRecs<PushRec> push_; RuleRecs<double> push_scale_;   // device [n] each (allocated by the first dtrl_push_schedule / dtrl_push_scale; scales 1.0)
	RuleRecs<PerturbRow> pert_rows_;                         // device [n]: the rows of one dtrl_add_perturb (allocated by the first call)
	int PushAlloc();                                               // the two push arrays, once
	// episode limit: settings, per-env records and per-env flags are batch state. The DEVICE records and flags are the only copy in both terrain modes (the host
	// form is staging): the rule runs in Backend::EpisodeLimit on the group's stream in front of every other boundary rule (RulesBehindFrame) -- first in DeviceFrameWork
	// (-terrain_gen= device), behind the group's frame launch in LaunchGroup (host terrain: the wait HostFrameWork makes anyway covers it, and its loop reads the amended status)
	bool episode_on_ = false;
	EpisodeCfg episode_cfg_{};
	RuleRecs<EpisodeRec> episode_; RuleRecs<uint8_t> episode_flag_;   // device [n] each (allocated by the first dtrl_episode_limit / dtrl_episode_limit_envs; flags 1)
	int EpisodeAlloc();                                              // the two arrays, once
	// frame trace: the rings, the per-env counters and the per-group lists of traced indices are batch state and live in device memory only (snapshots, restores,
	// clones, blobs and resets leave them alone). The rule runs in Backend::TraceRecord on the group's stream right behind the episode limit (RulesBehindFrame), in
	// both terrain modes; dtrl_trace replaces all of it with the streams idle, so stream order is the whole timing rule.
	struct TraceState {
		TraceView v{};                           // (the three key arrays are filled in when a launch is queued: a family may be created after the trace)
		std::vector<int32_t> ids, index_of;      // traced index -> env id (the caller's order); env id -> traced index or -1
		std::vector<int32_t> group_off, group_n; // per env group: its slice of d_list
		int32_t* d_env_of = nullptr; int32_t* d_list = nullptr;   // device [n_traced] each: env_of, and the traced indices regrouped by env group
	} trace_;
	char* trace_stage_ = nullptr; size_t trace_stage_bytes_ = 0;   // page-locked staging of the two reads (list, counts and -- dtrl_trace_read -- the rows), grown on demand
	void TraceFree();
	// episode log: one ring of `capacity` rows per env group with its four cursor words {written, boundary, reserved, 0}, all in page-locked host memory the device writes (a drain
	// queues nothing), and the per-env records in device memory (the only copy). Batch state: snapshots, restores, clones, blobs and resets leave it alone. The rule
	// runs in Backend::EpisodeLog on the group's stream behind the limit and the trace (RulesBehindFrame), in both terrain modes; dtrl_episode_log sets, replaces and
	// removes all of it with the streams idle, so stream order is the whole timing rule. drained / lost: per group, rows handed to the caller or found overwritten.
	struct LogState { int32_t capacity = 0; LogRow* rings = nullptr; int64_t* cursors = nullptr; std::vector<int64_t> drained, lost; } log_;
	RuleRecs<LogRec> log_recs_;              // device [n] (allocated by the first dtrl_episode_log)
	std::vector<LogRow> log_stage_;          // the rows a drain has copied out of the rings, before the merge
	void LogFree();
	int32_t* d_relayout_ = nullptr;   // device weight index -> index into the caller's Caffe-order blob (-1 = padding), built at Create
	std::string err_;
};

}  // namespace dtrl
