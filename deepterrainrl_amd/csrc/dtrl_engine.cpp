// dtrl_engine.cpp -- batch engine logic (host side of the frame loop). See dtrl_engine.h.
//
// Frame loop = cScenarioExp::Update / cScenarioPoliEval::Update over the whole batch
// (scenarios/ScenarioExp.cpp:83-98, scenarios/ScenarioPoliEval.cpp:110-125):
//   1. one kernel launch advances every env by num_update_steps env-steps and runs the end-of-frame fall logic;
//   2. the host reads back 16 B per env (root x, reset request);
//   3. envs that fell get a fresh terrain window (cScenarioSimChar::ResetGround, scenarios/ScenarioSimChar.cpp:574-583)
//      and are flagged so the next launch performs the character/controller reset on device;
//   4. every other env's window slides if the character came within view distance of its end
//      (cScenarioSimChar::UpdateGround, :564-572). Doing this at frame boundaries instead of every env-step is
//      equivalent because the window is rebuilt 1 m before any sample can reach its end (DESIGN.md "Ground").
#include "dtrl_engine.h"
#include "dtrl_terrain_dev.h"
#include "dtrl_topo.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include "../../include/dtrl.h"
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <thread>

namespace dtrl {

namespace {
constexpr double kViewDist = 10.0;          // cCharController view distance (sim/TerrainRLCharController.cpp:12)
constexpr double kGroundSpawnOffset = -1.0; // scenarios/ScenarioSimChar.cpp:19
constexpr double kViewPad = 1.0;            // gCharViewDistPad, scenarios/ScenarioSimChar.cpp:18
}

// Persistent host workers for the frame-boundary terrain regeneration: every env owns its RNG stream and its window, so the rebuilds of one
// frame are independent (the reference runs one OS thread per scene, scenarios/ScenarioTrain.cpp:100-115). The pool is process-wide and
// created on first use; a frame with fewer than kMinParallel rebuilds stays on the calling thread.
namespace {
class WorkerPool {
public:
	static WorkerPool& Get() { static WorkerPool p; return p; }
	void ParallelFor(int count, const std::function<void(int)>& fn)
	{
		if (count <= 0) return;
		if (count < kMinParallel || threads_.empty()) { for (int i = 0; i < count; ++i) fn(i); return; }
		std::lock_guard<std::mutex> one_caller(call_m_);   // batches driven from different host threads take turns
		// one Job object per call: function, item count and the item cursor travel together, so a worker that wakes late from an earlier call still
		// holds THAT call's (exhausted) cursor and can neither run this call's function on a stale index nor count an item twice
		auto job = std::make_shared<Job>();
		job->fn = &fn; job->count = count;
		{ std::lock_guard<std::mutex> lk(m_); job_ = job; ++epoch_; }
		cv_.notify_all();
		Run(*job);   // the caller works too
		std::unique_lock<std::mutex> lk(m_);
		cv_done_.wait(lk, [&] { return job->done == job->count; });   // every item has RETURNED (done is bumped after the call): fn may go out of scope
		job_.reset();
	}
	int num_threads() const { return static_cast<int>(threads_.size()) + 1; }
private:
	struct Job { const std::function<void(int)>* fn = nullptr; int count = 0; std::atomic<int> next{0}; int done = 0; };
	static constexpr int kMinParallel = 8;
	WorkerPool()
	{
		// DTRL_HOST_THREADS overrides. Default: half the hardware threads, at most 16, shared between the ranks of this node (one process per GPU:
		// LOCAL_WORLD_SIZE as torch.distributed.run / torchrun export it), so that 8 ranks do not start 8 pools of 16 on the same cores
		int n = 0;
		if (const char* env = std::getenv("DTRL_HOST_THREADS")) n = std::atoi(env);
		else {
			int ranks = 1;
			if (const char* lw = std::getenv("LOCAL_WORLD_SIZE")) ranks = std::max(1, std::atoi(lw));
			n = std::max(1, std::min(16, static_cast<int>(std::thread::hardware_concurrency()) / (2 * ranks)));
		}
		for (int t = 1; t < n; ++t) threads_.emplace_back([this] { Loop(); });
	}
	~WorkerPool()
	{
		{ std::lock_guard<std::mutex> lk(m_); stop_ = true; ++epoch_; }
		cv_.notify_all();
		for (auto& t : threads_) t.join();
	}
	void Run(Job& j)
	{
		int finished = 0;
		for (;;) {
			const int i = j.next.fetch_add(1);
			if (i >= j.count) break;
			(*j.fn)(i); ++finished;
		}
		if (finished) { std::lock_guard<std::mutex> lk(m_); j.done += finished; if (j.done == j.count) cv_done_.notify_all(); }
	}
	void Loop()
	{
		long seen = 0;
		for (;;) {
			std::shared_ptr<Job> j;
			{
				std::unique_lock<std::mutex> lk(m_);
				cv_.wait(lk, [&] { return epoch_ != seen; });
				seen = epoch_;
				if (stop_) return;
				j = job_;   // the generation this wake-up belongs to (or a newer one; never a mix of two)
			}
			if (j) Run(*j);
		}
	}
	std::vector<std::thread> threads_;
	std::mutex m_, call_m_; std::condition_variable cv_, cv_done_;
	std::shared_ptr<Job> job_;
	long epoch_ = 0; bool stop_ = false;
};
}  // namespace

Engine::~Engine()
{
	if (be_) {
		be_->Sync();
		for (Snapshot* s : snapshots_) { be_->Free(s->payload); s->payload = nullptr; s->owner = nullptr; }   // (the handles stay valid for dtrl_snapshot_info / _free)
		TraceFree(); be_->FreeHostStaging(trace_stage_);
		LogFree();
		be_->FreeHostStaging(snap_ids_);
		be_->FreeHostStaging(slot_keys_.part); be_->FreeHostStaging(variant_keys_.part); be_->FreeHostStaging(terrain_keys_.part);
		if (ext_meta_) be_->FreeHostStaging(ext_meta_);
		for (void* p : allocs_) be_->Free(p);
		for (void* p : host_allocs_) be_->FreeHostStaging(p);
		be_->FreeHostStaging(pin_drain_); be_->FreeHostStaging(pin_recs_); be_->FreeHostStaging(pin_order_); be_->FreeHostStaging(pin_ids_); be_->FreeHostStaging(status_); be_->FreeHostStaging(stage_slot_);
		delete be_;
	}
}

// number of floats of the device-side weight layout (InnerProduct blobs are padded to 4-input blocks)
static int64_t DevNumParams(const NetDesc& d)
{
	int64_t n = 0; int cin = 1, w = d.n_terrain;
	for (int l = 0; l < 3; ++l) { n += pad4(static_cast<int64_t>(d.conv_ch[l]) * cin * d.conv_k[l]) + pad4(d.conv_ch[l]); cin = d.conv_ch[l]; w = w - d.conv_k[l] + 1; }
	n += fc_dev_size(d.fc_terr, cin * w) + pad4(d.fc_terr);
	n += fc_dev_size(d.fc_trunk, d.fc_terr + d.n_char) + pad4(d.fc_trunk);
	n += (fc_dev_size(d.fc_head, d.fc_trunk) + pad4(d.fc_head)) * (1 + d.n_frags);
	n += fc_dev_size(d.n_frags, d.fc_head) + pad4(d.n_frags) + static_cast<int64_t>(d.n_frags) * (fc_dev_size(d.frag_size, d.fc_head) + pad4(d.frag_size));
	return n;
}

int Engine::Create(const char* const* argv, int argc, int num_envs, int device_id)
{
	if (num_envs <= 0) return Fail(DTRL_ERR_ARG, "num_envs must be positive");
	// optimizer/Main.cpp:19-32: command line first, then the arg file appended (first match wins -> command line overrides)
	ArgParser& args = args_;   // kept: dtrl_variant_load_* runs the loader again with these arguments
	args = ArgParser(argv, argc);
	std::string arg_file;
	if (args.ParseString("arg_file", arg_file)) {
		std::string root; args.ParseString("data_root", root);
		std::string path = (arg_file.empty() || arg_file[0] == '/' || root.empty()) ? arg_file : root + "/" + arg_file;
		if (!args.AppendArgs(path)) return Fail(DTRL_ERR_IO, "Failed to load args from: " + path);
	}
	{   // (a misspelt mode is an argument error, not a file error)
		std::string pm;
		if (args.ParseString("policy_mode", pm) && pm != "internal" && pm != "external") return Fail(DTRL_ERR_ARG, "-policy_mode= must be internal (the policy net runs inside the frame kernel) or external (envs park at their decisions, the caller supplies the actions), not '" + pm + "'");
	}
	if (!LoadScenario(args, cfg_, err_)) return DTRL_ERR_IO;
	n_ = num_envs;
	const DevModel& m = cfg_.model;
	// external policy mode takes the place of cBaseControllerMACE::DecideAction (sim/BaseControllerMACE.cpp:267-296); the Q and CACLA controllers decide differently
	if (cfg_.external_policy && m.ctrl_type != 1)
		return Fail(DTRL_ERR_ARG, "-policy_mode= external needs a MACE controller (dog_mace, goat_mace, raptor_mace): char_ctrl '" + cfg_.char_ctrl + "' is a " + (m.ctrl_type == 0 ? "Q" : "CACLA") + " controller");
	S_ = kNumGroundSamples + (2 * m.L - 1) + 2 * m.L;   // sim/TerrainRLCharController.cpp:308-342
	// sim/BaseControllerMACE.cpp:28-31; sim/BaseControllerCacla.cpp:13-16 (the parameters alone); sim/BaseControllerQ.cpp:12-23 (one-hot over the base actions)
	A_ = (m.ctrl_type == 2) ? m.n_opt : (m.ctrl_type == 0 ? m.n_actions : 1 + m.n_opt);
	W_ = 1 + 2 * S_ + A_;                               // learning/MACETrainer.cpp:373-376

	be_ = MakeBackend();
	{ int reserve = -1; if (args.ParseInt("reserve_cus", reserve)) be_->SetReserveCus(reserve); }   // (else the DTRL_RESERVE_CUS environment variable; include/dtrl.h: dtrl_side_stream)
	if (!be_->Init(device_id, err_)) return DTRL_ERR_NO_DEVICE;

	auto alloc = [&](size_t bytes) -> void* { void* p = be_->Alloc(bytes); if (p) allocs_.push_back(p); return p; };
	d_model_ = static_cast<DevModel*>(alloc(sizeof(DevModel)));
	// (external policy mode: the delivered action rows and the per-env counts follow the state records in the same allocation -- DevBuffers::ext_envs)
	buf_.st = static_cast<EnvState*>(alloc((sizeof(EnvState) + (cfg_.external_policy ? sizeof(ExtAction) + sizeof(ExtCount) : 0)) * n_));
	if (cfg_.external_policy) {
		buf_.ext_envs = n_;
		ext_meta_ = static_cast<int32_t*>(be_->HostStaging(sizeof(int32_t) * 4));
		d_ext_ids_ = static_cast<int32_t*>(alloc(sizeof(int32_t) * n_));
		d_ext_action_ids_ = static_cast<int32_t*>(alloc(sizeof(int32_t) * n_));
		d_ext_flags_ = static_cast<uint32_t*>(alloc(sizeof(uint32_t) * n_));
		d_ext_states_ = static_cast<double*>(alloc(sizeof(double) * S_ * n_));
		d_ext_params_ = static_cast<double*>(alloc(sizeof(double) * std::max(1, m.n_opt) * n_));
		if (!ext_meta_ || !d_ext_ids_ || !d_ext_action_ids_ || !d_ext_flags_ || !d_ext_states_ || !d_ext_params_) return Fail(DTRL_ERR_DEVICE, "device allocation failed: " + be_->error());
	}
	buf_.gr = static_cast<GroundRec*>(alloc(sizeof(GroundRec) * n_));
	buf_.status = static_cast<EnvStatus*>(alloc(sizeof(EnvStatus) * n_));
	buf_.poli_state = static_cast<real*>(alloc(sizeof(real) * S_ * n_));
	buf_.tup_s0 = static_cast<real*>(alloc(sizeof(real) * S_ * n_));
	buf_.tup_a = static_cast<real*>(alloc(sizeof(real) * A_ * n_));
	buf_.S = S_; buf_.A = A_; buf_.W = W_; buf_.model_D = m.D; buf_.model_topo = match_topology(m.parent, m.L);
	// a tuple per env per cycle (~13 frames) at most; room for 2 per env between drains, at least the reference's ring size
	// (-tuple_ring_capacity= overrides; dtrl_tuple_stats reports how many rows were dropped because the ring was full)
	buf_.tuple_cap = std::max(2 * n_, cfg_.tuple_buffer_size);
	if (cfg_.tuple_ring_capacity > 0) buf_.tuple_cap = cfg_.tuple_ring_capacity;
	// (-tuple_ring= host: page-locked host memory the kernels address through the same pointers -- a tuple is 2.4 KB of fire-and-forget stores over the link and
	// one system-scope atomic on the cursor, ~0.6 MB per frame at 4096 dogs; dtrl_drain_tuples then reads the ring without queueing anything on the GPU)
	if (!AllocRing(ring_[0])) return Fail(DTRL_ERR_DEVICE, "tuple ring allocation failed: " + be_->error());
	UseRing(buf_, 0);
	d_env_list_ = static_cast<int32_t*>(alloc(sizeof(int32_t) * n_));
	d_order_ = static_cast<int32_t*>(alloc(sizeof(int32_t) * n_));
	if (cfg_.device_terrain) {
		buf_.gen = static_cast<GroundGen*>(alloc(sizeof(GroundGen) * n_));
		d_tcfg_ = static_cast<TerrainCfg*>(alloc(sizeof(TerrainCfg)));
		buf_.tcfg = d_tcfg_;
		buf_.dist_cap = kDistRingCap;
		buf_.dist_ring = static_cast<DistRec*>(alloc(sizeof(DistRec) * buf_.dist_cap));
		buf_.dist_count = static_cast<int32_t*>(alloc(sizeof(int32_t) * 4));
		if (!buf_.gen || !d_tcfg_ || !buf_.dist_ring || !buf_.dist_count) return Fail(DTRL_ERR_DEVICE, "device allocation failed: " + be_->error());
	}
	pin_recs_ = static_cast<GroundRec*>(be_->HostStaging(sizeof(GroundRec) * n_));
	pin_order_ = static_cast<int32_t*>(be_->HostStaging(sizeof(int32_t) * n_));
	pin_ids_ = static_cast<int32_t*>(be_->HostStaging(sizeof(int32_t) * n_));
	if (!pin_recs_ || !pin_order_ || !pin_ids_) return Fail(DTRL_ERR_DEVICE, "host staging allocation failed: " + be_->error());
	// env groups (one stream each): one group fills the resident-wavefront slots while another's frame-boundary host work runs. Round 1 (boundary work = copies
	// + scatter launches) measured 2 as the optimum (1: 10.1, 2: 13.7, 3: 10.9, 4: 12.6, 8: 6.3 M env-steps/s). Round 4, zero-copy boundary: a group's launch lasts
	// as long as ITS slowest env, so while the slowest envs (characters lying on 13-24 constraint rows) ran the slow Gauss-Seidel path, smaller groups were ahead
	// (2 / 3 / 4 groups: 16.7 / 16.8 / 17.0 M); with every row count on the register path the tail is gone and the count no longer matters for the rollout
	// (17.73 / 17.76 / 17.78 M) while the per-frame loops pay for every extra group's boundary work (exchange leg without a collective 16.9 / 16.6 / 15.8 M):
	// two it stays. DTRL_GROUPS overrides.
	{
		int G = n_ >= 1024 ? 2 : 1;
		if (const char* env = std::getenv("DTRL_GROUPS")) G = std::max(1, std::min(be_->NumStreams(), std::atoi(env)));
		G = std::min(G, n_);
		groups_.clear();
		for (int g = 0; g < G; ++g) { Group gr; gr.e0 = static_cast<int>(static_cast<int64_t>(n_) * g / G); gr.n = static_cast<int>(static_cast<int64_t>(n_) * (g + 1) / G) - gr.e0; groups_.push_back(gr); }
		for (int e = 0; e < n_; ++e) pin_order_[e] = e;
		if (!be_->H2D(d_order_, pin_order_, sizeof(int32_t) * n_)) return Fail(DTRL_ERR_DEVICE, be_->error());
	}
	buf_.prof = static_cast<unsigned long long*>(alloc(sizeof(unsigned long long) * kProfMax * n_));
	if (!d_model_ || !buf_.st || !buf_.gr || !buf_.status || !buf_.poli_state || !buf_.tup_s0 || !buf_.tup_a || !buf_.tuple_rows || !buf_.tuple_flags || !buf_.tuple_env || !buf_.tuple_count)
		return Fail(DTRL_ERR_DEVICE, "device allocation failed: " + be_->error());
	if (cfg_.has_policy_net) {
		const NetDesc& d = cfg_.net;
		buf_.net = d;
		buf_.nn_out = static_cast<real*>(alloc(sizeof(real) * static_cast<size_t>(d.out_size) * n_));
		float* w_dev = static_cast<float*>(alloc(sizeof(float) * static_cast<size_t>(DevNumParams(d))));
		weights_alt_ = static_cast<float*>(alloc(sizeof(float) * static_cast<size_t>(DevNumParams(d))));   // second weight buffer: hand-overs during a frame (SetPolicyDevice)
		weights_buf0_ = w_dev;
		real* io = static_cast<real*>(alloc(sizeof(real) * d.in_size)); real* is = static_cast<real*>(alloc(sizeof(real) * d.in_size));
		real* oo = static_cast<real*>(alloc(sizeof(real) * d.out_size)); real* os = static_cast<real*>(alloc(sizeof(real) * d.out_size));
		if (!buf_.nn_out || !w_dev || !weights_alt_ || !io || !is || !oo || !os) return Fail(DTRL_ERR_DEVICE, "device allocation failed: " + be_->error());
		{ std::vector<real> zeros(static_cast<size_t>(d.out_size) * n_, 0.0); if (!be_->H2D(buf_.nn_out, zeros.data(), sizeof(real) * zeros.size())) return Fail(DTRL_ERR_DEVICE, be_->error()); }   // dtrl_get_policy_output before the first forward
		buf_.weights = w_dev; buf_.in_off = io; buf_.in_scale = is; buf_.out_off = oo; buf_.out_scale = os;
		cfg_.model.has_net = 1;
		BuildRelayoutMap(relayout_);
		d_relayout_ = static_cast<int32_t*>(alloc(sizeof(int32_t) * relayout_.size()));
		if (!d_relayout_ || !be_->H2D(d_relayout_, relayout_.data(), sizeof(int32_t) * relayout_.size())) return Fail(DTRL_ERR_DEVICE, "device allocation failed: " + be_->error());
	}
	if (!be_->H2D(d_model_, &cfg_.model, sizeof(DevModel))) return Fail(DTRL_ERR_DEVICE, be_->error());

	// per-env grounds: cGroundVar2D seeded per env (terrain_seed + global env id) so a trajectory is shard-invariant
	grounds_.resize(n_);
	status_ = static_cast<EnvStatus*>(be_->HostStaging(sizeof(EnvStatus) * n_));
	if (!status_) return Fail(DTRL_ERR_DEVICE, "host staging allocation failed: " + be_->error());
	// host terrain mode: no copy at the frame boundary. The frame kernel writes its 24-byte status records straight into this page-locked host array,
	// and the launch order, the reset lists and the regenerated terrain records are read by the kernels from the page-locked arrays the host filled
	// (a copy is a blit kernel that queues behind 2048 resident wavefronts: ~160 us each, three to four per group-frame). In device terrain mode the status
	// stays in device memory, where the boundary kernels read it.
	zero_copy_ = !cfg_.device_terrain;
	if (zero_copy_) {
		buf_.status = status_;
		stage_slot_ = static_cast<int32_t*>(be_->HostStaging(sizeof(int32_t) * n_));
		if (!stage_slot_) return Fail(DTRL_ERR_DEVICE, "host staging allocation failed: " + be_->error());
		std::memset(stage_slot_, 0, sizeof(int32_t) * n_);
		buf_.stage_slot = stage_slot_; buf_.gr_stage = pin_recs_;
	}
	double params[kNumTerrainParams];
	LerpTerrainParams(cfg_, cfg_.terrain_blend, params);
	terrain_lerp_ = cfg_.terrain_blend;
	if (cfg_.device_terrain) {
		// every env's window is built by the GPU from its own counter stream (key: terrain seed + global env id)
		grounds_.clear();
		int rc = UploadTerrainCfg(params);
		if (rc != DTRL_OK) return rc;
		std::vector<GroundGen> gen(n_);
		for (int e = 0; e < n_; ++e) { gen[e].key = terrain_stream_key(cfg_.terrain_seed, cfg_.run.env_id_base + e); gen[e].ctr = 0; gen[e].builds = 0; gen[e].overflow = 0; }
		if (!be_->H2D(buf_.gen, gen.data(), sizeof(GroundGen) * n_)) return Fail(DTRL_ERR_DEVICE, be_->error());
		if (!Boundary(EnvSpan{0, n_, nullptr}, 1) || !be_->Sync()) return Fail(DTRL_ERR_DEVICE, be_->error());
	} else {
	std::vector<GroundRec> recs(n_);
	for (int e = 0; e < n_; ++e) {
		GroundWindow& g = grounds_[e];
		g.Configure(cfg_.terrain_type, params, cfg_.model.world_scale, 2 * kViewDist);
		g.SeedRand(static_cast<unsigned long>(cfg_.terrain_seed + static_cast<uint64_t>(cfg_.run.env_id_base) + e));
		g.InitSegments(-kViewDist + kGroundSpawnOffset, kViewDist + kGroundSpawnOffset);   // scenarios/ScenarioSimChar.cpp:344-369
		if (!g.FillRecord(recs[e], err_)) return DTRL_ERR_CAPACITY;
	}
	if (!be_->H2D(buf_.gr, recs.data(), sizeof(GroundRec) * n_)) return Fail(DTRL_ERR_DEVICE, be_->error());
	if (stage_slot_) std::memset(stage_slot_, 0, sizeof(int32_t) * n_);
	}
	std::vector<EnvState> st(n_);
	std::memset(st.data(), 0, sizeof(EnvState) * n_);
	for (int e = 0; e < n_; ++e) { st[e].do_init = 1; st[e].cmd_action = -1; st[e].pert_link = -1; }
	if (!be_->H2D(buf_.st, st.data(), sizeof(EnvState) * n_)) return Fail(DTRL_ERR_DEVICE, be_->error());
	// cScenarioSimChar::Init on every env now (a 0-step launch), so getters and dtrl_set_pose_vel see / act on the initial state
	// before the first step, as with the reference's Init()
	if (!be_->Launch(d_model_, cfg_.run, buf_, n_, 0, 0.0, false) || !be_->Sync()) return Fail(DTRL_ERR_DEVICE, be_->error());
	return DTRL_OK;
}

// tmp_rec_ = the env's current ground record: the device copy, or -- host terrain mode -- the regenerated record still waiting in page-locked
// memory for the env's next launch to copy it in (call after Sync())
bool Engine::FetchGroundRec(int env)
{
	if (zero_copy_ && stage_slot_[env] > 0) { std::memcpy(&tmp_rec_, &pin_recs_[stage_slot_[env] - 1], sizeof(GroundRec)); return true; }
	return be_->D2H(&tmp_rec_, &buf_.gr[env], sizeof(GroundRec));
}

bool Engine::UploadGround(int env)
{
	if (!grounds_[env].FillRecord(tmp_rec_, err_)) return false;
	if (zero_copy_) stage_slot_[env] = 0;   // a record waiting for the env's next launch is superseded
	if (!be_->H2D(&buf_.gr[env], &tmp_rec_, sizeof(GroundRec))) { err_ = be_->error(); return false; }
	return true;
}
const int32_t* Engine::StageIds(const std::vector<int32_t>& ids, int off)
{
	std::memcpy(pin_ids_ + off, ids.data(), sizeof(int32_t) * ids.size());
	if (zero_copy_) return pin_ids_ + off;
	if (!be_->H2DAsync(d_env_list_ + off, pin_ids_ + off, sizeof(int32_t) * ids.size())) { err_ = be_->error(); return nullptr; }
	return d_env_list_ + off;
}
// device-side half of a reset (cSimCharacter::Reset + controller reset + InitCharacterPos), on the listed envs only:
// a compact 0-step launch, so getters observe the reset state right after Update() as with the reference.
// group >= 0: the group's stream and its slices of the staging / list buffers; group < 0: whole batch on stream 0 (user resets).
int Engine::ApplyResets(const std::vector<int32_t>& ids, int group, const int32_t* staged)
{
	if (ids.empty()) return DTRL_OK;
	const int off = group >= 0 ? groups_[group].e0 : 0;
	DevBuffers b = buf_;
	b.env_list = staged ? staged : StageIds(ids, off);
	if (!b.env_list) return DTRL_ERR_DEVICE;
	b.reset_listed = 1;
	if (!LaunchEnvs(b, static_cast<int>(ids.size()), 0, 0.0, false, pin_ids_ + off, group >= 0 ? off : n_)) return Fail(DTRL_ERR_DEVICE, be_->error());
	return DTRL_OK;
}

// DTRL_HOST_TIMING=1: print where the frame-boundary host work goes when the engine is destroyed (diagnosis only)
namespace {
struct HostTiming {
	bool on = std::getenv("DTRL_HOST_TIMING") != nullptr;
	double t_sync = 0, t_loop = 0, t_sort = 0, t_reset = 0, t_launch = 0; long n = 0, regen = 0;
	double d_wait = 0, d_count = 0, d_copy = 0; long d_n = 0;
	~HostTiming() { if (on && d_n) std::fprintf(stderr, "[dtrl host] per tuple drain: wait for the ring's frame %.1f us, count read-back %.1f us, rows + reset %.1f us (n=%ld)\n", 1e6 * d_wait / d_n, 1e6 * d_count / d_n, 1e6 * d_copy / d_n, d_n);
		if (on && n) std::fprintf(stderr, "[dtrl host] per group-frame: status read-back %.1f us, env loop %.1f us (%.2f regen), order %.1f us, resets %.1f us, launch %.1f us (n=%ld)\n", 1e6 * t_sync / n, 1e6 * t_loop / n, double(regen) / n, 1e6 * t_sort / n, 1e6 * t_reset / n, 1e6 * t_launch / n, n); }
} g_ht;
inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}
int Engine::LaunchGroup(int group, int n_steps, double dt_step, bool frame_end)
{
	const Group& g = groups_[group];
	be_->SelectStream(group);
	DevBuffers b = buf_;
	b.env_list = (zero_copy_ ? pin_order_ : d_order_) + g.e0;   // the group's launch order (global env ids), costliest first
	const double lt0 = g_ht.on ? now_s() : 0;
	bool ok = true;
	if (group < static_cast<int>(policy_wait_.size()) && policy_wait_[group]) { ok = be_->WaitPolicyReady(group); policy_wait_[group] = 0; }   // dtrl_set_policy_device_async
	ok = ok && LaunchEnvs(b, g.n, n_steps, dt_step, frame_end, zero_copy_ ? pin_order_ + g.e0 : nullptr, g.e0);
	// tuple pipelining: the drain of this frame's ring runs on a stream of its own one frame later and must follow THIS launch on the device -- the host
	// has not necessarily waited for it by then (-terrain_gen= device queues the boundary work and the next frame without a sync)
	if (ok && tuple_pipelining_ && n_steps > 0) ok = be_->MarkFrame(group, wr_ring_);
	// the policy hand-over is double-buffered: remember which weight buffer this launch reads, so that a later gather INTO it can wait for the launch on the device
	if (ok && weights_alt_ && n_steps > 0) ok = be_->MarkWeightReader(group, b.weights == weights_buf0_ ? 0 : 1);
	// episode limit, trace and episode log, host terrain: the rules are queued behind the group's frame so that the limit has amended the status records when HostFrameWork's wait
	// for this stream returns and its loop reads them, and trace and log have read the keys before that loop moves them (device terrain: DeviceFrameWork queues it in front of the boundary launch)
	if (ok && !cfg_.device_terrain && n_steps > 0) ok = RulesBehindFrame(group);
	if (g_ht.on) g_ht.t_launch += now_s() - lt0;
	be_->SelectStream(0);
	return ok ? DTRL_OK : Fail(DTRL_ERR_DEVICE, be_->error());
}

// every launch of the frame kernels after the batch's creation comes through here: a batch without slots and without variants launches exactly as it always did
bool Engine::LaunchEnvs(const DevBuffers& b, int n_envs, int n_steps, real dt, bool frame_end, const int32_t* list_host, int part_off)
{
	const bool variants = !var_models_.empty();   // (variants and slots exclude each other: dtrl_variants_create / dtrl_slots_create)
	if (!variants && slots_.empty()) return be_->Launch(d_model_, cfg_.run, b, n_envs, n_steps, dt, frame_end);
	EnvKeyView v = (variants ? variant_keys_ : slot_keys_).View(list_host, part_off);
	if (variants) { v.models_dev = d_var_models_; if (rescale_table_) v.n_keys += n_; }   // (the private records of a variant rescale: keys V .. V + num_envs - 1)
	else { v.slots_dev = d_slot_table_; v.slots_host = slot_table_.data(); }
	return be_->LaunchKeyed(variants ? d_var_models_ : d_model_, cfg_.run, b, v, n_envs, n_steps, dt, frame_end);
}

TerrainCfg Engine::MakeTerrainCfg(int type, const double* params) const
{
	TerrainCfg c{};
	c.type = type;
	std::memcpy(c.params, params, sizeof(c.params));
	c.world_scale = cfg_.model.world_scale; c.segment_width = 2 * kViewDist;
	c.view_min = -2; c.view_max = kViewDist + kViewPad;
	c.spawn_min = -kViewDist + kGroundSpawnOffset; c.spawn_max = kViewDist + kGroundSpawnOffset;
	return c;
}
int Engine::UploadTerrainCfg(const double* params)
{
	const TerrainCfg c = MakeTerrainCfg(cfg_.terrain_type, params);
	be_->Sync();
	if (!be_->H2D(d_tcfg_, &c, sizeof(c))) return Fail(DTRL_ERR_DEVICE, be_->error());
	if (d_terrain_table_ && !be_->H2D(d_terrain_table_, &c, sizeof(c))) return Fail(DTRL_ERR_DEVICE, be_->error());   // terrain 0 of a batch with terrain sets
	return DTRL_OK;
}

// -terrain_gen= device: the frame boundary of one env group as three launches on the group's stream, behind its frame kernel and in front of its next
// one -- the host neither waits nor loops over envs:
//   dtrl_episode_limit     (with an episode limit) the envs whose episode reached its frame limit or the distance get need_reset, as if they had fallen
//   dtrl_trace_record      (with a trace) the group's traced envs write the row of the frame that has just ended
//   dtrl_episode_log       (with an episode log) the group's envs whose episode ended append one row each to the group's ring in page-locked host memory
//   dtrl_terrain_boundary  fresh windows for the envs that fell, slid windows where the character got close to an edge, episode distances logged
//   dtrl_order_by_cost     launch order of the next frame (costliest wavefronts first)
//   dtrl_variant_redraw    (with a variant redraw) the envs that fell draw the model variant of their next episode
//   dtrl_variant_rescale   (with a variant rescale) the envs that fell under a private record get its mass and motor scalars redrawn
//   dtrl_push_schedule     (with a push schedule) the envs whose wait ran out get a random push into their perturbation slot
//   0-step frame launch    the device half of the reset, taken by the envs that fell, skipped by the others (reset_listed = 2)
int Engine::DeviceFrameWork(int group)
{
	const Group& grp = groups_[group];
	be_->SelectStream(group);
	struct Restore { Backend* b; ~Restore() { b->SelectStream(0); } } restore{be_};
	DevBuffers b = buf_;
	b.env_list = nullptr; b.reset_listed = 2;
	const EnvSpan span{grp.e0, grp.n, nullptr};
	// (the order of the rules: dtrl_engine.h)
	if (!RulesBehindFrame(group) || !Boundary(span, 0) || !be_->OrderByCost(buf_.status, grp.e0, grp.n, d_order_) || !RulesBeforeResets(span)) return Fail(DTRL_ERR_DEVICE, be_->error());
	b.env_list = d_order_ + grp.e0;
	if (!LaunchEnvs(b, grp.n, 0, 0.0, false, nullptr, grp.e0)) return Fail(DTRL_ERR_DEVICE, be_->error());
	return DTRL_OK;
}
// device distance ring -> dist_log_ (completion order inside the ring is whatever the atomics produced; GetDistLog groups by env, and one env
// finishes at most one episode per frame, so the per-env time order is kept by draining between frames or by the ring order of separate launches)
int Engine::DrainDeviceDistLog()
{
	if (!cfg_.device_terrain) return DTRL_OK;
	be_->Sync();
	int32_t cnt = 0;
	if (!be_->D2H(&cnt, buf_.dist_count, sizeof(cnt))) return Fail(DTRL_ERR_DEVICE, be_->error());
	const bool overflow = cnt > buf_.dist_cap;   // the ring keeps the first dist_cap records of the interval; the rest were counted, not stored
	if (overflow) cnt = buf_.dist_cap;
	if (cnt > 0) {
		std::vector<DistRec> tmp(cnt);
		if (!be_->D2H(tmp.data(), buf_.dist_ring, sizeof(DistRec) * cnt)) return Fail(DTRL_ERR_DEVICE, be_->error());
		for (const DistRec& r : tmp) dist_log_.emplace_back(r.env, r.dist);
		const int32_t zero = 0;
		if (!be_->H2D(buf_.dist_count, &zero, sizeof(zero))) return Fail(DTRL_ERR_DEVICE, be_->error());
	}
	if (overflow) return Fail(DTRL_ERR_CAPACITY, "episode distance ring overflowed (records beyond its capacity were dropped): call dtrl_get_dist_log more often");
	return DTRL_OK;
}

// frame-boundary host work of one env group, on the group's stream
int Engine::HostFrameWork(int group)
{
	if (cfg_.device_terrain) return DeviceFrameWork(group);
	const double ht0 = g_ht.on ? now_s() : 0;
	const Group& grp = groups_[group];
	const int e0 = grp.e0, e1 = grp.e0 + grp.n;
	be_->SelectStream(group);
	struct Restore { Backend* b; ~Restore() { b->SelectStream(0); } } restore{be_};
	// the status read-back synchronises the group's stream: its frame kernel and every upload queued during its previous frame
	// have completed, so its slice of the staging arena can be reused from the start
	if (!be_->SyncSelected()) return Fail(DTRL_ERR_DEVICE, be_->error());   // (the kernel wrote status_ itself: host terrain mode moves no copies, see Init)
	const double ht1 = g_ht.on ? now_s() : 0;
	reset_ids_.clear();
	work_.clear();
	bool level_moved = false, variant_moved = false;
	RedrawCfg rd = redraw_cfg_; rd.cum = redraw_cum_.host.data();
	for (int e = e0; e < e1; ++e) {
		const EnvStatus& s = status_[e];
		if (redraw_on_) {   // the redraw's rule: an env that fell draws the variant its next episode runs under (the reset launch below reads the key)
			int32_t& k = variant_keys_.env_key[e];
			const int32_t next = var_redraw_step(redraw_.host[e], k, (s.need_reset & 1) != 0, rd, rd.cum, e);
			if (next != k) { k = next; variant_moved = true; }
		}
		if (ladder_on_) {   // the ladder's rule, in front of the env's terrain work: the window built or slid below is already the new level's
			int32_t& k = terrain_keys_.env_key[e];
			const int32_t next = tg_ladder_step(ladder_.host[e], k, s, ladder_cfg_, 0, e);
			if (next != k) { k = next; const TerrainCfg& c = terrain_table_[k]; grounds_[e].SetTerrain(c.type, c.params); level_moved = true; }
		}
		if (s.need_reset & 2) dist_log_.emplace_back(e, s.episode_dist);   // cScenarioPoliEval::RecordDistTraveled -> mDistLog
		if (s.need_reset) { reset_ids_.push_back(e); work_.push_back(e); }
		else if (grounds_[e].NeedsUpdate(s.root_x - 2, s.root_x + kViewDist + kViewPad)) work_.push_back(e);
	}
	// (the device copy of the keys, which dtrl_terrain_stats reduces over: the group's slice, when a level in it moved; no launch reads it)
	if (level_moved && !be_->H2D(terrain_keys_.d_env_key + e0, terrain_keys_.env_key.data() + e0, sizeof(int32_t) * static_cast<size_t>(grp.n))) return Fail(DTRL_ERR_DEVICE, be_->error());
	// (the variant keys are read by a launch: the group's slice goes up on the group's stream in front of the reset launch)
	if (variant_moved && !be_->H2D(variant_keys_.d_env_key + e0, variant_keys_.env_key.data() + e0, sizeof(int32_t) * static_cast<size_t>(grp.n))) return Fail(DTRL_ERR_DEVICE, be_->error());
	const int used = static_cast<int>(work_.size());
	if (used > 0) {
		// the rebuilds of one frame are independent (own RNG stream, own window per env): host workers share them; every rebuilt record goes into
		// its slot of the group's page-locked slice, from which the env's own wavefront copies it in when its next launch starts (stage_slot_)
		std::atomic<int> failed{0};
		WorkerPool::Get().ParallelFor(used, [&](int k) {
			const int e = work_[k];
			GroundWindow& g = grounds_[e];
			const EnvStatus& s = status_[e];
			if (s.need_reset) {
				// cScenarioSimChar::ResetGround: Clear + Update around the spawn point -> InitSegments with the SAME rng stream
				g.Clear();
				g.Update(-kViewDist + kGroundSpawnOffset, kViewDist + kGroundSpawnOffset);
			} else g.Update(s.root_x - 2, s.root_x + kViewDist + kViewPad);
			std::string err;
			if (!g.FillRecord(pin_recs_[e0 + k], err)) failed.store(1);
			stage_slot_[e] = e0 + k + 1;   // the env's wavefront copies the record in at the start of its next launch (the reset launch below, or the next frame)
		});
		if (failed.load()) return Fail(DTRL_ERR_CAPACITY, "terrain segment exceeds kSegCap vertices");
	}
	const double ht2 = g_ht.on ? now_s() : 0;
	// longest-processing-time-first: a launch is as long as its slowest wavefront (a stumbling character with ~20 constraint
	// rows per substep costs 3x a running one), so the envs that were costliest last frame are dispatched first.
	// Counting sort on cost / 16 (stable, O(n)).
	constexpr int kBuckets = 1024;
	bucket_.assign(kBuckets + 1, 0);
	auto key = [&](int e) { int k = status_[e].cost >> 4; if (k < 0) k = 0; if (k >= kBuckets) k = kBuckets - 1; return kBuckets - 1 - k; };
	for (int e = e0; e < e1; ++e) ++bucket_[key(e) + 1];
	for (int k = 0; k < kBuckets; ++k) bucket_[k + 1] += bucket_[k];
	for (int e = e0; e < e1; ++e) pin_order_[e0 + bucket_[key(e)]++] = e;
	const double ht3 = g_ht.on ? now_s() : 0;
	// variant rescale, then push schedule: the same launches as in device terrain mode, on the group's stream (idle since the wait above; the redraw's key upload is
	// queued on it) in front of the reset launch; status_ is the page-locked array the frame kernel wrote, which the device reads through the same pointer
	if (!RulesBeforeResets(EnvSpan{e0, grp.n, nullptr})) return Fail(DTRL_ERR_DEVICE, be_->error());
	const int rc = ApplyResets(reset_ids_, group);
	if (g_ht.on) { const double ht4 = now_s(); g_ht.t_sync += ht1 - ht0; g_ht.t_loop += ht2 - ht1; g_ht.t_sort += ht3 - ht2; g_ht.t_reset += ht4 - ht3; g_ht.regen += used; ++g_ht.n; }
	return rc;
}

int Engine::StepBegin(double dt)
{
	if (step_pending_) return Fail(DTRL_ERR_ARG, early_any_ ? "dtrl_step_begin after dtrl_step_poll relaunched a group: call dtrl_step_end_begin" : "dtrl_step_begin called twice without dtrl_step_end");
	if (dt <= 0) return DTRL_OK;   // cScenarioSimChar::Update returns early (scenarios/ScenarioSimChar.cpp:148-151)
	if (cfg_.model.has_net && !policy_set_ && !cfg_.external_policy) return Fail(DTRL_ERR_ARG, "policy_net was given but dtrl_set_policy has not been called");
	// (external policy mode: the launch is a TICK -- every env starts or continues its own frame of `steps` env-steps: dtrl_kernel.h env_frame_impl)
	const int steps = cfg_.model.num_update_steps;
	ApplyPendingPolicy();
	if (tuple_pipelining_) { wr_ring_ ^= 1; UseRing(buf_, wr_ring_); }   // this frame's tuples go to the ring that is not being drained
	for (size_t g = 0; g < groups_.size(); ++g) { int rc = LaunchGroup(static_cast<int>(g), steps, dt / steps, true); if (rc != DTRL_OK) return rc; }
	step_pending_ = true;
	return DTRL_OK;
}

int Engine::StepEnd()
{
	if (!step_pending_) return DTRL_OK;
	if (early_any_) return Fail(DTRL_ERR_ARG, "dtrl_step_end after dtrl_step_poll relaunched a group: the groups are a frame apart, call dtrl_step_end_begin first");
	step_pending_ = false;
	for (size_t g = 0; g < groups_.size(); ++g) { int rc = HostFrameWork(static_cast<int>(g)); if (rc != DTRL_OK) return rc; }
	return DTRL_OK;
}

// dtrl_step_end + dtrl_step_begin without the barrier between them: every env group gets its frame-boundary host work and its next launch as soon as
// ITS frame is done (the scheduling of RunFrames, one frame at a time), so one group's stragglers are covered by the other groups' next launches.
// With tuple pipelining on, the new launches write the other tuple ring and the frame that has just ended can be drained when this returns.
int Engine::StepEndBegin(double dt)
{
	if (cfg_.external_policy) return Fail(DTRL_ERR_ARG, "dtrl_step_end_begin: not available with -policy_mode= external (envs wait for the caller's actions between ticks: use dtrl_step or dtrl_step_begin / dtrl_step_end)");
	if (!step_pending_) return StepBegin(dt);
	if (dt <= 0) return StepEnd();
	const int G = static_cast<int>(groups_.size());
	const int steps = cfg_.model.num_update_steps;
	ApplyPendingPolicy();   // (every group's NEXT launch runs with the weights handed over during the frame that is ending)
	if (tuple_pipelining_) { wr_ring_ ^= 1; UseRing(buf_, wr_ring_); }
	std::vector<char> done(static_cast<size_t>(G), 0);
	int remaining = G;
	for (int c = 0; c < G; ++c) if (c < static_cast<int>(early_.size()) && early_[c]) { done[c] = 1; --remaining; }   // relaunched by dtrl_step_poll already (into the ring just switched to)
	early_.assign(static_cast<size_t>(G), 0); early_any_ = false;
	for (; remaining > 0; --remaining) {
		int g = -1;
		for (int c = 0; c < G; ++c) if (!done[c] && be_->StreamIdle(c)) { g = c; break; }
		if (g < 0) for (int c = 0; c < G; ++c) if (!done[c]) { g = c; break; }
		int rc = HostFrameWork(g);
		if (rc == DTRL_OK) rc = LaunchGroup(g, steps, dt / steps, true);
		if (rc != DTRL_OK) return rc;
		done[g] = 1;
	}
	return DTRL_OK;
}

// Between two dtrl_step_end_begin calls, with tuple pipelining on and the idle ring drained: every env group whose frame has ALREADY ended gets its
// boundary work and its next launch now (into the idle ring) instead of at the next dtrl_step_end_begin -- a caller that spends milliseconds between the two
// calls (a trainer working through the drained tuples) would otherwise leave a finished group's half of the GPU idle until it comes back. Never blocks.
// The next dtrl_step_end_begin handles the remaining groups only. Until then the tuple rings must not be touched (both are being written).
int Engine::StepPoll(double dt, int* relaunched)
{
	if (relaunched) *relaunched = 0;
	if (cfg_.external_policy) return Fail(DTRL_ERR_ARG, "dtrl_step_poll: not available with -policy_mode= external (it relaunches frames, and tuple pipelining is off in this mode)");
	if (!step_pending_ || !tuple_pipelining_ || dt <= 0 || cfg_.device_terrain) return DTRL_OK;
	const int G = static_cast<int>(groups_.size());
	if (static_cast<int>(early_.size()) != G) early_.assign(static_cast<size_t>(G), 0);
	if (!early_any_) {
		// the ring the early launches will write must be empty: it is the one the caller has just drained
		DevBuffers o = buf_; UseRing(o, wr_ring_ ^ 1);
		int32_t cnt = 0;
		if (cfg_.tuple_ring_host) cnt = *o.tuple_count;
		else return DTRL_OK;   // (a device ring's cursor cannot be read without queueing a copy behind the frame: the early relaunch is a host-ring feature)
		if (cnt != 0) return DTRL_OK;
	}
	const int steps = cfg_.model.num_update_steps;
	for (int g = 0; g < G; ++g) {
		if (early_[g] || !be_->StreamIdle(g)) continue;
		int rc = HostFrameWork(g);
		if (rc != DTRL_OK) return rc;
		DevBuffers keep = buf_;
		UseRing(buf_, wr_ring_ ^ 1);
		const int ring_now = wr_ring_; wr_ring_ ^= 1;          // (LaunchGroup marks the frame under the ring it writes)
		rc = LaunchGroup(g, steps, dt / steps, true);
		wr_ring_ = ring_now; buf_ = keep;
		if (rc != DTRL_OK) return rc;
		early_[g] = 1; early_any_ = true;
		if (relaunched) ++*relaunched;
	}
	return DTRL_OK;
}

int Engine::Step(double dt)
{
	int rc = StepBegin(dt);
	return rc != DTRL_OK ? rc : StepEnd();
}

// The one idle guard: refuse with `refusal` while a frame is in flight -- refuse, do not wait: that frame ends with the caller's own dtrl_step_end, and after
// dtrl_step_poll the env groups are a frame apart -- and, with `drain`, wait for every stream (with dtrl_step_poll or -terrain_gen= device the host has not
// otherwise waited for the launches it queued). Leaves stream 0 selected.
int Engine::RequireIdle(const std::string& refusal, bool drain)
{
	if (step_pending_ || early_any_) return Fail(DTRL_ERR_ARG, refusal);
	if (!drain) return DTRL_OK;
	be_->SelectStream(0);
	if (!be_->Sync()) return Fail(DTRL_ERR_DEVICE, be_->error());
	return DTRL_OK;
}
// the x a reset leaves in q[0] (dtrl_kernel.h reset_env, cScenarioSimChar::InitCharacterPos)
static double SpawnX(const DevModel& m) { return static_cast<double>(m.valid_init_pos_x ? m.init_pos_x : m.pose0[0]); }
static const char* const kFrameInFlight = " between dtrl_step_begin and dtrl_step_end (or after dtrl_step_poll relaunched a group): a frame is in flight; call dtrl_step_end first";

int Engine::StepUpdates(int n)
{
	if (cfg_.external_policy) return Fail(DTRL_ERR_ARG, "dtrl_step_updates: not available with -policy_mode= external (every env keeps its own frame of num_update_steps env-steps: use dtrl_step)");
	if (n <= 0) return DTRL_OK;
	if (int rc = RequireIdle("dtrl_step_updates while a frame is in flight (dtrl_step_begin / dtrl_step_poll): call dtrl_step_end_begin / dtrl_step_end first", false); rc != DTRL_OK) return rc;
	if (cfg_.model.has_net && !policy_set_) return Fail(DTRL_ERR_ARG, "policy_net was given but dtrl_set_policy has not been called");
	const double dt = (1.0 / 30.0) / cfg_.model.num_update_steps;
	ApplyPendingPolicy();
	for (size_t g = 0; g < groups_.size(); ++g) { int rc = LaunchGroup(static_cast<int>(g), n, dt, false); if (rc != DTRL_OK) return rc; }
	for (size_t g = 0; g < groups_.size(); ++g) { int rc = HostFrameWork(static_cast<int>(g)); if (rc != DTRL_OK) return rc; }
	return DTRL_OK;
}

// `frames` outer frames for every env. The envs are independent, so there is no frame barrier across groups: each group starts its
// next frame as soon as its own frame-boundary host work is done, and the tail of one group's launch (its slowest wavefronts) is
// covered by the other groups' next launches. Same results as `frames` calls of Step(dt).
int Engine::RunFrames(int frames, double dt)
{
	if (cfg_.external_policy) return Fail(DTRL_ERR_ARG, "dtrl_run_frames: not available with -policy_mode= external (envs wait for the caller's actions between ticks: use dtrl_step)");
	if (frames <= 0 || dt <= 0) return DTRL_OK;
	if (int rc = RequireIdle("dtrl_run_frames while a frame is in flight (dtrl_step_begin / dtrl_step_poll): call dtrl_step_end_begin / dtrl_step_end first", false); rc != DTRL_OK) return rc;
	if (cfg_.model.has_net && !policy_set_) return Fail(DTRL_ERR_ARG, "policy_net was given but dtrl_set_policy has not been called");
	const int G = static_cast<int>(groups_.size());
	const int steps = cfg_.model.num_update_steps;
	ApplyPendingPolicy();
	if (cfg_.device_terrain) {
		// nothing on the host depends on a frame's outcome: queue everything; the streams run ahead of the host by as much as the HIP queues hold
		for (int f = 0; f < frames; ++f) for (int g = 0; g < G; ++g) {
			int rc = LaunchGroup(g, steps, dt / steps, true);
			if (rc == DTRL_OK) rc = DeviceFrameWork(g);
			if (rc != DTRL_OK) return rc;
		}
		return DTRL_OK;
	}
	std::vector<int> done(G, 0);
	for (int g = 0; g < G; ++g) { int rc = LaunchGroup(g, steps, dt / steps, true); if (rc != DTRL_OK) return rc; }
	int next = 0;   // oldest outstanding launch (launch order is round-robin)
	for (int remaining = G * frames; remaining > 0;) {
		// serve whichever group has finished its frame; if none has, block on the oldest launch
		int g = -1;
		for (int k = 0; k < G; ++k) { const int c = (next + k) % G; if (done[c] < frames && be_->StreamIdle(c)) { g = c; break; } }
		if (g < 0) { for (int k = 0; k < G; ++k) { const int c = (next + k) % G; if (done[c] < frames) { g = c; break; } } }
		int rc = HostFrameWork(g);
		if (rc != DTRL_OK) return rc;
		--remaining;
		if (++done[g] < frames) { rc = LaunchGroup(g, steps, dt / steps, true); if (rc != DTRL_OK) return rc; }
		if (g == next) next = (next + 1) % G;
	}
	return DTRL_OK;
}

int Engine::Reset(const int32_t* env_ids, int n, const uint64_t* seeds)
{
	if (env_ids && n < 0) return Fail(DTRL_ERR_ARG, "negative env count");
	be_->Sync();
	const int cnt = env_ids ? n : n_;
	reset_ids_.clear();
	// an env listed twice is reset once (its first seed wins): the reset list feeds buffers sized for num_envs entries
	std::vector<char> seen(static_cast<size_t>(n_), 0);
	for (int i = 0; i < cnt; ++i) {
		int e = EnvIndex(env_ids, i);
		if (e < 0 || e >= n_) return Fail(DTRL_ERR_ARG, "env id out of range");
		if (seen[e]) continue;
		seen[e] = 1;
		if (cfg_.device_terrain) {
			if (seeds) {   // a fresh stream for this env (cGroundVar2D::SeedRand)
				GroundGen gg; gg.key = terrain_stream_key(seeds[i], 0); gg.ctr = 0; gg.builds = 0; gg.overflow = 0;
				if (!be_->H2D(&buf_.gen[e], &gg, sizeof(uint64_t) * 2)) return Fail(DTRL_ERR_DEVICE, be_->error());
			}
			reset_ids_.push_back(e);
			continue;
		}
		GroundWindow& g = grounds_[e];
		if (ladder_on_) tg_ladder_step(ladder_.host[e], terrain_keys_.env_key[e], status_[e], ladder_cfg_, 1, e);   // (device terrain: the boundary launch below does it)
		if (seeds) g.SeedRand(static_cast<unsigned long>(seeds[i]));
		g.Clear();
		g.Update(-kViewDist + kGroundSpawnOffset, kViewDist + kGroundSpawnOffset);
		if (!UploadGround(e)) return DTRL_ERR_CAPACITY;
		reset_ids_.push_back(e);
	}
	return StartEpisodes(reset_ids_, true, 1);   // every rule once per listed env, the draws included: the reset runs under the new model
}

int Engine::StartEpisodes(const std::vector<int32_t>& ids, bool draw_models, int terrain_mode)
{
	if (!ids.empty()) {
		const int32_t* list = StageIds(ids);
		if (!list) return DTRL_ERR_DEVICE;
		const EnvSpan span{0, static_cast<int>(ids.size()), list};
		if (cfg_.device_terrain && !Boundary(span, terrain_mode)) return Fail(DTRL_ERR_DEVICE, be_->error());
		if (draw_models) {
			if (int rc = RedrawListed(ids); rc != DTRL_OK) return rc;
			if (!RescaleQueue(nullptr, span)) return Fail(DTRL_ERR_DEVICE, be_->error());
		}
		if (int rc = ApplyResets(ids, -1, list); rc != DTRL_OK) return rc;
		if (!PushQueue(nullptr, span) || !EpisodeQueue(nullptr, span) || !LogQueue(nullptr, span, -1)) return Fail(DTRL_ERR_DEVICE, be_->error());
	}
	return DevOk(be_->Sync());
}

// device weight layout (dtrl_kernel.h conv_tile / fc_partial / fc_layer) as an index map into the caller's blob (Caffe blob order of the deploy net, W then b
// per layer): conv blobs [cout][cin][k] -> [cin][k][cout]; InnerProduct blobs [nout][nin] -> [ceil(nin/4)][nout][4] (zero padded); biases
// unchanged; same blob order. -1 = a padding / zero entry. CACLA actor: the all-zero critic head (val_ip0, val_ip1) is inserted behind the
// trunk so that the device sees a one-fragment MACE net; the boundary keeps the actor's blob order and sizes.
void Engine::BuildRelayoutMap(std::vector<int32_t>& map) const
{
	const NetDesc& d = cfg_.net;
	map.assign(static_cast<size_t>(DevNumParams(d)), -1);
	const size_t n_user = static_cast<size_t>(cfg_.user_num_params);
	const size_t head = static_cast<size_t>(d.fc_head) * d.fc_trunk + d.fc_head + d.fc_head + 1;
	const size_t tail = static_cast<size_t>(d.fc_head) * d.fc_trunk + d.fc_head + static_cast<size_t>(d.frag_size) * d.fc_head + d.frag_size;   // ip2, output
	// index into the MACE-ordered (padded) blob -> index into the caller's blob
	auto user = [&](size_t p) -> int32_t {
		if (!cfg_.actor_only) return static_cast<int32_t>(p);
		if (p < n_user - tail) return static_cast<int32_t>(p);
		if (p < n_user - tail + head) return -1;
		return static_cast<int32_t>(p - head);
	};
	size_t src = 0, dst = 0; int cin = 1, wdt = d.n_terrain;
	for (int l = 0; l < 3; ++l) {
		const int co = d.conv_ch[l], k = d.conv_k[l];
		for (int o = 0; o < co; ++o) for (int c = 0; c < cin; ++c) for (int u = 0; u < k; ++u)
			map[dst + (static_cast<size_t>(c) * k + u) * co + o] = user(src + (static_cast<size_t>(o) * cin + c) * k + u);
		src += static_cast<size_t>(co) * cin * k; dst += static_cast<size_t>(pad4(static_cast<int64_t>(co) * cin * k));
		for (int o = 0; o < co; ++o) map[dst + o] = user(src + o);
		src += co; dst += static_cast<size_t>(pad4(co)); cin = co; wdt = wdt - k + 1;
	}
	auto block = [&](int nout, int nin) {
		for (int o = 0; o < nout; ++o) for (int i = 0; i < nin; ++i)
			map[dst + (static_cast<size_t>(i / 4) * nout + o) * 4 + (i % 4)] = user(src + static_cast<size_t>(o) * nin + i);
		src += static_cast<size_t>(nout) * nin; dst += static_cast<size_t>(fc_dev_size(nout, nin));
		for (int o = 0; o < nout; ++o) map[dst + o] = user(src + o);
		src += nout; dst += static_cast<size_t>(pad4(nout));
	};
	{
		// terr_ip0 consumes conv2's output tile by tile (dtrl_kernel.h nn_eval): input (c, t) of Caffe's channel-major flattening sits at
		// tile * cin * V + c * vt + (t - tile * V), V positions per tile (vt in the last one)
		const int nout = d.fc_terr, V = kConvTile - (d.conv_k[1] - 1) - (d.conv_k[2] - 1);
		for (int o = 0; o < nout; ++o) for (int c = 0; c < cin; ++c) for (int t = 0; t < wdt; ++t) {
			const int tile = t / V, vt = std::min(V, wdt - tile * V);
			const size_t i = static_cast<size_t>(tile) * cin * V + static_cast<size_t>(c) * vt + (t - tile * V);
			map[dst + ((i / 4) * nout + o) * 4 + (i % 4)] = user(src + static_cast<size_t>(o) * cin * wdt + static_cast<size_t>(c) * wdt + t);
		}
		src += static_cast<size_t>(nout) * cin * wdt; dst += static_cast<size_t>(fc_dev_size(nout, cin * wdt));
		for (int o = 0; o < nout; ++o) map[dst + o] = user(src + o);
		src += nout; dst += static_cast<size_t>(pad4(nout));
	}
	block(d.fc_trunk, d.fc_terr + d.n_char);
	block(d.fc_head, d.fc_trunk); block(d.n_frags, d.fc_head);
	for (int f = 0; f < d.n_frags; ++f) { block(d.fc_head, d.fc_trunk); block(d.frag_size, d.fc_head); }
}

int Engine::SetPolicy(const float* w, size_t n, const double* io, const double* is, const double* oo, const double* os)
{
	if (cfg_.external_policy) return Fail(DTRL_ERR_ARG, "dtrl_set_policy: not available with -policy_mode= external (the caller's policy decides: dtrl_pending_actions / dtrl_supply_actions; no policy net runs inside the frame kernel)");
	if (!cfg_.has_policy_net) return Fail(DTRL_ERR_ARG, "no -policy_net= in the arguments: this batch has no network");
	const NetDesc& d = cfg_.net;
	if (!w || n != static_cast<size_t>(cfg_.user_num_params)) return Fail(DTRL_ERR_ARG, "weight count does not match the deploy prototxt");
	be_->Sync();
	if (!policy_wait_.empty()) { if (!be_->SyncPolicyReady()) return Fail(DTRL_ERR_DEVICE, be_->error()); policy_wait_.assign(policy_wait_.size(), 0); }   // (an asynchronous hand-over still on its way: let it land, then supersede it)
	policy_flip_pending_ = false;   // (a deferred device hand-over is superseded)
	std::vector<float> dev_w(relayout_.size());
	for (size_t i = 0; i < relayout_.size(); ++i) dev_w[i] = relayout_[i] >= 0 ? w[relayout_[i]] : 0.0f;
	// CACLA actor: a neutral critic slot in front of the output normalisers (the device net's one zero critic output)
	const int pad = d.out_size - cfg_.user_out_size;
	// cNeuralNet without a scale file: identity normalisation (learning/NeuralNet.cpp:925-933) for every vector passed as NULL
	if (io) in_off_.assign(io, io + d.in_size); else in_off_.assign(d.in_size, 0.0);
	if (is) in_scale_.assign(is, is + d.in_size); else in_scale_.assign(d.in_size, 1.0);
	out_off_.assign(d.out_size, 0.0); out_scale_.assign(d.out_size, 1.0);
	if (oo) std::copy(oo, oo + cfg_.user_out_size, out_off_.begin() + pad);
	if (os) std::copy(os, os + cfg_.user_out_size, out_scale_.begin() + pad);
	if (!be_->H2D(const_cast<float*>(buf_.weights), dev_w.data(), sizeof(float) * dev_w.size())) return Fail(DTRL_ERR_DEVICE, be_->error());
	int rc = UploadNormalizers();
	if (rc != DTRL_OK) return rc;
	policy_set_ = true;
	return DTRL_OK;
}

// dtrl_set_policy with every pointer in DEVICE memory (the trainer's own tensors): no host round trip. Weights are gathered into the
// device layout by a kernel; NULL normalisers keep their current values.
// While a frame is in flight (between dtrl_step_begin and dtrl_step_end) a weights-only hand-over does NOT wait for it: the weights are gathered into a
// second buffer on the drain stream and the kernels switch to it with the next frame launch (the same moment the synchronous path would have taken effect).
void Engine::ApplyPendingPolicy()
{
	if (!policy_flip_pending_) return;
	const float* cur = buf_.weights; buf_.weights = weights_alt_; weights_alt_ = const_cast<float*>(cur);
	policy_flip_pending_ = false;
}
// dtrl_set_policy_device_async: the weights-only hand-over with NO host wait at all. The gather into the second weight buffer is queued on the caller's
// stream (behind whatever produced w_dev there: a broadcast, the trainer's last step), every env group's NEXT launch waits for it on the device and switches
// to the buffer. Valid at any time (frame in flight or not); w_dev must stay unchanged until the caller's stream has passed this point.
int Engine::SetPolicyDeviceAsync(const float* w_dev, size_t n, void* stream)
{
	if (cfg_.external_policy) return Fail(DTRL_ERR_ARG, "dtrl_set_policy_device_async: not available with -policy_mode= external (the caller's policy decides: dtrl_pending_actions / dtrl_supply_actions; no policy net runs inside the frame kernel)");
	if (!cfg_.has_policy_net) return Fail(DTRL_ERR_ARG, "no -policy_net= in the arguments: this batch has no network");
	if (!w_dev || n != static_cast<size_t>(cfg_.user_num_params)) return Fail(DTRL_ERR_ARG, "weight count does not match the deploy prototxt");
	if (!policy_set_ || !weights_alt_) return Fail(DTRL_ERR_ARG, "dtrl_set_policy_device_async needs a policy (normalisers) installed by dtrl_set_policy / dtrl_set_policy_device first");
	if (!stream && std::string(be_->Name()) == "hip") return Fail(DTRL_ERR_ARG, "dtrl_set_policy_device_async: a stream (hipStream_t) of the caller's is required");
	// a second asynchronous hand-over before any launch consumed the first: the first gather may still be writing the same buffer from another stream
	if (policy_flip_pending_ && !policy_wait_.empty() && !be_->SyncPolicyReady()) return Fail(DTRL_ERR_DEVICE, be_->error());
	if (!be_->WaitWeightReaders(stream, weights_alt_ == weights_buf0_ ? 0 : 1, static_cast<int>(groups_.size()))) return Fail(DTRL_ERR_DEVICE, be_->error());
	if (!be_->GatherF32Async(stream, weights_alt_, w_dev, d_relayout_, relayout_.size())) return Fail(DTRL_ERR_DEVICE, be_->error());
	policy_flip_pending_ = true;
	policy_wait_.assign(groups_.size(), 1);
	return DTRL_OK;
}
int Engine::SetPolicyDevice(const float* w_dev, size_t n, const double* io_dev, const double* is_dev, const double* oo_dev, const double* os_dev, void* stream)
{
	if (cfg_.external_policy) return Fail(DTRL_ERR_ARG, "dtrl_set_policy_device: not available with -policy_mode= external (the caller's policy decides: dtrl_pending_actions / dtrl_supply_actions; no policy net runs inside the frame kernel)");
	if (!cfg_.has_policy_net) return Fail(DTRL_ERR_ARG, "no -policy_net= in the arguments: this batch has no network");
	const NetDesc& d = cfg_.net;
	if (!w_dev || n != static_cast<size_t>(cfg_.user_num_params)) return Fail(DTRL_ERR_ARG, "weight count does not match the deploy prototxt");
	if (step_pending_ && policy_set_ && weights_alt_ && !io_dev && !is_dev && !oo_dev && !os_dev) {
		struct Restore { Backend* b; ~Restore() { b->SelectStream(0); } } restore{be_};
		be_->SelectStream(be_->NumStreams() - 1);
		// an ASYNCHRONOUS hand-over (dtrl_set_policy_device_async) may still be gathering into this very buffer on another stream: order behind it, and drop the
		// frame launches' wait on its event -- this gather is the newer one
		if (!policy_wait_.empty()) { if (!be_->SyncPolicyReady()) return Fail(DTRL_ERR_DEVICE, be_->error()); policy_wait_.assign(policy_wait_.size(), 0); }
		// (synchronised: the caller may change w_dev when this returns. On the caller's stream -- the trainer's -- the gather follows the steps queued there and
		// ONE wait covers both; on the drain stream it would wait for a wavefront slot of its own behind the frame in flight)
		// a frame kernel may still be READING the buffer about to be overwritten: a group dtrl_step_poll relaunched ran its launch on the buffer that the
		// flip in the following dtrl_step_end_begin turned into weights_alt_ (that call skips the group without a sync), and in -terrain_gen= device mode no
		// frame is ever waited for on the host. The gather waits on the device for every group's latest reader of this buffer (events of launches that have
		// completed cost nothing; in host terrain mode without dtrl_step_poll they always have).
		if (!be_->WaitWeightReaders(stream, weights_alt_ == weights_buf0_ ? 0 : 1, static_cast<int>(groups_.size()))) return Fail(DTRL_ERR_DEVICE, be_->error());
		if (!be_->GatherF32On(stream, weights_alt_, w_dev, d_relayout_, relayout_.size())) return Fail(DTRL_ERR_DEVICE, be_->error());
		policy_flip_pending_ = true;
		return DTRL_OK;
	}
	be_->Sync();
	if (!policy_wait_.empty()) { if (!be_->SyncPolicyReady()) return Fail(DTRL_ERR_DEVICE, be_->error()); policy_wait_.assign(policy_wait_.size(), 0); }   // an asynchronous hand-over still on its way
	ApplyPendingPolicy();
	if (!be_->GatherF32(const_cast<float*>(buf_.weights), w_dev, d_relayout_, relayout_.size())) return Fail(DTRL_ERR_DEVICE, be_->error());
	if (in_off_.empty()) { in_off_.assign(d.in_size, 0.0); in_scale_.assign(d.in_size, 1.0); out_off_.assign(d.out_size, 0.0); out_scale_.assign(d.out_size, 1.0); int rc = UploadNormalizers(); if (rc != DTRL_OK) return rc; }
	const int pad = d.out_size - cfg_.user_out_size;
	bool ok = true;
	if (sizeof(real) != sizeof(double) && (io_dev || is_dev || oo_dev || os_dev)) return Fail(DTRL_ERR_ARG, "the fp32 build takes device-resident WEIGHTS only; hand the normalisers over through dtrl_set_policy (host doubles)");
	if (io_dev) ok = ok && be_->D2D(const_cast<real*>(buf_.in_off), io_dev, sizeof(real) * d.in_size) && be_->D2H(in_off_.data(), buf_.in_off, sizeof(real) * d.in_size);
	if (is_dev) ok = ok && be_->D2D(const_cast<real*>(buf_.in_scale), is_dev, sizeof(real) * d.in_size) && be_->D2H(in_scale_.data(), buf_.in_scale, sizeof(real) * d.in_size);
	if (oo_dev) ok = ok && be_->D2D(const_cast<real*>(buf_.out_off) + pad, oo_dev, sizeof(real) * cfg_.user_out_size) && be_->D2H(out_off_.data(), buf_.out_off, sizeof(real) * d.out_size);
	if (os_dev) ok = ok && be_->D2D(const_cast<real*>(buf_.out_scale) + pad, os_dev, sizeof(real) * cfg_.user_out_size) && be_->D2H(out_scale_.data(), buf_.out_scale, sizeof(real) * d.out_size);
	if (!ok) return Fail(DTRL_ERR_DEVICE, be_->error());
	policy_set_ = true;
	return DTRL_OK;
}

int Engine::UploadNormalizers()
{
	const NetDesc& d = cfg_.net;
	// (the host copies are double whatever the kernel's arithmetic type: dtrl_types.h `real`)
	const std::vector<real> a(in_off_.begin(), in_off_.end()), b(in_scale_.begin(), in_scale_.end()), c(out_off_.begin(), out_off_.end()), e(out_scale_.begin(), out_scale_.end());
	bool ok = be_->H2D(const_cast<real*>(buf_.in_off), a.data(), sizeof(real) * d.in_size)
		&& be_->H2D(const_cast<real*>(buf_.in_scale), b.data(), sizeof(real) * d.in_size)
		&& be_->H2D(const_cast<real*>(buf_.out_off), c.data(), sizeof(real) * d.out_size)
		&& be_->H2D(const_cast<real*>(buf_.out_scale), e.data(), sizeof(real) * d.out_size);
	return ok ? DTRL_OK : Fail(DTRL_ERR_DEVICE, be_->error());
}

// cNeuralNet::LoadScale, learning/NeuralNet.cpp:137-215
int Engine::LoadScaleFile(const char* path)
{
	if (cfg_.external_policy) return Fail(DTRL_ERR_ARG, "dtrl_load_scale_file: not available with -policy_mode= external (the caller's policy decides: dtrl_pending_actions / dtrl_supply_actions; no policy net runs inside the frame kernel)");
	if (!cfg_.has_policy_net) return Fail(DTRL_ERR_ARG, "no -policy_net= in the arguments: this batch has no network");
	if (!path) return Fail(DTRL_ERR_ARG, "null path");
	const NetDesc& d = cfg_.net;
	Json root; std::string err;
	if (!Json::parse_file(path, root, err)) return Fail(DTRL_ERR_IO, std::string("Failed to read scale file ") + path + ": " + err);
	if (in_off_.empty()) { in_off_.assign(d.in_size, 0.0); in_scale_.assign(d.in_size, 1.0); out_off_.assign(d.out_size, 0.0); out_scale_.assign(d.out_size, 1.0); }
	struct Slot { const char* key; std::vector<double>* vec; int size; const char* what; };
	const Slot slots[4] = {{"InputOffset", &in_off_, d.in_size, "input offset"}, {"InputScale", &in_scale_, d.in_size, "input scale"},
		{"OutputOffset", &out_off_, cfg_.user_out_size, "output offset"}, {"OutputScale", &out_scale_, cfg_.user_out_size, "output scale"}};
	const int pad = d.out_size - cfg_.user_out_size;   // CACLA actor: 1 (the unused critic slot of the device net), else 0
	std::vector<double> tmp[4];
	for (int k = 0; k < 4; ++k) {
		const Json* j = root.find(slots[k].key);
		if (!j || j->type == Json::kNull) continue;
		if (j->type != Json::kArr) return Fail(DTRL_ERR_IO, std::string(slots[k].key) + " is not an array in " + path);
		if (static_cast<int>(j->arr.size()) != slots[k].size)
			return Fail(DTRL_ERR_IO, std::string("Invalid ") + slots[k].what + " size, expecting " + std::to_string(slots[k].size) + ", but got " + std::to_string(j->arr.size()));
		for (const Json& v : j->arr) tmp[k].push_back(v.num);
	}
	for (int k = 0; k < 4; ++k) if (!tmp[k].empty()) { if (k >= 2 && pad) tmp[k].insert(tmp[k].begin(), pad, k == 2 ? 0.0 : 1.0); *slots[k].vec = tmp[k]; }
	be_->Sync();
	return UploadNormalizers();
}

// cNeuralNet::WriteOffsetScale, learning/NeuralNet.cpp:1182-1205 (cJsonUtil::BuildVectorJson: std::to_string per element)
int Engine::WriteScaleFile(const char* path)
{
	if (!cfg_.has_policy_net) return Fail(DTRL_ERR_ARG, "no -policy_net= in the arguments: this batch has no network");
	const NetDesc& d = cfg_.net;
	if (in_off_.empty()) { in_off_.assign(d.in_size, 0.0); in_scale_.assign(d.in_size, 1.0); out_off_.assign(d.out_size, 0.0); out_scale_.assign(d.out_size, 1.0); }
	FILE* f = path ? std::fopen(path, "w") : nullptr;
	if (!f) return Fail(DTRL_ERR_IO, std::string("Failed to write offset and scale to ") + (path ? path : "(null)"));
	auto vec_json = [](const std::vector<double>& v) { std::string s = "["; for (size_t i = 0; i < v.size(); ++i) { if (i) s += ", "; s += std::to_string(v[i]); } return s + "]"; };
	std::fprintf(f, "{\n\"InputOffset\": %s,\n\"InputScale\": %s,\n\"OutputOffset\": %s,\n\"OutputScale\": %s\n}",
		vec_json(in_off_).c_str(), vec_json(in_scale_).c_str(),
		vec_json(std::vector<double>(out_off_.begin() + (d.out_size - cfg_.user_out_size), out_off_.end())).c_str(),
		vec_json(std::vector<double>(out_scale_.begin() + (d.out_size - cfg_.user_out_size), out_scale_.end())).c_str());
	std::fclose(f);
	return DTRL_OK;
}

int Engine::SetExplore(int enable, double rate, double temp, double base_rate)
{
	cfg_.run.enable_exp = enable ? 1 : 0; cfg_.run.exp_rate = rate; cfg_.run.exp_temp = temp; cfg_.run.exp_base_rate = base_rate;
	return DTRL_OK;
}

int Engine::SetTerrainLerp(double lerp)
{
	double params[kNumTerrainParams];
	LerpTerrainParams(cfg_, lerp, params);
	terrain_lerp_ = lerp;
	if (!terrain_table_.empty()) terrain_table_[0] = MakeTerrainCfg(cfg_.terrain_type, params);   // terrain sets: this is entry 0, and only its envs move
	if (cfg_.device_terrain) return UploadTerrainCfg(params);
	for (int e = 0; e < n_; ++e) if (terrain_table_.empty() || terrain_keys_.env_key[e] == 0) grounds_[e].SetParams(params);   // takes effect at the next segment build, as in the reference
	return DTRL_OK;
}

// ---- tuple rings. Without pipelining there is one ring and every drain waits for all streams. With it (SetTuplePipelining) dtrl_step_begin switches
// the ring the kernels write; between dtrl_step_begin and dtrl_step_end the drains below work on the OTHER ring (the frame that has ended), on a stream of
// their own, and do not wait for the frame in flight.
bool Engine::AllocRing(TupleRing& r)
{
	const size_t rb = sizeof(float) * static_cast<size_t>(W_) * buf_.tuple_cap, fb = sizeof(uint32_t) * static_cast<size_t>(buf_.tuple_cap), eb = sizeof(int32_t) * static_cast<size_t>(buf_.tuple_cap), cb = sizeof(int32_t) * 4;
	auto get = [&](size_t bytes) -> void* {
		void* p = cfg_.tuple_ring_host ? be_->HostStaging(bytes) : be_->Alloc(bytes);
		if (!p) return nullptr;
		if (cfg_.tuple_ring_host) { std::memset(p, 0, bytes); host_allocs_.push_back(p); } else allocs_.push_back(p);
		return p;
	};
	r.rows = static_cast<float*>(get(rb)); r.flags = static_cast<uint32_t*>(get(fb)); r.env = static_cast<int32_t*>(get(eb));
	r.count = static_cast<int32_t*>(get(cb));   // [0] ring cursor, [1] / [2] rows drained / dropped by packed drains since the last fold
	return r.rows && r.flags && r.env && r.count;
}
// the ring's words as the host sees them: a plain read / write when the ring is host memory (no kernel is using it: callers hold DrainSync), else a copy
bool Engine::RingRead(void* dst, const void* src, size_t n) { if (cfg_.tuple_ring_host) { std::memcpy(dst, src, n); return true; } return be_->D2H(dst, src, n); }
bool Engine::RingWrite(void* dst, const void* src, size_t n) { if (cfg_.tuple_ring_host) { std::memcpy(dst, src, n); return true; } return be_->H2D(dst, src, n); }
int Engine::SetTuplePipelining(bool on)
{
	if (on && cfg_.external_policy) return Fail(DTRL_ERR_ARG, "dtrl_set_tuple_pipelining(1): not available with -policy_mode= external (a tick is not a frame: envs complete their frames in different ticks, so no ring is ever idle)");
	if (step_pending_) return Fail(DTRL_ERR_ARG, "dtrl_set_tuple_pipelining between dtrl_step_begin and dtrl_step_end");
	if (!be_->Sync()) return Fail(DTRL_ERR_DEVICE, be_->error());
	if (on && !ring_[1].rows) {
		if (!AllocRing(ring_[1])) return Fail(DTRL_ERR_DEVICE, "tuple ring allocation failed: " + be_->error());
	}
	if (!on && tuple_pipelining_) {
		// back to one ring: whatever waits in the idle ring would be stranded
		DevBuffers o = buf_; UseRing(o, wr_ring_ ^ 1);
		int32_t cnt = 0;
		if (!RingRead(&cnt, o.tuple_count, sizeof(cnt))) return Fail(DTRL_ERR_DEVICE, be_->error());
		if (cnt != 0) return Fail(DTRL_ERR_ARG, "drain the pending tuples before switching tuple pipelining off");
	}
	tuple_pipelining_ = on;
	return DTRL_OK;
}
// DrainSync failed: an API-order error (a drain while dtrl_step_poll's early relaunches hold both rings) is DTRL_ERR_ARG, anything else a device error
int Engine::DrainFail()
{
	if (drain_order_error_) { drain_order_error_ = false; return Fail(DTRL_ERR_ARG, err_); }
	return Fail(DTRL_ERR_DEVICE, be_->error());
}
bool Engine::DrainSync()
{
	if (early_any_) { err_ = "tuple rings are both in use: dtrl_step_poll relaunched a group; call dtrl_step_end_begin first"; drain_order_error_ = true; return false; }
	if (tuple_pipelining_ && step_pending_) {   // the drain ring's frame ended with dtrl_step_end; the frame in flight writes the other ring
		// "ended" is a host-side fact only in host terrain mode (HostFrameWork synchronises the group's stream). In device terrain mode the frame may
		// still be running: the drain stream waits on the device for the mark behind every group's launch of that frame -- a torn row (the cursor is
		// bumped before the row is written) or a cursor zeroed under a running kernel would lose, duplicate or reorder tuples without an error.
		be_->SelectStream(be_->NumStreams() - 1);
		return be_->WaitFrames(DrainRing(), static_cast<int>(groups_.size())) && be_->SyncSelected();
	}
	be_->SelectStream(0);
	return be_->Sync();
}
// rows the kernel could not store because the ring was full are counted, never silently lost: the cursor keeps counting past the capacity
int Engine::PendingTuples(int32_t* stored, int32_t* overflow)
{
	int32_t cnt = 0;
	DevBuffers d = buf_; UseRing(d, DrainRing());
	struct Restore { Backend* b; ~Restore() { b->SelectStream(0); } } restore{be_};
	if (!DrainSync()) return DrainFail();
	if (!RingRead(&cnt, d.tuple_count, sizeof(cnt))) return Fail(DTRL_ERR_DEVICE, be_->error());
	*overflow = cnt > buf_.tuple_cap ? cnt - buf_.tuple_cap : 0;
	*stored = cnt - *overflow;
	return DTRL_OK;
}
int Engine::DrainTuples(float* rows, uint32_t* flags, int32_t* env_ids, int cap, int* out_n, bool device_dst)
{
	if (cap < 0 || !out_n || (cap > 0 && !rows)) return Fail(DTRL_ERR_ARG, "bad arguments");
	DevBuffers d = buf_; UseRing(d, DrainRing());
	struct Restore { Backend* b; ~Restore() { b->SelectStream(0); } } restore{be_};
	// Host destination: everything goes through ONE page-locked staging area with two synchronisations (the count; then rows + flags + ids + the cursor's reset
	// queued together) -- a copy into pageable caller memory is a staged, synchronous affair per call in the runtime (five of them before; with frames in
	// flight each could wait for a wavefront slot).
	if (cfg_.tuple_ring_host && !device_dst) {
		const double ht0 = g_ht.on ? now_s() : 0;
		if (!DrainSync()) return DrainFail();
		const double ht1 = g_ht.on ? now_s() : 0;
		const int32_t cnt_all = *d.tuple_count;
		const int32_t over = cnt_all > buf_.tuple_cap ? cnt_all - buf_.tuple_cap : 0;
		const int n = std::min<int>(cnt_all - over, cap);
		if (n < cnt_all - over) return Fail(DTRL_ERR_CAPACITY, "caller buffer smaller than the number of pending tuples");
		if (n > 0) {
			std::memcpy(rows, d.tuple_rows, sizeof(float) * static_cast<size_t>(W_) * n);
			if (flags) std::memcpy(flags, d.tuple_flags, sizeof(uint32_t) * static_cast<size_t>(n));
			if (env_ids) std::memcpy(env_ids, d.tuple_env, sizeof(int32_t) * static_cast<size_t>(n));
		}
		*d.tuple_count = 0;
		tuples_drained_ += n; tuples_dropped_ += over;
		*out_n = n;
		if (g_ht.on) { g_ht.d_wait += ht1 - ht0; g_ht.d_copy += now_s() - ht1; ++g_ht.d_n; }
		return DTRL_OK;
	}
	if (!pin_drain_) {
		pin_drain_bytes_ = 64 + (sizeof(float) * static_cast<size_t>(W_) + sizeof(uint32_t) + sizeof(int32_t)) * static_cast<size_t>(buf_.tuple_cap);
		pin_drain_ = static_cast<char*>(be_->HostStaging(pin_drain_bytes_));
		if (!pin_drain_) return Fail(DTRL_ERR_DEVICE, "host staging allocation failed: " + be_->error());
		std::memset(pin_drain_, 0, 64);
	}
	int32_t* p_cnt = reinterpret_cast<int32_t*>(pin_drain_); int32_t* p_zero = p_cnt + 1;   // (p_zero stays 0)
	const double ht0 = g_ht.on ? now_s() : 0;
	if (!DrainSync()) return DrainFail();
	const double ht1 = g_ht.on ? now_s() : 0;
	if (cfg_.tuple_ring_host) *p_cnt = *d.tuple_count;      // (device destination, host ring)
	else if (!be_->D2HAsync(p_cnt, d.tuple_count, sizeof(int32_t)) || !be_->SyncSelected()) return Fail(DTRL_ERR_DEVICE, be_->error());
	const double ht2 = g_ht.on ? now_s() : 0;
	const int32_t cnt_all = *p_cnt;
	const int32_t over = cnt_all > buf_.tuple_cap ? cnt_all - buf_.tuple_cap : 0;
	const int32_t cnt = cnt_all - over;
	const int n = std::min<int>(cnt, cap);
	if (n < cnt) return Fail(DTRL_ERR_CAPACITY, "caller buffer smaller than the number of pending tuples");
	const size_t rb = sizeof(float) * static_cast<size_t>(W_) * n, fb = sizeof(uint32_t) * static_cast<size_t>(n), eb = sizeof(int32_t) * static_cast<size_t>(n);
	char* p_rows = pin_drain_ + 64; char* p_flags = p_rows + sizeof(float) * static_cast<size_t>(W_) * buf_.tuple_cap; char* p_env = p_flags + sizeof(uint32_t) * static_cast<size_t>(buf_.tuple_cap);
	bool ok = true;
	if (n > 0) {
		if (device_dst) {
			if (cfg_.tuple_ring_host) ok = be_->H2D(rows, d.tuple_rows, rb) && (!flags || be_->H2D(flags, d.tuple_flags, fb)) && (!env_ids || be_->H2D(env_ids, d.tuple_env, eb));
			else ok = be_->D2D(rows, d.tuple_rows, rb) && (!flags || be_->D2D(flags, d.tuple_flags, fb)) && (!env_ids || be_->D2D(env_ids, d.tuple_env, eb));
		} else {
			ok = be_->D2HAsync(p_rows, d.tuple_rows, rb) && (!flags || be_->D2HAsync(p_flags, d.tuple_flags, fb)) && (!env_ids || be_->D2HAsync(p_env, d.tuple_env, eb));
		}
	}
	if (cfg_.tuple_ring_host) { ok = ok && be_->SyncSelected(); *d.tuple_count = 0; }
	else ok = ok && be_->H2DAsync(d.tuple_count, p_zero, sizeof(int32_t)) && be_->SyncSelected();
	if (!ok) return Fail(DTRL_ERR_DEVICE, be_->error());
	if (n > 0 && !device_dst) {
		std::memcpy(rows, p_rows, rb);
		if (flags) std::memcpy(flags, p_flags, fb);
		if (env_ids) std::memcpy(env_ids, p_env, eb);
	}
	tuples_drained_ += n; tuples_dropped_ += over;
	*out_n = n;
	if (g_ht.on) { g_ht.d_wait += ht1 - ht0; g_ht.d_count += ht2 - ht1; g_ht.d_copy += now_s() - ht2; ++g_ht.d_n; }
	return DTRL_OK;
}
// totals of the device-side (packed) drains -> host counters
int Engine::FoldTupleTotals()
{
	struct Restore { Backend* b; ~Restore() { b->SelectStream(0); } } restore{be_};
	if (!DrainSync()) return DrainFail();
	for (int r = 0; r < 2; ++r) {
		if (!ring_[r].count || (tuple_pipelining_ && step_pending_ && r == wr_ring_)) continue;   // (the ring in flight folds after its frame)
		int32_t c[4] = {0, 0, 0, 0};
		if (!RingRead(c, ring_[r].count, sizeof(c))) return Fail(DTRL_ERR_DEVICE, be_->error());
		if (c[1] || c[2]) {
			tuples_drained_ += c[1]; tuples_dropped_ += c[2];
			const int32_t zero[2] = {0, 0};
			if (!RingWrite(ring_[r].count + 1, zero, sizeof(zero))) return Fail(DTRL_ERR_DEVICE, be_->error());
		}
	}
	return DTRL_OK;
}
int Engine::DrainTuplesPacked(float* block_dev, int block_rows, int* out_n)
{
	if (!block_dev || block_rows < 0) return Fail(DTRL_ERR_ARG, "bad arguments");
	DevBuffers d = buf_; UseRing(d, DrainRing());
	struct Restore { Backend* b; ~Restore() { b->SelectStream(0); } } restore{be_};
	if (!pack_.order) {
		auto alloc = [&](size_t bytes) -> void* { void* p = be_->Alloc(bytes); if (p) allocs_.push_back(p); return p; };
		const size_t cap = static_cast<size_t>(buf_.tuple_cap);
		pack_.order = static_cast<int32_t*>(alloc(sizeof(int32_t) * cap));
		pack_.hist = static_cast<int32_t*>(alloc(sizeof(int32_t) * (static_cast<size_t>(n_) + 1)));
		pack_.meta = static_cast<int32_t*>(alloc(sizeof(int32_t) * 4));
		pack_.rows = static_cast<float*>(alloc(sizeof(float) * static_cast<size_t>(W_) * cap));
		pack_.flags = static_cast<uint32_t*>(alloc(sizeof(uint32_t) * cap));
		pack_.env = static_cast<int32_t*>(alloc(sizeof(int32_t) * cap));
		if (!pack_.order || !pack_.hist || !pack_.meta || !pack_.rows || !pack_.flags || !pack_.env || !be_->Sync()) { pack_ = PackScratch(); return Fail(DTRL_ERR_DEVICE, "device allocation failed: " + be_->error()); }
	}
	if (!DrainSync()) return DrainFail();   // the frame kernels that wrote this ring have finished
	if (!be_->PackTuples(d, block_dev, block_rows, cfg_.run.env_id_base, n_, pack_)) return Fail(DTRL_ERR_DEVICE, be_->error());
	if (out_n) { int32_t n = 0; if (!be_->D2H(&n, block_dev, sizeof(n))) return Fail(DTRL_ERR_DEVICE, be_->error()); *out_n = n; }
	return DTRL_OK;
}
int Engine::TupleStats(int64_t* pending, int64_t* drained, int64_t* dropped, int32_t* capacity)
{
	int32_t cnt = 0, over = 0;
	int rc = FoldTupleTotals();
	if (rc == DTRL_OK) rc = PendingTuples(&cnt, &over);
	if (rc != DTRL_OK) return rc;
	if (pending) *pending = cnt;
	if (drained) *drained = tuples_drained_;
	if (dropped) *dropped = tuples_dropped_ + over;
	if (capacity) *capacity = buf_.tuple_cap;
	return DTRL_OK;
}

// cScenarioPoliEval::GetDistLog for the batch: every recorded episode distance since Init / Clear, grouped by env (the order in which
// cOptScenarioPoliEval::OutputResults walks its pool, optimizer/scenarios/OptScenarioPoliEval.cpp:213-239), episodes of one env in time order
int Engine::GetDistLog(double* dist, int32_t* env_ids, int cap, int* out_n)
{
	if (!out_n || cap < 0) return Fail(DTRL_ERR_ARG, "bad arguments");
	{ int rc = DrainDeviceDistLog(); if (rc != DTRL_OK) return rc; }
	std::vector<std::pair<int32_t, double>> v = dist_log_;
	std::stable_sort(v.begin(), v.end(), [](const std::pair<int32_t, double>& a, const std::pair<int32_t, double>& b) { return a.first < b.first; });
	*out_n = static_cast<int>(v.size());
	for (int i = 0; i < *out_n && i < cap; ++i) { if (dist) dist[i] = v[i].second; if (env_ids) env_ids[i] = v[i].first; }
	return *out_n <= cap || (!dist && !env_ids) ? DTRL_OK : Fail(DTRL_ERR_CAPACITY, "caller buffer smaller than the dist log");
}
// cScenarioPoliEval::ResetAvgDist on every env: mAvgDist = 0, mEpisodeCount = 0 (the dist log and the cycle counters stay)
int Engine::ResetAvgDist()
{
	std::vector<EnvState> st;
	int rc = GetStates(nullptr, n_, st);
	if (rc != DTRL_OK) return rc;
	for (EnvState& s : st) { s.avg_dist = 0; s.num_episodes = 0; }
	if (!be_->H2D(buf_.st, st.data(), sizeof(EnvState) * n_)) return Fail(DTRL_ERR_DEVICE, be_->error());
	return DTRL_OK;
}

int Engine::GetStates(const int32_t* env_ids, int n, std::vector<EnvState>& out)
{
	if (n < 0) return Fail(DTRL_ERR_ARG, "negative env count");
	be_->Sync();
	out.resize(n);
	if (!env_ids) {
		if (n > n_) return Fail(DTRL_ERR_ARG, "env id out of range");
		if (!be_->D2H(out.data(), buf_.st, sizeof(EnvState) * n)) return Fail(DTRL_ERR_DEVICE, be_->error());
		return DTRL_OK;
	}
	for (int i = 0; i < n; ++i) {
		int e = env_ids[i];
		if (e < 0 || e >= n_) return Fail(DTRL_ERR_ARG, "env id out of range");
		if (!be_->D2H(&out[i], &buf_.st[e], sizeof(EnvState))) return Fail(DTRL_ERR_DEVICE, be_->error());
	}
	return DTRL_OK;
}

int Engine::SetPoseVel(const int32_t* env_ids, int n, const double* q, const double* qd)
{
	if (n < 0 || !q || !qd) return Fail(DTRL_ERR_ARG, "bad arguments");
	be_->Sync();
	const int D = cfg_.model.D;
	EnvState st;
	for (int i = 0; i < n; ++i) {
		int e = EnvIndex(env_ids, i);
		if (e < 0 || e >= n_) return Fail(DTRL_ERR_ARG, "env id out of range");
		if (!be_->D2H(&st, &buf_.st[e], sizeof(EnvState))) return Fail(DTRL_ERR_DEVICE, be_->error());
		for (int k = 0; k < D; ++k) { st.q[k] = q[i * D + k]; st.qd[k] = qd[i * D + k]; }
		// a teleported character drops its persistent contact rows (Bullet's refreshContactPoints removes manifold points that moved out of the breaking
		// threshold): cached impulses of the old pose would warm-start whichever sample points happen to touch in the new one. A caller that restores a
		// saved state calls dtrl_set_contact_cache AFTER this (include/dtrl.h)
		st.ws_R = 0;
		for (int k = 0; k < kMaxRows; ++k) { st.ws_id[k] = 0xffff; st.ws_lam[k] = 0.0; }
		if (!be_->H2D(&buf_.st[e], &st, sizeof(EnvState))) return Fail(DTRL_ERR_DEVICE, be_->error());
	}
	return DTRL_OK;
}

// the persistent contact points' identities and applied impulses (EnvState::ws_*; include/dtrl.h dtrl_get_contact_cache)
int Engine::GetContactCache(const int32_t* env_ids, int n, int32_t* count, int32_t* ids, double* lambda)
{
	if (n < 0 || !count || !ids || !lambda) return Fail(DTRL_ERR_ARG, "bad arguments");
	std::vector<EnvState> st; int rc = GetStates(env_ids, n, st);
	if (rc != DTRL_OK) return rc;
	const int cnt = static_cast<int>(st.size());
	for (int i = 0; i < cnt; ++i) {
		count[i] = st[i].ws_R;
		for (int k = 0; k < kMaxRows; ++k) { ids[i * kMaxRows + k] = k < st[i].ws_R ? st[i].ws_id[k] : 0xffff; lambda[i * kMaxRows + k] = k < st[i].ws_R ? st[i].ws_lam[k] : 0.0; }
	}
	return DTRL_OK;
}
int Engine::SetContactCache(const int32_t* env_ids, int n, const int32_t* count, const int32_t* ids, const double* lambda)
{
	if (n < 0 || !count || !ids || !lambda) return Fail(DTRL_ERR_ARG, "bad arguments");
	if (!env_ids && n > n_) return Fail(DTRL_ERR_ARG, "more rows than envs");
	be_->Sync();
	const int cnt = n;                       // env_ids == NULL: envs 0 .. n - 1, like dtrl_get_contact_cache and dtrl_set_pose_vel
	EnvState st;
	for (int i = 0; i < cnt; ++i) {
		const int e = EnvIndex(env_ids, i);
		if (e < 0 || e >= n_) return Fail(DTRL_ERR_ARG, "env id out of range");
		if (count[i] < 0 || count[i] > kMaxRows) return Fail(DTRL_ERR_ARG, "contact cache: row count out of range");
		if (!be_->D2H(&st, &buf_.st[e], sizeof(EnvState))) return Fail(DTRL_ERR_DEVICE, be_->error());
		st.ws_R = count[i];
		for (int k = 0; k < kMaxRows; ++k) {
			const bool on = k < count[i];
			if (on && (ids[i * kMaxRows + k] < 0 || ids[i * kMaxRows + k] > 0xffff)) return Fail(DTRL_ERR_ARG, "contact cache: row id out of range");
			st.ws_id[k] = on ? static_cast<uint16_t>(ids[i * kMaxRows + k]) : 0xffff; st.ws_lam[k] = on ? lambda[i * kMaxRows + k] : 0.0;
		}
		if (!be_->H2D(&buf_.st[e], &st, sizeof(EnvState))) return Fail(DTRL_ERR_DEVICE, be_->error());
	}
	return DTRL_OK;
}

// cCharController::CommandAction (sim/DogController.cpp:309-320, sim/RaptorController.cpp): the base action the controller takes at its next cycle instead
// of asking the policy. The reference keeps a STACK of commands (the latest is served first, older ones at later cycles); the engine keeps the top of
// that stack only -- one pending command per env, a new one replaces it (cScenarioExp::Reset's random first action, scenarios/ScenarioExp.cpp:63-73,
// sits in the same slot).
int Engine::CommandAction(const int32_t* env_ids, int n, const int32_t* action_ids)
{
	if ((env_ids && n < 0) || !action_ids) return Fail(DTRL_ERR_ARG, "bad arguments");
	be_->Sync();
	const int cnt = env_ids ? n : n_;
	EnvState st;
	for (int i = 0; i < cnt; ++i) {
		const int e = EnvIndex(env_ids, i);
		if (e < 0 || e >= n_) return Fail(DTRL_ERR_ARG, "env id out of range");
		if (action_ids[i] < 0 || action_ids[i] >= cfg_.model.n_actions) return Fail(DTRL_ERR_ARG, "action id out of range");   // the reference asserts (and ignores the command in release builds)
		if (!be_->D2H(&st, &buf_.st[e], sizeof(EnvState))) return Fail(DTRL_ERR_DEVICE, be_->error());
		st.cmd_action = action_ids[i];
		if (!be_->H2D(&buf_.st[e], &st, sizeof(EnvState))) return Fail(DTRL_ERR_DEVICE, be_->error());
	}
	return DTRL_OK;
}

// cScenarioSimChar::AddPerturb -> cWorld::AddPerturb (scenarios/ScenarioSimChar.cpp:204-207): a world-frame force on a body part at a
// body-local offset for `duration` seconds of simulated time. Planar characters: the in-plane components. One slot per env.
int Engine::AddPerturb(const int32_t* env_ids, int n, const int32_t* link, const double* local_pos, const double* force, const double* duration)
{
	if (env_ids && n < 0) return Fail(DTRL_ERR_ARG, "negative env count");
	be_->Sync();
	if (int rc = KeysRefresh(variant_keys_); rc != DTRL_OK) return rc;
	const int cnt = env_ids ? n : n_;
	// The list becomes one row per env, the env's LAST row (applied in list order the last one won; a thread per row must not race), and goes into the slots in
	// one launch (Backend::PerturbScatter). A bad row stops the list where the sequential loop stopped: the rows in front of it are applied, then the error returns.
	std::vector<PerturbRow>& rows = pert_rows_.host;
	rows.clear();
	std::vector<int32_t> row_of(static_cast<size_t>(n_), -1);
	const char* bad = nullptr;
	for (int i = 0; i < cnt && !bad; ++i) {
		const int e = EnvIndex(env_ids, i);
		if (e < 0 || e >= n_) { bad = "env id out of range"; break; }
		const DevModel& m = ModelOf(e);   // (body_theta is the env's variant's)
		const int l = link[i];
		if (l < 0 || l >= m.L) { bad = "perturbation link out of range"; break; }
		if (!(duration[i] >= 0)) { bad = "perturbation duration must be non-negative"; break; }
		// the body frame is the joint frame turned by the body's attach angle: store the offset in the joint frame (the kernel has cos/sin of that)
		const double c = std::cos(m.body_theta[l]), sn = std::sin(m.body_theta[l]);
		const double lx = local_pos ? local_pos[2 * i] : 0.0, ly = local_pos ? local_pos[2 * i + 1] : 0.0;
		PerturbRow r;
		r.env = e; r.link = l;
		r.lp[0] = c * lx - sn * ly; r.lp[1] = sn * lx + c * ly;
		r.f[0] = force[2 * i]; r.f[1] = force[2 * i + 1];
		r.dur = duration[i];
		if (row_of[e] < 0) { row_of[e] = static_cast<int32_t>(rows.size()); rows.push_back(r); } else rows[row_of[e]] = r;
	}
	if (!rows.empty()) {
		if (int rc = RecsAlloc(pert_rows_, static_cast<size_t>(n_)); rc != DTRL_OK) return rc;
		if (!pert_rows_.Push(*be_) || !be_->PerturbScatter(buf_.st, pert_rows_.dev, static_cast<int>(rows.size())) || !be_->SyncSelected())
			return Fail(DTRL_ERR_DEVICE, be_->error());
	}
	if (bad) return Fail(DTRL_ERR_ARG, bad);
	return DTRL_OK;
}

// cScenarioSimChar::ApplyRandForce (scenarios/ScenarioSimChar.cpp:209-235): a random body part, a random 3-D direction scaled to a random
// magnitude in [min_perturb, max_perturb] (the planar character keeps x, y), a random duration. The reference draws from its racy,
// time-seeded global RNG; here the stream is a counter-based hash of (seed, global env id), so a run is reproducible.
int Engine::ApplyRandForce(const int32_t* env_ids, int n, uint64_t seed)
{
	if (env_ids && n < 0) return Fail(DTRL_ERR_ARG, "negative env count");
	const DevModel& m = cfg_.model;
	const int cnt = env_ids ? n : n_;
	std::vector<int32_t> link(cnt); std::vector<double> f(2 * static_cast<size_t>(cnt)), dur(cnt);
	for (int i = 0; i < cnt; ++i) {
		const int e = EnvIndex(env_ids, i);
		if (e < 0 || e >= n_) return Fail(DTRL_ERR_ARG, "env id out of range");
		uint64_t ctr = 0;
		const uint64_t key = rng_mix(seed ^ rng_mix(static_cast<uint64_t>(cfg_.run.env_id_base + e) + 0x5851F42D4C957F2DULL));
		auto uni = [&]() { const uint64_t z = rng_mix(key + (ctr++) * 0xD1342543DE82EF95ULL); return static_cast<double>(z >> 11) * (1.0 / 9007199254740992.0); };
		int part = static_cast<int>(uni() * m.L); if (part >= m.L) part = m.L - 1;        // every link of the shipped characters has a body
		double d[3];
		for (int k = 0; k < 3; ++k) { const double sgn = uni() < 0.5 ? -1.0 : 1.0; d[k] = sgn * uni(); }
		double nrm = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]); if (nrm == 0) { d[0] = 1; nrm = 1; }
		const double mag = cfg_.min_perturb + uni() * (cfg_.max_perturb - cfg_.min_perturb);
		link[i] = part; f[2 * i] = mag * d[0] / nrm; f[2 * i + 1] = mag * d[1] / nrm;
		dur[i] = cfg_.min_perturb_duration + uni() * (cfg_.max_perturb_duration - cfg_.min_perturb_duration);
	}
	return AddPerturb(env_ids, cnt, link.data(), nullptr, f.data(), dur.data());
}

// n values of the kernel's arithmetic type from device memory into the ABI's doubles
bool Engine::D2HReal(double* dst, const real* src, size_t n)
{
	if (sizeof(real) == sizeof(double)) return be_->D2H(dst, src, sizeof(real) * n);
	std::vector<real> tmp(n);
	if (!be_->D2H(tmp.data(), src, sizeof(real) * n)) return false;
	for (size_t k = 0; k < n; ++k) dst[k] = static_cast<double>(tmp[k]);
	return true;
}

int Engine::GetPoliState(const int32_t* env_ids, int n, double* s)
{
	if (n < 0 || !s) return Fail(DTRL_ERR_ARG, "bad arguments");
	be_->Sync();
	for (int i = 0; i < n; ++i) {
		int e = EnvIndex(env_ids, i);
		if (e < 0 || e >= n_) return Fail(DTRL_ERR_ARG, "env id out of range");
		if (!D2HReal(s + static_cast<size_t>(i) * S_, buf_.poli_state + static_cast<size_t>(e) * S_, S_)) return Fail(DTRL_ERR_DEVICE, be_->error());
	}
	return DTRL_OK;
}

int Engine::GetPolicyOutput(const int32_t* env_ids, int n, double* y)
{
	if (n < 0 || !y) return Fail(DTRL_ERR_ARG, "bad arguments");
	if (!cfg_.has_policy_net) return Fail(DTRL_ERR_ARG, "no -policy_net= in the arguments: this batch has no network");
	be_->Sync();
	const int pad = cfg_.net.out_size - cfg_.user_out_size;   // the device net of a single-head controller carries an unused critic slot in front
	for (int i = 0; i < n; ++i) {
		int e = EnvIndex(env_ids, i);
		if (e < 0 || e >= n_) return Fail(DTRL_ERR_ARG, "env id out of range");
		if (!D2HReal(y + static_cast<size_t>(i) * cfg_.user_out_size, buf_.nn_out + static_cast<size_t>(e) * cfg_.net.out_size + pad, cfg_.user_out_size)) return Fail(DTRL_ERR_DEVICE, be_->error());
	}
	return DTRL_OK;
}

int Engine::SampleGround(int env, int n, const double* x, double* h, int32_t* seg, int32_t* oi, int32_t* oj)
{
	if (env < 0 || env >= n_) return Fail(DTRL_ERR_ARG, "env id out of range");
	be_->Sync();
	// reads back the env's ground record as the kernel will see it and applies the same sampling routine the kernel uses
	if (!FetchGroundRec(env)) return Fail(DTRL_ERR_DEVICE, be_->error());
	for (int i = 0; i < n; ++i) {
		int a, b, s;
		h[i] = sample_ground(tmp_rec_, x[i], nullptr, &a, &b, &s);
		if (seg) seg[i] = s;
		if (oi) oi[i] = a;
		if (oj) oj[i] = b;
	}
	return DTRL_OK;
}

int Engine::GroundWindowRec(int env, int32_t* w2, double* min_x2, double* max_x2, float* h0, float* h1, int cap, int64_t* num_builds)
{
	if (env < 0 || env >= n_) return Fail(DTRL_ERR_ARG, "env id out of range");
	be_->Sync();
	if (!FetchGroundRec(env)) return Fail(DTRL_ERR_DEVICE, be_->error());
	float* dst[2] = {h0, h1};
	for (int s = 0; s < 2; ++s) {
		if (w2) w2[s] = tmp_rec_.w[s];
		if (min_x2) min_x2[s] = tmp_rec_.min_x[s];
		if (max_x2) max_x2[s] = tmp_rec_.max_x[s];
		if (dst[s]) std::memcpy(dst[s], tmp_rec_.data[s], sizeof(float) * std::max(0, std::min<int>(cap, tmp_rec_.w[s])));
	}
	if (num_builds) {
		*num_builds = -1;
		if (cfg_.device_terrain) { GroundGen g; if (!be_->D2H(&g, &buf_.gen[env], sizeof(g))) return Fail(DTRL_ERR_DEVICE, be_->error()); *num_builds = g.builds; if (g.overflow) return Fail(DTRL_ERR_CAPACITY, "terrain segment exceeds kSegCap vertices"); }
	}
	return DTRL_OK;
}

int Engine::EvalStats(double* avg_dist, int64_t* episodes, int64_t* cycles, int64_t* resets)
{
	std::vector<EnvState> st;
	int rc = GetStates(nullptr, n_, st);
	if (rc != DTRL_OK) return rc;
	double sum = 0; int64_t ep = 0, cy = 0, rs = 0;
	for (const EnvState& s : st) { sum += s.avg_dist * s.num_episodes; ep += s.num_episodes; cy += s.num_cycles; rs += s.num_resets; }
	if (avg_dist) *avg_dist = ep > 0 ? sum / ep : 0.0;
	if (episodes) *episodes = ep;
	if (cycles) *cycles = cy;
	if (resets) *resets = rs;
	return DTRL_OK;
}

int Engine::KernelTime(double* avg_ms, int64_t* launches) { be_->KernelTime(avg_ms, launches); return DTRL_OK; }

int Engine::ProfileSections(unsigned long long* out, int cap)
{
	be_->Sync();
	std::vector<unsigned long long> all(static_cast<size_t>(kProfMax) * n_);
	if (!be_->D2H(all.data(), buf_.prof, all.size() * sizeof(unsigned long long))) return Fail(DTRL_ERR_DEVICE, be_->error());
	for (int k = 0; k < kProfMax && k < cap; ++k) { unsigned long long s = 0; for (int e = 0; e < n_; ++e) s += all[static_cast<size_t>(e) * kProfMax + k]; out[k] = s; }
	return DTRL_OK;
}

// per-env values of one profile section (developer builds)
int Engine::ProfileEnv(int section, unsigned long long* out, int cap)
{
	if (section < 0 || section >= kProfMax || !out || cap < n_) return Fail(DTRL_ERR_ARG, "bad arguments");
	be_->Sync();
	std::vector<unsigned long long> all(static_cast<size_t>(kProfMax) * n_);
	if (!be_->D2H(all.data(), buf_.prof, all.size() * sizeof(unsigned long long))) return Fail(DTRL_ERR_DEVICE, be_->error());
	for (int e = 0; e < n_; ++e) out[e] = all[static_cast<size_t>(e) * kProfMax + section];
	return DTRL_OK;
}

// ---- env snapshots (include/dtrl.h: dtrl_snapshot_save / _restore / _export / _import, dtrl_clone_envs) ----
// A snapshot holds, per listed env, every record that decides the env's future: EnvState (FSM state and phase, action, PD targets, timers, the soft-fall
// filter, bookkeeping, the exploration counter, a pending command, the perturbation slot, the pending reset / init flags), its GroundRec, its GroundGen
// (-terrain_gen= device) or its host GroundWindow (host generator), the policy state, the begin state and action of the tuple in progress, the net's last
// output and the EnvStatus record the next frame boundary reads. Batch settings (policy, RunParams, terrain lerp) and outputs (tuple rings, totals, dist log) stay out.
namespace {
constexpr uint32_t pad8(uint32_t b) { return (b + 7u) & ~7u; }
size_t SnapBlobBytes(const SnapHeader& h) { return sizeof(SnapHeader) + pad8(4u * static_cast<uint32_t>(h.n_envs)) + static_cast<size_t>(h.n_envs) * (static_cast<size_t>(h.env_bytes) + h.host_bytes); }
}

int Engine::SnapReady(const char* what)
{
	if (int rc = RequireIdle(std::string(what) + kFrameInFlight); rc != DTRL_OK) return rc;
	if (!snap_ids_) {
		snap_ids_ = static_cast<int32_t*>(be_->HostStaging(sizeof(int32_t) * 2 * static_cast<size_t>(n_)));
		if (!snap_ids_) return Fail(DTRL_ERR_DEVICE, "host staging allocation failed: " + be_->error());
	}
	return DTRL_OK;
}

SnapPlan Engine::MakeSnapPlan() const
{
	SnapPlan p;
	auto add = [&](void* slab, size_t bytes, bool host) { SnapRec& r = p.rec[p.n_rec++]; r.slab = static_cast<char*>(slab); r.bytes = static_cast<uint32_t>(bytes); r.off = p.env_bytes; r.host = host ? 1 : 0; p.env_bytes += pad8(r.bytes); };
	add(buf_.st, sizeof(EnvState), false);
	if (zero_copy_) { p.gr_rec = p.n_rec; p.gr_stage = pin_recs_; p.stage_slot = stage_slot_; }   // a regenerated record may still wait for the env's next launch (FetchGroundRec)
	add(buf_.gr, sizeof(GroundRec), false);
	if (cfg_.device_terrain) add(buf_.gen, sizeof(GroundGen), false);
	add(buf_.status, sizeof(EnvStatus), zero_copy_);   // host terrain mode: the page-locked array the frame kernel writes and HostFrameWork reads
	add(buf_.poli_state, sizeof(real) * S_, false);
	add(buf_.tup_s0, sizeof(real) * S_, false);
	add(buf_.tup_a, sizeof(real) * A_, false);
	if (buf_.nn_out) add(buf_.nn_out, sizeof(real) * static_cast<size_t>(cfg_.net.out_size), false);
	if (cfg_.external_policy) add(ext_actions(buf_), sizeof(ExtAction), false);   // a delivered, not yet consumed action row (EnvState carries the park state itself)
	return p;
}

SnapHeader Engine::MakeSnapHeader(int n) const
{
	SnapHeader h{};
	h.magic = kSnapMagic; h.version = kSnapVersion; h.header_bytes = sizeof(SnapHeader);
	h.sizeof_real = sizeof(real); h.sizeof_env_state = sizeof(EnvState); h.sizeof_ground_rec = sizeof(GroundRec); h.sizeof_ground_gen = sizeof(GroundGen);
	h.sizeof_env_status = sizeof(EnvStatus); h.sizeof_ground_host = sizeof(GroundWindowState);
	const DevModel& m = cfg_.model;
	h.char_type = m.char_type; h.ctrl_type = m.ctrl_type; h.L = m.L; h.D = m.D; h.S = S_; h.A = A_; h.nn_out = cfg_.has_policy_net ? cfg_.net.out_size : 0;
	h.terrain_mode = cfg_.device_terrain ? 1 : 0;
	h.env_bytes = MakeSnapPlan().env_bytes; h.host_bytes = cfg_.device_terrain ? 0 : static_cast<uint32_t>(sizeof(GroundWindowState));
	h.n_envs = n;
	h.policy_mode = cfg_.external_policy ? 1 : 0;
	return h;
}

// the snapshot (or blob) was made by a batch of the same shape: same precision, record layouts, character, controller, sizes and terrain mode
int Engine::CheckSnapHeader(const SnapHeader& h, const char* what)
{
	const SnapHeader me = MakeSnapHeader(h.n_envs);
	auto bad = [&](const char* field, long long got, long long want, const char* hint) {
		return Fail(DTRL_ERR_ARG, std::string(what) + ": snapshot does not fit this batch: " + field + " is " + std::to_string(got) + ", the batch has " + std::to_string(want) + hint);
	};
	if (h.magic != kSnapMagic) return Fail(DTRL_ERR_ARG, std::string(what) + ": not a snapshot blob (magic)");
	if (h.version != kSnapVersion) return bad("format version", h.version, kSnapVersion, "");
	if (h.header_bytes != sizeof(SnapHeader)) return bad("header size", h.header_bytes, sizeof(SnapHeader), "");
	if (h.sizeof_real != me.sizeof_real) return bad("sizeof(real)", h.sizeof_real, me.sizeof_real, " (the other precision's library: -physics_precision=)");
	if (h.sizeof_env_state != me.sizeof_env_state) return bad("sizeof(EnvState)", h.sizeof_env_state, me.sizeof_env_state, "");
	if (h.sizeof_ground_rec != me.sizeof_ground_rec) return bad("sizeof(GroundRec)", h.sizeof_ground_rec, me.sizeof_ground_rec, "");
	if (h.sizeof_ground_gen != me.sizeof_ground_gen) return bad("sizeof(GroundGen)", h.sizeof_ground_gen, me.sizeof_ground_gen, "");
	if (h.sizeof_env_status != me.sizeof_env_status) return bad("sizeof(EnvStatus)", h.sizeof_env_status, me.sizeof_env_status, "");
	if (h.sizeof_ground_host != me.sizeof_ground_host) return bad("sizeof(GroundWindowState)", h.sizeof_ground_host, me.sizeof_ground_host, "");
	if (h.char_type != me.char_type) return bad("character type", h.char_type, me.char_type, " (another character)");
	if (h.ctrl_type != me.ctrl_type) return bad("controller type", h.ctrl_type, me.ctrl_type, "");
	if (h.L != me.L) return bad("L (links)", h.L, me.L, "");
	if (h.D != me.D) return bad("D (dofs)", h.D, me.D, "");
	if (h.S != me.S) return bad("S (policy state size)", h.S, me.S, "");
	if (h.A != me.A) return bad("A (policy action size)", h.A, me.A, "");
	if (h.nn_out != me.nn_out) return bad("net output size", h.nn_out, me.nn_out, "");
	if (h.policy_mode != me.policy_mode) return bad("policy_mode", h.policy_mode, me.policy_mode, " (0 = internal, 1 = -policy_mode= external)");
	if (h.terrain_mode != me.terrain_mode) return bad("terrain mode", h.terrain_mode, me.terrain_mode, " (0 = host generator, 1 = -terrain_gen= device)");
	if (h.env_bytes != me.env_bytes) return bad("device bytes per env", h.env_bytes, me.env_bytes, "");
	if (h.host_bytes != me.host_bytes) return bad("host bytes per env", h.host_bytes, me.host_bytes, "");
	return DTRL_OK;
}

int Engine::CheckSlots(const int32_t* ids, int n, const char* what)
{
	std::vector<char> seen(static_cast<size_t>(n_), 0);
	for (int i = 0; i < n; ++i) {
		const int e = ids[i];
		if (e < 0 || e >= n_) return Fail(DTRL_ERR_ARG, std::string(what) + ": env id out of range");
		if (seen[e]) return Fail(DTRL_ERR_ARG, std::string(what) + ": env " + std::to_string(e) + " is listed twice");
		seen[e] = 1;
	}
	return DTRL_OK;
}

Snapshot* Engine::NewSnapshot(int n)
{
	std::unique_ptr<Snapshot> s(new Snapshot());
	s->hdr = MakeSnapHeader(n);
	s->ids.resize(static_cast<size_t>(n));
	s->host.resize(static_cast<size_t>(n) * s->hdr.host_bytes);
	s->payload = static_cast<char*>(be_->Alloc(static_cast<size_t>(n) * s->hdr.env_bytes));
	if (!s->payload) return nullptr;
	s->owner = this;
	snapshots_.push_back(s.get());
	return s.release();
}

void Engine::SnapshotRelease(Snapshot* s)
{
	if (!s) return;
	auto it = std::find(snapshots_.begin(), snapshots_.end(), s);
	if (it != snapshots_.end()) snapshots_.erase(it);
	if (s->payload) { be_->Sync(); be_->Free(s->payload); }
	delete s;
}

int Engine::SnapshotSave(const int32_t* env_ids, int n, Snapshot** out)
{
	if (!out) return Fail(DTRL_ERR_ARG, "dtrl_snapshot_save: null output");
	*out = nullptr;
	if (env_ids && n <= 0) return Fail(DTRL_ERR_ARG, "dtrl_snapshot_save: empty env list");
	int rc = SnapReady("dtrl_snapshot_save");
	if (rc != DTRL_OK) return rc;
	const int cnt = env_ids ? n : n_;
	if (cnt > n_) return Fail(DTRL_ERR_ARG, "dtrl_snapshot_save: more envs listed than the batch has");
	for (int i = 0; i < cnt; ++i) snap_ids_[i] = EnvIndex(env_ids, i);
	rc = CheckSlots(snap_ids_, cnt, "dtrl_snapshot_save");
	if (rc != DTRL_OK) return rc;
	Snapshot* s = NewSnapshot(cnt);
	if (!s) return Fail(DTRL_ERR_DEVICE, "device allocation failed: " + be_->error());
	std::memcpy(s->ids.data(), snap_ids_, sizeof(int32_t) * cnt);
	bool ok = be_->SnapGather(MakeSnapPlan(), s->payload, snap_ids_, cnt);
	if (!ok) { Fail(DTRL_ERR_DEVICE, be_->error()); SnapshotRelease(s); return DTRL_ERR_DEVICE; }
	if (!cfg_.device_terrain) {
		GroundWindowState gs;
		for (int i = 0; i < cnt && ok; ++i) { ok = grounds_[snap_ids_[i]].SaveState(gs); std::memcpy(s->host.data() + static_cast<size_t>(i) * sizeof(gs), &gs, sizeof(gs)); }
		if (!ok) { SnapshotRelease(s); return Fail(DTRL_ERR_CAPACITY, "terrain segment exceeds kSegCap vertices"); }
	}
	*out = s;
	return DTRL_OK;
}

int Engine::SnapshotRestore(const Snapshot* s, const int32_t* env_ids, int n)
{
	if (!s) return Fail(DTRL_ERR_ARG, "dtrl_snapshot_restore: null snapshot");
	int rc = SnapReady("dtrl_snapshot_restore");
	if (rc != DTRL_OK) return rc;
	if (s->owner != this) return Fail(DTRL_ERR_ARG, "dtrl_snapshot_restore: the snapshot's payload lives with another batch; carry it over with dtrl_snapshot_export / dtrl_snapshot_import");
	rc = CheckSnapHeader(s->hdr, "dtrl_snapshot_restore");
	if (rc != DTRL_OK) return rc;
	if (env_ids && (n <= 0 || n > s->hdr.n_envs)) return Fail(DTRL_ERR_ARG, "dtrl_snapshot_restore: the slot list must name between 1 and the snapshot's env count slots");
	const int cnt = env_ids ? n : s->hdr.n_envs;
	if (cnt > n_) return Fail(DTRL_ERR_ARG, "dtrl_snapshot_restore: env id out of range (the snapshot holds more envs than the batch)");
	for (int i = 0; i < cnt; ++i) snap_ids_[i] = env_ids ? env_ids[i] : s->ids[i];
	rc = CheckSlots(snap_ids_, cnt, "dtrl_snapshot_restore");
	if (rc != DTRL_OK) return rc;
	if (!cfg_.device_terrain) {
		// the host generator's window first (it validates its record): segments built after the restore are the ones the saved env would have built
		GroundWindowState gs;
		std::vector<GroundWindow> tmp(static_cast<size_t>(cnt));
		for (int i = 0; i < cnt; ++i) {
			std::memcpy(&gs, s->host.data() + static_cast<size_t>(i) * sizeof(gs), sizeof(gs));
			tmp[i] = grounds_[snap_ids_[i]];   // (keeps the batch's terrain type and current parameters)
			if (!tmp[i].LoadState(gs)) return Fail(DTRL_ERR_ARG, "dtrl_snapshot_restore: malformed ground window record of saved env " + std::to_string(i));
		}
		for (int i = 0; i < cnt; ++i) grounds_[snap_ids_[i]] = tmp[i];
	}
	if (zero_copy_) for (int i = 0; i < cnt; ++i) stage_slot_[snap_ids_[i]] = 0;   // a record waiting for the env's next launch is superseded (UploadGround)
	if (!be_->SnapScatter(MakeSnapPlan(), s->payload, snap_ids_, cnt)) return Fail(DTRL_ERR_DEVICE, be_->error());
	return DTRL_OK;
}

int Engine::CloneEnvs(const int32_t* src_ids, const int32_t* dst_ids, int n)
{
	if (!src_ids || !dst_ids || n <= 0) return Fail(DTRL_ERR_ARG, "dtrl_clone_envs: source and destination lists are required");
	int rc = SnapReady("dtrl_clone_envs");
	if (rc != DTRL_OK) return rc;
	if (n > n_) return Fail(DTRL_ERR_ARG, "dtrl_clone_envs: more envs listed than the batch has");
	int32_t* src = snap_ids_; int32_t* dst = snap_ids_ + n_;
	std::vector<char> written(static_cast<size_t>(n_), 0);
	for (int i = 0; i < n; ++i) { src[i] = src_ids[i]; dst[i] = dst_ids[i]; if (src[i] < 0 || src[i] >= n_) return Fail(DTRL_ERR_ARG, "dtrl_clone_envs: env id out of range"); }
	rc = CheckSlots(dst, n, "dtrl_clone_envs (destination)");   // (a source may repeat: one env duplicated across the batch)
	if (rc != DTRL_OK) return rc;
	for (int i = 0; i < n; ++i) written[dst[i]] = 1;
	bool overlap = false;
	for (int i = 0; i < n; ++i) overlap = overlap || written[src[i]];
	const SnapPlan plan = MakeSnapPlan();
	std::vector<GroundWindow> tmp;
	if (!cfg_.device_terrain) { tmp.resize(static_cast<size_t>(n)); for (int i = 0; i < n; ++i) tmp[i] = grounds_[src[i]]; }
	bool ok = true;
	if (!overlap) {
		if (zero_copy_) for (int i = 0; i < n; ++i) stage_slot_[dst[i]] = 0;
		ok = be_->SnapCopy(plan, src, dst, n);
	} else {
		// an env is both read and written: read all, then write all, through a staging payload (two launches; wavefronts of one launch run in no order)
		if (!snap_scratch_) {
			snap_scratch_ = static_cast<char*>(be_->Alloc(static_cast<size_t>(n_) * plan.env_bytes));
			if (!snap_scratch_) return Fail(DTRL_ERR_DEVICE, "device allocation failed: " + be_->error());
			allocs_.push_back(snap_scratch_);
		}
		ok = be_->SnapGather(plan, snap_scratch_, src, n);
		if (ok && zero_copy_) for (int i = 0; i < n; ++i) stage_slot_[dst[i]] = 0;
		ok = ok && be_->SnapScatter(plan, snap_scratch_, dst, n);
	}
	if (!ok) return Fail(DTRL_ERR_DEVICE, be_->error());
	for (size_t i = 0; i < tmp.size(); ++i) {
		grounds_[dst[i]] = tmp[i];
		if (!terrain_table_.empty()) { const TerrainCfg& c = terrain_table_[terrain_keys_.env_key[dst[i]]]; grounds_[dst[i]].SetTerrain(c.type, c.params); }   // the window moves, the env's terrain stays
	}
	return DTRL_OK;
}

int Engine::SnapshotExport(const Snapshot* s, void* buf, size_t cap, size_t* bytes)
{
	if (!s) return Fail(DTRL_ERR_ARG, "dtrl_snapshot_export: null snapshot");
	const size_t total = SnapBlobBytes(s->hdr);
	if (bytes) *bytes = total;
	if (cap == 0) return DTRL_OK;
	if (!buf) return Fail(DTRL_ERR_ARG, "dtrl_snapshot_export: null buffer");
	if (cap < total) return Fail(DTRL_ERR_CAPACITY, "dtrl_snapshot_export: buffer smaller than the blob (" + std::to_string(total) + " bytes)");
	int rc = SnapReady("dtrl_snapshot_export");
	if (rc != DTRL_OK) return rc;
	char* p = static_cast<char*>(buf);
	const size_t nb = static_cast<size_t>(s->hdr.n_envs);
	std::memcpy(p, &s->hdr, sizeof(SnapHeader)); p += sizeof(SnapHeader);
	std::memset(p, 0, pad8(4u * s->hdr.n_envs)); std::memcpy(p, s->ids.data(), sizeof(int32_t) * nb); p += pad8(4u * s->hdr.n_envs);
	if (!be_->D2H(p, s->payload, nb * s->hdr.env_bytes)) return Fail(DTRL_ERR_DEVICE, be_->error());
	p += nb * s->hdr.env_bytes;
	if (!s->host.empty()) std::memcpy(p, s->host.data(), s->host.size());
	return DTRL_OK;
}

int Engine::SnapshotImport(const void* blob, size_t bytes, Snapshot** out)
{
	if (!out) return Fail(DTRL_ERR_ARG, "dtrl_snapshot_import: null output");
	*out = nullptr;
	if (!blob || bytes < sizeof(SnapHeader)) return Fail(DTRL_ERR_ARG, "dtrl_snapshot_import: blob truncated (shorter than its header)");
	SnapHeader h;
	std::memcpy(&h, blob, sizeof(h));
	int rc = CheckSnapHeader(h, "dtrl_snapshot_import");
	if (rc != DTRL_OK) return rc;
	if (h.n_envs <= 0 || h.n_envs > (1 << 24)) return Fail(DTRL_ERR_ARG, "dtrl_snapshot_import: env count out of range");
	if (bytes != SnapBlobBytes(h)) return Fail(DTRL_ERR_ARG, "dtrl_snapshot_import: blob truncated or padded: " + std::to_string(bytes) + " bytes, its header describes " + std::to_string(SnapBlobBytes(h)));
	rc = SnapReady("dtrl_snapshot_import");
	if (rc != DTRL_OK) return rc;
	const char* p = static_cast<const char*>(blob) + sizeof(SnapHeader);
	const char* p_ids = p; p += pad8(4u * h.n_envs);
	const char* p_dev = p; p += static_cast<size_t>(h.n_envs) * h.env_bytes;
	const char* p_host = p;
	// a blob may have been edited (Snapshot.env_state in the Python package): whatever the kernels use as an index is checked before it reaches the device
	const SnapPlan plan = MakeSnapPlan();
	const DevModel& m = cfg_.model;
	for (int i = 0; i < h.n_envs; ++i) {
		EnvState st; GroundRec gr;
		std::memcpy(&st, p_dev + static_cast<size_t>(i) * h.env_bytes + plan.rec[0].off, sizeof(st));
		std::memcpy(&gr, p_dev + static_cast<size_t>(i) * h.env_bytes + plan.rec[1].off, sizeof(gr));
		const char* bad = nullptr;
		if (st.ws_R < 0 || st.ws_R > kMaxRows) bad = "ws_R";
		else if (st.action_id < 0 || st.action_id >= std::max(1, m.n_actions)) bad = "action_id";
		else if (st.cmd_action < -1 || st.cmd_action >= std::max(1, m.n_actions)) bad = "cmd_action";
		else if (st.pert_link < -1 || st.pert_link >= m.L) bad = "pert_link";
		else if (st.state < 0 || st.state >= 4) bad = "state";
		else if (st.stance < 0 || st.stance > 1) bad = "stance";
		else if (st.ext_park < 0 || st.ext_park > (cfg_.external_policy ? kExtReady : 0)) bad = "ext_park";
		else if (st.ext_steps_left < (st.ext_park != 0 ? 1 : 0) || st.ext_steps_left > (cfg_.external_policy ? m.num_update_steps : 0)) bad = "ext_steps_left";   // (an env parks INSIDE an env-step: at least that one is left)
		else if (gr.w[0] < 0 || gr.w[0] > kSegCap || gr.w[1] < 0 || gr.w[1] > kSegCap) bad = "ground segment width";
		if (bad) return Fail(DTRL_ERR_ARG, std::string("dtrl_snapshot_import: ") + bad + " of saved env " + std::to_string(i) + " is out of range");
	}
	if (h.host_bytes) {
		GroundWindowState gs; GroundWindow probe;
		for (int i = 0; i < h.n_envs; ++i) {
			std::memcpy(&gs, p_host + static_cast<size_t>(i) * sizeof(gs), sizeof(gs));
			if (!probe.LoadState(gs)) return Fail(DTRL_ERR_ARG, "dtrl_snapshot_import: malformed ground window record of saved env " + std::to_string(i));
		}
	}
	Snapshot* s = NewSnapshot(h.n_envs);
	if (!s) return Fail(DTRL_ERR_DEVICE, "device allocation failed: " + be_->error());
	std::memcpy(s->ids.data(), p_ids, sizeof(int32_t) * static_cast<size_t>(h.n_envs));
	if (!s->host.empty()) std::memcpy(s->host.data(), p_host, s->host.size());
	if (!be_->H2D(s->payload, p_dev, static_cast<size_t>(h.n_envs) * h.env_bytes)) { Fail(DTRL_ERR_DEVICE, be_->error()); SnapshotRelease(s); return DTRL_ERR_DEVICE; }
	*out = s;
	return DTRL_OK;
}

// ---- external policy mode (include/dtrl.h: dtrl_pending_actions ... dtrl_ext_stats) ----
int Engine::ExtRefuse(const char* what)
{
	if (!cfg_.external_policy) return Fail(DTRL_ERR_ARG, std::string(what) + ": the batch runs in internal policy mode (create it with -policy_mode= external)");
	return RequireIdle(std::string(what) + " between dtrl_step_begin and dtrl_step_end: a tick is in flight; call dtrl_step_end first");
}

int Engine::PendingActions(int32_t* env_ids, void* states, int cap, int* out_n, bool device)
{
	const char* what = device ? "dtrl_pending_actions_device" : "dtrl_pending_actions";
	if (out_n) *out_n = 0;
	int rc = ExtRefuse(what);
	if (rc != DTRL_OK) return rc;
	if (cap < 0 || !out_n || (cap > 0 && !env_ids)) return Fail(DTRL_ERR_ARG, std::string(what) + ": env_ids and out_n are required, cap must not be negative");
	cap = std::min(cap, n_);
	if (device) {
		if (!be_->ExtCollect(buf_, n_, cap, cap > 0 ? env_ids : d_ext_ids_, cap > 0 ? states : nullptr, true, ext_meta_)) return Fail(DTRL_ERR_DEVICE, be_->error());
		*out_n = ext_meta_[0];
		return DTRL_OK;
	}
	if (!be_->ExtCollect(buf_, n_, cap, d_ext_ids_, (states && cap > 0) ? d_ext_states_ : nullptr, false, ext_meta_)) return Fail(DTRL_ERR_DEVICE, be_->error());
	const int m = ext_meta_[0];
	if (m > 0 && !be_->D2H(env_ids, d_ext_ids_, sizeof(int32_t) * m)) return Fail(DTRL_ERR_DEVICE, be_->error());
	if (m > 0 && states && !be_->D2H(states, d_ext_states_, sizeof(double) * static_cast<size_t>(m) * S_)) return Fail(DTRL_ERR_DEVICE, be_->error());
	*out_n = m;
	return DTRL_OK;
}

int Engine::SupplyActions(const int32_t* env_ids, int n, const int32_t* action_ids, const void* params, const uint32_t* flags, bool device, int* rejected)
{
	const char* what = device ? "dtrl_supply_actions_device" : "dtrl_supply_actions";
	if (rejected) *rejected = 0;
	int rc = ExtRefuse(what);
	if (rc != DTRL_OK) return rc;
	if (n < 0 || n > n_) return Fail(DTRL_ERR_ARG, std::string(what) + ": row count out of range (0 .. num_envs)");
	if (n == 0) return DTRL_OK;
	if (!env_ids || !params) return Fail(DTRL_ERR_ARG, std::string(what) + ": env_ids and params are required");
	const int n_opt = cfg_.model.n_opt, n_labels = std::max(1, cfg_.model.n_actions);
	int32_t rej = 0;
	if (device) {
		// rows straight from the caller's device arrays; a row that does not apply (id or label out of range, env not awaiting, env named twice) is skipped and counted
		if (!be_->ExtSupply(buf_, n_, n_opt, n_labels, env_ids, n, action_ids, params, true, flags, true, &rej)) return Fail(DTRL_ERR_DEVICE, be_->error());
		if (rejected) *rejected = rej;
		return DTRL_OK;
	}
	// host rows: all or nothing. Ids in range and distinct (host), every env awaiting (a counting pass of the scatter), labels in range -- then the scatter
	std::vector<char> seen(static_cast<size_t>(n_), 0);
	for (int i = 0; i < n; ++i) {
		const int e = env_ids[i];
		if (e < 0 || e >= n_) return Fail(DTRL_ERR_ARG, std::string(what) + ": env id " + std::to_string(e) + " out of range; nothing applied");
		if (seen[e]) return Fail(DTRL_ERR_ARG, std::string(what) + ": env " + std::to_string(e) + " is listed twice; nothing applied");
		seen[e] = 1;
		if (action_ids && (action_ids[i] < 0 || action_ids[i] >= n_labels)) return Fail(DTRL_ERR_ARG, std::string(what) + ": action_id of row " + std::to_string(i) + " out of range (0 .. " + std::to_string(n_labels - 1) + ", the range a snapshot accepts); nothing applied");
	}
	if (!be_->H2D(d_ext_ids_, env_ids, sizeof(int32_t) * n) || !be_->H2D(d_ext_params_, params, sizeof(double) * static_cast<size_t>(n) * n_opt)) return Fail(DTRL_ERR_DEVICE, be_->error());
	if (action_ids && !be_->H2D(d_ext_action_ids_, action_ids, sizeof(int32_t) * n)) return Fail(DTRL_ERR_DEVICE, be_->error());
	if (flags && !be_->H2D(d_ext_flags_, flags, sizeof(uint32_t) * n)) return Fail(DTRL_ERR_DEVICE, be_->error());
	if (!be_->ExtSupply(buf_, n_, n_opt, n_labels, d_ext_ids_, n, action_ids ? d_ext_action_ids_ : nullptr, d_ext_params_, false, flags ? d_ext_flags_ : nullptr, false, &rej)) return Fail(DTRL_ERR_DEVICE, be_->error());
	if (rej > 0) {
		std::vector<EnvState> st;
		std::string which;
		if (GetStates(env_ids, n, st) == DTRL_OK) for (int i = 0; i < n && which.empty(); ++i) if (st[i].ext_park != kExtAwaiting) which = " (first: env " + std::to_string(env_ids[i]) + (st[i].ext_park == kExtReady ? ", which already has its action)" : ", which is running)");
		return Fail(DTRL_ERR_ARG, std::string(what) + ": " + std::to_string(rej) + " of " + std::to_string(n) + " rows name an env that is not awaiting an action" + which + "; nothing applied");
	}
	if (!be_->ExtSupply(buf_, n_, n_opt, n_labels, d_ext_ids_, n, action_ids ? d_ext_action_ids_ : nullptr, d_ext_params_, false, flags ? d_ext_flags_ : nullptr, true, &rej)) return Fail(DTRL_ERR_DEVICE, be_->error());
	if (rejected) *rejected = rej;
	return DTRL_OK;
}

int Engine::ExtStats(int64_t* awaiting, int64_t* ready, int64_t* env_steps_total, int64_t* env_frames_total)
{
	int rc = ExtRefuse("dtrl_ext_stats");
	if (rc != DTRL_OK) return rc;
	if (!be_->ExtCollect(buf_, n_, 0, d_ext_ids_, nullptr, false, ext_meta_)) return Fail(DTRL_ERR_DEVICE, be_->error());
	if (awaiting) *awaiting = ext_meta_[1];
	if (ready) *ready = ext_meta_[2];
	if (env_steps_total || env_frames_total) {
		std::vector<ExtCount> c(static_cast<size_t>(n_));
		if (!be_->D2H(c.data(), ext_counts(buf_), sizeof(ExtCount) * c.size())) return Fail(DTRL_ERR_DEVICE, be_->error());
		int64_t s = 0, f = 0;
		for (const ExtCount& x : c) { s += x.env_steps; f += x.env_frames; }
		if (env_steps_total) *env_steps_total = s;
		if (env_frames_total) *env_frames_total = f;
	}
	return DTRL_OK;
}

int Engine::ExtEnvInfo(const int32_t* env_ids, int n, int32_t* park, int32_t* steps_left)
{
	int rc = ExtRefuse("dtrl_ext_env_info");
	if (rc != DTRL_OK) return rc;
	const int cnt = env_ids ? n : n_;
	std::vector<EnvState> st;
	rc = GetStates(env_ids, cnt, st);
	if (rc != DTRL_OK) return rc;
	for (int i = 0; i < cnt; ++i) { if (park) park[i] = st[i].ext_park; if (steps_left) steps_left[i] = st[i].ext_steps_left; }
	return DTRL_OK;
}

// ---- per-env keys: what policy slots and model variants share (dtrl_engine.h EnvAssignment) ----
void* Engine::KeysAllocate(EnvAssignment& a, size_t table_bytes)
{
	void* table = be_->Alloc(table_bytes); if (table) allocs_.push_back(table);
	a.d_env_key = static_cast<int32_t*>(be_->Alloc(sizeof(int32_t) * n_)); if (a.d_env_key) allocs_.push_back(a.d_env_key);   // (zero-filled: every env starts under key 0)
	a.part = static_cast<int32_t*>(be_->HostStaging(sizeof(int32_t) * 2 * static_cast<size_t>(n_)));
	if (!table || !a.d_env_key || !a.part || !be_->Sync()) { Fail(DTRL_ERR_DEVICE, "device allocation failed: " + be_->error()); return nullptr; }
	a.env_key.assign(static_cast<size_t>(n_), 0);
	return table;
}

// The order of the checks is part of the behaviour: no keys, key out of range, frame in flight. dtrl_slot_stats is the one call that waits for a frame in
// flight instead of refusing it (wait_in_flight): train_loop's overlapped loop logs its greedy envs through it while the next frame runs, as it does with
// dtrl_eval_stats. dtrl_variant_stats refuses like every other variant call; nothing is known to need either behaviour of the other family, so both stay.
int Engine::KeysIdle(const EnvAssignment& a, const char* what, int key, bool wait_in_flight)
{
	if (a.filled.empty()) return Fail(DTRL_ERR_ARG, std::string(what) + ": " + a.none_text);
	if (key < 0 || key >= a.n_keys()) return Fail(DTRL_ERR_ARG, std::string(what) + ": " + a.noun + " " + std::to_string(key) + " out of range (0 .. " + std::to_string(a.n_keys() - 1) + ")");
	if (!wait_in_flight) return RequireIdle(std::string(what) + kFrameInFlight);
	be_->SelectStream(0);
	return be_->Sync() ? DTRL_OK : Fail(DTRL_ERR_DEVICE, be_->error());
}

int Engine::DevOk(bool ok) { return ok ? DTRL_OK : Fail(DTRL_ERR_DEVICE, be_->error()); }
template <class Rec> int Engine::RecsAlloc(RuleRecs<Rec>& r, size_t n) { return r.Alloc(*be_, n, allocs_) ? DTRL_OK : Fail(DTRL_ERR_DEVICE, "device allocation failed: " + be_->error()); }
template <class Rec> int Engine::RecsAlloc(RuleRecs<Rec>& r, size_t n, const Rec& fill)
{
	if (r.dev) return DTRL_OK;
	if (int rc = RecsAlloc(r, n); rc != DTRL_OK) return rc;
	r.host.assign(n, fill);
	return DevOk(r.Push(*be_));
}
int Engine::RuleCallBegin(const char* what, EnvAssignment* keys, const char* no_rule, const EnvListArg& list, RecsBase* recs)
{
	const std::string w = std::string(what) + ": ";
	if (int rc = keys ? KeysIdle(*keys, what, 0) : RequireIdle(what + std::string(kFrameInFlight)); rc != DTRL_OK) return rc;
	if (no_rule) return Fail(DTRL_ERR_ARG, w + no_rule);
	if (keys) if (int rc = KeysRefresh(*keys); rc != DTRL_OK) return rc;
	if (int rc = CheckEnvList(w, list.ids, list.n, list.tail, list.name, list.required); rc != DTRL_OK) return rc;
	return recs ? DevOk(recs->Pull(*be_)) : DTRL_OK;
}
int Engine::KeysRefresh(EnvAssignment& a)
{
	if (!a.on_device || !a.stale) return DTRL_OK;
	if (!be_->D2H(a.env_key.data(), a.d_env_key, sizeof(int32_t) * a.env_key.size()) || !a.recs->Pull(*be_)) return Fail(DTRL_ERR_DEVICE, be_->error());
	a.stale = false;
	return DTRL_OK;
}
int Engine::KeysCurrent(EnvAssignment& a, const char* what, bool always)
{
	if (!a.on_device && !always) return DTRL_OK;
	if (int rc = KeysIdle(a, what, 0); rc != DTRL_OK) return rc;
	return KeysRefresh(a);
}

int Engine::CheckEnvList(const std::string& w, const int32_t* env_ids, int n, const char* tail, const char* name, const void* required)
{
	if (n < 0 || n > n_ || (name && n > 0 && !required)) return Fail(DTRL_ERR_ARG, w + (name ? std::string(name) + " is required and the env count" : std::string("the env count")) + " must be 0 .. num_envs");
	for (int i = 0; i < n; ++i) { const int e = EnvIndex(env_ids, i); if (e < 0 || e >= n_) return Fail(DTRL_ERR_ARG, w + "env id " + std::to_string(e) + " out of range" + tail); }
	return DTRL_OK;
}

int Engine::KeysAssign(EnvAssignment& a, const char* what, const int32_t* env_ids, int n, const int32_t* keys)
{
	int rc = KeysIdle(a, what, 0);
	if (rc != DTRL_OK) return rc;
	const std::string w = std::string(what) + ": ";
	if (n < 0 || n > n_ || (n > 0 && !keys)) return Fail(DTRL_ERR_ARG, w + a.noun + "s is required and the env count must be 0 .. num_envs");
	for (int i = 0; i < n; ++i) {   // all or nothing
		const int e = EnvIndex(env_ids, i), k = keys[i];
		if (e < 0 || e >= n_) return Fail(DTRL_ERR_ARG, w + "env id " + std::to_string(e) + " out of range; nothing assigned");
		if (k < 0 || k >= a.n_keys()) return Fail(DTRL_ERR_ARG, w + a.noun + " " + std::to_string(k) + " out of range (0 .. " + std::to_string(a.n_keys() - 1) + "); nothing assigned");
		if (!a.filled[k]) return Fail(DTRL_ERR_ARG, w + a.noun + " " + std::to_string(k) + " " + a.empty_text + "; nothing assigned");
	}
	for (int i = 0; i < n; ++i) a.env_key[EnvIndex(env_ids, i)] = keys[i];
	if (!be_->H2D(a.d_env_key, a.env_key.data(), sizeof(int32_t) * a.env_key.size())) return Fail(DTRL_ERR_DEVICE, be_->error());
	return DTRL_OK;
}

int Engine::KeysGet(const EnvAssignment& a, const char* what, const int32_t* env_ids, int n, int32_t* keys_out)
{
	const std::string w = std::string(what) + ": ";
	if (a.filled.empty()) return Fail(DTRL_ERR_ARG, w + a.none_text);
	if (int rc = CheckEnvList(w, env_ids, n, "", (std::string(a.noun) + "s_out").c_str(), keys_out); rc != DTRL_OK) return rc;
	for (int i = 0; i < n; ++i) keys_out[i] = a.env_key[EnvIndex(env_ids, i)];
	return DTRL_OK;
}

// Backend::SlotReduce over the family's per-env array; its kernels are sized by kMaxSlots, so the window of kMaxSlots keys that holds `key` (policy slots: the one window)
int Engine::KeysStats(const EnvAssignment& a, const char* what, bool wait_in_flight, int key, int64_t* n_envs, double* avg_dist, int64_t* episodes, int64_t* cycles, int64_t* resets)
{
	if (int rc = KeysIdle(a, what, key, wait_in_flight); rc != DTRL_OK) return rc;
	const int base = key / kMaxSlots * kMaxSlots, cnt = std::min(kMaxSlots, a.n_keys() - base);
	SlotSums sums[kMaxSlots];
	if (!be_->SlotReduce(buf_.st, a.d_env_key, n_, cnt, sums, base)) return Fail(DTRL_ERR_DEVICE, be_->error());
	const SlotSums& t = sums[key - base];
	if (n_envs) *n_envs = t.n_envs;
	if (avg_dist) *avg_dist = t.episodes > 0 ? t.dist_sum / static_cast<double>(t.episodes) : 0.0;
	if (episodes) *episodes = t.episodes;
	if (cycles) *cycles = t.cycles;
	if (resets) *resets = t.resets;
	return DTRL_OK;
}

// ---- policy slots (include/dtrl.h: dtrl_slots_create ... dtrl_slot_stats) ----
// Two things keep a launch in flight from ever reading a half-written record. (1) The table and the per-env array change only in calls that refuse a frame in
// flight and then wait for every stream (KeysIdle) -- with dtrl_step_poll or -terrain_gen= device the host has not otherwise waited for the launches it queued.
// (2) What DOES change while launches run -- slot 0's weight buffer (the double-buffered hand-over) and dtrl_set_explore -- is not in the table at all: slot 0
// and its aliases carry kSlotLaunchPolicy / kSlotLaunchExplore and take those values from the launch's own by-value arguments, exactly where the single-policy
// kernels take them. So MarkWeightReader / WaitWeightReaders / WaitPolicyReady and the flip order a hand-over for slot 0 and for every alias of it at once.
int Engine::UploadSlotTable()
{
	for (size_t s = 0; s < slots_.size(); ++s) {
		const SlotHost& h = slots_[s]; const SlotHost& root = slots_[SlotRoot(static_cast<int>(s))];
		SlotRec r{};
		if (&root == &slots_[0]) r.flags |= kSlotLaunchPolicy;
		else { r.weights = root.weights; r.in_off = root.norm[0]; r.in_scale = root.norm[1]; r.out_off = root.norm[2]; r.out_scale = root.norm[3]; }
		if (s == 0) r.flags |= kSlotLaunchExplore;
		else { r.enable_exp = h.enable_exp; r.exp_rate = static_cast<real>(h.rate); r.exp_temp = static_cast<real>(h.temp); r.exp_base_rate = static_cast<real>(h.base_rate); }
		slot_table_[s] = r;
	}
	if (!be_->H2D(d_slot_table_, slot_table_.data(), sizeof(SlotRec) * slot_table_.size())) return Fail(DTRL_ERR_DEVICE, be_->error());
	return DTRL_OK;
}

int Engine::SlotsCreate(int n_slots)
{
	if (cfg_.external_policy) return Fail(DTRL_ERR_ARG, "dtrl_slots_create: not available with -policy_mode= external (the caller's policy decides; no policy net runs inside the frame kernel)");
	if (!cfg_.has_policy_net) return Fail(DTRL_ERR_ARG, "dtrl_slots_create: no -policy_net= in the arguments: this batch has no network");
	if (!var_models_.empty()) return Fail(DTRL_ERR_ARG, "dtrl_slots_create: not available on a batch with model variants (dtrl_variants_create): policy slots together with model variants are not supported");
	if (n_slots < 1 || n_slots > kMaxSlots) return Fail(DTRL_ERR_ARG, "dtrl_slots_create: n_slots must be 1 .. " + std::to_string(kMaxSlots) + ", not " + std::to_string(n_slots));
	if (!slots_.empty()) {
		if (n_slots == static_cast<int>(slots_.size())) return DTRL_OK;
		return Fail(DTRL_ERR_ARG, "dtrl_slots_create: the batch already has " + std::to_string(slots_.size()) + " slots; a second call with another count (" + std::to_string(n_slots) + ") is refused");
	}
	if (int rc = RequireIdle(std::string("dtrl_slots_create") + kFrameInFlight); rc != DTRL_OK) return rc;
	d_slot_table_ = static_cast<SlotRec*>(KeysAllocate(slot_keys_, sizeof(SlotRec) * n_slots));
	if (!d_slot_table_) return DTRL_ERR_DEVICE;
	slots_.assign(static_cast<size_t>(n_slots), SlotHost());
	for (SlotHost& h : slots_) { h.enable_exp = cfg_.run.enable_exp; h.rate = cfg_.run.exp_rate; h.temp = cfg_.run.exp_temp; h.base_rate = cfg_.run.exp_base_rate; }   // every slot starts with the batch's exploration settings
	slot_table_.assign(static_cast<size_t>(n_slots), SlotRec{});
	int rc = UploadSlotTable();
	if (rc != DTRL_OK) { slots_.clear(); return rc; }
	slot_keys_.filled.assign(static_cast<size_t>(n_slots), 0); slot_keys_.filled[0] = 1;
	return DTRL_OK;
}

int Engine::SlotSetPolicy(int slot, const float* w, size_t n, const double* io, const double* is, const double* oo, const double* os, bool device)
{
	const char* what = device ? "dtrl_slot_set_policy_device" : "dtrl_slot_set_policy";
	int rc = KeysIdle(slot_keys_, what, slot);
	if (rc != DTRL_OK) return rc;
	if (slot == 0) return device ? SetPolicyDevice(w, n, io, is, oo, os) : SetPolicy(w, n, io, is, oo, os);
	const NetDesc& d = cfg_.net;
	if (!w || n != static_cast<size_t>(cfg_.user_num_params)) return Fail(DTRL_ERR_ARG, std::string(what) + ": weight count does not match the deploy prototxt");
	if (device && sizeof(real) != sizeof(double) && (io || is || oo || os)) return Fail(DTRL_ERR_ARG, "the fp32 build takes device-resident WEIGHTS only; hand the normalisers over through dtrl_slot_set_policy (host doubles)");
	SlotHost& h = slots_[slot];
	const bool fresh = !h.weights;
	if (fresh) {
		float* wd = static_cast<float*>(be_->Alloc(sizeof(float) * relayout_.size())); if (wd) allocs_.push_back(wd);
		real* nm[4];
		for (int k = 0; k < 4; ++k) { nm[k] = static_cast<real*>(be_->Alloc(sizeof(real) * (k < 2 ? d.in_size : d.out_size))); if (nm[k]) allocs_.push_back(nm[k]); }
		if (!wd || !nm[0] || !nm[1] || !nm[2] || !nm[3] || !be_->Sync()) return Fail(DTRL_ERR_DEVICE, "device allocation failed: " + be_->error());
		h.weights = wd; for (int k = 0; k < 4; ++k) h.norm[k] = nm[k];
	}
	const int pad = d.out_size - cfg_.user_out_size;   // CACLA actor: the neutral critic slot in front of the output normalisers (Engine::SetPolicy)
	bool ok = true;
	if (!device || fresh) {   // identity for every vector passed as NULL (a device hand-over into a slot that has a policy keeps the vectors it has)
		std::vector<real> v[4];
		v[0].assign(d.in_size, 0.0); v[1].assign(d.in_size, 1.0); v[2].assign(d.out_size, 0.0); v[3].assign(d.out_size, 1.0);
		if (!device) {
			if (io) for (int k = 0; k < d.in_size; ++k) v[0][k] = static_cast<real>(io[k]);
			if (is) for (int k = 0; k < d.in_size; ++k) v[1][k] = static_cast<real>(is[k]);
			if (oo) for (int k = 0; k < cfg_.user_out_size; ++k) v[2][pad + k] = static_cast<real>(oo[k]);
			if (os) for (int k = 0; k < cfg_.user_out_size; ++k) v[3][pad + k] = static_cast<real>(os[k]);
		}
		for (int k = 0; k < 4; ++k) ok = ok && be_->H2D(h.norm[k], v[k].data(), sizeof(real) * v[k].size());
	}
	if (device) {
		ok = ok && be_->GatherF32(h.weights, w, d_relayout_, relayout_.size());
		if (io) ok = ok && be_->D2D(h.norm[0], io, sizeof(real) * d.in_size);
		if (is) ok = ok && be_->D2D(h.norm[1], is, sizeof(real) * d.in_size);
		if (oo) ok = ok && be_->D2D(h.norm[2] + pad, oo, sizeof(real) * cfg_.user_out_size);
		if (os) ok = ok && be_->D2D(h.norm[3] + pad, os, sizeof(real) * cfg_.user_out_size);
	} else {
		std::vector<float> dev_w(relayout_.size());
		for (size_t i = 0; i < relayout_.size(); ++i) dev_w[i] = relayout_[i] >= 0 ? w[relayout_[i]] : 0.0f;
		ok = ok && be_->H2D(h.weights, dev_w.data(), sizeof(float) * dev_w.size());
	}
	if (!ok) return Fail(DTRL_ERR_DEVICE, be_->error());
	h.alias = -1; slot_keys_.filled[slot] = 1;
	return UploadSlotTable();
}

int Engine::SlotAlias(int slot, int src_slot)
{
	int rc = KeysIdle(slot_keys_, "dtrl_slot_alias", slot);
	if (rc != DTRL_OK) return rc;
	if (slot == 0) return Fail(DTRL_ERR_ARG, "dtrl_slot_alias: slot 0 is the batch's own policy and cannot be an alias");
	if (src_slot < 0 || src_slot >= static_cast<int>(slots_.size())) return Fail(DTRL_ERR_ARG, "dtrl_slot_alias: source slot " + std::to_string(src_slot) + " out of range (0 .. " + std::to_string(slots_.size() - 1) + ")");
	if (src_slot == slot) return Fail(DTRL_ERR_ARG, "dtrl_slot_alias: slot " + std::to_string(slot) + " cannot be an alias of itself");
	if (!slot_keys_.filled[src_slot]) return Fail(DTRL_ERR_ARG, "dtrl_slot_alias: source slot " + std::to_string(src_slot) + " " + slot_keys_.empty_text);
	for (int s = src_slot; s >= 0; s = slots_[s].alias) if (s == slot) return Fail(DTRL_ERR_ARG, "dtrl_slot_alias: slot " + std::to_string(src_slot) + " reads slot " + std::to_string(slot) + " itself: the alias would be an alias of itself");
	slots_[slot].alias = src_slot; slot_keys_.filled[slot] = 1;
	return UploadSlotTable();
}

int Engine::SlotSetExplore(int slot, int enable, double rate, double temp, double base_rate)
{
	if (slot == 0 && !slots_.empty()) return SetExplore(enable, rate, temp, base_rate);   // (valid at any time, as dtrl_set_explore is: it travels by value with every launch)
	int rc = KeysIdle(slot_keys_, "dtrl_slot_set_explore", slot);
	if (rc != DTRL_OK) return rc;
	SlotHost& h = slots_[slot];
	h.enable_exp = enable ? 1 : 0; h.rate = rate; h.temp = temp; h.base_rate = base_rate;
	return UploadSlotTable();
}

// ---- model variants (include/dtrl.h: dtrl_variants_create ... dtrl_variant_stats) ----
// The timing rules are those of the slot calls (KeysIdle). Nothing of a variant changes while launches run: unlike slot 0's weights, the batch's own model is
// fixed at creation, so the table holds a plain copy of it as record 0 and no launch argument has to stand in for a table entry.
int Engine::VariantsCreate(int n_variants)
{
	if (cfg_.external_policy) return Fail(DTRL_ERR_ARG, "dtrl_variants_create: not available with -policy_mode= external (model variants together with external policy mode are not supported)");
	if (!slots_.empty()) return Fail(DTRL_ERR_ARG, "dtrl_variants_create: not available on a batch with policy slots (dtrl_slots_create): model variants together with policy slots are not supported");
	if (!var_models_.empty()) return Fail(DTRL_ERR_ARG, "dtrl_variants_create: the batch already has " + std::to_string(var_models_.size()) + " variants; it is called once per batch");
	if (n_variants < 1 || n_variants > n_) return Fail(DTRL_ERR_ARG, "dtrl_variants_create: n_variants must be 1 .. num_envs (" + std::to_string(n_) + "), not " + std::to_string(n_variants));
	if (int rc = RequireIdle(std::string("dtrl_variants_create") + kFrameInFlight); rc != DTRL_OK) return rc;
	d_var_models_ = static_cast<DevModel*>(KeysAllocate(variant_keys_, sizeof(DevModel) * static_cast<size_t>(n_variants)));
	if (!d_var_models_) return DTRL_ERR_DEVICE;
	if (!be_->H2D(d_var_models_, &cfg_.model, sizeof(DevModel))) return Fail(DTRL_ERR_DEVICE, be_->error());
	var_models_.assign(static_cast<size_t>(n_variants), cfg_.model);   // (an empty variant holds the batch's model until it is loaded; it cannot be assigned)
	var_scalars_.assign(static_cast<size_t>(n_variants), cfg_.scalars);
	variant_keys_.filled.assign(static_cast<size_t>(n_variants), 0); variant_keys_.filled[0] = 1;
	return DTRL_OK;
}

// what of a variant must equal the batch's model: the skeleton the fast kernels are compiled for, the scene, and the whole controller part -- the batch has one
// policy, one action table and one set of output normalisers, and they must mean the same thing for every env. Returns the first field that differs, or nullptr.
static const char* VariantMisfit(const DevModel& a, const DevModel& b)
{
#define DTRL_SAME(f) if (std::memcmp(&a.f, &b.f, sizeof(a.f)) != 0) return #f
	DTRL_SAME(L); DTRL_SAME(D); DTRL_SAME(parent);
	DTRL_SAME(char_type); DTRL_SAME(ctrl_type); DTRL_SAME(scenario); DTRL_SAME(num_update_steps); DTRL_SAME(num_sim_substeps); DTRL_SAME(world_scale); DTRL_SAME(valid_init_pos_x);
	DTRL_SAME(P); DTRL_SAME(n_opt); DTRL_SAME(opt_index); DTRL_SAME(n_sets); DTRL_SAME(ctrl_params); DTRL_SAME(n_actions);
	DTRL_SAME(act_idx0); DTRL_SAME(act_idx1); DTRL_SAME(act_blend); DTRL_SAME(act_cyclic); DTRL_SAME(default_action); DTRL_SAME(enable_grav_comp); DTRL_SAME(enable_vf);
#undef DTRL_SAME
	return nullptr;
}

int Engine::VariantLoad(int v, const char* character_file, const char* text, size_t bytes)
{
	const char* what = text ? "dtrl_variant_load_json" : "dtrl_variant_load_file";
	int rc = KeysIdle(variant_keys_, what, v);
	if (rc != DTRL_OK) return rc;
	if (v == 0) return Fail(DTRL_ERR_ARG, std::string(what) + ": variant 0 is the batch's own model and cannot be replaced");
	if (rescale_on_ && v == rescale_base_) return Fail(DTRL_ERR_ARG, std::string(what) + ": variant " + std::to_string(v) + " is the base of the variant rescale (dtrl_variant_rescale): the private records are scaled copies of it; remove the rescale first");
	std::string doc; CharSource src;
	if (text) { doc.assign(text, bytes); src.name = "variant " + std::to_string(v) + " (JSON text)"; }
	else {
		if (!character_file || !*character_file) return Fail(DTRL_ERR_ARG, std::string(what) + ": character_file is required");
		src.name = character_file;
		const std::string path = ResolveDataPath(cfg_.data_root, character_file);
		FILE* fp = std::fopen(path.c_str(), "rb");
		if (!fp) return Fail(DTRL_ERR_IO, std::string(what) + ": cannot open " + path);
		char chunk[4096]; size_t k;
		while ((k = std::fread(chunk, 1, sizeof(chunk), fp)) > 0) doc.append(chunk, k);
		std::fclose(fp);
	}
	src.text = &doc;
	{   // the joint count first: the loader itself refuses a skeleton its controller does not expect, and that is a misfit, not a broken file
		Json root; std::string jerr;
		if (!Json::parse(doc, root, jerr)) return Fail(DTRL_ERR_IO, std::string(what) + ": " + src.name + ": " + jerr);
		const Json* skel = root.find("Skeleton"); const Json* joints = skel ? skel->find("Joints") : nullptr;
		if (joints && static_cast<int>(joints->arr.size()) != cfg_.model.L)
			return Fail(DTRL_ERR_ARG, std::string(what) + ": variant " + std::to_string(v) + " does not fit the batch: L differs (" + std::to_string(joints->arr.size()) + " joints, the batch's model has " + std::to_string(cfg_.model.L) + ")");
	}
	ScenarioConfig vc; std::string lerr;
	if (!LoadScenario(args_, vc, lerr, &src)) return Fail(DTRL_ERR_IO, std::string(what) + ": " + lerr);
	vc.model.has_net = cfg_.model.has_net;   // (the creation-time fix-up)
	if (const char* f = VariantMisfit(vc.model, cfg_.model))
		return Fail(DTRL_ERR_ARG, std::string(what) + ": variant " + std::to_string(v) + " does not fit the batch: " + f + " differs from the batch's model (the skeleton, the scene and the controller part -- parameters, actions, default action -- are one per batch)");
	if (!be_->H2D(d_var_models_ + v, &vc.model, sizeof(DevModel))) return Fail(DTRL_ERR_DEVICE, be_->error());
	var_models_[v] = vc.model; var_scalars_[v] = vc.scalars; variant_keys_.filled[v] = 1;
	return DTRL_OK;
}

// ---- variant redraw (include/dtrl.h: dtrl_variant_redraw, dtrl_variant_redraw_info) ----
// The rule is var_redraw_step (dtrl_terrain_dev.h), run at an env's episode start in front of the reset launch: by HostFrameWork's status loop (host terrain), by
// Backend::VariantRedraw queued between the boundary work and the reset launch (-terrain_gen= device), by RedrawListed under dtrl_reset. dtrl_engine.h says who
// owns the key array when.
int Engine::AssignVariants(const int32_t* env_ids, int n, const int32_t* variants)
{
	if (int rc = KeysCurrent(variant_keys_, "dtrl_assign_variants"); rc != DTRL_OK) return rc;   // (the whole-array upload below would otherwise undo every draw the kernel made)
	return KeysAssign(variant_keys_, "dtrl_assign_variants", env_ids, n, variants);
}
int Engine::GetVariants(const int32_t* env_ids, int n, int32_t* variants_out)
{
	if (int rc = KeysCurrent(variant_keys_, "dtrl_get_variants"); rc != DTRL_OK) return rc;   // with a redraw on device terrain: the variants as of the last completed boundary
	return KeysGet(variant_keys_, "dtrl_get_variants", env_ids, n, variants_out);
}
// (dtrl_reset only, never per frame: the streams are idle, and both arrays go up whole with synchronous copies -- O(num_envs) per call, whatever the list's length)
int Engine::RedrawListed(const std::vector<int32_t>& ids)
{
	if (!redraw_on_ || ids.empty()) return DTRL_OK;
	if (int rc = KeysRefresh(variant_keys_); rc != DTRL_OK) return rc;
	RedrawCfg rd = redraw_cfg_; rd.cum = redraw_cum_.host.data();
	for (int32_t e : ids) variant_keys_.env_key[e] = var_redraw_step(redraw_.host[e], variant_keys_.env_key[e], true, rd, rd.cum, e);
	return DevOk(be_->H2D(variant_keys_.d_env_key, variant_keys_.env_key.data(), sizeof(int32_t) * variant_keys_.env_key.size()) && redraw_.Push(*be_));
}

int Engine::VariantRedraw(int lo, int hi, uint64_t seed, const double* weights)
{
	const std::string w = "dtrl_variant_redraw: ";
	if (int rc = KeysIdle(variant_keys_, "dtrl_variant_redraw", 0); rc != DTRL_OK) return rc;
	if (int rc = KeysRefresh(variant_keys_); rc != DTRL_OK) return rc;   // (a redraw in place: the host keys and counters are current again before it goes or is replaced)
	if (lo > hi) { redraw_on_ = variant_keys_.on_device = false; return DTRL_OK; }   // the envs keep the variants they have, the counters stay
	const int V = variant_keys_.n_keys();
	if (lo < 0 || hi >= V) return Fail(DTRL_ERR_ARG, w + "variants " + std::to_string(lo) + " .. " + std::to_string(hi) + " out of range (variants 0 .. " + std::to_string(V - 1) + ")");
	for (int v = lo; v <= hi; ++v) if (!variant_keys_.filled[v]) return Fail(DTRL_ERR_ARG, w + "variant " + std::to_string(v) + " " + variant_keys_.empty_text + ": every variant of the redraw must be filled");
	const int m = hi - lo + 1;
	std::vector<double> cum(static_cast<size_t>(m));
	double sum = 0;
	for (int j = 0; j < m; ++j) {
		const double wj = weights ? weights[j] : 1.0;
		if (!(wj >= 0) || !std::isfinite(wj)) return Fail(DTRL_ERR_ARG, w + "weight " + std::to_string(j) + " (" + std::to_string(wj) + ") must be a non-negative finite number");
		sum += wj; cum[j] = sum;
	}
	if (!(sum > 0)) return Fail(DTRL_ERR_ARG, w + "the weights are all zero");
	if (!std::isfinite(sum)) return Fail(DTRL_ERR_ARG, w + "the sum of the weights is not a finite number");
	for (int j = 0; j < m; ++j) cum[j] /= sum;
	cum[m - 1] = 1.0;
	if (cfg_.device_terrain) {
		if (int rc = RecsAlloc(redraw_, static_cast<size_t>(n_)); rc != DTRL_OK) return rc;
		if (int rc = RecsAlloc(redraw_cum_, static_cast<size_t>(V)); rc != DTRL_OK) return rc;
	}
	if (redraw_.host.empty()) redraw_.host.assign(static_cast<size_t>(n_), RedrawRec{0});
	redraw_cum_.host.swap(cum);
	if (int rc = DevOk(redraw_cum_.Push(*be_) && redraw_.Push(*be_)); rc != DTRL_OK) return rc;
	redraw_cfg_ = RedrawCfg{lo, hi, seed, static_cast<int64_t>(cfg_.run.env_id_base), redraw_cum_.dev};
	redraw_on_ = true;
	variant_keys_.recs = &redraw_; variant_keys_.on_device = cfg_.device_terrain; variant_keys_.stale = false;
	return DTRL_OK;
}

int Engine::VariantRedrawInfo(const int32_t* env_ids, int n, int32_t* lo, int32_t* hi, int32_t* variant, int32_t* draws)
{
	if (int rc = RuleCallBegin("dtrl_variant_redraw_info", &variant_keys_, redraw_on_ ? nullptr : "the batch has no variant redraw (call dtrl_variant_redraw first)", {env_ids, n}, nullptr); rc != DTRL_OK) return rc;
	if (lo) *lo = redraw_cfg_.lo;
	if (hi) *hi = redraw_cfg_.hi;
	for (int i = 0; i < n; ++i) {
		const int e = EnvIndex(env_ids, i);
		if (variant) variant[i] = variant_keys_.env_key[e];
		if (draws) draws[i] = redraw_.host[e].draws;
	}
	return DTRL_OK;
}

// ---- variant rescale (include/dtrl.h: dtrl_variant_rescale, dtrl_variant_rescale_info, dtrl_variant_scalars) ----
// The rule is rescale_step (dtrl_terrain_dev.h), run by Backend::VariantRescale on the group's stream at every frame boundary, behind the redraw and in front of the
// push schedule and the reset launch -- queued by DeviceFrameWork and by HostFrameWork alike (RulesBeforeResets) -- and in its listed form by StartEpisodes under dtrl_reset. dtrl_engine.h
// says where the private records live and who writes them when.
int Engine::VariantRescale(int base, const int32_t* env_ids, int n, uint64_t seed, const double* lo4, const double* hi4, uint32_t per_link, bool remove)
{
	const std::string w = "dtrl_variant_rescale: ";
	if (int rc = KeysIdle(variant_keys_, "dtrl_variant_rescale", 0); rc != DTRL_OK) return rc;
	if (int rc = KeysRefresh(variant_keys_); rc != DTRL_OK) return rc;   // (a redraw on device terrain: the whole-array uploads below must not undo its draws)
	const int V = variant_keys_.n_keys();
	if (remove) {   // the envs under a private record go back to the base; counters and records stay
		if (!rescale_on_) return DTRL_OK;
		for (int32_t& k : variant_keys_.env_key) if (k >= V) k = rescale_base_;
		rescale_on_ = false;
		return DevOk(be_->H2D(variant_keys_.d_env_key, variant_keys_.env_key.data(), sizeof(int32_t) * variant_keys_.env_key.size()));
	}
	if (base < 0 || base >= V) return Fail(DTRL_ERR_ARG, w + "base " + std::to_string(base) + " out of range (variants 0 .. " + std::to_string(V - 1) + ")");
	if (!variant_keys_.filled[base]) return Fail(DTRL_ERR_ARG, w + "base: variant " + std::to_string(base) + " " + variant_keys_.empty_text);
	static const char* const name[kRescaleQuantities] = {"mass", "kp", "kd", "torque_lim"};
	for (int q = 0; q < kRescaleQuantities; ++q) {
		const double lo = lo4[q], hi = hi4[q];
		if (!std::isfinite(lo) || !std::isfinite(hi)) return Fail(DTRL_ERR_ARG, w + "range " + name[q] + " (" + std::to_string(lo) + ", " + std::to_string(hi) + ") must be two finite numbers");
		if (!(lo > 0)) return Fail(DTRL_ERR_ARG, w + "range " + name[q] + ": lo (" + std::to_string(lo) + ") must be greater than 0");
		if (lo > hi) return Fail(DTRL_ERR_ARG, w + "range " + name[q] + ": lo (" + std::to_string(lo) + ") exceeds hi (" + std::to_string(hi) + ")");
	}
	if (per_link >> kRescaleQuantities) return Fail(DTRL_ERR_ARG, w + "per_link (" + std::to_string(per_link) + ") has bits beyond the four quantities (mass 1, kp 2, kd 4, torque_lim 8)");
	if (int rc = CheckEnvList(w, env_ids, n, "; nothing changed"); rc != DTRL_OK) return rc;
	if (rescale_on_ && base != rescale_base_)
		for (int32_t k : variant_keys_.env_key) if (k >= V) return Fail(DTRL_ERR_ARG, w + "base " + std::to_string(base) + " differs from the rescale's base (" + std::to_string(rescale_base_) + ") while envs run under private records of that one: remove the rescale first");
	if (!rescale_table_) {   // once: the device table grows to V + num_envs records (the streams are idle), the old records copied from their host form
		DevModel* grown = static_cast<DevModel*>(be_->Alloc(sizeof(DevModel) * (static_cast<size_t>(V) + static_cast<size_t>(n_))));
		if (!grown) return Fail(DTRL_ERR_DEVICE, "device allocation failed: " + be_->error());
		allocs_.push_back(grown);
		if (!be_->H2D(grown, var_models_.data(), sizeof(DevModel) * static_cast<size_t>(V))) return Fail(DTRL_ERR_DEVICE, be_->error());
		auto old = std::find(allocs_.begin(), allocs_.end(), static_cast<void*>(d_var_models_));
		if (old != allocs_.end()) { be_->Free(*old); allocs_.erase(old); }
		d_var_models_ = grown;
		d_rescale_base_ = static_cast<ModelScalarsD*>(be_->Alloc(sizeof(ModelScalarsD)));
		if (!d_rescale_base_) return Fail(DTRL_ERR_DEVICE, "device allocation failed: " + be_->error());
		allocs_.push_back(d_rescale_base_);
		if (int rc = RecsAlloc(rescale_, static_cast<size_t>(n_)); rc != DTRL_OK) return rc;
		rescale_table_ = true;
	}
	if (!be_->H2D(d_rescale_base_, &var_scalars_[base], sizeof(ModelScalarsD))) return Fail(DTRL_ERR_DEVICE, be_->error());
	rescale_cfg_ = RescaleCfg{};
	for (int q = 0; q < kRescaleQuantities; ++q) { rescale_cfg_.lo[q] = lo4[q]; rescale_cfg_.hi[q] = hi4[q]; }
	rescale_cfg_.per_link = per_link; rescale_cfg_.L = cfg_.model.L; rescale_cfg_.seed = seed; rescale_cfg_.env_id_base = static_cast<int64_t>(cfg_.run.env_id_base);
	rescale_base_ = base; rescale_on_ = true;
	// the listed envs: key V + e, the private record a copy of the base (all factors 1) until the env's next episode start
	for (int i = 0; i < n; ++i) {
		const int e = EnvIndex(env_ids, i);
		if (!be_->H2D(d_var_models_ + V + e, &var_models_[base], sizeof(DevModel))) return Fail(DTRL_ERR_DEVICE, be_->error());
		variant_keys_.env_key[e] = V + e;
	}
	if (n > 0 && !be_->H2D(variant_keys_.d_env_key, variant_keys_.env_key.data(), sizeof(int32_t) * variant_keys_.env_key.size())) return Fail(DTRL_ERR_DEVICE, be_->error());
	return DTRL_OK;
}

int Engine::VariantRescaleInfo(const int32_t* env_ids, int n, int32_t* base, uint64_t* seed, double* lo4, double* hi4, uint32_t* per_link, int32_t* key, int32_t* episodes, double* factors)
{
	if (int rc = RuleCallBegin("dtrl_variant_rescale_info", &variant_keys_, rescale_on_ ? nullptr : "the batch has no variant rescale (call dtrl_variant_rescale first)", {env_ids, n}, &rescale_); rc != DTRL_OK) return rc;
	if (base) *base = rescale_base_;
	if (seed) *seed = rescale_cfg_.seed;
	for (int q = 0; q < kRescaleQuantities; ++q) { if (lo4) lo4[q] = rescale_cfg_.lo[q]; if (hi4) hi4[q] = rescale_cfg_.hi[q]; }
	if (per_link) *per_link = rescale_cfg_.per_link;
	const int L = cfg_.model.L, V = variant_keys_.n_keys();
	for (int i = 0; i < n; ++i) {
		const int e = EnvIndex(env_ids, i);
		const int32_t k = variant_keys_.env_key[e], ep = rescale_.host[e].episodes;
		if (key) key[i] = k;
		if (episodes) episodes[i] = ep;
		if (!factors) continue;
		// the factors of the env's CURRENT episode, by the rule from episode number episodes - 1; an env that is not under its private record, or has not started
		// an episode under the rescale yet, runs under factors 1
		const uint64_t sk = rescale_stream_key(rescale_cfg_.seed, rescale_cfg_.env_id_base + e);
		for (int q = 0; q < kRescaleQuantities; ++q) for (int j = 0; j < L; ++j)
			factors[(static_cast<size_t>(i) * kRescaleQuantities + q) * L + j] = (k == V + e && ep > 0) ? rescale_factor(rescale_cfg_, sk, ep - 1, q, j) : 1.0;
	}
	return DTRL_OK;
}

int Engine::VariantScalars(int env, double* out6L, double* total_mass)
{
	const std::string w = "dtrl_variant_scalars: ";
	if (int rc = RequireIdle("dtrl_variant_scalars" + std::string(kFrameInFlight)); rc != DTRL_OK) return rc;
	if (env < 0 || env >= n_) return Fail(DTRL_ERR_ARG, w + "env id " + std::to_string(env) + " out of range");
	const DevModel* src = d_model_;
	if (!var_models_.empty()) {
		if (int rc = KeysRefresh(variant_keys_); rc != DTRL_OK) return rc;
		src = d_var_models_ + variant_keys_.env_key[env];
	}
	DevModel m;
	if (!be_->D2H(&m, src, sizeof(m))) return Fail(DTRL_ERR_DEVICE, be_->error());
	const int L = m.L;
	const real* const rows[6] = {m.mass, m.inertia, m.sub_mass, m.kp, m.kd, m.torque_lim};
	if (out6L) for (int r = 0; r < 6; ++r) for (int j = 0; j < L; ++j) out6L[r * L + j] = static_cast<double>(rows[r][j]);
	if (total_mass) *total_mass = static_cast<double>(m.total_mass);
	return DTRL_OK;
}

// ---- push schedule (include/dtrl.h: dtrl_push_schedule, dtrl_push_scale, dtrl_push_info) ----
// The rule is push_step (dtrl_terrain_dev.h), run by Backend::PushSchedule on the group's stream at every frame boundary in front of the reset launch -- queued by
// DeviceFrameWork (-terrain_gen= device) and by HostFrameWork (host terrain) alike (RulesBeforeResets) -- and with `start` by StartEpisodes under dtrl_reset and a terrain restart.
// Records and scales live in device memory only.
int Engine::PushAlloc()
{
	if (int rc = RecsAlloc(push_, static_cast<size_t>(n_), PushRec{0, 0u, 0, -1, {0.0, 0.0}, 0.0}); rc != DTRL_OK) return rc;   // (last_link -1: no push yet)
	return RecsAlloc(push_scale_, static_cast<size_t>(n_), 1.0);
}
int Engine::PushSchedule(int min_wait, int max_wait, uint64_t seed, double min_force, double max_force, double min_dur, double max_dur)
{
	const std::string w = "dtrl_push_schedule: ";
	if (cfg_.external_policy) return Fail(DTRL_ERR_ARG, w + "not available with -policy_mode= external (a parked env's boundaries are not frames: a wait counted in ticks would depend on the caller's pace)");
	if (int rc = RequireIdle("dtrl_push_schedule" + std::string(kFrameInFlight)); rc != DTRL_OK) return rc;
	if (min_wait > max_wait) { push_on_ = false; return DTRL_OK; }   // records, counters and scales stay; a push already in a slot runs out as it would have
	if (min_wait < 1) return Fail(DTRL_ERR_ARG, w + "min_wait (" + std::to_string(min_wait) + ") must be at least 1 frame boundary");
	if (std::isnan(min_force)) min_force = cfg_.min_perturb;
	if (std::isnan(max_force)) max_force = cfg_.max_perturb;
	if (std::isnan(min_dur)) min_dur = cfg_.min_perturb_duration;
	if (std::isnan(max_dur)) max_dur = cfg_.max_perturb_duration;
	const double v[4] = {min_force, max_force, min_dur, max_dur};
	const char* const name[4] = {"min_force", "max_force", "min_dur", "max_dur"};
	for (int i = 0; i < 4; ++i) if (!(v[i] >= 0) || !std::isfinite(v[i])) return Fail(DTRL_ERR_ARG, w + name[i] + " (" + std::to_string(v[i]) + ") must be a non-negative finite number");
	if (min_force > max_force) return Fail(DTRL_ERR_ARG, w + "min_force exceeds max_force");
	if (min_dur > max_dur) return Fail(DTRL_ERR_ARG, w + "min_dur exceeds max_dur");
	if (int rc = PushAlloc(); rc != DTRL_OK) return rc;
	push_cfg_ = PushCfg{min_wait, max_wait, min_force, max_force, min_dur, max_dur, seed, static_cast<int64_t>(cfg_.run.env_id_base), cfg_.model.L, 0};
	push_on_ = true;
	// every env of the schedule draws its first wait under the new settings (the counters go on where they were)
	return DevOk(PushQueue(nullptr, EnvSpan{0, n_, nullptr}) && be_->Sync());
}
int Engine::PushScale(const int32_t* env_ids, int n, const double* scales)
{
	const std::string w = "dtrl_push_scale: ";
	if (int rc = RuleCallBegin("dtrl_push_scale", nullptr, nullptr, {env_ids, n, "; nothing changed", "scales", scales}, nullptr); rc != DTRL_OK) return rc;
	for (int i = 0; i < n; ++i) {   // all or nothing
		const int e = EnvIndex(env_ids, i);
		if (!(scales[i] >= 0) || !std::isfinite(scales[i])) return Fail(DTRL_ERR_ARG, w + "scale " + std::to_string(scales[i]) + " of env " + std::to_string(e) + " must be a non-negative finite number; nothing changed");
	}
	if (int rc = PushAlloc(); rc != DTRL_OK) return rc;
	if (int rc = DevOk(push_scale_.Pull(*be_)); rc != DTRL_OK) return rc;
	for (int i = 0; i < n; ++i) push_scale_.host[EnvIndex(env_ids, i)] = scales[i];
	return DevOk(push_scale_.Push(*be_));
}
int Engine::PushInfo(const int32_t* env_ids, int n, int32_t* wait, int32_t* pushes, int32_t* last_link, double* last_force, double* last_dur)
{
	if (int rc = RuleCallBegin("dtrl_push_info", nullptr, push_.dev ? nullptr : "the batch has no push schedule (call dtrl_push_schedule first)", {env_ids, n}, &push_); rc != DTRL_OK) return rc;
	for (int i = 0; i < n; ++i) {
		const PushRec& r = push_.host[EnvIndex(env_ids, i)];
		if (wait) wait[i] = r.wait;
		if (pushes) pushes[i] = r.pushes;
		if (last_link) last_link[i] = r.last_link;
		if (last_force) { last_force[2 * i] = r.last_f[0]; last_force[2 * i + 1] = r.last_f[1]; }
		if (last_dur) last_dur[i] = r.last_dur;
	}
	return DTRL_OK;
}

// ---- episode limit (include/dtrl.h: dtrl_episode_limit, dtrl_episode_limit_envs, dtrl_episode_info) ----
// The rule is episode_limit_step (dtrl_terrain_dev.h), run by Backend::EpisodeLimit on the group's stream at every frame boundary in front of every other rule --
// queued first by DeviceFrameWork (-terrain_gen= device), behind the frame launch by LaunchGroup (host terrain) (RulesBehindFrame) -- and in its listed form by
// StartEpisodes under dtrl_reset and a terrain restart, and by dtrl_episode_limit_envs for an env coming in. Records and flags live in device memory only.
int Engine::EpisodeAlloc()
{
	if (int rc = RecsAlloc(episode_, static_cast<size_t>(n_)); rc != DTRL_OK) return rc;   // (zero-filled: no episode yet)
	return RecsAlloc(episode_flag_, static_cast<size_t>(n_), uint8_t(1));
}
int Engine::EpisodeLimit(int min_frames, int max_frames, double max_dist, uint64_t seed)
{
	const std::string w = "dtrl_episode_limit: ";
	if (cfg_.external_policy) return Fail(DTRL_ERR_ARG, w + "not available with -policy_mode= external (a parked env's boundaries are ticks, not frames: an episode counted in them would depend on the caller's pace)");
	if (int rc = RequireIdle("dtrl_episode_limit" + std::string(kFrameInFlight)); rc != DTRL_OK) return rc;
	if (std::isnan(max_dist)) return Fail(DTRL_ERR_ARG, w + "max_dist is NaN (+inf or a value <= 0 means no distance limit); nothing changed");
	if (min_frames < 0) return Fail(DTRL_ERR_ARG, w + "min_frames (" + std::to_string(min_frames) + ") must not be negative; nothing changed");
	if (min_frames > max_frames) return Fail(DTRL_ERR_ARG, w + "min_frames (" + std::to_string(min_frames) + ") exceeds max_frames (" + std::to_string(max_frames) + "); nothing changed");
	if (min_frames == 0 && max_frames != 0) return Fail(DTRL_ERR_ARG, w + "exactly one of min_frames / max_frames is 0 (both 0 mean no frame limit, else 1 <= min_frames <= max_frames); nothing changed");
	if (!(max_dist > 0)) max_dist = std::numeric_limits<double>::infinity();
	if (max_frames == 0 && std::isinf(max_dist)) { episode_on_ = false; return DTRL_OK; }   // removed: records, counters and flags stay
	if (int rc = EpisodeAlloc(); rc != DTRL_OK) return rc;
	episode_cfg_ = EpisodeCfg{min_frames, max_frames, max_dist, SpawnX(cfg_.model), seed, static_cast<int64_t>(cfg_.run.env_id_base), cfg_.model.scenario == kScnPoliEval ? 1 : 0, 0};
	episode_on_ = true;
	// every env under the limit starts an episode under the new settings: frames 0, a new limit (the counters and the draw streams go on where they were)
	return DevOk(EpisodeQueue(nullptr, EnvSpan{0, n_, nullptr}) && be_->Sync());
}
int Engine::EpisodeLimitEnvs(const int32_t* env_ids, int n, const uint8_t* on)
{
	if (int rc = RuleCallBegin("dtrl_episode_limit_envs", nullptr, nullptr, {env_ids, n, "; nothing changed", "on", on}, nullptr); rc != DTRL_OK) return rc;
	if (int rc = EpisodeAlloc(); rc != DTRL_OK) return rc;
	if (int rc = DevOk(episode_flag_.Pull(*be_)); rc != DTRL_OK) return rc;
	const std::vector<uint8_t> before = episode_flag_.host;
	for (int i = 0; i < n; ++i) episode_flag_.host[EnvIndex(env_ids, i)] = on[i] ? 1 : 0;   // (an env listed twice: its last flag holds)
	std::vector<int32_t> came_in;
	for (int e = 0; e < n_; ++e) if (episode_flag_.host[e] && !before[e]) came_in.push_back(e);
	if (int rc = DevOk(episode_flag_.Push(*be_)); rc != DTRL_OK) return rc;
	if (episode_on_ && !came_in.empty()) {   // an env that comes in while a limit runs starts an episode record now
		const int32_t* list = StageIds(came_in);
		if (!list) return DTRL_ERR_DEVICE;
		if (!EpisodeQueue(nullptr, EnvSpan{0, static_cast<int>(came_in.size()), list})) return Fail(DTRL_ERR_DEVICE, be_->error());
	}
	return DevOk(be_->Sync());
}
int Engine::EpisodeInfo(const int32_t* env_ids, int n, int32_t* frames, int32_t* limit, int64_t* by_fall, int64_t* by_limit, int32_t* last_frames, double* last_dist, int32_t* last_cause)
{
	if (int rc = RuleCallBegin("dtrl_episode_info", nullptr, episode_.dev ? nullptr : "the batch has no episode limit (call dtrl_episode_limit or dtrl_episode_limit_envs first)", {env_ids, n}, &episode_); rc != DTRL_OK) return rc;
	for (int i = 0; i < n; ++i) {
		const EpisodeRec& r = episode_.host[EnvIndex(env_ids, i)];
		if (frames) frames[i] = r.frames;
		if (limit) limit[i] = r.limit;
		if (by_fall) by_fall[i] = r.by_fall;
		if (by_limit) by_limit[i] = r.by_limit;
		if (last_frames) last_frames[i] = r.last_frames;
		if (last_dist) last_dist[i] = r.last_dist;
		if (last_cause) last_cause[i] = r.last_cause;
	}
	return DTRL_OK;
}

// ---- frame trace (include/dtrl.h: dtrl_trace, dtrl_trace_info, dtrl_trace_read, dtrl_trace_read_device) ----
// The rule is trace_due / trace_value / trace_int (dtrl_terrain_dev.h), run by Backend::TraceRecord on the group's stream at every frame boundary right behind the
// episode limit (RulesBehindFrame: queued by DeviceFrameWork with -terrain_gen= device, behind the frame launch by LaunchGroup with host terrain) over the group's
// own list of traced indices. No listed episode start queues it. Rings, counters and lists live in device memory only.
void Engine::TraceFree()
{
	void* const owned[] = {trace_.v.vals, trace_.v.ints, trace_.v.written, trace_.d_env_of, trace_.d_list};
	for (void* p : owned) if (p) be_->Free(p);
	trace_ = TraceState();
}
bool Engine::TraceQueue(int group)
{
	if (trace_.v.n_traced == 0 || trace_.group_n[group] == 0) return true;
	TraceView v = trace_.v;
	v.env_slot = slot_keys_.d_env_key; v.env_variant = variant_keys_.d_env_key; v.env_terrain = terrain_keys_.d_env_key;
	return be_->TraceRecord(buf_.st, buf_.status, v, trace_.d_list + trace_.group_off[group], trace_.group_n[group]);
}
int Engine::Trace(const int32_t* env_ids, int n, int frames)
{
	const std::string w = "dtrl_trace: ";
	if (int rc = RequireIdle("dtrl_trace" + std::string(kFrameInFlight)); rc != DTRL_OK) return rc;
	if (n == 0) { TraceFree(); return DTRL_OK; }   // removed
	if (!env_ids) n = n_;   // every env
	if (n < 0 || n > n_) return Fail(DTRL_ERR_ARG, w + "the env count must be 0 .. num_envs (" + std::to_string(n_) + "), not " + std::to_string(n) + "; nothing changed");
	if (frames < 1) return Fail(DTRL_ERR_ARG, w + "frames must be >= 1, not " + std::to_string(frames) + "; nothing changed");
	std::vector<int32_t> ids(static_cast<size_t>(n));
	for (int i = 0; i < n; ++i) ids[i] = EnvIndex(env_ids, i);
	if (int rc = CheckSlots(ids.data(), n, "dtrl_trace"); rc != DTRL_OK) { err_ += "; nothing changed"; return rc; }
	// the old trace goes first: a second call replaces it, and a ring that does not fit leaves the batch without one
	TraceFree();
	const int D = cfg_.model.D, W = 3 * D + 2;
	const size_t rows = static_cast<size_t>(n) * static_cast<size_t>(frames);
	if (rows > (static_cast<size_t>(1) << 40) / (sizeof(double) * W))   // (n and frames are ints: the product fits; beyond 2^40 bytes the byte counts below are not formed at all)
		return Fail(DTRL_ERR_CAPACITY, w + std::to_string(n) + " envs x " + std::to_string(frames) + " rows do not fit; the batch has no trace");
	TraceState& t = trace_;
	t.v.vals = static_cast<double*>(be_->Alloc(rows * W * sizeof(double)));
	t.v.ints = t.v.vals ? static_cast<int32_t*>(be_->Alloc(rows * kTraceInts * sizeof(int32_t))) : nullptr;
	t.v.written = t.v.ints ? static_cast<int64_t*>(be_->Alloc(sizeof(int64_t) * ids.size())) : nullptr;
	t.d_env_of = t.v.written ? static_cast<int32_t*>(be_->Alloc(sizeof(int32_t) * ids.size())) : nullptr;
	t.d_list = t.d_env_of ? static_cast<int32_t*>(be_->Alloc(sizeof(int32_t) * ids.size())) : nullptr;
	if (!t.d_list) { const std::string why = be_->error(); TraceFree(); return Fail(DTRL_ERR_CAPACITY, w + "the ring of " + std::to_string(n) + " envs x " + std::to_string(frames) + " rows does not fit (" + why + "); the batch has no trace"); }
	// the per-group lists: the traced indices regrouped by env group, the caller's order kept inside a group
	const int G = static_cast<int>(groups_.size());
	t.group_off.assign(static_cast<size_t>(G), 0); t.group_n.assign(static_cast<size_t>(G), 0);
	t.index_of.assign(static_cast<size_t>(n_), -1);
	std::vector<int32_t> list;
	for (int g = 0; g < G; ++g) {
		t.group_off[g] = static_cast<int32_t>(list.size());
		for (int i = 0; i < n; ++i) if (ids[i] >= groups_[g].e0 && ids[i] < groups_[g].e0 + groups_[g].n) list.push_back(i);
		t.group_n[g] = static_cast<int32_t>(list.size()) - t.group_off[g];
	}
	for (int i = 0; i < n; ++i) t.index_of[ids[i]] = i;
	if (!be_->H2D(t.d_env_of, ids.data(), sizeof(int32_t) * ids.size()) || !be_->H2D(t.d_list, list.data(), sizeof(int32_t) * list.size()) || !be_->Sync()) {   // (Alloc's zero fill is queued: the rings and counters are 0 behind the wait)
		const std::string why = be_->error(); TraceFree(); return Fail(DTRL_ERR_DEVICE, why);
	}
	t.ids.swap(ids);
	t.v.env_of = t.d_env_of; t.v.frames = frames; t.v.D = D; t.v.W = W; t.v.n_traced = n;
	return DTRL_OK;
}
int Engine::TraceInfo(int32_t* n_traced, int32_t* frames, int32_t* width, int32_t* env_ids_out, int64_t* rows_written_out)
{
	if (int rc = RequireIdle("dtrl_trace_info" + std::string(kFrameInFlight)); rc != DTRL_OK) return rc;
	const TraceView& v = trace_.v;
	if (n_traced) *n_traced = v.n_traced;
	if (frames) *frames = v.frames;
	if (width) *width = 3 * cfg_.model.D + 2;
	if (env_ids_out) std::copy(trace_.ids.begin(), trace_.ids.end(), env_ids_out);
	if (rows_written_out && v.n_traced > 0) return DevOk(be_->D2H(rows_written_out, v.written, sizeof(int64_t) * static_cast<size_t>(v.n_traced)));
	return DTRL_OK;
}
int Engine::TraceRead(const int32_t* env_ids, int n, int max_rows, double* vals, int32_t* ints, int32_t* counts, bool device)
{
	const char* what = device ? "dtrl_trace_read_device" : "dtrl_trace_read";
	const std::string w = std::string(what) + ": ";
	if (int rc = RequireIdle(what + std::string(kFrameInFlight)); rc != DTRL_OK) return rc;
	const TraceView& v = trace_.v;
	if (v.n_traced == 0) return Fail(DTRL_ERR_ARG, w + "the batch has no trace (call dtrl_trace first)");
	if (!env_ids) n = v.n_traced;   // every traced env, in the order dtrl_trace listed them
	if (n < 0 || n > v.n_traced) return Fail(DTRL_ERR_ARG, w + "the env count must be 0 .. " + std::to_string(v.n_traced) + " (the traced envs), not " + std::to_string(n));
	if (max_rows < 0 || (n > 0 && (!counts || (max_rows > 0 && (!vals || !ints))))) return Fail(DTRL_ERR_ARG, w + "vals, ints and counts are required and max_rows must not be negative");
	if (n == 0) return DTRL_OK;
	const int cap = std::min(max_rows, v.frames);   // rows a slice can hold at most
	if (static_cast<int64_t>(n) * std::max(cap, 1) > INT32_MAX) return Fail(DTRL_ERR_CAPACITY, w + std::to_string(n) + " envs x " + std::to_string(cap) + " rows are more than one call moves: read fewer envs or rows per call");
	// staging: [vals n x cap x W, host read only][ints n x cap x 12, host read only][list n][counts n]
	const size_t rows = device ? 0 : static_cast<size_t>(n) * cap;
	const size_t off_ints = rows * v.W * sizeof(double), off_list = off_ints + rows * kTraceInts * sizeof(int32_t), bytes = off_list + 2 * sizeof(int32_t) * static_cast<size_t>(n);
	if (trace_stage_bytes_ < bytes) {
		be_->FreeHostStaging(trace_stage_);
		trace_stage_bytes_ = 0;
		trace_stage_ = static_cast<char*>(be_->HostStaging(bytes));
		if (!trace_stage_) return Fail(DTRL_ERR_CAPACITY, w + "page-locked staging for " + std::to_string(n) + " envs x " + std::to_string(cap) + " rows does not fit: read fewer envs or rows per call");
		trace_stage_bytes_ = bytes;
	}
	double* s_vals = reinterpret_cast<double*>(trace_stage_); int32_t* s_ints = reinterpret_cast<int32_t*>(trace_stage_ + off_ints);
	int32_t* s_list = reinterpret_cast<int32_t*>(trace_stage_ + off_list); int32_t* s_counts = s_list + n;
	for (int i = 0; i < n; ++i) {
		const int e = env_ids ? env_ids[i] : trace_.ids[i];
		if (e < 0 || e >= n_) return Fail(DTRL_ERR_ARG, w + "env id " + std::to_string(e) + " out of range");
		if (trace_.index_of[e] < 0) return Fail(DTRL_ERR_ARG, w + "env " + std::to_string(e) + " is not traced");
		s_list[i] = trace_.index_of[e]; s_counts[i] = 0;
	}
	const bool ok = device ? be_->TraceGather(v, s_list, n, max_rows, max_rows, vals, ints, s_counts, false) : be_->TraceGather(v, s_list, n, max_rows, cap, s_vals, s_ints, s_counts, true);
	if (!ok || !be_->Sync()) return Fail(DTRL_ERR_DEVICE, be_->error());
	for (int i = 0; i < n; ++i) {
		counts[i] = s_counts[i];
		if (device) continue;
		const size_t c = static_cast<size_t>(s_counts[i]), src = static_cast<size_t>(i) * cap, dst = static_cast<size_t>(i) * max_rows;
		std::copy(s_vals + src * v.W, s_vals + (src + c) * v.W, vals + dst * v.W);
		std::copy(s_ints + src * kTraceInts, s_ints + (src + c) * kTraceInts, ints + dst * kTraceInts);
	}
	return DTRL_OK;
}

// ---- episode log (include/dtrl.h: dtrl_episode_log, dtrl_episode_log_info, dtrl_episode_log_drain, dtrl_variant_rescale_factors) ----
// The rule is log_count / log_row / log_start (dtrl_terrain_dev.h), run by Backend::EpisodeLog on the group's stream at every frame boundary behind the episode
// limit and the trace (RulesBehindFrame: queued by DeviceFrameWork with -terrain_gen= device, behind the frame launch by LaunchGroup with host terrain) over the
// group's span into the group's own ring, and in its listed form by StartEpisodes. Rings and cursor words are page-locked host memory: a drain reads them with
// plain loads and queues nothing, also while a frame is in flight.
constexpr int kLogCursorWords = 4;   // per group: written, boundary, reserved, 0
void Engine::LogFree()
{
	be_->FreeHostStaging(log_.rings); be_->FreeHostStaging(log_.cursors);
	log_ = LogState();
}
bool Engine::LogQueue(const EnvStatus* status, const EnvSpan& span, int group)
{
	if (log_.capacity == 0) return true;
	LogView v{};
	v.recs = log_recs_.dev;
	if (status) { v.ring = log_.rings + static_cast<size_t>(group) * static_cast<size_t>(log_.capacity); v.cursor = log_.cursors + static_cast<size_t>(group) * kLogCursorWords; }
	if (episode_on_) { v.episode = episode_.dev; v.episode_on = episode_flag_.dev; }
	v.env_slot = slot_keys_.d_env_key; v.env_variant = variant_keys_.d_env_key; v.env_terrain = terrain_keys_.d_env_key;   // (a family may be created after the log)
	if (rescale_table_ && rescale_.dev) { v.rescale = rescale_.dev; v.private_base = static_cast<int32_t>(var_models_.size()); }
	v.spawn_x = SpawnX(cfg_.model); v.capacity = log_.capacity; v.external = cfg_.external_policy ? 1 : 0;
	return be_->EpisodeLog(buf_.st, status, span, v);
}
int Engine::EpisodeLog(int capacity)
{
	const std::string w = "dtrl_episode_log: ";
	if (int rc = RequireIdle("dtrl_episode_log" + std::string(kFrameInFlight)); rc != DTRL_OK) return rc;
	if (capacity < 0) return Fail(DTRL_ERR_ARG, w + "capacity (" + std::to_string(capacity) + ") must not be negative (0 removes the log); nothing changed");
	// the old log goes first: a second call replaces it, and a ring that does not fit leaves the batch without one
	LogFree();
	if (capacity == 0) return DTRL_OK;   // removed (the records stay allocated; the next log zeroes them)
	if (int rc = RecsAlloc(log_recs_, static_cast<size_t>(n_)); rc != DTRL_OK) return rc;
	const size_t G = groups_.size(), rows = G * static_cast<size_t>(capacity);
	const std::string no_fit = w + std::to_string(G) + " rings of " + std::to_string(capacity) + " rows do not fit";
	if (rows > (static_cast<size_t>(1) << 40) / sizeof(LogRow)) return Fail(DTRL_ERR_CAPACITY, no_fit + "; the batch has no episode log");
	log_.rings = static_cast<LogRow*>(be_->HostStaging(rows * sizeof(LogRow)));
	log_.cursors = log_.rings ? static_cast<int64_t*>(be_->HostStaging(G * kLogCursorWords * sizeof(int64_t))) : nullptr;
	if (!log_.cursors) { const std::string why = be_->error(); LogFree(); return Fail(DTRL_ERR_CAPACITY, no_fit + " into page-locked host memory (" + why + "); the batch has no episode log"); }
	std::memset(static_cast<void*>(log_.rings), 0, rows * sizeof(LogRow)); std::memset(log_.cursors, 0, G * kLogCursorWords * sizeof(int64_t));
	log_.drained.assign(G, 0); log_.lost.assign(G, 0);
	log_recs_.host.assign(static_cast<size_t>(n_), LogRec{0, 0, 0, 0, 0});
	if (!log_recs_.Push(*be_)) { const std::string why = be_->error(); LogFree(); return Fail(DTRL_ERR_DEVICE, why); }
	log_.capacity = capacity;
	// every env's logged episode starts here: frames 0, cycles counted from the env's cycle counter as it stands
	if (!LogQueue(nullptr, EnvSpan{0, n_, nullptr}, -1) || !be_->Sync()) { const std::string why = be_->error(); LogFree(); return Fail(DTRL_ERR_DEVICE, why); }
	return DTRL_OK;
}
int Engine::EpisodeLogInfo(int32_t* capacity, int32_t* n_groups, int64_t* written, int64_t* lost)
{
	if (int rc = RequireIdle("dtrl_episode_log_info" + std::string(kFrameInFlight)); rc != DTRL_OK) return rc;
	int64_t w = 0, l = 0;
	for (size_t g = 0; g < log_.drained.size(); ++g) {
		const int64_t wg = log_.cursors[g * kLogCursorWords];
		w += wg;
		l += log_.lost[g] + std::max<int64_t>(0, wg - log_.drained[g] - log_.capacity);   // found by a drain, or overwritten since the last one
	}
	if (capacity) *capacity = log_.capacity;
	if (n_groups) *n_groups = log_.capacity ? static_cast<int32_t>(groups_.size()) : 0;
	if (written) *written = w;
	if (lost) *lost = l;
	return DTRL_OK;
}
// Per group: read the cursor w0, copy rows [drained, w0) (at most the last `capacity`), then read the reservation and the cursor again and drop every copied row
// whose slot a boundary written meanwhile has taken, or was taking. The groups' rows are then merged in (boundary, env) order; what max_rows leaves stays.
int Engine::EpisodeLogDrain(void* out, int max_rows, int32_t* n_out, int64_t* lost)
{
	const std::string w = "dtrl_episode_log_drain: ";
	if (n_out) *n_out = 0;
	if (lost) *lost = 0;
	if (log_.capacity == 0) return Fail(DTRL_ERR_ARG, w + "the batch has no episode log (call dtrl_episode_log first)");
	if (max_rows < 0 || (max_rows > 0 && !out) || !n_out) return Fail(DTRL_ERR_ARG, w + "out and n are required and max_rows must not be negative");
	if (!step_pending_ && !early_any_) {   // no frame in flight: every boundary queued so far is visible behind the wait. In flight: what has been published, no wait
		be_->SelectStream(0);
		if (!be_->Sync()) return Fail(DTRL_ERR_DEVICE, be_->error());
	}
	const size_t G = log_.drained.size();
	const int64_t cap = log_.capacity;
	std::vector<size_t> begin(G + 1, 0);
	log_stage_.clear();
	int64_t lost_now = 0;
	for (size_t g = 0; g < G; ++g) {
		const int64_t* cur = log_.cursors + g * kLogCursorWords;
		const LogRow* ring = log_.rings + g * static_cast<size_t>(cap);
		const int64_t w0 = __atomic_load_n(cur, __ATOMIC_ACQUIRE);
		int64_t from = std::max(log_.drained[g], w0 - cap);
		begin[g] = log_stage_.size();
		for (int64_t i = from; i < w0; ++i) log_stage_.push_back(ring[i % cap]);
		__atomic_thread_fence(__ATOMIC_SEQ_CST);
		const int64_t r1 = __atomic_load_n(cur + 2, __ATOMIC_ACQUIRE), w1 = __atomic_load_n(cur, __ATOMIC_ACQUIRE);
		const int64_t valid = std::max(from, std::max(r1, w1) - cap);
		if (valid > from) { const size_t drop = static_cast<size_t>(std::min(valid, w0) - from); log_stage_.erase(log_stage_.begin() + begin[g], log_stage_.begin() + begin[g] + drop); from = std::min(valid, w0); }
		lost_now += from - log_.drained[g]; log_.lost[g] += from - log_.drained[g];
		log_.drained[g] = from;
	}
	begin[G] = log_stage_.size();
	std::vector<size_t> at(begin.begin(), begin.begin() + G);
	int32_t n = 0;
	while (n < max_rows) {
		int best = -1;
		for (size_t g = 0; g < G; ++g) {
			if (at[g] == begin[g + 1]) continue;
			const LogRow& c = log_stage_[at[g]];
			if (best < 0 || c.boundary < log_stage_[at[best]].boundary || (c.boundary == log_stage_[at[best]].boundary && c.env < log_stage_[at[best]].env)) best = static_cast<int>(g);
		}
		if (best < 0) break;
		std::memcpy(static_cast<char*>(out) + static_cast<size_t>(n++) * sizeof(LogRow), &log_stage_[at[best]++], sizeof(LogRow));   // (the caller's buffer need not be 16-byte aligned)
		log_.drained[best] += 1;
	}
	*n_out = n;
	if (lost) *lost = lost_now;
	return DTRL_OK;
}
int Engine::VariantRescaleFactors(const int32_t* env_ids, const int32_t* draws, int n, double* factors)
{
	const std::string w = "dtrl_variant_rescale_factors: ";
	if (!rescale_on_) return Fail(DTRL_ERR_ARG, w + "the batch has no variant rescale (call dtrl_variant_rescale first)");
	if (n < 0 || (n > 0 && (!env_ids || !draws || !factors))) return Fail(DTRL_ERR_ARG, w + "env_ids, draws and factors are required and n must not be negative");
	const int L = cfg_.model.L;
	for (int i = 0; i < n; ++i) if (env_ids[i] < 0 || env_ids[i] >= n_ || draws[i] < -1) return Fail(DTRL_ERR_ARG, w + "pair " + std::to_string(i) + ": env id " + std::to_string(env_ids[i]) + " out of range, or a draw below -1");
	for (int i = 0; i < n; ++i) {
		const uint64_t sk = rescale_stream_key(rescale_cfg_.seed, rescale_cfg_.env_id_base + env_ids[i]);
		for (int q = 0; q < kRescaleQuantities; ++q) for (int j = 0; j < L; ++j)
			factors[(static_cast<size_t>(i) * kRescaleQuantities + q) * L + j] = draws[i] >= 0 ? rescale_factor(rescale_cfg_, sk, draws[i], q, j) : 1.0;
	}
	return DTRL_OK;
}

// ---- terrain sets (include/dtrl.h: dtrl_terrains_create ... dtrl_terrain_stats) ----
// The third per-env key family, and the one no frame launch reads: a terrain decides what an env's NEXT segments look like, and segments are built at the frame
// boundary -- by the env's GroundWindow on the host, or by the boundary kernel (-terrain_gen= device), which takes the table and the per-env array as two extra
// pointers. So terrains neither touch LaunchEnvs nor exclude slots, variants or external policy mode. The timing rules are those of the other families (KeysIdle).
// With a terrain ladder on device terrain the DEVICE key array is the truth while frames run: the calls that read or upload it refresh the host copy first (KeysCurrent).
int Engine::TerrainsCreate(int n_terrains)
{
	if (n_terrains < 1 || n_terrains > n_) return Fail(DTRL_ERR_ARG, "dtrl_terrains_create: n_terrains must be 1 .. num_envs (" + std::to_string(n_) + "), not " + std::to_string(n_terrains));
	if (!terrain_table_.empty()) {
		if (n_terrains == static_cast<int>(terrain_table_.size())) return DTRL_OK;
		return Fail(DTRL_ERR_ARG, "dtrl_terrains_create: the batch already has " + std::to_string(terrain_table_.size()) + " terrains; a second call with another count (" + std::to_string(n_terrains) + ") is refused");
	}
	if (int rc = RequireIdle(std::string("dtrl_terrains_create") + kFrameInFlight); rc != DTRL_OK) return rc;
	TerrainCfg* table = static_cast<TerrainCfg*>(KeysAllocate(terrain_keys_, sizeof(TerrainCfg) * static_cast<size_t>(n_terrains)));
	if (!table) return DTRL_ERR_DEVICE;
	double params[kNumTerrainParams];
	LerpTerrainParams(cfg_, terrain_lerp_, params);
	std::vector<TerrainCfg> host(static_cast<size_t>(n_terrains), MakeTerrainCfg(cfg_.terrain_type, params));   // (an empty terrain holds the batch's until it is filled; it cannot be assigned)
	if (!be_->H2D(table, host.data(), sizeof(TerrainCfg) * host.size())) return Fail(DTRL_ERR_DEVICE, be_->error());
	d_terrain_table_ = table; terrain_table_.swap(host);
	terrain_src_.assign(static_cast<size_t>(n_terrains), TerrainSource());
	terrain_keys_.filled.assign(static_cast<size_t>(n_terrains), 0); terrain_keys_.filled[0] = 1;
	return DTRL_OK;
}

int Engine::TerrainFill(const char* what, int t, int type, const double* params)
{
	const TerrainCfg c = MakeTerrainCfg(type, params);
	if (!be_->H2D(d_terrain_table_ + t, &c, sizeof(c))) return Fail(DTRL_ERR_DEVICE, std::string(what) + ": " + be_->error());
	terrain_table_[t] = c; terrain_keys_.filled[t] = 1;
	if (!cfg_.device_terrain) for (int e = 0; e < n_; ++e) if (terrain_keys_.env_key[e] == t) grounds_[e].SetTerrain(type, params);   // next segment build, like a curriculum step
	return DTRL_OK;
}

int Engine::TerrainSetFile(int t, const char* terrain_file, double lerp)
{
	const char* what = "dtrl_terrain_set_file";
	if (int rc = KeysIdle(terrain_keys_, what, t); rc != DTRL_OK) return rc;
	if (t == 0) return Fail(DTRL_ERR_ARG, std::string(what) + ": terrain 0 is the batch's own terrain (-terrain_file=) and cannot be replaced; dtrl_set_terrain_lerp moves it");
	if (!terrain_file || !*terrain_file) return Fail(DTRL_ERR_ARG, std::string(what) + ": terrain_file is required");
	const std::string path = ResolveDataPath(cfg_.data_root, terrain_file);
	TerrainSource src; int type = 0; std::string lerr;
	const int bad = LoadTerrainFile(path, type, src.sets, lerr);
	if (bad == 1) return Fail(DTRL_ERR_IO, std::string(what) + ": terrain " + std::to_string(t) + ": " + lerr);
	if (bad) return Fail(DTRL_ERR_ARG, std::string(what) + ": terrain " + std::to_string(t) + ": " + path + ": " + lerr);
	double params[kNumTerrainParams];
	LerpTerrainParams(src.sets, lerp, params);
	src.lerp = lerp;
	if (int rc = TerrainFill(what, t, type, params); rc != DTRL_OK) return rc;
	terrain_src_[t] = src;
	return DTRL_OK;
}

int Engine::TerrainSetParams(int t, const char* type_name, const double* params40)
{
	const char* what = "dtrl_terrain_set_params";
	if (int rc = KeysIdle(terrain_keys_, what, t); rc != DTRL_OK) return rc;
	if (t == 0) return Fail(DTRL_ERR_ARG, std::string(what) + ": terrain 0 is the batch's own terrain (-terrain_file=) and cannot be replaced; dtrl_set_terrain_lerp moves it");
	if (!type_name || !params40) return Fail(DTRL_ERR_ARG, std::string(what) + ": type_name and params40 are required");
	const int type = TerrainTypeByName(type_name);
	if (type < 0) return Fail(DTRL_ERR_ARG, std::string(what) + ": terrain " + std::to_string(t) + ": unsupported terrain type " + type_name);
	if (int rc = TerrainFill(what, t, type, params40); rc != DTRL_OK) return rc;
	terrain_src_[t] = TerrainSource();
	return DTRL_OK;
}

int Engine::TerrainInfo(int t, char* type_out, int type_cap, double* params40_out, int* filled_out)
{
	const EnvAssignment& a = terrain_keys_;
	if (a.filled.empty()) return Fail(DTRL_ERR_ARG, std::string("dtrl_terrain_info: ") + a.none_text);
	if (t < 0 || t >= a.n_keys()) return Fail(DTRL_ERR_ARG, "dtrl_terrain_info: terrain " + std::to_string(t) + " out of range (0 .. " + std::to_string(a.n_keys() - 1) + ")");
	const TerrainCfg& c = terrain_table_[t];
	if (type_out && type_cap > 0) std::snprintf(type_out, static_cast<size_t>(type_cap), "%s", kTerrainTypeNames[c.type]);
	if (params40_out) std::memcpy(params40_out, c.params, sizeof(c.params));
	if (filled_out) *filled_out = a.filled[t] ? 1 : 0;
	return DTRL_OK;
}

// restart: the listed envs start over as at creation, under their new terrain -- the terrain stream from (terrain seed, GLOBAL env id), build count 0, a fresh
// two-segment window around the spawn point, then the device half of a reset. The exploration counter rng_ctr is not rewound (a reset never rewinds it).
int Engine::AssignTerrains(const int32_t* env_ids, int n, const int32_t* terrains, bool restart)
{
	const char* what = "dtrl_assign_terrains";
	if (int rc = KeysCurrent(terrain_keys_, what, ladder_on_); rc != DTRL_OK) return rc;   // (with a ladder on device terrain the upload below would otherwise overwrite every move the kernel made)
	if (int rc = KeysAssign(terrain_keys_, what, env_ids, n, terrains); rc != DTRL_OK) return rc;
	reset_ids_.clear();
	std::vector<char> seen(static_cast<size_t>(n_), 0);
	for (int i = 0; i < n; ++i) { const int e = EnvIndex(env_ids, i); if (!seen[e]) { seen[e] = 1; reset_ids_.push_back(e); } }   // (an env listed twice: its last terrain holds, it restarts once)
	if (ladder_on_) {
		// the listed envs' marks: the env's current root x, or -- restart -- the spawn point (host terrain here; device terrain: the mode-2 boundary launch below)
		for (int32_t e : reset_ids_) {
			if (restart) { if (!cfg_.device_terrain) tg_ladder_step(ladder_.host[e], terrain_keys_.env_key[e], status_[e], ladder_cfg_, 2, e); }
			else if (int rc = RootX(e, &ladder_.host[e].mark_x); rc != DTRL_OK) return rc;
		}
		if (int rc = DevOk(ladder_.Push(*be_)); rc != DTRL_OK) return rc;
	}
	if (!cfg_.device_terrain) {
		for (int32_t e : reset_ids_) {
			GroundWindow& g = grounds_[e];
			const TerrainCfg& c = terrain_table_[terrain_keys_.env_key[e]];
			g.SetTerrain(c.type, c.params);
			if (!restart) continue;
			g.SeedRand(static_cast<unsigned long>(cfg_.terrain_seed + static_cast<uint64_t>(cfg_.run.env_id_base) + e));
			g.Clear(); g.ResetBuilds();
			g.InitSegments(-kViewDist + kGroundSpawnOffset, kViewDist + kGroundSpawnOffset);
			if (!UploadGround(e)) return DTRL_ERR_CAPACITY;
		}
	}
	if (!restart || reset_ids_.empty()) return DTRL_OK;
	if (cfg_.device_terrain) {
		std::vector<GroundGen> gen(static_cast<size_t>(n_));
		if (!be_->D2H(gen.data(), buf_.gen, sizeof(GroundGen) * gen.size())) return Fail(DTRL_ERR_DEVICE, be_->error());
		for (int32_t e : reset_ids_) gen[e].key = terrain_stream_key(cfg_.terrain_seed, cfg_.run.env_id_base + e);
		if (!be_->H2D(buf_.gen, gen.data(), sizeof(GroundGen) * gen.size())) return Fail(DTRL_ERR_DEVICE, be_->error());
	}
	return StartEpisodes(reset_ids_, false, 2);   // the listed envs start over: a new push wait and a new episode record each; a restart draws no model
}

int Engine::GetTerrains(const int32_t* env_ids, int n, int32_t* terrains_out)
{
	if (int rc = KeysCurrent(terrain_keys_, "dtrl_get_terrains", ladder_on_); rc != DTRL_OK) return rc;   // with a ladder: the levels as of the last completed boundary
	return KeysGet(terrain_keys_, "dtrl_get_terrains", env_ids, n, terrains_out);
}

// ---- terrain ladder (include/dtrl.h: dtrl_terrain_ladder, dtrl_ladder_info) ----
// The rule is tg_ladder_step (dtrl_terrain_dev.h), run at every frame boundary in front of the env's terrain work: by HostFrameWork / Reset / AssignTerrains on
// the host (host terrain), inside the boundary launch (-terrain_gen= device, Backend::TerrainBoundary). dtrl_engine.h says who owns the key array when.
int Engine::RootX(int e, double* x)
{
	real q0 = 0;
	if (!be_->D2H(&q0, &buf_.st[e].q[0], sizeof(q0))) return Fail(DTRL_ERR_DEVICE, be_->error());
	*x = static_cast<double>(q0);
	return DTRL_OK;
}
int Engine::TerrainLadder(int lo, int hi, double up_dist, double down_dist, int at_top)
{
	const std::string w = "dtrl_terrain_ladder: ";
	if (int rc = KeysIdle(terrain_keys_, "dtrl_terrain_ladder", 0); rc != DTRL_OK) return rc;
	if (int rc = KeysRefresh(terrain_keys_); rc != DTRL_OK) return rc;   // (a ladder in place: the host keys are current again before it goes or is replaced)
	if (lo > hi) { ladder_on_ = terrain_keys_.on_device = false; return DTRL_OK; }   // the levels stay where they are
	const int T = terrain_keys_.n_keys();
	if (lo < 0 || hi >= T) return Fail(DTRL_ERR_ARG, w + "levels " + std::to_string(lo) + " .. " + std::to_string(hi) + " out of range (terrains 0 .. " + std::to_string(T - 1) + ")");
	for (int t = lo; t <= hi; ++t) if (!terrain_keys_.filled[t]) return Fail(DTRL_ERR_ARG, w + "terrain " + std::to_string(t) + " " + terrain_keys_.empty_text + ": every level of the ladder must be filled");
	if (!(up_dist > 0)) return Fail(DTRL_ERR_ARG, w + "up_dist must be > 0, not " + std::to_string(up_dist));
	if (!(down_dist >= 0)) return Fail(DTRL_ERR_ARG, w + "down_dist must be >= 0, not " + std::to_string(down_dist));
	if (at_top != 0 && at_top != 1) return Fail(DTRL_ERR_ARG, w + "at_top must be 0 or 1, not " + std::to_string(at_top));
	// one spawn x for the batch
	auto spawn_of = SpawnX;
	const double spawn_x = spawn_of(cfg_.model);
	for (size_t v = 0; v < var_models_.size(); ++v)
		if (spawn_of(var_models_[v]) != spawn_x) return Fail(DTRL_ERR_ARG, w + "model variant " + std::to_string(v) + " spawns at another root x (" + std::to_string(spawn_of(var_models_[v])) + ") than the batch's model (" + std::to_string(spawn_x) + "): the ladder keeps one spawn x per batch");
	if (cfg_.device_terrain) if (int rc = RecsAlloc(ladder_, static_cast<size_t>(n_)); rc != DTRL_OK) return rc;
	std::vector<LadderRec> rec(static_cast<size_t>(n_));
	for (int e = 0; e < n_; ++e) { rec[e].ups = 0; rec[e].downs = 0; if (int rc = RootX(e, &rec[e].mark_x); rc != DTRL_OK) return rc; }
	ladder_.host.swap(rec);
	ladder_cfg_ = LadderCfg{lo, hi, at_top, 0, up_dist, down_dist, spawn_x, cfg_.terrain_seed, static_cast<int64_t>(cfg_.run.env_id_base)};
	ladder_on_ = true;
	terrain_keys_.recs = &ladder_; terrain_keys_.on_device = cfg_.device_terrain; terrain_keys_.stale = false;
	return DevOk(ladder_.Push(*be_));
}

int Engine::LadderInfo(const int32_t* env_ids, int n, double* mark_x_out, int32_t* ups_out, int32_t* downs_out)
{
	const std::string w = "dtrl_ladder_info: ";
	if (terrain_keys_.filled.empty()) return Fail(DTRL_ERR_ARG, w + terrain_keys_.none_text);
	if (!ladder_on_) return Fail(DTRL_ERR_ARG, w + "the batch has no terrain ladder (call dtrl_terrain_ladder first)");
	if (int rc = RuleCallBegin("dtrl_ladder_info", &terrain_keys_, nullptr, {env_ids, n}, nullptr); rc != DTRL_OK) return rc;   // (this call refuses a missing rule in front of a frame in flight)
	for (int i = 0; i < n; ++i) {
		const LadderRec& r = ladder_.host[EnvIndex(env_ids, i)];
		if (mark_x_out) mark_x_out[i] = r.mark_x;
		if (ups_out) ups_out[i] = r.ups;
		if (downs_out) downs_out[i] = r.downs;
	}
	return DTRL_OK;
}

}  // namespace dtrl

#include "dtrl_backend_defaults.cpp"   // Backend's default implementations: part of this unit (see there)
