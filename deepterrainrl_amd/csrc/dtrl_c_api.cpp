// dtrl_c_api.cpp -- extern "C" surface declared in include/dtrl.h; thin wrappers over dtrl::Engine.
#include "../../include/dtrl.h"
#include "dtrl_engine.h"
#include <cmath>
#include <cstdio>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

using dtrl::Engine;
using dtrl::EnvState;
using dtrl::LogRow;

struct dtrl_batch { Engine eng; };

static thread_local std::string g_create_error;

// nothing may propagate across the C boundary (the reference's convention is bool + message, no exceptions): allocation failures and
// anything else thrown below the ABI become a status code and a message
static int dtrl_on_exception(const dtrl_batch* b)
{
	std::string msg = "internal error";
	int code = DTRL_ERR_DEVICE;
	try { throw; }
	catch (const std::bad_alloc&) { msg = "out of host memory"; code = DTRL_ERR_CAPACITY; }
	catch (const std::length_error& e) { msg = std::string("invalid size: ") + e.what(); code = DTRL_ERR_ARG; }
	catch (const std::exception& e) { msg = std::string("internal error: ") + e.what(); }
	catch (...) {}
	if (b) const_cast<dtrl_batch*>(b)->eng.set_error(msg); else g_create_error = msg;
	return code;
}

// The one place where anything thrown below the ABI is caught: f()'s value, or thrown()'s where f threw (called inside the handler: dtrl_on_exception rethrows)
template <class F, class T> static auto caught(F&& f, T&& thrown) -> decltype(f())
{
	try { return f(); } catch (...) { return thrown(); }
}
// a batch entry point: DTRL_ERR_ARG without a batch, else f(the batch's engine) as a status; a call without a batch: f(), the message going where dtrl_create's goes
template <class F> static dtrl_status guarded(const dtrl_batch* b, F&& f)
{
	if (!b) return DTRL_ERR_ARG;
	return caught([&] { return static_cast<dtrl_status>(f(const_cast<dtrl_batch*>(b)->eng)); }, [&] { return static_cast<dtrl_status>(dtrl_on_exception(b)); });
}
template <class F> static dtrl_status guarded_free(F&& f) { return caught([&] { return static_cast<dtrl_status>(f()); }, [] { return static_cast<dtrl_status>(dtrl_on_exception(nullptr)); }); }

extern "C" {

const char* dtrl_version(void) { return sizeof(dtrl::real) == 4 ? "dtrl-mi355x 0.6 (round 6), fp32 build (opt-in: -physics_precision= f32)" : "dtrl-mi355x 0.6 (round 6), fp64"; }

const char* dtrl_last_error(const dtrl_batch* b) { return b ? b->eng.error().c_str() : g_create_error.c_str(); }

dtrl_status dtrl_create(const char* const* argv, int argc, int num_envs, int device_id, dtrl_batch** out)
try {
	if (!out) return DTRL_ERR_ARG;
	*out = nullptr;
	dtrl_batch* b = new (std::nothrow) dtrl_batch();
	if (!b) return DTRL_ERR_DEVICE;
	int rc = b->eng.Create(argv, argc, num_envs, device_id);
	if (rc != DTRL_OK) { g_create_error = b->eng.error(); delete b; return static_cast<dtrl_status>(rc); }
	*out = b;
	return DTRL_OK;
} catch (...) { return static_cast<dtrl_status>(dtrl_on_exception(nullptr)); }
dtrl_status dtrl_destroy(dtrl_batch* b) { delete b; return DTRL_OK; }

dtrl_status dtrl_reset(dtrl_batch* b, const int32_t* env_ids, int n, const uint64_t* seeds) { return guarded(b, [&](Engine& eng) { return eng.Reset(env_ids, n, seeds); }); }
dtrl_status dtrl_step(dtrl_batch* b, double dt) { return guarded(b, [&](Engine& eng) { return eng.Step(dt); }); }
dtrl_status dtrl_step_begin(dtrl_batch* b, double dt) { return guarded(b, [&](Engine& eng) { return eng.StepBegin(dt); }); }
dtrl_status dtrl_step_end(dtrl_batch* b) { return guarded(b, [&](Engine& eng) { return eng.StepEnd(); }); }
dtrl_status dtrl_step_updates(dtrl_batch* b, int n) { return guarded(b, [&](Engine& eng) { return eng.StepUpdates(n); }); }
dtrl_status dtrl_run_frames(dtrl_batch* b, int frames, double dt) { return guarded(b, [&](Engine& eng) { return eng.RunFrames(frames, dt); }); }
dtrl_status dtrl_set_policy(dtrl_batch* b, const float* w, size_t n, const double* io, const double* is, const double* oo, const double* os) { return guarded(b, [&](Engine& eng) { return eng.SetPolicy(w, n, io, is, oo, os); }); }
dtrl_status dtrl_policy_num_params(const dtrl_batch* b, size_t* n)
{ return guarded(b, [&](Engine& eng) -> int {
	if (!eng.cfg().has_policy_net) { *n = 0; return DTRL_OK; }
	*n = static_cast<size_t>(eng.cfg().user_num_params); return DTRL_OK;
}); }
dtrl_status dtrl_build_output_offset_scale(const dtrl_batch* b, double* out_off, double* out_scale)
{ return guarded(b, [&](Engine& eng) -> int {
	if (!eng.cfg().has_policy_net) return DTRL_ERR_ARG;
	std::vector<double> off, sc;
	dtrl::BuildOutputOffsetScale(eng.cfg().model, eng.cfg().net, off, sc);
	for (size_t i = 0; i < off.size(); ++i) { out_off[i] = off[i]; out_scale[i] = sc[i]; }
	return DTRL_OK;
}); }
dtrl_status dtrl_load_scale_file(dtrl_batch* b, const char* path) { return guarded(b, [&](Engine& eng) { return eng.LoadScaleFile(path); }); }
dtrl_status dtrl_write_scale_file(dtrl_batch* b, const char* path) { return guarded(b, [&](Engine& eng) { return eng.WriteScaleFile(path); }); }
dtrl_status dtrl_set_explore(dtrl_batch* b, int enable, double rate, double temp, double base_rate) { return guarded(b, [&](Engine& eng) { return eng.SetExplore(enable, rate, temp, base_rate); }); }
dtrl_status dtrl_set_terrain_lerp(dtrl_batch* b, double lerp) { return guarded(b, [&](Engine& eng) { return eng.SetTerrainLerp(lerp); }); }
dtrl_status dtrl_drain_tuples(dtrl_batch* b, float* rows, uint32_t* flags, int32_t* env_ids, int cap, int* out_n) { return guarded(b, [&](Engine& eng) { return eng.DrainTuples(rows, flags, env_ids, cap, out_n); }); }

dtrl_status dtrl_get_pose_vel(dtrl_batch* b, const int32_t* env_ids, int n, double* q, double* qd)
{ return guarded(b, [&](Engine& eng) -> int {
	std::vector<EnvState> st; int rc = eng.GetStates(env_ids, n, st);
	if (rc != DTRL_OK) return rc;
	const int D = eng.cfg().model.D;
	for (int i = 0; i < n; ++i) for (int k = 0; k < D; ++k) { if (q) q[i * D + k] = st[i].q[k]; if (qd) qd[i * D + k] = st[i].qd[k]; }
	return DTRL_OK;
}); }
void* dtrl_side_stream(dtrl_batch* b, int k, double* start_delay_us) { return caught([&]() -> void* { return b ? b->eng.SideStream(k, start_delay_us) : nullptr; }, []() -> void* { return nullptr; }); }
dtrl_status dtrl_command_action(dtrl_batch* b, const int32_t* env_ids, int n, const int32_t* action_ids) { return guarded(b, [&](Engine& eng) { return eng.CommandAction(env_ids, n, action_ids); }); }
dtrl_status dtrl_set_pose_vel(dtrl_batch* b, const int32_t* env_ids, int n, const double* q, const double* qd) { return guarded(b, [&](Engine& eng) { return eng.SetPoseVel(env_ids, n, q, qd); }); }
dtrl_status dtrl_get_contact_cache(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* count, int32_t* ids, double* lambda) { return guarded(b, [&](Engine& eng) { return eng.GetContactCache(env_ids, n, count, ids, lambda); }); }
dtrl_status dtrl_set_contact_cache(dtrl_batch* b, const int32_t* env_ids, int n, const int32_t* count, const int32_t* ids, const double* lambda) { return guarded(b, [&](Engine& eng) { return eng.SetContactCache(env_ids, n, count, ids, lambda); }); }
dtrl_status dtrl_add_perturb(dtrl_batch* b, const int32_t* env_ids, int n, const int32_t* link, const double* local_pos, const double* force, const double* duration)
{ return guarded(b, [&](Engine& eng) -> int {
	if (!link || !force || !duration) { eng.set_error("dtrl_add_perturb: link, force and duration are required"); return DTRL_ERR_ARG; }
	return eng.AddPerturb(env_ids, n, link, local_pos, force, duration);
}); }
dtrl_status dtrl_apply_rand_force(dtrl_batch* b, const int32_t* env_ids, int n, uint64_t seed) { return guarded(b, [&](Engine& eng) { return eng.ApplyRandForce(env_ids, n, seed); }); }
dtrl_status dtrl_get_policy_output(dtrl_batch* b, const int32_t* env_ids, int n, double* y) { return guarded(b, [&](Engine& eng) { return eng.GetPolicyOutput(env_ids, n, y); }); }
dtrl_status dtrl_get_poli_state(dtrl_batch* b, const int32_t* env_ids, int n, double* s) { return guarded(b, [&](Engine& eng) { return eng.GetPoliState(env_ids, n, s); }); }

dtrl_status dtrl_get_flags(dtrl_batch* b, const int32_t* env_ids, int n, uint32_t* bits)
{ return guarded(b, [&](Engine& eng) -> int {
	std::vector<EnvState> st; int rc = eng.GetStates(env_ids, n, st);
	if (rc != DTRL_OK) return rc;
	const int L = eng.cfg().model.L;
	for (int i = 0; i < n; ++i) {
		const EnvState& s = st[i];
		bool flipped = std::fabs(dtrl::wrap_pi(s.q[2])) > 3.14159265358979323846 * 0.8;
		bool fallen = s.sum_fall_contact > 0.25 || s.fail_fall_dist != 0 || flipped;
		uint32_t stumble_mask = (eng.cfg().model.char_type == 1)
			? ~((1u << dtrl::rRightToe) | (1u << dtrl::rLeftToe) | (1u << dtrl::rRightAnkle) | (1u << dtrl::rLeftAnkle))
			: ~((1u << dtrl::jToe) | (1u << dtrl::jFinger) | (1u << dtrl::jAnkle) | (1u << dtrl::jWrist));
		bool stumbled = (s.contact_bits & stumble_mask & ((1u << L) - 1u)) != 0;
		bool new_cycle = s.state == 0 && s.phase == 0;
		bits[i] = (fallen ? DTRL_FLAG_FALLEN : 0u) | (stumbled ? DTRL_FLAG_STUMBLED : 0u) | (new_cycle ? DTRL_FLAG_NEW_CYCLE : 0u) | (static_cast<uint32_t>(s.state) << DTRL_FLAG_STATE_SHIFT);
	}
	return DTRL_OK;
}); }
dtrl_status dtrl_get_torques(dtrl_batch* b, const int32_t* env_ids, int n, double* tau_ctrl, double* tau_applied)
{ return guarded(b, [&](Engine& eng) -> int {
	std::vector<EnvState> st; int rc = eng.GetStates(env_ids, n, st);
	if (rc != DTRL_OK) return rc;
	const int D = eng.cfg().model.D;
	for (int i = 0; i < n; ++i) for (int k = 0; k < D; ++k) { if (tau_ctrl) tau_ctrl[i * D + k] = st[i].tau_ctrl[k]; if (tau_applied) tau_applied[i * D + k] = st[i].tau[k]; }
	return DTRL_OK;
}); }
dtrl_status dtrl_get_link_states(dtrl_batch* b, const int32_t* env_ids, int n, double* com_xy, double* com_vel_xy, double* angle)
{ return guarded(b, [&](Engine& eng) -> int {
	std::vector<EnvState> st; int rc = eng.GetStates(env_ids, n, st);
	if (rc == DTRL_OK) rc = eng.VariantKeysCurrent();   // (a variant redraw on device terrain: the keys ModelOf reads are the device's; GetStates has waited for the streams)
	if (rc != DTRL_OK) return rc;
	const int L = eng.cfg().model.L;
	for (int e = 0; e < n; ++e) {
		const EnvState& s = st[e];
		const dtrl::DevModel& m = eng.ModelOf(env_ids ? env_ids[e] : e);   // attach points and body angles are the env's variant's (GetStates has checked the ids)
		double phi[dtrl::kMaxL], w[dtrl::kMaxL], px[dtrl::kMaxL], py[dtrl::kMaxL], vx[dtrl::kMaxL], vy[dtrl::kMaxL];
		for (int j = 0; j < L; ++j) {   // parents precede children (cKinTree joint order)
			const int pa = m.parent[j];
			if (pa < 0) { phi[j] = s.q[2]; w[j] = s.qd[2]; px[j] = s.q[0]; py[j] = s.q[1]; vx[j] = s.qd[0]; vy[j] = s.qd[1]; }
			else {
				const double c = std::cos(phi[pa]), sn = std::sin(phi[pa]);
				const double rx = c * m.attach[j][0] - sn * m.attach[j][1], ry = sn * m.attach[j][0] + c * m.attach[j][1];
				phi[j] = phi[pa] + s.q[j + 2]; w[j] = w[pa] + s.qd[j + 2];
				px[j] = px[pa] + rx; py[j] = py[pa] + ry;
				vx[j] = vx[pa] - w[pa] * ry; vy[j] = vy[pa] + w[pa] * rx;
			}
			const double c = std::cos(phi[j]), sn = std::sin(phi[j]);
			const double bx = c * m.body_attach[j][0] - sn * m.body_attach[j][1], by = sn * m.body_attach[j][0] + c * m.body_attach[j][1];
			const size_t o = static_cast<size_t>(e) * L + j;
			if (com_xy) { com_xy[2 * o] = px[j] + bx; com_xy[2 * o + 1] = py[j] + by; }
			if (com_vel_xy) { com_vel_xy[2 * o] = vx[j] - w[j] * by; com_vel_xy[2 * o + 1] = vy[j] + w[j] * bx; }
			if (angle) angle[o] = phi[j] + m.body_theta[j];
		}
	}
	return DTRL_OK;
}); }
dtrl_status dtrl_get_contacts(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* flags)
{ return guarded(b, [&](Engine& eng) -> int {
	std::vector<EnvState> st; int rc = eng.GetStates(env_ids, n, st);
	if (rc != DTRL_OK) return rc;
	const int L = eng.cfg().model.L;
	for (int i = 0; i < n; ++i) for (int j = 0; j < L; ++j) flags[i * L + j] = (st[i].contact_bits >> j) & 1u;
	return DTRL_OK;
}); }
dtrl_status dtrl_get_ctrl(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* state, double* phase, int32_t* action_id, double* params, double* pd_targets)
{ return guarded(b, [&](Engine& eng) -> int {
	std::vector<EnvState> st; int rc = eng.GetStates(env_ids, n, st);
	if (rc != DTRL_OK) return rc;
	const int L = eng.cfg().model.L, P = eng.cfg().model.P;
	for (int i = 0; i < n; ++i) {
		if (state) state[i] = st[i].state;
		if (phase) phase[i] = st[i].phase;
		if (action_id) action_id[i] = st[i].action_id;
		if (params) for (int k = 0; k < P; ++k) params[i * P + k] = st[i].params[k];
		if (pd_targets) for (int j = 0; j < L; ++j) pd_targets[i * L + j] = st[i].pd_target[j];
	}
	return DTRL_OK;
}); }
dtrl_status dtrl_get_cycle_info(dtrl_batch* b, const int32_t* env_ids, int n, int64_t* num_cycles, int64_t* num_resets, double* cycle_start_com, double* cycle_start_time, double* opt_params)
{ return guarded(b, [&](Engine& eng) -> int {
	std::vector<EnvState> st; int rc = eng.GetStates(env_ids, n, st);
	if (rc != DTRL_OK) return rc;
	const dtrl::DevModel& m = eng.cfg().model;
	for (int i = 0; i < n; ++i) {
		if (num_cycles) num_cycles[i] = st[i].num_cycles;
		if (num_resets) num_resets[i] = st[i].num_resets;
		if (cycle_start_com) { cycle_start_com[2 * i] = st[i].prev_com[0]; cycle_start_com[2 * i + 1] = st[i].prev_com[1]; }
		if (cycle_start_time) cycle_start_time[i] = st[i].time - st[i].curr_cycle_time;
		if (opt_params) for (int k = 0; k < m.n_opt; ++k) opt_params[static_cast<size_t>(i) * m.n_opt + k] = st[i].params[m.opt_index[k]];
	}
	return DTRL_OK;
}); }
dtrl_status dtrl_get_action_table(dtrl_batch* b, int* n_actions, double* table)
{ return guarded(b, [&](Engine& eng) -> int {
	const dtrl::DevModel& m = eng.cfg().model;
	if (n_actions) *n_actions = m.n_actions;
	if (table) for (int a = 0; a < m.n_actions; ++a) {
		const dtrl::real* p0 = m.ctrl_params[m.act_idx0[a]]; const dtrl::real* p1 = m.ctrl_params[m.act_idx1[a]]; const double bl = m.act_blend[a];
		for (int k = 0; k < m.n_opt; ++k) { const int i = m.opt_index[k]; table[static_cast<size_t>(a) * m.n_opt + k] = (1 - bl) * p0[i] + bl * p1[i]; }
	}
	return DTRL_OK;
}); }
dtrl_status dtrl_sample_ground(dtrl_batch* b, int env, int n, const double* x, double* h, int32_t* seg, int32_t* i, int32_t* j) { return guarded(b, [&](Engine& eng) { return eng.SampleGround(env, n, x, h, seg, i, j); }); }
dtrl_status dtrl_step_end_begin(dtrl_batch* b, double dt) { return guarded(b, [&](Engine& eng) { return eng.StepEndBegin(dt); }); }
dtrl_status dtrl_step_poll(dtrl_batch* b, double dt, int* relaunched) { return guarded(b, [&](Engine& eng) { return eng.StepPoll(dt, relaunched); }); }
dtrl_status dtrl_set_tuple_pipelining(dtrl_batch* b, int on) { return guarded(b, [&](Engine& eng) { return eng.SetTuplePipelining(on != 0); }); }
dtrl_status dtrl_drain_tuples_packed(dtrl_batch* b, float* block_dev, int block_rows, int* out_n) { return guarded(b, [&](Engine& eng) { return eng.DrainTuplesPacked(block_dev, block_rows, out_n); }); }
dtrl_status dtrl_get_ground_window(dtrl_batch* b, int env, int32_t* w2, double* min_x2, double* max_x2, float* heights0, float* heights1, int cap, int64_t* num_builds) { return guarded(b, [&](Engine& eng) { return eng.GroundWindowRec(env, w2, min_x2, max_x2, heights0, heights1, cap, num_builds); }); }
dtrl_status dtrl_eval_stats(dtrl_batch* b, double* avg_dist, int64_t* episodes, int64_t* cycles, int64_t* resets) { return guarded(b, [&](Engine& eng) { return eng.EvalStats(avg_dist, episodes, cycles, resets); }); }
dtrl_status dtrl_dims(const dtrl_batch* b, int* L, int* D, int* S, int* A, int* P, int* nn_out, int* num_frags, int* frag_size)
{ return guarded(b, [&](Engine& eng) -> int {
	const dtrl::ScenarioConfig& c = eng.cfg();
	if (L) *L = c.model.L;
	if (D) *D = c.model.D;
	if (S) *S = eng.S();
	if (A) *A = eng.A();
	if (P) *P = c.model.P;
	if (nn_out) *nn_out = c.has_policy_net ? c.user_out_size : 0;
	if (num_frags) *num_frags = (c.has_policy_net && !c.actor_only) ? c.net.n_frags : 0;
	if (frag_size) *frag_size = c.model.n_opt;
	return DTRL_OK;
}); }
// ---- external policy mode ----
dtrl_status dtrl_pending_actions(dtrl_batch* b, int32_t* env_ids, double* states, int cap, int* out_n) { return guarded(b, [&](Engine& eng) { return eng.PendingActions(env_ids, states, cap, out_n, false); }); }
dtrl_status dtrl_pending_actions_device(dtrl_batch* b, int32_t* env_ids_dev, float* states_dev, int cap, int* out_n) { return guarded(b, [&](Engine& eng) { return eng.PendingActions(env_ids_dev, states_dev, cap, out_n, true); }); }
dtrl_status dtrl_supply_actions(dtrl_batch* b, const int32_t* env_ids, int n, const int32_t* action_ids, const double* params, const uint32_t* flags) { return guarded(b, [&](Engine& eng) { return eng.SupplyActions(env_ids, n, action_ids, params, flags, false, nullptr); }); }
dtrl_status dtrl_supply_actions_device(dtrl_batch* b, const int32_t* env_ids_dev, int n, const int32_t* action_ids_dev, const float* params_dev, const uint32_t* flags_dev, int* rejected) { return guarded(b, [&](Engine& eng) { return eng.SupplyActions(env_ids_dev, n, action_ids_dev, params_dev, flags_dev, true, rejected); }); }
dtrl_status dtrl_ext_stats(dtrl_batch* b, int64_t* awaiting, int64_t* ready, int64_t* env_steps_total, int64_t* env_frames_total) { return guarded(b, [&](Engine& eng) { return eng.ExtStats(awaiting, ready, env_steps_total, env_frames_total); }); }
dtrl_status dtrl_ext_env_info(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* park, int32_t* steps_left) { return guarded(b, [&](Engine& eng) { return eng.ExtEnvInfo(env_ids, n, park, steps_left); }); }
// policy slots
dtrl_status dtrl_slots_create(dtrl_batch* b, int n_slots) { return guarded(b, [&](Engine& eng) { return eng.SlotsCreate(n_slots); }); }
dtrl_status dtrl_slot_set_policy(dtrl_batch* b, int slot, const float* weights, size_t n, const double* in_off, const double* in_scale, const double* out_off, const double* out_scale) { return guarded(b, [&](Engine& eng) { return eng.SlotSetPolicy(slot, weights, n, in_off, in_scale, out_off, out_scale, false); }); }
dtrl_status dtrl_slot_set_policy_device(dtrl_batch* b, int slot, const float* weights_dev, size_t n, const double* in_off_dev, const double* in_scale_dev, const double* out_off_dev, const double* out_scale_dev) { return guarded(b, [&](Engine& eng) { return eng.SlotSetPolicy(slot, weights_dev, n, in_off_dev, in_scale_dev, out_off_dev, out_scale_dev, true); }); }
dtrl_status dtrl_slot_alias(dtrl_batch* b, int slot, int src_slot) { return guarded(b, [&](Engine& eng) { return eng.SlotAlias(slot, src_slot); }); }
dtrl_status dtrl_slot_set_explore(dtrl_batch* b, int slot, int enable, double rate, double temp, double base_rate) { return guarded(b, [&](Engine& eng) { return eng.SlotSetExplore(slot, enable, rate, temp, base_rate); }); }
dtrl_status dtrl_assign_slots(dtrl_batch* b, const int32_t* env_ids, int n, const int32_t* slots) { return guarded(b, [&](Engine& eng) { return eng.AssignSlots(env_ids, n, slots); }); }
dtrl_status dtrl_get_slots(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* slots_out) { return guarded(b, [&](Engine& eng) { return eng.GetSlots(env_ids, n, slots_out); }); }
dtrl_status dtrl_slot_stats(dtrl_batch* b, int slot, int64_t* n_envs, double* avg_dist, int64_t* episodes, int64_t* cycles, int64_t* resets) { return guarded(b, [&](Engine& eng) { return eng.SlotStats(slot, n_envs, avg_dist, episodes, cycles, resets); }); }
// model variants
dtrl_status dtrl_variants_create(dtrl_batch* b, int n_variants) { return guarded(b, [&](Engine& eng) { return eng.VariantsCreate(n_variants); }); }
dtrl_status dtrl_variant_load_file(dtrl_batch* b, int v, const char* character_file) { return guarded(b, [&](Engine& eng) { return eng.VariantLoad(v, character_file, nullptr, 0); }); }
dtrl_status dtrl_variant_load_json(dtrl_batch* b, int v, const char* text, size_t bytes)
{ return guarded(b, [&](Engine& eng) -> int {
	if (!text) { eng.set_error("dtrl_variant_load_json: text is required"); return DTRL_ERR_ARG; }
	return eng.VariantLoad(v, nullptr, text, bytes);
}); }
dtrl_status dtrl_assign_variants(dtrl_batch* b, const int32_t* env_ids, int n, const int32_t* variants) { return guarded(b, [&](Engine& eng) { return eng.AssignVariants(env_ids, n, variants); }); }
dtrl_status dtrl_get_variants(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* variants_out) { return guarded(b, [&](Engine& eng) { return eng.GetVariants(env_ids, n, variants_out); }); }
dtrl_status dtrl_variant_redraw(dtrl_batch* b, int lo, int hi, uint64_t seed, const double* weights) { return guarded(b, [&](Engine& eng) { return eng.VariantRedraw(lo, hi, seed, weights); }); }
dtrl_status dtrl_variant_redraw_info(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* lo, int32_t* hi, int32_t* variant, int32_t* draws) { return guarded(b, [&](Engine& eng) { return eng.VariantRedrawInfo(env_ids, n, lo, hi, variant, draws); }); }
dtrl_status dtrl_variant_rescale(dtrl_batch* b, int base, const int32_t* env_ids, int n, uint64_t seed, const dtrl_rescale_desc* d)
{ return guarded(b, [&](Engine& eng) -> int {
	if (!d) return eng.VariantRescale(base, env_ids, n, seed, nullptr, nullptr, 0, true);
	const double lo[4] = {d->mass[0], d->kp[0], d->kd[0], d->torque_lim[0]}, hi[4] = {d->mass[1], d->kp[1], d->kd[1], d->torque_lim[1]};
	return eng.VariantRescale(base, env_ids, n, seed, lo, hi, d->per_link, false);
}); }
dtrl_status dtrl_variant_rescale_info(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* base, uint64_t* seed, dtrl_rescale_desc* d, int32_t* key, int32_t* episodes, double* factors)
{ return guarded(b, [&](Engine& eng) -> int {
	double lo[4], hi[4]; uint32_t per_link = 0;
	const int rc = eng.VariantRescaleInfo(env_ids, n, base, seed, lo, hi, &per_link, key, episodes, factors);
	if (rc == DTRL_OK && d) { double* const r[4] = {d->mass, d->kp, d->kd, d->torque_lim}; for (int q = 0; q < 4; ++q) { r[q][0] = lo[q]; r[q][1] = hi[q]; } d->per_link = per_link; d->reserved = 0; }
	return rc;
}); }
dtrl_status dtrl_variant_scalars(dtrl_batch* b, int env, double* out, double* total_mass) { return guarded(b, [&](Engine& eng) { return eng.VariantScalars(env, out, total_mass); }); }
dtrl_status dtrl_variant_stats(dtrl_batch* b, int v, int64_t* n_envs, double* avg_dist, int64_t* episodes, int64_t* cycles, int64_t* resets) { return guarded(b, [&](Engine& eng) { return eng.VariantStats(v, n_envs, avg_dist, episodes, cycles, resets); }); }
// push schedule
dtrl_status dtrl_push_schedule(dtrl_batch* b, int min_wait, int max_wait, uint64_t seed, double min_force, double max_force, double min_dur, double max_dur) { return guarded(b, [&](Engine& eng) { return eng.PushSchedule(min_wait, max_wait, seed, min_force, max_force, min_dur, max_dur); }); }
dtrl_status dtrl_push_scale(dtrl_batch* b, const int32_t* env_ids, int n, const double* scales) { return guarded(b, [&](Engine& eng) { return eng.PushScale(env_ids, n, scales); }); }
dtrl_status dtrl_push_info(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* wait, int32_t* pushes, int32_t* last_link, double* last_force, double* last_dur) { return guarded(b, [&](Engine& eng) { return eng.PushInfo(env_ids, n, wait, pushes, last_link, last_force, last_dur); }); }
// episode limit
dtrl_status dtrl_episode_limit(dtrl_batch* b, int min_frames, int max_frames, double max_dist, uint64_t seed) { return guarded(b, [&](Engine& eng) { return eng.EpisodeLimit(min_frames, max_frames, max_dist, seed); }); }
dtrl_status dtrl_episode_limit_envs(dtrl_batch* b, const int32_t* env_ids, int n, const uint8_t* on) { return guarded(b, [&](Engine& eng) { return eng.EpisodeLimitEnvs(env_ids, n, on); }); }
dtrl_status dtrl_episode_info(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* frames, int32_t* limit, int64_t* by_fall, int64_t* by_limit, int32_t* last_frames, double* last_dist, int32_t* last_cause) { return guarded(b, [&](Engine& eng) { return eng.EpisodeInfo(env_ids, n, frames, limit, by_fall, by_limit, last_frames, last_dist, last_cause); }); }
// frame trace
dtrl_status dtrl_trace(dtrl_batch* b, const int32_t* env_ids, int n, int frames) { return guarded(b, [&](Engine& eng) { return eng.Trace(env_ids, n, frames); }); }
dtrl_status dtrl_trace_info(dtrl_batch* b, int32_t* n_traced, int32_t* frames, int32_t* width, int32_t* env_ids_out, int64_t* rows_written_out) { return guarded(b, [&](Engine& eng) { return eng.TraceInfo(n_traced, frames, width, env_ids_out, rows_written_out); }); }
dtrl_status dtrl_trace_read(dtrl_batch* b, const int32_t* env_ids, int n, int max_rows, double* vals, int32_t* ints, int32_t* counts) { return guarded(b, [&](Engine& eng) { return eng.TraceRead(env_ids, n, max_rows, vals, ints, counts, false); }); }
dtrl_status dtrl_trace_read_device(dtrl_batch* b, const int32_t* env_ids, int n, int max_rows, double* vals_dev, int32_t* ints_dev, int32_t* counts) { return guarded(b, [&](Engine& eng) { return eng.TraceRead(env_ids, n, max_rows, vals_dev, ints_dev, counts, true); }); }
// episode log (the row of the header is the rule's LogRow, field for field)
static_assert(sizeof(dtrl_episode_row) == sizeof(LogRow) && offsetof(dtrl_episode_row, boundary) == offsetof(LogRow, boundary) && offsetof(dtrl_episode_row, dist) == offsetof(LogRow, dist)
	&& offsetof(dtrl_episode_row, need_reset) == offsetof(LogRow, need_reset) && offsetof(dtrl_episode_row, slot) == offsetof(LogRow, slot) && offsetof(dtrl_episode_row, rescale_draw) == offsetof(LogRow, rescale_draw),
	"dtrl_episode_row is LogRow");
dtrl_status dtrl_episode_log(dtrl_batch* b, int32_t capacity) { return guarded(b, [&](Engine& eng) { return eng.EpisodeLog(capacity); }); }
dtrl_status dtrl_episode_log_info(dtrl_batch* b, int32_t* capacity, int32_t* n_groups, int64_t* written, int64_t* lost) { return guarded(b, [&](Engine& eng) { return eng.EpisodeLogInfo(capacity, n_groups, written, lost); }); }
dtrl_status dtrl_episode_log_drain(dtrl_batch* b, dtrl_episode_row* out, int32_t max_rows, int32_t* n, int64_t* lost) { return guarded(b, [&](Engine& eng) { return eng.EpisodeLogDrain(out, max_rows, n, lost); }); }
dtrl_status dtrl_variant_rescale_factors(dtrl_batch* b, const int32_t* env_ids, const int32_t* draws, int32_t n, double* factors) { return guarded(b, [&](Engine& eng) { return eng.VariantRescaleFactors(env_ids, draws, n, factors); }); }
// terrain sets
dtrl_status dtrl_terrains_create(dtrl_batch* b, int n_terrains) { return guarded(b, [&](Engine& eng) { return eng.TerrainsCreate(n_terrains); }); }
dtrl_status dtrl_terrain_set_file(dtrl_batch* b, int t, const char* terrain_file, double lerp) { return guarded(b, [&](Engine& eng) { return eng.TerrainSetFile(t, terrain_file, lerp); }); }
dtrl_status dtrl_terrain_set_params(dtrl_batch* b, int t, const char* type_name, const double* params40) { return guarded(b, [&](Engine& eng) { return eng.TerrainSetParams(t, type_name, params40); }); }
dtrl_status dtrl_terrain_info(dtrl_batch* b, int t, char* type_out, int type_cap, double* params40_out, int* filled_out) { return guarded(b, [&](Engine& eng) { return eng.TerrainInfo(t, type_out, type_cap, params40_out, filled_out); }); }
dtrl_status dtrl_assign_terrains(dtrl_batch* b, const int32_t* env_ids, int n, const int32_t* terrains, int restart) { return guarded(b, [&](Engine& eng) { return eng.AssignTerrains(env_ids, n, terrains, restart != 0); }); }
dtrl_status dtrl_get_terrains(dtrl_batch* b, const int32_t* env_ids, int n, int32_t* terrains_out) { return guarded(b, [&](Engine& eng) { return eng.GetTerrains(env_ids, n, terrains_out); }); }
dtrl_status dtrl_terrain_stats(dtrl_batch* b, int t, int64_t* n_envs, double* avg_dist, int64_t* episodes, int64_t* cycles, int64_t* resets) { return guarded(b, [&](Engine& eng) { return eng.TerrainStats(t, n_envs, avg_dist, episodes, cycles, resets); }); }
dtrl_status dtrl_terrain_ladder(dtrl_batch* b, int lo, int hi, double up_dist, double down_dist, int at_top) { return guarded(b, [&](Engine& eng) { return eng.TerrainLadder(lo, hi, up_dist, down_dist, at_top); }); }
dtrl_status dtrl_ladder_info(dtrl_batch* b, const int32_t* env_ids, int n, double* mark_x_out, int32_t* ups_out, int32_t* downs_out) { return guarded(b, [&](Engine& eng) { return eng.LadderInfo(env_ids, n, mark_x_out, ups_out, downs_out); }); }
dtrl_status dtrl_action_dims(const dtrl_batch* b, int* n_opt, int* n_labels, int* num_update_steps, int* external)
{ return guarded(b, [&](Engine& eng) -> int {
	const dtrl::ScenarioConfig& c = eng.cfg();
	if (n_opt) *n_opt = c.model.n_opt;
	if (n_labels) *n_labels = c.model.n_actions > 1 ? c.model.n_actions : 1;
	if (num_update_steps) *num_update_steps = c.model.num_update_steps;
	if (external) *external = c.external_policy ? 1 : 0;
	return DTRL_OK;
}); }
double dtrl_ext_launch_ms(dtrl_batch* b, int which) { return caught([&] { return b ? b->eng.ExtLaunchMs(which) : -1.0; }, [] { return -1.0; }); }
dtrl_status dtrl_kernel_time_ms(dtrl_batch* b, double* avg_ms, int64_t* launches) { return guarded(b, [&](Engine& eng) { return eng.KernelTime(avg_ms, launches); }); }

dtrl_status dtrl_drain_tuples_device(dtrl_batch* b, float* rows_dev, uint32_t* flags_dev, int32_t* env_ids_dev, int cap, int* out_n) { return guarded(b, [&](Engine& eng) { return eng.DrainTuples(rows_dev, flags_dev, env_ids_dev, cap, out_n, true); }); }
dtrl_status dtrl_tuple_stats(dtrl_batch* b, int64_t* pending, int64_t* drained, int64_t* dropped, int32_t* capacity) { return guarded(b, [&](Engine& eng) { return eng.TupleStats(pending, drained, dropped, capacity); }); }
dtrl_status dtrl_set_policy_device(dtrl_batch* b, const float* w_dev, size_t n, const double* io_dev, const double* is_dev, const double* oo_dev, const double* os_dev) { return guarded(b, [&](Engine& eng) { return eng.SetPolicyDevice(w_dev, n, io_dev, is_dev, oo_dev, os_dev); }); }
dtrl_status dtrl_set_policy_device_on(dtrl_batch* b, const float* w_dev, size_t n, void* stream) { return guarded(b, [&](Engine& eng) { return eng.SetPolicyDevice(w_dev, n, nullptr, nullptr, nullptr, nullptr, stream); }); }
dtrl_status dtrl_set_policy_device_async(dtrl_batch* b, const float* w_dev, size_t n, void* stream) { return guarded(b, [&](Engine& eng) { return eng.SetPolicyDeviceAsync(w_dev, n, stream); }); }
dtrl_status dtrl_get_dist_log(dtrl_batch* b, double* dist, int32_t* env_ids, int cap, int* out_n) { return guarded(b, [&](Engine& eng) { return eng.GetDistLog(dist, env_ids, cap, out_n); }); }
dtrl_status dtrl_reset_avg_dist(dtrl_batch* b) { return guarded(b, [&](Engine& eng) { return eng.ResetAvgDist(); }); }
// cOptScenarioPoliEval::OutputResults (optimizer/scenarios/OptScenarioPoliEval.cpp:213-239): one line appended to `path`, the distances of every
// recorded episode pool member by pool member, std::to_string formatting, ", " separated
dtrl_status dtrl_write_dist_log(dtrl_batch* b, const char* path)
{ return guarded(b, [&](Engine& eng) -> int {
	if (!path) { eng.set_error("null path"); return DTRL_ERR_ARG; }
	int n = 0;
	int rc = eng.GetDistLog(nullptr, nullptr, 0, &n);
	if (rc != DTRL_OK) return rc;
	std::vector<double> d(static_cast<size_t>(n));
	rc = eng.GetDistLog(d.data(), nullptr, n, &n);
	if (rc != DTRL_OK) return rc;
	std::string str;
	for (int i = 0; i < n; ++i) { if (!str.empty()) str += ", "; str += std::to_string(d[i]); }
	str += "\n";
	FILE* f = std::fopen(path, "a");   // cFileUtil::AppendText
	if (!f) { eng.set_error(std::string("Failed to output results to ") + path); return DTRL_ERR_IO; }
	std::fputs(str.c_str(), f); std::fclose(f);
	return DTRL_OK;
}); }

dtrl_status dtrl_terrain_build(const char* type_name, const double* params40, uint64_t seed, double width, float* out, int cap, int* out_n, double* out_width)
{ return guarded_free([&]() -> int {
	if (!type_name || !params40 || !out_n || cap < 0 || (cap > 0 && !out)) return DTRL_ERR_ARG;
	std::string name = type_name;
	if (name.empty()) name = "flat";   // cTerrainGen2D::ParseType: "" == flat
	int type = -1;
	for (int i = 0; i < dtrl::kTerrTypeMax; ++i) if (name == dtrl::kTerrainTypeNames[i]) type = i;
	if (type < 0) { g_create_error = "unsupported terrain type " + name; return DTRL_ERR_ARG; }
	dtrl::TerrainRand rnd; rnd.Seed(static_cast<unsigned long>(seed));
	std::vector<float> data;
	const double w = dtrl::BuildTerrain(type, width, params40, rnd, data);
	*out_n = static_cast<int>(data.size());
	if (out_width) *out_width = w;
	for (int i = 0; i < *out_n && i < cap; ++i) out[i] = data[i];
	return *out_n <= cap ? DTRL_OK : DTRL_ERR_CAPACITY;
}); }
dtrl_status dtrl_terrain_load_file(const char* path, char* type_out, int type_cap, double* params_out, int max_sets, int* out_sets)
{ return guarded_free([&]() -> int {
	if (!path || !out_sets || max_sets < 0 || (max_sets > 0 && !params_out)) return DTRL_ERR_ARG;
	dtrl::Json tf; std::string err;
	if (!dtrl::Json::parse_file(path, tf, err)) { g_create_error = err; return DTRL_ERR_IO; }
	const dtrl::Json* ty = tf.find("Type");
	const std::string tname = ty ? ty->str : "";
	if (type_out && type_cap > 0) { std::snprintf(type_out, static_cast<size_t>(type_cap), "%s", tname.c_str()); }
	int n = 0;
	const dtrl::Json* ps = tf.find("Params");
	if (ps) for (const dtrl::Json& obj : ps->arr) {
		if (n >= max_sets) break;
		for (int k = 0; k < dtrl::kNumTerrainParams; ++k) params_out[n * dtrl::kNumTerrainParams + k] = obj.get_num(dtrl::kTerrainParamNames[k], dtrl::kTerrainParamDefaults[k]);
		++n;
	}
	*out_sets = n;
	return DTRL_OK;
}); }
dtrl_status dtrl_args_parse_string(const char* const* argv, int argc, const char* key, char* out, int cap, int* found, int* n_tokens)
{ return guarded_free([&]() -> int {
	if (!key || !found || argc < 0 || (argc > 0 && !argv)) return DTRL_ERR_ARG;
	dtrl::ArgParser args(argv, argc);
	std::string arg_file;
	if (args.ParseString("arg_file", arg_file)) {
		std::string root; args.ParseString("data_root", root);
		const std::string path = (arg_file.empty() || arg_file[0] == '/' || root.empty()) ? arg_file : root + "/" + arg_file;
		if (!args.AppendArgs(path)) { g_create_error = "Failed to load args from: " + path; return DTRL_ERR_IO; }
	}
	std::string v;
	*found = args.ParseString(key, v) ? 1 : 0;
	if (out && cap > 0) std::snprintf(out, static_cast<size_t>(cap), "%s", *found ? v.c_str() : "");
	if (n_tokens) *n_tokens = args.GetNumArgs();
	return DTRL_OK;
}); }

// ---- env snapshots (the handle is a dtrl::Snapshot; its payload lives with the batch that saved or imported it) ----
static dtrl::Snapshot* snap_of(const dtrl_snapshot* s) { return reinterpret_cast<dtrl::Snapshot*>(const_cast<dtrl_snapshot*>(s)); }
dtrl_status dtrl_snapshot_save(dtrl_batch* b, const int32_t* env_ids, int n, dtrl_snapshot** out)
{ return guarded(b, [&](Engine& eng) -> int {
	dtrl::Snapshot* s = nullptr;
	const int rc = eng.SnapshotSave(env_ids, n, out ? &s : nullptr);
	if (out) *out = reinterpret_cast<dtrl_snapshot*>(s);
	return rc;
}); }
dtrl_status dtrl_snapshot_restore(dtrl_batch* b, const dtrl_snapshot* snap, const int32_t* env_ids, int n) { return guarded(b, [&](Engine& eng) { return eng.SnapshotRestore(snap_of(snap), env_ids, n); }); }
dtrl_status dtrl_clone_envs(dtrl_batch* b, const int32_t* src_ids, const int32_t* dst_ids, int n) { return guarded(b, [&](Engine& eng) { return eng.CloneEnvs(src_ids, dst_ids, n); }); }
dtrl_status dtrl_snapshot_export(const dtrl_snapshot* snap, void* buf, size_t cap, size_t* bytes)
{ return guarded_free([&]() -> int {
	dtrl::Snapshot* s = snap_of(snap);
	if (!s) { g_create_error = "dtrl_snapshot_export: null snapshot"; return DTRL_ERR_ARG; }
	if (!s->owner) { g_create_error = "dtrl_snapshot_export: the batch that held this snapshot's payload has been destroyed"; return DTRL_ERR_ARG; }
	return static_cast<dtrl_status>(s->owner->SnapshotExport(s, buf, cap, bytes));
}); }
dtrl_status dtrl_snapshot_import(dtrl_batch* b, const void* blob, size_t bytes, dtrl_snapshot** out)
{ return guarded(b, [&](Engine& eng) -> int {
	dtrl::Snapshot* s = nullptr;
	const int rc = eng.SnapshotImport(blob, bytes, out ? &s : nullptr);
	if (out) *out = reinterpret_cast<dtrl_snapshot*>(s);
	return rc;
}); }
dtrl_status dtrl_snapshot_info(const dtrl_snapshot* snap, int32_t* n_envs, size_t* bytes_per_env, size_t* sizeof_env_state, size_t* host_bytes_per_env)
{
	const dtrl::Snapshot* s = snap_of(snap);
	if (!s) return DTRL_ERR_ARG;
	if (n_envs) *n_envs = s->hdr.n_envs;
	if (bytes_per_env) *bytes_per_env = s->hdr.env_bytes;
	if (sizeof_env_state) *sizeof_env_state = s->hdr.sizeof_env_state;
	if (host_bytes_per_env) *host_bytes_per_env = s->hdr.host_bytes;
	return DTRL_OK;
}
dtrl_status dtrl_snapshot_free(dtrl_snapshot* snap)
{ return guarded_free([&]() -> int {
	dtrl::Snapshot* s = snap_of(snap);
	if (!s) return DTRL_OK;
	if (s->owner) s->owner->SnapshotRelease(s); else delete s;
	return DTRL_OK;
}); }

// not part of include/dtrl.h: developer hook used by tools/gpu_sections.py with the DTRL_PROFILE build
int dtrlx_profile_env(dtrl_batch* b, int section, unsigned long long* out, int cap) { return caught([&] { return b ? b->eng.ProfileEnv(section, out, cap) : 1; }, [&] { return dtrl_on_exception(b); }); }
// device time (ms, HIP events) of the snapshot kernel launches since the last call; -1 on a backend without launches (tools/snapshot_bench.py)
double dtrlx_snapshot_launch_ms(dtrl_batch* b) { return b ? b->eng.SnapLaunchMs() : -1.0; }
int dtrlx_profile_sections(dtrl_batch* b, unsigned long long* out, int cap) { return caught([&] { return b ? b->eng.ProfileSections(out, cap) : 1; }, [&] { return dtrl_on_exception(b); }); }

}  // extern "C"
