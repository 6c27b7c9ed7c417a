// dtrl_trainer_capi.inc -- the C ABI of include/dtrl_trainer.h over TrainerCore<Backend>; included by the HIP backend (product) and by the plain-loop
// check build (tests/emul, TESTS ONLY) after `Backend` is defined.
#include "../../include/dtrl_trainer.h"
#include "dtrl_trainer_files.h"
#include <cstdlib>
#include <new>
#include <random>

struct dtrl_trainer {
	dtrl_tr::TrainerCore<Backend>* core = nullptr;
	std::string err;
	float* host_x = nullptr; float* host_y = nullptr;      // device staging of the host-pointer calls (dtrl_trainer_eval_host / _step_host), made on first use
	std::vector<float> fx, fy;
	int fused_mode = 1;                                     // DTRL_TRAINER_FUSED as read at creation (dtrl_trainer_fused_info)
};
namespace {
std::string g_tr_create_error;
// a description the allocations and kernels below cannot take: every size that becomes a divisor, a loop bound or an allocation must be positive
bool tr_bad_desc(const dtrl_trainer_desc& s, std::string& why)
{
	auto bad = [&](const char* field, int idx, long long v) { why = std::string("bad trainer description: ") + field + (idx >= 0 ? "[" + std::to_string(idx) + "]" : std::string()) + " = " + std::to_string(v); return true; };
	if (s.n_heads < 1 || s.n_heads > dtrl_tr::kMaxHeads) return bad("n_heads", -1, s.n_heads);
	if (s.batch < 1) return bad("batch", -1, s.batch);
	if (s.max_eval < s.batch) return bad("max_eval", -1, s.max_eval);
	if (s.n_terrain < 1) return bad("n_terrain", -1, s.n_terrain);
	if (s.state_size <= s.n_terrain) return bad("state_size", -1, s.state_size);
	for (int l = 0; l < 3; ++l) {
		if (s.conv_ch[l] < 1) return bad("conv_ch", l, s.conv_ch[l]);
		if (s.conv_k[l] < 1) return bad("conv_k", l, s.conv_k[l]);
	}
	if (s.fc_terr < 1) return bad("fc_terr", -1, s.fc_terr);
	if (s.fc_trunk < 1) return bad("fc_trunk", -1, s.fc_trunk);
	if (s.fc_head < 1) return bad("fc_head", -1, s.fc_head);
	for (int f = 0; f < s.n_heads; ++f) if (s.head_out[f] < 1) return bad("head_out", f, s.head_out[f]);
	if (s.n_frags < 0) return bad("n_frags", -1, s.n_frags);
	if (s.frag_size < 0) return bad("frag_size", -1, s.frag_size);
	return false;
}
}

extern "C" {

int dtrl_trainer_create(const dtrl_trainer_desc* desc, int device_id, dtrl_trainer** out)
try {
	if (!desc || !out) return 1;
	*out = nullptr;
	if (tr_bad_desc(*desc, g_tr_create_error)) return 1;
	dtrl_tr::TrainerConfig c;
	dtrl_tr::NetDims& d = c.dims;
	std::memset(&d, 0, sizeof(d));
	d.S = desc->state_size; d.n_terr = desc->n_terrain;
	for (int l = 0; l < 3; ++l) { d.C[l + 1] = desc->conv_ch[l]; d.Kw[l] = desc->conv_k[l]; }
	d.fc_terr = desc->fc_terr; d.fc_trunk = desc->fc_trunk; d.fc_head = desc->fc_head; d.n_heads = desc->n_heads;
	for (int f = 0; f < d.n_heads; ++f) d.head_out[f] = desc->head_out[f];
	dtrl_tr::finish_dims(d);
	if (d.T[3] <= 0) { g_tr_create_error = "convolution kernels longer than the terrain slice"; return 1; }
	c.batch = desc->batch; c.max_eval = desc->max_eval; c.n_frags = desc->n_frags; c.frag_size = desc->frag_size;
	c.base_lr = desc->base_lr; c.momentum = desc->momentum; c.weight_decay = desc->weight_decay; c.discount = desc->discount;
	if (c.n_frags > 0 && (d.n_heads != 1 + c.n_frags || d.head_out[0] != c.n_frags)) { g_tr_create_error = "MACE layout: head 0 must hold n_frags values, heads 1.. the fragments"; return 1; }
	dtrl_trainer* t = new dtrl_trainer();
	{ const char* e = std::getenv("DTRL_TRAINER_FUSED"); t->fused_mode = e ? std::atoi(e) : 1; }   // (the HIP backend's setup_fused reads the same variable during Init)
	t->core = new dtrl_tr::TrainerCore<Backend>(c);
	t->core->cfg_target_frozen = desc->freeze_target != 0;
	t->core->be.device_id = device_id;
	if (!t->core->Init(t->err)) { g_tr_create_error = t->err; delete t->core; delete t; return 3; }
	*out = t;
	return 0;
} catch (const std::exception& e) { g_tr_create_error = e.what(); return 5; } catch (...) { g_tr_create_error = "unknown exception"; return 5; }

void dtrl_trainer_destroy(dtrl_trainer* t) { if (t) { if (t->host_x) t->core->be.free_dev(t->host_x); if (t->host_y) t->core->be.free_dev(t->host_y); delete t->core; delete t; } }
const char* dtrl_trainer_last_error(const dtrl_trainer* t) { return t ? t->err.c_str() : g_tr_create_error.c_str(); }
#define TR_GUARD(expr) try { if (!t) return 1; if (!(expr)) { t->err = t->core->be.error().empty() ? "bad arguments" : t->core->be.error(); return t->core->be.error().empty() ? 1 : 4; } return 0; } catch (const std::exception& e) { t->err = e.what(); return 5; } catch (...) { t->err = "unknown exception"; return 5; }
// which cut of the step this trainer runs: host-only, answered from fused_plan() of the net's dimensions and the mode read at creation (both builds; the check build
// reports the plan although it always runs the layer-by-layer form)
int dtrl_trainer_fused_info(const dtrl_trainer* t, int* plan_ok, int* lds_bytes, int* mode)
{
	if (!t) return 1;
	const dtrl_tr::FusedPlan p = dtrl_tr::fused_plan(t->core->cfg.dims);
	if (plan_ok) *plan_ok = p.ok ? 1 : 0;
	if (lds_bytes) *lds_bytes = p.lds_bytes;
	if (mode) *mode = t->fused_mode;
	return 0;
}
int dtrl_trainer_set_stream(dtrl_trainer* t, void* s) { TR_GUARD((t->core->be.set_stream(s), true)) }
int dtrl_trainer_sync(dtrl_trainer* t) { TR_GUARD((t->core->be.sync(), t->core->be.ok())) }
int64_t dtrl_trainer_num_params(const dtrl_trainer* t) { return t ? t->core->cfg.dims.num_params : 0; }
static float* tr_param_ptr(dtrl_trainer* t, int which)
{
	switch (which) { case 0: return t->core->w_cur; case 1: return t->core->w_tgt; case 2: return t->core->hist; case 3: return t->core->rate_mult; case 4: return t->core->decay_mult;
		case 5: return dtrl_tr::solver_needs_h2(t->core->solver.type) ? t->core->hist2 : nullptr; }
	return nullptr;
}
int dtrl_trainer_set_params(dtrl_trainer* t, int which, const float* host, int64_t n)
{ TR_GUARD(host && n == t->core->cfg.dims.num_params && tr_param_ptr(t, which) && (t->core->be.sync(), t->core->be.h2d(tr_param_ptr(t, which), host, sizeof(float) * n), t->core->be.ok())) }
int dtrl_trainer_get_params(dtrl_trainer* t, int which, float* host, int64_t n)
{ TR_GUARD(host && n == t->core->cfg.dims.num_params && tr_param_ptr(t, which) && (t->core->be.sync(), t->core->be.d2h(host, tr_param_ptr(t, which), sizeof(float) * n), t->core->be.ok())) }
// test / diagnosis hook: n floats of an internal device buffer (10 eval.xin, 11 eval.out, 12 new_q, 13 train.xin, 14 train.out, 15 train.dout, 16 gradient)
int dtrl_trainer_debug_get(dtrl_trainer* t, int which, float* host, int64_t n)
{
	float* p = nullptr;
	if (t) switch (which) { case 10: p = t->core->eval.xin; break; case 11: p = t->core->eval.out; break; case 12: p = t->core->newq; break; case 13: p = t->core->train.xin; break;
		case 14: p = t->core->train.out; break; case 15: p = t->core->train.dout; break; case 16: p = t->core->grad; break; }
	TR_GUARD(host && p && n > 0 && (t->core->be.sync(), t->core->be.d2h(host, p, sizeof(float) * n), t->core->be.ok()))
}
int dtrl_trainer_params_device(dtrl_trainer* t, int which, float** p) { TR_GUARD(p && (which == 0 || which == 1) && ((*p = tr_param_ptr(t, which)), true)) }
int dtrl_trainer_set_normalizers(dtrl_trainer* t, const double* io, const double* is, const double* oo, const double* os)
try {
	if (!t) return 1;
	const dtrl_tr::NetDims& d = t->core->cfg.dims;
	t->core->be.sync();
	auto put = [&](float* dst, const double* src, int n) { if (!src) return; std::vector<float> v(n); for (int i = 0; i < n; ++i) v[i] = static_cast<float>(src[i]); t->core->be.h2d(dst, v.data(), sizeof(float) * n); };
	put(t->core->in_off, io, d.S); put(t->core->in_scale, is, d.S); put(t->core->out_off, oo, d.out_size); put(t->core->out_scale, os, d.out_size);
	if (!t->core->be.ok()) { t->err = t->core->be.error(); return 4; }
	return 0;
} catch (...) { return 5; }
int dtrl_trainer_update_target(dtrl_trainer* t) { TR_GUARD((t->core->UpdateTarget(), t->core->be.ok())) }
int dtrl_trainer_eval(dtrl_trainer* t, int which, const float* X, int n, float* Y) { TR_GUARD(X && Y && t->core->Eval(which, X, n, Y)) }
int dtrl_trainer_step(dtrl_trainer* t, const float* X, const float* Y) { TR_GUARD(X && Y && t->core->Step(X, Y)) }
int dtrl_trainer_bind_replay(dtrl_trainer* t, const float* mem, const int64_t* flags, int W)
{ TR_GUARD(mem && flags && (t->core->cfg.n_frags > 0 ? W == 1 + 2 * t->core->cfg.dims.S + 1 + t->core->cfg.frag_size : W >= 2 * t->core->cfg.dims.S + 2) && (t->core->BindReplay(mem, flags, W), true)) }
float* dtrl_trainer_stage_rows(dtrl_trainer* t) { return (t && t->core->EnsureStage()) ? t->core->stage_rows : nullptr; }
int64_t* dtrl_trainer_stage_flags(dtrl_trainer* t) { return (t && t->core->EnsureStage()) ? t->core->stage_flags : nullptr; }
int dtrl_trainer_stage_capacity(dtrl_trainer* t) { return t ? t->core->kStageRows : 0; }
int dtrl_trainer_add_staged(dtrl_trainer* t, int first, int n, int64_t head, int64_t mem_size) { TR_GUARD(t->core->AddStaged(first, n, head, mem_size)) }
int64_t* dtrl_trainer_idx(dtrl_trainer* t) { return t ? t->core->idx_host : nullptr; }
int32_t* dtrl_trainer_better(dtrl_trainer* t) { return t ? t->core->better_host : nullptr; }
float* dtrl_trainer_loss(dtrl_trainer* t) { return t ? t->core->loss_host : nullptr; }
int dtrl_trainer_critic_step(dtrl_trainer* t) { TR_GUARD(t->core->CriticStep()) }
int dtrl_trainer_critic_step_and_filter(dtrl_trainer* t) { TR_GUARD(t->core->CriticStepAndFilter()) }
int dtrl_trainer_actor_filter(dtrl_trainer* t, int n) { TR_GUARD(t->core->ActorFilter(n)) }
int dtrl_trainer_actor_step(dtrl_trainer* t) { TR_GUARD(t->core->ActorStep()) }
int dtrl_trainer_value_step(dtrl_trainer* t, int kind) { TR_GUARD(t->core->ValueStep(kind)) }
int dtrl_trainer_td_filter(dtrl_trainer* t, int n) { TR_GUARD(t->core->TdFilter(n)) }
float* dtrl_trainer_td(dtrl_trainer* t) { return t ? t->core->td_host : nullptr; }
int dtrl_trainer_action_step(dtrl_trainer* t) { TR_GUARD(t->core->ActionStep()) }
// ---- entry points for a C++ host that has nothing but the reference's files and host arrays (include/BatchNeuralNet.h) ----
// ---- the six solver types (cNNSolver::BuildSolver, learning/NNSolver.cpp:9-35) ----
static dtrl_tr::SolverCfg tr_solver_cfg(const dtrl_solver_desc& s)
{
	dtrl_tr::SolverCfg c;
	c.type = s.type; c.policy = s.lr_policy; c.base_lr = s.base_lr; c.momentum = s.momentum; c.momentum2 = s.momentum2; c.rms_decay = s.rms_decay; c.delta = s.delta;
	c.weight_decay = s.weight_decay; c.gamma = s.gamma; c.power = s.power; c.clip = s.clip_gradients; c.stepsize = s.stepsize;
	return c;
}
int dtrl_trainer_set_solver(dtrl_trainer* t, const dtrl_solver_desc* s)
try {
	if (!t || !s) return 1;
	std::string why;
	if (!t->core->SetSolver(tr_solver_cfg(*s), why)) { t->err = why; return t->core->be.ok() ? 1 : 4; }
	return 0;
} catch (const std::exception& e) { t->err = e.what(); return 5; } catch (...) { t->err = "unknown exception"; return 5; }
int dtrl_trainer_get_solver(dtrl_trainer* t, dtrl_solver_desc* s, int64_t* iter)
try {
	if (!t) return 1;
	const dtrl_tr::SolverCfg& c = t->core->solver;
	if (s) { s->type = c.type; s->lr_policy = c.policy; s->base_lr = c.base_lr; s->momentum = c.momentum; s->momentum2 = c.momentum2; s->rms_decay = c.rms_decay; s->delta = c.delta;
		s->weight_decay = c.weight_decay; s->gamma = c.gamma; s->power = c.power; s->clip_gradients = c.clip; s->stepsize = c.stepsize; }
	const int64_t it = t->core->GetIter();
	if (iter) *iter = it;
	if (!t->core->be.ok()) { t->err = t->core->be.error(); return 4; }
	return 0;
} catch (...) { return 5; }
int dtrl_trainer_set_solver_iter(dtrl_trainer* t, int64_t iter) { TR_GUARD(iter >= 0 && (t->core->SetIter(iter), t->core->be.ok())) }
int dtrl_trainer_create_from_files(const char* net_file, const char* solver_file, const char* data_root, float discount, int freeze_target, int device_id, dtrl_trainer** out)
try {
	if (!net_file || !out) return 1;
	dtrl_tr::TrainerFiles f; std::string err;
	if (!dtrl_tr::ParseTrainerFiles(net_file, solver_file ? solver_file : "", data_root ? data_root : "", f, err)) { g_tr_create_error = err; return 1; }
	f.desc.discount = discount; f.desc.freeze_target = freeze_target;
	int rc = dtrl_trainer_create(&f.desc, device_id, out);
	if (rc != 0) return rc;
	dtrl_trainer* t = *out;
	if (static_cast<int64_t>(f.lr_mult.size()) != t->core->cfg.dims.num_params) { g_tr_create_error = "parameter count of the prototxt does not match the net built from it"; dtrl_trainer_destroy(t); *out = nullptr; return 1; }
	t->core->be.h2d(t->core->rate_mult, f.lr_mult.data(), sizeof(float) * f.lr_mult.size());
	t->core->be.h2d(t->core->decay_mult, f.decay_mult.data(), sizeof(float) * f.decay_mult.size());
	t->core->be.sync();
	if (!t->core->be.ok()) { g_tr_create_error = t->core->be.error(); dtrl_trainer_destroy(t); *out = nullptr; return 4; }
	if (f.has_solver) {       // the solver file's type and policy (a file that names none: SGD / "fixed", which is what the description alone gives)
		const int rs = dtrl_trainer_set_solver(t, &f.solver);
		if (rs != 0) { g_tr_create_error = f.solver_file + ": " + t->err; dtrl_trainer_destroy(t); *out = nullptr; return rs; }
	}
	return 0;
} catch (const std::exception& e) { g_tr_create_error = e.what(); return 5; } catch (...) { g_tr_create_error = "unknown exception"; return 5; }
int dtrl_trainer_dims(const dtrl_trainer* t, int* in_size, int* out_size, int* batch, int* max_eval)
{
	if (!t) return 1;
	if (in_size) *in_size = t->core->cfg.dims.S;
	if (out_size) *out_size = t->core->cfg.dims.out_size;
	if (batch) *batch = t->core->cfg.batch;
	if (max_eval) *max_eval = t->core->cfg.max_eval;
	return 0;
}
// Caffe's "xavier" weight filler (uniform +- sqrt(3 / fan_in)) and constant-0 biases, what the family's prototxts ask for; both nets and a cleared history
int dtrl_trainer_init_xavier(dtrl_trainer* t, uint64_t seed)
try {
	if (!t) return 1;
	const dtrl_tr::NetDims& d = t->core->cfg.dims;
	std::vector<float> w(static_cast<size_t>(d.num_params), 0.0f);
	std::mt19937_64 rng(seed);
	auto fill = [&](int64_t off, int64_t n, int64_t fan_in) { const double s = std::sqrt(3.0 / static_cast<double>(fan_in)); std::uniform_real_distribution<double> u(-s, s); for (int64_t i = 0; i < n; ++i) w[static_cast<size_t>(off + i)] = static_cast<float>(u(rng)); };
	for (int l = 0; l < 3; ++l) fill(d.wo_conv[l], static_cast<int64_t>(d.C[l + 1]) * d.C[l] * d.Kw[l], static_cast<int64_t>(d.C[l]) * d.Kw[l]);
	fill(d.wo_terr, static_cast<int64_t>(d.fc_terr) * d.n_flat, d.n_flat);
	fill(d.wo_ip0, static_cast<int64_t>(d.fc_trunk) * (d.fc_terr + d.n_char), d.fc_terr + d.n_char);
	for (int f = 0; f < d.n_heads; ++f) { fill(d.wo_h0[f], static_cast<int64_t>(d.fc_head) * d.fc_trunk, d.fc_trunk); fill(d.wo_h1[f], static_cast<int64_t>(d.head_out[f]) * d.fc_head, d.fc_head); }
	t->core->be.sync();
	t->core->be.h2d(t->core->w_cur, w.data(), sizeof(float) * w.size()); t->core->be.h2d(t->core->w_tgt, w.data(), sizeof(float) * w.size());
	t->core->ClearSolverState();      // both histories and the counter
	t->core->be.sync();
	if (!t->core->be.ok()) { t->err = t->core->be.error(); return 4; }
	return 0;
} catch (...) { return 5; }
static bool tr_host_stage(dtrl_trainer* t)
{
	const dtrl_tr::NetDims& d = t->core->cfg.dims;
	const size_t rows = static_cast<size_t>(t->core->cfg.max_eval);
	if (!t->host_x) t->host_x = static_cast<float*>(t->core->be.alloc_dev(sizeof(float) * rows * d.S));
	if (!t->host_y) t->host_y = static_cast<float*>(t->core->be.alloc_dev(sizeof(float) * rows * d.out_size));
	return t->host_x && t->host_y;
}
// cNeuralNet::Eval / EvalBatch with HOST arrays of doubles (Eigen's storage): Y[n][out] = un-normalised outputs of net `which` on X[n][in]; any n; synchronous
int dtrl_trainer_eval_host(dtrl_trainer* t, int which, const double* X, int n, double* Y)
try {
	if (!t || !X || !Y || n < 0 || !tr_host_stage(t)) return 1;
	const dtrl_tr::NetDims& d = t->core->cfg.dims;
	const int cap = t->core->cfg.max_eval;
	for (int k = 0; k < n; k += cap) {
		const int m = n - k < cap ? n - k : cap;
		t->fx.resize(static_cast<size_t>(m) * d.S); t->fy.resize(static_cast<size_t>(m) * d.out_size);
		for (size_t i = 0; i < t->fx.size(); ++i) t->fx[i] = static_cast<float>(X[static_cast<size_t>(k) * d.S + i]);
		t->core->be.sync();
		t->core->be.h2d(t->host_x, t->fx.data(), sizeof(float) * t->fx.size());
		if (!t->core->Eval(which, t->host_x, m, t->host_y)) { t->err = t->core->be.error(); return 4; }
		t->core->be.sync();
		t->core->be.d2h(t->fy.data(), t->host_y, sizeof(float) * t->fy.size());
		t->core->be.sync();
		for (size_t i = 0; i < t->fy.size(); ++i) Y[static_cast<size_t>(k) * d.out_size + i] = t->fy[i];
	}
	if (!t->core->be.ok()) { t->err = t->core->be.error(); return 4; }
	return 0;
} catch (...) { return 5; }
// cNeuralNet::Train on one batch of HOST doubles: X[batch][in], un-normalised labels Y[batch][out]; synchronous, *loss (may be NULL) = the EuclideanLoss
int dtrl_trainer_step_host(dtrl_trainer* t, const double* X, const double* Y, double* loss)
try {
	if (!t || !X || !Y || !tr_host_stage(t)) return 1;
	const dtrl_tr::NetDims& d = t->core->cfg.dims;
	const int m = t->core->cfg.batch;
	t->fx.resize(static_cast<size_t>(m) * d.S); t->fy.resize(static_cast<size_t>(m) * d.out_size);
	for (size_t i = 0; i < t->fx.size(); ++i) t->fx[i] = static_cast<float>(X[i]);
	for (size_t i = 0; i < t->fy.size(); ++i) t->fy[i] = static_cast<float>(Y[i]);
	t->core->be.sync();
	t->core->be.h2d(t->host_x, t->fx.data(), sizeof(float) * t->fx.size()); t->core->be.h2d(t->host_y, t->fy.data(), sizeof(float) * t->fy.size());
	if (!t->core->Step(t->host_x, t->host_y)) { t->err = t->core->be.error(); return 4; }
	t->core->be.sync();
	if (loss) *loss = t->core->loss_host[0];
	if (!t->core->be.ok()) { t->err = t->core->be.error(); return 4; }
	return 0;
} catch (...) { return 5; }
int dtrl_trainer_get_normalizers(dtrl_trainer* t, double* io, double* is, double* oo, double* os)
try {
	if (!t) return 1;
	const dtrl_tr::NetDims& d = t->core->cfg.dims;
	t->core->be.sync();
	auto get = [&](const float* src, double* dst, int n) { if (!dst) return; std::vector<float> v(n); t->core->be.d2h(v.data(), src, sizeof(float) * n); t->core->be.sync(); for (int i = 0; i < n; ++i) dst[i] = v[i]; };
	get(t->core->in_off, io, d.S); get(t->core->in_scale, is, d.S); get(t->core->out_off, oo, d.out_size); get(t->core->out_scale, os, d.out_size);
	return t->core->be.ok() ? 0 : 4;
} catch (...) { return 5; }
// cNeuralNet::CopyModel (learning/NeuralNet.cpp:722-733): the current net's parameters and the four normaliser vectors of `src` into `dst` (same topology, same
// device), device to device; dst's solver history is kept (Caffe's solver keeps its history across CopyTrainedLayersFrom as well)
int dtrl_trainer_copy_model(dtrl_trainer* dst, dtrl_trainer* src)
try {
	if (!dst || !src) return 1;
	const dtrl_tr::NetDims& a = dst->core->cfg.dims; const dtrl_tr::NetDims& b = src->core->cfg.dims;
	if (a.num_params != b.num_params || a.S != b.S || a.out_size != b.out_size) { dst->err = "dtrl_trainer_copy_model: different topologies"; return 1; }
	src->core->be.sync(); dst->core->be.sync();
	dst->core->be.d2d(dst->core->w_cur, src->core->w_cur, sizeof(float) * a.num_params);
	dst->core->be.d2d(dst->core->in_off, src->core->in_off, sizeof(float) * a.S); dst->core->be.d2d(dst->core->in_scale, src->core->in_scale, sizeof(float) * a.S);
	dst->core->be.d2d(dst->core->out_off, src->core->out_off, sizeof(float) * a.out_size); dst->core->be.d2d(dst->core->out_scale, src->core->out_scale, sizeof(float) * a.out_size);
	dst->core->be.sync();
	if (!dst->core->be.ok()) { dst->err = dst->core->be.error(); return 4; }
	return 0;
} catch (...) { return 5; }

int dtrl_trainer_bind_grad(dtrl_trainer* t, float* grad_dev) { TR_GUARD((t->core->be.sync(), t->core->BindGrad(grad_dev), t->core->be.ok())) }
int dtrl_trainer_grad_device(dtrl_trainer* t, float** p) { TR_GUARD(p && ((*p = t->core->grad), true)) }
int dtrl_trainer_grad_step(dtrl_trainer* t, const float* X, const float* Y) { TR_GUARD(X && Y && t->core->GradStep(X, Y)) }
int dtrl_trainer_critic_grad(dtrl_trainer* t) { TR_GUARD(t->core->CriticGrad()) }
int dtrl_trainer_actor_grad(dtrl_trainer* t) { TR_GUARD(t->core->ActorGrad()) }
int dtrl_trainer_zero_grad(dtrl_trainer* t) { TR_GUARD(t->core->ZeroGrad()) }
int dtrl_trainer_apply_grad(dtrl_trainer* t, int slot) { TR_GUARD(t->core->ApplyGrad(slot)) }

}  // extern "C"
