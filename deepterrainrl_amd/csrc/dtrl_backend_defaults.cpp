// dtrl_backend_defaults.cpp -- the Backend interface's default implementations (dtrl_engine.h): snapshot transport, external-policy hand-over, launches over
// envs of several slots or variants and the per-slot sums, and the per-env rules of the frame boundary (terrain work under the batch's terrain, a terrain set
// or a ladder; variant redraw; variant rescale; push schedule; perturbation rows; episode limit; frame trace; episode log), each built from the interface's own copies and Launch. The rules all run over an EnvSpan that
// SpanList turns into a host vector. What the lane-loop check build runs; the HIP backend overrides every one of them with kernels and keeps these as its
// cross-check (DTRL_SNAPSHOT_FALLBACK=1, DTRL_SLOTS_FALLBACK=1, DTRL_VARIANTS_FALLBACK=1, DTRL_TERRAINS_FALLBACK=1, DTRL_PUSH_FALLBACK=1, DTRL_PERTURB_FALLBACK=1, DTRL_EPISODE_FALLBACK=1, DTRL_TRACE_FALLBACK=1, DTRL_EPISODE_LOG_FALLBACK=1).
// Compiled as the tail of dtrl_engine.cpp (included there, listed in no Makefile): whoever builds the engine's three host sources -- the libraries, the
// lane-loop check build of any tests/ tree, the sanitizer scripts -- has the defaults, and no source list can lack them.
#include "dtrl_engine.h"
#include "dtrl_terrain_dev.h"
#include <algorithm>
#include <cstddef>

namespace dtrl {

// where env e's record r is read from, and whether that is host memory (the status array of host terrain mode; a staged terrain record)
static const char* SnapSrc(const SnapPlan& p, int r, int e, bool* host)
{
	if (r == p.gr_rec && p.stage_slot && p.stage_slot[e] > 0) { *host = true; return reinterpret_cast<const char*>(&p.gr_stage[p.stage_slot[e] - 1]); }
	*host = p.rec[r].host != 0;
	return p.rec[r].slab + static_cast<size_t>(e) * p.rec[r].bytes;
}
bool Backend::SnapGather(const SnapPlan& p, char* payload, const int32_t* ids, int n)
{
	for (int i = 0; i < n; ++i) for (int r = 0; r < p.n_rec; ++r) {
		bool host; const char* src = SnapSrc(p, r, ids[i], &host);
		char* dst = payload + static_cast<size_t>(i) * p.env_bytes + p.rec[r].off;
		if (!(host ? H2D(dst, src, p.rec[r].bytes) : D2D(dst, src, p.rec[r].bytes))) return false;
	}
	return true;
}
bool Backend::SnapScatter(const SnapPlan& p, const char* payload, const int32_t* ids, int n)
{
	for (int i = 0; i < n; ++i) for (int r = 0; r < p.n_rec; ++r) {
		char* dst = p.rec[r].slab + static_cast<size_t>(ids[i]) * p.rec[r].bytes;
		const char* src = payload + static_cast<size_t>(i) * p.env_bytes + p.rec[r].off;
		if (!(p.rec[r].host ? D2H(dst, src, p.rec[r].bytes) : D2D(dst, src, p.rec[r].bytes))) return false;
	}
	return true;
}
bool Backend::SnapCopy(const SnapPlan& p, const int32_t* src_ids, const int32_t* dst_ids, int n)
{
	for (int i = 0; i < n; ++i) for (int r = 0; r < p.n_rec; ++r) {
		bool host; const char* src = SnapSrc(p, r, src_ids[i], &host);
		char* dst = p.rec[r].slab + static_cast<size_t>(dst_ids[i]) * p.rec[r].bytes;
		if (p.rec[r].host) { for (uint32_t k = 0; k < p.rec[r].bytes; ++k) dst[k] = src[k]; continue; }   // host to host (the streams are idle)
		if (!(host ? H2D(dst, src, p.rec[r].bytes) : D2D(dst, src, p.rec[r].bytes))) return false;
	}
	return true;
}
bool Backend::ExtCollect(const DevBuffers& buf, int n_envs, int cap, int32_t* ids, void* states, bool f32, int32_t* meta)
{
	int m = 0, na = 0, nr = 0;
	std::vector<real> row(static_cast<size_t>(buf.S));
	std::vector<float> rf(f32 ? row.size() : 0); std::vector<double> rd(f32 ? 0 : row.size());
	for (int e = 0; e < n_envs; ++e) {
		int32_t park = 0;
		if (!D2H(&park, &buf.st[e].ext_park, sizeof(park))) return false;
		if (park == kExtReady) ++nr;
		if (park != kExtAwaiting) continue;
		++na;
		if (m >= cap) continue;
		const int32_t id = e;
		if (!H2D(ids + m, &id, sizeof(id))) return false;
		if (states) {
			if (!D2H(row.data(), buf.poli_state + static_cast<size_t>(e) * buf.S, sizeof(real) * row.size())) return false;
			if (f32) { for (size_t k = 0; k < row.size(); ++k) rf[k] = static_cast<float>(row[k]); if (!H2D(static_cast<float*>(states) + static_cast<size_t>(m) * buf.S, rf.data(), sizeof(float) * rf.size())) return false; }
			else { for (size_t k = 0; k < row.size(); ++k) rd[k] = static_cast<double>(row[k]); if (!H2D(static_cast<double*>(states) + static_cast<size_t>(m) * buf.S, rd.data(), sizeof(double) * rd.size())) return false; }
		}
		++m;
	}
	meta[0] = m; meta[1] = na; meta[2] = nr; meta[3] = 0;
	return true;
}
bool Backend::ExtSupply(const DevBuffers& buf, int n_envs, int n_opt, int n_labels, const int32_t* ids, int n, const int32_t* action_ids, const void* params, bool f32, const uint32_t* flags, bool apply, int32_t* rejected)
{
	*rejected = 0;
	std::vector<float> pf(f32 ? n_opt : 0); std::vector<double> pd(f32 ? 0 : n_opt);
	for (int i = 0; i < n; ++i) {
		int32_t e = -1, park = 0;
		if (!D2H(&e, ids + i, sizeof(e))) return false;
		if (e >= 0 && e < n_envs && !D2H(&park, &buf.st[e].ext_park, sizeof(park))) return false;
		ExtAction a{};
		if (action_ids && !D2H(&a.action_id, action_ids + i, sizeof(int32_t))) return false;
		if (e < 0 || e >= n_envs || park != kExtAwaiting || a.action_id < 0 || a.action_id >= n_labels) { ++*rejected; continue; }
		if (!apply) continue;
		if (flags && !D2H(&a.flags, flags + i, sizeof(uint32_t))) return false;
		if (f32) { if (!D2H(pf.data(), static_cast<const float*>(params) + static_cast<size_t>(i) * n_opt, sizeof(float) * n_opt)) return false; for (int k = 0; k < n_opt; ++k) a.params[k] = static_cast<real>(pf[k]); }
		else { if (!D2H(pd.data(), static_cast<const double*>(params) + static_cast<size_t>(i) * n_opt, sizeof(double) * n_opt)) return false; for (int k = 0; k < n_opt; ++k) a.params[k] = static_cast<real>(pd[k]); }
		park = kExtReady;
		if (!H2D(&ext_actions(buf)[e], &a, sizeof(a)) || !H2D(&buf.st[e].ext_park, &park, sizeof(park))) return false;
	}
	return true;
}
// The launch list of `buf` (n_envs entries; no list: envs 0 .. n_envs - 1) regrouped by key_of_env[] into `part`, list order kept inside a key; n_of[k] = entries
// of key k, in key order. list_host: the list in host-readable form, nullptr = read it back. Waits for the selected stream before it writes `part`.
// key_dev != nullptr (a variant redraw on device terrain: the device array is the truth): the listed envs' keys are read back from there, behind that wait.
static bool SplitLaunchList(Backend& be, const DevBuffers& buf, int n_envs, const int32_t* list_host, const int32_t* key_of_env, const int32_t* key_dev, int n_keys, int32_t* part, std::vector<int32_t>& n_of)
{
	std::vector<int32_t> list(static_cast<size_t>(n_envs));
	if (!buf.env_list) { for (int i = 0; i < n_envs; ++i) list[i] = i; }
	else if (list_host) { for (int i = 0; i < n_envs; ++i) list[i] = list_host[i]; }
	else if (!be.D2H(list.data(), buf.env_list, sizeof(int32_t) * list.size())) return false;   // (an order computed on the device: behind everything queued, this launch's list included)
	if (!be.SyncSelected()) return false;   // an earlier launch of this stream may still be reading `part`
	std::vector<int32_t> fetched; int32_t first = 0;
	if (key_dev) {   // one copy of the span of the key array that holds the listed envs
		const auto mm = std::minmax_element(list.begin(), list.end());
		first = *mm.first;
		fetched.resize(static_cast<size_t>(*mm.second - first + 1));
		if (!be.D2H(fetched.data(), key_dev + first, sizeof(int32_t) * fetched.size())) return false;
		key_of_env = fetched.data();
	}
	n_of.assign(static_cast<size_t>(n_keys), 0);
	std::vector<int32_t> at(static_cast<size_t>(n_keys));
	for (int32_t e : list) ++n_of[key_of_env[e - first]];
	for (int s = 0, k = 0; s < n_keys; ++s) { at[s] = k; k += n_of[s]; }
	for (int32_t e : list) part[at[key_of_env[e - first]]++] = e;
	return true;
}
bool Backend::LaunchKeyed(const DevModel* gm, const RunParams& rp, const DevBuffers& buf, const EnvKeyView& keys, int n_envs, int n_steps, real dt, bool frame_end)
{
	if (n_envs <= 0) return true;
	std::vector<int32_t> n_of;
	if (!SplitLaunchList(*this, buf, n_envs, keys.env_list_host, keys.env_key_host, keys.keys_on_device ? keys.env_key_dev : nullptr, keys.n_keys, keys.part, n_of)) return false;
	for (int k = 0, at = 0; k < keys.n_keys; at += n_of[k], ++k) {
		if (n_of[k] == 0) continue;
		RunParams r = rp; DevBuffers b = buf;
		if (keys.slots_host) slot_patch(keys.slots_host[k], r, b);
		b.env_list = keys.part + at;
		if (!Launch(keys.models_dev ? keys.models_dev + k : gm, r, b, n_of[k], n_steps, dt, frame_end)) return false;
	}
	return true;
}
bool Backend::SlotReduce(const EnvState* st, const int32_t* env_slot, int n_envs, int n_slots, SlotSums* sums, int slot_base)
{
	std::vector<EnvState> host(static_cast<size_t>(n_envs)); std::vector<int32_t> slot(static_cast<size_t>(n_envs));
	if (!D2H(host.data(), st, sizeof(EnvState) * host.size()) || !D2H(slot.data(), env_slot, sizeof(int32_t) * slot.size())) return false;
	for (int s = 0; s < n_slots; ++s) sums[s] = SlotSums{0, 0, 0, 0, 0.0};
	for (int e = 0; e < n_envs; ++e) {
		const int s = slot[e] - slot_base;
		if (s < 0 || s >= n_slots) continue;
		SlotSums& a = sums[s];
		++a.n_envs; a.episodes += host[e].num_episodes; a.cycles += host[e].num_cycles; a.resets += host[e].num_resets;
		a.dist_sum += static_cast<double>(host[e].avg_dist) * static_cast<double>(host[e].num_episodes);
	}
	return true;
}
bool Backend::SpanList(const EnvSpan& span, std::vector<int32_t>& list)
{
	list.resize(static_cast<size_t>(span.n > 0 ? span.n : 0));
	if (span.list) return list.empty() || D2H(list.data(), span.list, sizeof(int32_t) * list.size());
	for (int k = 0; k < span.n; ++k) span_env(k, span.e0, span.n, nullptr, list[k]);
	return true;
}
// The opening of every rule default below: the span as a host vector and, with `wait`, the wait for the selected stream. False: the default is over, and *done
// is what it returns -- true for an empty span, false where a copy or the wait failed
static bool SpanOpen(Backend& be, const EnvSpan& span, bool wait, std::vector<int32_t>& list, bool* done)
{
	*done = be.SpanList(span, list) && (list.empty() || !wait || be.SyncSelected());
	return *done && !list.empty();
}
// Variant redraw: the rule (var_redraw_step) on the host, env by env; key and counter go back where they changed. The first D2H waits for the selected stream.
bool Backend::VariantRedraw(const EnvStatus* status, const EnvSpan& span, int32_t* env_model, RedrawRec* recs, const RedrawCfg& cfg)
{
	std::vector<int32_t> list; bool done;
	if (!SpanOpen(*this, span, false, list, &done)) return done;
	std::vector<double> cum(static_cast<size_t>(cfg.hi - cfg.lo + 1));
	if (!D2H(cum.data(), cfg.cum, sizeof(double) * cum.size())) return false;
	EnvStatus st; RedrawRec r; int32_t key = 0;
	for (int32_t e : list) {
		if (!D2H(&st, status + e, sizeof(st))) return false;
		if (!(st.need_reset & 1)) continue;
		if (!D2H(&key, env_model + e, sizeof(key)) || !D2H(&r, recs + e, sizeof(r))) return false;
		const int32_t draws0 = r.draws;
		const int32_t next = var_redraw_step(r, key, true, cfg, cum.data(), e);
		if (next != key && !H2D(env_model + e, &next, sizeof(next))) return false;
		if (r.draws != draws0 && !H2D(recs + e, &r, sizeof(r))) return false;
	}
	return true;
}
// Variant rescale: the rule (rescale_step) on the host, env by env, on a copy of the env's private record; the seven fields the rule writes -- and only those --
// and the counter go back. Waits for the selected stream first.
bool Backend::VariantRescale(const EnvStatus* status, const EnvSpan& span, const int32_t* env_model, DevModel* models, int key_base, RescaleRec* recs, const ModelScalarsD* base, const RescaleCfg& cfg)
{
	std::vector<int32_t> list; bool done;
	if (!SpanOpen(*this, span, true, list, &done)) return done;
	ModelScalarsD b;
	if (!D2H(&b, base, sizeof(b))) return false;
	EnvStatus st; RescaleRec r; int32_t key = 0; DevModel m;
	for (int32_t e : list) {
		if (status) { if (!D2H(&st, status + e, sizeof(st))) return false; if (!(st.need_reset & 1)) continue; }
		if (!D2H(&key, env_model + e, sizeof(key))) return false;
		if (key != key_base + e) continue;
		DevModel* dst = models + key;
		if (!D2H(&r, recs + e, sizeof(r)) || !D2H(&m, dst, sizeof(m))) return false;
		if (!rescale_step(r, true, true, cfg, b, e, m)) continue;
		const size_t row = sizeof(real) * static_cast<size_t>(cfg.L);
		if (!H2D(dst->mass, m.mass, row) || !H2D(dst->sub_mass, m.sub_mass, row) || !H2D(dst->inertia, m.inertia, row) || !H2D(dst->kp, m.kp, row) || !H2D(dst->kd, m.kd, row)
			|| !H2D(dst->torque_lim, m.torque_lim, row) || !H2D(&dst->total_mass, &m.total_mass, sizeof(real)) || !H2D(recs + e, &r, sizeof(r))) return false;
	}
	return true;
}
// Push schedule: the rule (push_step) on the host, env by env; record and slot go back where they changed. The first D2H waits for the selected stream.
// The slot's seven fields are two runs of EnvState: pert_link / pert_on, and pert_f .. pert_dur.
static bool WriteSlotFields(Backend& be, EnvState* dst, const EnvState& src)
{
	static_assert(offsetof(EnvState, pert_on) == offsetof(EnvState, pert_link) + sizeof(int32_t), "pert_link / pert_on are one run");
	static_assert(offsetof(EnvState, pert_dur) == offsetof(EnvState, pert_f) + 6 * sizeof(real), "pert_f .. pert_dur are one run");
	char* d = reinterpret_cast<char*>(dst); const char* s = reinterpret_cast<const char*>(&src);
	return be.H2D(d + offsetof(EnvState, pert_link), s + offsetof(EnvState, pert_link), 2 * sizeof(int32_t))
		&& be.H2D(d + offsetof(EnvState, pert_f), s + offsetof(EnvState, pert_f), 7 * sizeof(real));
}
bool Backend::PushSchedule(const EnvStatus* status, const EnvSpan& span, EnvState* st, PushRec* recs, const double* scale, const PushCfg& cfg)
{
	std::vector<int32_t> list; bool done;
	if (!SpanOpen(*this, span, true, list, &done)) return done;
	EnvStatus es; PushRec r; double sc = 0; EnvState slot;
	for (int32_t e : list) {
		if (!D2H(&sc, scale + e, sizeof(sc))) return false;
		if (sc == 0) continue;
		bool start = true;
		if (status) { if (!D2H(&es, status + e, sizeof(es))) return false; start = es.need_reset != 0; }
		if (!D2H(&r, recs + e, sizeof(r))) return false;
		PushOut out;
		const bool fired = push_step(r, sc, start, cfg, e, out);
		if (fired) { push_write_slot(slot, out); if (!WriteSlotFields(*this, st + e, slot)) return false; }
		if (!H2D(recs + e, &r, sizeof(r))) return false;   // (an env in the schedule moves its record at every boundary: the wait, or the counter)
	}
	return true;
}
// Episode limit: the rule (episode_limit_step) on the host, env by env, behind a wait for the selected stream; the record goes back where it moved, and for an env
// the rule ends, episode_end's three state fields and the status record. A held-out env costs one flag read.
bool Backend::EpisodeLimit(EnvStatus* status, const EnvSpan& span, EnvState* st, EpisodeRec* recs, const uint8_t* on, const EpisodeCfg& cfg)
{
	std::vector<int32_t> list; bool done;
	if (!SpanOpen(*this, span, true, list, &done)) return done;
	EnvStatus es; EpisodeRec r; uint8_t flag = 0; EnvState s;
	for (int32_t e : list) {
		if (!D2H(&flag, on + e, sizeof(flag))) return false;
		if (!flag) continue;
		if (status && !D2H(&es, status + e, sizeof(es))) return false;
		if (!D2H(&r, recs + e, sizeof(r))) return false;
		if (episode_limit_step(r, status ? &es : nullptr, cfg, e) != kEpisodeRuns) {
			if (!D2H(&s, st + e, sizeof(s))) return false;
			episode_end(s, es, cfg);
			if (!H2D(&st[e].avg_dist, &s.avg_dist, sizeof(s.avg_dist)) || !H2D(&st[e].num_episodes, &s.num_episodes, sizeof(s.num_episodes)) || !H2D(&st[e].need_reset, &s.need_reset, sizeof(s.need_reset))
				|| !H2D(&status[e].need_reset, &es.need_reset, sizeof(es.need_reset)) || !H2D(&status[e].episode_dist, &es.episode_dist, sizeof(es.episode_dist))) return false;
		}
		if (!H2D(recs + e, &r, sizeof(r))) return false;   // (an env under the limit moves its record at every boundary: the frame count)
	}
	return true;
}
// Frame trace: the rule (trace_due / trace_value / trace_int) on the host, traced index by traced index, behind a wait for the selected stream: the env's state and
// status record, its counter and its keys come down, the row goes up into its ring slot, then the counter.
bool Backend::TraceRecord(const EnvState* st, const EnvStatus* status, const TraceView& tv, const int32_t* list, int n)
{
	if (n <= 0) return true;
	std::vector<int32_t> ts(static_cast<size_t>(n));
	if (!D2H(ts.data(), list, sizeof(int32_t) * ts.size()) || !SyncSelected()) return false;
	EnvState s; EnvStatus es;
	std::vector<double> vals(static_cast<size_t>(tv.W)); int32_t ints[kTraceInts];
	for (int32_t t : ts) {
		int32_t e = 0; int64_t w = 0; int32_t key[3] = {0, 0, 0};
		if (!D2H(&e, tv.env_of + t, sizeof(e)) || !D2H(&s, st + e, sizeof(s))) return false;
		if (!trace_due(s)) continue;
		const int32_t* const key_dev[3] = {tv.env_slot, tv.env_variant, tv.env_terrain};
		for (int k = 0; k < 3; ++k) if (key_dev[k] && !D2H(&key[k], key_dev[k] + e, sizeof(int32_t))) return false;
		if (!D2H(&es, status + e, sizeof(es)) || !D2H(&w, tv.written + t, sizeof(w))) return false;
		for (int k = 0; k < tv.W; ++k) vals[k] = trace_value(s, tv.D, k);
		for (int k = 0; k < kTraceInts; ++k) ints[k] = trace_int(s, es, w, key[0], key[1], key[2], k);
		const size_t row = static_cast<size_t>(t) * tv.frames + trace_slot(w, tv.frames);
		w += 1;
		if (!H2D(tv.vals + row * tv.W, vals.data(), sizeof(double) * vals.size()) || !H2D(tv.ints + row * kTraceInts, ints, sizeof(ints)) || !H2D(tv.written + t, &w, sizeof(w))) return false;
	}
	return true;
}
// The rings unrolled on the host, row by row: down from the ring, then into the destination -- with plain stores where it is page-locked memory, else up again.
bool Backend::TraceGather(const TraceView& tv, const int32_t* list, int n, int max_rows, int row_stride, double* vals_out, int32_t* ints_out, int32_t* counts, bool dst_host)
{
	if (n <= 0) return true;
	if (!SyncSelected()) return false;
	std::vector<double> vals(static_cast<size_t>(tv.W)); int32_t ints[kTraceInts];
	for (int i = 0; i < n; ++i) {
		const int32_t t = list[i];
		int64_t w = 0;
		if (!D2H(&w, tv.written + t, sizeof(w))) return false;
		const int32_t c = trace_count(w, tv.frames, max_rows);
		counts[i] = c;
		for (int32_t r = 0; r < c; ++r) {
			const size_t src = static_cast<size_t>(t) * tv.frames + trace_read_slot(w, c, r, tv.frames), dst = static_cast<size_t>(i) * row_stride + r;
			if (!D2H(vals.data(), tv.vals + src * tv.W, sizeof(double) * vals.size()) || !D2H(ints, tv.ints + src * kTraceInts, sizeof(ints))) return false;
			if (dst_host) { std::copy(vals.begin(), vals.end(), vals_out + dst * tv.W); std::copy(ints, ints + kTraceInts, ints_out + dst * kTraceInts); }
			else if (!H2D(vals_out + dst * tv.W, vals.data(), sizeof(double) * vals.size()) || !H2D(ints_out + dst * kTraceInts, ints, sizeof(ints))) return false;
		}
	}
	return true;
}
// Episode log: the rule (log_count / log_row / log_start) on the host, env by env in ascending env id, behind a wait for the selected stream: what the rule reads
// comes down by per-env copies, the record goes back where it moved; ring and cursor words are page-locked host memory and are written with plain stores, in the
// kernel's order (reservation, rows, boundary counter, cursor). The rows of a boundary are collected first: of more than `capacity` only the last are stored.
bool Backend::EpisodeLog(const EnvState* st, const EnvStatus* status, const EnvSpan& span, const LogView& v)
{
	std::vector<int32_t> list; bool done;
	if (!SpanOpen(*this, span, true, list, &done)) return done;
	LogRec r; int64_t num_cycles = 0;
	if (!status) {
		for (int32_t e : list) {
			if (!D2H(&r, v.recs + e, sizeof(r)) || !D2H(&num_cycles, &st[e].num_cycles, sizeof(num_cycles))) return false;
			log_start(r, num_cycles);
			if (!H2D(v.recs + e, &r, sizeof(r))) return false;
		}
		return true;
	}
	const int64_t written = v.cursor[0], boundary = v.cursor[1];
	std::vector<LogRow> rows;
	EnvStatus es; int32_t left = 0;
	for (int32_t e : list) {
		if (v.external) { if (!D2H(&left, &st[e].ext_steps_left, sizeof(left))) return false; if (left != 0) continue; }
		if (!D2H(&r, v.recs + e, sizeof(r)) || !D2H(&es, status + e, sizeof(es))) return false;
		if (!log_count(r, es, true)) { if (!H2D(&v.recs[e].frames, &r.frames, sizeof(r.frames))) return false; continue; }
		LogEnv le{0, 0, 0, 0, 0};
		uint8_t on = 0;
		if (v.episode) { if (!D2H(&on, v.episode_on + e, sizeof(on))) return false; if (on && !D2H(&le.limit_cause, &v.episode[e].last_cause, sizeof(int32_t))) return false; }
		if (v.env_slot && !D2H(&le.slot, v.env_slot + e, sizeof(int32_t))) return false;
		if (v.env_variant && !D2H(&le.variant, v.env_variant + e, sizeof(int32_t))) return false;
		if (v.env_terrain && !D2H(&le.terrain, v.env_terrain + e, sizeof(int32_t))) return false;
		if (v.rescale && !D2H(&le.rescale_episodes, &v.rescale[e].episodes, sizeof(int32_t))) return false;
		if (!D2H(&num_cycles, &st[e].num_cycles, sizeof(num_cycles))) return false;
		rows.push_back(log_row(r, es, num_cycles, boundary, le, v, e));
		if (!H2D(v.recs + e, &r, sizeof(r))) return false;
	}
	const int64_t total = static_cast<int64_t>(rows.size());
	if (total > 0) { v.cursor[2] = written + total; __atomic_thread_fence(__ATOMIC_SEQ_CST); }
	for (int64_t k = 0; k < total; ++k) if (log_row_kept(total, k, v.capacity)) v.ring[log_slot(written, k, v.capacity)] = rows[static_cast<size_t>(k)];
	__atomic_thread_fence(__ATOMIC_SEQ_CST);
	v.cursor[1] = boundary + 1; v.cursor[0] = written + total;
	return true;
}
// dtrl_add_perturb's rows, env by env: the whole EnvState down, the seven fields, the whole EnvState up (what Engine::AddPerturb did before there was a launch for it)
bool Backend::PerturbScatter(EnvState* st, const PerturbRow* rows, int n)
{
	if (n <= 0) return true;
	std::vector<PerturbRow> host(static_cast<size_t>(n));
	if (!D2H(host.data(), rows, sizeof(PerturbRow) * host.size())) return false;
	EnvState es;
	for (const PerturbRow& r : host) {
		if (!D2H(&es, st + r.env, sizeof(EnvState))) return false;
		perturb_write_slot(es, r);
		if (!H2D(st + r.env, &es, sizeof(EnvState))) return false;
	}
	return true;
}
// The terrain work: tg_env_boundary on the host, env by env, under the TerrainCfg the rule names -- the batch's own, the env's table entry, or the entry of the
// level the ladder's rule (tg_ladder_step) has just moved the env to; key and ladder record go back where they changed. A finished episode goes to the device
// distance ring as the kernel would have put it there (one cursor read at the start, one write at the end: nothing else runs on this stream meanwhile -- D2H
// waits for it).
bool Backend::TerrainBoundary(const DevBuffers& buf, const EnvSpan& span, int mode, const TerrainRule& rule)
{
	return rule.table ? TerrainBoundaryLoop(buf, span, mode, rule) : TerrainBoundary(buf, span.e0, span.n, mode, span.list);
}
bool Backend::TerrainBoundary(const DevBuffers& buf, int e0, int n, int mode, const int32_t* env_list) { return TerrainBoundaryLoop(buf, EnvSpan{e0, n, env_list}, mode, TerrainRule{}); }
bool Backend::TerrainBoundaryLoop(const DevBuffers& buf, const EnvSpan& span, int mode, const TerrainRule& rule)
{
	std::vector<int32_t> list; bool done;
	if (!SpanOpen(*this, span, false, list, &done)) return done;
	int32_t cursor = 0;
	if (buf.dist_ring && !D2H(&cursor, buf.dist_count, sizeof(cursor))) return false;
	const int32_t cursor0 = cursor;
	GroundRec rec; GroundGen gen; EnvStatus st; TerrainCfg cfg; int32_t key = 0;
	for (int32_t e : list) {
		if ((rule.table && !D2H(&key, rule.env_terrain + e, sizeof(key))) || !D2H(&st, buf.status + e, sizeof(st))) return false;
		if (rule.ladder) {
			LadderRec lr;
			if (!D2H(&lr, rule.ladder + e, sizeof(lr))) return false;
			const LadderRec lr0 = lr;
			const int32_t next = tg_ladder_step(lr, key, st, rule.lc, mode, e);
			if (next != key && !H2D(rule.env_terrain + e, &next, sizeof(next))) return false;
			if ((lr.mark_x != lr0.mark_x || lr.ups != lr0.ups || lr.downs != lr0.downs) && !H2D(rule.ladder + e, &lr, sizeof(lr))) return false;
			key = next;
		}
		if (!D2H(&cfg, rule.table ? rule.table + key : buf.tcfg, sizeof(cfg)) || !D2H(&gen, buf.gen + e, sizeof(gen)) || !D2H(&rec, buf.gr + e, sizeof(rec))) return false;
		const GroundGen gen0 = gen;
		DistRec one; int32_t got = 0;
		tg_env_boundary(rec, gen, st, cfg, mode, e, buf.dist_ring ? &one : nullptr, &got, 1);
		if (got > 0) { if (cursor < buf.dist_cap && !H2D(buf.dist_ring + cursor, &one, sizeof(one))) return false; ++cursor; }
		if (gen.builds == gen0.builds && gen.ctr == gen0.ctr && mode == 0) continue;   // the window stayed: nothing to write back
		if (!H2D(buf.gr + e, &rec, sizeof(rec)) || !H2D(buf.gen + e, &gen, sizeof(gen))) return false;
	}
	if (cursor != cursor0 && !H2D(buf.dist_count, &cursor, sizeof(cursor))) return false;
	return true;
}

}  // namespace dtrl
