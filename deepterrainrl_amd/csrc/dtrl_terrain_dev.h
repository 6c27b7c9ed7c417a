// On-device terrain: the sliding two-segment window of cGroundVar2D (sim/GroundVar2D.cpp:43-91 Update, :312-355 BuildSegment, :392-455 tSegment::Init)
// and the strip generator of cTerrainGen2D (dtrl_terrain_gen.h) run by the GPU at the frame boundary, one thread per env, straight into the env's
// GroundRec -- no status read-back, no per-env host loop, no upload. Same generator code as the host path; the random source is a counter-based
// stream per env instead of a libstdc++ engine (a std::default_random_engine + std::uniform_*_distribution cannot be reproduced bit-for-bit on the
// device without shipping libstdc++'s algorithms), so windows are equal IN DISTRIBUTION to the host mode's, deterministic, and shard-invariant.
// The window logic is a template over the random source: tests/terrain_dev instantiates it with the HOST stream and checks it record-for-record
// against GroundWindow.
#pragma once
#include "dtrl_types.h"
#include "dtrl_terrain_gen.h"

namespace dtrl {

// vertex container over one GroundRec slot
struct SegBuf {
	float* d; int n, cap; int overflow;
	DTRL_TG_HD size_t size() const { return static_cast<size_t>(n); }
	DTRL_TG_HD bool empty() const { return n == 0; }
	DTRL_TG_HD float back() const { return d[n - 1]; }
	DTRL_TG_HD void push_back(float v) { if (n < cap) d[n++] = v; else overflow = 1; }
	DTRL_TG_HD float& operator[](size_t i) { return d[i]; }
};

DTRL_TG_HD inline uint64_t tg_mix(uint64_t x)
{
	x += 0x9E3779B97F4A7C15ULL;
	x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
	x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
	return x ^ (x >> 31);
}
// the draws cTerrainGen2D makes (util/Rand.cpp: RandDouble / RandInt / FlipCoin / RandSign, degenerate ranges consume nothing), from a counter stream
struct CtrRand {
	uint64_t key; uint64_t* ctr;
	DTRL_TG_HD double u01() { const uint64_t z = tg_mix(key + (*ctr) * 0xD1342543DE82EF95ULL); ++(*ctr); return static_cast<double>(z >> 11) * (1.0 / 9007199254740992.0); }
	DTRL_TG_HD double RandDouble(double mn, double mx) { if (mn == mx) return mn; const double r = u01(); return mn + (r * (mx - mn)); }
	DTRL_TG_HD int RandInt(int mn, int mx) { if (mn == mx) return mn; const int r = mn + static_cast<int>(u01() * (mx - mn)); return r >= mx ? mx - 1 : r; }
	DTRL_TG_HD bool FlipCoin() { return RandDouble(0, 1) < 0.5; }
	DTRL_TG_HD int RandSign() { return FlipCoin() ? -1 : 1; }
};
DTRL_TG_HD inline uint64_t terrain_stream_key(uint64_t terrain_seed, int64_t global_env) { return tg_mix(tg_mix(terrain_seed) ^ (0x7E44A1ULL + static_cast<uint64_t>(global_env))); }

// cGroundVar2D::BuildSegment into logical slot `slot` of the record (0 = min segment, 1 = max segment)
template <class R>
DTRL_TG_HD inline void tg_build_segment(GroundRec& rec, int slot, double bmin, double bmax, bool align_min, double fix_y, const TerrainCfg& c, R& rnd, GroundGen* gen)
{
	SegBuf v{rec.data[slot], 0, kSegCap, 0};
	if (bmin <= 0 && bmax >= 0) { tgen::Strip<SegBuf> s(v); const double a = bmax - bmin, b = 1 - bmin; s.flat(a < b ? a : b); }   // flat padding around x = 0
	tgen::build_terrain(c.type, bmax - bmin, c.params, rnd, v);
	const int n = v.n;
	const float end_h = n > 0 ? (align_min ? v.d[0] : v.d[n - 1]) : 0.f;
	const float off = static_cast<float>(fix_y - end_h);
	for (int i = 0; i < n; ++i) v.d[i] += off;
	const double sp = static_cast<double>(tgen::kSpacing);
	const double min_x = align_min ? bmin : (bmax - (n - 1) * sp);
	const double max_x = min_x + (n - 1) * sp;
	const double centre = 0.5 * (min_x + max_x);
	const float bt_origin = static_cast<float>(c.world_scale) * static_cast<float>(centre);       // tSegment::Init: Bullet keeps float origins / scalings
	rec.origin_x[slot] = static_cast<double>(bt_origin) / c.world_scale;
	rec.scale_x[slot] = static_cast<double>(static_cast<float>(sp * c.world_scale)) / c.world_scale;
	rec.min_x[slot] = min_x; rec.max_x[slot] = max_x; rec.w[slot] = n;
	if (gen) { gen->builds += 1; gen->overflow += v.overflow; }
}
DTRL_TG_HD inline void tg_copy_slot(GroundRec& rec, int dst, int src)
{
	rec.origin_x[dst] = rec.origin_x[src]; rec.scale_x[dst] = rec.scale_x[src]; rec.min_x[dst] = rec.min_x[src]; rec.max_x[dst] = rec.max_x[src]; rec.w[dst] = rec.w[src];
	for (int i = 0; i < rec.w[src]; ++i) rec.data[dst][i] = rec.data[src][i];
}
// cGroundVar2D::InitSegments after Clear(): [mid - w, mid] ending at height 0, then [mid, mid + w] starting at height 0 (this draw order)
template <class R>
DTRL_TG_HD inline void tg_init_segments(GroundRec& rec, double bmin, double bmax, const TerrainCfg& c, R& rnd, GroundGen* gen)
{
	const double mid = 0.5 * (bmax + bmin), w = c.segment_width;
	tg_build_segment(rec, 0, -w + mid, mid, false, 0.0, c, rnd, gen);
	tg_build_segment(rec, 1, mid, w + mid, true, 0.0, c, rnd, gen);
}
// cGroundVar2D::Update: slide the window so that it covers [bmin, bmax]; the record stays in logical order (the reference flips a segment index)
template <class R>
DTRL_TG_HD inline bool tg_window_update(GroundRec& rec, double bmin, double bmax, const TerrainCfg& c, R& rnd, GroundGen* gen)
{
	const double min_x = rec.min_x[0], max_x = rec.max_x[1];
	if (bmax < max_x && bmin > min_x) return false;
	if (bmax <= min_x || bmin >= max_x) { tg_init_segments(rec, bmin, bmax, c, rnd, gen); return true; }
	if (bmax >= max_x) {
		const double fix_y = rec.data[1][rec.w[1] - 1];
		tg_copy_slot(rec, 0, 1);
		tg_build_segment(rec, 1, max_x, max_x + c.segment_width, true, fix_y, c, rnd, gen);
	} else {
		const double fix_y = rec.data[0][0];
		tg_copy_slot(rec, 1, 0);
		tg_build_segment(rec, 0, min_x - c.segment_width, min_x, false, fix_y, c, rnd, gen);
	}
	return true;
}

// the frame-boundary work of one env: what Engine::HostFrameWork does on the host in the default mode.
//   mode 0: after a frame -- a fallen env (status.need_reset) gets a fresh window around the spawn point (cScenarioSimChar::ResetGround: Clear + Update),
//           any other env has its window slid along with the character; a finished poli_eval episode (bit 1) is appended to the distance log
//   mode 1: (re)initialise unconditionally (Init, user resets)
//   mode 2: re-seed + initialise (dtrl_assign_terrains with restart): the env's stream starts over at its key (the host has written it: terrain seed + GLOBAL
//           env id), the build count goes to 0, then as mode 1 -- the env's window is what creation would have built under this terrain
// (always inlined on the device: with two kernels calling it -- dtrl_terrain_boundary and dtrl_terrain_boundary_keyed -- the compiler would otherwise keep ONE copy
// behind a call, and the shipped kernel would get a stack frame and the callee's register count; inlined, each kernel is compiled as the shipped one always was)
#if defined(__HIPCC__)
__attribute__((always_inline))
#endif
DTRL_TG_HD inline void tg_env_boundary(GroundRec& rec, GroundGen& gen, const EnvStatus& st, const TerrainCfg& c, int mode, int env, DistRec* dist_ring, int32_t* dist_count, int32_t dist_cap)
{
	CtrRand rnd{gen.key, &gen.ctr};
	if (mode == 2) { gen.ctr = 0; gen.builds = 0; gen.overflow = 0; }   // (the stream reads its counter through the pointer: it starts over)
	if (mode == 1 || mode == 2) { tg_init_segments(rec, c.spawn_min, c.spawn_max, c, rnd, &gen); return; }
	if (st.need_reset & 2) {
		if (dist_ring) {
#if defined(__HIP_DEVICE_COMPILE__)
			const int32_t k = atomicAdd(dist_count, 1);
#else
			const int32_t k = (*dist_count)++;
#endif
			if (k < dist_cap) { dist_ring[k].env = env; dist_ring[k].dist = st.episode_dist; }
		}
	}
	if (st.need_reset) tg_init_segments(rec, c.spawn_min, c.spawn_max, c, rnd, &gen);
	else tg_window_update(rec, st.root_x + c.view_min, st.root_x + c.view_max, c, rnd, &gen);
}

// ---- env span: which envs a per-env rule runs over at a frame boundary ----
// envs [e0, e0 + n), or list[0 .. n) when a list is given (device memory for a kernel and for Backend's entries; local env ids)
struct EnvSpan { int e0, n; const int32_t* list; };
// the env of thread or iteration k of a span: false (env untouched) when k is beyond it. Takes the span as the three scalars the kernels have as arguments and is
// always inlined on the device, so a kernel that opens with it is compiled as when it spelled the three lines out
#if defined(__HIPCC__)
__attribute__((always_inline))
#endif
DTRL_TG_HD inline bool span_env(int k, int e0, int n, const int32_t* env_list, int& env)
{
	if (k >= n) return false;
	env = env_list ? env_list[k] : e0 + k;
	return true;
}

// ---- terrain ladder (include/dtrl.h dtrl_terrain_ladder): envs climb and descend a range of the terrain set by their episodes ----
// per-env record: the root x at which the env last spawned or last changed level, and how often it went up / down
struct LadderRec { double mark_x; int32_t ups, downs; };
// the batch's ladder: terrains [lo, hi] ordered easy to hard, the distances, what happens at the top, and what the rule needs besides (the x a reset leaves in
// q[0], the terrain seed and the env-id base of the at_top draw). A kernel ARGUMENT, like the table and the key array: DevBuffers keeps its layout
struct LadderCfg {
	int32_t lo, hi, at_top, pad_;
	double up_dist, down_dist, spawn_x;
	uint64_t seed; int64_t env_id_base;
};
// the at_top draw: counter-based like the terrain streams, a function of (terrain seed, GLOBAL env id, moves so far) only -- shard-invariant
DTRL_TG_HD inline uint64_t ladder_draw(uint64_t terrain_seed, int64_t global_env, int32_t moves)
{
	return tg_mix(tg_mix(tg_mix(terrain_seed) ^ (0x1ADDE2ULL + static_cast<uint64_t>(global_env))) + static_cast<uint64_t>(moves) * 0xD1342543DE82EF95ULL);
}
// The rule, the one body of host and device: the level of env `env` (local id) after its frame boundary, given its level k in front of it. Runs IN FRONT OF the
// env's terrain work (tg_env_boundary, GroundWindow::Clear / Update), so the window built or slid in the same boundary is the new level's. An env whose level is
// outside [lo, hi] is not on the ladder: nothing happens. Modes as tg_env_boundary's: 0 = after a frame, 1 / 2 = (re)initialise (the level stays, the mark goes
// to the spawn point). Every comparison in double; no exploration, no reward, no episode_dist, no other env.
DTRL_TG_HD inline int32_t tg_ladder_step(LadderRec& lr, int32_t k, const EnvStatus& st, const LadderCfg& lc, int mode, int env)
{
	if (k < lc.lo || k > lc.hi) return k;
	if (mode != 0) { lr.mark_x = lc.spawn_x; return k; }
	if (st.need_reset) {   // the episode ended: early falls go down
		if (st.root_x - lr.mark_x < lc.down_dist && k > lc.lo) { k -= 1; lr.downs += 1; }
		lr.mark_x = lc.spawn_x;
	} else if (st.root_x - lr.mark_x >= lc.up_dist) {
		if (k < lc.hi) { k += 1; lr.ups += 1; }
		else if (lc.at_top == 1) {
			const uint64_t draw = ladder_draw(lc.seed, lc.env_id_base + env, lr.ups + lr.downs);
			k = lc.lo + static_cast<int32_t>(draw % static_cast<uint64_t>(lc.hi - lc.lo + 1));
			lr.ups += 1;
		}
		lr.mark_x = st.root_x;
	}
	return k;
}

// ---- variant redraw (include/dtrl.h dtrl_variant_redraw): envs draw a new model variant at each episode start ----
// per-env record: how many draws the env has made (the counter of its draw stream)
struct RedrawRec { int32_t draws; };
// the batch's redraw: variants [lo, hi], the draw's seed and env-id base, and the cumulative weight table cum[hi - lo + 1] (ascending, last entry exactly 1.0;
// device memory for the kernel and the backend default, host memory for the engine's own loops). A kernel ARGUMENT: DevBuffers and RunParams keep their layout
struct RedrawCfg {
	int32_t lo, hi;
	uint64_t seed; int64_t env_id_base;
	const double* cum;
};
// counter-based like ladder_draw, under a constant of its own: a function of (seed, GLOBAL env id, the env's draws so far) only -- shard-invariant
DTRL_TG_HD inline uint64_t redraw_bits(uint64_t seed, int64_t global_env, int32_t draws)
{
	return tg_mix(tg_mix(tg_mix(seed) ^ (0x5EDBA77ULL + static_cast<uint64_t>(global_env))) + static_cast<uint64_t>(draws) * 0xD1342543DE82EF95ULL);
}
// The rule, the one body of host and device: the variant of env `env` (local id) after an episode start, given its variant k in front of it. `start`: the env is
// at an episode start (a frame boundary with need_reset & 1, or dtrl_reset naming it). Runs IN FRONT OF the reset launch, so reset_env runs under the new model.
// An env whose variant is outside [lo, hi] is not in the redraw: nothing of it is touched. `cum` is c.cum as the caller can read it. Doubles and integers only.
DTRL_TG_HD inline int32_t var_redraw_step(RedrawRec& r, int32_t k, bool start, const RedrawCfg& c, const double* cum, int env)
{
	if (!start || k < c.lo || k > c.hi) return k;
	const double u = static_cast<double>(redraw_bits(c.seed, c.env_id_base + env, r.draws) >> 11) * (1.0 / 9007199254740992.0);
	int32_t a = 0, b = c.hi - c.lo + 1;   // #{ j : cum[j] <= u } by binary search
	while (a < b) { const int32_t mid = (a + b) >> 1; if (cum[mid] <= u) a = mid + 1; else b = mid; }
	r.draws += 1;
	const int32_t next = c.lo + a;
	return next > c.hi ? c.hi : next;
}

// ---- variant rescale (include/dtrl.h dtrl_variant_rescale): envs under a private model record draw continuous mass and motor scales at each episode start ----
// per-env record: how many episodes the env has started under the rescale (the episode number of its draw stream)
struct RescaleRec { int32_t episodes; };
// the batch's rescale: the four ranges [lo[q], hi[q]] (0 < lo <= hi, finite) of q = 0 mass, 1 kp, 2 kd, 3 torque_lim, the per_link mask (bit q: quantity q draws
// one factor per link, else one for all links), the link count, the stream's seed and env-id base. A kernel ARGUMENT: DevBuffers and RunParams keep their layout
enum RescaleQuantity { kRescaleMass = 0, kRescaleKp = 1, kRescaleKd = 2, kRescaleTorqueLim = 3, kRescaleQuantities = 4 };
struct RescaleCfg {
	double lo[kRescaleQuantities], hi[kRescaleQuantities];
	uint32_t per_link; int32_t L;
	uint64_t seed; int64_t env_id_base;
};
// counter-based like the other rules, under a constant of its own: a function of (seed, GLOBAL env id) -- shard-invariant
DTRL_TG_HD inline uint64_t rescale_stream_key(uint64_t seed, int64_t global_env) { return tg_mix(tg_mix(seed) ^ (0x5CA1EDULL + static_cast<uint64_t>(global_env))); }
// factor of quantity q for link j in the env's episode n. The index layout n * 4 L + q L + j is fixed, and a quantity that is not per link reads index j = 0 for
// every link: switching one quantity between the two forms moves no other quantity's draws
DTRL_TG_HD inline double rescale_factor(const RescaleCfg& c, uint64_t key, int32_t n, int q, int j)
{
	const uint64_t L = static_cast<uint64_t>(c.L);
	const uint64_t idx = static_cast<uint64_t>(n) * 4u * L + static_cast<uint64_t>(q) * L + (((c.per_link >> q) & 1u) ? static_cast<uint64_t>(j) : 0u);
	const double u = static_cast<double>(tg_mix(key + idx * 0xD1342543DE82EF95ULL) >> 11) * (1.0 / 9007199254740992.0);
	return c.lo[q] + u * (c.hi[q] - c.lo[q]);
}
// what the rule writes for one link from its own draws: the loader's formulas (dtrl_host.cpp LoadScenario), operation by operation, on the character file's
// doubles times the factor -- doubles until the one cast to `real`
struct RescaleLink { real mass, inertia, kp, kd, torque_lim; };
DTRL_TG_HD inline RescaleLink rescale_link(const RescaleCfg& c, uint64_t key, int32_t n, const ModelScalarsD& b, int j)
{
	RescaleLink o;
	o.mass = static_cast<real>(b.m0[j] * rescale_factor(c, key, n, kRescaleMass, j));
	o.inertia = static_cast<real>(o.mass / 12.0 * b.s2[j]);
	o.kp = static_cast<real>(b.kp[j] * rescale_factor(c, key, n, kRescaleKp, j));
	o.kd = static_cast<real>(b.kd[j] * rescale_factor(c, key, n, kRescaleKd, j));
	o.torque_lim = static_cast<real>(b.torque_lim[j] * rescale_factor(c, key, n, kRescaleTorqueLim, j));
	return o;
}
// The rule, the one body of host and device (the kernel runs rescale_link on its lanes and takes the two sums below by lane broadcasts in the same order): env
// `env` (local id) at a frame boundary or under dtrl_reset. `start`: the env is at an episode start; `is_private`: its key is its private record's. Otherwise
// nothing is touched. Rewrites mass, total_mass (running sum in link order, in `real`), inertia, sub_mass (double sum over the bits of sub_mask in ascending
// order, cast once), kp, kd and torque_lim of the env's private record `m` -- geometry, margins, contact points and limits do not move -- and counts the episode.
// Runs IN FRONT OF the reset launch, so reset_env runs under the new scales. true: the record was rewritten.
DTRL_TG_HD inline bool rescale_step(RescaleRec& r, bool start, bool is_private, const RescaleCfg& c, const ModelScalarsD& b, int env, DevModel& m)
{
	if (!start || !is_private) return false;
	const uint64_t key = rescale_stream_key(c.seed, c.env_id_base + env);
	m.total_mass = 0;
	for (int j = 0; j < c.L; ++j) {
		const RescaleLink o = rescale_link(c, key, r.episodes, b, j);
		m.mass[j] = o.mass; m.total_mass += m.mass[j];
		m.inertia[j] = o.inertia; m.kp[j] = o.kp; m.kd[j] = o.kd; m.torque_lim[j] = o.torque_lim;
	}
	for (int j = 0; j < c.L; ++j) { double sm = 0; for (int k = 0; k < c.L; ++k) if ((m.sub_mask[j] >> k) & 1u) sm += m.mass[k]; m.sub_mass[j] = static_cast<real>(sm); }
	r.episodes += 1;
	return true;
}

// ---- push schedule (include/dtrl.h dtrl_push_schedule): random external pushes at per-env random times, written into the env's perturbation slot ----
// per-env record: frame boundaries left until the env's next push, the counter of its draw stream, how many pushes it got, and the last one as it was drawn
// (force and duration in double, before the cast to `real` with which they are stored into EnvState)
struct PushRec { int32_t wait; uint32_t ctr; int32_t pushes, last_link; double last_f[2]; double last_dur; };
// the batch's schedule: the wait between two pushes of an env in frame boundaries (1 <= min_wait <= max_wait), the ranges of force magnitude and duration, the
// stream's seed and env-id base, and the link count the link draw runs over. A kernel ARGUMENT: DevBuffers and RunParams keep their layout
struct PushCfg {
	int32_t min_wait, max_wait;
	double min_force, max_force, min_dur, max_dur;
	uint64_t seed; int64_t env_id_base;
	int32_t L, pad_;
};
// what a push puts into the slot (Engine::AddPerturb's fields for a push at the link's COM: the rest of the slot is zero)
struct PushOut { int32_t link; double f[2]; double dur; };
// counter-based like ladder_draw and redraw_bits, under a constant of its own: a function of (seed, GLOBAL env id) -- shard-invariant
DTRL_TG_HD inline uint64_t push_stream_key(uint64_t seed, int64_t global_env) { return tg_mix(tg_mix(seed) ^ (0x9054ED1ULL + static_cast<uint64_t>(global_env))); }
DTRL_TG_HD inline double push_u01(uint64_t key, PushRec& r)
{
	const uint64_t z = tg_mix(key + static_cast<uint64_t>(r.ctr) * 0xD1342543DE82EF95ULL);
	r.ctr += 1;
	return static_cast<double>(z >> 11) * (1.0 / 9007199254740992.0);
}
DTRL_TG_HD inline int32_t push_draw_wait(uint64_t key, PushRec& r, const PushCfg& c)
{
	const int32_t w = c.min_wait + static_cast<int32_t>(push_u01(key, r) * static_cast<double>(c.max_wait - c.min_wait + 1));
	return w > c.max_wait ? c.max_wait : w;
}
// The rule, the one body of host and device: env `env` (local id) at its frame boundary. `start`: an episode of the env starts in this boundary (it fell:
// status.need_reset != 0; creation of the schedule; dtrl_reset naming it; a terrain restart) -- the wait is drawn afresh and no push happens, so the rule does not
// depend on whether it runs in front of or behind the reset launch that clears the slot. Otherwise the wait counts down, and at 0 a push is drawn in the order
// Engine::ApplyRandForce draws (link, three (sign, magnitude) pairs, force magnitude, duration), returned in `out` (true: the caller writes the slot), recorded,
// and the next wait is drawn. scale == 0: the env is not in the schedule, nothing of it is touched. Doubles and integers only; every product, sum, divide and
// square root below is a single correctly rounded operation (the sources are compiled without contraction), so host and device give the same bits.
DTRL_TG_HD inline bool push_step(PushRec& r, double scale, bool start, const PushCfg& c, int env, PushOut& out)
{
	if (scale == 0) return false;
	const uint64_t key = push_stream_key(c.seed, c.env_id_base + env);
	if (start) { r.wait = push_draw_wait(key, r, c); return false; }
	r.wait -= 1;
	if (r.wait > 0) return false;
	int32_t link = static_cast<int32_t>(push_u01(key, r) * static_cast<double>(c.L));
	if (link >= c.L) link = c.L - 1;
	double d[3];
	for (int k = 0; k < 3; ++k) { const double sgn = push_u01(key, r) < 0.5 ? -1.0 : 1.0; d[k] = sgn * push_u01(key, r); }
	double nrm = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
	if (nrm == 0) { d[0] = 1; nrm = 1; }
	const double mag = scale * (c.min_force + push_u01(key, r) * (c.max_force - c.min_force));
	out.link = link;
	out.f[0] = mag * d[0] / nrm; out.f[1] = mag * d[1] / nrm;
	out.dur = c.min_dur + push_u01(key, r) * (c.max_dur - c.min_dur);
	r.last_link = link; r.last_f[0] = out.f[0]; r.last_f[1] = out.f[1]; r.last_dur = out.dur;
	r.pushes += 1;
	r.wait = push_draw_wait(key, r, c);
	return true;
}
// the slot as Engine::AddPerturb writes it for a push at the link's COM (values cast to `real` here and nowhere else)
DTRL_TG_HD inline void push_write_slot(EnvState& st, const PushOut& p)
{
	st.pert_link = p.link; st.pert_on = 0;
	st.pert_lp[0] = 0; st.pert_lp[1] = 0;
	st.pert_f[0] = static_cast<real>(p.f[0]); st.pert_f[1] = static_cast<real>(p.f[1]);
	st.pert_torque = 0; st.pert_time = 0; st.pert_dur = static_cast<real>(p.dur);
}
// ---- episode limit (include/dtrl.h dtrl_episode_limit): an env's episode ends after a per-episode drawn number of frame boundaries, or at a distance ----
// per-env record: boundaries the running episode has seen, the limit drawn for it (0: none), the counter of the env's draw stream, the last episode that ended
// (its length in boundaries, root_x - spawn_x at its end, cause 1 = fall, 2 = frame limit, 3 = distance; 0 = none yet) and how many ended by a fall / by a limit.
// 48 bytes on a 16-byte boundary: a thread moves its record as three 16-byte words; what moves at a boundary that ends nothing is the first word alone
struct alignas(16) EpisodeRec { int32_t frames, limit, draws, last_frames, last_cause, pad_; int64_t by_fall, by_limit; double last_dist; };
static_assert(sizeof(EpisodeRec) == 48, "EpisodeRec is three 16-byte words");
enum EpisodeCause { kEpisodeRuns = 0, kEpisodeFall = 1, kEpisodeFrames = 2, kEpisodeDist = 3 };
// the batch's limit: the range the per-episode frame limit is drawn from (both 0: no frame limit), the distance (+inf: none), the x a reset leaves in q[0], the
// stream's seed and env-id base, and whether the scenario is poli_eval (episode_end). A kernel ARGUMENT: DevBuffers and RunParams keep their layout
struct EpisodeCfg {
	int32_t min_frames, max_frames;
	double max_dist, spawn_x;
	uint64_t seed; int64_t env_id_base;
	int32_t poli_eval, pad_;
};
// counter-based like the other rules, under a constant of its own: a function of (seed, GLOBAL env id, the env's draws so far) -- shard-invariant
DTRL_TG_HD inline uint64_t episode_stream_key(uint64_t seed, int64_t global_env) { return tg_mix(tg_mix(seed) ^ (0xE9150DEULL + static_cast<uint64_t>(global_env))); }
DTRL_TG_HD inline void episode_draw_limit(EpisodeRec& r, const EpisodeCfg& c, int env)
{
	if (c.max_frames == 0) { r.limit = 0; return; }   // no frame limit: nothing is drawn
	const uint64_t key = episode_stream_key(c.seed, c.env_id_base + env);
	const uint64_t z = tg_mix(key + static_cast<uint64_t>(r.draws) * 0xD1342543DE82EF95ULL);
	r.draws += 1;
	const double u = static_cast<double>(z >> 11) * (1.0 / 9007199254740992.0);
	const int32_t l = c.min_frames + static_cast<int32_t>(u * static_cast<double>(c.max_frames - c.min_frames + 1));
	r.limit = l > c.max_frames ? c.max_frames : l;
}
// The rule, the one body of host and device: env `env` (local id, not held out) at its frame boundary, given its status record as the frame kernel left it;
// status == nullptr: an episode of the env starts without a boundary (the limit is set; dtrl_reset names the env; a terrain restart). Runs IN FRONT OF every other
// boundary rule. Returns the cause for which the CALLER ends the env's episode (kEpisodeFrames, kEpisodeDist: episode_end below), else kEpisodeRuns -- also for an
// env that fell, whose episode the frame kernel has ended already; a fall wins over a limit reached in the same frame. Doubles and integers only.
DTRL_TG_HD inline int32_t episode_limit_step(EpisodeRec& r, const EnvStatus* status, const EpisodeCfg& c, int env)
{
	if (!status) { r.frames = 0; episode_draw_limit(r, c, env); return kEpisodeRuns; }
	r.frames += 1;
	const double dist = status->root_x - c.spawn_x;
	int32_t cause = kEpisodeRuns;
	if (status->need_reset != 0) cause = kEpisodeFall;
	else if (r.limit > 0 && r.frames >= r.limit) cause = kEpisodeFrames;
	else if (dist >= c.max_dist) cause = kEpisodeDist;
	if (cause == kEpisodeRuns) return cause;
	if (cause == kEpisodeFall) r.by_fall += 1; else r.by_limit += 1;
	r.last_frames = r.frames; r.last_dist = dist; r.last_cause = cause;
	r.frames = 0;
	episode_draw_limit(r, c, env);
	return cause == kEpisodeFall ? static_cast<int32_t>(kEpisodeRuns) : cause;
}
// What the caller of the rule does for an env whose episode the rule ended: frame_end()'s writes for a fall (dtrl_kernel.h), operation by operation in `real`,
// without scenario_new_cycle -- no tuple is recorded, the one in progress is dropped by the reset. Reads q[0], pos_start_x, avg_dist, num_episodes and
// num_cycles of the env's state; writes its avg_dist, num_episodes and need_reset, and need_reset / episode_dist of its status record.
DTRL_TG_HD inline void episode_end(EnvState& st, EnvStatus& es, const EpisodeCfg& c)
{
	int32_t need = 1;
	if (c.poli_eval && st.num_cycles >= 1) {
		real dist = st.q[0] - st.pos_start_x;
		st.avg_dist = (st.num_episodes * st.avg_dist + dist) / (st.num_episodes + 1.0);
		st.num_episodes += 1;
		es.episode_dist = dist; need = 3;
	}
	st.need_reset = need; es.need_reset = need;
}

// ---- frame trace (include/dtrl.h dtrl_trace): a ring of per-frame state rows of chosen envs, written behind the frame and in front of every rule that resets ----
// A traced env has an index t (its place in the caller's list): env_of[t] is its local env id, its ring is rows [t * frames, (t + 1) * frames) of `vals`
// (W = 3 D + 2 doubles a row) and `ints` (kTraceInts int32 a row), and written[t] counts the rows it has written since the trace was set -- one counter per env,
// so the groups' streams need no common frame number. The three key arrays are the families' device arrays (nullptr: the family has no table, the key reads 0).
// A kernel ARGUMENT: DevBuffers and RunParams keep their layout
constexpr int kTraceInts = 12;
enum TraceInt { kTraceRow = 0, kTraceNeedReset, kTraceActionId, kTraceState, kTraceStance, kTraceContactBits, kTraceNumCycles, kTraceNumResets, kTraceSlot, kTraceVariant, kTraceTerrain, kTraceReserved };
struct TraceView {
	double* vals; int32_t* ints; int64_t* written;
	const int32_t* env_of;
	const int32_t* env_slot; const int32_t* env_variant; const int32_t* env_terrain;
	int32_t frames, D, W, n_traced;
};
// The rule, the one body of host and device. trace_due: the env completed a frame in the launch in front of the rule (external policy mode: a parked env has
// env-steps of its frame left and writes nothing; internal mode: the counter is always 0)
DTRL_TG_HD inline bool trace_due(const EnvState& s) { return s.ext_steps_left == 0; }
// word k < W of the row's value part: time, phase, q[D], qd[D], tau[D], each `real` converted to double exactly as the getters convert it
DTRL_TG_HD inline double trace_value(const EnvState& s, int D, int k)
{
	if (k < 2) return static_cast<double>(k == 0 ? s.time : s.phase);
	const int j = k - 2;
	return static_cast<double>(j < D ? s.q[j] : (j < 2 * D ? s.qd[j - D] : s.tau[j - 2 * D]));
}
// word k < kTraceInts of the row's integer part; `row` = the env's counter in front of the write
DTRL_TG_HD inline int32_t trace_int(const EnvState& s, const EnvStatus& es, int64_t row, int32_t slot, int32_t variant, int32_t terrain, int k)
{
	switch (k) {
	case kTraceRow: return static_cast<int32_t>(row);
	case kTraceNeedReset: return es.need_reset;
	case kTraceActionId: return s.action_id;
	case kTraceState: return s.state;
	case kTraceStance: return s.stance;
	case kTraceContactBits: return static_cast<int32_t>(s.contact_bits);
	case kTraceNumCycles: return static_cast<int32_t>(s.num_cycles);
	case kTraceNumResets: return static_cast<int32_t>(s.num_resets);
	case kTraceSlot: return slot;
	case kTraceVariant: return variant;
	case kTraceTerrain: return terrain;
	default: return 0;
	}
}
// ring slot of the row an env writes next, and where the r-th of the last `count` rows sits (chronological read-out: oldest first)
DTRL_TG_HD inline int32_t trace_slot(int64_t written, int32_t frames) { return static_cast<int32_t>(written % frames); }
DTRL_TG_HD inline int32_t trace_count(int64_t written, int32_t frames, int32_t max_rows) { const int64_t c = written < frames ? written : frames; return static_cast<int32_t>(c < max_rows ? c : max_rows); }
DTRL_TG_HD inline int32_t trace_read_slot(int64_t written, int32_t count, int32_t r, int32_t frames) { return static_cast<int32_t>((written - count + r) % frames); }

// ---- episode log (include/dtrl.h dtrl_episode_log): one compact row per ended episode, written at the frame boundary in front of every rule that moves a key ----
// per-env record (device memory, the only copy): boundaries the running episode has seen, the episodes of this env logged since the log was set, and
// EnvState::num_cycles at the episode's start. 32 bytes on a 16-byte boundary: word 0 {frames, episodes}, word 1 {cycles0}; a boundary that ends nothing stores
// the frame count alone
struct alignas(16) LogRec { int32_t frames, pad_; int64_t episodes; int64_t cycles0, pad2_; };
static_assert(sizeof(LogRec) == 32, "LogRec is two 16-byte words");
// a row: 64 bytes as four 16-byte words (the layout of dtrl_episode_row, include/dtrl.h; dtrl_c_api.cpp holds the two to each other)
struct alignas(16) LogRow {
	int32_t env, cause, frames, cycles;                 // local env id; 1 fall, 2 frame limit, 3 distance; boundaries the episode saw; num_cycles - cycles0
	int64_t boundary, episode;                          // the group's boundary counter at which the episode ended (0-based since the log was set); the env's ordinal
	double dist; int32_t need_reset, zero_;             // status.root_x - spawn_x; the status record's need_reset as every later rule sees it
	int32_t slot, variant, terrain, rescale_draw;       // the keys as the device holds them (0 without a table; a private rescale key reads V + e); the draw n of the episode's factors, or -1
};
static_assert(sizeof(LogRow) == 64, "LogRow is four 16-byte words");
// one env group's ring and cursor words {written, boundary, reserved, 0} (page-locked host memory the device writes; reserved = written + the rows of the
// boundary being written, stored in FRONT of its first row: written <= reserved, and a slot of index i is being overwritten only once reserved > i + capacity), and what the rule reads beside state and status: the
// limit's records and flags (nullptr: no limit in force, every cause is a fall), the three key arrays (nullptr: the family has no table, the key reads 0), the
// rescale's counters with the first private key V (nullptr: no rescale, the draw reads -1). A kernel ARGUMENT: DevBuffers and RunParams keep their layout
struct LogView {
	LogRec* recs; LogRow* ring; int64_t* cursor;
	const EpisodeRec* episode; const uint8_t* episode_on;
	const int32_t* env_slot; const int32_t* env_variant; const int32_t* env_terrain;
	const RescaleRec* rescale;
	double spawn_x;
	int32_t capacity, private_base, external, pad_;   // private_base: V, the key of env 0's private rescale record (with `rescale`); external: -policy_mode= external
};
// what a row takes from the arrays above, loaded by whoever runs the rule (the kernel from device memory, the host default by copies): EpisodeRec::last_cause of an
// env under a limit (else 0), the three keys, RescaleRec::episodes (0 without a rescale)
struct LogEnv { int32_t limit_cause, slot, variant, terrain, rescale_episodes; };
// The rule, the one body of host and device. log_count: env at a frame boundary -- `due`: it completed a frame in the launch in front of the rule (trace_due; read
// in external policy mode only) -- counts the boundary; true: its episode ended and the caller appends log_row. Doubles and integers only.
DTRL_TG_HD inline bool log_count(LogRec& r, const EnvStatus& es, bool due)
{
	if (!due) return false;
	r.frames += 1;
	return es.need_reset != 0;
}
// the row of the episode that ended at `boundary`, from the env's status record, its cycle counter and `k` as they stand IN FRONT OF every rule that moves a key
// or redraws a scale; the record then starts the next episode. The cause of an env under a limit is the one the limit rule recorded just in front of this rule on
// the same stream; without a limit every episode ends by a fall
DTRL_TG_HD inline LogRow log_row(LogRec& r, const EnvStatus& es, int64_t num_cycles, int64_t boundary, const LogEnv& k, const LogView& v, int env)
{
	LogRow o;
	o.env = env;
	o.cause = k.limit_cause != 0 ? k.limit_cause : static_cast<int32_t>(kEpisodeFall);
	o.frames = r.frames; o.cycles = static_cast<int32_t>(num_cycles - r.cycles0);
	o.boundary = boundary; o.episode = r.episodes;
	o.dist = es.root_x - v.spawn_x; o.need_reset = es.need_reset; o.zero_ = 0;
	o.slot = k.slot; o.variant = k.variant; o.terrain = k.terrain;
	o.rescale_draw = (v.rescale && k.variant == v.private_base + env) ? k.rescale_episodes - 1 : -1;
	r.frames = 0; r.episodes += 1; r.cycles0 = num_cycles;
	return o;
}
// a listed episode start (dtrl_reset, a terrain restart; the log is set): the running episode is abandoned without a row
DTRL_TG_HD inline void log_start(LogRec& r, int64_t num_cycles) { r.frames = 0; r.cycles0 = num_cycles; }
// of `total` rows appended in one boundary behind `written` earlier ones, the k-th is stored only if it is among the last `capacity` (no two rows of one launch
// share a slot), at slot (written + k) % capacity
DTRL_TG_HD inline bool log_row_kept(int64_t total, int64_t k, int32_t capacity) { return k >= total - capacity; }
DTRL_TG_HD inline int32_t log_slot(int64_t written, int64_t k, int32_t capacity) { return static_cast<int32_t>((written + k) % capacity); }

// one row of dtrl_add_perturb as the engine uploads it (Backend::PerturbScatter): the rotated offset is the host's, bit for bit
struct PerturbRow { int32_t env, link; real f[2], lp[2], dur; };
DTRL_TG_HD inline void perturb_write_slot(EnvState& st, const PerturbRow& r)
{
	st.pert_link = r.link; st.pert_on = 0;
	st.pert_lp[0] = r.lp[0]; st.pert_lp[1] = r.lp[1];
	st.pert_f[0] = r.f[0]; st.pert_f[1] = r.f[1];
	st.pert_torque = 0; st.pert_time = 0; st.pert_dur = r.dur;
}

}  // namespace dtrl
