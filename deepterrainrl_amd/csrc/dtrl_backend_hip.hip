// dtrl_backend_hip.hip -- the product backend: the HIP runtime behind the Backend interface (streams, events, copies) and every auxiliary kernel. The frame
// kernels are launched from here and compiled elsewhere, one translation unit per family (dtrl_frame_entry.h: dtrl_backend_hip_frame.hip, _ext.hip, _slots.hip, _variants.hip),
// so that what changes here cannot change their instructions.
#include "dtrl_engine.h"
#include "dtrl_frame_entry.h"
#include "dtrl_terrain_dev.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <thread>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

namespace dtrl {

// ---- external policy mode: the hand-over kernels (include/dtrl.h dtrl_pending_actions* / dtrl_supply_actions*) ----
// dtrl_ext_collect: ids[0 .. m) = the awaiting envs in ascending env id, m = min(#awaiting, cap). One workgroup; thread t owns the contiguous env range
// [t c, (t + 1) c): it counts its awaiting envs, the counts are scanned across the workgroup (wave shuffles + one LDS level), and it writes its ids behind the
// ranges in front of it -- a deterministic compaction, no atomic cursor. meta (page-locked): {m, #awaiting, #ready, 0}.
constexpr int kExtThreads = 1024;
__global__ void __launch_bounds__(kExtThreads) dtrl_ext_collect(const EnvState* __restrict__ st, int n_envs, int cap, int32_t* __restrict__ ids, int32_t* __restrict__ meta)
{
	__shared__ int part_a[kExtThreads / 64], part_r[kExtThreads / 64];
	const int t = static_cast<int>(threadIdx.x);
	const int chunk = (n_envs + kExtThreads - 1) / kExtThreads;
	const int c0 = t * chunk < n_envs ? t * chunk : n_envs, c1 = c0 + chunk < n_envs ? c0 + chunk : n_envs;
	int na = 0, nr = 0;
	for (int e = c0; e < c1; ++e) { const int p = st[e].ext_park; na += p == kExtAwaiting; nr += p == kExtReady; }
	int incl = na, rsum = nr;
	for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d, 64); if ((t & 63) >= d) incl += o; }
	for (int d = 32; d > 0; d >>= 1) rsum += __shfl_xor(rsum, d, 64);
	if ((t & 63) == 63) part_a[t >> 6] = incl;
	if ((t & 63) == 0) part_r[t >> 6] = rsum;
	__syncthreads();
	int base = 0, total = 0, ready = 0;
	for (int w = 0; w < kExtThreads / 64; ++w) { const int c = part_a[w]; if (w < (t >> 6)) base += c; total += c; ready += part_r[w]; }
	int k = base + incl - na;
	for (int e = c0; e < c1 && k < cap; ++e) if (st[e].ext_park == kExtAwaiting) ids[k++] = e;
	if (t == 0) { meta[0] = total < cap ? total : cap; meta[1] = total; meta[2] = ready; meta[3] = 0; }
}
// dtrl_ext_states: one wavefront per collected env copies its S policy-state values into row i of the dense block [m][S] (reads and writes are consecutive
// per lane: coalesced rows), converting to the caller's type (float: device call, double: host call)
template <class T>
__global__ void __launch_bounds__(kGroup) dtrl_ext_states(const real* __restrict__ poli_state, int S, const int32_t* __restrict__ ids, const int32_t* __restrict__ meta, int n_envs, T* __restrict__ out)
{
	const int i = static_cast<int>(blockIdx.x);
	if (i >= meta[0]) return;
	const int e = ids[i];
	if (e < 0 || e >= n_envs) return;
	const real* src = poli_state + static_cast<size_t>(e) * S;
	T* dst = out + static_cast<size_t>(i) * S;
	for (int k = static_cast<int>(threadIdx.x); k < S; k += kGroup) dst[k] = static_cast<T>(src[k]);
}
// dtrl_ext_supply: one wavefront per delivered row. Lane 0 claims the env (env id and label in range, then awaiting -> ready by compare-and-swap: of two rows for one env the
// second is rejected), the wavefront writes the row into the env's slab record. apply == 0: validate only (count the rows that would be rejected, write nothing)
template <class T>
__global__ void __launch_bounds__(kGroup) dtrl_ext_supply(EnvState* __restrict__ st, ExtAction* __restrict__ slab, int n_envs, int n_opt, int n_labels, const int32_t* __restrict__ ids, int n,
	const int32_t* __restrict__ action_ids, const T* __restrict__ params, const uint32_t* __restrict__ flags, int apply, int32_t* __restrict__ rejected)
{
	const int i = static_cast<int>(blockIdx.x);
	if (i >= n) return;
	const int lane = static_cast<int>(threadIdx.x);
	const int e = ids[i];   // wave-uniform
	int ok = 0;
	if (lane == 0) {
		const int label = action_ids ? action_ids[i] : 0;
		if (e >= 0 && e < n_envs && label >= 0 && label < n_labels) {
			if (apply) ok = atomicCAS(&st[e].ext_park, static_cast<int>(kExtAwaiting), static_cast<int>(kExtReady)) == kExtAwaiting;
			else ok = st[e].ext_park == kExtAwaiting;
		}
		if (!ok) atomicAdd(rejected, 1);
	}
	ok = __shfl(ok, 0, 64);
	if (!ok || !apply) return;
	ExtAction& a = slab[e];
	if (lane == 0) { a.action_id = action_ids ? action_ids[i] : 0; a.flags = flags ? flags[i] : 0u; }
	if (lane < n_opt && lane < kMaxP) a.params[lane] = static_cast<real>(params[static_cast<size_t>(i) * n_opt + lane]);
}

// dst[i] = idx[i] >= 0 ? src[idx[i]] : 0: re-lays a policy blob handed over in device memory into the kernel's weight layout
// Calibration of the side streams (HipBackend::CalibrateSideStreams). dtrl_occupy: a stand-in for a frame launch's residency (one wavefront per workgroup,
// 20 KB of LDS -> 8 per compute unit, alive for `ticks` of the 100 MHz wall clock); block 0 stamps its start. dtrl_stamp: when did this stream's kernel get to run.
__global__ void __launch_bounds__(64) dtrl_occupy(long long ticks, long long* __restrict__ start_stamp)
{
	__shared__ float pad[5 * 1024];
	const long long t0 = wall_clock64();
	if (blockIdx.x == 0 && threadIdx.x == 0 && start_stamp) *start_stamp = t0;
	pad[threadIdx.x] = 1.0f;
	while (wall_clock64() - t0 < ticks) pad[threadIdx.x] += 1.0f;
	if (pad[threadIdx.x] < 0) __builtin_trap();
}
__global__ void __launch_bounds__(256) dtrl_stamp(long long* __restrict__ out)
{
	__shared__ float pad[4 * 1024];          // (a side kernel's typical footprint: does not fit beside a resident frame workgroup set)
	pad[threadIdx.x] = 1.0f;
	__syncthreads();
	if (blockIdx.x == 0 && threadIdx.x == 0) *out = wall_clock64() + (pad[1] > 2.0f ? 1 : 0);
}

__global__ void dtrl_gather_f32(float* __restrict__ dst, const float* __restrict__ src, const int32_t* __restrict__ idx, size_t n)
{
	for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * blockDim.x) {
		const int32_t k = idx[i];
		dst[i] = k >= 0 ? src[k] : 0.0f;
	}
}

// Env snapshots (dtrl_engine.h SnapPlan; include/dtrl.h dtrl_snapshot_save / _restore, dtrl_clone_envs): one wavefront per listed env moves every record of that
// env as consecutive 64-bit words (32-bit words for a record whose size is not a multiple of 8: the fp32 library's policy-state rows), lane k taking words
// k, k + 64, ... -- every load and store a coalesced burst, all records of all listed envs in ONE launch.
//   mode 0  gather   payload slice i <- env a[i]   (an env whose regenerated terrain record still waits in page-locked memory is read from there)
//   mode 1  scatter  env a[i] <- payload slice i
//   mode 2  copy     env b[i] <- env a[i]          (no env is both read and written: Engine::CloneEnvs stages overlapping lists)
template <class Word>
__device__ inline void snap_copy_words(char* __restrict__ dst, const char* __restrict__ src, uint32_t bytes, int lane)
{
	Word* d = reinterpret_cast<Word*>(dst); const Word* s = reinterpret_cast<const Word*>(src);
	const uint32_t n = bytes / static_cast<uint32_t>(sizeof(Word));
#pragma unroll 4
	for (uint32_t w = static_cast<uint32_t>(lane); w < n; w += kGroup) d[w] = s[w];
}
__global__ void __launch_bounds__(kGroup) dtrl_snap_move(SnapPlan p, char* payload, const int32_t* __restrict__ a, const int32_t* __restrict__ b, int n, int mode)
{
	const int i = static_cast<int>(blockIdx.x);
	if (i >= n) return;
	const int lane = static_cast<int>(threadIdx.x);
	const int ea = a[i], eb = mode == 2 ? b[i] : 0;   // wave-uniform
	char* slice = payload ? payload + static_cast<size_t>(i) * p.env_bytes : nullptr;
	for (int r = 0; r < p.n_rec; ++r) {
		const SnapRec rec = p.rec[r];
		const char* src; char* dst;
		if (mode == 1) { src = slice + rec.off; dst = rec.slab + static_cast<size_t>(ea) * rec.bytes; }
		else {
			src = rec.slab + static_cast<size_t>(ea) * rec.bytes;
			if (r == p.gr_rec && p.stage_slot != nullptr) { const int slot = p.stage_slot[ea] - 1; if (slot >= 0) src = reinterpret_cast<const char*>(&p.gr_stage[slot]); }
			dst = mode == 0 ? slice + rec.off : rec.slab + static_cast<size_t>(eb) * rec.bytes;
		}
		if ((rec.bytes & 7u) == 0) snap_copy_words<uint64_t>(dst, src, rec.bytes, lane);
		else snap_copy_words<uint32_t>(dst, src, rec.bytes, lane);
	}
}

// gr[ids[b]] = staged[b]: one workgroup per record (4 176 B as 16-byte words)
// -terrain_gen= device: one thread per env; only the few envs whose window must move (or that fell) do any work
__global__ void dtrl_terrain_boundary(DevBuffers buf, int e0, int n, int mode, const int32_t* __restrict__ env_list)
{
	int e;
	if (!span_env(static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x), e0, n, env_list, e)) return;
	tg_env_boundary(buf.gr[e], buf.gen[e], buf.status[e], *buf.tcfg, mode, e, buf.dist_ring, buf.dist_count, buf.dist_cap);
}
// Terrain sets (include/dtrl.h dtrl_terrains_create ...): the same thread-per-env boundary with one TerrainCfg per env. The table and the per-env terrain array
// are two extra pointer ARGUMENTS -- DevBuffers keeps its size and layout, so the by-value argument block of every other kernel is what it was. A terrain record
// is read through the pointer where it is used (type, then the parameters the type's generator draws from); lanes whose envs sit in terrains of different types
// part ways in tgen::build_terrain's type dispatch and run their generators one type after the other (docs/EXPERIMENTS.md, terrain sets).
__global__ void dtrl_terrain_boundary_keyed(DevBuffers buf, int e0, int n, int mode, const int32_t* __restrict__ env_list, const TerrainCfg* __restrict__ table, const int32_t* __restrict__ env_terrain)
{
	int e;
	if (!span_env(static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x), e0, n, env_list, e)) return;
	tg_env_boundary(buf.gr[e], buf.gen[e], buf.status[e], table[env_terrain[e]], mode, e, buf.dist_ring, buf.dist_count, buf.dist_cap);
}
// Terrain ladder (include/dtrl.h dtrl_terrain_ladder): the keyed boundary with the rule in front of it, in the same launch -- the env's level moves by its own
// status record (tg_ladder_step, dtrl_terrain_dev.h), the key and the ladder record are written back where they changed, and the terrain work runs under the NEW
// level's table entry. The ladder records and settings are arguments like the table and the key array. Thread per env, every word per env: no atomics of its own.
__global__ void dtrl_terrain_boundary_ladder(DevBuffers buf, int e0, int n, int mode, const int32_t* __restrict__ env_list, const TerrainCfg* __restrict__ table, int32_t* __restrict__ env_terrain,
	LadderRec* __restrict__ ladder, LadderCfg lc)
{
	int e;
	if (!span_env(static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x), e0, n, env_list, e)) return;
	const int32_t level = env_terrain[e];
	LadderRec lr = ladder[e];
	const LadderRec lr0 = lr;
	const int32_t next = tg_ladder_step(lr, level, buf.status[e], lc, mode, e);
	if (next != level) env_terrain[e] = next;
	if (lr.mark_x != lr0.mark_x || lr.ups != lr0.ups || lr.downs != lr0.downs) ladder[e] = lr;
	tg_env_boundary(buf.gr[e], buf.gen[e], buf.status[e], table[next], mode, e, buf.dist_ring, buf.dist_count, buf.dist_cap);
}
// Variant redraw (include/dtrl.h dtrl_variant_redraw): the envs of a group that fell draw the model variant of their next episode, behind the group's frame and
// boundary work and in front of its reset launch (var_redraw_step, dtrl_terrain_dev.h). A kernel of its own: the boundary kernels above stay as they are. Thread
// per env, every word per env, key and counter written back only where they changed: no atomics. The settings and the cumulative table are arguments.
__global__ void dtrl_variant_redraw(const EnvStatus* __restrict__ status, int e0, int n, const int32_t* __restrict__ env_list, int32_t* __restrict__ env_model, RedrawRec* __restrict__ recs, RedrawCfg rc)
{
	int e;
	if (!span_env(static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x), e0, n, env_list, e)) return;
	if (!(status[e].need_reset & 1)) return;
	const int32_t v = env_model[e];
	RedrawRec r = recs[e];
	const int32_t draws0 = r.draws;
	const int32_t next = var_redraw_step(r, v, true, rc, rc.cum, e);
	if (next != v) env_model[e] = next;
	if (r.draws != draws0) recs[e] = r;
}
// Variant rescale (include/dtrl.h dtrl_variant_rescale): the envs of a group that start an episode under their private model record get its mass and motor
// scalars redrawn, behind the group's frame and boundary work and in front of its reset launch (rescale_link, dtrl_terrain_dev.h). One wavefront per env of the
// span, lanes are links. An env that is not at an episode start, or not under its private key key_base + e, is left after two loads (wave-uniform). Every lane
// draws its own link's factors; the total (in `real`, link order) and the subtree masses (in double, ascending over the bits of sub_mask) are taken by
// broadcasting the lanes' masses one after the other, as the loader's loops add them. The six arrays are stored one element per lane, total_mass and the counter by
// lane 0: no atomics, no scratch. status == nullptr: every listed env starts (dtrl_reset). A kernel of its own: every other kernel of this unit stays as it is.
__global__ void __launch_bounds__(kGroup) dtrl_variant_rescale(const EnvStatus* __restrict__ status, int e0, int n, const int32_t* __restrict__ env_list, const int32_t* __restrict__ env_model,
	DevModel* __restrict__ models, int key_base, RescaleRec* __restrict__ recs, const ModelScalarsD* __restrict__ base, RescaleCfg rc)
{
	int e;
	if (!span_env(static_cast<int>(blockIdx.x), e0, n, env_list, e)) return;
	if (status && !(status[e].need_reset & 1)) return;
	if (env_model[e] != key_base + e) return;
	const int lane = static_cast<int>(threadIdx.x);
	const int32_t episode = recs[e].episodes;
	DevModel& m = models[key_base + e];
	const uint64_t key = rescale_stream_key(rc.seed, rc.env_id_base + e);
	const bool link = lane < rc.L;
	RescaleLink o{0, 0, 0, 0, 0};
	uint32_t sub = 0;
	if (link) { o = rescale_link(rc, key, episode, *base, lane); sub = m.sub_mask[lane]; }
	real total = 0; double sm = 0;
	for (int k = 0; k < rc.L; ++k) {
		const real mk = __shfl(o.mass, k, kGroup);
		total += mk;
		if ((sub >> k) & 1u) sm += mk;
	}
	if (link) { m.mass[lane] = o.mass; m.sub_mass[lane] = static_cast<real>(sm); m.inertia[lane] = o.inertia; m.kp[lane] = o.kp; m.kd[lane] = o.kd; m.torque_lim[lane] = o.torque_lim; }
	if (lane == 0) { m.total_mass = total; recs[e].episodes = episode + 1; }
}
// Push schedule (include/dtrl.h dtrl_push_schedule): the envs of a group count their waits down behind the group's frame and boundary work, and the ones that reach
// 0 get a random push into their perturbation slot (push_step, dtrl_terrain_dev.h). A kernel of its own: the frame and boundary kernels stay as they are. Thread
// per env, every word per env: no atomics. An env of scale 0 is left after one load; record and slot are written back only where they changed. status == nullptr:
// every listed env starts an episode (creation of the schedule, dtrl_reset, a terrain restart).
__global__ void __launch_bounds__(64) dtrl_push_schedule(const EnvStatus* __restrict__ status, int e0, int n, const int32_t* __restrict__ env_list, EnvState* __restrict__ st, PushRec* __restrict__ recs,
	const double* __restrict__ scale, PushCfg pc)
{
	int e;
	if (!span_env(static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x), e0, n, env_list, e)) return;
	const double sc = scale[e];
	if (sc == 0) return;
	const bool start = status ? status[e].need_reset != 0 : true;
	PushRec r = recs[e];
	PushOut out;
	if (push_step(r, sc, start, pc, e, out)) push_write_slot(st[e], out);
	recs[e] = r;   // (an env in the schedule moves its record at every boundary: the wait, or the counter)
}
// Episode limit (include/dtrl.h dtrl_episode_limit): the envs of a group count the boundaries of their episodes behind the group's frame and IN FRONT OF every
// other boundary rule, and an env that reached its drawn frame limit or the distance has its episode ended as a fall ends it (episode_limit_step / episode_end,
// dtrl_terrain_dev.h): need_reset goes into its status record and its state, and everything queued behind -- boundary work, redraw, rescale, push schedule, the
// reset launch -- sees an env whose episode ended. A kernel of its own: the frame and boundary kernels stay as they are. Thread per env, every word per env: no
// atomics, no scratch. A held-out env is left after one byte load. The record is 48 bytes on a 16-byte boundary and is read as three 16-byte words; a boundary
// that ends nothing stores the frame count alone, an episode start or end the whole record. status == nullptr: every listed env starts an episode.
__global__ void __launch_bounds__(64) dtrl_episode_limit(EnvStatus* __restrict__ status, int e0, int n, const int32_t* __restrict__ env_list, EnvState* __restrict__ st, EpisodeRec* __restrict__ recs,
	const uint8_t* __restrict__ on, EpisodeCfg ec)
{
	int e;
	if (!span_env(static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x), e0, n, env_list, e)) return;
	if (!on[e]) return;
	EpisodeRec r = recs[e];
	const int32_t cause = episode_limit_step(r, status ? status + e : nullptr, ec, e);
	if (cause != kEpisodeRuns) episode_end(st[e], status[e], ec);
	if (r.frames != 0) recs[e].frames = r.frames; else recs[e] = r;   // (frames == 0: an episode started or ended in this call)
}
// Frame trace (include/dtrl.h dtrl_trace): the traced envs of a group write the row of the frame that has just ended, behind the group's frame and the episode limit
// and IN FRONT OF everything that moves a key or resets an env (trace_due / trace_value / trace_int, dtrl_terrain_dev.h). One wavefront per entry of the group's own
// list of traced indices (built on the host when the trace is set; a group without a traced env launches nothing). An env that did not complete a frame (external
// policy mode: parked) is left after two loads (wave-uniform). Lanes take consecutive words of the row: W = 3 D + 2 doubles (71 for the dog, 65 for the raptor:
// more than a wavefront, so a lane-strided loop) read from consecutive elements of q, qd and tau, and lanes 0 .. 11 the integer part. The counter is read by every
// lane in front of the stores and written by lane 0 behind them; nothing else touches the env's ring or counter while launches run: no atomics, no scratch. A
// kernel of its own, all of it arguments: the frame, boundary and rule kernels stay as they are.
__global__ void __launch_bounds__(kGroup) dtrl_trace_record(const EnvState* __restrict__ st, const EnvStatus* __restrict__ status, TraceView tv, const int32_t* __restrict__ list, int n)
{
	const int i = static_cast<int>(blockIdx.x);
	if (i >= n) return;
	const int t = list[i];            // wave-uniform, as everything down to the lane loops
	const int e = tv.env_of[t];
	const EnvState& s = st[e];
	if (!trace_due(s)) return;
	const int lane = static_cast<int>(threadIdx.x);
	const int64_t w = tv.written[t];
	const size_t row = static_cast<size_t>(t) * tv.frames + trace_slot(w, tv.frames);
	double* vals = tv.vals + row * tv.W;
	for (int k = lane; k < tv.W; k += kGroup) vals[k] = trace_value(s, tv.D, k);
	if (lane < kTraceInts) {
		const int32_t slot = tv.env_slot ? tv.env_slot[e] : 0, variant = tv.env_variant ? tv.env_variant[e] : 0, terrain = tv.env_terrain ? tv.env_terrain[e] : 0;
		tv.ints[row * kTraceInts + lane] = trace_int(s, status[e], w, slot, variant, terrain, lane);
	}
	if (lane == 0) tv.written[t] = w + 1;
}
// dtrl_trace_read / dtrl_trace_read_device: the rings unrolled into chronological order. One wavefront per (listed env i, row r) of a grid of n x max(cap, 1), cap =
// min(frames, max_rows): row r < c = min(written, frames, max_rows) of slice i comes from ring slot (written - c + r) % frames, lanes taking consecutive words; rows
// beyond c are not touched; the wavefront of row 0 stores c. The destination is memory the device addresses: the caller's device buffers, or page-locked staging.
__global__ void __launch_bounds__(kGroup) dtrl_trace_gather(TraceView tv, const int32_t* __restrict__ list, int n, int cap, int max_rows, int row_stride, double* __restrict__ vals_out, int32_t* __restrict__ ints_out,
	int32_t* __restrict__ counts)
{
	const int per = cap > 0 ? cap : 1;
	const int i = static_cast<int>(blockIdx.x) / per, r = static_cast<int>(blockIdx.x) % per;
	if (i >= n) return;
	const int lane = static_cast<int>(threadIdx.x);
	const int t = list[i];            // wave-uniform
	const int64_t w = tv.written[t];
	const int32_t c = trace_count(w, tv.frames, max_rows);
	if (r == 0 && lane == 0) counts[i] = c;
	if (r >= c) return;
	const size_t src = static_cast<size_t>(t) * tv.frames + trace_read_slot(w, c, r, tv.frames), dst = static_cast<size_t>(i) * row_stride + r;
	const double* vs = tv.vals + src * tv.W; double* vd = vals_out + dst * tv.W;
	for (int k = lane; k < tv.W; k += kGroup) vd[k] = vs[k];
	if (lane < kTraceInts) ints_out[dst * kTraceInts + lane] = tv.ints[src * kTraceInts + lane];
}
// Episode log (include/dtrl.h dtrl_episode_log): the envs of a group count the boundaries of their episodes behind the group's frame, the episode limit and the
// trace and IN FRONT OF everything that moves a key or redraws a scale, and every env whose episode ended appends one 64-byte row to the group's ring in
// page-locked host memory (log_count / log_row, dtrl_terrain_dev.h). Shaped like dtrl_ext_collect: ONE workgroup per env group and frame; thread t owns the
// contiguous range [t c, (t + 1) c) of the group's span, counts its ended episodes, the counts are scanned across the workgroup (wave shuffles + one LDS level),
// and the thread writes its rows behind the ranges in front of it, in ascending env id, each as four 16-byte stores at slot (written + k) % capacity. More than
// `capacity` rows in one boundary: only the last `capacity` are stored (no two rows of a launch share a slot), the cursor advances by all of them. Publication:
// thread 0 first stores the reservation written + rows (cursor word 2) behind a system-scope fence and a barrier, so that a host reader whose copy this launch
// overwrites can tell; every thread that stored a row fences at system scope, the workgroup meets at a barrier, then thread 0 stores boundary + 1 and the new
// cursor -- the host never sees a cursor ahead of its rows. Thread 0 reads the pair once and hands it on through LDS. No atomics, no scratch; a kernel of its own, all of it arguments.
constexpr int kLogThreads = 1024;
// a record of whole 16-byte words moved as such (the compiler otherwise splits the struct along its fields)
typedef int32_t log_word __attribute__((ext_vector_type(4)));
template <class T> __device__ __forceinline__ T load_words(const T* src)
{
	static_assert(sizeof(T) % 16 == 0 && alignof(T) >= 16, "whole 16-byte words");
	log_word w[sizeof(T) / 16];
	for (size_t i = 0; i < sizeof(T) / 16; ++i) w[i] = reinterpret_cast<const log_word*>(src)[i];
	T v; __builtin_memcpy(&v, w, sizeof(T));
	return v;
}
template <class T> __device__ __forceinline__ void store_words(T* dst, const T& v)
{
	static_assert(sizeof(T) % 16 == 0 && alignof(T) >= 16, "whole 16-byte words");
	log_word w[sizeof(T) / 16];
	__builtin_memcpy(w, &v, sizeof(T));
	for (size_t i = 0; i < sizeof(T) / 16; ++i) reinterpret_cast<log_word*>(dst)[i] = w[i];
}
__device__ __forceinline__ bool log_due(const EnvState* __restrict__ st, const LogView& v, int e) { return !v.external || st[e].ext_steps_left == 0; }
__global__ void __launch_bounds__(kLogThreads) dtrl_episode_log(const EnvState* __restrict__ st, const EnvStatus* __restrict__ status, int e0, int n, LogView v)
{
	__shared__ int part[kLogThreads / 64];
	__shared__ int64_t cur[2];
	const int t = static_cast<int>(threadIdx.x);
	const int chunk = (n + kLogThreads - 1) / kLogThreads;
	const int c0 = t * chunk < n ? t * chunk : n, c1 = c0 + chunk < n ? c0 + chunk : n;
	if (t == 0) { cur[0] = v.cursor[0]; cur[1] = v.cursor[1]; }
	int mine = 0;
	for (int k = c0; k < c1; ++k) mine += log_due(st, v, e0 + k) && status[e0 + k].need_reset != 0;
	int incl = mine;
	for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d, 64); if ((t & 63) >= d) incl += o; }
	if ((t & 63) == 63) part[t >> 6] = incl;
	__syncthreads();
	int base = 0, total = 0;
	for (int w = 0; w < kLogThreads / 64; ++w) { const int c = part[w]; if (w < (t >> 6)) base += c; total += c; }
	const int64_t written = cur[0], boundary = cur[1];
	if (total > 0) {   // (uniform) the reservation goes out in front of the first row: a reader that copied a slot this launch overwrites finds out
		if (t == 0) { v.cursor[2] = written + total; __threadfence_system(); }
		__syncthreads();
	}
	int64_t row_k = base + incl - mine;
	for (int k = c0; k < c1; ++k) {
		const int e = e0 + k;
		if (!log_due(st, v, e)) continue;
		LogRec r = load_words(v.recs + e);
		const EnvStatus es = status[e];
		if (!log_count(r, es, true)) { v.recs[e].frames = r.frames; continue; }
		LogEnv le;
		le.limit_cause = (v.episode && v.episode_on[e]) ? v.episode[e].last_cause : 0;
		le.slot = v.env_slot ? v.env_slot[e] : 0; le.variant = v.env_variant ? v.env_variant[e] : 0; le.terrain = v.env_terrain ? v.env_terrain[e] : 0;
		le.rescale_episodes = v.rescale ? v.rescale[e].episodes : 0;
		const LogRow row = log_row(r, es, st[e].num_cycles, boundary, le, v, e);
		if (log_row_kept(total, row_k, v.capacity)) store_words(v.ring + log_slot(written, row_k, v.capacity), row);
		row_k += 1;
		store_words(v.recs + e, r);
	}
	if (mine) __threadfence_system();
	__syncthreads();
	if (t == 0) { v.cursor[1] = boundary + 1; v.cursor[0] = written + total; }
}
// the listed form (dtrl_reset, a terrain restart, the log is set): thread per listed env, the running episode is abandoned without a row (log_start)
__global__ void __launch_bounds__(64) dtrl_episode_log_start(int e0, int n, const int32_t* __restrict__ env_list, const EnvState* __restrict__ st, LogRec* __restrict__ recs)
{
	int e;
	if (!span_env(static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x), e0, n, env_list, e)) return;
	LogRec r = recs[e];
	log_start(r, st[e].num_cycles);
	recs[e] = r;
}
// dtrl_add_perturb in one launch: a thread per row (the engine has reduced the rows to one per env), the seven slot fields each
__global__ void __launch_bounds__(64) dtrl_perturb_scatter(EnvState* __restrict__ st, const PerturbRow* __restrict__ rows, int n)
{
	int k;
	if (!span_env(static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x), 0, n, nullptr, k)) return;
	const PerturbRow r = rows[k];
	perturb_write_slot(st[r.env], r);
}
// launch order of a group's next frame: counting sort on cost / 16, costliest first (one workgroup; the order inside a bucket is whatever the
// atomics produce -- it only decides which wavefront starts first)
constexpr int kOrderBuckets = 1024;
__global__ void __launch_bounds__(1024) dtrl_order_by_cost(const EnvStatus* __restrict__ status, int e0, int n, int32_t* __restrict__ order)
{
	__shared__ int hist[kOrderBuckets];
	__shared__ int part[kOrderBuckets / 64];
	const int t = static_cast<int>(threadIdx.x);
	hist[t] = 0;
	__syncthreads();
	auto key = [&](int e) { int k = status[e].cost >> 4; k = k < 0 ? 0 : (k >= kOrderBuckets ? kOrderBuckets - 1 : k); return kOrderBuckets - 1 - k; };
	for (int i = t; i < n; i += kOrderBuckets) atomicAdd(&hist[key(e0 + i)], 1);
	__syncthreads();
	// exclusive scan of 1024 counters: per-wave serial prefix over 64 entries by lane 0 of each wave would idle; a two-level scan instead
	int v = hist[t];
	int incl = v;
	for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d, 64); if ((t & 63) >= d) incl += o; }
	if ((t & 63) == 63) part[t >> 6] = incl;
	__syncthreads();
	if (t == 0) { int run = 0; for (int w = 0; w < kOrderBuckets / 64; ++w) { const int c = part[w]; part[w] = run; run += c; } }
	__syncthreads();
	hist[t] = part[t >> 6] + incl - v;
	__syncthreads();
	for (int i = t; i < n; i += kOrderBuckets) { const int e = e0 + i; order[e0 + atomicAdd(&hist[key(e)], 1)] = e; }
}
// packed tuple drain (dtrl_drain_tuples_packed). The pending rows of the ring are put in (env id, ring position) order by a segmented counting sort on the
// env id -- O(rows + envs), one workgroup (round 2 ranked every row against every other: 36 M compares at a full 65 536-env ring) --, the first block_rows
// of them are copied into the caller's block, and whatever does not fit is CARRIED: moved to the front of the ring, where the next drain of this ring
// finds it in front of the newer rows (nothing is dropped because a block was small). Three launches on the drain stream:
//   dtrl_tuple_order   order[r] = ring position of the r-th row; meta = {take, lost to a full ring, carried, stored}
//   dtrl_tuple_pack    block row 1 + r <- ring row order[r] (r < take), carry staging row r - take <- ring row order[r] (r >= take)
//   dtrl_tuple_finish  ring rows [0, carried) <- staging, header row of the block, ring cursor = carried, drained / dropped totals
constexpr int kOrderThreads = 1024;
__global__ void __launch_bounds__(kOrderThreads) dtrl_tuple_order(DevBuffers buf, int block_rows, int n_envs, int32_t* __restrict__ order, int32_t* __restrict__ hist, int32_t* __restrict__ meta)
{
	__shared__ int part[kOrderThreads];
	const int t = static_cast<int>(threadIdx.x);
	const int cnt = buf.tuple_count[0];
	const int n = cnt < buf.tuple_cap ? cnt : buf.tuple_cap;
	for (int e = t; e <= n_envs; e += kOrderThreads) hist[e] = 0;
	__syncthreads();
	for (int k = t; k < n; k += kOrderThreads) atomicAdd(&hist[buf.tuple_env[k]], 1);
	__syncthreads();
	// exclusive scan over the envs: a contiguous chunk per thread, the chunk totals scanned across the workgroup
	const int chunk = (n_envs + kOrderThreads - 1) / kOrderThreads;
	const int c0 = t * chunk, c1 = (c0 + chunk < n_envs) ? c0 + chunk : n_envs;
	int sum = 0;
	for (int e = c0; e < c1; ++e) sum += hist[e];
	part[t] = sum;
	__syncthreads();
	for (int d = 1; d < kOrderThreads; d <<= 1) { const int o = t >= d ? part[t - d] : 0; __syncthreads(); part[t] += o; __syncthreads(); }
	int run = part[t] - sum;
	for (int e = c0; e < c1; ++e) { const int c = hist[e]; hist[e] = run; run += c; }
	__syncthreads();
	// scatter: the atomics hand out the slots of an env's segment in arbitrary order ...
	for (int k = t; k < n; k += kOrderThreads) order[atomicAdd(&hist[buf.tuple_env[k]], 1)] = k;
	__syncthreads();
	// ... so every segment with more than one row (an env that completed two cycles between drains, or carried rows) is put in ring order; after the
	// scatter hist[e] is the END of env e's segment
	for (int e = t; e < n_envs; e += kOrderThreads) {
		const int s0 = e ? hist[e - 1] : 0, s1 = hist[e];
		for (int i = s0 + 1; i < s1; ++i) { const int v = order[i]; int j = i - 1; while (j >= s0 && order[j] > v) { order[j + 1] = order[j]; --j; } order[j + 1] = v; }
	}
	if (t == 0) { const int take = n < block_rows ? n : block_rows; meta[0] = take; meta[1] = cnt - n; meta[2] = n - take; meta[3] = n; }
}
__global__ void dtrl_tuple_pack(DevBuffers buf, const int32_t* __restrict__ order, const int32_t* __restrict__ meta, float* __restrict__ block, int64_t env_id_base, float* __restrict__ c_rows, uint32_t* __restrict__ c_flags, int32_t* __restrict__ c_env)
{
	const int take = meta[0], n = meta[3], W = buf.W;
	for (int r = static_cast<int>(blockIdx.x); r < n; r += static_cast<int>(gridDim.x)) {
		const int k = order[r];
		const float* src = buf.tuple_rows + static_cast<size_t>(k) * W;
		if (r < take) {
			float* dst = block + static_cast<size_t>(1 + r) * (W + 2);
			for (int i = static_cast<int>(threadIdx.x); i < W; i += static_cast<int>(blockDim.x)) dst[i] = src[i];
			if (threadIdx.x == 0) { dst[W] = __int_as_float(static_cast<int>(buf.tuple_flags[k])); dst[W + 1] = __int_as_float(static_cast<int>(env_id_base + buf.tuple_env[k])); }
		} else {
			float* dst = c_rows + static_cast<size_t>(r - take) * W;
			for (int i = static_cast<int>(threadIdx.x); i < W; i += static_cast<int>(blockDim.x)) dst[i] = src[i];
			if (threadIdx.x == 0) { c_flags[r - take] = buf.tuple_flags[k]; c_env[r - take] = buf.tuple_env[k]; }
		}
	}
}
__global__ void dtrl_tuple_finish(DevBuffers buf, const int32_t* __restrict__ meta, float* __restrict__ block, const float* __restrict__ c_rows, const uint32_t* __restrict__ c_flags, const int32_t* __restrict__ c_env)
{
	const int take = meta[0], lost = meta[1], carry = meta[2], W = buf.W;
	const int t = static_cast<int>(threadIdx.x);
	for (int r = static_cast<int>(blockIdx.x); r < carry; r += static_cast<int>(gridDim.x)) {
		float* dst = buf.tuple_rows + static_cast<size_t>(r) * W;
		const float* src = c_rows + static_cast<size_t>(r) * W;
		for (int i = t; i < W; i += static_cast<int>(blockDim.x)) dst[i] = src[i];
		if (t == 0) { buf.tuple_flags[r] = c_flags[r]; buf.tuple_env[r] = c_env[r]; }
	}
	if (blockIdx.x == 0) {
		for (int i = t; i < W + 2; i += static_cast<int>(blockDim.x)) block[i] = (i == 0) ? __int_as_float(take) : (i == 1) ? __int_as_float(lost) : (i == 2) ? __int_as_float(carry) : 0.0f;
		if (t == 0) { buf.tuple_count[1] += take; buf.tuple_count[2] += lost; buf.tuple_count[0] = carry; }
	}
}
// ---- dtrl_slot_stats: per-slot sums over the EnvState records, on the device ----
// dtrl_slot_partials: the workgroups' wavefronts stride over the envs; per pass a wavefront folds, slot by slot, its 64 lanes' contributions with a butterfly of
// shuffles and lane 0 adds the result to the wavefront's row in LDS; the workgroup then adds its wavefronts' rows in wavefront order and writes ONE row of
// partials. dtrl_slot_final (one workgroup) adds the rows in workgroup order. No atomics anywhere: every sum has one fixed order, the bytes repeat from call to call.
constexpr int kReduceThreads = 256, kReduceWaves = kReduceThreads / 64;

__device__ __forceinline__ long long wave_sum(long long v) { for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64); return v; }
__device__ __forceinline__ double wave_sum(double v) { for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64); return v; }

__global__ void __launch_bounds__(kReduceThreads) dtrl_slot_partials(const EnvState* __restrict__ st, const int32_t* __restrict__ env_slot, int n_envs, int n_slots, int slot_base, SlotSums* __restrict__ rows)
{
	__shared__ SlotSums part[kReduceWaves][kMaxSlots];
	const int t = static_cast<int>(threadIdx.x), wave = t >> 6, lane = t & 63;
	for (int k = t; k < kReduceWaves * kMaxSlots; k += kReduceThreads) part[k / kMaxSlots][k % kMaxSlots] = SlotSums{0, 0, 0, 0, 0.0};
	__syncthreads();
	const int stride = static_cast<int>(gridDim.x) * kReduceThreads;
	const int passes = (n_envs + stride - 1) / stride;   // the same for every thread: the shuffles below need whole wavefronts
	for (int p = 0; p < passes; ++p) {
		const int e = p * stride + static_cast<int>(blockIdx.x) * kReduceThreads + t;
		int s = -1; long long ep = 0, cy = 0, rs = 0; double ds = 0.0;
		if (e < n_envs) {
			s = env_slot[e] - slot_base;   // (outside 0 .. n_slots - 1: counted nowhere)
			ep = st[e].num_episodes; cy = st[e].num_cycles; rs = st[e].num_resets;
			ds = static_cast<double>(st[e].avg_dist) * static_cast<double>(ep);
		}
		for (int q = 0; q < n_slots; ++q) {
			const bool mine = s == q;
			if (__ballot(mine) == 0) continue;   // (wave-uniform)
			const long long c = wave_sum(static_cast<long long>(mine ? 1 : 0)), a = wave_sum(mine ? ep : 0LL), b = wave_sum(mine ? cy : 0LL), r = wave_sum(mine ? rs : 0LL);
			const double d = wave_sum(mine ? ds : 0.0);
			if (lane == 0) { SlotSums& o = part[wave][q]; o.n_envs += c; o.episodes += a; o.cycles += b; o.resets += r; o.dist_sum += d; }
		}
	}
	__syncthreads();
	if (t < n_slots) {
		SlotSums o = part[0][t];
		for (int w = 1; w < kReduceWaves; ++w) { const SlotSums& x = part[w][t]; o.n_envs += x.n_envs; o.episodes += x.episodes; o.cycles += x.cycles; o.resets += x.resets; o.dist_sum += x.dist_sum; }
		rows[static_cast<size_t>(blockIdx.x) * kMaxSlots + t] = o;
	}
}

__global__ void __launch_bounds__(64) dtrl_slot_final(const SlotSums* __restrict__ rows, int n_rows, int n_slots, SlotSums* __restrict__ out)
{
	const int t = static_cast<int>(threadIdx.x);
	if (t >= n_slots) return;
	SlotSums o = rows[t];
	for (int b = 1; b < n_rows; ++b) { const SlotSums& x = rows[static_cast<size_t>(b) * kMaxSlots + t]; o.n_envs += x.n_envs; o.episodes += x.episodes; o.cycles += x.cycles; o.resets += x.resets; o.dist_sum += x.dist_sum; }
	out[t] = o;
}

constexpr int kSlotReduceMaxRows = 64;
static int SlotReduceRows(int n_envs) { const int g = (n_envs + kReduceThreads - 1) / kReduceThreads; return g < 1 ? 1 : (g > kSlotReduceMaxRows ? kSlotReduceMaxRows : g); }

// scratch: device memory for (SlotReduceRows(n_envs) + 1) * kMaxSlots records; the totals land in its last kMaxSlots records
static hipError_t LaunchSlotReduce(hipStream_t s, const EnvState* st, const int32_t* env_slot, int n_envs, int n_slots, int slot_base, SlotSums* scratch)
{
	const int rows = SlotReduceRows(n_envs);
	hipLaunchKernelGGL(dtrl_slot_partials, dim3(rows), dim3(kReduceThreads), 0, s, st, env_slot, n_envs, n_slots, slot_base, scratch);
	hipLaunchKernelGGL(dtrl_slot_final, dim3(1), dim3(64), 0, s, scratch, rows, n_slots, scratch + static_cast<size_t>(rows) * kMaxSlots);
	return hipGetLastError();
}

class HipBackend : public Backend {
public:
	~HipBackend() override
	{
		for (auto& ev : events_) { hipEventDestroy(ev.first); hipEventDestroy(ev.second); }
		for (auto& m : marks_) if (m.second) hipEventDestroy(m.second);
		for (hipEvent_t ev : timed_ev_) if (ev) hipEventDestroy(ev);
		if (policy_ready_) hipEventDestroy(policy_ready_);
		if (ext_rej_) hipFree(ext_rej_);
		if (slot_scratch_) hipFree(slot_scratch_);
		if (!owned_.empty()) { for (int i = kNumStreams / 2; i < kNumStreams; ++i) streams_[i] = nullptr; for (hipStream_t st : owned_) hipStreamDestroy(st); }
		for (hipStream_t st : streams_) if (st) hipStreamDestroy(st);
	}
	bool Init(int device_id, std::string& err) override
	{
		int count = 0;
		hipError_t e = hipGetDeviceCount(&count);
		if (e != hipSuccess || count <= 0) { err = std::string("no usable HIP device (") + hipGetErrorString(e) + "); the engine has no CPU fallback"; return false; }
		if (device_id >= 0) { e = hipSetDevice(device_id); if (e != hipSuccess) { err = std::string("hipSetDevice: ") + hipGetErrorString(e); return false; } }
		streams_.assign(kNumStreams, nullptr);
		// DTRL_RESERVE_CUS=k keeps k compute units per XCD out of the frame launches: a frame launch fills every wavefront slot of the CUs it may use for
		// milliseconds, and whatever else needs the GPU meanwhile -- RCCL's collective kernels, the tuple drain, a trainer's copies -- would wait for a wavefront
		// to retire (nothing does in the first ~2 ms of a frame). The env-group streams (the first kNumStreams / 2) get a CU mask without those units (mask
		// bit i = compute unit i / #XCD of XCD i % #XCD, so the top 8 k bits are k units on each of the 8 XCDs); the other streams, and every other stream of
		// the process, may use all of them. Costs k / 32 of the rollout rate; worth it when something has to overlap the rollout (multi-rank exchange).
		int reserve = reserve_arg_;
		if (reserve < 0) { reserve = 0; if (const char* env = std::getenv("DTRL_RESERVE_CUS")) reserve = std::atoi(env); }
		reserve = std::max(0, std::min(8, reserve));
		hipDeviceProp_t prop;
		int cus = 0;
		if (reserve > 0 && hipGetDeviceProperties(&prop, device_id >= 0 ? device_id : 0) == hipSuccess) cus = prop.multiProcessorCount;
		constexpr int kXcd = 8;
		for (int i = 0; i < kNumStreams; ++i) {
			if (reserve > 0 && cus >= 2 * kXcd * reserve && i < kNumStreams / 2) {
				std::vector<uint32_t> mask((cus + 31) / 32, 0u);
				for (int b = 0; b < cus - kXcd * reserve; ++b) mask[b / 32] |= 1u << (b % 32);
				e = hipExtStreamCreateWithCUMask(&streams_[i], static_cast<uint32_t>(mask.size()), mask.data());
			} else e = hipStreamCreateWithFlags(&streams_[i], hipStreamNonBlocking);
			if (e != hipSuccess) { err = std::string("hipStreamCreate: ") + hipGetErrorString(e); return false; }
		}
		stream_ = streams_[0];
		masked_ = reserve > 0 && cus >= 2 * kXcd * reserve;
		if (masked_ && !CalibrateSideStreams(err)) return false;
		return true;
	}
	// Which streams can actually USE the reserved compute units while frame launches are in flight? Measured on the MI355X (tools/microbench/cu_mask_probe.hip,
	// DESIGN 9): a launch that is waiting for wavefront slots (the second env group's, while the first fills the unmasked units) holds up OTHER hardware queues
	// too -- 3 to 5 of 10 plain streams of a process see their kernels start only when that launch has been placed or has finished (2.7 / 5.6 ms for a 3 ms
	// occupant), although the reserved units are idle; the rest start within 7 us. Which streams are affected depends on how the runtime mapped them onto
	// hardware queues, so it is measured here, once: two occupant launches on the env-group streams 0 and 1, a stamp kernel on every candidate stream, and the
	// candidates ordered by how long after the occupants' start their stamp ran (worst of 3 rounds). The plain engine streams (kNumStreams / 2 ..) are then
	// re-seated on the quickest candidates -- the tuple-drain stream first -- and the next two are handed out as side streams (dtrl_side_stream: the trainer's
	// launches, the exchange's collective).
	bool CalibrateSideStreams(std::string& err)
	{
		constexpr int kCand = 12, kBurst = 10;
		constexpr long long kTicks = 120000;         // 1.2 ms per occupant
		std::vector<hipStream_t> cand;
		for (int i = kNumStreams / 2; i < kNumStreams; ++i) cand.push_back(streams_[i]);
		while (static_cast<int>(cand.size()) < kCand) { hipStream_t st; if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) break; cand.push_back(st); extra_.push_back(st); }
		long long* stamps = nullptr;
		auto drop_extras = [&]() { for (hipStream_t st : extra_) hipStreamDestroy(st); extra_.clear(); };   // (a failed calibration keeps the engine's own streams only)
		// the assignment below hands out kNumStreams / 2 + 2 streams (the plain engine streams + two side streams): with fewer candidates (stream creation failed)
		// there is nothing to choose from -- keep the engine's own streams, hand out no side streams
		if (static_cast<int>(cand.size()) < kNumStreams - kNumStreams / 2 + 2) { drop_extras(); err = "side-stream calibration: could not create enough candidate streams"; return false; }
		if (!Check(hipHostMalloc(&stamps, sizeof(long long) * 4, hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc")) { err = err_; drop_extras(); return false; }
		std::vector<long long> worst(cand.size(), 0);   // microseconds x 100 (the sort below only compares)
		for (int r = 0; r < 3; ++r) {                 // (round 0 warms the code objects and the streams' queues up; the worse of rounds 1 and 2 counts)
			for (size_t c = 0; c < cand.size(); ++c) {
				stamps[0] = 0;
				hipDeviceSynchronize();
				hipLaunchKernelGGL(dtrl_occupy, dim3(2048), dim3(64), 0, streams_[0], r == 0 ? 2000LL : kTicks, stamps);
				hipLaunchKernelGGL(dtrl_occupy, dim3(2048), dim3(64), 0, streams_[1], r == 0 ? 2000LL : kTicks, static_cast<long long*>(nullptr));
				{   // the first occupant is running, the second waits for slots (bounded wait: a launch that never starts must not hang the creation)
					const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(2);
					while (*static_cast<volatile long long*>(stamps) == 0 && std::chrono::steady_clock::now() < deadline) {}
					if (*static_cast<volatile long long*>(stamps) == 0) { hipDeviceSynchronize(); hipHostFree(stamps); drop_extras(); err = "side-stream calibration: the occupant kernel did not start within 2 s"; return false; }
				}
				std::this_thread::sleep_for(std::chrono::microseconds(r == 0 ? 0 : 200));
				const auto t0 = std::chrono::steady_clock::now();
				for (int k = 0; k < kBurst; ++k) hipLaunchKernelGGL(dtrl_stamp, dim3(96), dim3(256), 0, cand[c], stamps + 1);
				if (!Check(hipStreamSynchronize(cand[c]), "side-stream calibration")) { err = err_; hipHostFree(stamps); drop_extras(); return false; }
				const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
				if (r > 0) worst[c] = std::max(worst[c], static_cast<long long>(us * 100.0));
			}
		}
		hipDeviceSynchronize();
		hipHostFree(stamps);
		std::vector<int> ord(cand.size());
		for (size_t c = 0; c < cand.size(); ++c) ord[c] = static_cast<int>(c);
		std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return worst[a] < worst[b]; });
		side_delay_us_.clear();
		for (int c : ord) side_delay_us_.push_back(worst[c] / 100.0);
		// the drain stream (kNumStreams - 1) gets the quickest, then the two side streams, then the other plain engine streams
		std::vector<hipStream_t> pick;
		for (int c : ord) pick.push_back(cand[c]);
		streams_[kNumStreams - 1] = pick[0];
		side_[0] = pick[1]; side_[1] = pick[2];
		for (int i = kNumStreams / 2, k = 3; i < kNumStreams - 1; ++i, ++k) streams_[i] = pick[k];
		calibrated_ = true;
		owned_.assign(cand.begin(), cand.end());      // every candidate stays alive (destroying one could re-seat the others) and is destroyed with the backend
		if (std::getenv("DTRL_HOST_TIMING")) {
			std::fprintf(stderr, "[dtrl] side-stream calibration: 10-kernel burst beside the occupants, us per candidate (sorted):");
			for (double v : side_delay_us_) std::fprintf(stderr, " %.0f", v);
			std::fprintf(stderr, "\n");
		}
		return true;
	}
	void SetReserveCus(int k) override { reserve_arg_ = k; }
	// (without a reservation there is nothing to hand out: measured, a calibrated stream then did no better than any other -- A/B on one box, dog training loop:
	// 10.0 / 10.1 / 11.2 / 10.9 M with it, 11.2 / 11.3 / 11.2 / 11.2 M on the framework's own stream -- the occupants of the calibration leave room the frame kernel does not)
	void* SideStream(int k) override { return (masked_ && calibrated_ && k >= 0 && k < 2) ? static_cast<void*>(side_[k]) : nullptr; }
	double SideStreamDelayUs(int k) override { return (calibrated_ && k >= 0 && k + 1 < static_cast<int>(side_delay_us_.size())) ? side_delay_us_[k + 1] : -1.0; }
	void* Alloc(size_t bytes) override
	{
		void* p = nullptr;
		if (!Check(hipMalloc(&p, bytes), "hipMalloc")) return nullptr;
		if (!Check(hipMemsetAsync(p, 0, bytes, stream_), "hipMemset")) return nullptr;
		return p;
	}
	void Free(void* p) override { hipFree(p); }
	bool H2D(void* dst, const void* src, size_t n) override { return Check(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, stream_), "hipMemcpy H2D") && Check(hipStreamSynchronize(stream_), "sync"); }
	bool D2HAsync(void* dst, const void* src, size_t n) override { return Check(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync D2H"); }
	bool H2DAsync(void* dst, const void* src, size_t n) override { return Check(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, stream_), "hipMemcpyAsync H2D"); }
	void* HostStaging(size_t bytes) override { void* p = nullptr; return Check(hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc") ? p : nullptr; }
	bool SyncSelected() override { return Check(hipStreamSynchronize(stream_), "hipStreamSynchronize"); }
	void FreeHostStaging(void* p) override { if (p) hipHostFree(p); }
	bool D2H(void* dst, const void* src, size_t n) override { return Check(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, stream_), "hipMemcpy D2H") && Check(hipStreamSynchronize(stream_), "sync"); }
	bool D2D(void* dst, const void* src, size_t n) override { return Check(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, stream_), "hipMemcpy D2D") && Check(hipStreamSynchronize(stream_), "sync"); }
	// snapshot transport: one launch each. DTRL_SNAPSHOT_FALLBACK=1 takes the copy-per-record defaults instead (the A/B of profiles/r08_snapshot.txt)
	bool SnapMove(const SnapPlan& p, char* payload, const int32_t* a, const int32_t* b, int n, int mode)
	{
		if (n <= 0) return true;
		if (!TimedBegin()) return false;
		hipLaunchKernelGGL(dtrl_snap_move, dim3(n), dim3(kGroup), 0, stream_, p, payload, a, b, n, mode);
		return TimedEnd(snap_ms_, "snapshot launch", "snapshot");
	}
	double SnapLaunchMs() override { const double v = snap_ms_; snap_ms_ = 0; return v; }
	// A timed section of the selected stream: TimedBegin, the caller's launches, TimedEnd -- which waits for the stream and adds the launches' device time to
	// `sum_ms`. One event pair serves every section: each ends synchronised. (Snapshot transport; external policy mode's collection and scatter.)
	bool TimedBegin()
	{
		if (!timed_ev_[0] && (!Check(hipEventCreate(&timed_ev_[0]), "hipEventCreate") || !Check(hipEventCreate(&timed_ev_[1]), "hipEventCreate"))) return false;
		return Check(hipEventRecord(timed_ev_[0], stream_), "hipEventRecord");
	}
	bool TimedEnd(double& sum_ms, const char* launch_what, const char* sync_what)
	{
		hipEventRecord(timed_ev_[1], stream_);
		if (!Check(hipGetLastError(), launch_what) || !Check(hipStreamSynchronize(stream_), sync_what)) return false;
		float ms = 0;
		if (hipEventElapsedTime(&ms, timed_ev_[0], timed_ev_[1]) == hipSuccess) sum_ms += ms;
		return true;
	}
	bool ExtEnd(int which) { return TimedEnd(ext_ms_[which], "external-policy launch", "external-policy hand-over"); }
	bool ExtCollect(const DevBuffers& buf, int n_envs, int cap, int32_t* ids, void* states, bool f32, int32_t* meta) override
	{
		if (!TimedBegin()) return false;
		hipLaunchKernelGGL(dtrl_ext_collect, dim3(1), dim3(kExtThreads), 0, stream_, buf.st, n_envs, cap, ids, meta);
		const int rows = std::min(cap, n_envs);
		if (states && rows > 0) {
			if (f32) hipLaunchKernelGGL(dtrl_ext_states<float>, dim3(rows), dim3(kGroup), 0, stream_, buf.poli_state, buf.S, ids, meta, n_envs, static_cast<float*>(states));
			else hipLaunchKernelGGL(dtrl_ext_states<double>, dim3(rows), dim3(kGroup), 0, stream_, buf.poli_state, buf.S, ids, meta, n_envs, static_cast<double*>(states));
		}
		return ExtEnd(0);
	}
	bool ExtSupply(const DevBuffers& buf, int n_envs, int n_opt, int n_labels, const int32_t* ids, int n, const int32_t* action_ids, const void* params, bool f32, const uint32_t* flags, bool apply, int32_t* rejected) override
	{
		*rejected = 0;
		if (n <= 0) return true;
		if (!ext_rej_ && !Check(hipMalloc(&ext_rej_, sizeof(int32_t)), "hipMalloc")) return false;
		if (!Check(hipMemsetAsync(ext_rej_, 0, sizeof(int32_t), stream_), "hipMemset") || !TimedBegin()) return false;
		if (f32) hipLaunchKernelGGL(dtrl_ext_supply<float>, dim3(n), dim3(kGroup), 0, stream_, buf.st, ext_actions(buf), n_envs, n_opt, n_labels, ids, n, action_ids, static_cast<const float*>(params), flags, apply ? 1 : 0, ext_rej_);
		else hipLaunchKernelGGL(dtrl_ext_supply<double>, dim3(n), dim3(kGroup), 0, stream_, buf.st, ext_actions(buf), n_envs, n_opt, n_labels, ids, n, action_ids, static_cast<const double*>(params), flags, apply ? 1 : 0, ext_rej_);
		if (!ExtEnd(1)) return false;
		return Check(hipMemcpyAsync(rejected, ext_rej_, sizeof(int32_t), hipMemcpyDeviceToHost, stream_), "hipMemcpy D2H") && Check(hipStreamSynchronize(stream_), "sync");
	}
	double ExtLaunchMs(int which) override { const int k = which ? 1 : 0; const double v = ext_ms_[k]; ext_ms_[k] = 0; return v; }
	// an A/B and cross-check switch of the environment is set and non-zero (read per call, like DTRL_KERNEL: a test switches it inside one process)
	static bool EnvFlag(const char* name) { const char* e = std::getenv(name); return e && std::atoi(e) != 0; }
	bool SnapGather(const SnapPlan& p, char* payload, const int32_t* ids, int n) override { return EnvFlag("DTRL_SNAPSHOT_FALLBACK") ? Backend::SnapGather(p, payload, ids, n) : SnapMove(p, payload, ids, nullptr, n, 0); }
	bool SnapScatter(const SnapPlan& p, const char* payload, const int32_t* ids, int n) override { return EnvFlag("DTRL_SNAPSHOT_FALLBACK") ? Backend::SnapScatter(p, payload, ids, n) : SnapMove(p, const_cast<char*>(payload), ids, nullptr, n, 1); }
	bool SnapCopy(const SnapPlan& p, const int32_t* src_ids, const int32_t* dst_ids, int n) override { return EnvFlag("DTRL_SNAPSHOT_FALLBACK") ? Backend::SnapCopy(p, src_ids, dst_ids, n) : SnapMove(p, nullptr, src_ids, dst_ids, n, 2); }
	// the one gather launch; the three entry points differ in the stream and in what follows the launch
	bool GatherLaunch(hipStream_t st, float* dst, const float* src, const int32_t* idx, size_t n)
	{
		hipLaunchKernelGGL(dtrl_gather_f32, dim3(1024), dim3(256), 0, st, dst, src, idx, n);
		return Check(hipGetLastError(), "gather launch");
	}
	bool GatherF32(float* dst, const float* src, const int32_t* idx, size_t n) override { return GatherF32On(nullptr, dst, src, idx, n); }
	bool GatherF32On(void* stream, float* dst, const float* src, const int32_t* idx, size_t n) override
	{
		hipStream_t st = stream ? static_cast<hipStream_t>(stream) : stream_;
		return GatherLaunch(st, dst, src, idx, n) && Check(hipStreamSynchronize(st), "sync");
	}
	bool PackTuples(const DevBuffers& buf, float* block, int block_rows, int64_t env_id_base, int n_envs, const PackScratch& sc) override
	{
		const int grid = std::max(1, std::min<int>(buf.tuple_cap, 2048));
		hipLaunchKernelGGL(dtrl_tuple_order, dim3(1), dim3(kOrderThreads), 0, stream_, buf, block_rows, n_envs, sc.order, sc.hist, sc.meta);
		hipLaunchKernelGGL(dtrl_tuple_pack, dim3(grid), dim3(256), 0, stream_, buf, sc.order, sc.meta, block, env_id_base, sc.rows, sc.flags, sc.env);
		hipLaunchKernelGGL(dtrl_tuple_finish, dim3(grid), dim3(256), 0, stream_, buf, sc.meta, block, sc.rows, sc.flags, sc.env);
		return Check(hipGetLastError(), "tuple pack launch") && Check(hipStreamSynchronize(stream_), "tuple pack");
	}
	// Marks: an event per (env group, key) behind the group's latest launch of that kind. Keys 0, 1: the frame that wrote tuple ring `slot` (MarkFrame /
	// WaitFrames); kWeightReader + wbuf: the latest reader of weight buffer `wbuf` (the double-buffered policy hand-over, Engine::SetPolicyDevice)
	enum MarkKey { kWeightReader = 8, kMarkKeys = 16 };
	bool Mark(int group, int key)
	{
		hipEvent_t& ev = marks_[group * kMarkKeys + key];
		if (!ev && !Check(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate")) return false;
		return Check(hipEventRecord(ev, streams_[group]), "hipEventRecord");
	}
	bool WaitMarks(hipStream_t st, int key, int n_groups)   // `st` waits, on the device, for every group's mark under `key`
	{
		for (int g = 0; g < n_groups; ++g) {
			auto it = marks_.find(g * kMarkKeys + key);
			if (it != marks_.end() && it->second && !Check(hipStreamWaitEvent(st, it->second, 0), "hipStreamWaitEvent")) return false;
		}
		return true;
	}
	bool MarkFrame(int group, int slot) override { return Mark(group, slot); }
	bool WaitFrames(int slot, int n_groups) override { return WaitMarks(stream_, slot, n_groups); }
	bool GatherF32Async(void* stream, float* dst, const float* src, const int32_t* idx, size_t n) override
	{
		hipStream_t st = static_cast<hipStream_t>(stream);
		if (!GatherLaunch(st, dst, src, idx, n)) return false;
		if (!policy_ready_ && !Check(hipEventCreateWithFlags(&policy_ready_, hipEventDisableTiming), "hipEventCreate")) return false;
		return Check(hipEventRecord(policy_ready_, st), "hipEventRecord");
	}
	bool WaitPolicyReady(int group) override { return !policy_ready_ || Check(hipStreamWaitEvent(streams_[group], policy_ready_, 0), "hipStreamWaitEvent"); }
	bool SyncPolicyReady() override { return !policy_ready_ || Check(hipEventSynchronize(policy_ready_), "hipEventSynchronize"); }
	bool MarkWeightReader(int group, int wbuf) override { return Mark(group, kWeightReader + wbuf); }
	bool WaitWeightReaders(void* stream, int wbuf, int n_groups) override { return WaitMarks(stream ? static_cast<hipStream_t>(stream) : stream_, kWeightReader + wbuf, n_groups); }
	// The per-env launches of the frame boundary: one thread per env or row, 64 per workgroup, on the selected stream; `what` names the launch in the error text
	template <class... P, class... A>
	bool LaunchPerEnv(void (*kernel)(P...), int n, const char* what, const A&... args)
	{
		if (n <= 0) return true;
		hipLaunchKernelGGL(kernel, dim3((n + 63) / 64), dim3(64), 0, stream_, args...);
		return Check(hipGetLastError(), what);
	}
	// ONE launch per group and frame, whatever the rule: the batch's own terrain, one table entry per env (terrain sets), or the ladder's rule in front of that, in
	// the same launch. DTRL_TERRAINS_FALLBACK=1 takes the host default for the two forms with a table (A/B and cross-check)
	bool TerrainBoundary(const DevBuffers& buf, const EnvSpan& s, int mode, const TerrainRule& r) override
	{
		if (!r.table) return LaunchPerEnv(dtrl_terrain_boundary, s.n, "terrain boundary launch", buf, s.e0, s.n, mode, s.list);
		if (EnvFlag("DTRL_TERRAINS_FALLBACK")) return TerrainBoundaryLoop(buf, s, mode, r);
		if (!r.ladder) return LaunchPerEnv(dtrl_terrain_boundary_keyed, s.n, "keyed terrain boundary launch", buf, s.e0, s.n, mode, s.list, r.table, r.env_terrain);
		return LaunchPerEnv(dtrl_terrain_boundary_ladder, s.n, "ladder terrain boundary launch", buf, s.e0, s.n, mode, s.list, r.table, r.env_terrain, r.ladder, r.lc);
	}
	// variant redraw, variant rescale, push schedule, dtrl_add_perturb: ONE launch each, queued like the boundary work. DTRL_VARIANTS_FALLBACK=1 / DTRL_PUSH_FALLBACK=1 /
	// DTRL_PERTURB_FALLBACK=1 takes the host default
	bool VariantRedraw(const EnvStatus* status, const EnvSpan& s, int32_t* env_model, RedrawRec* recs, const RedrawCfg& cfg) override
	{
		if (EnvFlag("DTRL_VARIANTS_FALLBACK")) return Backend::VariantRedraw(status, s, env_model, recs, cfg);
		return LaunchPerEnv(dtrl_variant_redraw, s.n, "variant redraw launch", status, s.e0, s.n, s.list, env_model, recs, cfg);
	}
	// (one wavefront per env of the span)
	bool VariantRescale(const EnvStatus* status, const EnvSpan& s, const int32_t* env_model, DevModel* models, int key_base, RescaleRec* recs, const ModelScalarsD* base, const RescaleCfg& cfg) override
	{
		if (EnvFlag("DTRL_VARIANTS_FALLBACK")) return Backend::VariantRescale(status, s, env_model, models, key_base, recs, base, cfg);
		if (s.n <= 0) return true;
		hipLaunchKernelGGL(dtrl_variant_rescale, dim3(s.n), dim3(kGroup), 0, stream_, status, s.e0, s.n, s.list, env_model, models, key_base, recs, base, cfg);
		return Check(hipGetLastError(), "variant rescale launch");
	}
	bool PushSchedule(const EnvStatus* status, const EnvSpan& s, EnvState* st, PushRec* recs, const double* scale, const PushCfg& cfg) override
	{
		if (EnvFlag("DTRL_PUSH_FALLBACK")) return Backend::PushSchedule(status, s, st, recs, scale, cfg);
		return LaunchPerEnv(dtrl_push_schedule, s.n, "push schedule launch", status, s.e0, s.n, s.list, st, recs, scale, cfg);
	}
	// episode limit: ONE launch, queued in front of the boundary work. DTRL_EPISODE_FALLBACK=1 takes the host default
	bool EpisodeLimit(EnvStatus* status, const EnvSpan& s, EnvState* st, EpisodeRec* recs, const uint8_t* on, const EpisodeCfg& cfg) override
	{
		if (EnvFlag("DTRL_EPISODE_FALLBACK")) return Backend::EpisodeLimit(status, s, st, recs, on, cfg);
		return LaunchPerEnv(dtrl_episode_limit, s.n, "episode limit launch", status, s.e0, s.n, s.list, st, recs, on, cfg);
	}
	// frame trace: ONE launch per group and frame over the group's list of traced indices, ONE per read. DTRL_TRACE_FALLBACK=1 takes the host defaults
	bool TraceRecord(const EnvState* st, const EnvStatus* status, const TraceView& tv, const int32_t* list, int n) override
	{
		if (EnvFlag("DTRL_TRACE_FALLBACK")) return Backend::TraceRecord(st, status, tv, list, n);
		if (n <= 0) return true;
		hipLaunchKernelGGL(dtrl_trace_record, dim3(n), dim3(kGroup), 0, stream_, st, status, tv, list, n);
		return Check(hipGetLastError(), "trace record launch");
	}
	bool TraceGather(const TraceView& tv, const int32_t* list, int n, int max_rows, int row_stride, double* vals_out, int32_t* ints_out, int32_t* counts, bool dst_host) override
	{
		if (EnvFlag("DTRL_TRACE_FALLBACK")) return Backend::TraceGather(tv, list, n, max_rows, row_stride, vals_out, ints_out, counts, dst_host);
		if (n <= 0) return true;
		const int cap = std::min(max_rows, tv.frames);   // (the engine has checked that n x max(cap, 1) is a grid size)
		hipLaunchKernelGGL(dtrl_trace_gather, dim3(static_cast<unsigned>(n) * static_cast<unsigned>(std::max(cap, 1))), dim3(kGroup), 0, stream_, tv, list, n, cap, max_rows, row_stride, vals_out, ints_out, counts);
		return Check(hipGetLastError(), "trace gather launch") && Check(hipStreamSynchronize(stream_), "trace gather");
	}
	// episode log: ONE launch of one workgroup per group and frame; the listed form is a per-env launch. DTRL_EPISODE_LOG_FALLBACK=1 takes the host default
	bool EpisodeLog(const EnvState* st, const EnvStatus* status, const EnvSpan& s, const LogView& v) override
	{
		if (EnvFlag("DTRL_EPISODE_LOG_FALLBACK")) return Backend::EpisodeLog(st, status, s, v);
		if (!status) return LaunchPerEnv(dtrl_episode_log_start, s.n, "episode log start launch", s.e0, s.n, s.list, st, v.recs);
		if (s.n <= 0) return true;
		hipLaunchKernelGGL(dtrl_episode_log, dim3(1), dim3(kLogThreads), 0, stream_, st, status, s.e0, s.n, v);
		return Check(hipGetLastError(), "episode log launch");
	}
	bool PerturbScatter(EnvState* st, const PerturbRow* rows, int n) override
	{
		if (EnvFlag("DTRL_PERTURB_FALLBACK")) return Backend::PerturbScatter(st, rows, n);
		return LaunchPerEnv(dtrl_perturb_scatter, n, "perturb scatter launch", st, rows, n);
	}
	bool OrderByCost(const EnvStatus* status, int e0, int n, int32_t* order) override
	{
		if (n <= 0) return true;
		hipLaunchKernelGGL(dtrl_order_by_cost, dim3(1), dim3(kOrderBuckets), 0, stream_, status, e0, n, order);
		return Check(hipGetLastError(), "order launch");
	}
	bool Launch(const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end) override { return LaunchFrame(gm, rp, buf, n_envs, n_steps, dt, frame_end, FrameExtra{}); }
	// policy slots / model variants: ONE launch of the family's kernels (dtrl_backend_hip_slots.hip, dtrl_backend_hip_variants.hip) over the list as it stands -- the
	// group's costliest-first order is kept across keys. DTRL_SLOTS_FALLBACK=1 / DTRL_VARIANTS_FALLBACK=1 takes the per-key default instead (A/B and cross-check)
	bool LaunchKeyed(const DevModel* gm, const RunParams& rp, const DevBuffers& buf, const EnvKeyView& keys, int n_envs, int n_steps, real dt, bool frame_end) override
	{
		if (EnvFlag(keys.models_dev ? "DTRL_VARIANTS_FALLBACK" : "DTRL_SLOTS_FALLBACK")) return Backend::LaunchKeyed(gm, rp, buf, keys, n_envs, n_steps, dt, frame_end);
		FrameExtra x;
		if (keys.models_dev) { x.models = keys.models_dev; x.env_model = keys.env_key_dev; }
		else { x.slots = keys.slots_dev; x.env_slot = keys.env_key_dev; }
		return LaunchFrame(gm, rp, buf, n_envs, n_steps, dt, frame_end, x);
	}
	bool SlotReduce(const EnvState* st, const int32_t* env_slot, int n_envs, int n_slots, SlotSums* sums, int slot_base) override
	{
		const size_t recs = static_cast<size_t>(SlotReduceRows(n_envs) + 1) * kMaxSlots;
		if (slot_scratch_recs_ < recs) {
			if (slot_scratch_) hipFree(slot_scratch_);
			slot_scratch_ = nullptr; slot_scratch_recs_ = 0;
			if (!Check(hipMalloc(&slot_scratch_, sizeof(SlotSums) * recs), "hipMalloc")) return false;
			slot_scratch_recs_ = recs;
		}
		return Check(LaunchSlotReduce(stream_, st, env_slot, n_envs, n_slots, slot_base, slot_scratch_), "slot reduction launch")
			&& Check(hipMemcpyAsync(sums, slot_scratch_ + (recs - kMaxSlots), sizeof(SlotSums) * n_slots, hipMemcpyDeviceToHost, stream_), "hipMemcpy D2H") && Check(hipStreamSynchronize(stream_), "slot reduction");
	}
	bool LaunchFrame(const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end, const FrameExtra& extra)
	{
		// only stepping launches are timed (the compact 0-step reset launches would skew the per-frame average)
		const bool timed = n_steps > 0;
		std::pair<hipEvent_t, hipEvent_t> ev{};
		if (timed) {
			if (free_events_.empty()) { hipEventCreate(&ev.first); hipEventCreate(&ev.second); events_.push_back(ev); }
			else { ev = free_events_.back(); free_events_.pop_back(); }
			hipEventRecord(ev.first, stream_);
		}
		// the four families of frame kernels, a translation unit each (dtrl_frame_entry.h): model variants, policy slots, external policy mode, the shipped kernels
		const FrameLauncher launch = extra.models ? LaunchVariantFrame : extra.slots ? LaunchSlotFrame : buf.ext_envs != 0 ? LaunchExtFrame : LaunchPlainFrame;
		const hipError_t launched = launch(stream_, gm, rp, buf, n_envs, n_steps, dt, frame_end, extra);
		if (timed) {
			hipEventRecord(ev.second, stream_); pending_.push_back(ev);
			// a long run never asks for the timing: fold finished pairs into the running sum so the event pool stays bounded
			if (pending_.size() > kMaxPendingEvents) FoldFinished(false);
		}
		return Check(launched, "kernel launch");
	}
	bool Sync() override { bool ok = true; for (hipStream_t st : streams_) ok = Check(hipStreamSynchronize(st), "hipStreamSynchronize") && ok; return ok; }
	int NumStreams() const override { return kNumStreams; }
	void SelectStream(int sid) override { stream_ = streams_[(sid >= 0 && sid < kNumStreams) ? sid : 0]; }
	bool StreamIdle(int sid) override { return hipStreamQuery(streams_[(sid >= 0 && sid < kNumStreams) ? sid : 0]) == hipSuccess; }
	void KernelTime(double* avg_ms, int64_t* launches) override
	{
		for (hipStream_t st : streams_) hipStreamSynchronize(st);
		FoldFinished(true);
		if (avg_ms) *avg_ms = time_n_ > 0 ? time_sum_ms_ / time_n_ : 0.0;
		if (launches) *launches = time_n_;
		time_sum_ms_ = 0; time_n_ = 0;
	}
	const char* Name() const override { return "hip"; }
private:
	// move the event pairs whose launch has completed (all of them when `all`: the streams were synchronised) into the running sum
	void FoldFinished(bool all)
	{
		size_t keep = 0;
		for (size_t i = 0; i < pending_.size(); ++i) {
			auto& ev = pending_[i];
			if (all || hipEventQuery(ev.second) == hipSuccess) {
				float ms = 0;
				if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) { time_sum_ms_ += ms; ++time_n_; }
				free_events_.push_back(ev);
			} else pending_[keep++] = ev;
		}
		pending_.resize(keep);
	}
	static constexpr size_t kMaxPendingEvents = 64;
	double time_sum_ms_ = 0; int64_t time_n_ = 0;
	bool Check(hipError_t e, const char* what) { if (e == hipSuccess) return true; err_ = std::string(what) + ": " + hipGetErrorString(e); return false; }
	static constexpr int kNumStreams = 8;
	int reserve_arg_ = -1;             // -reserve_cus= (else DTRL_RESERVE_CUS)
	bool masked_ = false, calibrated_ = false;
	hipStream_t side_[2] = {nullptr, nullptr};
	std::vector<hipStream_t> extra_, owned_;
	std::vector<double> side_delay_us_;
	std::vector<hipStream_t> streams_;
	hipStream_t stream_ = nullptr;   // the selected one
	std::vector<std::pair<hipEvent_t, hipEvent_t>> events_, free_events_, pending_;
	int32_t* ext_rej_ = nullptr; double ext_ms_[2] = {0, 0};   // external policy mode: rejected-row counter (device), device time of the collection / scatter launches
	hipEvent_t timed_ev_[2] = {nullptr, nullptr};   // TimedBegin / TimedEnd
	double snap_ms_ = 0;   // device time of the snapshot launches since the last SnapLaunchMs()
	SlotSums* slot_scratch_ = nullptr; size_t slot_scratch_recs_ = 0;   // dtrl_slot_stats: partial rows + totals (device)
	hipEvent_t policy_ready_ = nullptr;   // behind the latest asynchronous policy gather (GatherF32Async)
	std::map<int, hipEvent_t> marks_;   // group * kMarkKeys + key -> event (Mark / WaitMarks)
};

Backend* MakeBackend() { return new HipBackend(); }

}  // namespace dtrl
