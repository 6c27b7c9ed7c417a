// dtrl_backend_hip_slots.hip -- the frame kernels of a batch with policy slots (include/dtrl.h dtrl_slots_create): the device code of dtrl_kernel.h /
// dtrl_kernel_fast.h behind a per-env choice of policy, and the per-slot statistics reduction of dtrl_slot_stats. A translation unit of its own for the reason
// dtrl_backend_hip_ext.hip is one: a second caller of the shared inline functions in the unit of the shipped kernels changes what the compiler inlines into
// them -- kept apart, the single-policy kernels stay the instructions they were (tools/asm_same.py --only dtrl_frame_kernel).
//
// A wavefront is one env. It reads its env's slot, makes the number wave-uniform (readfirstlane: the record then comes through scalar loads, like the kernel
// arguments it replaces), patches its private copies of `rp` and `buf` (slot_patch, dtrl_engine.h) and runs the unchanged env_frame_impl<Path, false>.
#include "dtrl_engine.h"
#include "dtrl_kernel_fast.h"
#include "dtrl_launch_cfg.h"
#include <hip/hip_runtime.h>

namespace dtrl {

__device__ __forceinline__ void slot_select(const SlotRec* __restrict__ slots, const int32_t* __restrict__ env_slot, int env, RunParams& rp, DevBuffers& buf)
{
#if defined(__HIP_DEVICE_COMPILE__)
	const int s = __builtin_amdgcn_readfirstlane(env_slot[env]);
	slot_patch(slots[s], rp, buf);
#endif
}

__global__ void __launch_bounds__(kGroup) dtrl_slot_frame_kernel(const DevModel* __restrict__ gm, RunParams rp, DevBuffers buf, int n_envs, int n_steps, real dt, int frame_end,
	const SlotRec* __restrict__ slots, const int32_t* __restrict__ env_slot)
{
	__shared__ WSRef ws;
	if (static_cast<int>(blockIdx.x) >= n_envs) return;
	const int env = buf.env_list ? buf.env_list[blockIdx.x] : static_cast<int>(blockIdx.x);
	slot_select(slots, env_slot, env, rp, buf);
	env_frame_impl<RefPath, false>(ws, *gm, rp, buf, env, n_steps, dt, frame_end != 0);
}

template <class Topo>
__global__ void __launch_bounds__(kGroup, WavesPerEu<Topo>::value) dtrl_slot_frame_kernel_fast(const DevModel* __restrict__ gm, RunParams rp, DevBuffers buf, int n_envs, int n_steps, real dt, int frame_end,
	const SlotRec* __restrict__ slots, const int32_t* __restrict__ env_slot)
{
#if defined(DTRL_DYN_LDS)
	extern __shared__ __align__(16) unsigned char dtrl_dyn_lds[];
	WSFast& ws = *reinterpret_cast<WSFast*>(dtrl_dyn_lds);
#else
	__shared__ WSFast ws;
#endif
	if (static_cast<int>(blockIdx.x) >= n_envs) return;
	const int env = buf.env_list ? buf.env_list[blockIdx.x] : static_cast<int>(blockIdx.x);
#if defined(__HIP_DEVICE_COMPILE__)
	slot_select(slots, env_slot, env, rp, buf);
	env_frame_impl<FastPath<Topo>, false>(ws, *gm, rp, buf, env, n_steps, dt, frame_end != 0);
#endif
}

bool LaunchSlotFrame(void* stream, bool use_ref, unsigned dyn_lds, const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end,
	const SlotRec* slots, const int32_t* env_slot)
{
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (!use_ref && buf.model_topo == TopoDog::kId)
		hipLaunchKernelGGL(dtrl_slot_frame_kernel_fast<TopoDog>, dim3(n_envs), dim3(kGroup), dyn_lds, st, gm, rp, buf, n_envs, n_steps, dt, frame_end ? 1 : 0, slots, env_slot);
	else if (!use_ref && buf.model_topo == TopoRaptor::kId)
		hipLaunchKernelGGL(dtrl_slot_frame_kernel_fast<TopoRaptor>, dim3(n_envs), dim3(kGroup), dyn_lds, st, gm, rp, buf, n_envs, n_steps, dt, frame_end ? 1 : 0, slots, env_slot);
	else
		hipLaunchKernelGGL(dtrl_slot_frame_kernel, dim3(n_envs), dim3(kGroup), 0, st, gm, rp, buf, n_envs, n_steps, dt, frame_end ? 1 : 0, slots, env_slot);
	return hipGetLastError() == hipSuccess;
}

// ---- dtrl_slot_stats: per-slot sums over the EnvState records, on the device ----
// dtrl_slot_partials: the workgroups' wavefronts stride over the envs; per pass a wavefront folds, slot by slot, its 64 lanes' contributions with a butterfly of
// shuffles and lane 0 adds the result to the wavefront's row in LDS; the workgroup then adds its wavefronts' rows in wavefront order and writes ONE row of
// partials. dtrl_slot_final (one workgroup) adds the rows in workgroup order. No atomics anywhere: every sum has one fixed order, the bytes repeat from call to call.
constexpr int kReduceThreads = 256, kReduceWaves = kReduceThreads / 64;

__device__ __forceinline__ long long wave_sum(long long v) { for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64); return v; }
__device__ __forceinline__ double wave_sum(double v) { for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64); return v; }

__global__ void __launch_bounds__(kReduceThreads) dtrl_slot_partials(const EnvState* __restrict__ st, const int32_t* __restrict__ env_slot, int n_envs, int n_slots, SlotSums* __restrict__ rows)
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
			s = env_slot[e];
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

int SlotReduceRows(int n_envs) { const int g = (n_envs + kReduceThreads - 1) / kReduceThreads; return g < 1 ? 1 : (g > kSlotReduceMaxRows ? kSlotReduceMaxRows : g); }

// scratch: device memory for (SlotReduceRows(n_envs) + 1) * kMaxSlots records; the totals land in its last kMaxSlots records
bool LaunchSlotReduce(void* stream, const EnvState* st, const int32_t* env_slot, int n_envs, int n_slots, SlotSums* scratch)
{
	hipStream_t s = static_cast<hipStream_t>(stream);
	const int rows = SlotReduceRows(n_envs);
	hipLaunchKernelGGL(dtrl_slot_partials, dim3(rows), dim3(kReduceThreads), 0, s, st, env_slot, n_envs, n_slots, scratch);
	hipLaunchKernelGGL(dtrl_slot_final, dim3(1), dim3(64), 0, s, scratch, rows, n_slots, scratch + static_cast<size_t>(rows) * kMaxSlots);
	return hipGetLastError() == hipSuccess;
}

}  // namespace dtrl
