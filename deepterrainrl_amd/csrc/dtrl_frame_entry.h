// dtrl_frame_entry.h -- what the four translation units that instantiate the frame kernels share (dtrl_backend_hip_frame.hip: internal policy mode, the shipped
// kernels; dtrl_backend_hip_ext.hip: external policy mode; dtrl_backend_hip_slots.hip: policy slots; dtrl_backend_hip_variants.hip: model variants): the register budget of the fast kernels, the kernels' entry
// body, and the host-side choice among a unit's three kernels. The entry body is shared as TEXT (a macro), not through a call: moved into a __forceinline__
// function template it compiles to other instructions in the fast kernels (docs/EXPERIMENTS.md 19), and tools/asm_same.py holds them fixed.
#pragma once
#include "dtrl_kernel.h"
#include "dtrl_topo.h"
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>

namespace dtrl {

#ifndef DTRL_WAVES_PER_EU
#define DTRL_WAVES_PER_EU 2
#endif
#ifndef DTRL_WAVES_DOG
#define DTRL_WAVES_DOG DTRL_WAVES_PER_EU
#endif
#ifndef DTRL_WAVES_RAPTOR
#define DTRL_WAVES_RAPTOR DTRL_WAVES_PER_EU
#endif
template <class Topo> struct WavesPerEu { static constexpr int value = DTRL_WAVES_PER_EU; };
template <> struct WavesPerEu<TopoDog> { static constexpr int value = DTRL_WAVES_DOG; };          // (the fp32 build gives each skeleton's instance its own register budget:
template <> struct WavesPerEu<TopoRaptor> { static constexpr int value = DTRL_WAVES_RAPTOR; };    //  profiles/r06_fp32_physics.txt)

// Workspace of a fast kernel. Experiment builds (docs/EXPERIMENTS.md 13, tools/occupancy_ab.sh; never the shipped library): -DDTRL_DYN_LDS puts it into DYNAMIC
// LDS, so that the compiler no longer derives "two waves per SIMD at most" from the 20 KB static allocation and honours -DDTRL_WAVES_PER_EU=3 (<= 168 registers
// per lane): the register diet a third wave per SIMD would need, priced at unchanged occupancy. Run-time knob of the shipped kernels: DTRL_LDS_PAD=<bytes> of
// dynamic LDS on top (fewer workgroups per CU: the throughput-vs-occupancy curve from the other side).
#if defined(DTRL_DYN_LDS)
#define DTRL_WS_FAST extern __shared__ __align__(16) unsigned char dtrl_dyn_lds[]; WSFast& ws = *reinterpret_cast<WSFast*>(dtrl_dyn_lds)
#else
#define DTRL_WS_FAST __shared__ WSFast ws
#endif
// the frame code exists in the device pass only (the fast path is written in gfx950 builtins)
#if defined(__HIP_DEVICE_COMPILE__)
#define DTRL_DEVICE_ONLY(...) __VA_ARGS__
#else
#define DTRL_DEVICE_ONLY(...)
#endif

// one 64-lane workgroup = one env of the launch list; PRE runs in front of the frame (it may rewrite the kernel's own copies of rp / buf and re-point gm)
#define DTRL_FRAME_BODY(WS, PATH, EXT, PRE) \
	WS; \
	if (static_cast<int>(blockIdx.x) >= n_envs) return; \
	const int env = buf.env_list ? buf.env_list[blockIdx.x] : static_cast<int>(blockIdx.x); \
	DTRL_DEVICE_ONLY(PRE; env_frame_impl<PATH, EXT>(ws, *gm, rp, buf, env, n_steps, dt, frame_end != 0);)

// Defines the kernel pair NAME (the LDS-phase reference form, dtrl_kernel.h) and NAME_fast<Topo> (the register-resident fast path, dtrl_kernel_fast.h: one
// instantiation per skeleton of the shipped characters, dtrl_topo.h). EXT: env_frame_impl's external-policy flag; PRE: one statement in front of the frame (may
// be empty); the variadic rest: kernel parameters behind frame_end. Needs dtrl_kernel_fast.h in front of its use.
#define DTRL_FRAME_KERNELS(NAME, EXT, PRE, ...) \
__global__ void __launch_bounds__(kGroup) NAME(const DevModel* __restrict__ gm, RunParams rp, DevBuffers buf, int n_envs, int n_steps, real dt, int frame_end, ##__VA_ARGS__) \
{ \
	DTRL_FRAME_BODY(__shared__ WSRef ws, RefPath, EXT, PRE) \
} \
template <class Topo> \
__global__ void __launch_bounds__(kGroup, WavesPerEu<Topo>::value) NAME##_fast(const DevModel* __restrict__ gm, RunParams rp, DevBuffers buf, int n_envs, int n_steps, real dt, int frame_end, ##__VA_ARGS__) \
{ \
	DTRL_FRAME_BODY(DTRL_WS_FAST, FastPath<Topo>, EXT, PRE) \
}

// dynamic LDS of a fast-path launch: 0 in the shipped library; the workspace itself (ws_bytes) in a -DDTRL_DYN_LDS experiment build; plus DTRL_LDS_PAD bytes
inline unsigned FastDynLds(unsigned ws_bytes)
{
	static const unsigned bytes = [ws_bytes]() {
		unsigned b = 0;
#if defined(DTRL_DYN_LDS)
		b = ws_bytes;
#else
		(void)ws_bytes;
#endif
		if (const char* e = std::getenv("DTRL_LDS_PAD")) b += static_cast<unsigned>(std::atoi(e));
		return b;
	}();
	return bytes;
}

// Launches the one of a unit's three kernels that the model's skeleton asks for, on `stream`, one workgroup per env; `extra`: the kernels' parameters behind
// frame_end. DTRL_KERNEL=ref selects the reference form (A/B and bitwise cross-check; read per launch: a test switches it inside one process).
template <class... Extra> using FrameKernel = void (*)(const DevModel*, RunParams, DevBuffers, int, int, real, int, Extra...);
template <class... Extra>
hipError_t LaunchFrameKernel(FrameKernel<Extra...> ref, FrameKernel<Extra...> dog, FrameKernel<Extra...> raptor, unsigned ws_bytes, hipStream_t stream,
	const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end, Extra... extra)
{
	const char* sel = std::getenv("DTRL_KERNEL");
	const bool use_ref = sel && std::strcmp(sel, "ref") == 0;
	const FrameKernel<Extra...> k = use_ref ? ref : buf.model_topo == TopoDog::kId ? dog : buf.model_topo == TopoRaptor::kId ? raptor : ref;
	hipLaunchKernelGGL(k, dim3(n_envs), dim3(kGroup), k == ref ? 0u : FastDynLds(ws_bytes), stream, gm, rp, buf, n_envs, n_steps, dt, frame_end ? 1 : 0, extra...);
	return hipGetLastError();
}

// the units' launchers, one signature (HipBackend::LaunchFrame chooses). FrameExtra: what the kernels of a family take behind the common parameters, all device
// memory -- slots / env_slot: read by the slot unit's kernels only (env e runs under the record slots[env_slot[e]]); models / env_model: read by the variant
// unit's kernels only (env e runs under the model models[env_model[e]])
struct SlotRec;
struct FrameExtra { const SlotRec* slots = nullptr; const int32_t* env_slot = nullptr; const DevModel* models = nullptr; const int32_t* env_model = nullptr; };
using FrameLauncher = hipError_t (*)(hipStream_t stream, const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end, const FrameExtra& extra);
hipError_t LaunchPlainFrame(hipStream_t stream, const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end, const FrameExtra&);
hipError_t LaunchExtFrame(hipStream_t stream, const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end, const FrameExtra&);
hipError_t LaunchSlotFrame(hipStream_t stream, const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end, const FrameExtra& extra);
hipError_t LaunchVariantFrame(hipStream_t stream, const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end, const FrameExtra& extra);

}  // namespace dtrl
