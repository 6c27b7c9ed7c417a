// dtrl_launch_cfg.h -- register budget of the fast frame kernels, shared by the translation units that instantiate them (dtrl_backend_hip.hip: internal policy
// mode; dtrl_backend_hip_ext.hip: external policy mode; dtrl_backend_hip_slots.hip: policy slots)
#pragma once
#include "dtrl_kernel.h"
#include "dtrl_topo.h"

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

// launches the external-mode instantiation of the frame kernel (dtrl_backend_hip_ext.hip) on `stream` (a hipStream_t); use_ref: the LDS-phase reference form
bool LaunchExtFrame(void* stream, bool use_ref, unsigned dyn_lds, const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end);

// policy slots (dtrl_backend_hip_slots.hip): the slot instantiation of the frame kernel, env e under the record slots[env_slot[e]] (both device memory) ...
struct SlotRec; struct SlotSums;
bool LaunchSlotFrame(void* stream, bool use_ref, unsigned dyn_lds, const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end,
	const SlotRec* slots, const int32_t* env_slot);
// ... and the per-slot sums of dtrl_slot_stats: two launches on `stream`; scratch is device memory for (SlotReduceRows(n_envs) + 1) * kMaxSlots SlotSums records,
// the totals are its last kMaxSlots records
constexpr int kSlotReduceMaxRows = 64;
int SlotReduceRows(int n_envs);
bool LaunchSlotReduce(void* stream, const EnvState* st, const int32_t* env_slot, int n_envs, int n_slots, SlotSums* scratch);

}  // namespace dtrl
