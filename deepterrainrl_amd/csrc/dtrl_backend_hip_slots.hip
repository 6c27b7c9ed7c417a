// dtrl_backend_hip_slots.hip -- the frame kernels of a batch with policy slots (include/dtrl.h dtrl_slots_create): the device code of dtrl_kernel.h /
// dtrl_kernel_fast.h behind a per-env choice of policy. A translation unit of its own for the reason dtrl_backend_hip_frame.hip is one: a second caller of the
// shared inline functions in a unit changes what the compiler inlines into the first.
//
// A wavefront is one env. It reads its env's slot, makes the number wave-uniform (readfirstlane: the record then comes through scalar loads, like the kernel
// arguments it replaces), patches its private copies of `rp` and `buf` (slot_patch, dtrl_engine.h) and runs the unchanged env_frame_impl<Path, false>.
#include "dtrl_engine.h"
#include "dtrl_kernel_fast.h"
#include "dtrl_frame_entry.h"

namespace dtrl {

__device__ __forceinline__ void slot_select(const SlotRec* __restrict__ slots, const int32_t* __restrict__ env_slot, int env, RunParams& rp, DevBuffers& buf)
{
#if defined(__HIP_DEVICE_COMPILE__)
	const int s = __builtin_amdgcn_readfirstlane(env_slot[env]);
	slot_patch(slots[s], rp, buf);
#endif
}

DTRL_FRAME_KERNELS(dtrl_slot_frame_kernel, false, slot_select(slots, env_slot, env, rp, buf), const SlotRec* __restrict__ slots, const int32_t* __restrict__ env_slot)

hipError_t LaunchSlotFrame(hipStream_t stream, const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end, const FrameExtra& extra)
{
	return LaunchFrameKernel(dtrl_slot_frame_kernel, dtrl_slot_frame_kernel_fast<TopoDog>, dtrl_slot_frame_kernel_fast<TopoRaptor>, sizeof(WSFast), stream, gm, rp, buf, n_envs, n_steps, dt, frame_end,
		extra.slots, extra.env_slot);
}

}  // namespace dtrl
