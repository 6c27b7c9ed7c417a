// dtrl_backend_hip_frame.hip -- the shipped frame kernels (internal policy mode, one policy) and their launcher, and nothing else.
//
// Launch geometry: one 64-lane wavefront (one workgroup) per environment, so every __syncthreads() in the lane-phase
// code is a single-wave barrier; a 4096-env batch is 4096 workgroups (16 per CU), enough to fill all 256 CUs / 8 XCDs.
// Workgroup b lands on XCD b % 8 (observed dispatch order), i.e. consecutive envs spread across XCDs and each XCD's L2
// holds only its own envs' state/terrain records -- the per-env records are private, nothing is shared between XCDs
// except the read-only model and policy weights.
//
// Why a unit of its own: what the compiler inlines into these kernels depends on who else in the translation unit calls the inline functions of dtrl_kernel.h /
// dtrl_kernel_fast.h. Alone here, they stay the instructions they were whatever the host class, the auxiliary kernels (dtrl_backend_hip.hip) and the other
// instantiations (dtrl_backend_hip_ext.hip, dtrl_backend_hip_slots.hip) become (tools/asm_same.py).
#include "dtrl_kernel_fast.h"
#include "dtrl_frame_entry.h"

namespace dtrl {

DTRL_FRAME_KERNELS(dtrl_frame_kernel, false, )

hipError_t LaunchPlainFrame(hipStream_t stream, const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end, const FrameExtra&)
{
	return LaunchFrameKernel<>(dtrl_frame_kernel, dtrl_frame_kernel_fast<TopoDog>, dtrl_frame_kernel_fast<TopoRaptor>, sizeof(WSFast), stream, gm, rp, buf, n_envs, n_steps, dt, frame_end);
}

}  // namespace dtrl
