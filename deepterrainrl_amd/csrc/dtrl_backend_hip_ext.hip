// dtrl_backend_hip_ext.hip -- the frame kernels of external policy mode (-policy_mode= external): the device code of dtrl_kernel.h / dtrl_kernel_fast.h with the
// park / resume hand-over compiled in (env_frame_impl<Path, true>). A translation unit of its own for the reason dtrl_backend_hip_frame.hip is one: a second
// caller of the shared inline functions in a unit changes what the compiler inlines into the first.
#include "dtrl_kernel_fast.h"
#include "dtrl_frame_entry.h"

namespace dtrl {

DTRL_FRAME_KERNELS(dtrl_ext_frame_kernel, true, )

hipError_t LaunchExtFrame(hipStream_t stream, const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end, const FrameExtra&)
{
	return LaunchFrameKernel<>(dtrl_ext_frame_kernel, dtrl_ext_frame_kernel_fast<TopoDog>, dtrl_ext_frame_kernel_fast<TopoRaptor>, sizeof(WSFast), stream, gm, rp, buf, n_envs, n_steps, dt, frame_end);
}

}  // namespace dtrl
