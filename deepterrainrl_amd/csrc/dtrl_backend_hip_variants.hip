// dtrl_backend_hip_variants.hip -- the frame kernels of a batch with model variants (include/dtrl.h dtrl_variants_create): the device code of dtrl_kernel.h /
// dtrl_kernel_fast.h behind a per-env choice of character model. A translation unit of its own for the reason dtrl_backend_hip_frame.hip is one: a second caller
// of the shared inline functions in a unit changes what the compiler inlines into the first.
//
// A wavefront is one env. It reads its env's variant, makes the number wave-uniform (readfirstlane: the record's address then lives in scalar registers and the
// record comes through scalar loads, like the single record it replaces), re-points `gm` at that record of the table and runs the unchanged
// env_frame_impl<Path, false>. The host has checked every entry of env_model against the table's size (Engine::AssignVariants).
#include "dtrl_kernel_fast.h"
#include "dtrl_frame_entry.h"

namespace dtrl {

__device__ __forceinline__ const DevModel* var_select(const DevModel* __restrict__ models, const int32_t* __restrict__ env_model, int env)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return models + __builtin_amdgcn_readfirstlane(env_model[env]);
#else
	return models;
#endif
}

DTRL_FRAME_KERNELS(dtrl_var_frame_kernel, false, gm = var_select(models, env_model, env), const DevModel* __restrict__ models, const int32_t* __restrict__ env_model)

hipError_t LaunchVariantFrame(hipStream_t stream, const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end, const FrameExtra& extra)
{
	return LaunchFrameKernel(dtrl_var_frame_kernel, dtrl_var_frame_kernel_fast<TopoDog>, dtrl_var_frame_kernel_fast<TopoRaptor>, sizeof(WSFast), stream, gm, rp, buf, n_envs, n_steps, dt, frame_end,
		extra.models, extra.env_model);
}

}  // namespace dtrl
