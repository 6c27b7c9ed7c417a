// dtrl_backend_hip_ext.hip -- the frame kernels of external policy mode (-policy_mode= external): the device code of dtrl_kernel.h / dtrl_kernel_fast.h with the
// park / resume hand-over compiled in (env_frame_impl<Path, true>). A translation unit of its own: the internal-mode kernels of dtrl_backend_hip.hip share every
// inline function with these, and a second caller in the same unit changes what the compiler inlines into them -- kept apart, the shipped kernels stay the
// instructions they were (tools/asm_same.py --only dtrl_frame_kernel).
#include "dtrl_engine.h"
#include "dtrl_kernel_fast.h"
#include "dtrl_launch_cfg.h"
#include <hip/hip_runtime.h>

namespace dtrl {

__global__ void __launch_bounds__(kGroup) dtrl_ext_frame_kernel(const DevModel* __restrict__ gm, RunParams rp, DevBuffers buf, int n_envs, int n_steps, real dt, int frame_end)
{
	__shared__ WSRef ws;
	if (static_cast<int>(blockIdx.x) >= n_envs) return;
	const int env = buf.env_list ? buf.env_list[blockIdx.x] : static_cast<int>(blockIdx.x);
	env_frame_impl<RefPath, true>(ws, *gm, rp, buf, env, n_steps, dt, frame_end != 0);
}

template <class Topo>
__global__ void __launch_bounds__(kGroup, WavesPerEu<Topo>::value) dtrl_ext_frame_kernel_fast(const DevModel* __restrict__ gm, RunParams rp, DevBuffers buf, int n_envs, int n_steps, real dt, int frame_end)
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
	env_frame_impl<FastPath<Topo>, true>(ws, *gm, rp, buf, env, n_steps, dt, frame_end != 0);
#endif
}

bool LaunchExtFrame(void* stream, bool use_ref, unsigned dyn_lds, const DevModel* gm, const RunParams& rp, const DevBuffers& buf, int n_envs, int n_steps, real dt, bool frame_end)
{
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (!use_ref && buf.model_topo == TopoDog::kId)
		hipLaunchKernelGGL(dtrl_ext_frame_kernel_fast<TopoDog>, dim3(n_envs), dim3(kGroup), dyn_lds, st, gm, rp, buf, n_envs, n_steps, dt, frame_end ? 1 : 0);
	else if (!use_ref && buf.model_topo == TopoRaptor::kId)
		hipLaunchKernelGGL(dtrl_ext_frame_kernel_fast<TopoRaptor>, dim3(n_envs), dim3(kGroup), dyn_lds, st, gm, rp, buf, n_envs, n_steps, dt, frame_end ? 1 : 0);
	else
		hipLaunchKernelGGL(dtrl_ext_frame_kernel, dim3(n_envs), dim3(kGroup), 0, st, gm, rp, buf, n_envs, n_steps, dt, frame_end ? 1 : 0);
	return hipGetLastError() == hipSuccess;
}

}  // namespace dtrl
