// kernel_select.h — the kernel selectors (kernel_select.hip), one per templated family: plain
// arguments in, the host function pointer of exactly that instantiation out, nullptr for a
// combination no unit compiles. They decide nothing; which arguments a frame or a query asks
// for is its launch function's policy, and a launch site turns nullptr into PBRT_E_HIP before
// it launches anything. pbrt_diag_kernel_choice reads them, and tests/test_kernel_selectors.py
// holds each table equal to the compiled instantiations.
#pragma once

#include "render_kernels.h"

#pragma GCC visibility push(hidden)   // the host units' own: not among the library's exported symbols
namespace pbrtk {

using ChainKernel = decltype(&k_chain_ci<1>);
using PathsCiKernel = decltype(&k_paths_ci<4>);
using PathsCamKernel = decltype(&k_paths_cam<4, false>);
using LiKernel = decltype(&k_li<false, 0>);
using LiStratKernel = decltype(&k_li_strat<false, 0>);
using DirectLiKernel = decltype(&k_li_direct<false, 0>);
using PathStepKernel = decltype(&k_path_step<false, 0>);
using SerialKernel = decltype(&k_render_exact<1>);

ChainKernel chain_kernel(int w, int depth, bool kx, int eu, bool spwin, bool multi);
PathsCiKernel paths_ci_kernel(int P, bool mb, bool kx);
// dynamic LDS of a k_paths_ci<P> workgroup that stages `staged_values` stratified values (-1: no such P)
int paths_ci_lds(int P, int staged_values);
PathsCamKernel paths_cam_kernel(int P, bool mb, bool stack);   // stack: k_paths_cam_stack
// the device queries: kDepth 0 on an LDS-staged tree, 64 beyond (li_query.h: kernel_args)
LiKernel li_kernel(bool kx, int depth);
LiStratKernel li_strat_kernel(bool kx, int depth);
DirectLiKernel direct_li_kernel(bool kx, int depth);
PathStepKernel path_step_kernel(bool kx, int depth);
SerialKernel serial_kernel(int min_waves);   // the amdgpu_waves_per_eu builds of k_render_exact

// the launch log's name of a kernel by its host function pointer (pbrt_gpu_launch_log)
const char* kernel_name_of(const void* fn, const char* unknown = "?");
// the kernels diag.hip defines (k_probe), for the names above
const KernelName* diag_kernel_names(size_t* n);

}  // namespace pbrtk
#pragma GCC visibility pop
