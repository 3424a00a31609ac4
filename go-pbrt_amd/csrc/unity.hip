// unity.hip — every translation unit of the library as one, for the diagnostics
// and experiment builds (Makefile: steptime, meshcount, diag, variant), whose
// __device__ counters must exist once. The kernel definitions come before the
// host units (kernel_select.hip, render.hip, queries.hip, diag.hip, group.hip):
// their launch bounds must be on the first declaration a kernel sees
// (render_kernels.h's plain declarations first would leave every kernel at the
// default 1024-thread bound, i.e. 128 VGPRs, and spilling).
#include "mesh_bvh.hip"
#include "k_chain_1.hip"
#include "k_chain_n.hip"
#include "k_chain_x.hip"
#include "k_chain_g.hip"
#include "k_paths_m.hip"
#include "k_paths_x.hip"
#include "k_chain_c.hip"
#include "k_paths_c.hip"
#include "k_serial.hip"
#include "k_pw.hip"
#include "k_frame.hip"
#include "k_group.hip"
#include "k_query.hip"
#include "k_li.hip"
#include "k_li_direct.hip"
#include "k_path_step.hip"
#include "k_film_q.hip"
#include "k_strat.hip"
#include "kernel_select.hip"
#include "render.hip"
#include "queries.hip"
#include "diag.hip"
#include "group.hip"
