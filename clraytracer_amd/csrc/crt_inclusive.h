// crt_inclusive.h -- the device queries under the inclusive box test (CRT_RAYS_INCLUSIVE, CRT_AO_INCLUSIVE; definition: include/crt_api.h):
// the kernels' declarations. They are crt_rays_body / crt_ao_body (crt_rays.h, crt_ao.h) with INCLUSIVE = true -- intersect_aabb<true> in
// every box test, nothing else -- compiled in a translation unit of their own (crt_inclusive.hip, the fourth of libcrt_hip.so), so that the
// device code of the other three units is the same with and without them. Arguments, grid, cull, ctl: those of the plain kernels; launched
// from crt_query_host.h / crt_ao_host.h through the same launch_query. crt_ao_filter_kernel serves both rules as it is.
#pragma once
#include "crt_rays.h"
#include "crt_ao.h"

template <bool ANYHIT, bool TLAS> __global__ void crt_rays_inclusive_kernel(CrtDevScene S0, CrtRaysArgs A);
template <int SOURCE, bool TLAS> __global__ void crt_ao_inclusive_kernel(CrtDevScene S0, CrtAoArgs A, CrtFrame F);
