// orp_conv3x3_bn_host.hpp -- what the host sides of the three fused conv2 kernels (orp_conv3x3_bn{,_deep,_s2}.hip) share.  Host code
// only: each file keeps its kernel, its Args, its channel / stride rule (`ok`), its tile arithmetic with the 2^31 guards and its table.
#pragma once
#include "../../include/orp_hip.h"
#include "orp_launch.hpp"
#include "orp_dcn_split.hpp"

namespace orp_conv3x3 {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
constexpr int kThreads = 512;      // eight waves, every kernel of the family

// the packed weight: two fp16 planes [2][tap][C/16][2][C][8] (4 bytes per weight), then 16 bytes that hold the planes' scale.
// ok: the file's own rule for (c_in, c_out) -- a packer refuses the other kernels' shapes
inline size_t packed_bytes(int ok, int c_in, int c_out) { return ok ? (size_t)4 * c_in * c_out * 9 + 16 : 0; }
inline int pack_weight(int ok, const float* weight, int c_in, int c_out, void* packed, void* stream) {
  if (!weight || !packed || ((uintptr_t)packed & 15) || !ok) return ORP_EINVAL;
  uint16_t* planes = reinterpret_cast<uint16_t*>(packed);
  const size_t n = (size_t)c_in * c_out * 9;
  hipError_t e = orp_split::pack_planes16(weight, c_out, c_in, 9, planes, reinterpret_cast<float*>(planes + 2 * n), (hipStream_t)stream);
  return e == hipSuccess ? ORP_OK : (int)e;
}

// what every entry point refuses with ORP_EINVAL, next to its own `ok`
inline bool bad_launch_args(const float* x, const void* weight_packed, const float* scale, const float* shift, const uint32_t* range_in,
                            const float* y, int batch, int height, int width) {
  return !x || !weight_packed || ((uintptr_t)weight_packed & 15) || !scale || !shift || !range_in || !y || y == x || batch <= 0 ||
         height <= 0 || width <= 0;
}

// the fields the three Args have in common (the types stay distinct: each kernel's kernarg layout is its own)
template <class Args>
void fill_common(Args& A, const float* x, const void* weight_packed, const float* scale, const float* shift, const uint32_t* range_in,
                 float* y, int c_in, int c_out, int height, int width, int relu) {
  A.x = x; A.scale = scale; A.shift = shift; A.y = y; A.range = range_in;
  A.planes = reinterpret_cast<const uint16_t*>(weight_packed);
  A.plane_stride = (size_t)c_out * c_in * 9;
  A.wscale = reinterpret_cast<const float*>(A.planes + 2 * A.plane_stride);
  A.H = height; A.W = width; A.relu = relu ? 1 : 0;
}

// a row of a routing table, at one key (the file says which: channels or stride) and batch: only square maps were timed, so a map
// is routed where BOTH sides lie inside [side_min, side_max] and no further
struct PaidSquare { int key, side_min, side_max, batch; };
template <size_t N>
int paid(const PaidSquare (&rows)[N], int key, int height, int width, int batch) {
  for (const PaidSquare& s : rows)
    if (s.key == key && s.batch == batch && height >= s.side_min && height <= s.side_max && width >= s.side_min && width <= s.side_max)
      return 1;
  return 0;
}

// one instantiation's launch: `grid` workgroups with `smem` bytes of dynamic LDS.  Tag: a type of the call site, one per instantiation
// (set_max_dynamic_lds_once keeps one flag array per Tag)
template <class Tag, class Args>
hipError_t launch_with_lds(void (*kernel)(const Args), long grid, size_t smem, hipStream_t st, const Args& A) {
  hipError_t e = orp::set_max_dynamic_lds_once<Tag>(reinterpret_cast<const void*>(kernel), smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kThreads), smem, st, A);
  return hipGetLastError();
}

}  // namespace orp_conv3x3
