// orp_conv1x1_bn_host.hpp -- what the host sides of orp_conv1x1_bn.hip (fp32 MFMA) and orp_conv1x1_bn_pieces.hip (bf16 pieces) share:
// the argument rules of their entry points, the fields their kernel arguments have in common, the choice of a tile's instantiation
// (RANGE, MODE, VEC) and the row type of their routing tables.  Host code only; each file keeps its kernels, its Args, its pick_tile
// and its tables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/orp_hip.h"
#include "orp_launch.hpp"

namespace orp_c1x1 {

struct Tile { int bm, bn; };   // workgroup tile: channels x positions

// a row of a routing table: a closed range of positions per image at one (Cin, Cout, batch)
struct PaidRow { int cin, cout, hw_min, hw_max, batch; };
template <size_t N>
int paid(const PaidRow (&rows)[N], int c_in, int c_out, int hw, int batch) {
  for (const PaidRow& s : rows)
    if (s.cin == c_in && s.cout == c_out && s.batch == batch && hw >= s.hw_min && hw <= s.hw_max) return 1;
  return 0;
}

// The one place that lists a tile's instantiations: f(mode, range, vec), the three as std::integral_constant.  MODE: the residual
// term (0 nothing, 1 res, 2 res with its own affine); RANGE: the range word leaves with the outputs (conv1: no residual); VEC.
template <class Args, class F>
void dispatch(const Args& A, bool vec, F f) {
  auto with_vec = [&](auto mode, auto range) {
    if (vec) f(mode, range, std::true_type{});
    else f(mode, range, std::false_type{});
  };
  if (A.range) with_vec(std::integral_constant<int, 0>{}, std::true_type{});
  else if (!A.res) with_vec(std::integral_constant<int, 0>{}, std::false_type{});
  else if (!A.scale2) with_vec(std::integral_constant<int, 1>{}, std::false_type{});
  else with_vec(std::integral_constant<int, 2>{}, std::false_type{});
}

template <class Args>
dim3 grid_of(const Args& A, int batch) { return dim3((unsigned)((long)A.ntm * A.ntn * batch)); }

// An entry point of either file: the argument rules, the common fields of A, the range word's fill, then launch_tile(A, t, vec, st),
// which sets the file's weight fields and launches tile t's kernel.  shape_ok: the file's own channel rule; pick_tile: its tile rule.
// range_out (or NULL): one word of device memory that is left holding max range_bits(y) as float bits -- zeroed here by a kernel
// launch (orp_launch.hpp fill_async: a captured graph replays it), raised by one conditional atomicMax per workgroup.  No residual
// with it (conv1 is what feeds a range-reading convolution).
template <class Args, class Launch>
int run(const float* x, const void* weight, const float* scale, const float* shift, const float* residual, const float* scale2,
        const float* shift2, float* y, int batch, int c_in, int c_out, int hw, int relu, uint32_t* range_out, void* stream,
        bool shape_ok, Tile (*pick_tile)(int, int, int), Launch launch_tile) {
  if (range_out && residual) return ORP_EINVAL;
  if (!x || !weight || !scale || !shift || !y || batch <= 0 || hw <= 0 || !shape_ok) return ORP_EINVAL;
  if ((scale2 != nullptr) != (shift2 != nullptr) || (scale2 && !residual) || (const float*)y == x || (const float*)y == residual)
    return ORP_EINVAL;
  if ((uintptr_t)weight & 15) return ORP_EINVAL;
  const Tile t = pick_tile(c_out, hw, batch);
  Args A;
  A.x = x; A.scale = scale; A.shift = shift; A.res = residual; A.scale2 = scale2; A.shift2 = shift2; A.y = y;
  A.cin = c_in; A.cout = c_out; A.hw = hw; A.relu = relu ? 1 : 0;
  A.ntm = (c_out + t.bm - 1) / t.bm; A.ntn = (hw + t.bn - 1) / t.bn;
  A.range = range_out;
  if ((long)A.ntm * A.ntn * batch >= (1L << 31)) return ORP_ETOOBIG;
  const bool vec = (hw & 3) == 0 && ((uintptr_t)x & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  if (range_out) {
    hipError_t fe = orp::fill_async(range_out, 0, sizeof(uint32_t), st);
    if (fe != hipSuccess) return (int)fe;
  }
  launch_tile(A, t, vec, st);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ORP_OK : (int)e;
}

}  // namespace orp_c1x1
