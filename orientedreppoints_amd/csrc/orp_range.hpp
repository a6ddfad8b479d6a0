// The range rule of the fp16-pieces contractions (DeformConv forward / backward, tower and FPN convolutions, their weight
// gradients): every operand tensor is multiplied by ONE power of two 2^k chosen from its largest magnitude so that it lands in
// [2^14, 2^15), split into hi = fp16(v) and lo = fp16(v - hi), contracted in fp32, and the accumulator is scaled back by
// 2^-(kx + kw).  One definition for every kernel and producer that takes part; the header is plain C++ as well, so that the host
// test (tests/host_harness/range_host.cpp) compiles the same functions with g++.
//
//   range_bits(v)     what a range pre-pass / producer folds into its max: |v| as float bits, 0 for Inf and NaN.  A non-finite
//                     element spreads to the outputs that read it (fp16 Inf / NaN pieces) and to no other: were its bits taken
//                     (exponent field 255) the scale of the whole call would flush every finite operand to zero.
//   range_bound_bits  the same for a computed upper bound (GroupNorm): a hair above it, 0 when it is not finite.
//   range_exp(am)     k for a range word (max of range_bits): 14 - floor(log2 max), clamped so that 2^k is a normal float,
//                     [-126, 127]; 0 for an all-zero tensor (and for a non-finite word, which no producer leaves).  The upper
//                     clamp only binds below 2^-113 (tiny tensors keep what fp16 holds of them after 2^127); the lower one never
//                     binds for a finite maximum (2^-113 x FLT_MAX < 2^15).
//   range_scale(k)    2^k as a float (k in [-126, 127]: normal).
//   range_exp_of(s)   k of such a scale (a normal power of two), for a scale handed over through memory.
//   range_unscale     acc x 2^-(kx + kw) as one ldexp: one rounding, exact wherever the result is a normal float, and no
//                     intermediate 1 / (2^kx 2^kw) that overflows to Inf (-> 0) when kx + kw > 127.  For operands inside the
//                     old clamp its bits are those of the power-of-two multiply it replaces.
//   range_split, range_raise   (device only) see below
#pragma once
#include <stdint.h>
#include <string.h>
#include <math.h>

#if defined(__HIPCC__)
#define ORP_RANGE_FN __host__ __device__ __forceinline__
#else
#define ORP_RANGE_FN inline
#endif

namespace orp {

ORP_RANGE_FN unsigned range_float_bits(float v) {
  unsigned u;
  memcpy(&u, &v, sizeof u);
  return u;
}

ORP_RANGE_FN float range_bits_float(unsigned u) {
  float v;
  memcpy(&v, &u, sizeof v);
  return v;
}

ORP_RANGE_FN unsigned range_bits(float v) {
  const unsigned u = range_float_bits(v) & 0x7fffffffu;
  return u < 0x7f800000u ? u : 0u;
}

ORP_RANGE_FN unsigned range_bound_bits(float bound) {
  const unsigned u = range_float_bits(bound) & 0x7fffffffu;
  if (u >= 0x7f800000u) return 0u;
  const float up = bound * 1.0001f;                         // (a hair above the rounding of the bound itself)
  return range_bits(up) == 0u && u != 0u ? 0x7f7fffffu : range_float_bits(up) & 0x7fffffffu;
}

ORP_RANGE_FN int range_exp(unsigned am) {
  if (am == 0u || am >= 0x7f800000u) return 0;
  int e = (int)(am >> 23);                                  // (subnormal maximum: e = 0 -> the clamp)
  int k = 14 - (e - 127);
  return k < -126 ? -126 : k > 127 ? 127 : k;
}

ORP_RANGE_FN float range_scale(int k) { return range_bits_float((unsigned)(127 + k) << 23); }

ORP_RANGE_FN int range_exp_of(float scale) { return (int)((range_float_bits(scale) >> 23) & 0xffu) - 127; }

ORP_RANGE_FN float range_unscale(float acc, int k) { return ldexpf(acc, -k); }

#if defined(__HIPCC__)
// device only (the host test has no fp16 type and no atomics)
//   range_split       the two pieces of an ALREADY SCALED value into element e of two arrays or vectors of halves: hi = the nearest
//                     fp16, lo = the residual (exact in fp32), rounded
//   range_raise       fold `bits` (a max of range_bits) into a range word: the atomic only where it would change the value (thousands
//                     of workgroups, one address -- a contended atomicMax per workgroup serialises in the L2)
template <typename H, typename L>
__device__ __forceinline__ void range_split(float sv, H& hi, L& lo, int e) {
  const _Float16 h = (_Float16)sv;
  hi[e] = h;
  lo[e] = (_Float16)(sv - (float)h);
}
__device__ __forceinline__ void range_raise(unsigned* word, unsigned bits) {
  if (bits > __atomic_load_n(word, __ATOMIC_RELAXED)) atomicMax(word, bits);
}
#endif

}  // namespace orp
