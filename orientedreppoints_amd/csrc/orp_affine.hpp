// orp_affine.hpp -- the per-channel affine (+ ReLU) expressions of the eval-mode BatchNorm passes (orp_norm.hip: affine_act_kernel,
// affine2_act_kernel, the GroupNorm passes) and of the epilogue of the fused 1x1 convolution (orp_conv1x1_bn.hip).  The scalar
// tails of the two pass kernels and the fused epilogue call the same affine_act / affine_res_act; the passes' float4 bodies spell the
// same operations per component (affine_act4, add, relu4).  Both files are built with contraction on: x * a + b is one fma.
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ void relu4(float4& t) { t.x = fmaxf(t.x, 0.f); t.y = fmaxf(t.y, 0.f); t.z = fmaxf(t.z, 0.f); t.w = fmaxf(t.w, 0.f); }
__device__ __forceinline__ float affine_act(float x, float a, float b, int relu) {
  float t = x * a + b;
  if (relu) t = fmaxf(t, 0.f);
  return t;
}
// one coefficient pair (a, b) per component
__device__ __forceinline__ void affine_act4(float4& t, float2 k0, float2 k1, float2 k2, float2 k3, int relu) {
  t.x = t.x * k0.x + k0.y; t.y = t.y * k1.x + k1.y; t.z = t.z * k2.x + k2.y; t.w = t.w * k3.x + k3.y;
  if (relu) relu4(t);
}
__device__ __forceinline__ void affine_act4(float4& t, float a, float b, int relu) {
  const float2 k = make_float2(a, b);
  affine_act4(t, k, k, k, k, relu);
}
// The tail of affine_act_kernel / affine2_act_kernel for one element: t = x * a + b, then the residual (rounded to fp32 on its own when
// it carries an affine), then the ReLU.
__device__ __forceinline__ float affine_res_act(float x, float a, float b, float r, int relu) {
  float t = affine_act(x, a, b, 0);
  t += r;
  if (relu) t = fmaxf(t, 0.f);
  return t;
}

}  // namespace
