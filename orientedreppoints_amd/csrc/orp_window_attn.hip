// orp_window_attn.hip -- Swin's (shifted-)window attention at inference as ONE fp32 kernel (orp_window_attention, include/orp_hip.h).
//
// What it replaces (mmdet/models/backbones/swin_transformer.py: SwinTransformerBlock.forward:199-250, WindowAttention.forward:122-155,
// the mask of BasicLayer.forward:370-390): pad to whole windows, cyclic roll, window partition, q k^T + relative-position bias +
// shift mask, softmax, P V, window reverse, un-roll, crop.  All of that except the two small contractions is index arithmetic, and
// qkv / proj are per-token linears, so the kernel reads the qkv of the UN-padded, UN-rolled tokens once and writes every real token's
// attention result to its own place once.  A padded token enters the reference's attention as a zero vector AFTER norm1, so its
// q / k / v are the qkv bias (or zero): it is a key like any other and has no output.
//
// One wave per (window, head); the heads of a window are neighbours in the grid, so the window's token rows are fetched together.
//   * K and V of the window (49 x head_dim floats each) and the head's 169 bias values are staged in LDS with 16-byte loads.
//   * lane i < 49 owns query row i: q in registers, the keys walked in ascending order twice (K rows read with broadcast
//     ds_read_b128 -- every lane the same address, no bank conflict): once for the row maximum, once more for exp(score - max), the
//     sum and the head_dim outputs.  The softmax needs no cross-lane step, and forming the 49 scores twice instead of keeping them
//     takes every head dim to three waves per SIMD or more without a spilled register.  The reduction order of every output is
//     fixed by this file alone: it does not depend on the grid, on other work on the device or on replay.
//   * expf is the device library's (full fp32 accuracy), not the fast intrinsic.
// No allocation, no host synchronisation: capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orp_hip.h"

namespace {

constexpr int WS = 7;                 // window side: the only one supported
constexpr int NTOK = WS * WS;         // 49 tokens per window
constexpr int NBIAS = (2 * WS - 1) * (2 * WS - 1);

// band of a ROLLED coordinate (BasicLayer.forward:376-384: slices (0, -ws), (-ws, -shift), (-shift, None) of the padded map)
__device__ __forceinline__ int band_of(int r, int padded, int shift) { return r < padded - WS ? 0 : (r < padded - shift ? 1 : 2); }

template <int HD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3)))   // 168 registers: what the LDS of head dim 32 admits anyway
void window_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ qkv_bias, const float* __restrict__ bias_table,
                        int height, int width, int heads, int nwy, int nwx, int shift, float scale, float* __restrict__ out) {
  constexpr int HD4 = HD / 4;
  constexpr int KU = HD >= 28 ? 1 : WS;     // keys of a window row unrolled together (the widest heads: one, to stay inside 168 registers)
  __shared__ float4 sk[NTOK * HD4];
  __shared__ float4 sv[NTOK * HD4];
  __shared__ float sb[NBIAS];

  const int lane = threadIdx.x;
  size_t bid = blockIdx.x;
  const int head = (int)(bid % (size_t)heads);
  bid /= (size_t)heads;
  const int wx = (int)(bid % (size_t)nwx);
  bid /= (size_t)nwx;
  const int wy = (int)(bid % (size_t)nwy);
  const size_t b = bid / (size_t)nwy;
  const int hp = nwy * WS, wp = nwx * WS;
  const size_t c = (size_t)heads * HD;                         // channels of one of q / k / v
  const size_t img = b * (size_t)height * (size_t)width;       // first token of this image

  // K, V: 49 x HD4 16-byte pieces each, consecutive lanes on consecutive pieces of a token's row
  for (int idx = lane; idx < NTOK * HD4; idx += 64) {
    const int t = idx / HD4, p = idx - t * HD4;
    int r = wy * WS + t / WS + shift, col = wx * WS + t % WS + shift;
    r -= r >= hp ? hp : 0;
    col -= col >= wp ? wp : 0;
    float4 k4 = make_float4(0.f, 0.f, 0.f, 0.f), v4 = k4;
    if (r < height && col < width) {
      const float* src = qkv + (img + (size_t)r * width + col) * (3 * c) + (size_t)head * HD + (size_t)p * 4;
      k4 = *reinterpret_cast<const float4*>(src + c);
      v4 = *reinterpret_cast<const float4*>(src + 2 * c);
    } else if (qkv_bias) {
      const float* src = qkv_bias + (size_t)head * HD + (size_t)p * 4;
      k4 = *reinterpret_cast<const float4*>(src + c);
      v4 = *reinterpret_cast<const float4*>(src + 2 * c);
    }
    sk[idx] = k4;
    sv[idx] = v4;
  }
  for (int idx = lane; idx < NBIAS; idx += 64) sb[idx] = bias_table[(size_t)idx * heads + head];
  __syncthreads();
  if (lane >= NTOK) return;

  // this lane's query
  const int qi = lane / WS, qj = lane - qi * WS;
  int r = wy * WS + qi + shift, col = wx * WS + qj + shift;
  r -= r >= hp ? hp : 0;
  col -= col >= wp ? wp : 0;
  const bool real = r < height && col < width;
  float q[HD];
  {
    const float* src = real ? qkv + (img + (size_t)r * width + col) * (3 * c) : qkv_bias;
    if (src) {
      src += (size_t)head * HD;
#pragma unroll
      for (int p = 0; p < HD4; ++p) {
        const float4 t4 = *reinterpret_cast<const float4*>(src + p * 4);
        q[4 * p] = t4.x, q[4 * p + 1] = t4.y, q[4 * p + 2] = t4.z, q[4 * p + 3] = t4.w;
      }
    } else {
#pragma unroll
      for (int d = 0; d < HD; ++d) q[d] = 0.f;
    }
  }
  const int qband = shift > 0 ? 3 * band_of(wy * WS + qi, hp, shift) + band_of(wx * WS + qj, wp, shift) : 0;
  const int qrel = (qi + WS - 1) * (2 * WS - 1) + (qj + WS - 1);

  // the score of key (ki, kj): key rows are wave-uniform addresses (broadcast reads), the band of a key is scalar arithmetic
  auto score = [&](int ki, int kj) -> float {
    const float4* krow = sk + (ki * WS + kj) * HD4;
    float dot = 0.f;
#pragma unroll
    for (int p = 0; p < HD4; ++p) {
      const float4 k4 = krow[p];
      dot = fmaf(q[4 * p], k4.x, dot);
      dot = fmaf(q[4 * p + 1], k4.y, dot);
      dot = fmaf(q[4 * p + 2], k4.z, dot);
      dot = fmaf(q[4 * p + 3], k4.w, dot);
    }
    float sc = fmaf(scale, dot, sb[qrel - (ki * (2 * WS - 1) + kj)]);
    if (shift > 0) {
      const int kband = 3 * band_of(wy * WS + ki, hp, shift) + band_of(wx * WS + kj, wp, shift);
      sc += kband != qband ? -100.f : 0.f;
    }
    return sc;
  };
  // pass 1: the row maximum.  Pass 2 forms the same scores again (the same instructions on the same operands) instead of keeping 49
  // of them per lane: the contraction is a small part of the kernel's time, and 49 live registers less is a wave more per SIMD.
  float m = -__builtin_inff();
#pragma unroll 1
  for (int ki = 0; ki < WS; ++ki) {
#pragma unroll KU
    for (int kj = 0; kj < WS; ++kj) m = fmaxf(m, score(ki, kj));
  }
  float sum = 0.f;
  float acc[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) acc[d] = 0.f;
#pragma unroll 1
  for (int ki = 0; ki < WS; ++ki) {
#pragma unroll KU
    for (int kj = 0; kj < WS; ++kj) {
      const float e = expf(score(ki, kj) - m);
      sum += e;
      const float4* vrow = sv + (ki * WS + kj) * HD4;
#pragma unroll
      for (int p = 0; p < HD4; ++p) {
        const float4 v4 = vrow[p];
        acc[4 * p] = fmaf(e, v4.x, acc[4 * p]);
        acc[4 * p + 1] = fmaf(e, v4.y, acc[4 * p + 1]);
        acc[4 * p + 2] = fmaf(e, v4.z, acc[4 * p + 2]);
        acc[4 * p + 3] = fmaf(e, v4.w, acc[4 * p + 3]);
      }
    }
  }
  if (!real) return;                                             // a padded token is a key only
  const float inv = 1.0f / sum;
  float* dst = out + (img + (size_t)r * width + col) * c + (size_t)head * HD;
#pragma unroll
  for (int p = 0; p < HD4; ++p)
    *reinterpret_cast<float4*>(dst + p * 4) = make_float4(acc[4 * p] * inv, acc[4 * p + 1] * inv, acc[4 * p + 2] * inv, acc[4 * p + 3] * inv);
}

template <int HD>
hipError_t launch(const float* qkv, const float* qkv_bias, const float* bias_table, size_t blocks, int height, int width, int heads,
                  int nwy, int nwx, int shift, float scale, float* out, hipStream_t st) {
  hipLaunchKernelGGL(window_attn_kernel<HD>, dim3((unsigned)blocks), dim3(64), 0, st, qkv, qkv_bias, bias_table, height, width, heads,
                     nwy, nwx, shift, scale, out);
  return hipGetLastError();
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int orp_window_attention(const float* qkv, const float* qkv_bias, const float* bias_table, int batch, int height, int width,
                                    int heads, int head_dim, int window, int shift, float scale, float* out, void* stream) {
  if (!qkv || !bias_table || !out || batch < 1 || height < 1 || width < 1 || heads < 1) return ORP_EINVAL;
  if (window != WS || shift < 0 || shift >= WS || head_dim < 4 || head_dim > 32 || head_dim % 4) return ORP_EINVAL;
  if (!aligned16(qkv) || !aligned16(qkv_bias) || !aligned16(out)) return ORP_EINVAL;   // 16-byte loads and stores
  const int nwy = (height + WS - 1) / WS, nwx = (width + WS - 1) / WS;
  const size_t blocks = (size_t)batch * (size_t)nwy * (size_t)nwx * (size_t)heads;
  if (blocks > 0x7fffffffu) return ORP_EINVAL;                   // one block per (window, head) along grid x
  hipStream_t st = (hipStream_t)stream;
  hipError_t e;
  switch (head_dim) {
#define ORP_WA_CASE(HD) case HD: e = launch<HD>(qkv, qkv_bias, bias_table, blocks, height, width, heads, nwy, nwx, shift, scale, out, st); break;
    ORP_WA_CASE(4) ORP_WA_CASE(8) ORP_WA_CASE(12) ORP_WA_CASE(16) ORP_WA_CASE(20) ORP_WA_CASE(24) ORP_WA_CASE(28) ORP_WA_CASE(32)
#undef ORP_WA_CASE
    default: return ORP_EINVAL;
  }
  return e == hipSuccess ? ORP_OK : (int)e;
}
