// orp_window_attn.hip -- Swin's (shifted-)window attention, everything the library has of it (include/orp_hip.h): ONE forward kernel, ONE
// backward kernel and ONE reduction kernel behind orp_window_attention (fp32 inference), orp_window_attention_train /
// orp_window_attention_backward (fp32 training) and orp_window_attention_h / orp_window_attention_backward_h (fp16 / bf16 OPERANDS, the
// memory format of a block under autocast).  The kernels are templates over the head dim and the operand type.
//
// What it replaces (mmdet/models/backbones/swin_transformer.py: SwinTransformerBlock.forward:199-250, WindowAttention.forward:122-155,
// the mask of BasicLayer.forward:370-390): pad to whole windows, cyclic roll, window partition, q k^T + relative-position bias +
// shift mask, softmax, P V, window reverse, un-roll, crop.  All of that except the two small contractions is index arithmetic, and
// qkv / proj are per-token linears, so the kernels read the qkv of the UN-padded, UN-rolled tokens once and write every real token's
// result to its own place once.  A padded token enters the reference's attention as a zero vector AFTER norm1, so its q / k / v are
// the qkv bias (or zero): it is a key like any other and has no output -- hence no grad_out: a padded QUERY contributes nothing to
// any gradient, a padded KEY's dK / dV are gradients of the qkv bias.  The shift mask is a constant.
//
// One wave per (window, head); the heads of a window are neighbours in the grid, so the window's token rows are fetched together.
//
// Forward:
//   * K and V of the window (49 x head_dim floats each) and the head's 169 bias values are staged in LDS, four elements per load.
//   * lane i < 49 owns query row i: q in registers, the keys walked in ascending order twice (K rows read with broadcast
//     ds_read_b128 -- every lane the same address, no bank conflict): once for the row maximum, once more for exp(score - max), the
//     sum and the head_dim outputs.  The softmax needs no cross-lane step, and forming the 49 scores twice instead of keeping them
//     takes every head dim to three waves per SIMD or more without a spilled register.  The reduction order of every output is
//     fixed by this file alone: it does not depend on the grid, on other work on the device or on replay.
//   * expf is the device library's (full fp32 accuracy), not the fast intrinsic.
//   * with a non-NULL `lse` it also leaves lse = row maximum + logf(row sum) for every real token, which is all the backward needs
//     besides the operands.  It is the same kernel with or without: `out` is bit for bit the same.
//
// Backward, with P_ij = expf(s_ij - lse_i), D_i = grad_out_i . out_i, dS_ij = P_ij (grad_out_i . V_j - D_i):
//   phase A, lane i = query row i: q_i, grad_out_i in registers, K and V of the window in LDS (broadcast reads, keys ascending):
//     dQ_i = scale sum_j dS_ij K_j in registers; dS_ij added into a 169-entry LDS array at bin (dy, dx) -- at one key step the 49 lanes
//     hit 49 distinct bins and the adds of a bin happen in key order: race-free, one fixed order;
//   phase B, lane j = key row j: k_j, v_j in registers, Q and grad_out of the window in LDS (broadcast reads, real queries ascending):
//     P_ij / dS_ij formed again, dK_j = scale sum_i dS_ij Q_i, dV_j = sum_i P_ij grad_out_i.
// What changed against staging K, V, Q and grad_out side by side (25 KB at head dim 32: five blocks per CU): phase A reads only K and
// V from LDS and phase B only Q and grad_out, so the two phases SHARE two 49 x head_dim buffers -- between them every lane takes its
// own k / v row into registers and puts its q / grad_out row in its place.  14.3 KB at head dim 32, eleven blocks per CU.
// Every real token lies in exactly one window: every element of grad_qkv is written once, no pre-zeroing, no atomics.  The block's 169
// bias-bin sums and the dK / dV of its padded keys (summed over the padded keys in ascending order) go to the workspace; the
// reduction kernel sums them over windows and images in an order fixed by this file (sixteen interleaved slices of the windows, each
// ascending, then the slices ascending).  Nothing depends on the grid's scheduling, on other work on the device or on replay.
//
// The operand type (Operand<DT>: 0 = fp32, 1 = fp16, 2 = bf16, the dtype codes of orp_dcn_forward_multi_h) is what is in MEMORY.  The
// arithmetic is one and the same, expression by expression: every product, sum, expf and logf is fp32.
//   * qkv, out, grad_out and grad_qkv are of the operand type: four elements per load, widened as they are loaded, and rounded once,
//     to nearest even, as they are stored (fp32: 16-byte loads and stores of the values as they are);
//   * qkv_bias, bias_table, lse, the bias / table gradients and the workspace are fp32 whatever the operands (fp32 parameters under
//     autocast);
//   * a padded token's q / k / v are the qkv bias ROUNDED TO THE OPERAND TYPE -- what the 16-bit linear layer emits for a zero row --
//     which the kernel does itself from the fp32 bias.
// K / V (phase B: Q / grad_out) are staged in LDS as fp32 after widening, so the LDS bytes, the broadcast reads and the summation
// order of every output are the same for every operand type: given fp32 copies of the same 16-bit operands (and the rounded bias)
// the fp32 instantiation forms the same fp32 results, and the 16-bit ones store them rounded once.  lse, grad_qkv_bias and
// grad_bias_table are the fp32 instantiation's bit for bit.
// No atomics, no allocation, no host synchronisation: capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/orp_hip.h"

namespace {

constexpr int WS = 7;                 // window side: the only one supported
constexpr int NTOK = WS * WS;         // 49 tokens per window
constexpr int NBIAS = (2 * WS - 1) * (2 * WS - 1);
constexpr int RED_ELEMS = 32;         // reduction kernel: elements of a block's partial per workgroup ...
constexpr int RED_SLICES = 16;        // ... times interleaved slices of the windows

// band of a ROLLED coordinate (BasicLayer.forward:376-384: slices (0, -ws), (-ws, -shift), (-shift, None) of the padded map)
__device__ __forceinline__ int band_of(int r, int padded, int shift) { return r < padded - WS ? 0 : (r < padded - shift ? 1 : 2); }

// The same LDS row, read a second time: the compiler does not see that it is the same address, so it reads the row again where it is
// used instead of keeping the first read's head_dim registers alive across the score (at head dim 32 that is the difference between
// 168 registers and spilling).
__device__ __forceinline__ const float4* again(const float4* row) {
  asm volatile("" : "+v"(row));
  return row;
}

// At head dim 32 a lane holds 96 (phase A: q, grad_out, dQ) to 128 (phase B: k, v, dK, dV) registers of its own row; with a whole LDS row
// in flight on top of them the compiler spills 4 registers under the cap of 168.  Between the halves of a row the scheduler may
// move nothing, so only half a row is ever in flight: 168 registers, no spill.
template <int HD>
__device__ __forceinline__ void half_row(int p) {
  if (HD >= 32 && p == HD / 8) __builtin_amdgcn_sched_barrier(0);
}

// floats of one (window, head)'s partial in the workspace: 169 bias bins, then dK and dV of its padded keys
__host__ __device__ constexpr int partial_floats(int hd) { return NBIAS + 2 * hd; }

// ---- the operand type: what is in memory; fp32 in registers ----
template <int DT> struct Operand;
template <> struct Operand<0> {       // fp32: as it is
  using elem = float;
};
template <> struct Operand<1> {       // fp16
  using elem = uint16_t;
  static __device__ __forceinline__ float widen(uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits); }
  // The value to round is an fp32 RESULT (acc * inv, scale * dq): without the empty asm the compiler folds the multiplication into the
  // conversion (v_fma_mixlo_f16: the exact product rounded once to fp16), which is not the fp32 kernels' value rounded to fp16.
  static __device__ __forceinline__ uint32_t round(float f) {
    asm volatile("" : "+v"(f));
    return __builtin_bit_cast(uint16_t, (_Float16)f);                                                                // nearest even
  }
};
template <> struct Operand<2> {       // bf16
  using elem = uint16_t;
  static __device__ __forceinline__ float widen(uint32_t bits) { return __uint_as_float(bits << 16); }
  static __device__ __forceinline__ uint32_t round(float f) {                                                       // nearest even
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  }
};

// four consecutive elements: one 8-byte load, widened (fp32: one 16-byte load)
template <int DT>
__device__ __forceinline__ float4 load4(const typename Operand<DT>::elem* p) {
  if constexpr (DT == 0) {
    return *reinterpret_cast<const float4*>(p);
  } else {
    const uint2 raw = *reinterpret_cast<const uint2*>(p);
    return make_float4(Operand<DT>::widen(raw.x & 0xffffu), Operand<DT>::widen(raw.x >> 16), Operand<DT>::widen(raw.y & 0xffffu),
                       Operand<DT>::widen(raw.y >> 16));
  }
}

// ... and rounded once, one 8-byte store (fp32: one 16-byte store)
template <int DT>
__device__ __forceinline__ void store4(typename Operand<DT>::elem* p, float a, float b, float c, float d) {
  if constexpr (DT == 0) {
    *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
  } else {
    uint2 raw;
    raw.x = Operand<DT>::round(a) | (Operand<DT>::round(b) << 16);
    raw.y = Operand<DT>::round(c) | (Operand<DT>::round(d) << 16);
    *reinterpret_cast<uint2*>(p) = raw;
  }
}

// four values of the fp32 qkv bias as the linear layer of the operand type emits them for a zero row (fp32: unrounded)
template <int DT>
__device__ __forceinline__ float4 bias4(const float* p) {
  const float4 b = *reinterpret_cast<const float4*>(p);
  if constexpr (DT == 0) {
    return b;
  } else {
    return make_float4(Operand<DT>::widen(Operand<DT>::round(b.x)), Operand<DT>::widen(Operand<DT>::round(b.y)),
                       Operand<DT>::widen(Operand<DT>::round(b.z)), Operand<DT>::widen(Operand<DT>::round(b.w)));
  }
}

// registers per lane the kernels are held to: three waves per SIMD (168), what the LDS of head dim 32 admits anyway
constexpr int WAVES_PER_EU = 3;

template <int HD, int DT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES_PER_EU)))
void wattn_fwd_kernel(const typename Operand<DT>::elem* __restrict__ qkv, const float* __restrict__ qkv_bias,
                      const float* __restrict__ bias_table, int height, int width, int heads, int nwy, int nwx, int shift, float scale,
                      typename Operand<DT>::elem* __restrict__ out, float* __restrict__ lse) {
  using elem = typename Operand<DT>::elem;
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

  // K, V: 49 x HD4 pieces of four elements each, consecutive lanes on consecutive pieces of a token's row; fp32 in LDS
  for (int idx = lane; idx < NTOK * HD4; idx += 64) {
    const int t = idx / HD4, p = idx - t * HD4;
    int r = wy * WS + t / WS + shift, col = wx * WS + t % WS + shift;
    r -= r >= hp ? hp : 0;
    col -= col >= wp ? wp : 0;
    float4 k4 = make_float4(0.f, 0.f, 0.f, 0.f), v4 = k4;
    if (r < height && col < width) {
      const elem* src = qkv + (img + (size_t)r * width + col) * (3 * c) + (size_t)head * HD + (size_t)p * 4;
      k4 = load4<DT>(src + c);
      v4 = load4<DT>(src + 2 * c);
    } else if (qkv_bias) {
      const float* src = qkv_bias + (size_t)head * HD + (size_t)p * 4;
      k4 = bias4<DT>(src + c);
      v4 = bias4<DT>(src + 2 * c);
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
  if (real) {
    const elem* src = qkv + (img + (size_t)r * width + col) * (3 * c) + (size_t)head * HD;
#pragma unroll
    for (int p = 0; p < HD4; ++p) {
      const float4 t4 = load4<DT>(src + p * 4);
      q[4 * p] = t4.x, q[4 * p + 1] = t4.y, q[4 * p + 2] = t4.z, q[4 * p + 3] = t4.w;
    }
  } else if (qkv_bias) {
    const float* src = qkv_bias + (size_t)head * HD;
#pragma unroll
    for (int p = 0; p < HD4; ++p) {
      const float4 t4 = bias4<DT>(src + p * 4);
      q[4 * p] = t4.x, q[4 * p + 1] = t4.y, q[4 * p + 2] = t4.z, q[4 * p + 3] = t4.w;
    }
  } else {
#pragma unroll
    for (int d = 0; d < HD; ++d) q[d] = 0.f;
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
  const size_t tok = img + (size_t)r * width + col;
  elem* dst = out + tok * c + (size_t)head * HD;
#pragma unroll
  for (int p = 0; p < HD4; ++p) store4<DT>(dst + p * 4, acc[4 * p] * inv, acc[4 * p + 1] * inv, acc[4 * p + 2] * inv, acc[4 * p + 3] * inv);
  if (lse) lse[tok * heads + head] = m + logf(sum);              // (wave-uniform: inference keeps none)
}

template <int HD, int DT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES_PER_EU)))
void wattn_bwd_kernel(const typename Operand<DT>::elem* __restrict__ qkv, const float* __restrict__ qkv_bias,
                      const float* __restrict__ bias_table, const typename Operand<DT>::elem* __restrict__ out,
                      const float* __restrict__ lse, const typename Operand<DT>::elem* __restrict__ grad_out, int height, int width,
                      int heads, int nwy, int nwx, int shift, float scale, typename Operand<DT>::elem* __restrict__ grad_qkv,
                      int bias_grad, float* __restrict__ partial) {
  using elem = typename Operand<DT>::elem;
  constexpr int HD4 = HD / 4;
  __shared__ float4 sa[NTOK * HD4];         // phase A: K    phase B: Q          then: dK of the padded keys
  __shared__ float4 sc[NTOK * HD4];         // phase A: V    phase B: grad_out   then: dV of the padded keys
  __shared__ float sb[NBIAS];               // the head's bias values
  __shared__ float sdb[NBIAS];              // ... and this block's sums of dS per bin
  __shared__ float slse[NTOK];
  __shared__ float sdd[NTOK];               // D_i

  const int lane = threadIdx.x;
  size_t bid = blockIdx.x;
  float* part = partial + bid * (size_t)partial_floats(HD);
  const int head = (int)(bid % (size_t)heads);
  bid /= (size_t)heads;
  const int wx = (int)(bid % (size_t)nwx);
  bid /= (size_t)nwx;
  const int wy = (int)(bid % (size_t)nwy);
  const size_t b = bid / (size_t)nwy;
  const int hp = nwy * WS, wp = nwx * WS;
  const size_t c = (size_t)heads * HD;
  const size_t img = b * (size_t)height * (size_t)width;

  // whether position t of this window is a real token: scalar arithmetic for a wave-uniform t
  auto is_real = [&](int t) -> bool {
    int r = wy * WS + t / WS + shift, col = wx * WS + t % WS + shift;
    r -= r >= hp ? hp : 0;
    col -= col >= wp ? wp : 0;
    return r < height && col < width;
  };

  for (int idx = lane; idx < NTOK * HD4; idx += 64) {
    const int t = idx / HD4, p = idx - t * HD4;
    int r = wy * WS + t / WS + shift, col = wx * WS + t % WS + shift;
    r -= r >= hp ? hp : 0;
    col -= col >= wp ? wp : 0;
    float4 k4 = make_float4(0.f, 0.f, 0.f, 0.f), v4 = k4;
    if (r < height && col < width) {
      const elem* src = qkv + (img + (size_t)r * width + col) * (3 * c) + (size_t)head * HD + (size_t)p * 4;
      k4 = load4<DT>(src + c);
      v4 = load4<DT>(src + 2 * c);
    } else if (qkv_bias) {
      const float* src = qkv_bias + (size_t)head * HD + (size_t)p * 4;
      k4 = bias4<DT>(src + c);
      v4 = bias4<DT>(src + 2 * c);
    }
    sa[idx] = k4;
    sc[idx] = v4;
  }
  for (int idx = lane; idx < NBIAS; idx += 64) {
    sb[idx] = bias_table[(size_t)idx * heads + head];
    sdb[idx] = 0.f;
  }
  __syncthreads();

  // this lane's token: query row of phase A, key row of phase B (lanes 49 .. 63 own none and only help with the copies)
  const bool act = lane < NTOK;
  const int ti = lane / WS, tj = lane - ti * WS;
  int r = wy * WS + ti + shift, col = wx * WS + tj + shift;
  r -= r >= hp ? hp : 0;
  col -= col >= wp ? wp : 0;
  const bool real = act && r < height && col < width;
  const size_t tok = img + (size_t)r * width + col;             // (only used where real)
  const int band = shift > 0 ? 3 * band_of(wy * WS + ti, hp, shift) + band_of(wx * WS + tj, wp, shift) : 0;
  const int qrel = (ti + WS - 1) * (2 * WS - 1) + (tj + WS - 1);   // this token as a query ...
  const int krel = ti * (2 * WS - 1) + tj;                          // ... and as a key: bin = qrel(query) - krel(key)

  float q[HD], g[HD];
  if (act) {
    // ---- phase A: this lane's query row ----
    float dd = 0.f, l = 0.f;
    if (real) {
      const elem* src = qkv + tok * (3 * c) + (size_t)head * HD;
      const elem* gs = grad_out + tok * c + (size_t)head * HD;
      const elem* os = out + tok * c + (size_t)head * HD;
#pragma unroll
      for (int p = 0; p < HD4; ++p) {
        const float4 t4 = load4<DT>(src + p * 4);
        q[4 * p] = t4.x, q[4 * p + 1] = t4.y, q[4 * p + 2] = t4.z, q[4 * p + 3] = t4.w;
      }
#pragma unroll
      for (int p = 0; p < HD4; ++p) {
        const float4 g4 = load4<DT>(gs + p * 4);
        const float4 o4 = load4<DT>(os + p * 4);
        g[4 * p] = g4.x, g[4 * p + 1] = g4.y, g[4 * p + 2] = g4.z, g[4 * p + 3] = g4.w;
        dd = fmaf(g4.x, o4.x, dd);
        dd = fmaf(g4.y, o4.y, dd);
        dd = fmaf(g4.z, o4.z, dd);
        dd = fmaf(g4.w, o4.w, dd);
      }
      l = lse[tok * heads + head];
    } else {
      if (qkv_bias) {
        const float* src = qkv_bias + (size_t)head * HD;
#pragma unroll
        for (int p = 0; p < HD4; ++p) {
          const float4 t4 = bias4<DT>(src + p * 4);
          q[4 * p] = t4.x, q[4 * p + 1] = t4.y, q[4 * p + 2] = t4.z, q[4 * p + 3] = t4.w;
        }
      } else {
#pragma unroll
        for (int d = 0; d < HD; ++d) q[d] = 0.f;
      }
#pragma unroll
      for (int d = 0; d < HD; ++d) g[d] = 0.f;
    }
    slse[lane] = l;
    sdd[lane] = dd;
    float dq[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) dq[d] = 0.f;
    volatile float* vdb = sdb;                                   // (another lane adds to this bin at the next key: keep the program's order)
#pragma unroll 1
    for (int ki = 0; ki < WS; ++ki) {
#pragma unroll 1
      for (int kj = 0; kj < WS; ++kj) {
        const float4* krow = sa + (ki * WS + kj) * HD4;
        const float4* vrow = sc + (ki * WS + kj) * HD4;
        float dot = 0.f, dp = 0.f;
#pragma unroll
        for (int p = 0; p < HD4; ++p) {
          half_row<HD>(p);
          const float4 k4 = krow[p];
          dot = fmaf(q[4 * p], k4.x, dot);
          dot = fmaf(q[4 * p + 1], k4.y, dot);
          dot = fmaf(q[4 * p + 2], k4.z, dot);
          dot = fmaf(q[4 * p + 3], k4.w, dot);
        }
#pragma unroll
        for (int p = 0; p < HD4; ++p) {
          half_row<HD>(p);
          const float4 v4 = vrow[p];
          dp = fmaf(g[4 * p], v4.x, dp);
          dp = fmaf(g[4 * p + 1], v4.y, dp);
          dp = fmaf(g[4 * p + 2], v4.z, dp);
          dp = fmaf(g[4 * p + 3], v4.w, dp);
        }
        const int bin = qrel - (ki * (2 * WS - 1) + kj);
        float s = fmaf(scale, dot, sb[bin]);                     // the forward's score expression
        if (shift > 0) {
          const int kband = 3 * band_of(wy * WS + ki, hp, shift) + band_of(wx * WS + kj, wp, shift);
          s += kband != band ? -100.f : 0.f;
        }
        const float ds = real ? expf(s - l) * (dp - dd) : 0.f;   // a padded query has no output: it contributes nothing
        vdb[bin] = vdb[bin] + ds;                                // 49 lanes, 49 bins; a bin's adds in key order
        const float4* krow2 = again(krow);
#pragma unroll
        for (int p = 0; p < HD4; ++p) {
          half_row<HD>(p);
          const float4 k4 = krow2[p];
          dq[4 * p] = fmaf(ds, k4.x, dq[4 * p]);
          dq[4 * p + 1] = fmaf(ds, k4.y, dq[4 * p + 1]);
          dq[4 * p + 2] = fmaf(ds, k4.z, dq[4 * p + 2]);
          dq[4 * p + 3] = fmaf(ds, k4.w, dq[4 * p + 3]);
        }
      }
    }
    if (real) {
      elem* dst = grad_qkv + tok * (3 * c) + (size_t)head * HD;
#pragma unroll
      for (int p = 0; p < HD4; ++p)
        store4<DT>(dst + p * 4, scale * dq[4 * p], scale * dq[4 * p + 1], scale * dq[4 * p + 2], scale * dq[4 * p + 3]);
    }
  }

  // ---- between the phases: every lane takes its own k / v row out of LDS and puts its q / grad_out row in its place ----
  float k[HD], v[HD];
  if (act) {
#pragma unroll
    for (int p = 0; p < HD4; ++p) {
      const float4 k4 = sa[lane * HD4 + p], v4 = sc[lane * HD4 + p];
      k[4 * p] = k4.x, k[4 * p + 1] = k4.y, k[4 * p + 2] = k4.z, k[4 * p + 3] = k4.w;
      v[4 * p] = v4.x, v[4 * p + 1] = v4.y, v[4 * p + 2] = v4.z, v[4 * p + 3] = v4.w;
    }
  }
  __syncthreads();
  if (act) {
#pragma unroll
    for (int p = 0; p < HD4; ++p) {
      sa[lane * HD4 + p] = make_float4(q[4 * p], q[4 * p + 1], q[4 * p + 2], q[4 * p + 3]);
      sc[lane * HD4 + p] = make_float4(g[4 * p], g[4 * p + 1], g[4 * p + 2], g[4 * p + 3]);
    }
  }
  __syncthreads();

  // ---- phase B: this lane's key row, the real queries in ascending order ----
  float dk[HD], dv[HD];
  if (act) {
#pragma unroll
    for (int d = 0; d < HD; ++d) dk[d] = 0.f, dv[d] = 0.f;
#pragma unroll 1
    for (int i = 0; i < NTOK; ++i) {
      if (!is_real(i)) continue;                                 // wave-uniform
      const int qi = i / WS, qj = i - qi * WS;
      const float4* qrow = sa + i * HD4;
      const float4* grow = sc + i * HD4;
      float dot = 0.f, dp = 0.f;
#pragma unroll
      for (int p = 0; p < HD4; ++p) {
        half_row<HD>(p);
        const float4 q4 = qrow[p];
        dot = fmaf(q4.x, k[4 * p], dot);
        dot = fmaf(q4.y, k[4 * p + 1], dot);
        dot = fmaf(q4.z, k[4 * p + 2], dot);
        dot = fmaf(q4.w, k[4 * p + 3], dot);
      }
#pragma unroll
      for (int p = 0; p < HD4; ++p) {
        half_row<HD>(p);
        const float4 g4 = grow[p];
        dp = fmaf(g4.x, v[4 * p], dp);
        dp = fmaf(g4.y, v[4 * p + 1], dp);
        dp = fmaf(g4.z, v[4 * p + 2], dp);
        dp = fmaf(g4.w, v[4 * p + 3], dp);
      }
      float s = fmaf(scale, dot, sb[(qi + WS - 1) * (2 * WS - 1) + (qj + WS - 1) - krel]);
      if (shift > 0) {
        const int qband = 3 * band_of(wy * WS + qi, hp, shift) + band_of(wx * WS + qj, wp, shift);
        s += band != qband ? -100.f : 0.f;
      }
      const float pr = expf(s - slse[i]);
      const float ds = pr * (dp - sdd[i]);
      const float4* qrow2 = again(qrow);
      const float4* grow2 = again(grow);
#pragma unroll
      for (int p = 0; p < HD4; ++p) {
        half_row<HD>(p);
        const float4 q4 = qrow2[p];
        dk[4 * p] = fmaf(ds, q4.x, dk[4 * p]);
        dk[4 * p + 1] = fmaf(ds, q4.y, dk[4 * p + 1]);
        dk[4 * p + 2] = fmaf(ds, q4.z, dk[4 * p + 2]);
        dk[4 * p + 3] = fmaf(ds, q4.w, dk[4 * p + 3]);
      }
#pragma unroll
      for (int p = 0; p < HD4; ++p) {
        half_row<HD>(p);
        const float4 g4 = grow2[p];
        dv[4 * p] = fmaf(pr, g4.x, dv[4 * p]);
        dv[4 * p + 1] = fmaf(pr, g4.y, dv[4 * p + 1]);
        dv[4 * p + 2] = fmaf(pr, g4.z, dv[4 * p + 2]);
        dv[4 * p + 3] = fmaf(pr, g4.w, dv[4 * p + 3]);
      }
    }
#pragma unroll
    for (int d = 0; d < HD; ++d) dk[d] *= scale;
    if (real) {
      elem* dst = grad_qkv + tok * (3 * c) + (size_t)head * HD;
#pragma unroll
      for (int p = 0; p < HD4; ++p) {
        store4<DT>(dst + c + p * 4, dk[4 * p], dk[4 * p + 1], dk[4 * p + 2], dk[4 * p + 3]);
        store4<DT>(dst + 2 * c + p * 4, dv[4 * p], dv[4 * p + 1], dv[4 * p + 2], dv[4 * p + 3]);
      }
    }
  }

  // ---- the block's partials (fp32): the 169 bin sums, and dK / dV summed over its padded keys in ascending order ----
  for (int idx = lane; idx < NBIAS; idx += 64) part[idx] = sdb[idx];
  if (!bias_grad) return;                                        // wave-uniform
  __syncthreads();                                               // phase B's reads of Q / grad_out are done
  if (act && !real) {
#pragma unroll
    for (int p = 0; p < HD4; ++p) {
      sa[lane * HD4 + p] = make_float4(dk[4 * p], dk[4 * p + 1], dk[4 * p + 2], dk[4 * p + 3]);
      sc[lane * HD4 + p] = make_float4(dv[4 * p], dv[4 * p + 1], dv[4 * p + 2], dv[4 * p + 3]);
    }
  }
  __syncthreads();
  if (lane < 2 * HD) {
    const float* rows = lane < HD ? reinterpret_cast<const float*>(sa) + lane : reinterpret_cast<const float*>(sc) + (lane - HD);
    float sum = 0.f;
#pragma unroll 1
    for (int t = 0; t < NTOK; ++t)
      if (!is_real(t)) sum += rows[t * HD];
    part[NBIAS + lane] = sum;
  }
}

// grad_bias_table and the k / v thirds of grad_qkv_bias (fp32 whatever the operands): every element's partials summed over the windows
// of all images in RED_SLICES interleaved slices (slice s: windows s, s + RED_SLICES, ... ascending), then the slices in ascending order
__global__ __launch_bounds__(RED_ELEMS * RED_SLICES)
void wattn_reduce_kernel(const float* __restrict__ partial, size_t windows, int heads, int hd, int elems,
                         float* __restrict__ grad_bias_table, float* __restrict__ grad_qkv_bias) {
  __shared__ float red[RED_SLICES][RED_ELEMS];
  const int el = threadIdx.x % RED_ELEMS, slice = threadIdx.x / RED_ELEMS;
  const int e = blockIdx.x * RED_ELEMS + el, head = blockIdx.y;
  const int pf = partial_floats(hd);
  float sum = 0.f;
  if (e < elems) {
    const float* src = partial + (size_t)head * pf + e;
    const size_t step = (size_t)heads * pf;
#pragma unroll 4
    for (size_t w = slice; w < windows; w += RED_SLICES) sum += src[w * step];
  }
  red[slice][el] = sum;
  __syncthreads();
  if (slice != 0 || e >= elems) return;
  sum = red[0][el];
#pragma unroll
  for (int s = 1; s < RED_SLICES; ++s) sum += red[s][el];
  if (e < NBIAS) {
    grad_bias_table[(size_t)e * heads + head] = sum;
  } else {
    const size_t c = (size_t)heads * hd;
    const int d = e - NBIAS;                                     // [0, hd): dK   [hd, 2 hd): dV
    grad_qkv_bias[c + (size_t)(d / hd) * c + (size_t)head * hd + d % hd] = sum;
    if (d < hd) grad_qkv_bias[(size_t)head * hd + d] = 0.f;      // a padded query has no output: the q third is exactly zero
  }
}

// ---- host side ----
bool aligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }      // (NULL is aligned)

// four elements of the operand type per load and store
uintptr_t operand_bytes(int dt) { return dt == 0 ? 16 : 8; }

// The supported set; leaves the grid in nwy / nwx / blocks.  `reduces`: every call but orp_window_attention also keeps the heads inside
// the reduction's grid y, so that whatever the training forward takes, the backward takes too.
bool supported(int batch, int height, int width, int heads, int head_dim, int window, int shift, bool reduces, int* nwy, int* nwx,
               size_t* blocks) {
  if (batch < 1 || height < 1 || width < 1 || heads < 1) return false;
  if (window != WS || shift < 0 || shift >= WS || head_dim < 4 || head_dim > 32 || head_dim % 4) return false;
  *nwy = (height + WS - 1) / WS, *nwx = (width + WS - 1) / WS;
  *blocks = (size_t)batch * (size_t)*nwy * (size_t)*nwx * (size_t)heads;
  return *blocks <= 0x7fffffffu && (!reduces || heads <= 65535);  // one block per (window, head) along grid x
}

// The one head-dim / operand-type switch: f(head dim, operand type) as compile-time constants; false for a pair there is no kernel for.
template <class F>
bool dispatch(int head_dim, int dt, F&& f) {
  switch (dt * 64 + head_dim) {
#define ORP_WA_CASE(HD)                                                                                                          \
  case HD: f(std::integral_constant<int, HD>(), std::integral_constant<int, 0>()); return true;                                   \
  case 64 + HD: f(std::integral_constant<int, HD>(), std::integral_constant<int, 1>()); return true;                              \
  case 128 + HD: f(std::integral_constant<int, HD>(), std::integral_constant<int, 2>()); return true;
    ORP_WA_CASE(4) ORP_WA_CASE(8) ORP_WA_CASE(12) ORP_WA_CASE(16) ORP_WA_CASE(20) ORP_WA_CASE(24) ORP_WA_CASE(28) ORP_WA_CASE(32)
#undef ORP_WA_CASE
    default: return false;
  }
}

// the three forward calls: checks, one launch, error return
int forward(int dt, bool reduces, const void* qkv, const float* qkv_bias, const float* bias_table, int batch, int height, int width,
            int heads, int head_dim, int window, int shift, float scale, void* out, float* lse, void* stream) {
  int nwy, nwx;
  size_t blocks;
  if (!qkv || !bias_table || !out) return ORP_EINVAL;
  if (!supported(batch, height, width, heads, head_dim, window, shift, reduces, &nwy, &nwx, &blocks)) return ORP_EINVAL;
  if (!aligned(qkv, operand_bytes(dt)) || !aligned(out, operand_bytes(dt)) || !aligned(qkv_bias, 16)) return ORP_EINVAL;
  if (!aligned(bias_table, 4) || !aligned(lse, 4)) return ORP_EINVAL;
  const bool ok = dispatch(head_dim, dt, [&](auto hd, auto op) {
    using elem = typename Operand<decltype(op)::value>::elem;
    hipLaunchKernelGGL((wattn_fwd_kernel<decltype(hd)::value, decltype(op)::value>), dim3((unsigned)blocks), dim3(64), 0,
                       (hipStream_t)stream, reinterpret_cast<const elem*>(qkv), qkv_bias, bias_table, height, width, heads, nwy, nwx,
                       shift, scale, reinterpret_cast<elem*>(out), lse);
  });
  if (!ok) return ORP_EINVAL;
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ORP_OK : (int)e;
}

// the two backward calls: checks, the workspace, the blocks' launch, the reduction's launch, error return
int backward(int dt, const void* qkv, const float* qkv_bias, const float* bias_table, const void* out, const float* lse,
             const void* grad_out, int batch, int height, int width, int heads, int head_dim, int window, int shift, float scale,
             void* grad_qkv, float* grad_qkv_bias, float* grad_bias_table, void* workspace, size_t workspace_bytes, void* stream) {
  int nwy, nwx;
  size_t blocks;
  if (!qkv || !bias_table || !out || !lse || !grad_out || !grad_qkv || !grad_bias_table || !workspace) return ORP_EINVAL;
  if (grad_qkv_bias && !qkv_bias) return ORP_EINVAL;             // without a qkv bias there is nothing its gradient could belong to
  if (!supported(batch, height, width, heads, head_dim, window, shift, true, &nwy, &nwx, &blocks)) return ORP_EINVAL;
  const uintptr_t ob = operand_bytes(dt);
  if (!aligned(qkv, ob) || !aligned(out, ob) || !aligned(grad_out, ob) || !aligned(grad_qkv, ob) || !aligned(qkv_bias, 16)) return ORP_EINVAL;
  if (!aligned(bias_table, 4) || !aligned(lse, 4) || !aligned(grad_qkv_bias, 4) || !aligned(grad_bias_table, 4)) return ORP_EINVAL;
  // the partials are fp32 whatever the operands: one workspace figure
  if (!aligned(workspace, 4) || workspace_bytes < blocks * (size_t)partial_floats(head_dim) * sizeof(float)) return ORP_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  float* partial = reinterpret_cast<float*>(workspace);
  const int bias_grad = grad_qkv_bias ? 1 : 0;
  const bool ok = dispatch(head_dim, dt, [&](auto hd, auto op) {
    using elem = typename Operand<decltype(op)::value>::elem;
    hipLaunchKernelGGL((wattn_bwd_kernel<decltype(hd)::value, decltype(op)::value>), dim3((unsigned)blocks), dim3(64), 0, st,
                       reinterpret_cast<const elem*>(qkv), qkv_bias, bias_table, reinterpret_cast<const elem*>(out), lse,
                       reinterpret_cast<const elem*>(grad_out), height, width, heads, nwy, nwx, shift, scale,
                       reinterpret_cast<elem*>(grad_qkv), bias_grad, partial);
  });
  if (!ok) return ORP_EINVAL;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const int elems = bias_grad ? partial_floats(head_dim) : NBIAS;   // (without a bias gradient the blocks leave no dK / dV partials)
  hipLaunchKernelGGL(wattn_reduce_kernel, dim3((unsigned)((elems + RED_ELEMS - 1) / RED_ELEMS), (unsigned)heads), dim3(RED_ELEMS * RED_SLICES), 0,
                     st, partial, blocks / (size_t)heads, heads, head_dim, elems, grad_bias_table, grad_qkv_bias);
  e = hipGetLastError();
  return e == hipSuccess ? ORP_OK : (int)e;
}

}  // namespace

extern "C" int orp_window_attention(const float* qkv, const float* qkv_bias, const float* bias_table, int batch, int height, int width,
                                    int heads, int head_dim, int window, int shift, float scale, float* out, void* stream) {
  return forward(0, false, qkv, qkv_bias, bias_table, batch, height, width, heads, head_dim, window, shift, scale, out, nullptr, stream);
}

extern "C" int orp_window_attention_train(const float* qkv, const float* qkv_bias, const float* bias_table, int batch, int height,
                                          int width, int heads, int head_dim, int window, int shift, float scale, float* out, float* lse,
                                          void* stream) {
  if (!lse) return ORP_EINVAL;
  return forward(0, true, qkv, qkv_bias, bias_table, batch, height, width, heads, head_dim, window, shift, scale, out, lse, stream);
}

extern "C" int orp_window_attention_h(const void* qkv, const float* qkv_bias, const float* bias_table, int batch, int height, int width,
                                      int heads, int head_dim, int window, int shift, float scale, void* out, float* lse, int dtype,
                                      void* stream) {
  if (dtype != 1 && dtype != 2) return ORP_EINVAL;
  return forward(dtype, true, qkv, qkv_bias, bias_table, batch, height, width, heads, head_dim, window, shift, scale, out, lse, stream);
}

extern "C" size_t orp_window_attention_backward_workspace_bytes(int batch, int height, int width, int heads, int head_dim, int window) {
  int nwy, nwx;
  size_t blocks;
  if (!supported(batch, height, width, heads, head_dim, window, 0, true, &nwy, &nwx, &blocks)) return 0;
  return blocks * (size_t)partial_floats(head_dim) * sizeof(float);
}

extern "C" int orp_window_attention_backward(const float* qkv, const float* qkv_bias, const float* bias_table, const float* out,
                                             const float* lse, const float* grad_out, int batch, int height, int width, int heads,
                                             int head_dim, int window, int shift, float scale, float* grad_qkv, float* grad_qkv_bias,
                                             float* grad_bias_table, void* workspace, size_t workspace_bytes, void* stream) {
  return backward(0, qkv, qkv_bias, bias_table, out, lse, grad_out, batch, height, width, heads, head_dim, window, shift, scale, grad_qkv,
                  grad_qkv_bias, grad_bias_table, workspace, workspace_bytes, stream);
}

extern "C" int orp_window_attention_backward_h(const void* qkv, const float* qkv_bias, const float* bias_table, const void* out,
                                               const float* lse, const void* grad_out, int batch, int height, int width, int heads,
                                               int head_dim, int window, int shift, float scale, void* grad_qkv, float* grad_qkv_bias,
                                               float* grad_bias_table, void* workspace, size_t workspace_bytes, int dtype, void* stream) {
  if (dtype != 1 && dtype != 2) return ORP_EINVAL;
  return backward(dtype, qkv, qkv_bias, bias_table, out, lse, grad_out, batch, height, width, heads, head_dim, window, shift, scale, grad_qkv,
                  grad_qkv_bias, grad_bias_table, workspace, workspace_bytes, stream);
}
