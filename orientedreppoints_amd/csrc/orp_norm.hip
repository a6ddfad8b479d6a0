// orp_norm.hip -- fused normalisation + activation passes of the dense head / backbone for gfx950 (inference).
//
// The reference runs conv -> GroupNorm(32) -> ReLU six times per FPN level in the head towers
// (mmdet/models/anchor_heads/orientedreppoints_head.py:91-113, mmdet/ops/conv_module.py:130-140) and
// conv -> BatchNorm(eval) -> (+identity) -> ReLU in every ResNet bottleneck (mmdet/models/backbones/resnet.py:133-170)
// as separate framework kernels.  Profiled on MI355X (round 1, profiles/r01_bench_v2_step.txt) the stock GroupNorm
// costs 1.29 ms / image: 32 groups x B = 32 workgroups for a 16.8 MB tensor, then a second pass, then the ReLU pass.
// These are bandwidth ops: here they are one read-only statistics pass plus ONE read-modify-write pass, all FPN
// levels in one launch.
//
//   orp_groupnorm_act_multi : y = relu?((x - mean_g) * rstd_g * gamma[c] + beta[c]), NCHW, statistics per (image, group)
//       pass 1: one workgroup per 4096-float chunk of a group's contiguous span -> (mean, M2) partials (the chunk is
//               held in registers, so M2 is taken around the chunk mean: no E[x^2] - mean^2 cancellation);
//       pass 2: every workgroup merges its group's partials with the parallel-variance formula (<= a few dozen pairs),
//               then normalises + scales + activates its own chunk with float4 traffic.
//   orp_affine_act          : y = relu?(x * scale[c] + shift[c] (+ residual)) -- eval-mode BatchNorm folded to a
//               per-channel affine, fused with the bottleneck's residual add and ReLU; in place allowed.
//   orp_affine2_act         : the same pass with a second affine on the residual (the downsample branch's BatchNorm);
//   orp_affine_act_backward / orp_affine2_act_backward : training, the backward of the two passes above with the BatchNorm's
//               dweight / dbias: one pass that leaves per-workgroup partial sums, one small kernel that adds them in float64;
//   orp_affine_relu_maxpool : the stem's BatchNorm + ReLU applied inside its 3x3 / stride-2 max-pool, one read of the input;
//   orp_fpn_topdown_nhwc    : the FPN laterals' GroupNorm + top-down sum + transposition as one pass behind the statistics.
//   orp_bias_act_multi      : y = relu?(x + bias[c] (+ residual)), y2 = y - sub[c], all FPN levels in one launch -- the
//               bias / ReLU / `+ pts_out_init` / `- dcn_base_offset` passes around the head's output convolutions.
//
// The GroupNorm routes (NCHW, transposed, top-down, channels-last, training) are held to each other bit for bit by the tests, and
// they are by construction: each step exists once.  chunk_load_sum / chunk_m2 are the chunk statistics, merge_span is the merge
// of a span's partials, gn_coef the per-channel coefficients, affine_act / affine_act4 / relu4 the step itself; level_of,
// block_sum and block_max are the searches and reductions around them.  Host side: fill / fill_cl + fill_status, set_affine,
// launch_status, plane_blocks; gn_nchw_forward is the one body of the inference and the training forward entry.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/orp_hip.h"
#include "orp_affine.hpp"
#include "orp_launch.hpp"
#include "orp_range.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 4096;            // floats per workgroup (16 per thread)
constexpr int kMaxLevels = 8;              // orp_bias_act_multi
constexpr int kGnMaxLevels = 16;           // GroupNorm: both towers' five levels in one launch pair

struct GnLevel {
  const float* x; float* y;
  const float* gamma; const float* beta;     // this tensor's affine parameters
  int hw;                 // H*W
  int cpg;                // chunks per (image, group)
  int chunk0;             // first chunk of this level
};
struct GnParams {
  GnLevel lv[kGnMaxLevels];
  int nlev, B, C, G;
  float eps; int relu;
  float2* partial;        // [total_chunks] (mean, M2)
  float2* stats;          // training: [nlev][B * G] (mean, rstd) per (image, group): level i, image b, group g at (i * B + b) * G + g; or NULL
  // backward (orp_groupnorm_act_multi_backward)
  const float* dy[kGnMaxLevels];
  float* dx[kGnMaxLevels];
  float4* bpart;          // [total_chunks][C / G] (sum dy', sum dy' xhat) per channel of the chunk's group, chunk-local
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                       // red may still be read from a previous call
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
// block-wide maximum of a word (range bits, or the bits of non-negative floats: the same order), in every thread
__device__ __forceinline__ unsigned block_max(unsigned v, unsigned* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
  __syncthreads();                       // red may still be read from a previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return max(max(red[0], red[1]), max(red[2], red[3]));
}

// the level an id (chunk, or blockIdx.x) belongs to: the last i with id >= first(i); first(0) is 0
template <class First>
__device__ __forceinline__ int level_of(First first, int nlev, int id) {
  int lvl = 0;
#pragma unroll 1
  for (int i = 1; i < nlev; i++) if (id >= first(i)) lvl = i;
  return lvl;
}

// (mean, var) of a span from its chunk partials (mean_k, M2_k) (Chan et al.): mean = sum n_k mean_k / N,
// M2 = sum M2_k + n_k (mean_k - mean)^2.  A chunk holds `chunk` units of `unit` elements, the last one what is left of `count`
// units: unit = 1 for the NCHW spans, C / G with chunks counted in positions for the channels-last ones.  THE merge of this file:
// every route that normalises goes through these statements and this reduction order, which is why their statistics are the same bits.
__device__ __forceinline__ float2 merge_span(const float2* part, int nchunks, int chunk, int count, int unit, float* red) {
  const float total = (float)count * (float)unit;
  float sm = 0.f;
  for (int k = threadIdx.x; k < nchunks; k += kThreads) {
    const int nk = min(chunk, count - k * chunk) * unit;
    sm += (float)nk * part[k].x;
  }
  const float mean = block_sum(sm, red) / total;
  float m2 = 0.f;
  for (int k = threadIdx.x; k < nchunks; k += kThreads) {
    const int nk = min(chunk, count - k * chunk) * unit;
    const float2 p = part[k];
    const float d = p.x - mean;
    m2 += p.y + (float)nk * d * d;
  }
  return make_float2(mean, block_sum(m2, red) / total);
}

// y = relu?(x * a + b) with the GroupNorm's per-channel coefficients (a, b) = (rstd gamma_c, beta_c - mean a).  The expressions
// are left to the compiler's contraction (this file is built with it on): x * a + b is one fma, as is beta_c - mean * a.
__device__ __forceinline__ float2 gn_coef(float mean, float rstd, float gamma_c, float beta_c) {
  const float a = rstd * gamma_c;
  return make_float2(a, beta_c - mean * a);
}
// (relu4, affine_act, affine_act4: orp_affine.hpp, shared with the fused 1x1 convolution's epilogue)

// A chunk of n <= 4096 floats held in registers, 16 per thread: as float4s (vec: n % 4 == 0 and src 16-byte aligned) thread t holds
// elements 4 (t + 256 q) .. + 3, else elements t + 256 q; 0 past the end.  Returns the thread's sum.
__device__ __forceinline__ float chunk_load_sum(const float* src, int n, bool vec, float (&v)[16]) {
  if (vec) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int e = (threadIdx.x + q * kThreads) * 4;
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e < n) t = *reinterpret_cast<const float4*>(src + e);
      v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 16; q++) { const int e = threadIdx.x + q * kThreads; v[q] = (e < n) ? src[e] : 0.f; }
  }
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < 16; q++) s += v[q];
  return s;
}
// the thread's share of the chunk's M2 around `mean`, over the elements that exist
__device__ __forceinline__ float chunk_m2(const float (&v)[16], int n, bool vec, float mean) {
  float m2 = 0.f;
  if (vec) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int e = (threadIdx.x + q * kThreads) * 4;
      if (e < n) {
#pragma unroll
        for (int u = 0; u < 4; u++) { const float d = v[4 * q + u] - mean; m2 += d * d; }
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < 16; q++) { const int e = threadIdx.x + q * kThreads; if (e < n) { const float d = v[q] - mean; m2 += d * d; } }
  }
  return m2;
}

// chunk id -> level, (image, group), chunk-in-span; returns the span geometry
struct ChunkGeom { int lvl, bg, k, span, n0, n; };
__device__ __forceinline__ ChunkGeom locate(const GnParams& P, int chunk) {
  ChunkGeom g;
  g.lvl = level_of([&](int i) { return P.lv[i].chunk0; }, P.nlev, chunk);
  const GnLevel& L = P.lv[g.lvl];
  const int id = chunk - L.chunk0;
  g.bg = id / L.cpg; g.k = id - g.bg * L.cpg;
  g.span = (P.C / P.G) * L.hw;
  g.n0 = g.k * kChunk;
  g.n = min(kChunk, g.span - g.n0);
  return g;
}

__global__ void __launch_bounds__(kThreads)
gn_stats_kernel(const GnParams P) {
  __shared__ float red[4];
  const ChunkGeom g = locate(P, blockIdx.x);
  const float* src = P.lv[g.lvl].x + (size_t)g.bg * g.span + g.n0;
  float v[16];
  const bool vec = ((g.span & 3) == 0);
  const float s = chunk_load_sum(src, g.n, vec, v);
  const float mean = block_sum(s, red) / (float)g.n;
  const float m2 = block_sum(chunk_m2(v, g.n, vec, mean), red);
  if (threadIdx.x == 0) P.partial[blockIdx.x] = make_float2(mean, m2);
}

__global__ void __launch_bounds__(kThreads)
gn_apply_kernel(const GnParams P) {
  __shared__ float red[4];
  const ChunkGeom g = locate(P, blockIdx.x);
  const GnLevel& L = P.lv[g.lvl];
  const float2 mv = merge_span(P.partial + L.chunk0 + (size_t)g.bg * L.cpg, L.cpg, kChunk, g.span, 1, red);
  const float mean = mv.x, rstd = rsqrtf(mv.y + P.eps);
  if (P.stats && g.k == 0 && threadIdx.x == 0) P.stats[(size_t)g.lvl * P.B * P.G + g.bg] = make_float2(mean, rstd);

  const int cg = P.C / P.G;
  const int grp = g.bg % P.G;
  const float* src = L.x + (size_t)g.bg * g.span + g.n0;
  float* dst = L.y + (size_t)g.bg * g.span + g.n0;
  const bool vec = ((L.hw & 3) == 0);
  if (vec) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int e = (threadIdx.x + q * kThreads) * 4;
      if (e < g.n) {
        const int c = grp * cg + (g.n0 + e) / L.hw;       // 4 consecutive elements share a channel (hw % 4 == 0)
        const float2 k = gn_coef(mean, rstd, L.gamma[c], L.beta[c]);
        float4 t = *reinterpret_cast<const float4*>(src + e);
        affine_act4(t, k.x, k.y, P.relu);
        *reinterpret_cast<float4*>(dst + e) = t;
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const int e = threadIdx.x + q * kThreads;
      if (e < g.n) {
        const int c = grp * cg + (g.n0 + e) / L.hw;
        const float2 k = gn_coef(mean, rstd, L.gamma[c], L.beta[c]);
        dst[e] = affine_act(src[e], k.x, k.y, P.relu);
      }
    }
  }
}

// Pass 2 of orp_groupnorm_act_multi_nhwc: the same normalise + scale + activate as gn_apply_kernel, written TRANSPOSED --
// y_nhwc[b, p, c] -- through a 32 x 33 LDS tile (32 channels = 4 groups x 32 positions per workgroup: 128-byte rows on both
// sides), and optionally also in place / NCHW (the regression tower's last layer feeds a plain convolution AND the
// DeformConv).  The head's DeformConv reads its input channels-last; this replaces the separate nchw_to_nhwc launch (one
// more read + write of every tower output per image).  merge_span, gn_coef and affine_act as in gn_apply_kernel: identical values.
struct GnNhwc {
  float* out[kGnMaxLevels];       // [B, hw, C] per level
  float* nchw[kGnMaxLevels];      // nullptr, or the NCHW output (may alias x)
  int bx0[kGnMaxLevels + 1];      // first blockIdx.x of each level (32-position tiles)
};
__global__ void __launch_bounds__(kThreads)
gn_apply_nhwc_kernel(const GnParams P, const GnNhwc T) {
  __shared__ float tile[32][33];
  __shared__ float2 sStat[32];                    // (mean, rstd) of the tile's groups (32 channels / (C / G) <= 32 groups)
  const int lvl = level_of([&](int i) { return T.bx0[i]; }, P.nlev, (int)blockIdx.x);
  const GnLevel& L = P.lv[lvl];
  const int hw = L.hw, cg = P.C / P.G;
  const int b = blockIdx.z, c0 = blockIdx.y * 32, p0 = ((int)blockIdx.x - T.bx0[lvl]) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int ngrp = (32 + cg - 1) / cg;            // groups touched by this channel tile (c0 is a multiple of cg: cg | 32)
  const int span = cg * hw;
  __shared__ float red[4];
  for (int gi = 0; gi < ngrp; gi++) {
    const int grp = c0 / cg + gi;
    if (grp >= P.G) break;                          // (block-uniform)
    const float2 mv = merge_span(P.partial + L.chunk0 + (size_t)(b * P.G + grp) * L.cpg, L.cpg, kChunk, span, 1, red);
    if (threadIdx.x == 0) sStat[gi] = make_float2(mv.x, rsqrtf(mv.y + P.eps));
  }
  __syncthreads();
  const float* src = L.x + (size_t)b * P.C * hw;
  float* nchw = T.nchw[lvl] ? T.nchw[lvl] + (size_t)b * P.C * hw : nullptr;
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r, p = p0 + tx;
    float t = 0.f;
    if (c < P.C && p < hw) {
      const float2 st = sStat[r / cg];
      const float2 k = gn_coef(st.x, st.y, L.gamma[c], L.beta[c]);
      t = affine_act(src[(size_t)c * hw + p], k.x, k.y, P.relu);
      if (nchw) nchw[(size_t)c * hw + p] = t;
    }
    tile[r][tx] = t;
  }
  __syncthreads();
  float* dst = T.out[lvl] + (size_t)b * hw * P.C;
  for (int r = ty; r < 32; r += 8) {
    const int p = p0 + r, c = c0 + tx;
    if (p < hw && c < P.C) dst[(size_t)p * P.C + c] = tile[tx][r];
  }
}

// The FPN's top-down path as one pass behind its statistics (orp_fpn_topdown_nhwc): level l's output is
//   g_l + up(g_{l+1} + up(g_{l+2} + ...)),  g_j = GroupNorm(lateral j), up = nearest-neighbour upsampling by exactly 2,
// written channels-last through the 32 x 33 tile of gn_apply_nhwc_kernel, max |.| of everything written folded into *amax as
// to_channels_last_kernel does.  The coarser levels' normalised values are recomputed at every fine position (1/4 and 1/16 of
// the reads) with gn_coef / affine_act, and summed innermost level first, each partial sum an fp32: the values the
// separate normalise / upsample / add launches leave.
//
// Statistics: gn_stats_kernel, then gn_merge_kernel -- one workgroup per (level, image, group) span merges the span's partials
// (merge_span) into (mean, rstd).  One merge per span instead of one per workgroup
// of the pass that applies them: the merge is a chain of dependent loads and reductions, and a few thousand workgroups each
// waiting for it was most of that pass when it was done there (traced at 1024^2: 48 us, against 21 + 5 for the merge kernel).
constexpr int kTdMaxLevels = 4;
constexpr int kTdTiles = 8;
struct TdLevels {
  float* out[kTdMaxLevels];       // [B, hw, C] per level
  int width[kTdMaxLevels];
  int bx0[kTdMaxLevels + 1];      // first blockIdx.x of each level (kTdTiles tiles of 32 positions per workgroup)
  float2* stats;                  // [nlev][B * G] (mean, rstd)
  unsigned* amax;                 // nullptr, or one word of float bits, zeroed by gn_merge_kernel
};

__global__ void __launch_bounds__(kThreads)
gn_merge_kernel(const GnParams P, const TdLevels T) {
  __shared__ float red[4];
  const int bg = blockIdx.x, lvl = blockIdx.y;        // (image, group), level
  const GnLevel& L = P.lv[lvl];
  const int span = (P.C / P.G) * L.hw;
  if (bg == 0 && lvl == 0 && threadIdx.x == 0 && T.amax) *T.amax = 0u;
  const float2 mv = merge_span(P.partial + L.chunk0 + (size_t)bg * L.cpg, L.cpg, kChunk, span, 1, red);
  if (threadIdx.x == 0) T.stats[(size_t)lvl * P.B * P.G + bg] = make_float2(mv.x, rsqrtf(mv.y + P.eps));
}

// the tiles of one workgroup, NL = number of levels summed (this one and the coarser ones) as a compile-time constant: every
// load of a tile is unconditional and issued before the first use; returns the thread's max |.| as range bits
template <int NL>
__device__ __forceinline__ unsigned td_tiles(const GnParams& P, const TdLevels& T, int lvl, int b, int c0, int bx, float (*tile)[33],
                                             const float2 (*sStat)[32]) {
  const int cg = P.C / P.G;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int hw = P.lv[lvl].hw;
  // per (level, channel) coefficients; this thread's channels are c0 + ty + 8 i
  float ca[NL][4], cb[NL][4];
  const float* src[NL];
#pragma unroll
  for (int sh = 0; sh < NL; sh++) {
    const GnLevel& L = P.lv[lvl + sh];
    src[sh] = L.x + ((size_t)b * P.C + c0 + ty) * L.hw;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int r = ty + 8 * i, c = c0 + r;
      const float2 st = sStat[sh][r / cg];
      const float2 k = gn_coef(st.x, st.y, L.gamma[c], L.beta[c]);
      ca[sh][i] = k.x; cb[sh][i] = k.y;
    }
  }
  float* dst = T.out[lvl] + (size_t)b * hw * P.C;
  unsigned m = 0u;
#pragma unroll 1
  for (int it = 0; it < kTdTiles; it++) {
    const int p0 = (bx * kTdTiles + it) * 32;
    if (p0 >= hw) break;                            // (block-uniform)
    const int p = min(p0 + tx, hw - 1);
    const int h = p / T.width[lvl], w = p - h * T.width[lvl];
    float x[NL][4];
#pragma unroll
    for (int sh = 0; sh < NL; sh++) {
      const size_t hwj = (size_t)P.lv[lvl + sh].hw;
      const float* q = src[sh] + (size_t)(h >> sh) * T.width[lvl + sh] + (w >> sh);
#pragma unroll
      for (int i = 0; i < 4; i++) x[sh][i] = q[(size_t)(8 * i) * hwj];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
      float t = affine_act(x[NL - 1][i], ca[NL - 1][i], cb[NL - 1][i], 0);           // innermost (coarsest) level first
#pragma unroll
      for (int sh = NL - 2; sh >= 0; sh--) {
        float g = affine_act(x[sh][i], ca[sh][i], cb[sh][i], 0);
        g += t;
        t = g;
      }
      if (p0 + tx >= hw) t = 0.f;
      tile[ty + 8 * i][tx] = t;
      m = max(m, orp::range_bits(t));
    }
    __syncthreads();
#pragma unroll
    for (int r = ty; r < 32; r += 8) {
      const int pp = p0 + r, c = c0 + tx;
      if (pp < hw) dst[(size_t)pp * P.C + c] = tile[tx][r];
    }
    __syncthreads();
  }
  return m;
}

__global__ void __launch_bounds__(kThreads)
fpn_topdown_nhwc_kernel(const GnParams P, const TdLevels T) {
  __shared__ float tile[32][33];
  __shared__ float2 sStat[kTdMaxLevels][32];      // (mean, rstd) of the tile's groups, this level and every coarser one
  const int lvl = level_of([&](int i) { return T.bx0[i]; }, P.nlev, (int)blockIdx.x);
  const int cg = P.C / P.G;
  const int b = blockIdx.z, c0 = blockIdx.y * 32, bx = (int)blockIdx.x - T.bx0[lvl];
  const int ngrp = 32 / cg;                         // groups of this channel tile (cg | 32, 32 | C)
  const int nl = P.nlev - lvl;
  if ((int)threadIdx.x < nl * ngrp) {
    const int sh = threadIdx.x / ngrp, gi = threadIdx.x - sh * ngrp;
    sStat[sh][gi] = T.stats[(size_t)(lvl + sh) * P.B * P.G + b * P.G + c0 / cg + gi];
  }
  __syncthreads();
  unsigned m;
  switch (nl) {                                     // (block-uniform)
    case 1: m = td_tiles<1>(P, T, lvl, b, c0, bx, tile, sStat); break;
    case 2: m = td_tiles<2>(P, T, lvl, b, c0, bx, tile, sStat); break;
    case 3: m = td_tiles<3>(P, T, lvl, b, c0, bx, tile, sStat); break;
    default: m = td_tiles<4>(P, T, lvl, b, c0, bx, tile, sStat); break;
  }
  if (T.amax) {
    __shared__ unsigned redm[4];
    const unsigned mx = block_max(m, redm);
    // one address, thousands of workgroups: the atomic only where it would raise the value (see to_channels_last_kernel)
    if (threadIdx.x == 0) orp::range_raise(T.amax, mx);
  }
}

// y = act(x * scale[c] + shift[c] (+ residual)), NCHW.  grid.y = (image, channel) plane, so the per-channel constants are
// block-uniform scalars and no integer division sits in the element loop; float4 traffic when HW % 4 == 0.
// RANGE: the word `range` is raised to max range_bits(y) (one conditional atomic per workgroup); a template parameter so that the
// plain instantiation keeps its instruction stream.
template <bool RANGE>
__global__ void __launch_bounds__(kThreads)
affine_act_kernel(const float* __restrict__ x, const float* __restrict__ res, const float* __restrict__ scale,
                  const float* __restrict__ shift, float* __restrict__ y, int C, int hw, int relu, unsigned* __restrict__ range) {
  unsigned rmax = 0u;
  const int plane = blockIdx.y;                       // b * C + c
  const int c = plane % C;
  const float a = scale[c], b = shift[c];
  const size_t base = (size_t)plane * hw;
  if ((hw & 3) == 0) {
    const int hw4 = hw >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x + base);
    const float4* r4 = res ? reinterpret_cast<const float4*>(res + base) : nullptr;
    float4* y4 = reinterpret_cast<float4*>(y + base);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw4; i += gridDim.x * blockDim.x) {
      float4 t = x4[i];
      affine_act4(t, a, b, 0);
      if (r4) { const float4 r = r4[i]; t.x += r.x; t.y += r.y; t.z += r.z; t.w += r.w; }
      if (relu) relu4(t);
      y4[i] = t;
      if (RANGE) rmax = max(max(rmax, orp::range_bits(t.x)), max(orp::range_bits(t.y), max(orp::range_bits(t.z), orp::range_bits(t.w))));
    }
  } else {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
      const float t = res ? affine_res_act(x[base + i], a, b, res[base + i], relu) : affine_act(x[base + i], a, b, relu);
      y[base + i] = t;
      if (RANGE) rmax = max(rmax, orp::range_bits(t));
    }
  }
  if (RANGE) {
    __shared__ unsigned redm[4];
    const unsigned mx = block_max(rmax, redm);
    if (threadIdx.x == 0) orp::range_raise(range, mx);
  }
}

// y = act((x * scale[c] + shift[c]) + (res * scale2[c] + shift2[c])): the last pass of a stage's FIRST bottleneck, whose identity
// branch is conv -> BatchNorm.  The second affine is the downsample BatchNorm, applied while the raw convolution output is read
// instead of in a read-modify-write pass of its own; it is rounded to fp32 before the add, which is the value that pass stored.
__global__ void __launch_bounds__(kThreads)
affine2_act_kernel(const float* __restrict__ x, const float* __restrict__ res, const float* __restrict__ scale,
                   const float* __restrict__ shift, const float* __restrict__ scale2, const float* __restrict__ shift2,
                   float* __restrict__ y, int C, int hw, int relu) {
  const int plane = blockIdx.y;                       // b * C + c
  const int c = plane % C;
  const float a = scale[c], b = shift[c];
  const float a2 = scale2[c], b2 = shift2[c];
  const size_t base = (size_t)plane * hw;
  if ((hw & 3) == 0) {
    const int hw4 = hw >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x + base);
    const float4* r4 = reinterpret_cast<const float4*>(res + base);
    float4* y4 = reinterpret_cast<float4*>(y + base);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw4; i += gridDim.x * blockDim.x) {
      float4 t = x4[i];
      float4 r = r4[i];
      affine_act4(t, a, b, 0);
      affine_act4(r, a2, b2, 0);
      t.x += r.x; t.y += r.y; t.z += r.z; t.w += r.w;
      if (relu) relu4(t);
      y4[i] = t;
    }
  } else {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
      y[base + i] = affine_res_act(x[base + i], a, b, affine_act(res[base + i], a2, b2, 0), relu);
    }
  }
}

// Training: the backward of affine_act_kernel / affine2_act_kernel, one read of grad_y, y and x (orp_affine_act_backward,
// orp_affine2_act_backward).  g = grad_y where y > 0 (y: the forward's output is the ReLU mask; NULL = no ReLU), grad_x = g a[c],
// grad_x2 = g a2[c], grad_res = g (may alias grad_y: a thread reads its elements before it writes them).  The launch has the forward's
// shape -- grid.y = (image, channel) plane, grid.x = plane_blocks(hw) -- so the channel's constants are block-uniform.
// STATS: a BatchNorm's parameters want their gradient.  Each workgroup leaves (sum g, sum g xhat, sum g xhat2) of its elements,
// xhat = (x - mean[c]) rstd[c], in part[plane * gridDim.x + blockIdx.x]: the thread's elements in loop order, the wave by butterfly,
// the four waves in order (block_sum).  x / x2 are NULL where that BatchNorm wants nothing, and are then not read.
struct AffineBwd {
  const float* gy; const float* y; const float* x; const float* x2;
  const float* scale; const float* mean; const float* rstd;
  const float* scale2; const float* mean2; const float* rstd2;
  float* gx; float* gx2; float* gres;
  float4* part;
  int C, hw, vec;
};

template <bool STATS>
__global__ void __launch_bounds__(kThreads)
affine_act_bwd_kernel(const AffineBwd P) {
  const int plane = blockIdx.y;                       // b * C + c
  const int c = plane % P.C;
  const float a = P.scale[c];
  const float a2 = P.gx2 ? P.scale2[c] : 0.f;
  float m = 0.f, r = 0.f, m2 = 0.f, r2 = 0.f;
  if (STATS) {
    if (P.x) { m = P.mean[c]; r = P.rstd[c]; }
    if (P.x2) { m2 = P.mean2[c]; r2 = P.rstd2[c]; }
  }
  float sg = 0.f, sx = 0.f, sx2 = 0.f;
  const size_t base = (size_t)plane * P.hw;
  if (P.vec) {
    const int hw4 = P.hw >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(P.gy + base);
    const float4* y4 = P.y ? reinterpret_cast<const float4*>(P.y + base) : nullptr;
    const float4* x4 = (STATS && P.x) ? reinterpret_cast<const float4*>(P.x + base) : nullptr;
    const float4* x24 = (STATS && P.x2) ? reinterpret_cast<const float4*>(P.x2 + base) : nullptr;
    float4* gx4 = reinterpret_cast<float4*>(P.gx + base);
    float4* gx24 = P.gx2 ? reinterpret_cast<float4*>(P.gx2 + base) : nullptr;
    float4* gr4 = P.gres ? reinterpret_cast<float4*>(P.gres + base) : nullptr;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw4; i += gridDim.x * blockDim.x) {
      float4 g = g4[i];
      if (y4) {
        const float4 t = y4[i];
        g.x = t.x > 0.f ? g.x : 0.f; g.y = t.y > 0.f ? g.y : 0.f; g.z = t.z > 0.f ? g.z : 0.f; g.w = t.w > 0.f ? g.w : 0.f;
      }
      if (gr4) gr4[i] = g;
      gx4[i] = make_float4(g.x * a, g.y * a, g.z * a, g.w * a);
      if (gx24) gx24[i] = make_float4(g.x * a2, g.y * a2, g.z * a2, g.w * a2);
      if (STATS) {
        sg += g.x; sg += g.y; sg += g.z; sg += g.w;
        if (x4) {
          const float4 t = x4[i];
          sx += g.x * ((t.x - m) * r); sx += g.y * ((t.y - m) * r); sx += g.z * ((t.z - m) * r); sx += g.w * ((t.w - m) * r);
        }
        if (x24) {
          const float4 t = x24[i];
          sx2 += g.x * ((t.x - m2) * r2); sx2 += g.y * ((t.y - m2) * r2); sx2 += g.z * ((t.z - m2) * r2); sx2 += g.w * ((t.w - m2) * r2);
        }
      }
    }
  } else {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < P.hw; i += gridDim.x * blockDim.x) {
      float g = P.gy[base + i];
      if (P.y) g = P.y[base + i] > 0.f ? g : 0.f;
      if (P.gres) P.gres[base + i] = g;
      P.gx[base + i] = g * a;
      if (P.gx2) P.gx2[base + i] = g * a2;
      if (STATS) {
        sg += g;
        if (P.x) sx += g * ((P.x[base + i] - m) * r);
        if (P.x2) sx2 += g * ((P.x2[base + i] - m2) * r2);
      }
    }
  }
  if (STATS) {
    __shared__ float red[4];
    sg = block_sum(sg, red);
    sx = block_sum(sx, red);
    sx2 = block_sum(sx2, red);
    if (threadIdx.x == 0) P.part[(size_t)plane * gridDim.x + blockIdx.x] = make_float4(sg, sx, sx2, 0.f);
  }
}

// one wave per channel adds the channel's B * bx partials in float64: lane l takes partials l, l + 64, ... in that order (image-major,
// then block), then the butterfly over the lanes -- one fixed order, so the same data give the same bits.  dbias2 is dbias's sum.
__global__ void __launch_bounds__(kThreads)
affine_act_bwd_finish_kernel(const float4* __restrict__ part, int B, int C, int bx, float* __restrict__ dw, float* __restrict__ db,
                             float* __restrict__ dw2, float* __restrict__ db2) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (c >= C) return;                                 // (wave-uniform; no barrier below)
  double sg = 0., sx = 0., sx2 = 0.;
  const int n = B * bx;
  for (int j = lane; j < n; j += 64) {
    const int b = j / bx, k = j - b * bx;
    const float4 p = part[((size_t)b * C + c) * bx + k];
    sg += (double)p.x; sx += (double)p.y; sx2 += (double)p.z;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sg += __shfl_xor(sg, o, 64); sx += __shfl_xor(sx, o, 64); sx2 += __shfl_xor(sx2, o, 64);
  }
  if (lane == 0) {
    if (dw) { dw[c] = (float)sx; db[c] = (float)sg; }
    if (dw2) { dw2[c] = (float)sx2; db2[c] = (float)sg; }
  }
}

// The stem: y = maxpool3x3/s2/p1(relu(x * scale[c] + shift[c])), NCHW -> a new [B, C, Ho, Wo] tensor.  grid.y = (image, channel)
// plane as in affine_act_kernel.  A thread owns four input columns (two outputs) of kPoolRows output rows: it walks down its
// 2 * kPoolRows + 1 input rows once, the activated odd row carried over as the next window's top row, so inside a strip every
// element is loaded once (16-byte loads when W % 4 == 0; the column left of the quad is a 4-byte load of a line that is in
// the L1 anyway) and only the row between two strips is read twice.
// relu(.) is fmaxf(., 0): +0 or larger, never NaN (the pass this replaces had the same fmaxf in front of the pooling), so the
// maximum of a window is one bit pattern whatever the order, and a padded position can stand in as +0 -- every window holds at
// least one real element.
constexpr int kPoolRows = 4;
template <bool kVec>
__global__ void __launch_bounds__(kThreads)
affine_relu_maxpool_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                           float* __restrict__ y, int C, int H, int W, int Ho, int Wo, int nq, int nitems) {
  const int plane = blockIdx.y;                       // b * C + c
  const int c = plane % C;
  const float a = scale[c], b = shift[c];
  const float* src = x + (size_t)plane * H * W;
  float* dst = y + (size_t)plane * Ho * Wo;
  for (int it = blockIdx.x * blockDim.x + threadIdx.x; it < nitems; it += gridDim.x * blockDim.x) {
    const int s = it / nq, q = it - s * nq;
    const int col = 4 * q;                            // input columns col - 1 .. col + 3 -> outputs 2q, 2q + 1
    const int ho0 = s * kPoolRows;
    // the activated values of one input row at the five columns (+0 outside the image)
    auto load_row = [&](int row, float (&v)[5]) {
      if (row < 0 || row >= H) { v[0] = v[1] = v[2] = v[3] = v[4] = 0.f; return; }
      const float* p = src + (size_t)row * W + col;
      float t0, t1, t2, t3, t4;
      if (kVec) {
        const float4 f = *reinterpret_cast<const float4*>(p);
        t1 = f.x; t2 = f.y; t3 = f.z; t4 = f.w;
      } else {
        t1 = p[0];
        t2 = (col + 1 < W) ? p[1] : 0.f; t3 = (col + 2 < W) ? p[2] : 0.f; t4 = (col + 3 < W) ? p[3] : 0.f;
      }
      t0 = (col > 0) ? p[-1] : 0.f;
      v[0] = fmaxf(t0 * a + b, 0.f); v[1] = fmaxf(t1 * a + b, 0.f); v[2] = fmaxf(t2 * a + b, 0.f);
      v[3] = fmaxf(t3 * a + b, 0.f); v[4] = fmaxf(t4 * a + b, 0.f);
      if (col == 0) v[0] = 0.f;
      if (!kVec) { if (col + 1 >= W) v[2] = 0.f; if (col + 2 >= W) v[3] = 0.f; if (col + 3 >= W) v[4] = 0.f; }
    };
    float top[5];
    load_row(2 * ho0 - 1, top);
#pragma unroll
    for (int k = 0; k < kPoolRows; k++) {
      const int ho = ho0 + k;
      if (ho < Ho) {
        float mid[5], bot[5];
        load_row(2 * ho, mid);
        load_row(2 * ho + 1, bot);
        float m[5];
#pragma unroll
        for (int u = 0; u < 5; u++) { m[u] = fmaxf(fmaxf(top[u], mid[u]), bot[u]); top[u] = bot[u]; }
        const float o0 = fmaxf(fmaxf(m[0], m[1]), m[2]), o1 = fmaxf(fmaxf(m[2], m[3]), m[4]);
        float* d = dst + (size_t)ho * Wo + 2 * q;
        if (kVec) {
          *reinterpret_cast<float2*>(d) = make_float2(o0, o1);
        } else {
          d[0] = o0;
          if (2 * q + 1 < Wo) d[1] = o1;
        }
      }
    }
  }
}

// y = act(x + bias[c] (+ residual)), optionally y2 = y - sub[c]; NCHW, several tensors (FPN levels) per launch.  The
// head's output convolutions run without their bias and this launch adds it for all five levels at once, together with
// what follows in OrientedRepPointsHead.forward_single (head :156-170): ReLU, `+ pts_out_init`, `- dcn_base_offset`.
// Operation order per element is the framework's: fl(x + b), then fl(. + r), then max(., 0), then fl(. - s).
struct BiasLevel {
  const float* x; const float* res; float* y; float* y2;
  int hw;
  int bx0;                // first blockIdx.x of this level
};
struct BiasParams {
  BiasLevel lv[kMaxLevels];
  int nlev, C, relu;
  const float* bias; const float* sub;
};
__global__ void __launch_bounds__(kThreads)
bias_act_multi_kernel(const BiasParams P) {
  int l = 0;                                          // level_of, unrolled over all eight slots: the levels stay in scalar registers
#pragma unroll
  for (int i = 1; i < kMaxLevels; i++) l = (i < P.nlev && (int)blockIdx.x >= P.lv[i].bx0) ? i : l;
  const BiasLevel L = P.lv[l];
  const int plane = blockIdx.y;                       // b * C + c
  const int c = plane % P.C;
  const float b = P.bias ? P.bias[c] : 0.f;
  const float sb = P.sub ? P.sub[c] : 0.f;
  const size_t base = (size_t)plane * L.hw;
  const int bx = blockIdx.x - L.bx0;
  const int nbx = ((l + 1 < P.nlev) ? P.lv[l + 1].bx0 : (int)gridDim.x) - L.bx0;
  if ((L.hw & 3) == 0) {
    const int hw4 = L.hw >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(L.x + base);
    const float4* r4 = L.res ? reinterpret_cast<const float4*>(L.res + base) : nullptr;
    float4* y4 = reinterpret_cast<float4*>(L.y + base);
    float4* z4 = L.y2 ? reinterpret_cast<float4*>(L.y2 + base) : nullptr;
    for (int i = bx * kThreads + threadIdx.x; i < hw4; i += nbx * kThreads) {
      float4 t = x4[i];
      t.x += b; t.y += b; t.z += b; t.w += b;
      if (r4) { const float4 r = r4[i]; t.x += r.x; t.y += r.y; t.z += r.z; t.w += r.w; }
      if (P.relu) relu4(t);
      y4[i] = t;
      if (z4) { t.x -= sb; t.y -= sb; t.z -= sb; t.w -= sb; z4[i] = t; }
    }
  } else {
    for (int i = bx * kThreads + threadIdx.x; i < L.hw; i += nbx * kThreads) {
      float t = L.x[base + i] + b;
      if (L.res) t += L.res[base + i];
      if (P.relu) t = fmaxf(t, 0.f);
      L.y[base + i] = t;
      if (L.y2) L.y2[base + i] = t - sb;
    }
  }
}

// ---- GroupNorm (+ ReLU) backward, all levels in one launch pair -------------------------------------------------------------
// y = relu?(xhat * gamma_c + beta_c), xhat = (x - mean_g) * rstd_g.  With dy' = dy * [y > 0]:
//   dgamma_c = sum_{b,hw} dy' xhat,  dbeta_c = sum_{b,hw} dy'
//   dx = rstd_g * (dy' gamma_c - (A + xhat * Bq) / span),  A = sum_g dy' gamma_c,  Bq = sum_g dy' gamma_c xhat
// pass 1 (one workgroup per 4096-float chunk, as the forward): per channel of the chunk's group the chunk-local sums
//         (sum dy', sum dy' xhat) -> bpart[chunk][cg]; pass 2: every workgroup adds its group's partials in chunk order
//         (fixed order: reproducible), forms A and Bq and writes dx for its chunk; pass 3: dgamma / dbeta per parameter
//         set by a fixed-order sum over tensors, images and chunks.
__global__ void __launch_bounds__(kThreads)
gn_bwd_partial_kernel(const GnParams P) {
  __shared__ float red[4];
  const ChunkGeom g = locate(P, blockIdx.x);
  const GnLevel& L = P.lv[g.lvl];
  const int cg = P.C / P.G;
  const float2 st = P.stats[(size_t)g.lvl * P.B * P.G + g.bg];
  const float mean = st.x, rstd = st.y;
  const float* x = L.x + (size_t)g.bg * g.span + g.n0;
  const float* y = L.y + (size_t)g.bg * g.span + g.n0;             // the forward's output: the ReLU mask is read, not recomputed
  const float* dy = P.dy[g.lvl] + (size_t)g.bg * g.span + g.n0;
  // the chunk's elements e in [0, n): channel (g.n0 + e) / hw of the group; accumulate per channel (<= cg of them)
  const int c_first = g.n0 / L.hw, c_last = (g.n0 + g.n - 1) / L.hw;
  for (int cl = c_first; cl <= c_last; cl++) {
    const int e0 = max(cl * L.hw - g.n0, 0), e1 = min((cl + 1) * L.hw - g.n0, g.n);
    float s1 = 0.f, s2 = 0.f;
    for (int e = e0 + threadIdx.x; e < e1; e += kThreads) {
      const float xv = x[e];
      float d = dy[e];
      if (P.relu && !(y[e] > 0.f)) d = 0.f;
      s1 += d; s2 += d * ((xv - mean) * rstd);
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    if (threadIdx.x == 0) P.bpart[(size_t)blockIdx.x * cg + cl] = make_float4(s1, s2, 0.f, 0.f);
  }
  // channels of the group this chunk does not touch: zero entries (every slot is read by pass 2 / 3)
  for (int cl = threadIdx.x; cl < cg; cl += kThreads)
    if (cl < c_first || cl > c_last) P.bpart[(size_t)blockIdx.x * cg + cl] = make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ void __launch_bounds__(kThreads)
gn_bwd_apply_kernel(const GnParams P) {
  __shared__ float red[4];
  const ChunkGeom g = locate(P, blockIdx.x);
  const GnLevel& L = P.lv[g.lvl];
  const int cg = P.C / P.G, grp = g.bg % P.G;
  const float2 st = P.stats[(size_t)g.lvl * P.B * P.G + g.bg];
  const float mean = st.x, rstd = st.y;
  // the group's partials: thread t takes entries t, t + 256, ... (chunk-major, channel-minor), then a fixed reduction tree
  float pa = 0.f, pb = 0.f;
  {
    const float4* part = P.bpart + ((size_t)L.chunk0 + (size_t)g.bg * L.cpg) * cg;
    for (int i = threadIdx.x; i < L.cpg * cg; i += kThreads) {
      const float4 p = part[i];
      const float gm = L.gamma[grp * cg + i % cg];
      pa += gm * p.x; pb += gm * p.y;
    }
  }
  const float inv = 1.f / (float)g.span;
  const float A = block_sum(pa, red) * inv;
  const float Bq = block_sum(pb, red) * inv;
  const float* x = L.x + (size_t)g.bg * g.span + g.n0;
  const float* y = L.y + (size_t)g.bg * g.span + g.n0;
  const float* dy = P.dy[g.lvl] + (size_t)g.bg * g.span + g.n0;
  float* dx = P.dx[g.lvl] + (size_t)g.bg * g.span + g.n0;
  for (int e = threadIdx.x; e < g.n; e += kThreads) {
    const int c = grp * cg + (g.n0 + e) / L.hw;
    const float gm = L.gamma[c];
    const float xv = x[e];
    float d = dy[e];
    if (P.relu && !(y[e] > 0.f)) d = 0.f;
    const float xh = (xv - mean) * rstd;
    // d * gm rounded on its own, as the terms of A were: contracted into the subtraction (an fma) it keeps the product's low
    // bits, and a span of ONE element -- where A is that very product and dx is 0 -- got rstd = eps^-1/2 times them
    float dg;
    {
#pragma clang fp contract(off)
      dg = d * gm;
    }
    dx[e] = rstd * (dg - A - xh * Bq);
  }
}

// dgamma / dbeta of ONE parameter set: the tensors whose gamma pointer equals `gamma`, fixed order (tensor, image, chunk)
__global__ void gn_bwd_param_kernel(const GnParams P, const float* gamma, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= P.C) return;
  const int cg = P.C / P.G, grp = c / cg, cl = c - grp * cg;
  float s1 = 0.f, s2 = 0.f;
  for (int i = 0; i < P.nlev; i++) {
    const GnLevel& L = P.lv[i];
    if (L.gamma != gamma) continue;
    for (int b = 0; b < P.B; b++) {
      const float4* part = P.bpart + ((size_t)L.chunk0 + (size_t)(b * P.G + grp) * L.cpg) * cg;
      for (int k = 0; k < L.cpg; k++) { const float4 p = part[(size_t)k * cg + cl]; s1 += p.x; s2 += p.y; }
    }
  }
  dbeta[c] = s1; dgamma[c] = s2;
}

// ---- GroupNorm (+ ReLU) of channels-last tensors [B][HW][C] (orp_groupnorm_act_multi_cl) ---------------------------------------
// What sits between two orp_conv_split_multi launches (orp_conv_split.hip): the convolution reads and writes channels-last, so
// the normalisation does too.  A chunk = 4096 / C whole positions (rows of C floats): with 1024 % C == 0 every thread's
// float4s all fall on the SAME four channels, i.e. one group -- the per-channel constants are per-thread constants, and the
// chunk's per-group statistics are a sum over a fixed set of threads.
//   pass 1 (gn_cl_stats): (mean, M2 around that mean) of every group over the chunk's positions, the chunk held in registers;
//   pass 2 (gn_cl_merge): one wave per (tensor, image, group): Chan's merge of the chunk partials -> (mean, rstd);
//   pass 3 (gn_cl_apply): y = relu?(x * a[c] + b[c]), a = rstd * gamma, b = beta - mean * a -- one float4 pass, in place allowed.
struct GnClLevel {
  const float* x; float* y;
  const float* gamma; const float* beta;
  int hw;                 // H*W
  int cpi;                // chunks per image
  int chunk0;             // first chunk of this tensor
};
struct GnClParams {
  GnClLevel lv[kGnMaxLevels];
  int nlev, B, C, G;
  float eps; int relu;
  float2* partial;        // [total_chunks][G] (mean, M2)
  float2* stats;          // [nlev][B][G] (mean, rstd)
  // optional: an upper bound of max |y| over the tensors of a slot, as float bits (what the fp16-pieces convolution that reads
  // y scales its samples by -- orp_conv_split_multi's amax_in -- so that it needs no pass of its own over y)
  float* pmax;            // [total_chunks][G] max |x| of the chunk's group (same layout as partial), or nullptr
  unsigned* amax;         // [nslots], zeroed by the entry
  int slot[kGnMaxLevels];
};

struct ClGeom { int lvl, b, p0, np; };
__device__ __forceinline__ ClGeom cl_locate(const GnClParams& P, int chunk) {
  ClGeom g;
  g.lvl = level_of([&](int i) { return P.lv[i].chunk0; }, P.nlev, chunk);
  const GnClLevel& L = P.lv[g.lvl];
  const int id = chunk - L.chunk0, ppc = kChunk / P.C;
  g.b = id / L.cpi;
  g.p0 = (id - g.b * L.cpi) * ppc;
  g.np = min(ppc, L.hw - g.p0);
  return g;
}

// sum over the threads that hold this thread's group, in a fixed order: thread t holds channels 4 * (t % tpc) .. + 3 of rows
// t / tpc, t / tpc + 256 / tpc, ...; its group's members are rep * tpc + grp * tg + j  (rep < 256 / tpc, j < tg)
__device__ __forceinline__ float group_total(float v, float* sh, int tpc, int tg, int grp) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  float s = 0.f;
  for (int rep = 0; rep < kThreads / tpc; rep++)
    for (int j = 0; j < tg; j++) s += sh[rep * tpc + grp * tg + j];
  return s;
}

__device__ __forceinline__ float group_max(float v, float* sh, int tpc, int tg, int grp) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  float s = 0.f;
  for (int rep = 0; rep < kThreads / tpc; rep++)
    for (int j = 0; j < tg; j++) s = fmaxf(s, sh[rep * tpc + grp * tg + j]);
  return s;
}

__global__ void __launch_bounds__(kThreads)
gn_cl_stats_kernel(const GnClParams P) {
  __shared__ float sh[kThreads];
  const ClGeom g = cl_locate(P, blockIdx.x);
  const GnClLevel& L = P.lv[g.lvl];
  const int n = g.np * P.C;
  const float* src = L.x + ((size_t)g.b * L.hw + g.p0) * P.C;
  const int tpc = P.C >> 2, cg = P.C / P.G, tg = cg >> 2;
  const int grp = (threadIdx.x % tpc) / tg;
  float v[16];
  const float s = chunk_load_sum(src, n, true, v);
  const float mean = group_total(s, sh, tpc, tg, grp) / (float)(g.np * cg);
  const float m2 = group_total(chunk_m2(v, n, true, mean), sh, tpc, tg, grp);
  // partials of one (tensor, image, group) are contiguous over the image's chunks: [tensor][image][group][chunk]
  const size_t slot_ = (size_t)L.chunk0 * P.G + ((size_t)g.b * P.G + grp) * L.cpi + g.p0 / (kChunk / P.C);
  if (threadIdx.x < tpc && threadIdx.x % tg == 0) P.partial[slot_] = make_float2(mean, m2);
  if (P.pmax) {                                            // (block-uniform)
    float am = 0.f;
#pragma unroll
    for (int q = 0; q < 16; q++) am = fmaxf(am, fabsf(v[q]));          // (elements past the chunk's end were loaded as 0)
    am = group_max(am, sh, tpc, tg, grp);
    if (threadIdx.x < tpc && threadIdx.x % tg == 0) P.pmax[slot_] = am;
  }
}

// one workgroup per (tensor, image, group)
__global__ void __launch_bounds__(kThreads)
gn_cl_merge_kernel(const GnClParams P) {
  __shared__ float red[4];
  const int grp = blockIdx.x, b = blockIdx.y, lvl = blockIdx.z;
  const GnClLevel& L = P.lv[lvl];
  const int ppc = kChunk / P.C, cg = P.C / P.G;
  const float2 mv = merge_span(P.partial + (size_t)L.chunk0 * P.G + ((size_t)b * P.G + grp) * L.cpi, L.cpi, ppc, L.hw, cg, red);
  const float mean = mv.x, rstd = rsqrtf(mv.y + P.eps);
  if (threadIdx.x == 0) P.stats[((size_t)lvl * P.B + b) * P.G + grp] = make_float2(mean, rstd);
  if (P.pmax) {
    // |y| = |(x - mean) rstd gamma_c + beta_c| <= (max |x| + |mean|) rstd max |gamma| + max |beta| over the group's channels
    const float* pm = P.pmax + (size_t)L.chunk0 * P.G + ((size_t)b * P.G + grp) * L.cpi;
    float xm = 0.f;
    for (int k = threadIdx.x; k < L.cpi; k += kThreads) xm = fmaxf(xm, pm[k]);
    // the chunk maxima are fmaxf(0, |x|): never negative, never NaN, so their bits order as they do
    __shared__ unsigned redm[4];
    xm = __uint_as_float(block_max(__float_as_uint(xm), redm));
    if (threadIdx.x == 0) {
      float gm = 0.f, bm = 0.f;
      for (int c = grp * cg; c < (grp + 1) * cg; c++) { gm = fmaxf(gm, fabsf(L.gamma[c])); bm = fmaxf(bm, fabsf(L.beta[c])); }
      const float bound = (xm + fabsf(mean)) * rstd * gm + bm;
      atomicMax(P.amax + P.slot[lvl], orp::range_bound_bits(bound));                // (NaN / Inf: no bound, 0)
    }
  }
}

__global__ void __launch_bounds__(kThreads)
gn_cl_apply_kernel(const GnClParams P) {
  const ClGeom g = cl_locate(P, blockIdx.x);
  const GnClLevel& L = P.lv[g.lvl];
  const int n = g.np * P.C;
  const size_t base = ((size_t)g.b * L.hw + g.p0) * P.C;
  const int tpc = P.C >> 2, cg = P.C / P.G;
  const int c0 = (threadIdx.x % tpc) * 4;
  const float2 st = P.stats[((size_t)g.lvl * P.B + g.b) * P.G + c0 / cg];
  const float4 ga = *reinterpret_cast<const float4*>(L.gamma + c0), be = *reinterpret_cast<const float4*>(L.beta + c0);
  const float2 k0 = gn_coef(st.x, st.y, ga.x, be.x), k1 = gn_coef(st.x, st.y, ga.y, be.y);
  const float2 k2 = gn_coef(st.x, st.y, ga.z, be.z), k3 = gn_coef(st.x, st.y, ga.w, be.w);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int e = (threadIdx.x + q * kThreads) * 4;
    if (e < n) {
      float4 t = *reinterpret_cast<const float4*>(L.x + base + e);
      affine_act4(t, k0, k1, k2, k3, P.relu);
      *reinterpret_cast<float4*>(L.y + base + e) = t;
    }
  }
}

// y = relu?(x * a[c] + b[c]) with per-(tensor, image, channel) coefficients (orp_conv_split_gn_finish): the LAST normalisation of a
// tower, materialised for the consumers that cannot apply it on the fly; block 0 also folds the per-group bounds of max |y| into one
// range word per tensor set
__global__ void __launch_bounds__(kThreads)
affine_cl_kernel(const GnClParams P, const float2* __restrict__ coef, const unsigned* __restrict__ bound_in, unsigned* __restrict__ slot_out,
                 int nsets, int per_set) {
  const ClGeom g = cl_locate(P, blockIdx.x);
  const GnClLevel& L = P.lv[g.lvl];
  const int n = g.np * P.C;
  const size_t base = ((size_t)g.b * L.hw + g.p0) * P.C;
  const int tpc = P.C >> 2;
  const int c0 = (threadIdx.x % tpc) * 4;
  const float2* cf = coef + ((size_t)g.lvl * P.B + g.b) * P.C + c0;
  const float2 k0 = cf[0], k1 = cf[1], k2 = cf[2], k3 = cf[3];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int e = (threadIdx.x + q * kThreads) * 4;
    if (e < n) {
      float4 t = *reinterpret_cast<const float4*>(L.x + base + e);
      t.x = fmaf(t.x, k0.x, k0.y); t.y = fmaf(t.y, k1.x, k1.y); t.z = fmaf(t.z, k2.x, k2.y); t.w = fmaf(t.w, k3.x, k3.y);
      if (P.relu) relu4(t);
      *reinterpret_cast<float4*>(L.y + base + e) = t;
    }
  }
  if (blockIdx.x == 0 && bound_in && slot_out) {
    __shared__ unsigned red[4];
    for (int s_ = 0; s_ < nsets; s_++) {
      unsigned m = 0u;
      for (int i = threadIdx.x; i < per_set; i += kThreads) m = max(m, bound_in[(size_t)s_ * per_set + i]);
      m = block_max(m, red);
      if (threadIdx.x == 0) slot_out[s_] = m;
    }
  }
}

// fills P's levels; returns the number of chunks, -1 on bad arguments, -2 when a tensor is too large
int fill_cl(const orp_norm_level* levels, int nlevels, int batch, int channels, int groups, GnClParams& P) {
  if (!levels || nlevels <= 0 || nlevels > kGnMaxLevels || batch <= 0 || batch > 65535 || channels <= 0 || groups <= 0 ||
      channels % groups != 0 || 1024 % channels != 0 || (channels / groups) % 4 != 0)
    return -1;
  P.nlev = nlevels; P.B = batch; P.C = channels; P.G = groups;
  const int ppc = kChunk / channels;
  long chunks = 0;
  for (int i = 0; i < nlevels; i++) {
    const orp_norm_level& lv = levels[i];
    if (!lv.input || !lv.output || lv.height <= 0 || lv.width <= 0) return -1;
    const long hw = (long)lv.height * lv.width;
    if (hw >= (1L << 31) / channels) return -2;
    GnClLevel& L = P.lv[i];
    L.x = lv.input; L.y = lv.output; L.gamma = nullptr; L.beta = nullptr;
    L.hw = (int)hw; L.cpi = (int)((hw + ppc - 1) / ppc); L.chunk0 = (int)chunks;
    chunks += (long)batch * L.cpi;
    if (chunks >= (1L << 30)) return -2;
  }
  for (int i = nlevels; i < kGnMaxLevels; i++) { P.lv[i] = P.lv[0]; P.lv[i].chunk0 = 0x7fffffff; }
  return (int)chunks;
}


int fill(const orp_norm_level* levels, int nlevels, int batch, int channels, int groups, GnParams& P) {
  if (!levels || nlevels <= 0 || nlevels > kGnMaxLevels || batch <= 0 || channels <= 0 || groups <= 0 ||
      channels % groups)
    return -1;
  int chunks = 0;
  for (int i = 0; i < nlevels; i++) {
    if (!levels[i].input || !levels[i].output || levels[i].height <= 0 || levels[i].width <= 0) return -1;
    GnLevel& L = P.lv[i];
    L.x = levels[i].input; L.y = levels[i].output;
    L.gamma = nullptr; L.beta = nullptr;
    L.hw = levels[i].height * levels[i].width;
    const long span = (long)(channels / groups) * L.hw;
    if (span >= (1L << 30)) return -2;
    L.cpg = (int)((span + kChunk - 1) / kChunk);
    L.chunk0 = chunks;
    chunks += batch * groups * L.cpg;
  }
  for (int i = nlevels; i < kGnMaxLevels; i++) { P.lv[i] = P.lv[0]; P.lv[i].chunk0 = 0x7fffffff; }
  P.nlev = nlevels; P.B = batch; P.C = channels; P.G = groups;
  return chunks;
}

// what fill / fill_cl's count means to an entry
int fill_status(int chunks) { return chunks == -2 ? ORP_ETOOBIG : chunks <= 0 ? ORP_EINVAL : ORP_OK; }

// the levels' affine parameters (GnParams / GnClParams); false when one is missing (ORP_EINVAL)
template <class Params>
bool set_affine(Params& P, const float* const* gammas, const float* const* betas, int n) {
  for (int i = 0; i < n; i++) {
    if (!gammas[i] || !betas[i]) return false;
    P.lv[i].gamma = gammas[i]; P.lv[i].beta = betas[i];
  }
  return true;
}

int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? ORP_OK : (int)e;
}

// grid.x of the per-plane kernels: about 4 work items (float4s when hw % 4 == 0) per thread, between 1 and 64 blocks
int plane_blocks(int hw) {
  const int per = ((hw & 3) == 0) ? (hw >> 2) : hw;
  const int bx = (per + kThreads * 4 - 1) / (kThreads * 4);
  return bx < 1 ? 1 : bx > 64 ? 64 : bx;
}

// orp_groupnorm_act_multi_ex and _train: the launch pair, the second one also storing (mean, rstd) per span when asked to
int gn_nchw_forward(const orp_norm_level* levels, const float* const* gammas_host, const float* const* betas_host, int nlevels,
                    int batch, int channels, int groups, float eps, int relu, bool train, float* stats, void* workspace,
                    size_t workspace_bytes, void* stream) {
  GnParams P;
  const int chunks = fill(levels, nlevels, batch, channels, groups, P);
  if (const int rc = fill_status(chunks)) return rc;
  if (!gammas_host || !betas_host || (train && !stats)) return ORP_EINVAL;
  if (!workspace || workspace_bytes < sizeof(float2) * (size_t)chunks) return ORP_EWORKSPACE;
  if (!set_affine(P, gammas_host, betas_host, nlevels)) return ORP_EINVAL;
  P.eps = eps; P.relu = relu;
  P.partial = reinterpret_cast<float2*>(workspace);
  P.stats = train ? reinterpret_cast<float2*>(stats) : nullptr;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gn_stats_kernel, dim3(chunks), dim3(kThreads), 0, st, P);
  hipLaunchKernelGGL(gn_apply_kernel, dim3(chunks), dim3(kThreads), 0, st, P);
  return launch_status();
}

}  // namespace

extern "C" {

size_t orp_groupnorm_workspace_bytes(const orp_norm_level* levels, int nlevels, int batch, int channels, int groups) {
  GnParams P;
  const int chunks = fill(levels, nlevels, batch, channels, groups, P);
  return chunks > 0 ? sizeof(float2) * (size_t)chunks + 256 : 256;
}

int orp_groupnorm_act_multi_ex(const orp_norm_level* levels, const float* const* gammas_host,
                               const float* const* betas_host, int nlevels, int batch, int channels, int groups,
                               float eps, int relu, void* workspace, size_t workspace_bytes, void* stream) {
  return gn_nchw_forward(levels, gammas_host, betas_host, nlevels, batch, channels, groups, eps, relu, false, nullptr, workspace,
                         workspace_bytes, stream);
}

int orp_groupnorm_act_multi_nhwc(const orp_norm_level* levels, const float* const* gammas_host,
                                 const float* const* betas_host, float* const* nhwc_out_host, int nlevels, int batch,
                                 int channels, int groups, float eps, int relu, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  GnParams P;
  if (!levels || nlevels <= 0 || nlevels > kGnMaxLevels) return ORP_EINVAL;
  orp_norm_level tmp[kGnMaxLevels];
  for (int i = 0; i < nlevels; i++) { tmp[i] = levels[i]; if (!tmp[i].output) tmp[i].output = const_cast<float*>(tmp[i].input); }
  const int chunks = fill(tmp, nlevels, batch, channels, groups, P);
  if (const int rc = fill_status(chunks)) return rc;
  if (!gammas_host || !betas_host || !nhwc_out_host) return ORP_EINVAL;
  if (channels % 32 != 0 || 32 % (channels / groups) != 0 || batch > 65535) return ORP_EINVAL;
  if (!workspace || workspace_bytes < sizeof(float2) * (size_t)chunks) return ORP_EWORKSPACE;
  GnNhwc T;
  int bx = 0;
  if (!set_affine(P, gammas_host, betas_host, nlevels)) return ORP_EINVAL;
  for (int i = 0; i < nlevels; i++) {
    if (!nhwc_out_host[i]) return ORP_EINVAL;
    T.out[i] = nhwc_out_host[i];
    T.nchw[i] = levels[i].output;                       // NULL: the channels-last tensor is the only output
    T.bx0[i] = bx;
    bx += (P.lv[i].hw + 31) / 32;
  }
  for (int i = nlevels; i <= kGnMaxLevels; i++) T.bx0[i] = 0x7fffffff;
  for (int i = nlevels; i < kGnMaxLevels; i++) { T.out[i] = T.out[0]; T.nchw[i] = nullptr; }
  P.eps = eps; P.relu = relu;
  P.partial = reinterpret_cast<float2*>(workspace);
  P.stats = nullptr;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gn_stats_kernel, dim3(chunks), dim3(kThreads), 0, st, P);
  hipLaunchKernelGGL(gn_apply_nhwc_kernel, dim3(bx, channels / 32, batch), dim3(kThreads), 0, st, P, T);
  return launch_status();
}

static size_t gn_cl_stat_offset(size_t chunks, int groups) { return (sizeof(float2) * chunks * groups + 255) & ~(size_t)255; }

size_t orp_groupnorm_cl_workspace_bytes(const orp_norm_level* levels, int nlevels, int batch, int channels, int groups) {
  GnClParams P;
  const int chunks = fill_cl(levels, nlevels, batch, channels, groups, P);
  if (chunks <= 0) return 0;
  // partials | (mean, rstd) per (tensor, image, group) | per-chunk group maxima of the _amax entry
  return ((gn_cl_stat_offset(chunks, groups) + sizeof(float2) * (size_t)nlevels * batch * groups + 255) & ~(size_t)255) +
         sizeof(float) * (size_t)chunks * groups;
}

static int gn_cl_impl(const orp_norm_level* levels, const float* const* gammas_host, const float* const* betas_host,
                      int nlevels, int batch, int channels, int groups, float eps, int relu, const int* slots_host,
                      uint32_t* amax_out, int nslots, void* workspace, size_t workspace_bytes, void* stream) {
  GnClParams P;
  const int chunks = fill_cl(levels, nlevels, batch, channels, groups, P);
  if (const int rc = fill_status(chunks)) return rc;
  if (!gammas_host || !betas_host) return ORP_EINVAL;
  if (amax_out && (!slots_host || nslots <= 0)) return ORP_EINVAL;
  const size_t stat_off = gn_cl_stat_offset(chunks, groups);
  const size_t pmax_off = (stat_off + sizeof(float2) * (size_t)nlevels * batch * groups + 255) & ~(size_t)255;
  const size_t need = amax_out ? pmax_off + sizeof(float) * (size_t)chunks * groups : pmax_off;
  if (!workspace || workspace_bytes < need) return ORP_EWORKSPACE;
  if (!set_affine(P, gammas_host, betas_host, nlevels)) return ORP_EINVAL;
  for (int i = 0; i < nlevels; i++) {
    if (amax_out && (slots_host[i] < 0 || slots_host[i] >= nslots)) return ORP_EINVAL;
    P.slot[i] = amax_out ? slots_host[i] : 0;
  }
  for (int i = nlevels; i < kGnMaxLevels; i++) P.slot[i] = 0;
  P.eps = eps; P.relu = relu;
  P.partial = reinterpret_cast<float2*>(workspace);
  P.stats = reinterpret_cast<float2*>(reinterpret_cast<char*>(workspace) + stat_off);
  P.pmax = amax_out ? reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + pmax_off) : nullptr;
  P.amax = amax_out;
  hipStream_t st = (hipStream_t)stream;
  if (amax_out) {
    const hipError_t me = orp::fill_async(amax_out, 0, sizeof(unsigned) * (size_t)(nslots), st);
    if (me != hipSuccess) return (int)me;
  }
  hipLaunchKernelGGL(gn_cl_stats_kernel, dim3(chunks), dim3(kThreads), 0, st, P);
  hipLaunchKernelGGL(gn_cl_merge_kernel, dim3(groups, batch, nlevels), dim3(kThreads), 0, st, P);
  hipLaunchKernelGGL(gn_cl_apply_kernel, dim3(chunks), dim3(kThreads), 0, st, P);
  return launch_status();
}

int orp_affine_act_multi_cl(const orp_norm_level* levels, int nlevels, int batch, int channels, const float* coef, int relu,
                            const uint32_t* bound_in, int nsets, int per_set, uint32_t* slot_out, void* stream) {
  GnClParams P;
  const int chunks = fill_cl(levels, nlevels, batch, channels, 1, P);
  if (const int rc = fill_status(chunks)) return rc;
  if (!coef || (bound_in && (!slot_out || nsets <= 0 || per_set <= 0))) return ORP_EINVAL;
  P.eps = 0.f; P.relu = relu ? 1 : 0; P.partial = nullptr; P.stats = nullptr; P.pmax = nullptr; P.amax = nullptr;
  hipLaunchKernelGGL(affine_cl_kernel, dim3(chunks), dim3(kThreads), 0, (hipStream_t)stream, P, reinterpret_cast<const float2*>(coef),
                     bound_in, slot_out, nsets, per_set);
  return launch_status();
}

int orp_groupnorm_act_multi_cl(const orp_norm_level* levels, const float* const* gammas_host, const float* const* betas_host,
                               int nlevels, int batch, int channels, int groups, float eps, int relu, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return gn_cl_impl(levels, gammas_host, betas_host, nlevels, batch, channels, groups, eps, relu, nullptr, nullptr, 0, workspace,
                    workspace_bytes, stream);
}

int orp_groupnorm_act_multi_cl_amax(const orp_norm_level* levels, const float* const* gammas_host, const float* const* betas_host,
                                    int nlevels, int batch, int channels, int groups, float eps, int relu, const int* slots_host,
                                    uint32_t* amax_out, int nslots, void* workspace, size_t workspace_bytes, void* stream) {
  if (!amax_out) return ORP_EINVAL;
  return gn_cl_impl(levels, gammas_host, betas_host, nlevels, batch, channels, groups, eps, relu, slots_host, amax_out, nslots,
                    workspace, workspace_bytes, stream);
}

int orp_groupnorm_act_multi_train(const orp_norm_level* levels, const float* const* gammas_host,
                                  const float* const* betas_host, int nlevels, int batch, int channels, int groups,
                                  float eps, int relu, float* stats, void* workspace, size_t workspace_bytes, void* stream) {
  return gn_nchw_forward(levels, gammas_host, betas_host, nlevels, batch, channels, groups, eps, relu, true, stats, workspace,
                         workspace_bytes, stream);
}

size_t orp_groupnorm_backward_workspace_bytes(const orp_norm_level* levels, int nlevels, int batch, int channels, int groups) {
  GnParams P;
  const int chunks = fill(levels, nlevels, batch, channels, groups, P);
  return chunks > 0 ? sizeof(float4) * (size_t)chunks * (size_t)(channels / groups) + 256 : 256;
}

int orp_groupnorm_act_multi_backward(const orp_norm_level* levels, const float* const* grad_outputs_host,
                                     float* const* grad_inputs_host, const float* const* gammas_host,
                                     const float* const* betas_host, float* const* dgammas_host, float* const* dbetas_host,
                                     int nlevels, int batch, int channels, int groups, int relu, const float* stats,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  GnParams P;
  const int chunks = fill(levels, nlevels, batch, channels, groups, P);
  if (const int rc = fill_status(chunks)) return rc;
  if (!grad_outputs_host || !grad_inputs_host || !gammas_host || !betas_host || !dgammas_host ||
      !dbetas_host || !stats)
    return ORP_EINVAL;
  const int cg = channels / groups;
  if (!workspace || workspace_bytes < sizeof(float4) * (size_t)chunks * cg) return ORP_EWORKSPACE;
  if (!set_affine(P, gammas_host, betas_host, nlevels)) return ORP_EINVAL;
  for (int i = 0; i < nlevels; i++) {
    if (!grad_outputs_host[i] || !grad_inputs_host[i]) return ORP_EINVAL;
    P.dy[i] = grad_outputs_host[i]; P.dx[i] = grad_inputs_host[i];
  }
  for (int i = nlevels; i < kGnMaxLevels; i++) { P.dy[i] = nullptr; P.dx[i] = nullptr; }
  P.eps = 0.f; P.relu = relu;
  P.partial = nullptr;
  P.stats = reinterpret_cast<float2*>(const_cast<float*>(stats));
  P.bpart = reinterpret_cast<float4*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gn_bwd_partial_kernel, dim3(chunks), dim3(kThreads), 0, st, P);
  hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3(chunks), dim3(kThreads), 0, st, P);
  // one launch per distinct parameter set (the tensors sharing a GroupNorm module)
  for (int i = 0; i < nlevels; i++) {
    bool first = true;
    for (int j = 0; j < i; j++) if (gammas_host[j] == gammas_host[i]) first = false;
    if (!first || !dgammas_host[i] || !dbetas_host[i]) continue;
    hipLaunchKernelGGL(gn_bwd_param_kernel, dim3((channels + 255) / 256), dim3(256), 0, st, P, gammas_host[i], dgammas_host[i],
                       dbetas_host[i]);
  }
  return launch_status();
}

int orp_groupnorm_act_multi(const orp_norm_level* levels, int nlevels, int batch, int channels, int groups,
                            const float* gamma, const float* beta, float eps, int relu, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (nlevels <= 0 || nlevels > kGnMaxLevels) return ORP_EINVAL;
  const float* g[kGnMaxLevels]; const float* b[kGnMaxLevels];
  for (int i = 0; i < nlevels; i++) { g[i] = gamma; b[i] = beta; }
  return orp_groupnorm_act_multi_ex(levels, g, b, nlevels, batch, channels, groups, eps, relu, workspace, workspace_bytes,
                                    stream);
}

// range_out (or NULL): one word left holding max range_bits(y) as float bits, zeroed here by a kernel launch (fill_async)
int orp_affine_act_range(const float* x, const float* residual, const float* scale, const float* shift, float* y, int batch,
                         int channels, int hw, int relu, uint32_t* range_out, void* stream) {
  if (!x || !scale || !shift || !y || batch <= 0 || channels <= 0 || hw <= 0) return ORP_EINVAL;
  if ((long)batch * channels > 65535L * 1024) return ORP_ETOOBIG;
  const dim3 grid(plane_blocks(hw), batch * channels);
  if (range_out) {
    hipError_t e = orp::fill_async(range_out, 0, sizeof(uint32_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(affine_act_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, x, residual, scale, shift, y, channels,
                       hw, relu, range_out);
  } else {
    hipLaunchKernelGGL(affine_act_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, x, residual, scale, shift, y, channels,
                       hw, relu, (unsigned*)nullptr);
  }
  return launch_status();
}

int orp_affine_act(const float* x, const float* residual, const float* scale, const float* shift, float* y, int batch,
                   int channels, int hw, int relu, void* stream) {
  return orp_affine_act_range(x, residual, scale, shift, y, batch, channels, hw, relu, nullptr, stream);
}

int orp_affine2_act(const float* x, const float* residual, const float* scale, const float* shift, const float* scale2,
                    const float* shift2, float* y, int batch, int channels, int hw, int relu, void* stream) {
  if (!x || !residual || !scale || !shift || !scale2 || !shift2 || !y || batch <= 0 || channels <= 0 || hw <= 0) return ORP_EINVAL;
  if ((long)batch * channels > 65535L * 1024) return ORP_ETOOBIG;
  hipLaunchKernelGGL(affine2_act_kernel, dim3(plane_blocks(hw), batch * channels), dim3(kThreads), 0, (hipStream_t)stream, x, residual,
                     scale, shift, scale2, shift2, y, channels, hw, relu);
  return launch_status();
}

size_t orp_affine_act_backward_workspace_bytes(int batch, int channels, int hw) {
  if (batch <= 0 || channels <= 0 || hw <= 0) return sizeof(float4);
  return sizeof(float4) * (size_t)batch * (size_t)channels * (size_t)plane_blocks(hw);
}

int orp_affine2_act_backward(const float* grad_y, const float* y, const float* x, const float* scale, const float* mean,
                             const float* rstd, const float* x2, const float* scale2, const float* mean2, const float* rstd2,
                             float* grad_x, float* grad_x2, float* grad_res, float* dweight, float* dbias, float* dweight2,
                             float* dbias2, int batch, int channels, int hw, void* workspace, size_t workspace_bytes, void* stream) {
  if (!grad_y || !scale || !grad_x || batch <= 0 || channels <= 0 || hw <= 0) return ORP_EINVAL;
  if ((dweight == nullptr) != (dbias == nullptr) || (dweight2 == nullptr) != (dbias2 == nullptr)) return ORP_EINVAL;
  if (dweight && (!x || !mean || !rstd)) return ORP_EINVAL;
  if (dweight2 && (!x2 || !mean2 || !rstd2)) return ORP_EINVAL;
  if (grad_x2 && !scale2) return ORP_EINVAL;
  if (grad_x == grad_y || (grad_x2 && (grad_x2 == grad_y || grad_x2 == grad_x || grad_x2 == grad_res)) || grad_res == grad_x) return ORP_EINVAL;
  if ((long)batch * channels > 65535L * 1024) return ORP_ETOOBIG;
  const bool stats = dweight || dweight2;
  if (stats && (!workspace || ((uintptr_t)workspace & 15) != 0 ||
                workspace_bytes < orp_affine_act_backward_workspace_bytes(batch, channels, hw)))
    return ORP_EINVAL;
  AffineBwd P;
  P.gy = grad_y; P.y = y; P.x = dweight ? x : nullptr; P.x2 = dweight2 ? x2 : nullptr;
  P.scale = scale; P.mean = mean; P.rstd = rstd; P.scale2 = scale2; P.mean2 = mean2; P.rstd2 = rstd2;
  P.gx = grad_x; P.gx2 = grad_x2; P.gres = grad_res;
  P.part = reinterpret_cast<float4*>(workspace);
  P.C = channels; P.hw = hw;
  const uintptr_t bits = (uintptr_t)P.gy | (uintptr_t)P.y | (uintptr_t)P.x | (uintptr_t)P.x2 | (uintptr_t)P.gx | (uintptr_t)P.gx2 |
                         (uintptr_t)P.gres;
  P.vec = ((hw & 3) == 0 && (bits & 15) == 0) ? 1 : 0;
  const int bx = plane_blocks(hw);
  const dim3 grid(bx, batch * channels);
  hipStream_t st = (hipStream_t)stream;
  if (stats) {
    hipLaunchKernelGGL(affine_act_bwd_kernel<true>, grid, dim3(kThreads), 0, st, P);
    hipLaunchKernelGGL(affine_act_bwd_finish_kernel, dim3((channels + kThreads / 64 - 1) / (kThreads / 64)), dim3(kThreads), 0, st,
                       (const float4*)P.part, batch, channels, bx, dweight, dbias, dweight2, dbias2);
  } else {
    hipLaunchKernelGGL(affine_act_bwd_kernel<false>, grid, dim3(kThreads), 0, st, P);
  }
  return launch_status();
}

int orp_affine_act_backward(const float* grad_y, const float* y, const float* x, const float* scale, const float* mean,
                            const float* rstd, float* grad_x, float* grad_res, float* dweight, float* dbias, int batch, int channels,
                            int hw, void* workspace, size_t workspace_bytes, void* stream) {
  return orp_affine2_act_backward(grad_y, y, x, scale, mean, rstd, nullptr, nullptr, nullptr, nullptr, grad_x, nullptr, grad_res,
                                  dweight, dbias, nullptr, nullptr, batch, channels, hw, workspace, workspace_bytes, stream);
}

int orp_affine_relu_maxpool(const float* x, const float* scale, const float* shift, float* y, int batch, int channels,
                            int height, int width, void* stream) {
  if (!x || !scale || !shift || !y || x == y || batch <= 0 || channels <= 0 || height <= 0 || width <= 0) return ORP_EINVAL;
  if ((long)batch * channels > 65535L || (long)height * width >= (1L << 31)) return ORP_ETOOBIG;
  const int ho = (height - 1) / 2 + 1, wo = (width - 1) / 2 + 1;   // kernel 3, stride 2, padding 1, floor mode
  const int nq = (wo + 1) / 2;                                      // column quads: two outputs each
  const long items = (long)nq * ((ho + kPoolRows - 1) / kPoolRows);
  long bx = (items + kThreads - 1) / kThreads;
  if (bx > 65535) bx = 65535;                                       // (the kernel strides over the rest)
  const bool vec = (width & 3) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 7) == 0;
  const dim3 grid((unsigned)bx, batch * channels);
  if (vec)
    hipLaunchKernelGGL(affine_relu_maxpool_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, x, scale, shift, y, channels,
                       height, width, ho, wo, nq, (int)items);
  else
    hipLaunchKernelGGL(affine_relu_maxpool_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, x, scale, shift, y, channels,
                       height, width, ho, wo, nq, (int)items);
  return launch_status();
}

// workspace of orp_fpn_topdown_nhwc: chunk partials | (mean, rstd) per (level, image, group)
static size_t td_stats_offset(size_t chunks) { return (sizeof(float2) * chunks + 255) & ~(size_t)255; }

size_t orp_fpn_topdown_workspace_bytes(const orp_norm_level* levels, int nlevels, int batch, int channels, int groups) {
  GnParams P;
  const int chunks = fill(levels, nlevels, batch, channels, groups, P);
  if (chunks <= 0) return 256;
  return td_stats_offset(chunks) + sizeof(float2) * (size_t)nlevels * batch * groups;
}

int orp_fpn_topdown_nhwc(const orp_norm_level* levels, const float* const* gammas_host, const float* const* betas_host,
                         int nlevels, int batch, int channels, int groups, float eps, uint32_t* amax_out, void* workspace,
                         size_t workspace_bytes, void* stream) {
  GnParams P;
  if (!levels || nlevels <= 0 || nlevels > kTdMaxLevels) return ORP_EINVAL;
  const int chunks = fill(levels, nlevels, batch, channels, groups, P);
  if (const int rc = fill_status(chunks)) return rc;
  if (!gammas_host || !betas_host) return ORP_EINVAL;
  if (channels % 32 != 0 || 32 % (channels / groups) != 0 || batch > 65535) return ORP_EINVAL;
  const size_t nspan = (size_t)nlevels * batch * groups;
  const size_t stat_off = td_stats_offset(chunks);
  if (!workspace || ((uintptr_t)workspace & 7) != 0 || workspace_bytes < stat_off + sizeof(float2) * nspan) return ORP_EWORKSPACE;
  TdLevels T;
  int bx = 0;
  if (!set_affine(P, gammas_host, betas_host, nlevels)) return ORP_EINVAL;
  for (int i = 0; i < nlevels; i++) {
    if (levels[i].output == levels[i].input) return ORP_EINVAL;
    // every level exactly twice the next in both dimensions: what makes nearest-neighbour upsampling an index shift
    if (i + 1 < nlevels && (levels[i].height != 2 * levels[i + 1].height || levels[i].width != 2 * levels[i + 1].width))
      return ORP_EINVAL;
    T.out[i] = levels[i].output; T.width[i] = levels[i].width;
    T.bx0[i] = bx;
    bx += (P.lv[i].hw + 32 * kTdTiles - 1) / (32 * kTdTiles);
  }
  for (int i = nlevels; i <= kTdMaxLevels; i++) T.bx0[i] = 0x7fffffff;
  for (int i = nlevels; i < kTdMaxLevels; i++) { T.out[i] = T.out[0]; T.width[i] = T.width[0]; }
  T.stats = reinterpret_cast<float2*>(reinterpret_cast<char*>(workspace) + stat_off);
  T.amax = amax_out;
  P.eps = eps; P.relu = 0;
  P.partial = reinterpret_cast<float2*>(workspace);
  P.stats = nullptr;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gn_stats_kernel, dim3(chunks), dim3(kThreads), 0, st, P);
  hipLaunchKernelGGL(gn_merge_kernel, dim3(batch * groups, nlevels), dim3(kThreads), 0, st, P, T);
  hipLaunchKernelGGL(fpn_topdown_nhwc_kernel, dim3(bx, channels / 32, batch), dim3(kThreads), 0, st, P, T);
  return launch_status();
}

int orp_bias_act_multi(const orp_bias_level* levels_host, int nlevels, int batch, int channels, const float* bias,
                       const float* sub, int relu, void* stream) {
  if (!levels_host || nlevels <= 0 || nlevels > kMaxLevels || batch <= 0 || channels <= 0) return ORP_EINVAL;
  if ((long)batch * channels > 65535L) return ORP_ETOOBIG;
  BiasParams P;
  P.nlev = nlevels; P.C = channels; P.relu = relu ? 1 : 0; P.bias = bias; P.sub = sub;
  int bx = 0;
  for (int i = 0; i < nlevels; i++) {
    const orp_bias_level& lv = levels_host[i];
    if (!lv.input || !lv.output || lv.height <= 0 || lv.width <= 0 || (lv.output2 && !sub)) return ORP_EINVAL;
    BiasLevel& L = P.lv[i];
    L.x = lv.input; L.res = lv.residual; L.y = lv.output; L.y2 = lv.output2;
    L.hw = lv.height * lv.width;
    L.bx0 = bx;
    bx += plane_blocks(L.hw);
  }
  for (int i = nlevels; i < kMaxLevels; i++) { P.lv[i] = P.lv[0]; P.lv[i].bx0 = 0x7fffffff; }
  hipLaunchKernelGGL(bias_act_multi_kernel, dim3(bx, batch * channels), dim3(kThreads), 0, (hipStream_t)stream, P);
  return launch_status();
}

}  // extern "C"
