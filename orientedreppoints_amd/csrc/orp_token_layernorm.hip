// orp_token_layernorm.hip -- nn.LayerNorm over the last axis of fp32 tokens, with the layout glue next to it folded into the same
// launch (include/orp_hip.h has the contract; docs/notebook/round32.md the measurements).
//
//   y = (x - mean) * rsqrt(var + eps) * gamma + beta        per row of C floats, biased variance, eps inside the root
//
// ONE statistics routine and ONE affine step (`normalise`) for four (source, destination) layouts, which differ only in how a row's
// values reach the registers and where the results go:
//   TOKENS     [T][C] -> [T][C]                              a block's norm1 / norm2
//   MERGE      [B][H][W][C/4] -> [B ceil(H/2) ceil(W/2)][C]  pad + cat of the 2 x 2 neighbourhood + PatchMerging.norm: a gather on load
//   FROM_NCHW  [B][C][L] -> [B L][C]                         the contiguous copy of the transposed view + PatchEmbed.norm
//   TO_NCHW    [B L][C] -> [B][C][L]                         norm<i> + permute(0, 3, 1, 2).contiguous()
//
// A row is held by L lanes of one wave (L = 8, 16, 32 or 64: the fewest with at most four float4 per lane, 64 beyond that), lane j
// owning the float4 number v * L + j for v = 0 .. V - 1; 256 / L rows per pass of a workgroup of 256 threads.  Row loads and stores
// are 16 bytes per lane, consecutive lanes on consecutive addresses.  The row stays in registers for both passes: the mean first, then
// sum (x - mean)^2 (no E[x^2] - mean^2).  Each sum is the lane's own elements in ascending order followed by an xor butterfly over the L
// lanes (fp32 addition commutes, so every lane ends with the same bits): the order is a function of C alone, a row's result does not
// depend on T, on its place in the launch or on the layout.  Every multiply-add is written as fmaf and no other product feeds a sum
// (the mean and the variance are divisions), so contraction has nothing left to decide and the four layouts' instantiations cannot
// round differently.  No atomics, no workspace.
//
// The two NCHW variants transpose a tile of RT tokens x C channels through LDS so that both global sides run along their contiguous
// axis: channel-major in LDS, [C][RT + 1] floats, element (c, r) at c (RT + 1) + ((r + (c / 32) m) mod RT) with m = rows per half
// wave.  Row side (lane j touches channels 4 (vL + j) + e): the 32 lanes of a half wave fall on 32 banks for every L.  Channel side
// (RT consecutive tokens of one channel per RT lanes): conflict-free at RT = 32, two channels per bank at RT = 16 and 8 (free for the
// stores of FROM_NCHW; the loads of TO_NCHW pay one extra LDS cycle there, far below the HBM time of the tile).  RT is 32, 16 or 8:
// the widest whose tile fits 64 KB and still gives every CU a workgroup, else 8 (C = 4096 at RT = 8 is 147 456 B of the 160 KB).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orp_hip.h"
#include "orp_launch.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kCUs = 256;
constexpr int kPlainLds = 65536;        // dynamic LDS a launch may ask for without the function attribute
constexpr int kMaxLds = 163840;
enum { TOKENS = ORP_LN_TOKENS, MERGE = ORP_LN_MERGE, FROM_NCHW = ORP_LN_FROM_NCHW, TO_NCHW = ORP_LN_TO_NCHW };

struct Args {
  const float* x;
  const float* gamma;
  const float* beta;
  float* y;
  long rows;                 // output rows
  int H, W, C;               // MERGE: the source map and the normalised width 4 * (source channels)
  int L;                     // NCHW variants: tokens per image
  int rt_log2, tiles;        // NCHW variants: log2 of the tile's tokens, tiles per image
  float eps;
};

template <int L>
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = L / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// THE statistics and THE affine step: x[v] is the row's float4 number v * L + j (zeros where that is past the row), replaced by y
template <int L, int V>
__device__ __forceinline__ void normalise(float4 (&x)[V], int j, int nv, float c, float eps, const float* __restrict__ gamma,
                                          const float* __restrict__ beta) {
  float s = 0.f;
#pragma unroll
  for (int v = 0; v < V; v++)
    if (v * L + j < nv) s = (((s + x[v].x) + x[v].y) + x[v].z) + x[v].w;
  const float mean = row_sum<L>(s) / c;
  float q = 0.f;
#pragma unroll
  for (int v = 0; v < V; v++)
    if (v * L + j < nv) {
      x[v].x -= mean; x[v].y -= mean; x[v].z -= mean; x[v].w -= mean;
      q = fmaf(x[v].x, x[v].x, q); q = fmaf(x[v].y, x[v].y, q); q = fmaf(x[v].z, x[v].z, q); q = fmaf(x[v].w, x[v].w, q);
    }
  const float r = rsqrtf(row_sum<L>(q) / c + eps);
#pragma unroll
  for (int v = 0; v < V; v++)
    if (v * L + j < nv) {
      const float4 g = reinterpret_cast<const float4*>(gamma)[v * L + j], b = reinterpret_cast<const float4*>(beta)[v * L + j];
      x[v].x = fmaf(x[v].x * r, g.x, b.x); x[v].y = fmaf(x[v].y * r, g.y, b.y);
      x[v].z = fmaf(x[v].z * r, g.z, b.z); x[v].w = fmaf(x[v].w * r, g.w, b.w);
    }
}

// LDS float of channel c, token r of the tile (file comment); M = rows per half wave
template <int M>
__device__ __forceinline__ int tile_at(int c, int r, int rt) {
  return c * (rt + 1) + ((r + (c >> 5) * M) & (rt - 1));
}

template <int LAYOUT, int L, int V>
__global__ __launch_bounds__(kThreads) void token_layernorm_kernel(const Args A) {
  extern __shared__ float tile[];
  constexpr int R = kThreads / L, M = L >= 32 ? 1 : 32 / L;
  const int j = threadIdx.x % L, rl = threadIdx.x / L, nv = A.C >> 2;
  const float c = (float)A.C;
  float4 x[V];
  if (LAYOUT == TOKENS || LAYOUT == MERGE) {
    const long row = (long)blockIdx.x * R + rl;
    const bool live = row < A.rows;
    if (LAYOUT == TOKENS) {
      const float4* src = reinterpret_cast<const float4*>(A.x) + (size_t)(live ? row : 0) * nv;
#pragma unroll
      for (int v = 0; v < V; v++) x[v] = (live && v * L + j < nv) ? src[v * L + j] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      // output row (b, i, k) gathers source positions (2 i + dr, 2 k + dc); quarter q of the row is (dr, dc) = (q & 1, q >> 1): the
      // released weights' order (even, even), (odd, even), (even, odd), (odd, odd).  Positions past an odd H or W are zeros.
      const int Ho = (A.H + 1) >> 1, Wo = (A.W + 1) >> 1, cs4 = nv >> 2;
      const long rr = live ? row : 0;
      const int k = (int)(rr % Wo), i = (int)((rr / Wo) % Ho);
      const long b = rr / ((long)Wo * Ho);
#pragma unroll
      for (int v = 0; v < V; v++) {
        const int f = v * L + j, q = f / cs4, w = f - q * cs4;
        const int hh = 2 * i + (q & 1), ww = 2 * k + (q >> 1);
        const bool in = live && f < nv && hh < A.H && ww < A.W;
        x[v] = in ? reinterpret_cast<const float4*>(A.x)[((size_t)(b * A.H + hh) * A.W + ww) * cs4 + w] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    normalise<L, V>(x, j, nv, c, A.eps, A.gamma, A.beta);
    if (live) {
      float4* dst = reinterpret_cast<float4*>(A.y) + (size_t)row * nv;
#pragma unroll
      for (int v = 0; v < V; v++)
        if (v * L + j < nv) dst[v * L + j] = x[v];
    }
  } else {
    const int rt = 1 << A.rt_log2;
    const int b = blockIdx.x / A.tiles, l0 = (blockIdx.x - b * A.tiles) << A.rt_log2;
    const int n = min(rt, A.L - l0);                                   // live tokens of this tile
    const size_t image = (size_t)b * A.C * A.L + l0;                   // channel-major side: + c * L + r
    if (LAYOUT == FROM_NCHW) {
      for (int t = threadIdx.x; t < (A.C << A.rt_log2); t += kThreads) {
        const int ch = t >> A.rt_log2, r = t & (rt - 1);
        if (r < n) tile[tile_at<M>(ch, r, rt)] = A.x[image + (size_t)ch * A.L + r];
      }
      __syncthreads();
    }
    for (int r0 = 0; r0 < rt; r0 += R) {
      const int r = r0 + rl;
      const bool live = r < n;
      const size_t row = (size_t)b * A.L + l0 + (live ? r : 0);
#pragma unroll
      for (int v = 0; v < V; v++) {
        const int f = v * L + j;
        x[v] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live && f < nv) {
          if (LAYOUT == FROM_NCHW) {
            x[v].x = tile[tile_at<M>(4 * f, r, rt)]; x[v].y = tile[tile_at<M>(4 * f + 1, r, rt)];
            x[v].z = tile[tile_at<M>(4 * f + 2, r, rt)]; x[v].w = tile[tile_at<M>(4 * f + 3, r, rt)];
          } else {
            x[v] = reinterpret_cast<const float4*>(A.x)[row * nv + f];
          }
        }
      }
      normalise<L, V>(x, j, nv, c, A.eps, A.gamma, A.beta);
      if (live) {
#pragma unroll
        for (int v = 0; v < V; v++) {
          const int f = v * L + j;
          if (f < nv) {
            if (LAYOUT == FROM_NCHW) {
              reinterpret_cast<float4*>(A.y)[row * nv + f] = x[v];
            } else {
              tile[tile_at<M>(4 * f, r, rt)] = x[v].x; tile[tile_at<M>(4 * f + 1, r, rt)] = x[v].y;
              tile[tile_at<M>(4 * f + 2, r, rt)] = x[v].z; tile[tile_at<M>(4 * f + 3, r, rt)] = x[v].w;
            }
          }
        }
      }
    }
    if (LAYOUT == TO_NCHW) {
      __syncthreads();
      for (int t = threadIdx.x; t < (A.C << A.rt_log2); t += kThreads) {
        const int ch = t >> A.rt_log2, r = t & (rt - 1);
        if (r < n) A.y[image + (size_t)ch * A.L + r] = tile[tile_at<M>(ch, r, rt)];
      }
    }
  }
}

// lanes per row and float4 per lane: functions of C alone
struct Shape { int lanes, v; };
Shape shape_of(int c) {
  const int nv = c / 4;
  int l = 8;
  while (l < 64 && nv > 4 * l) l *= 2;
  const int v = (nv + l - 1) / l;
  return Shape{l, v <= 4 ? 4 : (v <= 8 ? 8 : 16)};
}

// tokens per tile of the NCHW variants (file comment)
int tile_tokens(long batch, long tokens, int c) {
  const int cand[3] = {32, 16, 8};
  for (int i = 0; i < 3; i++)
    if ((long)c * (cand[i] + 1) * 4 <= kPlainLds && batch * ((tokens + cand[i] - 1) / cand[i]) >= kCUs) return cand[i];
  return 8;
}

template <int LAYOUT, int L, int V>
struct Tag {};

template <int LAYOUT, int L, int V>
hipError_t launch(const Args& A, unsigned grid, size_t lds, hipStream_t st) {
  if (lds > (size_t)kPlainLds) {
    hipError_t e = orp::set_max_dynamic_lds_once<Tag<LAYOUT, L, V>>(
        reinterpret_cast<const void*>(&token_layernorm_kernel<LAYOUT, L, V>), kMaxLds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((token_layernorm_kernel<LAYOUT, L, V>), dim3(grid), dim3(kThreads), lds, st, A);
  return hipGetLastError();
}

template <int LAYOUT>
hipError_t launch_shape(const Args& A, Shape s, unsigned grid, size_t lds, hipStream_t st) {
  if (s.v == 16) return launch<LAYOUT, 64, 16>(A, grid, lds, st);
  if (s.v == 8) return launch<LAYOUT, 64, 8>(A, grid, lds, st);
  if (s.lanes == 64) return launch<LAYOUT, 64, 4>(A, grid, lds, st);
  if (s.lanes == 32) return launch<LAYOUT, 32, 4>(A, grid, lds, st);
  if (s.lanes == 16) return launch<LAYOUT, 16, 4>(A, grid, lds, st);
  return launch<LAYOUT, 8, 4>(A, grid, lds, st);
}

bool known_layout(int layout) { return layout >= TOKENS && layout <= TO_NCHW; }

// output rows and, for the NCHW variants, tokens per image; false where an extent is negative or the counts leave 31 bits
bool extents(int batch, int h, int w, int layout, long* rows, long* per_image) {
  if (batch < 0 || h < 0 || w < 0) return false;
  const long ho = layout == MERGE ? (h + 1) / 2 : h, wo = layout == MERGE ? (w + 1) / 2 : w;
  *per_image = ho * wo;
  *rows = batch * *per_image;
  return true;
}

}  // namespace

extern "C" {

int orp_token_layernorm_ok(int c) { return (c >= 32 && c <= 4096 && c % 32 == 0) ? 1 : 0; }

// lanes per row, rows per workgroup (TOKENS, MERGE) or tokens per tile (the NCHW variants), and the launch's dynamic LDS bytes
int orp_token_layernorm_plan(int batch, int h, int w, int c, int layout, int* lanes, int* rows, int* lds_bytes) {
  long n = 0, per_image = 0;
  if (!orp_token_layernorm_ok(c) || !known_layout(layout) || !lanes || !rows || !lds_bytes || !extents(batch, h, w, layout, &n, &per_image))
    return 0;
  const Shape s = shape_of(c);
  const bool nchw = layout == FROM_NCHW || layout == TO_NCHW;
  const int rt = nchw ? tile_tokens(batch, per_image, c) : 0;
  *lanes = s.lanes;
  *rows = nchw ? rt : kThreads / s.lanes;
  *lds_bytes = nchw ? c * (rt + 1) * 4 : 0;
  return 1;
}

// THE routing rule of the token LayerNorm: where its one launch was measured faster than the stock span it replaces on MI355X -- the
// framework's LayerNorm alone (TOKENS), pad + cat + LayerNorm (MERGE), the contiguous copy + LayerNorm (FROM_NCHW), LayerNorm + the
// permuting copy (TO_NCHW) --, slowest run of this kernel against the fastest stock run (tests/checks/time_swin_norm.py;
// docs/notebook/round32.md has the tables).  A closed table: every span of Swin-T was timed at the token counts of one 1024^2 image and
// of one 1536^2 image; a row routes the token counts from the first to the second where both ends paid.  Nothing below the smallest or
// beyond the largest timed count is routed, and no width or layout that was not timed.  All 24 timed points paid: 1.0 to 1.2 x at stage
// 4's norm1 / norm2 (4.76 us against 4.80 at 1024 rows, the closest), 1.5 to 7.5 x everywhere else.
int orp_token_layernorm_pays(long tokens, int c, int layout) {
  if (!orp_token_layernorm_ok(c) || !known_layout(layout) || tokens <= 0) return 0;
  struct Row { int c, layout; long t_min, t_max; };
  static const Row paid[] = {
      {96, FROM_NCHW, 65536, 147456},                                                                           // PatchEmbed.norm
      {96, TOKENS, 65536, 147456},  {192, TOKENS, 16384, 36864},  {384, TOKENS, 4096, 9216},  {768, TOKENS, 1024, 2304},    // norm1 / norm2
      {96, TO_NCHW, 65536, 147456}, {192, TO_NCHW, 16384, 36864}, {384, TO_NCHW, 4096, 9216}, {768, TO_NCHW, 1024, 2304},   // norm<i>
      {384, MERGE, 16384, 36864},   {768, MERGE, 4096, 9216},     {1536, MERGE, 1024, 2304},                    // PatchMerging.norm
  };
  for (const Row& r : paid)
    if (r.c == c && r.layout == layout && tokens >= r.t_min && tokens <= r.t_max) return 1;
  return 0;
}

int orp_token_layernorm(const float* x, const float* gamma, const float* beta, float* y, int batch, int h, int w, int c, float eps,
                        int layout, void* stream) {
  long rows = 0, per_image = 0;
  if (!x || !gamma || !beta || !y || !orp_token_layernorm_ok(c) || !known_layout(layout) || !extents(batch, h, w, layout, &rows, &per_image))
    return ORP_EINVAL;
  if (((uintptr_t)x & 15) || ((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15) || ((uintptr_t)y & 15) || (const float*)y == x) return ORP_EINVAL;
  if (rows == 0) return ORP_OK;
  if (rows >= (1L << 31) - 64 || (long)batch * h * w >= (1L << 31) - 64) return ORP_ETOOBIG;
  const Shape s = shape_of(c);
  Args A{};
  A.x = x; A.gamma = gamma; A.beta = beta; A.y = y;
  A.rows = rows; A.H = h; A.W = w; A.C = c; A.eps = eps;
  long grid = 0;
  size_t lds = 0;
  if (layout == FROM_NCHW || layout == TO_NCHW) {
    const int rt = tile_tokens(batch, per_image, c);
    A.L = (int)per_image;
    A.rt_log2 = rt == 32 ? 5 : (rt == 16 ? 4 : 3);
    A.tiles = (int)((per_image + rt - 1) / rt);
    grid = (long)batch * A.tiles;
    lds = (size_t)c * (rt + 1) * 4;
  } else {
    const int r = kThreads / s.lanes;
    grid = (rows + r - 1) / r;
  }
  if (grid >= (1L << 31)) return ORP_ETOOBIG;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e;
  if (layout == TOKENS) e = launch_shape<TOKENS>(A, s, (unsigned)grid, lds, st);
  else if (layout == MERGE) e = launch_shape<MERGE>(A, s, (unsigned)grid, lds, st);
  else if (layout == FROM_NCHW) e = launch_shape<FROM_NCHW>(A, s, (unsigned)grid, lds, st);
  else e = launch_shape<TO_NCHW>(A, s, (unsigned)grid, lds, st);
  return e == hipSuccess ? ORP_OK : (int)e;
}

}  // extern "C"
