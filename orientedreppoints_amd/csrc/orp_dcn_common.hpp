// orp_dcn_common.hpp -- what the DeformConv sources share: the bilinear sampling table entry of the forward kernels, the tile
// mapping, the NCHW -> NHWC transposition of a launch's levels, and the host helpers of the launchers (output size, workspace
// alignment, tile height, level-slot padding).  Plain functions in the including file's own unnamed namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace {

constexpr int MAX_TAPS = 9;
constexpr int MAX_LEVELS = 8;

// ---- host -----------------------------------------------------------------------------------------------------------------------
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int out_dim(int in, int pad, int dil, int k, int stride) { return (in + 2 * pad - (dil * (k - 1) + 1)) / stride + 1; }

// tile height (in units of 32 output positions) of one forward launch: the cheapest of MT = 1, 2, 3 by rounds of 256 workgroups x
// rows per tile (B = 1, 1024 x 1024: MT = 3 -> 228 tiles, one round), ties towards the taller tile (fewer weight reloads per
// position).  The ONE place that decides it: the fp32 and half launchers and the exported query orp_dcn_forward_h_tile_rows.
inline int pick_tile_rows(long npos_all, int nlevels) {
  int MT = 1;
  long best = -1;
  for (int mt = 1; mt <= 3; mt++) {
    const long t = (npos_all + 32 * mt - 1) / (32 * mt) + nlevels;     // upper bound incl. per-level remainders
    const long cost = ((t + 255) / 256) * mt * 100 + (mt == 1 ? 40 : mt == 2 ? 10 : 0);
    if (best < 0 || cost < best) { best = cost; MT = mt; }
  }
  return MT;
}

// unused level slots of a kernel's parameter block: valid pointers, never selected by level_of_tile
template <typename Level, int N>
inline void pad_level_slots(Level (&lv)[N], int nlev) {
  for (int i = nlev; i < N; i++) { lv[i] = lv[0]; lv[i].tile0 = 0x7fffffff; }
}

// ---- device: tile mapping -------------------------------------------------------------------------------------------------------
// XCD-aware remap: hardware places block b on XCD b % 8; XCD x takes the contiguous slab [x * per, (x + 1) * per) of the work, so
// a feature-map row is pulled into ONE XCD's L2.  The caller drops indices >= total.
__device__ __forceinline__ int xcd_slab_index(int b, int total) { return (b & 7) * ((total + 7) >> 3) + (b >> 3); }

template <typename Level>
__device__ __forceinline__ int level_of_tile(const Level* lv, int nlev, int tile) {
  int lvl = 0;
#pragma unroll 1
  for (int i = 1; i < nlev; i++) if (tile >= lv[i].tile0) lvl = i;
  return lvl;
}

// ---- device: one entry of the bilinear coefficient table ------------------------------------------------------------------------
// Sample `tap` of output position p (b, ho, wo in one index over the level) -> the four neighbour weights (top-left, top-right,
// bottom-left, bottom-right; DCNv2 modulation multiplied in last) and their pixel indices into the NHWC [B * H * W] table.  As the
// reference defines it (deform_conv_cuda_kernel.cu:84-115,190-243): a sample at or beyond -1 / H / W is zero, a neighbour outside
// the image contributes nothing (its index is clamped into the image, its weight is zero).  Zeros for p >= npos.
// P: kh kw sh sw ph pw dh dw; L: H W Ho Wo; off [B, 2 taps, Ho, Wo], mask [B, taps, Ho, Wo] or nullptr, of element type T.
template <typename T, typename Params, typename Level>
__device__ __forceinline__ void sample_entry(const Params& P, const Level& L, const T* off, const T* mask, long p, long npos, int tap,
                                             int taps, int HoWo, float4& w_out, int4& ix_out) {
  float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
  int4 ix = make_int4(0, 0, 0, 0);
  if (p < npos) {
    const int b = (int)(p / HoWo), hw = (int)(p - (long)b * HoWo);
    const int ho = hw / L.Wo, wo = hw - ho * L.Wo;
    const int ki = tap / P.kw, kj = tap - ki * P.kw;
    const T* ob = off + ((size_t)b * 2 * taps + 2 * tap) * HoWo + hw;
    const float off_h = (float)ob[0], off_w = (float)ob[HoWo];
    const float h_im = (float)(ho * P.sh - P.ph + ki * P.dh) + off_h;
    const float w_im = (float)(wo * P.sw - P.pw + kj * P.dw) + off_w;
    if (h_im > -1.f && w_im > -1.f && h_im < (float)L.H && w_im < (float)L.W) {
      const int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
      const int h_high = h_low + 1, w_high = w_low + 1;
      const float lh = h_im - (float)h_low, lw = w_im - (float)w_low;
      const float hh = 1.f - lh, hw_ = 1.f - lw;
      const bool t_ok = h_low >= 0, b_ok = h_high <= L.H - 1, l_ok = w_low >= 0, r_ok = w_high <= L.W - 1;
      const int hl = t_ok ? h_low : 0, hhg = b_ok ? h_high : L.H - 1, wl = l_ok ? w_low : 0, whg = r_ok ? w_high : L.W - 1;
      w.x = (t_ok && l_ok) ? hh * hw_ : 0.f;
      w.y = (t_ok && r_ok) ? hh * lw : 0.f;
      w.z = (b_ok && l_ok) ? lh * hw_ : 0.f;
      w.w = (b_ok && r_ok) ? lh * lw : 0.f;
      const int base = b * L.H;
      ix.x = (base + hl) * L.W + wl;
      ix.y = (base + hl) * L.W + whg;
      ix.z = (base + hhg) * L.W + wl;
      ix.w = (base + hhg) * L.W + whg;
      if (mask) {                                       // DCNv2: the sample is scaled by its modulation scalar
        const float mm = (float)mask[((size_t)b * taps + tap) * HoWo + hw];
        w.x *= mm; w.y *= mm; w.z *= mm; w.w *= mm;
      }
    }
  }
  w_out = w; ix_out = ix;
}

// ---- [B][C][HW] -> [B][HW][C] through a 32x33 LDS tile, for every level (of up to two layers) of one launch ---------------------
// blockIdx.x walks the tensors' position tiles back to back.  E: float, or unsigned short for the 2-byte types.
struct TransposeLevels {
  const void* in[2 * MAX_LEVELS];
  void* out[2 * MAX_LEVELS];
  int hw[2 * MAX_LEVELS];
  int bx0[2 * MAX_LEVELS + 1];        // first blockIdx.x of each tensor; bx0[n] = gridDim.x
  int n;
};
template <typename E>
__global__ void nchw_to_nhwc_levels_kernel(const TransposeLevels T, int C) {
  __shared__ E tile[32][33];
  int l = 0;
#pragma unroll
  for (int i = 1; i < 2 * MAX_LEVELS; i++) l = (i < T.n && (int)blockIdx.x >= T.bx0[i]) ? i : l;
  const int HW = T.hw[l];
  const int b = blockIdx.z;
  const int c0 = blockIdx.y * 32, p0 = ((int)blockIdx.x - T.bx0[l]) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 threads: 8 rows per pass
  const E* src = reinterpret_cast<const E*>(T.in[l]) + (size_t)b * C * HW;
  E* dst = reinterpret_cast<E*>(T.out[l]) + (size_t)b * C * HW;
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r, p = p0 + tx;
    tile[r][tx] = (c < C && p < HW) ? src[(size_t)c * HW + p] : (E)0;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int p = p0 + r, c = c0 + tx;
    if (p < HW && c < C) dst[(size_t)p * C + c] = tile[tx][r];
  }
}
// host: start with n = 0, append every tensor, then launch once (at most 2 * MAX_LEVELS tensors: the caller checks)
inline void transpose_append(TransposeLevels& T, const void* in, void* out, int hw) {
  if (T.n == 0) T.bx0[0] = 0;
  T.in[T.n] = in; T.out[T.n] = out; T.hw[T.n] = hw;
  T.bx0[T.n + 1] = T.bx0[T.n] + (hw + 31) / 32;
  T.n++;
}
template <typename E>
inline void transpose_launch(TransposeLevels& T, int C, int batch, hipStream_t st) {
  for (int i = T.n; i < 2 * MAX_LEVELS; i++) { T.in[i] = T.in[0]; T.out[i] = T.out[0]; T.hw[i] = 0; T.bx0[i + 1] = T.bx0[T.n]; }
  hipLaunchKernelGGL(nchw_to_nhwc_levels_kernel<E>, dim3(T.bx0[T.n], (C + 31) / 32, batch), dim3(256), 0, st, T, C);
}

}  // namespace
