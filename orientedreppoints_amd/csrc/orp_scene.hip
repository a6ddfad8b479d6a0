// orp_scene.hip -- the device steps between a whole DOTA scene and the per-patch detector (gfx950).
//
//   orp_scene_tiles    crop + channel swap + normalise + type conversion of T tiles of a uint8 HWC scene in one launch: what the
//                      reference does per patch on the host (SplitOnlyImage's crop, the test pipeline's Normalize + Pad +
//                      ImageToTensor), written straight into the detector's input buffer.
//   orp_scene_tiles_resized  the same with the test pipeline's per-patch resize in front (RotateResize(keep_ratio): bilinear,
//                      align_corners=False, rounded to uint8) and Pad's zeros behind: T patches of any size -> [T, 3, pad_h, pad_w].
//   orp_scene_collect  the packed per-tile detections of the static post-processing -> per-class segments of scene-coordinate
//                      fp64 rows, the input of orp_poly_nms_f64_batched; replaces the Task1 text files the reference writes per
//                      patch and parses back (parse_pkl_mege_results_for_dota_evaluation.py, ResultMerge_multi_process.py:182-223).
//
// Built with -ffp-contract=off: the normalisation is imnormalize's two fp32 operations, the translation is poly2origpoly's
// add and divide in fp64, each rounded on its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orp_hip.h"

namespace {

inline int done() { hipError_t e = hipGetLastError(); return e == hipSuccess ? ORP_OK : (int)e; }

// ---- tiles ----------------------------------------------------------------------------------------------------------------
// One lane produces 16 bytes of every output plane: kPix = 4 (fp32) or 8 (fp16 / bf16) consecutive pixels of one tile row,
// i.e. 3 * kPix interleaved source bytes at an arbitrary byte address.  The lane loads the kPix * 3 / 4 + 1 aligned dwords
// that cover them (one wide load where they all lie inside the scene row, byte by byte at the row's ends), shifts the byte
// stream into place with a funnel shift and looks every byte up in a 3 x 256 table of finished output values.  The table is
// built per block from imnormalize's own expression, so the result is the reference's to the bit and the per-pixel work is
// one LDS read.

template <typename T> struct OutOf;
template <> struct OutOf<float> {
  static __device__ __forceinline__ float make(float v) { return v; }
};
template <> struct OutOf<_Float16> {
  static __device__ __forceinline__ _Float16 make(float v) { return (_Float16)v; }          // round to nearest even
};
struct bf16_bits { unsigned short u; };
template <> struct OutOf<bf16_bits> {
  static __device__ __forceinline__ bf16_bits make(float v) {                               // round to nearest even
    const unsigned u = __float_as_uint(v);
    bf16_bits r;
    r.u = (v != v) ? (unsigned short)0x7fc0 : (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    return r;
  }
};

template <int N> struct __attribute__((packed, aligned(4))) Dwords { unsigned v[N]; };
template <typename T, int N> struct __attribute__((aligned(16))) Vec16 { T v[N]; };

constexpr int kTileThreads = 256;
constexpr int kTileIters = 2;          // item chunks per block: the table costs 768 divisions per block

struct Norm3 { float mean[3]; float std[3]; };

// kFlip (the test pipeline's RandomFlip, horizontal, between the crop and Normalize): output column x holds the tile's column
// S - 1 - x.  A lane still loads one aligned group of kPix source pixels -- the mirrored group -- and stores them in reverse.
template <typename T, bool kFlip>
__global__ void __launch_bounds__(kTileThreads)
scene_tiles_kernel(const unsigned char* __restrict__ scene, int H, int W, long long row_stride,
                   const int32_t* __restrict__ origins, int S, Norm3 nrm, int to_rgb, T* __restrict__ out) {
  constexpr int kPix = 16 / (int)sizeof(T);
  constexpr int kWords = kPix * 3 / 4;             // dwords of the aligned byte stream of kPix pixels
  __shared__ T lut[3][256];
  for (int i = threadIdx.x; i < 768; i += kTileThreads) {
    const int c = i >> 8;
    lut[c][i & 255] = OutOf<T>::make(__fdiv_rn((float)(i & 255) - nrm.mean[c], nrm.std[c]));
  }
  __syncthreads();
  const int t = blockIdx.y;
  const int left = origins[2 * t], up = origins[2 * t + 1];
  const int groups = S / kPix;                     // lanes per tile row
  const long long items = (long long)S * groups;
  const T zero = OutOf<T>::make(0.f);
#pragma unroll 1
  for (int it = 0; it < kTileIters; it++) {
    const long long item = ((long long)blockIdx.x * kTileIters + it) * kTileThreads + threadIdx.x;
    if (item >= items) break;
    const int y = (int)(item / groups);
    const int x0 = (int)(item % groups) * kPix;
    const long long ys = (long long)up + y, xs = (long long)left + (kFlip ? S - kPix - x0 : x0);
    unsigned w[kWords];
#pragma unroll
    for (int j = 0; j < kWords; j++) w[j] = 0u;
    const bool any = (ys >= 0) & (ys < H) & (xs < W) & (xs + kPix > 0);
    if (any) {
      const unsigned char* lo = scene + ys * row_stride;               // the scene row's bytes are [lo, hi)
      const unsigned char* hi = lo + (long long)W * 3;
      const long long first = xs * 3;                                  // the lane's first byte, relative to lo
      const unsigned mis = (unsigned)(((uintptr_t)lo + (uintptr_t)first) & 3);
      const unsigned char* al = lo + (first - mis);                    // dword-aligned (pointer arithmetic keeps the address space)
      unsigned d[kWords + 1];
      if ((al >= lo) & (al + 4 * (kWords + 1) <= hi)) {
        const Dwords<kWords + 1> q = *reinterpret_cast<const Dwords<kWords + 1>*>(al);
#pragma unroll
        for (int j = 0; j <= kWords; j++) d[j] = q.v[j];
      } else {                                                         // a row end: nothing outside [lo, hi) is read
#pragma unroll
        for (int j = 0; j <= kWords; j++) {
          unsigned v = 0u;
#pragma unroll
          for (int b = 0; b < 4; b++) {
            const unsigned char* p = al + 4 * j + b;
            if ((p >= lo) & (p < hi)) v |= (unsigned)(*p) << (8 * b);
          }
          d[j] = v;
        }
      }
      const unsigned sh = 8u * mis;
#pragma unroll
      for (int j = 0; j < kWords; j++) w[j] = __funnelshift_r(d[j], d[j + 1], sh);
    }
    Vec16<T, kPix> o[3];
#pragma unroll
    for (int p = 0; p < kPix; p++) {
      const bool in = any & (xs + p >= 0) & (xs + p < W);
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const int k = 3 * p + c;                                       // byte k of the stream: pixel p, source channel c
        const unsigned byte = (w[k >> 2] >> (8 * (k & 3))) & 255u;
        o[c].v[kFlip ? kPix - 1 - p : p] = in ? lut[to_rgb ? 2 - c : c][byte] : zero;
      }
    }
    const size_t plane = (size_t)S * S;
    T* dst = out + (size_t)t * 3 * plane + (size_t)y * S + x0;
#pragma unroll
    for (int c = 0; c < 3; c++) *reinterpret_cast<Vec16<T, kPix>*>(dst + (to_rgb ? 2 - c : c) * plane) = o[c];
  }
}

template <typename T, bool kFlip>
int launch_tiles(const uint8_t* scene, int H, int W, long long stride, const int32_t* origins, int T_, int S, const Norm3& nrm,
                 int to_rgb, void* out, hipStream_t st) {
  constexpr int kPix = 16 / (int)sizeof(T);
  if (S % kPix != 0) return ORP_EINVAL;
  const long long items = (long long)S * (S / kPix);
  const long long per_block = (long long)kTileThreads * kTileIters;
  const long long blocks = (items + per_block - 1) / per_block;
  if (blocks > 0x7fffffffLL || T_ > 65535) return ORP_ETOOBIG;
  hipLaunchKernelGGL((scene_tiles_kernel<T, kFlip>), dim3((unsigned)blocks, (unsigned)T_), dim3(kTileThreads), 0, st, scene, H, W, stride,
                     origins, S, nrm, to_rgb, reinterpret_cast<T*>(out));
  return done();
}

// ---- tiles, resampled ------------------------------------------------------------------------------------------------------
// The test pipeline's RotateResize(keep_ratio) + Normalize + Pad of T patches in one launch.  The lane mapping is the one above
// (16 bytes of every output plane per lane, the normalisation by LDS table); a block is 64 lanes along a row by 4 rows, twice,
// so the axis tables of its kResCols columns and kResRows rows sit in LDS next to the normalisation table.  Per pixel and
// channel: four source bytes, the two horizontal blends, the vertical one -- every product and sum rounded to fp32 on its own
// (the __f*_rn forms never contract) --, rint, clamp, one table read.  With new == src every weight is 0 or 1 and the value is
// the source byte: orp_scene_tiles' output.

constexpr int kResRows = 4 * kTileIters;             // output rows per block

// kFlip mirrors inside the resized patch's own width (Resize -> RandomFlip -> Normalize -> Pad): output column x < new_w takes the
// axis-table entry of column new_w - 1 - x, so the arithmetic per pixel -- and with it every value -- is the unflipped kernel's.
template <typename T, bool kFlip>
__global__ void __launch_bounds__(kTileThreads)
scene_tiles_resized_kernel(const unsigned char* __restrict__ scene, int H, int W, long long row_stride,
                           const int32_t* __restrict__ origins, int src_w, int src_h, int new_w, int new_h, int pad_w, int pad_h,
                           const int32_t* __restrict__ x_i0, const float* __restrict__ x_w1, const int32_t* __restrict__ y_i0,
                           const float* __restrict__ y_w1, Norm3 nrm, int to_rgb, T* __restrict__ out) {
  constexpr int kPix = 16 / (int)sizeof(T);
  constexpr int kResCols = 64 * kPix;                // output columns per block
  __shared__ T lut[3][256];
  __shared__ __attribute__((aligned(16))) int col_i0[kResCols];
  __shared__ __attribute__((aligned(16))) float col_w1[kResCols];
  __shared__ int row_i0[kResRows];
  __shared__ float row_w1[kResRows];
  for (int i = threadIdx.x; i < 768; i += kTileThreads) {
    const int c = i >> 8;
    lut[c][i & 255] = OutOf<T>::make(__fdiv_rn((float)(i & 255) - nrm.mean[c], nrm.std[c]));
  }
  const int col0 = (int)blockIdx.x * kResCols, rowb = (int)blockIdx.y * kResRows;
  for (int i = threadIdx.x; i < kResCols; i += kTileThreads) {
    const int x = col0 + i;
    const bool in = x < new_w;
    const int xt = kFlip ? new_w - 1 - x : x;               // (in [0, new_w) whenever x is)
    col_i0[i] = in ? min(max(x_i0[xt], 0), src_w - 1) : 0;  // (clamped: a wrong table cannot leave the patch)
    col_w1[i] = in ? x_w1[xt] : 0.f;
  }
  if (threadIdx.x < kResRows) {
    const int y = rowb + (int)threadIdx.x;
    const bool in = y < new_h;
    row_i0[threadIdx.x] = in ? min(max(y_i0[y], 0), src_h - 1) : 0;
    row_w1[threadIdx.x] = in ? y_w1[y] : 0.f;
  }
  __syncthreads();
  const int t = blockIdx.z;
  // the patch is kept inside the scene (src_w <= W and src_h <= H are checked on the host): no read leaves the scene
  const int left = min(max(origins[2 * t], 0), W - src_w), up = min(max(origins[2 * t + 1], 0), H - src_h);
  const int lx = (int)(threadIdx.x & 63), ly = (int)(threadIdx.x >> 6);
  const int x0 = col0 + lx * kPix;
  const T zero = OutOf<T>::make(0.f);
  const size_t plane = (size_t)pad_h * pad_w;
  const unsigned char* patch = scene + (long long)up * row_stride + (long long)left * 3;
#pragma unroll 1
  for (int it = 0; it < kTileIters; it++) {
    const int r = it * 4 + ly;
    const int y = rowb + r;
    if ((y >= pad_h) | (x0 >= pad_w)) break;         // (pad_w % kPix == 0: a lane's 16 bytes are inside the row or outside it)
    Vec16<T, kPix> o[3];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int p = 0; p < kPix; p++) o[c].v[p] = zero;
    if ((y < new_h) & (x0 < new_w)) {
      const int ya = row_i0[r], yb = min(ya + 1, src_h - 1);
      const float wy1 = row_w1[r], wy0 = __fsub_rn(1.f, wy1);
      const unsigned char* top = patch + (long long)ya * row_stride;
      const unsigned char* bot = patch + (long long)yb * row_stride;
#pragma unroll
      for (int p = 0; p < kPix; p++) {
        if (x0 + p < new_w) {
          const int xa = col_i0[lx * kPix + p], xb = min(xa + 1, src_w - 1);
          const float wx1 = col_w1[lx * kPix + p], wx0 = __fsub_rn(1.f, wx1);
#pragma unroll
          for (int c = 0; c < 3; c++) {              // c: source channel
            const float a = (float)top[3 * xa + c], b = (float)top[3 * xb + c];
            const float e = (float)bot[3 * xa + c], f = (float)bot[3 * xb + c];
            const float tv = __fadd_rn(__fmul_rn(wx0, a), __fmul_rn(wx1, b));
            const float bv = __fadd_rn(__fmul_rn(wx0, e), __fmul_rn(wx1, f));
            const float v = __fadd_rn(__fmul_rn(wy0, tv), __fmul_rn(wy1, bv));
            const int byte = (int)fminf(fmaxf(rintf(v), 0.f), 255.f);
            o[c].v[p] = lut[to_rgb ? 2 - c : c][byte];
          }
        }
      }
    }
    T* dst = out + (size_t)t * 3 * plane + (size_t)y * pad_w + x0;
#pragma unroll
    for (int c = 0; c < 3; c++) *reinterpret_cast<Vec16<T, kPix>*>(dst + (to_rgb ? 2 - c : c) * plane) = o[c];
  }
}

struct Axes { const int32_t* x_i0; const float* x_w1; const int32_t* y_i0; const float* y_w1; };

template <typename T, bool kFlip>
int launch_tiles_resized(const uint8_t* scene, int H, int W, long long stride, const int32_t* origins, int T_, int src_w,
                         int src_h, int new_w, int new_h, int pad_w, int pad_h, const Axes& ax, const Norm3& nrm, int to_rgb,
                         void* out, hipStream_t st) {
  constexpr int kPix = 16 / (int)sizeof(T);
  if (pad_w % kPix != 0) return ORP_EINVAL;
  const int bx = (pad_w + 64 * kPix - 1) / (64 * kPix), by = (pad_h + kResRows - 1) / kResRows;
  if (by > 65535 || T_ > 65535) return ORP_ETOOBIG;
  hipLaunchKernelGGL((scene_tiles_resized_kernel<T, kFlip>), dim3((unsigned)bx, (unsigned)by, (unsigned)T_), dim3(kTileThreads), 0, st,
                     scene, H, W, stride, origins, src_w, src_h, new_w, new_h, pad_w, pad_h, ax.x_i0, ax.x_w1, ax.y_i0, ax.y_w1,
                     nrm, to_rgb, reinterpret_cast<T*>(out));
  return done();
}

// ---- collect --------------------------------------------------------------------------------------------------------------
// counts per (tile, class) -> exclusive scan (classes outer, tiles inner) -> ranked scatter.  A row's place is
// seg_offsets[class] + rows of that class in earlier tiles + rows of that class earlier in its own tile: the order in which the
// file route appends lines to a class file, computed without any order-dependent atomic.

constexpr int kRow = 28;               // packed row: 18 point coordinates, 8 corners, score, label
constexpr int kCollectThreads = 256;

// rows the tile contributes: its count clamped to [0, m], 0 when it reported overflow (flagged in tile_flag)
__device__ __forceinline__ int tile_rows(const float* __restrict__ tail, int m, int* overflow) {
  const float c = tail[0];
  *overflow = tail[1] != 0.f;
  if (*overflow || !(c > 0.f)) return 0;
  return c < (float)m ? (int)c : m;
}
__device__ __forceinline__ int row_label(const float* __restrict__ row, int C) {
  const float l = row[kRow - 1];
  return (l >= 0.f && l < (float)C) ? (int)l : -1;      // a label outside [0, C) (or NaN) drops the row
}

__global__ void __launch_bounds__(kCollectThreads)
collect_count_kernel(const float* __restrict__ packed, int m, int C, int32_t* __restrict__ cnt, int32_t* __restrict__ tile_flag) {
  extern __shared__ int hist[];
  const int t = blockIdx.x;
  const float* base = packed + (size_t)t * (m + 1) * kRow;
  for (int c = threadIdx.x; c < C; c += kCollectThreads) hist[c] = 0;
  __syncthreads();
  int ovf;
  const int n = tile_rows(base + (size_t)m * kRow, m, &ovf);
  for (int r = threadIdx.x; r < n; r += kCollectThreads) {
    const int l = row_label(base + (size_t)r * kRow, C);
    if (l >= 0) atomicAdd(&hist[l], 1);                   // LDS counter: the sum does not depend on arrival order
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += kCollectThreads) cnt[(size_t)t * C + c] = hist[c];
  if (threadIdx.x == 0) tile_flag[t] = ovf;
}

// one block: cnt [T, C] -> first output row of every (tile, class) in place; seg_offsets [C + 1]; flag
__global__ void __launch_bounds__(kCollectThreads)
collect_scan_kernel(int32_t* __restrict__ cnt, const int32_t* __restrict__ tile_flag, int T_, int C,
                    int32_t* __restrict__ seg_offsets, int32_t* __restrict__ flag) {
  extern __shared__ int total[];                           // [C] rows of a class, then its first row
  __shared__ int any_flag;
  if (threadIdx.x == 0) any_flag = 0;
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += kCollectThreads) {
    int run = 0;
    for (int t = 0; t < T_; t++) {
      const int v = cnt[(size_t)t * C + c];
      cnt[(size_t)t * C + c] = run;
      run += v;
    }
    total[c] = run;
  }
  int f = 0;
  for (int t = threadIdx.x; t < T_; t += kCollectThreads) f |= tile_flag[t];
  if (f) any_flag = 1;                                     // every writer writes the same value
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int c = 0; c < C; c++) {
      const int v = total[c];
      total[c] = run;
      seg_offsets[c] = run;
      run += v;
    }
    seg_offsets[C] = run;
    flag[0] = any_flag;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += kCollectThreads) {
    const int first = total[c];
    for (int t = 0; t < T_; t++) cnt[(size_t)t * C + c] += first;
  }
}

__global__ void __launch_bounds__(kCollectThreads)
collect_scatter_kernel(const float* __restrict__ packed, int m, int C, const int32_t* __restrict__ origins, double rate,
                       const int32_t* __restrict__ first, int capacity_rows, double* __restrict__ dets,
                       int32_t* __restrict__ src) {
  extern __shared__ int next_row[];                        // [C] next output row of every class of this tile
  __shared__ int lab[kCollectThreads];
  const int t = blockIdx.x;
  const float* base = packed + (size_t)t * (m + 1) * kRow;
  for (int c = threadIdx.x; c < C; c += kCollectThreads) next_row[c] = first[(size_t)t * C + c];
  int ovf;
  const int n = tile_rows(base + (size_t)m * kRow, m, &ovf);
  const double left = (double)origins[2 * t], up = (double)origins[2 * t + 1];
  for (int r0 = 0; r0 < n; r0 += kCollectThreads) {
    const int r = r0 + threadIdx.x;
    const float* row = base + (size_t)r * kRow;
    const int l = r < n ? row_label(row, C) : -1;
    lab[threadIdx.x] = l;
    __syncthreads();                                       // (also orders next_row's initialisation / previous update)
    int before = 0, same = 0;
    if (l >= 0) {
      for (int j = 0; j < kCollectThreads; j++) {
        const int e = lab[j] == l;
        same += e;
        before += e & (j < (int)threadIdx.x);
      }
      const int o = next_row[l] + before;
      if (o < capacity_rows) {
        double* d = dets + (size_t)o * 9;
#pragma unroll
        for (int k = 0; k < 4; k++) {                      // poly2origpoly: float(poly[2k] + x) / float(rate)
          d[2 * k] = ((double)row[18 + 2 * k] + left) / rate;
          d[2 * k + 1] = ((double)row[19 + 2 * k] + up) / rate;
        }
        d[8] = (double)row[26];
        src[2 * (size_t)o] = t;
        src[2 * (size_t)o + 1] = r;
      }
    }
    __syncthreads();
    if (l >= 0 && before == 0) next_row[l] += same;        // one writer per class present in the chunk
  }
}

// ---- the entry points' bodies: plain and mirrored differ in one template argument
template <bool kFlip>
int scene_tiles_entry(const uint8_t* scene, int height, int width, long long row_stride_bytes, const int32_t* origins,
                    int num_tiles, int tile, const float* mean_host, const float* std_host, int to_rgb, int out_dtype,
                    void* out, void* stream) {
  if (!scene || !origins || !mean_host || !std_host || !out || height <= 0 || width <= 0 || num_tiles < 0 || tile <= 0 ||
      row_stride_bytes < (long long)width * 3 || ((uintptr_t)out & 15) != 0)
    return ORP_EINVAL;
  if (num_tiles == 0) return ORP_OK;
  Norm3 nrm;
  for (int c = 0; c < 3; c++) { nrm.mean[c] = mean_host[c]; nrm.std[c] = std_host[c]; }
  hipStream_t st = (hipStream_t)stream;
  switch (out_dtype) {
    case 0: return launch_tiles<float, kFlip>(scene, height, width, row_stride_bytes, origins, num_tiles, tile, nrm, to_rgb != 0, out, st);
    case 1: return launch_tiles<_Float16, kFlip>(scene, height, width, row_stride_bytes, origins, num_tiles, tile, nrm, to_rgb != 0, out, st);
    case 2: return launch_tiles<bf16_bits, kFlip>(scene, height, width, row_stride_bytes, origins, num_tiles, tile, nrm, to_rgb != 0, out, st);
    default: return ORP_EINVAL;
  }
}

template <bool kFlip>
int scene_tiles_resized_entry(const uint8_t* scene, int height, int width, long long row_stride_bytes, const int32_t* origins,
                            int num_tiles, int src_w, int src_h, int new_w, int new_h, int pad_w, int pad_h, const int32_t* x_i0,
                            const float* x_w1, const int32_t* y_i0, const float* y_w1, const float* mean_host,
                            const float* std_host, int to_rgb, int out_dtype, void* out, void* stream) {
  if (!scene || !origins || !x_i0 || !x_w1 || !y_i0 || !y_w1 || !mean_host || !std_host || !out || height <= 0 || width <= 0 ||
      num_tiles < 0 || src_w <= 0 || src_h <= 0 || src_w > width || src_h > height || new_w <= 0 || new_h <= 0 || pad_w < new_w ||
      pad_h < new_h || row_stride_bytes < (long long)width * 3 || ((uintptr_t)out & 15) != 0)
    return ORP_EINVAL;
  if (num_tiles == 0) return ORP_OK;
  Norm3 nrm;
  for (int c = 0; c < 3; c++) { nrm.mean[c] = mean_host[c]; nrm.std[c] = std_host[c]; }
  const Axes ax = {x_i0, x_w1, y_i0, y_w1};
  hipStream_t st = (hipStream_t)stream;
  switch (out_dtype) {
    case 0: return launch_tiles_resized<float, kFlip>(scene, height, width, row_stride_bytes, origins, num_tiles, src_w, src_h, new_w, new_h,
                                               pad_w, pad_h, ax, nrm, to_rgb != 0, out, st);
    case 1: return launch_tiles_resized<_Float16, kFlip>(scene, height, width, row_stride_bytes, origins, num_tiles, src_w, src_h, new_w,
                                                  new_h, pad_w, pad_h, ax, nrm, to_rgb != 0, out, st);
    case 2: return launch_tiles_resized<bf16_bits, kFlip>(scene, height, width, row_stride_bytes, origins, num_tiles, src_w, src_h, new_w,
                                                   new_h, pad_w, pad_h, ax, nrm, to_rgb != 0, out, st);
    default: return ORP_EINVAL;
  }
}

}  // namespace

extern "C" {

int orp_scene_tiles(const uint8_t* scene, int height, int width, long long row_stride_bytes, const int32_t* origins,
                    int num_tiles, int tile, const float* mean_host, const float* std_host, int to_rgb, int out_dtype,
                    void* out, void* stream) {
  return scene_tiles_entry<false>(scene, height, width, row_stride_bytes, origins, num_tiles, tile, mean_host, std_host, to_rgb,
                                  out_dtype, out, stream);
}

int orp_scene_tiles_flip(const uint8_t* scene, int height, int width, long long row_stride_bytes, const int32_t* origins,
                         int num_tiles, int tile, const float* mean_host, const float* std_host, int to_rgb, int out_dtype,
                         void* out, void* stream) {
  return scene_tiles_entry<true>(scene, height, width, row_stride_bytes, origins, num_tiles, tile, mean_host, std_host, to_rgb,
                                 out_dtype, out, stream);
}

int orp_scene_tiles_resized(const uint8_t* scene, int height, int width, long long row_stride_bytes, const int32_t* origins,
                            int num_tiles, int src_w, int src_h, int new_w, int new_h, int pad_w, int pad_h, const int32_t* x_i0,
                            const float* x_w1, const int32_t* y_i0, const float* y_w1, const float* mean_host,
                            const float* std_host, int to_rgb, int out_dtype, void* out, void* stream) {
  return scene_tiles_resized_entry<false>(scene, height, width, row_stride_bytes, origins, num_tiles, src_w, src_h, new_w, new_h,
                                          pad_w, pad_h, x_i0, x_w1, y_i0, y_w1, mean_host, std_host, to_rgb, out_dtype, out, stream);
}

int orp_scene_tiles_resized_flip(const uint8_t* scene, int height, int width, long long row_stride_bytes, const int32_t* origins,
                                 int num_tiles, int src_w, int src_h, int new_w, int new_h, int pad_w, int pad_h,
                                 const int32_t* x_i0, const float* x_w1, const int32_t* y_i0, const float* y_w1,
                                 const float* mean_host, const float* std_host, int to_rgb, int out_dtype, void* out,
                                 void* stream) {
  return scene_tiles_resized_entry<true>(scene, height, width, row_stride_bytes, origins, num_tiles, src_w, src_h, new_w, new_h,
                                         pad_w, pad_h, x_i0, x_w1, y_i0, y_w1, mean_host, std_host, to_rgb, out_dtype, out, stream);
}

size_t orp_scene_collect_workspace_bytes(int num_tiles, int num_classes) {
  const size_t t = num_tiles > 0 ? (size_t)num_tiles : 1, c = num_classes > 0 ? (size_t)num_classes : 1;
  return 4 * t * c + 4 * t;
}

int orp_scene_collect(const float* packed, int num_tiles, int max_rows, const int32_t* origins, double rate, int num_classes,
                      int capacity_rows, double* dets, int32_t* seg_offsets, int32_t* src, int32_t* flag, void* workspace,
                      size_t workspace_bytes, void* stream) {
  if (!packed || !origins || !dets || !seg_offsets || !src || !flag || !workspace || num_tiles <= 0 || max_rows <= 0 ||
      num_classes <= 0 || capacity_rows < 0 || !(rate > 0.0))
    return ORP_EINVAL;
  if (num_classes > 8192 || (long long)num_tiles * max_rows > 0x7fffffffLL) return ORP_ETOOBIG;
  if (workspace_bytes < orp_scene_collect_workspace_bytes(num_tiles, num_classes)) return ORP_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int32_t* cnt = reinterpret_cast<int32_t*>(workspace);
  int32_t* tile_flag = cnt + (size_t)num_tiles * num_classes;
  const size_t lds = sizeof(int) * (size_t)num_classes;
  hipLaunchKernelGGL(collect_count_kernel, dim3(num_tiles), dim3(kCollectThreads), lds, st, packed, max_rows, num_classes, cnt,
                     tile_flag);
  hipLaunchKernelGGL(collect_scan_kernel, dim3(1), dim3(kCollectThreads), lds, st, cnt, tile_flag, num_tiles, num_classes,
                     seg_offsets, flag);
  hipLaunchKernelGGL(collect_scatter_kernel, dim3(num_tiles), dim3(kCollectThreads), lds, st, packed, max_rows, num_classes,
                     origins, rate, cnt, capacity_rows, dets, src);
  return done();
}

}  // extern "C"
