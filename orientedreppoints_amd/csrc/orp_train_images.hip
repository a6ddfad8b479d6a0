// orp_train_images.hip -- the image half of the training pipelines on the device (gfx950): the raw uint8 HWC images of a batch ->
// the padded, normalised, collated [B, 3, out_h, out_w] float32 tensor the detector trains on.
//
//   stage A  train_resize_kernel   RotateResize / PolyResize (keep_ratio, bilinear) + RandomFlip (horizontal or vertical) of every
//                                  sample in one launch, each with its own geometry.  A sample that does not rotate is finished
//                                  here (Normalize, Pad, the collate's zeros); one that rotates is written as uint8 HWC to scratch.
//   stage B  train_rotate_kernel   PolyRandomRotate's warp (cv2.warpAffine: bilinear, constant-0 border, auto_bound=False) of the
//                                  rotating samples from scratch, then Normalize, Pad and the collate's zeros.  Launched only when
//                                  a sample rotates.
//
// The resample is orp_scene_tiles_resized's arithmetic and lane mapping (orp_scene.hip): 16 bytes of every output plane per lane,
// the axis tables of a block's columns and rows in LDS, the normalisation by a 3 x 256 LDS table built from imnormalize's own
// expression.  Built with -ffp-contract=off: every product and sum below is rounded on its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orp_hip.h"

namespace {

inline int done() { hipError_t e = hipGetLastError(); return e == hipSuccess ? ORP_OK : (int)e; }

constexpr int kThreads = 256;
constexpr int kIters = 2;              // row groups per block: the table costs 768 divisions per block
constexpr int kPix = 4;                // fp32 pixels per lane and plane (16 bytes)
constexpr int kCols = 64 * kPix;       // output columns per block
constexpr int kRows = 4 * kIters;      // output rows per block

struct Norm3 { float mean[3]; float std[3]; };
struct __attribute__((aligned(16))) Vec4 { float v[kPix]; };
struct __attribute__((aligned(4))) Bytes12 { unsigned v[3]; };

typedef orp_train_image_desc Desc;

__device__ __forceinline__ void build_lut(float (*lut)[256], const Norm3& nrm) {
  for (int i = threadIdx.x; i < 768; i += kThreads) {
    const int c = i >> 8;
    lut[c][i & 255] = __fdiv_rn((float)(i & 255) - nrm.mean[c], nrm.std[c]);
  }
}

// what a pixel outside the resized image holds: Pad's value inside the sample's pad shape, the collate's 0 beyond it
__device__ __forceinline__ float outside_value(const Desc& d, int y, int x, float pad_value) {
  return ((y < d.pad_h) & (x < d.pad_w)) ? pad_value : 0.f;
}

__global__ void __launch_bounds__(kThreads)
train_resize_kernel(const unsigned char* __restrict__ images, const Desc* __restrict__ desc, const int32_t* __restrict__ axis_i0,
                    const float* __restrict__ axis_w1, Norm3 nrm, int to_rgb, int pad_first, float* __restrict__ out, int out_h,
                    int out_w, unsigned char* __restrict__ scratch) {
  __shared__ float lut[3][256];
  __shared__ __attribute__((aligned(16))) int col_i0[kCols];
  __shared__ __attribute__((aligned(16))) float col_w1[kCols];
  __shared__ int row_i0[kRows];
  __shared__ float row_w1[kRows];
  const int b = blockIdx.z;
  const Desc d = desc[b];
  const int col0 = (int)blockIdx.x * kCols, rowb = (int)blockIdx.y * kRows;
  const bool rot = d.rotate != 0;
  if (rot & ((rowb >= d.new_h) | (col0 >= d.new_w))) return;      // (block-uniform) stage B writes this sample's out
  build_lut(lut, nrm);
  for (int i = threadIdx.x; i < kCols; i += kThreads) {
    const int x = col0 + i;
    const bool in = x < d.new_w;
    const int xt = d.flip == 1 ? d.new_w - 1 - x : x;               // (in [0, new_w) whenever x is)
    col_i0[i] = in ? min(max(axis_i0[d.x_table + xt], 0), d.src_w - 1) : 0;   // (clamped: a wrong table cannot leave the image)
    col_w1[i] = in ? axis_w1[d.x_table + xt] : 0.f;
  }
  if (threadIdx.x < kRows) {
    const int y = rowb + (int)threadIdx.x;
    const bool in = y < d.new_h;
    const int yt = d.flip == 2 ? d.new_h - 1 - y : y;
    row_i0[threadIdx.x] = in ? min(max(axis_i0[d.y_table + yt], 0), d.src_h - 1) : 0;
    row_w1[threadIdx.x] = in ? axis_w1[d.y_table + yt] : 0.f;
  }
  __syncthreads();
  const int lx = (int)(threadIdx.x & 63), ly = (int)(threadIdx.x >> 6);
  const int x0 = col0 + lx * kPix;
  const size_t plane = (size_t)out_h * out_w;
  const long long src_stride = (long long)d.src_w * 3;
  const unsigned char* img = images + d.src_offset;
  const long long scr_stride = ((long long)d.new_w * 3 + 3) & ~3LL;
  float pad_value[3];
#pragma unroll
  for (int c = 0; c < 3; c++) pad_value[c] = pad_first ? lut[to_rgb ? 2 - c : c][0] : 0.f;   // c: source channel
#pragma unroll 1
  for (int it = 0; it < kIters; it++) {
    const int r = it * 4 + ly;
    const int y = rowb + r;
    if ((y >= out_h) | (x0 >= out_w)) break;           // (out_w % 4 == 0: a lane's 16 bytes are inside the row or outside it)
    unsigned byte[kPix][3];
#pragma unroll
    for (int p = 0; p < kPix; p++)
#pragma unroll
      for (int c = 0; c < 3; c++) byte[p][c] = 0u;
    const bool row_in = y < d.new_h;
    if (row_in & (x0 < d.new_w)) {
      const int ya = row_i0[r], yb = min(ya + 1, d.src_h - 1);
      const float wy1 = row_w1[r], wy0 = __fsub_rn(1.f, wy1);
      const unsigned char* top = img + (long long)ya * src_stride;
      const unsigned char* bot = img + (long long)yb * src_stride;
#pragma unroll
      for (int p = 0; p < kPix; p++) {
        if (x0 + p < d.new_w) {
          const int xa = col_i0[lx * kPix + p], xb = min(xa + 1, d.src_w - 1);
          const float wx1 = col_w1[lx * kPix + p], wx0 = __fsub_rn(1.f, wx1);
#pragma unroll
          for (int c = 0; c < 3; c++) {                // c: source channel
            const float a = (float)top[3 * xa + c], bb = (float)top[3 * xb + c];
            const float e = (float)bot[3 * xa + c], f = (float)bot[3 * xb + c];
            const float tv = __fadd_rn(__fmul_rn(wx0, a), __fmul_rn(wx1, bb));
            const float bv = __fadd_rn(__fmul_rn(wx0, e), __fmul_rn(wx1, f));
            const float v = __fadd_rn(__fmul_rn(wy0, tv), __fmul_rn(wy1, bv));
            byte[p][c] = (unsigned)(int)fminf(fmaxf(rintf(v), 0.f), 255.f);
          }
        }
      }
    }
    if (rot) {                                         // uint8 HWC into scratch, rows padded to whole dwords
      if (!row_in | (x0 >= d.new_w)) continue;
      unsigned char* dst = scratch + d.scratch_offset + (long long)y * scr_stride + (long long)x0 * 3;
      if (x0 + kPix <= d.new_w) {
        Bytes12 q;
#pragma unroll
        for (int j = 0; j < 3; j++) {
          unsigned w = 0u;
#pragma unroll
          for (int k = 0; k < 4; k++) w |= byte[(4 * j + k) / 3][(4 * j + k) % 3] << (8 * k);
          q.v[j] = w;
        }
        *reinterpret_cast<Bytes12*>(dst) = q;          // (scratch_offset, scr_stride and 3 * x0 are multiples of 4)
      } else {
#pragma unroll
        for (int p = 0; p < kPix; p++)
          if (x0 + p < d.new_w)
#pragma unroll
            for (int c = 0; c < 3; c++) dst[3 * p + c] = (unsigned char)byte[p][c];
      }
      continue;
    }
    float* o = out + (size_t)b * 3 * plane + (size_t)y * out_w + x0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const int oc = to_rgb ? 2 - c : c;
      Vec4 v;
#pragma unroll
      for (int p = 0; p < kPix; p++)
        v.v[p] = (row_in & (x0 + p < d.new_w)) ? lut[oc][byte[p][c]] : outside_value(d, y, x0 + p, pad_value[c]);
      *reinterpret_cast<Vec4*>(o + oc * plane) = v;
    }
  }
}

// Stage B.  Output pixel (x, y) of a rotating sample, in float64 with every operation rounded on its own:
//   sx = (i00*x + i01*y) + i02, sy = (i10*x + i11*y) + i12; x0 = floor(sx), fx = (float)(sx - x0); y0, fy likewise;
// then in fp32, every product and sum rounded on its own: top = (1 - fx)*a + fx*b, bot = (1 - fx)*c + fx*d,
// v = (1 - fy)*top + fy*bot with a, b, c, d the scratch bytes at (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), 0 outside
// the resized image; rint, clamp, the table.
__global__ void __launch_bounds__(kThreads)
train_rotate_kernel(const Desc* __restrict__ desc, const double* __restrict__ inv_affine, Norm3 nrm, int to_rgb, int pad_first,
                    float* __restrict__ out, int out_h, int out_w, const unsigned char* __restrict__ scratch) {
  __shared__ float lut[3][256];
  const int b = blockIdx.z;
  const Desc d = desc[b];
  if (d.rotate == 0) return;                           // (block-uniform) stage A finished this sample
  build_lut(lut, nrm);
  __syncthreads();
  const double i00 = inv_affine[6 * b], i01 = inv_affine[6 * b + 1], i02 = inv_affine[6 * b + 2];
  const double i10 = inv_affine[6 * b + 3], i11 = inv_affine[6 * b + 4], i12 = inv_affine[6 * b + 5];
  const int lx = (int)(threadIdx.x & 63), ly = (int)(threadIdx.x >> 6);
  const int x0 = (int)blockIdx.x * kCols + lx * kPix;
  const size_t plane = (size_t)out_h * out_w;
  const long long scr_stride = ((long long)d.new_w * 3 + 3) & ~3LL;
  const unsigned char* img = scratch + d.scratch_offset;
  float pad_value[3];
#pragma unroll
  for (int c = 0; c < 3; c++) pad_value[c] = pad_first ? lut[to_rgb ? 2 - c : c][0] : 0.f;
#pragma unroll 1
  for (int it = 0; it < kIters; it++) {
    const int y = (int)blockIdx.y * kRows + it * 4 + ly;
    if ((y >= out_h) | (x0 >= out_w)) break;
    unsigned byte[kPix][3];
#pragma unroll
    for (int p = 0; p < kPix; p++)
#pragma unroll
      for (int c = 0; c < 3; c++) byte[p][c] = 0u;
    const bool row_in = y < d.new_h;
    if (row_in & (x0 < d.new_w)) {
      const double yd = (double)y;
#pragma unroll
      for (int p = 0; p < kPix; p++) {
        const double xd = (double)(x0 + p);
        const double sx = (i00 * xd + i01 * yd) + i02;
        const double sy = (i10 * xd + i11 * yd) + i12;
        // a pixel with a tap inside the image: -1 < sx < new_w and -1 < sy < new_h (false for NaN); every other pixel is 0
        if ((x0 + p < d.new_w) & (sx > -1.0) & (sx < (double)d.new_w) & (sy > -1.0) & (sy < (double)d.new_h)) {
          const double fx0 = floor(sx), fy0 = floor(sy);
          const float fx = (float)(sx - fx0), fy = (float)(sy - fy0);
          const float gx = __fsub_rn(1.f, fx), gy = __fsub_rn(1.f, fy);
          const int xa = (int)fx0, ya = (int)fy0;      // in [-1, new_w - 1] and [-1, new_h - 1]
          const bool xa_in = xa >= 0, xb_in = xa + 1 < d.new_w, ya_in = ya >= 0, yb_in = ya + 1 < d.new_h;
          const unsigned char* top = img + (long long)max(ya, 0) * scr_stride;
          const unsigned char* bot = img + (long long)min(ya + 1, d.new_h - 1) * scr_stride;
          const int xl = 3 * max(xa, 0), xr = 3 * min(xa + 1, d.new_w - 1);
#pragma unroll
          for (int c = 0; c < 3; c++) {
            const float a = (ya_in & xa_in) ? (float)top[xl + c] : 0.f, bb = (ya_in & xb_in) ? (float)top[xr + c] : 0.f;
            const float e = (yb_in & xa_in) ? (float)bot[xl + c] : 0.f, f = (yb_in & xb_in) ? (float)bot[xr + c] : 0.f;
            const float tv = __fadd_rn(__fmul_rn(gx, a), __fmul_rn(fx, bb));
            const float bv = __fadd_rn(__fmul_rn(gx, e), __fmul_rn(fx, f));
            const float v = __fadd_rn(__fmul_rn(gy, tv), __fmul_rn(fy, bv));
            byte[p][c] = (unsigned)(int)fminf(fmaxf(rintf(v), 0.f), 255.f);
          }
        }
      }
    }
    float* o = out + (size_t)b * 3 * plane + (size_t)y * out_w + x0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const int oc = to_rgb ? 2 - c : c;
      Vec4 v;
#pragma unroll
      for (int p = 0; p < kPix; p++)
        v.v[p] = (row_in & (x0 + p < d.new_w)) ? lut[oc][byte[p][c]] : outside_value(d, y, x0 + p, pad_value[c]);
      *reinterpret_cast<Vec4*>(o + oc * plane) = v;
    }
  }
}

inline size_t scratch_image_bytes(int new_w, int new_h) {
  if (new_w <= 0 || new_h <= 0) return 0;
  const size_t stride = ((size_t)new_w * 3 + 3) & ~(size_t)3;
  return (stride * (size_t)new_h + 255) & ~(size_t)255;
}

}  // namespace

extern "C" {

size_t orp_train_images_scratch_bytes(int new_w, int new_h) { return scratch_image_bytes(new_w, new_h); }

int orp_train_images(const uint8_t* images, size_t images_bytes, const orp_train_image_desc* desc_host,
                     const orp_train_image_desc* desc, int num_images, const double* inv_affine, const int32_t* axis_i0,
                     const float* axis_w1, int axis_len, const float* mean_host, const float* std_host, int to_rgb,
                     int pad_before_normalize, float* out, int out_h, int out_w, void* scratch, size_t scratch_bytes,
                     void* stream) {
  if (!images || !desc_host || !desc || !inv_affine || !axis_i0 || !axis_w1 || !mean_host || !std_host || !out || num_images < 0 ||
      num_images > 65535 || out_h <= 0 || out_w <= 0 || out_w % kPix != 0 || axis_len < 0 || ((uintptr_t)out & 15) != 0)
    return ORP_EINVAL;
  bool any_rotate = false;
  for (int b = 0; b < num_images; b++) {
    const orp_train_image_desc& d = desc_host[b];
    if (d.src_h <= 0 || d.src_w <= 0 || d.new_h <= 0 || d.new_w <= 0 || d.pad_h < d.new_h || d.pad_w < d.new_w || d.pad_h > out_h ||
        d.pad_w > out_w || d.flip < 0 || d.flip > 2 || d.src_offset < 0 ||
        (unsigned long long)d.src_offset + 3ull * (unsigned long long)d.src_h * (unsigned long long)d.src_w > images_bytes ||
        d.x_table < 0 || (long long)d.x_table + d.new_w > axis_len || d.y_table < 0 || (long long)d.y_table + d.new_h > axis_len)
      return ORP_EINVAL;
    if (d.rotate) {
      any_rotate = true;
      if (!scratch || d.scratch_offset < 0 || (d.scratch_offset & 3) != 0 || ((uintptr_t)scratch & 3) != 0 ||
          (unsigned long long)d.scratch_offset + scratch_image_bytes(d.new_w, d.new_h) > scratch_bytes)
        return ORP_EINVAL;
    }
  }
  if (num_images == 0) return ORP_OK;
  const int bx = (out_w + kCols - 1) / kCols, by = (out_h + kRows - 1) / kRows;
  if (by > 65535) return ORP_ETOOBIG;
  Norm3 nrm;
  for (int c = 0; c < 3; c++) { nrm.mean[c] = mean_host[c]; nrm.std[c] = std_host[c]; }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)bx, (unsigned)by, (unsigned)num_images);
  hipLaunchKernelGGL(train_resize_kernel, grid, dim3(kThreads), 0, st, images, desc, axis_i0, axis_w1, nrm, to_rgb != 0,
                     pad_before_normalize != 0, out, out_h, out_w, reinterpret_cast<unsigned char*>(scratch));
  if (any_rotate)
    hipLaunchKernelGGL(train_rotate_kernel, grid, dim3(kThreads), 0, st, desc, inv_affine, nrm, to_rgb != 0,
                       pad_before_normalize != 0, out, out_h, out_w, reinterpret_cast<const unsigned char*>(scratch));
  return done();
}

}  // extern "C"
