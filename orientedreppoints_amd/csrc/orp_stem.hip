// orp_stem.hip -- the ResNet stem as ONE launch (gfx950, inference only):
//   y = maxpool3x3/s2/p1( relu( conv7x7/s2/p3(x, w) * a[c] + b[c] ) ),   x [B,3,H,W] fp32 NCHW  ->  y [B,64,Hp,Wp] fp32 NCHW,
//   Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1 (the conv MAP), Hp = (Ho - 1) / 2 + 1, Wp = (Wo - 1) / 2 + 1.
// It replaces the library's 7x7 convolution (which writes a 67 MB raw map at 1024^2) and affine_relu_maxpool_kernel (orp_norm.hip,
// which reads it back): the raw map never leaves the CU.  Arithmetic: exact fp32 MFMA (v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain),
// no operand is split, one accumulator per output, one fixed order, so an output does not depend on its tile or on the batch size.
//
// Tile.  A workgroup (four waves) owns PH x PW = 4 x 16 pooled outputs of one image = the TR x TC = 9 x 33 conv outputs
//   rows 2 ph0 - 1 .. 2 ph0 + 7, columns 2 pw0 - 1 .. 2 pw0 + 31 (the one-pixel pooling halo is recomputed), whose input patch is
//   PR x PC = 23 x 71 pixels x 3 channels, staged in LDS once with its columns de-interleaved by parity:
//     patch[c][row][parity][36], patch column pc -> parity pc & 1, slot pc >> 1
//   so the 32 consecutive conv columns of an MFMA column block read consecutive dwords for every kx.  Pixels outside the image are
//   zeros in LDS.
// K order (the ONE order of this file): k = c * 49 + ky * 7 + kx, k = 0 .. 146, i.e. the weight tensor's own memory order, padded by
//   ONE tap k = 147 to 74 MFMA steps of two; step s contracts k = 2 s (lanes 0..31) and k = 2 s + 1 (lanes 32..63).  The padding tap
//   has a zero weight AND reads a dedicated zero word of LDS (kZeroSlot), never a pixel: 0 x Inf would poison the output.
// Contraction.  D[channel][position]: output channels are the MFMA rows (two blocks of 32), the 297 positions of the conv tile,
//   linearised row-major and padded to 320, the columns (ten blocks of 32).  Wave w owns channel block w & 1 and the five column
//   blocks 5 (w >> 1) .. + 4: its 74 weight words (one per lane and step, packed by orp_stem_pack_weight) live in registers for the
//   whole tile and each step is one 4-byte LDS read per column block and five independent MFMAs.
// Epilogue (pool = 1).  relu(acc * a[c] + b[c]) -- affine_act of orp_affine.hpp, one fma, then fmaxf(., 0) -- goes to LDS as the conv
//   tile [64][297] (it reuses the patch's space); conv positions outside the MAP are +0 there exactly as in affine_relu_maxpool_kernel,
//   i.e. they take no part (every window holds a real position and relu(.) >= +0), and the 3x3 / stride 2 maxima are taken in that
//   kernel's order (three rows per column, then three columns).  Non-finite values: as there (fmaxf(NaN, 0) = 0, +Inf stays).
// Raw mode (pool = 0): the same staging and K loop; the accumulators of the tile's OWN 8 x 32 conv positions go to y [B,64,Ho,Wo]
//   as they are (no BatchNorm), so that contraction and epilogue can be tested apart.
// Resources: 76 032 B of LDS and at most 256 registers per lane, so two workgroups share a CU (one stages while the other multiplies);
//   no atomics, no split-K, no scratch (tests/test_stem_host.py compiles this file and checks).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orp_hip.h"
#include "orp_affine.hpp"

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int kCin = 3, kCout = 64, kK = 7, kTaps = kCin * kK * kK;   // 147
constexpr int kSteps = (kTaps + 1) / 2;                                // 74 MFMA steps of two taps
constexpr int PH = 4, PW = 16;                                         // pooled outputs per tile
constexpr int TR = 2 * PH + 1, TC = 2 * PW + 1, kPos = TR * TC;        // conv tile 9 x 33 = 297 positions
constexpr int kBlocks = 10, kBlocksPerWave = 5;                        // column blocks of 32 positions (320 >= 297)
constexpr int PR = 2 * (TR - 1) + kK, PC = 2 * (TC - 1) + kK;          // input patch 23 x 71
constexpr int kHalf = 36, kRowStride = 2 * kHalf;                      // one patch row: 36 even + 36 odd columns
constexpr int kChanStride = PR * kRowStride;                           // 1656
constexpr int kZeroSlot = kCin * kChanStride;                          // the word the padding tap reads
constexpr int kPatchFloats = kZeroSlot + 1;
constexpr int kTileFloats = kCout * kPos;                              // the conv tile of the epilogue (over the patch)
constexpr int kLdsFloats = kTileFloats > kPatchFloats ? kTileFloats : kPatchFloats;
constexpr int kThreads = 256;
constexpr int kPatchElems = kCin * PR * kRowStride;                    // 4968 words staged per tile
constexpr int kStageIters = (kPatchElems + kThreads - 1) / kThreads;   // 20 per thread
static_assert(kBlocks * 32 >= kPos && kBlocks == 2 * kBlocksPerWave, "column blocks cover the conv tile");
static_assert((PC + 1) / 2 <= kHalf, "patch row fits its slots");
static_assert(kLdsFloats * 4 * 2 <= 163840, "two workgroups per CU");
static_assert(kStageIters * kThreads + 1 <= kLdsFloats, "the staging rounds' overhang stays inside the LDS array");

// patch offset of tap k relative to a position's base (2 r) * kRowStride + j
__host__ __device__ constexpr int tap_offset(int k) {
  return k >= kTaps ? 0 : (k / 49) * kChanStride + ((k % 49) / 7) * kRowStride + ((k % 7) & 1) * kHalf + ((k % 7) >> 1);
}

struct Args {
  const float* x; const float* wp; const float* scale; const float* shift; float* y;
  int H, W, Ho, Wo, Hp, Wp;
};

template <bool kPool>
__global__ void __launch_bounds__(kThreads, 2)
stem_kernel(const Args A) {
  __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 31, kh = lane >> 5;
  const int cb = wave & 1, b0 = (wave >> 1) * kBlocksPerWave;
  const int ph0 = blockIdx.y * PH, pw0 = blockIdx.x * PW, img = blockIdx.z;
  const int oy0 = 2 * ph0 - 1, ox0 = 2 * pw0 - 1;                       // conv coordinates of tile position (0, 0)
  const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;                       // image coordinates of patch element (0, 0)

  // the patch: element e = (channel * PR + row) * kRowStride + pc; pc == PC is the unused 72nd slot, written as zero.  All of a
  // thread's loads are issued before the first is waited for (one memory latency per tile, not one per element), in front of the
  // weights' so that the LDS writes go out while those are still in flight.
  float px[kStageIters];
  const auto patch_elem = [&](int i, int& cr, int& pc, int& c, int& iy, int& ix) {
    const int e = tid + i * kThreads;
    cr = e / kRowStride; pc = e - cr * kRowStride;
    c = cr / PR;
    iy = iy0 + cr - c * PR; ix = ix0 + pc;
  };
  {
    const float* xi = A.x + (size_t)img * kCin * A.H * A.W;
    const size_t HW = (size_t)A.H * A.W;
#pragma unroll
    for (int i = 0; i < kStageIters; i++) {
      int cr, pc, c, iy, ix;
      patch_elem(i, cr, pc, c, iy, ix);
      // an unconditional load of a clamped (always valid) address, the select comes later: no branch, no wait between the loads
      const int cc = min(c, kCin - 1), cy = min(max(iy, 0), A.H - 1), cx = min(max(ix, 0), A.W - 1);
      px[i] = xi[cc * HW + (size_t)cy * A.W + cx];
    }
  }
  // this lane's weights: packed [channel block][step][lane]
  float w[kSteps];
  {
    const float* wq = A.wp + (size_t)cb * kSteps * 64 + lane;
#pragma unroll
    for (int s = 0; s < kSteps; s++) w[s] = wq[s * 64];
  }
#pragma unroll
  for (int i = 0; i < kStageIters; i++) {
    int cr, pc, c, iy, ix;
    patch_elem(i, cr, pc, c, iy, ix);
    const bool in = (pc < PC) & (iy >= 0) & (iy < A.H) & (ix >= 0) & (ix < A.W);
    // the last round's elements past the patch go to unused words behind the zero word (the conv tile's space)
    const int e = tid + i * kThreads;
    const int idx = e < kPatchElems ? cr * kRowStride + (pc & 1) * kHalf + (pc >> 1) : e + 1;
    lds[idx] = in ? px[i] : 0.f;
  }
  if (tid == 0) lds[kZeroSlot] = 0.f;
  // position p = 32 b + n of the conv tile -> (r, j); p >= kPos (the padding of the last block) computes position 0 and is dropped
  int base[kBlocksPerWave];
#pragma unroll
  for (int i = 0; i < kBlocksPerWave; i++) {
    int p = (b0 + i) * 32 + n;
    p = p < kPos ? p : 0;
    const int r = p / TC, j = p - r * TC;
    base[i] = 2 * r * kRowStride + j;
  }
  __syncthreads();

  floatx16 acc[kBlocksPerWave];
#pragma unroll
  for (int i = 0; i < kBlocksPerWave; i++) acc[i] = floatx16{0};
#pragma unroll
  for (int s = 0; s < kSteps; s++) {
    const int off = kh ? tap_offset(2 * s + 1) : tap_offset(2 * s);
    float a[kBlocksPerWave];
#pragma unroll
    for (int i = 0; i < kBlocksPerWave; i++) {
      int idx = base[i] + off;
      if (2 * s + 1 >= kTaps) idx = kh ? kZeroSlot : idx;               // the padding tap reads the zero word
      a[i] = lds[idx];
    }
#pragma unroll
    for (int i = 0; i < kBlocksPerWave; i++) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[s], a[i], acc[i], 0, 0, 0);
  }

  // accumulator register q of a lane: channel cb * 32 + (q & 3) + 8 (q >> 2) + 4 kh, position 32 b + n
  if (!kPool) {
#pragma unroll
    for (int i = 0; i < kBlocksPerWave; i++) {
      const int p = (b0 + i) * 32 + n;
      const int r = p / TC, j = p - r * TC;
      const int oy = oy0 + r, ox = ox0 + j;
      // the tile's own positions (rows / columns 1 ..: row / column 0 belongs to the neighbour) inside the map
      if ((p < kPos) & (r >= 1) & (j >= 1) & (oy < A.Ho) & (ox < A.Wo)) {
        float* dst = A.y + ((size_t)img * kCout + cb * 32 + 4 * kh) * A.Ho * A.Wo + (size_t)oy * A.Wo + ox;
#pragma unroll
        for (int q = 0; q < 16; q++) dst[(size_t)((q & 3) + 8 * (q >> 2)) * A.Ho * A.Wo] = acc[i][q];
      }
    }
    return;
  }

  float sa[16], sb[16];
#pragma unroll
  for (int q = 0; q < 16; q++) {
    const int ch = cb * 32 + (q & 3) + 8 * (q >> 2) + 4 * kh;
    sa[q] = A.scale[ch]; sb[q] = A.shift[ch];
  }
  __syncthreads();                                                      // every wave has read its last patch word
#pragma unroll
  for (int i = 0; i < kBlocksPerWave; i++) {
    const int p = (b0 + i) * 32 + n;
    const int r = p / TC, j = p - r * TC;
    const int oy = oy0 + r, ox = ox0 + j;
    const bool in = (oy >= 0) & (oy < A.Ho) & (ox >= 0) & (ox < A.Wo);
    if (p < kPos) {
#pragma unroll
      for (int q = 0; q < 16; q++) {
        const int ch = cb * 32 + (q & 3) + 8 * (q >> 2) + 4 * kh;
        lds[ch * kPos + p] = in ? affine_act(acc[i][q], sa[q], sb[q], 1) : 0.f;
      }
    }
  }
  __syncthreads();
  // pooled output (ch, ph, pw): thread -> pw = tid & 15, (ch, ph) = (tid >> 4) + 16 it
  const int pw = tid & (PW - 1);
  const bool col_in = pw0 + pw < A.Wp;
#pragma unroll 4
  for (int it = 0; it < kCout * PH / (kThreads / PW); it++) {
    const int cp = (tid >> 4) + (kThreads / PW) * it;
    const int ch = cp >> 2, ph = cp & (PH - 1);
    if (col_in & (ph0 + ph < A.Hp)) {
      const float* t = lds + ch * kPos + 2 * ph * TC + 2 * pw;
      float m[3];
#pragma unroll
      for (int u = 0; u < 3; u++) m[u] = fmaxf(fmaxf(t[u], t[TC + u]), t[2 * TC + u]);
      A.y[(((size_t)img * kCout + ch) * A.Hp + ph0 + ph) * A.Wp + pw0 + pw] = fmaxf(fmaxf(m[0], m[1]), m[2]);
    }
  }
}

// packed[(cb * kSteps + s) * 64 + lane] = w[cb * 32 + (lane & 31)][k = 2 s + (lane >> 5)], zero for the padding tap k = 147
__global__ void stem_pack_kernel(const float* __restrict__ w, float* __restrict__ packed) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * kSteps * 64) return;
  const int lane = i & 63, s = (i >> 6) % kSteps, cb = (i >> 6) / kSteps;
  const int k = 2 * s + (lane >> 5), ch = cb * 32 + (lane & 31);
  packed[i] = k < kTaps ? w[ch * kTaps + k] : 0.f;
}

}  // namespace

extern "C" {

int orp_stem_ok(int c_in, int c_out, int kernel, int stride, int padding) {
  return (c_in == kCin && c_out == kCout && kernel == kK && stride == 2 && padding == 3) ? 1 : 0;
}

size_t orp_stem_packed_bytes(int c_in, int c_out) {
  return (c_in == kCin && c_out == kCout) ? sizeof(float) * 2 * kSteps * 64 : 0;
}

int orp_stem_pack_weight(const float* weight, int c_in, int c_out, void* packed, void* stream) {
  if (!weight || !packed || ((uintptr_t)packed & 3) || !orp_stem_packed_bytes(c_in, c_out)) return ORP_EINVAL;
  hipLaunchKernelGGL(stem_pack_kernel, dim3((2 * kSteps * 64 + 255) / 256), dim3(256), 0, (hipStream_t)stream, weight,
                     reinterpret_cast<float*>(packed));
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ORP_OK : (int)e;
}

// THE routing rule of this launch: where it was measured faster than library convolution + orp_affine_relu_maxpool on MI355X, slowest
// new run against the fastest library run (tests/checks/time_stem.py; docs/notebook/round25.md has the tables).  A closed table of
// (IMAGE side, images) filled from timed corners only: both sides inside [side_min, side_max].
int orp_stem_pays(int height, int width, int batch) {
  if (height <= 0 || width <= 0 || batch <= 0) return 0;
  static const struct { int side_min, side_max, batch; } paid[] = {
      {1024, 1536, 1}, {1024, 1024, 2},
  };
  for (const auto& s : paid)
    if (s.batch == batch && height >= s.side_min && height <= s.side_max && width >= s.side_min && width <= s.side_max) return 1;
  return 0;
}

int orp_stem_conv_bn_relu_pool(const float* x, const void* weight_packed, const float* scale, const float* shift, float* y, int batch,
                               int c_in, int c_out, int height, int width, int kernel, int stride, int padding, int pool, void* stream) {
  if (!x || !weight_packed || ((uintptr_t)weight_packed & 3) || !y || (const float*)y == x || batch <= 0 || height <= 0 || width <= 0 ||
      !orp_stem_ok(c_in, c_out, kernel, stride, padding) || (pool != 0 && pool != 1) || (pool && (!scale || !shift)))
    return ORP_EINVAL;
  if (batch > 65535 || (long)height * width >= (1L << 31)) return ORP_ETOOBIG;
  Args A;
  A.x = x; A.wp = reinterpret_cast<const float*>(weight_packed); A.scale = scale; A.shift = shift; A.y = y;
  A.H = height; A.W = width;
  A.Ho = (height - 1) / 2 + 1; A.Wo = (width - 1) / 2 + 1;             // (H + 6 - 7) / 2 + 1
  A.Hp = (A.Ho - 1) / 2 + 1; A.Wp = (A.Wo - 1) / 2 + 1;                 // (Ho + 2 - 3) / 2 + 1, floor mode
  const int tx = (A.Wp + PW - 1) / PW, ty = (A.Hp + PH - 1) / PH;
  if (ty > 65535) return ORP_ETOOBIG;
  const dim3 grid(tx, ty, batch);
  if (pool)
    hipLaunchKernelGGL(stem_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, A);
  else
    hipLaunchKernelGGL(stem_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, A);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ORP_OK : (int)e;
}

}  // extern "C"
