// orp_conv3x3_bn_s2.hip -- the stride-2 3x3 / padding 1 convolution of the first bottleneck of ResNet stages 2 and 3 (conv2, 128 -> 128
// and 256 -> 256 channels), with its eval-mode BatchNorm and ReLU in the epilogue, in the fp16-pieces arithmetic (gfx950, inference):
//
//   y = relu?( fma(conv3x3(x, w), a[c], b[c]) ),   x, y NCHW fp32, Cin = Cout in {128, 256}, stride 2
//
// The arithmetic is conv3x3_bn_act_kernel's (orp_conv3x3_bn.hip), nothing new numerically: one power-of-two scale from the launch's
// range word (orp_range.hpp), two fp16 planes per operand, lo * hi and hi * lo into a side accumulator, hi * hi into the main one, one
// range_unscale, then orp_affine.hpp's affine_act; padding is zero after the scale; the weights are pack_planes16's
// [pl][tap][C/16][2][C][8] planes.
//
// The layout is conv3x3_bn_deep_kernel<2, 2>'s (orp_conv3x3_bn_deep.hip) with NARROW staging passes, so that two workgroups fit a CU and
// one stages while the other multiplies (that kernel's 128-channel pass is 89 760 B, one workgroup per CU, its staging not overlapped
// with anything):
//   * a workgroup is one 2 x 16 output tile x 128 output channels: eight waves = 4 output-channel groups of 32 x 2 K groups; K group g
//     contracts input channels [g C / 2, (g + 1) C / 2).  The grid is tiles x C / 128, a tile's channel groups neighbours in it.
//   * the 5 x 33 halo is staged in C / 64 passes of 64 channels, 32 from each K group's half, side by side: two fp16 planes
//     [halo pixel][64 + 8] = 47 520 B.  A barrier pair per pass, nine phases per pass (one per tap, two 16-channel chunks each).  Halo
//     columns are stored de-interleaved by parity, column (hx & 1) * 17 + (hx >> 1): the 16 lanes of a ds_read_b128 group (consecutive
//     output columns) read rows ONE pixel apart, 36 dwords, which lands them on the 64 banks once each.  Tap (ki, kj) reads parity
//     plane kj & 1 at column tx + (kj >> 1) of halo row 2 ty + ki.  Tile columns are rotated by two per tile row.
//   * the weight ring (one phase deep, refilled in place behind its use) and the one-chunk A read-ahead are the existing kernels'; the
//     ring's loads for the next pass are in flight across that pass's staging.
//   * the kernel is held to 128 registers (four waves per SIMD), so that LDS and registers both admit two workgroups per CU.
//
// THE order of accumulation of an output (channel o, position p), fixed: K group g in {0, 1} runs passes 0 .. C / 64 - 1; in pass s taps
// 0 .. 8 (row-major); in a tap the chunks j = 0, 1 of input channels g C / 2 + 32 s + 16 j .. + 16; a chunk is three MFMAs (32x32x16
// f16): side += w_hi x_lo, side += w_lo x_hi, acc += w_hi x_hi.  Then t = (acc_0 + side_0) + (acc_1 + side_1), K group 1's sum handed
// over through LDS; range_unscale(t); affine_act.  No atomics; the same at every tile, grid, batch and map size.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orp_hip.h"
#include "orp_affine.hpp"
#include "orp_range.hpp"
#include "orp_conv3x3_bn_host.hpp"

namespace {

using namespace orp_conv3x3;       // floatx16 / h8 / h2, kThreads and the host helpers

constexpr int TH = 2, TW = 16;     // output tile: one 32-position MFMA block
constexpr int KS = 2;              // K groups of a workgroup
constexpr int WN = 8 / KS;         // waves over output channels
constexpr int CG = 32 * WN;        // output channels of a workgroup
constexpr int CST = 64;            // channels staged per pass: SH of each K group
constexpr int SH = CST / KS;
constexpr int NCH = SH / 16;       // 16-channel chunks per phase: a phase is one tap of a pass
constexpr int PPH = 9;             // phases per pass
constexpr int HROWS = (TH - 1) * 2 + 3, HCOLS = (TW - 1) * 2 + 3;   // 5 x 33
constexpr int ROWS = HROWS * HCOLS;                                 // halo pixels
constexpr int ASTR = CST + 8;      // halves per halo pixel
constexpr int PLANE = ROWS * ASTR;
constexpr size_t kSmem = (size_t)2 * PLANE * 2;
static_assert(kSmem == 47520 && 2 * kSmem <= 163840, "two workgroups per CU");
static_assert(kSmem >= (size_t)(KS - 1) * WN * 16 * 64 * sizeof(float), "the reduction reuses the halo's area");

// halo pixel (hy, hx) -> its LDS row
__device__ __forceinline__ constexpr int halo_row(int hy, int hx) { return hy * HCOLS + (hx & 1) * 17 + (hx >> 1); }

struct Args {
  const float* x;                  // [B][C][H][W]
  const uint16_t* planes;          // two fp16 planes [pl][tap][C/16][2][C][8]
  size_t plane_stride;
  const float* wscale;             // device scalar: the planes' power-of-two scale
  const unsigned* range;           // device scalar: bits of (a bound of) max |x|
  const float* scale; const float* shift;   // [C]
  float* y;                        // [B][C][Ho][Wo]
  int H, W, Ho, Wo, relu, tiles_x, tiles_per_image;
};

template <int C>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
conv3x3_bn_s2_kernel(const Args P) {
  constexpr int KH = C / KS, NPASS = C / CST;
  static_assert(C % CG == 0 && KH % SH == 0, "whole channel groups and passes");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t* sA = reinterpret_cast<uint16_t*>(smem);        // [2 planes][ROWS][CST + 8]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cgrp = blockIdx.x % (C / CG), tile = blockIdx.x / (C / CG);
  const int img = tile / P.tiles_per_image, tt = tile - img * P.tiles_per_image;
  const int trow = tt / P.tiles_x;
  const int y0 = trow * TH, x0 = (tt - trow * P.tiles_x) * TW;
  const int H = P.H, W = P.W;
  const size_t hw = (size_t)H * W;

  const int kx = orp::range_exp(*P.range);
  const float sx = orp::range_scale(kx);
  const int kxw = kx + orp::range_exp_of(*P.wscale);

  // ---- weight fragments: lane (output channel n_wave + lane % 32, k-group lane / 32) reads the 8 k-values of a chunk per plane ----
  const int wn = wave % WN, g = wave / WN;
  const int n_wave = cgrp * CG + wn * 32;
  const int mrow = lane & 31, kg = lane >> 5;
  const uint16_t* wp = P.planes + ((size_t)kg * C + n_wave + mrow) * 8;
  constexpr size_t wblk = (size_t)2 * C * 8;
  // phase q of the launch = pass * 9 + tap; its chunk j is 16-channel block (g * KH + pass * SH) / 16 + j of tap's C / 16
  auto load_b = [&](int q, int j, h8 (&b)[2]) {
    const int pass = q / PPH, tap = q - pass * PPH;
    const uint16_t* a = wp + (size_t)(tap * (C / 16) + (g * KH + pass * SH) / 16 + j) * wblk;
#pragma unroll
    for (int pl = 0; pl < 2; pl++) b[pl] = *reinterpret_cast<const h8*>(a + (size_t)pl * P.plane_stride);
  };
  h8 bq[NCH][2];
#pragma unroll
  for (int j = 0; j < NCH; j++) load_b(0, j, bq[j]);
  __builtin_amdgcn_sched_barrier(0);                       // (the weights go out first: see conv_halo_kernel's prologue)

  // ---- A fragments: lane (position m = lane % 32 of the tile, k-group) reads 16 B of its halo row per plane ----
  const int ty = mrow >> 4, tx = (mrow - 2 * ty) & 15;     // (columns rotated by two per tile row: conv3x3_bn_act_kernel)
  const uint16_t* abase = sA + (size_t)halo_row(2 * ty, 0) * ASTR + (size_t)tx * ASTR + g * SH + 8 * kg;
  auto a_off = [&](int tap) {
    const int ki = tap / 3, kj = tap - 3 * ki;
    return halo_row(ki, kj) * ASTR;
  };
  auto load_a = [&](int off, int j, h8 (&a)[2]) {
#pragma unroll
    for (int pl = 0; pl < 2; pl++) a[pl] = *reinterpret_cast<const h8*>(abase + pl * PLANE + off + j * 16);
  };

  floatx16 acc = floatx16{0}, side = floatx16{0};
  constexpr int nphase = NPASS * PPH;

#pragma unroll 1
  for (int pass = 0; pass < NPASS; pass++) {
    if (pass > 0) __syncthreads();                         // (every wave has read the pass before)
    // ---- staging: a wave-instruction = 16 halo pixels x 4 channel pairs; the eight waves cover the pass's 64 channels of the 16
    // pixels.  The loads of a pass go out in two batches (the register budget of four waves per SIMD) from clamped addresses, every one
    // unconditional (conv3x3_bn_act_kernel); LDS channel l holds channel (l / SH) * KH + pass * SH + l % SH: the K groups' shares side by side
    {
      const int px = lane & 15, cq = lane >> 4;
      const int l = (wave * 4 + cq) * 2;
      const float* xb = P.x + ((size_t)img * C + (size_t)((l / SH) * KH + pass * SH + l % SH)) * hw;
      constexpr int G = (ROWS + 15) / 16, GB = (G + 1) / 2;
#pragma unroll
      for (int g0 = 0; g0 < G; g0 += GB) {
        float v[GB][2];
        bool in[GB];
#pragma unroll
        for (int gi = 0; gi < GB; gi++) {
          const int h = (g0 + gi) * 16 + px;
          const int hy = h / HCOLS, hx = h - hy * HCOLS;
          const int yy = 2 * y0 - 1 + hy, xx = 2 * x0 - 1 + hx;
          in[gi] = h < ROWS && yy >= 0 && yy < H && xx >= 0 && xx < W;
          const float* src = xb + (in[gi] ? (size_t)yy * W + xx : (size_t)0);
          v[gi][0] = src[0];
          v[gi][1] = src[hw];
        }
#pragma unroll
        for (int gi = 0; gi < GB; gi++) { asm volatile("" : "+v"(v[gi][0])); asm volatile("" : "+v"(v[gi][1])); }
#pragma unroll
        for (int gi = 0; gi < GB; gi++) {
          const int h = (g0 + gi) * 16 + px;
          const int hy = h / HCOLS, hx = h - hy * HCOLS;
          const float s0 = in[gi] ? v[gi][0] * sx : 0.f, s1 = in[gi] ? v[gi][1] * sx : 0.f;   // (padding is zero AFTER the scale)
          h2 hh, ll;
          orp::range_split(s0, hh, ll, 0);
          orp::range_split(s1, hh, ll, 1);
          if (h < ROWS) {
            uint16_t* dst = sA + (size_t)halo_row(hy, hx) * ASTR + l;
            *reinterpret_cast<unsigned*>(dst) = __builtin_bit_cast(unsigned, hh);
            *reinterpret_cast<unsigned*>(dst + PLANE) = __builtin_bit_cast(unsigned, ll);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();

    h8 a[2][2];
    load_a(a_off(0), 0, a[0]);
    // one phase: the A fragment of the next chunk -- of the next phase's first chunk behind the last one -- is read before the MFMAs of
    // this one are issued; a chunk's weight registers are refilled for the next phase (of the next pass behind a pass's last one) right
    // after use (the last phase re-reads its own: every load of the loop is unconditional, so the compiler's vmcnt counts are exact)
#pragma unroll 1
    for (int ph = 0; ph < PPH; ph++) {
      const int q = pass * PPH + ph;
      const int q_n = q + 1 < nphase ? q + 1 : q;
      const int off = a_off(ph), off_n = a_off(ph + 1 < PPH ? ph + 1 : ph);
#pragma unroll
      for (int j = 0; j < NCH; j++) {
        if (j + 1 < NCH) load_a(off, j + 1, a[(j + 1) & 1]);
        else             load_a(off_n, 0, a[0]);
        __builtin_amdgcn_sched_barrier(0);
        // D[channel][position]: lo * hi and hi * lo into the side accumulator, hi * hi into the main one (conv_halo_kernel's order)
        side = __builtin_amdgcn_mfma_f32_32x32x16_f16(bq[j][0], a[j & 1][1], side, 0, 0, 0);
        side = __builtin_amdgcn_mfma_f32_32x32x16_f16(bq[j][1], a[j & 1][0], side, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(bq[j][0], a[j & 1][0], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        load_b(q_n, j, bq[j]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // ---- the K groups meet: group 1 leaves acc + side in the halo's area, group 0 adds it to its own ----
  float* red = reinterpret_cast<float*>(smem) + (size_t)wn * 16 * 64 + lane;   // [wn][r][lane]
  __syncthreads();                                         // (every wave has read the halo)
  if (g > 0) {
#pragma unroll
    for (int r = 0; r < 16; r++) red[r * 64] = acc[r] + side[r];
  }
  __syncthreads();
  if (g > 0) return;

  // ---- epilogue: un-scale, BatchNorm as one fma, ReLU last; register r of a lane is channel n_wave + (r & 3) + 8 (r >> 2) + 4 kg ----
  const int yy = y0 + ty, xx = x0 + tx;
  if (yy < P.Ho && xx < P.Wo) {
    const size_t hwo = (size_t)P.Ho * P.Wo;
    float* o = P.y + (size_t)img * C * hwo + (size_t)yy * P.Wo + xx;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int ch = n_wave + (r & 3) + 8 * (r >> 2) + 4 * kg;
      const float t = (acc[r] + side[r]) + red[r * 64];
      const float v = orp::range_unscale(t, kxw);
      o[(size_t)ch * hwo] = affine_act(v, P.scale[ch], P.shift[ch], P.relu);
    }
  }
}

template <int C>
hipError_t launch(const Args& A, long tiles, hipStream_t st) {
  struct Tag {};
  return launch_with_lds<Tag>(&conv3x3_bn_s2_kernel<C>, tiles * (C / CG), kSmem, st, A);
}

}  // namespace

extern "C" {

int orp_conv3x3_bn_s2_ok(int c_in, int c_out) {
  return (c_in == c_out && (c_in == 128 || c_in == 256)) ? 1 : 0;
}

size_t orp_conv3x3_bn_s2_packed_bytes(int c_in, int c_out) { return packed_bytes(orp_conv3x3_bn_s2_ok(c_in, c_out), c_in, c_out); }

int orp_conv3x3_bn_s2_pack_weight(const float* weight, int c_in, int c_out, void* packed, void* stream) {
  return pack_weight(orp_conv3x3_bn_s2_ok(c_in, c_out), weight, c_in, c_out, packed, stream);
}

// THE routing rule of this launch: where it was measured faster than library convolution + pass on MI355X, slowest new run plus what
// the range word costs conv1 against the fastest library run (tests/checks/time_bottleneck_3x3.py --kernel s2; docs/notebook/round24.md
// has the tables).  A closed table of (channels, INPUT map side, images) filled from timed corners only: square maps, both sides inside
// [side_min, side_max].
int orp_conv3x3_bn_s2_pays(int c_in, int c_out, int height, int width, int batch) {
  if (!orp_conv3x3_bn_s2_ok(c_in, c_out) || height <= 0 || width <= 0 || batch <= 0) return 0;
  static const PaidSquare rows[] = {
      {128, 256, 384, 1}, {128, 256, 256, 2},                // stage 2 block 0: the 1024^2 image's map to the 1536^2 image's; two images
      {256, 128, 192, 1}, {256, 128, 128, 2},                // stage 3 block 0
  };
  return paid(rows, c_in, height, width, batch);
}

int orp_conv3x3_bn_s2(const float* x, const void* weight_packed, const float* scale, const float* shift, const uint32_t* range_in,
                      float* y, int batch, int c_in, int c_out, int height, int width, int relu, void* stream) {
  if (bad_launch_args(x, weight_packed, scale, shift, range_in, y, batch, height, width) || !orp_conv3x3_bn_s2_ok(c_in, c_out))
    return ORP_EINVAL;
  Args A;
  fill_common(A, x, weight_packed, scale, shift, range_in, y, c_in, c_out, height, width, relu);
  A.Ho = (height - 1) / 2 + 1; A.Wo = (width - 1) / 2 + 1;
  A.tiles_x = (A.Wo + TW - 1) / TW;
  const long tpi = (long)A.tiles_x * ((A.Ho + TH - 1) / TH);
  if (tpi * batch * 2 >= (1L << 31) || (long)height * width >= (1L << 31)) return ORP_ETOOBIG;
  A.tiles_per_image = (int)tpi;
  hipStream_t st = (hipStream_t)stream;
  // (one layout per C at every shape: an image's bits do not depend on the batch or the map)
  hipError_t e = c_in == 128 ? launch<128>(A, tpi * batch, st) : launch<256>(A, tpi * batch, st);
  return e == hipSuccess ? ORP_OK : (int)e;
}

}  // extern "C"
