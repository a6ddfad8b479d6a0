// orp_conv3x3_bn_deep.hip -- the 512 -> 512 channel 3x3 / padding 1 convolution of a ResNet stage 4 bottleneck (conv2), stride 1 or 2,
// with its eval-mode BatchNorm and ReLU in the epilogue, in the fp16-pieces arithmetic (gfx950, inference):
//
//   y = relu?( fma(conv3x3(x, w), a[c], b[c]) ),   x, y NCHW fp32, Cin = Cout = 512
//
// The arithmetic is conv3x3_bn_act_kernel's (orp_conv3x3_bn.hip), nothing new numerically: one power-of-two scale from the launch's
// range word (orp_range.hpp), two fp16 planes per operand, lo * hi and hi * lo into a side accumulator, hi * hi into the main one, one
// range_unscale, then orp_affine.hpp's affine_act; padding is zero after the scale; the weights are pack_planes16's
// [pl][tap][C/16][2][C][8] planes.
//
// What differs from conv3x3_bn_act_kernel: at 512 channels a 2 x 16 tile's weight stream is what costs, so K is split INSIDE the
// workgroup, into KS groups of waves, and a workgroup covers 32 * 8 / KS output channels only:
//   * eight waves = 8 / KS output-channel groups of 32 x KS K groups; K group g contracts input channels [g C / KS, (g + 1) C / KS) over
//     all nine taps in a fixed order.  The grid is tiles x (4 KS / 2): a tile's channel groups are neighbours in the grid and share the
//     halo in L2, and with workgroups dealt to the eight XCDs in turn an XCD sees one or two channel groups' weights only (1.2 - 2.4 MB
//     of the 9.4: they stay in its L2).  After the loop K groups 1 .. KS - 1 leave acc + side in LDS (the halo's area, behind a
//     barrier), K group 0 adds them to its own acc + side in their order and runs the epilogue.  No atomics, one KS per stride: an
//     output's value does not depend on its tile, on the grid or on the batch.
//   * stride 1, KS = 4 (64 output channels per workgroup, 256 workgroups for a 32 x 32 map -- with KS = 2 its 128 workgroups left half
//     the CUs idle: 33.5 us against 27.3 measured; two images are slower this way, 53 us against 45, and a 48 x 48 map the same):
//     the whole 4 x 18 halo of all 512 channels is staged once, two fp16 planes [halo pixel][512 + 8] = 149 760 B; the K loop (18
//     phases of four 16-channel chunks per K group, tap-major) has no barrier.  Row stride 260 dwords = 4 modulo 32.
//   * stride 2, KS = 2 (128 output channels per workgroup): the 5 x 33 halo does not fit at 512 channels; it is staged in four passes of
//     128 channels, 64 from each K group's half
//     (165 x 136 x 2 x 2 = 89 760 B, a barrier pair per pass; nine phases per pass).  Halo columns are stored de-interleaved by parity,
//     column (hx & 1) * 17 + (hx >> 1): the 16 lanes of a ds_read_b128 group (consecutive output columns) then read rows ONE pixel
//     apart, 68 dwords = 4 modulo 64 as in the stride-1 kernels; interleaved storage would put them 136 dwords = 8 modulo 64 apart, a
//     two-way conflict.  Tap (ki, kj) reads parity plane kj & 1 at column tx + (kj >> 1) of halo row 2 ty + ki.
//   * the weight ring (one phase deep, refilled in place behind its use) and the one-chunk A read-ahead are the existing kernel's; the
//     ring's loads for the next pass are in flight across that pass's staging.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orp_hip.h"
#include "orp_affine.hpp"
#include "orp_range.hpp"
#include "orp_conv3x3_bn_host.hpp"

namespace {

using namespace orp_conv3x3;       // floatx16 / h8 / h2, kThreads and the host helpers

constexpr int C = 512;             // input = output channels
constexpr int TH = 2, TW = 16;     // output tile: one 32-position MFMA block
constexpr int NCH = 4;             // 16-channel chunks per phase (64 channels of one tap)

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

template <int S, int KS>
struct Cfg {
  static constexpr int WN = 8 / KS;                        // waves over output channels
  static constexpr int CG = 32 * WN;                       // output channels of a workgroup
  static constexpr int KH = C / KS;                        // input channels of a K group
  static constexpr int HROWS = (TH - 1) * S + 3, HCOLS = (TW - 1) * S + 3;   // 4 x 18 / 5 x 33
  static constexpr int ROWS = HROWS * HCOLS;               // halo pixels
  static constexpr int CST = S == 1 ? C : 128;             // channels staged per pass: CST / KS of each K group
  static constexpr int NPASS = C / CST;
  static constexpr int PB = CST / KS / 64;                 // 64-channel blocks of a K group per pass
  static constexpr int PPH = 9 * PB;                       // phases per pass
  static constexpr int ASTR = CST + 8;                     // halves per halo pixel
  static constexpr size_t smem = (size_t)2 * ROWS * ASTR * 2;
  static_assert(smem <= 163840, "a workgroup may take 160 KiB of LDS");
  static_assert(PB >= 1 && smem >= (size_t)(KS - 1) * WN * 16 * 64 * sizeof(float), "the reduction reuses the halo's area");
  // halo pixel (hy, hx) -> its LDS row
  static __device__ __forceinline__ int row(int hy, int hx) { return S == 1 ? hy * HCOLS + hx : hy * HCOLS + (hx & 1) * 17 + (hx >> 1); }
};

template <int S, int KS>
__global__ void __launch_bounds__(kThreads)
conv3x3_bn_deep_kernel(const Args P) {
  using K = Cfg<S, KS>;
  constexpr int CG = K::CG, KH = K::KH;
  constexpr int ASTR = K::ASTR, PLANE = K::ROWS * ASTR, HCOLS = K::HCOLS;
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
  const int wn = wave % K::WN, g = wave / K::WN;
  const int n_wave = cgrp * CG + wn * 32;
  const int mrow = lane & 31, kg = lane >> 5;
  const uint16_t* wp = P.planes + ((size_t)kg * C + n_wave + mrow) * 8;
  constexpr size_t wblk = (size_t)2 * C * 8;
  // phase q of the launch = pass * PPH + (tap * PB + channel block); its chunk j is 16-channel block
  // (g * KH + pass * CST / KS + block * 64) / 16 + j of tap's C / 16
  auto load_b = [&](int q, int j, h8 (&b)[2]) {
    const int pass = q / K::PPH, ph = q - pass * K::PPH;
    const int tap = ph / K::PB, cb = ph - tap * K::PB;
    const uint16_t* a = wp + (size_t)(tap * (C / 16) + (g * KH + pass * (K::CST / KS) + cb * 64) / 16 + j) * wblk;
#pragma unroll
    for (int pl = 0; pl < 2; pl++) b[pl] = *reinterpret_cast<const h8*>(a + (size_t)pl * P.plane_stride);
  };
  h8 bq[NCH][2];
#pragma unroll
  for (int j = 0; j < NCH; j++) load_b(0, j, bq[j]);
  __builtin_amdgcn_sched_barrier(0);                       // (the weights go out first: see conv_halo_kernel's prologue)

  // ---- A fragments: lane (position m = lane % 32 of the tile, k-group) reads 16 B of its halo row per plane ----
  const int ty = mrow >> 4, tx = (mrow - 2 * ty) & 15;     // (columns rotated by two per tile row: conv3x3_bn_act_kernel)
  const uint16_t* abase = sA + (size_t)K::row(S * ty, 0) * ASTR + (size_t)tx * ASTR + g * (K::CST / KS) + 8 * kg;
  auto a_off = [&](int ph) {
    const int tap = ph / K::PB, cb = ph - tap * K::PB;
    const int ki = tap / 3, kj = tap - 3 * ki;
    return K::row(ki, kj) * ASTR + cb * 64;
  };
  auto load_a = [&](int off, int j, h8 (&a)[2]) {
#pragma unroll
    for (int pl = 0; pl < 2; pl++) a[pl] = *reinterpret_cast<const h8*>(abase + pl * PLANE + off + j * 16);
  };

  floatx16 acc = floatx16{0}, side = floatx16{0};
  constexpr int nphase = K::NPASS * K::PPH;

#pragma unroll 1
  for (int pass = 0; pass < K::NPASS; pass++) {
    if (pass > 0) __syncthreads();                         // (every wave has read the pass before)
    // ---- staging: a wave-instruction = 16 halo pixels x 4 channel pairs; the eight waves cover 64 channels of the 16 pixels.  All
    // loads of a pass go out at once from clamped addresses, every one unconditional (conv3x3_bn_act_kernel); LDS channel block cb
    // holds channels (cb / PB) * KH + pass * CST / KS + (cb % PB) * 64 .. + 64: the K groups' shares side by side
    {
      const int px = lane & 15, cq = lane >> 4;
      const float* xb = P.x + ((size_t)img * C + (size_t)pass * (K::CST / KS) + (size_t)((wave * 4 + cq) * 2)) * hw;
      constexpr int NPB = (K::ROWS + 15) / 16, NCB = K::CST / 64;
      constexpr int G = S == 1 ? 5 : 11;
      static_assert(G >= NPB, "one batch of loads per pass");
      float v[G][NCB][2];
      bool in[G];
#pragma unroll
      for (int gi = 0; gi < G; gi++) {
        const int h = gi * 16 + px;
        const int hy = h / HCOLS, hx = h - hy * HCOLS;
        const int yy = S * y0 - 1 + hy, xx = S * x0 - 1 + hx;
        in[gi] = h < K::ROWS && yy >= 0 && yy < H && xx >= 0 && xx < W;
        const float* src = xb + (in[gi] ? (size_t)yy * W + xx : (size_t)0);
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) {
          const int ch = (cb / K::PB) * KH + (cb % K::PB) * 64;
          v[gi][cb][0] = src[(size_t)ch * hw];
          v[gi][cb][1] = src[(size_t)(ch + 1) * hw];
        }
      }
#pragma unroll
      for (int gi = 0; gi < G; gi++)
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) { asm volatile("" : "+v"(v[gi][cb][0])); asm volatile("" : "+v"(v[gi][cb][1])); }
#pragma unroll
      for (int gi = 0; gi < G; gi++) {
        const int h = gi * 16 + px;
        const int hy = h / HCOLS, hx = h - hy * HCOLS;
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) {
          const float s0 = in[gi] ? v[gi][cb][0] * sx : 0.f, s1 = in[gi] ? v[gi][cb][1] * sx : 0.f;   // (padding is zero AFTER the scale)
          h2 hh, ll;
          orp::range_split(s0, hh, ll, 0);
          orp::range_split(s1, hh, ll, 1);
          if (h < K::ROWS) {
            uint16_t* dst = sA + (size_t)K::row(hy, hx) * ASTR + cb * 64 + (wave * 4 + cq) * 2;
            *reinterpret_cast<unsigned*>(dst) = __builtin_bit_cast(unsigned, hh);
            *reinterpret_cast<unsigned*>(dst + PLANE) = __builtin_bit_cast(unsigned, ll);
          }
        }
      }
    }
    __syncthreads();

    h8 a[2][2];
    load_a(a_off(0), 0, a[0]);
    // one phase: the A fragment of the next chunk -- of the next phase's first chunk behind the last one -- is read before the MFMAs of
    // this one are issued; a chunk's weight registers are refilled for the next phase (of the next pass behind a pass's last one) right
    // after use (the last phase re-reads its own: every load of the loop is unconditional, so the compiler's vmcnt counts are exact)
#pragma unroll 1
    for (int ph = 0; ph < K::PPH; ph++) {
      const int q = pass * K::PPH + ph;
      const int q_n = q + 1 < nphase ? q + 1 : q;
      const int off = a_off(ph), off_n = a_off(ph + 1 < K::PPH ? ph + 1 : ph);
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

  // ---- the K groups meet: groups 1 .. KS - 1 leave acc + side in the halo's area, group 0 adds them to its own in their order ----
  float* red = reinterpret_cast<float*>(smem) + (size_t)wn * 16 * 64 + lane;   // [g - 1][wn][r][lane]
  constexpr int RG = K::WN * 16 * 64;
  __syncthreads();                                         // (every wave has read the halo)
  if (g > 0) {
#pragma unroll
    for (int r = 0; r < 16; r++) red[(g - 1) * RG + r * 64] = acc[r] + side[r];
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
      float t = acc[r] + side[r];
#pragma unroll
      for (int k = 0; k < KS - 1; k++) t += red[k * RG + r * 64];
      const float v = orp::range_unscale(t, kxw);
      o[(size_t)ch * hwo] = affine_act(v, P.scale[ch], P.shift[ch], P.relu);
    }
  }
}

template <int S, int KS>
hipError_t launch(const Args& A, long tiles, hipStream_t st) {
  using K = Cfg<S, KS>;
  struct Tag {};
  return launch_with_lds<Tag>(&conv3x3_bn_deep_kernel<S, KS>, tiles * (C / K::CG), K::smem, st, A);
}

}  // namespace

extern "C" {

int orp_conv3x3_bn_deep_ok(int c_in, int c_out, int stride) {
  return (c_in == C && c_out == C && (stride == 1 || stride == 2)) ? 1 : 0;
}

size_t orp_conv3x3_bn_deep_packed_bytes(int c_in, int c_out) { return packed_bytes(orp_conv3x3_bn_deep_ok(c_in, c_out, 1), c_in, c_out); }

int orp_conv3x3_bn_deep_pack_weight(const float* weight, int c_in, int c_out, void* packed, void* stream) {
  return pack_weight(orp_conv3x3_bn_deep_ok(c_in, c_out, 1), weight, c_in, c_out, packed, stream);
}

// THE routing rule of this launch: where it was measured faster than library convolution + pass on MI355X, slowest new run plus what
// the range word costs conv1 against the fastest library run (tests/checks/time_bottleneck_3x3.py --kernel deep; docs/notebook/round23.md
// has the tables).  A closed table of (stride, INPUT map side, images) filled from timed corners only: square maps, both sides inside
// [side_min, side_max].
int orp_conv3x3_bn_deep_pays(int c_in, int c_out, int height, int width, int stride, int batch) {
  if (!orp_conv3x3_bn_deep_ok(c_in, c_out, stride) || height <= 0 || width <= 0 || batch <= 0) return 0;
  static const PaidSquare rows[] = {
      {1, 32, 48, 1}, {1, 32, 32, 2},                        // blocks 1 and 2: the 1024^2 image's map to the 1536^2 image's; two images
      {2, 64, 96, 1}, {2, 64, 64, 2},                        // block 0 (input map)
  };
  return paid(rows, stride, height, width, batch);
}

int orp_conv3x3_bn_deep(const float* x, const void* weight_packed, const float* scale, const float* shift, const uint32_t* range_in,
                        float* y, int batch, int c_in, int c_out, int height, int width, int stride, int relu, void* stream) {
  if (bad_launch_args(x, weight_packed, scale, shift, range_in, y, batch, height, width) || !orp_conv3x3_bn_deep_ok(c_in, c_out, stride))
    return ORP_EINVAL;
  Args A;
  fill_common(A, x, weight_packed, scale, shift, range_in, y, c_in, c_out, height, width, relu);
  A.Ho = (height - 1) / stride + 1; A.Wo = (width - 1) / stride + 1;
  A.tiles_x = (A.Wo + TW - 1) / TW;
  const long tpi = (long)A.tiles_x * ((A.Ho + TH - 1) / TH);
  if (tpi * batch * 8 >= (1L << 31) || (long)height * width >= (1L << 31)) return ORP_ETOOBIG;
  A.tiles_per_image = (int)tpi;
  hipStream_t st = (hipStream_t)stream;
  // (one K split per stride at every shape: an image's bits do not depend on the batch or the map)
  hipError_t e = stride == 1 ? launch<1, 4>(A, tpi * batch, st) : launch<2, 2>(A, tpi * batch, st);
  return e == hipSuccess ? ORP_OK : (int)e;
}

}  // extern "C"
