// orp_conv3x3_bn.hip -- a ResNet bottleneck's 3x3 / stride 1 / padding 1 convolution (conv2) with its eval-mode BatchNorm and ReLU in
// the epilogue, in the fp16-pieces arithmetic (gfx950, inference):
//
//   y = relu?( fma(conv3x3(x, w), a[c], b[c]) ),   x, y NCHW fp32, Cin = Cout in {64, 128, 256}
//
// The arithmetic is conv_halo_kernel's (orp_dcn_split.hip; the range rule is orp_range.hpp): every input is multiplied by ONE power of
// two taken from the launch's range word (left by the producer of x: orp_conv1x1_bn_act_range / orp_affine_act_range), split into two
// fp16 pieces, contracted with the weights' two fp16 planes (orp_conv3x3_bn_pack_weight: pack_planes16_kernel's format) as lo*hi, hi*lo, hi*hi into fp32
// accumulators -- the two small products into a side set that is added once at the end -- and scaled back by one ldexp.  The
// BatchNorm and the ReLU are orp_affine.hpp's expressions on the un-scaled accumulator: the raw convolution output never exists.
//
// What differs from conv_halo_kernel:
//   * the input is NCHW: the tile's (TH + 2) x 18 halo is read per channel as runs of 18 consecutive floats and written TRANSPOSED
//     into LDS as two fp16 planes [halo pixel][C + 8] (row stride 36 / 68 / 132 dwords = 4 modulo 32), scaled and split once per
//     element; padding is zero after the scale.  A wave-instruction of the staging covers 16 halo pixels x 4 channel pairs: a
//     ds_write_b32 half-wave puts 16 pixels x 2 pairs on banks 4 p + pair, two lanes per bank, which a 32-bit store does not pay for.
//     The MFMA operand of a lane is 16 B of halo row (tile row + ki) * 18 + (column + kj); a tile row's 16 columns are rotated by
//     two per tile row so that row index = lane modulo 16 whatever the tile row: the 16 lanes of every ds_read_b128 group sit on
//     16 different rows = all 64 banks (the tap's offset is one constant for all lanes).
//   * eight waves = WM (positions) x C / 32 (channels): 4 x 2 with two 32-position blocks per wave at 64 channels (16 x 16 tiles),
//     2 x 4 at 128 (4 x 16), 1 x 8 at 256 (2 x 16).  A tile never crosses an image.  The R-50 maps of a 1024^2 image give
//     256 / 256 / 128 tiles.
//   * the whole halo is staged in front of the loop, so the loop has no barrier at all: 9 taps x C / 64 phases of four 16-channel
//     chunks, A fragments read one chunk ahead, the weight ring (one phase) refilled in place right behind its use.
// Deterministic: fixed order, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orp_hip.h"
#include "orp_affine.hpp"
#include "orp_range.hpp"
#include "orp_conv3x3_bn_host.hpp"

namespace {

using namespace orp_conv3x3;       // floatx16 / h8 / h2, kThreads and the host helpers

constexpr int TW = 16;             // tile width
constexpr int HWID = TW + 2;       // halo width
constexpr int NCH = 4;             // 16-channel chunks per phase (64 channels of one tap)

struct Args {
  const float* x;                  // [B][C][H][W]
  const uint16_t* planes;          // two fp16 planes [pl][tap][C/16][2][C][8]
  size_t plane_stride;
  const float* wscale;             // device scalar: the planes' power-of-two scale
  const unsigned* range;           // device scalar: bits of (a bound of) max |x|
  const float* scale; const float* shift;   // [C]
  float* y;                        // [B][C][H][W]
  int H, W, relu, tiles_x, tiles_per_image;
};

template <int C, int WM, int MT>
struct Cfg {
  static constexpr int WN = 8 / WM;
  static_assert(WN * 32 == C, "a wave owns 32 output channels");
  static constexpr int TH = 2 * WM * MT;                   // tile height: 32 MT positions per wave = 2 MT rows of 16
  static constexpr int ROWS = (TH + 2) * HWID;             // halo pixels
  static constexpr int ASTR = C + 8;                       // halves per halo pixel
  static constexpr size_t smem = (size_t)2 * ROWS * ASTR * 2;
};

template <int C, int WM, int MT>
__global__ void __launch_bounds__(kThreads)
conv3x3_bn_act_kernel(const Args P) {
  using K = Cfg<C, WM, MT>;
  constexpr int ASTR = K::ASTR, PLANE = K::ROWS * ASTR;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t* sA = reinterpret_cast<uint16_t*>(smem);        // [2 planes][ROWS][C + 8]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x;
  const int img = tile / P.tiles_per_image, tt = tile - img * P.tiles_per_image;
  const int trow = tt / P.tiles_x;
  const int y0 = trow * K::TH, x0 = (tt - trow * P.tiles_x) * TW;
  const int H = P.H, W = P.W;
  const size_t hw = (size_t)H * W;

  const int kx = orp::range_exp(*P.range);
  const float sx = orp::range_scale(kx);
  const int kxw = kx + orp::range_exp_of(*P.wscale);

  // ---- weight fragments: lane (output channel n_wave + lane % 32, k-group lane / 32) reads the 8 k-values of a chunk per plane ----
  const int wn = wave % K::WN, wm = wave / K::WN;
  const int n_wave = wn * 32;
  const int mrow = lane & 31, kg = lane >> 5;
  const uint16_t* wp = P.planes + ((size_t)kg * C + n_wave + mrow) * 8;
  constexpr size_t wblk = (size_t)2 * C * 8;
  auto load_b = [&](int ph, int j, h8 (&b)[2]) {            // phase ph = tap * (C / 64) + channel block: chunks are consecutive
    const uint16_t* a = wp + ((size_t)ph * NCH + j) * wblk;
#pragma unroll
    for (int pl = 0; pl < 2; pl++) b[pl] = *reinterpret_cast<const h8*>(a + (size_t)pl * P.plane_stride);
  };
  h8 bq[NCH][2];
#pragma unroll
  for (int j = 0; j < NCH; j++) load_b(0, j, bq[j]);
  __builtin_amdgcn_sched_barrier(0);                       // (the weights go out first: see conv_halo_kernel's prologue)

  // ---- staging: a wave-instruction = 16 halo pixels x 4 channel pairs; the eight waves cover 64 channels of the 16 pixels ----
  // Loads go out in batches of G pixel groups from clamped addresses, every one unconditional (the empty asm keeps the compiler
  // from sinking a load under its pixel's padding test, one exposed latency per pixel group); the splits and stores follow.
  {
    const int px = lane & 15, cq = lane >> 4;
    const float* xb = P.x + (size_t)img * C * hw + (size_t)((wave * 4 + cq) * 2) * hw;
    constexpr int NPB = (K::ROWS + 15) / 16, G = C == 64 ? 7 : C == 128 ? 4 : 3, NCB = C / 64;
#pragma unroll 1
    for (int pb0 = 0; pb0 < NPB; pb0 += G) {
      float v[G][NCB][2];
      bool in[G];
#pragma unroll
      for (int g = 0; g < G; g++) {
        const int h = (pb0 + g) * 16 + px;
        const int hy = h / HWID, hx = h - hy * HWID;
        const int yy = y0 - 1 + hy, xx = x0 - 1 + hx;
        in[g] = h < K::ROWS && yy >= 0 && yy < H && xx >= 0 && xx < W;
        const float* src = xb + (in[g] ? (size_t)yy * W + xx : (size_t)0);
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) {
          v[g][cb][0] = src[(size_t)(cb * 64) * hw];
          v[g][cb][1] = src[(size_t)(cb * 64 + 1) * hw];
        }
      }
#pragma unroll
      for (int g = 0; g < G; g++)
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) { asm volatile("" : "+v"(v[g][cb][0])); asm volatile("" : "+v"(v[g][cb][1])); }
#pragma unroll
      for (int g = 0; g < G; g++) {
        const int h = (pb0 + g) * 16 + px;
#pragma unroll
        for (int cb = 0; cb < NCB; cb++) {
          const float s0 = in[g] ? v[g][cb][0] * sx : 0.f, s1 = in[g] ? v[g][cb][1] * sx : 0.f;   // (padding is zero AFTER the scale)
          h2 hh, ll;
          orp::range_split(s0, hh, ll, 0);
          orp::range_split(s1, hh, ll, 1);
          if (h < K::ROWS) {
            uint16_t* dst = sA + (size_t)h * ASTR + cb * 64 + (wave * 4 + cq) * 2;
            *reinterpret_cast<unsigned*>(dst) = __builtin_bit_cast(unsigned, hh);
            *reinterpret_cast<unsigned*>(dst + PLANE) = __builtin_bit_cast(unsigned, ll);
          }
        }
      }
    }
  }
  __syncthreads();

  // ---- A fragments: lane (position m = block * 32 + lane % 32 of the tile, k-group) reads 16 B of its halo row per plane ----
  auto tyx = [&](int m, int& ty, int& tx) { ty = m >> 4; tx = (m - 2 * ty) & 15; };
  const uint16_t* abase[MT];
#pragma unroll
  for (int mt = 0; mt < MT; mt++) {
    int ty, tx;
    tyx((wm * MT + mt) * 32 + mrow, ty, tx);
    abase[mt] = sA + (size_t)(ty * HWID + tx) * ASTR + 8 * kg;
  }
  auto a_off = [&](int ph) {
    const int tap = ph / (C / 64), cb = ph - tap * (C / 64);
    const int ki = tap / 3;
    return (ki * HWID + tap - 3 * ki) * ASTR + cb * 64;
  };
  auto load_a = [&](int off, int j, h8 (&a)[MT][2]) {
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
      for (int pl = 0; pl < 2; pl++) a[mt][pl] = *reinterpret_cast<const h8*>(abase[mt] + pl * PLANE + off + j * 16);
  };

  floatx16 acc[MT], side[MT];
#pragma unroll
  for (int mt = 0; mt < MT; mt++) { acc[mt] = floatx16{0}; side[mt] = floatx16{0}; }
  constexpr int nphase = 9 * (C / 64);
  h8 a[2][MT][2];
  load_a(a_off(0), 0, a[0]);
  // one phase: the A fragments of the next chunk -- of the next phase's first chunk behind the last one -- are read before the MFMAs
  // of this one are issued; a chunk's weight registers are refilled for the next phase right after use (the last phase re-reads its
  // own: every load of the loop is unconditional, so the compiler's vmcnt counts are exact)
#pragma unroll 1
  for (int ph = 0; ph < nphase; ph++) {
    const int ph_n = ph + 1 < nphase ? ph + 1 : ph;
    const int off = a_off(ph), off_n = a_off(ph_n);
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      if (j + 1 < NCH) load_a(off, j + 1, a[(j + 1) & 1]);
      else             load_a(off_n, 0, a[0]);
      __builtin_amdgcn_sched_barrier(0);
      // D[channel][position]: lo * hi and hi * lo into the side set, hi * hi into the main one (conv_halo_kernel's order)
#pragma unroll
      for (int mt = 0; mt < MT; mt++) side[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bq[j][0], a[j & 1][mt][1], side[mt], 0, 0, 0);
#pragma unroll
      for (int mt = 0; mt < MT; mt++) side[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bq[j][1], a[j & 1][mt][0], side[mt], 0, 0, 0);
#pragma unroll
      for (int mt = 0; mt < MT; mt++) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bq[j][0], a[j & 1][mt][0], acc[mt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      load_b(ph_n, j, bq[j]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- epilogue: un-scale, BatchNorm as one fma, ReLU last; register r of a lane is channel n_wave + (r & 3) + 8 (r >> 2) + 4 kg ----
  float ca[16], cb_[16];
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int ch = n_wave + (r & 3) + 8 * (r >> 2) + 4 * kg;
    ca[r] = P.scale[ch]; cb_[r] = P.shift[ch];
  }
  float* yb = P.y + (size_t)img * C * hw;
#pragma unroll
  for (int mt = 0; mt < MT; mt++) {
    int ty, tx;
    tyx((wm * MT + mt) * 32 + mrow, ty, tx);
    const int yy = y0 + ty, xx = x0 + tx;
    if (yy < H && xx < W) {
      float* o = yb + (size_t)yy * W + xx;
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int ch = n_wave + (r & 3) + 8 * (r >> 2) + 4 * kg;
        const float v = orp::range_unscale(acc[mt][r] + side[mt][r], kxw);
        o[(size_t)ch * hw] = affine_act(v, ca[r], cb_[r], P.relu);
      }
    }
  }
}

struct Layout { int wm, wn, mt, th; };

bool layout_of(int c, Layout& l) {
  if (c == 64) l = Layout{4, 2, 2, 16};
  else if (c == 128) l = Layout{2, 4, 1, 4};
  else if (c == 256) l = Layout{1, 8, 1, 2};
  else return false;
  return true;
}

template <int C, int WM, int MT>
hipError_t launch(const Args& A, long tiles, hipStream_t st) {
  struct Tag {};
  return launch_with_lds<Tag>(&conv3x3_bn_act_kernel<C, WM, MT>, tiles, Cfg<C, WM, MT>::smem, st, A);
}

}  // namespace

extern "C" {

int orp_conv3x3_bn_act_ok(int c_in, int c_out) {
  return (c_in == c_out && (c_in == 64 || c_in == 128 || c_in == 256)) ? 1 : 0;
}

size_t orp_conv3x3_bn_packed_bytes(int c_in, int c_out) { return packed_bytes(orp_conv3x3_bn_act_ok(c_in, c_out), c_in, c_out); }

int orp_conv3x3_bn_pack_weight(const float* weight, int c_in, int c_out, void* packed, void* stream) {
  return pack_weight(orp_conv3x3_bn_act_ok(c_in, c_out), weight, c_in, c_out, packed, stream);
}

int orp_conv3x3_bn_act_tile(int c_in, int c_out, int height, int width, int batch, int* tile_h, int* tile_w, int* waves_pos,
                            int* waves_ch) {
  Layout l;
  if (!orp_conv3x3_bn_act_ok(c_in, c_out) || height <= 0 || width <= 0 || batch <= 0 || !layout_of(c_in, l)) return 0;
  if (tile_h) *tile_h = l.th;
  if (tile_w) *tile_w = TW;
  if (waves_pos) *waves_pos = l.wm;
  if (waves_ch) *waves_ch = l.wn;
  return 1;
}

// THE routing rule: where the fused launch was measured faster than library convolution + pass on MI355X (slowest fused run against
// fastest library run, tests/checks/time_bottleneck_3x3.py; docs/notebook/round15.md has the tables).  A closed table as
// orp_conv1x1_bn_act_pays: per channel count the R-50 map of a 1024^2 image with one image and with two, and the map of a 1536^2
// image with one image; one image is routed from the 1024^2 map to the 1536^2 map where both ends paid, two images at the 1024^2
// map only.  Nothing beyond a timed corner is routed.  Every timed point paid, with what the range word costs conv1 (a fill launch
// and the epilogue's maximum, 4 - 13 us) charged to this launch: 29 - 36 us against 64 - 68 at stage 1, 23 - 29 against 58 - 62 at
// stage 2, 30 - 36 against 51 - 55 at stage 3 (one image, 1024^2).
int orp_conv3x3_bn_act_pays(int c_in, int c_out, int height, int width, int batch) {
  if (!orp_conv3x3_bn_act_ok(c_in, c_out) || height <= 0 || width <= 0 || batch <= 0) return 0;
  // (channels, map side at 1024^2, at 1536^2, images): height and width each inside [side_min, side_max] -- only square maps were
  // timed, so a map is routed where BOTH sides lie between the timed corners' and no further
  static const PaidSquare rows[] = {
      {64, 256, 384, 1},  {64, 256, 256, 2},                         // stage 1: blocks 0 - 2
      {128, 128, 192, 1}, {128, 128, 128, 2},                        // stage 2: blocks 1 - 3
      {256, 64, 96, 1},   {256, 64, 64, 2},                          // stage 3: blocks 1 - 5
  };
  return paid(rows, c_in, height, width, batch);
}

int orp_conv3x3_bn_act(const float* x, const void* weight_packed, const float* scale, const float* shift, const uint32_t* range_in,
                       float* y, int batch, int c_in, int c_out, int height, int width, int relu, void* stream) {
  Layout l;
  if (bad_launch_args(x, weight_packed, scale, shift, range_in, y, batch, height, width) || !orp_conv3x3_bn_act_ok(c_in, c_out) ||
      !layout_of(c_in, l))
    return ORP_EINVAL;
  Args A;
  fill_common(A, x, weight_packed, scale, shift, range_in, y, c_in, c_out, height, width, relu);
  A.tiles_x = (width + TW - 1) / TW;
  const long tpi = (long)A.tiles_x * ((height + l.th - 1) / l.th);
  if (tpi * batch >= (1L << 31) || (long)height * width >= (1L << 31)) return ORP_ETOOBIG;
  A.tiles_per_image = (int)tpi;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = c_in == 64 ? launch<64, 4, 2>(A, tpi * batch, st)
               : c_in == 128 ? launch<128, 2, 1>(A, tpi * batch, st) : launch<256, 1, 1>(A, tpi * batch, st);
  return e == hipSuccess ? ORP_OK : (int)e;
}

}  // extern "C"
