// orp_dcn_split.hpp -- interface between orp_dcn.hip (entry points, layout conversion, tile table) and orp_dcn_split.hip (the
// fp32-by-bf16-splitting DeformConv forward kernel).  Internal to liborp_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace orp_split {

constexpr int kMaxLevels = 8;

struct Level {
  const float* x[2];    // NHWC [B, H, W, Cin] of layer 0 / layer 1 (pair launch: both layers read the same offsets / mask)
  const float* off;     // NCHW [B, 2*taps, Ho, Wo]
  const float* mask;    // DCNv2 modulation [B, taps, Ho, Wo] or nullptr
  float* out[2];        // NCHW [B, Cout, Ho, Wo] or NHWC [B, Ho, Wo, Cout]
  int H, W, Ho, Wo;
  const uint16_t* planes;   // nullptr, or this level's own weight planes / bias (single-layer launches: a different layer per
  const float* bias;        // level, e.g. the FPN's output convolutions) instead of Args::planes[0] / bias[0]
  const float* wscale;      //   ... and (nprod == 3) the scale of its fp16 planes
};

struct Args {
  Level lv[kMaxLevels];
  int nlev, B, Cin, Cout;
  int kh, kw, sh, sw, ph, pw, dh, dw;
  const uint16_t* planes[2];   // per layer: planes_of(packed, ..., nprod): [3 planes hi|mid|lo] bf16 or [2 planes hi|lo] fp16,
                               // each [tap][Cin/16][2][Cout][8] (pack_planes)
  const float* bias[2];        // [Cout] or nullptr
  int relu, nconv, out_nchw;
  int nprod;                   // 6 or 9 partial products of three bf16 pieces; 3 = two fp16 pieces (hi*hi, hi*lo, lo*hi)
  const float* wscale[2];      // nprod == 3: wscale_of(packed, ...) per layer (device scalar: the planes' power-of-two scale)
  unsigned* scratch;           // nprod == 3: >= 8 bytes of device memory of the caller's (max |x| of the inputs, per layer)
  const unsigned* amax_in;     // nprod == 3: nullptr (a pre-pass over the inputs fills `scratch`), or float bits of upper bounds of
  int amax_stride;             //   max |x| the producer of the inputs left: layer cv takes the maximum of the amax_count words at
  int amax_count = 0;          //   amax_in[cv * amax_stride] (0 / 1: one word)
  // GroupNorm fused around a PLAIN launch (orp_conv_split_multi_gn): tiles never span two images; the inputs are read as
  // relu?(x * a[c] + b[c]) (coef_in [layer][level][image][Cin] (a, b) pairs, or nullptr); every output tile leaves its per-group
  // statistics in gn_part [layer][tile][group] (mean, M2, max |y|, count), or nullptr
  int per_image = 0;
  const float* coef_in = nullptr;
  int relu_in = 0;
  float* gn_part = nullptr;
  int groups = 0;
};

// the tile table of a launch (what the kernel and orp_conv_split_gn_finish agree on)
struct Plan {
  int MT, tiles; int tile0[kMaxLevels], tpi[kMaxLevels];
  int halo;                                // 1: the halo kernel's spatial tiles of th[l] x tw[l] positions (tpi[l] = tiles per image, row-major)
  int th[kMaxLevels], tw[kMaxLevels];
};
Plan plan(const Args& a);
// The one place that chooses between the two plain-convolution kernels: true when the launch `a` takes the halo kernel (fp16-pieces mode,
// 3x3, stride 1, dilation 1, padding 1, Cin % 64 == 0, Cin <= 256, no offsets) and `on`, with the tile shape per level.  plan() asks it
// with `on` = halo_switch(); a caller that sizes a buffer for either choice asks with on = 1.
bool halo_tiles(const Args& a, int on, int* th, int* tw);
int halo_switch();                         // ORP_CONV_HALO (default 1) unless set_halo() said otherwise
void set_halo(int on);                     // 0 / 1; -1: back to the environment's choice

// cin % 64 == 0, cout % 64 == 0, taps <= 9
bool shape_ok(int c_in, int c_out, int kh, int kw);
// number of uint16_t elements of one layer's planes (bf16 planes + fp16 planes + the fp16 planes' scale)
size_t plane_elems(int c_out, int c_in, int taps);
// within the buffer orp_dcn_pack_weight fills (2 N floats of fp32 packings first): the plane set of a mode, the fp16 scale
const uint16_t* planes_of(const float* packed, int c_out, int c_in, int taps, int nprod);
const float* wscale_of(const float* packed, int c_out, int c_in, int taps);
hipError_t pack_planes(const float* weight /* [o][c][tap] */, int c_out, int c_in, int taps, uint16_t* planes, hipStream_t st);
// the three bf16 planes alone (3 N elements at planes; no shape_ok: any c_out, c_in % 16 == 0) -- what pack_planes does first
hipError_t pack_planes_bf16(const float* weight, int c_out, int c_in, int taps, uint16_t* planes, hipStream_t st);
// the two fp16 planes alone (2 N elements at planes16) and their tail (tail[0] the scale, tail[1] max |w| as float bits)
hipError_t pack_planes16(const float* weight, int c_out, int c_in, int taps, uint16_t* planes16, float* tail, hipStream_t st);
hipError_t launch(const Args& a, hipStream_t st);
// dev aid (orp_debug_amax_log): returns the number of launches logged since the previous call
int set_amax_log(unsigned* log, int capacity_launches);

// ---- the exact three-piece bf16 split in registers, shared by every kernel that stages fp32 operands for v_mfma_f32_32x32x16_bf16 ----
// two fp32 values whose low 16 bits are zero (or may be dropped) -> one dword of two bf16: (a >> 16) | (b & 0xffff0000)
__device__ __forceinline__ unsigned pack_hi16(float a, float b) {
  return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
}

// elements k (a) and k + 1 (b) of one row -> the packed dword of each plane
__device__ __forceinline__ void split_pair(float a, float b, unsigned (&d)[3]) {
  const float a0 = __uint_as_float(__float_as_uint(a) & 0xffff0000u), b0 = __uint_as_float(__float_as_uint(b) & 0xffff0000u);
  const float ar = a - a0, br = b - b0;
  const float a1 = __uint_as_float(__float_as_uint(ar) & 0xffff0000u), b1 = __uint_as_float(__float_as_uint(br) & 0xffff0000u);
  d[0] = pack_hi16(a0, b0);
  d[1] = pack_hi16(a1, b1);
  d[2] = pack_hi16(ar - a1, br - b1);
}

}  // namespace orp_split
