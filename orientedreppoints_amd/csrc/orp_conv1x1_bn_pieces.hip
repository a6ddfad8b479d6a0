// orp_conv1x1_bn_pieces.hip -- orp_conv1x1_bn.hip's operator on the 16-bit matrix pipe (gfx950, inference):
//
//   y = relu?( fma(conv1x1(x, w), a[c], b[c]) (+ r) ),  r = nothing | res | fma(res, a2[c], b2[c]) rounded to fp32
//
// NCHW fp32 in and out, stride 1, the same argument set (the optional range word included) and the same epilogue expressions
// (orp_affine.hpp).  What changes is the instruction of the contraction.  v_mfma_f32_32x32x2_f32 runs at the vector rate; here every
// fp32 operand is split EXACTLY into three bf16 pieces by truncation, as in orp_dcn_split.hip,
//
//      v = v0 + v1 + v2,   v0 = v & 0xffff0000,   v1 = (v - v0) & 0xffff0000,   v2 = (v - v0) - v1        (8 + 8 + 8 bits)
//
// and x w becomes the six products x2 w0, x0 w2, x1 w1, x1 w0, x0 w1, x0 w0 (smallest first; x1 w2, x2 w1 and x2 w2, each at most
// 2^-24 |x w|, are dropped) on v_mfma_f32_32x32x16_bf16.  Each product of pieces is exact in the fp32 accumulator; bf16 carries
// fp32's exponent, so no range word is read and no operand is scaled.  Every output has ONE accumulator fed in a fixed order --
// ascending 16-channel chunks, the six products of a chunk in the order above: no split-K, no atomics, and the value of an output
// does not depend on the tile it falls in.  Not bit-identical to the fp32 kernel (other grouping of the sum); exact data (every
// partial sum an integer multiple of one unit below 2^24 of them) gives the same bits.
//
// Non-finite x: the split of +-inf leaves inf - inf, so an infinite x gives NaN where the fp32 kernel gives +-inf (and a zero piece
// of a weight times an infinite piece is NaN as well).  The outputs of that POSITION are non-finite, of possibly another class
// than fp32's; no other position is touched: the columns of the product are independent and no cross-lane operation sits in
// the K loop.
//
// Per image Y[Cout][HW] = W[Cout][Cin] X[Cin][HW], output channels as MFMA rows and positions as columns (a store instruction
// writes 32 consecutive positions of two channels).
//   * weights: packed once per weight tensor (orp_conv1x1_bn_pieces_pack_weight) into three bf16 planes [plane][Cin/16][2][Cout][8]:
//     one 16-byte load is the 8 k-values of an MFMA lane.  They go from L2 straight into a register ring of one K step, refilled in
//     place right behind their use.
//   * activations: K runs in steps of 32 (128-position tiles) or 64 channels.  A thread fetches rows k and k + 1 of four consecutive positions (two 16-byte loads along
//     positions), splits the eight values in registers and writes the three planes to LDS as [position][K step + 8] bf16, one packed
//     dword (k, k + 1) per position and plane.  The row stride of 20 or 36 dwords = 4 x odd puts the 16 rows of every ds_read_b128 lane
//     group on 16 different 16-byte slots of the 64 banks.  For the stores (banks modulo 32) a thread's four positions lie 20 or 4
//     banks apart and the threads of a row 16 apart: a thread writes its positions in an order rotated by (position quad / 2) % 4, which
//     leaves a half wave two lanes per bank -- what a 32-bit store does not pay for.  LDS is double buffered: step t + 1 is written
//     while step t is contracted, one barrier per step; the loads of step t + 2 are in flight meanwhile (the narrow tiles run one or
//     two workgroups per CU: a K step's MFMAs alone do not cover a trip to memory).
//   * one workgroup = 4 waves.  Wide layout: each wave owns 32 channels and all positions of the tile (128 channels x 128, 64 or 32
//     positions): no weight is fetched twice by a workgroup.  Cout = 64: 2 x 2 waves on 64 channels x 128 positions.  A tile
//     never crosses an image; the last tile of a plane is ragged (loads clamped and zeroed, stores masked), channels past Cout read
//     the last channel's weights and are not stored.
//   * the residual of a wave's outputs is requested before the last K step's MFMAs.
//   * MODE 3 (orp_conv1x1_bn_act_pieces_dual): r is contracted HERE, out of a second input x2 sampled with stride 1 or 2 and a second
//     packed weight -- a stage's first block, conv3 with the downsample convolution.  The workgroup runs the branch's K loop on the
//     same accumulator (its fetch reads x2 at offsets computed once per thread; the elements a stride of 2 skips are never loaded),
//     turns it into r = fma(acc, a2, b2) in registers, clears it and runs the main K loop; the epilogue is MODE 1's on r.  Each
//     contraction keeps the rule above, so for finite data the bits are those of this kernel launched on the sampled x2 (MODE 0, no
//     ReLU) and launched again on x with that as its residual (MODE 1).  The 4 x 1 wave layout at 64 or 32 positions only: r costs 16
//     registers per 32 positions of a wave through the whole main loop.
// LDS 27 - 60 KB + the BatchNorm constants.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/orp_hip.h"
#include "orp_affine.hpp"
#include "orp_range.hpp"
#include "orp_launch.hpp"
#include "orp_conv1x1_bn_host.hpp"
#include "orp_dcn_split.hpp"

namespace {

constexpr int kThreads = 256;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));

struct Args {
  const float* x;                  // [B][Cin][hw]
  const uint16_t* planes;          // three bf16 planes [pl][Cin/16][2][Cout][8]
  size_t plane_stride;             // elements between two planes
  const float* scale; const float* shift;       // [Cout]
  const float* res;                // [B][Cout][hw] or NULL
  const float* scale2; const float* shift2;     // [Cout] or NULL: the residual's own affine
  float* y;                        // [B][Cout][hw]
  int cin, cout, hw, relu;
  int ntm, ntn;                    // tiles per image: channels, positions
  unsigned* range;                 // RANGE: one word, raised to max range_bits(y)
};
// MODE 3 (the residual is contracted here): r = fma(conv1x1(x2 sampled with stride s2, planes2), scale2, shift2).  Arguments of
// their own, so that the other launches' kernel arguments stay as they are.
struct DualArgs : Args {
  const float* x2;                 // [B][Cin2][hw2]
  const uint16_t* planes2;         // three bf16 planes [pl][Cin2/16][2][Cout][8]
  size_t plane_stride2;
  int cin2, hw2, w2, wo, s2;       // input plane and row length, output row length, stride (1 | 2)
};

using orp_split::split_pair;      // rows k and k + 1 of one position -> the packed dword of each plane (orp_dcn_split.hpp)

// WCH waves over channels (32 each) x 4 / WCH waves over positions (32 WN each).  VEC: hw % 4 == 0 and x 16-byte aligned.  MODE: the
// residual term (0 nothing, 1 res, 2 res with its own affine, 3 contracted here out of x2 in front of the main contraction, with
// its own affine); RANGE: the stored values' range word leaves with them -- template parameters for the reasons
// orp_conv1x1_bn.hip gives.  SAMP (MODE 3 with VEC): x2 is sampled with stride 2 and the output rows are whole position quads
// (four 4-byte loads 8 bytes apart per row); VEC without it: stride 1, x2 is fetched as x is; without VEC: one offset per position.
template <int WCH, int WN, int BK, bool VEC, int MODE, bool RANGE = false, bool SAMP = false>
__global__ void __launch_bounds__(kThreads, 2)
conv1x1_bn_pieces_kernel(const typename std::conditional<MODE == 3, DualArgs, Args>::type P) {
  constexpr int ASTR = BK + 8;       // bf16 elements per position row in LDS: 20 or 36 dwords = 4 x odd
  constexpr int NCH = BK / 16;       // MFMA chunks of 16 channels per K step
  constexpr int WPOS = 4 / WCH;
  constexpr int BM = 32 * WCH, BN = 32 * WN * WPOS;
  constexpr int PLANE = BN * ASTR, BUF = 3 * PLANE;            // bf16 elements
  constexpr int ITEMS = (BK / 2) * (BN / 4);                   // (row pair, position quad) items of a K step
  constexpr int XV = (ITEMS + kThreads - 1) / kThreads;
  __shared__ __align__(16) uint16_t lds[2 * BUF + 8 * BM];     // (one array, as in orp_conv1x1_bn.hip)
  float* Cs = reinterpret_cast<float*>(lds + 2 * BUF);         // [4][BM]: scale, shift, scale2, shift2 of the tile's channels

  const int tid = threadIdx.x;
  const int bid = blockIdx.x;
  const int mt = bid % P.ntm, rest = bid / P.ntm;
  const int nt = rest % P.ntn, b = rest / P.ntn;
  const int m0 = mt * BM, p0 = nt * BN;
  const int hw = P.hw, cout = P.cout;
  const float* xb = P.x + (size_t)b * P.cin * hw;
  if (tid < BM) {                  // (visible behind the first barrier, never rewritten)
    const int ch = min(m0 + tid, cout - 1);
    Cs[tid] = P.scale[ch]; Cs[BM + tid] = P.shift[ch];
    if (MODE >= 2) { Cs[2 * BM + tid] = P.scale2[ch]; Cs[3 * BM + tid] = P.shift2[ch]; }
  }

  const int lane = tid & 63, wave = tid >> 6;
  const int kg = lane >> 5, l31 = lane & 31;
  const int wm0 = (wave / WPOS) * 32, wn0 = (wave % WPOS) * 32 * WN;      // the wave's corner inside the workgroup tile

  // ---- weights: lane (channel, k-group) reads the 8 k-values of a chunk per plane; a register ring of one K step ----
  const uint16_t* wp = P.planes + ((size_t)kg * cout + min(m0 + wm0 + l31, cout - 1)) * 8;
  const uint16_t* wp2 = nullptr;
  size_t ps2 = 0;
  if constexpr (MODE == 3) ps2 = P.plane_stride2;
  if constexpr (MODE == 3) wp2 = P.planes2 + ((size_t)kg * cout + min(m0 + wm0 + l31, cout - 1)) * 8;      // (Cout rows too)
  const size_t wblk = (size_t)2 * cout * 8;
  bf8 wq[NCH][3];
  auto load_w = [&](bool br, int t, int c) {        // br: the branch's weights (MODE 3; a constant at every call)
    const uint16_t* a = (br ? wp2 : wp) + (size_t)(t * NCH + c) * wblk;
    const size_t ps = br ? ps2 : P.plane_stride;
#pragma unroll
    for (int pl = 0; pl < 3; pl++) wq[c][pl] = *reinterpret_cast<const bf8*>(a + (size_t)pl * ps);
  };
#pragma unroll
  for (int c = 0; c < NCH; c++) load_w(MODE == 3, 0, c);

  // ---- activations: item idx of a K step = rows 2 kp, 2 kp + 1 of positions 4 pq .. 4 pq + 3.  16 consecutive lanes take 16
  // consecutive quads of one row pair (256 contiguous bytes per row); a half wave holds two row pairs (BN = 32: 8 quads x 4 pairs)
  float4 xr[2][XV][2];             // two K steps in flight: step t + 2 is requested while step t is contracted
  int xpq[XV], xkp[XV];
#pragma unroll
  for (int i = 0; i < XV; i++) {
    const int idx = tid + i * kThreads;
    if (BN >= 64) {
      const int r = idx >> 5;
      xpq[i] = (idx & 15) + 16 * (r % (BN / 64));
      xkp[i] = ((idx >> 4) & 1) + 2 * (r / (BN / 64));
    } else {
      xpq[i] = idx & (BN / 4 - 1);
      xkp[i] = idx / (BN / 4);
    }
    xkp[i] &= BK / 2 - 1;          // (threads past ITEMS repeat an item's loads and store nothing)
  }
  // MODE 3: where an item's positions lie in a plane of x2 -- position p is input (s2 (p / wo), s2 (p % wo)) -- the same in every K
  // step; clamped as the main fetch clamps.  VEC: one offset per item (the four positions share an input row, s2 elements apart)
  constexpr int NXO = MODE == 3 ? (VEC ? 1 : 4) : 0;
  int xo[XV][NXO > 0 ? NXO : 1];
  const float* x2b = nullptr;
  if constexpr (MODE == 3) {
    x2b = P.x2 + (size_t)b * P.cin2 * P.hw2;
#pragma unroll
    for (int i = 0; i < XV; i++) {
      const int col = p0 + 4 * xpq[i];
#pragma unroll
      for (int j = 0; j < NXO; j++) {
        const int p = VEC ? min(col, hw - 4) : min(col + j, hw - 1);
        const int oy = p / P.wo;
        xo[i][j] = P.s2 * (oy * P.w2 + (p - oy * P.wo));
      }
    }
  }
  auto fetch2 = [&](int k0, float4 (&xr)[XV][2]) {
    if constexpr (MODE == 3)
#pragma unroll
    for (int i = 0; i < XV; i++) {
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const float* src = x2b + (size_t)(k0 + 2 * xkp[i] + h) * P.hw2;
        if (VEC && !SAMP) {
          xr[i][h] = *reinterpret_cast<const float4*>(src + xo[i][0]);
        } else if (VEC) {
          const float* q = src + xo[i][0];
          xr[i][h].x = q[0]; xr[i][h].y = q[2]; xr[i][h].z = q[4]; xr[i][h].w = q[6];
        } else {
          xr[i][h].x = src[xo[i][0]]; xr[i][h].y = src[xo[i][NXO > 1 ? 1 : 0]];
          xr[i][h].z = src[xo[i][NXO > 1 ? 2 : 0]]; xr[i][h].w = src[xo[i][NXO > 1 ? 3 : 0]];
        }
      }
    }
  };
  auto fetch = [&](int k0, float4 (&xr)[XV][2]) {
#pragma unroll
    for (int i = 0; i < XV; i++) {
      const int col = p0 + 4 * xpq[i];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const float* src = xb + (size_t)(k0 + 2 * xkp[i] + h) * hw;
        if (VEC) {
          xr[i][h] = *reinterpret_cast<const float4*>(src + min(col, hw - 4));
        } else if (MODE == 3) {
          // (each offset through a copy the compiler cannot fold into a running address of its own: sixteen of those, held
          // through the main loop next to r, do not fit)
          int o[4];
#pragma unroll
          for (int j = 0; j < 4; j++) { o[j] = min(col + j, hw - 1); asm volatile("" : "+v"(o[j])); }
          xr[i][h].x = src[o[0]]; xr[i][h].y = src[o[1]]; xr[i][h].z = src[o[2]]; xr[i][h].w = src[o[3]];
        } else {
          xr[i][h].x = src[min(col, hw - 1)]; xr[i][h].y = src[min(col + 1, hw - 1)];
          xr[i][h].z = src[min(col + 2, hw - 1)]; xr[i][h].w = src[min(col + 3, hw - 1)];
        }
      }
    }
  };
  auto stage = [&](int buf, const float4 (&xr)[XV][2]) {
#pragma unroll
    for (int i = 0; i < XV; i++) {
      if (ITEMS % kThreads != 0 && tid + i * kThreads >= ITEMS) continue;
      const int col = p0 + 4 * xpq[i];
      float v[2][4];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        v[h][0] = col < hw ? xr[i][h].x : 0.f; v[h][1] = col + 1 < hw ? xr[i][h].y : 0.f;
        v[h][2] = col + 2 < hw ? xr[i][h].z : 0.f; v[h][3] = col + 3 < hw ? xr[i][h].w : 0.f;
      }
      // rotate the four positions by rot = (pq / 2) % 4: store j then writes position (j + rot) % 4
      const int rot = (xpq[i] >> 1) & 3;
#pragma unroll
      for (int h = 0; h < 2; h++) {
        if (rot & 1) { const float t0 = v[h][0]; v[h][0] = v[h][1]; v[h][1] = v[h][2]; v[h][2] = v[h][3]; v[h][3] = t0; }
        if (rot & 2) { const float t0 = v[h][0], t1 = v[h][1]; v[h][0] = v[h][2]; v[h][1] = v[h][3]; v[h][2] = t0; v[h][3] = t1; }
      }
      unsigned* base = reinterpret_cast<unsigned*>(lds + buf * BUF) + xkp[i];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        unsigned d[3];
        split_pair(v[0][j], v[1][j], d);
        unsigned* dst = base + (4 * xpq[i] + ((j + rot) & 3)) * (ASTR / 2);
#pragma unroll
        for (int pl = 0; pl < 3; pl++) dst[pl * (PLANE / 2)] = d[pl];
      }
    }
  };

  f32x16 acc[WN];
#pragma unroll
  for (int ni = 0; ni < WN; ni++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[ni][r] = 0.f;

  // one K step out of buffer `buf`; the weights of chunk c are refilled for step t_next right behind their use
  auto mma = [&](bool wnext, int buf, int t_next) {
    const uint16_t* xa = lds + buf * BUF + (wn0 + l31) * ASTR + 8 * kg;
    auto load_x = [&](int c, bf8 (&q)[WN][3]) {
#pragma unroll
      for (int ni = 0; ni < WN; ni++)
#pragma unroll
        for (int pl = 0; pl < 3; pl++) q[ni][pl] = *reinterpret_cast<const bf8*>(xa + pl * PLANE + ni * 32 * ASTR + c * 16);
    };
    // the narrow tiles read a chunk's fragments one chunk ahead: six or twelve MFMAs do not hide an LDS read behind themselves
    // with one or two waves per SIMD; at 128 positions per wave the registers go to the accumulators instead
    constexpr bool AHEAD = WN <= 2 && !(MODE == 3 && WN == 2);     // (MODE 3 at 64 positions per wave: the registers go to r)
    bf8 xqs[AHEAD ? 2 : 1][WN][3];
    load_x(0, xqs[0]);
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      bf8 (&xq)[WN][3] = xqs[AHEAD ? (c & 1) : 0];
      if (AHEAD) { if (c + 1 < NCH) load_x(c + 1, xqs[(c + 1) & 1]); }
      else if (c > 0) load_x(c, xqs[0]);
      __builtin_amdgcn_sched_barrier(0);
      // D[channel][position]; smallest products first
#pragma unroll
      for (int ni = 0; ni < WN; ni++) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[c][0], xq[ni][2], acc[ni], 0, 0, 0);
#pragma unroll
      for (int ni = 0; ni < WN; ni++) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[c][2], xq[ni][0], acc[ni], 0, 0, 0);
#pragma unroll
      for (int ni = 0; ni < WN; ni++) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[c][1], xq[ni][1], acc[ni], 0, 0, 0);
#pragma unroll
      for (int ni = 0; ni < WN; ni++) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[c][0], xq[ni][1], acc[ni], 0, 0, 0);
#pragma unroll
      for (int ni = 0; ni < WN; ni++) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[c][1], xq[ni][0], acc[ni], 0, 0, 0);
#pragma unroll
      for (int ni = 0; ni < WN; ni++) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[c][0], xq[ni][0], acc[ni], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      load_w(wnext, t_next, c);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // Step t (not the last): request step t + 2 into the register set step t's data left, contract step t out of buffer t & 1, write
  // step t + 1 (requested a step ago) into the other buffer -- its last readers are behind the previous barrier -- one barrier.
  // Every load is unconditional (past the end the last step is requested again), so the compiler's vmcnt counts are exact.
  const int nk = P.cin / BK;
  auto step = [&](bool br, int nk, int t, float4 (&cur)[XV][2], float4 (&nxt)[XV][2], int buf) {
    if (MODE == 3 && br) fetch2(min(t + 2, nk - 1) * BK, cur);
    else fetch(min(t + 2, nk - 1) * BK, cur);
    __builtin_amdgcn_sched_barrier(0);      // the requests go out in front of the MFMAs
    mma(br, buf, t + 1);
    stage(buf ^ 1, nxt);
    __syncthreads();
  };
  float rv[WN][16];
  if constexpr (MODE == 3) {
    // The branch first, on the same accumulator.  Its last MFMAs run with the main contraction's steps 0 and 1 requested and its
    // step-0 weights refilled behind them; then r leaves the accumulator, rounded to fp32 as the two-launch form stores it.
    const int nk2 = P.cin2 / BK;
    fetch2(0, xr[0]);
    stage(0, xr[0]);
    fetch2(min(1, nk2 - 1) * BK, xr[1]);
    __syncthreads();
    int t = 0;
    for (; t + 2 < nk2; t += 2) {
      step(true, nk2, t, xr[0], xr[1], 0);
      step(true, nk2, t + 1, xr[1], xr[0], 1);
    }
    if (t + 1 < nk2) step(true, nk2, t, xr[0], xr[1], 0);
    fetch(0, xr[0]);
    fetch(min(1, nk - 1) * BK, xr[1]);
    __builtin_amdgcn_sched_barrier(0);
    mma(false, (nk2 - 1) & 1, 0);
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const float* cs = Cs + wm0 + 8 * g + 4 * kg;
      const float4 c4 = *reinterpret_cast<const float4*>(cs + 2 * BM);
      const float4 d4 = *reinterpret_cast<const float4*>(cs + 3 * BM);
      const float a2v[4] = {c4.x, c4.y, c4.z, c4.w}, b2v[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int ni = 0; ni < WN; ni++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          rv[ni][4 * g + q] = affine_act(acc[ni][4 * g + q], a2v[q], b2v[q], 0);
          acc[ni][4 * g + q] = 0.f;
        }
    }
    __syncthreads();          // every wave is behind the branch's last LDS reads
    stage(0, xr[0]);
  } else {
    fetch(0, xr[0]);
    stage(0, xr[0]);
    fetch(min(1, nk - 1) * BK, xr[1]);
  }
  __syncthreads();
  int t = 0;
  for (; t + 2 < nk; t += 2) {
    step(false, nk, t, xr[0], xr[1], 0);
    step(false, nk, t + 1, xr[1], xr[0], 1);
  }
  if (t + 1 < nk) step(false, nk, t, xr[0], xr[1], 0);

  // Epilogue addressing.  Register r of tile ni is channel m0 + wm0 + 8 (r >> 2) + 4 kg + (r & 3) at position
  // p0 + wn0 + 32 ni + l31: a store instruction writes 32 consecutive positions of two channels.
  const size_t plane0 = (size_t)b * cout;
  if (MODE == 1 || MODE == 2) {   // requested before the last K step's MFMAs (clamped addresses: no branch per load)
#pragma unroll
    for (int ni = 0; ni < WN; ni++) {
      const int p = min(p0 + wn0 + 32 * ni + l31, hw - 1);
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int ch = min(m0 + wm0 + 8 * (r >> 2) + 4 * kg + (r & 3), cout - 1);
        rv[ni][r] = P.res[(plane0 + ch) * hw + p];
      }
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  mma(false, (nk - 1) & 1, nk - 1);

  unsigned rmax = 0u;
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const int chg = m0 + wm0 + 8 * g + 4 * kg;          // four consecutive channels (Cout % 4 == 0: all in or out)
    const float* cs = Cs + wm0 + 8 * g + 4 * kg;
    const float4 a4 = *reinterpret_cast<const float4*>(cs);
    const float4 b4 = *reinterpret_cast<const float4*>(cs + BM);
    const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
    float a2v[4] = {0.f, 0.f, 0.f, 0.f}, b2v[4] = {0.f, 0.f, 0.f, 0.f};
    if (MODE == 2) {
      const float4 c4 = *reinterpret_cast<const float4*>(cs + 2 * BM);
      const float4 d4 = *reinterpret_cast<const float4*>(cs + 3 * BM);
      a2v[0] = c4.x; a2v[1] = c4.y; a2v[2] = c4.z; a2v[3] = c4.w;
      b2v[0] = d4.x; b2v[1] = d4.y; b2v[2] = d4.z; b2v[3] = d4.w;
    }
#pragma unroll
    for (int ni = 0; ni < WN; ni++) {
      const int p = p0 + wn0 + 32 * ni + l31;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int r = 4 * g + q;
        const float v = acc[ni][r];
        float t;
        if (MODE == 0) t = affine_act(v, av[q], bv[q], P.relu);
        else if (MODE == 1 || MODE == 3) t = affine_res_act(v, av[q], bv[q], rv[ni][r], P.relu);
        else t = affine_res_act(v, av[q], bv[q], affine_act(rv[ni][r], a2v[q], b2v[q], 0), P.relu);
        if (chg < cout && p < hw) {
          P.y[(plane0 + chg + q) * hw + p] = t;
          if (RANGE) rmax = max(rmax, orp::range_bits(t));
        }
      }
    }
  }
  if (RANGE) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rmax = max(rmax, (unsigned)__shfl_xor((int)rmax, o, 64));
    unsigned* red = reinterpret_cast<unsigned*>(lds);          // (free once every wave is behind its last MFMAs)
    __syncthreads();
    if (lane == 0) red[wave] = rmax;
    __syncthreads();
    if (tid == 0) orp::range_raise(P.range, max(max(red[0], red[1]), max(red[2], red[3])));
  }
}

using orp_c1x1::Tile;

// the workgroup tile of a launch.  Cout <= 64: the 2 x 2 layout.  Otherwise the widest position tile of the 128-channel layout that
// still gives the 256 CUs two workgroups each, else the narrowest.
Tile pick_tile(int cout, int hw, int batch) {
  if (cout <= 64) return Tile{64, 128};
  const Tile cand[3] = {{128, 128}, {128, 64}, {128, 32}};
  for (int i = 0; i < 3; i++) {
    const Tile t = cand[i];
    const long wgs = (long)((cout + t.bm - 1) / t.bm) * ((hw + t.bn - 1) / t.bn) * batch;
    if (wgs >= 512) return t;
  }
  return cand[2];
}

template <int WCH, int WN, int BK>
void launch(const Args& A, int batch, bool vec, hipStream_t st) {
  orp_c1x1::dispatch(A, vec, [&](auto mode, auto range, auto v) {
    hipLaunchKernelGGL((conv1x1_bn_pieces_kernel<WCH, WN, BK, decltype(v)::value, decltype(mode)::value, decltype(range)::value>),
                       orp_c1x1::grid_of(A, batch), dim3(kThreads), 0, st, A);
  });
}

// MODE 3 runs on the 4 x 1 wave layout without its widest tile (r costs 16 registers per 32 positions of a wave through the whole
// main contraction): pick_tile's rule without its first candidate
Tile pick_tile_dual(int cout, int hw, int batch) {
  const long wgs = (long)((cout + 127) / 128) * ((hw + 63) / 64) * batch;
  return wgs >= 512 ? Tile{128, 64} : Tile{128, 32};
}

template <int WN>
void launch_dual(const DualArgs& A, int batch, bool vec, hipStream_t st) {
  const dim3 grid((unsigned)((long)A.ntm * A.ntn * batch));
  if (vec && A.s2 == 1) hipLaunchKernelGGL((conv1x1_bn_pieces_kernel<4, WN, 64, true, 3, false, false>), grid, dim3(kThreads), 0, st, A);
  else if (vec) hipLaunchKernelGGL((conv1x1_bn_pieces_kernel<4, WN, 64, true, 3, false, true>), grid, dim3(kThreads), 0, st, A);
  else hipLaunchKernelGGL((conv1x1_bn_pieces_kernel<4, WN, 64, false, 3, false, true>), grid, dim3(kThreads), 0, st, A);
}

}  // namespace

extern "C" {

int orp_conv1x1_bn_act_pieces_ok(int c_in, int c_out) {
  return (c_in >= 64 && c_in <= 2048 && c_in % 64 == 0 && c_out >= 64 && c_out <= 4096 && c_out % 32 == 0) ? 1 : 0;
}

// the workgroup tile (channels x positions) a launch of this shape runs with; 0 where the shape is not supported
int orp_conv1x1_bn_act_pieces_tile(int c_in, int c_out, int hw, int batch, int* tile_channels, int* tile_positions) {
  if (!orp_conv1x1_bn_act_pieces_ok(c_in, c_out) || hw <= 0 || batch <= 0) return 0;
  const Tile t = pick_tile(c_out, hw, batch);
  if (tile_channels) *tile_channels = t.bm;
  if (tile_positions) *tile_positions = t.bn;
  return 1;
}

// THE routing rule of the pieces kernel: where its launch was measured faster than BOTH other sides on MI355X -- library convolution
// + pass and the fp32 fused launch -- slowest pieces run against the fastest run of either (tests/checks/time_bottleneck_1x1_pieces.py;
// docs/notebook/round16.md has the tables).  A closed table as orp_conv1x1_bn_act_pays: three corners were timed per (Cin, Cout)
// pair of R-50, the map of a 1024^2 image with one image and with two, and the map of a 1536^2 image with one image; a row routes
// one image from the 1024^2 map to the 1536^2 map where both ends paid, two images at the 1024^2 map only.  Nothing beyond a timed
// corner is routed.  Both residual forms paid wherever one did, so has_residual does not enter.  45 of the 48 timed points paid.
// The three that lost and the rows they leave out: 64 -> 64 with two images and at the 1536^2 map (bandwidth-bound, level with the
// fp32 kernel: only its 1024^2 corner is routed) and 2048 -> 512 at one image's 1024 positions (64 workgroups' worth of work,
// the library's GEMM wins: only its other two corners are routed).
int orp_conv1x1_bn_act_pieces_pays(int c_in, int c_out, int hw, int batch, int has_residual) {
  if (!orp_conv1x1_bn_act_pieces_ok(c_in, c_out) || hw <= 0 || batch <= 0) return 0;
  (void)has_residual;
  static const orp_c1x1::PaidRow paid[] = {
      {64, 64, 65536, 65536, 1},                                        // stage 1: conv1 of block 0
      {256, 64, 65536, 147456, 1},  {256, 64, 65536, 65536, 2},         //          conv1 of the others
      {64, 256, 65536, 147456, 1},  {64, 256, 65536, 65536, 2},         //          conv3
      {256, 128, 65536, 147456, 1}, {256, 128, 65536, 65536, 2},        // stage 2: conv1 of block 0
      {512, 128, 16384, 36864, 1},  {512, 128, 16384, 16384, 2},        //          conv1 of the others
      {128, 512, 16384, 36864, 1},  {128, 512, 16384, 16384, 2},        //          conv3
      {512, 256, 16384, 36864, 1},  {512, 256, 16384, 16384, 2},        // stage 3: conv1 of block 0
      {1024, 256, 4096, 9216, 1},   {1024, 256, 4096, 4096, 2},         //          conv1 of the others
      {256, 1024, 4096, 9216, 1},   {256, 1024, 4096, 4096, 2},         //          conv3
      {1024, 512, 4096, 9216, 1},   {1024, 512, 4096, 4096, 2},         // stage 4: conv1 of block 0
      {2048, 512, 2304, 2304, 1},   {2048, 512, 1024, 1024, 2},         //          conv1 of the others
      {512, 2048, 1024, 2304, 1},   {512, 2048, 1024, 1024, 2},         //          conv3
  };
  return orp_c1x1::paid(paid, c_in, c_out, hw, batch);
}

int orp_conv1x1_bn_act_pieces_dual_ok(int c_in, int c_in2, int c_out) {
  return (orp_conv1x1_bn_act_pieces_ok(c_in, c_out) && orp_conv1x1_bn_act_pieces_ok(c_in2, c_out)) ? 1 : 0;
}

int orp_conv1x1_bn_act_pieces_dual_tile(int c_in, int c_in2, int c_out, int hw, int batch, int* tile_channels, int* tile_positions) {
  if (!orp_conv1x1_bn_act_pieces_dual_ok(c_in, c_in2, c_out) || hw <= 0 || batch <= 0) return 0;
  const Tile t = pick_tile_dual(c_out, hw, batch);
  if (tile_channels) *tile_channels = t.bm;
  if (tile_positions) *tile_positions = t.bn;
  return 1;
}

// THE routing rule of the dual launch (conv3 with the downsample convolution contracted in front of it): where its slowest run
// beat the fastest run of what it replaces -- library downsample convolution + the pieces conv3 launch that applies the
// downsample BatchNorm to it -- on MI355X (tests/checks/time_bottleneck_dual.py; docs/notebook/round17.md has the tables).  A
// closed table of its own as orp_conv1x1_bn_act_pieces_pays, the same three corners per R-50 stage; hw = output positions.  9 of the
// 12 timed points are routed: stages 1 - 3 at every corner (16 to 57 us less per launch).  Stage 4 has no row: it lost at the 1024^2
// map with one image and with two (level with the pair: the 128 x 32 tile's weight stream), and its 0.8 us of 150 at the 1536^2 map
// is inside either side's own spread of 3 - 4 us.  The pair that was timed runs conv3 on the pieces kernel, so a row also requires
// that conv3 alone is routed there (orp_conv1x1_bn_act_pieces_pays with a residual; true of every row today).
int orp_conv1x1_bn_act_pieces_dual_pays(int c_in, int c_in2, int c_out, int hw, int stride2, int batch) {
  if (!orp_conv1x1_bn_act_pieces_dual_ok(c_in, c_in2, c_out) || hw <= 0 || batch <= 0) return 0;
  if (!orp_conv1x1_bn_act_pieces_pays(c_in, c_out, hw, batch, 1)) return 0;
  static const struct { int cin, cin2, cout, stride, hw_min, hw_max, batch; } paid[] = {
      {64, 64, 256, 1, 65536, 147456, 1},    {64, 64, 256, 1, 65536, 65536, 2},        // stage 1
      {128, 256, 512, 2, 16384, 36864, 1},   {128, 256, 512, 2, 16384, 16384, 2},      // stage 2
      {256, 512, 1024, 2, 4096, 9216, 1},    {256, 512, 1024, 2, 4096, 4096, 2},       // stage 3
  };
  for (const auto& s : paid)
    if (s.cin == c_in && s.cin2 == c_in2 && s.cout == c_out && s.stride == stride2 && s.batch == batch && hw >= s.hw_min &&
        hw <= s.hw_max)
      return 1;
  return 0;
}

// the packed weight: three bf16 planes [3][Cin/16][2][Cout][8] (6 bytes per weight)
size_t orp_conv1x1_bn_pieces_packed_bytes(int c_in, int c_out) {
  return orp_conv1x1_bn_act_pieces_ok(c_in, c_out) ? (size_t)6 * c_in * c_out : 0;
}

// orp_dcn_split.hip's bf16 packer at one tap: the same split, element order and layout.  The argument rule is this file's own
// (Cout % 32 == 0, which orp_split::shape_ok does not take): the packer's index arithmetic holds for any Cout and Cin % 16 == 0.
int orp_conv1x1_bn_pieces_pack_weight(const float* weight, int c_in, int c_out, void* packed, void* stream) {
  if (!weight || !packed || ((uintptr_t)packed & 15) || !orp_conv1x1_bn_act_pieces_ok(c_in, c_out)) return ORP_EINVAL;
  hipError_t e = orp_split::pack_planes_bf16(weight, c_out, c_in, 1, reinterpret_cast<uint16_t*>(packed), (hipStream_t)stream);
  return e == hipSuccess ? ORP_OK : (int)e;
}

// range_out (or NULL): the range word, as orp_c1x1::run describes it
int orp_conv1x1_bn_act_pieces(const float* x, const void* weight_packed, const float* scale, const float* shift, const float* residual,
                              const float* scale2, const float* shift2, float* y, int batch, int c_in, int c_out, int hw, int relu,
                              uint32_t* range_out, void* stream) {
  return orp_c1x1::run<Args>(x, weight_packed, scale, shift, residual, scale2, shift2, y, batch, c_in, c_out, hw, relu, range_out, stream,
                             orp_conv1x1_bn_act_pieces_ok(c_in, c_out) != 0, pick_tile, [&](Args& A, Tile t, bool vec, hipStream_t st) {
    A.planes = reinterpret_cast<const uint16_t*>(weight_packed); A.plane_stride = (size_t)c_in * c_out;
    if (t.bm == 64) launch<2, 2, 32>(A, batch, vec, st);        // (K steps of 64 at 128 positions would leave one workgroup per CU)
    else if (t.bn == 128) launch<4, 4, 32>(A, batch, vec, st);
    else if (t.bn == 64) launch<4, 2, 64>(A, batch, vec, st);
    else launch<4, 1, 64>(A, batch, vec, st);
  });
}

// y = relu?( fma(conv1x1(x, w), a, b) + r ),  r = fma(conv1x1(x2 sampled at (stride2 oy, stride2 ox), w2), a2, b2) rounded to fp32: a
// bottleneck's conv3 with the downsample convolution of its block contracted in the same launch (MODE 3), the downsample output
// never in memory.  Each contraction follows the kernel's rule (one accumulator, ascending 16-channel chunks, six products smallest
// first, no dependence on the tile); for finite data the bits are those of orp_conv1x1_bn_act_pieces on the sampled x2 (no residual,
// no ReLU) followed by orp_conv1x1_bn_act_pieces on x with that as its residual.  No range word, no atomics.
int orp_conv1x1_bn_act_pieces_dual(const float* x, const void* w_packed, const float* scale, const float* shift, const float* x2,
                                   const void* w2_packed, const float* scale2, const float* shift2, int c_in2, int h2, int w2,
                                   int stride2, float* y, int batch, int c_in, int c_out, int ho, int wo, int relu, void* stream) {
  if (!x || !w_packed || !scale || !shift || !x2 || !w2_packed || !scale2 || !shift2 || !y || batch <= 0 || ho <= 0 || wo <= 0 ||
      h2 <= 0 || w2 <= 0 || !orp_conv1x1_bn_act_pieces_dual_ok(c_in, c_in2, c_out))
    return ORP_EINVAL;
  if (stride2 != 1 && stride2 != 2) return ORP_EINVAL;
  if (ho != (h2 - 1) / stride2 + 1 || wo != (w2 - 1) / stride2 + 1) return ORP_EINVAL;
  if ((const float*)y == x || (const float*)y == x2) return ORP_EINVAL;
  if (((uintptr_t)w_packed & 15) || ((uintptr_t)w2_packed & 15)) return ORP_EINVAL;
  if ((long)ho * wo >= (1L << 31) / 4 || (long)h2 * w2 >= (1L << 31) / 4) return ORP_ETOOBIG;
  const int hw = ho * wo;
  const Tile t = pick_tile_dual(c_out, hw, batch);
  DualArgs A{};
  A.x = x; A.planes = reinterpret_cast<const uint16_t*>(w_packed); A.plane_stride = (size_t)c_in * c_out;
  A.scale = scale; A.shift = shift; A.res = nullptr; A.scale2 = scale2; A.shift2 = shift2; A.y = y;
  A.cin = c_in; A.cout = c_out; A.hw = hw; A.relu = relu ? 1 : 0;
  A.ntm = (c_out + t.bm - 1) / t.bm; A.ntn = (hw + t.bn - 1) / t.bn;
  A.range = nullptr;
  A.x2 = x2; A.planes2 = reinterpret_cast<const uint16_t*>(w2_packed); A.plane_stride2 = (size_t)c_in2 * c_out;
  A.cin2 = c_in2; A.hw2 = h2 * w2; A.w2 = w2; A.wo = wo; A.s2 = stride2;
  if ((long)A.ntm * A.ntn * batch >= (1L << 31)) return ORP_ETOOBIG;
  const bool vec = (hw & 3) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)x2 & 15) == 0 && (stride2 == 1 || (wo & 3) == 0);
  hipStream_t st = (hipStream_t)stream;
  if (t.bn == 64) launch_dual<2>(A, batch, vec, st);
  else launch_dual<1>(A, batch, vec, st);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ORP_OK : (int)e;
}

}  // extern "C"
