// orp_conv1x1_bn.hip -- a ResNet bottleneck's 1x1 convolution with what follows it in its epilogue (gfx950, inference).
//
//   y = relu?( fma(conv1x1(x, w), a[c], b[c]) (+ r) ),  r = nothing | res | fma(res, a2[c], b2[c]) rounded to fp32
//
// for NCHW fp32 tensors at stride 1: conv3 + bn3 + identity (+ the downsample BatchNorm) + ReLU and conv1 + bn1 + ReLU.  The library
// writes the raw convolution output and orp_affine_act / orp_affine2_act read it back with the residual; here the accumulators go
// through the same expressions (orp_affine.hpp) on their way out and the intermediate tensor never exists.
//
// Per image the convolution is Y[Cout][HW] = W[Cout][Cin] X[Cin][HW].  v_mfma_f32_32x32x2_f32 (exact fp32 products and sums, bitwise
// an fmaf chain in ascending k) with output channels as rows and positions as columns: a lane's B element is x[b][k][p], positions
// are contiguous in NCHW, so nothing is transposed; its A element is w[c][k], read from the weights stored [Cin][Cout] (packed once
// per weight tensor by the caller).  Every output has ONE accumulator fed in ascending k: no split-K, no atomics, and the value
// does not depend on the tile an output falls in.
//
// One workgroup = 4 waves as 2 (channels) x 2 (positions), a wave owns WM x WN tiles of 32 x 32: workgroup tiles of 128 x 128,
// 64 x 128 or 64 x 64 (channels x positions), chosen per launch so that the grid gives every CU two workgroups where the shape allows.
// K runs in steps of 32: the [32][BM] weight rows and [32][BN] input rows of step t + 1 are fetched with 16-byte loads into registers
// while step t's MFMAs read their operands from LDS (ds_read_b32, 32 consecutive floats per half wave: conflict-free), and are
// written to LDS behind them.  A tile never crosses an image: p runs within one [H*W] plane, the last tile of a plane is ragged
// (loads clamped to the plane and zeroed, stores masked).  LDS 17 - 34 KB; at most 182 / 113 / 60 registers: two (three without a
// residual) / four / eight workgroups per CU.
// The residual of a wave's outputs is requested before the last K step's MFMAs, so it arrives under them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orp_hip.h"
#include "orp_affine.hpp"
#include "orp_range.hpp"
#include "orp_launch.hpp"
#include "orp_conv1x1_bn_host.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int BK = 32;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Args {
  const float* x;        // [B][Cin][hw]
  const float* wt;       // [Cin][Cout]
  const float* scale; const float* shift;       // [Cout]
  const float* res;      // [B][Cout][hw] or NULL
  const float* scale2; const float* shift2;     // [Cout] or NULL: the residual's own affine
  float* y;              // [B][Cout][hw]
  int cin, cout, hw, relu;
  int ntm, ntn;          // tiles per image: channels, positions
  unsigned* range;       // RANGE: one word, raised to max range_bits(y) (orp_range.hpp) for the fp16-pieces kernel that reads y
};

// VEC: hw % 4 == 0 and x 16-byte aligned -> the input rows are fetched as float4.  MODE: the residual term (0 nothing, 1 res,
// 2 res with its own affine) -- a template parameter so that the epilogue is straight-line code: with a run-time mode the requested
// residual values meet an undefined value at a join and the compiler waits for every one of them in front of the last MFMAs.
// RANGE: the stored values' range word leaves with them (a wave maximum, the four waves' through LDS, one conditional atomic per
// workgroup); a template parameter so that the other instantiations keep their instruction stream.
template <int WM, int WN, bool VEC, int MODE, bool RANGE = false>
__global__ void __launch_bounds__(kThreads, 2)
conv1x1_bn_act_kernel(const Args P) {
  constexpr int BM = 64 * WM, BN = 64 * WN;
  constexpr int WV = BK * BM / 4 / kThreads, XV = BK * BN / 4 / kThreads;     // float4s per thread and K step
  __shared__ __align__(16) float lds[BK * (BM + BN) + 4 * BM];      // (one array: a second object de-pipelines the K loop's waits)
  float* Ws = lds;                 // [BK][BM]
  float* Xs = lds + BK * BM;       // [BK][BN]
  float* Cs = Xs + BK * BN;        // [4][BM]: scale, shift, scale2, shift2 of the tile's channels

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
    if (MODE == 2) { Cs[2 * BM + tid] = P.scale2[ch]; Cs[3 * BM + tid] = P.shift2[ch]; }
  }

  // what this thread stages: float4 `i` of a K step is row idx / (B? / 4), columns 4 (idx % (B? / 4)) .. + 3
  float4 wr[WV], xr[XV];
  int wcol[WV], xcol[XV];          // clamped column of the float4 inside the tensor; the mask is recomputed when it is written
#pragma unroll
  for (int i = 0; i < WV; i++) wcol[i] = min(m0 + ((tid + i * kThreads) % (BM / 4)) * 4, cout - 4);
#pragma unroll
  for (int i = 0; i < XV; i++) xcol[i] = p0 + ((tid + i * kThreads) % (BN / 4)) * 4;

  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < WV; i++) {
      const int row = (tid + i * kThreads) / (BM / 4);
      wr[i] = *reinterpret_cast<const float4*>(P.wt + (size_t)(k0 + row) * cout + wcol[i]);
    }
#pragma unroll
    for (int i = 0; i < XV; i++) {
      const int row = (tid + i * kThreads) / (BN / 4);
      const float* src = xb + (size_t)(k0 + row) * hw;
      if (VEC) {
        xr[i] = *reinterpret_cast<const float4*>(src + min(xcol[i], hw - 4));
      } else {
        xr[i].x = src[min(xcol[i], hw - 1)]; xr[i].y = src[min(xcol[i] + 1, hw - 1)];
        xr[i].z = src[min(xcol[i] + 2, hw - 1)]; xr[i].w = src[min(xcol[i] + 3, hw - 1)];
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < WV; i++) {
      const int idx = tid + i * kThreads;
      float4 v = wr[i];
      if (m0 + (idx % (BM / 4)) * 4 >= cout) v = make_float4(0.f, 0.f, 0.f, 0.f);      // (Cout % 4 == 0: all four in or out)
      *reinterpret_cast<float4*>(Ws + (idx / (BM / 4)) * BM + (idx % (BM / 4)) * 4) = v;
    }
#pragma unroll
    for (int i = 0; i < XV; i++) {
      const int idx = tid + i * kThreads;
      float4 v = xr[i];
      const int p = xcol[i];
      if (p >= hw) v.x = 0.f;
      if (p + 1 >= hw) v.y = 0.f;
      if (p + 2 >= hw) v.z = 0.f;
      if (p + 3 >= hw) v.w = 0.f;
      *reinterpret_cast<float4*>(Xs + (idx / (BN / 4)) * BN + (idx % (BN / 4)) * 4) = v;
    }
  };

  const int lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int wm0 = (wave >> 1) * 32 * WM, wn0 = (wave & 1) * 32 * WN;      // the wave's corner inside the workgroup tile
  f32x16 acc[WM][WN];
#pragma unroll
  for (int mi = 0; mi < WM; mi++)
#pragma unroll
    for (int ni = 0; ni < WN; ni++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[mi][ni][r] = 0.f;

  auto mma = [&]() {
    const float* wa = Ws + half * BM + wm0 + l31;
    const float* xa = Xs + half * BN + wn0 + l31;
#pragma unroll
    for (int kk = 0; kk < BK / 2; kk++) {
      float a[WM], bb[WN];
#pragma unroll
      for (int mi = 0; mi < WM; mi++) a[mi] = wa[kk * 2 * BM + mi * 32];
#pragma unroll
      for (int ni = 0; ni < WN; ni++) bb[ni] = xa[kk * 2 * BN + ni * 32];
#pragma unroll
      for (int mi = 0; mi < WM; mi++)
#pragma unroll
        for (int ni = 0; ni < WN; ni++) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi], bb[ni], acc[mi][ni], 0, 0, 0);
    }
  };

  const int nk = P.cin / BK;
  fetch(0);
  stage();
  __syncthreads();
  for (int t = 0; t + 1 < nk; t++) {
    fetch((t + 1) * BK);
    __builtin_amdgcn_sched_barrier(0);      // the requests go out in front of the MFMAs (the scheduler otherwise sinks them behind)
    mma();
    __builtin_amdgcn_sched_barrier(0);      // ... and nothing that waits for them moves up between the MFMAs
    __syncthreads();          // every wave has read step t
    stage();
    __syncthreads();
  }

  // Epilogue addressing.  Register r of tile (mi, ni) is channel m0 + wm0 + 32 mi + 8 (r >> 2) + 4 half + (r & 3) at position
  // p0 + wn0 + 32 ni + l31: a store instruction writes 32 consecutive positions of two channels.
  const size_t plane0 = (size_t)b * cout;
  float rv[WM][WN][16];
  if (MODE) {               // requested before the last K step's MFMAs (clamped addresses: no branch per load)
#pragma unroll
    for (int mi = 0; mi < WM; mi++)
#pragma unroll
      for (int ni = 0; ni < WN; ni++) {
        const int p = min(p0 + wn0 + 32 * ni + l31, hw - 1);
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const int ch = min(m0 + wm0 + 32 * mi + 8 * (r >> 2) + 4 * half + (r & 3), cout - 1);
          rv[mi][ni][r] = P.res[(plane0 + ch) * hw + p];
        }
      }
  }
  __builtin_amdgcn_sched_barrier(0);
  mma();

  unsigned rmax = 0u;
#pragma unroll
  for (int mi = 0; mi < WM; mi++) {
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int chg = m0 + wm0 + 32 * mi + 8 * g + 4 * half;          // four consecutive channels (Cout % 4 == 0: all in or out)
      const float* cs = Cs + wm0 + 32 * mi + 8 * g + 4 * half;
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
          const float v = acc[mi][ni][r];
          float t;
          if (MODE == 0) t = affine_act(v, av[q], bv[q], P.relu);
          else if (MODE == 1) t = affine_res_act(v, av[q], bv[q], rv[mi][ni][r], P.relu);
          else t = affine_res_act(v, av[q], bv[q], affine_act(rv[mi][ni][r], a2v[q], b2v[q], 0), P.relu);
          if (chg < cout && p < hw) {
            P.y[(plane0 + chg + q) * hw + p] = t;
            if (RANGE) rmax = max(rmax, orp::range_bits(t));
          }
        }
      }
    }
  }
  if (RANGE) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rmax = max(rmax, (unsigned)__shfl_xor((int)rmax, o, 64));
    unsigned* red = reinterpret_cast<unsigned*>(Ws);          // (free once every wave is behind its last MFMAs)
    __syncthreads();
    if (lane == 0) red[wave] = rmax;
    __syncthreads();
    if (tid == 0) orp::range_raise(P.range, max(max(red[0], red[1]), max(red[2], red[3])));
  }
}

using orp_c1x1::Tile;

// the workgroup tile of a launch: the largest one that still gives the 256 CUs two workgroups each, else the smallest
Tile pick_tile(int cout, int hw, int batch) {
  const Tile cand[3] = {{128, 128}, {64, 128}, {64, 64}};
  for (int i = 0; i < 3; i++) {
    const Tile t = cand[i];
    if (t.bm > ((cout + 63) / 64) * 64) continue;
    const long wgs = (long)((cout + t.bm - 1) / t.bm) * ((hw + t.bn - 1) / t.bn) * batch;
    if (wgs >= 512) return t;
  }
  return cand[2];
}

template <int WM, int WN>
void launch(const Args& A, int batch, bool vec, hipStream_t st) {
  orp_c1x1::dispatch(A, vec, [&](auto mode, auto range, auto v) {
    hipLaunchKernelGGL((conv1x1_bn_act_kernel<WM, WN, decltype(v)::value, decltype(mode)::value, decltype(range)::value>),
                       orp_c1x1::grid_of(A, batch), dim3(kThreads), 0, st, A);
  });
}

}  // namespace

extern "C" {

int orp_conv1x1_bn_act_ok(int c_in, int c_out) {
  return (c_in >= 64 && c_in <= 2048 && c_in % 32 == 0 && c_out >= 64 && c_out <= 4096 && c_out % 32 == 0) ? 1 : 0;
}

// the workgroup tile (channels x positions) a launch of this shape runs with; 0 where the shape is not supported
int orp_conv1x1_bn_act_tile(int c_in, int c_out, int hw, int batch, int* tile_channels, int* tile_positions) {
  if (!orp_conv1x1_bn_act_ok(c_in, c_out) || hw <= 0 || batch <= 0) return 0;
  const Tile t = pick_tile(c_out, hw, batch);
  if (tile_channels) *tile_channels = t.bm;
  if (tile_positions) *tile_positions = t.bn;
  return 1;
}

// THE routing rule: where the fused launch was measured faster than library convolution + pass on MI355X (slowest fused run against
// fastest library run, tests/checks/time_bottleneck_1x1.py; docs/notebook/round12.md has the tables).  Three points were timed per
// (Cin, Cout) pair: the R-50 map of a 1024^2 image with one image and with two, and the map of a 1536^2 image with one image.  A row
// is a closed range: one image from the 1024^2 map to the 1536^2 map where both ends paid (map sizes between the two are the one
// interpolation this table makes), two images at the 1024^2 map only.  Nothing beyond the timed corners is routed.  Both residual
// forms paid wherever one did, so has_residual does not enter.  The matrix-bound pairs win by the pass they absorb, a few
// microseconds, and the library's GEMMs gain more from a second image or a larger map than this kernel does, hence their
// narrower rows.  Measured and lost everywhere, hence absent: 512 -> 256, 1024 -> 512 and 2048 -> 512 (conv1 of the first blocks
// of stages 3 and 4, stage 4's other conv1).
int orp_conv1x1_bn_act_pays(int c_in, int c_out, int hw, int batch, int has_residual) {
  if (!orp_conv1x1_bn_act_ok(c_in, c_out) || hw <= 0 || batch <= 0) return 0;
  (void)has_residual;
  static const orp_c1x1::PaidRow paid[] = {
      {64, 64, 65536, 147456, 1},   {64, 64, 65536, 65536, 2},        // stage 1: conv1 of block 0
      {256, 64, 65536, 147456, 1},  {256, 64, 65536, 65536, 2},       //          conv1 of the others
      {64, 256, 65536, 147456, 1},  {64, 256, 65536, 65536, 2},       //          conv3
      {256, 128, 65536, 147456, 1}, {256, 128, 65536, 65536, 2},      // stage 2: conv1 of block 0
      {512, 128, 16384, 36864, 1},                                    //          conv1 of the others
      {128, 512, 16384, 36864, 1},  {128, 512, 16384, 16384, 2},      //          conv3
      {1024, 256, 4096, 4096, 1},                                     // stage 3: conv1 of blocks 1..
      {256, 1024, 4096, 9216, 1},   {256, 1024, 4096, 4096, 2},       //          conv3
      {512, 2048, 1024, 1024, 1},                                     // stage 4: conv3
  };
  return orp_c1x1::paid(paid, c_in, c_out, hw, batch);
}

// range_out (or NULL): the range word, as orp_c1x1::run describes it
int orp_conv1x1_bn_act_range(const float* x, const float* weight_t, const float* scale, const float* shift, const float* residual,
                             const float* scale2, const float* shift2, float* y, int batch, int c_in, int c_out, int hw, int relu,
                             uint32_t* range_out, void* stream) {
  return orp_c1x1::run<Args>(x, weight_t, scale, shift, residual, scale2, shift2, y, batch, c_in, c_out, hw, relu, range_out, stream,
                             orp_conv1x1_bn_act_ok(c_in, c_out) != 0, pick_tile, [&](Args& A, Tile t, bool vec, hipStream_t st) {
    A.wt = weight_t;
    if (t.bm == 128) launch<2, 2>(A, batch, vec, st);
    else if (t.bn == 128) launch<1, 2>(A, batch, vec, st);
    else launch<1, 1>(A, batch, vec, st);
  });
}

int orp_conv1x1_bn_act(const float* x, const float* weight_t, const float* scale, const float* shift, const float* residual,
                       const float* scale2, const float* shift2, float* y, int batch, int c_in, int c_out, int hw, int relu,
                       void* stream) {
  return orp_conv1x1_bn_act_range(x, weight_t, scale, shift, residual, scale2, shift2, y, batch, c_in, c_out, hw, relu, nullptr, stream);
}

}  // extern "C"
