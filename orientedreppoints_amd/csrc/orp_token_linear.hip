// orp_token_linear.hip -- a per-token linear layer with its epilogue, on the 16-bit matrix pipe (gfx950, inference):
//
//   y[t][n] = epi( sum_k x[t][k] w[n][k] ),   epi(v) = act(v + bias[n]) + res[t][n]
//
// x [T][K], w [N][K] (nn.Linear's layout), y and res [T][N], all fp32 with contiguous rows; bias and res optional; act = identity or the
// exact GELU 0.5 u (1 + erff(u sqrt(1/2))).  What a Swin block runs four times (attn.qkv, attn.proj + residual, mlp.fc1 + GELU, mlp.fc2 +
// residual) and PatchMerging once: with the epilogue here the hidden tensor is written once and never re-read by a GELU or an addition.
//
// The arithmetic is orp_conv1x1_bn_pieces.hip's: every fp32 operand is split EXACTLY into three bf16 pieces by truncation
// (orp_dcn_split.hpp: split_pair), and x w becomes the six products x2 w0, x0 w2, x1 w1, x1 w0, x0 w1, x0 w0 (smallest first; x1 w2, x2 w1
// and x2 w2, each at most 2^-24 |x w|, are dropped) on v_mfma_f32_32x32x16_bf16.  Each product of pieces is exact in the fp32 accumulator;
// bf16 carries fp32's exponent, so nothing is scaled.  Every output has ONE accumulator fed in a fixed order -- ascending 16-wide K
// chunks, the six products of a chunk in the order above: no split-K, no atomics, and the value of an output does not depend on T, on
// the tile it falls in or on the launch it is part of.  The epilogue is plain fp32 in the order written above.
//
// Non-finite x: the split of +-inf leaves inf - inf, so an infinite x gives NaN where fp32 gives +-inf (and a zero piece of a weight
// times an infinite piece is NaN as well).  The outputs of that TOKEN are non-finite, of possibly another class than fp32's; no other
// token's row is touched: the rows of the product are independent and no cross-lane operation sits in the K loop.
//
// Tokens are the MFMA rows and output channels its columns, so a store instruction writes 32 consecutive channels (128 bytes) of two tokens.
//   * weights: packed once per weight tensor (orp_token_linear_pack_weight: orp_dcn_split.hip's bf16 packer at one tap) into three bf16
//     planes [plane][K/16][2][N][8]: one 16-byte load is the 8 k-values of an MFMA lane.  They go from L2 straight into a register ring of
//     one K step, refilled in place right behind their use.
//   * activations: K runs in steps of 32 (128-token tiles) or 64.  A token row is K-contiguous: a thread fetches four consecutive k of one
//     token (one 16-byte load; 8 or 16 lanes cover a row's K step), splits them in registers and writes each plane's two packed dwords to
//     LDS as [token][K step + 8] bf16 -- the row stride of 20 or 36 dwords = 4 x odd that puts the 16 rows of every ds_read_b128 lane group
//     on 16 different 16-byte slots.  LDS is double buffered: step t + 1 is written while step t is contracted, one barrier per step; the
//     loads of step t + 2 are in flight meanwhile.
//   * one workgroup = 4 waves = 128 channels x 128, 64 or 32 tokens; each wave owns 32 channels and all tokens of the tile, so no weight is
//     fetched twice by a workgroup.  N need not fill the tile (N = 96, 288): a wave whose channels lie past N stages activations and
//     contracts nothing.  T is arbitrary: on the last tile loads are clamped and zeroed, stores masked.  K need not be a whole number of
//     K steps (K = 96 with the 64-wide step): the chunks past K of the last step are not contracted and no weight past K is read.
//   * the residual of a wave's outputs is requested before the last K step's MFMAs (64 or 32 tokens per wave; behind them at 128).
// LDS 27 - 60 KB: two workgroups per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orp_hip.h"
#include "orp_launch.hpp"
#include "orp_dcn_split.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kTileN = 128;        // channels of a workgroup tile: 4 waves x 32

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));

using orp_split::split_pair;

struct Args {
  const float* x;                  // [T][K]
  const uint16_t* planes;          // three bf16 planes [pl][K/16][2][N][8]
  size_t plane_stride;             // elements between two planes
  const float* bias;               // [N] or NULL
  const float* res;                // [T][N] or NULL
  float* y;                        // [T][N]
  int T, K, N;
  int ntn;                         // channel tiles (the token tiles are the grid's other factor)
};

__device__ __forceinline__ float gelu_exact(float u) { return 0.5f * u * (1.f + erff(u * 0.70710678118654752440f)); }

// WN: 32-token blocks per wave (tile of 32 WN tokens x 128 channels).  BK: channels of a K step.  ACT: 1 = GELU.  RES: a residual is added.
template <int WN, int BK, int ACT, bool RES>
__global__ void __launch_bounds__(kThreads, 2)
token_linear_kernel(const Args P) {
  constexpr int ASTR = BK + 8;       // bf16 elements per token row in LDS: 20 or 36 dwords = 4 x odd
  constexpr int NCH = BK / 16;       // MFMA chunks of 16 k per K step
  constexpr int BT = 32 * WN;
  constexpr int PLANE = BT * ASTR, BUF = 3 * PLANE;            // bf16 elements
  constexpr int QPR = BK / 4;                                  // 16-byte quads of a token row per K step
  constexpr int ITEMS = BT * QPR;
  constexpr int XV = ITEMS / kThreads;
  static_assert(ITEMS % kThreads == 0, "every thread stages the same number of quads");
  __shared__ __align__(16) uint16_t lds[2 * BUF];

  const int tid = threadIdx.x;
  const int bid = blockIdx.x;
  const int nt = bid % P.ntn, tt = bid / P.ntn;      // (neighbouring workgroups share the token tile: it stays in L2)
  const int n0 = nt * kTileN, t0 = tt * BT;
  const int T = P.T, K = P.K, N = P.N;
  const int nchunks = K / 16;
  const int nk = (K + BK - 1) / BK;

  const int lane = tid & 63, wave = tid >> 6;
  const int kg = lane >> 5, l31 = lane & 31;
  const int nb = n0 + 32 * wave;                     // the wave's 32 channels
  const bool live = nb < N;                          // (N % 32 == 0: a wave is live or idle as a whole)

  // ---- weights: lane (channel, k-group) reads the 8 k-values of a chunk per plane; a register ring of one K step ----
  const uint16_t* wp = P.planes + ((size_t)kg * N + min(nb + l31, N - 1)) * 8;
  const size_t wblk = (size_t)2 * N * 8;
  bf8 wq[NCH][3];
  auto load_w = [&](int t, int c) {                  // (past K the last chunk is read again and never used)
    const uint16_t* a = wp + (size_t)min(t * NCH + c, nchunks - 1) * wblk;
#pragma unroll
    for (int pl = 0; pl < 3; pl++) wq[c][pl] = *reinterpret_cast<const bf8*>(a + (size_t)pl * P.plane_stride);
  };
#pragma unroll
  for (int c = 0; c < NCH; c++) load_w(0, c);

  // ---- activations: item idx of a K step = k-quad idx % QPR of token idx / QPR: QPR consecutive lanes read one token's 4 BK bytes ----
  float4 xr[2][XV];                // two K steps in flight: step t + 2 is requested while step t is contracted
  const float* xsrc[XV];
  int xkq[XV];
#pragma unroll
  for (int i = 0; i < XV; i++) {
    const int idx = tid + i * kThreads;
    xkq[i] = idx % QPR;
    xsrc[i] = P.x + (size_t)min(t0 + idx / QPR, T - 1) * K;
  }
  auto fetch = [&](int k0, float4 (&xr)[XV]) {
#pragma unroll
    for (int i = 0; i < XV; i++) xr[i] = *reinterpret_cast<const float4*>(xsrc[i] + min(k0 + 4 * xkq[i], K - 4));
  };
  auto stage = [&](int buf, const float4 (&xr)[XV]) {
#pragma unroll
    for (int i = 0; i < XV; i++) {
      const int tok = (tid + i * kThreads) / QPR;
      const bool in = t0 + tok < T;
      unsigned d01[3], d23[3];
      split_pair(in ? xr[i].x : 0.f, in ? xr[i].y : 0.f, d01);
      split_pair(in ? xr[i].z : 0.f, in ? xr[i].w : 0.f, d23);
      unsigned* dst = reinterpret_cast<unsigned*>(lds + buf * BUF) + tok * (ASTR / 2) + 2 * xkq[i];
#pragma unroll
      for (int pl = 0; pl < 3; pl++) *reinterpret_cast<uint2*>(dst + pl * (PLANE / 2)) = make_uint2(d01[pl], d23[pl]);
    }
  };

  f32x16 acc[WN];
#pragma unroll
  for (int ni = 0; ni < WN; ni++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[ni][r] = 0.f;

  // one K step out of buffer `buf`, its first `nc` chunks (NCH but in a ragged last step); the weights of chunk c are refilled for
  // step t_next right behind their use
  auto mma = [&](int buf, int nc, int t_next) {
    if (!live) return;
    const uint16_t* xa = lds + buf * BUF + l31 * ASTR + 8 * kg;
    auto load_x = [&](int c, bf8 (&q)[WN][3]) {
#pragma unroll
      for (int ni = 0; ni < WN; ni++)
#pragma unroll
        for (int pl = 0; pl < 3; pl++) q[ni][pl] = *reinterpret_cast<const bf8*>(xa + pl * PLANE + ni * 32 * ASTR + c * 16);
    };
    // the narrow tiles read a chunk's fragments one chunk ahead (orp_conv1x1_bn_pieces.hip: six or twelve MFMAs do not hide an LDS
    // read behind themselves); at 128 tokens per wave the registers go to the accumulators instead
    constexpr bool AHEAD = WN <= 2;
    bf8 xqs[AHEAD ? 2 : 1][WN][3];
    load_x(0, xqs[0]);
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      bf8 (&xq)[WN][3] = xqs[AHEAD ? (c & 1) : 0];
      if (AHEAD) { if (c + 1 < NCH) load_x(c + 1, xqs[(c + 1) & 1]); }
      else if (c > 0) load_x(c, xqs[0]);
      __builtin_amdgcn_sched_barrier(0);
      if (c < nc) {
        // D[token][channel]; smallest products first
#pragma unroll
        for (int ni = 0; ni < WN; ni++) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xq[ni][2], wq[c][0], acc[ni], 0, 0, 0);
#pragma unroll
        for (int ni = 0; ni < WN; ni++) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xq[ni][0], wq[c][2], acc[ni], 0, 0, 0);
#pragma unroll
        for (int ni = 0; ni < WN; ni++) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xq[ni][1], wq[c][1], acc[ni], 0, 0, 0);
#pragma unroll
        for (int ni = 0; ni < WN; ni++) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xq[ni][1], wq[c][0], acc[ni], 0, 0, 0);
#pragma unroll
        for (int ni = 0; ni < WN; ni++) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xq[ni][0], wq[c][1], acc[ni], 0, 0, 0);
#pragma unroll
        for (int ni = 0; ni < WN; ni++) acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xq[ni][0], wq[c][0], acc[ni], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      load_w(t_next, c);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // Step t (not the last): request step t + 2 into the register set step t's data left, contract step t out of buffer t & 1, write
  // step t + 1 (requested a step ago) into the other buffer -- its last readers are behind the previous barrier -- one barrier.
  // Every load is unconditional (past the end the last step is requested again), so the compiler's vmcnt counts are exact.
  auto step = [&](int t, float4 (&cur)[XV], float4 (&nxt)[XV], int buf) {
    fetch(min(t + 2, nk - 1) * BK, cur);
    __builtin_amdgcn_sched_barrier(0);      // the requests go out in front of the MFMAs
    mma(buf, NCH, t + 1);
    stage(buf ^ 1, nxt);
    __syncthreads();
  };
  fetch(0, xr[0]);
  stage(0, xr[0]);
  fetch(min(1, nk - 1) * BK, xr[1]);
  __syncthreads();
  int t = 0;
  for (; t + 2 < nk; t += 2) {
    step(t, xr[0], xr[1], 0);
    step(t + 1, xr[1], xr[0], 1);
  }
  if (t + 1 < nk) step(t, xr[0], xr[1], 0);

  // Epilogue addressing.  Register r of block ni is token t0 + 32 ni + 8 (r >> 2) + 4 kg + (r & 3) at channel nb + l31.
  if (!live) return;                // (behind the last barrier)
  const int n = nb + l31;
  // The residual of a wave's outputs is requested before the last K step's MFMAs (clamped addresses: no branch per load); at 128 tokens
  // per wave those 64 registers do not fit next to the accumulators, and each 32-token block requests its own behind the MFMAs.
  constexpr bool EARLY = RES && WN <= 2;
  float rv[EARLY ? WN : 1][16];
  auto load_res = [&](int ni, float (&v)[16]) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int tk = min(t0 + 32 * ni + 8 * (r >> 2) + 4 * kg + (r & 3), T - 1);
      v[r] = P.res[(size_t)tk * N + n];
    }
  };
  if (EARLY) {
#pragma unroll
    for (int ni = 0; ni < WN; ni++) load_res(ni, rv[ni]);
  }
  const bool has_bias = P.bias != nullptr;
  const float bv = has_bias ? P.bias[n] : 0.f;
  __builtin_amdgcn_sched_barrier(0);
  mma((nk - 1) & 1, nchunks - (nk - 1) * NCH, nk - 1);

#pragma unroll
  for (int ni = 0; ni < WN; ni++) {
    float late[16];
    if (RES && !EARLY) load_res(ni, late);
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int tk = t0 + 32 * ni + 8 * (r >> 2) + 4 * kg + (r & 3);
      float u = acc[ni][r];
      if (has_bias) u = u + bv;
      if (ACT == 1) u = gelu_exact(u);
      if (RES) u = u + (EARLY ? rv[EARLY ? ni : 0][r] : late[r]);
      if (tk < T) P.y[(size_t)tk * N + n] = u;
    }
  }
}

// the token tile of a launch: the widest that still gives the 256 CUs two workgroups each, else the narrowest
int pick_tokens(long T, int N) {
  const long ntn = (N + kTileN - 1) / kTileN;
  const int cand[3] = {128, 64, 32};
  for (int i = 0; i < 3; i++)
    if (ntn * ((T + cand[i] - 1) / cand[i]) >= 512) return cand[i];
  return 32;
}

template <int WN, int BK>
void launch(const Args& A, unsigned grid, int act, hipStream_t st) {
  if (act == 1) {
    if (A.res) hipLaunchKernelGGL((token_linear_kernel<WN, BK, 1, true>), dim3(grid), dim3(kThreads), 0, st, A);
    else hipLaunchKernelGGL((token_linear_kernel<WN, BK, 1, false>), dim3(grid), dim3(kThreads), 0, st, A);
  } else {
    if (A.res) hipLaunchKernelGGL((token_linear_kernel<WN, BK, 0, true>), dim3(grid), dim3(kThreads), 0, st, A);
    else hipLaunchKernelGGL((token_linear_kernel<WN, BK, 0, false>), dim3(grid), dim3(kThreads), 0, st, A);
  }
}

}  // namespace

extern "C" {

int orp_token_linear_ok(int k, int n) {
  return (k >= 32 && k <= 8192 && k % 32 == 0 && n >= 32 && n <= 16384 && n % 32 == 0) ? 1 : 0;
}

// THE routing rule of the token linear: where its launch was measured faster than the stock span it replaces -- the library's GEMM plus
// its GELU or residual kernels -- on MI355X, slowest run of this kernel against the fastest stock run (tests/checks/time_token_linear.py;
// docs/notebook/round29.md has the tables).  A closed table: the four linears of a block of every Swin-T stage and the three merges were
// timed with their own epilogue at the token counts of one 1024^2 image and of one 1536^2 image; a row routes T from the first to the
// second where both ends paid.  Nothing beyond a timed corner is routed, and no epilogue that was not timed with the shape.  36 of the
// 38 timed points paid.  The two that lost, both at the 1024^2 image's 1024 tokens and N = 768, where 192 workgroups of 32 tokens do not
// fill the 256 CUs and each walks a long K alone: stage 4's fc2 (K = 3072: 56 us against 47) and stage 3's merge (K = 1536: 29 us against
// 25); only their 1536^2 corner is routed.
int orp_token_linear_pays(long tokens, int k, int n, int epilogue) {
  if (!orp_token_linear_ok(k, n) || tokens <= 0 || epilogue < 0 || epilogue > 7) return 0;
  struct Row { int k, n, epilogue; long t_min, t_max; };
  enum { QKV = 1, FC1 = 3, RES = 5, MERGE = 0 };        // bias | bias + GELU | bias + residual (proj, fc2) | nothing
  static const Row paid[] = {
      {96, 288, QKV, 65536, 147456},  {96, 96, RES, 65536, 147456},  {96, 384, FC1, 65536, 147456},  {384, 96, RES, 65536, 147456},   // stage 1
      {384, 192, MERGE, 16384, 36864},
      {192, 576, QKV, 16384, 36864},  {192, 192, RES, 16384, 36864}, {192, 768, FC1, 16384, 36864},  {768, 192, RES, 16384, 36864},   // stage 2
      {768, 384, MERGE, 4096, 9216},
      {384, 1152, QKV, 4096, 9216},   {384, 384, RES, 4096, 9216},   {384, 1536, FC1, 4096, 9216},   {1536, 384, RES, 4096, 9216},    // stage 3
      {1536, 768, MERGE, 2304, 2304},
      {768, 2304, QKV, 1024, 2304},   {768, 768, RES, 1024, 2304},   {768, 3072, FC1, 1024, 2304},   {3072, 768, RES, 2304, 2304},    // stage 4
  };
  for (const Row& r : paid)
    if (r.k == k && r.n == n && r.epilogue == epilogue && tokens >= r.t_min && tokens <= r.t_max) return 1;
  return 0;
}

// the packed weight: three bf16 planes [3][K/16][2][N][8] (6 bytes per weight)
size_t orp_token_linear_packed_bytes(int k, int n) { return orp_token_linear_ok(k, n) ? (size_t)6 * k * n : 0; }

// orp_dcn_split.hip's bf16 packer at one tap: the same split, element order and layout ([N][K] is its [Cout][Cin][1])
int orp_token_linear_pack_weight(const float* weight, int k, int n, void* packed, void* stream) {
  if (!weight || !packed || ((uintptr_t)weight & 15) || ((uintptr_t)packed & 15) || !orp_token_linear_ok(k, n)) return ORP_EINVAL;
  hipError_t e = orp_split::pack_planes_bf16(weight, n, k, 1, reinterpret_cast<uint16_t*>(packed), (hipStream_t)stream);
  return e == hipSuccess ? ORP_OK : (int)e;
}

int orp_token_linear(const float* x, const void* weight_packed, const float* bias, const float* residual, float* y, long tokens, int k,
                     int n, int act, void* stream) {
  if (!x || !weight_packed || !y || tokens < 0 || !orp_token_linear_ok(k, n) || (act != 0 && act != 1)) return ORP_EINVAL;
  if (((uintptr_t)x & 15) || ((uintptr_t)weight_packed & 15) || ((uintptr_t)y & 15) || ((uintptr_t)bias & 15) || ((uintptr_t)residual & 15))
    return ORP_EINVAL;
  if ((const float*)y == x || (const float*)y == residual) return ORP_EINVAL;
  if (tokens == 0) return ORP_OK;
  if (tokens >= (1L << 31) - 128) return ORP_ETOOBIG;
  const int bt = pick_tokens(tokens, n);
  Args A{};
  A.x = x; A.planes = reinterpret_cast<const uint16_t*>(weight_packed); A.plane_stride = (size_t)k * n;
  A.bias = bias; A.res = residual; A.y = y;
  A.T = (int)tokens; A.K = k; A.N = n;
  A.ntn = (n + kTileN - 1) / kTileN;
  const long wgs = (long)A.ntn * ((tokens + bt - 1) / bt);
  if (wgs >= (1L << 31)) return ORP_ETOOBIG;
  hipStream_t st = (hipStream_t)stream;
  if (bt == 128) launch<4, 32>(A, (unsigned)wgs, act, st);
  else if (bt == 64) launch<2, 64>(A, (unsigned)wgs, act, st);
  else launch<1, 64>(A, (unsigned)wgs, act, st);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? ORP_OK : (int)e;
}

}  // extern "C"
