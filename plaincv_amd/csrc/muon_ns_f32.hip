// plaincv_amd/csrc/muon_ns_f32.hip -- Muon's Newton-Schulz chain in exact fp32, on many CUs.
//
// optax.contrib.muon orthogonalises in the parameter dtype (fp32 in every reference config); the
// default path here runs the chain on bf16 MFMA operands (muon_fused.hip, optim/muon.py).  This
// file is the opt-in Muon(ns_dtype="float32") chain: every product on v_mfma_f32_16x16x4_f32
// (bit-for-bit a k-ordered fp32 fma chain).  An fp32 X, A and B of one 128 x 256 matrix do not fit
// one CU's LDS, and one CU would serialise ~40 M MACs per matrix, so each NS phase is ONE launch
// over 32 x 32 output tiles of ALL routed matrices (a device tile table built once by Muon.init:
// tile -> matrix, tile row, tile column; first the upper-triangle tiles of the r' x r' products,
// then the r' x c' tiles of the update):
//
//   gram    A  = X X^T            K = c'   upper-triangle tiles, mirrored on store
//   poly    B  = b A + c A A      K = r'   same tiling; A = A^T, so both operands are read along k
//   update  X' = a X + B X        K = r'   X ping-pongs x0 -> x1 -> x0 ...; the last iteration
//                                          writes the fixed output buffer `out`
//
// With nine ViT matrices a launch has ~90 / ~288 tiles on 256 CUs: the per-tile k chain is the
// critical path, not throughput.  So, as gemm_f32_small_kernel (precond.hip) does, a tile is
// 32 x 32, the workgroup's eight waves split K, each wave feeds its MFMAs straight from global
// memory (one float4 along k per lane and 16-long k slab, contraction index 4 g + q inside a slab
// for both operands), and the eight partial tiles are summed in LDS in wave order.  No atomics;
// every sum has a fixed order: two runs give the same bits.
//
// The update's second operand X is summed over its ROW index.  Lane (g, r16) reads the float2
// X[k0 + 4 g + q][n0 + 2 r16 .. + 1] for q = 0..3 (128 contiguous bytes per 16 lanes): element e of
// the pair is the B operand of column sub-tile e, i.e. sub-tile e holds the tile's columns
// 2 j + e.  Only the staging index of the partial tile knows about that permutation.
//
// Normalisation is folded into iteration 0: pcv_muon_prep (or the split step's gradient phase)
// leaves x0 un-normalised with its squared norm in the fp64 slots; iteration 0 multiplies every
// loaded element of x0 by inv = 1 / (||x0||_F + eps) (muon_inv_norm), which is bit-for-bit
// normalising first.  ns_steps = 0 takes one scale-only launch (out = inv x0).
//
// Ragged shapes: rows / columns past the matrix are loaded as zero (per element along k, so K need
// not be a multiple of 4 or 16) and never stored.  Row strides are multiples of 4 floats.
#include "common.h"
#include "optim_types.h"

namespace pcv {
namespace {

constexpr int NF_T = 32;                  // tile edge
constexpr int NF_LD = NF_T + 1;
constexpr int NF_WAVES = 8;               // K split over the workgroup's waves
constexpr int NF_THREADS = 64 * NF_WAVES;
constexpr int NF_SLABS = 4;               // 16-long k slabs per load batch

// One routed matrix's NS workspaces (pcv_muon_ns_f32_rec_size() bytes; built by optim/muon.py).
struct NsMat {
  float *x0, *x1;        // X ping-pong [r'][ldx]; x0 is the MuonMat's x32 (written by the prep)
  float *A, *B;          // [r'][lda]
  float* out;            // X_ns [r'][ldx]: the MuonMat's xo under the *_f32 consumers
  const double* norm2;   // the MuonMat's MUON_NSLOT norm slots
  int r, c, ldx, lda;    // r' = min, c' = max of the kernel shape; row strides (multiples of 4)
};
static_assert(sizeof(NsMat) == 64, "NsMat layout is mirrored by optim/muon.py");

struct NsTile { int mat, tm, tn, pad; };

enum { NS_GRAM = 0, NS_POLY = 1, NS_UPD = 2 };

__device__ __forceinline__ float ns_inv_norm(const NsMat& M, float eps, double* sh) {
  MuonMat mm{};
  mm.norm2 = const_cast<double*>(M.norm2);
  return muon_inv_norm(mm, eps, sh);
}

// rows of a row-major image along k: float4 at [row][k .. k+3], zero outside rows / [.., ke)
__device__ __forceinline__ float4 ns_ld_k(const float* __restrict__ P, int ld, int row, int nrows, int k, int ke,
                                          float xs) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row < nrows && k < ke) {
    v = *reinterpret_cast<const float4*>(P + (int64_t)row * ld + k);   // k % 4 == 0, ld % 4 == 0: inside the row
    v.x *= xs;
    v.y = k + 1 < ke ? v.y * xs : 0.f;
    v.z = k + 2 < ke ? v.z * xs : 0.f;
    v.w = k + 3 < ke ? v.w * xs : 0.f;
  }
  return v;
}

template <int PH>
__global__ __launch_bounds__(NF_THREADS) void ns_phase_kernel(const NsMat* __restrict__ mats,
                                                              const NsTile* __restrict__ tiles, int it, int last,
                                                              float eps, float ca, float cb, float cc) {
  __shared__ __attribute__((aligned(16))) float part[NF_WAVES][NF_T][NF_LD];
  const NsTile tl = tiles[blockIdx.x];
  const NsMat M = mats[tl.mat];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, r16 = lane & 15, g = lane >> 4;
  // iteration 0 reads the un-normalised x0: scale it on load
  float xs = 1.f;
  if (PH != NS_POLY && it == 0) xs = ns_inv_norm(M, eps, reinterpret_cast<double*>(&part[0][0][0]));
  const float* __restrict__ Xs = (it & 1) ? M.x1 : M.x0;   // this iteration's X
  const int m0 = tl.tm * NF_T, n0 = tl.tn * NF_T;
  const int Mr = M.r;                                       // output rows: r' in every phase
  const int Nc = PH == NS_UPD ? M.c : M.r;                  // output columns
  const int K = PH == NS_GRAM ? M.c : M.r;
  const float* __restrict__ P = PH == NS_GRAM ? Xs : (PH == NS_POLY ? M.A : M.B);
  const int ldp = PH == NS_GRAM ? M.ldx : M.lda;
  const float ps = PH == NS_GRAM ? xs : 1.f;
  // this wave's K range: whole 16-long slabs
  const int kq = (((K + NF_WAVES - 1) / NF_WAVES) + 15) & ~15;
  const int kb = w * kq, ke = min(K, kb + kq);
  f32x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = kb; k0 < ke; k0 += 16 * NF_SLABS) {
    float4 fa[NF_SLABS][2], fb[NF_SLABS][2];
#pragma unroll
    for (int sl = 0; sl < NF_SLABS; ++sl) {
      const int k = k0 + 16 * sl + 4 * g;
#pragma unroll
      for (int a = 0; a < 2; ++a) fa[sl][a] = ns_ld_k(P, ldp, m0 + 16 * a + r16, Mr, k, ke, ps);
      if (PH != NS_UPD) {
#pragma unroll
        for (int b = 0; b < 2; ++b) fb[sl][b] = ns_ld_k(P, ldp, n0 + 16 * b + r16, Nc, k, ke, ps);
      } else {
        // X[k + q][n0 + 2 r16 + e]: (&fb[sl][e].x)[q]
        const int col = n0 + 2 * r16;
        float* f0 = &fb[sl][0].x;
        float* f1 = &fb[sl][1].x;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float2 v = make_float2(0.f, 0.f);
          if (k + q < ke && col < Nc) {
            v = *reinterpret_cast<const float2*>(Xs + (int64_t)(k + q) * M.ldx + col);   // col even, ldx % 4 == 0
            v.x *= xs;
            v.y = col + 1 < Nc ? v.y * xs : 0.f;
          }
          f0[q] = v.x;
          f1[q] = v.y;
        }
      }
    }
    // slab by slab (the loads retire in issue order, so slab 0's MFMAs start under the later loads)
#pragma unroll
    for (int sl = 0; sl < NF_SLABS; ++sl) {
      if (k0 + 16 * sl >= ke) break;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32((&fa[sl][a].x)[q], (&fb[sl][b].x)[q], acc[a][b], 0, 0, 0);
    }
  }
  // lane holds C[16 a + 4 g + i][column r16 of sub-tile b]; the update's sub-tile b is columns 2 j + b
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        part[w][16 * a + 4 * g + i][PH == NS_UPD ? 2 * r16 + b : 16 * b + r16] = acc[a][b][i];
  __syncthreads();
  constexpr int PER = NF_T * NF_T / NF_THREADS;          // outputs per thread (2), consecutive columns
  const int lr = tid / (NF_T / PER), lc = (tid % (NF_T / PER)) * PER, row = m0 + lr;
  float* __restrict__ dst = PH == NS_GRAM ? M.A : (PH == NS_POLY ? M.B : (last ? M.out : ((it & 1) ? M.x0 : M.x1)));
  const int ldd = PH == NS_UPD ? M.ldx : M.lda;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int col = n0 + lc + q;
    if (row >= Mr || col >= Nc) continue;
    float sum = 0.f;
#pragma unroll
    for (int ww = 0; ww < NF_WAVES; ++ww) sum += part[ww][lr][lc + q];   // wave order: deterministic
    float v;
    if (PH == NS_GRAM) v = sum;
    else if (PH == NS_POLY) v = cb * M.A[(int64_t)row * M.lda + col] + cc * sum;
    else v = ca * (xs * Xs[(int64_t)row * M.ldx + col]) + sum;
    dst[(int64_t)row * ldd + col] = v;
    // symmetric products: only tiles with tm <= tn exist; a diagonal tile is computed whole
    if (PH != NS_UPD && tl.tm != tl.tn) dst[(int64_t)col * ldd + row] = v;
  }
}

// ns_steps = 0: out = x0 / (||x0||_F + eps) over the update's tiles
__global__ __launch_bounds__(NF_THREADS) void ns_scale_kernel(const NsMat* __restrict__ mats,
                                                              const NsTile* __restrict__ tiles, float eps) {
  __shared__ double sh;
  const NsTile tl = tiles[blockIdx.x];
  const NsMat M = mats[tl.mat];
  const float xs = ns_inv_norm(M, eps, &sh);
  const int tid = threadIdx.x;
  const int row = tl.tm * NF_T + tid / 16, col = tl.tn * NF_T + (tid % 16) * 2;
#pragma unroll
  for (int q = 0; q < 2; ++q)
    if (row < M.r && col + q < M.c) M.out[(int64_t)row * M.ldx + col + q] = M.x0[(int64_t)row * M.ldx + col + q] * xs;
}

}  // namespace
}  // namespace pcv

using namespace pcv;

extern "C" int pcv_muon_ns_f32_rec_size(void) { return (int)sizeof(NsMat); }
extern "C" int pcv_muon_ns_f32_tile(void) { return NF_T; }

extern "C" int pcv_muon_ns_f32(const void* recs, int nmats, const void* tiles, int nsym, int nupd, float eps,
                               float ns_a, float ns_b, float ns_c, int ns_steps, void* stream) {
  if (!recs || !tiles || nmats <= 0 || nsym <= 0 || nupd <= 0 || ns_steps < 0 || ns_b == 0.f) return PCV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const NsMat* m = (const NsMat*)recs;
  const NsTile* ts = (const NsTile*)tiles;   // [0, nsym): symmetric products; [nsym, nsym + nupd): update
  const NsTile* tu = ts + nsym;
  if (ns_steps == 0) hipLaunchKernelGGL(ns_scale_kernel, dim3(nupd), dim3(NF_THREADS), 0, s, m, tu, eps);
  for (int it = 0; it < ns_steps; ++it) {
    const int last = it == ns_steps - 1;
    hipLaunchKernelGGL(ns_phase_kernel<NS_GRAM>, dim3(nsym), dim3(NF_THREADS), 0, s, m, ts, it, last, eps, ns_a, ns_b,
                       ns_c);
    hipLaunchKernelGGL(ns_phase_kernel<NS_POLY>, dim3(nsym), dim3(NF_THREADS), 0, s, m, ts, it, last, eps, ns_a, ns_b,
                       ns_c);
    hipLaunchKernelGGL(ns_phase_kernel<NS_UPD>, dim3(nupd), dim3(NF_THREADS), 0, s, m, tu, it, last, eps, ns_a, ns_b,
                       ns_c);
  }
  return pcv_launch_status();
}
