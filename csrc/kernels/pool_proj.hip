// pool_proj.hip -- ResNet-D projection shortcut for gfx950: sc = conv1x1(avgpool2x2/2(a)), a either a
// materialised activation or relu(scale * x + shift) of a raw pre-BN tensor, and its data gradient.
// bf16 NHWC activations, bf16 weights, fp32 accumulation; H and W even, Cin % 8 == 0, Cout % 8 == 0.
//
// Both passes are one implicit GEMM at POOLED resolution (M = N * H/2 * W/2 rows) on
// v_mfma_f32_16x16x32_bf16; the pool lives in the forward pass's operand loader and the un-pool in
// the data gradient's epilogue, so no pooled or un-pooled tensor makes a round trip through memory
// (the quarter-size stash `ap` the weight gradient reads is written on the way, never re-read here).
//
// pool_proj_kernel<MODE, BN>: a workgroup (4 waves, 2 x 2) owns 64 pooled pixels x BN columns and
// walks the reduction in steps of 64.
//   * Pixel operand, forward: a thread owns one 8-channel piece of two pooled pixels: four 16-byte
//     loads per pixel at (2p, 2q), (2p, 2q+1), (2p+1, 2q), (2p+1, 2q+1) (8 threads cover 128
//     contiguous bytes of each source pixel). A raw input gets relu(scale * x + shift) in fp32, each
//     term rounded to bf16 (bn_relu_piece, what the fused-prologue convs compute); the terms are
//     added in fp32 as (t00 + t01) + (t10 + t11), times 0.25, rounded once, written to LDS. The
//     workgroups of column block 0 also store the piece to the stash from the same register.
//     Data gradient: the piece is one plain 16-byte load of d_out.
//   * Weight operand: [columns][reduction] bf16 in both passes (the forward weights; for the data
//     gradient the [Cin][1][1][Cout] copy the stride-1 1x1 data gradients already keep), plain
//     16-byte loads.
//   * Both tiles are register-staged and double-buffered: the loads of step k+1 are issued before
//     the MFMAs of step k and land in the other LDS stage after them, one barrier per step. LDS rows
//     are 144 bytes apart (128 + 16 of padding): the 16 rows of a fragment read start 36 dwords
//     apart, so ds_read_b128 covers the 64 banks once.
//   * The weights are the MFMA's A operand and the pixels its B operand, so a lane ends up with 4
//     consecutive channels of one pixel: 8-byte LDS writes (rows 4 banks apart, conflict-free), then
//     16-byte row stores. The data gradient stores bf16(0.25 * g) to the four pixels (2p+i, 2q+j):
//     every element of da is written, none accumulated.
//   * Column blocks of one pixel tile are consecutive logical workgroups and xcd_remap keeps them on
//     one XCD, so the re-reads of the pixel operand (once per column block) meet in that XCD's L2.
// No atomics: the bits depend on the inputs and the launch shape only. One configuration per
// geometry from pp_pick_bn; nothing here is autotuned.
#include "drn_common.h"

// Argument block (ctypes mirror: ops/_lib.py DrnPoolProjArgs). The entry points fill P .. ncb.
struct DrnPoolProjArgs {
  const void* x;       // fwd: bf16 [N][H][W][Cin], raw (scale / shift set) or materialised
  const void* w;       // fwd: bf16 [Cout][Cin]; dgrad: bf16 [Cin][Cout]
  const float* scale;  // fwd, optional: fp32 [Cin] published BatchNorm scale / shift
  const float* shift;
  void* sc;            // fwd out: bf16 [N][P][Q][Cout]
  void* ap;            // fwd out: bf16 [N][P][Q][Cin], the pooled operand (weight gradient input)
  const void* dy;      // dgrad: bf16 [N][P][Q][Cout]
  void* da;            // dgrad out: bf16 [N][H][W][Cin]
  int32_t N, H, W, Cin, Cout;
  int32_t P, Q, M, K, NC, ncb;  // pooled size, GEMM rows / reduction / columns, column blocks
};

namespace drn {

constexpr int PP_BM = 64;                  // pooled pixels per workgroup
constexpr int PP_BK = 64;                  // reduction elements per step
constexpr int PP_PITCH = PP_BK * 2 + 16;   // LDS bytes per operand row

enum { PP_FWD_ACT = 0, PP_FWD_RAW = 1, PP_DGRAD = 2 };

template <int MODE, int BN>
__global__ __launch_bounds__(256) void pool_proj_kernel(DrnPoolProjArgs a) {
  constexpr bool DG = MODE == PP_DGRAD;
  constexpr int NSRC = DG ? 1 : 4;         // 16-byte loads per pixel piece
  constexpr int NFW = BN / 32;             // 16-column weight fragments per wave
  constexpr int WPT = BN / 32;             // weight pieces per thread and step
  constexpr int A_BYTES = PP_BM * PP_PITCH, STAGE = A_BYTES + BN * PP_PITCH;
  constexpr int OPITCH = BN * 2 + 16;      // staged output row
  static_assert(PP_BM * OPITCH <= 2 * STAGE, "the staged output reuses the operand stages");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  __shared__ long long pixbase[PP_BM];     // pixel (n, 2p, 2q) of each row, -1 past M

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const int wm = wave & 1, wn = wave >> 1;
  const int M = a.M, K = a.K, NC = a.NC;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int mt = lin / a.ncb, cb = lin - mt * a.ncb;
  const int m0 = mt * PP_BM, n0 = cb * BN;

  if (tid < PP_BM) {
    const int m = m0 + tid;
    long long b = -1;
    if (m < M) {
      const int pq = a.P * a.Q;
      const int n = m / pq, r = m - n * pq;
      const int p = r / a.Q, q = r - p * a.Q;
      b = ((long long)n * a.H + 2 * p) * a.W + 2 * q;
    }
    pixbase[tid] = b;
  }
  __syncthreads();

  const bf16_t* __restrict__ A = reinterpret_cast<const bf16_t*>(DG ? a.dy : a.x);
  const bf16_t* __restrict__ Wt = reinterpret_cast<const bf16_t*>(a.w);
  bf16_t* __restrict__ AP = reinterpret_cast<bf16_t*>(a.ap);

  // the thread's pieces: reduction piece pc of rows prow and prow + 32 (pixels), prow + 32 j (weights)
  const int pc = tid & 7, prow = tid >> 3;
  long long abase[2];
  bool aok[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const long long pb = pixbase[prow + 32 * j];
    aok[j] = pb >= 0;
    abase[j] = DG ? (long long)(m0 + prow + 32 * j) * K : pb * K;
  }
  const long long row_step = (long long)a.W * K;   // forward: one source row down
  const bool stash = !DG && cb == 0;

  u32x4_t ra[2][NSRC], rb[WPT];
  f32x2_t sc2[4], sh2[4];
  const u32x4_t zero4 = {0u, 0u, 0u, 0u};

  auto load = [&](int kt) {
    const int kc = kt * PP_BK + pc * 8;
    const bool kok = kc < K;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int s = 0; s < NSRC; ++s) {
        const long long off = abase[j] + kc + (DG ? 0 : (s >> 1) * row_step + (s & 1) * K);
        ra[j][s] = (aok[j] && kok) ? *reinterpret_cast<const u32x4_t*>(A + off) : zero4;
      }
    if constexpr (MODE == PP_FWD_RAW) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        sc2[p] = kok ? *reinterpret_cast<const f32x2_t*>(a.scale + kc + 2 * p) : f32x2_t{0.f, 0.f};
        sh2[p] = kok ? *reinterpret_cast<const f32x2_t*>(a.shift + kc + 2 * p) : f32x2_t{0.f, 0.f};
      }
    }
#pragma unroll
    for (int j = 0; j < WPT; ++j) {
      const int col = n0 + prow + 32 * j;
      rb[j] = (col < NC && kok) ? *reinterpret_cast<const u32x4_t*>(Wt + (long long)col * K + kc) : zero4;
    }
  };

  auto store = [&](int kt, char* st) {
    const int kc = kt * PP_BK + pc * 8;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      u32x4_t v;
      if constexpr (DG) {
        v = ra[j][0];
      } else {
        float t[4][8], o[8];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          if constexpr (MODE == PP_FWD_RAW) {
            unpack8v(bn_relu_piece<true>(ra[j][s], sc2, sh2), t[s]);
          } else {
            unpack8v(ra[j][s], t[s]);
          }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = ((t[0][e] + t[1][e]) + (t[2][e] + t[3][e])) * 0.25f;
        const bool ok = aok[j] && kc < K;
        v = ok ? pack8v(o) : zero4;
        if (stash && ok) *reinterpret_cast<u32x4_t*>(AP + (long long)(m0 + prow + 32 * j) * K + kc) = v;
      }
      *reinterpret_cast<u32x4_t*>(st + (prow + 32 * j) * PP_PITCH + pc * 16) = v;
    }
#pragma unroll
    for (int j = 0; j < WPT; ++j)
      *reinterpret_cast<u32x4_t*>(st + A_BYTES + (prow + 32 * j) * PP_PITCH + pc * 16) = rb[j];
  };

  // acc[f][j][i]: column wn * BN/2 + 16 f + 4 g + i of pixel row wm * 32 + 16 j + l16
  f32x4_t acc[NFW][2];
#pragma unroll
  for (int f = 0; f < NFW; ++f)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[f][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nk = (K + PP_BK - 1) / PP_BK;
  load(0);
  store(0, smem);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;
    if (more) load(kt + 1);
    const char* sa = smem + (kt & 1) * STAGE;
    const char* sb = sa + A_BYTES;
#pragma unroll
    for (int ks = 0; ks < PP_BK / 32; ++ks) {
      bf16x8_t wf[NFW], pf[2];
#pragma unroll
      for (int f = 0; f < NFW; ++f)
        wf[f] = *reinterpret_cast<const bf16x8_t*>(sb + (wn * (BN / 2) + 16 * f + l16) * PP_PITCH + ks * 64 + g * 16);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        pf[j] = *reinterpret_cast<const bf16x8_t*>(sa + (wm * 32 + 16 * j + l16) * PP_PITCH + ks * 64 + g * 16);
#pragma unroll
      for (int f = 0; f < NFW; ++f)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[f][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[f], pf[j], acc[f][j], 0, 0, 0);
    }
    if (more) store(kt + 1, smem + ((kt + 1) & 1) * STAGE);
    __syncthreads();  // stage kt + 1 is complete, and every wave is done with stage kt
  }

  const float osc = DG ? 0.25f : 1.0f;
#pragma unroll
  for (int f = 0; f < NFW; ++f)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = wm * 32 + 16 * j + l16, col = wn * (BN / 2) + 16 * f + 4 * g;
      *reinterpret_cast<uint2*>(smem + row * OPITCH + col * 2) =
          make_uint2(pack2bf(acc[f][j][0] * osc, acc[f][j][1] * osc), pack2bf(acc[f][j][2] * osc, acc[f][j][3] * osc));
    }
  __syncthreads();
  bf16_t* __restrict__ OUT = reinterpret_cast<bf16_t*>(DG ? a.da : a.sc);
  for (int i = tid; i < PP_BM * (BN / 8); i += 256) {
    const int row = i / (BN / 8), opc = i - row * (BN / 8);
    const int col = n0 + opc * 8;
    const long long pb = pixbase[row];
    if (pb < 0 || col >= NC) continue;
    const uint4 v = *reinterpret_cast<const uint4*>(smem + row * OPITCH + opc * 16);
    if constexpr (DG) {
      bf16_t* o = OUT + pb * NC + col;
      const long long down = (long long)a.W * NC;
      *reinterpret_cast<uint4*>(o) = v;
      *reinterpret_cast<uint4*>(o + NC) = v;
      *reinterpret_cast<uint4*>(o + down) = v;
      *reinterpret_cast<uint4*>(o + down + NC) = v;
    } else {
      *reinterpret_cast<uint4*>(OUT + (long long)(m0 + row) * NC + col) = v;
    }
  }
}

// Column block of a geometry: 128 columns halve the re-reads of the pixel operand; 64 where the
// columns fit one block or 128 would leave fewer than two workgroups per CU.
static int pp_pick_bn(int M, int NC) {
  const int64_t ntm = (M + PP_BM - 1) / PP_BM;
  if (NC <= 64) return 64;
  return ntm * ((NC + 127) / 128) >= 512 ? 128 : 64;
}

static bool pp_aligned(const void* p) { return p != nullptr && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Validate the geometry and fill the GEMM fields; false outside the domain.
static bool pp_plan(DrnPoolProjArgs* a, bool dgrad) {
  if (a->N < 1 || a->H < 2 || a->W < 2 || (a->H & 1) || (a->W & 1)) return false;
  if (a->Cin < 8 || a->Cout < 8 || a->Cin % 8 != 0 || a->Cout % 8 != 0) return false;
  a->P = a->H / 2;
  a->Q = a->W / 2;
  const int64_t M = (int64_t)a->N * a->P * a->Q;
  if (M > ((int64_t)1 << 30)) return false;
  a->M = (int)M;
  a->K = dgrad ? a->Cout : a->Cin;
  a->NC = dgrad ? a->Cin : a->Cout;
  const int bn = pp_pick_bn(a->M, a->NC);
  a->ncb = (a->NC + bn - 1) / bn;
  return ((M + PP_BM - 1) / PP_BM) * a->ncb < ((int64_t)1 << 31);
}

template <int MODE>
static int pp_launch(DrnPoolProjArgs* a, hipStream_t s) {
  const int ntm = (a->M + PP_BM - 1) / PP_BM;
  const dim3 grid((unsigned)(ntm * a->ncb));
  if (pp_pick_bn(a->M, a->NC) == 128)
    drn::launch(pool_proj_kernel<MODE, 128>, grid, dim3(256), 0, s, *a);
  else
    drn::launch(pool_proj_kernel<MODE, 64>, grid, dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

}  // namespace drn

DRN_API int drn_pool_proj_args_size() { return (int)sizeof(DrnPoolProjArgs); }

// sc = conv1x1(avgpool2x2(a)), ap = the pooled operand; a = x, or relu(scale * x + shift) with scale set
DRN_API int drn_pool_proj_fwd(DrnPoolProjArgs* a, hipStream_t s) {
  if (!drn::pp_plan(a, false)) return (int)hipErrorInvalidValue;
  if (!drn::pp_aligned(a->x) || !drn::pp_aligned(a->w) || !drn::pp_aligned(a->sc) || !drn::pp_aligned(a->ap))
    return (int)hipErrorInvalidValue;
  if ((a->scale == nullptr) != (a->shift == nullptr)) return (int)hipErrorInvalidValue;
  if (a->scale != nullptr) {
    if (!drn::pp_aligned(a->scale) || !drn::pp_aligned(a->shift)) return (int)hipErrorInvalidValue;
    return drn::pp_launch<drn::PP_FWD_RAW>(a, s);
  }
  return drn::pp_launch<drn::PP_FWD_ACT>(a, s);
}

// da[n, 2p+i, 2q+j, :] = bf16(0.25 * sum_k dy[n, p, q, k] w[:, k]) for i, j in {0, 1}; w is [Cin][Cout]
DRN_API int drn_pool_proj_dgrad(DrnPoolProjArgs* a, hipStream_t s) {
  if (!drn::pp_plan(a, true)) return (int)hipErrorInvalidValue;
  if (!drn::pp_aligned(a->dy) || !drn::pp_aligned(a->w) || !drn::pp_aligned(a->da)) return (int)hipErrorInvalidValue;
  return drn::pp_launch<drn::PP_DGRAD>(a, s);
}
