// drop_path.hip -- stochastic depth (Huang et al. 2016; "drop path") for gfx950: the per-sample scaled
// residual add of a block whose drop probability is > 0, and the branch gradient of its backward.
// bf16 NHWC activations; the factors f[n] = keep / (1 - p) are fp32 in device memory, drawn on the host
// for every step (data/drop_path.py), so a recorded launch follows the draws of the step it replays in.
//
//   forward   out[n] = bf16(fma(f[n], u[n], shortcut[n]))     (+ the next BatchNorm's statistics of out)
//   backward  du[n]  = bf16(f[n] * d_out[n])
//
// Both are one streaming kernel, drop_path_kernel<BWD>. Byte-bound: every tensor is touched once, 16
// bytes per access.
//   * A workgroup owns a 256-channel slab (all C below that) of one sample's pixel range. A thread keeps
//     ONE 8-channel chunk for its whole life and walks pixels `planes` = 256 / (slab / 8) apart, so a
//     wave's accesses cover whole pixel rows and the statistics of its chunk stay in 16 registers.
//   * The sample is workgroup-uniform, so its factor is read once into a scalar register and the kept /
//     dropped decision is a scalar branch around the whole pixel walk, not a per-element select:
//       dropped, forward   u is never loaded; out gets the shortcut's bits (nothing is stored when out IS
//                          the shortcut buffer) and the statistics come from them;
//       dropped, backward  zeros are stored, d_out is never loaded.
//     A dropped sample so moves 2 of the 3 (forward) or 1 of the 2 (backward) tensors' bytes.
//   * The pixel split S is chosen on the host per geometry (dp_splits): about 2048 workgroups, never less
//     than one pixel per thread, at most 64 splits.
//   * Statistics: sum and sum of squares of the STORED (rounded) values per thread, combined once per
//     workgroup through LDS (planes in order) and added into replica (workgroup % rep) of [rep][2][C] --
//     the protocol of the conv epilogue this kernel stands in for. With statistics a workgroup strides
//     over samples so that at most 1024 workgroups per slab add: with >= 1024 replicas (the deterministic
//     mode) every slot receives exactly one add. No other atomics.
#include "drn_common.h"

// Argument block of both entry points (ctypes mirror: ops/_lib.py DrnDropPathArgs); the entry points
// fill the tiling fields.
struct DrnDropPathArgs {
  const void* x;     // bf16 [N][HW][C]: u (forward) / d_out (backward)
  const void* y;     // bf16 [N][HW][C]: the shortcut (forward; may be `out` itself)
  void* out;         // bf16 [N][HW][C]: out (forward) / du (backward)
  const float* f;    // fp32 [N]: the block's row of the factor table
  float* stats;      // optional fp32 [stats_rep][2][C] (+= sum, sum of squares of out; forward)
  int32_t N, HW, C, stats_rep;
  // filled by the entry points
  int32_t S, pps, slab, cpw, planes, pad_;
};

namespace drn {

constexpr int DP_SLAB = 256;        // channels per workgroup
constexpr int DP_MAX_SPLIT = 64;    // pixel splits per sample
constexpr int DP_STAT_WGS = 1024;   // statistics-producing workgroups per slab (= replicas needed)

template <bool BWD>
__global__ __launch_bounds__(256) void drop_path_kernel(DrnDropPathArgs a) {
  __shared__ float red[2][256 * 8];
  const int tid = threadIdx.x;
  const int plane = tid / a.cpw, chunk = tid - plane * a.cpw;
  const int c = blockIdx.x * a.slab + chunk * 8;
  const int C = a.C;
  const int p0 = blockIdx.y * a.pps + plane, p1 = min(a.HW, ((int)blockIdx.y + 1) * a.pps);
  const bool active = plane < a.planes && c < C;
  const bool want = !BWD && a.stats != nullptr;
  const bool alias = !BWD && a.out == a.y;
  float ssum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ssq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int n = blockIdx.z; n < a.N; n += gridDim.z) {
    // (n is uniform: the factor lives in a scalar register and both branches below are scalar branches)
    const float f = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(a.f[n])));
    if (!active) continue;
    const size_t base = (size_t)n * a.HW * C + c;
    const bf16_t* __restrict__ X = reinterpret_cast<const bf16_t*>(a.x) + base;
    bf16_t* O = reinterpret_cast<bf16_t*>(a.out) + base;
    if (BWD) {
      if (f == 0.f) {
        const uint4 zero = {0u, 0u, 0u, 0u};
        for (int p = p0; p < p1; p += a.planes) *reinterpret_cast<uint4*>(O + (size_t)p * C) = zero;
      } else {
#pragma unroll 4
        for (int p = p0; p < p1; p += a.planes) {
          float g[8];
          unpack8(*reinterpret_cast<const uint4*>(X + (size_t)p * C), g);
#pragma unroll
          for (int e = 0; e < 8; ++e) g[e] *= f;
          *reinterpret_cast<uint4*>(O + (size_t)p * C) = pack8(g);
        }
      }
      continue;
    }
    const bf16_t* Y = reinterpret_cast<const bf16_t*>(a.y) + base;
    const bool dropped = f == 0.f;
#pragma unroll 4
    for (int p = p0; p < p1; p += a.planes) {
      uint4 packed = *reinterpret_cast<const uint4*>(Y + (size_t)p * C);
      float o[8];
      if (!dropped) {
        float u[8];
        unpack8(*reinterpret_cast<const uint4*>(X + (size_t)p * C), u);
        unpack8(packed, o);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = fmaf(f, u[e], o[e]);
        packed = pack8(o);
      }
      if (!(dropped && alias)) *reinterpret_cast<uint4*>(O + (size_t)p * C) = packed;
      if (want) {
        unpack8(packed, o);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          ssum[e] += o[e];
          ssq[e] = fmaf(o[e], o[e], ssq[e]);
        }
      }
    }
  }
  if (want) {
    const int pitch = a.cpw * 8;
    if (plane < a.planes) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        red[0][plane * pitch + chunk * 8 + e] = ssum[e];
        red[1][plane * pitch + chunk * 8 + e] = ssq[e];
      }
    }
    __syncthreads();
    const int ch = blockIdx.x * a.slab + tid;
    if (tid < pitch && ch < C) {
      float s0 = 0.f, s1 = 0.f;   // the planes in order
      for (int pl = 0; pl < a.planes; ++pl) {
        s0 += red[0][pl * pitch + tid];
        s1 += red[1][pl * pitch + tid];
      }
      const int rep = a.stats_rep > 1 ? a.stats_rep : 1;
      float* acc = a.stats + (size_t)((blockIdx.z * gridDim.y + blockIdx.y) % rep) * 2 * C;
      atomicAdd(acc + ch, s0);
      atomicAdd(acc + C + ch, s1);
    }
  }
}

static bool dp_domain(const DrnDropPathArgs* a) {
  return a->N >= 1 && a->N <= 65535 && a->HW >= 1 && a->C >= 8 && a->C % 8 == 0 && (int64_t)a->HW * a->C < (1ll << 40);
}

// The thread layout for C channels
static void dp_walk(DrnDropPathArgs* a) {
  a->slab = a->C < DP_SLAB ? a->C : DP_SLAB;
  a->cpw = a->slab / 8;
  a->planes = 256 / a->cpw;
}

// Pixel splits per sample: about 2048 workgroups, at least one pixel per thread, at most DP_MAX_SPLIT
static int dp_splits(int N, int HW, int C) {
  DrnDropPathArgs a{};
  a.C = C;
  dp_walk(&a);
  const int64_t wgs = (int64_t)N * ((C + DP_SLAB - 1) / DP_SLAB);
  int64_t s = 2048 / wgs;
  const int by_rows = HW / a.planes;
  if (s > by_rows) s = by_rows;
  if (s > DP_MAX_SPLIT) s = DP_MAX_SPLIT;
  if (s < 1) s = 1;
  const int pps = (HW + (int)s - 1) / (int)s;
  return (HW + pps - 1) / pps;
}

template <bool BWD>
static int dp_launch(DrnDropPathArgs* a, hipStream_t s) {
  dp_walk(a);
  a->S = dp_splits(a->N, a->HW, a->C);
  a->pps = (a->HW + a->S - 1) / a->S;
  int nz = a->N;
  if (!BWD && a->stats != nullptr && nz > DP_STAT_WGS / a->S) nz = DP_STAT_WGS / a->S;
  drn::launch(drop_path_kernel<BWD>, dim3((a->C + DP_SLAB - 1) / DP_SLAB, a->S, nz), dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

}  // namespace drn

DRN_API int drn_drop_path_args_size() { return (int)sizeof(DrnDropPathArgs); }

// Pixel splits per sample the kernels use for this geometry; 0: outside the domain
DRN_API int drn_drop_path_splits(int N, int HW, int C) {
  DrnDropPathArgs a{};
  a.N = N, a.HW = HW, a.C = C;
  return drn::dp_domain(&a) ? drn::dp_splits(N, HW, C) : 0;
}

// out = shortcut (y) + f[n] * u (x), + statistics of the stored out
DRN_API int drn_drop_path_fwd(DrnDropPathArgs* a, hipStream_t s) {
  if (!drn::dp_domain(a) || !a->x || !a->y || !a->out || !a->f) return (int)hipErrorInvalidValue;
  if (a->stats != nullptr && a->stats_rep < 1) return (int)hipErrorInvalidValue;
  return drn::dp_launch<false>(a, s);
}

// du (out) = f[n] * d_out (x)
DRN_API int drn_drop_path_bwd(DrnDropPathArgs* a, hipStream_t s) {
  if (!drn::dp_domain(a) || !a->x || !a->out || !a->f) return (int)hipErrorInvalidValue;
  a->y = nullptr;
  a->stats = nullptr;
  return drn::dp_launch<true>(a, s);
}
