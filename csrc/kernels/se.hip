// se.hip -- Squeeze-and-Excitation for gfx950: squeeze, gate (forward / backward / weight gradient),
// excite and the gate's data gradient. bf16 NHWC activations, fp32 gate (z, h, s and the four SE
// variables, read from the fp32 masters: reduce/kernel W1 [C][Cr], expand/kernel W2 [Cr][C]).
//
//   u -> z = mean_hw u -> h = relu(z W1 + b1) -> s = sigmoid(h W2 + b2) -> out = shortcut + s * u
//
// Two kinds of kernel, with nothing in common but the argument block:
//
// Streaming kernels (se_squeeze_kernel, se_stream_kernel<BWD>: excite and scale_bwd). Byte-bound:
// u is read once by the squeeze and once by the excite, 16 bytes per load.
//   * A workgroup owns one sample's pixel range [split] of a channel slab (all C up to 256 channels,
//     else 256-channel slabs). A thread keeps ONE 8-channel chunk for its whole life and walks pixels
//     `planes` = 256 / (slab / 8) apart: its 8 fp32 accumulators (squeeze), its 8 gate values s and
//     8 broadcast addends dz / HW (excite, scale_bwd) stay in registers, and a wave's loads cover
//     whole pixel rows (512 contiguous bytes per 32 lanes at C >= 256).
//   * The pixel split S is chosen on the host per geometry (se_splits): about 2048 workgroups when the
//     plane is large (56x56: S = 16 at batch 128), no split when it is small (7x7 x 2048 channels:
//     8 slabs x 128 samples already fill the chip), never fewer than two pixels per thread.
//   * Squeeze: the threads' accumulators meet in LDS [plane][channel] and one thread per channel adds
//     the planes in order into the workgroup's cell of [N][S][C]; the consumer (the gate kernel) adds
//     the S cells in order. No atomics: the bits are a function of the inputs and (N, HW, C, S). With
//     a second operand the terms are products g * u (exact in fp32): the backward's ds.
//   * Excite: out = bf16(fma(s, u, shortcut)), and the next BatchNorm's sum / sum of squares of the
//     STORED values per thread, combined once per workgroup through LDS (planes in order) and added
//     into replica (workgroup % rep) of [rep][2][C]: the protocol of the conv epilogue. A workgroup
//     strides over samples so that at most 1024 workgroups per slab produce statistics: with >= 1024
//     replicas (the deterministic mode) every slot receives exactly one add.
//
// Gate kernels (se_gate_kernel<BWD>, se_gate_wgrad_kernel). Tiny fp32 GEMMs on
// v_mfma_f32_16x16x4_f32; one launch each.
//   * A workgroup owns 16 samples (the M of the instruction) and a 128-column slab of the C outputs.
//     GEMM 1 reduces over all of C into [16][Cr]: the four waves split the reduction, each builds its
//     A fragments straight from global memory (a lane's element is the in-order sum of its S squeeze
//     cells, scaled by 1 / HW forward or by s (1 - s) backward) and streams the weights from global
//     memory as B fragments, up to 8 column tiles (128 columns of Cr) in registers per pass. The four
//     partial tiles meet in LDS, are added in wave order, get bias + ReLU (forward) or the stored
//     h > 0 mask (backward) and form the [16][Cr] tile in LDS that GEMM 2 reads as A. GEMM 2: a wave
//     per 16-column tile of the slab, all of Cr, then bias + sigmoid (1 / (1 + expf(-x)), library expf)
//     or the 1 / HW scale. Workgroups of the same samples recompute GEMM 1 (16 C Cr MACs) instead of
//     synchronising; only column slab 0 stores z / h (dl2 / dh). Rows past N load zeros and store
//     nothing.
//   * Weight gradients: dW1 = z^T dh, dW2 = h^T dl2: one wave per 16x16 output tile, the reduction
//     over ALL samples in order in steps of 4 (no split, no atomics); the tiles of the first row also
//     sum their 16 columns of dh / dl2 into db1 / db2.
#include "drn_common.h"
#include <atomic>

// Argument block of every entry point (ctypes mirror: ops/_lib.py DrnSeArgs). Each kernel reads the
// fields named in its entry point's comment; the entry points fill the tiling fields.
struct DrnSeArgs {
  const void* x;      // bf16 [N][HW][C]: u (squeeze, excite) / g (scale_bwd)
  const void* y;      // bf16 [N][HW][C]: squeeze's optional second operand / excite's shortcut
  void* out;          // bf16 [N][HW][C]: excite's out / scale_bwd's du
  float* cells;       // fp32 [N][S][C] squeeze cells
  const float* w1;    // fp32 [C][Cr]
  const float* b1;    // fp32 [Cr]
  const float* w2;    // fp32 [Cr][C]
  const float* b2;    // fp32 [C]
  float* z;           // fp32 [N][C]
  float* h;           // fp32 [N][Cr]
  float* s;           // fp32 [N][C]
  float* dl2;         // fp32 [N][C]
  float* dh;          // fp32 [N][Cr]
  float* dzs;         // fp32 [N][C]   dz / HW
  float* dw1;         // fp32 [C][Cr]
  float* db1;         // fp32 [Cr]
  float* dw2;         // fp32 [Cr][C]
  float* db2;         // fp32 [C]
  float* stats;       // optional fp32 [stats_rep][2][C] (+= sum, sum of squares of out)
  int32_t N, HW, C, Cr, S, stats_rep;
  // filled by the entry points
  int32_t pps, slab, cpw, planes;
  float inv_hw;
  int32_t pad_;
};

namespace drn {

constexpr int SE_SLAB = 256;         // channels per streaming workgroup
constexpr int SE_MAX_SPLIT = 64;     // pixel splits per sample
constexpr int SE_STAT_WGS = 1024;    // statistics-producing workgroups per slab (= replicas needed)
constexpr int SEG_CHUNK = 128;       // GEMM 1 columns per pass (8 tiles in registers)
constexpr int SEG_SLAB = 128;        // GEMM 2 columns per workgroup
constexpr int SEG_MAX_CR = 1024;
constexpr int SEG_U = 8;           // k-steps whose loads are issued together
constexpr int SEG_LDS = (4 * 16 * SEG_CHUNK + 16 * (SEG_MAX_CR + 4)) * 4;

__device__ __forceinline__ void se_load8(const float* p, float* f) {
  const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
  f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w;
  f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
}

// red[plane][slab channel] -> the in-order sum over planes of channel `tid`
__device__ __forceinline__ float se_plane_sum(const float* red, int planes, int pitch, int tid) {
  float t = 0.f;
  for (int pl = 0; pl < planes; ++pl) t += red[pl * pitch + tid];
  return t;
}

// cells[n][split][c] = sum over the split's pixels of x (or x * y)
__global__ __launch_bounds__(256) void se_squeeze_kernel(DrnSeArgs a) {
  __shared__ float red[256 * 8];
  const int tid = threadIdx.x;
  const int plane = tid / a.cpw, chunk = tid - plane * a.cpw;
  const int c = blockIdx.x * a.slab + chunk * 8;
  const int n = blockIdx.z, C = a.C;
  const int p1 = min(a.HW, ((int)blockIdx.y + 1) * a.pps);
  const bool active = plane < a.planes && c < C;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (active) {
    const bf16_t* __restrict__ X = reinterpret_cast<const bf16_t*>(a.x) + (size_t)n * a.HW * C + c;
    const bf16_t* __restrict__ Y = a.y ? reinterpret_cast<const bf16_t*>(a.y) + (size_t)n * a.HW * C + c : nullptr;
    if (Y == nullptr) {
#pragma unroll 4
      for (int p = blockIdx.y * a.pps + plane; p < p1; p += a.planes) {
        float f[8];
        unpack8(*reinterpret_cast<const uint4*>(X + (size_t)p * C), f);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += f[e];
      }
    } else {
#pragma unroll 4
      for (int p = blockIdx.y * a.pps + plane; p < p1; p += a.planes) {
        float f[8], g[8];
        unpack8(*reinterpret_cast<const uint4*>(X + (size_t)p * C), f);
        unpack8(*reinterpret_cast<const uint4*>(Y + (size_t)p * C), g);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(f[e], g[e], acc[e]);
      }
    }
  }
  const int pitch = a.cpw * 8;
  if (plane < a.planes) {
#pragma unroll
    for (int e = 0; e < 8; ++e) red[plane * pitch + chunk * 8 + e] = acc[e];
  }
  __syncthreads();
  const int ch = blockIdx.x * a.slab + tid;
  if (tid < pitch && ch < C) a.cells[((size_t)n * a.S + blockIdx.y) * C + ch] = se_plane_sum(red, a.planes, pitch, tid);
}

// excite (BWD = false): out = bf16(s * u + shortcut) (+ statistics of the stored out)
// scale_bwd (BWD = true): du = bf16(s * g + dzs), dzs broadcast over the pixels
template <bool BWD>
__global__ __launch_bounds__(256) void se_stream_kernel(DrnSeArgs a) {
  __shared__ float red[2][256 * 8];
  const int tid = threadIdx.x;
  const int plane = tid / a.cpw, chunk = tid - plane * a.cpw;
  const int c = blockIdx.x * a.slab + chunk * 8;
  const int C = a.C;
  const int p0 = blockIdx.y * a.pps + plane, p1 = min(a.HW, ((int)blockIdx.y + 1) * a.pps);
  const bool active = plane < a.planes && c < C;
  const bool want = !BWD && a.stats != nullptr;
  float ssum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ssq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (active) {
    for (int n = blockIdx.z; n < a.N; n += gridDim.z) {
      float sv[8], bv[8];
      se_load8(a.s + (size_t)n * C + c, sv);
      if (BWD) se_load8(a.dzs + (size_t)n * C + c, bv);
      const size_t base = (size_t)n * a.HW * C + c;
      const bf16_t* __restrict__ X = reinterpret_cast<const bf16_t*>(a.x) + base;
      const bf16_t* __restrict__ Y = BWD ? nullptr : reinterpret_cast<const bf16_t*>(a.y) + base;
      bf16_t* __restrict__ O = reinterpret_cast<bf16_t*>(a.out) + base;
#pragma unroll 4
      for (int p = p0; p < p1; p += a.planes) {
        float f[8], o[8];
        unpack8(*reinterpret_cast<const uint4*>(X + (size_t)p * C), f);
        if (!BWD) unpack8(*reinterpret_cast<const uint4*>(Y + (size_t)p * C), bv);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = fmaf(sv[e], f[e], bv[e]);
        const uint4 packed = pack8(o);
        *reinterpret_cast<uint4*>(O + (size_t)p * C) = packed;
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
      const int rep = a.stats_rep > 1 ? a.stats_rep : 1;
      float* acc = a.stats + (size_t)((blockIdx.z * gridDim.y + blockIdx.y) % rep) * 2 * C;
      atomicAdd(acc + ch, se_plane_sum(red[0], a.planes, pitch, tid));
      atomicAdd(acc + C + ch, se_plane_sum(red[1], a.planes, pitch, tid));
    }
  }
}

// Forward (BWD = false): z, h (column slab 0) and s [16 samples][SEG_SLAB columns] from the cells.
// Backward (BWD = true): the cells hold ds; dl2 = ds s (1 - s), dh = (dl2 W2^T) [h > 0] (column slab
// 0 stores both), dzs = dh W1^T / HW for the slab.
template <bool BWD>
__global__ __launch_bounds__(256) void se_gate_kernel(DrnSeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float se_smem[];
  float* part = se_smem;                   // [4 waves][16][SEG_CHUNK]
  float* ht = se_smem + 4 * 16 * SEG_CHUNK;  // [16][Cr + 4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g4 = lane >> 4;
  const int C = a.C, Cr = a.Cr, S = a.S, N = a.N;
  const int n0 = blockIdx.x * 16;
  const bool first = blockIdx.y == 0;
  const int hp = Cr + 4;
  const int row = n0 + l16;      // the lane's A row
  const bool rv = row < N;
  const int kw = C >> 2;         // the wave's share of GEMM 1's reduction (C % 16 == 0)

  for (int j0 = 0; j0 < Cr; j0 += SEG_CHUNK) {
    const int cw = min(SEG_CHUNK, Cr - j0);
    const int nt = (cw + 15) >> 4;
    f32x4_t acc[SEG_CHUNK / 16];
#pragma unroll
    for (int t = 0; t < SEG_CHUNK / 16; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // SEG_U k-steps per trip: their A and B loads are issued together (a step's loads are dependent
    // global reads; one step per trip left the loop latency-bound). Steps past the wave's share multiply
    // zeros, which changes no bit.
    const int kend = (wave + 1) * kw;
    for (int kb = wave * kw; kb < kend; kb += 4 * SEG_U) {
      float av[SEG_U];
#pragma unroll
      for (int i = 0; i < SEG_U; ++i) {
        const int c = kb + 4 * i + g4;
        av[i] = 0.f;
        if (rv && kb + 4 * i < kend) {
          const float* __restrict__ cell = a.cells + (size_t)row * S * C + c;
          float t = 0.f;
          for (int s = 0; s < S; ++s) t += cell[(size_t)s * C];
          if (BWD) {
            const float sg = a.s[(size_t)row * C + c];
            av[i] = t * sg * (1.f - sg);
          } else {
            av[i] = t * a.inv_hw;
          }
          if (first && j0 == 0) (BWD ? a.dl2 : a.z)[(size_t)row * C + c] = av[i];
        }
      }
#pragma unroll
      for (int t = 0; t < SEG_CHUNK / 16; ++t) {
        if (t < nt) {
          const int j = j0 + t * 16 + l16;
          float bv[SEG_U];
#pragma unroll
          for (int i = 0; i < SEG_U; ++i) {
            const int c = kb + 4 * i + g4;
            bv[i] = 0.f;
            if (j < Cr && kb + 4 * i < kend) bv[i] = BWD ? a.w2[(size_t)j * C + c] : a.w1[(size_t)c * Cr + j];
          }
#pragma unroll
          for (int i = 0; i < SEG_U; ++i) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[i], acc[t], 0, 0, 0);
        }
      }
    }
    // the lane holds rows 4 g4 .. 4 g4 + 3 of column l16 of each tile
#pragma unroll
    for (int t = 0; t < SEG_CHUNK / 16; ++t) {
      if (t < nt) {
#pragma unroll
        for (int v = 0; v < 4; ++v) part[(wave * 16 + 4 * g4 + v) * SEG_CHUNK + t * 16 + l16] = acc[t][v];
      }
    }
    __syncthreads();
    for (int idx = tid; idx < 16 * cw; idx += 256) {
      const int r = idx / cw, jj = idx - r * cw;
      const int j = j0 + jj, rr = n0 + r;
      float v = ((part[r * SEG_CHUNK + jj] + part[(16 + r) * SEG_CHUNK + jj]) + part[(32 + r) * SEG_CHUNK + jj]) +
                part[(48 + r) * SEG_CHUNK + jj];
      if (BWD) {
        const float hv = rr < N ? a.h[(size_t)rr * Cr + j] : 0.f;
        v = hv > 0.f ? v : 0.f;
      } else {
        v += a.b1[j];
        v = v > 0.f ? v : 0.f;
      }
      ht[r * hp + j] = v;
      if (first && rr < N) (BWD ? a.dh : a.h)[(size_t)rr * Cr + j] = v;
    }
    __syncthreads();  // the tile's columns are complete (and the partials free for the next pass)
  }

  for (int t = wave; t < SEG_SLAB / 16; t += 4) {
    const int col = blockIdx.y * SEG_SLAB + t * 16 + l16;
    if (col - l16 >= C) break;   // (C % 16 == 0: a tile is whole or absent)
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < Cr; kb += 4 * SEG_U) {
      float bv[SEG_U];
#pragma unroll
      for (int i = 0; i < SEG_U; ++i) {
        const int k = kb + 4 * i + g4;
        bv[i] = 0.f;
        if (kb + 4 * i < Cr) bv[i] = BWD ? a.w1[(size_t)col * Cr + k] : a.w2[(size_t)k * C + col];
      }
#pragma unroll
      for (int i = 0; i < SEG_U; ++i) {
        const float av = kb + 4 * i < Cr ? ht[l16 * hp + kb + 4 * i + g4] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[i], acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int r = n0 + 4 * g4 + v;
      if (r < N) {
        if (BWD) {
          a.dzs[(size_t)r * C + col] = acc[v] * a.inv_hw;
        } else {
          const float x = acc[v] + a.b2[col];
          a.s[(size_t)r * C + col] = 1.f / (1.f + expf(-x));
        }
      }
    }
  }
}

// dW1 [C][Cr] = z^T dh, db1 = sum_n dh, dW2 [Cr][C] = h^T dl2, db2 = sum_n dl2: a wave per 16 x 16
// tile of X^T Y (X [N][P], Y [N][Q]), all samples in order
__global__ __launch_bounds__(256) void se_gate_wgrad_kernel(DrnSeArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, g4 = lane >> 4;
  const int C = a.C, Cr = a.Cr, N = a.N;
  const int ntile = (C >> 4) * ((Cr + 15) >> 4);
  int t = blockIdx.x * 4 + wave;
  if (t >= 2 * ntile) return;
  const bool second = t >= ntile;
  if (second) t -= ntile;
  const float* __restrict__ X = second ? a.h : a.z;
  const float* __restrict__ Y = second ? a.dl2 : a.dh;
  const int P = second ? Cr : C, Q = second ? C : Cr;
  float* out = second ? a.dw2 : a.dw1;
  float* bias = second ? a.db2 : a.db1;
  const int qt = (Q + 15) >> 4;
  const int pi = t / qt, qi = t - pi * qt;
  const int p = pi * 16 + l16, q = qi * 16 + l16;
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  for (int n0 = 0; n0 < N; n0 += 4) {
    const int n = n0 + g4;
    const float av = (n < N && p < P) ? X[(size_t)n * P + p] : 0.f;
    const float bv = (n < N && q < Q) ? Y[(size_t)n * Q + q] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int pr = pi * 16 + 4 * g4 + v;
    if (pr < P && q < Q) out[(size_t)pr * Q + q] = acc[v];
  }
  if (pi == 0 && g4 == 0 && q < Q) {
    float sum = 0.f;
    for (int n = 0; n < N; ++n) sum += Y[(size_t)n * Q + q];
    bias[q] = sum;
  }
}

static bool se_domain(const DrnSeArgs* a) {
  return a->N >= 1 && a->N <= 65535 && a->HW >= 1 && a->C >= 16 && a->C <= 4096 && a->C % 16 == 0 && a->Cr >= 8 &&
         a->Cr <= SEG_MAX_CR && a->Cr % 8 == 0;
}

// The streaming kernels' thread layout for C channels
static void se_walk(DrnSeArgs* a) {
  a->slab = a->C < SE_SLAB ? a->C : SE_SLAB;
  a->cpw = a->slab / 8;
  a->planes = 256 / a->cpw;
}

// Pixel splits per sample: about 2048 workgroups, at least two pixels per thread, at most SE_MAX_SPLIT
static int se_splits(int N, int HW, int C) {
  DrnSeArgs a{};
  a.C = C;
  se_walk(&a);
  const int64_t wgs = (int64_t)N * ((C + SE_SLAB - 1) / SE_SLAB);
  int64_t s = 2048 / wgs;
  const int by_rows = HW / (2 * a.planes);
  if (s > by_rows) s = by_rows;
  if (s > SE_MAX_SPLIT) s = SE_MAX_SPLIT;
  if (s < 1) s = 1;
  const int pps = (HW + (int)s - 1) / (int)s;
  return (HW + pps - 1) / pps;
}

template <typename K>
static int se_lds_attr(K kern, std::atomic<uint64_t>* done) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  const uint64_t bit = (uint64_t)1 << (dev & 63);
  if (dev < 64 && (done->load(std::memory_order_acquire) & bit)) return 0;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, SEG_LDS);
  if (e != hipSuccess) return (int)e;
  done->fetch_or(bit, std::memory_order_release);
  return 0;
}

template <bool BWD>
static int se_gate_launch(DrnSeArgs* a, hipStream_t s) {
  static std::atomic<uint64_t> attr{0};
  auto kern = se_gate_kernel<BWD>;
  if (const int rc = se_lds_attr(kern, &attr)) return rc;
  a->inv_hw = 1.0f / (float)a->HW;
  const size_t lds = (size_t)(4 * 16 * SEG_CHUNK + 16 * (a->Cr + 4)) * 4;
  drn::launch(kern, dim3((a->N + 15) / 16, (a->C + SEG_SLAB - 1) / SEG_SLAB), dim3(256), lds, s, *a);
  return (int)hipGetLastError();
}

template <bool BWD>
static int se_stream_launch(DrnSeArgs* a, hipStream_t s) {
  se_walk(a);
  a->S = se_splits(a->N, a->HW, a->C);
  a->pps = (a->HW + a->S - 1) / a->S;
  const int nz = a->N < SE_STAT_WGS / a->S ? a->N : SE_STAT_WGS / a->S;
  drn::launch(se_stream_kernel<BWD>, dim3((a->C + SE_SLAB - 1) / SE_SLAB, a->S, nz), dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

}  // namespace drn

DRN_API int drn_se_args_size() { return (int)sizeof(DrnSeArgs); }

// Pixel splits S of drn_se_squeeze for this geometry (the cells are [N][S][C]); 0: outside the domain
DRN_API int drn_se_splits(int N, int HW, int C) {
  DrnSeArgs a{};
  a.N = N, a.HW = HW, a.C = C, a.Cr = 8;
  return drn::se_domain(&a) ? drn::se_splits(N, HW, C) : 0;
}

// cells[N][S][C] = per-split sums of x (of x * y when y is given); S = drn_se_splits
DRN_API int drn_se_squeeze(DrnSeArgs* a, hipStream_t s) {
  if (!drn::se_domain(a) || a->x == nullptr || a->cells == nullptr) return (int)hipErrorInvalidValue;
  if (a->S != drn::se_splits(a->N, a->HW, a->C)) return (int)hipErrorInvalidValue;
  drn::se_walk(a);
  a->pps = (a->HW + a->S - 1) / a->S;
  drn::launch(drn::se_squeeze_kernel, dim3((a->C + drn::SE_SLAB - 1) / drn::SE_SLAB, a->S, a->N), dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

// z, h, s from the cells of u (reads cells, w1, b1, w2, b2)
DRN_API int drn_se_gate_fwd(DrnSeArgs* a, hipStream_t s) {
  if (!drn::se_domain(a) || a->S < 1 || !a->cells || !a->w1 || !a->b1 || !a->w2 || !a->b2 || !a->z || !a->h || !a->s)
    return (int)hipErrorInvalidValue;
  return drn::se_gate_launch<false>(a, s);
}

// out = shortcut (y) + s * u (x), + statistics of the stored out
DRN_API int drn_se_excite(DrnSeArgs* a, hipStream_t s) {
  if (!drn::se_domain(a) || !a->x || !a->y || !a->out || !a->s) return (int)hipErrorInvalidValue;
  if (a->stats != nullptr && a->stats_rep < 1) return (int)hipErrorInvalidValue;
  return drn::se_stream_launch<false>(a, s);
}

// dl2, dh, dzs from the cells of g * u (reads cells, s, h, w1, w2)
DRN_API int drn_se_gate_bwd(DrnSeArgs* a, hipStream_t s) {
  if (!drn::se_domain(a) || a->S < 1 || !a->cells || !a->w1 || !a->w2 || !a->h || !a->s || !a->dl2 || !a->dh || !a->dzs)
    return (int)hipErrorInvalidValue;
  return drn::se_gate_launch<true>(a, s);
}

// dw1, db1, dw2, db2 from z, h, dl2, dh
DRN_API int drn_se_gate_wgrad(DrnSeArgs* a, hipStream_t s) {
  if (!drn::se_domain(a) || !a->z || !a->h || !a->dl2 || !a->dh || !a->dw1 || !a->db1 || !a->dw2 || !a->db2)
    return (int)hipErrorInvalidValue;
  const int ntile = (a->C / 16) * ((a->Cr + 15) / 16);
  drn::launch(drn::se_gate_wgrad_kernel, dim3((2 * ntile + 3) / 4), dim3(256), 0, s, *a);
  return (int)hipGetLastError();
}

// du (out) = s * g (x) + dzs
DRN_API int drn_se_scale_bwd(DrnSeArgs* a, hipStream_t s) {
  if (!drn::se_domain(a) || !a->x || !a->out || !a->s || !a->dzs) return (int)hipErrorInvalidValue;
  a->stats = nullptr;
  return drn::se_stream_launch<true>(a, s);
}
