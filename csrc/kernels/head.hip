// head.hip — classifier head on gfx950: final BN-ReLU + global average pool, dense layer
// (fp32 GEMMs), softmax cross-entropy with one-hot labels and the batch precision metric, and its
// label-smoothing / top-k variant (softmax_xent_ex_kernel), and that against the two-label target of
// Mixup / CutMix (softmax_xent_mix_kernel).
//
// Reference: final batch_norm_relu + average_pooling2d(VALID, pool = H) + dense
// (resnet_model_official.py:268-275 CIFAR, :336-343 ImageNet); softmax + mean
// softmax_cross_entropy (resnet_model.py:77-80); train "precision" = mean(argmax p == argmax y)
// (resnet_cifar_main.py:270-272).
#include "drn_common.h"

namespace drn {

// pooled[n][c] = mean_hw relu(x[n][hw][c]*scale[c] + shift[c])   (scale==nullptr: no BN)
__global__ __launch_bounds__(256) void bnrelu_pool_kernel(const bf16_t* __restrict__ x, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, float* __restrict__ pooled,
                                                          int HW, int C, int relu) {
  const int n = blockIdx.x;
  const int CV = C / 8;
  for (int cv = threadIdx.x; cv < CV; cv += blockDim.x) {
    const int c = cv * 8;
    float acc[8], sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc[j] = 0.f;
      sc[j] = scale ? scale[c + j] : 1.f;
      sh[j] = scale ? shift[c + j] : 0.f;
    }
    for (int hw = 0; hw < HW; ++hw) {
      float f[8];
      unpack8(*reinterpret_cast<const uint4*>(x + ((size_t)n * HW + hw) * C + c), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = f[j] * sc[j] + sh[j];
        if (relu) v = fmaxf(v, 0.f);
        acc[j] += v;
      }
    }
    const float inv = 1.f / (float)HW;
#pragma unroll
    for (int j = 0; j < 8; ++j) pooled[(size_t)n * C + c + j] = acc[j] * inv;
  }
}

// C[M][N] = alpha * op(A) op(B) + beta * C (+ bias[N]); row-major; op = transpose if flag.
// Exact-fp32 MFMA (v_mfma_f32_16x16x4_f32, the f32-input matrix path: 16x the VALU-FMA work
// per instruction, bitwise a k-ordered fmaf chain). 64x64 block tile, 4 waves each 32x32
// (2x2 MFMA tiles), K staged 32 at a time through double-buffered LDS ([k][m] and [k][n], +1
// padding): the next slab's global loads are issued into registers before the current slab's
// MFMAs and stored to the other buffer after them (one barrier per slab), so their latency
// hides behind the MFMA chain -- the unpipelined load/barrier/MFMA loop, one workgroup per CU,
// was latency-bound (60 us for the 0.5 GFLOP ResNet-50 logits GEMM).
// Used for the dense layer of the head (logits, dW, dpool: <1 GFLOP each).
__global__ __launch_bounds__(256) void sgemm_kernel(int ta, int tb, int M, int N, int K, float alpha,
                                                    const float* __restrict__ A, int lda,
                                                    const float* __restrict__ B, int ldb, float beta,
                                                    float* __restrict__ Cm, int ldc, const float* __restrict__ bias) {
  constexpr int BM = 64, BN = 64, BK = 32;
  constexpr int LA = BK * BM / 256, LB = BK * BN / 256;  // slab elements per thread
  __shared__ float As[2][BK][BM + 1];
  __shared__ float Bs[2][BK][BN + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  // split-K over gridDim.z: slice z sums k in [kb, ke) and writes its partial tile to
  // Cm + z * M * ldc (beta/bias are then applied by sgemm_finish_kernel)
  const int ksz = (((K + gridDim.z - 1) / gridDim.z) + BK - 1) / BK * BK;
  const int kb = blockIdx.z * ksz, ke = min(K, kb + ksz);
  if (gridDim.z > 1) {
    Cm += (size_t)blockIdx.z * M * ldc;
    beta = 0.f;
    bias = nullptr;
    alpha = 1.f;
  }
  f32x4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  // element t of a slab: A at [k][m] = (t / BM, t % BM) when transposed (m contiguous in
  // memory), else (t % BK, t / BK) (k contiguous); likewise B with n
  float ra[LA], rb[LB];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      const int t = tid + 256 * i;
      const int kk = ta ? t / BM : t % BK, mm = ta ? t % BM : t / BK;
      const int gm = m0 + mm, gk = k0 + kk;
      ra[i] = (gm < M && gk < ke) ? (ta ? A[(size_t)gk * lda + gm] : A[(size_t)gm * lda + gk]) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < LB; ++i) {
      const int t = tid + 256 * i;
      const int kk = tb ? t % BK : t / BN, nn = tb ? t / BK : t % BN;
      const int gn = n0 + nn, gk = k0 + kk;
      rb[i] = (gn < N && gk < ke) ? (tb ? B[(size_t)gn * ldb + gk] : B[(size_t)gk * ldb + gn]) : 0.f;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      const int t = tid + 256 * i;
      As[buf][ta ? t / BM : t % BK][ta ? t % BM : t / BK] = ra[i];
    }
#pragma unroll
    for (int i = 0; i < LB; ++i) {
      const int t = tid + 256 * i;
      Bs[buf][tb ? t % BK : t / BN][tb ? t / BK : t % BN] = rb[i];
    }
  };
  if (kb < ke) {
    load(kb);
    store(0);
  }
  __syncthreads();
  int buf = 0;
  for (int k0 = kb; k0 < ke; k0 += BK) {
    const bool more = k0 + BK < ke;
    if (more) load(k0 + BK);  // in flight during this slab's MFMAs
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      const int kr = kk + (lane >> 4);
      float a0 = As[buf][kr][wm + (lane & 15)], a1 = As[buf][kr][wm + 16 + (lane & 15)];
      float b0 = Bs[buf][kr][wn + (lane & 15)], b1 = Bs[buf][kr][wn + 16 + (lane & 15)];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    // the other buffer was last read before the previous barrier: safe to overwrite
    if (more) store(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gm = m0 + wm + 16 * i + 4 * (lane >> 4) + r;
        const int gn = n0 + wn + 16 * j + (lane & 15);
        if (gm < M && gn < N) {
          float v = alpha * acc[i][j][r];
          if (bias) v += bias[gn];
          if (beta != 0.f) v += beta * Cm[(size_t)gm * ldc + gn];
          Cm[(size_t)gm * ldc + gn] = v;
        }
      }
}

// C = alpha * sum_z ws[z] + beta * C (+ bias), fixed summation order (deterministic).
__global__ void sgemm_finish_kernel(const float* __restrict__ ws, int splits, int M, int N, int ldc, float alpha,
                                    float beta, float* __restrict__ Cm, const float* __restrict__ bias) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= M * N) return;
  const int m = idx / N, n = idx - m * N;
  float s = 0.f;
  for (int z = 0; z < splits; ++z) s += ws[(size_t)z * M * ldc + (size_t)m * ldc + n];
  float v = alpha * s;
  if (bias) v += bias[n];
  if (beta != 0.f) v += beta * Cm[(size_t)m * ldc + n];
  Cm[(size_t)m * ldc + n] = v;
}

// One block per sample: softmax, loss, dlogits = (p - y) * grad_scale, correct-count.
// labels: int32 class ids. out_loss[n] per-sample loss; probs optional.
__global__ __launch_bounds__(256) void softmax_xent_kernel(const float* __restrict__ logits,
                                                           const int* __restrict__ labels, int ncls,
                                                           float grad_scale, float* __restrict__ dlogits,
                                                           float* __restrict__ loss, float* __restrict__ probs,
                                                           int* __restrict__ correct) {
  const int n = blockIdx.x;
  const float* z = logits + (size_t)n * ncls;
  __shared__ float sred[8];
  __shared__ int sidx[8];
  float mx = -INFINITY;
  int amax = 0;
  for (int j = threadIdx.x; j < ncls; j += blockDim.x) {
    const float v = z[j];
    if (v > mx) { mx = v; amax = j; }
  }
  // block argmax (first index of the max)
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(mx, o, 64);
    const int oi = __shfl_xor(amax, o, 64);
    if (ov > mx || (ov == mx && oi < amax)) { mx = ov; amax = oi; }
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = blockDim.x >> 6;
  if (l == 0) { sred[w] = mx; sidx[w] = amax; }
  __syncthreads();
  mx = sred[0]; amax = sidx[0];
  for (int i = 1; i < nw; ++i)
    if (sred[i] > mx || (sred[i] == mx && sidx[i] < amax)) { mx = sred[i]; amax = sidx[i]; }
  __syncthreads();
  float se = 0.f;
  for (int j = threadIdx.x; j < ncls; j += blockDim.x) se += __expf(z[j] - mx);
  se = wave_sum(se);
  if (l == 0) sred[w] = se;
  __syncthreads();
  se = 0.f;
  for (int i = 0; i < nw; ++i) se += sred[i];
  const int y = labels[n];
  const float lse = mx + __logf(se);
  const float inv = 1.f / se;
  for (int j = threadIdx.x; j < ncls; j += blockDim.x) {
    const float p = __expf(z[j] - mx) * inv;
    if (probs) probs[(size_t)n * ncls + j] = p;
    if (dlogits) dlogits[(size_t)n * ncls + j] = (p - (j == y ? 1.f : 0.f)) * grad_scale;
  }
  if (threadIdx.x == 0) {
    loss[n] = lse - z[y];
    if (correct) correct[n] = (amax == y) ? 1 : 0;
  }
}

// softmax_xent_kernel with a smoothed target and a top-k count (one block per sample, one launch):
//   t_j     = (1 - eps) [j == y] + eps / K                     (K = ncls, eps = smoothing)
//   loss    = log(se) - (1 - eps) (z_y - mx) - (eps / K) sum_j (z_j - mx)
//   dlogits = (p_j - t_j) * grad_scale
//   rank    = #{j : z_j > z_y} + #{j < y : z_j == z_y};  correct_k = rank < top_k (0 for a NaN z_y)
// The max / argmax and the sum of exponentials are reduced exactly as in softmax_xent_kernel
// (256 threads striding the row, wave reduction, waves in index order), so at eps = 0 probs,
// dlogits and loss are the same bits and correct is the same rule; the two extra reductions (the rank
// count, an integer, and sum_j (z_j - mx)) ride along the same two barriers. REG: rows of up to
// 8 * 256 classes are read from memory once and kept in 8 registers per thread; longer rows are
// re-read like softmax_xent_kernel does. A label outside [0, ncls) reads nothing: its loss is NaN,
// its counts 0 and its gradient the plain p_j - eps / K.
constexpr int XENT_REG_ROW = 8;  // row elements per thread held in registers

template <bool REG>
__global__ __launch_bounds__(256) void softmax_xent_ex_kernel(const float* __restrict__ logits,
                                                              const int* __restrict__ labels, int ncls,
                                                              float grad_scale, float smoothing, int top_k,
                                                              float* __restrict__ dlogits, float* __restrict__ loss,
                                                              float* __restrict__ probs, int* __restrict__ correct,
                                                              int* __restrict__ correct_k) {
  const int n = blockIdx.x;
  const float* z = logits + (size_t)n * ncls;
  __shared__ float sred[8], ssum[8];
  __shared__ int sidx[8], scnt[8];
  const int y = labels[n];
  const bool yok = (unsigned)y < (unsigned)ncls;
  const float zy = yok ? z[y] : __builtin_nanf("");
  const int iters = REG ? XENT_REG_ROW : (ncls + 255) / 256;
  float r[XENT_REG_ROW];
  if (REG) {
#pragma unroll
    for (int i = 0; i < XENT_REG_ROW; ++i) {
      const int j = threadIdx.x + 256 * i;
      r[i] = j < ncls ? z[j] : -INFINITY;
    }
  }
  // element i of this thread's stride (j = threadIdx.x + 256 * i < ncls)
  auto at = [&](int i, int j) { return REG ? r[i] : z[j]; };
  float mx = -INFINITY;
  int amax = 0, cnt = 0;
#pragma unroll
  for (int i = 0; i < iters; ++i) {
    const int j = threadIdx.x + 256 * i;
    if (j < ncls) {
      const float v = at(i, j);
      if (v > mx) { mx = v; amax = j; }
      cnt += (v > zy || (v == zy && j < y)) ? 1 : 0;
    }
  }
  // block argmax (first index of the max) and the rank count
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(mx, o, 64);
    const int oi = __shfl_xor(amax, o, 64);
    if (ov > mx || (ov == mx && oi < amax)) { mx = ov; amax = oi; }
    cnt += __shfl_xor(cnt, o, 64);
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = blockDim.x >> 6;
  if (l == 0) { sred[w] = mx; sidx[w] = amax; scnt[w] = cnt; }
  __syncthreads();
  mx = sred[0]; amax = sidx[0]; cnt = scnt[0];
  for (int i = 1; i < nw; ++i) {
    if (sred[i] > mx || (sred[i] == mx && sidx[i] < amax)) { mx = sred[i]; amax = sidx[i]; }
    cnt += scnt[i];
  }
  __syncthreads();
  float se = 0.f, sz = 0.f;
#pragma unroll
  for (int i = 0; i < iters; ++i) {
    const int j = threadIdx.x + 256 * i;
    if (j < ncls) {
      const float d = at(i, j) - mx;
      se += __expf(d);
      sz += d;
    }
  }
  se = wave_sum(se);
  sz = wave_sum(sz);
  if (l == 0) { sred[w] = se; ssum[w] = sz; }
  __syncthreads();
  se = 0.f; sz = 0.f;
  for (int i = 0; i < nw; ++i) { se += sred[i]; sz += ssum[i]; }
  const float inv = 1.f / se;
  const float uni = smoothing / (float)ncls, hot = 1.f - smoothing;
#pragma unroll
  for (int i = 0; i < iters; ++i) {
    const int j = threadIdx.x + 256 * i;
    if (j < ncls) {
      const float p = __expf(at(i, j) - mx) * inv;
      if (probs) probs[(size_t)n * ncls + j] = p;
      if (dlogits) dlogits[(size_t)n * ncls + j] = (p - (j == y ? hot : 0.f) - uni) * grad_scale;
    }
  }
  if (threadIdx.x == 0) {
    // eps = 0: softmax_xent_kernel's own expression (the same bits; and no 0 * inf from a -inf logit)
    loss[n] = smoothing == 0.f ? (mx + __logf(se)) - zy : __logf(se) - hot * (zy - mx) - uni * sz;
    if (correct) correct[n] = (amax == y) ? 1 : 0;
    if (correct_k) correct_k[n] = (zy == zy && cnt < top_k) ? 1 : 0;
  }
}

// softmax_xent_ex_kernel against a target mixed from two labels (Mixup / CutMix): sample n's second
// label yb and weight lam come from its record of the batch's mix table (csrc/kernels/mix.hip
// MixRec), read from device memory when the kernel runs, so a graph or plan replay follows the
// table of its batch:
//   t_j     = (1 - eps) (lam [j == ya] + (1 - lam) [j == yb]) + eps / K
//   loss    = log(se) - (1 - eps) (lam (z_ya - mx) + (1 - lam) (z_yb - mx)) - (eps / K) sum_j (z_j - mx)
//   dlogits = (p_j - t_j) * grad_scale
// correct / correct_k: the rank rule against the dominant label (ya if lam >= 0.5, else yb).
// A separate kernel, not a flag of softmax_xent_ex_kernel: that one's code stays as it is. The
// reductions are its reductions in its order, and a record with lam == 1 takes its expressions (yb
// is then not read at all, whatever its value), so with lam == 1 everywhere every output is its
// bits. A yb outside [0, ncls) with lam != 1 reads nothing either: NaN loss, like a bad label.
struct XentMixRec {  // mix.hip MixRec
  float w, lam;
  int32_t y0, x0, y1, x1;
  int32_t label_b, pad_;
};
static_assert(sizeof(XentMixRec) == 32, "the 32-byte mix record");

template <bool REG>
__global__ __launch_bounds__(256) void softmax_xent_mix_kernel(const float* __restrict__ logits,
                                                               const int* __restrict__ labels,
                                                               const XentMixRec* __restrict__ table, int ncls,
                                                               float grad_scale, float smoothing, int top_k,
                                                               float* __restrict__ dlogits, float* __restrict__ loss,
                                                               float* __restrict__ probs, int* __restrict__ correct,
                                                               int* __restrict__ correct_k) {
  const int n = blockIdx.x;
  const float* z = logits + (size_t)n * ncls;
  __shared__ float sred[8], ssum[8];
  __shared__ int sidx[8], scnt[8];
  const int ya = labels[n];
  const float lam = table[n].lam;
  const bool pure = lam == 1.f;
  const int yb = pure ? -1 : table[n].label_b;
  const bool aok = (unsigned)ya < (unsigned)ncls, bok = (unsigned)yb < (unsigned)ncls;
  const float zya = aok ? z[ya] : __builtin_nanf("");
  const float zyb = bok ? z[yb] : __builtin_nanf("");
  // the dominant label: what correct / correct_k are counted against
  const bool dom_a = lam >= 0.5f;
  const int y = dom_a ? ya : yb;
  const float zy = dom_a ? zya : zyb;
  const int iters = REG ? XENT_REG_ROW : (ncls + 255) / 256;
  float r[XENT_REG_ROW];
  if (REG) {
#pragma unroll
    for (int i = 0; i < XENT_REG_ROW; ++i) {
      const int j = threadIdx.x + 256 * i;
      r[i] = j < ncls ? z[j] : -INFINITY;
    }
  }
  auto at = [&](int i, int j) { return REG ? r[i] : z[j]; };
  float mx = -INFINITY;
  int amax = 0, cnt = 0;
#pragma unroll
  for (int i = 0; i < iters; ++i) {
    const int j = threadIdx.x + 256 * i;
    if (j < ncls) {
      const float v = at(i, j);
      if (v > mx) { mx = v; amax = j; }
      cnt += (v > zy || (v == zy && j < y)) ? 1 : 0;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(mx, o, 64);
    const int oi = __shfl_xor(amax, o, 64);
    if (ov > mx || (ov == mx && oi < amax)) { mx = ov; amax = oi; }
    cnt += __shfl_xor(cnt, o, 64);
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, nw = blockDim.x >> 6;
  if (l == 0) { sred[w] = mx; sidx[w] = amax; scnt[w] = cnt; }
  __syncthreads();
  mx = sred[0]; amax = sidx[0]; cnt = scnt[0];
  for (int i = 1; i < nw; ++i) {
    if (sred[i] > mx || (sred[i] == mx && sidx[i] < amax)) { mx = sred[i]; amax = sidx[i]; }
    cnt += scnt[i];
  }
  __syncthreads();
  float se = 0.f, sz = 0.f;
#pragma unroll
  for (int i = 0; i < iters; ++i) {
    const int j = threadIdx.x + 256 * i;
    if (j < ncls) {
      const float d = at(i, j) - mx;
      se += __expf(d);
      sz += d;
    }
  }
  se = wave_sum(se);
  sz = wave_sum(sz);
  if (l == 0) { sred[w] = se; ssum[w] = sz; }
  __syncthreads();
  se = 0.f; sz = 0.f;
  for (int i = 0; i < nw; ++i) { se += sred[i]; sz += ssum[i]; }
  const float inv = 1.f / se;
  const float uni = smoothing / (float)ncls, hot = 1.f - smoothing;
  // the two hot entries of the target; lam == 1: (hot, nothing), softmax_xent_ex_kernel's row
  const float ha = pure ? hot : hot * lam, hb = hot * (1.f - lam);
#pragma unroll
  for (int i = 0; i < iters; ++i) {
    const int j = threadIdx.x + 256 * i;
    if (j < ncls) {
      const float p = __expf(at(i, j) - mx) * inv;
      if (probs) probs[(size_t)n * ncls + j] = p;
      if (dlogits) {
        float t = j == ya ? ha : 0.f;
        if (j == yb) t += hb;
        dlogits[(size_t)n * ncls + j] = (p - t - uni) * grad_scale;
      }
    }
  }
  if (threadIdx.x == 0) {
    float ls;
    if (pure) {
      ls = smoothing == 0.f ? (mx + __logf(se)) - zya : __logf(se) - hot * (zya - mx) - uni * sz;
    } else {
      const float mz = lam * (zya - mx) + (1.f - lam) * (zyb - mx);
      ls = smoothing == 0.f ? __logf(se) - mz : __logf(se) - hot * mz - uni * sz;
    }
    loss[n] = ls;
    if (correct) correct[n] = (amax == y) ? 1 : 0;
    if (correct_k) correct_k[n] = (zy == zy && cnt < top_k) ? 1 : 0;
  }
}

// column sums: out[j] = scale * sum_n in[n][j]  (dense bias gradient)
// Column sums (the dense bias gradient, sum over the batch of dlogits): a block covers 32
// columns with 8 row slices of 32 lanes (coalesced 128-byte row segments, 4 independent loads
// in flight per lane), then a fixed-order LDS reduction over the slices (deterministic). The
// earlier one-thread-per-column loop ran 128 dependent-latency iterations: ~47 us for 128 x 1001.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ in, int rows, int cols,
                                                     float* __restrict__ out, float scale, int accumulate) {
  __shared__ float red[8][33];
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int j = blockIdx.x * 32 + cl;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (j < cols) {
    int n = sl;
    for (; n + 24 < rows; n += 32) {
      s0 += in[(size_t)n * cols + j];
      s1 += in[(size_t)(n + 8) * cols + j];
      s2 += in[(size_t)(n + 16) * cols + j];
      s3 += in[(size_t)(n + 24) * cols + j];
    }
    for (; n < rows; n += 8) s0 += in[(size_t)n * cols + j];
  }
  red[sl][cl] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (sl == 0 && j < cols) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += red[k][cl];
    out[j] = accumulate ? out[j] + scale * s : scale * s;
  }
}

}  // namespace drn

DRN_API int drn_bnrelu_pool(const void* x, const float* scale, const float* shift, float* pooled, int N, int HW,
                            int C, int relu, hipStream_t s) {
  if (C % 8) return (int)hipErrorInvalidValue;
  drn::launch(drn::bnrelu_pool_kernel, dim3(N), dim3(256), 0, s, (const bf16_t*)x, scale, shift, pooled, HW, C,
                     relu);
  return (int)hipGetLastError();
}

// splits > 1 needs ws with room for splits * M * ldc floats.
DRN_API int drn_sgemm(int ta, int tb, int M, int N, int K, float alpha, const float* A, int lda, const float* B,
                      int ldb, float beta, float* C, int ldc, const float* bias, int splits, float* ws,
                      hipStream_t s) {
  if (splits < 1 || (splits > 1 && ws == nullptr)) return (int)hipErrorInvalidValue;
  dim3 grid((N + 63) / 64, (M + 63) / 64, splits);
  drn::launch(drn::sgemm_kernel, grid, dim3(256), 0, s, ta, tb, M, N, K, alpha, A, lda, B, ldb, beta,
                     splits > 1 ? ws : C, ldc, bias);
  if (splits > 1)
    drn::launch(drn::sgemm_finish_kernel, dim3((M * N + 255) / 256), dim3(256), 0, s, ws, splits, M, N, ldc,
                       alpha, beta, C, bias);
  return (int)hipGetLastError();
}

DRN_API int drn_softmax_xent(const float* logits, const int* labels, int N, int ncls, float grad_scale,
                             float* dlogits, float* loss, float* probs, int* correct, hipStream_t s) {
  drn::launch(drn::softmax_xent_kernel, dim3(N), dim3(256), 0, s, logits, labels, ncls, grad_scale, dlogits,
                     loss, probs, correct);
  return (int)hipGetLastError();
}

// drn_softmax_xent with label smoothing (0 <= smoothing < 1) and a top-k count (top_k >= 1):
// dlogits, probs, correct and correct_k may each be null.
DRN_API int drn_softmax_xent_ex(const float* logits, const int* labels, int N, int ncls, float grad_scale,
                                float smoothing, int top_k, float* dlogits, float* loss, float* probs, int* correct,
                                int* correct_k, hipStream_t s) {
  if (!(smoothing >= 0.f && smoothing < 1.f) || top_k < 1 || N < 1 || ncls < 1) return (int)hipErrorInvalidValue;
  auto kern = ncls <= 256 * drn::XENT_REG_ROW ? drn::softmax_xent_ex_kernel<true> : drn::softmax_xent_ex_kernel<false>;
  drn::launch(kern, dim3(N), dim3(256), 0, s, logits, labels, ncls, grad_scale, smoothing, top_k, dlogits, loss,
                     probs, correct, correct_k);
  return (int)hipGetLastError();
}

// drn_softmax_xent_ex against the two-label target of a mix table (N 32-byte records in device
// memory, csrc/kernels/mix.hip): one launch, one workgroup per sample.
DRN_API int drn_softmax_xent_mix(const float* logits, const int* labels, const void* table, int N, int ncls,
                                 float grad_scale, float smoothing, int top_k, float* dlogits, float* loss,
                                 float* probs, int* correct, int* correct_k, hipStream_t s) {
  if (!(smoothing >= 0.f && smoothing < 1.f) || top_k < 1 || N < 1 || ncls < 1 || table == nullptr)
    return (int)hipErrorInvalidValue;
  auto kern = ncls <= 256 * drn::XENT_REG_ROW ? drn::softmax_xent_mix_kernel<true> : drn::softmax_xent_mix_kernel<false>;
  drn::launch(kern, dim3(N), dim3(256), 0, s, logits, labels, (const drn::XentMixRec*)table, ncls, grad_scale,
                     smoothing, top_k, dlogits, loss, probs, correct, correct_k);
  return (int)hipGetLastError();
}

DRN_API int drn_colsum(const float* in, int rows, int cols, float* out, float scale, int accumulate, hipStream_t s) {
  drn::launch(drn::colsum_kernel, dim3((cols + 31) / 32), dim3(256), 0, s, in, rows, cols, out, scale,
                     accumulate);
  return (int)hipGetLastError();
}
