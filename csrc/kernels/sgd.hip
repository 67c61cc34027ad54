// sgd.hip — fused optimizer step and weight-layout maintenance on gfx950.
//
// Replaces TF's per-variable ApplyMomentum + L2Loss/AddN gradient of the weight-decay term
// (reference resnet_model.py:85-86 cost = xent + wd * sum(l2_loss(v)) over ALL trainable vars;
// :98-99 MomentumOptimizer(lr, 0.9), non-Nesterov) with ONE launch over the flat fp32
// master buffer (all 152/153 variables back to back):
//   g' = g * grad_scale + wd * w ;  m = mu * m + g' ;  w -= lr * m ;  w_bf16 = bf16(w)
// grad_scale folds the 1/world_size of the data-parallel average (SyncReplicas/Horovod mean).
// The learning rate is read from device memory so a captured HIP graph replays with the
// per-step LR written by the host (the reference feeds it through feed_dict each step,
// resnet_cifar_main.py:293-296).
#include "drn_common.h"

namespace drn {

// gradient element type: fp32 (local / fp32-wire gradients) or bf16 (the all-reduced bf16 wire
// buffer, consumed directly: no cast-back pass, half the gradient bytes)
__device__ __forceinline__ float4 grad4(const float* g, int64_t i) { return reinterpret_cast<const float4*>(g)[i]; }
__device__ __forceinline__ float4 grad4(const bf16_t* g, int64_t i) {
  const uint2 u = reinterpret_cast<const uint2*>(g)[i];
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}
__device__ __forceinline__ float grad1(const float* g, int64_t i) { return g[i]; }
__device__ __forceinline__ float grad1(const bf16_t* g, int64_t i) { return bf2f(g[i]); }

// Element updates g' -> m -> w of a float4, and of one element for the tail of a LARS slot. The two
// differ on purpose (what the compiler may contract into FMAs);
// test_lars_with_unit_trust_is_the_momentum_kernel pins that trust == 1 gives the momentum bits.
struct MomentumUpd {
  float lr, mu, wd, grad_scale;
  __device__ __forceinline__ void operator()(float& wv, float& mv, float gv) const {
    const float gg = gv * grad_scale + wd * wv; mv = mu * mv + gg; wv -= lr * mv;
  }
};
struct LarsUpd {
  float lr, mu, wd, grad_scale, trust;
  __device__ __forceinline__ void operator()(float& wv, float& mv, float gv) const {
    const float gg = trust * (gv * grad_scale + wd * wv);
    mv = __builtin_fmaf(mu, mv, gg);
    wv -= lr * mv;
  }
};
template <typename U>
__device__ __forceinline__ void upd4(const U& upd, float4& wv, float4& mv, const float4& gv) {
  upd(wv.x, mv.x, gv.x); upd(wv.y, mv.y, gv.y); upd(wv.z, mv.z, gv.z); upd(wv.w, mv.w, gv.w);
}

template <typename G>
__global__ __launch_bounds__(256) void sgd_momentum_kernel(float* __restrict__ w, float* __restrict__ m,
                                                           const G* __restrict__ g, bf16_t* __restrict__ wb,
                                                           int64_t n4, const float* __restrict__ lr_ptr, float mu,
                                                           float wd, float grad_scale, const int* __restrict__ skip) {
  // skip: the step's gradient exchange failed (P2P error word): apply no update at all
  if (skip != nullptr && *skip != 0) return;
  const float lr = *lr_ptr;
  const MomentumUpd upd{lr, mu, wd, grad_scale};
  auto store = [&](int64_t i, const float4& wv, const float4& mv) {
    reinterpret_cast<float4*>(w)[i] = wv;
    reinterpret_cast<float4*>(m)[i] = mv;
    if (wb) {
      uint2 o;
      o.x = pack2bf(wv.x, wv.y);
      o.y = pack2bf(wv.z, wv.w);
      reinterpret_cast<uint2*>(wb)[i] = o;
    }
  };
  // two float4 groups in flight per thread (3 streams read, 3 written: one group per iteration
  // left the pass latency-bound at ~4.3 TB/s)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) {
    float4 w0 = reinterpret_cast<float4*>(w)[i], w1 = reinterpret_cast<float4*>(w)[i + stride];
    float4 m0 = reinterpret_cast<float4*>(m)[i], m1 = reinterpret_cast<float4*>(m)[i + stride];
    const float4 g0 = grad4(g, i), g1 = grad4(g, i + stride);
    upd4(upd, w0, m0, g0);
    upd4(upd, w1, m1, g1);
    store(i, w0, m0);
    store(i + stride, w1, m1);
  }
  if (i < n4) {
    float4 w0 = reinterpret_cast<float4*>(w)[i];
    float4 m0 = reinterpret_cast<float4*>(m)[i];
    const float4 g0 = grad4(g, i);
    upd4(upd, w0, m0, g0);
    store(i, w0, m0);
  }
}

// ---------------------------------------------------------------------------------------------
// LARS (layer-wise adaptive rate scaling, You/Gitman/Ginsburg 2017; the apex "LARC" form):
//   wn = ||w_l||  gn = ||gs * g_l||   trust_l = eta * wn / (gn + wd * wn + eps)  (1 if wn or gn is 0,
//   1 for non-adapting slots)         g' = trust_l * (gs * g + wd * w) ; then the momentum update above.
// Two launches over a device-resident slot table (one entry per variable of the flat buffer):
// a norms pass and an update pass, both laid over (slot, chunk) pairs found through the table's
// chunk prefix sums (as weight_tflip_kernel finds its descriptor). Every partial sum has a fixed
// home in the workspace and is combined in a fixed order -- no floating-point atomics -- so every
// data-parallel rank derives bit-identical trust ratios from the same reduced gradient.
struct LarsSlot {
  int64_t offset;          // first element in the flat buffers (a multiple of 4)
  int32_t numel, padded;   // elements updated / slot length up to the next slot (padding is left alone)
  int32_t adapt, pad_;     // 0: trust = 1 (BatchNorm gamma / beta, biases)
  int64_t begin;           // prefix sum of chunk counts; entry [n] of an n-slot table holds the total
};

constexpr int LARS_CHUNK4 = 2048;  // float4 groups per chunk: 8 per thread (8192 elements)
constexpr int LARS_GRID = 2048;    // workgroups (8 per CU); each strides over the range's chunks

// slot owning chunk b (uniform scalar binary search over [s0, s0 + n))
__device__ __forceinline__ int lars_find(const LarsSlot* __restrict__ table, int s0, int n, int64_t b) {
  int lo = s0, hi = s0 + n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].begin <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// sum of (a, b) over the workgroup, identical in every thread: wave64 butterfly, then the four wave
// sums through LDS added in wave order (red: 8 floats; safe to call back to back)
__device__ __forceinline__ void lars_block_sum(float& a, float& b, float* red) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int wave = threadIdx.x >> 6;
  __syncthreads();  // the previous call's readers are done with red
  if ((threadIdx.x & 63) == 0) { red[wave] = a; red[4 + wave] = b; }
  __syncthreads();
  a = ((red[0] + red[1]) + red[2]) + red[3];
  b = ((red[4] + red[5]) + red[6]) + red[7];
}

template <typename G>
__global__ __launch_bounds__(256) void lars_norms_kernel(const float* __restrict__ w, const G* __restrict__ g,
                                                         const LarsSlot* __restrict__ table, int first_slot,
                                                         int nslots, float* __restrict__ partials, float grad_scale,
                                                         const int* __restrict__ skip) {
  __shared__ float red[8];
  if (skip != nullptr && *skip != 0) return;
  const int64_t b0 = table[first_slot].begin, b1 = table[first_slot + nslots].begin;
  for (int64_t b = b0 + blockIdx.x; b < b1; b += gridDim.x) {
    const LarsSlot d = table[lars_find(table, first_slot, nslots, b)];
    if (!d.adapt) continue;
    const int c = (int)(b - d.begin);
    const int64_t base4 = d.offset / 4;
    const int full4 = d.numel >> 2;  // whole float4 groups; the last elements of the slot go one by one
    const int i0 = c * LARS_CHUNK4;
    const int i1 = min(i0 + LARS_CHUNK4, full4);
    float sw = 0.f, sg = 0.f;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
      const float4 wv = reinterpret_cast<const float4*>(w)[base4 + i];
      float4 gv = grad4(g, base4 + i);
      gv.x *= grad_scale; gv.y *= grad_scale; gv.z *= grad_scale; gv.w *= grad_scale;
      sw += wv.x * wv.x; sw += wv.y * wv.y; sw += wv.z * wv.z; sw += wv.w * wv.w;
      sg += gv.x * gv.x; sg += gv.y * gv.y; sg += gv.z * gv.z; sg += gv.w * gv.w;
    }
    // numel % 4 trailing elements belong to the slot's last chunk
    if (threadIdx.x == 0 && (full4 << 2) < d.numel && i0 + LARS_CHUNK4 > full4 && i0 <= full4) {
      for (int e = full4 << 2; e < d.numel; ++e) {
        const float wv = w[d.offset + e];
        const float gv = grad1(g, d.offset + e) * grad_scale;
        sw += wv * wv;
        sg += gv * gv;
      }
    }
    lars_block_sum(sw, sg, red);
    if (threadIdx.x == 0) {
      partials[2 * b] = sw;
      partials[2 * b + 1] = sg;
    }
  }
}

// The slot's partial sums are re-added by every workgroup of the slot (fixed order: thread t takes
// partials t, t + 256, ..., then lars_block_sum) instead of by a finalize kernel between the two
// passes: at most a few hundred L2-resident floats per workgroup, against a third dependent launch
// (~6 us) in front of every update -- three of them in a deferred-tail step.
template <typename G>
__global__ __launch_bounds__(256) void lars_update_kernel(float* __restrict__ w, float* __restrict__ m,
                                                          const G* __restrict__ g, bf16_t* __restrict__ wb,
                                                          const LarsSlot* __restrict__ table, int first_slot,
                                                          int nslots, const float* __restrict__ partials,
                                                          float* __restrict__ trust_out,
                                                          const float* __restrict__ lr_ptr, float mu, float wd,
                                                          float grad_scale, float eta, float eps,
                                                          const int* __restrict__ skip) {
  __shared__ float red[8];
  if (skip != nullptr && *skip != 0) return;
  const float lr = *lr_ptr;
  const int64_t b0 = table[first_slot].begin, b1 = table[first_slot + nslots].begin;
  for (int64_t b = b0 + blockIdx.x; b < b1; b += gridDim.x) {
    const int slot = lars_find(table, first_slot, nslots, b);
    const LarsSlot d = table[slot];
    const int c = (int)(b - d.begin);
    float trust = 1.f;
    if (d.adapt) {
      const int nchunk = (int)(table[slot + 1].begin - d.begin);
      float sw = 0.f, sg = 0.f;
      for (int j = threadIdx.x; j < nchunk; j += 256) {
        sw += partials[2 * (d.begin + j)];
        sg += partials[2 * (d.begin + j) + 1];
      }
      lars_block_sum(sw, sg, red);
      if (sw > 0.f && sg > 0.f) {
        const float wn = sqrtf(sw), gn = sqrtf(sg);
        trust = eta * wn / (gn + wd * wn + eps);
      }
    }
    if (c == 0 && threadIdx.x == 0) trust_out[slot] = trust;
    // with trust == 1 bit for bit the update of sgd_momentum_kernel
    const LarsUpd upd{lr, mu, wd, grad_scale, trust};
    auto store = [&](int64_t i, const float4& wv, const float4& mv) {
      reinterpret_cast<float4*>(w)[i] = wv;
      reinterpret_cast<float4*>(m)[i] = mv;
      if (wb) {
        uint2 o;
        o.x = pack2bf(wv.x, wv.y);
        o.y = pack2bf(wv.z, wv.w);
        reinterpret_cast<uint2*>(wb)[i] = o;
      }
    };
    const int64_t base4 = d.offset / 4;
    const int full4 = d.numel >> 2;
    const int i0 = c * LARS_CHUNK4;
    const int i1 = min(i0 + LARS_CHUNK4, full4);
    // two float4 groups in flight per thread, as in sgd_momentum_kernel
    int i = i0 + threadIdx.x;
    for (; i + 256 < i1; i += 512) {
      const int64_t p = base4 + i, q = p + 256;
      float4 w0 = reinterpret_cast<float4*>(w)[p], w1 = reinterpret_cast<float4*>(w)[q];
      float4 m0 = reinterpret_cast<float4*>(m)[p], m1 = reinterpret_cast<float4*>(m)[q];
      const float4 g0 = grad4(g, p), g1 = grad4(g, q);
      upd4(upd, w0, m0, g0);
      upd4(upd, w1, m1, g1);
      store(p, w0, m0);
      store(q, w1, m1);
    }
    if (i < i1) {
      const int64_t p = base4 + i;
      float4 w0 = reinterpret_cast<float4*>(w)[p];
      float4 m0 = reinterpret_cast<float4*>(m)[p];
      const float4 g0 = grad4(g, p);
      upd4(upd, w0, m0, g0);
      store(p, w0, m0);
    }
    if (threadIdx.x == 0 && (full4 << 2) < d.numel && i0 + LARS_CHUNK4 > full4 && i0 <= full4) {
      for (int e = full4 << 2; e < d.numel; ++e) {
        const int64_t p = d.offset + e;
        float wv = w[p], mv = m[p];
        upd(wv, mv, grad1(g, p));
        w[p] = wv;
        m[p] = mv;
        if (wb) wb[p] = f2bf(wv);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Weight EMA (tf.train.ExponentialMovingAverage): ema <- ema - (1 - d) * (ema - w_new), applied to
// the freshly updated fp32 weight while it is still in a register -- one more read-modify-write
// stream in the optimizer's pass instead of a separate pass re-reading the master buffer. The decay
// d is read from device memory like the learning rate, so a captured graph / recorded plan replays
// with the warm-up value the host wrote for that step. These are kernels of their own: the element
// update is the MomentumUpd / LarsUpd of sgd_momentum_kernel / lars_update_kernel, so w, m and wb
// come out bit-identical, but the loads, stores and loops are repeated here. Calling one shared
// body, or shared load / store / range helpers, from thin kernels was tried and changes the machine
// code of the plain kernels (profiles/optimizer_loss_refactor_codegen.txt); with the EMA off a step
// launches exactly the kernels above, with the code they had.
__device__ __forceinline__ void ema1(float& e, float wv, float om) { e -= om * (e - wv); }
__device__ __forceinline__ void ema4(float4& e, const float4& wv, float om) {
  ema1(e.x, wv.x, om); ema1(e.y, wv.y, om); ema1(e.z, wv.z, om); ema1(e.w, wv.w, om);
}

template <typename G>
__global__ __launch_bounds__(256) void sgd_momentum_ema_kernel(float* __restrict__ w, float* __restrict__ m,
                                                               const G* __restrict__ g, bf16_t* __restrict__ wb,
                                                               int64_t n4, const float* __restrict__ lr_ptr, float mu,
                                                               float wd, float grad_scale,
                                                               const int* __restrict__ skip, float* __restrict__ ema,
                                                               const float* __restrict__ decay_ptr) {
  if (skip != nullptr && *skip != 0) return;  // the average is skipped with the update
  const float lr = *lr_ptr;
  const float om = 1.f - *decay_ptr;
  const MomentumUpd upd{lr, mu, wd, grad_scale};
  auto store = [&](int64_t i, const float4& wv, const float4& mv, const float4& ev) {
    reinterpret_cast<float4*>(w)[i] = wv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(ema)[i] = ev;
    if (wb) {
      uint2 o;
      o.x = pack2bf(wv.x, wv.y);
      o.y = pack2bf(wv.z, wv.w);
      reinterpret_cast<uint2*>(wb)[i] = o;
    }
  };
  // two float4 groups in flight per thread (4 streams read, 4 written)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) {
    float4 w0 = reinterpret_cast<float4*>(w)[i], w1 = reinterpret_cast<float4*>(w)[i + stride];
    float4 m0 = reinterpret_cast<float4*>(m)[i], m1 = reinterpret_cast<float4*>(m)[i + stride];
    float4 e0 = reinterpret_cast<float4*>(ema)[i], e1 = reinterpret_cast<float4*>(ema)[i + stride];
    const float4 g0 = grad4(g, i), g1 = grad4(g, i + stride);
    upd4(upd, w0, m0, g0);
    upd4(upd, w1, m1, g1);
    ema4(e0, w0, om);
    ema4(e1, w1, om);
    store(i, w0, m0, e0);
    store(i + stride, w1, m1, e1);
  }
  if (i < n4) {
    float4 w0 = reinterpret_cast<float4*>(w)[i];
    float4 m0 = reinterpret_cast<float4*>(m)[i];
    float4 e0 = reinterpret_cast<float4*>(ema)[i];
    const float4 g0 = grad4(g, i);
    upd4(upd, w0, m0, g0);
    ema4(e0, w0, om);
    store(i, w0, m0, e0);
  }
}

// lars_update_kernel + the EMA of the updated slots (ema: the base of a flat buffer in w's layout)
template <typename G>
__global__ __launch_bounds__(256) void lars_update_ema_kernel(float* __restrict__ w, float* __restrict__ m,
                                                              const G* __restrict__ g, bf16_t* __restrict__ wb,
                                                              const LarsSlot* __restrict__ table, int first_slot,
                                                              int nslots, const float* __restrict__ partials,
                                                              float* __restrict__ trust_out,
                                                              const float* __restrict__ lr_ptr, float mu, float wd,
                                                              float grad_scale, float eta, float eps,
                                                              const int* __restrict__ skip, float* __restrict__ ema,
                                                              const float* __restrict__ decay_ptr) {
  __shared__ float red[8];
  if (skip != nullptr && *skip != 0) return;
  const float lr = *lr_ptr;
  const float om = 1.f - *decay_ptr;
  const int64_t b0 = table[first_slot].begin, b1 = table[first_slot + nslots].begin;
  for (int64_t b = b0 + blockIdx.x; b < b1; b += gridDim.x) {
    const int slot = lars_find(table, first_slot, nslots, b);
    const LarsSlot d = table[slot];
    const int c = (int)(b - d.begin);
    float trust = 1.f;
    if (d.adapt) {
      const int nchunk = (int)(table[slot + 1].begin - d.begin);
      float sw = 0.f, sg = 0.f;
      for (int j = threadIdx.x; j < nchunk; j += 256) {
        sw += partials[2 * (d.begin + j)];
        sg += partials[2 * (d.begin + j) + 1];
      }
      lars_block_sum(sw, sg, red);
      if (sw > 0.f && sg > 0.f) {
        const float wn = sqrtf(sw), gn = sqrtf(sg);
        trust = eta * wn / (gn + wd * wn + eps);
      }
    }
    if (c == 0 && threadIdx.x == 0) trust_out[slot] = trust;
    const LarsUpd upd{lr, mu, wd, grad_scale, trust};
    auto store = [&](int64_t i, const float4& wv, const float4& mv, const float4& ev) {
      reinterpret_cast<float4*>(w)[i] = wv;
      reinterpret_cast<float4*>(m)[i] = mv;
      reinterpret_cast<float4*>(ema)[i] = ev;
      if (wb) {
        uint2 o;
        o.x = pack2bf(wv.x, wv.y);
        o.y = pack2bf(wv.z, wv.w);
        reinterpret_cast<uint2*>(wb)[i] = o;
      }
    };
    const int64_t base4 = d.offset / 4;
    const int full4 = d.numel >> 2;
    const int i0 = c * LARS_CHUNK4;
    const int i1 = min(i0 + LARS_CHUNK4, full4);
    int i = i0 + threadIdx.x;
    for (; i + 256 < i1; i += 512) {
      const int64_t p = base4 + i, q = p + 256;
      float4 w0 = reinterpret_cast<float4*>(w)[p], w1 = reinterpret_cast<float4*>(w)[q];
      float4 m0 = reinterpret_cast<float4*>(m)[p], m1 = reinterpret_cast<float4*>(m)[q];
      float4 e0 = reinterpret_cast<float4*>(ema)[p], e1 = reinterpret_cast<float4*>(ema)[q];
      const float4 g0 = grad4(g, p), g1 = grad4(g, q);
      upd4(upd, w0, m0, g0);
      upd4(upd, w1, m1, g1);
      ema4(e0, w0, om);
      ema4(e1, w1, om);
      store(p, w0, m0, e0);
      store(q, w1, m1, e1);
    }
    if (i < i1) {
      const int64_t p = base4 + i;
      float4 w0 = reinterpret_cast<float4*>(w)[p];
      float4 m0 = reinterpret_cast<float4*>(m)[p];
      float4 e0 = reinterpret_cast<float4*>(ema)[p];
      const float4 g0 = grad4(g, p);
      upd4(upd, w0, m0, g0);
      ema4(e0, w0, om);
      store(p, w0, m0, e0);
    }
    if (threadIdx.x == 0 && (full4 << 2) < d.numel && i0 + LARS_CHUNK4 > full4 && i0 <= full4) {
      for (int e = full4 << 2; e < d.numel; ++e) {
        const int64_t p = d.offset + e;
        float wv = w[p], mv = m[p], ev = ema[p];
        upd(wv, mv, grad1(g, p));
        ema1(ev, wv, om);
        w[p] = wv;
        m[p] = mv;
        ema[p] = ev;
        if (wb) wb[p] = f2bf(wv);
      }
    }
  }
}

__global__ __launch_bounds__(256) void cast_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y,
                                                        int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    uint2 o;
    o.x = pack2bf(v.x, v.y);
    o.y = pack2bf(v.z, v.w);
    reinterpret_cast<uint2*>(y)[i] = o;
  }
}

// Data-gradient weights for a batch of convolutions described by a device-resident table (one
// launch for the whole network): Wt[c][u][v][k] = W[k][r0 + dr*u][s0 + ds*v][c], u < Ru, v < Sv.
// Full flip (stride-1 data gradient): Ru=R, r0=R-1, dr=-1. Stride-2 data gradients use one
// sub-kernel per output phase (taps of one parity, dr=-2), so no MFMA work is spent on the
// zeros of a dilated dY.
//
// For one tap the map is a K x C -> C x K matrix transpose, so the kernel is a tiled transpose:
// one workgroup per (descriptor, tap, 64-k tile, 64-c tile); rows of 64 c are read with 16-byte
// coalesced loads into LDS, and rows of 64 k leave with 16-byte coalesced stores. (An
// element-per-thread gather reads each 2-byte element from its own 32-byte sector.) The LDS row
// pitch of 66 elements (33 dwords) spreads the column reads of a wave over distinct banks.
struct TDesc {
  int64_t src, dst;       // element offsets into the flat bf16 weight buffers
  int32_t K, R, S, C;     // source KRSC dims (K, C multiples of 8)
  int32_t Ru, Sv, r0, s0; // destination taps and first source tap
  int32_t dr, ds, tk, tc; // tap steps; 64-wide tile counts along K and C
  int64_t begin;          // prefix sum of tile counts (Ru*Sv*tk*tc per descriptor)
};

constexpr int TF_T = 64, TF_PITCH = 66;

__global__ __launch_bounds__(256) void weight_tflip_kernel(const bf16_t* __restrict__ w, bf16_t* __restrict__ wt,
                                                           const TDesc* __restrict__ table, int ntab) {
  __shared__ bf16_t tile[TF_T * TF_PITCH];
  // descriptor owning this tile (uniform scalar binary search)
  const int64_t b = blockIdx.x;
  int lo = 0, hi = ntab - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].begin <= b) lo = mid; else hi = mid - 1;
  }
  const TDesc d = table[lo];
  int t = (int)(b - d.begin);
  const int taps = d.Ru * d.Sv;
  const int uv = t % taps; t /= taps;
  const int kt = t % d.tk, ct = t / d.tk;
  const int u = uv / d.Sv, v = uv - u * d.Sv;
  const int rs = d.r0 + d.dr * u, ss = d.s0 + d.ds * v;
  const int k0 = kt * TF_T, c0 = ct * TF_T;
  const int tid = threadIdx.x, ch = tid & 7, row = tid >> 3;  // 8 chunks of 8 elements x 32 rows
  const int64_t kstride = (int64_t)d.R * d.S * d.C;
  const bf16_t* src = w + d.src + ((int64_t)rs * d.S + ss) * d.C;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = k0 + row + h * 32, c = c0 + ch * 8;
    uint4 val = make_uint4(0, 0, 0, 0);
    if (k < d.K && c < d.C) val = *reinterpret_cast<const uint4*>(src + k * kstride + c);
    uint32_t* l = reinterpret_cast<uint32_t*>(tile + (row + h * 32) * TF_PITCH + ch * 8);
    l[0] = val.x; l[1] = val.y; l[2] = val.z; l[3] = val.w;
  }
  __syncthreads();
  bf16_t* dst = wt + d.dst + (int64_t)uv * d.K;
  const int64_t cstride = (int64_t)taps * d.K;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int cl = row + h * 32, c = c0 + cl, k = k0 + ch * 8;
    if (c < d.C && k < d.K) {
      uint32_t o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t lo16 = tile[(ch * 8 + 2 * j) * TF_PITCH + cl];
        const uint32_t hi16 = tile[(ch * 8 + 2 * j + 1) * TF_PITCH + cl];
        o[j] = lo16 | (hi16 << 16);
      }
      *reinterpret_cast<uint4*>(dst + c * cstride + k) = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
}

__global__ void fill_f32_kernel(float* __restrict__ x, int64_t n, float v) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] = v;
}

static inline int grid_for(int64_t n) {
  int64_t b = (n + 255) / 256;
  return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
}

}  // namespace drn

// f(gradient pointer typed by g_bf16): bf16 (the all-reduced bf16 wire buffer), else fp32
template <typename F>
static void with_grad_type(const void* g, int g_bf16, F&& f) {
  if (g_bf16) f((const bf16_t*)g); else f((const float*)g);
}
template <typename P>
using grad_t = std::remove_const_t<std::remove_pointer_t<P>>;

// ema == nullptr: the plain kernel
static int sgd_momentum(float* w, float* m, const void* g, int g_bf16, void* w_bf16, int64_t n, const float* lr_ptr,
                        float momentum, float wd, float grad_scale, const int* skip, float* ema,
                        const float* decay_ptr, hipStream_t s) {
  if (n % 4) return (int)hipErrorInvalidValue;
  const dim3 grid(drn::grid_for(n / 4)), block(256);
  with_grad_type(g, g_bf16, [&](auto gp) {
    using G = grad_t<decltype(gp)>;
    if (ema)
      drn::launch(drn::sgd_momentum_ema_kernel<G>, grid, block, 0, s, w, m, gp, (bf16_t*)w_bf16, n / 4, lr_ptr,
                  momentum, wd, grad_scale, skip, ema, decay_ptr);
    else
      drn::launch(drn::sgd_momentum_kernel<G>, grid, block, 0, s, w, m, gp, (bf16_t*)w_bf16, n / 4, lr_ptr, momentum,
                  wd, grad_scale, skip);
  });
  return (int)hipGetLastError();
}

// the norms pass, then the update pass; ema == nullptr: the plain update kernel
static int lars_momentum(float* w, float* m, const void* g, int g_bf16, void* w_bf16, const void* table,
                         int first_slot, int nslots, float* partials, float* trust, const float* lr_ptr,
                         float momentum, float wd, float grad_scale, float eta, float eps, const int* skip,
                         float* ema, const float* decay_ptr, hipStream_t s) {
  if (first_slot < 0 || nslots < 1) return (int)hipErrorInvalidValue;
  const drn::LarsSlot* t = (const drn::LarsSlot*)table;
  const dim3 grid(drn::LARS_GRID), block(256);
  with_grad_type(g, g_bf16, [&](auto gp) {
    using G = grad_t<decltype(gp)>;
    drn::launch(drn::lars_norms_kernel<G>, grid, block, 0, s, (const float*)w, gp, t, first_slot, nslots, partials,
                grad_scale, skip);
    if (ema)
      drn::launch(drn::lars_update_ema_kernel<G>, grid, block, 0, s, w, m, gp, (bf16_t*)w_bf16, t, first_slot, nslots,
                  (const float*)partials, trust, lr_ptr, momentum, wd, grad_scale, eta, eps, skip, ema, decay_ptr);
    else
      drn::launch(drn::lars_update_kernel<G>, grid, block, 0, s, w, m, gp, (bf16_t*)w_bf16, t, first_slot, nslots,
                  (const float*)partials, trust, lr_ptr, momentum, wd, grad_scale, eta, eps, skip);
  });
  return (int)hipGetLastError();
}

// skip (nullable device int): when *skip != 0 at run time the launch changes nothing;
// g_bf16: the gradient is bf16 (the all-reduced bf16 wire buffer), else fp32
DRN_API int drn_sgd_momentum(float* w, float* m, const void* g, int g_bf16, void* w_bf16, int64_t n,
                             const float* lr_ptr, float momentum, float wd, float grad_scale, const int* skip,
                             hipStream_t s) {
  return sgd_momentum(w, m, g, g_bf16, w_bf16, n, lr_ptr, momentum, wd, grad_scale, skip, nullptr, nullptr, s);
}

// LARS + momentum over table slots [first_slot, first_slot + nslots) of the flat buffers (w, m, g,
// w_bf16 are the buffers' bases: the table holds absolute element offsets). table: LarsSlot entries
// with one closing entry (its begin = total chunks); partials: 2 floats per chunk of the whole
// table; trust: one float per slot. skip as in drn_sgd_momentum (trust is left alone too).
DRN_API int drn_lars_momentum(float* w, float* m, const void* g, int g_bf16, void* w_bf16, const void* table,
                              int first_slot, int nslots, float* partials, float* trust, const float* lr_ptr,
                              float momentum, float wd, float grad_scale, float eta, float eps, const int* skip,
                              hipStream_t s) {
  return lars_momentum(w, m, g, g_bf16, w_bf16, table, first_slot, nslots, partials, trust, lr_ptr, momentum, wd,
                       grad_scale, eta, eps, skip, nullptr, nullptr, s);
}

// drn_sgd_momentum + the weight EMA in the same launch: ema (n floats, 16-byte aligned like w) <-
// ema - (1 - *decay_ptr) * (ema - w_new); decay_ptr is a device float. Untouched when *skip != 0.
DRN_API int drn_sgd_momentum_ema(float* w, float* m, const void* g, int g_bf16, void* w_bf16, int64_t n,
                                 const float* lr_ptr, float momentum, float wd, float grad_scale, const int* skip,
                                 float* ema, const float* decay_ptr, hipStream_t s) {
  if (ema == nullptr || decay_ptr == nullptr) return (int)hipErrorInvalidValue;
  return sgd_momentum(w, m, g, g_bf16, w_bf16, n, lr_ptr, momentum, wd, grad_scale, skip, ema, decay_ptr, s);
}

// drn_lars_momentum + the weight EMA in its update pass (the norms pass is the same kernel): ema is
// the base of a flat buffer in w's layout, decay_ptr a device float, as in drn_sgd_momentum_ema.
DRN_API int drn_lars_momentum_ema(float* w, float* m, const void* g, int g_bf16, void* w_bf16, const void* table,
                                  int first_slot, int nslots, float* partials, float* trust, const float* lr_ptr,
                                  float momentum, float wd, float grad_scale, float eta, float eps, const int* skip,
                                  float* ema, const float* decay_ptr, hipStream_t s) {
  if (ema == nullptr || decay_ptr == nullptr) return (int)hipErrorInvalidValue;
  return lars_momentum(w, m, g, g_bf16, w_bf16, table, first_slot, nslots, partials, trust, lr_ptr, momentum, wd,
                       grad_scale, eta, eps, skip, ema, decay_ptr, s);
}

DRN_API int drn_lars_slot_size() { return (int)sizeof(drn::LarsSlot); }
DRN_API int drn_lars_chunk() { return drn::LARS_CHUNK4 * 4; }

DRN_API int drn_cast_bf16(const float* x, void* y, int64_t n, hipStream_t s) {
  if (n % 4) return (int)hipErrorInvalidValue;
  drn::launch(drn::cast_bf16_kernel, dim3(drn::grid_for(n / 4)), dim3(256), 0, s, x, (bf16_t*)y, n / 4);
  return (int)hipGetLastError();
}

// total = number of tiles (last begin + its count); every descriptor has K % 8 == C % 8 == 0.
DRN_API int drn_weight_tflip(const void* w, void* wt, const void* table, int ntab, int64_t total, hipStream_t s) {
  if (ntab < 1 || total < 1 || total > 0x7fffffff) return (int)hipErrorInvalidValue;
  drn::launch(drn::weight_tflip_kernel, dim3((unsigned)total), dim3(256), 0, s, (const bf16_t*)w,
                     (bf16_t*)wt, (const drn::TDesc*)table, ntab);
  return (int)hipGetLastError();
}

DRN_API int drn_fill_f32(float* x, int64_t n, float v, hipStream_t s) {
  drn::launch(drn::fill_f32_kernel, dim3(drn::grid_for(n)), dim3(256), 0, s, x, n, v);
  return (int)hipGetLastError();
}

DRN_API int drn_version() { return 1; }
