// adam.hip — fused Adam-family optimizer steps (AdamW, LAMB) over the flat fp32 buffers on gfx950.
//
// Per element, fp32 state (m: the first moment, kept in the momentum buffer; v: the second):
//   g' = gs * g                                   gs = grad_scale, g fp32 or the bf16 wire gradient
//   m <- b1 * m + (1 - b1) * g'                   v <- b2 * v + (1 - b2) * g'^2
//   u  = (m / c1) / (sqrt(v / c2) + eps) + wd * w        c1 = 1 - b1^t, c2 = 1 - b2^t
//   AdamW: w <- w - lr * u                        (decoupled decay, Loshchilov & Hutter 2019)
//   LAMB:  w <- w - lr * trust_l * u              trust_l = ||w_l|| / ||u_l||  (You et al. 2020, the apex
//                                                 FusedLAMB / timm form; 1 if a norm is 0 or the slot
//                                                 does not adapt: BatchNorm gamma / beta, dense bias)
// then w_bf16 = bf16(w) and, in the EMA variants, ema <- ema - (1 - d) * (ema - w), as in sgd.hip.
// lr, (c1, c2) and d are read from device memory: the host writes them before every step, so a captured
// HIP graph / recorded plan replays with the values of its step. A non-zero skip word leaves every
// buffer (w, m, v, w_bf16, ema, trust) as it was.
//
// The element arithmetic is written out operation by operation with contraction off: the plain and
// EMA instantiations, LAMB's two passes and its tail loop all derive bit-identical m, v and u. The
// divisions and the square root are the correctly rounded ones (no v_rcp / v_rsq shortcuts): the pass
// is HBM-bound and has the VALU cycles to spare.
#include "drn_common.h"

DRN_API int drn_lars_slot_size();
DRN_API int drn_lars_chunk();

namespace drn {
namespace {

__device__ __forceinline__ float4 ld4(const float* p, int64_t i) { return reinterpret_cast<const float4*>(p)[i]; }
__device__ __forceinline__ void st4(float* p, int64_t i, const float4& v) { reinterpret_cast<float4*>(p)[i] = v; }
__device__ __forceinline__ float4 grad4(const float* g, int64_t i) { return ld4(g, i); }
__device__ __forceinline__ float4 grad4(const bf16_t* g, int64_t i) {
  const uint2 u = reinterpret_cast<const uint2*>(g)[i];
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}
__device__ __forceinline__ float grad1(const float* g, int64_t i) { return g[i]; }
__device__ __forceinline__ float grad1(const bf16_t* g, int64_t i) { return bf2f(g[i]); }
__device__ __forceinline__ void st4bf(bf16_t* wb, int64_t i, const float4& wv) {
  uint2 o;
  o.x = pack2bf(wv.x, wv.y);
  o.y = pack2bf(wv.z, wv.w);
  reinterpret_cast<uint2*>(wb)[i] = o;
}

struct AdamUpd {
  float b1, omb1, b2, omb2, c1, c2, eps, wd, grad_scale;
  __device__ AdamUpd(float b1_, float b2_, const float* __restrict__ bc, float eps_, float wd_, float gs)
      : b1(b1_), omb1(1.f - b1_), b2(b2_), omb2(1.f - b2_), c1(bc[0]), c2(bc[1]), eps(eps_), wd(wd_),
        grad_scale(gs) {}
  __device__ __forceinline__ void moments(float& mv, float& vv, float gv) const {
#pragma clang fp contract(off)
    const float gg = gv * grad_scale;
    mv = __builtin_fmaf(b1, mv, omb1 * gg);
    vv = __builtin_fmaf(b2, vv, omb2 * (gg * gg));
  }
  // the update direction u from the NEW moments and the old weight
  __device__ __forceinline__ float dir(float wv, float mv, float vv) const {
#pragma clang fp contract(off)
    const float r = (mv / c1) / (sqrtf(vv / c2) + eps);
    return __builtin_fmaf(wd, wv, r);
  }
  // lrt = lr * trust
  __device__ __forceinline__ void apply(float& wv, float u, float lrt) const {
#pragma clang fp contract(off)
    const float step = lrt * u;
    wv = wv - step;
  }
  __device__ __forceinline__ void moments4(float4& m, float4& v, const float4& g) const {
    moments(m.x, v.x, g.x); moments(m.y, v.y, g.y); moments(m.z, v.z, g.z); moments(m.w, v.w, g.w);
  }
  __device__ __forceinline__ float4 dir4(const float4& w, const float4& m, const float4& v) const {
    return make_float4(dir(w.x, m.x, v.x), dir(w.y, m.y, v.y), dir(w.z, m.z, v.z), dir(w.w, m.w, v.w));
  }
  __device__ __forceinline__ void apply4(float4& w, const float4& u, float lrt) const {
    apply(w.x, u.x, lrt); apply(w.y, u.y, lrt); apply(w.z, u.z, lrt); apply(w.w, u.w, lrt);
  }
};

__device__ __forceinline__ void ema1(float& e, float wv, float om) {
#pragma clang fp contract(off)
  const float d = om * (e - wv);
  e = e - d;
}
__device__ __forceinline__ void ema4(float4& e, const float4& wv, float om) {
  ema1(e.x, wv.x, om); ema1(e.y, wv.y, om); ema1(e.z, wv.z, om); ema1(e.w, wv.w, om);
}

// ---------------------------------------------------------------------------------------------
// AdamW: one launch over a flat range of n4 float4 groups (element-wise, so the sharded optimizer
// runs it on its slice). The capped grid-stride shape of sgd_momentum_kernel: two float4 groups in
// flight per thread (4 streams read and 3 written, + the bf16 copy; 5 / 4 with the EMA).
template <typename G, bool EMA>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                    const G* __restrict__ g, bf16_t* __restrict__ wb, int64_t n4,
                                                    const float* __restrict__ lr_ptr, const float* __restrict__ bc,
                                                    float b1, float b2, float eps, float wd, float grad_scale,
                                                    const int* __restrict__ skip, float* __restrict__ ema,
                                                    const float* __restrict__ decay_ptr) {
  if (skip != nullptr && *skip != 0) return;
  const float lr = *lr_ptr;
  float om = 0.f;
  if constexpr (EMA) om = 1.f - *decay_ptr;
  const AdamUpd upd(b1, b2, bc, eps, wd, grad_scale);
  auto step = [&](float4& wv, float4& mv, float4& vv, const float4& gv, float4& ev) {
    upd.moments4(mv, vv, gv);
    const float4 u = upd.dir4(wv, mv, vv);
    upd.apply4(wv, u, lr);
    if constexpr (EMA) ema4(ev, wv, om);
  };
  auto store = [&](int64_t i, const float4& wv, const float4& mv, const float4& vv, const float4& ev) {
    st4(w, i, wv);
    st4(m, i, mv);
    st4(v, i, vv);
    if constexpr (EMA) st4(ema, i, ev);
    if (wb) st4bf(wb, i, wv);
  };
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (; i + stride < n4; i += 2 * stride) {
    const int64_t j = i + stride;
    float4 w0 = ld4(w, i), w1 = ld4(w, j);
    float4 m0 = ld4(m, i), m1 = ld4(m, j);
    float4 v0 = ld4(v, i), v1 = ld4(v, j);
    float4 e0 = w0, e1 = w1;
    if constexpr (EMA) { e0 = ld4(ema, i); e1 = ld4(ema, j); }
    const float4 g0 = grad4(g, i), g1 = grad4(g, j);
    step(w0, m0, v0, g0, e0);
    step(w1, m1, v1, g1, e1);
    store(i, w0, m0, v0, e0);
    store(j, w1, m1, v1, e1);
  }
  if (i < n4) {
    float4 w0 = ld4(w, i), m0 = ld4(m, i), v0 = ld4(v, i);
    float4 e0 = w0;
    if constexpr (EMA) e0 = ld4(ema, i);
    const float4 g0 = grad4(g, i);
    step(w0, m0, v0, g0, e0);
    store(i, w0, m0, v0, e0);
  }
}

// ---------------------------------------------------------------------------------------------
// LAMB: two launches over the slot table of the LARS kernels (sgd.hip `struct LarsSlot`, one entry
// per variable + a closing entry) and its (slot, 8192-element chunk) work layout, on the slot
// sub-range [first_slot, first_slot + nslots). The struct, the chunk search and the block sum are
// repeated here (the entry points check them against drn_lars_slot_size / drn_lars_chunk).
//   pass 1 (lamb_moments_kernel): m, v <- the new moments; each chunk's sum w^2 and sum u^2 go to the
//     chunk's own workspace cell (partials[2b], partials[2b + 1]);
//   pass 2 (lamb_update_kernel): every workgroup of a slot re-adds the slot's cells in the fixed
//     order of lars_update_kernel, derives the trust ratio (chunk 0 publishes it), recomputes u from
//     the stored m, v and w -- the same operations on the same bits as pass 1 -- and applies it.
// No floating-point atomics: the output bits are a function of the input bits and the launch shape.
struct LambSlot {
  int64_t offset;
  int32_t numel, padded;
  int32_t adapt, pad_;
  int64_t begin;
};

constexpr int LAMB_CHUNK4 = 2048;  // float4 groups per chunk (8192 elements, as LARS_CHUNK4)
constexpr int LAMB_GRID = 2048;

__device__ __forceinline__ int lamb_find(const LambSlot* __restrict__ table, int s0, int n, int64_t b) {
  int lo = s0, hi = s0 + n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].begin <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// sum of (a, b) over the workgroup, identical in every thread (wave64 butterfly, then the four wave
// sums through LDS in wave order; red: 8 floats; safe to call back to back)
__device__ __forceinline__ void lamb_block_sum(float& a, float& b, float* red) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[wave] = a; red[4 + wave] = b; }
  __syncthreads();
  a = ((red[0] + red[1]) + red[2]) + red[3];
  b = ((red[4] + red[5]) + red[6]) + red[7];
}

__device__ __forceinline__ void sq4(float& s, const float4& x) {
  s = __builtin_fmaf(x.x, x.x, s); s = __builtin_fmaf(x.y, x.y, s);
  s = __builtin_fmaf(x.z, x.z, s); s = __builtin_fmaf(x.w, x.w, s);
}

template <typename G>
__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ w, float* __restrict__ m,
                                                           float* __restrict__ v, const G* __restrict__ g,
                                                           const LambSlot* __restrict__ table, int first_slot,
                                                           int nslots, float* __restrict__ partials,
                                                           const float* __restrict__ bc, float b1, float b2,
                                                           float eps, float wd, float grad_scale,
                                                           const int* __restrict__ skip) {
  __shared__ float red[8];
  if (skip != nullptr && *skip != 0) return;  // m and v stay as they are
  const AdamUpd upd(b1, b2, bc, eps, wd, grad_scale);
  const int64_t c0 = table[first_slot].begin, c1 = table[first_slot + nslots].begin;
  for (int64_t b = c0 + blockIdx.x; b < c1; b += gridDim.x) {
    const LambSlot d = table[lamb_find(table, first_slot, nslots, b)];
    const int c = (int)(b - d.begin);
    const int64_t base4 = d.offset / 4;
    const int full4 = d.numel >> 2;  // whole float4 groups; the last numel % 4 elements go one by one
    const int i0 = c * LAMB_CHUNK4;
    const int i1 = min(i0 + LAMB_CHUNK4, full4);
    float sw = 0.f, su = 0.f;
    int i = i0 + threadIdx.x;
    for (; i + 256 < i1; i += 512) {
      const int64_t p = base4 + i, q = p + 256;
      const float4 w0 = ld4(w, p), w1 = ld4(w, q);
      float4 m0 = ld4(m, p), m1 = ld4(m, q);
      float4 v0 = ld4(v, p), v1 = ld4(v, q);
      const float4 g0 = grad4(g, p), g1 = grad4(g, q);
      upd.moments4(m0, v0, g0);
      upd.moments4(m1, v1, g1);
      st4(m, p, m0); st4(v, p, v0);
      st4(m, q, m1); st4(v, q, v1);
      sq4(sw, w0); sq4(su, upd.dir4(w0, m0, v0));
      sq4(sw, w1); sq4(su, upd.dir4(w1, m1, v1));
    }
    if (i < i1) {
      const int64_t p = base4 + i;
      const float4 w0 = ld4(w, p);
      float4 m0 = ld4(m, p), v0 = ld4(v, p);
      const float4 g0 = grad4(g, p);
      upd.moments4(m0, v0, g0);
      st4(m, p, m0); st4(v, p, v0);
      sq4(sw, w0); sq4(su, upd.dir4(w0, m0, v0));
    }
    // the numel % 4 trailing elements belong to the slot's last chunk (which may hold nothing else)
    if (threadIdx.x == 0 && (full4 << 2) < d.numel && i0 + LAMB_CHUNK4 > full4 && i0 <= full4) {
      for (int e = full4 << 2; e < d.numel; ++e) {
        const int64_t p = d.offset + e;
        const float wv = w[p];
        float mv = m[p], vv = v[p];
        upd.moments(mv, vv, grad1(g, p));
        m[p] = mv;
        v[p] = vv;
        const float u = upd.dir(wv, mv, vv);
        sw = __builtin_fmaf(wv, wv, sw);
        su = __builtin_fmaf(u, u, su);
      }
    }
    lamb_block_sum(sw, su, red);
    if (threadIdx.x == 0) {
      partials[2 * b] = sw;
      partials[2 * b + 1] = su;
    }
  }
}

template <bool EMA>
__global__ __launch_bounds__(256) void lamb_update_kernel(float* __restrict__ w, const float* __restrict__ m,
                                                          const float* __restrict__ v, bf16_t* __restrict__ wb,
                                                          const LambSlot* __restrict__ table, int first_slot,
                                                          int nslots, const float* __restrict__ partials,
                                                          float* __restrict__ trust_out,
                                                          const float* __restrict__ lr_ptr,
                                                          const float* __restrict__ bc, float b1, float b2, float eps,
                                                          float wd, const int* __restrict__ skip,
                                                          float* __restrict__ ema,
                                                          const float* __restrict__ decay_ptr) {
  __shared__ float red[8];
  if (skip != nullptr && *skip != 0) return;
  const float lr = *lr_ptr;
  float om = 0.f;
  if constexpr (EMA) om = 1.f - *decay_ptr;
  const AdamUpd upd(b1, b2, bc, eps, wd, 1.f);
  const int64_t c0 = table[first_slot].begin, c1 = table[first_slot + nslots].begin;
  for (int64_t b = c0 + blockIdx.x; b < c1; b += gridDim.x) {
    const int slot = lamb_find(table, first_slot, nslots, b);
    const LambSlot d = table[slot];
    const int c = (int)(b - d.begin);
    float trust = 1.f;
    if (d.adapt) {
      const int nchunk = (int)(table[slot + 1].begin - d.begin);
      float sw = 0.f, su = 0.f;
      for (int j = threadIdx.x; j < nchunk; j += 256) {
        sw += partials[2 * (d.begin + j)];
        su += partials[2 * (d.begin + j) + 1];
      }
      lamb_block_sum(sw, su, red);
      if (sw > 0.f && su > 0.f) trust = sqrtf(sw) / sqrtf(su);
    }
    if (c == 0 && threadIdx.x == 0) trust_out[slot] = trust;
    const float lrt = lr * trust;
    auto step = [&](int64_t p, float4 wv, const float4& mv, const float4& vv, float4 ev) {
      upd.apply4(wv, upd.dir4(wv, mv, vv), lrt);
      st4(w, p, wv);
      if constexpr (EMA) { ema4(ev, wv, om); st4(ema, p, ev); }
      if (wb) st4bf(wb, p, wv);
    };
    const int64_t base4 = d.offset / 4;
    const int full4 = d.numel >> 2;
    const int i0 = c * LAMB_CHUNK4;
    const int i1 = min(i0 + LAMB_CHUNK4, full4);
    int i = i0 + threadIdx.x;
    for (; i + 256 < i1; i += 512) {
      const int64_t p = base4 + i, q = p + 256;
      const float4 w0 = ld4(w, p), w1 = ld4(w, q);
      const float4 m0 = ld4(m, p), m1 = ld4(m, q);
      const float4 v0 = ld4(v, p), v1 = ld4(v, q);
      float4 e0 = w0, e1 = w1;
      if constexpr (EMA) { e0 = ld4(ema, p); e1 = ld4(ema, q); }
      step(p, w0, m0, v0, e0);
      step(q, w1, m1, v1, e1);
    }
    if (i < i1) {
      const int64_t p = base4 + i;
      const float4 w0 = ld4(w, p);
      float4 e0 = w0;
      if constexpr (EMA) e0 = ld4(ema, p);
      step(p, w0, ld4(m, p), ld4(v, p), e0);
    }
    if (threadIdx.x == 0 && (full4 << 2) < d.numel && i0 + LAMB_CHUNK4 > full4 && i0 <= full4) {
      for (int e = full4 << 2; e < d.numel; ++e) {
        const int64_t p = d.offset + e;
        float wv = w[p];
        upd.apply(wv, upd.dir(wv, m[p], v[p]), lrt);
        w[p] = wv;
        if constexpr (EMA) {
          float ev = ema[p];
          ema1(ev, wv, om);
          ema[p] = ev;
        }
        if (wb) wb[p] = f2bf(wv);
      }
    }
  }
}

static inline int adam_grid_for(int64_t n) {
  int64_t b = (n + 255) / 256;
  return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
}

}  // namespace
}  // namespace drn

// ema == nullptr: the plain kernels
static int adamw(float* w, float* m, float* v, const void* g, int g_bf16, void* w_bf16, int64_t n,
                 const float* lr_ptr, const float* bc_ptr, float b1, float b2, float eps, float wd, float grad_scale,
                 const int* skip, float* ema, const float* decay_ptr, hipStream_t s) {
  if (n < 0 || n % 4 || lr_ptr == nullptr || bc_ptr == nullptr) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const dim3 grid(drn::adam_grid_for(n / 4)), block(256);
  auto go = [&](auto gp) {
    using G = std::remove_const_t<std::remove_pointer_t<decltype(gp)>>;
    if (ema)
      drn::launch(drn::adamw_kernel<G, true>, grid, block, 0, s, w, m, v, gp, (bf16_t*)w_bf16, n / 4, lr_ptr, bc_ptr,
                  b1, b2, eps, wd, grad_scale, skip, ema, decay_ptr);
    else
      drn::launch(drn::adamw_kernel<G, false>, grid, block, 0, s, w, m, v, gp, (bf16_t*)w_bf16, n / 4, lr_ptr, bc_ptr,
                  b1, b2, eps, wd, grad_scale, skip, (float*)nullptr, (const float*)nullptr);
  };
  if (g_bf16) go((const bf16_t*)g); else go((const float*)g);
  return (int)hipGetLastError();
}

static int lamb(float* w, float* m, float* v, const void* g, int g_bf16, void* w_bf16, const void* table,
                int first_slot, int nslots, float* partials, float* trust, const float* lr_ptr, const float* bc_ptr,
                float b1, float b2, float eps, float wd, float grad_scale, const int* skip, float* ema,
                const float* decay_ptr, hipStream_t s) {
  if (first_slot < 0 || nslots < 1 || lr_ptr == nullptr || bc_ptr == nullptr || table == nullptr)
    return (int)hipErrorInvalidValue;
  if (drn_lars_slot_size() != (int)sizeof(drn::LambSlot) || drn_lars_chunk() != drn::LAMB_CHUNK4 * 4)
    return (int)hipErrorInvalidValue;
  const drn::LambSlot* t = (const drn::LambSlot*)table;
  const dim3 grid(drn::LAMB_GRID), block(256);
  if (g_bf16)
    drn::launch(drn::lamb_moments_kernel<bf16_t>, grid, block, 0, s, (const float*)w, m, v, (const bf16_t*)g, t,
                first_slot, nslots, partials, bc_ptr, b1, b2, eps, wd, grad_scale, skip);
  else
    drn::launch(drn::lamb_moments_kernel<float>, grid, block, 0, s, (const float*)w, m, v, (const float*)g, t,
                first_slot, nslots, partials, bc_ptr, b1, b2, eps, wd, grad_scale, skip);
  if (ema)
    drn::launch(drn::lamb_update_kernel<true>, grid, block, 0, s, w, (const float*)m, (const float*)v,
                (bf16_t*)w_bf16, t, first_slot, nslots, (const float*)partials, trust, lr_ptr, bc_ptr, b1, b2, eps,
                wd, skip, ema, decay_ptr);
  else
    drn::launch(drn::lamb_update_kernel<false>, grid, block, 0, s, w, (const float*)m, (const float*)v,
                (bf16_t*)w_bf16, t, first_slot, nslots, (const float*)partials, trust, lr_ptr, bc_ptr, b1, b2, eps,
                wd, skip, (float*)nullptr, (const float*)nullptr);
  return (int)hipGetLastError();
}

// AdamW on n elements (n % 4 == 0; all buffers 16-byte aligned, w_bf16 8-byte, nullable). lr_ptr: a
// device float; bc_ptr: two device floats, the bias corrections (c1, c2) of this update. skip
// (nullable device int): when *skip != 0 at run time the launch changes nothing. g_bf16: the gradient
// is bf16, else fp32.
DRN_API int drn_adamw(float* w, float* m, float* v, const void* g, int g_bf16, void* w_bf16, int64_t n,
                      const float* lr_ptr, const float* bc_ptr, float b1, float b2, float eps, float wd,
                      float grad_scale, const int* skip, hipStream_t s) {
  return adamw(w, m, v, g, g_bf16, w_bf16, n, lr_ptr, bc_ptr, b1, b2, eps, wd, grad_scale, skip, nullptr, nullptr, s);
}

// drn_adamw + the weight EMA in the same launch (ema, decay_ptr as in drn_sgd_momentum_ema)
DRN_API int drn_adamw_ema(float* w, float* m, float* v, const void* g, int g_bf16, void* w_bf16, int64_t n,
                          const float* lr_ptr, const float* bc_ptr, float b1, float b2, float eps, float wd,
                          float grad_scale, const int* skip, float* ema, const float* decay_ptr, hipStream_t s) {
  if (ema == nullptr || decay_ptr == nullptr) return (int)hipErrorInvalidValue;
  return adamw(w, m, v, g, g_bf16, w_bf16, n, lr_ptr, bc_ptr, b1, b2, eps, wd, grad_scale, skip, ema, decay_ptr, s);
}

// LAMB over table slots [first_slot, first_slot + nslots) of the flat buffers (w, m, v, g, w_bf16 are
// the buffers' bases). table, partials (2 floats per chunk of the whole table) and trust (one float
// per slot) as in drn_lars_momentum; lr_ptr, bc_ptr and skip as in drn_adamw (trust is left alone
// on a skipped step too).
DRN_API int drn_lamb(float* w, float* m, float* v, const void* g, int g_bf16, void* w_bf16, const void* table,
                     int first_slot, int nslots, float* partials, float* trust, const float* lr_ptr,
                     const float* bc_ptr, float b1, float b2, float eps, float wd, float grad_scale, const int* skip,
                     hipStream_t s) {
  return lamb(w, m, v, g, g_bf16, w_bf16, table, first_slot, nslots, partials, trust, lr_ptr, bc_ptr, b1, b2, eps, wd,
              grad_scale, skip, nullptr, nullptr, s);
}

// drn_lamb + the weight EMA in its update pass (the moments pass is the same kernel)
DRN_API int drn_lamb_ema(float* w, float* m, float* v, const void* g, int g_bf16, void* w_bf16, const void* table,
                         int first_slot, int nslots, float* partials, float* trust, const float* lr_ptr,
                         const float* bc_ptr, float b1, float b2, float eps, float wd, float grad_scale,
                         const int* skip, float* ema, const float* decay_ptr, hipStream_t s) {
  if (ema == nullptr || decay_ptr == nullptr) return (int)hipErrorInvalidValue;
  return lamb(w, m, v, g, g_bf16, w_bf16, table, first_slot, nslots, partials, trust, lr_ptr, bc_ptr, b1, b2, eps, wd,
              grad_scale, skip, ema, decay_ptr, s);
}
