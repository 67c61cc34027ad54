// gradguard.hip — global-norm gradient clipping and the non-finite step guard on gfx950.
//
// TF's clip_by_global_norm over the flat gradient buffer the optimizer is about to read, plus a
// guard that turns a step whose gradient holds a NaN / Inf into a no-op, both decided ON THE
// DEVICE so a captured HIP graph / recorded step plan follows each replay's gradients:
//   norm  = sqrt(sum_i (gs * g_i)^2)               gs = the optimizer's grad_scale (1 / world)
//   scale = clip / max(norm, clip)                  (1 when clip == 0 or the norm is not finite)
//   skip  = incoming skip word != 0  ||  (guard && the norm is not finite)
// Two launches: grad_sumsq_kernel leaves one partial sum per workgroup in its own workspace cell;
// grad_guard_apply_kernel re-adds the cells in every workgroup (fixed order, as lars_update_kernel
// re-adds its chunk sums instead of a finalize launch), publishes the record and, only when the
// clip triggers, scales g in place. No floating-point atomics: the result depends on the input
// bits and the launch shape alone, so every data-parallel rank derives the same scale from the
// same reduced gradient. The optimizer kernels (sgd.hip) are untouched: they read record.skip as
// their existing skip word and the already scaled gradient.
#include "drn_common.h"

namespace drn {

// the device record both the optimizer (skip) and the host (grad_guard_stats) read: 8 words
struct GuardRecord {
  float norm, scale;       // this step's global norm and clip factor
  int32_t skip;            // != 0: the optimizer kernels change nothing
  int32_t skipped_total;   // steps skipped for a non-finite norm (an incoming skip word is not counted)
  int32_t clipped_total;   // steps whose gradient was scaled
  int32_t steps_total;     // guarded steps
  int32_t reserved[2];
};

constexpr int GG_GRID = 2048;   // workgroups (8 per CU, as LARS_GRID): 25.6 M elements = 12 / 6 groups per thread
constexpr int GG_BLOCK = 256;

// one 16-byte group of gradients: 4 fp32 or 8 bf16
template <typename G> struct GVec;
template <> struct GVec<float> {
  static constexpr int N = 4;
  typedef float4 raw_t;
  static __device__ __forceinline__ void unpack(const raw_t& r, float* f) { f[0] = r.x; f[1] = r.y; f[2] = r.z; f[3] = r.w; }
  static __device__ __forceinline__ raw_t pack(const float* f) { return make_float4(f[0], f[1], f[2], f[3]); }
  static __device__ __forceinline__ float load1(const float* g, int64_t i) { return g[i]; }
  static __device__ __forceinline__ void store1(float* g, int64_t i, float v) { g[i] = v; }
};
template <> struct GVec<bf16_t> {
  static constexpr int N = 8;
  typedef uint4 raw_t;
  static __device__ __forceinline__ void unpack(const raw_t& r, float* f) { unpack8(r, f); }
  static __device__ __forceinline__ raw_t pack(const float* f) { return pack8(f); }  // round-to-nearest-even
  static __device__ __forceinline__ float load1(const bf16_t* g, int64_t i) { return bf2f(g[i]); }
  static __device__ __forceinline__ void store1(bf16_t* g, int64_t i, float v) { g[i] = f2bf(v); }
};

// sum of v over the workgroup, identical in every thread: wave64 butterfly, then the four wave sums
// through LDS added in wave order (lars_block_sum for one value). Every thread must call it.
__device__ __forceinline__ float gg_block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// partials[blockIdx.x] = this workgroup's share of sum (gs * g)^2. Element j of a group goes to
// accumulator j % 4 (independent chains), the n % N trailing elements to workgroup 0's thread 0.
template <typename G>
__global__ __launch_bounds__(GG_BLOCK) void grad_sumsq_kernel(const G* __restrict__ g, int64_t n, float gs,
                                                              float* __restrict__ partials) {
  typedef GVec<G> V;
  __shared__ float red[4];
  const typename V::raw_t* gv = reinterpret_cast<const typename V::raw_t*>(g);
  const int64_t nv = n / V::N;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  auto acc = [&](const typename V::raw_t& r) {
    float f[V::N];
    V::unpack(r, f);
#pragma unroll
    for (int j = 0; j < V::N; ++j) {
      const float v = gs * f[j];
      s[j & 3] += v * v;
    }
  };
  // two 16-byte groups in flight per thread, as in sgd_momentum_kernel
  const int64_t stride = (int64_t)gridDim.x * GG_BLOCK;
  int64_t i = blockIdx.x * (int64_t)GG_BLOCK + threadIdx.x;
  for (; i + stride < nv; i += 2 * stride) {
    const typename V::raw_t r0 = gv[i], r1 = gv[i + stride];
    acc(r0);
    acc(r1);
  }
  if (i < nv) acc(gv[i]);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int64_t e = nv * V::N; e < n; ++e) {
      const float v = gs * V::load1(g, e);
      s[(int)(e & 3)] += v * v;
    }
  }
  const float t = gg_block_sum((s[0] + s[1]) + (s[2] + s[3]), red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// Every workgroup re-adds the nparts partials (thread t takes t, t + 256, ..., then gg_block_sum)
// and derives norm / scale / skip; workgroup 0 publishes the record. The counters are plain
// read-modify-writes by that one thread (launches on one stream are ordered), so graph and plan
// replays keep counting. An unclipped or skipped step returns here without touching g -- after the
// block sum's barrier, the last one, and on a value uniform over the whole grid.
template <typename G>
__global__ __launch_bounds__(GG_BLOCK) void grad_guard_apply_kernel(G* __restrict__ g, int64_t n,
                                                                    const float* __restrict__ partials, int nparts,
                                                                    float clip, int guard,
                                                                    const int* __restrict__ skip_in,
                                                                    GuardRecord* __restrict__ rec) {
  typedef GVec<G> V;
  __shared__ float red[4];
  float p = 0.f;
  for (int j = threadIdx.x; j < nparts; j += GG_BLOCK) p += partials[j];
  const float norm = sqrtf(gg_block_sum(p, red));
  const bool finite = (__float_as_uint(norm) & 0x7f800000u) != 0x7f800000u;
  const int in = skip_in != nullptr ? *skip_in : 0;
  const bool bad = guard != 0 && !finite;
  const bool skip = in != 0 || bad;
  const float scale = (clip > 0.f && finite) ? clip / fmaxf(norm, clip) : 1.f;
  const bool clipped = !skip && scale != 1.f;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    rec->norm = norm;
    rec->scale = scale;
    rec->skip = skip ? 1 : 0;
    rec->skipped_total += bad ? 1 : 0;
    rec->clipped_total += clipped ? 1 : 0;
    rec->steps_total += 1;
  }
  if (!clipped) return;
  typename V::raw_t* gv = reinterpret_cast<typename V::raw_t*>(g);
  const int64_t nv = n / V::N;
  auto mul = [&](typename V::raw_t& r) {
    float f[V::N];
    V::unpack(r, f);
#pragma unroll
    for (int j = 0; j < V::N; ++j) f[j] *= scale;
    r = V::pack(f);
  };
  const int64_t stride = (int64_t)gridDim.x * GG_BLOCK;
  int64_t i = blockIdx.x * (int64_t)GG_BLOCK + threadIdx.x;
  for (; i + stride < nv; i += 2 * stride) {
    typename V::raw_t r0 = gv[i], r1 = gv[i + stride];
    mul(r0);
    mul(r1);
    gv[i] = r0;
    gv[i + stride] = r1;
  }
  if (i < nv) {
    typename V::raw_t r0 = gv[i];
    mul(r0);
    gv[i] = r0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t e = nv * V::N; e < n; ++e) V::store1(g, e, V::load1(g, e) * scale);
}

}  // namespace drn

// Global-norm clip + non-finite guard of the n gradients g (fp32, or bf16 when g_bf16; 16-byte
// aligned; any n >= 1) that the optimizer will scale by grad_scale. clip > 0: g *= clip / max(norm,
// clip) in place when norm > clip (0: never scaled). guard_nonfinite: record->skip is set when the
// norm is NaN / Inf. skip_in (nullable device int): ORed into record->skip. partials:
// drn_grad_guard_grid() floats of workspace; record: 8 words (drn::GuardRecord) the caller zeroed
// once. Pass &record->skip (word 2) to the optimizer launch that follows.
DRN_API int drn_grad_guard(void* g, int g_bf16, int64_t n, float grad_scale, float clip, int guard_nonfinite,
                           const int* skip_in, float* partials, void* record, hipStream_t s) {
  if (g == nullptr || partials == nullptr || record == nullptr || n < 1) return (int)hipErrorInvalidValue;
  if (!(clip >= 0.f) || !(clip <= 3.4028234663852886e38f) || !(grad_scale == grad_scale))
    return (int)hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(g) & 15) || (reinterpret_cast<uintptr_t>(partials) & 3) ||
      (reinterpret_cast<uintptr_t>(record) & 3) || (reinterpret_cast<uintptr_t>(skip_in) & 3))
    return (int)hipErrorInvalidValue;
  drn::GuardRecord* rec = (drn::GuardRecord*)record;
  // (every workgroup reads *skip_in while workgroup 0 writes the record: they must not overlap)
  if (skip_in != nullptr && (const char*)skip_in >= (const char*)rec && (const char*)skip_in < (const char*)(rec + 1))
    return (int)hipErrorInvalidValue;
  const dim3 grid(drn::GG_GRID), block(drn::GG_BLOCK);
  if (g_bf16) {
    drn::launch(drn::grad_sumsq_kernel<bf16_t>, grid, block, 0, s, (const bf16_t*)g, n, grad_scale, partials);
    drn::launch(drn::grad_guard_apply_kernel<bf16_t>, grid, block, 0, s, (bf16_t*)g, n, (const float*)partials,
                drn::GG_GRID, clip, guard_nonfinite, skip_in, rec);
  } else {
    drn::launch(drn::grad_sumsq_kernel<float>, grid, block, 0, s, (const float*)g, n, grad_scale, partials);
    drn::launch(drn::grad_guard_apply_kernel<float>, grid, block, 0, s, (float*)g, n, (const float*)partials,
                drn::GG_GRID, clip, guard_nonfinite, skip_in, rec);
  }
  return (int)hipGetLastError();
}

DRN_API int drn_grad_guard_grid() { return drn::GG_GRID; }
DRN_API int drn_grad_guard_block() { return drn::GG_BLOCK; }
DRN_API int drn_grad_guard_record_size() { return (int)sizeof(drn::GuardRecord); }
