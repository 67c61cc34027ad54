// randaug.hip — RandAugment (Cubuk et al. 2020) on the Inception-style ImageNet input, on 8-bit levels in
// integer arithmetic: the semantics are data/randaug.py `randaug_np` (numpy int64), and kernel and reference
// agree bit for bit.
//
// The input is the fp32 copy of the resampled (and flipped) crop that box_resample_kernel<true> leaves in
// its scratch buffer (input_box.hip). A pixel is quantised once, q = clamp(floor(255 x + 0.5), 0, 255);
// the image's chain of 1 to 4 operations (struct RaDesc, data/randaug.py RA_DESC: ids and integer
// parameters, all magnitude arithmetic done on the host) maps levels to levels; the result is normalised,
// bf16((float(q) * (1 / 255) - mean[c]) * istd[c]), and stored NHWC with the channels padded 3 -> 8.
//
// One 1024-thread workgroup per image. The working image lives in LDS as three 8-bit planes of O x O
// (a plane is padded to whole dwords), followed by a 3 x 256 dword table (histograms, LUTs) and 16 dword
// cells (sums, minima, maxima): 150,528 + 3,136 bytes at O = 224, so one workgroup per CU. The operation id
// is the same for the whole workgroup: the chain is a scalar branch per operation, with workgroup barriers
// between operations.
//   * Brightness, Color, Posterize, Solarize: in place, one dword (4 pixels) of each plane per lane.
//   * Contrast: per-lane integer sums of gray, added across a wave by shuffles and across waves with one
//     ds_add per wave; then in place. AutoContrast: the same with ds_min / ds_max, then a 256-entry LUT per
//     channel built by 768 threads. Equalize: a ds_add histogram per channel, the LUT (each of 768 threads
//     takes the exclusive prefix sum and the last non-zero level from broadcast LDS reads), then the LUT
//     applied. Integer atomics are exact, so the order in which the waves arrive does not matter.
//   * ShearX/Y, TranslateX/Y, Rotate and Sharpness gather from other pixels and cannot run in place: the
//     workgroup first writes its planes to its own slab of a global buffer ([N][3][plane] uint8, 16-byte
//     stores), synchronises, and gathers from the slab (hot in L2) back into LDS. A chain without such an
//     operation never leaves LDS.
// LDS is read and written as dwords everywhere. Left byte-wise: the gathers' slab reads (the affine source
// of four neighbouring outputs is four unrelated addresses; sharpness reads its 3 x 3 neighbourhood at
// byte offsets -1 / +1 of a row, which no aligned dword covers) and the LUT lookups (one table read per
// level). No floating-point atomics; plain vector stores only. The output bits depend on the input bits and
// the descriptors alone.
//
// The affine map is 16.16 fixed point (data/randaug.py affine_entries): with u = 2x + 1 - O,
// v = 2y + 1 - O the source column is floor((A00 u + A01 v + T0 + O 2^16) / 2^17) in int64, the row
// likewise from the second matrix row; a source outside the image gives 128.
#include <atomic>

#include "drn_common.h"

#pragma clang fp contract(off)

namespace drn {

struct RaOp {
  int32_t id;    // data/randaug.py OPS
  int32_t p;     // blend factor f = round(256 factor) | bits kept | solarize threshold
  int32_t m[6];  // A00, A01, T0, A10, A11, T1
};
struct RaDesc {
  int32_t nops;
  int32_t pad_[3];
  RaOp op[4];
};
static_assert(sizeof(RaDesc) == 144, "RaDesc is 144 bytes (data/randaug.py RA_DESC)");

struct RaNorm {
  float mean[3], istd[3];
};

enum {
  RA_IDENTITY, RA_SHEAR_X, RA_SHEAR_Y, RA_TRANSLATE_X, RA_TRANSLATE_Y, RA_ROTATE, RA_BRIGHTNESS, RA_COLOR,
  RA_CONTRAST, RA_SHARPNESS, RA_POSTERIZE, RA_SOLARIZE, RA_AUTOCONTRAST, RA_EQUALIZE
};

constexpr int RA_T = 1024;
constexpr int RA_MAX_SIDE = 224;
constexpr int RA_TAB = 3 * 256;  // dwords
constexpr int RA_CELLS = 16;     // dwords: [0] gray sum, [1..3] channel minima, [4..6] channel maxima
constexpr int RA_LDS_MAX = 3 * RA_MAX_SIDE * RA_MAX_SIDE + (RA_TAB + RA_CELLS) * 4;

__host__ __device__ inline int ra_plane_bytes(int O) { return ((O * O + 3) >> 2) * 4; }
__host__ __device__ inline int ra_planes_bytes(int O) { return (3 * ra_plane_bytes(O) + 15) & ~15; }

__device__ __forceinline__ int ra_clamp(int v) { return min(max(v, 0), 255); }
// The empty asm keeps the shift and the clamp apart: fused by hipcc into one v_ashr_pk_u8_i32 per two pixels,
// the level next to a saturated one came out wrong on the MI355X.
__device__ __forceinline__ int ra_blend(int a, int b, int f) {
  int v = (f * a + (256 - f) * b + 128) >> 8;
  asm volatile("" : "+v"(v));
  return ra_clamp(v);
}
__device__ __forceinline__ int ra_gray(int r, int g, int b) { return (77 * r + 150 * g + 29 * b + 128) >> 8; }
__device__ __forceinline__ int ra_byte(uint32_t w, int k) { return (int)((w >> (8 * k)) & 255u); }

__device__ __forceinline__ int ra_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int ra_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int ra_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// f(rgb) on every pixel, in place: lane i takes dword i of each plane.
template <typename F>
__device__ __forceinline__ void ra_point(uint32_t* plane, int P4, F f) {
  for (int i = threadIdx.x; i < P4; i += RA_T) {
    const uint32_t r = plane[i], g = plane[P4 + i], b = plane[2 * P4 + i];
    uint32_t o0 = 0, o1 = 0, o2 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int v[3] = {ra_byte(r, k), ra_byte(g, k), ra_byte(b, k)};
      f(v);
      o0 |= (uint32_t)v[0] << (8 * k);
      o1 |= (uint32_t)v[1] << (8 * k);
      o2 |= (uint32_t)v[2] << (8 * k);
    }
    plane[i] = o0;
    plane[P4 + i] = o1;
    plane[2 * P4 + i] = o2;
  }
}

// plane c through tab[c][.]
__device__ __forceinline__ void ra_apply_lut(uint32_t* plane, int P4, const uint32_t* tab) {
  for (int c = 0; c < 3; ++c) {
    const uint32_t* lut = tab + c * 256;
    for (int i = threadIdx.x; i < P4; i += RA_T) {
      const uint32_t w = plane[c * P4 + i];
      plane[c * P4 + i] = lut[w & 255u] | lut[(w >> 8) & 255u] << 8 | lut[(w >> 16) & 255u] << 16 | lut[w >> 24] << 24;
    }
  }
}

// the planes -> this image's slab; the barrier makes them visible to the workgroup's gathers
__device__ __forceinline__ void ra_spill(const uint8_t* lds, uint8_t* slab, int bytes16) {
  const uint4* s = reinterpret_cast<const uint4*>(lds);
  uint4* d = reinterpret_cast<uint4*>(slab);
  for (int i = threadIdx.x; i < (bytes16 >> 4); i += RA_T) d[i] = s[i];
  __threadfence_block();
  __syncthreads();
}

__device__ __forceinline__ void ra_affine(uint32_t* plane, const uint8_t* slab, int O, int P, int P4, const RaOp& op) {
  const int PS = P4 * 4;
  const int64_t a00 = op.m[0], a01 = op.m[1], t0 = op.m[2], a10 = op.m[3], a11 = op.m[4], t1 = op.m[5];
  const int64_t half = (int64_t)O << 16;
  for (int i = threadIdx.x; i < P4; i += RA_T) {
    uint32_t o0 = 0, o1 = 0, o2 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int pix = 4 * i + k;
      if (pix < P) {
        const int y = pix / O, x = pix - y * O;
        const int64_t u = 2 * x + 1 - O, v = 2 * y + 1 - O;
        const int64_t sx = (a00 * u + a01 * v + t0 + half) >> 17, sy = (a10 * u + a11 * v + t1 + half) >> 17;
        uint32_t r = 128, g = 128, b = 128;
        if (sx >= 0 && sx < O && sy >= 0 && sy < O) {
          const int sp = (int)sy * O + (int)sx;
          r = slab[sp];
          g = slab[PS + sp];
          b = slab[2 * PS + sp];
        }
        o0 |= r << (8 * k);
        o1 |= g << (8 * k);
        o2 |= b << (8 * k);
      }
    }
    plane[i] = o0;
    plane[P4 + i] = o1;
    plane[2 * P4 + i] = o2;
  }
}

__device__ __forceinline__ void ra_sharpness(uint32_t* plane, const uint8_t* slab, int O, int P, int P4, int f) {
  const int PS = P4 * 4;
  for (int i = threadIdx.x; i < P4; i += RA_T) {
    for (int c = 0; c < 3; ++c) {
      const uint8_t* sl = slab + c * PS;
      const uint32_t w = plane[c * P4 + i];
      uint32_t o = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int pix = 4 * i + k, p = ra_byte(w, k);
        int q = p;
        if (pix < P) {
          const int y = pix / O, x = pix - y * O;
          if (x > 0 && y > 0 && x < O - 1 && y < O - 1) {
            const uint8_t *up = sl + pix - O, *dn = sl + pix + O;
            const int s8 = up[-1] + up[0] + up[1] + sl[pix - 1] + sl[pix + 1] + dn[-1] + dn[0] + dn[1];
            q = ra_blend(p, (s8 + 5 * p + 6) / 13, f);
          }
        }
        o |= (uint32_t)q << (8 * k);
      }
      plane[c * P4 + i] = o;
    }
  }
}

__global__ __launch_bounds__(RA_T) void randaug_kernel(const float4* __restrict__ scratch,
                                                       const RaDesc* __restrict__ desc, uint4* __restrict__ out,
                                                       uint8_t* slabs, int O, RaNorm nm) {
  extern __shared__ __align__(16) uint8_t ra_lds[];
  const int n = blockIdx.x, t = threadIdx.x;
  const int P = O * O, P4 = (P + 3) >> 2;
  uint32_t* plane = reinterpret_cast<uint32_t*>(ra_lds);
  uint32_t* tab = reinterpret_cast<uint32_t*>(ra_lds + ra_planes_bytes(O));
  int* cell = reinterpret_cast<int*>(tab + RA_TAB);
  uint8_t* slab = slabs + (size_t)n * ra_planes_bytes(O);

  // quantise the fp32 pixels into the planes (the bytes past the image in a plane's last dword are 0)
  const float4* src = scratch + (size_t)n * P;
  for (int i = t; i < P4; i += RA_T) {
    uint32_t o0 = 0, o1 = 0, o2 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int pix = 4 * i + k;
      if (pix < P) {
        const float4 v = src[pix];
        o0 |= (uint32_t)(int)fminf(fmaxf(floorf(255.f * v.x + 0.5f), 0.f), 255.f) << (8 * k);
        o1 |= (uint32_t)(int)fminf(fmaxf(floorf(255.f * v.y + 0.5f), 0.f), 255.f) << (8 * k);
        o2 |= (uint32_t)(int)fminf(fmaxf(floorf(255.f * v.z + 0.5f), 0.f), 255.f) << (8 * k);
      }
    }
    plane[i] = o0;
    plane[P4 + i] = o1;
    plane[2 * P4 + i] = o2;
  }
  __syncthreads();

  const RaDesc& d = desc[n];
  const int nops = min(max(d.nops, 0), 4);
  for (int e = 0; e < nops; ++e) {
    const RaOp op = d.op[e];
    const int f = op.p;
    switch (op.id) {
      case RA_SHEAR_X:
      case RA_SHEAR_Y:
      case RA_TRANSLATE_X:
      case RA_TRANSLATE_Y:
      case RA_ROTATE:
        ra_spill(ra_lds, slab, ra_planes_bytes(O));
        ra_affine(plane, slab, O, P, P4, op);
        break;
      case RA_SHARPNESS:
        ra_spill(ra_lds, slab, ra_planes_bytes(O));
        ra_sharpness(plane, slab, O, P, P4, f);
        break;
      case RA_BRIGHTNESS:
        ra_point(plane, P4, [f](int* v) {
          for (int c = 0; c < 3; ++c) v[c] = ra_blend(v[c], 0, f);
        });
        break;
      case RA_COLOR:
        ra_point(plane, P4, [f](int* v) {
          const int g = ra_gray(v[0], v[1], v[2]);
          for (int c = 0; c < 3; ++c) v[c] = ra_blend(v[c], g, f);
        });
        break;
      case RA_CONTRAST: {
        if (t == 0) cell[0] = 0;
        __syncthreads();
        int s = 0;
        for (int i = t; i < P4; i += RA_T) {
          const uint32_t r = plane[i], g = plane[P4 + i], b = plane[2 * P4 + i];
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (4 * i + k < P) s += ra_gray(ra_byte(r, k), ra_byte(g, k), ra_byte(b, k));
        }
        s = ra_wave_sum(s);
        if ((t & 63) == 0) atomicAdd(&cell[0], s);
        __syncthreads();
        const int m = (cell[0] + P / 2) / P;
        ra_point(plane, P4, [f, m](int* v) {
          for (int c = 0; c < 3; ++c) v[c] = ra_blend(v[c], m, f);
        });
        break;
      }
      case RA_POSTERIZE: {
        const uint32_t mask = (0xffu << (8 - min(max(f, 0), 8))) & 0xffu;
        const uint32_t m4 = mask * 0x01010101u;
        for (int i = t; i < 3 * P4; i += RA_T) plane[i] &= m4;
        break;
      }
      case RA_SOLARIZE:
        ra_point(plane, P4, [f](int* v) {
          for (int c = 0; c < 3; ++c) v[c] = v[c] >= f ? 255 - v[c] : v[c];
        });
        break;
      case RA_AUTOCONTRAST: {
        if (t < 3) {
          cell[1 + t] = 255;
          cell[4 + t] = 0;
        }
        __syncthreads();
        for (int c = 0; c < 3; ++c) {
          int lo = 255, hi = 0;
          for (int i = t; i < P4; i += RA_T) {
            const uint32_t w = plane[c * P4 + i];
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (4 * i + k < P) {
                lo = min(lo, ra_byte(w, k));
                hi = max(hi, ra_byte(w, k));
              }
          }
          lo = ra_wave_min(lo);
          hi = ra_wave_max(hi);
          if ((t & 63) == 0) {
            atomicMin(&cell[1 + c], lo);
            atomicMax(&cell[4 + c], hi);
          }
        }
        __syncthreads();
        if (t < RA_TAB) {
          const int c = t >> 8, i = t & 255, lo = cell[1 + c], hi = cell[4 + c];
          tab[t] = hi > lo ? (uint32_t)ra_clamp(((i - lo) * 255 + (hi - lo) / 2) / (hi - lo)) : (uint32_t)i;
        }
        __syncthreads();
        ra_apply_lut(plane, P4, tab);
        break;
      }
      case RA_EQUALIZE: {
        if (t < RA_TAB) tab[t] = 0;
        __syncthreads();
        for (int c = 0; c < 3; ++c)
          for (int i = t; i < P4; i += RA_T) {
            const uint32_t w = plane[c * P4 + i];
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (4 * i + k < P) atomicAdd(&tab[c * 256 + ra_byte(w, k)], 1u);
          }
        __syncthreads();
        uint32_t lut = 0;
        if (t < RA_TAB) {
          const int c = t >> 8, i = t & 255;
          int pre = 0, last = 0;  // sum of h[j < i]; h of the last non-zero level
          for (int j = 0; j < 256; ++j) {
            const int h = (int)tab[c * 256 + j];
            if (j < i) pre += h;
            if (h != 0) last = h;
          }
          const int step = (P - last) / 255;
          lut = step == 0 ? (uint32_t)i : (uint32_t)min(255, (step / 2 + pre) / step);
        }
        __syncthreads();
        if (t < RA_TAB) tab[t] = lut;
        __syncthreads();
        ra_apply_lut(plane, P4, tab);
        break;
      }
      default:
        break;
    }
    __syncthreads();
  }

  // normalise and store: 16 bytes per pixel
  uint4* dst = out + (size_t)n * P;
  for (int i = t; i < P4; i += RA_T) {
    const uint32_t r = plane[i], g = plane[P4 + i], b = plane[2 * P4 + i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int pix = 4 * i + k;
      if (pix < P) {
        const float x[3] = {(float)ra_byte(r, k) * (1.f / 255.f), (float)ra_byte(g, k) * (1.f / 255.f),
                            (float)ra_byte(b, k) * (1.f / 255.f)};
        const float o[8] = {(x[0] - nm.mean[0]) * nm.istd[0], (x[1] - nm.mean[1]) * nm.istd[1],
                            (x[2] - nm.mean[2]) * nm.istd[2], 0.f, 0.f, 0.f, 0.f, 0.f};
        dst[pix] = pack8(o);
      }
    }
  }
}

// Allow RA_LDS_MAX bytes of dynamic LDS on the current device, once per device (conv_group.hip gc_lds_attr).
static int ra_lds_attr() {
  static std::atomic<uint64_t> done{0};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  const uint64_t bit = (uint64_t)1 << (dev & 63);
  if (dev < 64 && (done.load(std::memory_order_acquire) & bit)) return 0;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(randaug_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          RA_LDS_MAX);
  if (e != hipSuccess) return (int)e;
  done.fetch_or(bit, std::memory_order_release);
  return 0;
}

}  // namespace drn

// scratch: N x O x O float4 pixels on [0, 1] (box_resample_kernel<true>'s copy); desc: N RaDesc in device
// memory, read when the kernel runs; out: N x O x O pixels of 8 bf16; slab: N * drn_randaug_slab_bytes(O)
// bytes, 16-byte aligned, the gather operations' copy. O > drn_randaug_max_side(): hipErrorInvalidValue.
DRN_API int drn_randaug(const void* scratch, const void* desc, void* out, void* slab, int N, int O, float m0, float m1,
                        float m2, float s0, float s1, float s2, hipStream_t s) {
  if (scratch == nullptr || desc == nullptr || out == nullptr || slab == nullptr || N < 1 || N > 65535 || O < 1 ||
      O > drn::RA_MAX_SIDE || (uintptr_t)scratch % 16 != 0 || (uintptr_t)out % 16 != 0 || (uintptr_t)slab % 16 != 0 ||
      (uintptr_t)desc % 4 != 0)
    return (int)hipErrorInvalidValue;
  const int lds = drn::ra_planes_bytes(O) + (drn::RA_TAB + drn::RA_CELLS) * 4;
  if (lds > drn::RA_LDS_MAX) return (int)hipErrorInvalidValue;
  if (const int rc = drn::ra_lds_attr()) return rc;
  drn::RaNorm nm;
  const float ms[6] = {m0, m1, m2, s0, s1, s2};
  for (int c = 0; c < 3; ++c) {
    nm.mean[c] = ms[c];
    nm.istd[c] = 1.f / ms[3 + c];
  }
  drn::launch(drn::randaug_kernel, dim3(N), dim3(drn::RA_T), (size_t)lds, s, (const float4*)scratch,
              (const drn::RaDesc*)desc, (uint4*)out, (uint8_t*)slab, O, nm);
  return (int)hipGetLastError();
}

DRN_API int drn_randaug_slab_bytes(int O) { return O >= 1 && O <= drn::RA_MAX_SIDE ? drn::ra_planes_bytes(O) : 0; }
DRN_API int drn_randaug_max_side() { return drn::RA_MAX_SIDE; }
DRN_API int drn_randaug_desc_size() { return (int)sizeof(drn::RaDesc); }
