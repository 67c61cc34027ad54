// input_box.hip — Inception-style ImageNet input: crop-then-resize of one integer box per image with
// the separable anti-aliased triangle filter, optional colour jitter, per-channel mean / std
// normalisation, NHWC bf16 output with the channel dimension zero-padded 3 -> 8. The semantics are
// data/imagenet.py `box_preprocess_np` (fp64); all arithmetic is on [0, 1] pixels.
//
// Per axis (box length L -> output length O, scale = L / O, support = max(scale, 1)) output i takes the
// taps j in [lo, hi) with weight max(0, 1 - |j + 0.5 - scale (i + 0.5)| / support), normalised to sum
// 1 (torch's interpolate(bilinear, align_corners=False, antialias=True) on the crop). lo, hi and the
// weight's numerator t = (2j + 1) O - L (2i + 1) are exact integers: w = 1 - |t| / (2 max(L, O)), so a
// rounding can neither add nor drop a tap and the weights carry two fp32 roundings each.
//
// box_resample_kernel: one 256-thread workgroup per 16 x 16 output tile of one image. The tile's
// source footprint (uint8 rows, read as aligned dwords: image offsets are arbitrary byte offsets) is
// staged in LDS, a horizontal pass leaves footprint-rows x 16 fp32 pixels in an LDS strip and a vertical
// pass produces the outputs: Ty + Tx taps per pixel. A tile whose footprint exceeds the staging
// buffers (SRC_BYTES, FH_MAX rows: boxes shrunk more than ~4.5x per axis) takes the same arithmetic
// with direct global taps. The flip mirrors the output columns. LDS: 24 KiB + 18 KiB per workgroup,
// three workgroups per CU.
//
// Jitter off: that one launch normalises and stores. Jitter on: the launch stores the resampled fp32
// pixels to a scratch copy and one gray partial sum per workgroup in its own cell; box_color_kernel
// re-adds an image's cells in one fixed order (m0, the mean gray), applies the three colour
// operations in the image's order to the fp32 pixels, normalises and stores. No atomics: the output
// bits depend on the input bits and the launch shape alone. Factors (1, 1, 1) give the bits of the
// jitter-off launch (x * 1 and x + 0 * y are exact; contraction is off in this file so both launches
// round the shared arithmetic alike).
//
// A descriptor whose box does not lie inside its image, or whose image does not lie inside the packed
// buffer, reads nothing and yields NaN pixels.
#include "drn_common.h"

#pragma clang fp contract(off)

namespace drn {

struct BoxDesc {
  int64_t offset;          // byte offset of the HWC uint8 image in the packed buffer
  int32_t H, W;            // decoded size
  int32_t by, bx, bh, bw;  // the box, inside the image
  int32_t flip;
  int32_t order;           // colour operations, first to last, 2 bits each: 0 brightness 1 contrast 2 saturation
  float ab, ac, as;        // brightness, contrast, saturation factors
  int32_t pad_[3];
};
static_assert(sizeof(BoxDesc) == 64, "BoxDesc is 64 bytes (data/imagenet.py BOX_DESC)");

struct BoxNorm {
  float mean[3], istd[3];
};

constexpr int TS = 16;            // output tile side
constexpr int SRC_BYTES = 24576;  // staged uint8 footprint
constexpr int FH_MAX = 96;        // rows of the fp32 strip

__device__ __forceinline__ int tap_lo(int L, int O, int i) {
  const int num = (L >= O) ? L * (2 * i - 1) + O : L * (2 * i + 1) - O;
  return num <= 0 ? 0 : num / (2 * O);
}

__device__ __forceinline__ int tap_hi(int L, int O, int i) {
  const int num = (L >= O) ? L * (2 * i + 3) + O : L * (2 * i + 1) + 3 * O;
  return min(num / (2 * O), L);
}

// weight of tap j for output i: t = (2j + 1) O - L (2i + 1), inv = 1 / (2 max(L, O))
__device__ __forceinline__ float tap_w(int t, float inv) { return fmaxf(0.f, 1.f - fabsf((float)t) * inv); }

__device__ __forceinline__ float gray_of(const float* x) { return (0.299f * x[0] + 0.587f * x[1]) + 0.114f * x[2]; }

__device__ __forceinline__ uint4 norm_pack(const float* x, const BoxNorm& nm) {
  float f[8] = {(x[0] - nm.mean[0]) * nm.istd[0], (x[1] - nm.mean[1]) * nm.istd[1], (x[2] - nm.mean[2]) * nm.istd[2],
                0.f, 0.f, 0.f, 0.f, 0.f};
  return pack8(f);
}

__device__ __forceinline__ float block_sum4(float s, float* red) {
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

template <bool JIT>
__global__ __launch_bounds__(256) void box_resample_kernel(const uint8_t* __restrict__ in, int64_t nbytes,
                                                           const BoxDesc* __restrict__ desc, uint4* __restrict__ out,
                                                           float4* __restrict__ scratch, float* __restrict__ partial,
                                                           int OH, int OW, int tiles_x, BoxNorm nm, int force_direct) {
  __shared__ uint32_t src32[SRC_BYTES / 4];
  __shared__ float strip[FH_MAX * TS * 3];
  __shared__ float red[4];
  const int n = blockIdx.y, tile = blockIdx.x;
  const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
  const BoxDesc d = desc[n];
  const int t = threadIdx.x, ly = t >> 4, lx = t & 15;
  const int oy = tyi * TS + ly, ox = txi * TS + lx;  // (resampled coordinates: the flip moves the store)
  const bool live = oy < OH && ox < OW;
  const size_t opix = ((size_t)n * OH + min(oy, OH - 1)) * OW + (d.flip ? OW - 1 - min(ox, OW - 1) : min(ox, OW - 1));
  float x[3];

  const bool ok = d.offset >= 0 && d.H > 0 && d.W > 0 && d.by >= 0 && d.bx >= 0 && d.bh > 0 && d.bw > 0 &&
                  (int64_t)d.by + d.bh <= d.H && (int64_t)d.bx + d.bw <= d.W &&
                  d.offset + (int64_t)d.H * d.W * 3 <= nbytes;
  if (!ok) {
    x[0] = x[1] = x[2] = __int_as_float(0x7fc00000);
  } else {
    const int y_last = min(tyi * TS + TS, OH) - 1, x_last = min(txi * TS + TS, OW) - 1;
    const int fy0 = tap_lo(d.bh, OH, tyi * TS), FH = tap_hi(d.bh, OH, y_last) - fy0;
    const int fx0 = tap_lo(d.bw, OW, txi * TS), FW = tap_hi(d.bw, OW, x_last) - fx0;
    const int64_t W3 = (int64_t)d.W * 3;
    const int64_t g00 = d.offset + ((int64_t)(d.by + fy0) * d.W + d.bx + fx0) * 3;  // the footprint's first byte
    const int rowbytes = FW * 3;
    const int pitch = (rowbytes + 6) & ~3;  // a row starts up to 3 bytes into its first dword
    const bool staged = !force_direct && FH <= FH_MAX && (int64_t)FH * pitch <= SRC_BYTES;
    const float invy = 1.f / (2.f * (float)max(d.bh, OH)), invx = 1.f / (2.f * (float)max(d.bw, OW));
    const int oyc = min(oy, OH - 1), oxc = min(ox, OW - 1);
    const int ylo = tap_lo(d.bh, OH, oyc), yhi = tap_hi(d.bh, OH, oyc);
    float acc[3] = {0.f, 0.f, 0.f}, ws = 0.f;
    if (staged) {
      const int pdw = pitch >> 2;
      for (int idx = t; idx < FH * pdw; idx += 256) {
        const int r = idx / pdw, k = idx - r * pdw;
        const int64_t g = g00 + r * W3;
        const int64_t a = g - (g & 3) + 4 * k;
        if (a < g + rowbytes) {
          uint32_t w;
          if (a + 4 <= nbytes) {
            w = *reinterpret_cast<const uint32_t*>(in + a);
          } else {  // the last dword of the packed buffer's last image
            w = 0;
            for (int b = 0; b < 4; ++b)
              if (a + b < nbytes) w |= (uint32_t)in[a + b] << (8 * b);
          }
          src32[idx] = w;
        }
      }
      __syncthreads();
      const uint8_t* src8 = reinterpret_cast<const uint8_t*>(src32);
      for (int idx = t; idx < FH * TS; idx += 256) {
        const int r = idx >> 4, i = min(txi * TS + (idx & 15), OW - 1);
        const int lo = tap_lo(d.bw, OW, i), hi = tap_hi(d.bw, OW, i);
        int b = r * pitch + (int)((g00 + r * W3) & 3) + (lo - fx0) * 3;
        int tt = (2 * lo + 1) * OW - d.bw * (2 * i + 1);
        float h[3] = {0.f, 0.f, 0.f}, hs = 0.f;
        for (int j = lo; j < hi; ++j, b += 3, tt += 2 * OW) {
          const float w = tap_w(tt, invx);
          h[0] += w * (float)src8[b];
          h[1] += w * (float)src8[b + 1];
          h[2] += w * (float)src8[b + 2];
          hs += w;
        }
        strip[idx * 3 + 0] = h[0] / hs;
        strip[idx * 3 + 1] = h[1] / hs;
        strip[idx * 3 + 2] = h[2] / hs;
      }
      __syncthreads();
      int tt = (2 * ylo + 1) * OH - d.bh * (2 * oyc + 1);
      for (int j = ylo; j < yhi; ++j, tt += 2 * OH) {
        const float w = tap_w(tt, invy);
        const float* h = strip + ((j - fy0) * TS + lx) * 3;
        acc[0] += w * h[0];
        acc[1] += w * h[1];
        acc[2] += w * h[2];
        ws += w;
      }
    } else {
      const int lo = tap_lo(d.bw, OW, oxc), hi = tap_hi(d.bw, OW, oxc);
      int ty = (2 * ylo + 1) * OH - d.bh * (2 * oyc + 1);
      for (int jy = ylo; jy < yhi; ++jy, ty += 2 * OH) {
        const uint8_t* p = in + d.offset + ((int64_t)(d.by + jy) * d.W + d.bx + lo) * 3;
        int tt = (2 * lo + 1) * OW - d.bw * (2 * oxc + 1);
        float h[3] = {0.f, 0.f, 0.f}, hs = 0.f;
        for (int j = lo; j < hi; ++j, p += 3, tt += 2 * OW) {
          const float w = tap_w(tt, invx);
          h[0] += w * (float)p[0];
          h[1] += w * (float)p[1];
          h[2] += w * (float)p[2];
          hs += w;
        }
        const float w = tap_w(ty, invy);
        acc[0] += w * (h[0] / hs);
        acc[1] += w * (h[1] / hs);
        acc[2] += w * (h[2] / hs);
        ws += w;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = (acc[c] / ws) * (1.f / 255.f);
  }
  if (JIT) {
    if (live) scratch[opix] = make_float4(x[0], x[1], x[2], 0.f);
    const float s = block_sum4(live ? gray_of(x) : 0.f, red);
    if (t == 0) partial[(size_t)n * gridDim.x + tile] = s;
  } else {
    if (live) out[opix] = norm_pack(x, nm);
  }
}

__global__ __launch_bounds__(256) void box_color_kernel(const float4* __restrict__ scratch,
                                                        const float* __restrict__ partial,
                                                        const BoxDesc* __restrict__ desc, uint4* __restrict__ out,
                                                        int HW, int tiles, BoxNorm nm) {
  __shared__ float red[4];
  const int n = blockIdx.y, t = threadIdx.x;
  float s = 0.f;
  for (int k = t; k < tiles; k += 256) s += partial[(size_t)n * tiles + k];
  const float m0 = block_sum4(s, red) / (float)HW;
  const int pix = blockIdx.x * 256 + t;
  if (pix >= HW) return;
  const BoxDesc d = desc[n];
  const float4 p = scratch[(size_t)n * HW + pix];
  float x[3] = {p.x, p.y, p.z};
  // brightness scales the mean gray; saturation and contrast keep it
  float m = m0;
  for (int k = 0; k < 3; ++k) {
    const int op = (d.order >> (2 * k)) & 3;
    if (op == 0) m = m0 * d.ab;
    if (op == 1) break;
  }
  for (int k = 0; k < 3; ++k) {
    const int op = (d.order >> (2 * k)) & 3;
    if (op == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = d.ab * x[c];
    } else if (op == 1) {
      const float o = (1.f - d.ac) * m;
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = d.ac * x[c] + o;
    } else {
      const float o = (1.f - d.as) * gray_of(x);
#pragma unroll
      for (int c = 0; c < 3; ++c) x[c] = d.as * x[c] + o;
    }
  }
  out[(size_t)n * HW + pix] = norm_pack(x, nm);
}

static inline BoxNorm box_norm(const float* ms) {
  BoxNorm nm;
  for (int c = 0; c < 3; ++c) {
    nm.mean[c] = ms[c];
    nm.istd[c] = 1.f / ms[3 + c];
  }
  return nm;
}

}  // namespace drn

// in: the packed decoded batch (4-byte aligned, nbytes long); desc: N BoxDesc in device memory, read when
// the kernel runs; out: N x OH x OW pixels of 8 bf16, 16-byte aligned. force_direct != 0: every tile takes
// the direct-tap path (tests).
DRN_API int drn_box_preprocess(const uint8_t* in, int64_t nbytes, const void* desc, void* out, int N, int OH, int OW,
                               float m0, float m1, float m2, float s0, float s1, float s2, int force_direct,
                               hipStream_t s) {
  if (in == nullptr || desc == nullptr || out == nullptr || N < 1 || N > 65535 || OH < 1 || OW < 1 || nbytes < 0 ||
      OH > 16384 || OW > 16384 || (uintptr_t)in % 4 != 0 || (uintptr_t)out % 16 != 0 || (uintptr_t)desc % 8 != 0)
    return (int)hipErrorInvalidValue;
  const float ms[6] = {m0, m1, m2, s0, s1, s2};
  const int tx = (OW + drn::TS - 1) / drn::TS, ty = (OH + drn::TS - 1) / drn::TS;
  drn::launch(drn::box_resample_kernel<false>, dim3(tx * ty, N), dim3(256), 0, s, in, nbytes,
              (const drn::BoxDesc*)desc, (uint4*)out, (float4*)nullptr, (float*)nullptr, OH, OW, tx,
              drn::box_norm(ms), force_direct);
  return (int)hipGetLastError();
}

// The same with colour jitter: scratch holds N x OH x OW float4, partial drn_box_tiles(OH, OW) floats per image.
DRN_API int drn_box_preprocess_jitter(const uint8_t* in, int64_t nbytes, const void* desc, void* out, void* scratch,
                                      void* partial, int N, int OH, int OW, float m0, float m1, float m2, float s0,
                                      float s1, float s2, int force_direct, hipStream_t s) {
  if (in == nullptr || desc == nullptr || out == nullptr || scratch == nullptr || partial == nullptr || N < 1 ||
      N > 65535 || OH < 1 || OW < 1 || OH > 16384 || OW > 16384 || nbytes < 0 || (uintptr_t)in % 4 != 0 ||
      (uintptr_t)out % 16 != 0 || (uintptr_t)scratch % 16 != 0 || (uintptr_t)partial % 4 != 0 ||
      (uintptr_t)desc % 8 != 0)
    return (int)hipErrorInvalidValue;
  const float ms[6] = {m0, m1, m2, s0, s1, s2};
  const drn::BoxNorm nm = drn::box_norm(ms);
  const int tx = (OW + drn::TS - 1) / drn::TS, ty = (OH + drn::TS - 1) / drn::TS;
  drn::launch(drn::box_resample_kernel<true>, dim3(tx * ty, N), dim3(256), 0, s, in, nbytes,
              (const drn::BoxDesc*)desc, (uint4*)out, (float4*)scratch, (float*)partial, OH, OW, tx, nm, force_direct);
  drn::launch(drn::box_color_kernel, dim3((OH * OW + 255) / 256, N), dim3(256), 0, s, (const float4*)scratch,
              (const float*)partial, (const drn::BoxDesc*)desc, (uint4*)out, OH * OW, tx * ty, nm);
  return (int)hipGetLastError();
}

DRN_API int drn_box_tiles(int OH, int OW) {
  return ((OW + drn::TS - 1) / drn::TS) * ((OH + drn::TS - 1) / drn::TS);
}

DRN_API int drn_box_desc_size() { return (int)sizeof(drn::BoxDesc); }
