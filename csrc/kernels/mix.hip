// mix.hip — Mixup / CutMix of a batch with its own reversal, on the NHWC bf16 images with 8 stored
// channels (one 16-byte vector per pixel). The partner of sample n is m = N - 1 - n; one thread
// handles one pixel of one pair: it reads that pixel of both images, then writes both results.
//
// Per sample one 32-byte record (the table is also read by softmax_xent_mix_kernel, head.hip):
//   inside the half-open box [y0, y1) x [x0, x1):  dst[n] = src[m]                     (the same bits)
//   elsewhere:                                      dst[n] = bf16_rne(w * a + (1 - w) * b)   (fp32)
// with a = src[n], b = src[m]; w == 1 / w == 0 give a / b bit for bit. Mixup: w = lam and an empty
// box; CutMix: w = 1 and a box; the identity record is {w 1, lam 1, empty box}. The middle sample
// of an odd batch is its own partner and stays as it is, whatever its record says.
//
// dst == src (in place, the training path) or a dst that does not overlap src (the synthetic
// feeder keeps its pristine batch). In place a pixel that does not change is not stored, so a
// CutMix batch moves only the bytes inside its boxes and an identity table moves none.
#include "drn_common.h"

namespace drn {

struct MixRec {
  float w, lam;
  int32_t y0, x0, y1, x1;
  int32_t label_b, pad_;
};
static_assert(sizeof(MixRec) == 32, "MixRec is 32 bytes (ops/backend.py MIX_REC)");

// dst pixel of a sample with record r at (y, x): own pixel a, partner pixel b
__device__ __forceinline__ uint4 mix_pixel(const MixRec& r, bool inbox, const uint4& a, const uint4& b) {
  if (inbox || r.w == 0.f) return b;
  if (r.w == 1.f) return a;
  float fa[8], fb[8], o[8];
  unpack8(a, fa);
  unpack8(b, fb);
  const float w = r.w, v = 1.f - r.w;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = w * fa[j] + v * fb[j];
  return pack8(o);
}

// (src and dst may be the same buffer: neither is __restrict__)
__global__ __launch_bounds__(256) void mix_pairs_kernel(const uint4* src, uint4* dst,
                                                        const MixRec* __restrict__ table, int N, int HW, int W,
                                                        int inplace) {
  const int n = blockIdx.y, m = N - 1 - n;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const size_t ia = (size_t)n * HW + pix, ib = (size_t)m * HW + pix;
  if (n == m) {  // the middle sample of an odd batch
    if (!inplace) dst[ia] = src[ia];
    return;
  }
  const MixRec ra = table[n], rb = table[m];
  const int y = pix / W, x = pix - y * W;
  const bool ina = y >= ra.y0 && y < ra.y1 && x >= ra.x0 && x < ra.x1;
  const bool inb = y >= rb.y0 && y < rb.y1 && x >= rb.x0 && x < rb.x1;
  const bool wa = !inplace || ina || ra.w != 1.f, wb = !inplace || inb || rb.w != 1.f;
  if (!wa && !wb) return;
  // both pixels are read before either is written (dst may be src)
  const uint4 a = src[ia], b = src[ib];
  const uint4 oa = mix_pixel(ra, ina, a, b), ob = mix_pixel(rb, inb, b, a);
  if (wa) dst[ia] = oa;
  if (wb) dst[ib] = ob;
}

}  // namespace drn

// src, dst: N x HW pixels of 8 bf16 (HW = H * W rows of W pixels), 16-byte aligned; table: N MixRec
// in device memory, read when the kernel runs (a graph or plan replay sees the batch's own table).
DRN_API int drn_mix_pairs(const void* src, void* dst, const void* table, int N, int HW, int W, hipStream_t s) {
  if (src == nullptr || dst == nullptr || table == nullptr || N < 1 || HW <= 0 || W <= 0 || HW % W != 0)
    return (int)hipErrorInvalidValue;
  const int pairs = (N + 1) / 2;
  if (pairs > 65535 || ((uintptr_t)src | (uintptr_t)dst) % 16 != 0) return (int)hipErrorInvalidValue;
  drn::launch(drn::mix_pairs_kernel, dim3((HW + 255) / 256, pairs), dim3(256), 0, s, (const uint4*)src, (uint4*)dst,
              (const drn::MixRec*)table, N, HW, W, src == dst ? 1 : 0);
  return (int)hipGetLastError();
}

DRN_API int drn_mix_rec_size() { return (int)sizeof(drn::MixRec); }
