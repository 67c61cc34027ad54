// stem_deep.hip -- the ResNet-C deep stem for gfx950 (--deep_stem): three 3x3 convolutions at
// 112 x 112 in place of the 7x7 / 2 stem,
//   conv3x3/2 3(8) -> 32   BN ReLU   conv3x3/1 32 -> 32   BN ReLU   conv3x3/1 32 -> 64   max-pool 3x3/2
// bf16 NHWC activations, bf16 weights [K][3][3][C], fp32 accumulation; C in {8, 32}, K in {32, 64},
// stride 1 or 2 with the project's padding rule (leading pad 1), any H, W >= 1.
//
// All three layers are narrow in channels and large in pixels (conv 32 -> 32: 18 kFLOP per pixel on
// 128 compulsory bytes), so they are byte-bound and built like conv_group.hip, around the
// activation traffic, not like the dense implicit-GEMM tiles of conv_fwd.hip.
//
// One kernel family, stem_deep_kernel<CIN, KOUT, POOL>:
//   * A workgroup (4 waves) walks `tpw` spatial tiles of one image over ALL output channels. The
//     input halo tile ((th-1)s+3) x ((tw-1)s+3) x CIN is staged in LDS once per tile with 16-byte
//     loads and serves all nine taps. LDS pixels are 80 bytes apart at 32 channels (64 bytes of
//     channels + 16 of padding: the 16 pixels of a fragment read start 20 dwords apart, so their
//     ds_read_b128 spread over the banks as GC_PITCH's do), 16 bytes at 8 channels.
//   * BN + ReLU prologue, fused into the staging: with scale / shift given, every IN-IMAGE piece
//     becomes relu(scale * x + shift), one fma, rounded to bf16 once (bn_relu_piece's arithmetic),
//     so the layer reads its producer's RAW output and no bn_apply pass exists. Positions outside
//     the image are written as zeros and never pass through the affine map: the conv pads the
//     ACTIVATED tensor, and relu(shift) is not zero.
//   * v_mfma_f32_16x16x32_bf16, weights stationary in registers as the A operand. Every wave owns
//     32 output channels (two 16-channel A blocks, 72 VGPRs at C = 32): all of them at K = 32, where
//     the four waves split the tile's 16-pixel chunks four ways; one half at K = 64, where wave pairs
//     split the chunks. Each B fragment (one ds_read_b128 per lane: 16 pixels x 8 channels at one
//     tap) therefore feeds two MFMAs, which keeps the loop off the LDS read port.
//     C = 32: a k-step is one tap x 32 channels, 9 steps.
//     C = 8 (the first conv, stride 2): a k-step is FOUR taps x 8 channels, 3 steps with the last
//     three-quarters zero; lane group g reads tap 4 * step + g. Chosen over stem.hip's 4-channel
//     tap-pair layout (2 steps): the images are stored with 8 channels, so the 16-byte piece of a
//     pixel is the fragment as it stands and no repacking pass (a read and a write of every image)
//     runs in front of a kernel whose MFMA work is a few percent of its time either way.
//   * Epilogue, plain (conv2d, conv2d_1): bf16 results staged in LDS and stored as 16-byte pieces
//     of whole pixel rows; with `stats` the per-channel sum / sum of squares of the STORED values
//     are kept in registers over the workgroup's tiles, reduced through LDS and added once per
//     workgroup into replica blockIdx.x % rep of the [rep][2][K] accumulator. The grid never
//     exceeds 1024 workgroups, so with >= 1024 replicas (the deterministic mode) every slot gets
//     exactly one add.
//   * Epilogue, pooled (conv2d_2): a tile is th x tw POOLED pixels; its (2th+1) x (2tw+1) conv
//     tile is rounded to bf16 into LDS (the shared row / column is recomputed by the neighbour) and
//     the 3x3 / 2 'SAME' max-pool runs there: first maximum under a strict '>', taps outside the
//     conv image -inf, tap byte r * 3 + s -- stem_pool.hip's contract, the layout maxpool_bwd reads.
//     Only the pooled tensor, its argmax bytes and the pooled statistics reach memory.
//   * Tiles: up to 32 columns wide (16 pooled), at most 512 conv pixels (64 pooled), input + staged
//     output <= 80 KB, so two workgroups share a CU's 160 KB of LDS and one stages while the other
//     multiplies. 112 x 112: 16 x 28 (halo 1.21) for conv2d / conv2d_1; 4 x 14 pooled for conv2d_2
//     (9 x 29 conv pixels, 1.17x the MFMA work, an 11 x 31 input tile).
//
// One fixed configuration per variant; nothing here is autotuned.
#include "drn_common.h"
#include "drn_conv.h"
#include <atomic>

// Argument block (ctypes mirror: ops/_lib.py DrnStemDeepArgs). The entry points fill every field
// after stats_rep.
struct DrnStemDeepArgs {
  const void* x;       // bf16 [N][H][W][C]
  const void* w;       // bf16 [K][3][3][C]
  void* y;             // bf16 [N][P][Q][K], pooled: [N][PP][QP][K]
  uint8_t* arg;        // pooled: first-max tap [N][PP][QP][K]
  const float* scale;  // optional prologue relu(scale * x + shift), fp32 [C] (both or neither)
  const float* shift;
  float* stats;        // optional fp32 [stats_rep][2][K] (+= sum, sum of squares of y)
  int32_t N, H, W, C, K, stride, stats_rep;
  // filled by the entry points
  int32_t P, Q, PP, QP, ppad_h, ppad_w;       // conv output; pooled output and its leading pad
  int32_t th, tw, tiles_y, tiles_x, ntiles, tpw;
  int32_t cth, ctw, ih, iw, in_bytes, pad_;   // conv tile, input tile (pixels), LDS bytes of the latter
  DrnFastDiv fd_tw, fd_ctw, fd_iw, fd_tx, fd_txy;
};

namespace drn {

constexpr int SD_MAX_WGS = 1024;
constexpr int SD_LDS_MAX = 80 * 1024;
constexpr int SD_RED_BYTES = 256 * 17 * 4;   // the pooled statistics' reduction scratch

template <int CIN, int KOUT, bool POOL>
__global__ __launch_bounds__(256) void stem_deep_kernel(DrnStemDeepArgs a) {
  constexpr int IPITCH = CIN == 32 ? 80 : 16;   // LDS bytes per input pixel
  constexpr int OPITCH = KOUT * 2 + 16;         // ... per staged output pixel
  constexpr int NSTEP = CIN == 32 ? 9 : 3;
  constexpr int PCS = CIN / 8, OPC = KOUT / 8;  // 16-byte pieces per input / output pixel
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* lin = smem;
  char* lout = smem + a.in_bytes;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const int kh = KOUT == 64 ? (wave & 1) : 0;            // the wave's 32-channel half
  const int ch0 = KOUT == 64 ? (wave >> 1) : wave;       // its first 16-pixel chunk and their step
  constexpr int CHSTEP = KOUT == 64 ? 2 : 4;
  const int st = a.stride;
  const bf16_t* __restrict__ X = reinterpret_cast<const bf16_t*>(a.x);
  const bf16_t* __restrict__ W = reinterpret_cast<const bf16_t*>(a.w);
  bf16_t* __restrict__ Y = reinterpret_cast<bf16_t*>(a.y);

  // stationary weight fragments (A rows: the lane's output channel of each block) + the LDS offset
  // of each k-step's tap and channels for this lane
  bf16x8_t wf[2][NSTEP];
  int toff[NSTEP];
#pragma unroll
  for (int s = 0; s < NSTEP; ++s) {
    const int tap = CIN == 32 ? s : 4 * s + g;
    const bool live = tap < 9;                            // dead taps: zero weights, the read aliases tap 0
    toff[s] = live ? ((tap / 3) * a.iw + tap % 3) * IPITCH + (CIN == 32 ? g * 16 : 0) : 0;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int k = kh * 32 + b * 16 + l16;
      s16x8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (live) v = *reinterpret_cast<const s16x8_t*>(W + ((size_t)k * 9 + tap) * CIN + (CIN == 32 ? g * 8 : 0));
      wf[b][s] = __builtin_bit_cast(bf16x8_t, v);
    }
  }
  // the prologue's scale / shift of this thread's staging piece (its channel group is fixed:
  // 256 is a multiple of PCS)
  const bool pro = a.scale != nullptr;
  const int spc = tid & (PCS - 1);
  float psc[8], psh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    psc[e] = pro ? a.scale[spc * 8 + e] : 1.f;
    psh[e] = pro ? a.shift[spc * 8 + e] : 0.f;
  }

  const int npix = a.cth * a.ctw;
  const int nch = (npix + 15) >> 4;
  const bool want_stats = a.stats != nullptr;
  float ssum[2][4], ssq[2][4];   // plain: the lane's 2 x 4 channels
  float ps[8], pq[8];            // pooled: the thread's 8-channel group tid % OPC
#pragma unroll
  for (int i = 0; i < 8; ++i) ssum[i >> 2][i & 3] = ssq[i >> 2][i & 3] = ps[i] = pq[i] = 0.f;
  const int t_end = min(a.ntiles, ((int)blockIdx.x + 1) * a.tpw);

  for (int t = blockIdx.x * a.tpw; t < t_end; ++t) {
    const int n = (int)drn_fdiv((uint32_t)t, a.fd_txy);
    const int rem = t - n * (a.tiles_y * a.tiles_x);
    const int ty = (int)drn_fdiv((uint32_t)rem, a.fd_tx);
    const int ty0 = ty * a.th, tx0 = (rem - ty * a.tiles_x) * a.tw;   // origin in the tiled grid
    const int cy0 = POOL ? 2 * ty0 - a.ppad_h : ty0;                  // ... of the conv tile
    const int cx0 = POOL ? 2 * tx0 - a.ppad_w : tx0;
    const int iy0 = cy0 * st - 1, ix0 = cx0 * st - 1;                 // ... of the input tile

    // 1. the input halo tile -> LDS: zeros outside the image, else the (activated) input
    const int npc = a.ih * a.iw * PCS;
#pragma unroll 4
    for (int i = tid; i < npc; i += 256) {
      const int pix = i / PCS;
      const int r = (int)drn_fdiv((uint32_t)pix, a.fd_iw);
      const int c = pix - r * a.iw;
      const int y = iy0 + r, x = ix0 + c;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if ((unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W) {
        v = *reinterpret_cast<const uint4*>(X + (((size_t)n * a.H + y) * a.W + x) * CIN + spc * 8);
        if (pro) {
          float f[8];
          unpack8(v, f);
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] = fmaxf(bf2f(f2bf(fmaf(f[e], psc[e], psh[e]))), 0.f);
          v = pack8(f);
        }
      }
      *reinterpret_cast<uint4*>(lin + pix * IPITCH + spc * 16) = v;
    }
    __syncthreads();  // the tile is staged (and every thread is done with the previous tile's output)

    // 2. conv: 16-pixel chunks of the conv tile (row-major), every B fragment against both A blocks
    for (int ch = ch0; ch < nch; ch += CHSTEP) {
      const int p = ch * 16 + l16;
      const bool pv = p < npix;
      const int pp = pv ? p : 0;
      const int ly = (int)drn_fdiv((uint32_t)pp, a.fd_ctw);
      const int lx = pp - ly * a.ctw;
      const char* base = lin + ((ly * st) * a.iw + lx * st) * IPITCH;
      f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < NSTEP; ++s) {
        const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(base + toff[s]);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][s], b, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[1][s], b, acc1, 0, 0, 0);
      }
      // the lane holds channels kh*32 + blk*16 + 4g .. +3 of pixel p
      const uint32_t o[2][2] = {{pack2bf(acc0[0], acc0[1]), pack2bf(acc0[2], acc0[3])},
                                {pack2bf(acc1[0], acc1[1]), pack2bf(acc1[2], acc1[3])}};
      if (pv) {
        char* dst = lout + pp * OPITCH + (kh * 32 + 4 * g) * 2;
        *reinterpret_cast<uint2*>(dst) = make_uint2(o[0][0], o[0][1]);
        *reinterpret_cast<uint2*>(dst + 32) = make_uint2(o[1][0], o[1][1]);
      }
      if (!POOL && want_stats && pv && cy0 + ly < a.P && cx0 + lx < a.Q) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const float f[4] = {bf2f(o[b][0] & 0xffffu), bf2f(o[b][0] >> 16), bf2f(o[b][1] & 0xffffu),
                              bf2f(o[b][1] >> 16)};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            ssum[b][i] += f[i];
            ssq[b][i] += f[i] * f[i];
          }
        }
      }
    }
    __syncthreads();  // the staged conv tile is complete (and every wave is done with the input tile)

    if constexpr (!POOL) {
      // 3a. whole pixel rows of the tile, 16 bytes at a time
      const int nop = npix * OPC;
      for (int i = tid; i < nop; i += 256) {
        const int pix = i / OPC, pc = i % OPC;
        const int r = (int)drn_fdiv((uint32_t)pix, a.fd_ctw);
        const int c = pix - r * a.ctw;
        const int oy = cy0 + r, ox = cx0 + c;
        if (oy < a.P && ox < a.Q)
          *reinterpret_cast<uint4*>(Y + (((size_t)n * a.P + oy) * a.Q + ox) * KOUT + pc * 8) =
              *reinterpret_cast<const uint4*>(lout + pix * OPITCH + pc * 16);
      }
    } else {
      // 3b. max-pool 3x3 / 2 from the staged tile: item = (pooled pixel, 8-channel group); the 9 taps
      // are read unconditionally (always inside the tile) and masked to -inf outside the conv image
      const int nit = a.th * a.tw * OPC;
      const int pc = tid % OPC;
      for (int i = tid; i < nit; i += 256) {
        const int pix = i / OPC;
        const int pr = (int)drn_fdiv((uint32_t)pix, a.fd_tw);
        const int pcol = pix - pr * a.tw;
        const int py = ty0 + pr, px = tx0 + pcol;
        if (py >= a.PP || px >= a.QP) continue;
        float best[8];
        int bi[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          best[q] = -INFINITY;
          bi[q] = 0;
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int r = 2 * pr + tap / 3, c = 2 * pcol + tap % 3;
          const bool ok = (unsigned)(cy0 + r) < (unsigned)a.P && (unsigned)(cx0 + c) < (unsigned)a.Q;
          const uint4 tv = *reinterpret_cast<const uint4*>(lout + (r * a.ctw + c) * OPITCH + pc * 16);
          float f[8];
          unpack8(tv, f);
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const bool gt = ok && f[q] > best[q];
            best[q] = gt ? f[q] : best[q];
            bi[q] = gt ? tap : bi[q];
          }
        }
        const size_t o = (((size_t)n * a.PP + py) * a.QP + px) * KOUT + pc * 8;
        *reinterpret_cast<uint4*>(Y + o) = pack8(best);   // (exact: maxima of bf16 values)
        uint2 av;
        av.x = (uint32_t)bi[0] | ((uint32_t)bi[1] << 8) | ((uint32_t)bi[2] << 16) | ((uint32_t)bi[3] << 24);
        av.y = (uint32_t)bi[4] | ((uint32_t)bi[5] << 8) | ((uint32_t)bi[6] << 16) | ((uint32_t)bi[7] << 24);
        *reinterpret_cast<uint2*>(a.arg + o) = av;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          ps[q] += best[q];
          pq[q] += best[q] * best[q];
        }
      }
    }
  }

  if (!want_stats) return;   // (uniform)
  // statistics: one add per workgroup and channel, the partial sums reduced through LDS in a fixed order
  __syncthreads();           // every thread is done with the last tile's LDS
  float* red = reinterpret_cast<float*>(smem);
  float* accum = a.stats + (size_t)(blockIdx.x % (a.stats_rep > 1 ? a.stats_rep : 1)) * 2 * KOUT;
  if constexpr (!POOL) {
    // red[wave][sum | sumsq][32 channels of the wave's half]; the 16 lanes of a row hold 16 pixels
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float s = ssum[b][i], q = ssq[b][i];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          s += __shfl_xor(s, o, 64);
          q += __shfl_xor(q, o, 64);
        }
        if (l16 == 0) {
          red[wave * 64 + b * 16 + 4 * g + i] = s;
          red[wave * 64 + 32 + b * 16 + 4 * g + i] = q;
        }
      }
    __syncthreads();
    if (tid < 2 * KOUT) {
      const int which = tid / KOUT, c = tid % KOUT, h = c >> 5, cl = c & 31;
      float acc = 0.f;
      for (int wv = KOUT == 64 ? h : 0; wv < 4; wv += KOUT == 64 ? 2 : 1) acc += red[wv * 64 + which * 32 + cl];
      atomicAdd(accum + which * KOUT + c, acc);
    }
  } else {
    // red[thread][8 sums | 8 sums of squares]; thread u holds channel group u % OPC
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      red[tid * 17 + q] = ps[q];
      red[tid * 17 + 8 + q] = pq[q];
    }
    __syncthreads();
    if (tid < 2 * KOUT) {
      const int which = tid / KOUT, c = tid % KOUT, grp = c >> 3, q = c & 7;
      float acc = 0.f;
      for (int u = grp; u < 256; u += OPC) acc += red[u * 17 + which * 8 + q];
      atomicAdd(accum + which * KOUT + c, acc);
    }
  }
}

static DrnFastDiv sd_fastdiv(int d) {
  DrnFastDiv f;
  f.d = (uint32_t)(d < 1 ? 1 : d);
  f.s = 0;
  while ((1u << f.s) < f.d) ++f.s;
  f.m = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << f.s) - f.d)) / f.d + 1);
  f.pad_ = 0;
  return f;
}

// Leading pad of a 3x3 / 2 'SAME' max-pool over n positions (TF: the smaller half leads).
static int sd_pool_pad(int n) {
  const int total = ((n + 1) / 2 - 1) * 2 + 3 - n;
  return total > 0 ? total / 2 : 0;
}

// Validate the geometry and choose the tiling; returns the dynamic LDS bytes, 0 outside the domain.
static int sd_plan(DrnStemDeepArgs* a, bool pool) {
  if (a->N < 1 || a->H < 1 || a->W < 1 || (a->C != 8 && a->C != 32) || (a->K != 32 && a->K != 64)) return 0;
  if (a->stride != 1 && a->stride != 2) return 0;
  if (a->x == nullptr || a->w == nullptr || a->y == nullptr || (pool && a->arg == nullptr)) return 0;
  if ((a->scale == nullptr) != (a->shift == nullptr)) return 0;
  // the kernels move 16-byte pieces of x / w / y, 8-byte groups of argmax bytes and fp32 scalars
  const uintptr_t p16 = (uintptr_t)a->x | (uintptr_t)a->w | (uintptr_t)a->y;
  const uintptr_t p4 = (uintptr_t)a->scale | (uintptr_t)a->shift | (uintptr_t)a->stats;
  if ((p16 & 15) || (pool && ((uintptr_t)a->arg & 7)) || (p4 & 3)) return 0;
  if (a->stats != nullptr && a->stats_rep < 1) return 0;
  const int s = a->stride;
  a->P = (a->H - 1) / s + 1;
  a->Q = (a->W - 1) / s + 1;
  a->PP = (a->P + 1) / 2;
  a->QP = (a->Q + 1) / 2;
  a->ppad_h = sd_pool_pad(a->P);
  a->ppad_w = sd_pool_pad(a->Q);
  const int gy = pool ? a->PP : a->P, gx = pool ? a->QP : a->Q;
  const int ipitch = a->C == 32 ? 80 : 16, opitch = a->K * 2 + 16;
  const int twmax = pool ? 16 : 32;
  const int strips = (gx + twmax - 1) / twmax;
  const int tw = (gx + strips - 1) / strips;
  const int maxpix = pool ? 64 : 512;
  // the tallest tile of at most maxpix positions that fits the LDS budget: try a height, spread the
  // rows evenly over the tiles that height needs, and go one row lower while it does not fit
  int th = maxpix / tw < 1 ? 1 : maxpix / tw;
  if (th > gy) th = gy;
  int lds = 0;
  for (;;) {
    const int rows = (gy + th - 1) / th;   // tiles per column at this height
    th = (gy + rows - 1) / rows;
    a->cth = pool ? 2 * th + 1 : th;
    a->ctw = pool ? 2 * tw + 1 : tw;
    a->ih = (a->cth - 1) * s + 3;
    a->iw = (a->ctw - 1) * s + 3;
    a->in_bytes = a->ih * a->iw * ipitch;
    lds = a->in_bytes + a->cth * a->ctw * opitch;
    if (lds <= SD_LDS_MAX || th == 1) break;
    --th;
  }
  if (lds > SD_LDS_MAX) return 0;
  if (lds < SD_RED_BYTES) lds = SD_RED_BYTES;
  a->th = th;
  a->tw = tw;
  a->tiles_y = (gy + th - 1) / th;
  a->tiles_x = strips;
  if ((int64_t)a->N * a->tiles_y * a->tiles_x > (int64_t)1 << 30) return 0;
  a->ntiles = a->N * a->tiles_y * a->tiles_x;
  a->tpw = (a->ntiles + SD_MAX_WGS - 1) / SD_MAX_WGS;
  a->pad_ = 0;
  a->fd_tw = sd_fastdiv(tw);
  a->fd_ctw = sd_fastdiv(a->ctw);
  a->fd_iw = sd_fastdiv(a->iw);
  a->fd_tx = sd_fastdiv(a->tiles_x);
  a->fd_txy = sd_fastdiv(a->tiles_x * a->tiles_y);
  return lds;
}

// Allow SD_LDS_MAX bytes of dynamic LDS for the kernel on the current device, once per (kernel,
// device) -- conv_group.hip's gc_lds_attr; a host-side call that enqueues nothing.
template <int CIN, int KOUT, bool POOL>
static int sd_launch(DrnStemDeepArgs* a, int lds, hipStream_t s) {
  static std::atomic<uint64_t> done{0};
  auto kern = stem_deep_kernel<CIN, KOUT, POOL>;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  const uint64_t bit = (uint64_t)1 << (dev & 63);
  if (dev >= 64 || !(done.load(std::memory_order_acquire) & bit)) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            SD_LDS_MAX);
    if (e != hipSuccess) return (int)e;
    done.fetch_or(bit, std::memory_order_release);
  }
  const int grid = (a->ntiles + a->tpw - 1) / a->tpw;
  drn::launch(kern, dim3(grid), dim3(256), (size_t)lds, s, *a);
  return (int)hipGetLastError();
}

template <bool POOL>
static int sd_dispatch(DrnStemDeepArgs* a, hipStream_t s) {
  const int lds = sd_plan(a, POOL);
  if (lds == 0) return (int)hipErrorInvalidValue;
  if (a->C == 8) return a->K == 32 ? sd_launch<8, 32, POOL>(a, lds, s) : sd_launch<8, 64, POOL>(a, lds, s);
  return a->K == 32 ? sd_launch<32, 32, POOL>(a, lds, s) : sd_launch<32, 64, POOL>(a, lds, s);
}

}  // namespace drn

DRN_API int drn_stem_deep_args_size() { return (int)sizeof(DrnStemDeepArgs); }

// y = conv3x3(a, w), a = x or relu(scale * x + shift) (+ statistics of the stored y)
DRN_API int drn_stem_deep_conv(DrnStemDeepArgs* a, hipStream_t s) { return drn::sd_dispatch<false>(a, s); }

// y, arg = maxpool3x3/2 'SAME' of bf16(conv3x3(a, w)) (+ statistics of y); the conv output is not stored
DRN_API int drn_stem_deep_conv_pool(DrnStemDeepArgs* a, hipStream_t s) { return drn::sd_dispatch<true>(a, s); }
