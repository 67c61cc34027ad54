// conv_group.hip -- grouped 3x3 convolution for gfx950 (ResNeXt): forward (+ next-BN statistics),
// data gradient and weight gradient. bf16 NHWC activations, bf16 weights [K][3][3][cg], fp32
// accumulation; C == K, C % 32 == 0, group width cg = C / groups in {4, 8, 16, 32}, stride 1 or 2
// with the project's padding rule (leading pad 1).
//
// These layers are byte-bound (cg = 4 at 56x56: 18 FLOP per activation byte), so the kernels are
// built around the activation traffic, not the MFMA rate; they share nothing with the dense
// implicit-GEMM tiles of conv_fwd.hip / conv_wgrad.hip.
//
// Forward / data gradient (gconv3x3_kernel<MODE, CG32>)
//   * A workgroup (4 waves) owns a 64-channel slab and walks `tpw` spatial tiles of TH x TW output
//     pixels. In a grouped conv the output slab needs exactly the same input slab, so the
//     ((TH-1)s+3) x ((TW-1)s+3) x 64 input halo tile is staged in LDS once (16-byte loads +
//     ds_write_b128, out-of-image positions and the channel tail written as zeros) and all nine
//     taps are served from it: every input byte is read from memory once per tile plus the halo.
//     Tiles span the whole image width up to 32 columns (else ~28-column strips), TH*TW <= 256,
//     input + staged output <= 64 KB of the CU's 160 KB LDS (two or more workgroups per CU):
//       56x56 and 28x28 s1: 6x28, halo factor (8*30)/(6*28) = 1.43 (1.33 without the padding
//       columns);  14x14 and 7x7: the whole image, 1.0 (padding only)
//       stride 2, 56->28: 2x28 outputs from a 5x57 input tile, 285/224 = 1.27
//   * LDS pixel rows are 144 bytes apart (128 bytes of channels + 16 bytes of padding): the 16
//     pixels of a fragment read start 36 dwords apart, so their ds_read_b128 cover the 64 banks
//     once (padding, not an XOR swizzle: the lanes' pixels are not consecutive under stride 2 or
//     across a tile row, and padding keeps every such pattern at most 2-way).
//   * MFMA v_mfma_f32_16x16x32_bf16 with the weights stationary in registers as the A operand:
//     each wave owns 16 output channels. cg <= 16: the 16 channels read one 16-channel input
//     slab, a k-step of 32 is two taps x 16 channels (5 steps, the tenth half zero) and the A
//     fragments are the block-diagonal expansion of the wave's weights (4x / 2x / 1x MFMA work at
//     cg 4 / 8 / 16). cg == 32: a k-step is one tap x 32 channels, 9 steps, nothing wasted. The 5
//     or 9 fragments (20 / 36 VGPRs) are gathered once per workgroup straight from [K][3][3][cg]
//     and reused for all its tiles. B fragments are one ds_read_b128 per lane (16 pixels x 8
//     consecutive channels at one tap); each lane computes its own pixel address, so an M-chunk
//     is any 16 pixels of the tile (row-major over the tile, no width restriction).
//   * Epilogue: bf16 results staged in LDS, stored as 16-byte pieces of whole 128-byte pixel
//     rows; with `stats` the per-channel sum / sum of squares of the STORED (bf16-rounded) values
//     are kept in registers over all tiles of the workgroup and added once, into replica
//     blockIdx.y % rep of the [rep][2][K] accumulator the next BatchNorm consumes. The grid never
//     exceeds 1024 workgroups, so with >= 1024 replicas (the deterministic mode) every slot gets
//     exactly one add.
//   * Data gradient: the same main loop, with the fragments gathered flipped and within-group
//     transposed from the SAME forward weights (no second weight copy to refresh). Stride 2: a
//     tile is TH x TW positions (a, b) of dy; its (TH+1) x (TW+1) dy tile is staged once and the
//     four output parities (2a+ph, 2b+pw) are four small GEMMs over 1 / 2 / 2 / 4 taps (5 k-steps
//     at cg <= 16, 9 at cg == 32: the same fragment budget as the forward pass). No zero-dilated
//     dy, no MFMA on dilation zeros, one launch, and every dx element is written.
//
// Weight gradient (gconv3x3_wgrad_kernel<CG32>)
//   * Per tap D[k16][c16 | c32] += dy^T x over the pixels in steps of 32. Both operands are
//     channel-contiguous in LDS (the x halo tile and the dy tile of the same spatial tile) and
//     read transposed with ds_read_b64_tr_b16; all nine taps accumulate in registers (36 / 72
//     VGPRs per wave). The spatial tiles are split across workgroups; each workgroup writes only
//     the block diagonal of its partials into its own cell of the workspace, and the existing
//     fixed-order drn_splitk_reduce sums the cells into the fp32 gradient [K][3][3][cg]. No
//     floating-point atomics: the bits depend on the inputs and the launch shape only.
//
// One fixed configuration per (cg, stride, pass); nothing here is autotuned.
#include "drn_common.h"
#include "drn_conv.h"
#include <atomic>

// Argument block (ctypes mirror: ops/_lib.py DrnGconvArgs). H x W is the forward conv's input
// (x / dx), P x Q its output (y / dy). The entry points fill the tiling fields.
struct DrnGconvArgs {
  const void* x;    // bf16 [N][H][W][C]   (fwd, wgrad)
  const void* w;    // bf16 [C][3][3][cg]  (fwd, dgrad)
  void* y;          // bf16 [N][P][Q][C]   (fwd: out)
  const void* dy;   // bf16 [N][P][Q][C]   (dgrad, wgrad)
  void* dx;         // bf16 [N][H][W][C]   (dgrad: out)
  float* dw;        // fp32 [C][3][3][cg]  (wgrad: out)
  float* stats;     // optional fp32 [stats_rep][2][C] (+= sum, sum of squares of y)
  float* ws;        // wgrad workspace, >= drn_gconv_wgrad_ws_elems floats
  int64_t ws_elems;
  int32_t N, H, W, P, Q, C, cg, stride, stats_rep;
  // filled by the entry points
  int32_t cg_shift, th, tw, tiles_y, tiles_x, ntiles, tpw;
  int32_t ih, iw, oth, otw;              // LDS input tile / staged output tile (pixels)
  int32_t in_h, in_w, out_h, out_w;      // image the pass reads / writes
  int32_t in_bytes;                      // LDS bytes of the input tile
  DrnFastDiv fd_tw, fd_iw, fd_otw, fd_tx, fd_txy;
};

namespace drn {

constexpr int GC_PITCH = 144;   // LDS bytes per pixel: 64 channels + 16 bytes of padding
constexpr int GC_MAX_WGS = 1024;
constexpr int GC_LDS_MAX = 64 * 1024;

enum { GC_FWD = 0, GC_DGRAD1 = 1, GC_DGRAD2 = 2, GC_WGRAD = 3 };

// Output classes of a pass (the four parities of a stride-2 data gradient, else one), their tap
// counts and their k-steps (two taps per step at cg <= 16, one at cg == 32).
constexpr int gc_ncls(int mode) { return mode == GC_DGRAD2 ? 4 : 1; }
constexpr int gc_taps(int mode, int cls) { return mode == GC_DGRAD2 ? ((cls & 2) ? 2 : 1) * ((cls & 1) ? 2 : 1) : 9; }
constexpr int gc_steps(int mode, bool cg32, int cls) { return cg32 ? gc_taps(mode, cls) : (gc_taps(mode, cls) + 1) / 2; }
constexpr int gc_begin(int mode, bool cg32, int cls) {
  int b = 0;
  for (int i = 0; i < cls; ++i) b += gc_steps(mode, cg32, i);
  return b;
}

// Tap slot j of class cls: (dr, dc) its offset in the LDS tile from the lane's pixel, (r, s) the
// FORWARD weight tap it multiplies; slots past the class's taps are dead (zero weights; they alias
// slot 0 so their LDS read stays inside the tile).
struct GcTap {
  int dr, dc, r, s;
  bool live;
};

template <int MODE>
__device__ __forceinline__ GcTap gc_tap(int cls, int j) {
  GcTap t;
  if constexpr (MODE == GC_DGRAD2) {
    // dx row 2a + ph: ph = 0 sees tap r = 1 at dy row a; ph = 1 sees r = 2 at a and r = 0 at a + 1
    const int ph = cls >> 1, pw = cls & 1;
    const int nc = pw ? 2 : 1;
    t.live = j < (ph ? 2 : 1) * nc;
    const int jj = t.live ? j : 0;
    const int ri = jj / nc, ci = jj - ri * nc;
    t.dr = ph ? ri : 0;
    t.r = ph ? (ri ? 0 : 2) : 1;
    t.dc = pw ? ci : 0;
    t.s = pw ? (ci ? 0 : 2) : 1;
  } else {
    t.live = j < 9;
    const int jj = t.live ? j : 0;
    t.dr = jj / 3;
    t.dc = jj - 3 * t.dr;
    t.r = MODE == GC_DGRAD1 ? 2 - t.dr : t.dr;
    t.s = MODE == GC_DGRAD1 ? 2 - t.dc : t.dc;
  }
  return t;
}

// Stage the 64-channel slab c0 of the th x tw pixel tile at (y0, x0) of image n into LDS
// ([pixel][64 ch], GC_PITCH apart); positions outside the image and channels past C become zeros.
__device__ __forceinline__ void gc_stage(char* lds, const bf16_t* __restrict__ src, int n, int y0, int x0, int th,
                                         int tw, const DrnFastDiv& fd_w, int img_h, int img_w, int C, int c0) {
  const int npc = th * tw * 8;
#pragma unroll 4
  for (int i = threadIdx.x; i < npc; i += 256) {
    const int pix = i >> 3, pc = i & 7;
    const int r = (int)drn_fdiv((uint32_t)pix, fd_w);
    const int c = pix - r * tw;
    const int y = y0 + r, x = x0 + c, ch = c0 + pc * 8;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if ((unsigned)y < (unsigned)img_h && (unsigned)x < (unsigned)img_w && ch < C)
      v = *reinterpret_cast<const uint4*>(src + (((size_t)n * img_h + y) * img_w + x) * C + ch);
    *reinterpret_cast<uint4*>(lds + pix * GC_PITCH + pc * 16) = v;
  }
}

struct GcTile {
  int n, y0, x0;  // image, origin of the tile in the tiled grid
};

__device__ __forceinline__ GcTile gc_tile(const DrnGconvArgs& a, int t) {
  GcTile r;
  r.n = (int)drn_fdiv((uint32_t)t, a.fd_txy);
  const int rem = t - r.n * (a.tiles_y * a.tiles_x);
  const int ty = (int)drn_fdiv((uint32_t)rem, a.fd_tx);
  r.y0 = ty * a.th;
  r.x0 = (rem - ty * a.tiles_x) * a.tw;
  return r;
}

template <int MODE, bool CG32>
__global__ __launch_bounds__(256) void gconv3x3_kernel(DrnGconvArgs a) {
  constexpr int NSTEP = CG32 ? 9 : 5;
  constexpr int NCLS = gc_ncls(MODE);
  constexpr int OM = MODE == GC_DGRAD2 ? 2 : 1;  // output pixels per tiled-grid position
  static_assert(gc_begin(MODE, CG32, NCLS) == NSTEP, "k-steps");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* lin = smem;
  char* lout = smem + a.in_bytes;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const int C = a.C, cgs = a.cg_shift, cgm = a.cg - 1;
  const int c0 = blockIdx.x * 64;
  const int ps = MODE == GC_FWD ? a.stride : 1;   // LDS pixel step per tiled-grid position
  const int po = MODE == GC_DGRAD2 ? 0 : -1;      // tile origin: the leading pad
  const bf16_t* __restrict__ src = reinterpret_cast<const bf16_t*>(MODE == GC_FWD ? a.x : a.dy);
  bf16_t* __restrict__ dst = reinterpret_cast<bf16_t*>(MODE == GC_FWD ? a.y : a.dx);
  const bf16_t* __restrict__ W = reinterpret_cast<const bf16_t*>(a.w);

  // the lane's output channel (A rows) and its 8 input channels inside the slab (k of A and B)
  const int co = c0 + 16 * wave + l16;
  const int cib = CG32 ? (wave >> 1) * 32 + g * 8 : 16 * wave + (g & 1) * 8;

  // stationary weight fragments + the LDS offset of each k-step's tap for this lane
  bf16x8_t wf[NSTEP];
  int toff[NSTEP];
#pragma unroll
  for (int cls = 0; cls < NCLS; ++cls) {
#pragma unroll
    for (int st = 0; st < gc_steps(MODE, CG32, cls); ++st) {
      const int idx = gc_begin(MODE, CG32, cls) + st;
      const GcTap t = gc_tap<MODE>(cls, CG32 ? st : 2 * st + (g >> 1));
      toff[idx] = (t.dr * a.iw + t.dc) * GC_PITCH;
      s16x8_t v;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int ci = c0 + cib + e;
        const bool ok = t.live && co < C && ci < C && (ci >> cgs) == (co >> cgs);
        // forward: W[co][r][s][ci in group]; data gradient: W[ci][r][s][co in group]
        const size_t off = MODE == GC_FWD ? (((size_t)co * 9 + t.r * 3 + t.s) << cgs) + (ci & cgm)
                                          : (((size_t)ci * 9 + t.r * 3 + t.s) << cgs) + (co & cgm);
        v[e] = ok ? (short)W[off] : (short)0;
      }
      wf[idx] = __builtin_bit_cast(bf16x8_t, v);
    }
  }

  const int npix = a.th * a.tw;
  const int nch = (npix + 15) >> 4;
  const bool want_stats = MODE == GC_FWD && a.stats != nullptr;
  float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
  const int t_end = min(a.ntiles, ((int)blockIdx.y + 1) * a.tpw);

  for (int t = blockIdx.y * a.tpw; t < t_end; ++t) {
    const GcTile tl = gc_tile(a, t);
    gc_stage(lin, src, tl.n, tl.y0 * ps + po, tl.x0 * ps + po, a.ih, a.iw, a.fd_iw, a.in_h, a.in_w, C, c0);
    __syncthreads();  // the tile is staged (and every thread is done with the previous tile's stores)
    for (int ch = 0; ch < nch; ++ch) {
      const int p = ch * 16 + l16;
      const bool pv = p < npix;
      const int pp = pv ? p : 0;
      const int ly = (int)drn_fdiv((uint32_t)pp, a.fd_tw);
      const int lx = pp - ly * a.tw;
      const char* base = lin + ((ly * ps) * a.iw + lx * ps) * GC_PITCH + cib * 2;
#pragma unroll
      for (int cls = 0; cls < NCLS; ++cls) {
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < gc_steps(MODE, CG32, cls); ++st) {
          const int idx = gc_begin(MODE, CG32, cls) + st;
          const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(base + toff[idx]);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[idx], b, acc, 0, 0, 0);
        }
        // the lane holds channels 16*wave + 4g .. +3 of pixel p
        const int oly = OM * ly + (cls >> 1), olx = OM * lx + (cls & 1);
        const uint32_t lo = pack2bf(acc[0], acc[1]), hi = pack2bf(acc[2], acc[3]);
        if (pv) *reinterpret_cast<uint2*>(lout + (oly * a.otw + olx) * GC_PITCH + wave * 32 + g * 8) = make_uint2(lo, hi);
        if (want_stats && pv && tl.y0 + oly < a.out_h && tl.x0 + olx < a.out_w) {
          const float f[4] = {bf2f(lo & 0xffffu), bf2f(lo >> 16), bf2f(hi & 0xffffu), bf2f(hi >> 16)};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            ssum[i] += f[i];
            ssq[i] += f[i] * f[i];
          }
        }
      }
    }
    __syncthreads();  // the staged outputs are complete (and every thread is done with the input tile)
    const int nop = a.oth * a.otw * 8;
    for (int i = tid; i < nop; i += 256) {
      const int pix = i >> 3, pc = i & 7;
      const int r = (int)drn_fdiv((uint32_t)pix, a.fd_otw);
      const int c = pix - r * a.otw;
      const int oy = tl.y0 * OM + r, ox = tl.x0 * OM + c, chn = c0 + pc * 8;
      if (oy < a.out_h && ox < a.out_w && chn < C)
        *reinterpret_cast<uint4*>(dst + (((size_t)tl.n * a.out_h + oy) * a.out_w + ox) * C + chn) =
            *reinterpret_cast<const uint4*>(lout + pix * GC_PITCH + pc * 16);
    }
  }

  if (want_stats) {
    // the 16 lanes of a row hold 16 pixels of the same 4 channels
    const int rep = a.stats_rep > 1 ? a.stats_rep : 1;
    float* acc = a.stats + (size_t)(blockIdx.y % rep) * 2 * C;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s = ssum[i], q = ssq[i];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        s += __shfl_xor(s, o, 64);
        q += __shfl_xor(q, o, 64);
      }
      const int chn = c0 + 16 * wave + 4 * g + i;
      if (l16 == 0 && chn < C) {
        atomicAdd(acc + chn, s);
        atomicAdd(acc + C + chn, q);
      }
    }
  }
}

typedef short gc_s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) gc_s16x4 gc_lds_s16x4;

// ds_read_b64_tr_b16: the 16 lanes of a row address 4 LDS rows x 16 columns (lane = 4 * row +
// column / 4) and receive them column-major: lane i gets column i of the 4 rows.
__device__ __forceinline__ bf16x8_t gc_tr_pair(const char* base, int off0, int off1) {
  const gc_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((gc_lds_s16x4*)(base + off0));
  const gc_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((gc_lds_s16x4*)(base + off1));
  return __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <bool CG32>
__global__ __launch_bounds__(256) void gconv3x3_wgrad_kernel(DrnGconvArgs a) {
  constexpr int NB = CG32 ? 2 : 1;  // 16-channel blocks of x per wave (the group's channels)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* lxs = smem;
  char* ldy = smem + a.in_bytes;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
  const int C = a.C, cgs = a.cg_shift, cgm = a.cg - 1;
  const int c0 = blockIdx.x * 64;
  const int st = a.stride;
  const int xcb = CG32 ? (wave >> 1) * 32 : 16 * wave;
  const bf16_t* __restrict__ X = reinterpret_cast<const bf16_t*>(a.x);
  const bf16_t* __restrict__ DY = reinterpret_cast<const bf16_t*>(a.dy);

  const int npix = a.th * a.tw;
  // positions that are no pixel of dy (past the tile or the image) read this zero row for dy AND
  // for x: exact zeros, whatever x holds
  if (tid < GC_PITCH / 16) *reinterpret_cast<uint4*>(ldy + npix * GC_PITCH + tid * 16) = make_uint4(0u, 0u, 0u, 0u);

  const int xzero = a.in_bytes + npix * GC_PITCH + 4 * p4 * 2;  // the zero row, relative to the x tile
  f32x4_t acc[9][NB];
#pragma unroll
  for (int tp = 0; tp < 9; ++tp)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[tp][nb] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nch = (npix + 31) >> 5;
  const int t_end = min(a.ntiles, ((int)blockIdx.y + 1) * a.tpw);
  for (int t = blockIdx.y * a.tpw; t < t_end; ++t) {
    const GcTile tl = gc_tile(a, t);
    gc_stage(lxs, X, tl.n, tl.y0 * st - 1, tl.x0 * st - 1, a.ih, a.iw, a.fd_iw, a.H, a.W, C, c0);
    gc_stage(ldy, DY, tl.n, tl.y0, tl.x0, a.th, a.tw, a.fd_tw, a.P, a.Q, C, c0);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
      // the lane addresses pixel rows 8g + q4 and 8g + 4 + q4 of this 32-pixel step
      int dyo[2], xo[2];
      bool pvs[2];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int p = ch * 32 + 8 * g + 4 * hf + q4;
        const int pp = p < npix ? p : 0;
        const int ly = (int)drn_fdiv((uint32_t)pp, a.fd_tw);
        const int lx = pp - ly * a.tw;
        const bool pv = p < npix && tl.y0 + ly < a.P && tl.x0 + lx < a.Q;  // a pixel of dy
        pvs[hf] = pv;
        dyo[hf] = (pv ? pp : npix) * GC_PITCH + (16 * wave + 4 * p4) * 2;
        xo[hf] = ((ly * st) * a.iw + lx * st) * GC_PITCH + (xcb + 4 * p4) * 2;
      }
      const bf16x8_t fa = gc_tr_pair(ldy, dyo[0], dyo[1]);  // A: 16 dy channels x 32 pixels
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) {
        const int off = ((tp / 3) * a.iw + (tp % 3)) * GC_PITCH;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          const bf16x8_t fb = gc_tr_pair(lxs, pvs[0] ? xo[0] + off + nb * 32 : xzero, pvs[1] ? xo[1] + off + nb * 32 : xzero);
          acc[tp][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[tp][nb], 0, 0, 0);
        }
      }
    }
    __syncthreads();  // every wave is done with the tiles before the next one is staged
  }

  // block diagonal only: lane holds dy channels 4g .. 4g+3 (rows) of x channel l16 (column)
  float* out = gridDim.y > 1 ? a.ws + (size_t)blockIdx.y * ((size_t)C * 9 << cgs) : a.dw;
#pragma unroll
  for (int tp = 0; tp < 9; ++tp)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int c = c0 + xcb + nb * 16 + l16;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = c0 + 16 * wave + 4 * g + i;
        if (k < C && c < C && (k >> cgs) == (c >> cgs)) out[(((size_t)k * 9 + tp) << cgs) + (c & cgm)] = acc[tp][nb][i];
      }
    }
}

static DrnFastDiv gc_fastdiv(int d) {
  DrnFastDiv f;
  f.d = (uint32_t)(d < 1 ? 1 : d);
  f.s = 0;
  while ((1u << f.s) < f.d) ++f.s;
  f.m = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << f.s) - f.d)) / f.d + 1);
  f.pad_ = 0;
  return f;
}

// Validate the geometry and choose the tiling of a pass; returns the dynamic LDS bytes, 0 when
// the geometry is outside the supported domain.
static int gc_plan(DrnGconvArgs* a, int mode) {
  const int cg = a->cg;
  if (a->N < 1 || a->H < 1 || a->W < 1 || a->C < 32 || a->C % 32 != 0) return 0;
  if (cg != 4 && cg != 8 && cg != 16 && cg != 32) return 0;
  if (a->stride != 1 && a->stride != 2) return 0;
  const int s = a->stride;
  if (a->P != (a->H - 1) / s + 1 || a->Q != (a->W - 1) / s + 1) return 0;
  a->cg_shift = cg == 4 ? 2 : cg == 8 ? 3 : cg == 16 ? 4 : 5;
  const bool over_dx = mode == GC_DGRAD1;          // the tiled grid: dx for a stride-1 data gradient,
  const int gy = over_dx ? a->H : a->P;            // else y / dy
  const int gx = over_dx ? a->W : a->Q;
  const int ps = (mode == GC_FWD || mode == GC_WGRAD) ? s : 1;
  const int strips = gx <= 32 ? 1 : (gx + 27) / 28;
  const int tw = (gx + strips - 1) / strips;
  const int maxpix = mode == GC_DGRAD2 ? 64 : 256;
  int th = maxpix / tw < 1 ? 1 : maxpix / tw;
  if (th > gy) th = gy;
  int lds = 0;
  for (;; --th) {
    th = (gy + (gy + th - 1) / th - 1) / ((gy + th - 1) / th);  // even rows per tile
    a->ih = mode == GC_DGRAD2 ? th + 1 : (th - 1) * ps + 3;
    a->iw = mode == GC_DGRAD2 ? tw + 1 : (tw - 1) * ps + 3;
    a->oth = mode == GC_DGRAD2 ? 2 * th : th;
    a->otw = mode == GC_DGRAD2 ? 2 * tw : tw;
    a->in_bytes = a->ih * a->iw * GC_PITCH;
    lds = a->in_bytes + (a->oth * a->otw + 1) * GC_PITCH;  // (+ the weight gradient's zero row)
    if (lds <= GC_LDS_MAX || th == 1) break;
  }
  if (lds > GC_LDS_MAX) return 0;
  a->th = th;
  a->tw = tw;
  a->tiles_y = (gy + th - 1) / th;
  a->tiles_x = strips;
  if ((int64_t)a->N * a->tiles_y * a->tiles_x > (int64_t)1 << 30) return 0;
  a->ntiles = a->N * a->tiles_y * a->tiles_x;
  a->in_h = mode == GC_FWD ? a->H : a->P;
  a->in_w = mode == GC_FWD ? a->W : a->Q;
  a->out_h = mode == GC_FWD ? a->P : a->H;
  a->out_w = mode == GC_FWD ? a->Q : a->W;
  if (mode == GC_DGRAD1) a->in_h = a->H, a->in_w = a->W;
  a->fd_tw = gc_fastdiv(tw);
  a->fd_iw = gc_fastdiv(a->iw);
  a->fd_otw = gc_fastdiv(a->otw);
  a->fd_tx = gc_fastdiv(a->tiles_x);
  a->fd_txy = gc_fastdiv(a->tiles_x * a->tiles_y);
  return lds;
}

// Pixel splits of the weight gradient: enough workgroups to fill the chip, but no more workspace
// traffic (one fp32 gradient cell written and re-read per split) than activation traffic.
static int gc_wgrad_splits(const DrnGconvArgs* a) {
  const int slabs = (a->C + 63) / 64;
  int64_t splits = 512 / slabs < 1 ? 1 : 512 / slabs;
  const int64_t act = ((int64_t)a->N * a->H * a->W + (int64_t)a->N * a->P * a->Q) * a->C * 2;
  const int64_t cell = (int64_t)a->C * 9 * a->cg * 8;
  const int64_t cap = act / cell < 4 ? 4 : act / cell;
  if (splits > cap) splits = cap;
  if (splits > a->ntiles) splits = a->ntiles;
  const int tpw = (int)((a->ntiles + splits - 1) / splits);
  return (a->ntiles + tpw - 1) / tpw;
}

// Allow GC_LDS_MAX bytes of dynamic LDS for `kern` on the current device: once per (kernel,
// device), `done` holding one bit per device ordinal. Setting it twice is harmless, so two threads
// racing on the first launch are too; a device ordinal past 63 has no bit and sets it on every
// launch (a host-side call that enqueues nothing, so captures and plan recordings are unaffected).
// Returns the HIP error.
template <typename K>
static int gc_lds_attr(K kern, std::atomic<uint64_t>* done) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  const uint64_t bit = (uint64_t)1 << (dev & 63);
  if (dev < 64 && (done->load(std::memory_order_acquire) & bit)) return 0;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                          GC_LDS_MAX);
  if (e != hipSuccess) return (int)e;
  done->fetch_or(bit, std::memory_order_release);
  return 0;
}

template <int MODE, bool CG32>
static int gc_launch(DrnGconvArgs* a, int lds, hipStream_t s) {
  static std::atomic<uint64_t> attr{0};
  auto kern = gconv3x3_kernel<MODE, CG32>;
  if (const int rc = gc_lds_attr(kern, &attr)) return rc;
  const int slabs = (a->C + 63) / 64;
  a->tpw = (int)(((int64_t)a->ntiles * slabs + GC_MAX_WGS - 1) / GC_MAX_WGS);
  const int gy = (a->ntiles + a->tpw - 1) / a->tpw;
  drn::launch(kern, dim3(slabs, gy), dim3(256), (size_t)lds, s, *a);
  return (int)hipGetLastError();
}

}  // namespace drn

extern "C" int drn_splitk_reduce(const float* ws, float* out, int64_t n, int splits, float scale, int accumulate,
                                 hipStream_t s);

DRN_API int drn_gconv_args_size() { return (int)sizeof(DrnGconvArgs); }

// y = grouped conv(x, w) (+ statistics of the stored y)
DRN_API int drn_gconv_fwd(DrnGconvArgs* a, hipStream_t s) {
  const int lds = drn::gc_plan(a, drn::GC_FWD);
  if (lds == 0 || a->x == nullptr || a->w == nullptr || a->y == nullptr) return (int)hipErrorInvalidValue;
  if (a->stats != nullptr && a->stats_rep < 1) return (int)hipErrorInvalidValue;
  return a->cg == 32 ? drn::gc_launch<drn::GC_FWD, true>(a, lds, s) : drn::gc_launch<drn::GC_FWD, false>(a, lds, s);
}

// dx = data gradient of the grouped conv (every element of dx is written)
DRN_API int drn_gconv_dgrad(DrnGconvArgs* a, hipStream_t s) {
  const int mode = a->stride == 2 ? drn::GC_DGRAD2 : drn::GC_DGRAD1;
  const int lds = drn::gc_plan(a, mode);
  if (lds == 0 || a->dy == nullptr || a->w == nullptr || a->dx == nullptr) return (int)hipErrorInvalidValue;
  if (mode == drn::GC_DGRAD2)
    return a->cg == 32 ? drn::gc_launch<drn::GC_DGRAD2, true>(a, lds, s)
                       : drn::gc_launch<drn::GC_DGRAD2, false>(a, lds, s);
  return a->cg == 32 ? drn::gc_launch<drn::GC_DGRAD1, true>(a, lds, s)
                     : drn::gc_launch<drn::GC_DGRAD1, false>(a, lds, s);
}

// fp32 workspace elements drn_gconv_wgrad needs for this geometry (0: none; -1: unsupported)
DRN_API int64_t drn_gconv_wgrad_ws_elems(DrnGconvArgs* a) {
  if (drn::gc_plan(a, drn::GC_WGRAD) == 0) return -1;
  const int splits = drn::gc_wgrad_splits(a);
  return splits > 1 ? (int64_t)splits * a->C * 9 * a->cg : 0;
}

// dw[C][3][3][cg] = weight gradient (fp32), bitwise reproducible
DRN_API int drn_gconv_wgrad(DrnGconvArgs* a, hipStream_t s) {
  const int lds = drn::gc_plan(a, drn::GC_WGRAD);
  if (lds == 0 || a->x == nullptr || a->dy == nullptr || a->dw == nullptr) return (int)hipErrorInvalidValue;
  const int splits = drn::gc_wgrad_splits(a);
  const int64_t cell = (int64_t)a->C * 9 * a->cg;
  if (splits > 1 && (a->ws == nullptr || a->ws_elems < splits * cell)) return (int)hipErrorInvalidValue;
  a->tpw = (a->ntiles + splits - 1) / splits;
  static std::atomic<uint64_t> attr32{0}, attr16{0};
  const dim3 grid((a->C + 63) / 64, splits);
  if (a->cg == 32) {
    if (const int e = drn::gc_lds_attr(drn::gconv3x3_wgrad_kernel<true>, &attr32)) return e;
    drn::launch(drn::gconv3x3_wgrad_kernel<true>, grid, dim3(256), (size_t)lds, s, *a);
  } else {
    if (const int e = drn::gc_lds_attr(drn::gconv3x3_wgrad_kernel<false>, &attr16)) return e;
    drn::launch(drn::gconv3x3_wgrad_kernel<false>, grid, dim3(256), (size_t)lds, s, *a);
  }
  int rc = (int)hipGetLastError();
  if (rc == 0 && splits > 1) rc = drn_splitk_reduce(a->ws, a->dw, cell, splits, 1.0f, 0, s);
  return rc;
}
