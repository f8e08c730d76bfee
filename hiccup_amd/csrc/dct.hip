// dct.hip -- 8x8 block DCT-II + quantize (encode) and dequantize + DCT-III (decode)
// for MI355X (gfx950), bit-exact against hiccup's scipy/numpy path.
//
// Reference: transform.dct_channel / inv_dct_channel (transform.py:169-193),
// transform.dct2 / idct2 (transform.py:67-103) -> scipy.fftpack.dct / idct
// (pocketfft, scipy 1.15.3), quantization.jpeg_quantize / invert_jpeg_quantize
// (quantization.py:47-57,80-81).
//
// Design (DESIGN.md "forward kernel"):
//  * one 8x8 block per lane, 64 consecutive raster-order blocks per wave, so each
//    row load (8 B/lane) and each coefficient-row store (16 B/lane) of a wave is
//    one contiguous 512 B / 1 KiB segment of HBM; no LDS, no cross-lane traffic;
//  * float64 throughout, replicating pocketfft's length-8 operation order exactly
//    (built with -ffp-contract=off; the only FMAs are explicit ones whose product
//    is exact, e.g. y*2^-8);
//  * "half-scaled" DCT-II: pocketfft's x2 / x0.5 steps are exact power-of-two
//    scalings, so they are dropped and folded into the quantizer divisor
//    (DESIGN.md derives the bookkeeping: outputs 0 and 4 come out halved);
//  * the integer-exact prefix of each row transform (pixel sums/differences) runs
//    in int32, converting to float64 only where pocketfft first rounds;
//  * quantize = rint(b * (1/D)) with a near-tie guard: when the product lies
//    within 2^-30 of a half-integer (exact .5 ties occur at DC and at (4,4)), the
//    lane recomputes rint(b / D) with the IEEE-correct divide, which is what
//    numpy does.  The guard is > 10^3 x the reciprocal's error bound.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "color_core.h"
#include "dct_core.h"
#include "decode_batch.h"
#include "rle_core.h"

namespace hic {
namespace {

template <int TABLE, int LAYOUT, bool FAST>
__global__ __launch_bounds__(256) void k_dct_quant(const uint8_t *__restrict__ plane, int H, int W,
                                                   int64_t stride, int nbx, int nblk,
                                                   void *__restrict__ out) {
  constexpr SlotOf<LAYOUT> kSlot{};
  const int blk = blockIdx.x * 256 + threadIdx.x;
  if (blk >= nblk) return;
  const int bi = blk / nbx, bj = blk - bi * nbx;
  const int y0 = bi * 8, x0 = bj * 8;

  // ---- row pass (rows of the 8x8 block) ----
  int col0[8];   // y'[r][0], exact integers
  double a[8][8];  // y'[r][1..7]  (a[r][0] unused)
  if (FAST) {
    const uint8_t *p = plane + (int64_t)y0 * stride + x0;
    uint2 w[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) w[r] = *reinterpret_cast<const uint2 *>(p + r * stride);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      int x[8];
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        x[n] = (int)((w[r].x >> (8 * n)) & 0xFFu) - 128;
        x[n + 4] = (int)((w[r].y >> (8 * n)) & 0xFFu) - 128;
      }
      dct8h_int(x, col0[r], a[r]);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      int x[8];
      const int yy = y0 + r;
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const int xx = x0 + n;
        // pad_matrix pads the (pixel - 128) plane with 0 (transform.py:17-30)
        x[n] = (yy < H && xx < W) ? (int)plane[(int64_t)yy * stride + xx] - 128 : 0;
      }
      dct8h_int(x, col0[r], a[r]);
    }
  }

  // ---- column pass + quantize, packed to int16 in the output order ----
  uint32_t pk[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) pk[k] = 0;
  {
    int b0;
    double b[8];
    dct8h_int(col0, b0, b);
    put16(pk, kSlot.s[0], quantize<TABLE>((double)b0, 0));
#pragma unroll
    for (int u = 1; u < 8; ++u) put16(pk, kSlot.s[u * 8], quantize<TABLE>(b[u], u * 8));
  }
#pragma unroll
  for (int v = 1; v < 8; ++v) {
    double xc[8], b[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) xc[r] = a[r][v];
    dct8h(xc, b);
#pragma unroll
    for (int u = 0; u < 8; ++u) put16(pk, kSlot.s[u * 8 + v], quantize<TABLE>(b[u], u * 8 + v));
  }

  // ---- store ----
  if (LAYOUT == HIC_LAYOUT_ZIGZAG_I16) {
    if (!FAST && (y0 + 8 > H || x0 + 8 > W)) {
      // positions cropped by merge_blocks are 0 when jpeg_encode re-pads
#pragma unroll
      for (int z = 0; z < 64; ++z) {
        const int u = ZZ[z] / 8, v = ZZ[z] % 8;
        if (y0 + u >= H || x0 + v >= W) pk[z >> 1] &= (z & 1) ? 0x0000FFFFu : 0xFFFF0000u;
      }
    }
    uint4 *o = reinterpret_cast<uint4 *>(static_cast<int16_t *>(out) + (int64_t)blk * 64);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = make_uint4(pk[4 * k], pk[4 * k + 1], pk[4 * k + 2], pk[4 * k + 3]);
  } else if (LAYOUT == HIC_LAYOUT_RASTER_I16) {
    int16_t *o = static_cast<int16_t *>(out);
    if (FAST) {
#pragma unroll
      for (int u = 0; u < 8; ++u)
        *reinterpret_cast<uint4 *>(o + (int64_t)(y0 + u) * W + x0) =
            make_uint4(pk[4 * u], pk[4 * u + 1], pk[4 * u + 2], pk[4 * u + 3]);
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int v = 0; v < 8; ++v)
          if (y0 + u < H && x0 + v < W)
            o[(int64_t)(y0 + u) * W + x0 + v] = (int16_t)(pk[(u * 8 + v) >> 1] >> (16 * (v & 1)));
    }
  } else {  // RASTER_I32
    int32_t *o = static_cast<int32_t *>(out);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int q[8];
#pragma unroll
      for (int v = 0; v < 8; ++v) q[v] = (int)(int16_t)(pk[(u * 8 + v) >> 1] >> (16 * (v & 1)));
      if (FAST) {
        int4 *row = reinterpret_cast<int4 *>(o + (int64_t)(y0 + u) * W + x0);
        row[0] = make_int4(q[0], q[1], q[2], q[3]);
        row[1] = make_int4(q[4], q[5], q[6], q[7]);
      } else {
#pragma unroll
        for (int v = 0; v < 8; ++v)
          if (y0 + u < H && x0 + v < W) o[(int64_t)(y0 + u) * W + x0 + v] = q[v];
      }
    }
  }
}

// ---------------------------------------------------------------------------
__device__ __forceinline__ double sreg_f64(double k) {  // opaque wave-uniform constant
  asm volatile("" : "+s"(k));
  return k;
}
__device__ __forceinline__ double vreg_f64(double k) {
  asm volatile("" : "+v"(k));
  return k;
}
__device__ __forceinline__ double fma_scale_add(double y, double k_s, double c_v) {  // fl(y * k + c), one rounding
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(y), "s"(k_s), "v"(c_v));
  return d;
}

// Dequantize (q * T, exact in int32), the 2-D DCT-III in pocketfft's float64
// operation order, /256 + 128, truncate, wrap, and store the 8x8 pixels of the
// block at (y0, x0) of the H x W plane (FAST: whole block inside, 8-byte rows).
template <int TABLE>
__device__ __forceinline__ void idct_block_px(const int (&q)[64], uint32_t (&px)[16]) {
  // dequantize (q * T, exact in int32) and row pass
  double a[8][8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    int c[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) c[v] = q[u * 8 + v] * QT[TABLE][u * 8 + v];
    idct8<int>(c, a[u]);
  }
  // column pass, /256 (exact) + 128, truncate toward zero, wrap mod 256.  The
  // constants live in registers (2^-8 an SGPR pair, 128 a VGPR pair) for a
  // three-address v_fma_f64: LLVM's v_fmac_f64 form overwrote its accumulator,
  // so it re-materialised 128.0 (two v_mov_b32) before each of the 64 fmas
  const double k2m8 = sreg_f64(0x1p-8), k128 = vreg_f64(128.0);
  // row r: bytes v = 0..3 in px[2r], 4..7 in px[2r+1].  A truncated value's low
  // byte is the wrapped pixel; bytes are packed by byte permutes, a pair of columns
  // per v_perm and two pairs per dword (3 instructions per 4 pixels)
  uint32_t even[8];  // row r's pixel of the even column of the pair being packed
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    double xc[8], yv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) xc[u] = a[u][v];
    idct8<double>(xc, yv);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const double p = fma_scale_add(yv[r], k2m8, k128);  // == fl(y/256 + 128): y*2^-8 exact
      const uint32_t b = (uint32_t)__double2int_rz(p);
      if (!(v & 1)) {
        even[r] = b;
      } else {
        const uint32_t pair = __builtin_amdgcn_perm(b, even[r], 0x0C0C0400u);  // even.b0 | b.b0 << 8
        uint32_t &d = px[2 * r + (v >> 2)];
        d = (v & 2) ? __builtin_amdgcn_perm(pair, d, 0x05040100u) : pair;
      }
    }
  }
}
template <int TABLE, bool FAST>
__device__ __forceinline__ void idct_block_store(const int (&q)[64], int H, int W, int y0, int x0,
                                                 uint8_t *__restrict__ out, int64_t ostride) {
  uint32_t px[16];
  idct_block_px<TABLE>(q, px);
  if (FAST) {
    uint8_t *o = out + (int64_t)y0 * ostride + x0;  // one 64-bit multiply; rows step by the uniform stride
#pragma unroll
    for (int r = 0; r < 8; ++r) *reinterpret_cast<uint2 *>(o + r * ostride) = make_uint2(px[2 * r], px[2 * r + 1]);
  } else {
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int v = 0; v < 8; ++v)
        if (y0 + r < H && x0 + v < W)
          out[(int64_t)(y0 + r) * ostride + x0 + v] = (uint8_t)(px[2 * r + (v >> 2)] >> (8 * (v & 3)));
  }
}

template <int TABLE, int LAYOUT, bool FAST>
__global__ __launch_bounds__(256) void k_dequant_idct(const void *__restrict__ coef, int H, int W,
                                                      int nbx, int nblk, uint8_t *__restrict__ out,
                                                      int64_t ostride) {
  const int blk = blockIdx.x * 256 + threadIdx.x;
  if (blk >= nblk) return;
  const int bi = blk / nbx, bj = blk - bi * nbx;
  const int y0 = bi * 8, x0 = bj * 8;

  int q[64];  // raster [u][v]
  if (LAYOUT == HIC_LAYOUT_ZIGZAG_I16) {
    const uint4 *src = reinterpret_cast<const uint4 *>(static_cast<const int16_t *>(coef) + (int64_t)blk * 64);
    uint32_t w[32];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint4 t = src[k];
      w[4 * k] = t.x;
      w[4 * k + 1] = t.y;
      w[4 * k + 2] = t.z;
      w[4 * k + 3] = t.w;
    }
#pragma unroll
    for (int z = 0; z < 64; ++z) q[ZZ[z]] = (int)(int16_t)(w[z >> 1] >> (16 * (z & 1)));
    if (!FAST && (y0 + 8 > H || x0 + 8 > W)) {
#pragma unroll
      for (int i = 0; i < 64; ++i)
        if (y0 + i / 8 >= H || x0 + i % 8 >= W) q[i] = 0;
    }
  } else if (LAYOUT == HIC_LAYOUT_RASTER_I16) {
    const int16_t *c = static_cast<const int16_t *>(coef);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (FAST) {
        const uint4 t = *reinterpret_cast<const uint4 *>(c + (int64_t)(y0 + u) * W + x0);
        const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int v = 0; v < 8; ++v) q[u * 8 + v] = (int)(int16_t)(w[v >> 1] >> (16 * (v & 1)));
      } else {
#pragma unroll
        for (int v = 0; v < 8; ++v)
          q[u * 8 + v] = (y0 + u < H && x0 + v < W) ? (int)c[(int64_t)(y0 + u) * W + x0 + v] : 0;
      }
    }
  } else {
    const int32_t *c = static_cast<const int32_t *>(coef);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (FAST) {
        const int4 *row = reinterpret_cast<const int4 *>(c + (int64_t)(y0 + u) * W + x0);
        const int4 t0 = row[0], t1 = row[1];
        q[u * 8 + 0] = t0.x; q[u * 8 + 1] = t0.y; q[u * 8 + 2] = t0.z; q[u * 8 + 3] = t0.w;
        q[u * 8 + 4] = t1.x; q[u * 8 + 5] = t1.y; q[u * 8 + 6] = t1.z; q[u * 8 + 7] = t1.w;
      } else {
#pragma unroll
        for (int v = 0; v < 8; ++v)
          q[u * 8 + v] = (y0 + u < H && x0 + v < W) ? c[(int64_t)(y0 + u) * W + x0 + v] : 0;
      }
    }
  }

  idct_block_store<TABLE, FAST>(q, H, W, y0, x0, out, ostride);
}

// Indexed decode fused with the inverse transform: one wave per 64-block tile
// assembles its blocks in LDS from the symbols the encoder's tile index points at
// (as k_rld_indexed16 in rle.hip), then every lane runs the dequantize + IDCT of
// its block straight from LDS and stores pixels: the zig-zag blocks never reach
// HBM (codec.jpeg_decode's RLE / DC half, codec.py:397-421, + inv_dct_channel,
// transform.py:169-179, for one plane).
constexpr int kRowI16 = 68;  // LDS block row: 64 slots + pad (136 B, conflict-free 8 B reads)
// waves per SIMD: 3 (138 VGPRs, no spills) measured 2-6 % faster than 4 (128 VGPRs,
// ~10 spilled) once the gather went branch-free (profiles/r05/decode_wpe/)
#ifndef HIC_DEC_WPE
#define HIC_DEC_WPE 3
#endif
// The RGB of one 8x8 luma block (pixels px as idct_block_px leaves them) at block
// (bi, bj) of an H x W image, H and W multiples of 8: pyrUp(Cr), pyrUp(Cb) of the
// H/2 x W/2 chroma planes at its 64 pixels, then cvtColor(YCrCb2RGB)
// (compression.jpeg_decompression, compression.py:48-56).  The arithmetic is
// color.hip k_ycrcb420_rgb_walk's (cr | cb << 16 pairs biased by -1020 through both
// pyrUp passes, one v_dot2_i32_i16 per channel), so the bytes equal that kernel's
// on the same planes.  The chroma columns 4bj-1 / 4bj+4 next to the block's four come
// from the neighbouring lanes' blocks (DPP) or, at the wave's ends, from one extra
// dword load per row; reflect-101 at the top / left border, replicate at the
// bottom / right, as pyr_up_at.  Every lane of the wave must take part (the DPP
// reads); `live` gates the stores.
//
// The window form (WIN, geometry g: hic_window as the launcher checked it).  bi, bj,
// nbx, nby stay IMAGE coordinates, so the border rules do not move: reflect-101 at
// image row / column 0, replicate at the last; a window edge that is no image edge
// reads the chroma halo the window planes hold.  Only the addresses become
// window-relative: cr / cb are the window's chroma planes (chroma rows from g.cy0,
// columns from g.cx0, g.ch x g.cw samples, pitch g.cpitch), rgb the window's pixels
// (origin g.oy, g.ox).  All 64 lanes still run (the DPP reads), also those whose block
// lies outside the window: their chroma addresses are clamped into the window planes
// (a no-op for a block inside the window and for its left / right neighbour, whose
// columns the span holds by construction) and their stores are gated: a lane stores
// only a block of the wave's own block row wbi inside columns [g.bj0, g.bj1).
//
// The cropped form (CROP, with WIN; the batched region decode): rgb is a crop_h x
// crop_w x 3 result whose first pixel is image pixel (g.oy, g.ox), any pixel of the
// image, so a block of the aligned window may lie partly or wholly outside it and the
// address of a lane's 24 row bytes has any alignment.  A lane stores only its own bytes
// that fall inside the result: rows [0, crop_h), row bytes [0, 3 crop_w).  Its dwords
// that lie whole inside go out as dword stores at their own byte address (no alignment
// is promised to the compiler, which emits the store the target allows there; global
// memory takes misaligned dwords); a dword cut by the result's edge goes out byte by
// byte.  No lane ever writes a byte it does not own, so neighbours never race.
struct NoWin {};  // (WinGeo: decode_batch.h)
template <bool WIN>
using WinArg = std::conditional_t<WIN, WinGeo, NoWin>;
struct __attribute__((packed, aligned(1))) PackedU32 {
  uint32_t v;
};
// PITCH (the batched decode, whole planes): the chroma planes' rows are cpitch bytes
// apart instead of packed.
template <bool WIN = false, bool PITCH = false, bool CROP = false>
__device__ __forceinline__ void colour_block(const uint32_t (&px)[16], int bi, int bj, int nbx, int nby, int lane,
                                             bool live, const uint8_t *__restrict__ cr, const uint8_t *__restrict__ cb,
                                             uint8_t *__restrict__ rgb, int64_t rgb_stride,
                                             const WinArg<WIN> &g = WinArg<WIN>{}, int wbi = 0, int64_t cpitch = 0,
                                             int crop_h = 0, int crop_w = 0) {
  static_assert(!CROP || WIN, "the cropped store is the window form's");
  const int w = 4 * nbx, h = 4 * nby;
  // The packed pixels are opaque: otherwise the compiler forwards each truncated
  // pixel past its packing to the byte extracts below, and 64 live values instead
  // of 16 spill the IDCT.  bi, bj pass through the last of them, so no address
  // below is computed (and held) across the IDCT.
  uint32_t y[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    y[k] = px[k];
    asm volatile("" : "+v"(y[k]));
  }
  asm volatile("" : "+v"(bi), "+v"(bj) : "v"(y[15]));
  if constexpr (WIN) live = live && bi == wbi && bj >= g.bj0 && bj < g.bj1;
  // chroma rows 4bi-1 .. 4bi+4: its own four columns, and the wave-end lanes' outer
  // neighbour column (lane 0: the dword left of its own, lane 63: the one right)
  const int ce = lane == 0 ? (bj > 0 ? 4 * bj - 4 : 4 * bj) : (bj < nbx - 1 ? 4 * bj + 4 : 4 * bj);
  uint32_t dcr[6], dcb[6], ecr[6], ecb[6];
  if constexpr (WIN) {
    // window-relative dword columns, clamped into the planes (lanes outside the window)
    auto col = [&](int c) {
      c -= g.cx0;
      return c < 0 ? 0 : (c > g.cw - 4 ? g.cw - 4 : c);
    };
    const int c0 = col(4 * bj), c1 = col(ce);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      int s = 4 * bi - 1 + r;
      s = s < 0 ? 1 : (s >= h ? h - 1 : s);  // the image's border rule, then the window's origin
      s -= g.cy0;
      s = s < 0 ? 0 : (s > g.ch - 1 ? g.ch - 1 : s);
      const int ro = s * g.cpitch;  // (the launcher keeps ch * cpitch < 2^31)
      dcr[r] = *reinterpret_cast<const uint32_t *>(cr + ro + c0);
      dcb[r] = *reinterpret_cast<const uint32_t *>(cb + ro + c0);
      ecr[r] = *reinterpret_cast<const uint32_t *>(cr + ro + c1);
      ecb[r] = *reinterpret_cast<const uint32_t *>(cb + ro + c1);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      int s = 4 * bi - 1 + r;
      s = s < 0 ? 1 : (s >= h ? h - 1 : s);
      int64_t ro;
      if constexpr (PITCH) ro = (int64_t)s * cpitch;
      else ro = (int64_t)s * w;
      dcr[r] = *reinterpret_cast<const uint32_t *>(cr + ro + 4 * bj);
      dcb[r] = *reinterpret_cast<const uint32_t *>(cb + ro + 4 * bj);
      ecr[r] = *reinterpret_cast<const uint32_t *>(cr + ro + ce);
      ecb[r] = *reinterpret_cast<const uint32_t *>(cb + ro + ce);
    }
  }
  // KB: -1020 per half; K4 opaque (a splat 4 is strength-reduced to a shift + add)
  const uint32_t K4 = sreg(0x00040004u), K6 = 0x00060006u, KB = 0xFC04FC04u;
  const uint32_t kr = sreg((uint32_t)(uint16_t)kCR2R), kg = sreg((uint32_t)(uint16_t)kCR2G | (uint32_t)kCB2G << 16),
                 kb = sreg((uint32_t)kCB2B << 16);
  auto join = [](uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, 0x05040100u); };
  // horizontal pass of chroma row r: output columns 8bj .. 8bj+7 (x8 scale, biased)
  auto horiz = [&](int r, uint32_t (&hv)[8]) {
    uint32_t q[6];  // chroma columns 4bj-1 .. 4bj+4, packed cr | cb << 16
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j + 1] = __builtin_amdgcn_perm(dcb[r], dcr[r], 0x0C040C00u + 0x00010001u * j);
    uint32_t l = shr1(q[4]), rr = shl1(q[1]);
    l = lane == 0 ? __builtin_amdgcn_perm(ecb[r], ecr[r], 0x0C070C03u) : l;
    rr = lane == 63 ? __builtin_amdgcn_perm(ecb[r], ecr[r], 0x0C040C00u) : rr;
    q[0] = bj == 0 ? q[2] : l;         // reflect-101: column -1 -> 1
    q[5] = bj == nbx - 1 ? q[4] : rr;  // replicate: column w -> w - 1
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      hv[2 * c] = pk_mad_u16(q[c + 1], K6, pk_add_u16(q[c], pk_add_u16(q[c + 2], KB)));
      hv[2 * c + 1] = pk_mad_u16(pk_add_u16(q[c + 1], q[c + 2]), K4, KB);
    }
  };
  // output row 8bi + r8 from its vertical taps' packed sums v[8]
  auto emit = [&](int r8, const uint32_t (&v)[8]) {
    uint32_t o[6];
    int pend = 0;  // channel bytes waiting for their pair partner
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      const uint32_t crcb = pk_sra6(v[x]);  // (cr - 128, cb - 128)
      const int acc = (int)(((y[2 * r8 + (x >> 2)] >> (8 * (x & 3))) & 255u) << 14 | 8192u);
      const int c3[3] = {ycc_dot(crcb, kr, acc), ycc_dot(crcb, kg, acc), ycc_dot(crcb, kb, acc)};
      // bytes 3x .. 3x+2 of the row's 24: pairs (2m, 2m+1) -> one v_ashr_pk_u8_i32
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int byte = 3 * x + ch;
        if (byte & 1) {
          const uint32_t pr = sat_pk2(pend, c3[ch]);  // bytes byte-1, byte
          if ((byte >> 1) & 1) o[byte >> 2] = join(o[byte >> 2], pr);
          else o[byte >> 2] = pr;
        } else {
          pend = c3[ch];
        }
      }
    }
    if constexpr (CROP) {
      const int row = 8 * bi + r8 - g.oy;
      if (live && row >= 0 && row < crop_h) {
        // byte k of the lane's 24 is byte c0 + k of the result's row: it is stored when
        // lo <= k < hi (the pointer below is formed, never dereferenced, outside that)
        const int c0 = 24 * bj - 3 * g.ox, lo = -c0, hi = 3 * crop_w - c0;
        uint8_t *d = rgb + (int64_t)row * rgb_stride + c0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          if (4 * k >= lo && 4 * k + 4 <= hi) {
            reinterpret_cast<PackedU32 *>(d + 4 * k)->v = o[k];
          } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
              if (4 * k + b >= lo && 4 * k + b < hi) d[4 * k + b] = (uint8_t)(o[k] >> (8 * b));
          }
        }
      }
    } else if (live) {
      int oy = 0, ox = 0;
      if constexpr (WIN) oy = g.oy, ox = g.ox;
      uint2 *d = reinterpret_cast<uint2 *>(rgb + (int64_t)(8 * bi + r8 - oy) * rgb_stride + (24 * bj - 3 * ox));
      d[0] = make_uint2(o[0], o[1]);
      d[1] = make_uint2(o[2], o[3]);
      d[2] = make_uint2(o[4], o[5]);
    }
  };
  // a three-row window down chroma rows 4bi-1 .. 4bi+4: rows k, k+1, k+2 of it give
  // output rows 8bi + 2k ([1 6 1]) and 8bi + 2k + 1 ([4 4])
  uint32_t ha[8], hb[8], hc[8];
  horiz(0, ha);
  horiz(1, hb);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    horiz(k + 2, hc);
    uint32_t v[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) v[x] = pk_mad_u16(hb[x], K6, pk_add_u16(ha[x], hc[x]));
    emit(2 * k, v);
#pragma unroll
    for (int x = 0; x < 8; ++x) v[x] = pk_mad_u16(pk_add_u16(hb[x], hc[x]), K4, 0);
    emit(2 * k + 1, v);
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      ha[x] = hb[x];
      hb[x] = hc[x];
    }
  }
}

// RGB (luma plane only, TABLE 0, FAST): the pixels go through colour_block into
// the RGB image instead of to a Y plane -- the Y plane never reaches HBM
// (jpeg_decompression's decode of the luma channel + pyrUp + cvtColor, with the
// chroma planes decoded before).
// A second plane of the same shape and table (Cb beside Cr): the launch covers both
// planes' tiles, so the two share one tail (hic_rle_decode_idct_u8_indexed_pair).
struct DecPlane {
  const uint8_t *sym_len;
  const int16_t *sym_val;
  const int64_t *d_nsym;
  const int32_t *dc_diff;
  const int64_t *index;
  uint8_t *out;
  int64_t *d_status;
};
// One wave decodes tile t of plane p into the wave's LDS rows `tile` and stores its
// blocks: the body of k_rld_idct_indexed and of the batched k_rld_idct_batch, which
// differ in how a wave finds p and t.  TABLE, FAST, RGB, SLOTS, WIN as the kernels'.
// RSH >= 0 (the batch: Y 0, chroma 1): the records per tile are the compile-time
// 1 << RSH, rsh_arg is not read and the slot gather has no branch on it.  PITCH (the
// batch): the chroma planes' rows are `ostride` (plane form, stored as dwords: a
// multiple of 4, not of 8) or `cpitch` (RGB form, read) bytes apart.
// CROP (the batched region decode's luma launch): colour_block's cropped store into a
// crop_h x crop_w x 3 result.
template <int TABLE, bool FAST, bool RGB, bool SLOTS, bool WIN, bool PITCH = false, int RSH = -1, bool CROP = false>
__device__ __forceinline__ void decode_tile(const DecPlane &p, int64_t t, uint2 *tile, int lane, int H, int W, int nbx,
                                            int64_t nblk, int64_t ostride, const uint8_t *__restrict__ cr,
                                            const uint8_t *__restrict__ cb, int rsh_arg, const WinArg<WIN> &wg,
                                            int wbi, bool wfirst, int64_t cpitch = 0, int crop_h = 0, int crop_w = 0) {
  static_assert(!PITCH || (FAST && !WIN), "the pitched form holds whole planes of whole blocks");
  static_assert(!CROP || (RGB && WIN), "the cropped store is the RGB window form's");
  const int rsh = RSH >= 0 ? RSH : rsh_arg;
  const int64_t ntiles = (nblk + 63) / 64;
  int16_t *win = reinterpret_cast<int16_t *>(tile);
  const int64_t nsym_raw = *p.d_nsym, nsym = nsym_raw > 0 ? nsym_raw : 0;
  if constexpr (WIN) {
    if (wfirst && lane == 0) *p.d_status = nsym_raw < 1 ? -1 : wg.n_ac;
    if (nsym_raw < 1) return;  // a failed encode's count: nothing is decoded or stored
  }
  const int nvb = (int)(nblk - t * 64 < 64 ? nblk - t * 64 : 64);
  const int64_t blk = t * 64 + lane;
  // loads that depend on nothing else go out before the zero-fill: this lane's DC
  // difference and (slot layout) the tile's record index
  const int d = lane < nvb ? p.dc_diff[blk] : 0;
  // the gather (index, symbol loads, LDS scatter) at issue priority 1 over the
  // SIMD's waves in their IDCT / colour: 16K decode 0.713-0.766 vs 0.749-0.807 ms,
  // faster in 7 of 8 alternating rounds (profiles/r06/dec_prio/)
  __builtin_amdgcn_s_setprio(1);
  SlotTileIx six;
  if constexpr (SLOTS) six = slot_tile_ix(reinterpret_cast<const int32_t *>(p.index), t, rsh, nblk);
  for (int i = lane; i < 64 * kRowI16 / 4; i += 64) tile[i] = make_uint2(0, 0);
  __builtin_amdgcn_wave_barrier();
  // the symbols of the tile into its LDS rows (trash: the lane's row's first pad slot)
  int pdc;
  const int P = tile_symbols<kRowI16, SLOTS>(p.sym_len, p.sym_val, p.index, six, t, rsh, nsym, ntiles, nvb * 63, win,
                                             lane * kRowI16 + 64, lane, pdc);
  win[lane * kRowI16] = (int16_t)(pdc + wave_incl_sum_i32(d));
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_setprio(0);
  if (!WIN && t == ntiles - 1 && lane == 0)
    *p.d_status = stream_status<SLOTS>(nsym_raw, nsym, p.sym_len, p.sym_val, t * 64 * 63, P, nblk);
  if (!RGB && lane >= nvb) return;
  if constexpr (WIN && !RGB) {
    // the plane form needs no lane outside the window: only blocks of this wave's row
    const int wi = (int)(blk / nbx), wj = (int)(blk - (int64_t)wi * nbx);
    if (wi != wbi || wj < wg.bj0 || wj >= wg.bj1) return;
  }
  int qv[64];  // raster [u][v]
  {
    const uint2 *row = tile + (lane < nvb ? lane : nvb - 1) * (kRowI16 / 4);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint2 x = row[k];
      qv[ZZ[4 * k]] = (int)(int16_t)(x.x & 0xFFFFu);
      qv[ZZ[4 * k + 1]] = (int)(int16_t)(x.x >> 16);
      qv[ZZ[4 * k + 2]] = (int)(int16_t)(x.y & 0xFFFFu);
      qv[ZZ[4 * k + 3]] = (int)(int16_t)(x.y >> 16);
    }
  }
  const int64_t blk_c = lane < nvb ? blk : t * 64 + nvb - 1;  // RGB: the dead lanes redo the last block
  const int bi = (int)(blk_c / nbx), bj = (int)(blk_c - (int64_t)bi * nbx);
  if constexpr (RGB || PITCH) {
    uint32_t px[16];
    idct_block_px<TABLE>(qv, px);
    if constexpr (CROP) {
      colour_block<true, false, true>(px, bi, bj, nbx, H / 8, lane, lane < nvb, cr, cb, p.out, ostride, wg, wbi, 0,
                                      crop_h, crop_w);
    } else if constexpr (RGB && WIN) {
      colour_block<true>(px, bi, bj, nbx, H / 8, lane, lane < nvb, cr, cb, p.out, ostride, wg, wbi);
    } else if constexpr (RGB) {
      colour_block<false, PITCH>(px, bi, bj, nbx, H / 8, lane, lane < nvb, cr, cb, p.out, ostride, NoWin{}, 0, cpitch);
    } else {
      uint8_t *o = p.out + (int64_t)bi * 8 * ostride + bj * 8;
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        uint32_t *o32 = reinterpret_cast<uint32_t *>(o + rr * ostride);
        o32[0] = px[2 * rr];
        o32[1] = px[2 * rr + 1];
      }
    }
  } else if constexpr (WIN) {
    idct_block_store<TABLE, true>(qv, H, W, bi * 8 - wg.oy, bj * 8 - wg.ox, p.out, ostride);
  } else {
    idct_block_store<TABLE, FAST>(qv, H, W, bi * 8, bj * 8, p.out, ostride);
  }
}
// SLOTS: the symbols in the slot layout (slots.h), `index` the close's int32 record
// index, rsh = log2 records per 64-block tile.
// WIN: the window form (hic_rle_decode_idct_*_window).  The launch covers the blocks
// rows [wg.bi0, wg.bi0 + wg.nrows) x columns [wg.bj0, wg.bj1) of the plane, whole
// blocks, and `out` is a buffer of just those samples (origin wg.oy, wg.ox).  Waves
// are enumerated per block row: wg.tpr waves for row bi, wave k of them decoding tile
// floor((bi * nbx + bj0) / 64) + k while that is <= floor((bi * nbx + bj1 - 1) / 64).
// When nbx % 64 != 0 a tile wraps over two block rows and is decoded once per row it
// touches; each decode stores only the blocks of its own row inside the columns, so
// nothing outside the window's buffer is written and no block is written twice.
//  * A tile's carried zero run can start arbitrarily far before the window: the index
//    entry hands its start to the gather, which reads the tile's own symbols only
//    (index[3t], index[3(t + 1)] bound them), as in the whole-plane form.
//  * *d_status: the first wave of each plane writes -1 when *d_nsym < 1 and then no
//    wave decodes or stores anything; otherwise wg.n_ac (63 per block of the window).
//    No wave of a window launch writes the whole-stream completeness value: a window
//    does not see the whole stream.
template <int TABLE, bool FAST, bool RGB = false, bool SLOTS = false, bool WIN = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(HIC_DEC_WPE))) void k_rld_idct_indexed(
    DecPlane first, int H, int W, int nbx, int64_t nblk, int64_t ostride, const uint8_t *__restrict__ cr = nullptr,
    const uint8_t *__restrict__ cb = nullptr, DecPlane second = DecPlane{}, int rsh = 0,
    WinArg<WIN> wg = WinArg<WIN>{}) {
  static_assert(!RGB || (TABLE == 0 && FAST), "the RGB form decodes whole-block luma planes");
  static_assert(!WIN || FAST, "a window holds whole blocks");
  __shared__ uint2 s_tile[4][64 * kRowI16 / 4];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t ntiles = (nblk + 63) / 64;
  int64_t t = (int64_t)blockIdx.x * 4 + wv;
  int wbi = 0;          // WIN: the block row whose blocks this wave stores
  bool wsecond = false, wfirst = false;
  if constexpr (WIN) {
    // every quantity here is wave-uniform (scalar)
    int g = (int)t;
    const int nw = wg.nrows * wg.tpr;
    wsecond = !RGB && g >= nw;
    if (wsecond) {
      if (!second.sym_len || g >= 2 * nw) return;
      g -= nw;
    } else if (g >= nw) {
      return;
    }
    const int row = g / wg.tpr;
    wbi = wg.bi0 + row;
    const int64_t rb = (int64_t)wbi * nbx;
    t = (rb + wg.bj0) / 64 + (g - row * wg.tpr);
    if (t > (rb + wg.bj1 - 1) / 64) return;
    wfirst = g == 0;
  }
  const bool b = WIN ? wsecond : (!RGB && t >= ntiles);  // wave-uniform: the second plane's tile t - ntiles
  if constexpr (!WIN) {
    if (b) {
      if (!second.sym_len || t >= 2 * ntiles) return;
      t -= ntiles;
    } else if (t >= ntiles) {
      return;
    }
  }
  const DecPlane &f = first, &s = second;  // (a select of the whole by-value struct goes through scratch)
  const DecPlane pl{b ? s.sym_len : f.sym_len, b ? s.sym_val : f.sym_val, b ? s.d_nsym : f.d_nsym,
                    b ? s.dc_diff : f.dc_diff, b ? s.index : f.index, b ? s.out : f.out, b ? s.d_status : f.d_status};
  decode_tile<TABLE, FAST, RGB, SLOTS, WIN>(pl, t, s_tile[wv], lane, H, W, nbx, nblk, ostride, cr, cb, rsh, wg, wbi,
                                            wfirst);
}

// The batched form (hic_decode420_batch_u8, decode_batch.h): per wave the decode_tile
// of k_rld_idct_indexed<TABLE, true, RGB, SLOTS>, the plane's pointers read from the
// batch's table in device memory.  One wave per tile, per-wave LDS and
// only wave barriers, so the four waves of a workgroup may belong to different planes
// and to different images.  With g = blockIdx.x * 4 + wave and T = a.tiles waves per
// image (RGB: Y's tiles; else Cr's tiles, then Cb's): image g / T, plane (g % T) /
// ntiles, tile (g % T) % ntiles; a wave with g >= n * T returns.  All of it is
// wave-uniform and kept in SGPRs, so the table entry is read by scalar loads.  The
// records per tile are compile-time here (RSH).  The chroma planes' rows are a.cstride
// bytes apart (>= W / 2, a multiple of 4): plane form dword stores, RGB form dword loads.
struct DecBatchArgs {
  const DecBatchEntry *tab;
  uint32_t total, tiles;  // n * T, T
  int H, W, nbx;          // of the launch's planes
  int ntiles;             // of one plane
  int64_t nblk;
  int64_t ostride;        // RGB form: of the pixels; plane form: of the chroma planes
  int64_t cstride;        // RGB form: of the chroma planes it reads
};
template <int TABLE, bool RGB, bool SLOTS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(HIC_DEC_WPE))) void k_rld_idct_batch(DecBatchArgs a) {
  static_assert(!RGB || TABLE == 0, "the RGB form decodes luma planes");
  __shared__ uint2 s_tile[4][64 * kRowI16 / 4];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (uint32_t)wv);
  if (g >= a.total) return;
  const uint32_t img = g / a.tiles, r = g - img * a.tiles;
  const bool second = !RGB && r >= (uint32_t)a.ntiles;  // Cb's tiles follow Cr's
  const int64_t t = second ? r - (uint32_t)a.ntiles : r;
  // the entry through a constant-address-space pointer: a uniform address, scalar loads
  typedef const __attribute__((address_space(4))) DecBatchEntry centry;
  centry *ent = (centry *)(uintptr_t)(a.tab + img);
  const int ch = RGB ? 0 : (second ? 2 : 1);
  const DecPlane pl{ent->c[ch].sym_len, ent->c[ch].sym_val, ent->c[ch].d_nsym, ent->c[ch].dc_diff,
                    static_cast<const int64_t *>(ent->c[ch].index), ent->c[ch].out, ent->c[ch].d_status};
  const uint8_t *cr = RGB ? ent->c[1].out : nullptr, *cb = RGB ? ent->c[2].out : nullptr;
  decode_tile<TABLE, true, RGB, SLOTS, false, true, RGB ? 0 : 1>(pl, t, s_tile[wv], lane, a.H, a.W, a.nbx, a.nblk,
                                                                 a.ostride, cr, cb, 0, NoWin{}, 0, false, a.cstride);
}

// The batched window form (hic_decode420_window_batch_u8, decode_batch.h): per wave the
// decode_tile of k_rld_idct_indexed<TABLE, true, RGB, SLOTS, WIN>, the plane's pointers
// AND its window geometry read from the batch's table by scalar loads.  With g =
// blockIdx.x * 4 + wave and T = a.waves (uniform for the launch: the largest nrows * tpr
// any image of the batch plans, twice that in the chroma launch): image g / T, and
// within the image r = g % T enumerates (block row, k-th tile of the row) exactly as
// the one-image window form does with the image's OWN geometry: Cb's waves follow Cr's
// own nrows * tpr, a wave beyond its image's rows or its row's tiles returns.  The RGB
// form stores cropped (colour_block's CROP) into the image's h x w x 3 result, rows of
// a.ostride bytes; the plane form stores the chroma span into the image's chroma window
// buffer, rows of a.ostride bytes, which the RGB form then reads through g.cpitch.
struct DecWinBatchArgs {
  const DecWinBatchEntry *tab;
  uint32_t total, waves;  // n * T, T
  int H, W, nbx;          // of the launch's planes
  int crop_h, crop_w;     // RGB form: the result's rows and columns
  int64_t nblk;
  int64_t ostride;
};
template <int TABLE, bool RGB, bool SLOTS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(HIC_DEC_WPE))) void k_rld_idct_window_batch(
    DecWinBatchArgs a) {
  static_assert(!RGB || TABLE == 0, "the RGB form decodes luma planes");
  __shared__ uint2 s_tile[4][64 * kRowI16 / 4];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (uint32_t)wv);
  if (g >= a.total) return;
  const uint32_t img = g / a.waves;
  int r = (int)(g - img * a.waves);
  typedef const __attribute__((address_space(4))) DecWinBatchEntry centry;
  centry *ent = (centry *)(uintptr_t)(a.tab + img);
  const int gi = RGB ? 0 : 1;
  const WinGeo wg{ent->g[gi].bi0, ent->g[gi].nrows, ent->g[gi].bj0, ent->g[gi].bj1, ent->g[gi].tpr,   ent->g[gi].oy,
                  ent->g[gi].ox,  ent->g[gi].cy0,   ent->g[gi].cx0, ent->g[gi].ch,  ent->g[gi].cw,    ent->g[gi].cpitch,
                  ent->g[gi].n_ac};
  // every quantity here is wave-uniform (scalar), as in k_rld_idct_indexed's window form
  const int nw = wg.nrows * wg.tpr;
  const bool second = !RGB && r >= nw;  // Cb's waves follow Cr's
  if (second) r -= nw;
  if (r >= nw) return;
  const int row = r / wg.tpr, wbi = wg.bi0 + row;
  const int64_t rb = (int64_t)wbi * a.nbx;
  const int64_t t = (rb + wg.bj0) / 64 + (r - row * wg.tpr);
  if (t > (rb + wg.bj1 - 1) / 64) return;
  const int ch = RGB ? 0 : (second ? 2 : 1);
  const DecPlane pl{ent->c[ch].sym_len, ent->c[ch].sym_val, ent->c[ch].d_nsym, ent->c[ch].dc_diff,
                    static_cast<const int64_t *>(ent->c[ch].index), ent->c[ch].out, ent->c[ch].d_status};
  const uint8_t *cr = RGB ? ent->c[1].out : nullptr, *cb = RGB ? ent->c[2].out : nullptr;
  decode_tile<TABLE, true, RGB, SLOTS, true, false, RGB ? 0 : 1, RGB>(pl, t, s_tile[wv], lane, a.H, a.W, a.nbx, a.nblk,
                                                                      a.ostride, cr, cb, 0, wg, wbi, r == 0, 0,
                                                                      a.crop_h, a.crop_w);
}

// Production forward kernel for aligned planes: up to three planes per launch
// (Y, Cr, Cb of one image), one persistent grid over all their sets.  TABLE = -1:
// each plane's quantisation table is read at run time (its constants become scalar
// loads), so the three planes share one launch and one tail -- separate launches
// per table left a third of the waves idle in each tail.  TABLE = 0 / 1: a
// compile-time table (single-table callers).  One 8x8 block per lane, 64
// consecutive raster-order blocks ("a set" = one RLE tile) per wave iteration;
// persistent grid sized to the waves that fit at once.
// dct_block_aan (dct_core.h) writes the quantized coefficients straight to their
// slot in an LDS stage, which is copied out so that every store instruction writes
// one contiguous 1 KiB segment (zig-zag layout) or whole 16-byte row pieces
// (raster layouts).  TMF >= 0 (ZIGZAG_I16 only): the set's RLE tile record
// (rle_core.h) is written too -- the K1 pass of hic_rle_encode_i16 fused into the
// epilogue; TMF = 15 specialises max_len 15.
struct DctJob {
  const uint8_t *plane;
  int64_t stride;
  void *out;
  int64_t *tiles;
  int W, nbx, nblk, nsets, set0, table;
};
constexpr int kMaxPlaneJobs = 16;  // planes per launch (hic_dct_quant_rle_u8_batch)
struct DctJobs {
  DctJob j[kMaxPlaneJobs];
  int n, total_sets, M;
};

#ifndef HIC_DCT_WPE
#define HIC_DCT_WPE 3  // register budget: waves per SIMD (3: <= 168 VGPRs)
#endif
// (An LDS-DMA prefetch of the next set's pixels, round 6's dct_path 2, was bit-exact
// and within noise of these register loads: profiles/r06/glds_ab, commit "LDS-DMA
// prefetch form of the plane DCT"; removed.)
template <int TABLE, int LAYOUT, int TMF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(HIC_DCT_WPE))) void k_dct_planes(DctJobs jobs,
                                                                                                       int path) {
  __shared__ uint2 s_stage[4 * 64 * kStageU2];
  // wv is wave-uniform: keep it (and the set / job indices derived from it) in
  // SGPRs, so the job fields are scalar loads, not vector loads on vmcnt
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  const int g0 = blockIdx.x * 4 + wv;
  uint2 *st2 = s_stage + wv * 64 * kStageU2;
  int16_t *st = reinterpret_cast<int16_t *>(st2 + lane * kStageU2);
  // 16 B of block b's stage row, at 8-byte granularity (ds_read_b64 pairs)
  auto st16 = [&](int b, int k) {
    const uint2 lo = st2[b * kStageU2 + 2 * k], hi = st2[b * kStageU2 + 2 * k + 1];
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
  };
  const int M = jobs.M;

  // g is wave-uniform; readfirstlane keeps the job index in an SGPR (a VGPR index
  // into the by-value kernel argument copies it to scratch)
  auto job_of = [&](int g) {
    g = __builtin_amdgcn_readfirstlane(g);
    int k = 0;
    while (k + 1 < jobs.n && g >= jobs.j[k + 1].set0) ++k;
    return __builtin_amdgcn_readfirstlane(k);
  };
  auto load = [&](const DctJob &J, int set, uint2 (&w)[8]) {
    const int blk = set * 64 + lane;
    const int cblk = blk < J.nblk ? blk : J.nblk - 1;
    const int bi = cblk / J.nbx, bj = cblk - bi * J.nbx;
    const uint8_t *p = J.plane + (int64_t)bi * 8 * J.stride + bj * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) w[r] = *reinterpret_cast<const uint2 *>(p + r * J.stride);
  };
  // stage -> output layout (+ the RLE tile record)
  auto store = [&](const DctJob &J, int set) {
    __builtin_amdgcn_wave_barrier();
    const int blk = set * 64 + lane;
    if (LAYOUT == HIC_LAYOUT_ZIGZAG_I16) {
      uint4 *o = reinterpret_cast<uint4 *>(static_cast<int16_t *>(J.out) + (int64_t)set * 64 * 64);
      auto sv = [&](int k) { return st16(8 * k + (lane >> 3), lane & 7); };
      if ((set + 1) * 64 <= J.nblk) {
        // nontemporal stores (the compiler's own nt encoding; an inline-asm sc1
        // store was faster but broke the sharded encode, see DESIGN)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const uint4 t = sv(k);
          typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
          const u32x4 v = {t.x, t.y, t.z, t.w};
          __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(o + 64 * k + lane));
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (set * 64 + 8 * k + (lane >> 3) < J.nblk) o[64 * k + lane] = sv(k);
      }
      if (TMF >= 0) {
        uint32_t zw[32];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const uint4 t = st16(lane, k);
          zw[4 * k] = t.x; zw[4 * k + 1] = t.y; zw[4 * k + 2] = t.z; zw[4 * k + 3] = t.w;
        }
        tile_record16<TMF>(zw, blk < J.nblk, blk, M, J.tiles + (int64_t)set * 3);
      }
    } else if (blk < J.nblk) {
      const int bi = blk / J.nbx, bj = blk - bi * J.nbx;
      if (LAYOUT == HIC_LAYOUT_RASTER_I16) {
        int16_t *o = static_cast<int16_t *>(J.out) + (int64_t)bi * 8 * J.W + bj * 8;
#pragma unroll
        for (int u = 0; u < 8; ++u) *reinterpret_cast<uint4 *>(o + (int64_t)u * J.W) = st16(lane, u);
      } else {
        int32_t *o = static_cast<int32_t *>(J.out) + (int64_t)bi * 8 * J.W + bj * 8;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const uint4 t = st16(lane, u);
          const uint32_t wd[4] = {t.x, t.y, t.z, t.w};
          int q[8];
#pragma unroll
          for (int v = 0; v < 8; ++v) q[v] = (int)(int16_t)(wd[v >> 1] >> (16 * (v & 1)));
          int4 *row = reinterpret_cast<int4 *>(o + (int64_t)u * J.W);
          row[0] = make_int4(q[0], q[1], q[2], q[3]);
          row[1] = make_int4(q[4], q[5], q[6], q[7]);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  };

  // Main loop: the float64 AAN path.  A set with any coefficient inside the
  // quantiser's tie window is remembered (bit i of `redo` / `fix` = this wave's
  // i-th set; the launcher keeps every wave at <= 64 sets) and handled after the
  // loop -- a separate code region, so the paths do not share one register
  // allocation.  path 0 (A/B tests): exact replica only.
  uint64_t redo = 0, fix = 0;
  int i = 0;
  if (path != 0) {
    // the job's fields stay in SGPRs and are reloaded only when g enters the next
    // job (jobs are contiguous set ranges): no scalar loads on the per-set path
    int kj = g0 < jobs.total_sets ? job_of(g0) : 0;
    DctJob J = jobs.j[kj];
    int next0 = kj + 1 < jobs.n ? jobs.j[kj + 1].set0 : jobs.total_sets;
    // (a software-pipelined load of the next set's pixels into registers was measured
    // slower and removed: 160 vs 149 VGPRs, 8K luma 27.6-27.7 vs 25.6-26.2 us,
    // profiles/r03/s2/dct_pf/; the other waves of the SIMD hide the loads)
    for (int g = g0; g < jobs.total_sets; g += nwaves, ++i) {
      if (g >= next0) {
        kj = job_of(g);
        J = jobs.j[kj];
        next0 = kj + 1 < jobs.n ? jobs.j[kj + 1].set0 : jobs.total_sets;
      }
      const int set = g - J.set0;
      uint2 w[8];
      load(J, set, w);
      bool t26 = false;
      const bool f = dct_block_aan<TABLE, LAYOUT>(w, st, &t26, nullptr, J.table);
      if (__builtin_amdgcn_ballot_w64(f) != 0) redo |= 1ull << i;
      if (__builtin_amdgcn_ballot_w64(t26) != 0) fix |= 1ull << i;
      store(J, set);
    }
  } else {
    for (int g = g0; g < jobs.total_sets; g += nwaves, ++i) redo |= 1ull << i;
  }
  fix &= ~redo;
  // (2,2)-class exact ties: rewrite just those four coefficients of the set's
  // blocks in the output (and the set's RLE tile record)
  while (fix) {
    const int k = __builtin_ctzll(fix);
    fix &= fix - 1;
    const int g = g0 + k * nwaves;
    const DctJob &J = jobs.j[job_of(g)];
    const int set = g - J.set0;
    const int blk = set * 64 + lane;
    uint2 w[8];
    load(J, set, w);
    int q[4];
    dct_fix26<TABLE>(w, q, J.table);
    if (blk < J.nblk) {
      constexpr SlotOf<LAYOUT> kSlot{};
      constexpr int idx[4] = {18, 22, 50, 54};
      if (LAYOUT == HIC_LAYOUT_ZIGZAG_I16) {
        int16_t *o = static_cast<int16_t *>(J.out) + (int64_t)blk * 64;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[kSlot.s[idx[j]]] = (int16_t)q[j];
      } else {
        const int bi = blk / J.nbx, bj = blk - bi * J.nbx;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t at = (int64_t)(bi * 8 + idx[j] / 8) * J.W + bj * 8 + idx[j] % 8;
          if (LAYOUT == HIC_LAYOUT_RASTER_I16)
            static_cast<int16_t *>(J.out)[at] = (int16_t)q[j];
          else
            static_cast<int32_t *>(J.out)[at] = q[j];
        }
      }
    }
    if (LAYOUT == HIC_LAYOUT_ZIGZAG_I16 && TMF >= 0) {
      uint32_t zw[32];
      if (blk < J.nblk) {
        const uint4 *b4 = reinterpret_cast<const uint4 *>(static_cast<const int16_t *>(J.out) + (int64_t)blk * 64);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint4 t = b4[j];
          zw[4 * j] = t.x; zw[4 * j + 1] = t.y; zw[4 * j + 2] = t.z; zw[4 * j + 3] = t.w;
        }
      }
      tile_record16<TMF>(zw, blk < J.nblk, blk, M, J.tiles + (int64_t)set * 3);
    }
  }
  // any other tie (rare): the whole set again on the exact pocketfft replica
  while (redo) {
    const int k = __builtin_ctzll(redo);
    redo &= redo - 1;
    const int g = g0 + k * nwaves;
    const DctJob &J = jobs.j[job_of(g)];
    const int set = g - J.set0;
    uint2 w[8];
    load(J, set, w);
    dct_block_2ph<TABLE, LAYOUT>(w, st, J.table);
    store(J, set);
  }
}

// ---------------------------------------------------------------------------
// Block-level helpers (transform.dct2 / idct2, quantization.jpeg_quantize /
// invert_jpeg_quantize on arbitrary float64 / int blocks): one block per lane.
__global__ __launch_bounds__(256) void k_dct2_f64(const double *__restrict__ in, int64_t nblk, double *__restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= nblk) return;
  const double *p = in + b * 64;
  double a[8][8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    double x[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) x[n] = p[r * 8 + n];
    dct8h(x, a[r]);
  }
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    double xc[8], y[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) xc[r] = a[r][v];
    dct8h(xc, y);
#pragma unroll
    for (int u = 0; u < 8; ++u) out[b * 64 + u * 8 + v] = y[u] / (rho(u) * rho(v));  // exact power-of-2 rescale
  }
}

__global__ __launch_bounds__(256) void k_idct2_f64(const double *__restrict__ in, int64_t nblk, double *__restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= nblk) return;
  const double *p = in + b * 64;
  double a[8][8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    double x[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) x[n] = p[r * 8 + n];
    idct8<double>(x, a[r]);
  }
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    double xc[8], y[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) xc[r] = a[r][v];
    idct8<double>(xc, y);
#pragma unroll
    for (int r = 0; r < 8; ++r) out[b * 64 + r * 8 + v] = y[r] * 0x1p-8;  // == y / 256
  }
}

__global__ void k_quantize_f64(const double *__restrict__ in, int64_t n, int table, int32_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = (int32_t)__builtin_rint(in[i] / (double)QT[table][i & 63]);
}

__global__ void k_dequantize_i32(const int32_t *__restrict__ in, int64_t n, int table, int64_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = (int64_t)in[i] * QT[table][i & 63];
}

inline bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// Forward-path selection (A/B tests only; every path is bit-exact): knob
// "dct_path" 1 = float64 AAN fast path (k_dct_planes, the default), 2 = the same
// (its prefetch variant is compiled out), 0 = the exact pocketfft replica for every
// block; "dct_waves_per_cu" = persistent grid size (0 = one wave per set).  Round 5
// measured and removed the packed-float32 (path 3) and two-lanes-per-block (path 4)
// kernels (commit ae5c500 holds them).  Set through
// hic_set_knob (common.hip); the library reads no environment variables.
inline int dct_path() { return knob(HIC_KNOB_DCT_PATH); }
inline int dct_waves_per_cu(int njobs) {
  const int v = knob(HIC_KNOB_DCT_WAVES_PER_CU);
  if (v >= 0) return v;
  // float64 path: one wave per set for a multi-plane launch (the hardware's dispatch
  // balances the planes' mixed tail: 8K Y + Cr + Cb 37.5 us vs 39.7 for 12
  // persistent waves per CU), 12 persistent waves per CU for one plane (4K luma
  // 13.4 vs 13.8 us, 8K luma 27.4 vs 27.8; scripts/gpu_r2aj.sh)
  return njobs > 1 ? 0 : 12;
}

inline bool fwd_fast(int H, int W, int64_t stride, const void *plane, const void *out) {
  return (H % 8 == 0) && (W % 8 == 0) && (stride % 8 == 0) && aligned(plane, 8) && aligned(out, 16);
}

// Persistent launch of k_dct_planes over the jobs' sets (all fast-path planes).
template <int TABLE, int LAYOUT, int TMF>
int launch_planes(DctJobs &jobs, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  int total = 0;
  for (int k = 0; k < jobs.n; ++k) {
    jobs.j[k].set0 = total;
    total += jobs.j[k].nsets;
  }
  jobs.total_sets = total;
  int cap = dct_waves_per_cu(jobs.n) * cu_count();
  if (cap > 0 && (total + cap - 1) / cap > 64) cap = (total + 63) / 64;  // <= 64 sets per wave (redo mask)
  const int waves = (cap == 0 || total < cap) ? total : cap;
  const dim3 grid((waves + 3) / 4), block(256);
  const int path = dct_path();
  if (e0 || e1)
    hipExtLaunchKernelGGL((k_dct_planes<TABLE, LAYOUT, TMF>), grid, block, 0, s, e0, e1, 0, jobs, path);
  else
    hipLaunchKernelGGL((k_dct_planes<TABLE, LAYOUT, TMF>), grid, block, 0, s, jobs, path);
  return check_launch("k_dct_planes");
}

inline DctJob make_job(const uint8_t *plane, int H, int W, int64_t stride, int table, void *out, int64_t *tiles) {
  const int nbx = (W + 7) / 8, nblk = nbx * ((H + 7) / 8);
  return DctJob{plane, stride, out, tiles, W, nbx, nblk, (nblk + 63) / 64, 0, table};
}

template <int TABLE, int LAYOUT>
int launch_fwd(const uint8_t *plane, int H, int W, int64_t stride, void *out, hipStream_t s, hipEvent_t e0,
               hipEvent_t e1) {
  const int nbx = (W + 7) / 8, nby = (H + 7) / 8, nblk = nbx * nby;
  const bool fast = fwd_fast(H, W, stride, plane, out);
  const dim3 grid((nblk + 255) / 256), block(256);
  if (fast) {
    DctJobs jobs{};
    jobs.n = 1;
    jobs.j[0] = make_job(plane, H, W, stride, TABLE, out, nullptr);
    return launch_planes<TABLE, LAYOUT, -1>(jobs, s, e0, e1);
  } else if (e0 || e1)
    hipExtLaunchKernelGGL((k_dct_quant<TABLE, LAYOUT, false>), grid, block, 0, s, e0, e1, 0, plane, H, W, stride, nbx,
                          nblk, out);
  else
    hipLaunchKernelGGL((k_dct_quant<TABLE, LAYOUT, false>), grid, block, 0, s, plane, H, W, stride, nbx, nblk, out);
  return check_launch("k_dct_quant");
}

template <int TABLE, int LAYOUT>
int launch_inv(const void *coef, int H, int W, uint8_t *out, int64_t ostride, hipStream_t s) {
  const int nbx = (W + 7) / 8, nby = (H + 7) / 8, nblk = nbx * nby;
  const bool fast = (H % 8 == 0) && (W % 8 == 0) && (ostride % 8 == 0) && aligned(out, 8) && aligned(coef, 16);
  const dim3 grid((nblk + 255) / 256), block(256);
  if (fast)
    hipLaunchKernelGGL((k_dequant_idct<TABLE, LAYOUT, true>), grid, block, 0, s, coef, H, W, nbx, nblk, out, ostride);
  else
    hipLaunchKernelGGL((k_dequant_idct<TABLE, LAYOUT, false>), grid, block, 0, s, coef, H, W, nbx, nblk, out, ostride);
  return check_launch("k_dequant_idct");
}

bool dims_ok(int64_t H, int64_t W) {
  // one lane per block, int32 block / element indices
  return H > 0 && W > 0 && H < (1 << 20) && W < (1 << 20) && ((H + 7) / 8) * ((W + 7) / 8) < (1LL << 31) / 256;
}

}  // namespace
}  // namespace hic

using namespace hic;

extern "C" int hic_dct_quant_u8(const uint8_t *plane, int64_t H, int64_t W, int64_t stride, int table_id,
                                int layout, void *out, void *stream) {
  return hic_dct_quant_u8_timed(plane, H, W, stride, table_id, layout, out, stream, nullptr, nullptr);
}

extern "C" int hic_dct_quant_u8_timed(const uint8_t *plane, int64_t H, int64_t W, int64_t stride, int table_id,
                                      int layout, void *out, void *stream, void *ev_start, void *ev_stop) {
  if (!plane || !out) return arg_error("null pointer");
  if (!dims_ok(H, W) || stride < W) return arg_error("plane shape / stride");
  if (table_id != HIC_TABLE_LUMINANCE && table_id != HIC_TABLE_CHROMINANCE) return arg_error("table_id");
  hipStream_t s = as_stream(stream);
  const int h = (int)H, w = (int)W;
#define HIC_FWD(T, L) \
  return launch_fwd<T, L>(plane, h, w, stride, out, s, (hipEvent_t)ev_start, (hipEvent_t)ev_stop)
  if (table_id == 0) {
    if (layout == HIC_LAYOUT_RASTER_I32) HIC_FWD(0, HIC_LAYOUT_RASTER_I32);
    if (layout == HIC_LAYOUT_RASTER_I16) HIC_FWD(0, HIC_LAYOUT_RASTER_I16);
    if (layout == HIC_LAYOUT_ZIGZAG_I16) HIC_FWD(0, HIC_LAYOUT_ZIGZAG_I16);
  } else {
    if (layout == HIC_LAYOUT_RASTER_I32) HIC_FWD(1, HIC_LAYOUT_RASTER_I32);
    if (layout == HIC_LAYOUT_RASTER_I16) HIC_FWD(1, HIC_LAYOUT_RASTER_I16);
    if (layout == HIC_LAYOUT_ZIGZAG_I16) HIC_FWD(1, HIC_LAYOUT_ZIGZAG_I16);
  }
#undef HIC_FWD
  return arg_error("layout");
}

extern "C" int hic_dct_quant_rle_u8(const uint8_t *plane, int64_t H, int64_t W, int64_t stride, int table_id,
                                    int max_len, int16_t *out, void *rle_workspace, void *stream, void *ev_start,
                                    void *ev_stop) {
  hic_dct_plane_job job{plane, H, W, stride, table_id, out, rle_workspace};
  return hic_dct_quant_rle_u8_batch(1, &job, max_len, stream, ev_start, ev_stop);
}

extern "C" int hic_dct_quant_rle_u8_batch(int n, const hic_dct_plane_job *jobs, int max_len, void *stream,
                                          void *ev_start, void *ev_stop) {
  if (n < 1 || n > kMaxPlaneJobs || !jobs) return arg_error("1 <= n <= %d planes", kMaxPlaneJobs);
  if (max_len < 1 || max_len > 256) return arg_error("max_len must be in [1, 256]");
  hipStream_t s = as_stream(stream);
  const hipEvent_t e0 = (hipEvent_t)ev_start, e1 = (hipEvent_t)ev_stop;
  // fast-path planes: one launch for all of them (the kernel reads each plane's
  // table at run time)
  const bool merge = true;
  DctJobs fastj[2] = {};
  // rle_workspace: every job's or none (NULL: the records-free pass, DCT + quantize +
  // zig-zag only)
  const bool recs = jobs[0].rle_workspace != nullptr;
  // every job is checked before anything is launched (an error on job k > 0
  // used to return after the ragged planes before it were queued)
  for (int k = 0; k < n; ++k) {
    const hic_dct_plane_job &a = jobs[k];
    if (!a.plane || !a.out) return arg_error("plane %d: null pointer", k);
    if ((a.rle_workspace != nullptr) != recs) return arg_error("plane %d: rle_workspace for every plane or none", k);
    if (!dims_ok(a.H, a.W) || a.stride < a.W) return arg_error("plane %d: shape / stride", k);
    if (a.table_id != HIC_TABLE_LUMINANCE && a.table_id != HIC_TABLE_CHROMINANCE) return arg_error("plane %d: table_id", k);
  }
  for (int k = 0; k < n; ++k) {
    const hic_dct_plane_job &a = jobs[k];
    const int h = (int)a.H, w = (int)a.W;
    int64_t *tiles = static_cast<int64_t *>(a.rle_workspace);
    if (fwd_fast(h, w, a.stride, a.plane, a.out)) {
      DctJobs &J = fastj[merge ? 0 : a.table_id];
      J.j[J.n++] = make_job(a.plane, h, w, a.stride, a.table_id, a.out, tiles);
      continue;
    }
    // ragged plane: pocketfft replica, then the stand-alone tile pass
    const int e = a.table_id == 0 ? launch_fwd<0, HIC_LAYOUT_ZIGZAG_I16>(a.plane, h, w, a.stride, a.out, s, e0, e1)
                                  : launch_fwd<1, HIC_LAYOUT_ZIGZAG_I16>(a.plane, h, w, a.stride, a.out, s, e0, e1);
    if (e) return e;
    if (recs)
      if (int e2 = rle_tile16_launch(a.out, (int64_t)((h + 7) / 8) * ((w + 7) / 8), max_len, tiles, s)) return e2;
  }
  // the events (if any) time the first launch
  bool timed = false;
  for (int t = 0; t < 2; ++t) {
    DctJobs &J = fastj[t];
    if (J.n == 0) continue;
    J.M = max_len;
    const hipEvent_t a0 = timed ? nullptr : e0, a1 = timed ? nullptr : e1;
    timed = true;
    // one table for every job (a batch of luminance planes, say): the kernel compiled
    // for it, whose quantiser constants are literals instead of scalar loads per set
    int uni = J.j[0].table;
    for (int k = 1; k < J.n; ++k)
      if (J.j[k].table != uni) uni = -1;
    if (!merge) uni = t;
    int e;
    if (!recs)
      e = uni == 0   ? launch_planes<0, HIC_LAYOUT_ZIGZAG_I16, -1>(J, s, a0, a1)
          : uni == 1 ? launch_planes<1, HIC_LAYOUT_ZIGZAG_I16, -1>(J, s, a0, a1)
                     : launch_planes<-1, HIC_LAYOUT_ZIGZAG_I16, -1>(J, s, a0, a1);
    else if (uni == 0)
      e = max_len == 15 ? launch_planes<0, HIC_LAYOUT_ZIGZAG_I16, 15>(J, s, a0, a1)
                        : launch_planes<0, HIC_LAYOUT_ZIGZAG_I16, 0>(J, s, a0, a1);
    else if (uni == 1)
      e = max_len == 15 ? launch_planes<1, HIC_LAYOUT_ZIGZAG_I16, 15>(J, s, a0, a1)
                        : launch_planes<1, HIC_LAYOUT_ZIGZAG_I16, 0>(J, s, a0, a1);
    else
      e = max_len == 15 ? launch_planes<-1, HIC_LAYOUT_ZIGZAG_I16, 15>(J, s, a0, a1)
                        : launch_planes<-1, HIC_LAYOUT_ZIGZAG_I16, 0>(J, s, a0, a1);
    if (e) return e;
  }
  return HIC_OK;
}

extern "C" int hic_dequant_idct_u8(const void *coef, int layout, int64_t H, int64_t W, int table_id,
                                   uint8_t *out, int64_t out_stride, void *stream) {
  if (!coef || !out) return arg_error("null pointer");
  if (!dims_ok(H, W) || out_stride < W) return arg_error("plane shape / stride");
  if (table_id != HIC_TABLE_LUMINANCE && table_id != HIC_TABLE_CHROMINANCE) return arg_error("table_id");
  hipStream_t s = as_stream(stream);
  const int h = (int)H, w = (int)W;
#define HIC_INV(T, L) return launch_inv<T, L>(coef, h, w, out, out_stride, s)
  if (table_id == 0) {
    if (layout == HIC_LAYOUT_RASTER_I32) HIC_INV(0, HIC_LAYOUT_RASTER_I32);
    if (layout == HIC_LAYOUT_RASTER_I16) HIC_INV(0, HIC_LAYOUT_RASTER_I16);
    if (layout == HIC_LAYOUT_ZIGZAG_I16) HIC_INV(0, HIC_LAYOUT_ZIGZAG_I16);
  } else {
    if (layout == HIC_LAYOUT_RASTER_I32) HIC_INV(1, HIC_LAYOUT_RASTER_I32);
    if (layout == HIC_LAYOUT_RASTER_I16) HIC_INV(1, HIC_LAYOUT_RASTER_I16);
    if (layout == HIC_LAYOUT_ZIGZAG_I16) HIC_INV(1, HIC_LAYOUT_ZIGZAG_I16);
  }
#undef HIC_INV
  return arg_error("layout");
}

// ---- the fused tile decoders: six entry points, one launch of k_rld_idct_indexed.
// What a launch decodes, and from which kind of stream:
struct DecLaunch {
  DecPlane p[2];         // the plane, or the two planes of a chroma pair (one table, one shape)
  int nplanes;
  int64_t H, W;
  int table_id;
  int64_t out_stride;    // of every plane's `out` (the RGB form: of the interleaved pixels)
  bool rgb;              // luma straight to RGB: p[0].out is the pixels, cr / cb the decoded,
  const uint8_t *cr;     // upsampled chroma planes it reads
  const uint8_t *cb;
  bool slots;            // the symbols are in the slot layout (slots.h) and `index` is the close's
  int records_per_tile;  // int32 record index, 1 or 2 records per tile; otherwise a tile index
};

// Every check before any device call; then the grid and the kernel for (table, whole
// blocks, RGB, stream kind).
static int dec_planes_ok(const DecLaunch &d) {
  for (int k = 0; k < d.nplanes; ++k) {
    const DecPlane &p = d.p[k];
    char who[16] = "";
    if (d.nplanes > 1) snprintf(who, sizeof who, "plane %d: ", k);
    if (!p.sym_len || !p.sym_val || !p.d_nsym || !p.dc_diff || !p.index || !p.out || !p.d_status ||
        (d.rgb && (!d.cr || !d.cb)))
      return arg_error("%snull pointer", who);
    // the gathers read the symbols as uint4s
    if (!aligned(p.sym_len, 16) || !aligned(p.sym_val, 16))
      return arg_error("%s%s arrays must be 16-byte aligned", who, d.slots ? "slot" : "symbol");
  }
  return HIC_OK;
}
static int launch_rld_idct(const DecLaunch &d, void *stream) {
  if (int e = dec_planes_ok(d)) return e;
  if (d.rgb) {
    // the RGB form has no ragged path: whole 8x8 blocks, 8-byte pixel stores
    if (!dims_ok(d.H, d.W) || d.H % 8 || d.W % 8) return arg_error("plane shape (H, W multiples of 8)");
    if (d.out_stride < 3 * d.W || d.out_stride % 8 || !aligned(d.p[0].out, 8))
      return arg_error("rgb stride / alignment (8 B)");
    if (!aligned(d.cr, 4) || !aligned(d.cb, 4)) return arg_error("chroma planes must be 4-byte aligned");
  } else if (!dims_ok(d.H, d.W) || d.out_stride < d.W) {
    return arg_error("plane shape / stride");
  }
  if (d.table_id != HIC_TABLE_LUMINANCE && d.table_id != HIC_TABLE_CHROMINANCE) return arg_error("table_id");
  const int nbx = (int)((d.W + 7) / 8);
  const int64_t nblk = (int64_t)nbx * ((d.H + 7) / 8);
  if (nblk * 63 >= ((int64_t)1 << 31)) return arg_error("plane too large (AC stream >= 2^31)");
  if (d.slots) {
    if (d.records_per_tile != 1 && d.records_per_tile != 2) return arg_error("records_per_tile must be 1 or 2");
    if (nblk % (64 / d.records_per_tile)) return arg_error("the plane's blocks must form whole records");
  }
  bool fast = d.H % 8 == 0 && d.W % 8 == 0 && d.out_stride % 8 == 0;
  for (int k = 0; k < d.nplanes; ++k) fast = fast && aligned(d.p[k].out, 8);
  const int64_t ntiles = (nblk + 63) / 64;
  const dim3 grid((unsigned)((d.nplanes * ntiles + 3) / 4)), block(256);
  hipStream_t s = as_stream(stream);
  const DecPlane &a = d.p[0], second = d.nplanes > 1 ? d.p[1] : DecPlane{};
  const int rsh = d.slots && d.records_per_tile == 2 ? 1 : 0;
#define HIC_DEC(T, F, R, S)                                                                                         \
  hipLaunchKernelGGL((k_rld_idct_indexed<T, F, R, S>), grid, block, 0, s, a, (int)d.H, (int)d.W, nbx, nblk, \
                     d.out_stride, d.cr, d.cb, second, rsh)
#define HIC_DEC_PLANES(S)                                      \
  do {                                                         \
    if (d.table_id == 0 && fast) HIC_DEC(0, true, false, S);   \
    else if (d.table_id == 0) HIC_DEC(0, false, false, S);     \
    else if (fast) HIC_DEC(1, true, false, S);                 \
    else HIC_DEC(1, false, false, S);                          \
  } while (0)
  if (d.rgb && d.slots) HIC_DEC(0, true, true, true);  // (the checks above leave the RGB form whole blocks)
  else if (d.rgb) HIC_DEC(0, true, true, false);
  else if (d.slots) HIC_DEC_PLANES(true);
  else HIC_DEC_PLANES(false);
#undef HIC_DEC_PLANES
#undef HIC_DEC
  return check_launch("k_rld_idct_indexed");
}

// the slot layout's record index is int32; the kernel takes either index through one pointer
static const int64_t *slot_ix(const int32_t *d_index) { return reinterpret_cast<const int64_t *>(d_index); }

extern "C" int hic_rle_decode_idct_u8_indexed(const uint8_t *sym_len, const int16_t *sym_val, const int64_t *d_nsym,
                                              const int32_t *dc_diff, const int64_t *d_index, int64_t H, int64_t W,
                                              int table_id, uint8_t *out, int64_t out_stride, int64_t *d_status,
                                              void *stream) {
  DecLaunch d{};
  d.p[0] = DecPlane{sym_len, sym_val, d_nsym, dc_diff, d_index, out, d_status};
  d.nplanes = 1, d.H = H, d.W = W, d.table_id = table_id, d.out_stride = out_stride;
  return launch_rld_idct(d, stream);
}

extern "C" int hic_rle_decode_idct_u8_indexed_pair(const uint8_t *const *h_sym_len, const int16_t *const *h_sym_val,
                                                   const int64_t *const *h_d_nsym, const int32_t *const *h_dc_diff,
                                                   const int64_t *const *h_d_index, int64_t H, int64_t W, int table_id,
                                                   uint8_t *const *h_out, int64_t out_stride, int64_t *const *h_d_status,
                                                   void *stream) {
  if (!h_sym_len || !h_sym_val || !h_d_nsym || !h_dc_diff || !h_d_index || !h_out || !h_d_status)
    return arg_error("null pointer");
  DecLaunch d{};
  for (int k = 0; k < 2; ++k)
    d.p[k] = DecPlane{h_sym_len[k], h_sym_val[k], h_d_nsym[k], h_dc_diff[k], h_d_index[k], h_out[k], h_d_status[k]};
  d.nplanes = 2, d.H = H, d.W = W, d.table_id = table_id, d.out_stride = out_stride;
  return launch_rld_idct(d, stream);
}

extern "C" int hic_rle_decode_idct_rgb_indexed(const uint8_t *sym_len, const int16_t *sym_val, const int64_t *d_nsym,
                                               const int32_t *dc_diff, const int64_t *d_index, int64_t H, int64_t W,
                                               const uint8_t *cr, const uint8_t *cb, uint8_t *rgb, int64_t rgb_stride,
                                               int64_t *d_status, void *stream) {
  DecLaunch d{};
  d.p[0] = DecPlane{sym_len, sym_val, d_nsym, dc_diff, d_index, rgb, d_status};
  d.nplanes = 1, d.H = H, d.W = W, d.table_id = HIC_TABLE_LUMINANCE, d.out_stride = rgb_stride;
  d.rgb = true, d.cr = cr, d.cb = cb;
  return launch_rld_idct(d, stream);
}

extern "C" int hic_rle_decode_idct_u8_slots(const uint8_t *slot_len, const int16_t *slot_val, const int64_t *d_nsym,
                                            const int32_t *dc_diff, const int32_t *d_index, int records_per_tile,
                                            int64_t H, int64_t W, int table_id, uint8_t *out, int64_t out_stride,
                                            int64_t *d_status, void *stream) {
  DecLaunch d{};
  d.p[0] = DecPlane{slot_len, slot_val, d_nsym, dc_diff, slot_ix(d_index), out, d_status};
  d.nplanes = 1, d.H = H, d.W = W, d.table_id = table_id, d.out_stride = out_stride;
  d.slots = true, d.records_per_tile = records_per_tile;
  return launch_rld_idct(d, stream);
}

extern "C" int hic_rle_decode_idct_u8_slots_pair(const uint8_t *const *h_slot_len, const int16_t *const *h_slot_val,
                                                 const int64_t *const *h_d_nsym, const int32_t *const *h_dc_diff,
                                                 const int32_t *const *h_d_index, int records_per_tile, int64_t H,
                                                 int64_t W, int table_id, uint8_t *const *h_out, int64_t out_stride,
                                                 int64_t *const *h_d_status, void *stream) {
  if (!h_slot_len || !h_slot_val || !h_d_nsym || !h_dc_diff || !h_d_index || !h_out || !h_d_status)
    return arg_error("null pointer");
  DecLaunch d{};
  for (int k = 0; k < 2; ++k)
    d.p[k] = DecPlane{h_slot_len[k], h_slot_val[k], h_d_nsym[k], h_dc_diff[k], slot_ix(h_d_index[k]), h_out[k],
                      h_d_status[k]};
  d.nplanes = 2, d.H = H, d.W = W, d.table_id = table_id, d.out_stride = out_stride;
  d.slots = true, d.records_per_tile = records_per_tile;
  return launch_rld_idct(d, stream);
}

extern "C" int hic_rle_decode_idct_rgb_slots(const uint8_t *slot_len, const int16_t *slot_val, const int64_t *d_nsym,
                                             const int32_t *dc_diff, const int32_t *d_index, int records_per_tile,
                                             int64_t H, int64_t W, const uint8_t *cr, const uint8_t *cb, uint8_t *rgb,
                                             int64_t rgb_stride, int64_t *d_status, void *stream) {
  DecLaunch d{};
  d.p[0] = DecPlane{slot_len, slot_val, d_nsym, dc_diff, slot_ix(d_index), rgb, d_status};
  d.nplanes = 1, d.H = H, d.W = W, d.table_id = HIC_TABLE_LUMINANCE, d.out_stride = rgb_stride;
  d.rgb = true, d.cr = cr, d.cb = cb;
  d.slots = true, d.records_per_tile = records_per_tile;
  return launch_rld_idct(d, stream);
}

// ---- region decode: the window forms of the same kernel (DESIGN.md section 5,
// "Region decode").  hic_window_plan is the one statement of the geometry; the entry
// points accept only a window that equals the plan of its own aligned rectangle.
static int window_plan(int64_t H, int64_t W, int64_t y0, int64_t x0, int64_t h, int64_t w, hic_window *o) {
  if (!dims_ok(H, W) || H % 16 || W % 16) return arg_error("image shape (H, W multiples of 16)");
  if (h < 1 || w < 1 || y0 < 0 || x0 < 0 || y0 > H - h || x0 > W - w) return arg_error("window outside the image");
  auto dn = [](int64_t v, int64_t a) { return v / a * a; };
  auto up = [](int64_t v, int64_t a) { return (v + a - 1) / a * a; };
  o->Y0 = dn(y0, 16), o->X0 = dn(x0, 16), o->Y1 = up(y0 + h, 16), o->X1 = up(x0 + w, 16);
  // pyrUp's one-sample halo around chroma rows [Y0/2, Y1/2), clipped to the plane and
  // rounded out to whole 8x8 chroma blocks (H/2, W/2 are multiples of 8)
  const int64_t hc = H / 2, wc = W / 2;
  auto lo = [&](int64_t a) { return dn(a / 2 - 1 < 0 ? 0 : a / 2 - 1, 8); };
  auto hi = [&](int64_t b, int64_t n) { return up(b / 2 + 1 > n ? n : b / 2 + 1, 8); };
  o->cy0 = lo(o->Y0), o->cx0 = lo(o->X0);
  o->ch = hi(o->Y1, hc) - o->cy0, o->cw = hi(o->X1, wc) - o->cx0;
  return HIC_OK;
}

extern "C" int hic_window_plan(int64_t H, int64_t W, int64_t y0, int64_t x0, int64_t h, int64_t w, hic_window *out) {
  if (!out) return arg_error("null pointer");
  return window_plan(H, W, y0, x0, h, w, out);
}

// the most tiles one block row's columns [bj0, bj1) touch (rows [bi0, bi0 + nrows))
static int tiles_per_row(int nbx, int bi0, int nrows, int bj0, int bj1) {
  int m = 1;
  for (int bi = bi0; bi < bi0 + nrows; ++bi) {
    const int64_t rb = (int64_t)bi * nbx;
    const int n = (int)((rb + bj1 - 1) / 64 - (rb + bj0) / 64) + 1;
    m = n > m ? n : m;
  }
  return m;
}

// The kernels' geometry of one window launch: the luma launch over the aligned window
// (rgb) or the chroma launch over the chroma span, of a plane nbx blocks wide; cstride
// the chroma pitch the RGB form reads through.
static WinGeo window_geo(bool rgb, const hic_window &w, int nbx, int64_t cstride) {
  WinGeo g{};
  if (rgb) {
    g.bi0 = (int)(w.Y0 / 8), g.nrows = (int)((w.Y1 - w.Y0) / 8), g.bj0 = (int)(w.X0 / 8), g.bj1 = (int)(w.X1 / 8);
    g.oy = (int)w.Y0, g.ox = (int)w.X0;
  } else {
    g.bi0 = (int)(w.cy0 / 8), g.nrows = (int)(w.ch / 8), g.bj0 = (int)(w.cx0 / 8), g.bj1 = (int)((w.cx0 + w.cw) / 8);
    g.oy = (int)w.cy0, g.ox = (int)w.cx0;
  }
  g.cy0 = (int)w.cy0, g.cx0 = (int)w.cx0, g.ch = (int)w.ch, g.cw = (int)w.cw, g.cpitch = (int)cstride;
  g.tpr = tiles_per_row(nbx, g.bi0, g.nrows, g.bj0, g.bj1);
  g.n_ac = (int64_t)g.nrows * (g.bj1 - g.bj0) * 63;
  return g;
}

// d.H, d.W: the IMAGE's shape (the chroma pair's planes are H/2 x W/2); cstride: the
// RGB form's chroma pitch.  Every check before any device call.
static int launch_rld_idct_window(const DecLaunch &d, int kind, const hic_window *win, int64_t cstride, void *stream) {
  if (kind != HIC_STREAM_INDEXED && kind != HIC_STREAM_SLOTS) return arg_error("stream kind");
  if (int e = dec_planes_ok(d)) return e;
  if (!win) return arg_error("null pointer");
  const hic_window &w = *win;
  if (w.Y0 % 16 || w.X0 % 16 || w.Y1 % 16 || w.X1 % 16) return arg_error("the window must be 16-pixel aligned");
  hic_window want;
  if (int e = window_plan(d.H, d.W, w.Y0, w.X0, w.Y1 - w.Y0, w.X1 - w.X0, &want)) return e;
  if (w.cy0 != want.cy0 || w.cx0 != want.cx0 || w.ch != want.ch || w.cw != want.cw)
    return arg_error("the window's chroma span is not hic_window_plan's");
  const int64_t pH = d.rgb ? d.H : d.H / 2, pW = d.rgb ? d.W : d.W / 2;
  if (d.rgb) {
    if (d.out_stride < 3 * (w.X1 - w.X0) || d.out_stride % 8 || !aligned(d.p[0].out, 8))
      return arg_error("rgb stride / alignment (8 B)");
    // colour_block loads chroma dwords
    if (!aligned(d.cr, 4) || !aligned(d.cb, 4)) return arg_error("chroma planes must be 4-byte aligned");
    if (cstride < w.cw || cstride % 4) return arg_error("chroma pitch (>= the span, a multiple of 4)");
    if (w.ch * cstride >= ((int64_t)1 << 31)) return arg_error("chroma window too large");
  } else {
    // 8-byte row stores (and the RGB form's dword loads: 4 | 8)
    if (d.out_stride < w.cw || d.out_stride % 8) return arg_error("chroma pitch (>= the span, a multiple of 8)");
    for (int k = 0; k < d.nplanes; ++k)
      if (!aligned(d.p[k].out, 8)) return arg_error("plane %d: chroma planes must be 8-byte aligned", k);
  }
  const int nbx = (int)(pW / 8);
  const int64_t nblk = (int64_t)nbx * (pH / 8);
  if (nblk * 63 >= ((int64_t)1 << 31)) return arg_error("plane too large (AC stream >= 2^31)");
  if (d.slots) {
    if (d.records_per_tile != 1 && d.records_per_tile != 2) return arg_error("records_per_tile must be 1 or 2");
    if (nblk % (64 / d.records_per_tile)) return arg_error("the plane's blocks must form whole records");
  }
  const WinGeo g = window_geo(d.rgb, w, nbx, cstride);
  const int64_t waves = (int64_t)d.nplanes * g.nrows * g.tpr;
  const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
  hipStream_t s = as_stream(stream);
  const DecPlane &a = d.p[0], second = d.nplanes > 1 ? d.p[1] : DecPlane{};
  const int rsh = d.slots && d.records_per_tile == 2 ? 1 : 0;
#define HIC_DEC_WIN(T, R, S)                                                                                      \
  hipLaunchKernelGGL((k_rld_idct_indexed<T, true, R, S, true>), grid, block, 0, s, a, (int)pH, (int)pW, nbx, nblk, \
                     d.out_stride, d.cr, d.cb, second, rsh, g)
  if (d.rgb && d.slots) HIC_DEC_WIN(0, true, true);
  else if (d.rgb) HIC_DEC_WIN(0, true, false);
  else if (d.slots) HIC_DEC_WIN(1, false, true);
  else HIC_DEC_WIN(1, false, false);
#undef HIC_DEC_WIN
  return check_launch("k_rld_idct_indexed<window>");
}

extern "C" int hic_rle_decode_idct_u8_window_pair(int kind, const uint8_t *const *h_sym_len,
                                                  const int16_t *const *h_sym_val, const int64_t *const *h_d_nsym,
                                                  const int32_t *const *h_dc_diff, const void *const *h_d_index,
                                                  int records_per_tile, int64_t H, int64_t W, const hic_window *win,
                                                  uint8_t *const *h_out, int64_t out_stride,
                                                  int64_t *const *h_d_status, void *stream) {
  if (!h_sym_len || !h_sym_val || !h_d_nsym || !h_dc_diff || !h_d_index || !h_out || !h_d_status)
    return arg_error("null pointer");
  DecLaunch d{};
  for (int k = 0; k < 2; ++k)
    d.p[k] = DecPlane{h_sym_len[k], h_sym_val[k], h_d_nsym[k], h_dc_diff[k],
                      static_cast<const int64_t *>(h_d_index[k]), h_out[k], h_d_status[k]};
  d.nplanes = 2, d.H = H, d.W = W, d.table_id = HIC_TABLE_CHROMINANCE, d.out_stride = out_stride;
  d.slots = kind == HIC_STREAM_SLOTS, d.records_per_tile = records_per_tile;
  return launch_rld_idct_window(d, kind, win, 0, stream);
}

extern "C" int hic_rle_decode_idct_rgb_window(int kind, const uint8_t *sym_len, const int16_t *sym_val,
                                              const int64_t *d_nsym, const int32_t *dc_diff, const void *d_index,
                                              int records_per_tile, int64_t H, int64_t W, const hic_window *win,
                                              const uint8_t *cr, const uint8_t *cb, int64_t chroma_stride,
                                              uint8_t *rgb, int64_t rgb_stride, int64_t *d_status, void *stream) {
  DecLaunch d{};
  d.p[0] = DecPlane{sym_len, sym_val, d_nsym, dc_diff, static_cast<const int64_t *>(d_index), rgb, d_status};
  d.nplanes = 1, d.H = H, d.W = W, d.table_id = HIC_TABLE_LUMINANCE, d.out_stride = rgb_stride;
  d.rgb = true, d.cr = cr, d.cb = cb;
  d.slots = kind == HIC_STREAM_SLOTS, d.records_per_tile = records_per_tile;
  return launch_rld_idct_window(d, kind, win, chroma_stride, stream);
}

// ---- batched decode: n images of one shape in two launches (decode_batch.h, DESIGN.md
// section 5, "Batched decode").  The header of (kind, n, H, W, strides); nullptr =
// good, else what is wrong with them.
static const char *dec_batch_header(int kind, int n, int64_t H, int64_t W, int64_t rgb_stride, int64_t chroma_stride,
                                    DecBatchHeader &h) {
  if (kind != HIC_STREAM_INDEXED && kind != HIC_STREAM_SLOTS) return "stream kind";
  if (n < 1 || n > HIC_DECODE_BATCH_MAX) return "1 <= n <= HIC_DECODE_BATCH_MAX images";
  if (H < 16 || W < 16 || H % 16 || W % 16 || H >= (1 << 20) || W >= (1 << 20))
    return "image shape (H, W multiples of 16, at least 16)";
  if ((H / 8) * (W / 8) * 63 >= ((int64_t)1 << 31)) return "plane too large (AC stream >= 2^31)";
  if (!dims_ok(H, W)) return "image shape (too many blocks)";
  if (rgb_stride < 3 * W || rgb_stride % 8) return "rgb_stride (>= 3 W, a multiple of 8)";
  if (chroma_stride < W / 2 || chroma_stride % 4) return "chroma_stride (>= W / 2, a multiple of 4)";
  h = DecBatchHeader{};
  h.magic = kDecBatchMagic;
  h.kind = kind, h.n = n, h.H = H, h.W = W, h.rgb_stride = rgb_stride, h.chroma_stride = chroma_stride;
  h.nblk_y = (H / 8) * (W / 8), h.nblk_c = (H / 16) * (W / 16);
  if (kind == HIC_STREAM_SLOTS && (h.nblk_y % 64 || h.nblk_c % 32))
    return "the planes' blocks must form whole records (Y: 64, chroma: 32)";
  const int64_t ty = (h.nblk_y + 63) / 64, tc = 2 * ((h.nblk_c + 63) / 64);
  const int64_t gy = (n * ty + 3) / 4, gc = (n * tc + 3) / 4;
  // (the kernel counts waves in 32 bits, unsigned)
  if (gy > INT32_MAX || gc > INT32_MAX || 4 * gy > UINT32_MAX || 4 * gc > UINT32_MAX)
    return "grid above INT32_MAX workgroups";
  h.tiles_y = (int32_t)ty, h.tiles_c = (int32_t)tc, h.grid_y = (int32_t)gy, h.grid_c = (int32_t)gc;
  return nullptr;
}

extern "C" size_t hic_decode_batch_table_bytes(int n) {
  if (n < 1 || n > HIC_DECODE_BATCH_MAX) return 0;
  return sizeof(DecBatchHeader) + (size_t)n * sizeof(DecBatchEntry);
}

extern "C" int hic_decode_batch_table(int kind, int n, int64_t H, int64_t W, int64_t rgb_stride, int64_t chroma_stride,
                                      const hic_decode_image *images, void *h_table, size_t table_bytes) {
  DecBatchHeader h;
  if (const char *e = dec_batch_header(kind, n, H, W, rgb_stride, chroma_stride, h)) return arg_error(e);
  if (!images || !h_table) return arg_error("null pointer");
  if (table_bytes < hic_decode_batch_table_bytes(n))
    return arg_error("table of %lld bytes, %lld needed", (long long)table_bytes,
                     (long long)hic_decode_batch_table_bytes(n));
  // every image checked before a byte is written
  const bool slots = kind == HIC_STREAM_SLOTS;
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      const hic_decode_plane &p = images[i].c[k];
      if (!p.sym_len || !p.sym_val || !p.d_nsym || !p.dc_diff || !p.d_index || !p.out || !p.d_status)
        return arg_error("image %d channel %d: null pointer", i, k);
      // the gathers read the symbols as uint4s
      if (!aligned(p.sym_len, 16) || !aligned(p.sym_val, 16))
        return arg_error("image %d channel %d: %s arrays must be 16-byte aligned", i, k, slots ? "slot" : "symbol");
      // 8-byte pixel stores, dword chroma stores and loads
      if (!aligned(p.out, 8)) return arg_error("image %d channel %d: out must be 8-byte aligned", i, k);
      if (!aligned(p.d_nsym, 8) || !aligned(p.d_status, 8) || !aligned(p.dc_diff, 4) ||
          !aligned(p.d_index, slots ? 4 : 8))
        return arg_error("image %d channel %d: count / status / DC / index alignment", i, k);
    }
  // no two outputs of the batch may overlap (pixels, chroma planes, status words): sorted
  // by address, a range must end before the next one starts
  {
    struct Range {
      uintptr_t at, bytes;
      int image, chan, status;
    };
    std::vector<Range> r;
    r.reserve((size_t)6 * n);
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < 3; ++k) {
        const hic_decode_plane &p = images[i].c[k];
        const int64_t bytes = k == 0 ? (H - 1) * rgb_stride + 3 * W : (H / 2 - 1) * chroma_stride + W / 2;
        r.push_back(Range{reinterpret_cast<uintptr_t>(p.out), (uintptr_t)bytes, i, k, 0});
        r.push_back(Range{reinterpret_cast<uintptr_t>(p.d_status), 8, i, k, 1});
      }
    std::sort(r.begin(), r.end(), [](const Range &x, const Range &y) { return x.at < y.at; });
    const char *what[2] = {"output", "status word"};
    for (size_t i = 0; i + 1 < r.size(); ++i)
      if (r[i].at + r[i].bytes > r[i + 1].at)
        return arg_error("image %d channel %d: its %s overlaps the %s of image %d channel %d", r[i + 1].image,
                         r[i + 1].chan, what[r[i + 1].status], what[r[i].status], r[i].image, r[i].chan);
  }
  memcpy(h_table, &h, sizeof h);
  DecBatchEntry *ent = reinterpret_cast<DecBatchEntry *>(static_cast<char *>(h_table) + sizeof h);
  for (int i = 0; i < n; ++i) {
    DecBatchEntry e{};
    for (int k = 0; k < 3; ++k) {
      const hic_decode_plane &p = images[i].c[k];
      e.c[k] = DecBatchPlane{p.sym_len, p.sym_val, p.d_nsym, p.dc_diff, p.d_index, p.out, p.d_status};
    }
    memcpy(ent + i, &e, sizeof e);
  }
  return HIC_OK;
}

extern "C" int hic_decode420_batch_u8(const void *h_table, const void *d_table, void *stream) {
  if (!h_table || !d_table) return arg_error("null pointer");
  if (!aligned(d_table, 16)) return arg_error("d_table must be 16-byte aligned");
  DecBatchHeader h;
  memcpy(&h, h_table, sizeof h);
  if (h.magic != kDecBatchMagic) return arg_error("not a decode batch table (magic)");
  DecBatchHeader want;
  if (const char *e = dec_batch_header(h.kind, h.n, h.H, h.W, h.rgb_stride, h.chroma_stride, want)) return arg_error(e);
  if (memcmp(&want, &h, sizeof want)) return arg_error("damaged decode batch table header");
  DecBatchArgs a{};
  a.tab = reinterpret_cast<const DecBatchEntry *>(static_cast<const char *>(d_table) + sizeof h);
  const bool slots = h.kind == HIC_STREAM_SLOTS;
  hipStream_t s = as_stream(stream);
  const dim3 block(256);
  // every image's Cr and Cb planes ...
  a.total = (uint32_t)h.n * (uint32_t)h.tiles_c, a.tiles = (uint32_t)h.tiles_c;
  a.H = (int)(h.H / 2), a.W = (int)(h.W / 2), a.nbx = (int)(h.W / 16), a.ntiles = h.tiles_c / 2, a.nblk = h.nblk_c;
  a.ostride = h.chroma_stride, a.cstride = 0;
  if (slots) hipLaunchKernelGGL((k_rld_idct_batch<1, false, true>), dim3((unsigned)h.grid_c), block, 0, s, a);
  else hipLaunchKernelGGL((k_rld_idct_batch<1, false, false>), dim3((unsigned)h.grid_c), block, 0, s, a);
  if (int e = check_launch("k_rld_idct_batch<chroma>")) return e;
  // ... then every image's Y tiles straight to RGB, through its own chroma planes
  a.total = (uint32_t)h.n * (uint32_t)h.tiles_y, a.tiles = (uint32_t)h.tiles_y;
  a.H = (int)h.H, a.W = (int)h.W, a.nbx = (int)(h.W / 8), a.ntiles = h.tiles_y, a.nblk = h.nblk_y;
  a.ostride = h.rgb_stride, a.cstride = h.chroma_stride;
  if (slots) hipLaunchKernelGGL((k_rld_idct_batch<0, true, true>), dim3((unsigned)h.grid_y), block, 0, s, a);
  else hipLaunchKernelGGL((k_rld_idct_batch<0, true, false>), dim3((unsigned)h.grid_y), block, 0, s, a);
  return check_launch("k_rld_idct_batch<rgb>");
}

// ---- batched region decode: a window per image, n images of one shape, in two
// launches (decode_batch.h, DESIGN.md section 5, "Batched region decode").
// The largest aligned window and chroma span any origin can plan for an h x w request
// (pipeline.region_capacity), and the most waves per image each launch can then need.
struct WinCapacity {
  int64_t wh, ww, ch, cw;
  int64_t waves_y, waves_c;  // (waves_c: both chroma planes)
};
static WinCapacity window_capacity(int64_t H, int64_t W, int64_t h, int64_t w) {
  auto up16 = [](int64_t v) { return (v + 15) / 16 * 16; };
  WinCapacity c{};
  c.wh = std::min(H, up16(h + 15)), c.ww = std::min(W, up16(w + 15));
  c.ch = std::min(H / 2, c.wh / 2 + 16), c.cw = std::min(W / 2, c.ww / 2 + 16);
  // a run of L blocks of a raster touches at most (L + 62) / 64 + 1 tiles
  auto tpr = [](int64_t L, int64_t nblk) { return std::min((L + 62) / 64 + 1, (nblk + 63) / 64); };
  c.waves_y = c.wh / 8 * tpr(c.ww / 8, (H / 8) * (W / 8));
  c.waves_c = 2 * (c.ch / 8 * tpr(c.cw / 8, (H / 16) * (W / 16)));
  return c;
}

// The header of (kind, n, image shape, window shape, strides) but for the waves per
// image and the grids, which follow from the origins; nullptr = good, else what is wrong.
static const char *dec_win_batch_header(int kind, int n, int64_t H, int64_t W, int64_t h, int64_t w,
                                        int64_t out_row_stride, int64_t chroma_pitch, int64_t chroma_rows,
                                        DecWinBatchHeader &o) {
  DecBatchHeader whole;
  // (kind, n and the image shape as the whole-image batch takes them)
  if (const char *e = dec_batch_header(kind, n, H, W, 3 * W, W / 2, whole)) return e;
  if (h < 1 || w < 1 || h > H || w > W) return "window shape (1 <= h <= H, 1 <= w <= W)";
  if (out_row_stride < 3 * w || out_row_stride >= ((int64_t)1 << 31)) return "out_row_stride (>= 3 w, below 2^31)";
  const WinCapacity cap = window_capacity(H, W, h, w);
  // 8-byte chroma row stores, dword chroma loads; colour_block's row offsets are 32-bit
  if (chroma_pitch < cap.cw || chroma_pitch % 8) return "chroma_pitch (>= the capacity's columns, a multiple of 8)";
  if (chroma_rows < cap.ch) return "chroma_rows (>= the capacity's rows)";
  if (chroma_rows >= ((int64_t)1 << 31) / chroma_pitch) return "chroma window buffer too large";
  // (the kernel counts waves in 32 bits, unsigned)
  if (n * std::max(cap.waves_y, cap.waves_c) + 3 > (int64_t)INT32_MAX) return "grid above INT32_MAX / 4 workgroups";
  o = DecWinBatchHeader{};
  o.magic = kDecWinBatchMagic;
  o.kind = kind, o.n = n, o.H = H, o.W = W, o.h = h, o.w = w;
  o.out_row_stride = out_row_stride, o.chroma_pitch = chroma_pitch, o.chroma_rows = chroma_rows;
  o.nblk_y = whole.nblk_y, o.nblk_c = whole.nblk_c;
  return nullptr;
}

static void dec_win_batch_grids(DecWinBatchHeader &o, int64_t waves_y, int64_t waves_c) {
  o.waves_y = (int32_t)waves_y, o.waves_c = (int32_t)waves_c;
  o.grid_y = (int32_t)((o.n * waves_y + 3) / 4), o.grid_c = (int32_t)((o.n * waves_c + 3) / 4);
}

extern "C" size_t hic_decode_window_batch_table_bytes(int n) {
  if (n < 1 || n > HIC_DECODE_BATCH_MAX) return 0;
  return sizeof(DecWinBatchHeader) + (size_t)n * sizeof(DecWinBatchEntry);
}

extern "C" int hic_decode_window_batch_table(int kind, int n, int64_t H, int64_t W, int64_t h, int64_t w,
                                             const hic_decode_image *images, const int64_t *origins,
                                             int64_t out_row_stride, int64_t chroma_pitch, int64_t chroma_rows,
                                             void *h_table, size_t table_bytes) {
  DecWinBatchHeader hd;
  if (const char *e = dec_win_batch_header(kind, n, H, W, h, w, out_row_stride, chroma_pitch, chroma_rows, hd))
    return arg_error(e);
  if (!images || !origins || !h_table) return arg_error("null pointer");
  if (table_bytes < hic_decode_window_batch_table_bytes(n))
    return arg_error("table of %lld bytes, %lld needed", (long long)table_bytes,
                     (long long)hic_decode_window_batch_table_bytes(n));
  // every image checked and planned before a byte is written
  const bool slots = kind == HIC_STREAM_SLOTS;
  const WinCapacity cap = window_capacity(H, W, h, w);
  std::vector<DecWinBatchEntry> ents((size_t)n);
  int64_t waves_y = 1, waves_c = 2;
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < 3; ++k) {
      const hic_decode_plane &p = images[i].c[k];
      if (!p.sym_len || !p.sym_val || !p.d_nsym || !p.dc_diff || !p.d_index || !p.out || !p.d_status)
        return arg_error("image %d channel %d: null pointer", i, k);
      // the gathers read the symbols as uint4s
      if (!aligned(p.sym_len, 16) || !aligned(p.sym_val, 16))
        return arg_error("image %d channel %d: %s arrays must be 16-byte aligned", i, k, slots ? "slot" : "symbol");
      // 8-byte chroma row stores and dword chroma loads; the pixels are stored at any alignment
      if (k > 0 && !aligned(p.out, 8))
        return arg_error("image %d channel %d: the chroma window buffer must be 8-byte aligned", i, k);
      if (!aligned(p.d_nsym, 8) || !aligned(p.d_status, 8) || !aligned(p.dc_diff, 4) ||
          !aligned(p.d_index, slots ? 4 : 8))
        return arg_error("image %d channel %d: count / status / DC / index alignment", i, k);
    }
    const int64_t y0 = origins[2 * i], x0 = origins[2 * i + 1];
    hic_window win;
    if (y0 < 0 || x0 < 0 || y0 > H - h || x0 > W - w || window_plan(H, W, y0, x0, h, w, &win))
      return arg_error("image %d: window (%lld, %lld, %lld, %lld) outside the image", i, (long long)y0, (long long)x0,
                       (long long)h, (long long)w);
    if (win.Y1 - win.Y0 > cap.wh || win.X1 - win.X0 > cap.ww || win.ch > chroma_rows || win.cw > chroma_pitch)
      return arg_error("image %d: the window's plan exceeds the capacity", i);
    DecWinBatchEntry e{};
    for (int k = 0; k < 3; ++k) {
      const hic_decode_plane &p = images[i].c[k];
      e.c[k] = DecBatchPlane{p.sym_len, p.sym_val, p.d_nsym, p.dc_diff, p.d_index, p.out, p.d_status};
    }
    e.g[0] = window_geo(true, win, (int)(W / 8), chroma_pitch);
    e.g[0].oy = (int)y0, e.g[0].ox = (int)x0;  // the store crops: out's first pixel is the request's
    e.g[1] = window_geo(false, win, (int)(W / 16), chroma_pitch);
    e.y0 = (int32_t)y0, e.x0 = (int32_t)x0;
    waves_y = std::max(waves_y, (int64_t)e.g[0].nrows * e.g[0].tpr);
    waves_c = std::max(waves_c, 2 * (int64_t)e.g[1].nrows * e.g[1].tpr);
    ents[(size_t)i] = e;
  }
  if (waves_y > cap.waves_y || waves_c > cap.waves_c) return arg_error("internal: waves per image above the capacity's");
  // no two outputs of the batch may overlap (pixels, chroma window buffers, status words)
  {
    struct Range {
      uintptr_t at, bytes;
      int image, chan, status;
    };
    std::vector<Range> r;
    r.reserve((size_t)6 * n);
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < 3; ++k) {
        const hic_decode_plane &p = images[i].c[k];
        const int64_t bytes = k == 0 ? (h - 1) * out_row_stride + 3 * w : chroma_rows * chroma_pitch;
        r.push_back(Range{reinterpret_cast<uintptr_t>(p.out), (uintptr_t)bytes, i, k, 0});
        r.push_back(Range{reinterpret_cast<uintptr_t>(p.d_status), 8, i, k, 1});
      }
    std::sort(r.begin(), r.end(), [](const Range &x, const Range &y) { return x.at < y.at; });
    const char *what[2] = {"output", "status word"};
    for (size_t i = 0; i + 1 < r.size(); ++i)
      if (r[i].at + r[i].bytes > r[i + 1].at)
        return arg_error("image %d channel %d: its %s overlaps the %s of image %d channel %d", r[i + 1].image,
                         r[i + 1].chan, what[r[i + 1].status], what[r[i].status], r[i].image, r[i].chan);
  }
  dec_win_batch_grids(hd, waves_y, waves_c);
  memcpy(h_table, &hd, sizeof hd);
  memcpy(static_cast<char *>(h_table) + sizeof hd, ents.data(), (size_t)n * sizeof(DecWinBatchEntry));
  return HIC_OK;
}

extern "C" int hic_decode420_window_batch_u8(const void *h_table, const void *d_table, void *stream) {
  if (!h_table || !d_table) return arg_error("null pointer");
  if (!aligned(d_table, 16)) return arg_error("d_table must be 16-byte aligned");
  DecWinBatchHeader h;
  memcpy(&h, h_table, sizeof h);
  if (h.magic != kDecWinBatchMagic) return arg_error("not a window decode batch table (magic)");
  DecWinBatchHeader want;
  if (const char *e = dec_win_batch_header(h.kind, h.n, h.H, h.W, h.h, h.w, h.out_row_stride, h.chroma_pitch,
                                           h.chroma_rows, want))
    return arg_error(e);
  // the waves per image follow from the origins: any value up to the capacity's is a
  // table's (a wave checks itself against its own image's geometry), the rest must match
  const WinCapacity cap = window_capacity(h.H, h.W, h.h, h.w);
  if (h.waves_y < 1 || h.waves_y > cap.waves_y || h.waves_c < 2 || h.waves_c % 2 || h.waves_c > cap.waves_c)
    return arg_error("damaged window decode batch table header");
  dec_win_batch_grids(want, h.waves_y, h.waves_c);
  if (memcmp(&want, &h, sizeof want)) return arg_error("damaged window decode batch table header");
  DecWinBatchArgs a{};
  a.tab = reinterpret_cast<const DecWinBatchEntry *>(static_cast<const char *>(d_table) + sizeof h);
  const bool slots = h.kind == HIC_STREAM_SLOTS;
  hipStream_t s = as_stream(stream);
  const dim3 block(256);
  // every image's Cr and Cb spans into its chroma window buffers ...
  a.total = (uint32_t)h.n * (uint32_t)h.waves_c, a.waves = (uint32_t)h.waves_c;
  a.H = (int)(h.H / 2), a.W = (int)(h.W / 2), a.nbx = (int)(h.W / 16), a.nblk = h.nblk_c;
  a.ostride = h.chroma_pitch;
  if (slots) hipLaunchKernelGGL((k_rld_idct_window_batch<1, false, true>), dim3((unsigned)h.grid_c), block, 0, s, a);
  else hipLaunchKernelGGL((k_rld_idct_window_batch<1, false, false>), dim3((unsigned)h.grid_c), block, 0, s, a);
  if (int e = check_launch("k_rld_idct_window_batch<chroma>")) return e;
  // ... then every image's Y tiles of its aligned window straight to RGB, cropped
  a.total = (uint32_t)h.n * (uint32_t)h.waves_y, a.waves = (uint32_t)h.waves_y;
  a.H = (int)h.H, a.W = (int)h.W, a.nbx = (int)(h.W / 8), a.nblk = h.nblk_y;
  a.crop_h = (int)h.h, a.crop_w = (int)h.w, a.ostride = h.out_row_stride;
  if (slots) hipLaunchKernelGGL((k_rld_idct_window_batch<0, true, true>), dim3((unsigned)h.grid_y), block, 0, s, a);
  else hipLaunchKernelGGL((k_rld_idct_window_batch<0, true, false>), dim3((unsigned)h.grid_y), block, 0, s, a);
  return check_launch("k_rld_idct_window_batch<rgb>");
}

extern "C" int hic_dct2_f64(const double *in, int64_t nblk, double *out, void *stream) {
  if (!in || !out) return arg_error("null pointer");
  if (nblk <= 0) return arg_error("nblk");
  hipLaunchKernelGGL(k_dct2_f64, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, as_stream(stream), in, nblk, out);
  return check_launch("k_dct2_f64");
}

extern "C" int hic_idct2_f64(const double *in, int64_t nblk, double *out, void *stream) {
  if (!in || !out) return arg_error("null pointer");
  if (nblk <= 0) return arg_error("nblk");
  hipLaunchKernelGGL(k_idct2_f64, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, as_stream(stream), in, nblk, out);
  return check_launch("k_idct2_f64");
}

extern "C" int hic_quantize_f64(const double *in, int64_t nblk, int table_id, int32_t *out, void *stream) {
  if (!in || !out) return arg_error("null pointer");
  if (nblk <= 0) return arg_error("nblk");
  if (table_id != 0 && table_id != 1) return arg_error("table_id");
  const int64_t n = nblk * 64;
  hipLaunchKernelGGL(k_quantize_f64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), in, n,
                     table_id, out);
  return check_launch("k_quantize_f64");
}

extern "C" int hic_dequantize_i32(const int32_t *in, int64_t nblk, int table_id, int64_t *out, void *stream) {
  if (!in || !out) return arg_error("null pointer");
  if (nblk <= 0) return arg_error("nblk");
  if (table_id != 0 && table_id != 1) return arg_error("table_id");
  const int64_t n = nblk * 64;
  hipLaunchKernelGGL(k_dequantize_i32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), in, n,
                     table_id, out);
  return check_launch("k_dequantize_i32");
}
