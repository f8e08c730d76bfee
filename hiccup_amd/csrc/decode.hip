// decode.hip -- the fused tile decoders for MI355X (gfx950): RLE symbols (contiguous
// with a tile index, or the slot layout) -> dequantize + DCT-III (dct_core.h) ->
// pixels, one wave per 64-block tile, bit-exact against hiccup's scipy/numpy path.
// Device: colour_block, decode_tile (the body of every kernel) and the kernels, which
// differ in how a wave finds its plane and tile (one image, a batch, a window per image
// of a batch).  Host: the whole-plane and window entry points, and the two batch table
// formats (decode_batch.h) with their builders and launch calls.
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

}  // namespace
}  // namespace hic

using namespace hic;

// ---- the fused tile decoders: six entry points, one launch of k_rld_idct_indexed.
// What a launch decodes, and from which kind of stream:
struct DecLaunch {
  DecPlane p[2];         // the plane, or the two planes of a chroma pair (one table, one shape)
  int nplanes;
  int64_t H, W;
  int table_id;
  int64_t out_stride;    // of every plane's `out` (the RGB form: of the interleaved pixels)
  bool rgb;              // luma straight to RGB: p[0].out is the pixels, cr / cb the decoded,
  const uint8_t *cr, *cb;  // upsampled chroma planes it reads
  bool slots;            // the symbols are in the slot layout (slots.h) and `index` is the close's
  int records_per_tile;  // int32 record index, 1 or 2 records per tile; otherwise a tile index
  DecLaunch &to_rgb(const uint8_t *r, const uint8_t *b) { rgb = true, cr = r, cb = b; return *this; }
  DecLaunch &from_slots(bool on, int rpt) { slots = on, records_per_tile = rpt; return *this; }
};

// One plane's pointers and alignments: a launch's DecPlane or a batch table's
// hic_decode_plane (`index`: its index pointer), named `who` in the refusal.  out8: what
// `out` is when it must be 8-byte aligned (8-byte pixel or chroma row stores), else
// nullptr; table: also what the table formats ask of the count, status, DC and index.
template <typename Plane>
static int plane_ok(const char *who, const Plane &p, const void *index, bool slots, const char *out8, bool table) {
  if (!p.sym_len || !p.sym_val || !p.d_nsym || !p.dc_diff || !index || !p.out || !p.d_status)
    return arg_error("%snull pointer", who);
  // the gathers read the symbols as uint4s
  if (!aligned(p.sym_len, 16) || !aligned(p.sym_val, 16))
    return arg_error("%s%s arrays must be 16-byte aligned", who, slots ? "slot" : "symbol");
  if (out8 && !aligned(p.out, 8)) return arg_error("%s%s must be 8-byte aligned", who, out8);
  if (table && (!aligned(p.d_nsym, 8) || !aligned(p.d_status, 8) || !aligned(p.dc_diff, 4) ||
                !aligned(index, slots ? 4 : 8)))
    return arg_error("%scount / status / DC / index alignment", who);
  return HIC_OK;
}

// Every check before any device call; then the grid and the kernel for (table, whole
// blocks, RGB, stream kind).
static int dec_planes_ok(const DecLaunch &d) {
  if (d.rgb && (!d.cr || !d.cb)) return arg_error("null pointer");  // (one plane: no "plane k: ")
  for (int k = 0; k < d.nplanes; ++k) {
    char who[16] = "";
    if (d.nplanes > 1) snprintf(who, sizeof who, "plane %d: ", k);
    if (int e = plane_ok(who, d.p[k], d.p[k].index, d.slots, nullptr, false)) return e;
  }
  return HIC_OK;
}
// The launch's plane, pH x pW: its blocks per row and in all and log2 of the slot layout's
// records per tile, or a refusal (an AC stream of 2^31 positions, blocks short of records).
static int plane_limits(const DecLaunch &d, int64_t pH, int64_t pW, int &nbx, int64_t &nblk, int &rsh) {
  nbx = (int)((pW + 7) / 8);
  nblk = (int64_t)nbx * ((pH + 7) / 8);
  if (nblk * 63 >= ((int64_t)1 << 31)) return arg_error("plane too large (AC stream >= 2^31)");
  if (d.slots) {
    if (d.records_per_tile != 1 && d.records_per_tile != 2) return arg_error("records_per_tile must be 1 or 2");
    if (nblk % (64 / d.records_per_tile)) return arg_error("the plane's blocks must form whole records");
  }
  rsh = d.slots && d.records_per_tile == 2 ? 1 : 0;
  return HIC_OK;
}
static int launch_rld_idct(const DecLaunch &d, void *stream) {
  if (int e = dec_planes_ok(d)) return e;
  if (d.rgb) {
    // the RGB form has no ragged path: whole 8x8 blocks, 8-byte pixel stores
    if (!plane_dims_ok(d.H, d.W) || d.H % 8 || d.W % 8) return arg_error("plane shape (H, W multiples of 8)");
    if (d.out_stride < 3 * d.W || d.out_stride % 8 || !aligned(d.p[0].out, 8))
      return arg_error("rgb stride / alignment (8 B)");
    if (!aligned(d.cr, 4) || !aligned(d.cb, 4)) return arg_error("chroma planes must be 4-byte aligned");
  } else if (!plane_dims_ok(d.H, d.W) || d.out_stride < d.W) {
    return arg_error("plane shape / stride");
  }
  if (d.table_id != HIC_TABLE_LUMINANCE && d.table_id != HIC_TABLE_CHROMINANCE) return arg_error("table_id");
  int nbx, rsh;
  int64_t nblk;
  if (int e = plane_limits(d, d.H, d.W, nbx, nblk, rsh)) return e;
  bool fast = d.H % 8 == 0 && d.W % 8 == 0 && d.out_stride % 8 == 0;
  for (int k = 0; k < d.nplanes; ++k) fast = fast && aligned(d.p[k].out, 8);
  const int64_t ntiles = (nblk + 63) / 64;
  const dim3 grid((unsigned)((d.nplanes * ntiles + 3) / 4)), block(256);
  hipStream_t s = as_stream(stream);
  const DecPlane &a = d.p[0], second = d.nplanes > 1 ? d.p[1] : DecPlane{};
#define HIC_DEC(T, F, R, S)                                                                                        \
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

// The DecLaunch of an entry point's arguments: an indexed stream to a plane, unless to_rgb /
// from_slots say otherwise.  any_ix: the int64 tile index and the int32 record index share a pointer.
static const int64_t *any_ix(const void *d_index) { return static_cast<const int64_t *>(d_index); }
static DecLaunch one_plane(const DecPlane &p, int64_t H, int64_t W, int table_id, int64_t out_stride) {
  DecLaunch d{};
  d.p[0] = p, d.nplanes = 1, d.H = H, d.W = W, d.table_id = table_id, d.out_stride = out_stride;
  return d;
}
// The chroma pair, its pointers in host arrays of two (Cr, Cb).
template <typename Ix>
static int plane_pair(DecLaunch &d, const uint8_t *const *h_sym_len, const int16_t *const *h_sym_val,
                      const int64_t *const *h_d_nsym, const int32_t *const *h_dc_diff, const Ix *const *h_d_index,
                      uint8_t *const *h_out, int64_t *const *h_d_status, int64_t H, int64_t W, int table_id,
                      int64_t out_stride) {
  if (!h_sym_len || !h_sym_val || !h_d_nsym || !h_dc_diff || !h_d_index || !h_out || !h_d_status)
    return arg_error("null pointer");
  d = one_plane(DecPlane{}, H, W, table_id, out_stride), d.nplanes = 2;
  for (int k = 0; k < 2; ++k)
    d.p[k] = DecPlane{h_sym_len[k], h_sym_val[k], h_d_nsym[k], h_dc_diff[k], any_ix(h_d_index[k]), h_out[k],
                      h_d_status[k]};
  return HIC_OK;
}

extern "C" int hic_rle_decode_idct_u8_indexed(const uint8_t *sym_len, const int16_t *sym_val, const int64_t *d_nsym,
                                              const int32_t *dc_diff, const int64_t *d_index, int64_t H, int64_t W,
                                              int table_id, uint8_t *out, int64_t out_stride, int64_t *d_status,
                                              void *stream) {
  const DecPlane p{sym_len, sym_val, d_nsym, dc_diff, d_index, out, d_status};
  return launch_rld_idct(one_plane(p, H, W, table_id, out_stride), stream);
}

extern "C" int hic_rle_decode_idct_u8_indexed_pair(const uint8_t *const *h_sym_len, const int16_t *const *h_sym_val,
                                                   const int64_t *const *h_d_nsym, const int32_t *const *h_dc_diff,
                                                   const int64_t *const *h_d_index, int64_t H, int64_t W, int table_id,
                                                   uint8_t *const *h_out, int64_t out_stride, int64_t *const *h_d_status,
                                                   void *stream) {
  DecLaunch d;
  if (int e = plane_pair(d, h_sym_len, h_sym_val, h_d_nsym, h_dc_diff, h_d_index, h_out, h_d_status, H, W, table_id,
                         out_stride))
    return e;
  return launch_rld_idct(d, stream);
}

extern "C" int hic_rle_decode_idct_rgb_indexed(const uint8_t *sym_len, const int16_t *sym_val, const int64_t *d_nsym,
                                               const int32_t *dc_diff, const int64_t *d_index, int64_t H, int64_t W,
                                               const uint8_t *cr, const uint8_t *cb, uint8_t *rgb, int64_t rgb_stride,
                                               int64_t *d_status, void *stream) {
  const DecPlane p{sym_len, sym_val, d_nsym, dc_diff, d_index, rgb, d_status};
  return launch_rld_idct(one_plane(p, H, W, HIC_TABLE_LUMINANCE, rgb_stride).to_rgb(cr, cb), stream);
}

extern "C" int hic_rle_decode_idct_u8_slots(const uint8_t *slot_len, const int16_t *slot_val, const int64_t *d_nsym,
                                            const int32_t *dc_diff, const int32_t *d_index, int records_per_tile,
                                            int64_t H, int64_t W, int table_id, uint8_t *out, int64_t out_stride,
                                            int64_t *d_status, void *stream) {
  const DecPlane p{slot_len, slot_val, d_nsym, dc_diff, any_ix(d_index), out, d_status};
  return launch_rld_idct(one_plane(p, H, W, table_id, out_stride).from_slots(true, records_per_tile), stream);
}

extern "C" int hic_rle_decode_idct_u8_slots_pair(const uint8_t *const *h_slot_len, const int16_t *const *h_slot_val,
                                                 const int64_t *const *h_d_nsym, const int32_t *const *h_dc_diff,
                                                 const int32_t *const *h_d_index, int records_per_tile, int64_t H,
                                                 int64_t W, int table_id, uint8_t *const *h_out, int64_t out_stride,
                                                 int64_t *const *h_d_status, void *stream) {
  DecLaunch d;
  if (int e = plane_pair(d, h_slot_len, h_slot_val, h_d_nsym, h_dc_diff, h_d_index, h_out, h_d_status, H, W, table_id,
                         out_stride))
    return e;
  return launch_rld_idct(d.from_slots(true, records_per_tile), stream);
}

extern "C" int hic_rle_decode_idct_rgb_slots(const uint8_t *slot_len, const int16_t *slot_val, const int64_t *d_nsym,
                                             const int32_t *dc_diff, const int32_t *d_index, int records_per_tile,
                                             int64_t H, int64_t W, const uint8_t *cr, const uint8_t *cb, uint8_t *rgb,
                                             int64_t rgb_stride, int64_t *d_status, void *stream) {
  const DecPlane p{slot_len, slot_val, d_nsym, dc_diff, any_ix(d_index), rgb, d_status};
  DecLaunch d = one_plane(p, H, W, HIC_TABLE_LUMINANCE, rgb_stride);
  return launch_rld_idct(d.to_rgb(cr, cb).from_slots(true, records_per_tile), stream);
}

// ---- region decode: the window forms of the same kernel (DESIGN.md section 5,
// "Region decode").  hic_window_plan is the one statement of the geometry; the entry
// points accept only a window that equals the plan of its own aligned rectangle.
static int window_plan(int64_t H, int64_t W, int64_t y0, int64_t x0, int64_t h, int64_t w, hic_window *o) {
  if (!plane_dims_ok(H, W) || H % 16 || W % 16) return arg_error("image shape (H, W multiples of 16)");
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
  int nbx, rsh;
  int64_t nblk;
  if (int e = plane_limits(d, pH, pW, nbx, nblk, rsh)) return e;
  const WinGeo g = window_geo(d.rgb, w, nbx, cstride);
  const int64_t waves = (int64_t)d.nplanes * g.nrows * g.tpr;
  const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
  hipStream_t s = as_stream(stream);
  const DecPlane &a = d.p[0], second = d.nplanes > 1 ? d.p[1] : DecPlane{};
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
  DecLaunch d;
  if (int e = plane_pair(d, h_sym_len, h_sym_val, h_d_nsym, h_dc_diff, h_d_index, h_out, h_d_status, H, W,
                         HIC_TABLE_CHROMINANCE, out_stride))
    return e;
  return launch_rld_idct_window(d.from_slots(kind == HIC_STREAM_SLOTS, records_per_tile), kind, win, 0, stream);
}

extern "C" int hic_rle_decode_idct_rgb_window(int kind, const uint8_t *sym_len, const int16_t *sym_val,
                                              const int64_t *d_nsym, const int32_t *dc_diff, const void *d_index,
                                              int records_per_tile, int64_t H, int64_t W, const hic_window *win,
                                              const uint8_t *cr, const uint8_t *cb, int64_t chroma_stride,
                                              uint8_t *rgb, int64_t rgb_stride, int64_t *d_status, void *stream) {
  const DecPlane p{sym_len, sym_val, d_nsym, dc_diff, any_ix(d_index), rgb, d_status};
  DecLaunch d = one_plane(p, H, W, HIC_TABLE_LUMINANCE, rgb_stride);
  d.to_rgb(cr, cb).from_slots(kind == HIC_STREAM_SLOTS, records_per_tile);
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
  if (!plane_dims_ok(H, W)) return "image shape (too many blocks)";
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

// What both table builders ask of image i's three planes; out8_y, out8_c: plane_ok's
// out8 of the luma plane and of a chroma plane.
static int image_planes_ok(int i, const hic_decode_image &im, bool slots, const char *out8_y, const char *out8_c) {
  for (int k = 0; k < 3; ++k) {
    char who[40];
    snprintf(who, sizeof who, "image %d channel %d: ", i, k);
    if (int e = plane_ok(who, im.c[k], im.c[k].d_index, slots, k == 0 ? out8_y : out8_c, true)) return e;
  }
  return HIC_OK;
}
// No two outputs of a batch may overlap (pixels: luma_bytes, chroma planes or window buffers:
// chroma_bytes, status words): sorted by address, a range must end before the next one starts.
static int outputs_disjoint(int n, const hic_decode_image *images, int64_t luma_bytes, int64_t chroma_bytes) {
  struct Range {
    uintptr_t at, bytes;
    int image, chan, status;
  };
  std::vector<Range> r;
  r.reserve((size_t)6 * n);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      const hic_decode_plane &p = images[i].c[k];
      r.push_back(Range{reinterpret_cast<uintptr_t>(p.out), (uintptr_t)(k == 0 ? luma_bytes : chroma_bytes), i, k, 0});
      r.push_back(Range{reinterpret_cast<uintptr_t>(p.d_status), 8, i, k, 1});
    }
  std::sort(r.begin(), r.end(), [](const Range &x, const Range &y) { return x.at < y.at; });
  const char *what[2] = {"output", "status word"};
  for (size_t i = 0; i + 1 < r.size(); ++i)
    if (r[i].at + r[i].bytes > r[i + 1].at)
      return arg_error("image %d channel %d: its %s overlaps the %s of image %d channel %d", r[i + 1].image,
                       r[i + 1].chan, what[r[i + 1].status], what[r[i].status], r[i].image, r[i].chan);
  return HIC_OK;
}
// an image's three planes as a table entry holds them
static void table_planes(const hic_decode_image &im, DecBatchPlane (&c)[3]) {
  for (int k = 0; k < 3; ++k) {
    const hic_decode_plane &p = im.c[k];
    c[k] = DecBatchPlane{p.sym_len, p.sym_val, p.d_nsym, p.dc_diff, p.d_index, p.out, p.d_status};
  }
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
  // every image checked before a byte is written (out: 8-byte pixel stores, dword chroma stores and loads)
  for (int i = 0; i < n; ++i)
    if (int e = image_planes_ok(i, images[i], kind == HIC_STREAM_SLOTS, "out", "out")) return e;
  if (int e = outputs_disjoint(n, images, (H - 1) * rgb_stride + 3 * W, (H / 2 - 1) * chroma_stride + W / 2)) return e;
  memcpy(h_table, &h, sizeof h);
  DecBatchEntry *ent = reinterpret_cast<DecBatchEntry *>(static_cast<char *>(h_table) + sizeof h);
  for (int i = 0; i < n; ++i) {
    DecBatchEntry e{};
    table_planes(images[i], e.c);
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
    // 8-byte chroma row stores and dword chroma loads; the pixels are stored at any alignment
    if (int e = image_planes_ok(i, images[i], slots, nullptr, "the chroma window buffer")) return e;
    const int64_t y0 = origins[2 * i], x0 = origins[2 * i + 1];
    hic_window win;
    if (y0 < 0 || x0 < 0 || y0 > H - h || x0 > W - w || window_plan(H, W, y0, x0, h, w, &win))
      return arg_error("image %d: window (%lld, %lld, %lld, %lld) outside the image", i, (long long)y0, (long long)x0,
                       (long long)h, (long long)w);
    if (win.Y1 - win.Y0 > cap.wh || win.X1 - win.X0 > cap.ww || win.ch > chroma_rows || win.cw > chroma_pitch)
      return arg_error("image %d: the window's plan exceeds the capacity", i);
    DecWinBatchEntry e{};
    table_planes(images[i], e.c);
    e.g[0] = window_geo(true, win, (int)(W / 8), chroma_pitch);
    e.g[0].oy = (int)y0, e.g[0].ox = (int)x0;  // the store crops: out's first pixel is the request's
    e.g[1] = window_geo(false, win, (int)(W / 16), chroma_pitch);
    e.y0 = (int32_t)y0, e.x0 = (int32_t)x0;
    waves_y = std::max(waves_y, (int64_t)e.g[0].nrows * e.g[0].tpr);
    waves_c = std::max(waves_c, 2 * (int64_t)e.g[1].nrows * e.g[1].tpr);
    ents[(size_t)i] = e;
  }
  if (waves_y > cap.waves_y || waves_c > cap.waves_c) return arg_error("internal: waves per image above the capacity's");
  if (int e = outputs_disjoint(n, images, (h - 1) * out_row_stride + 3 * w, chroma_rows * chroma_pitch)) return e;
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
