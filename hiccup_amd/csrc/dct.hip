// dct.hip -- 8x8 block DCT-II + quantize (encode) and dequantize + DCT-III (decode)
// for MI355X (gfx950), bit-exact against hiccup's scipy/numpy path: the transform kernels
// on planes, the float64 block helpers and their entry points.  One block's dequantize +
// DCT-III is dct_core.h's, shared with the fused tile decoders (decode.hip).
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
#include "dct_core.h"
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
  if (!plane_dims_ok(H, W) || stride < W) return arg_error("plane shape / stride");
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
    if (!plane_dims_ok(a.H, a.W) || a.stride < a.W) return arg_error("plane %d: shape / stride", k);
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
  if (!plane_dims_ok(H, W) || out_stride < W) return arg_error("plane shape / stride");
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
