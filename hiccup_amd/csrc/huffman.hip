// huffman.hip -- the device half of hiccup's Huffman back end:
// the key histograms codec.jpeg_encode builds its nine trees from, and the bit
// packing of the coded streams.  The trees themselves (a heapq over at most a few
// thousand leaves, hiccup/huffman.py:11-58) stay on the host.
//
// Reference: codec.jpeg_encode (codec.py:304-334): huffman.HuffmanTree.
// construct_from_data(stream) = utils.group_by (keys in FIRST-APPEARANCE order,
// huffman.py:20-28 / utils.py:31-39: the tree's tie order depends on it) + counts;
// encode_data = the concatenated '0'/'1' codes (huffman.py:131-142); the
// container stores them MSB-first behind a pad-length byte (iohelper.py:35-56).
//
//  hic_key_range      min / max of a key stream (int8/16/32)
//  hic_key_histogram  per key in [key_min, key_min + nbins): count and the index of
//                     its first appearance (LDS-privatised: 4 B count + 4 B index
//                     per bin, nbins <= 8192; global atomics beyond)
//  hic_huffman_pack   per symbol its code (host table, <= 64 bits); tiles of 4096
//                     symbols assemble their bits in LDS (atomic OR into 32-bit
//                     words, MSB-first), interior words are stored, the two edge
//                     words shared with neighbouring tiles OR-ed in; *d_nbits = total
//                     bits (words past out_bytes are not written: the caller sizes
//                     the buffer from the histogram, sum of count x code length)
//  hic_slot_key_range / hic_slot_key_histogram / hic_slot_huffman_pack
//                     the same three steps over channels still in the slot layout
//                     (slots.h), every channel in one grid per phase and no compaction
//                     (the second half of this file)
//  hic_huffman_batch_key_range / _histogram / _pack
//                     the same three steps over the 9 n streams of n slot-layout
//                     images, one call per phase: the jobs in a table in device
//                     memory, the kernel bodies those of the entry points above
//                     (the end of this file)
#include <string.h>

#include <vector>

#include "hic_common.h"

namespace hic {
namespace {

constexpr int kHT = 256;                  // threads per workgroup
constexpr int kHPT = 16;                  // symbols per thread
constexpr int kHTile = kHT * kHPT;        // symbols per tile
constexpr int kHistLds = 8192;            // bins held in LDS
constexpr int kSlotCapMax = 64 * 63;      // symbols of the largest slot (slots.h)

__device__ __forceinline__ int key_at(const void *keys, int kb, int64_t i) {
  if (kb == 1) return (int)static_cast<const uint8_t *>(keys)[i];
  if (kb == 2) return (int)static_cast<const int16_t *>(keys)[i];
  return static_cast<const int32_t *>(keys)[i];
}

// min / max of the keys; keys at a 16-byte aligned address are read 16 bytes per
// load (the 8K jpeg_encode's nine streams: ~105 us per large stream read one key per
// load, 1- and 2-byte keys included)
// (workgroup wg of the nwg that share the stream)
template <int KB, bool VEC>
__device__ __forceinline__ void key_range_body(const void *__restrict__ keys, int64_t n, int *__restrict__ mm, int wg,
                                               int nwg) {
  int lo = 2147483647, hi = -2147483647 - 1;
  const int64_t t0 = (int64_t)wg * kHT + threadIdx.x, stride = (int64_t)nwg * kHT;
  int64_t tail = 0;
  if constexpr (VEC) {
    constexpr int kPer = 16 / KB;  // keys per 16-byte load
    const uint4 *v = static_cast<const uint4 *>(keys);
    const int64_t nv = n / kPer;
    for (int64_t i = t0; i < nv; i += stride) {
      const uint4 q = v[i];
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if constexpr (KB == 4) {
          lo = min(lo, (int)w[c]);
          hi = max(hi, (int)w[c]);
        } else if constexpr (KB == 2) {
          const int a = (int)(int16_t)(w[c] & 0xFFFFu), b = (int)(int16_t)(w[c] >> 16);
          lo = min(lo, min(a, b));
          hi = max(hi, max(a, b));
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int a = (int)((w[c] >> (8 * k)) & 0xFFu);
            lo = min(lo, a);
            hi = max(hi, a);
          }
        }
      }
    }
    tail = nv * kPer;
  }
  for (int64_t i = tail + t0; i < n; i += stride) {
    const int k = key_at(keys, KB, i);
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int a = __shfl_xor(lo, d, 64), b = __shfl_xor(hi, d, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  // one atomic pair per workgroup: thousands on one address serialise in the L2
  // (~100 us per large stream with one pair per wave)
  __shared__ int s_lo[kHT / 64], s_hi[kHT / 64];
  if ((threadIdx.x & 63) == 0) {
    s_lo[threadIdx.x >> 6] = lo;
    s_hi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kHT / 64; ++w) {
      lo = s_lo[w] < lo ? s_lo[w] : lo;
      hi = s_hi[w] > hi ? s_hi[w] : hi;
    }
    atomicMin(mm, lo);
    atomicMax(mm + 1, hi);
  }
}
template <int KB, bool VEC>
__global__ __launch_bounds__(kHT) void k_key_range(const void *__restrict__ keys, int64_t n, int *__restrict__ mm) {
  key_range_body<KB, VEC>(keys, n, mm, blockIdx.x, gridDim.x);
}

// counts / first: nbins entries, zero / 0xFFFFFFFF initialised by the launcher
// LDS: privatised bins; with `part` each workgroup stores its bins (count, first) to
// part[blockIdx.x] and k_hist_reduce sums them -- per-workgroup global atomics on
// every bin (512 workgroups x thousands of bins) took ~55 us per large stream
// (LDS: whether s_cnt / s_first hold the bins; workgroup wg of the stream's nwg)
__device__ __forceinline__ void key_hist_body(const bool LDS, uint32_t *s_cnt, uint32_t *s_first,
                                              const void *__restrict__ keys, int kb, int64_t n, int key_min, int nbins,
                                              uint32_t *__restrict__ counts, uint32_t *__restrict__ first,
                                              uint32_t *__restrict__ part, int wg, int nwg) {
  if (LDS) {
    for (int b = threadIdx.x; b < nbins; b += kHT) {
      s_cnt[b] = 0;
      s_first[b] = 0xFFFFFFFFu;
    }
    __syncthreads();
  }
  for (int64_t i = (int64_t)wg * kHT + threadIdx.x; i < n; i += (int64_t)nwg * kHT) {
    const int b = key_at(keys, kb, i) - key_min;
    if ((unsigned)b >= (unsigned)nbins) continue;  // outside the caller's range: not counted
    if (LDS) {
      atomicAdd(&s_cnt[b], 1u);
      // a bin's first index is found early and a thread's i only grows: read before
      // the atomic (it may miss a smaller value in flight; the atomic then keeps the min)
      if ((uint32_t)i < s_first[b]) atomicMin(&s_first[b], (uint32_t)i);
    } else {
      atomicAdd(&counts[b], 1u);
      atomicMin(&first[b], (uint32_t)i);
    }
  }
  if (LDS) {
    __syncthreads();
    if (part) {
      uint32_t *pc = part + (int64_t)wg * 2 * nbins;
      for (int b = threadIdx.x; b < nbins; b += kHT) {
        pc[b] = s_cnt[b];
        pc[nbins + b] = s_first[b];
      }
      return;
    }
    for (int b = threadIdx.x; b < nbins; b += kHT) {
      if (s_cnt[b]) {
        atomicAdd(&counts[b], s_cnt[b]);
        atomicMin(&first[b], s_first[b]);
      }
    }
  }
}
template <bool LDS>
__global__ __launch_bounds__(kHT) void k_key_hist(const void *__restrict__ keys, int kb, int64_t n, int key_min,
                                                  int nbins, uint32_t *__restrict__ counts,
                                                  uint32_t *__restrict__ first, uint32_t *__restrict__ part = nullptr) {
  __shared__ uint32_t s_cnt[LDS ? kHistLds : 1], s_first[LDS ? kHistLds : 1];
  key_hist_body(LDS, s_cnt, s_first, keys, kb, n, key_min, nbins, counts, first, part, blockIdx.x, gridDim.x);
}

// counts[b] / first[b] = the sum / min of the nwg workgroups' partial bins
__device__ __forceinline__ void hist_reduce_body(const uint32_t *__restrict__ part, int nwg, int nbins,
                                                 uint32_t *__restrict__ counts, uint32_t *__restrict__ first) {
  const int b = blockIdx.x * kHT + threadIdx.x;
  if (b >= nbins) return;
  uint32_t c = 0, f = 0xFFFFFFFFu;
  for (int w = 0; w < nwg; ++w) {
    const uint32_t *pc = part + (int64_t)w * 2 * nbins;
    c += pc[b];
    f = pc[nbins + b] < f ? pc[nbins + b] : f;
  }
  counts[b] = c;
  first[b] = f;
}
__global__ __launch_bounds__(kHT) void k_hist_reduce(const uint32_t *__restrict__ part, int nwg, int nbins,
                                                     uint32_t *__restrict__ counts, uint32_t *__restrict__ first) {
  hist_reduce_body(part, nwg, nbins, counts, first);
}

// block-wide exclusive sum (256 threads = 4 waves)
__device__ __forceinline__ int64_t blk_excl_sum(int64_t v, int64_t *s_w, int64_t &total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int64_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t o = __shfl_up(x, d, 64);
    if (lane >= d) x += o;
  }
  if (lane == 63) s_w[wv] = x;
  __syncthreads();
  int64_t pre = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < kHT / 64; ++k) {
    pre += k < wv ? s_w[k] : 0;
    total += s_w[k];
  }
  __syncthreads();
  return pre + x - v;
}

// pass A: bits per tile
__device__ __forceinline__ void pack_sizes_body(const void *__restrict__ keys, int kb, int64_t n, int key_min,
                                                int nbins, const uint8_t *__restrict__ code_len,
                                                int64_t *__restrict__ tile_bits) {
  __shared__ int64_t s_w[kHT / 64];
  const int64_t s0 = (int64_t)blockIdx.x * kHTile + (int64_t)threadIdx.x * kHPT;
  int64_t acc = 0;
#pragma unroll
  for (int k = 0; k < kHPT; ++k)
    if (s0 + k < n) {
      const int b = key_at(keys, kb, s0 + k) - key_min;
      acc += (unsigned)b < (unsigned)nbins ? code_len[b] : 0;  // a key outside the table codes to nothing
    }
  int64_t total;
  blk_excl_sum(acc, s_w, total);
  if (threadIdx.x == 0) tile_bits[blockIdx.x] = total;
}
__global__ __launch_bounds__(kHT) void k_pack_sizes(const void *__restrict__ keys, int kb, int64_t n, int key_min,
                                                    int nbins, const uint8_t *__restrict__ code_len,
                                                    int64_t *__restrict__ tile_bits) {
  pack_sizes_body(keys, kb, n, key_min, nbins, code_len, tile_bits);
}

// in-place exclusive scan of n int64 by one workgroup; *total = the sum
__device__ __forceinline__ void scan_in_place(int64_t *__restrict__ v, int64_t n, int64_t *__restrict__ total) {
  __shared__ int64_t s_w[kHT / 64];
  int64_t run = 0;
  for (int64_t c0 = 0; c0 < n; c0 += kHT) {
    const int64_t i = c0 + threadIdx.x;
    const int64_t x = i < n ? v[i] : 0;
    int64_t tot;
    const int64_t e = run + blk_excl_sum(x, s_w, tot);
    if (i < n) v[i] = e;
    run += tot;
  }
  if (threadIdx.x == 0) *total = run;
}
__global__ __launch_bounds__(kHT) void k_pack_scan(int64_t *__restrict__ v, int64_t n, int64_t *__restrict__ total) {
  scan_in_place(v, n, total);
}

__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

// pass B: each tile ORs its codes into an LDS word window (MSB-first), then writes
// the window: interior words stored (byte-swapped so memory is MSB-first bytes),
// the first / last word OR-ed atomically (shared with the neighbouring tiles).
// out must be zeroed; its words are big-endian bit runs.
constexpr int kPackWords = kHTile * 64 / 32 + 2;  // 64-bit codes at most
// one tile: ks = each thread's kHPT table indices in stream order (-1: codes to
// nothing), B0 = the tile's first bit.  Every thread of the workgroup must call it.
__device__ __forceinline__ void pack_tile(const int (&ks)[kHPT], const uint64_t *__restrict__ code_bits,
                                          const uint8_t *__restrict__ code_len, int64_t B0,
                                          uint32_t *__restrict__ out, int64_t out_words, uint32_t *s_words,
                                          int64_t *s_w) {
  int64_t acc = 0;
#pragma unroll
  for (int k = 0; k < kHPT; ++k) acc += ks[k] >= 0 ? code_len[ks[k]] : 0;
  int64_t tile_total;
  const int64_t my = blk_excl_sum(acc, s_w, tile_total);
  const int64_t w0 = B0 >> 5;                    // its first (global) word
  const int nwords = (int)(((B0 + tile_total + 31) >> 5) - w0);
  for (int i = threadIdx.x; i < nwords; i += kHT) s_words[i] = 0;
  __syncthreads();
  int64_t p = (B0 & 31) + my;  // bit position inside the window
#pragma unroll
  for (int k = 0; k < kHPT; ++k) {
    if (ks[k] < 0) continue;
    const int len = code_len[ks[k]];
    const uint64_t c = code_bits[ks[k]];
    // bits c[len-1 .. 0] go to window bits p .. p + len - 1 (MSB-first)
    int rem = len;
    int64_t q = p;
    while (rem > 0) {
      const int wi = (int)(q >> 5), off = (int)(q & 31);
      const int take = 32 - off < rem ? 32 - off : rem;
      const uint32_t piece = (uint32_t)((c >> (rem - take)) & ((take == 32) ? 0xFFFFFFFFull : ((1ull << take) - 1)));
      atomicOr(&s_words[wi], piece << (32 - off - take));
      rem -= take;
      q += take;
    }
    p += len;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nwords; i += kHT) {
    const uint32_t v = bswap32(s_words[i]);
    if (w0 + i >= out_words) break;  // buffer too small: *d_nbits tells the caller
    if ((i == 0 || i == nwords - 1)) {
      if (v) atomicOr(&out[w0 + i], v);
    } else {
      out[w0 + i] = v;
    }
  }
}
__device__ __forceinline__ void pack_bits_body(const void *__restrict__ keys, int kb, int64_t n, int key_min,
                                               int nbins, const uint64_t *__restrict__ code_bits,
                                               const uint8_t *__restrict__ code_len,
                                               const int64_t *__restrict__ tile_off, uint32_t *__restrict__ out,
                                               int64_t out_words, uint32_t *s_words) {
  __shared__ int64_t s_w[kHT / 64];
  const int64_t s0 = (int64_t)blockIdx.x * kHTile + (int64_t)threadIdx.x * kHPT;
  int ks[kHPT];
#pragma unroll
  for (int k = 0; k < kHPT; ++k) {
    ks[k] = s0 + k < n ? key_at(keys, kb, s0 + k) - key_min : -1;
    if ((unsigned)ks[k] >= (unsigned)nbins) ks[k] = -1;
  }
  pack_tile(ks, code_bits, code_len, tile_off[blockIdx.x], out, out_words, s_words, s_w);
}
__global__ __launch_bounds__(kHT) void k_pack_bits(const void *__restrict__ keys, int kb, int64_t n, int key_min,
                                                   int nbins, const uint64_t *__restrict__ code_bits,
                                                   const uint8_t *__restrict__ code_len,
                                                   const int64_t *__restrict__ tile_off, uint32_t *__restrict__ out,
                                                   int64_t out_words) {
  extern __shared__ uint32_t s_words[];
  pack_bits_body(keys, kb, n, key_min, nbins, code_bits, code_len, tile_off, out, out_words, s_words);
}

// The batched forms of the five kernels above (hic_huffman_batch_*): blockIdx.y = the
// stream, an int32 key stream (a DC stream) whose job is read from a table in device
// memory as the slot kernels' HsTable reads theirs; the bodies are the ones above.
// The grid's x is sized for the batch's longest stream: workgroups past a stream's
// own count leave at once, and the job's n bounds every load.
struct HkJob {
  const int32_t *keys;
  int64_t n;
  int key_min, nbins;
  uint32_t *cnt, *first;
  uint32_t *part;   // histogram: [nwg][2][nbins] per-workgroup bins; null: straight into cnt / first
  int nwg;          // histogram: the stream's workgroups
  int nt;           // pack: the stream's tiles
  const uint64_t *cbits;
  const uint8_t *clen;
  uint32_t *out;
  int64_t out_words;
  int64_t *tile;    // [nt]: the tiles' bits, then their first bits
  int64_t *d_nbits;
};
typedef const __attribute__((address_space(4))) HkJob HkJobC;
__device__ __forceinline__ HkJobC &hk_job(const HkJob *tab) { return *(HkJobC *)(uintptr_t)(tab + blockIdx.y); }

__global__ __launch_bounds__(kHT) void k_key_range_table(const HkJob *tab, int *__restrict__ mm) {
  HkJobC &J = hk_job(tab);
  key_range_body<4, true>(J.keys, J.n, mm + 2 * blockIdx.y, blockIdx.x, gridDim.x);
}
__global__ __launch_bounds__(kHT) void k_key_hist_table(const HkJob *tab) {
  __shared__ uint32_t s_cnt[kHistLds], s_first[kHistLds];
  HkJobC &J = hk_job(tab);
  if ((int)blockIdx.x >= J.nwg) return;
  key_hist_body(J.nbins <= kHistLds, s_cnt, s_first, J.keys, 4, J.n, J.key_min, J.nbins, J.cnt, J.first, J.part,
                blockIdx.x, J.nwg);
}
__global__ __launch_bounds__(kHT) void k_hist_reduce_table(const HkJob *tab) {
  HkJobC &J = hk_job(tab);
  if (!J.part) return;
  hist_reduce_body(J.part, J.nwg, J.nbins, J.cnt, J.first);
}
__global__ __launch_bounds__(kHT) void k_pack_sizes_table(const HkJob *tab) {
  HkJobC &J = hk_job(tab);
  if ((int)blockIdx.x >= J.nt) return;
  pack_sizes_body(J.keys, 4, J.n, J.key_min, J.nbins, J.clen, J.tile);
}
__global__ __launch_bounds__(kHT) void k_pack_scan_table(const HkJob *tab) {
  HkJobC &J = hk_job(tab);
  scan_in_place(J.tile, J.nt, J.d_nbits);
}
__global__ __launch_bounds__(kHT) void k_pack_bits_table(const HkJob *tab) {
  extern __shared__ uint32_t s_words[];
  HkJobC &J = hk_job(tab);
  if ((int)blockIdx.x >= J.nt) return;
  pack_bits_body(J.keys, 4, J.n, J.key_min, J.nbins, J.cbits, J.clen, J.tile, J.out, J.out_words, s_words);
}

// ---------------------------------------------------------------------------
// The same three steps over channels still in the slot layout (slots.h), with no
// compaction: a channel's "virtual stream" -- what hic_rle_slots_compact would
// write -- is, over its records r in order, nfill_r fillers (M - 1, 0) at stream
// offset offs_r, then slot r's n_r symbols, then the EOB (0, 0) when the count says
// there is one.  The EOB is handled as one more symbol of the LAST record (index
// n_r: a record whose every AC position is a symbol ends in a nonzero and has no
// EOB, so n_r + 1 never exceeds the slot).  Each channel gives two key streams:
// 0 = lengths (1-byte keys), 1 = values (2-byte keys); all kernels take every
// channel in one grid (blockIdx.y = the channel).
struct HsJob {
  const uint8_t *slot_len;
  const int16_t *slot_val;
  const int32_t *sidx;     // the close's {n, P, pdc, nfill} per record
  const int64_t *offs;     // the scan's offs[2 r] = record r's stream offset
  const int64_t *d_count;
  int64_t nrec;
  int capr;                // slot capacity (symbols): 4032 or 2016, whole 16-byte chunks
  int key_min[2], nbins[2];
  uint32_t *cnt[2], *first[2];
  uint32_t *part;          // histogram: per-workgroup bins [gridDim.x][2][nbins[0] + nbins[1]]; null: global atomics
  const uint64_t *cbits[2];
  const uint8_t *clen[2];
  uint32_t *out[2];
  int64_t out_words[2];
  int64_t *bits[2];        // per record: its bit size (pass A), then its first bit (the scan)
  int64_t *d_nbits;        // [2]
};
// Where a kernel's job comes from (its template parameter Src; blockIdx.y = the
// channel): one image's up to three jobs by value in the kernel arguments, or a
// batch's 3 n jobs in a table in device memory (hic_huffman_batch_*).  The table
// is complete before the launch and is read through a constant-address-space
// reference: the workgroup-uniform reads become scalar loads, and the pointers
// they yield are known to be global ones.  The kernel bodies are the same.
struct HsJobs {
  HsJob j[3];
  int n, M;
  __device__ const HsJob &job(int y) const { return j[y]; }
};
typedef const __attribute__((address_space(4))) HsJob HsJobC;
struct HsTable {
  const HsJob *tab;
  int M;
  __device__ HsJobC &job(int y) const { return *(HsJobC *)(uintptr_t)(tab + y); }
};
static_assert(kSlotCapMax <= kHTile, "a slot fits one pack tile");

// record r: its slot symbols n, those plus the EOB ne, its fillers and stream offset
template <class JT>
__device__ __forceinline__ void hs_record(JT &J, int64_t r, int &n, int &ne, int &nf, int64_t &off) {
  const int4 ix = *reinterpret_cast<const int4 *>(J.sidx + 4 * r);
  n = ix.x;
  nf = ix.w;
  off = J.offs[2 * r];
  ne = n + ((r == J.nrec - 1 && *J.d_count == off + nf + n + 1) ? 1 : 0);
}

// the keys of symbols 16 c .. 16 c + 15 of record r in stream S (16-byte loads; the
// EOB's key is 0); returns how many of them exist (0..16)
template <int S, class JT>
__device__ __forceinline__ int hs_keys16(JT &J, int64_t r, int c, int n, int ne, int (&key)[16]) {
  const int m = ne - 16 * c < 16 ? ne - 16 * c : 16;
  if (m <= 0) return 0;
  if (S == 0) {
    const uint4 q = reinterpret_cast<const uint4 *>(J.slot_len + r * J.capr)[c];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) key[k] = (int)((w[k >> 2] >> (8 * (k & 3))) & 0xFFu);
  } else {
    const uint4 *p = reinterpret_cast<const uint4 *>(J.slot_val + r * J.capr) + 2 * c;
    const uint4 q0 = p[0], q1 = p[1];
    const uint32_t w[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) key[k] = (int)(int16_t)(w[k >> 1] >> (16 * (k & 1)));
  }
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (16 * c + k >= n) key[k] = 0;
  return m;
}

// d_minmax[4 y .. 4 y + 3] = channel y's {min, max} of the lengths, of the values
template <class Src>
__global__ __launch_bounds__(kHT) void k_slot_range(Src jobs, int *__restrict__ mm) {
  __shared__ int s_r[4][kHT / 64];
  auto &J = jobs.job(blockIdx.y);
  const int64_t a = J.nrec * blockIdx.x / gridDim.x, b = J.nrec * (blockIdx.x + 1) / gridDim.x;
  int v[4] = {2147483647, -2147483647 - 1, 2147483647, -2147483647 - 1};
  auto see = [&](int s, int k) {
    v[2 * s] = k < v[2 * s] ? k : v[2 * s];
    v[2 * s + 1] = k > v[2 * s + 1] ? k : v[2 * s + 1];
  };
  for (int64_t r = a; r < b; ++r) {
    int n, ne, nf;
    int64_t off;
    hs_record(J, r, n, ne, nf, off);
    if (nf > 0) {
      see(0, jobs.M - 1);
      see(1, 0);
    }
    for (int c = threadIdx.x; 16 * c < ne; c += kHT) {
      int key[16];
      int m = hs_keys16<0>(J, r, c, n, ne, key);
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < m) see(0, key[k]);
      m = hs_keys16<1>(J, r, c, n, ne, key);
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < m) see(1, key[k]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const int o = __shfl_xor(v[i], d, 64);
      v[i] = (i & 1) ? (o > v[i] ? o : v[i]) : (o < v[i] ? o : v[i]);
    }
    if ((threadIdx.x & 63) == 0) s_r[i][threadIdx.x >> 6] = v[i];
  }
  __syncthreads();
  if (threadIdx.x < 4) {  // one atomic per workgroup and value (k_key_range)
    const int i = threadIdx.x;
    int x = s_r[i][0];
    for (int w = 1; w < kHT / 64; ++w) x = (i & 1) ? (s_r[i][w] > x ? s_r[i][w] : x) : (s_r[i][w] < x ? s_r[i][w] : x);
    if (i & 1)
      atomicMax(mm + 4 * blockIdx.y + i, x);
    else
      atomicMin(mm + 4 * blockIdx.y + i, x);
  }
}

// per bin the count and the first position in the virtual stream.  LDS bins (the
// channel's lengths then its values, <= kHistLds together) stored per workgroup to J.part for
// k_slot_hist_reduce, as k_key_hist does; a channel whose bins exceed the LDS
// (J.part null) adds into the zero / 0xFFFFFFFF initialised outputs.
template <class Src>
__global__ __launch_bounds__(kHT) void k_slot_hist(Src jobs) {
  __shared__ uint32_t s_cnt[kHistLds], s_first[kHistLds];
  auto &J = jobs.job(blockIdx.y);
  const bool lds = J.part != nullptr;
  const int nb0 = J.nbins[0], nbt = nb0 + J.nbins[1];
  if (lds) {
    for (int b = threadIdx.x; b < nbt; b += kHT) {
      s_cnt[b] = 0;
      s_first[b] = 0xFFFFFFFFu;
    }
    __syncthreads();
  }
  auto add = [&](int s, int key, uint32_t c, uint32_t pos) {
    const int b = key - J.key_min[s];
    if ((unsigned)b >= (unsigned)J.nbins[s]) return;  // outside the caller's range: not counted
    if (lds) {
      const int x = s ? nb0 + b : b;
      atomicAdd(&s_cnt[x], c);
      if (pos < s_first[x]) atomicMin(&s_first[x], pos);
    } else {
      atomicAdd(&J.cnt[s][b], c);
      atomicMin(&J.first[s][b], pos);
    }
  };
  const int64_t a = J.nrec * blockIdx.x / gridDim.x, e = J.nrec * (blockIdx.x + 1) / gridDim.x;
  for (int64_t r = a; r < e; ++r) {
    int n, ne, nf;
    int64_t off;
    hs_record(J, r, n, ne, nf, off);
    if (nf > 0 && threadIdx.x == 0) {  // the filler run: nf of one key, first at the record's offset
      add(0, jobs.M - 1, (uint32_t)nf, (uint32_t)off);
      add(1, 0, (uint32_t)nf, (uint32_t)off);
    }
    for (int c = threadIdx.x; 16 * c < ne; c += kHT) {
      const uint32_t p0 = (uint32_t)(off + nf + 16 * c);
      int key[16];
      int m = hs_keys16<0>(J, r, c, n, ne, key);
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < m) add(0, key[k], 1u, p0 + k);
      m = hs_keys16<1>(J, r, c, n, ne, key);
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < m) add(1, key[k], 1u, p0 + k);
    }
  }
  if (lds) {
    __syncthreads();
    uint32_t *pc = J.part + (int64_t)blockIdx.x * 2 * nbt;
    for (int b = threadIdx.x; b < nbt; b += kHT) {
      pc[b] = s_cnt[b];
      pc[nbt + b] = s_first[b];
    }
  }
}

// the sum / min of a channel's nwg partial bins into its two streams' outputs
template <class Src>
__global__ __launch_bounds__(kHT) void k_slot_hist_reduce(Src jobs, int nwg) {
  auto &J = jobs.job(blockIdx.y);
  const int nb0 = J.nbins[0], nbt = nb0 + J.nbins[1];
  const int b = blockIdx.x * kHT + threadIdx.x;
  if (!J.part || b >= nbt) return;
  uint32_t c = 0, f = 0xFFFFFFFFu;
  for (int w = 0; w < nwg; ++w) {
    const uint32_t *pc = J.part + (int64_t)w * 2 * nbt;
    c += pc[b];
    f = pc[nbt + b] < f ? pc[nbt + b] : f;
  }
  const int s = b >= nb0, x = s ? b - nb0 : b;
  J.cnt[s][x] = c;
  J.first[s][x] = f;
}

// a stream's filler code: (length, bits) of key `key`; length 0 outside the table
template <class JT>
__device__ __forceinline__ int hs_fill_code(JT &J, int s, int key, uint64_t &bits) {
  const int b = key - J.key_min[s];
  if ((unsigned)b >= (unsigned)J.nbins[s]) return 0;
  bits = J.cbits[s][b];
  return J.clen[s][b];
}

// the 16 table indices (-1: codes to nothing) of thread t's symbols of record r
template <int S, class JT>
__device__ __forceinline__ void hs_index16(JT &J, int64_t r, int n, int ne, int (&ks)[kHPT]) {
  static_assert(kHPT == 16, "one 16-byte chunk of lengths per thread");
  const int m = hs_keys16<S>(J, r, threadIdx.x, n, ne, ks);
#pragma unroll
  for (int k = 0; k < kHPT; ++k) {
    const int b = ks[k] - J.key_min[S];
    ks[k] = (k < m && (unsigned)b < (unsigned)J.nbins[S]) ? b : -1;
  }
}

// pack pass A: one workgroup per record: the bits of its fillers + its symbols, both streams
template <class Src>
__global__ __launch_bounds__(kHT) void k_slot_pack_sizes(Src jobs) {
  __shared__ int64_t s_w[kHT / 64];
  auto &J = jobs.job(blockIdx.y);
  const int64_t r = blockIdx.x;
  if (r >= J.nrec) return;
  int n, ne, nf;
  int64_t off;
  hs_record(J, r, n, ne, nf, off);
  int ks[kHPT];
  uint32_t a0 = 0, a1 = 0;  // <= 4032 x 64 bits each
  hs_index16<0>(J, r, n, ne, ks);
#pragma unroll
  for (int k = 0; k < kHPT; ++k) a0 += ks[k] >= 0 ? J.clen[0][ks[k]] : 0;
  hs_index16<1>(J, r, n, ne, ks);
#pragma unroll
  for (int k = 0; k < kHPT; ++k) a1 += ks[k] >= 0 ? J.clen[1][ks[k]] : 0;
  int64_t total;
  blk_excl_sum((int64_t)a0 | ((int64_t)a1 << 32), s_w, total);
  if (threadIdx.x == 0) {
    uint64_t c;
    J.bits[0][r] = (int64_t)nf * hs_fill_code(J, 0, jobs.M - 1, c) + (total & 0xFFFFFFFFll);
    J.bits[1][r] = (int64_t)nf * hs_fill_code(J, 1, 0, c) + (total >> 32);
  }
}

// the records' first bits: one workgroup per stream
template <class Src>
__global__ __launch_bounds__(kHT) void k_slot_pack_scan(Src jobs) {
  auto &J = jobs.job(blockIdx.y);
  scan_in_place(J.bits[blockIdx.x], J.nrec, J.d_nbits + blockIdx.x);
}

// pack pass B: one workgroup per record packs its slot's symbols (after its fillers'
// bits, which k_slot_pack_fill writes) as one tile of each stream
template <class Src>
__global__ __launch_bounds__(kHT) void k_slot_pack_bits(Src jobs) {
  extern __shared__ uint32_t s_words[];
  __shared__ int64_t s_w[kHT / 64];
  auto &J = jobs.job(blockIdx.y);
  const int64_t r = blockIdx.x;
  if (r >= J.nrec) return;
  int n, ne, nf;
  int64_t off;
  hs_record(J, r, n, ne, nf, off);
  if (ne == 0) return;
  int ks[kHPT];
  uint64_t c;
  hs_index16<0>(J, r, n, ne, ks);
  pack_tile(ks, J.cbits[0], J.clen[0], J.bits[0][r] + (int64_t)nf * hs_fill_code(J, 0, jobs.M - 1, c), J.out[0],
            J.out_words[0], s_words, s_w);
  hs_index16<1>(J, r, n, ne, ks);
  pack_tile(ks, J.cbits[1], J.clen[1], J.bits[1][r] + (int64_t)nf * hs_fill_code(J, 1, 0, c), J.out[1],
            J.out_words[1], s_words, s_w);
}

// word i of a filler run: nbits bits from bit F0 of the stream, the code (c, clen)
// repeated.  Words the run covers whole are stored, its edge words OR-ed in.
__device__ __forceinline__ void hs_fill_word(uint32_t *__restrict__ out, int64_t out_words, int64_t F0, int64_t nbits,
                                             uint64_t c, int clen, int64_t i) {
  const int64_t w = (F0 >> 5) + i;
  if (w >= out_words) return;
  const int64_t q0 = (w << 5) - F0;  // the run offset of the word's first bit (< 0 in the first word)
  const int64_t end = q0 + 32 < nbits ? q0 + 32 : nbits;
  int64_t q = q0 > 0 ? q0 : 0;
  int ph = (int)(q % clen);  // bits of the current code already behind q
  uint32_t v = 0;
  while (q < end) {
    int take = clen - ph;
    if (take > end - q) take = (int)(end - q);  // <= 32
    const uint32_t piece = (uint32_t)((c >> (clen - ph - take)) & (take == 32 ? 0xFFFFFFFFull : ((1ull << take) - 1)));
    v |= piece << (32 - (int)(q - q0) - take);
    q += take;
    ph = 0;
  }
  v = bswap32(v);
  if (q0 < 0 || q0 + 32 > nbits) {
    if (v) atomicOr(&out[w], v);
  } else {
    out[w] = v;
  }
}

// the filler runs' bits.  Every workgroup of a channel walks its records' nfill in
// batches of kHT; a short run (<= kFillShort words) is written by its thread in the
// batch's own workgroup (batches dealt round-robin), a long one -- a carried zero run
// can span nearly the whole channel -- word by word by ALL the channel's workgroups.
constexpr int kFillShort = 16;
template <class Src>
__global__ __launch_bounds__(kHT) void k_slot_pack_fill(Src jobs) {
  __shared__ int s_list[2 * kHT];
  __shared__ int s_nlist;
  auto &J = jobs.job(blockIdx.y);
  uint64_t fc[2] = {0, 0};
  const int fl[2] = {hs_fill_code(J, 0, jobs.M - 1, fc[0]), hs_fill_code(J, 1, 0, fc[1])};
  if (fl[0] == 0 && fl[1] == 0) return;  // no filler in the tables: no run
  for (int64_t r0 = 0, bt = 0; r0 < J.nrec; r0 += kHT, ++bt) {
    if (threadIdx.x == 0) s_nlist = 0;
    __syncthreads();
    const int64_t r = r0 + threadIdx.x;
    const int nf = r < J.nrec ? J.sidx[4 * r + 3] : 0;
    if (nf > 0) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (fl[s] == 0) continue;
        const int64_t F0 = J.bits[s][r], nbits = (int64_t)nf * fl[s];
        const int64_t nw = ((F0 + nbits + 31) >> 5) - (F0 >> 5);
        if (nw > kFillShort)
          s_list[atomicAdd(&s_nlist, 1)] = 2 * threadIdx.x + s;
        else if (bt % gridDim.x == blockIdx.x)
          for (int64_t i = 0; i < nw; ++i) hs_fill_word(J.out[s], J.out_words[s], F0, nbits, fc[s], fl[s], i);
      }
    }
    __syncthreads();
    const int nl = s_nlist;
    for (int e = 0; e < nl; ++e) {
      const int s = s_list[e] & 1;
      const int64_t rr = r0 + (s_list[e] >> 1);
      const int64_t F0 = J.bits[s][rr], nbits = (int64_t)J.sidx[4 * rr + 3] * fl[s];
      const int64_t nw = ((F0 + nbits + 31) >> 5) - (F0 >> 5);
      for (int64_t i = (int64_t)blockIdx.x * kHT + threadIdx.x; i < nw; i += (int64_t)gridDim.x * kHT)
        hs_fill_word(J.out[s], J.out_words[s], F0, nbits, fc[s], fl[s], i);
    }
    __syncthreads();
  }
}

}  // namespace
}  // namespace hic

using namespace hic;

extern "C" int hic_key_range(const void *keys, int key_bytes, int64_t n, int32_t *d_minmax, void *stream) {
  if (!keys || !d_minmax) return arg_error("null pointer");
  if (key_bytes != 1 && key_bytes != 2 && key_bytes != 4) return arg_error("key_bytes must be 1, 2 or 4");
  if (n <= 0) return arg_error("n");
  hipStream_t s = as_stream(stream);
  const int32_t init[2] = {2147483647, -2147483647 - 1};
  if (int e = hip_status(hipMemcpyAsync(d_minmax, init, sizeof init, hipMemcpyHostToDevice, s), "hipMemcpyAsync"))
    return e;
  const bool vec = reinterpret_cast<uintptr_t>(keys) % 16 == 0;
  const int per = vec ? 16 / key_bytes : 1;
  const int64_t want = (n + (int64_t)per * kHT - 1) / ((int64_t)per * kHT);
  const int grid = (int)(want < cu_count() ? want : cu_count());
  if (vec && key_bytes == 4)
    hipLaunchKernelGGL((k_key_range<4, true>), dim3(grid), dim3(kHT), 0, s, keys, n, d_minmax);
  else if (vec && key_bytes == 2)
    hipLaunchKernelGGL((k_key_range<2, true>), dim3(grid), dim3(kHT), 0, s, keys, n, d_minmax);
  else if (vec)
    hipLaunchKernelGGL((k_key_range<1, true>), dim3(grid), dim3(kHT), 0, s, keys, n, d_minmax);
  else if (key_bytes == 4)
    hipLaunchKernelGGL((k_key_range<4, false>), dim3(grid), dim3(kHT), 0, s, keys, n, d_minmax);
  else if (key_bytes == 2)
    hipLaunchKernelGGL((k_key_range<2, false>), dim3(grid), dim3(kHT), 0, s, keys, n, d_minmax);
  else
    hipLaunchKernelGGL((k_key_range<1, false>), dim3(grid), dim3(kHT), 0, s, keys, n, d_minmax);
  return check_launch("k_key_range");
}

extern "C" int hic_key_histogram(const void *keys, int key_bytes, int64_t n, int32_t key_min, int32_t nbins,
                                 uint32_t *d_counts, uint32_t *d_first, void *stream) {
  if (!keys || !d_counts || !d_first) return arg_error("null pointer");
  if (key_bytes != 1 && key_bytes != 2 && key_bytes != 4) return arg_error("key_bytes must be 1, 2 or 4");
  if (n <= 0 || n >= ((int64_t)1 << 32)) return arg_error("n");
  if (nbins < 1 || nbins > (1 << 24)) return arg_error("nbins");
  hipStream_t s = as_stream(stream);
  if (int e = hip_status(hipMemsetAsync(d_counts, 0, (size_t)nbins * 4, s), "hipMemsetAsync")) return e;
  if (int e = hip_status(hipMemsetAsync(d_first, 0xFF, (size_t)nbins * 4, s), "hipMemsetAsync")) return e;
  const int64_t want = (n + kHT * 8 - 1) / (kHT * 8);
  const int grid = (int)(want < 2 * cu_count() ? want : 2 * cu_count());
  if (nbins <= kHistLds && grid > 1) {
    // two phases: per-workgroup bins to a stream-ordered scratch, then one reduction
    void *part = nullptr;
    if (int e = hip_status(hipMallocAsync(&part, (size_t)grid * 2 * nbins * 4, s), "hipMallocAsync")) return e;
    hipLaunchKernelGGL(k_key_hist<true>, dim3(grid), dim3(kHT), 0, s, keys, key_bytes, n, key_min, nbins, d_counts,
                       d_first, static_cast<uint32_t *>(part));
    if (int e = check_launch("k_key_hist")) return e;
    hipLaunchKernelGGL(k_hist_reduce, dim3((unsigned)((nbins + kHT - 1) / kHT)), dim3(kHT), 0, s,
                       static_cast<const uint32_t *>(part), grid, nbins, d_counts, d_first);
    if (int e = check_launch("k_hist_reduce")) return e;
    return hip_status(hipFreeAsync(part, s), "hipFreeAsync");
  }
  if (nbins <= kHistLds)
    hipLaunchKernelGGL(k_key_hist<true>, dim3(grid), dim3(kHT), 0, s, keys, key_bytes, n, key_min, nbins, d_counts,
                       d_first);
  else
    hipLaunchKernelGGL(k_key_hist<false>, dim3(grid), dim3(kHT), 0, s, keys, key_bytes, n, key_min, nbins, d_counts,
                       d_first);
  return check_launch("k_key_hist");
}

extern "C" size_t hic_huffman_pack_workspace_bytes(int64_t n) {
  return (size_t)((n + kHTile - 1) / kHTile + 8) * sizeof(int64_t);
}

extern "C" int hic_huffman_pack(const void *keys, int key_bytes, int64_t n, int32_t key_min, int32_t nbins,
                                const uint64_t *d_code_bits, const uint8_t *d_code_len, uint8_t *out,
                                int64_t out_bytes, int64_t *d_nbits, void *workspace, void *stream) {
  if (!keys || !d_code_bits || !d_code_len || !out || !d_nbits || !workspace) return arg_error("null pointer");
  if (key_bytes != 1 && key_bytes != 2 && key_bytes != 4) return arg_error("key_bytes must be 1, 2 or 4");
  if (n <= 0) return arg_error("n");
  if (nbins < 1) return arg_error("nbins");
  if (reinterpret_cast<uintptr_t>(out) % 4 || out_bytes % 4 || out_bytes <= 0)
    return arg_error("out must be 4-byte aligned and sized");
  hipStream_t s = as_stream(stream);
  const int64_t nt = (n + kHTile - 1) / kHTile;
  int64_t *tile = static_cast<int64_t *>(workspace);
  if (int e = hip_status(hipMemsetAsync(out, 0, (size_t)out_bytes, s), "hipMemsetAsync")) return e;
  hipLaunchKernelGGL(k_pack_sizes, dim3((unsigned)nt), dim3(kHT), 0, s, keys, key_bytes, n, key_min, nbins,
                     d_code_len, tile);
  hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(kHT), 0, s, tile, nt, d_nbits);
  hipLaunchKernelGGL(k_pack_bits, dim3((unsigned)nt), dim3(kHT), kPackWords * sizeof(uint32_t), s, keys, key_bytes,
                     n, key_min, nbins, d_code_bits, d_code_len, tile, reinterpret_cast<uint32_t *>(out),
                     out_bytes / 4);
  return check_launch("k_pack_bits");
}

// ---- the slot layout's streams (the kernels' comment above) ----
// hic_slot_job[n] -> the kernels' jobs; everything is checked before any device call
static int hs_job_one(int k, const hic_slot_job &a, HsJob &j);
static int hs_jobs(int n, const hic_slot_job *jobs, int max_len, HsJobs &J, int64_t &max_nrec) {
  if (n < 1 || n > 3 || !jobs) return arg_error("1 <= n <= 3 jobs");
  if (max_len != 15) return arg_error("the slot layout needs max_len 15");
  J = HsJobs{};
  J.n = n;
  J.M = max_len;
  max_nrec = 0;
  for (int k = 0; k < n; ++k) {
    if (int e = hs_job_one(k, jobs[k], J.j[k])) return e;
    max_nrec = J.j[k].nrec > max_nrec ? J.j[k].nrec : max_nrec;
  }
  return HIC_OK;
}
// job k of an entry point: its checks, and the fields every phase reads
static int hs_job_one(int k, const hic_slot_job &a, HsJob &j) {
  if (!a.slot_len || !a.slot_val || !a.d_index || !a.workspace || !a.d_count) return arg_error("job %d: null pointer", k);
  // (a stream holds at most nblk * 63 + 1 symbols: positions fit 32 bits)
  if (a.nblk <= 0 || a.nblk > (int64_t)INT32_MAX / 63) return arg_error("job %d: nblk", k);
  if (a.records_per_tile != 1 && a.records_per_tile != 2) return arg_error("job %d: records_per_tile must be 1 or 2", k);
  const int64_t bpr = 64 / a.records_per_tile;
  if (a.nblk % bpr) return arg_error("job %d: nblk must be a multiple of %lld (whole records)", k, (long long)bpr);
  if ((reinterpret_cast<uintptr_t>(a.slot_len) | reinterpret_cast<uintptr_t>(a.slot_val) |
       reinterpret_cast<uintptr_t>(a.d_index)) % 16)
    return arg_error("job %d: slot arrays and index must be 16-byte aligned", k);
  if (a.workspace_bytes < (int64_t)hic_rle_slots_workspace_bytes(a.nblk, (int)a.records_per_tile))
    return arg_error("job %d: workspace too small", k);
  j.slot_len = a.slot_len;
  j.slot_val = a.slot_val;
  j.sidx = a.d_index;
  j.nrec = slot_nrec(a.nblk, a.records_per_tile);
  j.offs = static_cast<const int64_t *>(a.workspace) + rle_offs_word(j.nrec);
  j.d_count = a.d_count;
  j.capr = (int)(63 * bpr);
  return HIC_OK;
}

// hipMemsetAsync of m <= 6 regions, in address order with touching neighbours merged
// into one call (the six AC streams' outputs of one image are one block)
static int memset_regions(int m, uint8_t *const *p, const int64_t *bytes, int value, hipStream_t s) {
  int idx[6];
  for (int i = 0; i < m; ++i) {
    int k = i;
    for (; k > 0 && p[idx[k - 1]] > p[i]; --k) idx[k] = idx[k - 1];
    idx[k] = i;
  }
  for (int i = 0; i < m;) {
    uint8_t *base = p[idx[i]];
    int64_t len = bytes[idx[i]];
    for (++i; i < m && p[idx[i]] == base + len; ++i) len += bytes[idx[i]];
    if (int st = hip_status(hipMemsetAsync(base, value, (size_t)len, s), "hipMemsetAsync")) return st;
  }
  return HIC_OK;
}

extern "C" int hic_slot_key_range(int n, const hic_slot_job *jobs, int max_len, int32_t *d_minmax, void *stream) {
  HsJobs J;
  int64_t max_nrec;
  if (int e = hs_jobs(n, jobs, max_len, J, max_nrec)) return e;
  if (!d_minmax) return arg_error("null pointer");
  hipStream_t s = as_stream(stream);
  int32_t init[12];
  for (int i = 0; i < 4 * n; ++i) init[i] = (i & 1) ? -2147483647 - 1 : 2147483647;
  if (int e = hip_status(hipMemcpyAsync(d_minmax, init, sizeof(int32_t) * 4 * n, hipMemcpyHostToDevice, s),
                         "hipMemcpyAsync"))
    return e;
  const int64_t want = (max_nrec + 7) / 8;
  const int grid = (int)(want < cu_count() ? want : cu_count());
  hipLaunchKernelGGL(k_slot_range<HsJobs>, dim3(grid, n), dim3(kHT), 0, s, J, d_minmax);
  return check_launch("k_slot_range");
}

// key_min / nbins of the 2 n streams into the jobs
static int hs_tables(HsJobs &J, const int32_t *key_min, const int32_t *nbins) {
  if (!key_min || !nbins) return arg_error("null pointer");
  for (int i = 0; i < 2 * J.n; ++i) {
    if (nbins[i] < 1 || nbins[i] > (1 << 24)) return arg_error("stream %d: nbins", i);
    J.j[i / 2].key_min[i & 1] = key_min[i];
    J.j[i / 2].nbins[i & 1] = nbins[i];
  }
  return HIC_OK;
}

extern "C" int hic_slot_key_histogram(int n, const hic_slot_job *jobs, int max_len, const int32_t *key_min,
                                      const int32_t *nbins, uint32_t *d_counts, uint32_t *d_first,
                                      const int64_t *bin_offsets, void *stream) {
  HsJobs J;
  int64_t max_nrec;
  if (int e = hs_jobs(n, jobs, max_len, J, max_nrec)) return e;
  if (int e = hs_tables(J, key_min, nbins)) return e;
  if (!d_counts || !d_first || !bin_offsets) return arg_error("null pointer");
  uint8_t *pc[6], *pf[6];
  int64_t bytes[6];
  for (int i = 0; i < 2 * n; ++i) {
    if (bin_offsets[i] < 0) return arg_error("stream %d: bin offset", i);
    J.j[i / 2].cnt[i & 1] = d_counts + bin_offsets[i];
    J.j[i / 2].first[i & 1] = d_first + bin_offsets[i];
    pc[i] = reinterpret_cast<uint8_t *>(d_counts + bin_offsets[i]);
    pf[i] = reinterpret_cast<uint8_t *>(d_first + bin_offsets[i]);
    bytes[i] = (int64_t)nbins[i] * 4;
  }
  hipStream_t s = as_stream(stream);
  if (int e = memset_regions(2 * n, pc, bytes, 0, s)) return e;
  if (int e = memset_regions(2 * n, pf, bytes, 0xFF, s)) return e;
  const int64_t want = (max_nrec + 7) / 8;
  const int grid = (int)(want < cu_count() ? want : cu_count());
  // per-workgroup bins of the channels that fit the LDS, in one stream-ordered scratch
  int64_t words = 0, max_nbt = 0;
  for (int k = 0; k < n; ++k) {
    const int64_t nbt = (int64_t)J.j[k].nbins[0] + J.j[k].nbins[1];
    if (nbt > kHistLds) continue;
    words += (int64_t)grid * 2 * nbt;
    max_nbt = nbt > max_nbt ? nbt : max_nbt;
  }
  void *part = nullptr;
  if (words) {
    if (int e = hip_status(hipMallocAsync(&part, (size_t)words * 4, s), "hipMallocAsync")) return e;
    uint32_t *p = static_cast<uint32_t *>(part);
    for (int k = 0; k < n; ++k) {
      const int64_t nbt = (int64_t)J.j[k].nbins[0] + J.j[k].nbins[1];
      if (nbt > kHistLds) continue;
      J.j[k].part = p;
      p += (int64_t)grid * 2 * nbt;
    }
  }
  hipLaunchKernelGGL(k_slot_hist<HsJobs>, dim3(grid, n), dim3(kHT), 0, s, J);
  if (int e = check_launch("k_slot_hist")) return e;
  if (!words) return HIC_OK;
  hipLaunchKernelGGL(k_slot_hist_reduce<HsJobs>, dim3((unsigned)((max_nbt + kHT - 1) / kHT), n), dim3(kHT), 0, s, J, grid);
  if (int e = check_launch("k_slot_hist_reduce")) return e;
  return hip_status(hipFreeAsync(part, s), "hipFreeAsync");
}

extern "C" size_t hic_slot_huffman_pack_workspace_bytes(int n, const hic_slot_job *jobs) {
  int64_t words = 8;
  for (int k = 0; jobs && k < n && k < 3; ++k)
    words += 2 * slot_nrec(jobs[k].nblk > 0 ? jobs[k].nblk : 1, jobs[k].records_per_tile == 2 ? 2 : 1);
  return (size_t)words * sizeof(int64_t);
}

extern "C" int hic_slot_huffman_pack(int n, const hic_slot_job *jobs, int max_len, const int32_t *key_min,
                                     const int32_t *nbins, const uint64_t *const *h_code_bits,
                                     const uint8_t *const *h_code_len, uint8_t *const *h_out,
                                     const int64_t *out_bytes, int64_t *d_nbits, void *workspace, void *stream) {
  HsJobs J;
  int64_t max_nrec;
  if (int e = hs_jobs(n, jobs, max_len, J, max_nrec)) return e;
  if (int e = hs_tables(J, key_min, nbins)) return e;
  if (!h_code_bits || !h_code_len || !h_out || !out_bytes || !d_nbits || !workspace) return arg_error("null pointer");
  int64_t *ws = static_cast<int64_t *>(workspace);
  for (int i = 0; i < 2 * n; ++i) {
    if (!h_code_bits[i] || !h_code_len[i] || !h_out[i]) return arg_error("stream %d: null pointer", i);
    if (reinterpret_cast<uintptr_t>(h_out[i]) % 4 || out_bytes[i] % 4 || out_bytes[i] <= 0)
      return arg_error("stream %d: out must be 4-byte aligned and sized", i);
    HsJob &j = J.j[i / 2];
    j.cbits[i & 1] = h_code_bits[i];
    j.clen[i & 1] = h_code_len[i];
    j.out[i & 1] = reinterpret_cast<uint32_t *>(h_out[i]);
    j.out_words[i & 1] = out_bytes[i] / 4;
    j.bits[i & 1] = ws;
    ws += j.nrec;
    j.d_nbits = d_nbits + (i & ~1);
  }
  hipStream_t s = as_stream(stream);
  if (int e = memset_regions(2 * n, h_out, out_bytes, 0, s)) return e;
  hipLaunchKernelGGL(k_slot_pack_sizes<HsJobs>, dim3((unsigned)max_nrec, n), dim3(kHT), 0, s, J);
  hipLaunchKernelGGL(k_slot_pack_scan<HsJobs>, dim3(2, n), dim3(kHT), 0, s, J);
  hipLaunchKernelGGL(k_slot_pack_bits<HsJobs>, dim3((unsigned)max_nrec, n), dim3(kHT), kPackWords * sizeof(uint32_t), s, J);
  const int64_t batches = (max_nrec + kHT - 1) / kHT;
  const int fgrid = (int)(batches * 8 < cu_count() ? batches * 8 : cu_count());
  hipLaunchKernelGGL(k_slot_pack_fill<HsJobs>, dim3(fgrid, n), dim3(kHT), 0, s, J);
  return check_launch("k_slot_pack_fill");
}

// ---- the batch's 9 n streams, one pass per phase (hic_huffman_batch_*) ----
// Stream order of every per-stream array: the 3 n DC streams (image i's Y, Cr, Cb =
// 3 i .. 3 i + 2), then the 6 n slot streams (channel c = 3 i + k gives 3 n + 2 c,
// its lengths, and 3 n + 2 c + 1, its values).  Bins and outputs lie back to back in
// that order, so one memset covers each kind.  The jobs of a phase are written into
// two host tables, copied into the caller's workspace, and read there by the kernels.
namespace {

constexpr int kHbGrid = 256;  // the range / histogram grids' x per channel at most (an MI355X's compute units)

struct HbPlan {
  int n = 0;
  std::vector<HsJob> sj;  // 3 n
  std::vector<HkJob> kj;  // 3 n
  int64_t max_nrec = 0, max_keys = 0;
  int sgrid() const {  // workgroups per slot channel of the range and the histogram
    const int64_t want = (max_nrec + 7) / 8;
    return (int)(want < kHbGrid ? want : kHbGrid);
  }
};

size_t hb_table_bytes(int n) {
  return (size_t)(round_up(3 * (int64_t)n * sizeof(HsJob), 16) + round_up(3 * (int64_t)n * sizeof(HkJob), 16));
}

// every job checked, nothing launched
int hb_plan(int n, const hic_slot_job *jobs, const hic_key_stream *dc, int max_len, HbPlan &P) {
  if (n < 1 || n > HIC_SLOTS_BATCH_MAX) return arg_error("1 <= n <= HIC_SLOTS_BATCH_MAX images");
  if (!jobs || !dc) return arg_error("null pointer");
  if (max_len != 15) return arg_error("the slot layout needs max_len 15");
  P.n = n;
  P.sj.assign(3 * (size_t)n, HsJob{});
  P.kj.assign(3 * (size_t)n, HkJob{});
  for (int k = 0; k < 3 * n; ++k) {
    if (int e = hs_job_one(k, jobs[k], P.sj[k])) return e;
    P.max_nrec = P.sj[k].nrec > P.max_nrec ? P.sj[k].nrec : P.max_nrec;
    if (!dc[k].keys) return arg_error("DC stream %d: null pointer", k);
    if (reinterpret_cast<uintptr_t>(dc[k].keys) % 16) return arg_error("DC stream %d: keys must be 16-byte aligned", k);
    if (dc[k].n <= 0 || dc[k].n > INT32_MAX) return arg_error("DC stream %d: n", k);
    P.kj[k].keys = dc[k].keys;
    P.kj[k].n = dc[k].n;
    P.max_keys = dc[k].n > P.max_keys ? dc[k].n : P.max_keys;
  }
  // (a grid holds fewer than 2^32 threads)
  const int64_t wide = P.max_nrec > (P.max_keys + kHTile - 1) / kHTile ? P.max_nrec : (P.max_keys + kHTile - 1) / kHTile;
  if (wide * 3 * n > ((int64_t)1 << 32) / kHT - 1) return arg_error("the batch's records exceed one grid");
  return HIC_OK;
}

int hb_bins(HbPlan &P, const int32_t *key_min, const int32_t *nbins, int64_t &total) {
  if (!key_min || !nbins) return arg_error("null pointer");
  const int m = 3 * P.n;
  total = 0;
  for (int i = 0; i < 9 * P.n; ++i) {
    if (nbins[i] < 1 || nbins[i] > (1 << 24)) return arg_error("stream %d: nbins", i);
    total += nbins[i];
  }
  for (int i = 0; i < m; ++i) {
    P.kj[i].key_min = key_min[i];
    P.kj[i].nbins = nbins[i];
  }
  for (int i = 0; i < 2 * m; ++i) {
    P.sj[i / 2].key_min[i & 1] = key_min[m + i];
    P.sj[i / 2].nbins[i & 1] = nbins[m + i];
  }
  return HIC_OK;
}

int hb_workspace(const void *workspace, size_t have, size_t need) {
  if (!workspace) return arg_error("null pointer");
  if (reinterpret_cast<uintptr_t>(workspace) % 16) return arg_error("workspace must be 16-byte aligned");
  if (have < need) return arg_error("workspace too small");
  return HIC_OK;
}

// the two tables into the workspace's head: one copy
int hb_upload(const HbPlan &P, void *workspace, std::vector<char> &blob, const HsJob *&d_sj, const HkJob *&d_kj,
              hipStream_t s) {
  const size_t a = (size_t)round_up(P.sj.size() * sizeof(HsJob), 16);
  blob.assign(hb_table_bytes(P.n), 0);
  memcpy(blob.data(), P.sj.data(), P.sj.size() * sizeof(HsJob));
  memcpy(blob.data() + a, P.kj.data(), P.kj.size() * sizeof(HkJob));
  d_sj = static_cast<const HsJob *>(workspace);
  d_kj = reinterpret_cast<const HkJob *>(static_cast<const char *>(workspace) + a);
  return hip_status(hipMemcpyAsync(workspace, blob.data(), blob.size(), hipMemcpyHostToDevice, s), "hipMemcpyAsync");
}

// the histogram's per-workgroup bins behind the tables: `base` null = only the size (uint32 words)
int64_t hb_hist_parts(HbPlan &P, uint32_t *base, int64_t &max_nbt, int &max_nwg, int64_t &max_part_bins) {
  int64_t words = 0;
  max_nbt = 0, max_nwg = 1, max_part_bins = 0;
  const int g = P.sgrid();
  for (auto &j : P.sj) {
    const int64_t nbt = (int64_t)j.nbins[0] + j.nbins[1];
    j.part = nullptr;
    if (nbt > kHistLds) continue;  // the channel adds into its outputs with global atomics
    j.part = base ? base + words : reinterpret_cast<uint32_t *>(16);
    words += (int64_t)g * 2 * nbt;
    max_nbt = nbt > max_nbt ? nbt : max_nbt;
  }
  for (auto &j : P.kj) {
    const int64_t want = (j.n + kHT * 8 - 1) / (kHT * 8);
    j.nwg = (int)(want < 2 * kHbGrid ? want : 2 * kHbGrid);
    max_nwg = j.nwg > max_nwg ? j.nwg : max_nwg;
    j.part = nullptr;
    if (j.nbins > kHistLds || j.nwg == 1) continue;  // one workgroup's LDS bins go straight to the outputs
    j.part = base ? base + words : reinterpret_cast<uint32_t *>(16);
    words += (int64_t)j.nwg * 2 * j.nbins;
    max_part_bins = j.nbins > max_part_bins ? j.nbins : max_part_bins;
  }
  return words;
}

int64_t hb_pack_words(const HbPlan &P) {
  int64_t words = 8;
  for (auto &j : P.sj) words += 2 * j.nrec;
  for (auto &j : P.kj) words += (j.n + kHTile - 1) / kHTile;
  return words;
}

}  // namespace

extern "C" size_t hic_huffman_batch_key_range_workspace_bytes(int n) {
  return n >= 1 && n <= HIC_SLOTS_BATCH_MAX ? hb_table_bytes(n) : 0;
}

extern "C" int hic_huffman_batch_key_range(int n, const hic_slot_job *jobs, const hic_key_stream *dc, int max_len,
                                           int32_t *d_minmax, void *workspace, size_t workspace_bytes, void *stream) {
  HbPlan P;
  if (int e = hb_plan(n, jobs, dc, max_len, P)) return e;
  if (!d_minmax) return arg_error("null pointer");
  if (int e = hb_workspace(workspace, workspace_bytes, hb_table_bytes(n))) return e;
  hipStream_t s = as_stream(stream);
  std::vector<int32_t> init(18 * (size_t)n);
  for (size_t i = 0; i < init.size(); ++i) init[i] = (i & 1) ? -2147483647 - 1 : 2147483647;
  if (int e = hip_status(hipMemcpyAsync(d_minmax, init.data(), init.size() * 4, hipMemcpyHostToDevice, s),
                         "hipMemcpyAsync"))
    return e;
  std::vector<char> blob;
  const HsJob *d_sj;
  const HkJob *d_kj;
  if (int e = hb_upload(P, workspace, blob, d_sj, d_kj, s)) return e;
  const int64_t want = (P.max_keys + 4 * kHT - 1) / (4 * kHT);
  hipLaunchKernelGGL(k_key_range_table, dim3((unsigned)(want < kHbGrid ? want : kHbGrid), 3 * n), dim3(kHT), 0, s,
                     d_kj, d_minmax);
  if (int e = check_launch("k_key_range_table")) return e;
  hipLaunchKernelGGL(k_slot_range<HsTable>, dim3(P.sgrid(), 3 * n), dim3(kHT), 0, s, HsTable{d_sj, max_len},
                     d_minmax + 6 * n);
  return check_launch("k_slot_range");
}

extern "C" size_t hic_huffman_batch_histogram_workspace_bytes(int n, const hic_slot_job *jobs,
                                                              const hic_key_stream *dc, const int32_t *nbins) {
  HbPlan P;
  int64_t total, a, c;
  int b;
  if (hb_plan(n, jobs, dc, 15, P) || hb_bins(P, nbins, nbins, total)) return 0;
  return hb_table_bytes(n) + (size_t)hb_hist_parts(P, nullptr, a, b, c) * 4;
}

extern "C" int hic_huffman_batch_histogram(int n, const hic_slot_job *jobs, const hic_key_stream *dc, int max_len,
                                           const int32_t *key_min, const int32_t *nbins, uint32_t *d_counts,
                                           uint32_t *d_first, void *workspace, size_t workspace_bytes, void *stream) {
  HbPlan P;
  int64_t total, max_nbt, max_part_bins;
  int max_nwg;
  if (int e = hb_plan(n, jobs, dc, max_len, P)) return e;
  if (int e = hb_bins(P, key_min, nbins, total)) return e;
  if (!d_counts || !d_first) return arg_error("null pointer");
  if ((reinterpret_cast<uintptr_t>(d_counts) | reinterpret_cast<uintptr_t>(d_first)) % 4)
    return arg_error("bins must be 4-byte aligned");
  const size_t tb = hb_table_bytes(n);
  const int64_t words = hb_hist_parts(P, nullptr, max_nbt, max_nwg, max_part_bins);
  if (int e = hb_workspace(workspace, workspace_bytes, tb + (size_t)words * 4)) return e;
  hb_hist_parts(P, reinterpret_cast<uint32_t *>(static_cast<char *>(workspace) + tb), max_nbt, max_nwg, max_part_bins);
  int64_t off = 0;
  for (int i = 0; i < 9 * n; ++i) {
    if (i < 3 * n) {
      P.kj[i].cnt = d_counts + off;
      P.kj[i].first = d_first + off;
    } else {
      P.sj[(i - 3 * n) / 2].cnt[(i - 3 * n) & 1] = d_counts + off;
      P.sj[(i - 3 * n) / 2].first[(i - 3 * n) & 1] = d_first + off;
    }
    off += nbins[i];
  }
  hipStream_t s = as_stream(stream);
  if (int e = hip_status(hipMemsetAsync(d_counts, 0, (size_t)total * 4, s), "hipMemsetAsync")) return e;
  if (int e = hip_status(hipMemsetAsync(d_first, 0xFF, (size_t)total * 4, s), "hipMemsetAsync")) return e;
  std::vector<char> blob;
  const HsJob *d_sj;
  const HkJob *d_kj;
  if (int e = hb_upload(P, workspace, blob, d_sj, d_kj, s)) return e;
  hipLaunchKernelGGL(k_key_hist_table, dim3(max_nwg, 3 * n), dim3(kHT), 0, s, d_kj);
  if (int e = check_launch("k_key_hist_table")) return e;
  if (max_part_bins) {
    hipLaunchKernelGGL(k_hist_reduce_table, dim3((unsigned)((max_part_bins + kHT - 1) / kHT), 3 * n), dim3(kHT), 0, s,
                       d_kj);
    if (int e = check_launch("k_hist_reduce_table")) return e;
  }
  const HsTable T{d_sj, max_len};
  hipLaunchKernelGGL(k_slot_hist<HsTable>, dim3(P.sgrid(), 3 * n), dim3(kHT), 0, s, T);
  if (int e = check_launch("k_slot_hist")) return e;
  if (!max_nbt) return HIC_OK;
  hipLaunchKernelGGL(k_slot_hist_reduce<HsTable>, dim3((unsigned)((max_nbt + kHT - 1) / kHT), 3 * n), dim3(kHT), 0, s,
                     T, P.sgrid());
  return check_launch("k_slot_hist_reduce");
}

extern "C" size_t hic_huffman_batch_pack_workspace_bytes(int n, const hic_slot_job *jobs, const hic_key_stream *dc) {
  HbPlan P;
  if (hb_plan(n, jobs, dc, 15, P)) return 0;
  return hb_table_bytes(n) + (size_t)hb_pack_words(P) * sizeof(int64_t);
}

extern "C" int hic_huffman_batch_pack(int n, const hic_slot_job *jobs, const hic_key_stream *dc, int max_len,
                                      const int32_t *key_min, const int32_t *nbins, const uint64_t *d_code_bits,
                                      const uint8_t *d_code_len, uint8_t *d_out, const int64_t *out_bytes,
                                      int64_t *d_nbits, void *workspace, size_t workspace_bytes, void *stream) {
  HbPlan P;
  int64_t total;
  if (int e = hb_plan(n, jobs, dc, max_len, P)) return e;
  if (int e = hb_bins(P, key_min, nbins, total)) return e;
  if (!d_code_bits || !d_code_len || !d_out || !out_bytes || !d_nbits) return arg_error("null pointer");
  if (reinterpret_cast<uintptr_t>(d_code_bits) % 8 || reinterpret_cast<uintptr_t>(d_nbits) % 8)
    return arg_error("code bits and bit counts must be 8-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_out) % 4) return arg_error("out must be 4-byte aligned and sized");
  const size_t tb = hb_table_bytes(n);
  if (int e = hb_workspace(workspace, workspace_bytes, tb + (size_t)hb_pack_words(P) * sizeof(int64_t))) return e;
  int64_t *ws = reinterpret_cast<int64_t *>(static_cast<char *>(workspace) + tb);
  int64_t bin = 0, byte = 0, max_nt = 1;
  for (int i = 0; i < 9 * n; ++i) {
    if (out_bytes[i] % 4 || out_bytes[i] <= 0) return arg_error("stream %d: out must be 4-byte aligned and sized", i);
    uint32_t *out = reinterpret_cast<uint32_t *>(d_out + byte);
    if (i < 3 * n) {
      HkJob &j = P.kj[i];
      j.cbits = d_code_bits + bin;
      j.clen = d_code_len + bin;
      j.out = out;
      j.out_words = out_bytes[i] / 4;
      j.nt = (int)((j.n + kHTile - 1) / kHTile);
      j.tile = ws;
      ws += j.nt;
      j.d_nbits = d_nbits + i;
      max_nt = j.nt > max_nt ? j.nt : max_nt;
    } else {
      const int c = (i - 3 * n) / 2, w = (i - 3 * n) & 1;
      HsJob &j = P.sj[c];
      j.cbits[w] = d_code_bits + bin;
      j.clen[w] = d_code_len + bin;
      j.out[w] = out;
      j.out_words[w] = out_bytes[i] / 4;
      j.bits[w] = ws;
      ws += j.nrec;
      j.d_nbits = d_nbits + 3 * n + 2 * c;
    }
    bin += nbins[i];
    byte += out_bytes[i];
  }
  hipStream_t s = as_stream(stream);
  if (int e = hip_status(hipMemsetAsync(d_out, 0, (size_t)byte, s), "hipMemsetAsync")) return e;
  std::vector<char> blob;
  const HsJob *d_sj;
  const HkJob *d_kj;
  if (int e = hb_upload(P, workspace, blob, d_sj, d_kj, s)) return e;
  hipLaunchKernelGGL(k_pack_sizes_table, dim3((unsigned)max_nt, 3 * n), dim3(kHT), 0, s, d_kj);
  hipLaunchKernelGGL(k_pack_scan_table, dim3(1, 3 * n), dim3(kHT), 0, s, d_kj);
  hipLaunchKernelGGL(k_pack_bits_table, dim3((unsigned)max_nt, 3 * n), dim3(kHT), kPackWords * sizeof(uint32_t), s,
                     d_kj);
  if (int e = check_launch("k_pack_bits_table")) return e;
  const HsTable T{d_sj, max_len};
  hipLaunchKernelGGL(k_slot_pack_sizes<HsTable>, dim3((unsigned)P.max_nrec, 3 * n), dim3(kHT), 0, s, T);
  hipLaunchKernelGGL(k_slot_pack_scan<HsTable>, dim3(2, 3 * n), dim3(kHT), 0, s, T);
  hipLaunchKernelGGL(k_slot_pack_bits<HsTable>, dim3((unsigned)P.max_nrec, 3 * n), dim3(kHT),
                     kPackWords * sizeof(uint32_t), s, T);
  const int64_t batches = (P.max_nrec + kHT - 1) / kHT;
  hipLaunchKernelGGL(k_slot_pack_fill<HsTable>, dim3((unsigned)(batches * 8 < kHbGrid ? batches * 8 : kHbGrid), 3 * n),
                     dim3(kHT), 0, s, T);
  return check_launch("k_slot_pack_fill");
}
