// huffdec_lut.h -- one entry of the Huffman decoder's lookup table (huffdec.hip):
// the walk from the root over the first HIC_HD_LUT_BITS bits of a code.  One body
// for the host loop of the one-stream entry points (decode_prepare) and for
// k_hd_lut_table, which builds every stream's table on the GPU from the uploaded
// child[]; plain C, so a host test compiles it alone.
//
//   child[2n] / child[2n + 1] = node n's '1' / '0' child: >= 0 an internal node,
//   -1 missing, <= -2 leaf (-2 - leaf index); node 0 is the root
//   entry: [3:0] bits consumed - 1, [5:4] kind, [31:8] leaf / node index
#ifndef HIC_HUFFDEC_LUT_H
#define HIC_HUFFDEC_LUT_H
#include <stdint.h>

#if defined(__HIPCC__)
#define HIC_HD_FN __host__ __device__ inline
#else
#define HIC_HD_FN static inline
#endif

enum { HIC_HD_LUT_BITS = 12 };
// kind: a leaf reached, still internal after HIC_HD_LUT_BITS bits, a missing child
enum { HIC_HD_LEAF = 0, HIC_HD_NODE = 1, HIC_HD_MISSING = 2 };

// the entry of the HIC_HD_LUT_BITS-bit value v (its MSB is the first bit read)
HIC_HD_FN uint32_t hic_hd_lut_entry(const int32_t *child, int v) {
  int node = 0;
  uint32_t e = ((uint32_t)(HIC_HD_LUT_BITS - 1)) | ((uint32_t)HIC_HD_NODE << 4);
  for (int k = 0; k < HIC_HD_LUT_BITS; ++k) {
    const int c = child[2 * node + 1 - ((v >> (HIC_HD_LUT_BITS - 1 - k)) & 1)];
    if (c == -1) return (uint32_t)k | ((uint32_t)HIC_HD_MISSING << 4);
    if (c < 0) return (uint32_t)k | ((uint32_t)HIC_HD_LEAF << 4) | ((uint32_t)(-2 - c) << 8);
    node = c;
    e = ((uint32_t)(HIC_HD_LUT_BITS - 1)) | ((uint32_t)HIC_HD_NODE << 4) | ((uint32_t)node << 8);
  }
  return e;
}
#endif
