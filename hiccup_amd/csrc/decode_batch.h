// decode_batch.h -- the per-batch table of the batched decode (hic_decode_batch_table,
// hic_decode420_batch_u8): N images of one shape, each decoded as the one-image fused
// tile decoders decode it (k_rld_idct_indexed, dct.hip), by two launches for the whole
// batch: every image's Cr and Cb tiles, then every image's Y tiles straight to RGB.
// The 21 per-image pointers (per channel the symbols or slots, the count, the DC
// differences, the index, the output and the status word) do not fit by-value kernel
// arguments for a useful N: they live in device memory, one entry per image after a
// header the host reads (the blob is the same on both sides; the library fills the
// host copy, the caller uploads it once), as the batched encode's table (slots_batch.h).
#pragma once
#include <stdint.h>

namespace hic {

constexpr uint64_t kDecBatchMagic = 0x3142434544434948ull;  // "HICDECB1"

// one channel of one image (hic_decode_plane, include/hiccup_hip.h)
struct DecBatchPlane {
  const uint8_t *sym_len;  // or the slots
  const int16_t *sym_val;
  const int64_t *d_nsym;
  const int32_t *dc_diff;
  const void *index;       // int64 tile index, or the close's int32 record index
  uint8_t *out;            // Y: the image's RGB pixels; Cr / Cb: its H/2 x W/2 plane
  int64_t *d_status;
};
struct DecBatchEntry {
  DecBatchPlane c[3];  // Y, Cr, Cb
  int64_t pad[11];     // 256 bytes: an entry never straddles more cache lines than it needs
};
static_assert(sizeof(DecBatchEntry) == 256, "table entry size");

struct DecBatchHeader {
  uint64_t magic;
  int32_t kind, n;                    // HIC_STREAM_INDEXED / HIC_STREAM_SLOTS
  int64_t H, W;
  int64_t rgb_stride, chroma_stride;
  int32_t tiles_y, tiles_c;           // waves per image: Y's tiles; Cr's tiles + Cb's
  int32_t grid_y, grid_c;             // workgroups of the luma / the chroma launch
  int64_t nblk_y, nblk_c;             // blocks of the Y plane / of one chroma plane
  int64_t pad[6];
};
static_assert(sizeof(DecBatchHeader) == 128, "table header size");

}  // namespace hic
