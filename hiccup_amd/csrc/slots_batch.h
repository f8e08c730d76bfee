// slots_batch.h -- the per-batch table of the batched slot encode
// (hic_slots_batch_table, hic_encode420_slots_batch_u8, hic_rle_slots_close_batch):
// N images of one shape, each a whole image of the slot layout (slots.h), encoded
// by one fused launch and closed by one scan launch.  The 15 + 15 per-image kernel
// arguments (per channel the slots, DC differences, records and last DCs the
// encoder writes, and what the close adds from its RleJob16) do not fit by-value
// kernel arguments for a useful N: they live in device memory, one entry per image
// after a header the host reads (the blob is the same on both sides; the library
// fills the host copy, the caller uploads it once).
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef HIC_ENC_WPB
#define HIC_ENC_WPB 4  // the fused encoder's waves per workgroup (encode.hip)
#endif

namespace hic {

constexpr uint64_t kSlotBatchMagic = 0x3142544C53434948ull;  // "HICSLTB1"

// one channel of one image
struct SlotBatchChan {
  uint8_t *slot_len;
  int16_t *slot_val;
  int32_t *dc_diff;
  int64_t *ws;       // the records (encoder), offsets and hand-off granules (close)
  int32_t *rdc;      // the records' last DCs (in the workspace)
  int32_t *sidx;     // 4 int32 per record (close)
  int64_t *d_count;
  uint8_t *sym_len;  // the contiguous stream: the close writes its EOB
  int16_t *sym_val;
  int64_t cap;
};
struct SlotBatchEntry {
  SlotBatchChan c[3];  // Y, Cr, Cb
  int64_t pad[2];      // 256 bytes: an entry never straddles more cache lines than it needs
};
static_assert(sizeof(SlotBatchEntry) == 256, "table entry size");

struct SlotBatchHeader {
  uint64_t magic;
  int32_t n, max_len;
  int64_t H, W;
  int32_t wg_band, wg_flat;  // encoder workgroups per image: stacked bands / one unit per wave
  int32_t nstrips, nunits;   // per image
  int64_t nblk[3];           // per channel of one image
  int32_t nrec[3];           // records
  int32_t parts[3];          // the close's scan partitions
  int32_t parts_image;       // parts[0] + parts[1] + parts[2]
  int32_t pad[7];
};
static_assert(sizeof(SlotBatchHeader) == 128, "table header size");

// Checks a host blob's header against what the builder writes for its own (n, H, W)
// (a wrong magic, a foreign or damaged blob); nullptr = good, else what is wrong.
const char *slot_batch_header_error(const SlotBatchHeader &h);

}  // namespace hic
