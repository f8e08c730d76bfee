// decode_batch.h -- the per-batch table of the batched decode (hic_decode_batch_table,
// hic_decode420_batch_u8): N images of one shape, each decoded as the one-image fused
// tile decoders decode it (k_rld_idct_indexed, decode.hip), by two launches for the whole
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

// ---- the batched region decode (hic_decode_window_batch_table,
// hic_decode420_window_batch_u8): a window of one size h x w per image, each image at
// its own origin, cropped into one dense (n, h, w, 3) result by the same two launches.
// A table format of its own: besides the pointers an entry holds the geometry of its
// image's two window launches, which the waves read by scalar loads as they read the
// pointers.
constexpr uint64_t kDecWinBatchMagic = 0x3157434544434948ull;  // "HICDECW1"

// The geometry of one window launch over one plane (decode.hip, colour_block's and
// k_rld_idct_indexed's window forms).
struct WinGeo {
  int bi0, nrows, bj0, bj1;  // the launch plane's block rows [bi0, bi0 + nrows), columns [bj0, bj1)
  int tpr;                   // waves per block row (the most tiles a row's columns touch)
  int oy, ox;                // the plane coordinates of out's first sample
  int cy0, cx0, ch, cw;      // RGB form: the chroma planes' span
  int cpitch;
  int64_t n_ac;              // *d_status of a good launch: 63 per block of the window
};
static_assert(sizeof(WinGeo) == 56, "window geometry size");

struct DecWinBatchEntry {
  DecBatchPlane c[3];  // Y (out: the image's h x w x 3 pixels), Cr, Cb (out: its chroma window buffer)
  WinGeo g[2];         // the luma launch (oy, ox = the request's y0, x0: the store crops), the chroma launch
  int32_t y0, x0;      // the request's origin
  int64_t pad[28];     // 512 bytes, a power of two
};
static_assert(sizeof(DecWinBatchEntry) == 512, "window table entry size");

struct DecWinBatchHeader {
  uint64_t magic;
  int32_t kind, n;
  int64_t H, W, h, w;                  // the images' shape; the windows' shape
  int64_t out_row_stride;              // bytes between the pixel rows of one image's result
  int64_t chroma_pitch, chroma_rows;   // of every chroma window buffer (rows of chroma_pitch bytes)
  int32_t waves_y, waves_c;            // T of each launch: waves per image, the largest any image plans
  int32_t grid_y, grid_c;              // workgroups of the luma / the chroma launch
  int64_t nblk_y, nblk_c;              // blocks of the Y plane / of one chroma plane
  int64_t pad[3];
};
static_assert(sizeof(DecWinBatchHeader) == 128, "window table header size");

}  // namespace hic
