"""Device-resident JPEG-style encode / decode pipeline (the hot path, no host hops).

``Encoder.encode(rgb)`` = compression.jpeg_compression + the zig-zag / DC / RLE
half of codec.jpeg_encode (compression.py:16-39, codec.py:286-301) for one
H x W x 3 uint8 image that already lives in HBM:

  1+2. hic_encode420_u8       (W % 512 == 0 by default, any W % 16 on request;
                              H % 16 == 0) colour + 4:2:0 pyrDown +
                              8x8 DCT + quantize + zig-zag of the three planes + the
                              RLE tile records in ONE launch; the planes never reach
                              HBM.  Otherwise two launches:
  1. hic_rgb_to_ycrcb420      RGB -> Y (H x W) + pyrDown'd Cr, Cb (H/2 x W/2)
  2. hic_dct_quant_rle_u8_batch  8x8 DCT + quantize + zig-zag of the three planes in
                              one launch -> int16 blocks (ZIGZAG_I16), with the RLE
                              tile pass fused into the epilogue
  3. hic_rle_encode_i16_tiles_batch  DC DPCM + channel-wide AC RLE of all three
                              channels (one scan + one emit launch) -> (uint8 len, int16 val)

Slot layout (round 6, the default for a whole image with W % 512 == 0, H % 16 ==
0 and max_len 15): hic_encode420_slots_u8 writes every RLE record's symbols and DC
differences itself (slots.h), and hic_rle_slots_close (one scan launch) closes
the records' carried runs and writes the record index: two launches per image, no
int16 coefficients in HBM.  compact() / materialize() give the contiguous stream
and the zig-zag blocks when a caller asks (result(), hic_image()).

All launches are asynchronous on one stream; buffers are allocated once.
``Decoder.decode`` runs the inverse chain (codec.jpeg_decode's RLE/DC/izigzag
half + compression.jpeg_decompression).  The optional ``stitch`` tensors make
an encoder one tile-shard of a larger image (see sharding.py).
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib, device

CHANNELS = ("lum", "cr", "cb")
TABLES = {"lum": _lib.TABLE_LUMINANCE, "cr": _lib.TABLE_CHROMINANCE, "cb": _lib.TABLE_CHROMINANCE}


def _nblk(h, w):
    return -(-h // 8) * -(-w // 8)


def input_span(H, r0, r1):
    """Rows of an H-row image that hic_rgb_to_ycrcb420_rows needs for output rows [r0, r1)."""
    c0, c1 = r0 // 2, min(H // 2, r1 // 2)
    return max(0, 2 * c0 - 2), max(r1, min(H, 2 * c1 + 2))


# hic_rle_encode_* report failures through the count (include/hiccup_hip.h):
# -(symbols needed) when the buffer is too small, HIC_COUNT_SCAN_TIMEOUT when a
# cross-workgroup scan hand-off timed out (never expected; the stream is invalid)
COUNT_SCAN_TIMEOUT = -(2 ** 63)
COUNT_WIRE_OVERFLOW = -(2 ** 63) + 1  # a gathered segment's sender flagged an out-of-width value


def check_count(c, channel=""):
    """Raise the error a negative symbol count stands for."""
    if c >= 0:
        return
    if c == COUNT_SCAN_TIMEOUT:
        raise _lib.HipError("RLE scan hand-off timed out (channel %s): the stream is invalid" % channel)
    if c == COUNT_WIRE_OVERFLOW:
        raise _lib.HipError("a gathered shard flagged a coefficient outside its wire width (channel %s): the "
                            "stream is invalid" % channel)
    raise MemoryError("symbol buffer too small for channel %s: %d symbols needed" % (channel, -c))


def encoder_layout(H, W, rows=None, fused=None, index=False):
    """(fused, rpt) of an Encoder of rows `rows` of an H x W image (None: the whole
    image, its own encoder): whether it runs the fused kernel (None = the measured
    default: fusable, and for row shards or an encoder with a tile index W % 512 ==
    0 too), and its RLE records per 64-block tile per channel (the fused kernel's
    chroma: one per 32-block half tile; a whole image's ragged last strip: one per
    strip segment, see Encoder.seg)."""
    r0, r1 = rows if rows is not None else (0, H)
    a, b = input_span(H, r0, r1)
    # (hic_encode420_u8 reads the input rows through 32-bit buffer offsets)
    can_fuse = (W % 16 == 0 and H % 16 == 0 and r0 % 16 == 0 and r1 % 16 == 0
                and (b - a) * W * 3 <= 2**31 - 1)
    if fused and not can_fuse:
        raise ValueError("the fused encoder needs W, H and rows multiples of 16, "
                         "and < 2 GiB of input rows")
    seg = rows is None and not index  # a whole image's own encoder: records per strip segment
    f = (can_fuse and (W % 512 == 0 or seg)) if fused is None else bool(fused)
    half = f and (W % 512 == 0 or seg)
    return f, {"lum": 1, "cr": 2 if half else 1, "cb": 2 if half else 1}


def slots_eligible(H, W, max_len=15, rows=None, out=None, fused=None, landing_rpt=None):
    """Whether an Encoder of this shape can take the slot layout (hic_encode420_slots_u8:
    a whole image, W % 512 == 0, H % 16 == 0, max_len 15, < 2 GiB of RGB)."""
    return (rows is None and out is None and landing_rpt is None and fused is not False and max_len == 15
            and W % 512 == 0 and H % 16 == 0 and H >= 16 and H * W * 3 <= 2**31 - 1)


SLOT_RPT = {"lum": 1, "cr": 2, "cb": 2}  # the slot layout's records per 64-block tile


def slot_fill_job(k, block0, nblk, blocks=None, wire=None):
    """hic_slot_fill_job of channel k: blocks [block0, block0 + nblk) of the channel
    from `blocks` (int16 zig-zag blocks) or `wire` (hic_wire_pack_i16's format):
    device tensors or addresses, exactly one of the two."""
    p = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in (wire, blocks)]
    return _lib.SlotFillJob(p[0], p[1], nblk, block0, CHANNELS.index(k), TABLES[k])


class SlotIndex:
    """The slot-layout stream of an Encoder for Decoder.decode(index=...): per channel
    the slot arrays, the close's record index and the records per 64-block tile."""

    def __init__(self, enc):
        self.slot_len, self.slot_val, self.sidx, self.rpt = enc.slot_len, enc.slot_val, enc.sidx, enc.rpt

    def __getitem__(self, k):
        return self.sidx[k]


class Encoder:
    """rows=(r0, r1) makes this encoder one row-shard of an H x W image (r0 even;
    shards of one image split at multiples of 16 rows so chroma blocks align)."""

    def __init__(self, H, W, max_len=15, rows=None, out=None, fused=None, index=False, landing_rpt=None, slots=None):
        """out: optional {channel: (coef (n, 64) int16, dc (n,) int32)} device views the
        encoder writes into (a gathering rank points them at its slice of the whole
        image's buffers, so its own shard needs no copy).
        fused: colour + 4:2:0 + DCT in one kernel (hic_encode420_u8, the planes never
        reach HBM; W, H and the row range multiples of 16); None = the faster path
        as measured (encoder_layout): fused for a whole image with W % 16 == 0 (a
        ragged last strip gets one RLE record per strip segment: 3840x2160 38.1-40.1
        vs 40.5-41.4 us per image for the chain), and for a row
        shard or an encoder with a tile index when W % 512 == 0; False = the chain.
        landing_rpt: a landing zone only (the gathering rank of a stream gather): no
        transform, no plane buffers, and the RLE record layout of the shards that
        fill it (their encoder_layout rpt), whatever this shape alone would pick.
        slots: the slot layout (module docstring); None = whenever slots_eligible,
        False = the coefficient + emit chain.  slots=True with landing_rpt = SLOT_RPT
        is a slot landing zone (a whole image slots_eligible accepts): fill() writes
        its records from gathered segments, entropy() closes them, and everything
        after that is a slot encoder's."""
        if H < 2 or W < 2:
            raise ValueError("image must be at least 2 x 2")
        device.require_gpu()
        self.H, self.W, self.max_len = H, W, max_len
        r0, r1 = rows if rows is not None else (0, H)
        if r0 % 2 or not (0 <= r0 < r1 <= H):
            raise ValueError("bad row range %r" % ((r0, r1),))
        self.rows = (r0, r1)
        self.want_index = bool(index)
        self.landing = landing_rpt is not None
        ok = slots_eligible(H, W, max_len, rows, out, fused, landing_rpt)
        if slots and self.landing:
            # a slot landing zone (hic_slots_fill_batch fills it, fill()): the shape rule
            # of a whole-image slot encoder, and the slot layout's records
            ok = slots_eligible(H, W, max_len, rows, out, fused) and dict(landing_rpt) == SLOT_RPT
        if slots and not ok:
            raise ValueError("the slot layout needs a whole image with W % 512 == 0, H % 16 == 0 and max_len 15"
                             + (" (a landing zone: landing_rpt %r)" % (SLOT_RPT,) if self.landing else ""))
        self.slots = ok if slots is None else bool(slots)
        if self.landing:
            self.fused, self.rpt = False, dict(landing_rpt)
        elif self.slots:
            self.fused, self.rpt = True, {"lum": 1, "cr": 2, "cb": 2}
        else:
            self.fused, self.rpt = encoder_layout(H, W, rows, fused, index)
        # a whole image's ragged last strip (W % 512 != 0): the fused kernel writes one
        # RLE record per strip segment (hic_encode420_seg_u8) and the scan / emit walk
        # row segments (hic_rle_encode_i16_rows_batch): no tile pass
        self.seg = (not self.landing and not self.slots and self.fused and rows is None and W % 512 != 0
                    and not self.want_index)
        c0, c1 = r0 // 2, min(H // 2, r1 // 2)
        self.shapes = {"lum": (r1 - r0, W), "cr": (c1 - c0, W // 2), "cb": (c1 - c0, W // 2)}
        ys, cs = self.shapes["lum"], self.shapes["cr"]
        lib = _lib.load()
        # the planes exist only on the two-kernel path
        self.y = self.cr = self.cb = None
        if not self.fused and not self.landing:
            self.y = device.empty(ys, torch.uint8)
            self.cr = device.empty(cs, torch.uint8)
            self.cb = device.empty(cs, torch.uint8)
        self.planes = {"lum": self.y, "cr": self.cr, "cb": self.cb}
        self.coef, self.dc, self.sym_len, self.sym_val, self.ws, self.ws_bytes = {}, {}, {}, {}, {}, {}
        self.cap = {}
        self.counts = device.zeros((3,), torch.int64)
        self.summaries = device.zeros((3, 4), torch.int64)
        for k in CHANNELS:
            n = _nblk(*self.shapes[k])
            if out is not None:
                self.coef[k], self.dc[k] = out[k]
                if tuple(self.coef[k].shape) != (n, 64) or tuple(self.dc[k].shape) != (n,):
                    raise ValueError("out[%s]: expected (%d, 64) / (%d,) views" % (k, n, n))
            else:
                self.coef[k] = device.empty((n, 64), torch.int16)
                self.dc[k] = device.empty((n,), torch.int32)
            # a shard's stream can open with the fillers of a zero run carried from every
            # block before it (a flat previous shard): room for those too
            lead = (r0 // (8 if k == "lum" else 16)) * -(-self.shapes[k][1] // 8)
            self.cap[k] = n * 63 + 1 + (lead * 63 // max_len if max_len > 0 else 1)
            self.sym_len[k] = device.empty((self.cap[k],), torch.uint8)
            self.sym_val[k] = device.empty((self.cap[k],), torch.int16)
            # a whole image's row-segment records outnumber its 64-block tiles when the
            # image is narrow (W <= ~350): size by the records
            rowb = -(-self.shapes[k][1] // 8)
            self.ws_bytes[k] = (lib.hic_rle_rows_workspace_bytes(n, rowb, self.rpt[k]) if self.seg
                                else lib.hic_rle_workspace_bytes(n, 64))
            self.ws[k] = device.workspace(self.ws_bytes[k])
        if self.slots:
            # the slot layout: slots of 63 symbols per block, the close's record index
            # (4 int32 per record), the records + their last DCs in the workspace
            self.slot_len, self.slot_val, self.sidx = {}, {}, {}
            for k in CHANNELS:
                n = self.coef[k].shape[0]
                self.slot_len[k] = device.empty((n * 63,), torch.uint8)
                self.slot_val[k] = device.empty((n * 63,), torch.int16)
                self.sidx[k] = device.empty((4 * (n * self.rpt[k] // 64),), torch.int32)
                self.ws_bytes[k] = lib.hic_rle_slots_workspace_bytes(n, self.rpt[k])
                self.ws[k] = device.workspace(self.ws_bytes[k])
            self._mat_status = device.zeros((3,), torch.int64)
            self.index = SlotIndex(self)
            return
        # index=True: the encoder-side tile index a device decoder reads
        # (Decoder.decode(..., index=enc.index)): 3 int64 per 64-block tile
        self.index = ({k: device.empty((3 * -(-self.coef[k].shape[0] // 64),), torch.int64) for k in CHANNELS}
                      if self.want_index else None)

    @property
    def pixels(self):
        return (self.rows[1] - self.rows[0]) * self.W

    def input_span(self):
        """Image rows [in0, in1) this encoder reads: its rows plus the pyrDown halo."""
        return input_span(self.H, *self.rows)

    def transform(self, rgb, stream=None, in_row0=None, dct_events=None):
        """Steps 1-2: colour + 4:2:0 + DCT/quantize/zig-zag of the three planes.
        rgb holds image rows [in_row0, in_row0 + rgb.shape[0]) (default: the
        whole image for an unsharded encoder, input_span() for a shard)."""
        if self.landing:
            raise RuntimeError("a landing-zone Encoder does not transform")
        s = device.stream_ptr(stream)
        if in_row0 is None:
            in_row0 = 0 if self.rows == (0, self.H) else self.input_span()[0]
        r0, r1 = self.rows
        ev = (dct_events.start, dct_events.stop) if dct_events is not None else (None, None)
        if self.slots:
            # colour + pyrDown + DCT/quantize/zig-zag + the records' symbols and DC
            # differences, in ONE launch (slots.h): no coefficients reach HBM
            if in_row0 != 0 or rgb.shape[0] != self.H:
                raise ValueError("a slot-layout encoder takes the whole image")
            _lib.call("hic_encode420_slots_u8", device.ptr(rgb), self.H, self.W, self._slot_jobs(), self.max_len, s,
                      *ev)
            return
        if self.fused:
            # colour + pyrDown + DCT/quantize/zig-zag of the three planes + RLE tile
            # records in ONE launch (dct_events time it)
            rgb, in_row0 = self._fused_input(rgb, in_row0)
            coefs = [device.ptr(self.coef[k]) for k in CHANNELS]
            wss = [device.ptr(self.ws[k]) for k in CHANNELS]
            if self.seg:
                _lib.call("hic_encode420_seg_u8", device.ptr(rgb), in_row0, rgb.shape[0], self.H, self.W, r0, r1 - r0,
                          *coefs, *wss, self.ws_bytes["lum"], min(self.ws_bytes["cr"], self.ws_bytes["cb"]),
                          self.max_len, s, *ev)
            else:
                _lib.call("hic_encode420_u8", device.ptr(rgb), in_row0, rgb.shape[0], self.H, self.W, r0, r1 - r0,
                          *coefs, *wss, self.max_len, s, *ev)
            return
        _lib.call("hic_rgb_to_ycrcb420_rows", device.ptr(rgb), in_row0, rgb.shape[0], self.H, self.W, r0, r1 - r0,
                  device.ptr(self.y), device.ptr(self.cr), device.ptr(self.cb), s)
        # DCT + quantize + zig-zag of the three planes in ONE launch (each plane with
        # its own table), with the RLE tile pass fused into its epilogue; dct_events
        # (device.KernelEvents) receive the launch's own begin / end timestamps
        jobs = (_lib.DctPlaneJob * 3)()
        for i, k in enumerate(CHANNELS):
            h, w = self.shapes[k]
            p = self.planes[k]
            jobs[i] = _lib.DctPlaneJob(p.data_ptr(), h, w, p.stride(0), TABLES[k], self.coef[k].data_ptr(),
                                       self.ws[k].data_ptr())
        _lib.call("hic_dct_quant_rle_u8_batch", 3, jobs, self.max_len, s, *ev)

    def _fused_input(self, rgb, in_row0):
        """The fused kernel addresses its input rows with 32-bit offsets: hand it the
        span it reads (< 2 GiB by can_fuse) when the caller passes more rows."""
        a, b = self.input_span()
        if rgb.shape[0] * self.W * 3 > 2**31 - 1 and in_row0 <= a and in_row0 + rgb.shape[0] >= b:
            rgb, in_row0 = rgb[a - in_row0:b - in_row0], a
        return rgb, in_row0

    def batchable(self):
        """Whether transform_batch can take this encoder into a batched launch."""
        return (self.fused and not self.slots and not self.seg and not self.landing and self.W % 512 == 0)

    def _slot_jobs(self):
        jobs = (_lib.SlotJob * 3)()
        for i, k in enumerate(CHANNELS):
            jobs[i] = _lib.SlotJob(self.coef[k].shape[0], self.rpt[k], self.slot_len[k].data_ptr(),
                                   self.slot_val[k].data_ptr(), self.dc[k].data_ptr(), self.sidx[k].data_ptr(),
                                   self.ws[k].data_ptr(), self.ws_bytes[k], self.counts[i:i + 1].data_ptr(),
                                   self.sym_len[k].data_ptr(), self.sym_val[k].data_ptr(), self.cap[k])
        return jobs

    def fill(self, segs, stream=None):
        """Slot layout: segments of already-quantized blocks into their records' slots
        (hic_slots_fill_batch; what transform() writes for those records).  segs: a
        list of slot_fill_job(...) (32 per call), or a ready _lib.SlotFillJob array.
        entropy() closes the image once every record is filled."""
        if not self.slots:
            raise ValueError("fill() needs a slot-layout encoder")
        s = device.stream_ptr(stream)
        if isinstance(segs, ctypes.Array):
            segs = [segs]
        else:
            segs = [(_lib.SlotFillJob * len(segs[i:i + 32]))(*segs[i:i + 32]) for i in range(0, len(segs), 32)]
        jobs = self._slot_jobs()
        for arr in segs:
            _lib.call("hic_slots_fill_batch", 3, jobs, len(arr), arr, self.max_len, s)

    def compact(self, stream=None):
        """Slot layout: the contiguous symbol stream into sym_len / sym_val (what the
        emit writes; hic_rle_slots_compact).  A no-op for the coefficient chain."""
        if self.slots:
            _lib.call("hic_rle_slots_compact", 3, self._slot_jobs(), self.max_len, device.stream_ptr(stream))

    def materialize(self, stream=None):
        """Slot layout: the contiguous stream and the zig-zag blocks (self.coef,
        decoded from the slots: hic_rle_decode_i16_slots), as the coefficient chain
        leaves them.  A no-op for the coefficient chain."""
        if not self.slots:
            return
        self.compact(stream)
        s = device.stream_ptr(stream)
        for i, k in enumerate(CHANNELS):
            _lib.call("hic_rle_decode_i16_slots", device.ptr(self.slot_len[k]), device.ptr(self.slot_val[k]),
                      ctypes.c_void_p(self.counts.data_ptr() + 8 * i), device.ptr(self.dc[k]), self.coef[k].shape[0],
                      self.rpt[k], device.ptr(self.sidx[k]), device.ptr(self.coef[k]),
                      device.ptr(self._mat_status[i:i + 1]), s)

    def shard_summaries(self, stream=None):
        """Per-channel {trailing zeros, has nonzero, first DC, last DC} (sharded encode)."""
        if self.slots:
            raise ValueError("shard summaries are for row shards (a slot-layout encoder is a whole image)")
        if self.seg:
            raise ValueError("shard summaries read 64-block tile records (a row shard's); this whole-image "
                             "encoder keeps one per strip segment")
        s = device.stream_ptr(stream)
        for i, k in enumerate(CHANNELS):
            n = self.coef[k].shape[0]
            _lib.call("hic_rle_shard_summary_records", device.ptr(self.coef[k]), n, self.rpt[k], device.ptr(self.ws[k]),
                      device.ptr(self.summaries[i]), s)
        return self.summaries

    def entropy(self, stream=None, stitch=None):
        """Step 3: DC DPCM + AC RLE of the three channels (one scan launch and one
        emit launch for all three).  stitch: None or a (3, 4) int64 device tensor of
        per-channel {carry_zeros, emit_eob, has_prev_dc, prev_dc}."""
        s = device.stream_ptr(stream)
        if self.slots:
            if stitch is not None:
                raise ValueError("a slot-layout encoder is a whole image (no stitch)")
            _lib.call("hic_rle_slots_close", 3, self._slot_jobs(), self.max_len, s)
            return
        if self.seg:
            rowb = (ctypes.c_int64 * 3)(self.W // 8, self.W // 16, self.W // 16)
            _lib.call("hic_rle_encode_i16_rows_batch", 3, self._rle_jobs(stitch), rowb, self.max_len, s)
        else:
            # with a tile index wanted, the emit writes it too (hic_rle_job16.d_index:
            # hic_rle_tile_index_i16's words, no launch of its own)
            _lib.call("hic_rle_encode_i16_tiles_batch", 3, self._rle_jobs(stitch, index=True), self.max_len, s)

    def encode(self, rgb, stream=None, dct_events=None):
        self.transform(rgb, stream, dct_events=dct_events)
        self.entropy(stream)

    def _rle_jobs(self, stitch, index=False):
        jobs = (_lib.RleJob16 * 3)()
        for i, k in enumerate(CHANNELS):
            ix = self.index[k].data_ptr() if index and self.index is not None and stitch is None else None
            jobs[i] = _lib.RleJob16(self.coef[k].data_ptr(), self.coef[k].shape[0],
                                    stitch[i].data_ptr() if stitch is not None else None, self.dc[k].data_ptr(),
                                    self.sym_len[k].data_ptr(), self.sym_val[k].data_ptr(), self.cap[k],
                                    self.counts[i:i + 1].data_ptr(), self.ws[k].data_ptr(), self.rpt[k],
                                    self.ws_bytes[k], ix)
        return jobs

    def hic_image(self, stream=None, from_slots=False):
        """codec.jpeg_encode of this encode, from the device streams: the nine Huffman
        trees from GPU key histograms, the nine bit strings packed on the GPU
        (huffman.DeviceStreams); == codec.jpeg_encode(the encoded CompressedImage)
        for an unsharded encoder (syncs).  A slot-layout encoder compacts its stream
        first (sym_len / sym_val are valid afterwards); with from_slots=True the six AC
        streams are histogrammed and packed straight from the slots instead
        (huffman.SlotStream: no compaction, sym_len / sym_val hold only the EOB the
        close wrote).  from_slots changes nothing for the coefficient chain."""
        if self.rows != (0, self.H):
            raise ValueError("hic_image needs the whole image (an unsharded encoder)")
        from_slots = bool(from_slots) and self.slots
        if not from_slots:
            self.compact(stream)
        with device.on_stream(stream):  # the counts and histograms are read after the stream's kernels
            return self._hic_image(stream, from_slots)

    def _hic_image(self, stream, from_slots, counts=None):
        """counts: the three symbol counts when the caller has already read them
        (BatchEncoder.hic_images: one read for the batch)."""
        from . import hicimage as hic
        from . import huffman
        counts = self.counts.cpu().tolist() if counts is None else counts
        jobs = self._slot_jobs() if from_slots else None
        keys = {}
        for i, k in enumerate(CHANNELS):
            check_count(int(counts[i]), k)
            c = int(counts[i])
            dc = (self.dc[k], self.dc[k].numel())
            keys[k] = ((dc, huffman.SlotStream(jobs[i], c, 1), huffman.SlotStream(jobs[i], c, 0)) if from_slots else
                       (dc, (self.sym_val[k], c), (self.sym_len[k], c)))
        # the nine streams in payload order, their host round trips batched
        order = [(k, j) for j in range(3) for k in CHANNELS]
        ds = huffman.DeviceStreams([keys[k][j] for k, j in order], stream=stream)
        # DC keys as the reference holds them (numpy int32: dct_channel's dtype)
        tables = [hic.PayloadStringP(hic.TupP, [hic.TupP(np.int32(v) if j == 0 else int(v), c)
                                                for v, c in ds.trees[i].encode_table()])
                  for i, (k, j) in enumerate(order)]
        data = [hic.BitStringP.from_packed(*pk) for pk in ds.packed()]
        (h, w), (hc, wc) = self.shapes["lum"], self.shapes["cr"]
        return hic.HicImage.jpeg_image(tables + data + [hic.TupP(h, w), hic.TupP(hc, wc)])

    def result(self):
        """Host copies: {channel: (zigzag blocks, dc_diff, sym_len, sym_val)} (syncs;
        a slot-layout encoder materializes its stream and blocks first)."""
        self.materialize()
        device.sync()
        counts = self.counts.cpu().numpy()
        out = {}
        for i, k in enumerate(CHANNELS):
            c = int(counts[i])
            check_count(c, k)
            out[k] = (self.coef[k].cpu().numpy(), self.dc[k].cpu().numpy(), self.sym_len[k][:c].cpu().numpy(),
                      self.sym_val[k][:c].cpu().numpy())
        return out


def transform_batch(encoders, inputs, stream=None, in_row0s=None, dct_events=None):
    """Encoder.transform of several encoders -- the row shards of a multi-GPU group,
    one per image -- in ONE launch (hic_encode420_batch_u8) when every one is a fused
    coefficient encoder whose records its kernel writes (Encoder.batchable) and at
    most 8 share one max_len; else one transform each.  A shard is 1/N of an image,
    too few waves to fill the chip alone: at N = 8 eight launches in a row took 2.4x
    one whole-image launch.  dct_events (per encoder, None or device.KernelEvents):
    each pair spans the batched launch."""
    n = len(encoders)
    in_row0s = in_row0s if in_row0s is not None else [None] * n
    dct_events = dct_events if dct_events is not None else [None] * n
    if not (2 <= n <= 8 and all(e.batchable() for e in encoders)
            and len(set(e.max_len for e in encoders)) == 1):
        for e, x, r, ev in zip(encoders, inputs, in_row0s, dct_events):
            e.transform(x, stream, in_row0=r, dct_events=ev)
        return
    jobs = (_lib.Encode420Job * n)()
    for i, (e, x, r) in enumerate(zip(encoders, inputs, in_row0s)):
        if r is None:
            r = 0 if e.rows == (0, e.H) else e.input_span()[0]
        x, r = e._fused_input(x, r)
        r0, r1 = e.rows
        jobs[i] = _lib.Encode420Job(x.data_ptr(), r, x.shape[0], e.H, e.W, r0, r1 - r0,
                                    *(e.coef[k].data_ptr() for k in CHANNELS), *(e.ws[k].data_ptr() for k in CHANNELS))
    s = device.stream_ptr(stream)
    evs = [ev for ev in dct_events if ev is not None]
    for ev in evs[1:]:
        _lib.call("hic_event_record", ev.start, s)
    first = (evs[0].start, evs[0].stop) if evs else (None, None)
    _lib.call("hic_encode420_batch_u8", n, jobs, encoders[0].max_len, s, *first)
    for ev in evs[1:]:
        _lib.call("hic_event_record", ev.stop, s)


BATCH_MAX = 4096  # HIC_SLOTS_BATCH_MAX (include/hiccup_hip.h)


def batch_slots_eligible(n, H, W, max_len=15):
    """Whether BatchEncoder takes n images of H x W: 1 <= n <= BATCH_MAX whole images
    that slots_eligible accepts, their units together within the flattened grid's
    32-bit count (hic_slots_batch_table's limits)."""
    if not (1 <= n <= BATCH_MAX and slots_eligible(H, W, max_len)):
        return False
    bands = -(-(H // 16) // 4) * (W // 512)
    parts = sum(-(-(_nblk(h, w) // b) // 256) for h, w, b in ((H, W, 64), (H // 2, W // 2, 32), (H // 2, W // 2, 32)))
    return n * bands * 4 <= (2**31 - 1) // 64 and n * parts <= (2**31 - 1) // 64


def batched_default(n, H, W):
    """What BatchEncoder.hic_images(batched=None) resolves to for n images of H x W:
    the batched Huffman stage wherever its measured range lay at or below the
    per-image loop's on the parent commit -- every measured batch, 64 x 512^2 down to
    one 8K image (profiles/r17/huffman_batch/)."""
    return True


class BatchEncoder:
    """n images of one shape in the slot layout, encoded by ONE fused launch
    (hic_encode420_slots_batch_u8) and closed by ONE scan launch
    (hic_rle_slots_close_batch) instead of two launches per image: a 512 x 512 image
    is 8 workgroups of the fused kernel, and a run of such launches is bound by
    launch latency.  The batch holds n ordinary Encoder(H, W, slots=True) objects
    (batch[i], len(batch)) whose buffers the batched launches write, so everything
    after the close is an Encoder's, per image: batch[i].index for Decoder.decode,
    compact(), materialize(), result(), hic_image(from_slots=True).  Per image the
    results are bit for bit those of Encoder(H, W).encode."""

    def __init__(self, n, H, W):
        if not batch_slots_eligible(n, H, W):
            raise ValueError("a batch needs 1 <= n <= %d whole images with W %% 512 == 0 and H %% 16 == 0"
                             % BATCH_MAX)
        device.require_gpu()
        self.n, self.H, self.W = n, H, W
        self.encoders = [Encoder(H, W, slots=True) for _ in range(n)]
        # one counts tensor: each encoder's counts is a view of its row (one host read
        # checks the batch)
        self.counts = device.zeros((n, 3), torch.int64)
        for i, e in enumerate(self.encoders):
            e.counts = self.counts[i]
        # the per-batch table (hic_slots_batch_table): built on the host and uploaded once
        lib = _lib.load()
        jobs = (_lib.SlotJob * (3 * n))()
        for i, e in enumerate(self.encoders):
            for k, j in enumerate(e._slot_jobs()):
                jobs[3 * i + k] = j
        nbytes = lib.hic_slots_batch_table_bytes(n)
        self._h_table = ctypes.create_string_buffer(nbytes)
        _lib.call("hic_slots_batch_table", n, H, W, jobs, self._h_table, nbytes)
        self._d_table = device.to_device(np.frombuffer(self._h_table, np.uint8, nbytes))

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.encoders[i]

    def _stride(self, rgb):
        """The byte stride between images of an (n, H, W, 3) uint8 device tensor."""
        n, H, W = self.n, self.H, self.W
        if not (isinstance(rgb, torch.Tensor) and rgb.is_cuda and rgb.dtype == torch.uint8
                and tuple(rgb.shape) == (n, H, W, 3)):
            raise ValueError("a batch takes an (%d, %d, %d, 3) uint8 device tensor" % (n, H, W))
        if tuple(rgb.stride()[1:]) != (3 * W, 3, 1):
            raise ValueError("each image of the batch must be contiguous")
        stride = rgb.stride(0) if n > 1 else H * W * 3  # (a size-1 dimension's stride means nothing)
        if stride < H * W * 3 or stride % 8:
            raise ValueError("the images' stride must be >= H * W * 3 and a multiple of 8 (got %d)" % stride)
        return stride

    def transform(self, rgb, stream=None, dct_events=None):
        """Encoder.transform of all n images: one launch (dct_events time it)."""
        stride = self._stride(rgb)
        ev = (dct_events.start, dct_events.stop) if dct_events is not None else (None, None)
        _lib.call("hic_encode420_slots_batch_u8", device.ptr(rgb), stride, self._h_table, device.ptr(self._d_table),
                  15, device.stream_ptr(stream), *ev)

    def entropy(self, stream=None):
        """Encoder.entropy of all n images: the close of their 3 n channels in one scan launch."""
        _lib.call("hic_rle_slots_close_batch", self._h_table, device.ptr(self._d_table), 15,
                  device.stream_ptr(stream))

    def encode(self, rgb, stream=None, dct_events=None):
        self.transform(rgb, stream, dct_events=dct_events)
        self.entropy(stream)

    def hic_images(self, stream=None, from_slots=True, batched=None):
        """[batch[i].hic_image(stream, from_slots)] (syncs): one read of the batch's
        counts, then the Huffman stage.  batched=True: one pass per phase over all 9 n
        streams (huffman.BatchStreams: a number of library calls and host reads that
        does not grow with n; needs from_slots); False: the per-image stage, one
        huffman.DeviceStreams each; None: the measured default (batched_default).
        Byte for byte the same images either way."""
        if batched is None:
            batched = bool(from_slots) and batched_default(self.n, self.H, self.W)
        if batched and not from_slots:
            raise ValueError("the batched Huffman stage reads the slot layout: batched=True needs from_slots=True")
        if not from_slots:
            for e in self.encoders:
                e.compact(stream)
        with device.on_stream(stream):
            counts = self.counts.cpu().tolist()
            for c in counts:
                for v, k in zip(c, CHANNELS):
                    check_count(int(v), k)
            if batched:
                return self._hic_images_batched(stream, counts)
            return [e._hic_image(stream, bool(from_slots), counts[i]) for i, e in enumerate(self.encoders)]

    def _hic_images_batched(self, stream, counts):
        from . import huffman
        bs = huffman.BatchStreams([[e.dc[k] for k in CHANNELS] for e in self.encoders],
                                  [e._slot_jobs() for e in self.encoders], counts, stream=stream)
        collect = bs.packed_start()
        tables = self._tables(bs.trees)  # (while the GPU packs)
        return self._assemble(bs.trees, collect(), tables)

    @staticmethod
    def _tables(trees):
        """The table payloads, per image as Encoder._hic_image builds them (DC keys
        numpy int32, AC keys int: part of the byte format)."""
        from . import hicimage as hic
        return [[hic.PayloadStringP(hic.TupP, [hic.TupP(np.int32(v) if p < 3 else int(v), c)
                                               for v, c in t[p].encode_table()]) for p in range(9)] for t in trees]

    def _assemble(self, trees, packed, tables=None):
        """The batch's HicImages from its trees and packed streams: all that the
        batched stage leaves to Python."""
        from . import hicimage as hic
        tables = self._tables(trees) if tables is None else tables
        (h, w), (hc, wc) = self.encoders[0].shapes["lum"], self.encoders[0].shapes["cr"]
        return [hic.HicImage.jpeg_image(tables[i] + [hic.BitStringP.from_packed(*pk) for pk in one]
                                        + [hic.TupP(h, w), hic.TupP(hc, wc)]) for i, one in enumerate(packed)]


def stream_addresses(sym_len, sym_val, counts, dc, index, i, k):
    """Channel k's (the i-th of CHANNELS) five stream addresses as the indexed entry
    points and a DecodePlane take them: symbol (or slot) lengths, values, its word of
    the device count tensor (3,), the DC differences, the index."""
    return (sym_len[k].data_ptr(), sym_val[k].data_ptr(), counts.data_ptr() + 8 * i, dc[k].data_ptr(),
            index[k].data_ptr())


def _two(a, b):
    """Host array of two addresses (Cr's, Cb's): an argument of the *_pair entry points."""
    return (ctypes.c_void_p * 2)(a, b)


class Decoder:
    """Inverse chain: symbols -> zig-zag blocks -> pixels -> RGB (2h x 2w x 3)."""

    def __init__(self, H, W, chroma_pair=True):
        """chroma_pair: the indexed decode's Cr and Cb in one launch
        (hic_rle_decode_idct_u8_indexed_pair); False: one launch each."""
        device.require_gpu()
        self.H, self.W = H, W
        self.chroma_pair = chroma_pair
        self.shapes = {"lum": (H, W), "cr": (H // 2, W // 2), "cb": (H // 2, W // 2)}
        self.blocks, self.pix, self.status = {}, {}, device.zeros((3,), torch.int64)
        for k in CHANNELS:
            h, w = self.shapes[k]
            self.blocks[k] = device.empty((_nblk(h, w), 64), torch.int16)
            self.pix[k] = device.empty((h, w), torch.uint8)
        self.rgb = device.empty((2 * (H // 2), 2 * (W // 2), 3), torch.uint8)
        self._ws = {}

    def decode(self, sym_len, sym_val, counts, dc, stream=None, index=None, keep_blocks=False, planes=False):
        """sym_len/sym_val/dc: {channel: device tensor}; counts: host ints per channel.
        index: an Encoder(index=True)'s tile index ({channel: device tensor}), or a
        slot-layout encoder's SlotIndex (the *_slots forms of the same kernels); then
        counts is the encoder's device count tensor (3,), nothing crosses to the
        host, and each plane is decoded and inverse-transformed by ONE kernel
        (hic_rle_decode_idct_u8_indexed: no tile pass, scans, DC chain or zig-zag
        blocks in HBM); keep_blocks=True writes self.blocks too (the block-level
        indexed decode, then the IDCT).  With the index and whole 8x8 blocks (H, W
        multiples of 8) the chroma planes decode first and the luminance plane goes
        straight to RGB (hic_rle_decode_idct_rgb_indexed: self.pix["lum"] is not
        written); planes=True keeps the Y plane and the separate colour kernel."""
        s = device.stream_ptr(stream)
        lib = _lib.load()
        # The stream kind.  A SlotIndex: the encoder's slots, read through the close's
        # record index (the *_slots entry points, which also take the records per tile;
        # the sym_len / sym_val arguments are not read).  A plain {channel: tensor}: the
        # contiguous symbols and the tile index (*_indexed).
        slots = isinstance(index, SlotIndex)
        kind = "slots" if slots else "indexed"
        if slots:
            sym_len, sym_val = index.slot_len, index.slot_val
        # per channel, an indexed entry point's stream arguments: the five addresses
        # (the index last), then () or (records per tile,)
        addr, rpt = {}, {}
        if index is not None:
            for i, k in enumerate(CHANNELS):
                addr[k] = stream_addresses(sym_len, sym_val, counts, dc, index, i, k)
                rpt[k] = (index.rpt[k],) if slots else ()

        def status(i):
            return self.status.data_ptr() + 8 * i

        def decode_plane(i, k):
            """Channel k's symbols to its pixel plane, one kernel."""
            _lib.call("hic_rle_decode_idct_u8_" + kind, *addr[k], *rpt[k], *self.shapes[k], TABLES[k],
                      self.pix[k].data_ptr(), self.pix[k].stride(0), status(i), s)

        cr, cb = self.pix["cr"].data_ptr(), self.pix["cb"].data_ptr()
        if index is not None and not keep_blocks and not planes and self.H % 8 == 0 and self.W % 8 == 0:
            # Cr and Cb in one launch (one tail), then Y straight to RGB
            if self.chroma_pair:
                _lib.call("hic_rle_decode_idct_u8_%s_pair" % kind, *map(_two, addr["cr"], addr["cb"]), *rpt["cr"],
                          *self.shapes["cr"], TABLES["cr"], _two(cr, cb), self.pix["cr"].stride(0),
                          _two(status(1), status(2)), s)
            else:
                decode_plane(1, "cr")
                decode_plane(2, "cb")
            _lib.call("hic_rle_decode_idct_rgb_" + kind, *addr["lum"], *rpt["lum"], self.H, self.W, cr, cb,
                      self.rgb.data_ptr(), self.rgb.stride(0), status(0), s)
            return self.rgb
        for i, k in enumerate(CHANNELS):
            h, w = self.shapes[k]
            n = self.blocks[k].shape[0]
            if index is not None and not keep_blocks:
                decode_plane(i, k)
                continue
            if index is not None:
                # (the block-level forms take the block count, then the records per tile,
                # before the index)
                _lib.call("hic_rle_decode_i16_" + kind, *addr[k][:4], n, *rpt[k], addr[k][4], self.blocks[k].data_ptr(),
                          status(i), s)
            else:
                nsym = int(counts[i])
                need = lib.hic_rld_workspace_bytes(nsym, n)
                if k not in self._ws or self._ws[k].numel() * 8 < need:
                    self._ws[k] = device.workspace(need)
                _lib.call("hic_rle_decode_i16", device.ptr(sym_len[k]), device.ptr(sym_val[k]), nsym,
                          device.ptr(dc[k]), n, 64, device.ptr(self.blocks[k]), device.ptr(self.status[i:i + 1]),
                          device.ptr(self._ws[k]), s)
            _lib.call("hic_dequant_idct_u8", device.ptr(self.blocks[k]), _lib.LAYOUT_ZIGZAG_I16, h, w, TABLES[k],
                      device.ptr(self.pix[k]), self.pix[k].stride(0), s)
        h, w = self.shapes["cr"]
        _lib.call("hic_ycrcb420_to_rgb", device.ptr(self.pix["lum"]), self.pix["lum"].stride(0), cr, cb, h, w,
                  device.ptr(self.rgb), s)
        return self.rgb

    def check_status(self):
        """Raise unless every channel's stream decoded to exactly its blocks' AC
        positions (codec.jpeg_decode's length check, codec.py:418-419; syncs)."""
        st = self.status.cpu().tolist()
        for i, k in enumerate(CHANNELS):
            want = self.blocks[k].shape[0] * 63
            if st[i] != want:
                raise ValueError("channel %s: stream covers %d AC positions, expected %d" % (k, st[i], want))


# ------------------------------------------------------------------ batched decode
DECODE_BATCH_MAX = 4096  # HIC_DECODE_BATCH_MAX (include/hiccup_hip.h)


def batch_decode_eligible(n, H, W, slots=False):
    """Whether BatchDecoder takes n images of H x W (hic_decode_batch_table's limits): 1
    <= n <= DECODE_BATCH_MAX, H and W multiples of 16 (whole 8 x 8 blocks in all three
    planes) below 2^20, each plane's AC stream below 2^31 positions; slots=True: the
    planes also whole slot-layout records (Y: 64 blocks, chroma: 32)."""
    if not (1 <= n <= DECODE_BATCH_MAX and 16 <= H < 2**20 and 16 <= W < 2**20 and H % 16 == 0 and W % 16 == 0):
        return False
    ny, nc = _nblk(H, W), _nblk(H // 2, W // 2)
    if ny >= 2**31 // 256 or ny * 63 >= 2**31 or (slots and (ny % 64 or nc % 32)):
        return False
    ty, tc = -(-ny // 64), 2 * -(-nc // 64)
    return 4 * -(-n * ty // 4) <= 2**32 - 1 and 4 * -(-n * tc // 4) <= 2**32 - 1


class _DecodeSources:
    """The sources of a decode batch of self.n images of self.H x self.W (BatchDecoder,
    BatchRegionDecoder): their kind and stream addresses, read again only when the
    sources change (self._key, self._objs), and the DecodeImage array the table
    builders take."""

    _key = _objs = None

    def _source(self, i, src):
        """Source i as (kind, the 15 stream addresses: per channel symbols / slots, values,
        count, DC differences, index)."""
        nblk = (_nblk(self.H, self.W), _nblk(self.H // 2, self.W // 2), _nblk(self.H // 2, self.W // 2))
        if isinstance(src, Encoder):
            if (src.H, src.W) != (self.H, self.W) or src.rows != (0, src.H):
                raise ValueError("source %d: a whole %d x %d image is needed" % (i, self.H, self.W))
            if src.index is None:
                raise ValueError("source %d: the encoder has no index (a slot encoder or index=True)" % i)
            src = (src.sym_len, src.sym_val, src.counts, src.dc, src.index)
        if not (isinstance(src, (tuple, list)) and len(src) == 5):
            raise ValueError("source %d: an Encoder or (sym_len, sym_val, counts, dc, index)" % i)
        sym_len, sym_val, counts, dc, index = src
        slots = isinstance(index, SlotIndex)
        if slots:
            sym_len, sym_val = index.slot_len, index.slot_val
            if any(index.rpt[k] != SLOT_RPT[k] for k in CHANNELS):
                raise ValueError("source %d: not the slot layout's records per tile" % i)
        if not (isinstance(counts, torch.Tensor) and counts.is_cuda and counts.dtype == torch.int64
                and counts.numel() == 3 and counts.is_contiguous()):
            raise ValueError("source %d: counts must be a (3,) int64 device tensor" % i)
        addr = []
        for c, k in enumerate(CHANNELS):
            if dc[k].numel() != nblk[c]:
                raise ValueError("source %d channel %s: %d DC differences, a %d x %d image has %d blocks"
                                 % (i, k, dc[k].numel(), self.H, self.W, nblk[c]))
            want = 4 * (nblk[c] * SLOT_RPT[k] // 64) if slots else 3 * -(-nblk[c] // 64)
            if index[k].numel() != want or (slots and sym_len[k].numel() != nblk[c] * 63):
                raise ValueError("source %d channel %s: the index is not a %d x %d image's" % (i, k, self.H, self.W))
            addr += stream_addresses(sym_len, sym_val, counts, dc, index, c, k)
        return slots, addr

    def _resolve(self, sources):
        """The sources' (kind, addresses) when they differ from the previous call's, else
        None (self._key then holds them)."""
        # The same BatchEncoder, or the same Encoder objects, as the previous call: an
        # Encoder's buffers are allocated once, so the addresses are the same too, and
        # the 15 n data_ptr() reads (several us per image on the host, more than the
        # batch's GPU time for small images) are skipped.  Tuples are always compared
        # by address.
        whole = isinstance(sources, BatchEncoder)
        objs = (sources,) if whole else tuple(sources)
        if self._objs is not None and self._objs[0] == whole and len(objs) == len(self._objs[1]) and all(
                a is b for a, b in zip(objs, self._objs[1])):
            return None
        self._objs = None
        sources = objs[0].encoders if whole else list(objs)
        if len(sources) != self.n:
            raise ValueError("%d sources for a batch of %d" % (len(sources), self.n))
        kinds, addrs = zip(*(self._source(i, s) for i, s in enumerate(sources)))
        if len(set(kinds)) != 1:
            raise ValueError("the sources of a batch must be of one kind (slot layout or indexed streams)")
        key = (kinds[0], addrs)
        remember = (whole, objs) if all(isinstance(x, Encoder) for x in sources) else None
        if key == self._key:
            self._objs = remember
            return None
        return key, remember

    def _decode_images(self, addrs, outs):
        """The DecodeImage array of the resolved addresses: image i's Y, Cr, Cb planes
        decode into outs[0][i], outs[1][i], outs[2][i] and report in self.status[i]."""
        images = (_lib.DecodeImage * self.n)()
        for i, a in enumerate(addrs):
            for c in range(3):
                images[i].c[c] = _lib.DecodePlane(*a[5 * c:5 * c + 5], outs[c][i].data_ptr(),
                                                  self.status.data_ptr() + 8 * (3 * i + c))
        return images


class BatchDecoder(_DecodeSources):
    """Decoder.decode(index=...) of n images of one shape in TWO launches
    (hic_decode420_batch_u8) instead of two per image: every image's Cr and Cb tiles,
    then every image's Y tiles straight to RGB.  A 512 x 512 image is 8 + 16
    workgroups of the tile decoder, and a run of such launches is bound by launch
    latency.  Per image the results are bit for bit those of Decoder(H, W).decode:
    rgb (n, H, W, 3), cr / cb (n, H/2, W/2), status (n, 3)."""

    def __init__(self, n, H, W):
        if not batch_decode_eligible(n, H, W):
            raise ValueError("a decode batch needs 1 <= n <= %d images with H and W multiples of 16"
                             % DECODE_BATCH_MAX)
        device.require_gpu()
        self.n, self.H, self.W = n, H, W
        self.rgb = device.empty((n, H, W, 3), torch.uint8)
        self.cr = device.empty((n, H // 2, W // 2), torch.uint8)
        self.cb = device.empty((n, H // 2, W // 2), torch.uint8)
        self.status = device.zeros((n, 3), torch.int64)
        self._h_table = self._d_table = None

    def _table(self, sources, stream):
        new = self._resolve(sources)
        if new is None:
            return
        key, remember = new
        kinds, addrs = (key[0],), key[1]
        n, H, W = self.n, self.H, self.W
        if kinds[0] and not batch_decode_eligible(n, H, W, slots=True):
            raise ValueError("slot-layout sources need planes of whole records")
        images = self._decode_images(addrs, (self.rgb, self.cr, self.cb))
        nbytes = _lib.load().hic_decode_batch_table_bytes(n)
        h_table = ctypes.create_string_buffer(nbytes)
        _lib.call("hic_decode_batch_table", _lib.STREAM_SLOTS if kinds[0] else _lib.STREAM_INDEXED, n, H, W, 3 * W,
                  W // 2, images, h_table, nbytes)
        # uploaded on the decode's stream: the launches that read it follow the copy
        with device.on_stream(stream):
            d_table = device.to_device(np.frombuffer(h_table, np.uint8, nbytes))
        self._key, self._h_table, self._d_table, self._objs = key, h_table, d_table, remember

    def decode(self, sources, stream=None):
        """sources: a BatchEncoder, or a sequence of n Encoders (slot encoders or
        index=True encoders) or of n tuples (sym_len, sym_val, counts, dc, index) as
        Decoder.decode(index=...) takes them, counts the (3,) device tensor; all of one
        kind.  The table is rebuilt and uploaded only when the sources' addresses differ
        from the previous call's (the same BatchEncoder or Encoder objects as in the
        previous call have the same addresses: their buffers are allocated once);
        otherwise nothing crosses to or from the host.  Returns self.rgb."""
        self._table(sources, stream)
        if stream is not None:
            self._d_table.record_stream(stream)
        _lib.call("hic_decode420_batch_u8", self._h_table, device.ptr(self._d_table), device.stream_ptr(stream))
        return self.rgb

    def expected_status(self):
        c = _nblk(self.H // 2, self.W // 2) * 63
        return [_nblk(self.H, self.W) * 63, c, c]

    def check_status(self):
        """Raise unless every channel of every image decoded to exactly its blocks' AC
        positions (Decoder.check_status for the batch; one read, syncs)."""
        st = self.status.cpu().tolist()
        want = self.expected_status()
        for i, row in enumerate(st):
            for c, k in enumerate(CHANNELS):
                if row[c] != want[c]:
                    raise ValueError("image %d channel %s: stream covers %d AC positions, expected %d"
                                     % (i, k, row[c], want[c]))


# ------------------------------------------------------------------ region decode
class WindowPlan(collections.namedtuple("WindowPlan", "Y0 X0 Y1 X1 cy0 cx0 ch cw")):
    """hic_window (include/hiccup_hip.h): the 16-pixel-aligned covering window
    [Y0, Y1) x [X0, X1) of a request, and the span of the H/2 x W/2 chroma planes it
    needs: rows [cy0, cy0 + ch) x columns [cx0, cx0 + cw)."""

    def c_struct(self):
        return _lib.Window(*self)


def window_plan(H, W, y0, x0, h, w):
    """The Python twin of hic_window_plan: the geometry of decoding rows [y0, y0 + h)
    x columns [x0, x0 + w) of an H x W image (H, W multiples of 16; the window inside
    the image, h, w >= 1).  The kernels see only the aligned window, whole luma and
    chroma blocks; the chroma span is [Y0/2 - 1, Y1/2 + 1) -- pyrUp's one-sample halo
    -- clipped to the plane and rounded out to whole 8x8 chroma blocks."""
    if H < 16 or W < 16 or H % 16 or W % 16:
        raise ValueError("region decode needs H, W multiples of 16")
    if h < 1 or w < 1 or y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
        raise ValueError("window (%d, %d, %d, %d) outside the %d x %d image" % (y0, x0, h, w, H, W))
    Y0, X0, Y1, X1 = y0 // 16 * 16, x0 // 16 * 16, -(-(y0 + h) // 16) * 16, -(-(x0 + w) // 16) * 16

    def span(a, b, n):
        lo = max(0, a // 2 - 1) // 8 * 8
        return lo, -(-min(n, b // 2 + 1) // 8) * 8 - lo

    (cy0, ch), (cx0, cw) = span(Y0, Y1, H // 2), span(X0, X1, W // 2)
    return WindowPlan(Y0, X0, Y1, X1, cy0, cx0, ch, cw)


def window_tiles(plan, W, chroma=False):
    """The (block row, 64-block tile) pairs a window launch decodes, in wave order:
    per block row bi of the launch's blocks and its columns [bj0, bj1), the tiles
    floor((bi nbx + bj0) / 64) .. floor((bi nbx + bj1 - 1) / 64) of the plane's raster
    blocks (nbx blocks per row).  A tile that wraps two block rows appears once per
    row; each appearance stores only its own row's blocks."""
    if chroma:
        nbx, bi0, bi1, bj0, bj1 = W // 16, plan.cy0 // 8, (plan.cy0 + plan.ch) // 8, plan.cx0 // 8, (plan.cx0 + plan.cw) // 8
    else:
        nbx, bi0, bi1, bj0, bj1 = W // 8, plan.Y0 // 8, plan.Y1 // 8, plan.X0 // 8, plan.X1 // 8
    return [(bi, t) for bi in range(bi0, bi1)
            for t in range((bi * nbx + bj0) // 64, (bi * nbx + bj1 - 1) // 64 + 1)]


def window_status(plan):
    """The three status words a good window decode of `plan` leaves (Y, Cr, Cb): 63 per
    block of each launch's window, the aligned window for Y and the chroma span for
    Cr and Cb."""
    c = (plan.ch // 8) * (plan.cw // 8) * 63
    return [((plan.Y1 - plan.Y0) // 8) * ((plan.X1 - plan.X0) // 8) * 63, c, c]


def region_capacity(H, W, max_h, max_w):
    """((rows, columns) of the largest aligned window, (rows, columns) of the largest
    chroma span) any request (h, w) <= (max_h, max_w) of an H x W image can plan: an
    unaligned origin adds up to 15 pixels before rounding up to 16; the chroma span is
    half the window plus one halo block of 8 on each side."""
    wh, ww = min(H, -(-(max_h + 15) // 16) * 16), min(W, -(-(max_w + 15) // 16) * 16)
    return (wh, ww), (min(H // 2, wh // 2 + 16), min(W // 2, ww // 2 + 16))


class RegionDecoder:
    """Decoder.decode(index=...)[y0:y0+h, x0:x0+w] without the rest of the image: only
    the tiles holding the window's blocks are decoded (the window forms of the fused
    tile decoders), into buffers sized for the largest window a request of at most
    max_h x max_w can need (region_capacity): RGB plus the two chroma planes."""

    def __init__(self, H, W, max_h, max_w):
        device.require_gpu()
        if H % 16 or W % 16 or H < 16 or W < 16:
            raise ValueError("region decode needs H, W multiples of 16")
        if not (1 <= max_h <= H and 1 <= max_w <= W):
            raise ValueError("max_h, max_w must lie in the image")
        self.H, self.W, self.max_h, self.max_w = H, W, max_h, max_w
        (wh, ww), (ch, cw) = region_capacity(H, W, max_h, max_w)
        self.rgb = device.empty((wh * ww * 3,), torch.uint8)
        self.cr = device.empty((ch * cw,), torch.uint8)
        self.cb = device.empty((ch * cw,), torch.uint8)
        self.status = device.zeros((3,), torch.int64)
        self.plan = None

    def decode(self, y0, x0, h, w, sym_len, sym_val, counts, dc, index, stream=None):
        """The stream arguments as Decoder.decode(index=...): an Encoder(index=True)'s
        (or stream_index's) tile index with the contiguous symbols, or a SlotIndex;
        counts the device count tensor (3,).  Returns a device view (h, w, 3) of the
        window buffer, valid until the next decode; no host syncs."""
        if h > self.max_h or w > self.max_w:
            raise ValueError("window %d x %d exceeds this decoder's %d x %d" % (h, w, self.max_h, self.max_w))
        plan = window_plan(self.H, self.W, y0, x0, h, w)
        s = device.stream_ptr(stream)
        slots = isinstance(index, SlotIndex)
        kind = _lib.STREAM_SLOTS if slots else _lib.STREAM_INDEXED
        if slots:
            sym_len, sym_val = index.slot_len, index.slot_val
        y, cr, cb = (stream_addresses(sym_len, sym_val, counts, dc, index, i, k) for i, k in enumerate(CHANNELS))
        st = [self.status.data_ptr() + 8 * i for i in range(3)]
        win = plan.c_struct()
        # the windows are packed: pitch = the window's own width
        _lib.call("hic_rle_decode_idct_u8_window_pair", kind, *map(_two, cr, cb),
                  index.rpt["cr"] if slots else 0, self.H, self.W, ctypes.byref(win),
                  _two(self.cr.data_ptr(), self.cb.data_ptr()), plan.cw, _two(st[1], st[2]), s)
        Ww = plan.X1 - plan.X0
        _lib.call("hic_rle_decode_idct_rgb_window", kind, *y, index.rpt["lum"] if slots else 0, self.H,
                  self.W, ctypes.byref(win), self.cr.data_ptr(), self.cb.data_ptr(), plan.cw, self.rgb.data_ptr(),
                  3 * Ww, st[0], s)
        self.plan = plan
        return self.window()[y0 - plan.Y0:y0 - plan.Y0 + h, x0 - plan.X0:x0 - plan.X0 + w]

    def window(self):
        """The last decode's aligned window, a (Y1 - Y0, X1 - X0, 3) view."""
        p = self.plan
        n = (p.Y1 - p.Y0) * (p.X1 - p.X0) * 3
        return self.rgb[:n].view(p.Y1 - p.Y0, p.X1 - p.X0, 3)

    def chroma(self):
        """The last decode's chroma span: (cr, cb) views of shape (ch, cw)."""
        p = self.plan
        return tuple(b[:p.ch * p.cw].view(p.ch, p.cw) for b in (self.cr, self.cb))

    def expected_status(self):
        """What a good decode leaves in self.status (window_status of the last plan)."""
        return window_status(self.plan)

    def check_status(self):
        """Raise if a channel's symbol count was a failed encode's (status -1; syncs).
        A window does not see the whole stream: its completeness is stream_index's
        status, or the encoder's."""
        st = self.status.cpu().tolist()
        if st != self.expected_status():
            raise ValueError("region decode status %r, expected %r" % (st, self.expected_status()))


# ------------------------------------------------------------------ batched region decode
def batch_region_eligible(n, H, W, h, w, slots=False):
    """Whether BatchRegionDecoder takes an h x w window from each of n images of H x W
    (hic_decode_window_batch_table's limits): what batch_decode_eligible asks of n, H, W
    (and of the planes' records for slot-layout sources), 1 <= h <= H, 1 <= w <= W, and
    a chroma window buffer (region_capacity) below 2^31 bytes."""
    if not batch_decode_eligible(n, H, W, slots=slots):
        return False
    if not (1 <= h <= H and 1 <= w <= W) or 3 * w >= 2**31:
        return False
    (wh, ww), (ch, cw) = region_capacity(H, W, h, w)
    if ch >= 2**31 // cw:
        return False
    # the most waves per image either launch can need (a run of L blocks touches at most
    # (L + 62) // 64 + 1 tiles), in 32-bit wave counts
    ty = wh // 8 * min((ww // 8 + 62) // 64 + 1, -(-_nblk(H, W) // 64))
    tc = 2 * (ch // 8 * min((cw // 8 + 62) // 64 + 1, -(-_nblk(H // 2, W // 2) // 64)))
    return n * max(ty, tc) + 3 <= 2**31 - 1


class BatchRegionDecoder(_DecodeSources):
    """RegionDecoder.decode of one window per image, n images of one shape, in TWO
    launches (hic_decode420_window_batch_u8): every image's chroma span into its chroma
    window buffer, then every image's Y tiles of its aligned covering window straight to
    RGB, the store cropped to the request -- no aligned scratch window and no copies to
    form one tensor.  The windows share their size h x w; each image has its own origin.
    out (n, h, w, 3): out[i] equals Decoder(H, W).decode(index=...)[y0:y0+h, x0:x0+w] of
    image i bit for bit.  cr / cb (n, rows, pitch): the chroma window buffers, each of
    region_capacity's size; status (n, 3).  out=: a caller's (n, h, w, 3) uint8 device
    view to decode into (dense pixels, any row and image strides, any alignment)."""

    def __init__(self, n, H, W, h, w, out=None):
        if not batch_region_eligible(n, H, W, h, w):
            raise ValueError("a region decode batch needs 1 <= n <= %d images with H and W multiples of 16 and a "
                             "window of 1..H x 1..W" % DECODE_BATCH_MAX)
        device.require_gpu()
        self.n, self.H, self.W, self.h, self.w = n, H, W, h, w
        if out is None:
            out = device.empty((n, h, w, 3), torch.uint8)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8
                  and tuple(out.shape) == (n, h, w, 3) and out.stride(3) == 1 and out.stride(2) == 3
                  and out.stride(1) >= 3 * w and (n == 1 or out.stride(0) >= (h - 1) * out.stride(1) + 3 * w)):
            raise ValueError("out must be a (%d, %d, %d, 3) uint8 device tensor of dense pixels" % (n, h, w))
        self.out = out
        _, (ch, cw) = region_capacity(H, W, h, w)
        self.cr = device.empty((n, ch, cw), torch.uint8)
        self.cb = device.empty((n, ch, cw), torch.uint8)
        self.status = device.zeros((n, 3), torch.int64)
        self.origins = None
        nbytes = _lib.load().hic_decode_window_batch_table_bytes(n)
        # the table's host copy is pinned, so its upload is one queued DMA; _sent guards
        # the host copy against being rewritten while that DMA still reads it
        self._h_table = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self._d_table = device.empty((nbytes,), torch.uint8)
        self._sent = None
        self._images = None

    def decode(self, sources, origins, stream=None):
        """sources as BatchDecoder.decode takes them (a BatchEncoder, n Encoders, or n
        tuples (sym_len, sym_val, counts, dc, index)), all of one kind; origins: n (y0,
        x0) pairs.  The sources' 15 n addresses are read again only when the sources are
        not the previous call's objects; every call plans the n windows afresh
        (hic_decode_window_batch_table, microseconds on the host), uploads the table
        (the call's one host-to-device copy) and makes the two launches.  Nothing is
        read back.  Returns self.out."""
        new = self._resolve(sources)
        n, H, W, h, w = self.n, self.H, self.W, self.h, self.w
        if new is not None:
            (slots, addrs), remember = new
            if slots and not batch_region_eligible(n, H, W, h, w, slots=True):
                raise ValueError("slot-layout sources need planes of whole records")
            images = self._decode_images(addrs, (self.out, self.cr, self.cb))
            self._key, self._objs, self._images = (slots, addrs), remember, images
        origins = [(int(y0), int(x0)) for y0, x0 in origins]
        if len(origins) != n:
            raise ValueError("%d origins for a batch of %d" % (len(origins), n))
        flat = (ctypes.c_int64 * (2 * n))(*(v for o in origins for v in o))
        if self._sent is not None:
            self._sent.synchronize()
        _lib.call("hic_decode_window_batch_table", _lib.STREAM_SLOTS if self._key[0] else _lib.STREAM_INDEXED, n, H, W,
                  h, w, self._images, flat, self.out.stride(1), self.cr.stride(1), self.cr.shape[1],
                  self._h_table.data_ptr(), self._h_table.numel())
        with device.on_stream(stream):
            self._d_table.copy_(self._h_table, non_blocking=True)
            self._sent = torch.cuda.Event()
            self._sent.record()
        _lib.call("hic_decode420_window_batch_u8", self._h_table.data_ptr(), device.ptr(self._d_table),
                  device.stream_ptr(stream))
        self.origins = origins
        return self.out

    def plans(self):
        """The last decode's window_plan per image."""
        return [window_plan(self.H, self.W, y0, x0, self.h, self.w) for y0, x0 in self.origins]

    def expected_status(self):
        """What a good decode leaves in self.status: per image, 63 per block of each
        launch's window (window_status)."""
        return [window_status(p) for p in self.plans()]

    def check_status(self):
        """Raise if a channel's symbol count of any image was a failed encode's (status
        -1; one read, syncs).  A window does not see the whole stream: its completeness
        is stream_index's status, or the encoder's."""
        st, want = self.status.cpu().tolist(), self.expected_status()
        for i, (got, exp) in enumerate(zip(st, want)):
            if got != exp:
                raise ValueError("image %d: region decode status %r, expected %r" % (i, got, exp))


def stream_index(sym_len, sym_val, counts, dc, H, W, stream=None):
    """The tile index of bare contiguous streams (hic_rle_stream_index_i16): per channel
    the three int64 words per 64-block tile an Encoder(index=True) writes, built from
    the symbols and DC differences alone -- a Huffman-decoded .hic can then take
    Decoder.decode(index=...) and RegionDecoder.  counts: host ints per channel.
    Returns ({channel: index tensor}, status (3,) int64 on the device: per channel
    what the un-indexed decode would report, nblk * 63 for a whole stream)."""
    lib = _lib.load()
    s = device.stream_ptr(stream)
    if isinstance(counts, torch.Tensor):
        counts = counts.cpu().tolist()
    status = device.zeros((3,), torch.int64)
    index = {}
    with device.on_stream(stream):
        for i, k in enumerate(CHANNELS):
            n = _nblk(*((H, W) if k == "lum" else (H // 2, W // 2)))
            nsym = int(counts[i])
            index[k] = device.empty((3 * -(-n // 64),), torch.int64)
            ws = device.workspace(lib.hic_rle_stream_index_workspace_bytes(nsym, n))
            _lib.call("hic_rle_stream_index_i16", device.ptr(sym_len[k]), device.ptr(sym_val[k]), nsym,
                      device.ptr(dc[k]), n, device.ptr(index[k]), device.ptr(status[i:i + 1]), device.ptr(ws), s)
    return index, status
