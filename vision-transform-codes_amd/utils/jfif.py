"""
Baseline JFIF files written on the device: a JPEG any decoder opens.

utils.jpeg keeps the reference's pseudo-JPEG (AC part before DC, no DC
prediction, an end of block after a full block, unlimited codeword lengths);
its streams measure a length.  This module writes the standard's: ITU-T T.81
sequential DCT with Huffman coding, 8-bit samples, inside a JFIF 1.01 wrapper,
so the JPEG point of a rate-distortion curve is the size of a file that
libjpeg opens.  The reference has no such path; the rules are this project's
own statement of T.81 and are given to the operation in DESIGN.md 4.23.

The per-block work -- level shift, 8 x 8 DCT and quantisation, run-length
symbols with DC prediction and their counts, block lengths, the bit-contiguous
entropy-coded segment, 0xFF byte stuffing, and the way back from levels to
samples -- runs in the kernels of csrc/jfif.hip behind include/ext/vtc_jfif.h.
The Huffman tables (length-limited to 16 bits by package-merge, at most 256
symbols each) are built here on the host from the device counts, as utils.jpeg
builds its own; so are the scan geometry and the header segments.

The way back from the bytes -- decode_bytes, read_jpeg,
rate_distortion_image(from_stream=True) -- opens one baseline file, this
module's or another encoder's: the markers are walked here on the host
(parse_headers, frame_layout), byte unstuffing, the self-synchronising
parallel Huffman decode and the DC scan run in the kernels of
csrc/jfif_decode.hip behind include/ext/vtc_jfif_decode.h, and the planes come
from the inverse DCT above.  DESIGN.md 4.24.

Planes are (h, w) float32 device tensors holding samples in [0, 255]; images
are (h, w) or (h, w, 3) float32 device tensors.  A wrong shape raises
ValueError, a CPU tensor VtcHipError, a level beyond the baseline sizes (10
bits AC, 11 bits DC difference) ValueError, a symbol the tables lack KeyError
with its spelling as in utils.jpeg.
"""
import re

import numpy as np
import torch

import vtc_hip
from utils import jpeg
from utils import matrix_zigzag

MAX_CODE_BITS = 16
PAIR_SYMBOLS = 272   # symbol ids of include/ext/vtc_jfif.h: 272 t + id


# ------------------------------------------------------------ Huffman tables
def length_limited_lengths(counts, max_len=MAX_CODE_BITS,
                           reserve_all_ones=True):
  """Optimal codeword lengths under a length limit, by package-merge.

  counts : non-negative integers, one per symbol
  max_len : the longest codeword allowed
  reserve_all_ones : a pseudo-symbol of weight 0 takes part and receives a
      longest code; canonical_codes places it last, so no real symbol is
      assigned the all-ones codeword (T.81 Annex C)

  Returns int64 lengths, 0 for a symbol of count 0.  Integers only.  Leaves
  are ordered by (weight, symbol value), the pseudo-symbol first, and when a
  leaf and a package weigh the same the leaf comes first: the result is a
  function of the counts alone.  ValueError when the symbols do not fit under
  the limit.
  """
  counts = [int(c) for c in np.asarray(counts).reshape(-1)]
  if any(c < 0 for c in counts):
    raise ValueError('counts must be non-negative')
  max_len = int(max_len)
  lengths = np.zeros(len(counts), dtype=np.int64)
  used = [s for s, c in enumerate(counts) if c > 0]
  if not used:
    return lengths
  # (weight, symbol); the pseudo-symbol is symbol len(counts), weight 0, so it
  # sorts before every real symbol (real weights are at least 1)
  leaves = sorted((counts[s], s) for s in used)
  if reserve_all_ones:
    leaves.insert(0, (0, len(counts)))
  n = len(leaves)
  if max_len < 1 or n > (1 << max_len):
    raise ValueError('%d codewords do not fit under %d bits' % (n, max_len))
  if n == 1:
    lengths[leaves[0][1]] = 1
    return lengths
  # an item is (weight, leaf indices it contains)
  singles = [(w, (i,)) for i, (w, _) in enumerate(leaves)]
  items = singles
  for _ in range(max_len - 1):
    packages = [(items[j][0] + items[j + 1][0], items[j][1] + items[j + 1][1])
                for j in range(0, len(items) - 1, 2)]
    merged, a, b = [], 0, 0
    while a < n or b < len(packages):
      if b == len(packages) or (a < n and singles[a][0] <= packages[b][0]):
        merged.append(singles[a])
        a += 1
      else:
        merged.append(packages[b])
        b += 1
    items = merged
  depth = [0] * n
  for _, members in items[:2 * n - 2]:
    for i in members:
      depth[i] += 1
  for i, (_, s) in enumerate(leaves):
    if s < len(counts):
      lengths[s] = depth[i]
  return lengths


def canonical_codes(lengths):
  """The code of T.81 Annex C for codeword lengths (0 = symbol absent):
  codewords in ascending order of (length, symbol value).

  Returns (codes, BITS, HUFFVAL): codes uint16, one per symbol, the codeword
  in the low `length` bits; BITS the 16 counts of codewords of length 1 .. 16;
  HUFFVAL the symbols in code order.  This is what the device arrays and the
  DHT segment are both built from."""
  lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
  if lengths.size and (lengths.min() < 0 or lengths.max() > MAX_CODE_BITS):
    raise ValueError('codeword lengths must be in 0 .. %d' % MAX_CODE_BITS)
  codes = np.zeros(lengths.shape[0], dtype=np.uint16)
  bits = [0] * MAX_CODE_BITS
  huffval = []
  code = 0
  for length in range(1, MAX_CODE_BITS + 1):
    for symbol in np.flatnonzero(lengths == length):
      if code >> length:
        raise ValueError('lengths violate the Kraft inequality')
      codes[symbol] = code
      code += 1
      bits[length - 1] += 1
      huffval.append(int(symbol))
    code <<= 1
  return codes, bits, huffval


# ------------------------------------------------------ quantisation tables
def _scaled_table(base, quality):
  quality = int(quality)
  if not 1 <= quality <= 100:
    raise ValueError('quality must be in 1 .. 100, got %r' % (quality,))
  scale = 5000 // quality if quality < 50 else 200 - 2 * quality
  table = (np.asarray(base, dtype=np.int64) * scale + 50) // 100
  return np.clip(table, 1, 255).astype(np.uint16)


def _checked_table(table):
  t = np.asarray(table)
  if t.size != 64 or not np.issubdtype(t.dtype, np.integer) or (
      t.min() < 1 or t.max() > 255):
    raise ValueError('a quantisation table is 64 integers in 1 .. 255, in '
                     'zig-zag order')
  return np.ascontiguousarray(t.reshape(64).astype(np.uint16))


def quality_tables(quality):
  """(luma, chroma) uint16[64] tables in zig-zag order: libjpeg's scaling of
  Annex K.1 and K.2, scale = 5000 // q below 50 and 200 - 2 q from 50 on,
  (base * scale + 50) // 100 clamped to 1 .. 255.  Tables given in place of a
  quality -- one array of 64 integers in 1 .. 255 for both, or a (luma,
  chroma) pair -- are checked and returned."""
  if not isinstance(quality, (int, np.integer)):
    if isinstance(quality, np.ndarray) and quality.ndim == 1:
      return _checked_table(quality), _checked_table(quality)
    try:
      luma, chroma = quality
    except (TypeError, ValueError):
      raise ValueError('quality must be an integer in 1 .. 100, one table or '
                       'a (luma, chroma) pair of tables')
    return _checked_table(luma), _checked_table(chroma)
  # get_jpeg_quant_hifi_binwidths is Annex K.1: at quality 50 it is the table
  # libjpeg writes (tests/test_jfif_host.py)
  return (_scaled_table(jpeg.get_jpeg_quant_hifi_binwidths(), quality),
          _scaled_table(jpeg.get_jpeg_quant_chroma_binwidths(), quality))


# ------------------------------------------------------------ scan geometry
def _subsampling(subsampling):
  if subsampling is None:
    return None
  try:
    fv, fh = (int(f) for f in subsampling)
  except (TypeError, ValueError):
    raise ValueError('subsampling must be None, (1, 1) or (2, 2), got %r'
                     % (subsampling,))
  if (fv, fh) not in ((1, 1), (2, 2)):
    raise NotImplementedError(
        'subsampling %r: only 4:4:4 (1, 1) and 4:2:0 (2, 2) are written'
        % ((fv, fh),))
  return fv, fh


def scan_layout(shape, subsampling=None):
  """The geometry of one scan, in numpy on the host.

  shape : (h, w) of the image
  subsampling : None for one gray plane, (1, 1) for YCbCr 4:4:4, (2, 2) for
      YCbCr 4:2:0

  Returns a dict: 'rows' (blocks in the scan), 'plane_shapes' [(h, w)] and
  'grids' [(bh, bw)] (the padded block grid of each plane), 'sampling'
  [(H, V)] of each component, 'row_of_block' [int32 (bh * bw,)] (the row of
  the levels array that holds block (by, bx) of each plane, rows being in MCU
  order: for 4:2:0 Y00 Y01 Y10 Y11 Cb Cr), and per row 'component' uint8,
  'table_sel' uint8 (0 for Y, 1 for Cb and Cr) and 'pred' int32 (the row of
  the previous block of the same component in scan order, -1 for the first).
  """
  try:
    h, w = (int(v) for v in shape)
  except (TypeError, ValueError):
    raise ValueError('shape must be (h, w), got %r' % (shape,))
  if not (1 <= h <= 65535 and 1 <= w <= 65535):
    raise ValueError('a JFIF image is 1 .. 65535 pixels a side, got %r'
                     % ((h, w),))
  factors = _subsampling(subsampling)
  if factors is None:
    sampling = [(1, 1)]
  else:
    sampling = [(factors[1], factors[0]), (1, 1), (1, 1)]
  hmax = max(s[0] for s in sampling)
  vmax = max(s[1] for s in sampling)
  mcus_v, mcus_h = -(-h // (8 * vmax)), -(-w // (8 * hmax))
  per_mcu = sum(sh * sv for sh, sv in sampling)
  rows = mcus_v * mcus_h * per_mcu
  my, mx = np.meshgrid(np.arange(mcus_v), np.arange(mcus_h), indexing='ij')
  mcu_base = (my * mcus_h + mx) * per_mcu
  component = np.zeros(rows, dtype=np.uint8)
  pred = np.full(rows, -1, dtype=np.int32)
  plane_shapes, grids, row_of_block = [], [], []
  first = 0   # the component's first row inside an MCU
  for c, (sh, sv) in enumerate(sampling):
    plane_shapes.append((-(-h * sv // vmax), -(-w * sh // hmax)))
    bh, bw = mcus_v * sv, mcus_h * sh
    grids.append((bh, bw))
    rob = np.zeros((bh, bw), dtype=np.int32)
    for dy in range(sv):
      for dx in range(sh):
        rob[dy::sv, dx::sh] = mcu_base + first + dy * sh + dx
    row_of_block.append(rob.reshape(-1))
    mine = np.sort(rob.reshape(-1))   # the component's rows in scan order
    component[mine] = c
    pred[mine[1:]] = mine[:-1]
    first += sh * sv
  return {'shape': (h, w), 'subsampling': factors, 'rows': rows,
          'plane_shapes': plane_shapes, 'grids': grids, 'sampling': sampling,
          'row_of_block': row_of_block, 'component': component,
          'table_sel': (component > 0).astype(np.uint8), 'pred': pred}


def dct_basis():
  """float64 (8, 8): basis[u, k] = c(u) / 2 * cos((2 k + 1) u pi / 16),
  c(0) = 1 / sqrt(2), c(u > 0) = 1."""
  u = np.arange(8, dtype=np.float64)[:, None]
  k = np.arange(8, dtype=np.float64)[None, :]
  scale = np.where(u == 0, 1.0 / np.sqrt(2.0), 1.0)
  return scale / 2.0 * np.cos((2.0 * k + 1.0) * u * np.pi / 16.0)


# ------------------------------------------------------------- device calls
def _upload(array, device):
  return torch.from_numpy(np.ascontiguousarray(array)).to(device)


def _levels(levels):
  levels = vtc_hip.require_device_tensor(levels, 'levels', torch.int32)
  if levels.dim() != 2 or levels.shape[1] != 64 or levels.shape[0] < 1:
    raise ValueError('levels must be (d, 64) with d >= 1, got shape %s'
                     % (tuple(levels.shape),))
  return levels.contiguous()


def _plane(plane, name='plane'):
  if not torch.is_tensor(plane):
    raise TypeError('%s must be a torch.Tensor' % name)
  if plane.dim() != 2 or 0 in plane.shape:
    raise ValueError('%s must be (h, w), got shape %s'
                     % (name, tuple(plane.shape)))
  return vtc_hip.require_device_tensor(plane, name).contiguous()


def _rows_arguments(pred, table_sel, d, device):
  """(pred int32[d], table_sel uint8[d]) on the device; a pair that an earlier
  call already uploaded passes through."""
  if torch.is_tensor(pred) and torch.is_tensor(table_sel):
    pred = vtc_hip.require_device_tensor(pred, 'pred', torch.int32)
    table_sel = vtc_hip.require_device_tensor(table_sel, 'table_sel',
                                              torch.uint8)
    if tuple(pred.shape) != (d,) or tuple(table_sel.shape) != (d,):
      raise ValueError('pred and table_sel must have one entry per row (%d)'
                       % d)
    return pred.contiguous(), table_sel.contiguous()
  pred = np.ascontiguousarray(pred, dtype=np.int32).reshape(-1)
  table_sel = np.ascontiguousarray(table_sel, dtype=np.uint8).reshape(-1)
  if pred.shape[0] != d or table_sel.shape[0] != d:
    raise ValueError('pred and table_sel must have one entry per row (%d), '
                     'got %d and %d' % (d, pred.shape[0], table_sel.shape[0]))
  return _upload(pred, device), _upload(table_sel, device)


def symbol_of_id(symbol_id):
  """The spelling of a symbol id of include/ext/vtc_jfif.h: utils.jpeg's
  spelling, with the table pair in front."""
  pair, local = divmod(int(symbol_id), PAIR_SYMBOLS)
  return '%d:%s' % (pair, jpeg._symbol_of_id(local))


def _raise_status(over, missing, what):
  if over:
    raise ValueError(
        '%s: %d levels beyond the baseline sizes (10 bits AC, 11 bits DC '
        'difference) or stream bits outside the output' % (what, over))
  if missing:
    raise KeyError(symbol_of_id(missing - 1))


def forward_dct(plane, grid, qtable, row_of_block, levels):
  """Writes the quantiser levels of `plane`, padded to grid = (bh, bw) blocks
  by replication, into the rows of `levels` that row_of_block names.  Only
  enqueues."""
  lib = vtc_hip.load_library()
  plane = _plane(plane)
  if _levels(levels) is not levels:
    raise ValueError('levels must be contiguous: it is written in place')
  device = plane.device
  h, w = plane.shape
  bh, bw = (int(v) for v in grid)
  rob = np.ascontiguousarray(row_of_block, dtype=np.int32).reshape(-1)
  if rob.shape[0] != bh * bw:
    raise ValueError('row_of_block must have %d entries, got %d'
                     % (bh * bw, rob.shape[0]))
  # uint16 as int16 bits: torch moves bytes
  basis = _upload(dct_basis(), device)
  q = _upload(_checked_table(qtable).view(np.int16), device)
  rob = _upload(rob, device)
  vtc_hip.check(lib.vtc_jfif_forward_dct(
      vtc_hip.ptr(plane), h, w, bh, bw, vtc_hip.ptr(basis), vtc_hip.ptr(q),
      vtc_hip.ptr(rob), vtc_hip.ptr(levels), levels.shape[0],
      vtc_hip.current_stream(device)), 'vtc_jfif_forward_dct')
  return levels


def inverse_dct(levels, shape, grid, qtable, row_of_block):
  """The (h, w) float32 plane a decoder shows for `levels`: dequantise,
  inverse DCT, level shift, round, clamp to [0, 255], crop.  Only enqueues."""
  lib = vtc_hip.load_library()
  levels = _levels(levels)
  device = levels.device
  h, w = (int(v) for v in shape)
  bh, bw = (int(v) for v in grid)
  rob = np.ascontiguousarray(row_of_block, dtype=np.int32).reshape(-1)
  if rob.shape[0] != bh * bw:
    raise ValueError('row_of_block must have %d entries, got %d'
                     % (bh * bw, rob.shape[0]))
  if h < 1 or w < 1:
    raise ValueError('shape must be (h, w), got %r' % (shape,))
  plane = torch.empty((h, w), dtype=torch.float32, device=device)
  basis = _upload(dct_basis(), device)
  q = _upload(_checked_table(qtable).view(np.int16), device)
  rob = _upload(rob, device)
  vtc_hip.check(lib.vtc_jfif_inverse_dct(
      vtc_hip.ptr(levels), levels.shape[0], vtc_hip.ptr(rob), bh, bw,
      vtc_hip.ptr(basis), vtc_hip.ptr(q), vtc_hip.ptr(plane), h, w,
      vtc_hip.current_stream(device)), 'vtc_jfif_inverse_dct')
  return plane


def symbol_counts(levels, pred, table_sel):
  """(ac_counts int64 (2, 256), dc_counts int64 (2, 16)) as numpy arrays: how
  often each T.81 symbol occurs under each table pair.  One host read."""
  lib = vtc_hip.load_library()
  levels = _levels(levels)
  d, device = levels.shape[0], levels.device
  pred_dev, sel_dev = _rows_arguments(pred, table_sel, d, device)
  # counts and, behind them, the two status words as one int64: one read
  out = torch.empty(2 * 256 + 2 * 16 + 1, dtype=torch.int64, device=device)
  status = out[-1:].view(torch.int32)
  vtc_hip.check(lib.vtc_jfif_symbol_counts(
      vtc_hip.ptr(levels), d, vtc_hip.ptr(pred_dev), vtc_hip.ptr(sel_dev),
      vtc_hip.ptr(out), vtc_hip.ptr(out[512:]), vtc_hip.ptr(status),
      vtc_hip.current_stream(device)), 'vtc_jfif_symbol_counts')
  host = out.cpu().numpy()
  over, missing = host[-1:].view(np.int32).tolist()
  _raise_status(over, missing, 'symbol_counts')
  return host[:512].reshape(2, 256).copy(), host[512:544].reshape(2, 16).copy()


def tables_from_counts(ac_counts, dc_counts):
  """The Huffman tables of a scan from the counts of symbol_counts: a list of
  two pairs {'dc': lengths int64[16], 'ac': lengths int64[256]}, each
  length-limited to 16 bits with the all-ones codeword reserved; a pair that
  no row selects is None.  The tables hold the symbols of this image only."""
  ac_counts = np.asarray(ac_counts).reshape(2, 256)
  dc_counts = np.asarray(dc_counts).reshape(2, 16)
  tables = []
  for pair in range(2):
    if not dc_counts[pair].any() and not ac_counts[pair].any():
      tables.append(None)
      continue
    tables.append({'dc': length_limited_lengths(dc_counts[pair]),
                   'ac': length_limited_lengths(ac_counts[pair])})
  return tables


class _DeviceTables(object):
  """uint16 codes and uint8 lengths of both pairs, as the kernels read them."""

  def __init__(self, tables, device):
    ac_code = np.zeros((2, 256), dtype=np.uint16)
    dc_code = np.zeros((2, 16), dtype=np.uint16)
    ac_len = np.zeros((2, 256), dtype=np.uint8)
    dc_len = np.zeros((2, 16), dtype=np.uint8)
    if len(tables) != 2:
      raise ValueError('tables must be a list of two pairs (or None)')
    for pair, table in enumerate(tables):
      if table is None:
        continue
      for key, code, length, size in (('ac', ac_code, ac_len, 256),
                                      ('dc', dc_code, dc_len, 16)):
        lengths = np.asarray(table[key], dtype=np.int64).reshape(-1)
        if lengths.shape[0] != size:
          raise ValueError('%s lengths must have %d entries, got %d'
                           % (key, size, lengths.shape[0]))
        code[pair] = canonical_codes(lengths)[0]
        length[pair] = lengths
    # uint16 as int16 bits: torch moves bytes
    self.ac_code = _upload(ac_code.view(np.int16), device)
    self.dc_code = _upload(dc_code.view(np.int16), device)
    self.ac_len, self.dc_len = _upload(ac_len, device), _upload(dc_len, device)


def scan_bits_from_counts(ac_counts, dc_counts, tables):
  """Bits of the entropy-coded segment before padding, from the counts: every
  symbol costs its codeword and its size in value bits."""
  total = 0
  for pair, table in enumerate(tables):
    if table is None:
      continue
    for symbol in range(256):
      total += int(ac_counts[pair][symbol]) * (int(table['ac'][symbol]) +
                                               (symbol & 15))
    for category in range(16):
      total += int(dc_counts[pair][category]) * (int(table['dc'][category]) +
                                                 category)
  return total


def _pack(lib, levels, pred_dev, sel_dev, tables, raw_bytes, meta):
  """Enqueues block bits, offsets and the pack into a fresh raw tensor.  meta
  int32[8]: [0:2] the status of the bits call, [2:4] that of the pack."""
  d, device = levels.shape[0], levels.device
  stream = vtc_hip.current_stream(device)
  dev = _DeviceTables(tables, device)
  bits = torch.empty(d, dtype=torch.int32, device=device)
  vtc_hip.check(lib.vtc_jfif_block_bits(
      vtc_hip.ptr(levels), d, vtc_hip.ptr(pred_dev), vtc_hip.ptr(sel_dev),
      vtc_hip.ptr(dev.ac_len), vtc_hip.ptr(dev.dc_len), vtc_hip.ptr(bits),
      vtc_hip.ptr(meta[0:2]), stream), 'vtc_jfif_block_bits')
  offsets = jpeg.bit_offsets(bits)
  if raw_bytes is None:   # one host read
    raw_bytes = -(-int(offsets[d]) // 8)
  raw = torch.empty(max(1, raw_bytes), dtype=torch.uint8, device=device)
  vtc_hip.check(lib.vtc_jfif_pack(
      vtc_hip.ptr(levels), d, vtc_hip.ptr(pred_dev), vtc_hip.ptr(sel_dev),
      vtc_hip.ptr(dev.ac_code), vtc_hip.ptr(dev.ac_len),
      vtc_hip.ptr(dev.dc_code), vtc_hip.ptr(dev.dc_len), vtc_hip.ptr(offsets),
      vtc_hip.ptr(raw), raw.numel(), vtc_hip.ptr(meta[2:4]), stream),
                'vtc_jfif_pack')
  return raw[:raw_bytes], offsets


def pack_scan(levels, pred, table_sel, tables):
  """(raw, offsets): the entropy-coded segment of the (d, 64) int32 device
  `levels` before byte stuffing -- a uint8 device tensor, most significant bit
  first, the last byte padded with ones -- and the (d + 1,) int64 device
  tensor of the bit at which each block starts, the total last.  tables as
  tables_from_counts returns them.  ValueError for a level beyond the baseline
  sizes, KeyError for a symbol the tables lack."""
  lib = vtc_hip.load_library()
  levels = _levels(levels)
  d, device = levels.shape[0], levels.device
  pred_dev, sel_dev = _rows_arguments(pred, table_sel, d, device)
  meta = torch.zeros(8, dtype=torch.int32, device=device)
  raw, offsets = _pack(lib, levels, pred_dev, sel_dev, tables, None, meta)
  status = meta.cpu().tolist()
  _raise_status(status[0], status[1], 'pack_scan')
  _raise_status(status[2], status[3], 'pack_scan')
  return raw, offsets


def _stuff(lib, raw, capacity, meta):
  """Enqueues the stuffing of `raw` into a fresh tensor of `capacity` bytes.
  meta int32[8]: [4] the dropped count, [6:8] out_len as one int64."""
  device = raw.device
  n = raw.numel()
  out = torch.empty(max(1, capacity), dtype=torch.uint8, device=device)
  ws = vtc_hip.workspace(lib.vtc_jfif_stuff_bytes_workspace_bytes(n), device)
  vtc_hip.check(lib.vtc_jfif_stuff_bytes(
      vtc_hip.ptr(raw) if n else None, n, vtc_hip.ptr(out), capacity,
      vtc_hip.ptr(meta[6:8]), vtc_hip.ptr(meta[4:5]), vtc_hip.ptr(ws),
      ws.numel(), vtc_hip.current_stream(device)), 'vtc_jfif_stuff_bytes')
  return out


def stuff_bytes(raw, capacity=None):
  """(out, length, dropped): `raw` (a uint8 device tensor) with 0x00 inserted
  after every 0xFF, as a uint8 device tensor of min(length, capacity) bytes;
  length is n + the number of 0xFF bytes; dropped the bytes that did not fit
  under `capacity` (None: room for all).  One host read."""
  lib = vtc_hip.load_library()
  raw = vtc_hip.require_device_tensor(raw, 'raw', torch.uint8)
  if raw.dim() != 1:
    raise ValueError('raw must be (n,), got shape %s' % (tuple(raw.shape),))
  raw = raw.contiguous()
  capacity = 2 * raw.numel() if capacity is None else int(capacity)
  if capacity < 0:
    raise ValueError('capacity must not be negative')
  meta = torch.zeros(8, dtype=torch.int32, device=raw.device)
  out = _stuff(lib, raw, capacity, meta)
  host = meta.cpu().numpy()
  length, dropped = int(host[6:8].view(np.int64)[0]), int(host[4])
  return out[:min(length, capacity)], length, dropped


# ------------------------------------------------------------------ headers
def _segment(marker, payload):
  return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + payload


def file_headers(layout, qtables, tables):
  """SOI, APP0 'JFIF' 1.01, one DQT per table (8-bit, zig-zag order), SOF0,
  one DHT per table used, SOS: everything in front of the entropy-coded
  segment."""
  h, w = layout['shape']
  sampling = layout['sampling']
  out = [b'\xff\xd8',
         _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')]
  for index, table in enumerate(qtables):
    out.append(_segment(0xDB, bytes([index]) + bytes(
        int(v) for v in _checked_table(table))))
  frame = bytes([8]) + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + bytes(
      [len(sampling)])
  for c, (sh, sv) in enumerate(sampling):
    frame += bytes([c + 1, sh << 4 | sv, min(c, len(qtables) - 1)])
  out.append(_segment(0xC0, frame))
  for pair, table in enumerate(tables):
    if table is None:
      continue
    for klass, key in ((0, 'dc'), (1, 'ac')):
      _, bits, huffval = canonical_codes(table[key])
      out.append(_segment(0xC4, bytes([klass << 4 | pair]) + bytes(bits) +
                          bytes(huffval)))
  scan = bytes([len(sampling)])
  for c in range(len(sampling)):
    pair = min(c, 1)
    scan += bytes([c + 1, pair << 4 | pair])
  out.append(_segment(0xDA, scan + bytes([0, 63, 0])))
  return b''.join(out)


# ----------------------------------------------------------------- encoding
def encode_planes(planes, shape, subsampling=None, quality=75, qtables=None):
  """The JFIF file of planes laid out as utils.color.split_planes lays them
  out: [Y] with subsampling None, [Y, Cb, Cr] with (1, 1) or (2, 2).

  shape : (h, w) of the image
  quality : 1 .. 100, libjpeg's scale; qtables, when given, is the (luma,
      chroma) pair of uint16 tables in 1 .. 255 (zig-zag order) used instead

  Forward DCT, counts, tables, bits, offsets, pack and stuffing run on the
  device, with one host read for the counts and one for the length of the
  stuffed segment.  Returns (bytes, info); info holds 'layout' (scan_layout),
  'levels' (the (rows, 64) int32 device tensor in scan order), 'qtables',
  'tables' (tables_from_counts), 'scan_bits' (entropy-coded bits before
  padding), 'stuffed_bytes' (0x00 bytes inserted), 'header_bytes' (everything
  but the stuffed segment, EOI included), 'file_bytes' and 'bits_per_pixel'
  (8 * file_bytes / (h * w): the whole file).
  """
  lib = vtc_hip.load_library()
  layout = scan_layout(shape, subsampling)
  planes = [_plane(p, 'planes[%d]' % i) for i, p in enumerate(planes)]
  want = layout['plane_shapes']
  if [tuple(p.shape) for p in planes] != want:
    raise ValueError('planes of shapes %s, expected %s'
                     % ([tuple(p.shape) for p in planes], want))
  luma, chroma = quality_tables(quality if qtables is None else qtables)
  qtables = [luma] if len(planes) == 1 else [luma, chroma]
  device = planes[0].device
  d = layout['rows']
  levels = torch.empty((d, 64), dtype=torch.int32, device=device)
  for c, plane in enumerate(planes):
    forward_dct(plane, layout['grids'][c], qtables[min(c, 1)],
                layout['row_of_block'][c], levels)
  pred_dev, sel_dev = _rows_arguments(layout['pred'], layout['table_sel'], d,
                                      device)
  ac_counts, dc_counts = symbol_counts(levels, pred_dev, sel_dev)
  tables = tables_from_counts(ac_counts, dc_counts)
  scan_bits = scan_bits_from_counts(ac_counts, dc_counts, tables)
  raw_bytes = -(-scan_bits // 8)
  meta = torch.zeros(8, dtype=torch.int32, device=device)
  raw, _ = _pack(lib, levels, pred_dev, sel_dev, tables, raw_bytes, meta)
  out = _stuff(lib, raw, 2 * raw_bytes, meta)
  host = meta.cpu().numpy()
  _raise_status(int(host[0]), int(host[1]), 'encode_planes')
  _raise_status(int(host[2]) + int(host[4]), int(host[3]), 'encode_planes')
  length = int(host[6:8].view(np.int64)[0])
  segment = out[:length].cpu().numpy().tobytes()
  head = file_headers(layout, qtables, tables)
  data = head + segment + b'\xff\xd9'
  h, w = layout['shape']
  info = {'layout': layout, 'levels': levels, 'qtables': qtables,
          'tables': tables, 'scan_bits': scan_bits,
          'stuffed_bytes': length - raw_bytes,
          'header_bytes': len(head) + 2, 'file_bytes': len(data),
          'bits_per_pixel': 8.0 * len(data) / (h * w)}
  return data, info


def _image(image, dims, what):
  if not torch.is_tensor(image):
    raise TypeError('image must be a torch.Tensor')
  shape = tuple(int(v) for v in image.shape)
  if len(shape) != dims or 0 in shape or (dims == 3 and shape[2] != 3):
    raise ValueError('image must be %s, got shape %s' % (what, shape))
  return vtc_hip.require_device_tensor(image, 'image')


def encode_gray(image, quality=75, qtables=None):
  """(bytes, info) of one (h, w) float32 device image with samples in
  [0, 255]: a one-component JFIF file."""
  image = _image(image, 2, '(h, w)')
  return encode_planes([image], image.shape, None, quality, qtables)


def encode_rgb(image, subsampling=(2, 2), quality=75, qtables=None):
  """(bytes, info) of one (h, w, 3) float32 RGB device image with samples in
  [0, 255]: YCbCr through utils.color.split_planes (JFIF matrix, box
  subsampling), three components, 4:2:0 by default or 4:4:4 with (1, 1)."""
  from utils import color
  factors = _subsampling(subsampling)
  if factors is None:
    raise ValueError('a colour image needs subsampling (1, 1) or (2, 2)')
  image = _image(image, 3, '(h, w, 3)')
  planes = color.split_planes(image, factors)
  return encode_planes(planes, image.shape[:2], factors, quality, qtables)


def write_jpeg(path, image, subsampling=(2, 2), quality=75, qtables=None):
  """Writes the file of a (h, w) or (h, w, 3) image to `path`; returns the
  info dict of the encoder."""
  if torch.is_tensor(image) and image.dim() == 2:
    data, info = encode_gray(image, quality, qtables)
  else:
    data, info = encode_rgb(image, subsampling, quality, qtables)
  with open(path, 'wb') as f:
    f.write(data)
  return info


# ----------------------------------------------------------------- decoding
def decode_levels(info):
  """What a decoder shows for the levels of an encoder's info dict: the
  (h, w) float32 plane of a gray file, or the (h, w, 3) RGB image of a colour
  one -- planes through vtc_jfif_inverse_dct, chroma back to full resolution
  with the triangle filter of utils.color.merge_planes, RGB clamped to
  [0, 255]."""
  from utils import color
  layout = info['layout']
  planes = [inverse_dct(info['levels'], layout['plane_shapes'][c],
                        layout['grids'][c], info['qtables'][min(c, 1)],
                        layout['row_of_block'][c])
            for c in range(len(layout['plane_shapes']))]
  if len(planes) == 1:
    return planes[0]
  return color.merge_planes(planes, layout['shape'], layout['subsampling'],
                            upsampling='triangle', clamp=(0.0, 255.0))


# ------------------------------------------------------------ reading a file
_SOF_NAMES = {0xC1: 'extended sequential DCT (SOF1)',
              0xC2: 'progressive DCT (SOF2)', 0xC3: 'lossless (SOF3)',
              0xC5: 'differential sequential DCT (SOF5)',
              0xC6: 'differential progressive DCT (SOF6)',
              0xC7: 'differential lossless (SOF7)',
              0xC9: 'arithmetic coding (SOF9)',
              0xCA: 'arithmetic coding, progressive (SOF10)',
              0xCB: 'arithmetic coding, lossless (SOF11)',
              0xCD: 'arithmetic coding, differential (SOF13)',
              0xCE: 'arithmetic coding, differential progressive (SOF14)',
              0xCF: 'arithmetic coding, differential lossless (SOF15)',
              0xCC: 'arithmetic coding (DAC)'}
_MARKER_IN_SEGMENT = re.compile(b'\xff[^\x00]')


def _huffman_table(counts, values, size):
  """(lengths int64[size], codes uint16[size]) of one DHT table: codewords in
  file order (T.81 Annex C)."""
  lengths = np.zeros(size, dtype=np.int64)
  codes = np.zeros(size, dtype=np.uint16)
  code, k = 0, 0
  for length in range(1, MAX_CODE_BITS + 1):
    for _ in range(counts[length - 1]):
      symbol = values[k]
      k += 1
      if symbol >= size:
        raise ValueError('DHT: symbol 0x%02x in a table of %d' % (symbol, size))
      if lengths[symbol]:
        raise ValueError('DHT: symbol 0x%02x twice' % symbol)
      if code >> length:
        raise ValueError('DHT: lengths violate the Kraft inequality')
      lengths[symbol], codes[symbol] = length, code
      code += 1
    code <<= 1
  return lengths, codes


def parse_headers(data):
  """Walks the markers of a baseline JFIF file up to its SOS, on the host.

  Returns a dict: 'shape' (h, w); 'components' [(id, H, V, Tq)] in frame
  order; 'sampling' [(H, V)] as frame_layout takes it (a one-component file is
  (1, 1) whatever it says: its scan is not interleaved); 'qtables' {Tq:
  uint16[64] in zig-zag order}; 'tables', a list of two pairs {'dc': lengths
  int64[16], 'ac': lengths int64[256], 'dc_codes', 'ac_codes': uint16
  codewords in the file's order} as canonical_codes and _DeviceTables index
  them (None for an id the file does not define); 'selectors' [(Td, Ta)] per
  scan component; 'segment_at', the offset of the entropy-coded segment.

  ValueError for what is not a JPEG, is truncated or refers to a missing
  table; NotImplementedError, naming the feature, for what T.81 allows and
  this reader leaves out."""
  data = bytes(data)
  if data[:2] != b'\xff\xd8':
    raise ValueError('not a JPEG file: no SOI marker')
  at = 2
  qtables, frame, restart = {}, None, 0
  huffman = {}   # (class, id) -> (lengths, codes)
  adobe_transform = None
  while True:
    if at + 2 > len(data):
      raise ValueError('truncated: the file ends before its SOS marker')
    if data[at] != 0xFF:
      raise ValueError('not a JPEG file: 0x%02x at offset %d where a marker '
                       'should be' % (data[at], at))
    marker = data[at + 1]
    if marker == 0xFF:      # fill byte
      at += 1
      continue
    if marker == 0x01 or 0xD0 <= marker <= 0xD7:
      at += 2
      continue
    if marker == 0xD9:
      raise ValueError('truncated: EOI before any scan')
    if at + 4 > len(data):
      raise ValueError('truncated: marker 0x%02x without a length' % marker)
    size = int.from_bytes(data[at + 2:at + 4], 'big')
    body = data[at + 4:at + 2 + size]
    if size < 2 or at + 2 + size > len(data):
      raise ValueError('truncated: segment 0x%02x of %d bytes at offset %d'
                       % (marker, size, at))
    at += 2 + size
    if marker in _SOF_NAMES:
      raise NotImplementedError(_SOF_NAMES[marker] + ': only baseline '
                                'sequential DCT (SOF0) is read')
    if marker == 0xDB:
      while body:
        if body[0] >> 4:
          raise NotImplementedError('16-bit DQT entries')
        if len(body) < 65:
          raise ValueError('truncated: DQT')
        qtables[body[0] & 15] = np.array(list(body[1:65]), dtype=np.uint16)
        body = body[65:]
    elif marker == 0xC0:
      if len(body) < 6 or len(body) < 6 + 3 * body[5]:
        raise ValueError('truncated: SOF0')
      if body[0] != 8:
        raise NotImplementedError('%d-bit samples' % body[0])
      frame = {'h': int.from_bytes(body[1:3], 'big'),
               'w': int.from_bytes(body[3:5], 'big'),
               'components': [(body[6 + 3 * i], body[7 + 3 * i] >> 4,
                               body[7 + 3 * i] & 15, body[8 + 3 * i])
                              for i in range(body[5])]}
    elif marker == 0xC4:
      while body:
        klass, index = body[0] >> 4, body[0] & 15
        if len(body) < 17 or len(body) < 17 + sum(body[1:17]):
          raise ValueError('truncated: DHT')
        if klass > 1:
          raise ValueError('DHT: table class %d' % klass)
        if index > 1:
          raise NotImplementedError('Huffman table ids above 1 (baseline '
                                    'allows 0 and 1)')
        counts = list(body[1:17])
        huffman[(klass, index)] = _huffman_table(
            counts, list(body[17:17 + sum(counts)]), 256 if klass else 16)
        body = body[17 + sum(counts):]
    elif marker == 0xDD:
      if len(body) < 2:
        raise ValueError('truncated: DRI')
      restart = int.from_bytes(body[:2], 'big')
    elif marker == 0xEE and body[:5] == b'Adobe' and len(body) >= 12:
      adobe_transform = body[11]
    elif marker == 0xDA:
      break
  if frame is None:
    raise ValueError('SOS before any frame header')
  if restart:
    raise NotImplementedError('restart intervals (DRI %d)' % restart)
  comps = frame['components']
  if len(comps) not in (1, 3):
    raise NotImplementedError('%d components: one (gray) or three (YCbCr) '
                              'are read' % len(comps))
  if frame['h'] < 1 or frame['w'] < 1:
    raise ValueError('a frame of %d x %d' % (frame['h'], frame['w']))
  if len(comps) == 3:
    if adobe_transform == 0:
      raise NotImplementedError('an Adobe APP14 segment that says RGB')
    if comps[0][1] not in (1, 2) or comps[0][2] not in (1, 2):
      raise NotImplementedError('luma sampling %d x %d: 1 or 2 each way'
                                % (comps[0][1], comps[0][2]))
    if [c[1:3] for c in comps[1:]] != [(1, 1), (1, 1)]:
      raise NotImplementedError('chroma sampling other than 1 x 1')
    sampling = [c[1:3] for c in comps]
  else:
    sampling = [(1, 1)]
  if len(body) < 1 or len(body) < 4 + 2 * body[0]:
    raise ValueError('truncated: SOS')
  if body[0] != len(comps) or [body[1 + 2 * i] for i in range(body[0])] != [
      c[0] for c in comps]:
    raise NotImplementedError('a scan that does not hold all components in '
                              'frame order')
  if tuple(body[1 + 2 * body[0]:4 + 2 * body[0]]) != (0, 63, 0):
    raise NotImplementedError('Ss, Se, Ah/Al other than 0, 63, 0')
  selectors = [(body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15)
               for i in range(body[0])]
  for (td, ta), comp in zip(selectors, comps):
    if td > 1 or ta > 1:
      raise NotImplementedError('Huffman table ids above 1')
    if (0, td) not in huffman or (1, ta) not in huffman:
      raise ValueError('the scan refers to a Huffman table the file does '
                       'not define')
    if comp[3] not in qtables:
      raise ValueError('component %d refers to quantisation table %d, which '
                       'the file does not define' % (comp[0], comp[3]))
  tables = []
  for index in range(2):
    if (0, index) not in huffman and (1, index) not in huffman:
      tables.append(None)
      continue
    dc = huffman.get((0, index), (np.zeros(16, np.int64),
                                  np.zeros(16, np.uint16)))
    ac = huffman.get((1, index), (np.zeros(256, np.int64),
                                  np.zeros(256, np.uint16)))
    tables.append({'dc': dc[0], 'ac': ac[0], 'dc_codes': dc[1],
                   'ac_codes': ac[1]})
  return {'shape': (frame['h'], frame['w']), 'components': comps,
          'sampling': sampling, 'qtables': qtables, 'tables': tables,
          'selectors': selectors, 'segment_at': at}


def frame_layout(shape, sampling):
  """scan_layout for any frame this module reads: sampling is [(1, 1)] for a
  gray file or [(H, V), (1, 1), (1, 1)] with H and V of the luma component 1
  or 2 -- 4:4:4, 4:2:2 (2, 1), 4:4:0 (1, 2), 4:2:0 (2, 2).

  The keys of scan_layout, equal to it array for array where it knows the
  case ('subsampling' is (V, H) of the luma component, as utils.color takes
  it), and for vtc_jfif_dc_accumulate 'order' int32 (rows,) -- the rows sorted
  by component, then by scan order -- and 'start' uint8 (rows,), 1 where a
  component's chain begins."""
  try:
    h, w = (int(v) for v in shape)
    sampling = [(int(sh), int(sv)) for sh, sv in sampling]
  except (TypeError, ValueError):
    raise ValueError('shape must be (h, w) and sampling a list of (H, V)')
  if not (1 <= h <= 65535 and 1 <= w <= 65535):
    raise ValueError('a JFIF image is 1 .. 65535 pixels a side, got %r'
                     % ((h, w),))
  if sampling != [(1, 1)] and not (
      len(sampling) == 3 and sampling[0][0] in (1, 2) and
      sampling[0][1] in (1, 2) and sampling[1:] == [(1, 1), (1, 1)]):
    raise NotImplementedError('sampling %r: one component, or luma 1 or 2 '
                              'each way over 1 x 1 chroma' % (sampling,))
  hmax = max(s[0] for s in sampling)
  vmax = max(s[1] for s in sampling)
  mcus_v, mcus_h = -(-h // (8 * vmax)), -(-w // (8 * hmax))
  per_mcu = sum(sh * sv for sh, sv in sampling)
  rows = mcus_v * mcus_h * per_mcu
  my, mx = np.meshgrid(np.arange(mcus_v), np.arange(mcus_h), indexing='ij')
  mcu_base = (my * mcus_h + mx) * per_mcu
  component = np.zeros(rows, dtype=np.uint8)
  pred = np.full(rows, -1, dtype=np.int32)
  start = np.zeros(rows, dtype=np.uint8)
  plane_shapes, grids, row_of_block, order = [], [], [], []
  first = 0   # the component's first row inside an MCU
  for c, (sh, sv) in enumerate(sampling):
    plane_shapes.append((-(-h * sv // vmax), -(-w * sh // hmax)))
    bh, bw = mcus_v * sv, mcus_h * sh
    grids.append((bh, bw))
    rob = np.zeros((bh, bw), dtype=np.int32)
    for dy in range(sv):
      for dx in range(sh):
        rob[dy::sv, dx::sh] = mcu_base + first + dy * sh + dx
    row_of_block.append(rob.reshape(-1))
    mine = np.sort(rob.reshape(-1))   # the component's rows in scan order
    component[mine] = c
    pred[mine[1:]] = mine[:-1]
    start[len(order) and sum(len(o) for o in order)] = 1
    order.append(mine)
    first += sh * sv
  return {'shape': (h, w),
          'subsampling': None if len(sampling) == 1 else (vmax, hmax),
          'rows': rows, 'plane_shapes': plane_shapes, 'grids': grids,
          'sampling': sampling, 'row_of_block': row_of_block,
          'component': component,
          'table_sel': (component > 0).astype(np.uint8), 'pred': pred,
          'order': np.concatenate(order).astype(np.int32), 'start': start}


def unstuff_bytes(data, capacity=None):
  """(out, length, marker_at, dropped): `data` (a uint8 device tensor) up to
  its first marker -- a 0xFF that no 0x00 follows -- with the 0x00 behind every
  0xFF removed, as a uint8 device tensor of min(length, capacity) bytes;
  marker_at is data.numel() when there is no marker; dropped counts the bytes
  that did not fit under `capacity` (None: room for all).  One host read."""
  lib = vtc_hip.load_library()
  data = vtc_hip.require_device_tensor(data, 'data', torch.uint8)
  if data.dim() != 1:
    raise ValueError('data must be (n,), got shape %s' % (tuple(data.shape),))
  data = data.contiguous()
  capacity = data.numel() if capacity is None else int(capacity)
  if capacity < 0:
    raise ValueError('capacity must not be negative')
  meta = torch.zeros(8, dtype=torch.int64, device=data.device)
  out = _unstuff(lib, data, capacity, meta)
  host = meta.cpu().numpy()
  length, marker_at = int(host[0]), int(host[1])
  return (out[:min(length, capacity)], length, marker_at,
          int(host[2:3].view(np.int32)[0]))


def _unstuff(lib, data, capacity, meta):
  """Enqueues the unstuffing of `data` into a fresh tensor of `capacity`
  bytes.  meta int64[8]: [0:2] out_len, [2] the dropped count (its low int32)."""
  device = data.device
  n = data.numel()
  out = torch.empty(max(1, capacity), dtype=torch.uint8, device=device)
  ws = vtc_hip.workspace(lib.vtc_jfif_unstuff_bytes_workspace_bytes(n), device)
  vtc_hip.check(lib.vtc_jfif_unstuff_bytes(
      vtc_hip.ptr(data) if n else None, n, vtc_hip.ptr(out), capacity,
      vtc_hip.ptr(meta[0:2]), vtc_hip.ptr(meta[2:3]), vtc_hip.ptr(ws),
      ws.numel(), vtc_hip.current_stream(device)), 'vtc_jfif_unstuff_bytes')
  return out


class _DecodeTables(_DeviceTables):
  """_DeviceTables for a file that is read: where a pair carries the file's
  own codewords ('dc_codes', 'ac_codes': parse_headers), those are used; a
  DHT segment need not list the symbols of one length in ascending order."""

  def __init__(self, tables, device):
    _DeviceTables.__init__(self, tables, device)
    ac_code = self.ac_code.cpu().numpy().view(np.uint16).copy()
    dc_code = self.dc_code.cpu().numpy().view(np.uint16).copy()
    for pair, table in enumerate(tables):
      if table is not None and 'ac_codes' in table:
        ac_code[pair] = np.asarray(table['ac_codes'], dtype=np.uint16)
        dc_code[pair] = np.asarray(table['dc_codes'], dtype=np.uint16)
    self.ac_code = _upload(ac_code.view(np.int16), device)
    self.dc_code = _upload(dc_code.view(np.int16), device)


def _slots(layout, selectors):
  """(slot_dc, slot_ac) uint8: the table of each block position of an MCU."""
  sampling = layout['sampling']
  if len(selectors) != len(sampling):
    raise ValueError('selectors must hold one (Td, Ta) per component (%d)'
                     % len(sampling))
  slot_dc, slot_ac = [], []
  for (sh, sv), (td, ta) in zip(sampling, selectors):
    if td not in (0, 1) or ta not in (0, 1):
      raise ValueError('table selectors are 0 or 1, got %r' % ((td, ta),))
    slot_dc += [td] * (sh * sv)
    slot_ac += [ta] * (sh * sv)
  return (np.array(slot_dc, dtype=np.uint8), np.array(slot_ac, dtype=np.uint8))


def _unpack(lib, segment, layout, tables, selectors, status):
  """Enqueues the unpacking of `segment` into a fresh (rows, 64) tensor.
  status: int64[4] on the device."""
  device = segment.device
  rows = layout['rows']
  slot_dc, slot_ac = _slots(layout, selectors)
  dev = tables if isinstance(tables, _DeviceTables) else _DecodeTables(
      tables, device)
  levels = torch.empty((rows, 64), dtype=torch.int32, device=device)
  ws = vtc_hip.workspace(
      lib.vtc_jfif_unpack_workspace_bytes(segment.numel()), device)
  nslots = len(slot_dc)
  slot_dc, slot_ac = _upload(slot_dc, device), _upload(slot_ac, device)
  vtc_hip.check(lib.vtc_jfif_unpack(
      vtc_hip.ptr(segment), segment.numel(), vtc_hip.ptr(slot_dc),
      vtc_hip.ptr(slot_ac), nslots,
      vtc_hip.ptr(dev.ac_code), vtc_hip.ptr(dev.ac_len),
      vtc_hip.ptr(dev.dc_code), vtc_hip.ptr(dev.dc_len), vtc_hip.ptr(levels),
      rows, vtc_hip.ptr(status), vtc_hip.ptr(ws), ws.numel(),
      vtc_hip.current_stream(device)), 'vtc_jfif_unpack')
  return levels


def unpack_scan(segment, layout, tables, selectors=None):
  """(levels, status): the (rows, 64) int32 device levels of an unstuffed
  entropy-coded `segment` (a uint8 device tensor), DIFF in column 0, by
  self-synchronising parallel Huffman decoding; status the four integers of
  vtc_jfif_unpack -- 1 + bit of the first malformed token or 0, blocks
  completed, bit after block `rows` or -1, synchronisation rounds.  tables as
  tables_from_counts or parse_headers give them; selectors [(Td, Ta)] per
  component, by default (0, 0) for the first and (1, 1) for the others.  One
  host read; nothing is raised for a malformed stream."""
  lib = vtc_hip.load_library()
  segment = vtc_hip.require_device_tensor(segment, 'segment', torch.uint8)
  if segment.dim() != 1 or segment.numel() < 1:
    raise ValueError('segment must be (n,) with n >= 1, got shape %s'
                     % (tuple(segment.shape),))
  if selectors is None:
    selectors = [(min(c, 1), min(c, 1))
                 for c in range(len(layout['sampling']))]
  status = torch.zeros(4, dtype=torch.int64, device=segment.device)
  levels = _unpack(lib, segment.contiguous(), layout, tables, selectors,
                   status)
  return levels, status.cpu().tolist()


def _dc_accumulate(lib, levels, layout):
  device = levels.device
  d = levels.shape[0]
  order = np.ascontiguousarray(layout['order'], dtype=np.int32).reshape(-1)
  start = np.ascontiguousarray(layout['start'], dtype=np.uint8).reshape(-1)
  if order.shape[0] != d or start.shape[0] != d:
    raise ValueError('order and start must have one entry per row (%d)' % d)
  ws = vtc_hip.workspace(lib.vtc_jfif_dc_accumulate_workspace_bytes(d), device)
  order, start = _upload(order, device), _upload(start, device)
  vtc_hip.check(lib.vtc_jfif_dc_accumulate(
      vtc_hip.ptr(levels), d, vtc_hip.ptr(order), vtc_hip.ptr(start),
      vtc_hip.ptr(ws), ws.numel(),
      vtc_hip.current_stream(device)), 'vtc_jfif_dc_accumulate')
  return levels


def dc_accumulate(levels, layout):
  """Undoes DC prediction in place: column 0 of the (rows, 64) int32 device
  `levels` goes from DIFF to the DC level, along layout['order'] with a new
  chain where layout['start'] is set (frame_layout), as a segmented scan on
  the device.  Returns levels.  Only enqueues."""
  lib = vtc_hip.load_library()
  if _levels(levels) is not levels:
    raise ValueError('levels must be contiguous: it is updated in place')
  return _dc_accumulate(lib, levels, layout)


def decode_bytes(data):
  """(image, info) of the bytes of one baseline JFIF file: the (h, w) float32
  device plane of a gray file, or the (h, w, 3) RGB image of a colour one --
  planes through inverse_dct, chroma back to full resolution with the triangle
  filter of utils.color.merge_planes by the luma component's (V, H), RGB
  clamped to [0, 255].

  The headers are walked on the host (parse_headers), which also finds where
  the segment ends; unstuffing, the parallel Huffman decode, the DC scan and
  the inverse DCT run on the device, with one host read of the status records.
  info holds 'levels' (the (rows, 64) int32 device tensor in scan order,
  absolute DC), 'layout' (frame_layout), 'qtables' (one uint16[64] per
  component), 'planes', 'rounds' (synchronisation rounds of the decode),
  'trailing_bits_are_ones' (the pad bits of the last byte, T.81 F.1.2.3) and
  'headers'.  ValueError for a malformed or truncated segment, for bytes left
  over, and for anything but EOI behind the segment."""
  from utils import color
  lib = vtc_hip.load_library()
  data = bytes(data)
  headers = parse_headers(data)
  layout = frame_layout(headers['shape'], headers['sampling'])
  at = headers['segment_at']
  found = _MARKER_IN_SEGMENT.search(data, at)
  if found is None:
    raise ValueError('truncated: no marker behind the entropy-coded segment')
  marker_at = found.start() - at
  follows = data[found.start() + 1]
  if 0xD0 <= follows <= 0xD7:
    raise ValueError('a restart marker (RST%d) inside the scan: restart '
                     'intervals are not read' % (follows - 0xD0))
  if follows != 0xD9:
    raise ValueError('marker 0x%02x behind the entropy-coded segment where '
                     'EOI should be' % follows)
  seg_bytes = marker_at - data.count(b'\xff\x00', at, at + marker_at)
  if seg_bytes < 1:
    raise ValueError('truncated: an empty entropy-coded segment')
  device = torch.device('cuda', torch.cuda.current_device())
  # the marker travels too: the device finds it again (a writable copy)
  stuffed = _upload(np.array(np.frombuffer(
      data, dtype=np.uint8, count=marker_at + 2, offset=at)), device)
  meta = torch.zeros(8, dtype=torch.int64, device=device)
  segment = _unstuff(lib, stuffed, seg_bytes, meta)[:seg_bytes]
  levels = _unpack(lib, segment, layout, headers['tables'],
                   headers['selectors'], meta[4:8])
  _dc_accumulate(lib, levels, layout)
  qtables = [headers['qtables'][c[3]] for c in headers['components']]
  planes = [inverse_dct(levels, layout['plane_shapes'][c], layout['grids'][c],
                        qtables[c], layout['row_of_block'][c])
            for c in range(len(qtables))]
  host = meta.cpu().numpy()
  dropped = int(host[2:3].view(np.int32)[0])
  if (int(host[0]), int(host[1]), dropped) != (seg_bytes, marker_at, 0):
    raise ValueError('the device unstuffed %d bytes up to offset %d (%d '
                     'dropped), the host counted %d up to %d'
                     % (host[0], host[1], dropped, seg_bytes, marker_at))
  malformed, blocks, end, rounds = (int(v) for v in host[4:8])
  if malformed:
    raise ValueError('malformed token at bit %d of the entropy-coded segment '
                     '(block %d of %d)' % (malformed - 1, blocks,
                                           layout['rows']))
  if blocks < layout['rows'] or end < 0:
    raise ValueError('truncated: the segment holds %d of %d blocks'
                     % (blocks, layout['rows']))
  left = 8 * seg_bytes - end
  if left < 0:
    raise ValueError('truncated: the last token needs %d bits beyond the '
                     'segment' % -left)
  if left >= 8:
    raise ValueError('%d bits are left over behind block %d'
                     % (left, layout['rows']))
  last = 0xFF if data[at + marker_at - 2:at + marker_at] == b'\xff\x00' else (
      data[at + marker_at - 1])
  info = {'levels': levels, 'layout': layout, 'qtables': qtables,
          'planes': planes, 'rounds': rounds,
          'trailing_bits_are_ones': last & ((1 << left) - 1) == (1 << left) - 1,
          'headers': headers}
  if len(planes) == 1:
    return planes[0], info
  return color.merge_planes(planes, layout['shape'], layout['subsampling'],
                            upsampling='triangle', clamp=(0.0, 255.0)), info


def read_jpeg(path):
  """(image, info) of the baseline JFIF file at `path`: decode_bytes of its
  bytes."""
  with open(path, 'rb') as f:
    return decode_bytes(f.read())


def rate_distortion_image(image, quality=75, subsampling=(2, 2),
                          qtables=None, from_stream=False):
  """The JPEG point of a rate-distortion curve: `image` ((h, w) gray or
  (h, w, 3) RGB, samples in [0, 255]) is written as a JFIF file and decoded
  from its levels -- or, with from_stream, from the bytes of the file through
  decode_bytes, the way any reader of the file sees it; info['decoded_from']
  is then 'bytes'.

  Returns, in the order of utils.jpeg.rate_distortion_image,
  {'bits_per_pixel', 'pSNR', 'SSIM', 'tables'} and then 'bytes' and 'info':
  bits per pixel counts the whole file, 8 * len(bytes) / (h * w); pSNR is
  plotting.compute_pSNR against a range of 255; SSIM is
  plotting.compute_ssim_images against 255, of the image for a gray one and
  the mean over the R, G and B planes for a colour one."""
  from utils import plotting
  if torch.is_tensor(image) and image.dim() == 2:
    data, info = encode_gray(image, quality, qtables)
  else:
    data, info = encode_rgb(image, subsampling, quality, qtables)
  if from_stream:
    decoded = decode_bytes(data)[0]
    info['decoded_from'] = 'bytes'
  else:
    decoded = decode_levels(info)
  original = image.contiguous()
  if original.dim() == 2:
    pair = original[None], decoded[None]
  else:
    pair = (original.permute(2, 0, 1).contiguous(),
            decoded.permute(2, 0, 1).contiguous())
  ssim = plotting.compute_ssim_images(pair[0], pair[1], manual_sig_mag=255.0)
  return {'bits_per_pixel': info['bits_per_pixel'],
          'pSNR': plotting.compute_pSNR(original, decoded,
                                        manual_sig_mag=255.0),
          'SSIM': float(ssim.mean()),
          'tables': info['tables'], 'bytes': data, 'info': info}
