"""
The JPEG source coding of the reference's utils/jpeg.py on MI355X: how many
bits a set of quantised codes costs, and the bits themselves.

The reference's names are kept, with their return types --
get_jpeg_quant_hifi_binwidths, compute_huffman_table, jpg_coeff_to_binstr,
generate_ac_dc_huffman_tables, generate_jpg_binary_stream -- and beside them
a batch interface the reference lacks: quantize, dequantize, symbol_counts,
stream_bits, pack_streams, stream_as_str, rate_distortion_point,
rate_distortion_image (a whole image tiled, coded, decoded and reassembled,
with pSNR and SSIM measured on the image).  The per-patch work (run-length symbols, their counts, stream lengths, packing)
runs in the kernels of csrc/jpeg_codec.hip behind include/vtc_codec.h; the
Huffman tables, at most 272 symbols, are built here on the host from the
device counts.  DESIGN.md 4.11 states the coding rules.

The reference has no decoder: it only measures len(stream).  Here the packed
streams can be read back -- unpack_streams, parse_jpg_binary_stream (the
inverse of generate_jpg_binary_stream for one row), decode_patches -- through
csrc/jpeg_decode.hip behind include/vtc_decode.h; DESIGN.md 4.12.

Symbols are spelled as the reference spells them: an AC byte b is
'%x%x' % (b >> 4, b & 15), DC category 0 is '-', category c is '%x' % c.
Tables are dicts {symbol: string of '0' / '1'}.

Levels are (d, s) int32 device tensors, one patch per row in scan order,
relative to the zero codeword; 1 <= s <= 4096, |level| <= 32767 and codewords
of at most 64 bits.  A CPU tensor raises VtcHipError, a level beyond 32767
ValueError, a symbol the tables lack KeyError with its spelling (as the
reference's dict lookup does), a longer codeword NotImplementedError.
"""
import heapq

import numpy as np
import torch

import vtc_hip
from utils import matrix_zigzag

MAX_CODE_BITS = 64
EOB = '00'


# --------------------------------------------------------------- spellings
def ac_symbol(byte):
  return '%x%x' % (byte >> 4, byte & 15)


def dc_symbol(category):
  return '-' if category == 0 else '%x' % category


_AC_BYTE = {ac_symbol(b): b for b in range(256)}
_DC_CATEGORY = {dc_symbol(c): c for c in range(16)}


def _symbol_of_id(symbol_id):
  """Symbol ids of include/vtc_codec.h: AC byte b is b, DC category c is
  256 + c."""
  return ac_symbol(symbol_id) if symbol_id < 256 else dc_symbol(
      symbol_id - 256)


# ------------------------------------------------------------ host helpers
def get_jpeg_quant_hifi_binwidths():
  """The luminance quantisation table of ITU-T T.81 Annex K.1 (for data in
  [0, 255]) in zig-zag order, float64 (64,)."""
  table_k1 = np.array([[16, 11, 10, 16, 24, 40, 51, 61],
                       [12, 12, 14, 19, 26, 58, 60, 55],
                       [14, 13, 16, 24, 40, 57, 69, 56],
                       [14, 17, 22, 29, 51, 87, 80, 62],
                       [18, 22, 37, 56, 68, 109, 103, 77],
                       [24, 35, 55, 64, 81, 104, 113, 92],
                       [49, 64, 78, 87, 103, 121, 120, 101],
                       [72, 92, 95, 98, 112, 100, 103, 99]])
  return matrix_zigzag.zigzag(table_k1)


def get_jpeg_quant_chroma_binwidths():
  """The chrominance quantisation table of ITU-T T.81 Annex K.2 (for data in
  [0, 255]) in zig-zag order, float64 (64,): the bin widths of the Cb and Cr
  planes of utils.color.rate_distortion_image_color."""
  table_k2 = np.array([[17, 18, 24, 47, 99, 99, 99, 99],
                       [18, 21, 26, 66, 99, 99, 99, 99],
                       [24, 26, 56, 99, 99, 99, 99, 99],
                       [47, 66, 99, 99, 99, 99, 99, 99],
                       [99, 99, 99, 99, 99, 99, 99, 99],
                       [99, 99, 99, 99, 99, 99, 99, 99],
                       [99, 99, 99, 99, 99, 99, 99, 99],
                       [99, 99, 99, 99, 99, 99, 99, 99]])
  return matrix_zigzag.zigzag(table_k2)


def compute_huffman_table(symb2freq):
  """{symbol: codeword} of the Huffman code of {symbol: weight}.

  The two lightest subtrees are merged until one is left; a subtree is the
  list [weight, [symbol, code], [symbol, code], ...] and subtrees are ordered
  as Python orders lists, which settles every tie the way the reference's heap
  does.  The lighter of the two gets the prefix '0', the other '1'.  The
  result is ordered by (code length, [symbol, code])."""
  subtrees = [[weight, [symbol, '']] for symbol, weight in symb2freq.items()]
  heapq.heapify(subtrees)
  while len(subtrees) > 1:
    light = heapq.heappop(subtrees)
    heavy = heapq.heappop(subtrees)
    for bit, subtree in (('0', light), ('1', heavy)):
      for leaf in subtree[1:]:
        leaf[1] = bit + leaf[1]
    heapq.heappush(subtrees, [light[0] + heavy[0]] + light[1:] + heavy[1:])
  leaves = subtrees[0][1:]
  return dict(sorted(leaves, key=lambda leaf: (len(leaf[1]), leaf)))


def jpg_coeff_to_binstr(decimal_number):
  """Value bits of a level: '' for 0, the binary digits of a positive level,
  their complement for a negative one."""
  number = int(decimal_number)
  if number == 0:
    return ''
  digits = format(abs(number), 'b')
  if number > 0:
    return digits
  return digits.translate({ord('0'): '1', ord('1'): '0'})


def tables_from_counts(ac_counts, dc_counts):
  """(huff_table_ac, huff_table_dc) from the count arrays of symbol_counts.
  Every AC symbol with run 0..14 and size 0..9 and every DC category 1..14
  that was not seen enters with count 1, as in the reference; run 15 and
  category 0 enter only when seen."""
  counts_ac = {ac_symbol(b): int(n) for b, n in enumerate(ac_counts) if n}
  counts_dc = {dc_symbol(c): int(n) for c, n in enumerate(dc_counts) if n}
  for run in range(15):
    for size in range(10):
      counts_ac.setdefault(ac_symbol(run << 4 | size), 1)
  for category in range(1, 15):
    counts_dc.setdefault(dc_symbol(category), 1)
  return compute_huffman_table(counts_ac), compute_huffman_table(counts_dc)


def table_arrays(table, lookup, size):
  """(code uint64[size], length uint8[size]) of a {symbol: codeword} table;
  symbols the table lacks get length 0."""
  code = np.zeros(size, dtype=np.uint64)
  length = np.zeros(size, dtype=np.uint8)
  for symbol, word in table.items():
    if len(word) > MAX_CODE_BITS:
      raise NotImplementedError(
          'codeword of %d bits for symbol %r: the device packer takes at '
          'most %d' % (len(word), symbol, MAX_CODE_BITS))
    index = lookup[symbol]
    code[index] = int(word, 2) if word else 0
    length[index] = len(word)
  return code, length


# ------------------------------------------------------------ device calls
def _levels(levels):
  levels = vtc_hip.require_device_tensor(levels, 'levels', torch.int32)
  if levels.dim() != 2:
    raise ValueError('levels must be (d, s), got shape %s'
                     % (tuple(levels.shape),))
  return levels.contiguous()


def _upload(array, device):
  return torch.from_numpy(np.ascontiguousarray(array)).to(device)


def _scan_arguments(binwidths, order, s, device):
  widths = np.ascontiguousarray(binwidths, dtype=np.float64).reshape(-1)
  if widths.shape[0] != s:
    raise ValueError('binwidths must have %d entries, got %d'
                     % (s, widths.shape[0]))
  order_dev = None
  if order is not None:
    order = np.ascontiguousarray(order, dtype=np.int32).reshape(-1)
    if order.shape[0] != s or sorted(order.tolist()) != list(range(s)):
      raise ValueError('order must be a permutation of 0..%d' % (s - 1))
    order_dev = _upload(order, device)
  return _upload(widths, device), order_dev


def _raise_status(status, what):
  over, missing = status.tolist()
  if over:
    raise ValueError(
        '%s: %d levels beyond +-32767 (size category above 15) or stream '
        'bits outside the output' % (what, over))
  if missing:
    raise KeyError(_symbol_of_id(missing - 1))


def quantize(codes, binwidths, order=None):
  """levels (d, s) int32 = rint(float64(codes)[:, order] / binwidths), ties to
  even, exactly as numpy computes it.  codes: (d, s) float32 device tensor;
  binwidths: s host floats in scan order; order: s host integers (scan
  position k reads code column order[k]) or None for the identity."""
  lib = vtc_hip.load_library()
  codes = vtc_hip.require_device_tensor(codes, 'codes').contiguous()
  d, s = codes.shape
  widths, order_dev = _scan_arguments(binwidths, order, s, codes.device)
  levels = torch.empty((d, s), dtype=torch.int32, device=codes.device)
  vtc_hip.check(lib.vtc_jpeg_quantize(
      vtc_hip.ptr(codes), vtc_hip.ptr(widths), vtc_hip.ptr(order_dev),
      vtc_hip.ptr(levels), d, s, vtc_hip.current_stream(codes.device)),
                'vtc_jpeg_quantize')
  return levels


def dequantize(levels, binwidths, order=None):
  """codes (d, s) float32 with codes[:, order[k]] = levels[:, k] *
  binwidths[k], the product in float64 and rounded once."""
  lib = vtc_hip.load_library()
  levels = _levels(levels)
  d, s = levels.shape
  widths, order_dev = _scan_arguments(binwidths, order, s, levels.device)
  codes = torch.empty((d, s), dtype=torch.float32, device=levels.device)
  vtc_hip.check(lib.vtc_jpeg_dequantize(
      vtc_hip.ptr(levels), vtc_hip.ptr(widths), vtc_hip.ptr(order_dev),
      vtc_hip.ptr(codes), d, s, vtc_hip.current_stream(levels.device)),
                'vtc_jpeg_dequantize')
  return codes


def symbol_counts(levels):
  """(ac_counts int64[256] indexed by run << 4 | size, dc_counts int64[16]
  indexed by category) as numpy arrays: how often each run-length symbol
  occurs in the streams of all rows.  One host read."""
  lib = vtc_hip.load_library()
  levels = _levels(levels)
  d, s = levels.shape
  device = levels.device
  counts = torch.empty(256 + 16, dtype=torch.int64, device=device)
  status = torch.empty(2, dtype=torch.int32, device=device)
  vtc_hip.check(lib.vtc_jpeg_symbol_counts(
      vtc_hip.ptr(levels), d, s, vtc_hip.ptr(counts),
      vtc_hip.ptr(counts[256:]), vtc_hip.ptr(status),
      vtc_hip.current_stream(device)), 'vtc_jpeg_symbol_counts')
  _raise_status(status, 'symbol_counts')
  counts = counts.cpu().numpy()
  return counts[:256].copy(), counts[256:].copy()


class _DeviceTables(object):
  def __init__(self, table_ac, table_dc, device):
    ac_code, ac_len = table_arrays(table_ac, _AC_BYTE, 256)
    dc_code, dc_len = table_arrays(table_dc, _DC_CATEGORY, 16)
    # uint64 as int64 bits: torch moves bytes
    self.code = _upload(np.concatenate([ac_code, dc_code]).view(np.int64),
                        device)
    self.len = _upload(np.concatenate([ac_len, dc_len]), device)
    self.ac_code, self.dc_code = self.code, self.code[256:]
    self.ac_len, self.dc_len = self.len, self.len[256:]


def _stream_bits(lib, levels, tables, status):
  d, s = levels.shape
  bits = torch.empty(d, dtype=torch.int32, device=levels.device)
  vtc_hip.check(lib.vtc_jpeg_stream_bits(
      vtc_hip.ptr(levels), d, s, vtc_hip.ptr(tables.ac_len),
      vtc_hip.ptr(tables.dc_len), vtc_hip.ptr(bits), vtc_hip.ptr(status),
      vtc_hip.current_stream(levels.device)), 'vtc_jpeg_stream_bits')
  return bits


def bit_offsets(bits):
  """(d + 1,) int64 device tensor: exclusive prefix sum of the (d,) int32
  `bits`, the total last.  Only enqueues."""
  lib = vtc_hip.load_library()
  bits = vtc_hip.require_device_tensor(bits, 'bits', torch.int32).contiguous()
  d = bits.shape[0]
  offsets = torch.empty(d + 1, dtype=torch.int64, device=bits.device)
  ws = vtc_hip.workspace(lib.vtc_jpeg_bit_offsets_workspace_bytes(d),
                         bits.device)
  vtc_hip.check(lib.vtc_jpeg_bit_offsets(
      vtc_hip.ptr(bits), d, vtc_hip.ptr(offsets), vtc_hip.ptr(ws), ws.numel(),
      vtc_hip.current_stream(bits.device)), 'vtc_jpeg_bit_offsets')
  return offsets


def stream_bits(levels, table_ac, table_dc):
  """(d,) int32 device tensor: len() of the reference's stream of each row
  under the two tables.  One host read (the status)."""
  lib = vtc_hip.load_library()
  levels = _levels(levels)
  tables = _DeviceTables(table_ac, table_dc, levels.device)
  status = torch.empty(2, dtype=torch.int32, device=levels.device)
  bits = _stream_bits(lib, levels, tables, status)
  _raise_status(status, 'stream_bits')
  return bits


def pack_streams(levels, table_ac, table_dc):
  """(packed, offsets): the streams of all rows back to back in one uint8
  device tensor, most significant bit first (np.unpackbits gives the bits
  back; the last byte is zero-padded), and the (d + 1,) int64 device tensor of
  the bit at which each row's stream starts, the total last."""
  lib = vtc_hip.load_library()
  levels = _levels(levels)
  d, s = levels.shape
  device = levels.device
  tables = _DeviceTables(table_ac, table_dc, device)
  status = torch.empty(2, dtype=torch.int32, device=device)
  bits = _stream_bits(lib, levels, tables, status)
  _raise_status(status, 'pack_streams')
  offsets = bit_offsets(bits)
  total = int(offsets[d])
  packed = torch.empty(max(1, -(-total // 8)), dtype=torch.uint8,
                       device=device)
  vtc_hip.check(lib.vtc_jpeg_pack(
      vtc_hip.ptr(levels), d, s, vtc_hip.ptr(tables.ac_code),
      vtc_hip.ptr(tables.ac_len), vtc_hip.ptr(tables.dc_code),
      vtc_hip.ptr(tables.dc_len), vtc_hip.ptr(offsets), vtc_hip.ptr(packed),
      packed.numel(), vtc_hip.ptr(status), vtc_hip.current_stream(device)),
                'vtc_jpeg_pack')
  _raise_status(status, 'pack_streams')
  return packed, offsets


def stream_as_str(packed, offsets, i):
  """Row i's stream as the reference's string of '0' and '1'."""
  start, stop = int(offsets[i]), int(offsets[i + 1])
  chunk = packed[start // 8:-(-stop // 8)].cpu().numpy()
  bits = np.unpackbits(chunk)[start % 8:start % 8 + stop - start]
  return ''.join('1' if b else '0' for b in bits)


# ------------------------------------------------------------------ decoding
def check_prefix_free(table):
  """ValueError naming two symbols of a {symbol: codeword} table when the
  codeword of one equals the other's or is a prefix of it: such a table
  cannot be decoded.  In sorted order a prefix sits right before a word that
  starts with it, so neighbours suffice."""
  words = sorted((word, symbol) for symbol, word in table.items())
  for (short, first), (long_, second) in zip(words, words[1:]):
    if long_.startswith(short):
      raise ValueError(
          'not a prefix-free table: the codeword %r of symbol %r %s the '
          'codeword %r of symbol %r' % (
              short, first, 'equals' if short == long_ else 'is a prefix of',
              long_, second))


def unpack_streams(packed, offsets, s, table_ac, table_dc):
  """levels (d, s) int32 device tensor from what pack_streams returns: packed
  is a uint8 device tensor, offsets the (d + 1,) int64 device tensor of the bit
  at which each row's stream starts, the total last.  The inverse of
  pack_streams under the same two tables.

  ValueError for a table that is not prefix-free (both symbols named) and for
  malformed rows (their number and the first one named; include/vtc_decode.h
  lists what makes a row malformed), NotImplementedError for a codeword of
  more than 64 bits, VtcHipError for a CPU tensor.  One host read (the
  status)."""
  for table in (table_ac, table_dc):
    check_prefix_free(table)
  packed =vtc_hip.require_device_tensor(packed, 'packed', torch.uint8)
  offsets = vtc_hip.require_device_tensor(offsets, 'offsets', torch.int64)
  if packed.dim() != 1 or offsets.dim() != 1 or offsets.shape[0] < 2:
    raise ValueError('packed must be (bytes,) and offsets (d + 1,), got '
                     'shapes %s and %s' % (tuple(packed.shape),
                                           tuple(offsets.shape)))
  lib = vtc_hip.load_library()
  packed, offsets = packed.contiguous(), offsets.contiguous()
  device = packed.device
  d, s = offsets.shape[0] - 1, int(s)
  tables = _DeviceTables(table_ac, table_dc, device)
  levels = torch.empty((d, s), dtype=torch.int32, device=device)
  status = torch.empty(3, dtype=torch.int64, device=device)
  ws = vtc_hip.workspace(lib.vtc_jpeg_unpack_workspace_bytes(), device)
  vtc_hip.check(lib.vtc_jpeg_unpack(
      vtc_hip.ptr(packed), packed.numel(), vtc_hip.ptr(offsets), d, s,
      vtc_hip.ptr(tables.ac_code), vtc_hip.ptr(tables.ac_len),
      vtc_hip.ptr(tables.dc_code), vtc_hip.ptr(tables.dc_len),
      vtc_hip.ptr(levels), vtc_hip.ptr(status), vtc_hip.ptr(ws), ws.numel(),
      vtc_hip.current_stream(device)), 'vtc_jpeg_unpack')
  malformed, first, clash = status.tolist()
  if clash:   # the host check above saw the same tables
    raise ValueError('not a prefix-free table: symbol %r'
                     % _symbol_of_id(clash - 1))
  if malformed:
    raise ValueError('unpack_streams: %d malformed rows of %d, the first is '
                     'row %d' % (malformed, d, first - 1))
  return levels


def decode_patches(packed, offsets, dictionary, binwidths, quant_multiplier,
                   tables, order=None):
  """The reconstruction (d, n) float32 of the patches whose streams are in
  (packed, offsets): unpack_streams, dequantize with binwidths *
  quant_multiplier, then invertible_linear.apply_filter with the dictionary.
  With the arguments of rate_distortion_point it gives the reconstruction that
  function takes its pSNR from, but from the bytes.

  dictionary : (n, n) float32 device tensor
  tables : (huff_table_ac, huff_table_dc)
  """
  from analysis_transforms.fully_connected import invertible_linear
  dictionary = vtc_hip.require_device_tensor(dictionary, 'dictionary')
  widths = np.asarray(binwidths, dtype=np.float64) * quant_multiplier
  levels = unpack_streams(packed, offsets, dictionary.shape[0], tables[0],
                          tables[1])
  return invertible_linear.apply_filter(dequantize(levels, widths, order),
                                        dictionary.contiguous())


# ------------------------------------------------- the reference's interface
def _relative_levels(assignment_inds, inds_of_zero_valued_cw):
  """int32 levels relative to the zero codeword.  The subtraction and the
  cast are tensor plumbing done by torch on the tensor's device."""
  if not torch.is_tensor(assignment_inds):
    raise TypeError('assignment_inds must be a torch.Tensor')
  if not assignment_inds.is_cuda:
    raise vtc_hip.VtcHipError(
        'assignment_inds lives on %s: the MI355X engine only runs on HIP '
        'device tensors (no CPU path is provided on purpose)'
        % assignment_inds.device)
  if assignment_inds.dtype.is_floating_point:
    raise TypeError('assignment_inds must be an integer tensor')
  zero = torch.as_tensor(np.asarray(inds_of_zero_valued_cw)
                         if not torch.is_tensor(inds_of_zero_valued_cw)
                         else inds_of_zero_valued_cw)
  zero = zero.to(device=assignment_inds.device, dtype=torch.int64)
  return (assignment_inds.to(torch.int64) - zero).to(torch.int32)


def generate_ac_dc_huffman_tables(all_assignment_inds, inds_of_zero_valued_cw):
  """(huff_table_ac, huff_table_dc) for a training set of codeword indices.

  all_assignment_inds : integer device tensor (D, s)
  inds_of_zero_valued_cw : (s,) integers, the index of the zero codeword of
      each dimension
  """
  levels = _relative_levels(all_assignment_inds, inds_of_zero_valued_cw)
  return tables_from_counts(*symbol_counts(levels))


def generate_jpg_binary_stream(assignment_inds, inds_of_zero_valued_cw,
                               only_get_huffman_symbols=True,
                               huffman_table_ac=None, huffman_table_dc=None):
  """One data point, (s,) integer device tensor, through the batch path with
  d = 1.  Returns (list of AC symbols, DC symbol) when
  only_get_huffman_symbols, else the stream as a string."""
  levels = _relative_levels(assignment_inds, inds_of_zero_valued_cw)
  levels = levels.reshape(1, -1)
  if only_get_huffman_symbols:
    # a code that spells every symbol in 9 bits (a marker and the byte, the
    # DC category likewise): the packed stream then names the symbols in order
    table_ac = {ac_symbol(b): format(b, '09b') for b in range(256)}
    table_dc = {dc_symbol(c): format(256 + c, '09b') for c in range(16)}
    packed, offsets = pack_streams(levels, table_ac, table_dc)
    bits = stream_as_str(packed, offsets, 0)
    symbols, at = [], 0
    while True:
      word = int(bits[at:at + 9], 2)
      at += 9
      if word >= 256:
        assert at + (word - 256) == len(bits)
        return symbols, dc_symbol(word - 256)
      symbols.append(ac_symbol(word))
      if symbols[-1] != EOB:
        at += word & 15    # value bits
  assert (huffman_table_dc is not None) and (huffman_table_ac is not None)
  packed, offsets = pack_streams(levels, huffman_table_ac, huffman_table_dc)
  return stream_as_str(packed, offsets, 0)


def parse_jpg_binary_stream(stream, s, inds_of_zero_valued_cw,
                            huffman_table_ac, huffman_table_dc):
  """The inverse of generate_jpg_binary_stream(...,
  only_get_huffman_symbols=False) for one data point: the (s,) int64 device
  tensor of assignment indices whose stream is the string `stream` of '0' and
  '1'.  Through the batch path with d = 1, on the current HIP device (that of
  inds_of_zero_valued_cw when it is a device tensor)."""
  if not isinstance(stream, str) or set(stream) - set('01'):
    raise TypeError("stream must be a str of '0' and '1'")
  device = torch.device('cuda')
  if torch.is_tensor(inds_of_zero_valued_cw) and inds_of_zero_valued_cw.is_cuda:
    device = inds_of_zero_valued_cw.device
    zero = inds_of_zero_valued_cw.to(torch.int64)
  else:
    zero = torch.as_tensor(np.asarray(inds_of_zero_valued_cw),
                           dtype=torch.int64)
  bits = np.frombuffer(stream.encode('ascii'), dtype=np.uint8) - ord('0')
  host = np.packbits(bits) if len(stream) else np.zeros(1, dtype=np.uint8)
  ends = np.array([0, len(stream)], dtype=np.int64)
  levels = unpack_streams(_upload(host, device), _upload(ends, device), s,
                          huffman_table_ac, huffman_table_dc)
  return levels[0].to(torch.int64) + zero.to(device)


def rate_distortion_point(patches, dictionary, binwidths, quant_multiplier,
                          tables=None, order=None):
  """One point of a rate-distortion curve.

  patches : (d, n) float32 device tensor
  dictionary : (n, n) float32 device tensor, patches ~ codes @ dictionary
  binwidths : n floats in scan order; the bins used are binwidths *
      quant_multiplier
  tables : (huff_table_ac, huff_table_dc), or None to train them on these
      patches
  order : scan order of the code columns (matrix_zigzag.scan_order), or None

  Returns (bits per pixel, pSNR in dB of the reconstruction from the
  dequantised codes, (huff_table_ac, huff_table_dc)).
  """
  from analysis_transforms.fully_connected import invertible_linear
  from utils import plotting
  patches = vtc_hip.require_device_tensor(patches, 'patches').contiguous()
  widths = np.asarray(binwidths, dtype=np.float64) * quant_multiplier
  codes = invertible_linear.run(patches, dictionary)
  levels = quantize(codes, widths, order)
  if tables is None:
    tables = tables_from_counts(*symbol_counts(levels))
  bits = stream_bits(levels, tables[0], tables[1])
  total_bits = int(bit_offsets(bits)[-1])
  reconstruction = invertible_linear.apply_filter(
      dequantize(levels, widths, order), dictionary.contiguous())
  psnr = plotting.compute_pSNR(patches, reconstruction)
  return total_bits / float(patches.numel()), psnr, tables


def _component_means(component_means, n, device):
  if torch.is_tensor(component_means):
    means = component_means.to(device=device, dtype=torch.float32)
  else:
    means = _upload(np.asarray(component_means, dtype=np.float32), device)
  means = means.reshape(-1).contiguous()
  if means.shape[0] != n:
    raise ValueError('component_means must have %d entries, got %d'
                     % (n, means.shape[0]))
  return means


def rate_distortion_image(image, dictionary, patch_dimensions, binwidths,
                          quant_multiplier, tables=None, order=None,
                          component_means=None):
  """One point of a rate-distortion curve, measured on a whole image as the
  reference's experiments do (their fullimg_reshape_params): the image is
  tiled into patches, the patches are coded, quantised, packed into their
  JPEG streams, decoded from those bytes (decode_patches) and reassembled,
  and both distortions are taken between the reassembled image and the part
  of the original that the patches cover.

  image : (h, w) float32 device tensor
  dictionary : (n, n) float32 device tensor, n = ph * pw, patches ~ codes @
      dictionary
  patch_dimensions : (ph, pw); pixels right of and below the last whole patch
      are left out of every figure
  binwidths, quant_multiplier, tables, order : as in rate_distortion_point
  component_means : None, or n values subtracted from every patch before it
      is coded and added back after decoding, as the reference's experiments
      centre their patches

  Returns {'bits_per_pixel', 'pSNR', 'SSIM', 'tables'}: total stream bits over
  covered pixels, plotting.compute_pSNR and plotting.compute_ssim of (covered
  original, reassembled reconstruction), and (huff_table_ac, huff_table_dc).
  """
  from analysis_transforms.fully_connected import invertible_linear
  from utils import image_processing
  from utils import plotting
  image = vtc_hip.require_device_tensor(image, 'image')
  if image.dim() != 2:
    raise ValueError('image must be (h, w), got shape %s'
                     % (tuple(image.shape),))
  ph, pw = int(patch_dimensions[0]), int(patch_dimensions[1])
  patches, positions = image_processing.patches_from_single_image(
      image[:, :, None], (ph, pw), flatten_patches=True)
  if patches.shape[0] == 0:
    raise ValueError('image %s holds no %d x %d patch'
                     % (tuple(image.shape), ph, pw))
  original = image[:image.shape[0] // ph * ph, :image.shape[1] // pw * pw]
  coded = patches
  if component_means is not None:
    means = _component_means(component_means, patches.shape[1], image.device)
    coded = image_processing._column_apply(
        patches, vtc_hip.DTYPE_F32, vtc_hip.COLUMN_SUBTRACT, means)
  widths = np.asarray(binwidths, dtype=np.float64) * quant_multiplier
  levels = quantize(invertible_linear.run(coded, dictionary), widths, order)
  if tables is None:
    tables = tables_from_counts(*symbol_counts(levels))
  packed, offsets = pack_streams(levels, tables[0], tables[1])
  total_bits = int(offsets[-1])
  decoded = decode_patches(packed, offsets, dictionary, binwidths,
                           quant_multiplier, tables, order)
  if component_means is not None:   # x - (-m): the addition, in float32
    decoded = image_processing._column_apply(
        decoded, vtc_hip.DTYPE_F32, vtc_hip.COLUMN_SUBTRACT, -means)
  reconstruction = image_processing.assemble_image_from_patches(
      decoded, (ph, pw), positions)[:, :, 0]
  return {'bits_per_pixel': total_bits / float(patches.numel()),
          'pSNR': plotting.compute_pSNR(original, reconstruction),
          'SSIM': plotting.compute_ssim(original, reconstruction),
          'tables': tables}
