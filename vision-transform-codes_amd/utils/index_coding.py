"""
Huffman codes for the indices of the quantisers of utils.quantization and
utils.vector_quantization: what a set of quantised sparse codes costs under
tables trained elsewhere, and the bits themselves.

The reference's experiment (experiments/rate_distortion_sparse_coding.py:
763-827) trains one Huffman table per index stream on the training codes and
charges the test codes what those tables cost.  Here

  index_huffman_tables   counts of index_counts / vector_index_counts -> one
                         table per column, on the host (at most 4096 symbols
                         each), with jpeg.compute_huffman_table
  index_table_arrays     tables -> the (m, kmax) arrays the device reads
  index_code_bits        indices (b, m), tables -> bits per row and per column
  pack_index_streams     indices (b, m), tables -> (packed, offsets), the
                         layout of jpeg.pack_streams: jpeg.stream_as_str reads
                         a row back as a string of '0' and '1'
  unpack_index_streams   (packed, offsets), tables -> indices (b, m): the
                         inverse of pack_index_streams
  parse_index_stream     one string of '0' / '1', tables -> its m indices

A prefix code spends at least one bit per index; the range coder (rANS) of
include/vtc_index_ans.h does not:

  index_ans_frequencies  counts -> uint16 (m, kmax) frequencies, each column
                         summing to 2^15, on the host, pure integers
  index_ans_stream_bytes indices (b, m), freq -> bytes of every stream
  pack_index_ans         indices (b, m), freq -> (packed, offsets,
                         rows_per_stream), offsets in BYTES, one per stream
  unpack_index_ans       (packed, offsets), freq, b, rows_per_stream -> indices

The 15-bit tables of that coder stop at 4096 symbols a column.  The index of
the large vector quantiser (up to 131 072 codewords) is one column, coded as
two symbols, i >> 8 and i & 255, under the same states
(include/ext/vtc_index_ans_split.h):

  index_ans_split_frequencies   counts [kmax] -> (freq_hi uint16 [H], freq_lo
                                uint16 (H, 256)), H = ceil(kmax / 256)
  index_ans_split_stream_bytes  indices [b], tables -> bytes of every stream
  pack_index_ans_split          indices [b], tables -> (packed, offsets,
                                rows_per_stream)
  unpack_index_ans_split        (packed, offsets), tables, b, rows_per_stream
                                -> indices [b]

The R-D points of utils.quantization and utils.vector_quantization name none
of these functions.  Each source code is described once, at the end of this
module (Entropy, Huffman, Ans and AnsSplit, by name in SOURCE_CODES): its
symbol limit, what its tables are called, and train / total_bits / pack /
unpack.  Packed streams travel as a StreamSet, whose total is in bits whatever
its coder's offsets count; the two range coders' wrappers share one body.

The per-entry work runs in the kernels of csrc/index_code.hip behind
include/vtc_index_code.h, for the way back of
csrc/index_decode.hip behind include/vtc_index_decode.h, and
of csrc/index_ans.hip and csrc/index_ans_split.hip.  Indices are (b, m) int32
device tensors: m index streams ("columns") per row, each with a table of its
own, {int index: str of '0' / '1'}, or a row of frequencies.
"""
import collections

import numpy as np
import torch

import vtc_hip
from utils import jpeg

ABSENT = vtc_hip.INDEX_CODE_ABSENT
MAX_COLUMNS = vtc_hip.INDEX_CODE_MAX_COLUMNS
MAX_SYMBOLS = vtc_hip.INDEX_CODE_MAX_SYMBOLS


# ------------------------------------------------------------------ host side
def _host_rows(counts):
  """The rows of a 2-d count array as lists of Python integers (a weight may
  exceed int64 in a constructed table)."""
  if torch.is_tensor(counts):
    counts = counts.cpu().numpy()
  if isinstance(counts, np.ndarray):
    if counts.ndim == 1:
      counts = counts[None, :]
    if counts.ndim != 2:
      raise ValueError('counts must be (m, kmax), got shape %s'
                       % (counts.shape,))
    counts = counts.tolist()
  rows = [[int(c) for c in row] for row in counts]
  if not rows or not rows[0] or len(set(len(row) for row in rows)) != 1:
    raise ValueError('counts must be (m, kmax) with m, kmax >= 1')
  return rows


def _in_use(k, m, kmax):
  """The codewords in use of m columns of kmax slots as m ints: k as
  index_huffman_tables takes it."""
  if k is None:
    k = [kmax] * m
  else:
    if torch.is_tensor(k):
      k = k.cpu().numpy()
    k = [int(v) for v in np.asarray(k).reshape(-1)]
    if len(k) == 1:
      k = k * m
  if len(k) != m or min(k) < 1 or max(k) > kmax:
    raise ValueError('k must hold %d values in [1, %d]' % (m, kmax))
  return k


def index_huffman_tables(counts, k=None):
  """One Huffman table per column: a list of m dicts {index: codeword}.

  counts : (m, kmax) integers, what quantization.index_counts or
      vector_quantization.vector_index_counts (a [kmax] row is one column)
      return for the training indices; device tensor, array or lists
  k : the codewords in use of each column's codebook, m integers or one for
      all; None for kmax

  Every index i < k[j] that was not seen enters with weight 1, the rule
  jpeg.tables_from_counts applies to unseen JPEG symbols; seen indices keep
  their counts; indices >= k[j] are absent.  So every index that an `assign`
  against the same codebook can produce is codable, whatever data it is run
  on.  The code is jpeg.compute_huffman_table of those weights: its list
  ordering settles ties deterministically for integer symbols.  A column with
  k[j] = 1 gets {0: ''}, a code of no bits."""
  rows = _host_rows(counts)
  m, kmax = len(rows), len(rows[0])
  k = _in_use(k, m, kmax)
  return [jpeg.compute_huffman_table(
      {i: (row[i] if row[i] > 0 else 1) for i in range(k[j])})
          for j, row in enumerate(rows)]


def tables_kmax(tables):
  """The smallest kmax that holds every symbol of the tables."""
  return max(max(table) for table in tables) + 1


def index_table_arrays(tables, kmax):
  """(code uint64 (m, kmax), len uint8 (m, kmax)) of a list of m tables: the
  codeword right-aligned, 255 where the table lacks the symbol.  A codeword
  of more than 64 bits raises NotImplementedError, as jpeg.table_arrays
  does."""
  m, kmax = len(tables), int(kmax)
  code = np.zeros((m, kmax), dtype=np.uint64)
  length = np.full((m, kmax), ABSENT, dtype=np.uint8)
  for j, table in enumerate(tables):
    for index, word in table.items():
      if len(word) > jpeg.MAX_CODE_BITS:
        raise NotImplementedError(
            'codeword of %d bits for index %r of column %d: the device '
            'packer takes at most %d' % (len(word), index, j,
                                         jpeg.MAX_CODE_BITS))
      if not 0 <= index < kmax:
        raise ValueError('index %r of column %d falls outside [0, %d)'
                         % (index, j, kmax))
      code[j, index] = int(word, 2) if word else 0
      length[j, index] = len(word)
  return code, length


# ---------------------------------------------------------------- device side
def _indices(indices):
  indices = vtc_hip.require_device_tensor(indices, 'indices', torch.int32)
  if indices.dim() == 1:
    indices = indices[:, None]
  if indices.dim() != 2 or indices.numel() == 0:
    raise ValueError('indices must be (b, m), got shape %s'
                     % (tuple(indices.shape),))
  return indices.contiguous()


class _DeviceTables(object):
  def __init__(self, tables, m, device):
    tables = list(tables)
    if len(tables) != m:
      raise ValueError('%d tables for %d columns' % (len(tables), m))
    if m > MAX_COLUMNS:
      raise NotImplementedError('m = %d, at most %d' % (m, MAX_COLUMNS))
    self.kmax = tables_kmax(tables)
    if self.kmax > MAX_SYMBOLS:
      raise NotImplementedError('kmax = %d, at most %d'
                                % (self.kmax, MAX_SYMBOLS))
    code, length = index_table_arrays(tables, self.kmax)
    # uint64 as int64 bits: torch moves bytes
    self.code = torch.from_numpy(code.view(np.int64)).to(device)
    self.len = torch.from_numpy(length).to(device)


def _raise_status(indices, status, what):
  uncodable, first, dropped = status.tolist()
  if uncodable:
    row, column = divmod(first - 1, indices.shape[1])
    raise KeyError('%s: column %d has no codeword for index %d (row %d); %d '
                   'such entries' % (what, column, int(indices[row, column]),
                                     row, uncodable))
  if dropped:
    raise ValueError('%s: %d stream bits outside the output' % (what, dropped))


def _bits(lib, indices, tables, status):
  b, m = indices.shape
  device = indices.device
  row_bits = torch.empty(b, dtype=torch.int32, device=device)
  column_bits = torch.empty(m, dtype=torch.int64, device=device)
  vtc_hip.check(lib.vtc_index_code_bits(
      vtc_hip.ptr(indices), b, m, vtc_hip.ptr(tables.len), tables.kmax,
      vtc_hip.ptr(row_bits), vtc_hip.ptr(column_bits), vtc_hip.ptr(status),
      vtc_hip.current_stream(device)), 'vtc_index_code_bits')
  return row_bits, column_bits


def index_code_bits(indices, tables):
  """(row_bits int32 [b], column_bits int64 [m]) device tensors: the length of
  every row's stream, sum(len(tables[j][indices[r, j]])), and the same
  lengths summed down each column.  One host read (the status).  An index its
  column's table lacks (the -1 of a NaN code among them) raises KeyError
  naming the column and the index."""
  lib = vtc_hip.load_library()
  indices = _indices(indices)
  tables = _DeviceTables(tables, indices.shape[1], indices.device)
  status = torch.empty(3, dtype=torch.int64, device=indices.device)
  out = _bits(lib, indices, tables, status)
  _raise_status(indices, status, 'index_code_bits')
  return out


def pack_index_streams(indices, tables):
  """(packed, offsets): the streams of all rows back to back in one uint8
  device tensor, most significant bit first (the last byte zero-padded), and
  the (b + 1,) int64 device tensor of the bit at which each row's stream
  starts, the total last -- the return shapes of jpeg.pack_streams.  Row r's
  stream is ''.join(tables[j][indices[r, j]] for j in range(m))."""
  lib = vtc_hip.load_library()
  indices = _indices(indices)
  b, m = indices.shape
  device = indices.device
  tables = _DeviceTables(tables, m, device)
  status = torch.empty(3, dtype=torch.int64, device=device)
  row_bits, _ = _bits(lib, indices, tables, status)
  _raise_status(indices, status, 'pack_index_streams')
  offsets = jpeg.bit_offsets(row_bits)
  total = int(offsets[b])
  packed = torch.empty(max(1, -(-total // 8)), dtype=torch.uint8,
                       device=device)
  vtc_hip.check(lib.vtc_index_code_pack(
      vtc_hip.ptr(indices), b, m, vtc_hip.ptr(tables.code),
      vtc_hip.ptr(tables.len), tables.kmax, vtc_hip.ptr(offsets),
      vtc_hip.ptr(packed), packed.numel(), vtc_hip.ptr(status),
      vtc_hip.current_stream(device)), 'vtc_index_code_pack')
  _raise_status(indices, status, 'pack_index_streams')
  return packed, offsets


# ------------------------------------------------------------------ decoding
def unpack_index_streams(packed, offsets, tables, exact=True):
  """indices (b, m) int32 device tensor from what pack_index_streams returns:
  packed a uint8 device tensor, offsets the (b + 1,) int64 device tensor of the
  bit at which each row's stream starts, the total last; m = len(tables).  Row
  r reads one codeword per column from bit offsets[r] on and may use the bits
  below offsets[r + 1].

  ValueError for a column whose table is not prefix-free (before any device
  work; {0: ''} alone is fine), for malformed rows (their number, the first one
  and its first undecoded column named; include/vtc_index_decode.h lists what
  makes a row malformed) and, with exact=True, for rows that leave bits of
  their span offsets[r + 1] - offsets[r] unread.  NotImplementedError for a
  codeword of more than 64 bits, VtcHipError for a CPU tensor.  One host read
  in all."""
  tables = list(tables)
  for j, table in enumerate(tables):
    try:
      jpeg.check_prefix_free(table)
    except ValueError as e:
      raise ValueError('column %d: %s' % (j, e))
  packed = vtc_hip.require_device_tensor(packed, 'packed', torch.uint8)
  offsets = vtc_hip.require_device_tensor(offsets, 'offsets', torch.int64)
  if packed.dim() != 1 or offsets.dim() != 1 or offsets.shape[0] < 2:
    raise ValueError('packed must be (bytes,) and offsets (b + 1,), got '
                     'shapes %s and %s' % (tuple(packed.shape),
                                           tuple(offsets.shape)))
  lib = vtc_hip.load_library()
  packed, offsets = packed.contiguous(), offsets.contiguous()
  device = packed.device
  b, m = offsets.shape[0] - 1, len(tables)
  tables = _DeviceTables(tables, m, device)
  indices = torch.empty((b, m), dtype=torch.int32, device=device)
  row_bits = torch.empty(b, dtype=torch.int32, device=device)
  status = torch.empty(3, dtype=torch.int64, device=device)
  ws = vtc_hip.workspace(
      lib.vtc_index_code_unpack_workspace_bytes(m, tables.kmax), device)
  # a tensor without elements has a null data pointer; the call wants one
  # that is not null and never reads it when there are no bytes
  bits_from = packed if packed.numel() else ws
  vtc_hip.check(lib.vtc_index_code_unpack(
      vtc_hip.ptr(bits_from), packed.numel(), vtc_hip.ptr(offsets), b, m,
      vtc_hip.ptr(tables.code), vtc_hip.ptr(tables.len), tables.kmax,
      vtc_hip.ptr(indices), vtc_hip.ptr(row_bits), vtc_hip.ptr(status),
      vtc_hip.ptr(ws), ws.numel(), vtc_hip.current_stream(device)),
                'vtc_index_code_unpack')
  # what the message needs, gathered on the device for the one host read: the
  # first malformed row's first undecoded column, and the rows that did not
  # use up their span (tensor plumbing, b elements)
  first_row = (status[1] - 1).clamp(min=0)
  undecoded = (indices.index_select(0, first_row.reshape(1))[0] < 0)
  column = undecoded.to(torch.int32).argmax().to(torch.int64)
  loose = row_bits.to(torch.int64) != offsets[1:] - offsets[:-1]
  report = torch.stack([status[0], status[1], status[2], column,
                        loose.sum(), loose.to(torch.int32).argmax()])
  malformed, first, clash, column, loose, first_loose = report.tolist()
  if clash:   # the host check above saw the same tables
    raise ValueError('not a prefix-free table: column %d, index %d'
                     % divmod(clash - 1, tables.kmax))
  if malformed:
    raise ValueError('unpack_index_streams: %d malformed rows of %d, the '
                     'first is row %d, undecoded from column %d on'
                     % (malformed, b, first - 1, column))
  if exact and loose:
    raise ValueError('unpack_index_streams: %d rows of %d do not use up their '
                     'span of bits, the first is row %d'
                     % (loose, b, first_loose))
  return indices


def parse_index_stream(stream, tables):
  """The inverse of ''.join(tables[j][i] for j, i in enumerate(indices)) for
  one row: the list of m ints whose stream is the string `stream` of '0' and
  '1'.  Through the batch path with b = 1, on the current HIP device."""
  if not isinstance(stream, str) or set(stream) - set('01'):
    raise TypeError("stream must be a str of '0' and '1'")
  device = torch.device('cuda')
  bits = np.frombuffer(stream.encode('ascii'), dtype=np.uint8) - ord('0')
  host = np.packbits(bits) if len(stream) else np.zeros(1, dtype=np.uint8)
  ends = np.array([0, len(stream)], dtype=np.int64)
  indices = unpack_index_streams(torch.from_numpy(host).to(device),
                                 torch.from_numpy(ends).to(device), tables)
  return [int(i) for i in indices[0].tolist()]


# ------------------------------------------------------------- range coding
ANS_PROB_BITS = vtc_hip.INDEX_ANS_PROB_BITS
ANS_MAX_STREAM_SYMBOLS = 1 << vtc_hip.INDEX_ANS_MAX_STREAM_BITS


def index_ans_frequencies(counts, k=None):
  """uint16 numpy array (m, kmax): the frequencies of the range coder, every
  column summing to 2^15, from the (m, kmax) counts and the codewords in use k
  that index_huffman_tables takes.  On the host, Python integers only:

  1. the weight w_i is count_i, or 1 when count_i = 0, for every i < k[j] (so
     every index the codebook can produce is codable); 0 for i >= k[j];
  2. f_i = max(1, floor(w_i * 2^15 / W)) for i < k[j], W = sum w_i;
  3. the difference 2^15 - sum f is given out, or taken back, one unit at a
     time, going round the symbols in order of (-w_i, i) and skipping symbols
     at f = 1 when taking."""
  rows = _host_rows(counts)
  m, kmax = len(rows), len(rows[0])
  if kmax > MAX_SYMBOLS:
    raise NotImplementedError('kmax = %d, at most %d' % (kmax, MAX_SYMBOLS))
  k = _in_use(k, m, kmax)
  freq = np.zeros((m, kmax), dtype=np.uint16)
  for j, row in enumerate(rows):
    kj = k[j]
    if min(row[:kj]) < 0:
      raise ValueError('column %d has a negative count' % j)
    freq[j, :kj] = _ans_weights_to_frequencies(
        [c if c > 0 else 1 for c in row[:kj]])
  return freq


def _ans_weights_to_frequencies(w):
  """Steps 2 and 3 of the rule of index_ans_frequencies for the positive
  weights w of the symbols in use: as many frequencies, >= 1, summing to
  2^15."""
  scale = 1 << ANS_PROB_BITS
  kj = len(w)
  total = sum(w)
  f = [max(1, (wi << ANS_PROB_BITS) // total) for wi in w]
  order = sorted(range(kj), key=lambda i: (-w[i], i))
  d = scale - sum(f)
  # one unit at a time round the order, whole rounds taken at once
  if d > 0:
    rounds, rest = divmod(d, kj)
    for rank, i in enumerate(order):
      f[i] += rounds + (1 if rank < rest else 0)
  while d < 0:
    open_ = [i for i in order if f[i] > 1]   # not empty: sum f > 2^15 >= k
    rounds = min(-d // len(open_), min(f[i] for i in open_) - 1)
    if rounds:
      for i in open_:
        f[i] -= rounds
      d += rounds * len(open_)
    else:                                    # a last, partial round
      for i in open_[:-d]:
        f[i] -= 1
      d = 0
  return f


def _ans_freq(freq, m, device):
  """The (m, kmax) uint16 frequencies as a device tensor of int16 bit
  patterns (torch moves bytes), and kmax."""
  if torch.is_tensor(freq):
    freq = freq.cpu().numpy()
  freq = np.asarray(freq)
  if freq.ndim == 1:
    freq = freq[None, :]
  if freq.dtype != np.uint16 or freq.ndim != 2 or freq.shape[1] < 1:
    raise ValueError('freq must be a uint16 (m, kmax) array')
  if freq.shape[0] != m:
    raise ValueError('%d rows of frequencies for %d columns'
                     % (freq.shape[0], m))
  if m > MAX_COLUMNS:
    raise NotImplementedError('m = %d, at most %d' % (m, MAX_COLUMNS))
  if freq.shape[1] > MAX_SYMBOLS:
    raise NotImplementedError('kmax = %d, at most %d'
                              % (freq.shape[1], MAX_SYMBOLS))
  sums = freq.astype(np.int64).sum(1)
  wrong = np.nonzero(sums != 1 << ANS_PROB_BITS)[0]
  if len(wrong):
    raise ValueError('the frequencies of column %d sum to %d, not 2^%d'
                     % (wrong[0], sums[wrong[0]], ANS_PROB_BITS))
  host = np.ascontiguousarray(freq).view(np.int16)
  return torch.from_numpy(host).to(device), int(freq.shape[1])


def _ans_rows(rows_per_stream, m):
  if rows_per_stream is None:
    return max(1, 65536 // m)
  rows = int(rows_per_stream)
  if rows < 1 or rows * m > ANS_MAX_STREAM_SYMBOLS:
    raise ValueError('rows_per_stream = %d: at least 1 and at most %d symbols '
                     'in a stream' % (rows, ANS_MAX_STREAM_SYMBOLS))
  return rows


def _ans_bad(what, bad):
  # _ans_freq saw the same frequencies
  raise ValueError('%s: the frequencies of column %d do not sum to 2^%d'
                   % (what, bad - 1, ANS_PROB_BITS))


def _ans_streams(packed, offsets, b, rows):
  """The number of streams of b rows, `rows` each, after the check that
  `packed` and `offsets` have the shapes of that many."""
  n = -(-b // rows)
  if packed.dim() != 1 or offsets.dim() != 1 or offsets.shape[0] != n + 1:
    raise ValueError('packed must be (bytes,) and offsets (%d,) for %d rows in '
                     'streams of %d, got shapes %s and %s'
                     % (n + 1, b, rows, tuple(packed.shape),
                        tuple(offsets.shape)))
  return n


def _raise_ans_skipped(what, status):
  skipped = int(status[2])
  if skipped:
    raise ValueError('%s: %d streams outside the output' % (what, skipped))


def _raise_ans_unpack_status(what, bad_tables, status, used, offsets, rows,
                             exact):
  """The end of an unpack call, one host read: bad tables (bad_tables(what,
  bad) raises), malformed streams, and with `exact` streams that leave bytes
  of their span unread."""
  n = used.shape[0]
  loose = used.to(torch.int64) != offsets[1:] - offsets[:-1]
  report = torch.cat([status, torch.stack([
      loose.sum(), loose.to(torch.int32).argmax().to(torch.int64)])])
  malformed, first, bad, loose, first_loose = report.tolist()
  if bad:
    bad_tables(what, bad)
  if malformed:
    raise ValueError('%s: %d malformed streams of %d, the first is stream %d '
                     '(rows %d and on)'
                     % (what, malformed, n, first - 1, (first - 1) * rows))
  if exact and loose:
    raise ValueError('%s: %d streams of %d do not use up their span of bytes, '
                     'the first is stream %d' % (what, loose, n, first_loose))


def _raise_ans_status(indices, status, what):
  uncodable, first, bad = status.tolist()
  if bad:
    _ans_bad(what, bad)
  if uncodable:
    row, column = divmod(first - 1, indices.shape[1])
    raise KeyError('%s: column %d has no frequency for index %d (row %d); %d '
                   'such entries' % (what, column, int(indices[row, column]),
                                     row, uncodable))


def _ans_columns(freq):
  host = freq.cpu().numpy() if torch.is_tensor(freq) else np.asarray(freq)
  return 1 if host.ndim == 1 else host.shape[0]


# What the shared body of the two range coders' wrappers asks of a coder: the
# prefix `entry` of its C entry points; many_columns, whether they take m (the
# split coder has one column); indices -> the tensor the calls read; columns:
# tables -> m; tables: (tables, m, device) -> the checked tables as device
# tensors, then kmax; rows: (rows_per_stream, m) -> the rows of a stream; the
# raisers raise_status(indices, status, what) and raise_bad(what, bad).
_RangeCalls = collections.namedtuple(
    '_RangeCalls', 'entry many_columns indices columns tables rows '
    'raise_status raise_bad')


def _range_tables(coder, lib, tables, m, device):
  """(the device tables, kept alive for the calls; what every C call takes
  between b and the rows of a stream: [m,] the tables' pointers, kmax; the
  workspace; the status word)."""
  *held, kmax = coder.tables(tables, m, device)
  dims = (m,) if coder.many_columns else ()
  ws = vtc_hip.workspace(
      getattr(lib, coder.entry + '_workspace_bytes')(*dims, kmax), device)
  status = torch.empty(3, dtype=torch.int64, device=device)
  return (held, dims + tuple(vtc_hip.ptr(t) for t in held) + (kmax,), ws,
          status)


def _range_encode(coder, what, indices, tables, rows_per_stream, pack):
  """The body of index_ans[_split]_stream_bytes (pack false: the sizes) and
  of pack_index_ans[_split] (pack true: packed, offsets, rows)."""
  lib = vtc_hip.load_library()
  indices = coder.indices(indices)
  b, device = indices.shape[0], indices.device
  m = indices.shape[1] if coder.many_columns else 1
  rows = coder.rows(rows_per_stream, m)
  held, middle, ws, status = _range_tables(coder, lib, tables, m, device)
  stream = vtc_hip.current_stream(device)
  sizes = torch.empty(-(-b // rows), dtype=torch.int32, device=device)
  vtc_hip.check(getattr(lib, coder.entry + '_sizes')(
      vtc_hip.ptr(indices), b, *middle, rows, vtc_hip.ptr(sizes),
      vtc_hip.ptr(status), vtc_hip.ptr(ws), ws.numel(), stream),
                coder.entry + '_sizes')
  coder.raise_status(indices, status, what)
  if not pack:
    return sizes
  offsets = jpeg.bit_offsets(sizes)   # a plain prefix sum: of bytes here
  total = int(offsets[-1])
  packed = torch.empty(total, dtype=torch.uint8, device=device)
  vtc_hip.check(getattr(lib, coder.entry + '_pack')(
      vtc_hip.ptr(indices), b, *middle, rows, vtc_hip.ptr(sizes),
      vtc_hip.ptr(offsets), vtc_hip.ptr(packed), total, vtc_hip.ptr(status),
      vtc_hip.ptr(ws), ws.numel(), stream), coder.entry + '_pack')
  _raise_ans_skipped(what, status)
  return packed, offsets, rows


def _range_unpack(coder, what, packed, offsets, tables, b, rows_per_stream,
                  exact):
  """The body of unpack_index_ans[_split]."""
  packed = vtc_hip.require_device_tensor(packed, 'packed', torch.uint8)
  offsets = vtc_hip.require_device_tensor(offsets, 'offsets', torch.int64)
  b = int(b)
  m = coder.columns(tables)
  if b < 1:
    raise ValueError('b must be at least 1')
  rows = coder.rows(rows_per_stream, m)
  n = _ans_streams(packed, offsets, b, rows)
  lib = vtc_hip.load_library()
  packed, offsets = packed.contiguous(), offsets.contiguous()
  device = packed.device
  held, middle, ws, status = _range_tables(coder, lib, tables, m, device)
  indices = torch.empty((b, m) if coder.many_columns else b,
                        dtype=torch.int32, device=device)
  used = torch.empty(n, dtype=torch.int32, device=device)
  bytes_from = packed if packed.numel() else ws   # never read when empty
  vtc_hip.check(getattr(lib, coder.entry + '_unpack')(
      vtc_hip.ptr(bytes_from), packed.numel(), vtc_hip.ptr(offsets), b,
      *middle, rows, vtc_hip.ptr(indices), vtc_hip.ptr(used),
      vtc_hip.ptr(status), vtc_hip.ptr(ws), ws.numel(),
      vtc_hip.current_stream(device)), coder.entry + '_unpack')
  _raise_ans_unpack_status(what, coder.raise_bad, status, used, offsets, rows,
                           exact)
  return indices


_ANS = _RangeCalls('vtc_index_ans', True, _indices, _ans_columns, _ans_freq,
                   _ans_rows, _raise_ans_status, _ans_bad)


def index_ans_stream_bytes(indices, freq, rows_per_stream=None):
  """int32 device tensor [ceil(b / rows_per_stream)]: the bytes of every
  stream of the (b, m) indices under the (m, kmax) frequencies, 256 of end
  states and two per word.  rows_per_stream defaults to max(1, 65536 // m),
  which puts the 256-byte flush at about 0.03 bit per index.  One host read
  (the status).  An index of frequency 0 (the -1 of a NaN code among them)
  raises KeyError naming the column and the index."""
  return _range_encode(_ANS, 'index_ans_stream_bytes', indices, freq,
                       rows_per_stream, False)


def pack_index_ans(indices, freq, rows_per_stream=None):
  """(packed, offsets, rows_per_stream): the range-coded streams of the (b, m)
  indices back to back in one uint8 device tensor, the (n + 1,) int64 device
  tensor of the BYTE at which each of the n = ceil(b / rows_per_stream)
  streams starts, the total last, and the rows of a stream (the default of
  index_ans_stream_bytes when None), which the decoder needs again.  Stream s
  holds rows s * rows_per_stream and on in row-major order
  (include/vtc_index_ans.h)."""
  return _range_encode(_ANS, 'pack_index_ans', indices, freq, rows_per_stream,
                       True)


def unpack_index_ans(packed, offsets, freq, b, rows_per_stream, exact=True):
  """indices (b, m) int32 device tensor from what pack_index_ans returns;
  m = len(freq).  Stream s reads from byte offsets[s] on and may use the bytes
  below offsets[s + 1].

  ValueError for frequencies that do not sum to 2^15 (before any device
  work), for malformed streams (their number and the first one named;
  include/vtc_index_ans.h lists what makes a stream malformed: bad offsets, a
  slot without its 256 bytes of states, a stream that runs out of words, end
  states that are not 2^16) and, with exact=True, for streams that leave bytes
  of their span unread.  VtcHipError for a CPU tensor.  One host read."""
  return _range_unpack(_ANS, 'unpack_index_ans', packed, offsets, freq, b,
                       rows_per_stream, exact)


# ------------------------------------- range coding, more than 4096 symbols
ANS_SPLIT_MAX_SYMBOLS = vtc_hip.INDEX_ANS_SPLIT_MAX_SYMBOLS
ANS_SPLIT_LO_SYMBOLS = 1 << vtc_hip.INDEX_ANS_SPLIT_LO_BITS
ANS_SPLIT_ROWS = 65536   # rows of a stream when the caller names none


def index_ans_split_frequencies(counts, k=None):
  """(freq_hi uint16 [H], freq_lo uint16 (H, 256)) numpy arrays, H =
  ceil(kmax / 256): the tables of the split range coder
  (include/ext/vtc_index_ans_split.h) from the [kmax] counts of one index column
  (vector_quantization.vector_index_counts) and the codewords in use k (None
  for kmax).  On the host, Python integers only:

  1. the weight w_i is count_i, or 1 when count_i = 0, for i < k; 0 from k on;
  2. row h of freq_lo: the rule of index_ans_frequencies on the counts of
     block h (indices 256 h .. 256 h + 255) with k_h = clamp(k - 256 h, 0,
     256) symbols in use; a row with k_h = 0 is all zero;
  3. freq_hi: steps 2 and 3 of that rule on the block weights W_h = sum of the
     w_i of block h, for the ceil(k / 256) blocks in use; 0 beyond.

  Every index below k stays codable.  NotImplementedError for kmax >
  131072."""
  if (isinstance(counts, (list, tuple)) and counts and
      not hasattr(counts[0], '__len__')):
    counts = [counts]          # a plain row of Python integers
  rows = _host_rows(counts)
  if len(rows) != 1:
    raise ValueError('counts must hold one column, got %d' % len(rows))
  row = rows[0]
  kmax = len(row)
  if kmax > ANS_SPLIT_MAX_SYMBOLS:
    raise NotImplementedError('kmax = %d, at most %d'
                              % (kmax, ANS_SPLIT_MAX_SYMBOLS))
  if k is None:
    k = kmax
  else:
    if torch.is_tensor(k):
      k = k.cpu().numpy()
    k = np.asarray(k).reshape(-1)
    if len(k) != 1:
      raise ValueError('k must be one value')
    k = int(k[0])
  if not 1 <= k <= kmax:
    raise ValueError('k must lie in [1, %d]' % kmax)
  if min(row[:k]) < 0:
    raise ValueError('the column has a negative count')
  lo = ANS_SPLIT_LO_SYMBOLS
  top = -(-kmax // lo)
  freq_hi = np.zeros(top, dtype=np.uint16)
  freq_lo = np.zeros((top, lo), dtype=np.uint16)
  block_weights = []
  for h in range(-(-k // lo)):
    w = [c if c > 0 else 1 for c in row[lo * h:min(k, lo * (h + 1))]]
    freq_lo[h, :len(w)] = _ans_weights_to_frequencies(w)
    block_weights.append(sum(w))
  freq_hi[:len(block_weights)] = _ans_weights_to_frequencies(block_weights)
  return freq_hi, freq_lo


def _ans_split_tables(tables, device):
  """(freq_hi, freq_lo) as device tensors of int16 bit patterns, and the kmax
  the calls are given: 256 H, every symbol the tables can hold."""
  try:
    freq_hi, freq_lo = tables
  except (TypeError, ValueError):
    raise ValueError('tables must be the pair (freq_hi, freq_lo)')
  host = []
  for freq in (freq_hi, freq_lo):
    if torch.is_tensor(freq):
      freq = freq.cpu().numpy()
    host.append(np.asarray(freq))
  freq_hi, freq_lo = host
  lo = ANS_SPLIT_LO_SYMBOLS
  if (freq_hi.dtype != np.uint16 or freq_lo.dtype != np.uint16 or
      freq_hi.ndim != 1 or freq_hi.shape[0] < 1 or
      freq_lo.shape != (freq_hi.shape[0], lo)):
    raise ValueError('tables must be uint16 arrays [H] and (H, %d)' % lo)
  top = freq_hi.shape[0]
  if top * lo > ANS_SPLIT_MAX_SYMBOLS:
    raise NotImplementedError('kmax = %d, at most %d'
                              % (top * lo, ANS_SPLIT_MAX_SYMBOLS))
  scale = 1 << ANS_PROB_BITS
  if int(freq_hi.astype(np.int64).sum()) != scale:
    raise ValueError('the hi frequencies sum to %d, not 2^%d'
                     % (int(freq_hi.astype(np.int64).sum()), ANS_PROB_BITS))
  sums = freq_lo.astype(np.int64).sum(1)
  wrong = np.nonzero((sums != scale) & (freq_hi > 0))[0]
  if len(wrong):
    raise ValueError('the lo frequencies of row %d sum to %d, not 2^%d'
                     % (wrong[0], sums[wrong[0]], ANS_PROB_BITS))
  return (torch.from_numpy(np.ascontiguousarray(freq_hi).view(np.int16))
          .to(device),
          torch.from_numpy(np.ascontiguousarray(freq_lo).view(np.int16))
          .to(device), top * lo)


def _ans_split_column(indices):
  indices = vtc_hip.require_device_tensor(indices, 'indices', torch.int32)
  if indices.dim() == 2 and indices.shape[1] == 1:
    indices = indices[:, 0]
  if indices.dim() != 1 or indices.numel() == 0:
    raise ValueError('indices must be [b], one column, got shape %s'
                     % (tuple(indices.shape),))
  return indices.contiguous()


def _ans_split_rows(rows_per_stream, m=1):
  if rows_per_stream is None:
    return ANS_SPLIT_ROWS
  rows = int(rows_per_stream)
  if rows < 1 or rows > ANS_MAX_STREAM_SYMBOLS:
    raise ValueError('rows_per_stream = %d: at least 1 and at most %d symbols '
                     'in a stream' % (rows, ANS_MAX_STREAM_SYMBOLS))
  return rows


def _ans_split_bad(what, bad):
  # _ans_split_tables saw the same tables
  if bad == 1:
    raise ValueError('%s: the hi frequencies do not sum to 2^%d'
                     % (what, ANS_PROB_BITS))
  raise ValueError('%s: the lo frequencies of row %d do not sum to 2^%d or '
                   'are not 0 from kmax on' % (what, bad - 2, ANS_PROB_BITS))


def _raise_ans_split_status(indices, status, what):
  uncodable, first, bad = status.tolist()
  if bad:
    _ans_split_bad(what, bad)
  if uncodable:
    raise KeyError('%s: no frequency for index %d (row %d); %d such entries'
                   % (what, int(indices[first - 1]), first - 1, uncodable))


_ANS_SPLIT = _RangeCalls(
    'vtc_index_ans_split', False, _ans_split_column, lambda tables: 1,
    lambda tables, m, device: _ans_split_tables(tables, device),
    _ans_split_rows, _raise_ans_split_status, _ans_split_bad)


def index_ans_split_stream_bytes(indices, tables, rows_per_stream=None):
  """int32 device tensor [ceil(b / rows_per_stream)]: the bytes of every
  stream of the [b] indices under tables = (freq_hi, freq_lo), 256 of end
  states and two per word.  rows_per_stream defaults to 65536.  One host read
  (the status).  An index without a frequency (the -1 of a NaN code among
  them) raises KeyError naming its row and the index; tables whose sums are
  not 2^15 raise ValueError before any device work."""
  return _range_encode(_ANS_SPLIT, 'index_ans_split_stream_bytes', indices,
                       tables, rows_per_stream, False)


def pack_index_ans_split(indices, tables, rows_per_stream=None):
  """(packed, offsets, rows_per_stream) of the [b] indices under tables =
  (freq_hi, freq_lo): what pack_index_ans returns, for the streams of
  include/ext/vtc_index_ans_split.h."""
  return _range_encode(_ANS_SPLIT, 'pack_index_ans_split', indices, tables,
                       rows_per_stream, True)


def unpack_index_ans_split(packed, offsets, tables, b, rows_per_stream,
                           exact=True):
  """indices [b] int32 device tensor from what pack_index_ans_split returns.
  Errors are those of unpack_index_ans: ValueError for bad sums (before any
  device work), for malformed streams and, with exact=True, for streams that
  leave bytes of their span unread; VtcHipError for a CPU tensor.  One host
  read."""
  return _range_unpack(_ANS_SPLIT, 'unpack_index_ans_split', packed, offsets,
                       tables, b, rows_per_stream, exact)


# ------------------------------------------------ the source codes, described
# One set of index streams with what its decoder needs beside the tables:
# packed and offsets of the coder's pack function, the rows b and
# rows_per_stream (both None for Huffman streams, one per row, that come from
# outside) and the total in BITS (None for a set from outside).  Whether the
# offsets count bits or bytes is the coder's business alone.
StreamSet = collections.namedtuple(
    'StreamSet', 'packed offsets b rows_per_stream bits')


class Entropy(object):
  """source_code 'entropy': the empirical entropy of the indices, a figure
  (quantization.entropy_bits of their counts) and no code.  No tables, no
  streams, any number of symbols."""
  name = 'entropy'
  max_symbols = float('inf')
  one_column = False
  has_tables = writes_streams = False


class _TableCode(object):
  """What the R-D points of utils.quantization and utils.vector_quantization
  ask of a source code with tables, no instance state: its name; max_symbols,
  the most a column may have; one_column, whether it takes [b] indices and not
  (b, m); tables_noun, its tables in the missing-tables message; and
    train(counts, k) -> tables
    total_bits(indices, tables, rows_per_stream), nothing written
    pack(indices, tables, rows_per_stream) -> StreamSet
    unpack(streams, tables) -> indices"""
  has_tables = writes_streams = True

  @classmethod
  def train_column(cls, counts, k):
    """The tables of one column from its [kmax] counts."""
    tables = cls.train(counts, k)
    return tables if cls.one_column else tables[0]


class Huffman(_TableCode):
  """source_code 'huffman': one prefix code per column; a stream per row,
  offsets in bits."""
  name = 'huffman'
  max_symbols = MAX_SYMBOLS
  one_column = False
  tables_noun = 'the Huffman tables'
  train = staticmethod(index_huffman_tables)

  @staticmethod
  def total_bits(indices, tables, rows_per_stream=None):
    return int(index_code_bits(indices, tables)[1].sum())

  @staticmethod
  def pack(indices, tables, rows_per_stream=None):
    packed, offsets = pack_index_streams(indices, tables)
    return StreamSet(packed, offsets, indices.shape[0], None,
                     int(offsets[-1]))

  @staticmethod
  def unpack(streams, tables):
    return unpack_index_streams(streams.packed, streams.offsets, tables)


class _RangeCode(_TableCode):
  """A range coder: streams of rows_per_stream rows, offsets in bytes, from
  its three wrappers stream_bytes, pack_streams and unpack_streams."""
  tables_noun = 'the frequencies'

  @classmethod
  def total_bits(cls, indices, tables, rows_per_stream=None):
    return 8 * int(cls.stream_bytes(indices, tables, rows_per_stream).sum())

  @classmethod
  def pack(cls, indices, tables, rows_per_stream=None):
    packed, offsets, rows = cls.pack_streams(indices, tables, rows_per_stream)
    return StreamSet(packed, offsets, indices.shape[0], rows,
                     8 * int(offsets[-1]))

  @classmethod
  def unpack(cls, streams, tables):
    return cls.unpack_streams(streams.packed, streams.offsets, tables,
                              streams.b, streams.rows_per_stream)


class Ans(_RangeCode):
  """source_code 'ans': one row of frequencies per column."""
  name = 'ans'
  max_symbols = MAX_SYMBOLS
  one_column = False
  train = staticmethod(index_ans_frequencies)
  stream_bytes = staticmethod(index_ans_stream_bytes)
  pack_streams = staticmethod(pack_index_ans)
  unpack_streams = staticmethod(unpack_index_ans)


class AnsSplit(_RangeCode):
  """source_code 'ans_split': the one column of the large vector quantiser's
  index under (freq_hi, freq_lo)."""
  name = 'ans_split'
  max_symbols = ANS_SPLIT_MAX_SYMBOLS
  one_column = True
  train = staticmethod(index_ans_split_frequencies)
  stream_bytes = staticmethod(index_ans_split_stream_bytes)
  pack_streams = staticmethod(pack_index_ans_split)
  unpack_streams = staticmethod(unpack_index_ans_split)


SOURCE_CODES = {code.name: code for code in (Entropy, Huffman, Ans, AnsSplit)}
