"""Builders for the tests of the baseline JFIF reader (utils/jfif.py,
include/ext/vtc_jfif_decode.h): the sequential decoder the device unpack must
equal, written from the header's text alone; the foreign files of
tests/golden/jfif_foreign.npz and how they were made; byte strings with one
header field changed; the three device-free restatements of the small calls.
numpy only."""
import io
import pathlib

import numpy as np

import jfif_data as truth

GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden' / 'jfif_foreign.npz'
SUBSEQ_BYTES = 128
GROUP_BYTES = 256 * SUBSEQ_BYTES

# name -> PIL's save arguments; the image is foreign_image()
FOREIGN = {
    'gray': dict(mode='L', quality=85, optimize=True),
    '444': dict(mode='RGB', quality=85, optimize=True, subsampling=0),
    '422': dict(mode='RGB', quality=85, optimize=True, subsampling=1),
    '420': dict(mode='RGB', quality=85, optimize=True, subsampling=2),
    '420-default-tables': dict(mode='RGB', quality=85, optimize=False,
                               subsampling=2),
}


def foreign_image():
  """uint8 (64, 96, 3): the seeded colour image of tests/color_data.py."""
  return np.rint(truth.colour_image(64, 96, seed=2024)).astype(np.uint8)


def make_foreign():
  """{name: uint8 bytes} written by PIL (needs PIL): what
  tests/golden/jfif_foreign.npz holds."""
  from PIL import Image
  out = {}
  rgb = foreign_image()
  for name, args in FOREIGN.items():
    args = dict(args)
    mode = args.pop('mode')
    picture = Image.fromarray(rgb)
    if mode == 'L':
      picture = picture.convert('L')
    buf = io.BytesIO()
    picture.save(buf, format='JPEG', **args)
    out[name] = np.frombuffer(buf.getvalue(), dtype=np.uint8).copy()
  return out


def load_foreign():
  with np.load(GOLDEN) as g:
    return {name: g[name].tobytes() for name in g.files}


# -------------------------------------------------------- the small calls
def unstuff(data):
  """(bytes, marker_at) as vtc_jfif_unstuff_bytes defines them."""
  data = bytes(data)
  marker_at = len(data)
  for i, b in enumerate(data):
    if b == 0xFF and (i + 1 >= len(data) or data[i + 1] != 0x00):
      marker_at = i
      break
  return data[:marker_at].replace(b'\xff\x00', b'\xff'), marker_at


def dc_accumulate(levels, order, start):
  """levels with column 0 accumulated along order, int32 wrapping."""
  out = np.array(levels, dtype=np.int32)
  d, acc = out.shape[0], 0
  for j in range(len(order)):
    if start[j]:
      acc = 0
    r = int(order[j])
    if 0 <= r < d:
      acc = (acc + int(out[r, 0])) & 0xFFFFFFFF
      out[r, 0] = acc - (1 << 32) if acc >> 31 else acc
  return out


def table_arrays(tables, codes=None):
  """ac_code (2, 256) uint16, ac_len uint8, dc_code (2, 16), dc_len of a list
  of two pairs of lengths (None: absent): canonical codewords."""
  out = {'ac_code': np.zeros((2, 256), np.uint16),
         'ac_len': np.zeros((2, 256), np.uint8),
         'dc_code': np.zeros((2, 16), np.uint16),
         'dc_len': np.zeros((2, 16), np.uint8)}
  for pair, table in enumerate(tables):
    if table is None:
      continue
    for key in ('ac', 'dc'):
      out[key + '_len'][pair] = table[key]
      for symbol, (code, _) in truth.canonical(table[key])[0].items():
        out[key + '_code'][pair, symbol] = code
  return out


# ------------------------------------------------- the sequential decoder
def _extend(value, size):
  return value if value >> (size - 1) else value - (1 << size) + 1


def sequential_unpack(segment, slot_dc, slot_ac, arrays, rows):
  """(levels int32 (rows, 64) with DIFF in column 0, [status0, status1,
  status2]) of the decoder include/ext/vtc_jfif_decode.h states: bits beyond
  the segment read as ones, a token must start inside the segment, the first
  malformed token stops the walk."""
  segment = bytes(segment)
  total = 8 * len(segment)
  padded = segment + b'\xff' * 8

  def peek(p, n):    # n <= 16 bits from bit p on
    word = int.from_bytes(padded[p >> 3:(p >> 3) + 4], 'big')
    return word >> (32 - (p & 7) - n) & (1 << n) - 1

  books = {}
  for kind, size in (('dc', 16), ('ac', 256)):
    for t in range(2):
      book = {}
      for s in range(size):
        length = min(int(arrays[kind + '_len'][t, s]), 16)
        if length:
          book[(length, int(arrays[kind + '_code'][t, s]) &
                (1 << length) - 1)] = s
      books[(kind, t)] = book

  def symbol(book, p):
    for length in range(1, 17):
      hit = book.get((length, peek(p, length)))
      if hit is not None:
        return hit, length
    return None, 0

  levels = np.zeros((rows, 64), dtype=np.int32)
  p, row = 0, 0
  while row < rows:
    slot = row % len(slot_dc)
    z = 0
    while True:
      if p >= total:
        return levels, [0, row, -1]
      if z == 0:
        s, length = symbol(books[('dc', 1 if slot_dc[slot] else 0)], p)
        if s is None or s > 11:
          return levels, [p + 1, row, -1]
        if s:
          levels[row, 0] = _extend(peek(p + length, s), s)
        p += length + s
        z = 1
        continue
      s, length = symbol(books[('ac', 1 if slot_ac[slot] else 0)], p)
      if s is None:
        return levels, [p + 1, row, -1]
      run, size = s >> 4, s & 15
      if size == 0:
        if s == 0x00:
          p += length
          break
        if s != 0xF0 or z + 16 > 64:
          return levels, [p + 1, row, -1]
        p += length
        z += 16
      else:
        if size > 10 or z + run > 63:
          return levels, [p + 1, row, -1]
        levels[row, z + run] = _extend(peek(p + length, size), size)
        p += length + size
        z += run + 1
      if z == 64:
        break
    row += 1
  return levels, [0, rows, p]


# ------------------------------------------------------------ constructed
def diffs_of(levels):
  """levels of one chain (row r predicted from row r - 1) with DIFF in
  column 0."""
  out = np.array(levels, dtype=np.int32)
  out[1:, 0] = out[1:, 0] - np.asarray(levels)[:-1, 0]
  return out


def chain(d):
  return np.arange(-1, d - 1, dtype=np.int32)


def one_table_layout(d):
  """What unpack_scan and dc_accumulate need of a layout, for d rows of one
  component."""
  start = np.zeros(d, dtype=np.uint8)
  start[0] = 1
  return {'rows': d, 'sampling': [(1, 1)],
          'order': np.arange(d, dtype=np.int32), 'start': start}


def pack_host(levels, tables=None):
  """(segment bytes, tables, bit offsets) of one chain of rows under table
  pair 0, by the restatement."""
  levels = np.ascontiguousarray(levels, dtype=np.int32)
  d = levels.shape[0]
  tokens = truth.scan_tokens(levels, chain(d), np.zeros(d, dtype=np.uint8))
  if tables is None:
    tables = truth.build_tables(*truth.count_symbols(tokens))
  raw, _, offsets = truth.pack_tokens(tokens, tables)
  return raw, tables, offsets


def token_spans(levels, tables):
  """[(start, end of codeword, end of value bits, ends its block)] in bits,
  of every token of one chain of rows under table pair 0."""
  levels = np.ascontiguousarray(levels, dtype=np.int32)
  d = levels.shape[0]
  codes = {key: truth.canonical(tables[0][key])[0] for key in ('dc', 'ac')}
  out, at = [], 0
  for _, block in truth.scan_tokens(levels, chain(d),
                                    np.zeros(d, dtype=np.uint8)):
    for i, (kind, symbol, _, size) in enumerate(block):
      length = codes[kind][symbol][1]
      out.append((at, at + length, at + length + size, i == len(block) - 1))
      at += length + size
  return out


def token_rows():
  """The constructed rows of tests/test_jfif_gpu.py: zero runs around the
  0xF0 boundary, every size of both signs, a coefficient at index 63 followed
  by the next block's DC, an end of block as the last bits."""
  rows = []
  for run in (15, 16, 17, 31, 32, 62):
    first = np.zeros(64, dtype=np.int32)
    first[0], first[1 + run] = 3, -2
    rows.append(first)
    if run + 3 <= 63:
      between = np.zeros(64, dtype=np.int32)
      between[1], between[2 + run] = 5, 7
      rows.append(between)
      last = np.zeros(64, dtype=np.int32)
      last[62 - run], last[63] = -1, 1
      rows.append(last)
  ac = [2 ** k - 1 for k in range(1, 11)] + [2 ** k for k in range(0, 10)]
  for sign in (1, -1):
    for at in range(0, len(ac), 9):
      row = np.zeros(64, dtype=np.int32)
      for j, m in enumerate(ac[at:at + 9]):
        row[1 + 7 * j] = sign * m
      rows.append(row)
  dc = [2 ** k - 1 for k in range(1, 12)] + [2 ** k for k in range(0, 11)]
  for m in dc:       # DIFF = m, then -m: a DC level, then 0 again
    row = np.zeros(64, dtype=np.int32)
    row[0] = m
    rows += [row, np.zeros(64, dtype=np.int32)]
  only63 = np.zeros(64, dtype=np.int32)
  only63[0], only63[63] = 4, -9
  rows.append(only63)                       # index 63, then the next DC
  dense = np.arange(64, dtype=np.int32) % 5 - 2
  dense[0] = 7
  rows.append(dense)
  rows.append(np.zeros(64, dtype=np.int32))    # an end of block, last bits
  return np.stack(rows)


def geometric_tail_tables():
  """One table pair whose AC table holds all 256 symbols with counts in a
  geometric tail: package-merge gives 16-bit codewords."""
  ac = np.array([int(1e12 * 0.9 ** i) + 1 for i in range(256)], dtype=np.int64)
  dc = np.array([int(1e6 * 0.5 ** i) + 1 for i in range(16)], dtype=np.int64)
  table = {'dc': truth.package_merge(dc), 'ac': truth.package_merge(ac)}
  assert table['ac'].max() == 16 and table['ac'].min() >= 1
  return [table, None]


# ------------------------------------------------------------ header bytes
def segment(marker, payload):
  return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + bytes(
      payload)


def header_parts(components=((1, 1, 1, 0),), h=8, w=8, precision=8,
                 sof=0xC0, tables=((0, 0), (1, 0)), scan_tables=None,
                 spectral=(0, 63, 0), dqt=((0, 0),), extra=b'',
                 scan_components=None):
  """The segments of a file, in order, as a list of byte strings: SOI, APP0,
  `extra`, DQT per (precision, id), SOF, DHT per (class, id), SOS; one-symbol
  Huffman tables (symbol 0, one bit), which make 0-bits a stream of empty
  blocks."""
  out = [b'\xff\xd8',
         segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00'), extra]
  for pq, tq in dqt:
    out.append(segment(0xDB, bytes([pq << 4 | tq]) + bytes([1] * (
        128 if pq else 64))))
  frame = bytes([precision]) + h.to_bytes(2, 'big') + w.to_bytes(2, 'big')
  frame += bytes([len(components)])
  for cid, ch, cv, tq in components:
    frame += bytes([cid, ch << 4 | cv, tq])
  out.append(segment(sof, frame))
  for klass, index in tables:
    out.append(segment(0xC4, bytes([klass << 4 | index]) + bytes(
        [1] + [0] * 15) + bytes([0])))
  if scan_components is None:
    scan_components = [c[0] for c in components]
  if scan_tables is None:
    scan_tables = [(0, 0)] * len(scan_components)
  scan = bytes([len(scan_components)])
  for cid, (td, ta) in zip(scan_components, scan_tables):
    scan += bytes([cid, td << 4 | ta])
  out.append(segment(0xDA, scan + bytes(spectral)))
  return out


def header_file(**kwargs):
  """A whole file around header_parts: the segment byte 0x3F holds one empty
  block (DC category 0, end of block) and six pad bits."""
  return b''.join(header_parts(**kwargs)) + b'\x3f' + b'\xff\xd9'
